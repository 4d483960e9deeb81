// layered_scratch_check.cpp -- layered BP's slot rule (layered_slot_rule,
// exp_ldpc_amd/csrc/qdec_layered.h) driven through the scratch policy
// (qdec_scratch.h) over a fake memory that refuses, as tools/scratch_check.cpp
// does for the OSD and frame rules: a stand-alone program for ASan + UBSan with
// no HIP header on the include path.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/layered_scratch_check.cpp -o layered_scratch_check
//   layered_scratch_check  ->  per scenario a "# name" line, every memory operation
//                            as it happens and a "-> slots held mark code [text]"
//                            line after each call
// tests/test_layered_host.py compares the output with traces worked out by hand.
// It also prints the layouts of four graphs ("layout ..." lines) and the
// placement each request gets, so the limits the library launches by are
// checked without a device.
#include <cstdio>
#include <cstdlib>

#include "../exp_ldpc_amd/csrc/qdec_layered.h"

using namespace qdec;

struct FakeMem : ScratchMem {
    size_t limit = SIZE_MAX;  // larger requests are refused: out of memory (code 2)
    size_t free_b = 1 << 20;
    int error_once = 0;       // not 0: the next request fails with this code instead
    Alloc alloc(size_t bytes) override {
        if (error_once) {
            const int code = error_once;
            error_once = 0;
            std::printf("alloc %zu error %d\n", bytes, code);
            return {nullptr, code, false, "fake error"};
        }
        if (bytes > limit) {
            std::printf("alloc %zu oom\n", bytes);
            return {nullptr, 2, true, "out of memory"};
        }
        std::printf("alloc %zu ok\n", bytes);
        return {std::malloc(bytes), 0, false, ""};
    }
    void free(void* p, const char* what) override {
        std::printf("free (%s)\n", what);
        std::free(p);
    }
    void drain() override { std::printf("drain\n"); }
    size_t free_bytes() override {
        std::printf("free_bytes\n");
        return free_b;
    }
};

static FakeMem mem;
static const SlotRule kLayered = layered_slot_rule(1000, 8);  // slots of 1000 B, 8 by default

static void begin(const char* name) {
    std::printf("# %s\n", name);
    mem = FakeMem();
}

static void slots(SlotScratch& s, int64_t work) {
    try {
        const int64_t n = s.acquire(mem, kLayered, work);
        if (n * kLayered.slot > s.bytes) std::printf("more slots than held\n");
        std::memset(s.ptr, 0xab, s.bytes);
        std::printf("-> %lld %zu %zu 0\n", (long long)n, s.bytes, s.refused);
    } catch (const Fail& e) {
        std::printf("-> - %zu %zu %d %s\n", s.bytes, s.refused, e.code, e.what());
    }
}

static void layout(const char* name, int m, int n, int E, int64_t tsz) {
    DevGraph g{};
    g.m = m, g.n = n, g.E = E;
    g.m_pad = (m + 63) / 64 * 64, g.n_pad = (n + 63) / 64 * 64;
    const LayeredLayout L(g, tsz);
    std::printf("layout %s %lld %lld %lld %d %d %d\n", name, (long long)L.lds_bytes(false), (long long)L.lds_bytes(true),
                (long long)L.slot_bytes, layered_place(L, 0), layered_place(L, 1), layered_place(L, 2));
}

int main() {
    {
        begin("everything_refused");
        SlotScratch s;
        mem.limit = 0;
        slots(s, 100);
        slots(s, 100);
        s.release(mem, kLayered.free_what);
    }
    {
        begin("budget");
        SlotScratch s;
        mem.free_b = 3999;  // a quarter holds no slot
        slots(s, 100);
        mem.free_b = 12000;  // a quarter holds 3
        slots(s, 100);
        s.slots_cfg = 2;  // no grow: the budget is not consulted
        slots(s, 100);
        s.release(mem, kLayered.free_what);
    }
    {
        begin("halved");
        SlotScratch s;
        mem.limit = 2500;
        slots(s, 5);  // five shots: 5 -> 3 -> 2 slots
        slots(s, 5);
        s.release(mem, kLayered.free_what);
    }
    {
        begin("other_error");
        SlotScratch s;
        mem.error_once = 7;
        slots(s, 100);
        s.release(mem, kLayered.free_what);
    }
    std::printf("# layouts\n");
    layout("hz225_f32", 108, 225, 756, 4);
    layout("hz225_f64", 108, 225, 756, 8);
    layout("st225r2_f64", 324, 891, 3159, 8);  // fits LDS, but not eight times: auto goes to HBM
    layout("dem_f64", 648, 25684, 120000, 8);
    layout("huge_f32", 100000, 1200000, 4000000, 4);
    return 0;
}

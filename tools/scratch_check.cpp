// scratch_check.cpp -- the scratch policy (exp_ldpc_amd/csrc/qdec_scratch.h) as a
// stand-alone program over a fake memory that refuses, so the paths the library
// takes when device memory is short run under ASan + UBSan with a static runtime
// and no GPU stack (no HIP header is on the include path):
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tools/scratch_check.cpp -o scratch_check
//   scratch_check   ->  per scenario a "# name" line, then every memory operation
//                       as it happens and a "-> ..." line after each call
//
// The fake hands out real host blocks (a double free or a use after a free is a
// sanitizer report; every call's block is written over its whole length),
// refuses any single request above `limit`, returns one error that is not
// out-of-memory on demand, and reports a settable amount of free memory.
// tests/test_scratch_host.py compares the output with traces worked out by hand.
#include <cstdio>
#include <cstdlib>

#include "../exp_ldpc_amd/csrc/qdec_scratch.h"

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

// slots of 1000 B, 8 by default; the frame scratch has no budget
static const SlotRule kFrame{1000, 8, -97, "circuit: no memory for one frame slot of ", 0, nullptr,
                             "hipMalloc frame scratch", "hipFree frame scratch"};
static const SlotRule kOsd{1000, 8, -46, "no memory for one OSD slot of ", -45, "one OSD slot of ",
                           "hipMalloc OSD scratch", "hipFree OSD scratch"};

static void begin(const char* name) {
    std::printf("# %s\n", name);
    mem = FakeMem();
}

// "-> slots held mark code [text]"; a failed call has no slots
static void slots(SlotScratch& s, const SlotRule& r, int64_t work) {
    try {
        const int64_t n = s.acquire(mem, r, work);
        if (n * r.slot > s.bytes) std::printf("more slots than held\n");
        std::memset(s.ptr, 0xab, s.bytes);
        std::printf("-> %lld %zu %zu 0\n", (long long)n, s.bytes, s.refused);
    } catch (const Fail& e) {
        std::printf("-> - %zu %zu %d %s\n", s.bytes, s.refused, e.code, e.what());
    }
}

// "-> bytes|null held mark code [text]"
static void message(MessageScratch& s, size_t need, size_t floor) {
    try {
        size_t got = 0;
        void* p = s.acquire(mem, need, floor, &got);
        if (p) std::memset(p, 0xab, got);
        if (p) std::printf("-> %zu %zu %zu 0\n", got, s.bytes, s.refused);
        else std::printf("-> null %zu %zu 0\n", s.bytes, s.refused);
    } catch (const Fail& e) {
        std::printf("-> - %zu %zu %d %s\n", s.bytes, s.refused, e.code, e.what());
    }
}

static void everything_refused(const char* name, const SlotRule& r) {
    begin(name);
    SlotScratch s;
    mem.limit = 0;
    slots(s, r, 100);
    slots(s, r, 100);
    s.release(mem, r.free_what);
}

int main() {
    {
        begin("grow_once");
        SlotScratch s;
        slots(s, kFrame, 5);
        s.slots_cfg = 3;
        slots(s, kFrame, 5);
        s.release(mem, kFrame.free_what);
    }
    {
        begin("halved_then_not_asked_again");
        SlotScratch s;
        mem.limit = 2500;
        slots(s, kFrame, 100);
        slots(s, kFrame, 100);
        s.slots_cfg = 3;
        slots(s, kFrame, 100);
        s.release(mem, kFrame.free_what);
    }
    everything_refused("everything_refused_frame", kFrame);
    everything_refused("everything_refused_osd", kOsd);
    {
        begin("other_error");
        SlotScratch s;
        mem.error_once = 7;
        slots(s, kFrame, 100);
        slots(s, kFrame, 5);  // holds 5 slots
        mem.error_once = 7;
        slots(s, kFrame, 100);  // the old buffer is freed before the request that fails
        s.release(mem, kFrame.free_what);
    }
    {
        begin("osd_budget");
        SlotScratch s;
        mem.free_b = 3999;
        slots(s, kOsd, 100);
        mem.free_b = 12000;
        slots(s, kOsd, 100);
        s.slots_cfg = 2;  // no grow: the budget is not consulted
        slots(s, kOsd, 100);
        s.release(mem, kOsd.free_what);
        SlotScratch t;
        t.slots_cfg = 2;
        slots(t, kOsd, 100);
        t.slots_cfg = 0;
        mem.free_b = 2000;  // a cap of one slot, below the two held
        slots(t, kOsd, 100);
        t.release(mem, kOsd.free_what);
    }
    {
        begin("work_clamps");
        SlotScratch s;
        slots(s, kFrame, 0);
        slots(s, kFrame, -5);
        s.slots_cfg = 6;
        slots(s, kFrame, 4);
        s.release(mem, kFrame.free_what);
    }
    {
        begin("message_capped");
        MessageScratch s;
        mem.limit = 3000;
        message(s, 10000, 1000);
        message(s, 1500, 1000);  // fits what is held
        for (int i = 1; i <= 64; ++i) message(s, 10000, 1000);  // the 64th retries and is refused again
        for (int i = 1; i <= 63; ++i) message(s, 10000, 1000);
        mem.limit = SIZE_MAX;
        message(s, 10000, 1000);  // the 128th retries
        s.release(mem, "hipFree scratch");
    }
    {
        begin("message_floor_refused");
        MessageScratch s;
        mem.limit = 3000;
        message(s, 4000, 4000);
        message(s, 0, 0);
        s.release(mem, "hipFree scratch");
    }
    {
        begin("stage_regions");  // "region name offset bytes", then "-> total"; every region written whole
        StageRegions st;
        char h = 0;
        st.add(&h, 300, "a");
        st.add(nullptr, 5000, "b");
        st.add(&h, 256, "c");
        st.add(&h, 1, "d");
        auto* w = static_cast<unsigned char*>(std::malloc(st.total));
        for (const StageRegions::Reg& r : st.regs) {
            std::printf("region %s %zu %zu\n", r.name, r.off, r.bytes);
            std::memset(w + r.off, 0xab, r.bytes);
        }
        std::printf("-> %zu\n", st.total);
        std::free(w);
    }
    return 0;
}

// qdec_scratch.h -- the policy of the scratch areas that shrink when device
// memory is short: the slot scratches of osd_hbm_kernel and of the HBM-placed
// Pauli-frame kernels (SlotScratch) and the HBM message scratch of the workgroup
// BP kernels (MessageScratch); and the region layout of a host-buffer batch in
// the workspace (StageRegions).  Pure host code with no HIP header: the memory
// comes through a ScratchMem, which the library backs with HIP (qdec_abi.h) and
// the stand-alone checker (tools/scratch_check.cpp) with a fake that refuses.
#pragma once
#include "qdec_tables.h"

namespace qdec {

// One allocation's outcome: code 0 and the block, or the backend's error code
// and text, `oom` when that error is "out of memory".  Clearing a sticky error
// state after a refusal is the backend's business.
struct Alloc {
    void* ptr;
    int code;
    bool oom;
    const char* text;
};

// The memory of one scratch.  free, drain and free_bytes throw Fail themselves.
struct ScratchMem {
    virtual ~ScratchMem() = default;
    virtual Alloc alloc(size_t bytes) = 0;
    virtual void free(void* p, const char* what) = 0;
    virtual void drain() = 0;         // returns once the buffer's last user has finished
    virtual size_t free_bytes() = 0;  // free device memory
};

inline Fail alloc_fail(const Alloc& a, const char* what) {
    return Fail(-100 - a.code, std::string(what) + ": " + a.text);
}

struct ScratchBuf {
    void* ptr = nullptr;
    size_t bytes = 0;    // held
    size_t refused = 0;  // smallest size refused for lack of memory (0: none)

    // launches in flight may use the buffer: the drain comes before the free
    void release(ScratchMem& mem, const char* free_what) {
        mem.drain();
        if (ptr) mem.free(ptr, free_what);
        ptr = nullptr;
        bytes = 0;
    }

    // The shrinking allocation, with nothing held: asks for `size`, next(size),
    // ... down to `last` and keeps the first block granted.  Each refusal above
    // `last` lowers the mark; one at `last` is returned with nothing held and
    // the mark left to the caller.  Any error other than out-of-memory leaves
    // no mark and throws -100 - code under `what`.
    template <class Next>
    Alloc alloc_shrinking(ScratchMem& mem, const char* what, size_t size, size_t last, Next next) {
        for (;; size = next(size)) {
            const Alloc a = mem.alloc(size);
            if (a.code != 0 && !a.oom) throw alloc_fail(a, what);
            if (a.code == 0) ptr = a.ptr, bytes = size;
            if (a.code == 0 || size <= last) return a;
            refused = refused ? std::min(refused, size) : size;
        }
    }
};

// What tells the OSD slot scratch from the frame slot scratch.
struct SlotRule {
    size_t slot;              // bytes of one slot
    int64_t dflt;             // slots when none are configured
    int oom_code;             // one slot refused: the code, and its text up to the slot size
    const char* oom_text;
    int budget_code;          // not 0: a grow stays within a quarter of the free device memory; this
    const char* budget_text;  // code (text up to the slot size) when that is below one slot
    const char *alloc_what, *free_what;
};

// One slot per workgroup of a launch; results do not depend on the slot count.
struct SlotScratch : ScratchBuf {  // its mark only ever goes down and is never cleared
    int64_t slots_cfg = 0;   // configured (0: the rule's default)
    int64_t slots_last = 0;  // slots of the last launch

    // The slots to launch with over `work` units (shots, 64-shot words): the
    // configured or default count, at most `work`, at least one, at most what
    // is held after a grow.  On a refusal the count is halved down to one slot;
    // refused there too, nothing is held, the mark is the slot size and the
    // call fails with the rule's oom_code.
    int64_t acquire(ScratchMem& mem, const SlotRule& r, int64_t work) {
        int64_t want = slots_cfg > 0 ? slots_cfg : r.dflt;
        if (want > work) want = work;
        if (want < 1) want = 1;
        const int64_t held = (int64_t)(bytes / r.slot);
        // a size at or above the mark is not asked for again while at least one
        // slot is held; with nothing held every call tries again
        auto grows = [&] { return want > held && !(held >= 1 && refused && (size_t)want * r.slot >= refused); };
        if (r.budget_code && grows()) {  // the budget is consulted only when a grow would be attempted
            const int64_t cap = (int64_t)((mem.free_bytes() + bytes) / 4 / r.slot);  // the scratch held counts as free
            if (cap < 1)
                throw Fail(r.budget_code, r.budget_text + std::to_string(r.slot) + " B is beyond the scratch budget "
                                          "(a quarter of the free device memory)");
            if (want > cap) want = cap;
        }
        if (grows()) {
            release(mem, r.free_what);
            const Alloc a = alloc_shrinking(mem, r.alloc_what, (size_t)want * r.slot, r.slot,
                                            [&](size_t b) { return (b / r.slot + 1) / 2 * r.slot; });
            if (a.code != 0) {
                refused = refused ? std::min(refused, r.slot) : r.slot;
                throw Fail(r.oom_code, r.oom_text + std::to_string(r.slot) + " B");
            }
        }
        return std::min(want, (int64_t)(bytes / r.slot));
    }
};

// The message slices and slot groups of the workgroup BP kernels: `need` bytes
// run every slot group at once, `floor` bytes one; the launch sizes its grid
// from the bytes it gets, and results do not change.
struct MessageScratch : ScratchBuf {
    uint64_t capped_calls = 0;  // calls served the reduced scratch since the refusal

    // The scratch for a launch and in *got the bytes it may use (null for need
    // == 0, with no memory operation).  On a refusal the request goes half the
    // way down to `floor` each time; refused there too, nothing is held and the
    // call fails like any failed allocation, with the out-of-memory code.
    void* acquire(ScratchMem& mem, size_t need, size_t floor, size_t* got) {
        *got = need;
        if (need == 0) return nullptr;
        // capped: a request at or above the mark keeps the reduced scratch
        // untouched instead of draining and failing the same allocation every
        // call; every 64th such call retries the full size (the memory may be
        // free again), and a success there clears the mark
        if (need > bytes && ptr && refused && need >= refused && bytes >= floor && ++capped_calls % 64 != 0) {
            *got = bytes;
            return ptr;
        }
        if (need > bytes) {
            release(mem, "hipFree scratch");
            const Alloc a = alloc_shrinking(mem, "hipMalloc message scratch", need, floor,
                                            [&](size_t b) { return std::max(floor, floor + (b - floor) / 2); });
            if (a.code != 0) throw alloc_fail(a, "hipMalloc message scratch");
            if (bytes == need) refused = 0;
            *got = bytes;
        }
        return ptr;
    }
};

// The regions of one host-buffer batch in a handle's workspace, in the order
// they are added: 256-B aligned, and none for a null host pointer (its device
// pointer is null too).  `name` is the region's in the copies' error texts.
struct StageRegions {
    struct Reg {
        size_t off, bytes;
        void* host;
        const char* name;
    };
    std::vector<Reg> regs;
    size_t total = 0;  // bytes of workspace the regions need
    int add(const void* host, size_t bytes, const char* name) {
        regs.push_back({total, host ? bytes : 0, const_cast<void*>(host), name});
        if (host) total += (bytes + 255) / 256 * 256;
        return (int)regs.size() - 1;
    }
};

}  // namespace qdec

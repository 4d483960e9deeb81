// qdec_abi.h -- what the two ABI units (qdec_abi.cpp: graph handles;
// qdec_abi_circuit.cpp: compiled circuits) share: HIP error checks, the guard
// that keeps C++ exceptions inside the library, the device backends of
// TableSink and ScratchMem, the stream chain of a handle's buffers, and the
// staging of a host-buffer batch through a handle's workspace.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/qdec.h"
#include "qdec_internal.h"
#include "qdec_scratch.h"
#include "qdec_tables.h"

namespace qdec {

inline thread_local std::string g_last_error;  // qd_last_error

inline void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw Fail(-100 - (int)e, std::string(what) + ": " + hipGetErrorString(e));
}

template <typename F>
int guarded(F&& f) {
    try {
        f();
        return 0;
    } catch (const Fail& e) {
        g_last_error = e.what();
        return e.code;
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return -99;
    } catch (...) {
        g_last_error = "unknown error";
        return -99;
    }
}

// The tables of a device graph: one allocation each, owned by the graph.  (A
// host-only graph, qd_graph_create_host, keeps HostSink copies instead and
// makes no HIP call.)
struct DeviceSink : TableSink {
    std::vector<void*> ptrs;
    const void* put(const void* src, size_t bytes) override {
        void* d = nullptr;
        hip_check(hipMalloc(&d, std::max<size_t>(bytes, 16)), "hipMalloc");
        ptrs.push_back(d);
        if (bytes) hip_check(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice), "hipMemcpy H2D");
        return d;
    }
    void release() override {
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
    ~DeviceSink() override { release(); }
};

// Orders the users of a handle's buffers across streams: every user records the
// event on its stream behind its launches (release) and a user on another stream
// waits for it first (acquire), so the buffers are never used by two streams at
// once; a buffer is freed or regrown only after the event has completed (drain).
struct StreamChain {
    hipEvent_t ev = nullptr;
    bool live = false;
    hipStream_t last = nullptr;
    void acquire(hipStream_t s) {
        if (live && last != s) hip_check(hipStreamWaitEvent(s, ev, 0), "hipStreamWaitEvent");
    }
    void release(hipStream_t s) {
        if (!ev) hip_check(hipEventCreateWithFlags(&ev, hipEventDisableTiming), "hipEventCreate");
        hip_check(hipEventRecord(ev, s), "hipEventRecord");
        live = true;
        last = s;
    }
    void drain() { if (live) hip_check(hipEventSynchronize(ev), "hipEventSynchronize"); }
    void destroy() {  // a handle's destructor: errors are ignored
        if (live) (void)hipEventSynchronize(ev);
        if (ev) (void)hipEventDestroy(ev);
        ev = nullptr;
        live = false;
    }
};

// ScratchMem on the current device; drain_fn waits for the scratch's last user.
template <class Drain>
struct HipMem : ScratchMem {
    Drain drain_fn;
    explicit HipMem(Drain d) : drain_fn(d) {}
    Alloc alloc(size_t bytes) override {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) return {p, 0, false, ""};
        (void)hipGetLastError();  // clear the sticky error before any launch checks it
        return {nullptr, (int)e, e == hipErrorOutOfMemory, hipGetErrorString(e)};
    }
    void free(void* p, const char* what) override { hip_check(hipFree(p), what); }
    void drain() override { drain_fn(); }
    size_t free_bytes() override {
        size_t free_b = 0, total_b = 0;
        hip_check(hipMemGetInfo(&free_b, &total_b), "hipMemGetInfo");
        return free_b;
    }
};

// A slot scratch (qdec_scratch.h) chained over streams through an event of its
// own: two launches never share live slots.
struct ChainedSlots : SlotScratch {
    StreamChain chain;
    // the cross-stream wait is enqueued before anything else can throw: a
    // failed acquire leaves the stream ordered behind the last launch
    int64_t acquire(const SlotRule& r, int64_t work, hipStream_t s) {
        chain.acquire(s);
        HipMem mem([&] { chain.drain(); });
        return SlotScratch::acquire(mem, r, work);
    }
    void release(int64_t slots, hipStream_t s) { chain.release(s), slots_last = slots; }
    void destroy() {  // a launch may still use the slots: wait, then free
        chain.destroy();
        if (ptr) (void)hipFree(ptr);
    }
};

// A grow-only device buffer; `cap` is its capacity in the owner's unit.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    // a fresh allocation of `bytes` for capacity `c`, once drain() has waited
    // for the last user of the old one
    template <class Drain>
    void regrow(size_t c, size_t bytes, const char* free_what, const char* alloc_what, Drain&& drain) {
        drain();
        if (p) hip_check(hipFree(p), free_what);
        p = nullptr;
        cap = 0;
        hip_check(hipMalloc(&p, bytes), alloc_what);
        cap = c;
    }
};

// One host-buffer batch staged through a handle's workspace: the regions
// (StageRegions, inputs first), the workspace regrown once when they do not fit,
// copies in, and behind the launch the copies out and the stream synchronise.
// No drain before the regrow: every host entry point ends in that synchronise,
// so the workspace has no user left.
struct HostStage : StageRegions {
    uint8_t* w = nullptr;
    void place(DevBuf& ws) {
        if (total > ws.cap) ws.regrow(total, total, "hipFree", "hipMalloc workspace", [] {});
        w = static_cast<uint8_t*>(ws.p);
    }
    template <typename P = void>
    P* dev(int r) const {  // null for a region that was not passed
        return regs[r].bytes ? reinterpret_cast<P*>(w + regs[r].off) : nullptr;
    }
    // regions [first, last) host -> device (in) or device -> host; errors read "H2D <name>" / "D2H <name>"
    void copy(int first, int last, bool in, hipStream_t s) const {
        for (int r = first; r < last; ++r) {
            const Reg& g = regs[r];
            if (!g.bytes) continue;
            const hipError_t e = in ? hipMemcpyAsync(w + g.off, g.host, g.bytes, hipMemcpyHostToDevice, s)
                                    : hipMemcpyAsync(g.host, w + g.off, g.bytes, hipMemcpyDeviceToHost, s);
            if (e != hipSuccess) hip_check(e, ((in ? "H2D " : "D2H ") + std::string(g.name)).c_str());
        }
    }
    void finish(int first_out, hipStream_t s) const {
        copy(first_out, (int)regs.size(), false, s);
        hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    }
};

}  // namespace qdec

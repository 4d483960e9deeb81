// qdec_abi_window.cpp -- the extern "C" entry points of window boundaries
// (qd_window_*, include/qdec.h): the validated tables of one boundary
// (qdec_window.h) and, unless host-only, their copy on one device.  No C++
// exception crosses the ABI.
#include "qdec_abi.h"

using namespace qdec;

struct qd_window {
    WindowTables t;
    WindowDev d{};
    bool host_only = true;
    int device = 0;
    int num_cus = 0;
    int64_t blocks_cfg = 0;  // qd_window_set_blocks (0: the default)
    DeviceSink arena;
};

namespace {

int create_window(bool host_only, int32_t device, int32_t n_w, int32_t m_total, int32_t n_carry,
                  const int32_t* carry_rows, const int32_t* carry_ptr, const int32_t* carry_cols, int32_t k_acc,
                  const int32_t* acc_ptr, const int32_t* acc_cols, int32_t row0, int32_t m_next, qd_window** out) {
    return guarded([&] {
        if (!out) throw Fail(-26, "window: null output handle");
        *out = nullptr;
        std::unique_ptr<qd_window> W(new qd_window());
        window_build(W->t, n_w, m_total, n_carry, carry_rows, carry_ptr, carry_cols, k_acc, acc_ptr, acc_cols, row0,
                     m_next);
        W->host_only = host_only;
        const WindowTables& t = W->t;
        WindowDev& d = W->d;
        d.n_w = t.n_w, d.m_total = t.m_total, d.n_carry = t.n_carry, d.k_acc = t.k_acc, d.row0 = t.row0;
        d.m_next = t.m_next;
        if (!host_only) {
            int ndev = 0;
            hip_check(hipGetDeviceCount(&ndev), "hipGetDeviceCount");
            if (device < 0 || device >= ndev) throw Fail(-15, "device ordinal out of range");
            W->device = device;
            hip_check(hipSetDevice(device), "hipSetDevice");
            hipDeviceProp_t prop;
            hip_check(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties");
            W->num_cus = prop.multiProcessorCount;
            d.carry_rows = W->arena.upload(t.carry_rows);
            d.carry_ptr = W->arena.upload(t.carry_ptr);
            d.carry_cols = W->arena.upload(t.carry_cols);
            d.acc_ptr = W->arena.upload(t.acc_ptr);
            d.acc_cols = W->arena.upload(t.acc_cols);
        }
        *out = W.release();
    });
}

}  // namespace

extern "C" {

int qd_window_create(int32_t device, int32_t n_w, int32_t m_total, int32_t n_carry, const int32_t* carry_rows,
                     const int32_t* carry_ptr, const int32_t* carry_cols, int32_t k_acc, const int32_t* acc_ptr,
                     const int32_t* acc_cols, int32_t row0, int32_t m_next, qd_window** out) {
    return create_window(false, device, n_w, m_total, n_carry, carry_rows, carry_ptr, carry_cols, k_acc, acc_ptr,
                         acc_cols, row0, m_next, out);
}

int qd_window_create_host(int32_t n_w, int32_t m_total, int32_t n_carry, const int32_t* carry_rows,
                          const int32_t* carry_ptr, const int32_t* carry_cols, int32_t k_acc, const int32_t* acc_ptr,
                          const int32_t* acc_cols, int32_t row0, int32_t m_next, qd_window** out) {
    return create_window(true, 0, n_w, m_total, n_carry, carry_rows, carry_ptr, carry_cols, k_acc, acc_ptr, acc_cols,
                         row0, m_next, out);
}

int qd_window_set_blocks(qd_window* w, int64_t blocks) {
    return guarded([&] {
        if (!w) throw Fail(-26, "window: null handle");
        if (blocks < 0 || blocks > kWindowMaxBlocks) throw Fail(-29, "window: blocks must be 0 (default) .. 2^20");
        w->blocks_cfg = blocks;
    });
}

int qd_window_advance_device(qd_window* w, int64_t B, const uint8_t* x, uint8_t* syn_full, uint8_t* acc_out,
                             uint8_t* syn_next, void* stream) {
    return guarded([&] {
        if (!w) throw Fail(-26, "window: null handle");
        if (w->host_only) throw Fail(-16, "host-only window (qd_window_create_host): no device to run on");
        if (B < 0) throw Fail(-28, "window advance: negative batch size");
        const bool reads_syn = (x && w->t.n_carry > 0) || (syn_next && w->t.m_next > 0);
        if (B > 0 && reads_syn && !syn_full) throw Fail(-28, "window advance: null syn_full");
        if (B == 0) return;
        hip_check(hipSetDevice(w->device), "hipSetDevice");
        const WindowArgs a{B, x, syn_full, acc_out, syn_next};
        const int rc = launch_window(w->d, a, window_grid(w->blocks_cfg, w->num_cus, B), (hipStream_t)stream);
        if (rc != 0) throw Fail(-102, std::string("window advance launch failed: ") + hipGetErrorString((hipError_t)rc));
    });
}

int qd_window_destroy(qd_window* w) {
    return guarded([&] {
        if (!w) return;
        if (!w->host_only) (void)hipSetDevice(w->device);
        delete w;  // its sink frees the uploads
    });
}

}  // extern "C"

// qdec_window.hip -- window_advance_kernel: the step between two windows of a
// sliding-window decode (tables and arguments: qdec_window.h).
//
// A workgroup takes shots grid-strided.  Per shot, when a.x is given: the
// window's solution row is read once, byte by byte, and kept as bits in LDS
// (one ballot per 64 columns); then one thread per carry row and per
// accumulator row gathers its columns' bits from there and toggles its one
// output byte, so no two threads write the same byte and nothing is atomic.
// Behind a barrier, which makes the toggled syndrome bytes visible to the
// workgroup, one thread per row copies the next window's rows out.
#include "qdec_internal.h"

namespace qdec {

__global__ __launch_bounds__(kWindowBlock) void window_advance_kernel(WindowDev w, WindowArgs a) {
    extern __shared__ uint64_t xbits[];  // [(n_w + 63) / 64]
    const int tid = threadIdx.x;
    const int n_bits = (w.n_w + 63) / 64 * 64;
    for (int64_t shot = blockIdx.x; shot < a.B; shot += gridDim.x) {
        uint8_t* sf = a.syn_full + shot * w.m_total;
        if (a.x) {  // uniform
            const uint8_t* xr = a.x + shot * w.n_w;
            for (int j = tid; j < n_bits; j += kWindowBlock) {  // whole waves: n_bits is a multiple of 64
                const uint64_t word = __ballot(j < w.n_w && (xr[j] & 1));
                if ((tid & 63) == 0) xbits[j >> 6] = word;
            }
            __syncthreads();
            for (int i = tid; i < w.n_carry + w.k_acc; i += kWindowBlock) {
                const bool carry = i < w.n_carry;
                const int r = carry ? i : i - w.n_carry;
                const int32_t* ptr = carry ? w.carry_ptr : w.acc_ptr;
                const int32_t* cols = carry ? w.carry_cols : w.acc_cols;
                uint64_t v = 0;
                for (int e = ptr[r]; e < ptr[r + 1]; ++e) {
                    const int c = cols[e];
                    v ^= xbits[c >> 6] >> (c & 63);
                }
                if (v & 1) {
                    if (carry)
                        sf[w.carry_rows[r]] ^= 1;
                    else if (a.acc_out)
                        a.acc_out[shot * w.k_acc + r] ^= 1;
                }
            }
            __syncthreads();  // the carry is visible below, and xbits is free for the next shot
        }
        if (a.syn_next)
            for (int i = tid; i < w.m_next; i += kWindowBlock) a.syn_next[shot * w.m_next + i] = sf[w.row0 + i];
    }
}

int launch_window(const WindowDev& w, const WindowArgs& a, int64_t grid, hipStream_t stream) {
    if (a.B <= 0 || grid <= 0) return 0;
    const size_t lds = (size_t)(w.n_w + 63) / 64 * 8;
    hipLaunchKernelGGL(window_advance_kernel, dim3((unsigned)grid), dim3(kWindowBlock), lds, stream, w, a);
    return (int)hipGetLastError();
}

}  // namespace qdec

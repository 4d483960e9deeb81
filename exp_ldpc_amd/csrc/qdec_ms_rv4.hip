// qdec_ms_rv4.hip -- the min-sum wave kernels (bp_ms_wave_kernel and
// bp_ms_cmp_kernel, qdec_bp_ms.h) of the wave shapes with four variable
// rounds, (2, 4, 7) and (2, 4, 8); qdec_ms_rvx.hip builds the other shapes.
//
// Why the min-sum kernels are cut by shape and not by family or precision: the
// two families share helpers instantiated per shape (queue_push_packed<RV, RC>
// among them), and a kernel's code depends on which other callers of such a
// helper its translation unit holds.  bp_ms_wave_kernel compiled without
// bp_ms_cmp_kernel changes 15 instantiations (DEFER without LEAN), double
// compiled without float changes 2; a shape's kernels compiled together come
// out as they do in one unit of everything.
#include <hip/hip_runtime.h>

#include "qdec_device.h"
#include "qdec_bp_ms.h"
#include "qdec_kernels.h"

namespace qdec {

QDEC_STAMPS_READER(read_stamps_ms_rv4)

template <int RC, int RV, int DRC>
static void add_shape(KernelTable& wave, KernelTable& cmp) {
    if constexpr (ms_shape_in_rv4(RV)) add_ms_shape<RC, RV, DRC>(wave, cmp);
}

void add_ms_kernels_rv4(KernelTable& wave, KernelTable& cmp) {
#define QDEC_SHAPE(R, V, D) add_shape<R, V, D>(wave, cmp);
    QDEC_WAVE_SHAPES(QDEC_SHAPE)
#undef QDEC_SHAPE
}

}  // namespace qdec

// qdec_ms_rvx.hip -- the min-sum wave kernels (bp_ms_wave_kernel and
// bp_ms_cmp_kernel, qdec_bp_ms.h) of every wave shape but those with four
// variable rounds, which qdec_ms_rv4.hip builds (it says why the cut is by shape).
#include <hip/hip_runtime.h>

#include "qdec_device.h"
#include "qdec_bp_ms.h"
#include "qdec_kernels.h"

namespace qdec {

QDEC_STAMPS_READER(read_stamps_ms_rvx)

template <int RC, int RV, int DRC>
static void add_shape(KernelTable& wave, KernelTable& cmp) {
    if constexpr (!ms_shape_in_rv4(RV)) add_ms_shape<RC, RV, DRC>(wave, cmp);
}

void add_ms_kernels_rvx(KernelTable& wave, KernelTable& cmp) {
#define QDEC_SHAPE(R, V, D) add_shape<R, V, D>(wave, cmp);
    QDEC_WAVE_SHAPES(QDEC_SHAPE)
#undef QDEC_SHAPE
}

}  // namespace qdec

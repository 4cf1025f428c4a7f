// Wide train-mode affine-coupling kernels for hidden tiles HT = 3: affine_trainw_pick
// (nfx_affine_trainw_kernel.h) lists the shapes.
#include "nfx_affine_trainw_kernel.h"

namespace nfx {
template <> affine_trainw_kernel_t affine_trainw_pick_ht<3>(int D, int stage) { return affine_trainw_pick<3>(D, stage); }
}  // namespace nfx

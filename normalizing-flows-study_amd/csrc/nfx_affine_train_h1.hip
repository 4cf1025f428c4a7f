// Train-mode affine-coupling kernels for hidden tiles HT = 1: affine_train_pick
// (nfx_affine_train_kernel.h) lists the shapes.
#include "nfx_affine_train_kernel.h"

namespace nfx {
template <> affine_train_kernel_t affine_train_pick_ht<1>(int D, int stage) { return affine_train_pick<1>(D, stage); }
}  // namespace nfx

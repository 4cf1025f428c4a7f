// Train-mode affine-coupling kernels for hidden tiles HT = 2: affine_train_pick
// (nfx_affine_train_kernel.h) lists the shapes.
#include "nfx_affine_train_kernel.h"

namespace nfx {
template <> affine_train_kernel_t affine_train_pick_ht<2>(int D, int stage) { return affine_train_pick<2>(D, stage); }
}  // namespace nfx

// Affine-coupling kernels for hidden tiles HT = 3: affine_pick (nfx_affine_kernel.h) lists the shapes.
#include "nfx_affine_kernel.h"

namespace nfx {
template <> affine_kernel_t affine_pick_ht<3>(int d, int dir, bool logp) { return affine_pick<3>(d, dir, logp); }
}  // namespace nfx

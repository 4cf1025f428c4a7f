// Affine-coupling kernels for hidden tiles HT = 2: affine_pick (nfx_affine_kernel.h) lists the shapes.
#include "nfx_affine_kernel.h"

namespace nfx {
template <> affine_kernel_t affine_pick_ht<2>(int d, int dir, bool logp) { return affine_pick<2>(d, dir, logp); }
}  // namespace nfx

// Small-batch affine kernels for HT = 3 and 4: affine_small_pick (nfx_affine_small_kernel.h) lists the shapes.
#include "nfx_affine_small_kernel.h"

namespace nfx {
template <> affine_kernel_t affine_small_pick_ht<3>(int d, int dir, bool logp) { return affine_small_pick<3>(d, dir, logp); }
template <> affine_kernel_t affine_small_pick_ht<4>(int d, int dir, bool logp) { return affine_small_pick<4>(d, dir, logp); }
}  // namespace nfx

// Small-batch affine kernels for HT = 1 and 2: affine_small_pick (nfx_affine_small_kernel.h) lists the shapes.
#include "nfx_affine_small_kernel.h"

namespace nfx {
template <> affine_kernel_t affine_small_pick_ht<1>(int d, int dir, bool logp) { return affine_small_pick<1>(d, dir, logp); }
template <> affine_kernel_t affine_small_pick_ht<2>(int d, int dir, bool logp) { return affine_small_pick<2>(d, dir, logp); }
}  // namespace nfx

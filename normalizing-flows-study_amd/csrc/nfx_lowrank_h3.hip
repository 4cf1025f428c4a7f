// Planar / Radial / Sylvester stack kernel, padded dim 64.
#include "nfx_lowrank_kernel.h"

namespace nfx {
lowrank_kernel_t lowrank_pick_h3(int DP) { return DP == 64 ? lowrank_stack_kernel<64> : nullptr; }
}  // namespace nfx

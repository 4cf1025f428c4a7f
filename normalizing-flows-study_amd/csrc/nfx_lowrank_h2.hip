// Planar / Radial / Sylvester stack kernel, padded dim 32.
#include "nfx_lowrank_kernel.h"

namespace nfx {
lowrank_kernel_t lowrank_pick_h2(int DP) { return DP == 32 ? lowrank_stack_kernel<32> : nullptr; }
}  // namespace nfx

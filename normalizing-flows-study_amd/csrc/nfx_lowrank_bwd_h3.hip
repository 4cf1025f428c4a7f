// Planar / Radial / Sylvester stack backward kernels, padded dim 64.
#include "nfx_lowrank_bwd_kernel.h"

namespace nfx {
lowrank_bwd_kernel_t lowrank_bwd_pick_h3(int DP) {
    switch (DP) {
        case 64: return lowrank_bwd_kernel<64>;
    }
    return nullptr;
}
}  // namespace nfx

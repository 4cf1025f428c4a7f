// Planar / Radial / Sylvester stack backward kernels, padded dim 32.
#include "nfx_lowrank_bwd_kernel.h"

namespace nfx {
lowrank_bwd_kernel_t lowrank_bwd_pick_h2(int DP) {
    switch (DP) {
        case 32: return lowrank_bwd_kernel<32>;
    }
    return nullptr;
}
}  // namespace nfx

// Planar / Radial / Sylvester stack backward kernels, padded dim 2, 4, 8 and 16.
#include "nfx_lowrank_bwd_kernel.h"

namespace nfx {
lowrank_bwd_kernel_t lowrank_bwd_pick_h1(int DP) {
    switch (DP) {
        case 2: return lowrank_bwd_kernel<2>;
        case 4: return lowrank_bwd_kernel<4>;
        case 8: return lowrank_bwd_kernel<8>;
        case 16: return lowrank_bwd_kernel<16>;
    }
    return nullptr;
}
}  // namespace nfx

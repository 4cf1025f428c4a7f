// Instantiations of the IAF forward tile kernel with the base draw fused in (made_tile_kernel's
// SAMPLE variant, nfx_made_kernel.h): hidden tiles HT = 1..4, weights LDS-resident or L2-streamed.
// A translation unit of their own, so the parallel build stays balanced.
#include "nfx_made_kernel.h"

namespace nfx {

template <int HT>
made_sample_kernel_t made_tile_sample_pick_ht(bool wlds) {
    return wlds ? made_tile_kernel<HT, true, NFX_IAF_FORWARD, false, true, MadeDraw>
                : made_tile_kernel<HT, false, NFX_IAF_FORWARD, false, true, MadeDraw>;
}
template made_sample_kernel_t made_tile_sample_pick_ht<1>(bool);
template made_sample_kernel_t made_tile_sample_pick_ht<2>(bool);
template made_sample_kernel_t made_tile_sample_pick_ht<3>(bool);
template made_sample_kernel_t made_tile_sample_pick_ht<4>(bool);

}  // namespace nfx

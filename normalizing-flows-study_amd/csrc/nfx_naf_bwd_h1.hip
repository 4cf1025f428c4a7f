// NeuralAutoregressiveFlow backward kernel, widest hidden layer padded to 32 (one translation unit
// per padded width).
#include "nfx_naf_bwd_kernel.h"

namespace nfx {
template <> naf_bwd_kernel_t naf_bwd_pick_ht<1>() { return naf_bwd_kernel<1>; }
}  // namespace nfx

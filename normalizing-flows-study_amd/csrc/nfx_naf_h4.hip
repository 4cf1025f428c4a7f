// NeuralAutoregressiveFlow kernel, widest hidden layer padded to 128 (one translation unit per padded width).
#include "nfx_naf_kernel.h"

namespace nfx {
template <> naf_kernel_t naf_pick_ht<4>() { return naf_kernel<4>; }
}  // namespace nfx

// ARQS kernels for HT = 1 and 2: arqs_pick (nfx_arqs_kernel.h) lists the shapes.
#include "nfx_arqs_kernel.h"

namespace nfx {
template <> arqs_kernel_t arqs_pick_ht<1>(int K, int inverse) { return arqs_pick<1>(K, inverse); }
template <> arqs_kernel_t arqs_pick_ht<2>(int K, int inverse) { return arqs_pick<2>(K, inverse); }
}  // namespace nfx

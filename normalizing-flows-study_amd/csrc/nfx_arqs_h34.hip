// ARQS kernels for HT = 3 and 4: arqs_pick (nfx_arqs_kernel.h) lists the shapes.
#include "nfx_arqs_kernel.h"

namespace nfx {
template <> arqs_kernel_t arqs_pick_ht<3>(int K, int inverse) { return arqs_pick<3>(K, inverse); }
template <> arqs_kernel_t arqs_pick_ht<4>(int K, int inverse) { return arqs_pick<4>(K, inverse); }
}  // namespace nfx

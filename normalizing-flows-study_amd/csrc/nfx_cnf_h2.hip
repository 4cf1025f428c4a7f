// Continuous-flow RK4 kernels, H = 64 (one translation unit per hidden width).
#include "nfx_cnf_kernel.h"

namespace nfx {
template <> cnf_kernel_t cnf_pick_ht<2>(int d) { return cnf_pick<2>(d); }
}  // namespace nfx

// Continuous-flow RK4 kernels, H = 32 (one translation unit per hidden width).
#include "nfx_cnf_kernel.h"

namespace nfx {
template <> cnf_kernel_t cnf_pick_ht<1>(int d) { return cnf_pick<1>(d); }
}  // namespace nfx

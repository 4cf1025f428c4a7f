// Continuous-flow RK4 kernels, H = 64 (one translation unit per hidden width).
#include "nfx_cnf_kernel.h"

namespace nfx {
NFX_CNF_INSTANTIATE(2)
}  // namespace nfx

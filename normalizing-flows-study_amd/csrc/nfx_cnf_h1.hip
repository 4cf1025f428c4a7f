// Continuous-flow RK4 kernels, H = 32 (one translation unit per hidden width).
#include "nfx_cnf_kernel.h"

namespace nfx {
NFX_CNF_INSTANTIATE(1)
}  // namespace nfx

// Continuous-flow RK4 kernels, H = 128 (one translation unit per hidden width).
#include "nfx_cnf_kernel.h"

namespace nfx {
NFX_CNF_INSTANTIATE(4)
}  // namespace nfx

// Continuous-flow backward kernels and the trajectory-saving forward, H = 64 (one translation unit
// per hidden width).
#include "nfx_cnf_bwd_kernel.h"

namespace nfx {
template <> cnf_bwd_kernel_t cnf_bwd_pick_ht<2>(int d) { return cnf_bwd_pick<2>(d); }
template <> cnf_kernel_t cnf_save_pick_ht<2>(int d) { return cnf_save_pick<2>(d); }
}  // namespace nfx

// Continuous-flow backward kernels and the trajectory-saving forward, H = 32 (one translation unit
// per hidden width).
#include "nfx_cnf_bwd_kernel.h"

namespace nfx {
template <> cnf_bwd_kernel_t cnf_bwd_pick_ht<1>(int d) { return cnf_bwd_pick<1>(d); }
template <> cnf_kernel_t cnf_save_pick_ht<1>(int d) { return cnf_save_pick<1>(d); }
}  // namespace nfx

// made_seqp_kernel for S = 13 .. 16 slots: made_seqp_pick (nfx_made_seqp_kernel.h) lists the forms.
#include "nfx_made_seqp_kernel.h"

namespace nfx {
made_seqp_kernel_t made_seqp_pick_13(int HT, int S, int variant, bool logp) {
    return made_seqp_pick<13>(HT, S, variant, logp);
}
}  // namespace nfx

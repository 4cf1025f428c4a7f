// made_seqp_kernel for S = 5 .. 8 slots: made_seqp_pick (nfx_made_seqp_kernel.h) lists the forms.
#include "nfx_made_seqp_kernel.h"

namespace nfx {
made_seqp_kernel_t made_seqp_pick_5(int HT, int S, int variant, bool logp) {
    return made_seqp_pick<5>(HT, S, variant, logp);
}
}  // namespace nfx

// Prints which kernel every exported picker of libnfx.so returns, over the full cross product of its
// arguments plus one value below and one above each range. Two builds with equal output dispatch alike.
// Calls no HIP API and launches nothing; needs no GPU.
//   hipcc <build.py's CFLAGS> --cuda-host-only tools/pick_probe.hip -o pick_probe \
//       -L normalizing-flows-study_amd/nfs_amd -lnfx -ldl -Wl,-rpath,normalizing-flows-study_amd/nfs_amd
#include <dlfcn.h>

#include <cstdio>

#include "nfx_affine_small_kernel.h"
#include "nfx_affine_trainw_kernel.h"
#include "nfx_arqs_kernel.h"
#include "nfx_cnf_kernel.h"
#include "nfx_made_seqp_kernel.h"
#include "nfx_spline_bwd_kernel.h"
#include "nfx_spline_schain_kernel.h"

namespace nfx {
template <int HT>  // nfx_made_wide_kernel.h (its constants clash with the affine header's)
made_par_kernel_t made_wide_pick_ht(int variant, bool logp, int nw);
made_seqp_kernel_t made_seqp_pick_1(int HT, int S, int variant, bool logp);
made_seqp_kernel_t made_seqp_pick_5(int HT, int S, int variant, bool logp);
made_seqp_kernel_t made_seqp_pick_9(int HT, int S, int variant, bool logp);
made_seqp_kernel_t made_seqp_pick_13(int HT, int S, int variant, bool logp);
}  // namespace nfx
using namespace nfx;

template <class... A>
static void show(const char* what, const void* k, A... args) {
    Dl_info info{};
    printf("%s", what);
    (printf(" %d", (int)args), ...);
    if (k && dladdr(k, &info) && info.dli_sname) printf(" -> %s+%ld\n", info.dli_sname, (long)((const char*)k - (const char*)info.dli_saddr));
    else printf(" -> %s\n", k ? "?" : "null");
}

// f(int_constant) for every V of the list
template <int... Vs, class F>
static void each(F f) {
    (f(std::integral_constant<int, Vs>{}), ...);
}

int main() {
    const int dirs[] = {-2, -1, 0, 1, 2};
    each<1, 2, 3, 4>([&](auto HT) {
        for (int d = 0; d <= 9; ++d)
            for (int dir : dirs)
                for (int lp = 0; lp < 2; ++lp) {
                    show("affine", (const void*)affine_pick_ht<HT()>(d, dir, lp), HT(), d, dir, lp);
                    show("affine_small", (const void*)affine_small_pick_ht<HT()>(d, dir, lp), HT(), d, dir, lp);
                }
        for (int K = 1; K <= 12; ++K) {
            for (int inv = 0; inv < 2; ++inv) show("arqs", (const void*)arqs_pick_ht<HT()>(K, inv), HT(), K, inv);
            for (int dir : dirs)
                for (int lp = 0; lp < 2; ++lp) {
                    show("spline", (const void*)spline_pick_ht<HT(), 0>(K, dir, lp), HT(), K, dir, lp);
                    show("spline_d2", (const void*)spline_pick_ht<HT(), 2>(K, dir, lp), HT(), K, dir, lp);
                    show("spline_wide", (const void*)spline_wide_pick_ht<HT()>(K, dir, lp), HT(), K, dir, lp);
                }
        }
        for (int v = -1; v <= 4; ++v)
            for (int a = 0; a < 2; ++a) {
                show("made_par", (const void*)made_pick_ht<HT()>(a, v), HT(), a, v);
                for (int lp = 0; lp < 2; ++lp) show("made_tile", (const void*)made_tile_pick_ht<HT()>(a, v, lp), HT(), a, v, lp);
            }
        for (int v = -1; v <= 4; ++v) show("made_seq", (const void*)made_seq_pick_ht<HT()>(v), HT(), v);
        for (int a = 0; a < 2; ++a) show("made_tile_sample", (const void*)made_tile_sample_pick_ht<HT()>(a), HT(), a);
    });
    each<1, 2>([&](auto HT) {
        for (int D = 1; D <= 9; ++D)
            for (int st = -1; st <= 8; ++st) show("affine_train", (const void*)affine_train_pick_ht<HT()>(D, st), HT(), D, st);
        for (int D = 1; D <= 9; ++D)
            for (int st = -1; st <= 6; ++st)
                show("affine_trainw", (const void*)affine_trainw_pick_ht<HT() + 2>(D, st), HT() + 2, D, st);
        for (int K = 1; K <= 12; ++K) {
            for (int inv = 0; inv < 2; ++inv) show("spline_bwd", (const void*)spline_bwd_pick_ht<HT()>(K, inv), HT(), K, inv);
            for (int dir : dirs)
                for (int lp = 0; lp < 2; ++lp)
                    for (int sm = 0; sm < 2; ++sm)
                        show("spline_schain", (const void*)spline_schain_pick_ht<HT()>(K, dir, lp, sm), HT(), K, dir, lp, sm);
        }
        for (int v = -1; v <= 4; ++v)
            for (int lp = 0; lp < 2; ++lp) {
                show("made_seqs", (const void*)made_seqs_pick_ht<HT()>(v, lp), HT(), v, lp);
                for (int nw = 3; nw <= 9; ++nw) show("made_wide", (const void*)made_wide_pick_ht<HT()>(v, lp, nw), HT(), v, lp, nw);
            }
    });
    each<1, 2, 4>([&](auto HT) {
        for (int d = 0; d <= 9; ++d) show("cnf", (const void*)cnf_pick_ht<HT()>(d), HT(), d);
    });
    for (int HT = 0; HT <= 3; ++HT)
        for (int S = 0; S <= 17; ++S)
            for (int v = -1; v <= 4; ++v)
                for (int lp = 0; lp < 2; ++lp) {
                    show("made_seqp_1", (const void*)made_seqp_pick_1(HT, S, v, lp), HT, S, v, lp);
                    show("made_seqp_5", (const void*)made_seqp_pick_5(HT, S, v, lp), HT, S, v, lp);
                    show("made_seqp_9", (const void*)made_seqp_pick_9(HT, S, v, lp), HT, S, v, lp);
                    show("made_seqp_13", (const void*)made_seqp_pick_13(HT, S, v, lp), HT, S, v, lp);
                }
    return 0;
}

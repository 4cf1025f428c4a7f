// ContinuousFlow (src/flows/continuous/): the fixed-step ODE solve of a time-conditioned tanh MLP
// field with the log-det as an augmented state, in ONE launch per call.
//
// The reference integrates with torchdiffeq's fixed-grid 'rk4' (the 3/8 rule) at step 0.01: 100
// steps, 400 field evaluations, each a 3-layer MLP plus its Jacobian trace through double-backward
// autograd. Here a wave owns a tile of 32 samples from load to store: state, log-det and the
// stage derivatives stay in registers, the H x H layer runs on v_mfma_f32_32x32x2_f32 (W2 A
// fragments in registers for H <= 64, in LDS for H = 128) and the output layer is d VALU dot
// products. The divergence is exact for every d. With g1 = 1 - h1^2, g2 = 1 - h2^2 it is one
// forward-mode tangent per input dimension,
//   tr = sum_i W3[i, :] . (g2 * (W2 (g1 * W1[:, i]))) = sum_k g2[k] sum_j W2[k, j] N[k, j] g1[j],
//   N[k, j] = sum_i W3[i, k] W1[j, i],
// and the sum over i does not depend on the sample: the pack forms C = W2 * N (elementwise, float64
// products rounded once), and the kernel computes g2 . (C g1) — ONE H x H product beside layer 2
// instead of d, on the same MFMA k-steps. HBM sees each sample once on the way in and once on the
// way out.
//
// Cost per sample and evaluation: 2 * 2 H^2 flops executed in the two H x H products (H = 64: 16.4
// kflop; x 400 evaluations = 6.6 Mflop per sample) for what the per-dimension tangent form counts
// as (1 + d) * 2 H^2 (d = 2: 24.6 kflop, 9.8 Mflop per sample), all on the fp32 MFMA pipe (157.3 TF
// peak); the kernel is never memory-bound (one wave's latency at small batches, MFMA + tanh issue
// at large ones).
#include <math.h>

#include "nfx_cnf_kernel.h"

namespace nfx {

static cnf_kernel_t pick_cnf(bool save, int d, int H) {
    if (H % 32) return nullptr;
    if (save) return pick_of<1, 2>(H / 32, [&](auto HT) -> cnf_kernel_t { return cnf_save_pick_ht<HT()>(d); });
    return pick_of<1, 2, 4>(H / 32, [&](auto HT) -> cnf_kernel_t { return cnf_pick_ht<HT()>(d); });
}

static bool cnf_family(int d, int H) { return d >= 1 && d <= kCnfMaxD && (H == 32 || H == 64 || H == 128); }

__global__ void cnf_pack_kernel(const float* __restrict__ w1, const float* __restrict__ b1,
                                const float* __restrict__ w2, const float* __restrict__ b2,
                                const float* __restrict__ w3, const float* __restrict__ b3, int d, int H,
                                float* __restrict__ packed) {
    const int HT = H / 32;
    const CnfLayout L = cnf_layout(d, HT);
    for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < L.total; o += gridDim.x * blockDim.x) {
        float v = 0.f;
        if (o < L.b1) {  // w1: layer-1 A operand over [z; t]
            const RowCol e = a1_elem(o - L.w1, L.KS1);
            v = e.col <= d ? w1[e.row * (d + 1) + e.col] : 0.f;
        } else if (o < L.w3) {  // b1, b2
            const bool second = o >= L.b2;
            const int t = o - (second ? L.b2 : L.b1);
            const int row = acc_vec_row(t);
            v = second ? b2[row] : b1[row];
        } else if (o < L.b3) {  // w3: row j of W3
            const VecRow e = acc_rows_elem(o - L.w3, HT);
            v = w3[e.vec * H + e.row];
        } else if (o < L.c2) {  // b3
            const int j = o - L.b3;
            v = j < d ? b3[j] : 0.f;
        } else {  // c2, w2: A operands over (out row k, hidden input j)
            const bool trace = o < L.w2;
            const RowCol e = a_image_elem(o - (trace ? L.c2 : L.w2), HT);
            const int k = e.row, j = e.col;
            v = w2[k * H + j];
            if (trace) {  // C[k, j] = W2[k, j] * sum_i W3[i, k] W1[j, i]
                double n = 0.0;
                for (int i = 0; i < d; ++i) n += (double)w3[i * H + k] * (double)w1[j * (d + 1) + i];
                v = (float)((double)v * n);
            }
        }
        packed[o] = v;
    }
}

}  // namespace nfx

using namespace nfx;

extern "C" size_t nfx_cnf_packed_floats(int d, int H) {
    if (!cnf_family(d, H)) return 0;
    return (size_t)cnf_layout(d, H / 32).total;
}

extern "C" int nfx_cnf_supported(int64_t B, int d, int H) { return B >= 1 && cnf_family(d, H) ? 1 : 0; }

extern "C" int nfx_cnf_pack(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                            const float* b3, int d, int H, float* packed, void* stream) {
    if (d <= 0 || H <= 0) return set_error(NFX_EINVAL, "cnf_pack: bad shape d=%d H=%d", d, H);
    if (!cnf_family(d, H))
        return set_error(NFX_EUNSUPPORTED, "cnf: d=%d H=%d outside the compiled family (d<=8, H in {32,64,128})", d, H);
    if (int rc = check_pointers("cnf_pack", {w1, b1, w2, b2, w3, b3, packed})) return rc;
    const int total = (int)nfx_cnf_packed_floats(d, H);
    cnf_pack_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(w1, b1, w2, b2, w3, b3, d, H, packed);
    return check_launch("cnf_pack_kernel");
}

// One launch of the solve; `save` picks the instantiation that also writes the trajectory (H <= 64).
static int cnf_launch(bool save, const float* packed, const float* in, float* out, float* log_det, float* traj,
                      int64_t B, int d, int H, float t_begin, float t_end, float step_size, int accumulate,
                      void* stream) {
    if (B < 0 || d <= 0 || H <= 0) return set_error(NFX_EINVAL, "cnf: bad shape B=%lld d=%d H=%d", (long long)B, d, H);
    if (!(step_size > 0.f) || !isfinite(step_size) || !isfinite(t_begin) || !isfinite(t_end))
        return set_error(NFX_EINVAL, "cnf: times must be finite and step_size positive");
    cnf_kernel_t k = pick_cnf(save, d, H);
    if (!k)
        return set_error(NFX_EUNSUPPORTED, "cnf: d=%d H=%d outside the compiled family (d<=8, H in %s)", d, H,
                         save ? "{32,64}" : "{32,64,128}");
    CnfArgs A{};
    if (!cnf_grid(t_begin, t_end, step_size, A.g)) return set_error(NFX_EINVAL, "cnf: too many steps");
    if (B == 0) return NFX_OK;
    if (int rc = check_pointers("cnf", {packed, in, out, log_det})) return rc;
    if (save && A.g.nsteps > 0)
        if (int rc = check_pointers("cnf", {traj})) return rc;
    if (int rc = check_no_alias("cnf", in, out)) return rc;
    A.packed = packed;
    A.in = in;
    A.out = out;
    A.logdet = log_det;
    A.traj = traj;
    A.B = B;
    A.ntiles = (B + 31) / 32;
    A.accumulate = accumulate ? 1 : 0;
    const CnfLayout L = cnf_layout(d, H / 32);
    const size_t lds = (size_t)(H <= 64 ? L.w2 : L.total) * sizeof(float);
    const int threads = tile_owner_threads(A.ntiles), nw = threads / 64;
    return launch_resident((const void*)k, &A, threads, lds, (A.ntiles + nw - 1) / nw, (hipStream_t)stream,
                           save ? "cnf_save_kernel" : "cnf_kernel");
}

extern "C" int nfx_cnf_integrate(const float* packed, const float* in, float* out, float* log_det, int64_t B, int d,
                                 int H, float t_begin, float t_end, float step_size, int accumulate, void* stream) {
    return cnf_launch(false, packed, in, out, log_det, nullptr, B, d, H, t_begin, t_end, step_size, accumulate,
                      stream);
}

extern "C" int nfx_cnf_integrate_save(const float* packed, const float* in, float* out, float* log_det, float* traj,
                                      int64_t B, int d, int H, float t_begin, float t_end, float step_size,
                                      int accumulate, void* stream) {
    return cnf_launch(true, packed, in, out, log_det, traj, B, d, H, t_begin, t_end, step_size, accumulate, stream);
}

extern "C" size_t nfx_cnf_trajectory_floats(int64_t B, int d, float t_begin, float t_end, float step_size) {
    CnfGrid G{};
    if (B <= 0 || d <= 0 || !(step_size > 0.f) || !isfinite(step_size) || !isfinite(t_begin) || !isfinite(t_end) ||
        !cnf_grid(t_begin, t_end, step_size, G))
        return 0;
    return cnf_traj_floats(B, d, G.nsteps);
}

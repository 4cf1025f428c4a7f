// Backward of ContinuousFlow: the gradients of the fixed-step RK4 solve (nfx_cnf.hip) with respect
// to its input and the six parameters of the field, for d <= 8 and H in {32, 64}.
//
// The DISCRETE scheme is differentiated, not the ODE, so the gradients are those autograd gives for
// the torch composite. The saving forward (cnf_kernel<HT, D, true>) keeps y_k, the state at the
// start of every step, and the unclamped final state. The backward walks the steps k = n-1 .. 0.
// Per step it recomputes k1, k2, k3 from y_k, forms the stage inputs z2, z3, z4, and pulls the
// cotangents back through the four field evaluations in reverse stage order:
//   z4_bar = VJP(t1,         z4; dt/8 y_bar,                                     dt/8 l_bar)
//   z3_bar = VJP(t0 + 2dt/3, z3; 3dt/8 y_bar + dt z4_bar,                        3dt/8 l_bar)
//   z2_bar = VJP(t0 + dt/3,  z2; 3dt/8 y_bar - dt z4_bar + dt z3_bar,            3dt/8 l_bar)
//   z1_bar = VJP(t0,         y;  dt/8 y_bar + dt z4_bar - dt/3 z3_bar + dt/3 z2_bar, dt/8 l_bar)
//   y_bar += z1_bar + z2_bar + z3_bar + z4_bar
// (l_bar, the cotangent of the log-det, is constant over the steps; the forward's Kahan
// compensation terms carry no derivative). One VJP, with h1, h2, g1 = 1 - h1^2, g2 = 1 - h2^2,
// q = C g1 recomputed and cotangents (vb, tb) of (v, tr):
//   qb = tb g2,  a2 = g2 * (W3^T vb - 2 h2 * (tb q)),  a1 = g1 * (W2^T a2 - 2 h1 * (C^T qb)),
//   z_bar = W1[:, :d]^T a1,
//   dW3 += vb h2^T, db3 += vb, dW2 += a2 h1^T, db2 += a2, dC += qb g1^T, dW1 += a1 [z; t]^T, db1 += a1.
// Since C = W2 * N elementwise with N[k, j] = sum_i W3[i, k] W1[j, i], the finish adds, once,
//   dW2 += dC * N,  Nb = dC * W2,  dW3[i, k] += sum_j Nb[k, j] W1[j, i],  dW1[j, i] += sum_k Nb[k, j] W3[i, k].
//
// A wave owns a tile of 32 samples across all steps, as in the forward. The four H x H products of
// a VJP's data path (W2 h1, C g1, W2^T a2, C^T qb) take their A operands from LDS; the register
// file holds the dW2 and dC accumulators (16 HT^2 registers per lane each), so one wave runs per
// SIMD; the dW1 and dW3 sums are accumulator tiles kept in wave-private LDS (16 of their 32 columns,
// d + 1 <= 9 in use), read and written back around their MFMAs. The parameter products contract
// over the sample axis, which the accumulator layout keeps in lanes: h1, a2, h2 and a1 pass, one
// 32 x 32 tile at a time, through a wave-private LDS tile that returns them with the sample in the
// register index, the operand form of v_mfma_f32_32x32x2_f32 for that contraction (g1^T and g2^T
// follow elementwise).
//
// Cost per step: 3 recomputed evaluations (2 H x H products each) and 4 x (2 forward + 2 transposed
// + 2 parameter products) = 30 H x H products, against the forward's 8.
//
// No float atomics: each wave writes its partial sums to its own workspace slot, cnf_bwd_reduce
// sums the slots in index order in float64, and cnf_bwd_finish decodes the register order, applies
// the finish step and writes the six gradients in nn.Linear layout. Same inputs, same bits.
#include <math.h>

#include "nfx_cnf_bwd_kernel.h"

namespace nfx {

static bool cnf_bwd_family(int d, int H) { return d >= 1 && d <= kCnfMaxD && (H == 32 || H == 64); }

static cnf_bwd_kernel_t pick_cnf_bwd(int d, int H) {
    if (!cnf_bwd_family(d, H)) return nullptr;
    return pick_of<1, 2>(H / 32, [&](auto HT) -> cnf_bwd_kernel_t { return cnf_bwd_pick_ht<HT()>(d); });
}

// The part of the backward image behind the forward image (which nfx_cnf_pack writes).
__global__ void cnf_bwd_pack_kernel(const float* __restrict__ w1, const float* __restrict__ w2,
                                    const float* __restrict__ w3, int d, int H, float* __restrict__ packed) {
    const int HT = H / 32;
    const CnfBwdLayout L = cnf_bwd_layout(d, HT);
    for (int o = L.c2t + blockIdx.x * blockDim.x + threadIdx.x; o < L.total; o += gridDim.x * blockDim.x) {
        float v = 0.f;
        if (o < L.w1c) {  // c2t, w2t: A operands over (out row j, contraction index k) of M^T
            const bool trace = o < L.w2t;
            const RowCol e = a_image_elem(o - (trace ? L.c2t : L.w2t), HT);
            const int j = e.row, k = e.col;
            v = w2[k * H + j];
            if (trace) {  // C[k, j], rounded as the forward pack rounds it
                double n = 0.0;
                for (int i = 0; i < d; ++i) n += (double)w3[i * H + k] * (double)w1[j * (d + 1) + i];
                v = (float)((double)v * n);
            }
        } else if (o < L.w1c + d * HT * 32) {  // w1c: column i of W1
            const VecRow e = acc_rows_elem(o - L.w1c, HT);
            v = w1[e.row * (d + 1) + e.vec];
        }
        packed[o] = v;
    }
}

// tot[e] = sum over the slots, in slot order, float64.
__global__ void cnf_bwd_reduce_kernel(const float* __restrict__ ws, int nslots, int len, double* __restrict__ tot) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= len) return;
    double acc = 0.0;
    for (int sl = 0; sl < nslots; ++sl) acc += (double)ws[(size_t)sl * len + e];
    tot[e] = acc;
}

// One thread per gradient element: decode the register order, apply the finish step.
__global__ void cnf_bwd_finish_kernel(const double* __restrict__ tot, const float* __restrict__ w1,
                                      const float* __restrict__ w2, const float* __restrict__ w3, int d, int H,
                                      float* __restrict__ gw1, float* __restrict__ gb1, float* __restrict__ gw2,
                                      float* __restrict__ gb2, float* __restrict__ gw3, float* __restrict__ gb3) {
    const int HT = H / 32;
    const CnfBwdPartial P = cnf_bwd_partial(d, HT);
    const int nW2 = H * H, nW1 = H * (d + 1), nW3 = d * H;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    auto tile_hh = [&](int base, int k, int j) -> double {  // element (k, j) of a dumped H x H sum
        return tot[base + ((k >> 5) * HT + (j >> 5)) * 1024 + acc_dump_index(k & 31, j & 31)];
    };
    auto nb = [&](int k, int j) -> double { return tile_hh(P.c, k, j) * (double)w2[k * H + j]; };
    if (e < nW2) {
        const int k = e / H, j = e % H;
        double n = 0.0;
        for (int i = 0; i < d; ++i) n += (double)w3[i * H + k] * (double)w1[j * (d + 1) + i];
        gw2[e] = (float)(tile_hh(P.w2, k, j) + tile_hh(P.c, k, j) * n);
    } else if (e < nW2 + nW1) {
        const int j = (e - nW2) / (d + 1), i = (e - nW2) % (d + 1);
        double g = tot[P.g1 + (j >> 5) * 1024 + acc_dump_index(j & 31, i)];
        if (i < d)
            for (int k = 0; k < H; ++k) g += nb(k, j) * (double)w3[i * H + k];
        gw1[e - nW2] = (float)g;
    } else if (e < nW2 + nW1 + nW3) {
        const int i = (e - nW2 - nW1) / H, k = (e - nW2 - nW1) % H;
        double g = tot[P.g3 + (k >> 5) * 1024 + acc_dump_index(k & 31, i)];
        for (int j = 0; j < H; ++j) g += nb(k, j) * (double)w1[j * (d + 1) + i];
        gw3[e - nW2 - nW1] = (float)g;
    } else if (e < nW2 + nW1 + nW3 + 2 * H) {
        const int t = e - nW2 - nW1 - nW3;
        const int k = t % H, base = (t < H ? P.b1 : P.b2) + (k >> 5) * 64 + (k & 31);
        (t < H ? gb1 : gb2)[k] = (float)(tot[base] + tot[base + 32]);
    } else if (e < nW2 + nW1 + nW3 + 2 * H + d) {
        const int i = e - nW2 - nW1 - nW3 - 2 * H;
        double g = 0.0;
        for (int l = 0; l < 32; ++l) g += tot[P.b3 + i * 64 + l];
        gb3[i] = (float)g;
    }
}

// Workspace (floats): the slots, then the float64 totals of one slot's length.
static size_t cnf_bwd_ws_floats(int64_t ntiles, int d, int H) {
    const size_t len = (size_t)cnf_bwd_partial(d, H / 32).total;
    const size_t slots = (size_t)cnf_bwd_grid(ntiles) * (cnf_bwd_threads(ntiles) / 64);
    return slots * len + 2 * len;
}

}  // namespace nfx

using namespace nfx;

extern "C" int nfx_cnf_backward_supported(int64_t B, int d, int H) { return B >= 1 && cnf_bwd_family(d, H) ? 1 : 0; }

extern "C" size_t nfx_cnf_backward_packed_floats(int d, int H) {
    return cnf_bwd_family(d, H) ? (size_t)cnf_bwd_layout(d, H / 32).total : 0;
}

extern "C" size_t nfx_cnf_backward_slots(int64_t B, int d, int H) {
    if (B < 1 || !cnf_bwd_family(d, H)) return 0;
    const int64_t ntiles = (B + 31) / 32;
    return (size_t)cnf_bwd_grid(ntiles) * (cnf_bwd_threads(ntiles) / 64);
}

extern "C" size_t nfx_cnf_backward_block_threads(int64_t B, int d, int H) {
    if (B < 1 || !cnf_bwd_family(d, H)) return 0;
    return (size_t)cnf_bwd_threads((B + 31) / 32);
}

extern "C" size_t nfx_cnf_backward_workspace_floats(int64_t B, int d, int H) {
    if (B < 1 || !cnf_bwd_family(d, H)) return 0;
    return cnf_bwd_ws_floats((B + 31) / 32, d, H);
}

extern "C" int nfx_cnf_pack_backward(const float* w1, const float* b1, const float* w2, const float* b2,
                                     const float* w3, const float* b3, int d, int H, float* packed, void* stream) {
    if (d <= 0 || H <= 0) return set_error(NFX_EINVAL, "cnf_pack_backward: bad shape d=%d H=%d", d, H);
    if (!cnf_bwd_family(d, H))
        return set_error(NFX_EUNSUPPORTED, "cnf backward: d=%d H=%d outside the compiled family (d<=8, H in {32,64})", d,
                         H);
    int rc = check_pointers("cnf_pack_backward", {w1, b1, w2, b2, w3, b3, packed});
    if (rc) return rc;
    rc = nfx_cnf_pack(w1, b1, w2, b2, w3, b3, d, H, packed, stream);
    if (rc) return rc;
    const CnfBwdLayout L = cnf_bwd_layout(d, H / 32);
    cnf_bwd_pack_kernel<<<(L.total - L.c2t + 255) / 256, 256, 0, (hipStream_t)stream>>>(w1, w2, w3, d, H, packed);
    return check_launch("cnf_bwd_pack_kernel");
}

extern "C" int nfx_cnf_backward(const float* packed, const float* w1, const float* w2, const float* w3,
                                const float* in, const float* traj, const float* gy, const float* gld, float* gx,
                                float* gw1, float* gb1, float* gw2, float* gb2, float* gw3, float* gb3,
                                float* workspace, int64_t B, int d, int H, float t_begin, float t_end,
                                float step_size, void* stream) {
    if (B < 0 || d <= 0 || H <= 0)
        return set_error(NFX_EINVAL, "cnf backward: bad shape B=%lld d=%d H=%d", (long long)B, d, H);
    if (!(step_size > 0.f) || !isfinite(step_size) || !isfinite(t_begin) || !isfinite(t_end))
        return set_error(NFX_EINVAL, "cnf backward: times must be finite and step_size positive");
    cnf_bwd_kernel_t k = pick_cnf_bwd(d, H);
    if (!k)
        return set_error(NFX_EUNSUPPORTED, "cnf backward: d=%d H=%d outside the compiled family (d<=8, H in {32,64})", d,
                         H);
    CnfGrid G{};
    if (!cnf_grid(t_begin, t_end, step_size, G)) return set_error(NFX_EINVAL, "cnf backward: too many steps");
    if (B == 0) return NFX_OK;
    int rc = check_pointers("cnf backward", {gy, gx, gw1, gb1, gw2, gb2, gw3, gb3});
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (G.nsteps == 0) {  // equal times: the identity, no parameter takes part
        if (gx != gy && hipMemcpyAsync(gx, gy, sizeof(float) * (size_t)B * d, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return set_error(NFX_ELAUNCH, "cnf backward: copy failed");
        float* g[6] = {gw1, gb1, gw2, gb2, gw3, gb3};
        const size_t n[6] = {(size_t)H * (d + 1), (size_t)H, (size_t)H * H, (size_t)H, (size_t)d * H, (size_t)d};
        for (int i = 0; i < 6; ++i)
            if (hipMemsetAsync(g[i], 0, sizeof(float) * n[i], s) != hipSuccess)
                return set_error(NFX_ELAUNCH, "cnf backward: memset failed");
        return NFX_OK;
    }
    rc = check_pointers("cnf backward", {packed, w1, w2, w3, in, traj, gld, workspace});
    if (rc) return rc;
    if (gx == gy || gx == in) return set_error(NFX_EINVAL, "cnf backward: gx must not alias gy or in");
    CnfBwdArgs A{};
    A.packed = packed;
    A.x = in;
    A.traj = traj;
    A.gy = gy;
    A.gld = gld;
    A.gx = gx;
    A.ws = workspace;
    A.B = B;
    A.ntiles = (B + 31) / 32;
    A.g = G;
    const int HT = H / 32;
    const int threads = cnf_bwd_threads(A.ntiles), nw = threads / 64, grid = cnf_bwd_grid(A.ntiles);
    const size_t lds = sizeof(float) * ((size_t)cnf_bwd_layout(d, HT).total + (size_t)nw * cnf_bwd_wave_floats(HT));
    rc = prepare_lds((const void*)k, lds);
    if (rc) return rc;
    k<<<grid, threads, lds, s>>>(A);
    rc = check_launch("cnf_bwd_kernel");
    if (rc) return rc;
    const int len = cnf_bwd_partial(d, HT).total, nslots = grid * nw;
    double* tot = reinterpret_cast<double*>(workspace + (size_t)nslots * len);
    cnf_bwd_reduce_kernel<<<(len + 255) / 256, 256, 0, s>>>(workspace, nslots, len, tot);
    rc = check_launch("cnf_bwd_reduce_kernel");
    if (rc) return rc;
    const int nout = H * H + H * (d + 1) + d * H + 2 * H + d;
    cnf_bwd_finish_kernel<<<(nout + 255) / 256, 256, 0, s>>>(tot, w1, w2, w3, d, H, gw1, gb1, gw2, gb2, gw3, gb3);
    return check_launch("cnf_bwd_finish_kernel");
}

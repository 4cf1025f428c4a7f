// Backward of ResidualFlow in eval mode: the gradients of both directions with respect to the input
// and the six parameters, for 1 <= d <= 8 and 1 <= H <= 64 (padded to 32 or 64 as the forward pads).
//
// Everything runs on the effective (spectrally normalised) weights W1, W2, W3 that the pack works
// out on the device; parameter gradients are straight-through (the gradient of an effective weight
// is the parameter's, with no sigma term; u and v get none). Per sample:
//   a1 = W1 z + b1, h1 = act(a1), g1 = act'(a1), c1 = act''(a1); a2 = W2 h1 + b2, h2, g2, c2 likewise
//   T1 = diag(g1) W1 (H x d), U = W2 T1, T2 = diag(g2) U, J = W3 T2 (d x d)
//   N(z) = sum_{k=1..n} (-1)^(k+1) tr(J^k) / k
// One point evaluation P(z; vb, lb), cotangents vb of mlp(z) and lb of N(z):
//   G    = lb (sum_{k=1..n} (-1)^(k+1) J^(k-1))^T          (= dL/dJ; 0 when n = 0)
//   dT2  = W3^T G            dW3 += G T2^T + vb h2^T        db3 += vb
//   dg2  = rowsum(dT2 * U)   dU   = diag(g2) dT2
//   dT1  = W2^T dU           dg1  = rowsum(dT1 * W1)
//   ab2  = g2 * (W3^T vb) + c2 * dg2
//   ab1  = g1 * (W2^T ab2) + c1 * dg1
//   dW2 += dU T1^T + ab2 h1^T      db2 += ab2
//   dW1 += diag(g1) dT1 + ab1 z^T  db1 += ab1
//   zbar = W1^T ab1
// forward (x = z + f(z), ld = +N): P(z; gy, gld), gx = gy + zbar.
// inverse (z = g^-1(x), ld = -N): the implicit-function gradient at the returned z, not the unrolled
// iteration: P(z; 0, -gld) gives zbar and the log-det's parameter gradients; (I + J)^T w = gy + zbar
// is solved per sample in registers (LU with partial pivoting); gx = w; the parameter gradients of
// P(z; -w, 0) are added. Only z is needed, not x.
//
// A wave owns a tile of 32 samples (the shared core, nfx_tile_mlp.h), one wave per SIMD: the
// register file holds the dW2 accumulators and the h1, h2, dg1, dg2 tiles. Phase 1 computes J as
// the forward does (res_jacobian), G with the d x d powers in registers, and in the inverse
// direction the LU factors, kept by sample in LDS. Phase 2 recomputes h1 and h2 once and walks the
// tangents one at a time: T1_i, U_i = W2 T1_i, dT2_i (VALU, from the rows of W3), dT1_i = W2^T dU_i,
// and the parameter products; dg1 and dg2 are folded as it goes. Then the value-chain adjoint runs
// (twice in the inverse direction, around the solve). Products that contract over the samples
// (dW2 by MFMA; dW1, dW3 and the biases by VALU sums) take their operands through a wave-private
// LDS transposition tile.
//
// Cost per tile in H x H products: phase 1 d + ceil(d / g) (g tangents beside one value chain),
// phase 2 one for h2 and 3 d for the tangents (W2 T1_i, W2^T dU_i, dU_i T1_i^T), the adjoint 2 per
// pass (W2^T ab2, ab2 h1^T): 4 d + ceil(d / g) + 3 forward, 4 d + ceil(d / g) + 5 inverse.
//
// Padding stays exact: a padded hidden unit has h = 0 and zero weight rows and columns, so T1, U,
// dT2, dU, dT1, ab2 and ab1 are products with a zero weight there whatever act'(0) is, and the
// finish kernel writes real elements only.
//
// A row is dead when its z, a cotangent, an entry of J or a pivot of the solve is not finite (a zero
// pivot counts): it is known before any sum is touched, carries zeros through both phases and gets
// gx = 0. (A solve whose pivots are sound but whose solution overflows gets gx = 0 and adds no
// value-pass term.)
//
// No float atomics: each wave writes its partial sums to its own workspace slot, res_bwd_reduce sums
// the slots in index order in float64, res_bwd_finish writes the six gradients in nn.Linear layout.
// Same inputs, same bits. Nothing on the path reads back to the host.
#include <math.h>

#include "nfx_residual_bwd_kernel.h"

namespace nfx {

static bool res_bwd_family(int d, int H) { return d >= 1 && d <= kResMaxD && H >= 1 && H <= kResBwdMaxH; }
static bool res_bwd_activation(int a) { return a >= NFX_RESIDUAL_RELU && a <= NFX_RESIDUAL_TANH; }

static residual_bwd_kernel_t pick_res_bwd(int d, int H) {
    if (!res_bwd_family(d, H)) return nullptr;
    return pick_of<1, 2>(hidden_tiles(H), [&](auto HT) -> residual_bwd_kernel_t { return res_bwd_pick_ht<HT()>(d); });
}

// tot[e] = sum over the slots, in slot order, float64. A thread owns an element; it keeps 16 loads in
// flight and adds them in index order (up to 1,024 slots: the loop is latency, not bandwidth).
__global__ __launch_bounds__(64) void res_bwd_reduce_kernel(const float* __restrict__ ws, int nslots, int len,
                                                            double* __restrict__ tot) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= len) return;
    const float* p = ws + e;
    double acc = 0.0;
    int sl = 0;
    for (; sl + 16 <= nslots; sl += 16) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = p[(size_t)(sl + i) * len];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc += (double)v[i];
    }
    for (; sl < nslots; ++sl) acc += (double)p[(size_t)sl * len];
    tot[e] = acc;
}

// One thread per real gradient element: decode the dumped orders.
__global__ void res_bwd_finish_kernel(const double* __restrict__ tot, int d, int H, float* __restrict__ gw1,
                                      float* __restrict__ gb1, float* __restrict__ gw2, float* __restrict__ gb2,
                                      float* __restrict__ gw3, float* __restrict__ gb3) {
    const int HT = hidden_tiles(H);
    const ResBwdPartial P = res_bwd_partial(d, HT);
    const int nW2 = H * H, nW1 = H * d, nW3 = d * H;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    auto halves = [&](int base, int vec, int k) -> double {  // a [vec][HT][64] sum for hidden unit k
        const int o = base + (vec * HT + (k >> 5)) * 64 + (k & 31);
        return tot[o] + tot[o + 32];
    };
    if (e < nW2) {
        const int k = e / H, j = e % H;
        gw2[e] = (float)tot[P.w2 + ((k >> 5) * HT + (j >> 5)) * 1024 + acc_dump_index(k & 31, j & 31)];
    } else if (e < nW2 + nW1) {
        const int k = (e - nW2) / d, i = (e - nW2) % d;
        gw1[e - nW2] = (float)halves(P.g1, i, k);
    } else if (e < nW2 + nW1 + nW3) {
        const int j = (e - nW2 - nW1) / H, k = (e - nW2 - nW1) % H;
        gw3[e - nW2 - nW1] = (float)halves(P.g3, j, k);
    } else if (e < nW2 + nW1 + nW3 + 2 * H) {
        const int t = e - nW2 - nW1 - nW3;
        const int k = t % H;
        (t < H ? gb1 : gb2)[k] = (float)halves(t < H ? P.b1 : P.b2, 0, k);
    } else if (e < nW2 + nW1 + nW3 + 2 * H + d) {
        const int j = e - nW2 - nW1 - nW3 - 2 * H;
        double g = 0.0;
        for (int l = 0; l < 32; ++l) g += tot[P.b3 + j * 64 + l];
        gb3[j] = (float)g;
    }
}

static size_t res_bwd_slots(int64_t ntiles) { return (size_t)res_bwd_grid(ntiles) * (res_bwd_threads(ntiles) / 64); }

// Workspace (floats): the slots, then the float64 totals of one slot's length.
static size_t res_bwd_ws_floats(int64_t ntiles, int d, int H) {
    const size_t len = (size_t)res_bwd_partial(d, hidden_tiles(H)).total;
    return res_bwd_slots(ntiles) * len + 2 * len;
}

}  // namespace nfx

using namespace nfx;

extern "C" int nfx_residual_backward_supported(int64_t B, int d, int H, int activation) {
    return B >= 1 && res_bwd_family(d, H) && res_bwd_activation(activation) ? 1 : 0;
}

extern "C" size_t nfx_residual_backward_packed_floats(int d, int H) {
    return res_bwd_family(d, H) ? (size_t)res_bwd_layout(d, hidden_tiles(H)).total : 0;
}

extern "C" size_t nfx_residual_backward_slots(int64_t B, int d, int H) {
    if (B < 1 || !res_bwd_family(d, H)) return 0;
    return res_bwd_slots((B + 31) / 32);
}

extern "C" size_t nfx_residual_backward_block_threads(int64_t B, int d, int H) {
    if (B < 1 || !res_bwd_family(d, H)) return 0;
    return (size_t)res_bwd_threads((B + 31) / 32);
}

extern "C" size_t nfx_residual_backward_workspace_floats(int64_t B, int d, int H) {
    if (B < 1 || !res_bwd_family(d, H)) return 0;
    return res_bwd_ws_floats((B + 31) / 32, d, H);
}

extern "C" int nfx_residual_pack_backward(const float* w1, const float* b1, const float* u1, const float* v1, float c1,
                                          const float* w2, const float* b2, const float* u2, const float* v2, float c2,
                                          const float* w3, const float* b3, const float* u3, const float* v3, float c3,
                                          int d, int H, float* packed, void* stream) {
    if (d <= 0 || H <= 0) return set_error(NFX_EINVAL, "residual_pack_backward: bad shape d=%d H=%d", d, H);
    if (!res_bwd_family(d, H))
        return set_error(NFX_EUNSUPPORTED, "residual backward: d=%d H=%d outside the compiled family (d<=8, H<=64)", d,
                         H);
    if (int rc = check_pointers("residual_pack_backward", {w1, b1, u1, v1, w2, b2, u2, v2, w3, b3, u3, v3, packed}))
        return rc;
    return residual_pack_launch({w1, w2, w3}, {b1, b2, b3}, {u1, u2, u3}, {v1, v2, v3}, {c1, c2, c3}, d, H, packed, true,
                                (hipStream_t)stream);
}

extern "C" int nfx_residual_backward(const float* packed, const float* z, const float* gy, const float* gld, float* gx,
                                     float* gw1, float* gb1, float* gw2, float* gb2, float* gw3, float* gb3,
                                     float* workspace, int64_t B, int d, int H, int activation, int direction,
                                     int neumann_terms, void* stream) {
    if (B < 0 || d <= 0 || H <= 0)
        return set_error(NFX_EINVAL, "residual backward: bad shape B=%lld d=%d H=%d", (long long)B, d, H);
    if (int rc = check_direction("residual backward", direction)) return rc;
    if (neumann_terms < 0)
        return set_error(NFX_EINVAL, "residual backward: neumann_terms=%d must not be negative", neumann_terms);
    residual_bwd_kernel_t k = pick_res_bwd(d, H);
    if (!k)
        return set_error(NFX_EUNSUPPORTED, "residual backward: d=%d H=%d outside the compiled family (d<=8, H<=64)", d,
                         H);
    if (!res_bwd_activation(activation))
        return set_error(NFX_EUNSUPPORTED, "residual backward: activation=%d is not one of NFX_RESIDUAL_*", activation);
    if (B == 0) return NFX_OK;
    if (int rc = check_pointers("residual backward",
                                {packed, z, gy, gld, gx, gw1, gb1, gw2, gb2, gw3, gb3, workspace}))
        return rc;
    if (gx == gy || gx == z) return set_error(NFX_EINVAL, "residual backward: gx must not alias gy or z");
    ResBwdArgs A{};
    A.packed = packed;
    A.z = z;
    A.gy = gy;
    A.gld = gld;
    A.gx = gx;
    A.ws = workspace;
    A.B = B;
    A.ntiles = (B + 31) / 32;
    A.act = activation;
    A.inverse = direction == NFX_INVERSE ? 1 : 0;
    A.nterms = neumann_terms;
    hipStream_t s = (hipStream_t)stream;
    const int HT = hidden_tiles(H);
    const int threads = res_bwd_threads(A.ntiles), nw = threads / 64, grid = res_bwd_grid(A.ntiles);
    const size_t lds = sizeof(float) * ((size_t)res_bwd_layout(d, HT).total + (size_t)nw * res_bwd_wave(d, HT).total);
    int rc = prepare_lds((const void*)k, lds);
    if (rc) return rc;
    k<<<grid, threads, lds, s>>>(A);
    rc = check_launch("residual_bwd_kernel");
    if (rc) return rc;
    const int len = res_bwd_partial(d, HT).total, nslots = grid * nw;
    double* tot = reinterpret_cast<double*>(workspace + (size_t)nslots * len);
    res_bwd_reduce_kernel<<<(len + 63) / 64, 64, 0, s>>>(workspace, nslots, len, tot);
    rc = check_launch("res_bwd_reduce_kernel");
    if (rc) return rc;
    const int nout = H * H + 2 * H * d + 2 * H + d;
    res_bwd_finish_kernel<<<(nout + 255) / 256, 256, 0, s>>>(tot, d, H, gw1, gb1, gw2, gb2, gw3, gb3);
    return check_launch("res_bwd_finish_kernel");
}

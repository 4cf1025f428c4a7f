// ResidualFlow: x = z + f(z), f = W3 act(W2 act(W1 z + b1) + b2) + b3 with spectrally normalised
// weights, both directions in ONE launch (see nfx_residual.hip for the design notes).
#pragma once
#include <math.h>

#include "nfx_tile_mlp.h"

namespace nfx {

// Packed weight image (floats), hidden width padded to HP = 32 HT (padding rows and columns are 0;
// every activation maps 0 to 0, so the padding never reaches a result). All of it is staged in LDS.
//   w1  [HT][KS1][64]      A operand of layer 1 over k = 0..d-1, KS1 = layer1_ksteps(d) k-steps
//   b1  [HT][2][16]        layer-1 bias in accumulator order
//   b2  [HT][2][16]
//   w1c [d][HT][2][16]     column i of W1 in accumulator order: the seed of tangent i
//   w3  [d][HT][2][16]     row j of W3 in accumulator order (VALU dots)
//   b3  [up4(d)]
//   w2  [HT][HT][4][64][4] A operand of layer 2: [out tile][k tile][r/4][lane][r%4]
struct ResLayout {
    int d, HT, KS1;
    int w1, b1, b2, w1c, w3, b3, w2, total;
};

__host__ __device__ constexpr ResLayout res_layout(int d, int HT) {
    ResLayout L{};
    L.d = d;
    L.HT = HT;
    L.KS1 = layer1_ksteps(d);
    int o = 0;
    L.w1 = o; o += HT * L.KS1 * 64;
    L.b1 = o; o += HT * 32;
    L.b2 = o; o += HT * 32;
    L.w1c = o; o += d * HT * 32;
    L.w3 = o; o += d * HT * 32;
    L.b3 = o; o += (d + 3) & ~3;
    L.w2 = o; o += HT * HT * 1024;
    L.total = o;
    return L;
}

struct ResArgs {
    const float* packed;
    const float* in;
    float* out;
    float* logdet;
    int64_t B, ntiles;
    int accumulate;
    int act;        // NFX_RESIDUAL_*: the same for every wave
    int inverse;    // 0: x = z + f(z); 1: the fixed-point iteration
    int nterms;     // Neumann terms
    int max_iter;
    float tol;
};

constexpr int kResMaxD = 8;
constexpr int kResMaxH = 128;

// Tangent chains evaluated beside one value chain (the accumulator tiles of a pass are 1 + this).
constexpr int res_tangent_group(int HT, int D) {
    const int g = HT <= 1 ? 4 : 2;
    return D < g ? D : g;
}

// ---- the four activations, a tile of 16 accumulator registers at a time. `act` is uniform over
// the launch: one scalar branch per tile. The derivative is written from the activation's OUTPUT,
// in torch autograd's forms (relu out > 0; leaky_relu x > 0 ? 1 : 0.1 and elu x > 0 ? 1 : out + 1,
// where x > 0 exactly when out > 0; tanh 1 - out^2).
__device__ __forceinline__ void res_act16(int act, f32x16& a) {
    switch (act) {
        case NFX_RESIDUAL_RELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = trelu(a[r]);
            break;
        case NFX_RESIDUAL_ELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = a[r] > 0.f ? a[r] : expm1f(a[r]);
            break;
        case NFX_RESIDUAL_LEAKY_RELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = a[r] > 0.f ? a[r] : a[r] * 0.1f;
            break;
        default:
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = tanhf(a[r]);
            break;
    }
}

__device__ __forceinline__ f32x16 res_dact16(int act, const f32x16& o) {
    f32x16 g;
    switch (act) {
        case NFX_RESIDUAL_RELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = o[r] > 0.f ? 1.f : 0.f;
            break;
        case NFX_RESIDUAL_ELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = o[r] > 0.f ? 1.f : o[r] + 1.f;
            break;
        case NFX_RESIDUAL_LEAKY_RELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = o[r] > 0.f ? 1.f : 0.1f;
            break;
        default:
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = fmaf(-o[r], o[r], 1.f);
            break;
    }
    return g;
}

// One evaluation of the MLP for the wave's 32 samples: out = W3 h2 + b3 and, beside the value
// chain, NT tangent chains for the input dimensions I0 .. I0 + NT - 1,
//   Jc[t][j] = d out_j / d z_(I0 + t) = W3[j, :] . (g2 * (W2 (g1 * W1[:, I0 + t]))).
// A layer-2 A fragment is read from LDS once and feeds the value chain and every tangent chain of
// the pass.
template <int HT, int D, int NT, int I0>
__device__ __forceinline__ void res_eval(const float* sm, int act, int lane, const float (&z)[D], float (&out)[D],
                                         float (&Jc)[NT > 0 ? NT : 1][D]) {
    constexpr ResLayout L = res_layout(D, HT);
    const int h = lane >> 5;
    const int oz = opaque_zero();  // no hoisting of the LDS operands out of the caller's loops
    const float* s = sm + oz;
    const f32x4* w2l = reinterpret_cast<const f32x4*>(s + L.w2) + lane;

    // Layer 1 is layer1_preact's code written out: calling it here moved the register allocation of
    // residual_kernel<4, 6> and <4, 8> to 32 and 28 more scratch bytes per lane.
    constexpr int KS1 = L.KS1;
    float xb[KS1];
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
        const int k0 = 2 * ks, k1 = 2 * ks + 1;
        const float a = z[k0 < D ? k0 : 0];
        const float b = k1 < D ? z[k1 < D ? k1 : 0] : 0.f;
        xb[ks] = h ? b : a;
    }
    f32x16 h1[HT];
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) {
        f32x16 a = load_bias16(s + L.b1 + ht * 32, h);
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) a = mfma32(s[L.w1 + (ht * KS1 + ks) * 64 + lane], xb[ks], a);
        res_act16(act, a);
        h1[ht] = a;
    }
    __builtin_amdgcn_sched_barrier(0);
    float pv[D];
    float pj[NT > 0 ? NT : 1][D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        pv[j] = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) pj[t][j] = 0.f;
    }
#pragma unroll
    for (int hto = 0; hto < HT; ++hto) {
        f32x16 a = load_bias16(s + L.b2 + hto * 32, h);
        f32x16 c[NT > 0 ? NT : 1];
#pragma unroll
        for (int t = 0; t < NT; ++t) c[t] = f32x16{};
#pragma unroll
        for (int kt = 0; kt < HT; ++kt) {
            f32x16 g1 = {};
            if constexpr (NT > 0) g1 = res_dact16(act, h1[kt]);
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const f32x4 w = w2l[a_quad(a_tile(hto, kt, HT), rq) * 64];
                f32x4 wc[NT > 0 ? NT : 1];
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    wc[t] = *reinterpret_cast<const f32x4*>(s + L.w1c + ((I0 + t) * HT + kt) * 32 + 16 * h + 4 * rq);
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) {
                    a = mfma32(w[rr], h1[kt][4 * rq + rr], a);
#pragma unroll
                    for (int t = 0; t < NT; ++t) c[t] = mfma32(w[rr], g1[4 * rq + rr] * wc[t][rr], c[t]);
                }
            }
        }
        res_act16(act, a);
        if constexpr (NT > 0) {
            const f32x16 g2 = res_dact16(act, a);
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) c[t][r] *= g2[r];
        }
        // (the barriers keep the compiler from issuing every LDS operand of the evaluation ahead
        // of its use)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            __builtin_amdgcn_sched_barrier(0);
            const f32x16 w3 = load_bias16(s + L.w3 + (j * HT + hto) * 32, h);
            pv[j] = acc_dot16(w3, a, pv[j]);
#pragma unroll
            for (int t = 0; t < NT; ++t) pj[t][j] = acc_dot16(w3, c[t], pj[t][j]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < D; ++j) {
        out[j] = halves_sum(pv[j], pv[j]) + s[L.b3 + j];
#pragma unroll
        for (int t = 0; t < NT; ++t) Jc[t][j] = halves_sum(pj[t][j], pj[t][j]);
    }
}

// out and the full Jacobian J[j][i] = d out_j / d z_i, the tangents in groups of TG (each pass
// recomputes the value chain, whose second activation's derivative the tangents need).
template <int HT, int D, int TG, int I0>
__device__ __forceinline__ void res_jacobian(const float* sm, int act, int lane, const float (&z)[D],
                                             float (&out)[D], float (&J)[D][D]) {
    constexpr int NT = D - I0 < TG ? D - I0 : TG;
    float Jc[NT][D];
    res_eval<HT, D, NT, I0>(sm, act, lane, z, out, Jc);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < D; ++j) J[j][I0 + t] = Jc[t][j];
    if constexpr (I0 + NT < D) res_jacobian<HT, D, TG, I0 + NT>(sm, act, lane, z, out, J);
}

// sum_{k=1..n} (-1)^(k+1) tr(J^k) / k, the powers in registers, in the composite's order of
// operations: the trace, its sign, the division by k, the add; then P <- P J.
template <int D>
__device__ __forceinline__ float res_neumann(const float (&J)[D][D], int nterms) {
#pragma clang fp contract(off)
    float P[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) P[a][b] = J[a][b];
    float ld = 0.f;
#pragma unroll 1
    for (int k = 1; k <= nterms; ++k) {
        float tr = P[0][0];
#pragma unroll
        for (int a = 1; a < D; ++a) tr += P[a][a];
        ld += ((k & 1) ? tr : -tr) / (float)k;
        if (k < nterms) {
            float Q[D][D];
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b < D; ++b) {
                    float q = P[a][0] * J[0][b];
#pragma unroll
                    for (int c = 1; c < D; ++c) q = fmaf(P[a][c], J[c][b], q);
                    Q[a][b] = q;
                }
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b < D; ++b) P[a][b] = Q[a][b];
        }
    }
    return ld;
}

template <int HT, int D>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(tile_waves_per_simd(HT), tile_waves_per_simd(HT)))) void residual_kernel(ResArgs A) {
    constexpr ResLayout L = res_layout(D, HT);
    constexpr int TG = res_tangent_group(HT, D);
    extern __shared__ f32x4 lds4[];
    stage_image(lds4, A.packed, L.total / 4);
    const float* sm = reinterpret_cast<const float*>(lds4);

    const int lane = lane_id(), h = lane >> 5, col = lane & 31;
    const int nw = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int act = __builtin_amdgcn_readfirstlane(A.act);

    for (int64_t tile = (int64_t)blockIdx.x * nw + wave; tile < A.ntiles; tile += (int64_t)gridDim.x * nw) {
#pragma clang fp contract(off)  // the residual arithmetic rounds op by op, as the composite's
        const int64_t srow = tile * 32 + col;
        const bool live = srow < A.B;  // a dead column carries zeros and is never stored
        float x[D], z[D];
#pragma unroll
        for (int j = 0; j < D; ++j) z[j] = x[j] = live ? A.in[srow * D + j] : 0.f;

        if (A.inverse) {
            // z <- x - f(z) from z = x. A sample stops when its OWN step is shorter than tol and keeps
            // the iterate before that step; one that reaches max_iter keeps its last step. The wave
            // goes on while any of its live samples does; finished samples stay frozen.
            bool running = live;
#pragma unroll 1
            for (int it = 0; it < A.max_iter; ++it) {
                if (!__any(running)) break;
                float o[D], none[1][D];
                res_eval<HT, D, 0, 0>(sm, act, lane, z, o, none);
                float zn[D], ss = 0.f;
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const float f = (z[j] + o[j]) - z[j];
                    zn[j] = x[j] - f;
                    const float e = zn[j] - z[j];
                    ss += e * e;
                }
                if (sqrtf(ss) < A.tol) running = false;
#pragma unroll
                for (int j = 0; j < D; ++j) z[j] = running ? zn[j] : z[j];
            }
        }

        float o[D], J[D][D];
        res_jacobian<HT, D, TG, 0>(sm, act, lane, z, o, J);
        const float nsum = res_neumann<D>(J, A.nterms);
        float y[D];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const float f = (z[j] + o[j]) - z[j];
            y[j] = A.inverse ? z[j] : z[j] + f;
        }
        const float lo = A.inverse ? -nsum : nsum;
        if (live && h == 0) {
#pragma unroll
            for (int j = 0; j < D; ++j) A.out[srow * D + j] = y[j];
            A.logdet[srow] = A.accumulate ? A.logdet[srow] + lo : lo;
        }
    }
}

typedef void (*residual_kernel_t)(ResArgs);

// Defined once per padded width, in nfx_residual_h{1,2,4}.hip, as res_pick<HT>.
template <int HT>
residual_kernel_t res_pick_ht(int d);
template <>
residual_kernel_t res_pick_ht<1>(int d);
template <>
residual_kernel_t res_pick_ht<2>(int d);
template <>
residual_kernel_t res_pick_ht<4>(int d);

// The compiled shapes, listed here only: d = 1..kResMaxD.
template <int HT>
residual_kernel_t res_pick(int d) {
    return pick_range<1, kResMaxD>(d, [](auto D) -> residual_kernel_t { return residual_kernel<HT, D()>; });
}

}  // namespace nfx

// Continuous normalizing flow: the whole fixed-step RK4 (3/8 rule) integration of
//   dz/dt = v(z, t),  dl/dt = +tr(dv/dz),   v = W3 tanh(W2 tanh(W1 [z; t] + b1) + b2) + b3
// in ONE launch (see nfx_cnf.hip for the design notes and the cost model).
#pragma once
#include <math.h>

#include "nfx_tile_mlp.h"

namespace nfx {

// Packed weight image (floats), H = 32 HT, accumulator order = [tile][lane half][register]:
//   w1  [HT][KS1][64]      A operand of layer 1 over k = 0..d ([z; t], t is input column d),
//                          KS1 = layer1_ksteps(d + 1) k-steps, zero beyond k = d
//   b1  [HT][2][16]        layer-1 bias in accumulator order
//   b2  [HT][2][16]
//   w3  [d][HT][2][16]     W3[j, :] in accumulator order (VALU dots)
//   b3  [up4(d)]
//   c2  [HT][HT][4][64][4] A operand of the trace product, in w2's order: C = W2 * (W3^T W1[:, :d]^T)
//                          elementwise, so that tr(dv/dz) = g2^T C g1 (nfx_cnf.hip)
//   w2  [HT][HT][4][64][4] A operand of layer 2: [out tile][k tile][r/4][lane][r%4]
// Everything before w2 is staged in LDS; w2 lives in registers for H <= 64 and in LDS for H = 128.
struct CnfLayout {
    int d, HT, KS1;
    int w1, b1, b2, w3, b3, c2, w2, total;
};

__host__ __device__ constexpr CnfLayout cnf_layout(int d, int HT) {
    CnfLayout L{};
    L.d = d;
    L.HT = HT;
    L.KS1 = layer1_ksteps(d + 1);
    int o = 0;
    L.w1 = o; o += HT * L.KS1 * 64;
    L.b1 = o; o += HT * 32;
    L.b2 = o; o += HT * 32;
    L.w3 = o; o += d * HT * 32;
    L.b3 = o; o += (d + 3) & ~3;
    L.c2 = o; o += HT * HT * 1024;
    L.w2 = o; o += HT * HT * 1024;
    L.total = o;
    return L;
}

// The discrete scheme (grid, step times, stage times and stage inputs), defined once: the forward
// kernel runs it and the backward kernel (nfx_cnf_bwd_kernel.h) differentiates it, recomputing the
// inputs of stages 2..4 with the same functions, so they round exactly as the forward's. The field
// evaluation itself is written out in both kernels (DESIGN.md says why).
struct CnfGrid {
    int nsteps;         // grid points - 1; 0: equal times, the identity
    float s0, s1, h;    // ascending grid s_k = k h + s0, last point s1
    float sgn;          // t = sgn * s: -1 walks the grid downward (t_begin > t_end)
};

// The ascending grid of the fixed-step solver, in fp32 like the times tensor: n = ceil((s1 - s0)
// / h + 1) points s_k = k h + s0 with the last one pinned to s1. A decreasing interval is the
// negated-time problem (s = -t): the same grid walked downward with negative dt. False when the
// grid has too many points.
inline bool cnf_grid(float t_begin, float t_end, float step_size, CnfGrid& G) {
    G.sgn = t_begin <= t_end ? 1.f : -1.f;
    G.s0 = G.sgn * t_begin;
    G.s1 = G.sgn * t_end;
    G.h = step_size;
    G.nsteps = 0;
    if (t_begin != t_end) {
        const float n = ceilf((G.s1 - G.s0) / step_size + 1.f);  // fp32 throughout, as the composite
        if (!(n <= 16777216.f)) return false;
        G.nsteps = (int)n - 1;
    }
    return true;
}

// Step k of the grid: from t0 to t1 = t0 + dt.
struct CnfStep {
    float t0, t1, dt;
};
__device__ __forceinline__ CnfStep cnf_step(const CnfGrid& G, int k) {
#pragma clang fp contract(off)  // every mul/add rounds separately, as the torch composite's ops
    const float sk = (float)k * G.h + G.s0;
    const float sk1 = k + 1 == G.nsteps ? G.s1 : (float)(k + 1) * G.h + G.s0;
    const float t0 = G.sgn * sk, t1 = G.sgn * sk1;
    return {t0, t1, t1 - t0};
}

// Stage sg = 1..4 of the 3/8 rule, one coordinate: the stage input from the step's start y and the
// earlier stage derivatives (k_i counts for i < sg only); and the stage time. The callers pass sg
// as a constant inside their own branch on the stage.
__device__ __forceinline__ float cnf_stage_input(int sg, float dt, float y, float k1, float k2, float k3) {
#pragma clang fp contract(off)  // as cnf_step
    if (sg == 1) return y;
    if (sg == 2) return y + dt * k1 / 3.f;
    if (sg == 3) return y + dt * (k2 - k1 / 3.f);
    return y + dt * (k1 - k2 + k3);
}
__device__ __forceinline__ float cnf_stage_time(int sg, const CnfStep& S) {
#pragma clang fp contract(off)  // as cnf_step
    return sg == 1 ? S.t0 : sg == 2 ? S.t0 + S.dt / 3.f : sg == 3 ? S.t0 + 2.f * S.dt / 3.f : S.t1;
}

struct CnfArgs {
    const float* packed;
    const float* in;
    float* out;
    float* logdet;
    int64_t B, ntiles;
    int accumulate;
    CnfGrid g;
    float* traj;        // SAVE instantiations only: the trajectory the fused backward replays
};

// Trajectory of a SAVE launch (floats), nsteps = n >= 1: y_1 .. y_{n-1} step-major [n-1][B][d]
// (the state at the start of steps 1 .. n-1; y_0 is the input), then the last step's result before
// the guards, y_n [B][d] and its log-det [B]: the backward's clamp masks read those.
inline size_t cnf_traj_floats(int64_t B, int d, int nsteps) {
    return nsteps > 0 ? (size_t)nsteps * (size_t)B * d + (size_t)B : 0;
}

constexpr int kCnfMaxD = 8;

// (two waves per SIMD for H <= 64 means a handful of outer-loop spills at H = 64, d >= 6; H = 128
// runs without scratch)
template <int HT, int D, bool SAVE = false>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(tile_waves_per_simd(HT), tile_waves_per_simd(HT)))) void cnf_kernel(CnfArgs A) {
    constexpr CnfLayout L = cnf_layout(D, HT);
    constexpr bool W2REG = HT <= 2;
    constexpr int NLDS = W2REG ? L.w2 : L.total;
    extern __shared__ f32x4 lds4[];
    stage_image(lds4, A.packed, NLDS / 4);
    const float* sm = reinterpret_cast<const float*>(lds4);

    const int lane = lane_id(), h = lane >> 5, col = lane & 31;
    const int nw = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    // W2 as the layer-2 A operand: 16 HT^2 floats per lane, loaded once (H <= 64)
    f32x4 w2r[W2REG ? HT * HT * 4 : 1];
    if constexpr (W2REG) {
        const f32x4* wg = reinterpret_cast<const f32x4*>(A.packed + L.w2) + lane;
#pragma unroll
        for (int g = 0; g < HT * HT * 4; ++g) w2r[g] = wg[g * 64];
    }

    // One evaluation of the field and its exact divergence for the wave's 32 samples. The
    // divergence sum_i W3[i, :] . (g2 * (W2 (g1 * W1[:, i]))) is summed over i inside the weights:
    // it equals g2 . (C g1), ONE more H x H product beside layer 2 instead of d.
    auto field = [&](float t, const float (&z)[D], float (&v)[D], float& tr) {
        const float* s = sm + opaque_zero();  // no hoisting of the LDS operands out of the step loop
        const f32x4* w2l = reinterpret_cast<const f32x4*>(s + L.w2) + lane;
        const f32x4* c2l = reinterpret_cast<const f32x4*>(s + L.c2) + lane;
        float zt[D + 1];
#pragma unroll
        for (int j = 0; j < D; ++j) zt[j] = z[j];
        zt[D] = t;
        f32x16 h1[HT];
        layer1_preact<HT, D + 1>(s + L.w1, s + L.b1, lane, zt, h1);
#pragma unroll
        for (int ht = 0; ht < HT; ++ht)
#pragma unroll
            for (int r = 0; r < 16; ++r) h1[ht][r] = tanhf(h1[ht][r]);
        __builtin_amdgcn_sched_barrier(0);
        float pv[D];
#pragma unroll
        for (int j = 0; j < D; ++j) pv[j] = 0.f;
        float ptr = 0.f;
#pragma unroll
        for (int hto = 0; hto < HT; ++hto) {
            auto w2 = [&](int kt, int rq) -> f32x4 {
                if constexpr (W2REG) return w2r[(hto * HT + kt) * 4 + rq];
                else return w2l[a_quad(a_tile(hto, kt, HT), rq) * 64];
            };
            // h2 tile hto, and beside it the same tile of C g1 (g1 = 1 - h1^2): two independent chains
            f32x16 a = load_bias16(s + L.b2 + hto * 32, h);
            f32x16 c = {};
#pragma unroll
            for (int kt = 0; kt < HT; ++kt)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const f32x4 w = w2(kt, rq);
                    const f32x4 cw = c2l[a_quad(a_tile(hto, kt, HT), rq) * 64];
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const float hv = h1[kt][4 * rq + rr];
                        a = mfma32(w[rr], hv, a);
                        c = mfma32(cw[rr], fmaf(-hv, hv, 1.f), c);
                    }
                }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float th = tanhf(a[r]);
                a[r] = th;
                ptr = fmaf(fmaf(-th, th, 1.f), c[r], ptr);
            }
            // (the barriers keep the compiler from issuing every LDS operand of the evaluation
            // ahead of its use: that cost up to 256 AGPRs and scratch at H = 128)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                __builtin_amdgcn_sched_barrier(0);
                pv[j] = acc_dot16(s + L.w3 + (j * HT + hto) * 32, h, a, pv[j]);
                asm volatile("" : "+v"(pv[j]));  // the dots of row j end before the next barrier
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int j = 0; j < D; ++j) v[j] = halves_sum(pv[j], pv[j]) + s[L.b3 + j];
        tr = halves_sum(ptr, ptr);
    };

    for (int64_t tile = (int64_t)blockIdx.x * nw + wave; tile < A.ntiles; tile += (int64_t)gridDim.x * nw) {
        const int64_t srow = tile * 32 + col;
        const bool live = srow < A.B;  // a dead column integrates zeros and is never stored
        float x0[D], y[D];
#pragma unroll
        for (int j = 0; j < D; ++j) y[j] = x0[j] = live ? A.in[srow * D + j] : 0.f;
        float ld = 0.f;
        // State and log-det are carried across the steps as compensated (Kahan) sums: a hundred
        // fp32 adds of increments ~1e-2 into values ~1 otherwise random-walk to a few ulp, which
        // is the dominant error of an fp32 solve (the field's own rounding enters scaled by dt).
        float yc[D], ldc = 0.f;
#pragma unroll
        for (int j = 0; j < D; ++j) yc[j] = 0.f;

#pragma unroll 1
        for (int k = 0; k < A.g.nsteps; ++k) {
#pragma clang fp contract(off)  // every mul/add rounds separately, as the torch composite's ops
            const CnfStep S = cnf_step(A.g, k);
            const float dt = S.dt;
            if constexpr (SAVE) {
                if (k > 0 && live && h == 0) {
                    float* tj = A.traj + ((int64_t)(k - 1) * A.B + srow) * D;
#pragma unroll
                    for (int j = 0; j < D; ++j) tj[j] = y[j];
                }
            }
            float k1[D], k2[D], k3[D], zin[D];
            float l1 = 0.f, l2 = 0.f, l3 = 0.f;
            float t = cnf_stage_time(1, S);
#pragma unroll
            for (int j = 0; j < D; ++j) zin[j] = cnf_stage_input(1, dt, y[j], 0.f, 0.f, 0.f);
#pragma unroll 1
            for (int st = 0; st < 4; ++st) {
                float v[D], tr;
                field(t, zin, v, tr);
                if (st == 0) {
                    t = cnf_stage_time(2, S);
                    l1 = tr;
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        k1[j] = v[j];
                        zin[j] = cnf_stage_input(2, dt, y[j], k1[j], 0.f, 0.f);
                    }
                } else if (st == 1) {
                    t = cnf_stage_time(3, S);
                    l2 = tr;
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        k2[j] = v[j];
                        zin[j] = cnf_stage_input(3, dt, y[j], k1[j], k2[j], 0.f);
                    }
                } else if (st == 2) {
                    t = cnf_stage_time(4, S);
                    l3 = tr;
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        k3[j] = v[j];
                        zin[j] = cnf_stage_input(4, dt, y[j], k1[j], k2[j], k3[j]);
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        const float inc = (k1[j] + 3.f * (k2[j] + k3[j]) + v[j]) * dt * 0.125f - yc[j];
                        const float sum = y[j] + inc;
                        yc[j] = (sum - y[j]) - inc;
                        y[j] = sum;
                    }
                    const float inc = (l1 + 3.f * (l2 + l3) + tr) * dt * 0.125f - ldc;
                    const float sum = ld + inc;
                    ldc = (sum - ld) - inc;
                    ld = sum;
                }
            }
        }

        if constexpr (SAVE) {
            if (live && h == 0 && A.g.nsteps > 0) {
                float* tj = A.traj + ((int64_t)(A.g.nsteps - 1) * A.B + srow) * D;
#pragma unroll
                for (int j = 0; j < D; ++j) tj[j] = y[j];
                A.traj[(int64_t)A.g.nsteps * A.B * D + srow] = ld;
            }
        }
        if (live && h == 0) {
            float o[D];
            float lo = ld;
            if (A.g.nsteps > 0) {  // the guards (equal times return the input untouched)
#pragma unroll
                for (int j = 0; j < D; ++j) o[j] = tclamp(nonfinite(y[j]) ? x0[j] : y[j], -10.f, 10.f);
                lo = tclamp(nonfinite(ld) ? 0.f : ld, -10.f, 10.f);
            } else {
#pragma unroll
                for (int j = 0; j < D; ++j) o[j] = x0[j];
            }
#pragma unroll
            for (int j = 0; j < D; ++j) A.out[srow * D + j] = o[j];
            A.logdet[srow] = A.accumulate ? A.logdet[srow] + lo : lo;
        }
    }
}

typedef void (*cnf_kernel_t)(CnfArgs);

// Defined once per hidden width, in nfx_cnf_h{1,2,4}.hip, as cnf_pick<HT>.
template <int HT>
cnf_kernel_t cnf_pick_ht(int d);
template <>
cnf_kernel_t cnf_pick_ht<1>(int d);
template <>
cnf_kernel_t cnf_pick_ht<2>(int d);
template <>
cnf_kernel_t cnf_pick_ht<4>(int d);

// The compiled shapes, listed here only: d = 1..kCnfMaxD.
template <int HT>
cnf_kernel_t cnf_pick(int d) {
    return pick_range<1, kCnfMaxD>(d, [](auto D) -> cnf_kernel_t { return cnf_kernel<HT, D()>; });
}

// The trajectory-saving instantiations (H <= 64), defined in nfx_cnf_bwd_h{1,2}.hip.
template <int HT>
cnf_kernel_t cnf_save_pick_ht(int d);
template <>
cnf_kernel_t cnf_save_pick_ht<1>(int d);
template <>
cnf_kernel_t cnf_save_pick_ht<2>(int d);
template <int HT>
cnf_kernel_t cnf_save_pick(int d) {
    return pick_range<1, kCnfMaxD>(d, [](auto D) -> cnf_kernel_t { return cnf_kernel<HT, D(), true>; });
}

}  // namespace nfx

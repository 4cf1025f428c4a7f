// lowrank_stack_kernel<DP>: a stack of Planar / Radial / Sylvester layers at one dim, in one launch.
//
// One lane owns one sample for the whole stack: z (and, in the inverse direction, x) stay in DP
// registers from the load to the store, DP = dim padded to 2, 4, 8, 16, 32 or 64. Every layer is a
// fixed-size record of the device image (lr_record_floats(DP) floats, whatever its kind); the kind
// is a wave-uniform switch per layer and the record is read at wave-uniform addresses (plain
// loads the compiler turns into scalar loads, no LDS: the kernel uses none at all). Padding is
// exact: the padded components of w, u, z0, A and Bm are 0 and the padded components of z are 0, so
// they add 0 to every sum and stay 0; padded Sylvester transforms have A = b = S = 0, which gives
// tanh(0) = 0 and a pivot of exactly 1.
//
// The inverse is the fixed-point iteration z <- x - g(z) from z = x with the per-sample stopping
// rule of include/nfx.h. z_new depends on z through a few scalars per row only (tanh of one or
// eight dot products, or h(r)), so the step norm and the conditional update are formed from
// those scalars: z_new is never stored.
#pragma once

#include <math.h>

#include "nfx_common.h"

namespace nfx {

constexpr int kLrMaxDim = 64;
constexpr int kLrMaxTransforms = 8;
constexpr int kLrMaxIter = 1000;
constexpr int kLrMaxLayers = 256;

enum : int { kLrPlanar = 0, kLrRadial = 1, kLrSylvester = 2 };

// Record layout (floats). Header: [0] kind, [1] max_iter (both as int bits), [2] tol,
// [3] s0, [4] s1 (Planar: b, u.w; Radial: alpha, beta), [8..16) the Sylvester bias,
// [16..80) S = R R^T (8 x 8), then two blocks of 8 x DP: Planar w | u in the first 2 DP floats,
// Radial z0 in the first DP, Sylvester A (row m at m DP) and Bm^T (row m at 8 DP + m DP).
constexpr int kLrKind = 0, kLrIter = 1, kLrTol = 2, kLrS0 = 3, kLrS1 = 4, kLrBias = 8, kLrS = 16, kLrVec = 80;
__host__ __device__ constexpr int lr_record_floats(int DP) { return kLrVec + 2 * kLrMaxTransforms * DP; }
__host__ __device__ constexpr int lr_padded(int dim) {
    return dim <= 2 ? 2 : dim <= 4 ? 4 : dim <= 8 ? 8 : dim <= 16 ? 16 : dim <= 32 ? 32 : 64;
}

struct LowrankArgs {
    const float* image;
    const float* in;
    float* out;
    float* logdet;
    int64_t B;
    int dim, n_layers, inverse, accumulate;
};

// log(|det| + 1e-8) with the reference's NaN / Inf -> 0 guard.
__device__ __forceinline__ float lr_logabs(float det) {
    const float l = logf(fabsf(det) + 1e-8f);
    return nonfinite(l) ? 0.f : l;
}

// sum_j fma(j, .) over the DP components in up to eight interleaved partial sums, added as a tree:
// `fma(j, acc)` returns acc + (term j). A 64-term sequential sum would be one dependent chain (this
// kernel runs one or two waves per SIMD) and carries sqrt(8) times the rounding error.
template <int DP, class Fma>
__device__ __forceinline__ float lr_sum(Fma fma) {
    constexpr int N = DP < 8 ? DP : 8;
    float acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.f;
#pragma unroll
    for (int j = 0; j < DP; ++j) acc[j % N] = fma(j, acc[j % N]);
#pragma unroll
    for (int n = N / 2; n >= 1; n /= 2)
#pragma unroll
        for (int k = 0; k < n; ++k) acc[k] += acc[k + n];
    return acc[0];
}
template <int DP>
__device__ __forceinline__ float lr_dot(const float (&z)[DP], const float* __restrict__ w) {
    return lr_sum<DP>([&](int j, float acc) { return __builtin_fmaf(z[j], w[j], acc); });
}

// ---- Planar: g(z) = u tanh(w.z + b) ---------------------------------------------------------
template <int DP>
__device__ __forceinline__ float planar_act(const float (&z)[DP], const float* __restrict__ rec) {
    return tanhf(lr_dot<DP>(z, rec + kLrVec) + rec[kLrS0]);
}
__device__ __forceinline__ float planar_logdet(float t, const float* __restrict__ rec) {
    const float psi = 1.f - t * t;
    return lr_logabs(1.f + rec[kLrS1] * psi);
}

// ---- Radial: g(z) = beta h(r) (z - z0), h = 1 / (alpha + r + 1e-8) --------------------------
template <int DP>
__device__ __forceinline__ float radial_r(const float (&z)[DP], const float* __restrict__ rec) {
    const float* z0 = rec + kLrVec;
    return sqrtf(lr_sum<DP>([&](int j, float acc) {
        const float d = z[j] - z0[j];
        return __builtin_fmaf(d, d, acc);
    }));
}
__device__ __forceinline__ float radial_bh(float r, const float* __restrict__ rec) {
    return rec[kLrS1] * (1.0f / (rec[kLrS0] + r + 1e-8f));
}
__device__ __forceinline__ float radial_logdet(float r, int dim, const float* __restrict__ rec) {
    const float alpha = rec[kLrS0], beta = rec[kLrS1];
    const float ar = alpha + r;
    const float h = 1.0f / (ar + 1e-8f);
    const float hp = -1.0f / (ar * ar + 1e-8f);
    const float t1 = 1.f + beta * h;
    const float t2 = t1 + beta * hp * r;
    const float l = (float)(dim - 1) * logf(fabsf(t1) + 1e-8f) + logf(fabsf(t2) + 1e-8f);
    return nonfinite(l) ? 0.f : l;
}

// ---- Sylvester: g(z) = Bm tanh(A z + b) -----------------------------------------------------
template <int DP>
__device__ __forceinline__ void sylvester_act(const float (&z)[DP], const float* __restrict__ rec,
                                              float (&t)[kLrMaxTransforms]) {
#pragma unroll
    for (int m = 0; m < kLrMaxTransforms; ++m) {
        t[m] = tanhf(lr_dot<DP>(z, rec + kLrVec + m * DP) + rec[kLrBias + m]);
    }
}
// Component j of Bm t.
template <int DP>
__device__ __forceinline__ float sylvester_g(const float (&t)[kLrMaxTransforms], const float* __restrict__ rec,
                                             int j) {
    const float* bt = rec + kLrVec + kLrMaxTransforms * DP;
    float g = 0.f;
#pragma unroll
    for (int m = 0; m < kLrMaxTransforms; ++m) g = __builtin_fmaf(t[m], bt[m * DP + j], g);
    return g;
}
// log(|det(I + S diag(psi))| + 1e-8) as det(I + D^(1/2) S D^(1/2)), D = diag(psi), psi = 1 - t^2 in
// [0, 1]: symmetric positive definite with every pivot >= 1, so the unpivoted elimination below is
// stable; fully unrolled on constant indices, the matrix stays in registers.
__device__ __forceinline__ float sylvester_logdet(const float (&t)[kLrMaxTransforms], const float* __restrict__ rec) {
    constexpr int M = kLrMaxTransforms;
    float q[M], a[M][M];
#pragma unroll
    for (int m = 0; m < M; ++m) q[m] = sqrtf(1.f - t[m] * t[m]);
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = i; j < M; ++j) a[i][j] = (i == j ? 1.f : 0.f) + q[i] * rec[kLrS + i * M + j] * q[j];
    float det = 1.f;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        const float piv = a[k][k];
        det *= piv;
        const float inv = 1.0f / piv;
#pragma unroll
        for (int i = k + 1; i < M; ++i) {
            const float f = a[k][i] * inv;
#pragma unroll
            for (int j = i; j < M; ++j) a[i][j] = __builtin_fmaf(-f, a[k][j], a[i][j]);
        }
    }
    return lr_logabs(det);
}

// One fixed-point step's bookkeeping, shared by the three kinds. `step(j)` is component j of
// z_new = x - g(z); the same expression gives the norm and the update, so both see the same bits.
template <int DP, class Step>
__device__ __forceinline__ void lr_fixed_point_update(float (&z)[DP], bool& running, float tol, Step step) {
    const float s = lr_sum<DP>([&](int j, float acc) {
        const float d = step(j) - z[j];
        return __builtin_fmaf(d, d, acc);
    });
    // a NaN norm is not < tol: such a row runs to max_iter, as in the reference
    if (running && sqrtf(s) < tol) running = false;
    if (running) {
#pragma unroll
        for (int j = 0; j < DP; ++j) z[j] = step(j);
    }
}

template <int DP>
__global__ __launch_bounds__(256) void lowrank_stack_kernel(LowrankArgs A) {
    constexpr int REC = lr_record_floats(DP);
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = row < A.B;
    const int dim = A.dim;

    float z[DP];
#pragma unroll
    for (int j = 0; j < DP; ++j) z[j] = 0.f;
    if (live) {
        const float* src = A.in + row * dim;
        if (dim == DP && DP >= 4) {  // rows of 16-byte multiples on a 16-byte base (_lib.dense)
#pragma unroll
            for (int j = 0; j < DP; j += 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(src + j);
                z[j] = v[0], z[j + 1] = v[1], z[j + 2] = v[2], z[j + 3] = v[3];
            }
        } else {
#pragma unroll
            for (int j = 0; j < DP; ++j)
                if (j < dim) z[j] = src[j];
        }
    }
    float ld = (live && A.accumulate) ? A.logdet[row] : 0.f;

    for (int l = 0; l < A.n_layers; ++l) {
        const float* __restrict__ rec = A.image + (size_t)(A.inverse ? A.n_layers - 1 - l : l) * REC;
        const int kind = __builtin_amdgcn_readfirstlane(__float_as_int(rec[kLrKind]));
        if (!A.inverse) {
            if (kind == kLrPlanar) {
                const float t = planar_act<DP>(z, rec);
                const float* u = rec + kLrVec + DP;
#pragma unroll
                for (int j = 0; j < DP; ++j) z[j] = __builtin_fmaf(u[j], t, z[j]);
                ld += planar_logdet(t, rec);
            } else if (kind == kLrRadial) {
                const float r = radial_r<DP>(z, rec);
                const float bh = radial_bh(r, rec);
                const float* z0 = rec + kLrVec;
#pragma unroll
                for (int j = 0; j < DP; ++j) z[j] = __builtin_fmaf(bh, z[j] - z0[j], z[j]);
                ld += radial_logdet(r, dim, rec);
            } else {
                float t[kLrMaxTransforms];
                sylvester_act<DP>(z, rec, t);
#pragma unroll
                for (int j = 0; j < DP; ++j) z[j] += sylvester_g<DP>(t, rec, j);
                ld += sylvester_logdet(t, rec);
            }
            continue;
        }
        // inverse: z <- x - g(z) from z = x; a lane past the batch never runs
        const int max_iter = __builtin_amdgcn_readfirstlane(__float_as_int(rec[kLrIter]));
        const float tol = rec[kLrTol];
        float x[DP];
#pragma unroll
        for (int j = 0; j < DP; ++j) x[j] = z[j];
        bool running = live;
        if (kind == kLrPlanar) {
            const float* u = rec + kLrVec + DP;
            for (int it = 0; it < max_iter && __builtin_amdgcn_ballot_w64(running) != 0; ++it) {
                const float t = planar_act<DP>(z, rec);
                lr_fixed_point_update<DP>(z, running, tol, [&](int j) { return __builtin_fmaf(-u[j], t, x[j]); });
            }
            ld -= planar_logdet(planar_act<DP>(z, rec), rec);
        } else if (kind == kLrRadial) {
            const float* z0 = rec + kLrVec;
            for (int it = 0; it < max_iter && __builtin_amdgcn_ballot_w64(running) != 0; ++it) {
                const float bh = radial_bh(radial_r<DP>(z, rec), rec);
                lr_fixed_point_update<DP>(z, running, tol,
                                          [&](int j) { return __builtin_fmaf(-bh, z[j] - z0[j], x[j]); });
            }
            ld -= radial_logdet(radial_r<DP>(z, rec), dim, rec);
        } else {
            float t[kLrMaxTransforms];
            for (int it = 0; it < max_iter && __builtin_amdgcn_ballot_w64(running) != 0; ++it) {
                sylvester_act<DP>(z, rec, t);
                lr_fixed_point_update<DP>(z, running, tol, [&](int j) { return x[j] - sylvester_g<DP>(t, rec, j); });
            }
            sylvester_act<DP>(z, rec, t);
            ld -= sylvester_logdet(t, rec);
        }
    }

    if (!live) return;
    float* dst = A.out + row * dim;
    if (dim == DP && DP >= 4) {
#pragma unroll
        for (int j = 0; j < DP; j += 4) *reinterpret_cast<f32x4*>(dst + j) = f32x4{z[j], z[j + 1], z[j + 2], z[j + 3]};
    } else {
#pragma unroll
        for (int j = 0; j < DP; ++j)
            if (j < dim) dst[j] = z[j];
    }
    A.logdet[row] = ld;
}

typedef void (*lowrank_kernel_t)(LowrankArgs);
// The instantiations: nfx_lowrank_h1.hip (DP 2, 4, 8, 16), nfx_lowrank_h2.hip (32), nfx_lowrank_h3.hip (64).
lowrank_kernel_t lowrank_pick_h1(int DP);
lowrank_kernel_t lowrank_pick_h2(int DP);
lowrank_kernel_t lowrank_pick_h3(int DP);

}  // namespace nfx

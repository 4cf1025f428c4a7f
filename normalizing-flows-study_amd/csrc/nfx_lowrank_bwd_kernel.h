// lowrank_bwd_kernel<DP>: the reverse sweep of a Planar / Radial / Sylvester stack, one lane per row,
// the same DP padding and the same record image at wave-uniform addresses as lowrank_stack_kernel.
//
// NFX_FORWARD (one layer): at the layer's input z with the cotangents (y_bar, l_bar) of (y, ld) it
// forms z_bar = y_bar + J_g^T y_bar + l_bar dld/dz and the gradients of the RECORD entries.
// NFX_INVERSE (a whole stack): `point` is the stack's OUTPUT z. The inverse ran the layers
// L-1 ... 0, so the sweep visits 0 ... L-1; at layer l's output z
//     lam~ = z_bar - l_bar dld/dz,   x_bar = (I + J_g)^-T lam~   (the implicit-function gradient),
//     record gradients = -(dg/dtheta)^T x_bar - l_bar dld/dtheta,
// then z <- z + g(z) is the next layer's output (equal to layer l's input to within its tol) and
// x_bar its cotangent: O(1) memory per row, z and its cotangent in registers the whole way.
// (I + J_g)^-T is the closed rank-one formula for Planar and Radial (its denominators are the terms
// whose log the log-det takes) and, for Sylvester, the adjoint fixed-point iteration
// lam <- lam~ - A^T diag(psi) Bm^T lam at the frozen z with the layer's max_iter and a per-row stop at
// ||step|| <= tol ||lam~||: the forward iteration's contraction and cost. The stop is relative to lam~
// alone, so the result scales with the cotangents exactly as the gradient does.
//
// log(|d| + 1e-8) differentiates to sign(d) / (|d| + 1e-8), sign(0) = 0; a log-det the forward guard
// set to 0 takes no l_bar; r = 0 gives dr/dz = 0. The Sylvester log-det gradient comes from the SPD
// matrix N = I + D^1/2 S D^1/2 the forward eliminates: with Z = D^1/2 N^-1 D^1/2,
// (I + S D)^-1 = I - S Z and (I + S D)^-1 S = S - S Z S; nothing is divided by sqrt(psi).
//
// A row with a non-finite z, cotangent or coefficient at some layer adds nothing to that layer's or
// any later layer's record gradients and gets gx = 0 (autograd gives NaN there).
//
// Reduction over rows, deterministic, no float atomics: a workgroup is ONE wave; workgroup g owns the
// 64-row chunks g, g + G, g + 2G, ... and keeps the stack's gradient image (n_layers records, the
// record layout itself) in LDS. Per chunk and layer the lanes stage their row's z and cotangent
// (V0, V1) and 16 coefficients (C) in LDS; every record-vector gradient is sum_rows C[row][m] V[row][j],
// and lane e owns fixed entries (m, j) of it, summed over the 64 rows in row order. The workgroup
// writes its image once to its workspace slot; lowrank_bwd_reduce_kernel adds the slots in order.
//   image[l] layout: [0..8) column sums of C[8..16), [8..16) column sums of C[0..8), [16..80) S_bar,
//   [80 ..) G0[m][j] = sum C[m] V0[j] (w_bar | A_bar), then G1[m][j] = sum C[8+m] V1[j] (u_bar | Bm^T_bar).
#pragma once

#include "nfx_lowrank_kernel.h"

namespace nfx {

constexpr int kLrBwdRows = 64;          // rows per chunk: one wave
constexpr int kLrBwdMaxSlots = 1024;    // workgroups (workspace slots) at most
constexpr int kLrBwdCoefs = 16, kLrBwdCoefStride = 17, kLrBwdSStride = 65;
constexpr size_t kLrBwdLdsBudget = 160 * 1024;  // the one place the LDS budget is set

__host__ __device__ constexpr int lr_bwd_stage_floats(int DP) {
    return 2 * kLrBwdRows * (DP + 1) + kLrBwdRows * kLrBwdCoefStride + kLrBwdRows * kLrBwdSStride;
}
__host__ __device__ constexpr size_t lr_bwd_lds_bytes(int DP, int n_layers) {
    return ((size_t)n_layers * lr_record_floats(DP) + lr_bwd_stage_floats(DP)) * sizeof(float);
}
inline int lr_bwd_max_layers(int DP) {
    const size_t n = (kLrBwdLdsBudget - lr_bwd_stage_floats(DP) * sizeof(float)) / (lr_record_floats(DP) * sizeof(float));
    return n > (size_t)kLrMaxLayers ? kLrMaxLayers : (int)n;
}

// The pointers are separate __restrict__ kernel arguments, not members of the struct: the image is
// then known not to alias the gx stores inside the chunk loop, and its wave-uniform reads stay scalar
// loads as in lowrank_stack_kernel (which stores only at its end).
struct LowrankBwdArgs {
    int64_t B, n_chunks;
    int dim, n_layers, inverse;
};

__device__ __forceinline__ float lr_sign(float d) { return d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f; }
// d/dd log(|d| + 1e-8)
__device__ __forceinline__ float lr_dlogabs(float d) { return lr_sign(d) / (fabsf(d) + 1e-8f); }
// 0 for finite v, NaN otherwise, added to acc
__device__ __forceinline__ float lr_taint(float v, float acc) { return __builtin_fmaf(0.f, v, acc); }

template <int DP>
__device__ __forceinline__ bool lr_rows_finite(const float (&z)[DP], const float (&v)[DP], float lb) {
    const float s = lr_sum<DP>([&](int j, float acc) { return lr_taint(z[j], lr_taint(v[j], acc)); });
    return lr_taint(lb, s) == 0.f;
}

template <int DP>
__global__ __launch_bounds__(kLrBwdRows) void lowrank_bwd_kernel(
    const float* __restrict__ image,  // the stack's records
    const float* __restrict__ point,  // forward: the layer's input; inverse: the stack's output
    const float* __restrict__ gv,     // cotangent of the values [B, dim]
    const float* __restrict__ gld,    // cotangent of the log-det [B]
    float* __restrict__ gx, float* __restrict__ slots /* [gridDim.x][n_layers * REC] */, LowrankBwdArgs A) {
    constexpr int REC = lr_record_floats(DP);
    constexpr int M = kLrMaxTransforms;
    constexpr int VS = DP + 1;
    extern __shared__ float lds[];
    const int lane = threadIdx.x;
    const int dim = A.dim;
    const int total = A.n_layers * REC;
    float* img = lds;
    float* V0 = lds + total;
    float* V1 = V0 + kLrBwdRows * VS;
    float* C = V1 + kLrBwdRows * VS;
    float* SS = C + kLrBwdRows * kLrBwdCoefStride;

    for (int o = lane; o < total; o += kLrBwdRows) img[o] = 0.f;
    const float sg = A.inverse ? -1.f : 1.f;

    for (int64_t chunk = blockIdx.x; chunk < A.n_chunks; chunk += gridDim.x) {
        const int64_t row = chunk * kLrBwdRows + lane;
        const bool live = row < A.B;
        float z[DP], v[DP];
#pragma unroll
        for (int j = 0; j < DP; ++j) z[j] = 0.f, v[j] = 0.f;
        float lb = 0.f;
        if (live) {
            const float* pz = point + row * dim;
            const float* pv = gv + row * dim;
            if (dim == DP && DP >= 4) {
#pragma unroll
                for (int j = 0; j < DP; j += 4) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(pz + j);
                    const f32x4 b = *reinterpret_cast<const f32x4*>(pv + j);
                    z[j] = a[0], z[j + 1] = a[1], z[j + 2] = a[2], z[j + 3] = a[3];
                    v[j] = b[0], v[j + 1] = b[1], v[j + 2] = b[2], v[j + 3] = b[3];
                }
            } else {
#pragma unroll
                for (int j = 0; j < DP; ++j)
                    if (j < dim) z[j] = pz[j], v[j] = pv[j];
            }
            lb = gld[row];
        }
        bool dead = !live;

        for (int l = 0; l < A.n_layers; ++l) {
            const float* __restrict__ rec = image + (size_t)l * REC;
            const int kind = __builtin_amdgcn_readfirstlane(__float_as_int(rec[kLrKind]));
            float* gimg = img + l * REC;
            dead = dead || !lr_rows_finite<DP>(z, v, lb);
            float c[kLrBwdCoefs];
#pragma unroll
            for (int k = 0; k < kLrBwdCoefs; ++k) c[k] = 0.f;
            int nvec = 1;
            float chk = 0.f;

            if (kind == kLrPlanar) {
                const float* w = rec + kLrVec;
                const float* u = w + DP;
                const float t = planar_act<DP>(z, rec);
                const float psi = 1.f - t * t, uw = rec[kLrS1];
                const float D = 1.f + uw * psi;
                const float lbe = nonfinite(logf(fabsf(D) + 1e-8f)) ? 0.f : lb;
                const float sD = lr_dlogabs(D);
                const float le = lbe * sD * uw * (-2.f * t * psi);  // l_bar dld/da, a = w.z + b
                if (A.inverse) {
                    const float s = lr_sum<DP>(
                        [&](int j, float acc) { return __builtin_fmaf(u[j], __builtin_fmaf(-le, w[j], v[j]), acc); });
                    const float k = le + psi * s / D;
#pragma unroll
                    for (int j = 0; j < DP; ++j) v[j] = __builtin_fmaf(-k, w[j], v[j]);
                }
                const float abar = __builtin_fmaf(lr_dot<DP>(v, u), psi, le);
                c[0] = sg * abar;
                c[8] = sg * t;
                c[9] = sg * lbe * sD * psi;
#pragma unroll
                for (int j = 0; j < DP; ++j) V0[lane * VS + j] = z[j], V1[lane * VS + j] = v[j];
                if (A.inverse) {
#pragma unroll
                    for (int j = 0; j < DP; ++j) z[j] = __builtin_fmaf(u[j], t, z[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < DP; ++j) v[j] = __builtin_fmaf(abar, w[j], v[j]);
                }
            } else if (kind == kLrRadial) {
                const float* z0 = rec + kLrVec;
                const float alpha = rec[kLrS0], beta = rec[kLrS1];
                const float r = radial_r<DP>(z, rec);
                const float ar = alpha + r;
                const float h = 1.0f / (ar + 1e-8f);
                const float hp = -1.0f / (ar * ar + 1e-8f);
                const float dh = -h * h;            // the true dh/dr
                const float dhp = 2.f * ar * hp * hp;  // d hp / dr = d hp / d alpha
                const float t1 = 1.f + beta * h;
                const float t2 = t1 + beta * hp * r;
                const float ldv = (float)(dim - 1) * logf(fabsf(t1) + 1e-8f) + logf(fabsf(t2) + 1e-8f);
                const float lbe = nonfinite(ldv) ? 0.f : lb;
                const float s1 = (float)(dim - 1) * lr_dlogabs(t1), s2 = lr_dlogabs(t2);
                const float bdh = beta * dh;
                const float ld_r = s1 * bdh + s2 * (bdh + beta * (dhp * r + hp));
                const float ld_a = s1 * bdh + s2 * (bdh + beta * r * dhp);
                const float ld_b = s1 * h + s2 * (h + hp * r);
                const float invr = r > 0.f ? 1.0f / r : 0.f;
                if (A.inverse) {
                    const float kl = lbe * ld_r * invr;  // lam~ = v - kl d
                    const float dl = lr_sum<DP>([&](int j, float acc) {
                        const float d = z[j] - z0[j];
                        return __builtin_fmaf(d, __builtin_fmaf(-kl, d, v[j]), acc);
                    });
                    const float it1 = 1.0f / t1;
                    const float kd = kl * it1 + bdh * invr * dl * it1 / (t1 + bdh * r);
#pragma unroll
                    for (int j = 0; j < DP; ++j) v[j] = __builtin_fmaf(v[j], it1, -kd * (z[j] - z0[j]));
                }
                const float dv = lr_sum<DP>([&](int j, float acc) { return __builtin_fmaf(z[j] - z0[j], v[j], acc); });
                const float kappa = (bdh * dv + lbe * ld_r) * invr;
                const float bh = beta * h;
                c[0] = sg * kappa;
                c[8] = sg * bh;
                c[9] = sg * (bdh * dv + lbe * ld_a);
                c[10] = sg * (h * dv + lbe * ld_b);
#pragma unroll
                for (int j = 0; j < DP; ++j) V0[lane * VS + j] = z[j], V1[lane * VS + j] = v[j];
                if (A.inverse) {
#pragma unroll
                    for (int j = 0; j < DP; ++j) z[j] = __builtin_fmaf(bh, z[j] - z0[j], z[j]);
                } else {
#pragma unroll
                    for (int j = 0; j < DP; ++j) v[j] = __builtin_fmaf(bh, v[j], __builtin_fmaf(kappa, z[j] - z0[j], v[j]));
                }
            } else {
                nvec = M;
                const float* am = rec + kLrVec;
                const float* bt = am + M * DP;
                float t[M], psi[M], le[M];
                sylvester_act<DP>(z, rec, t);
#pragma unroll
                for (int m = 0; m < M; ++m) psi[m] = 1.f - t[m] * t[m];
                // z and the cotangent wait in their staging rows while the 8 x 8 work and the adjoint
                // iteration need the registers: the solve needs z through t and psi only
#pragma unroll
                for (int j = 0; j < DP; ++j) V0[lane * VS + j] = z[j], V1[lane * VS + j] = v[j];
                wave_lds_sync();
                {
                    // N^-1 by unpivoted Gauss-Jordan (N = I + D^1/2 S D^1/2 is SPD, every pivot >= 1), then
                    // Z = D^1/2 N^-1 D^1/2 in place
                    float q[M], a[M][M];
#pragma unroll
                    for (int m = 0; m < M; ++m) q[m] = sqrtf(psi[m]);
#pragma unroll
                    for (int i = 0; i < M; ++i)
#pragma unroll
                        for (int j = 0; j < M; ++j) a[i][j] = (i == j ? 1.f : 0.f) + q[i] * rec[kLrS + i * M + j] * q[j];
                    float det = 1.f;
#pragma unroll
                    for (int k = 0; k < M; ++k) {
                        const float piv = a[k][k];
                        det *= piv;
                        const float inv = 1.0f / piv;
                        a[k][k] = 1.f;
#pragma unroll
                        for (int j = 0; j < M; ++j) a[k][j] *= inv;
#pragma unroll
                        for (int i = 0; i < M; ++i) {
                            if (i == k) continue;
                            const float f = a[i][k];
                            a[i][k] = 0.f;
#pragma unroll
                            for (int j = 0; j < M; ++j) a[i][j] = __builtin_fmaf(-f, a[k][j], a[i][j]);
                        }
                    }
                    const float adet = fabsf(det);
                    const float lbf = nonfinite(logf(adet + 1e-8f)) ? 0.f : lb * (adet / (adet + 1e-8f));
#pragma unroll
                    for (int i = 0; i < M; ++i)
#pragma unroll
                        for (int j = 0; j < M; ++j) a[i][j] *= q[i] * q[j];
                    // row j of S Z: W[j][.] = delta - (S Z)[j][.], S_bar[i][j] = psi_j W[j][i], (W S)_jj
#pragma unroll
                    for (int j = 0; j < M; ++j) {
                        float wsjj = rec[kLrS + j * M + j];
#pragma unroll
                        for (int i = 0; i < M; ++i) {
                            float sz = 0.f;
#pragma unroll
                            for (int k = 0; k < M; ++k) sz = __builtin_fmaf(rec[kLrS + j * M + k], a[k][i], sz);
                            wsjj = __builtin_fmaf(-sz, rec[kLrS + i * M + j], wsjj);
                            const float sb = sg * lbf * psi[j] * ((i == j ? 1.f : 0.f) - sz);
                            chk = lr_taint(sb, chk);
                            SS[lane * kLrBwdSStride + i * M + j] = sb;
                        }
                        le[j] = lbf * wsjj * (-2.f * t[j] * psi[j]);
                    }
                }
                wave_lds_sync();
#pragma unroll
                for (int j = 0; j < DP; ++j) v[j] = V1[lane * VS + j];
                if (A.inverse) {
                    const int max_iter = __builtin_amdgcn_readfirstlane(__float_as_int(rec[kLrIter]));
                    float lam0[DP];
#pragma unroll
                    for (int j = 0; j < DP; ++j) {
                        float s = v[j];
#pragma unroll
                        for (int m = 0; m < M; ++m) s = __builtin_fmaf(-le[m], am[m * DP + j], s);
                        lam0[j] = s;
                        v[j] = s;
                    }
                    const float n0 = sqrtf(lr_sum<DP>([&](int j, float acc) { return __builtin_fmaf(lam0[j], lam0[j], acc); }));
                    // relative to the right-hand side alone: the solve is linear in it, and the cotangents of
                    // a mean over 2^20 rows are of order 1e-6, where any absolute floor would stop at once
                    const float thr = rec[kLrTol] * n0;
                    bool running = !dead && n0 == n0 && !nonfinite(n0);
                    for (int it = 0; it < max_iter && __builtin_amdgcn_ballot_w64(running) != 0; ++it) {
                        float s[M];
#pragma unroll
                        for (int m = 0; m < M; ++m) s[m] = psi[m] * lr_dot<DP>(v, bt + m * DP);
                        auto step = [&](int j) {
                            float acc = lam0[j];
#pragma unroll
                            for (int m = 0; m < M; ++m) acc = __builtin_fmaf(-s[m], am[m * DP + j], acc);
                            return acc;
                        };
                        const float dn = lr_sum<DP>([&](int j, float acc) {
                            const float d = step(j) - v[j];
                            return __builtin_fmaf(d, d, acc);
                        });
                        if (running) {
#pragma unroll
                            for (int j = 0; j < DP; ++j) v[j] = step(j);
                            if (!(sqrtf(dn) > thr)) running = false;  // (a zero or NaN step stops too)
                        }
                    }
                }
                float abar[M];
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    abar[m] = __builtin_fmaf(lr_dot<DP>(v, bt + m * DP), psi[m], le[m]);
                    c[m] = sg * abar[m];
                    c[8 + m] = sg * t[m];
                }
#pragma unroll
                for (int j = 0; j < DP; ++j) V1[lane * VS + j] = v[j];
                if (A.inverse) {
#pragma unroll
                    for (int j = 0; j < DP; ++j) z[j] = V0[lane * VS + j] + sylvester_g<DP>(t, rec, j);
                } else {
#pragma unroll
                    for (int j = 0; j < DP; ++j) {
                        float s = v[j];
#pragma unroll
                        for (int m = 0; m < M; ++m) s = __builtin_fmaf(abar[m], am[m * DP + j], s);
                        v[j] = s;
                    }
                }
            }

            // the row's coefficients and its new cotangent decide whether it counts at all
#pragma unroll
            for (int k = 0; k < kLrBwdCoefs; ++k) chk = lr_taint(c[k], chk);
            chk = lr_sum<DP>([&](int j, float acc) { return lr_taint(v[j], acc); }) + chk;
            dead = dead || !(chk == 0.f);
#pragma unroll
            for (int k = 0; k < kLrBwdCoefs; ++k) C[lane * kLrBwdCoefStride + k] = dead ? 0.f : c[k];
            if (dead) {
#pragma unroll
                for (int j = 0; j < DP; ++j) V0[lane * VS + j] = 0.f, V1[lane * VS + j] = 0.f;
                if (kind == kLrSylvester)
                    for (int k = 0; k < M * M; ++k) SS[lane * kLrBwdSStride + k] = 0.f;
            }
            wave_lds_sync();

            // lane e owns entries e, e + 64, ... of G0 and G1, summed over the rows in row order
            const int nent = nvec * DP;
            for (int e = lane; e < nent; e += kLrBwdRows) {
                const int m = e / DP, j = e - m * DP;
                float g0 = 0.f, g1 = 0.f;
#pragma unroll 8
                for (int r = 0; r < kLrBwdRows; ++r) {
                    g0 = __builtin_fmaf(C[r * kLrBwdCoefStride + m], V0[r * VS + j], g0);
                    g1 = __builtin_fmaf(C[r * kLrBwdCoefStride + 8 + m], V1[r * VS + j], g1);
                }
                gimg[kLrVec + e] += g0;
                gimg[kLrVec + M * DP + e] += g1;
            }
            if (lane < kLrBwdCoefs) {
                float s = 0.f;
#pragma unroll 8
                for (int r = 0; r < kLrBwdRows; ++r) s += C[r * kLrBwdCoefStride + lane];
                gimg[lane < 8 ? 8 + lane : lane - 8] += s;
            }
            if (kind == kLrSylvester) {
                float s = 0.f;
#pragma unroll 8
                for (int r = 0; r < kLrBwdRows; ++r) s += SS[r * kLrBwdSStride + lane];
                gimg[kLrS + lane] += s;
            }
            wave_lds_sync();
        }

        if (live) {
            float* dst = gx + row * dim;
#pragma unroll
            for (int j = 0; j < DP; ++j)
                if (j < dim) dst[j] = dead ? 0.f : v[j];
        }
    }

    float* slot = slots + (size_t)blockIdx.x * total;
    for (int o = lane; o < total; o += kLrBwdRows) slot[o] = img[o];
}

typedef void (*lowrank_bwd_kernel_t)(const float*, const float*, const float*, const float*, float*, float*,
                                     LowrankBwdArgs);
// The instantiations: nfx_lowrank_bwd_h1.hip (DP 2, 4, 8, 16), _h2.hip (32), _h3.hip (64).
lowrank_bwd_kernel_t lowrank_bwd_pick_h1(int DP);
lowrank_bwd_kernel_t lowrank_bwd_pick_h2(int DP);
lowrank_bwd_kernel_t lowrank_bwd_pick_h3(int DP);

}  // namespace nfx

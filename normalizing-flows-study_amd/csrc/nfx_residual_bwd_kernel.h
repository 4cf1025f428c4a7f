// Backward of ResidualFlow in eval mode: the gradients of x = z + f(z) and of the Neumann log-det
// with respect to the input and the six (effective) parameters, one launch (see
// nfx_residual_bwd.hip for the recurrences and the cost model).
#pragma once
#include "nfx_residual_kernel.h"

namespace nfx {

// Packed image of the backward (floats): the forward image (res_layout, bit for bit what
// nfx_residual_pack writes), then
//   w2t [HT][HT][4][64][4]  A operand of W2^T x: the w2 order with (W2^T)[j, k] = W2[k, j]
// Every other operand of the backward is already in the forward image: the rows of W3 and the
// columns of W1 in accumulator order serve the VALU products W3^T v and W1^T a.
struct ResBwdLayout {
    ResLayout F;
    int w2t, total;
};

__host__ __device__ constexpr ResBwdLayout res_bwd_layout(int d, int HT) {
    ResBwdLayout L{};
    L.F = res_layout(d, HT);
    L.w2t = L.F.total;
    L.total = (L.w2t + HT * HT * 1024 + 3) & ~3;
    return L;
}

// Wave-private LDS behind the image:
//   tb  [32][33]     the transposition tile between "hidden rows x sample lanes" and "sample rows x
//                    hidden lanes" (pitch 33)
//   zs  [d][32]      the point z by sample
//   vs  [d][32]      the value cotangent vb by sample
//   gs  [d * d][32]  G = dL/dJ by sample, entry (j, i) at j d + i
//   ms  [d * d][32]  the LU factors of (I + J)^T by sample (inverse only)
//   g1  [d][HT][64]  the wave's dW1 sums: lane l holds half (l >> 5) of the sum of column i for
//                    hidden unit 32 ht + (l & 31)
constexpr int kResBwdPitch = 33;
struct ResBwdWave {
    int zs, vs, gs, ms, g1, total;
};
__host__ __device__ constexpr ResBwdWave res_bwd_wave(int d, int HT) {
    ResBwdWave W{};
    int o = 32 * kResBwdPitch;
    W.zs = o; o += d * 32;
    W.vs = o; o += d * 32;
    W.gs = o; o += d * d * 32;
    W.ms = o; o += d * d * 32;
    W.g1 = o; o += d * HT * 64;
    W.total = o;
    return W;
}

// One wave's partial sums (floats), decoded by the finish kernel:
//   w2     [HT][HT][16][64]  dW2 tile (kt, jt) in register order: register r of lane l is element
//                            (32 kt + crow(r, l >> 5), 32 jt + (l & 31))
//   g1     [d][HT][64]       dW1[32 ht + (l & 31)][i], the two lane halves to be added
//   g3     [d][HT][64]       dW3[j][32 ht + (l & 31)], likewise
//   b1, b2 [HT][64]          likewise for hidden unit 32 ht + (l & 31)
//   b3     [d][64]           per-lane sums over the lane's samples (lanes 0..31 count)
struct ResBwdPartial {
    int w2, g1, g3, b1, b2, b3, total;
};

__host__ __device__ constexpr ResBwdPartial res_bwd_partial(int d, int HT) {
    ResBwdPartial P{};
    int o = 0;
    P.w2 = o; o += HT * HT * 1024;
    P.g1 = o; o += d * HT * 64;
    P.g3 = o; o += d * HT * 64;
    P.b1 = o; o += HT * 64;
    P.b2 = o; o += HT * 64;
    P.b3 = o; o += d * 64;
    P.total = o;
    return P;
}

// Launch shape, fixed on the host and independent of the device so that the workspace size is: a
// wave per 32-row tile up to kResBwdMaxWaves (one wave per SIMD of 256 CUs); one-wave workgroups
// while every tile can have a CU of its own, four waves sharing one staged image beyond.
constexpr int kResBwdMaxWaves = 1024;
constexpr int kResBwdWideTiles = 256;
constexpr int kResBwdMaxH = 64;
inline int res_bwd_threads(int64_t ntiles) { return ntiles > kResBwdWideTiles ? 256 : 64; }
inline int res_bwd_grid(int64_t ntiles) {
    const int nw = res_bwd_threads(ntiles) / 64;
    const int64_t g = (ntiles + nw - 1) / nw;
    return (int)(g < kResBwdMaxWaves / nw ? g : kResBwdMaxWaves / nw);
}
// The largest launch keeps the image and four waves' tables inside one CU's 160 KiB of LDS.
static_assert(4 * (res_bwd_layout(kResMaxD, 2).total + 4 * res_bwd_wave(kResMaxD, 2).total) <= 160 * 1024,
              "the backward's LDS footprint fits a CU");

struct ResBwdArgs {
    const float* packed;
    const float* z;      // [B][d]: the forward's input (forward) or its output (inverse)
    const float* gy;     // [B][d]
    const float* gld;    // [B]
    float* gx;           // [B][d]
    float* ws;           // [grid * waves][ResBwdPartial::total]
    int64_t B, ntiles;
    int act;             // NFX_RESIDUAL_*: the same for every wave
    int inverse;
    int nterms;
};

// act'' from the activation's OUTPUT, as autograd differentiates res_dact16's forms: 0 for relu and
// leaky_relu; elu 0 where out > 0, else out + 1; tanh -2 out (1 - out^2).
__device__ __forceinline__ f32x16 res_ddact16(int act, const f32x16& o) {
    f32x16 c;
    switch (act) {
        case NFX_RESIDUAL_ELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) c[r] = o[r] > 0.f ? 0.f : o[r] + 1.f;
            break;
        case NFX_RESIDUAL_TANH:
#pragma unroll
            for (int r = 0; r < 16; ++r) c[r] = -2.f * o[r] * fmaf(-o[r], o[r], 1.f);
            break;
        default:
#pragma unroll
            for (int r = 0; r < 16; ++r) c[r] = 0.f;
            break;
    }
    return c;
}

// A tile as a value the compiler cannot trace. act' and act'' of h1 and h2 do not change over the
// tangent loop; left alone, the compiler computes all four activations' forms of them ahead of the
// loop and keeps them live through it, in scratch.
__device__ __forceinline__ f32x16 opaque_tile(f32x16 x) {
    asm volatile("" : "+v"(x));
    return x;
}

// LU factors of M in place (unit lower triangle below the diagonal), rows exchanged whole as the
// pivots are chosen (partial pivoting, piv[c] = the row that column c took). False when a pivot is
// zero or not finite.
template <int D>
__device__ __forceinline__ bool res_lu(float (&M)[D][D], int (&piv)[D]) {
    bool ok = true;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        int p = c;
        float best = fabsf(M[c][c]);
#pragma unroll
        for (int r = c + 1; r < D; ++r) {
            const float v = fabsf(M[r][c]);
            if (v > best) {
                best = v;
                p = r;
            }
        }
        piv[c] = p;
#pragma unroll
        for (int r = c + 1; r < D; ++r) {
            const bool sw = p == r;
#pragma unroll
            for (int b = 0; b < D; ++b) {
                const float t = M[c][b];
                M[c][b] = sw ? M[r][b] : t;
                M[r][b] = sw ? t : M[r][b];
            }
        }
        const float pv = M[c][c];
        ok = ok && pv != 0.f && !nonfinite(pv);
        const float inv = 1.f / pv;
#pragma unroll
        for (int r = c + 1; r < D; ++r) {
            const float f = M[r][c] * inv;
            M[r][c] = f;
#pragma unroll
            for (int b = c + 1; b < D; ++b) M[r][b] = fmaf(-f, M[c][b], M[r][b]);
        }
    }
    return ok;
}

// x <- M^-1 x from res_lu's factors.
template <int D>
__device__ __forceinline__ void res_lu_solve(const float (&M)[D][D], const int (&piv)[D], float (&x)[D]) {
#pragma unroll
    for (int c = 0; c < D; ++c)
#pragma unroll
        for (int r = c + 1; r < D; ++r) {
            const bool sw = piv[c] == r;
            const float t = x[c];
            x[c] = sw ? x[r] : t;
            x[r] = sw ? t : x[r];
        }
#pragma unroll
    for (int c = 0; c < D; ++c)
#pragma unroll
        for (int r = c + 1; r < D; ++r) x[r] = fmaf(-M[r][c], x[c], x[r]);
#pragma unroll
    for (int c = D - 1; c >= 0; --c) {
        float s = x[c];
#pragma unroll
        for (int b = c + 1; b < D; ++b) s = fmaf(-M[c][b], x[b], s);
        x[c] = s / M[c][c];
    }
}

template <int HT, int D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void residual_bwd_kernel(ResBwdArgs A) {
    constexpr ResBwdLayout L = res_bwd_layout(D, HT);
    constexpr ResLayout F = L.F;
    constexpr ResBwdWave W = res_bwd_wave(D, HT);
    constexpr ResBwdPartial P = res_bwd_partial(D, HT);
    constexpr int TG = res_tangent_group(HT, D);
    constexpr int PITCH = kResBwdPitch;
    constexpr int KS1 = F.KS1;
    extern __shared__ f32x4 lds4[];
    stage_image(lds4, A.packed, L.total / 4);
    float* sm = reinterpret_cast<float*>(lds4);

    const int lane = lane_id(), h = lane >> 5, col = lane & 31;
    const int nw = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int act = __builtin_amdgcn_readfirstlane(A.act);
    const int inverse = __builtin_amdgcn_readfirstlane(A.inverse);
    const int nterms = __builtin_amdgcn_readfirstlane(A.nterms);
    float* tb = sm + L.total + wave * W.total;  // transposition tile
    float* zs = tb + W.zs;
    float* vs = tb + W.vs;
    float* gs = tb + W.gs;
    float* ms = tb + W.ms;
    float* g1s = tb + W.g1 + lane;  // this lane's dW1 sums, [d][HT] at stride 64

    // Gradient accumulators, carried across every tile of the wave.
    f32x16 aW2[HT * HT];
    float aW3[D][HT], ab1[HT], ab2[HT], ab3[D];
#pragma unroll
    for (int i = 0; i < HT * HT; ++i) aW2[i] = f32x16{};
#pragma unroll
    for (int i = 0; i < HT; ++i) ab1[i] = ab2[i] = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        ab3[j] = 0.f;
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) {
            aW3[j][ht] = 0.f;
            g1s[(j * HT + ht) * 64] = 0.f;
        }
    }

    // One accumulator tile X (32 hidden rows in registers, sample = lane & 31) -> X^T (hidden unit =
    // lane & 31, register r = sample crow(r, h)): the operand form of a product that contracts over
    // the samples.
    float* const tw = tb + 4 * h * PITCH + col;
    const float* const tr_ = tb + col * PITCH + 4 * h;
    auto transpose = [&](const f32x16& X) -> f32x16 {
        f32x16 XT;
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < 16; ++r) tw[crow(r, 0) * PITCH] = X[r];
        wave_lds_sync();
#pragma unroll
        for (int r = 0; r < 16; ++r) XT[r] = tr_[crow(r, 0)];
        return XT;
    };
    // sum over this lane half's 16 samples of X^T times a per-sample table row [32]
    auto dot_samples = [&](const f32x16& xT, const float* row) -> float {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * h + 8 * q);
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) s = fmaf(xT[4 * q + rr], v[rr], s);
        }
        return s;
    };
    auto sum16 = [](const f32x16& x) -> float {
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) s += x[r];
        return s;
    };

    for (int64_t tile = (int64_t)blockIdx.x * nw + wave; tile < A.ntiles; tile += (int64_t)gridDim.x * nw) {
        const int64_t srow = tile * 32 + col;
        const bool live = srow < A.B;
        // A row that is past the batch, or dead (a non-finite z, cotangent, entry of J, or solve),
        // carries zeros: it adds exact zeros to every sum and gets gx = 0.
        bool dead = !live;
        float z[D], gy[D];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            z[j] = live ? A.z[srow * D + j] : 0.f;
            gy[j] = live ? A.gy[srow * D + j] : 0.f;
            dead = dead || nonfinite(z[j]) || nonfinite(gy[j]);
        }
        float lb = live ? A.gld[srow] : 0.f;
        dead = dead || nonfinite(lb);
        if (inverse) lb = -lb;  // ld = -N(z)
#pragma unroll
        for (int j = 0; j < D; ++j) z[j] = dead ? 0.f : z[j];

        // ---- phase 1: J, then G = dL/dJ = lb (sum_k (-1)^(k+1) J^(k-1))^T, and in the inverse
        // direction the LU factors of (I + J)^T (a failed pivot kills the row before any sum).
        int piv[D] = {};
        {
            float o[D], J[D][D];
            res_jacobian<HT, D, TG, 0>(sm, act, lane, z, o, J);
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b < D; ++b) dead = dead || nonfinite(J[a][b]);
            if (inverse) {
                float M[D][D];
#pragma unroll
                for (int a = 0; a < D; ++a)
#pragma unroll
                    for (int b = 0; b < D; ++b) M[a][b] = (a == b ? 1.f : 0.f) + (dead ? 0.f : J[b][a]);
                dead = !res_lu<D>(M, piv) || dead;
                wave_lds_sync();
                if (h == 0) {
#pragma unroll
                    for (int a = 0; a < D; ++a)
#pragma unroll
                        for (int b = 0; b < D; ++b) ms[(a * D + b) * 32 + col] = M[a][b];
                }
            }
#pragma unroll
            for (int j = 0; j < D; ++j) {
                z[j] = dead ? 0.f : z[j];
                gy[j] = dead ? 0.f : gy[j];
#pragma unroll
                for (int b = 0; b < D; ++b) J[j][b] = dead ? 0.f : J[j][b];
            }
            lb = dead ? 0.f : lb;
            float S[D][D], Pw[D][D];
#pragma unroll
            for (int a = 0; a < D; ++a)
#pragma unroll
                for (int b = 0; b < D; ++b) {
                    S[a][b] = 0.f;
                    Pw[a][b] = a == b ? 1.f : 0.f;
                }
#pragma unroll 1
            for (int k = 1; k <= nterms; ++k) {
                const float sg = (k & 1) ? 1.f : -1.f;
#pragma unroll
                for (int a = 0; a < D; ++a)
#pragma unroll
                    for (int b = 0; b < D; ++b) S[a][b] = fmaf(sg, Pw[a][b], S[a][b]);
                if (k < nterms) {
#pragma unroll
                    for (int a = 0; a < D; ++a) {
                        float q[D];
#pragma unroll
                        for (int b = 0; b < D; ++b) {
                            q[b] = Pw[a][0] * J[0][b];
#pragma unroll
                            for (int c = 1; c < D; ++c) q[b] = fmaf(Pw[a][c], J[c][b], q[b]);
                        }
#pragma unroll
                        for (int b = 0; b < D; ++b) Pw[a][b] = q[b];
                    }
                }
            }
            wave_lds_sync();
            if (h == 0) {
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    zs[j * 32 + col] = z[j];
#pragma unroll
                    for (int i = 0; i < D; ++i) gs[(j * D + i) * 32 + col] = lb * S[i][j];
                }
            }
            wave_lds_sync();
        }

        // ---- phase 2: the value chain again (h1, h2 are kept), then one tangent at a time
        // (a fresh opaque zero per section: the LDS operands are neither hoisted out of the loops
        // nor kept in registers from one section to the next)
        f32x16 h1[HT], h2[HT];
        {
            const float* s = sm + opaque_zero();
            float xb[KS1];
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) {
                const int k0 = 2 * ks, k1 = 2 * ks + 1;
                const float a = z[k0 < D ? k0 : 0];
                const float b = k1 < D ? z[k1 < D ? k1 : 0] : 0.f;
                xb[ks] = h ? b : a;
            }
#pragma unroll
            for (int ht = 0; ht < HT; ++ht) {
                f32x16 a = load_bias16(s + F.b1 + ht * 32, h);
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) a = mfma32(s[F.w1 + (ht * KS1 + ks) * 64 + lane], xb[ks], a);
                res_act16(act, a);
                h1[ht] = a;
            }
        }
        // acc = (image at w) x, an H x H product on A fragments read from LDS
        auto hxh = [&](const float* w_, int ot, const f32x16 (&x)[HT], f32x16 acc) -> f32x16 {
            const f32x4* wl = reinterpret_cast<const f32x4*>(w_) + lane;
#pragma unroll
            for (int kt = 0; kt < HT; ++kt)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const f32x4 w = wl[a_quad(a_tile(ot, kt, HT), rq) * 64];
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) acc = mfma32(w[rr], x[kt][4 * rq + rr], acc);
                    __builtin_amdgcn_sched_barrier(0);  // (no A fragment is read far ahead of its use)
                }
            return acc;
        };
        {
            const float* s = sm + opaque_zero();
#pragma unroll
            for (int hto = 0; hto < HT; ++hto) {
                f32x16 a = hxh(s + F.w2, hto, h1, load_bias16(s + F.b2 + hto * 32, h));
                res_act16(act, a);
                h2[hto] = a;
            }
        }
        __builtin_amdgcn_sched_barrier(0);

        f32x16 dg1[HT], dg2[HT];
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) dg1[ht] = dg2[ht] = f32x16{};
        if (nterms > 0) {
#pragma unroll 1
            for (int i = 0; i < D; ++i) {
                const float* s = sm + opaque_zero();
                float Gi[D];
#pragma unroll
                for (int j = 0; j < D; ++j) Gi[j] = gs[(j * D + i) * 32 + col];
                // T1_i = g1 * W1[:, i]
                auto tangent1 = [&](int kt) -> f32x16 {
                    const f32x16 g = res_dact16(act, opaque_tile(h1[kt]));
                    const f32x16 w = load_bias16(s + F.w1c + (i * HT + kt) * 32, h);
                    f32x16 t;
#pragma unroll
                    for (int r = 0; r < 16; ++r) t[r] = g[r] * w[r];
                    return t;
                };
                f32x16 dU[HT];
                {
                    f32x16 T1[HT];
#pragma unroll
                    for (int kt = 0; kt < HT; ++kt) T1[kt] = tangent1(kt);
                    // U_i = W2 T1_i; dT2_i = W3^T G[:, i]; dg2 += dT2_i * U_i; dW3 += G[:, i] T2_i^T;
                    // dU_i = g2 * dT2_i
#pragma unroll
                    for (int hto = 0; hto < HT; ++hto) {
                        const f32x16 u = hxh(s + F.w2, hto, T1, f32x16{});
                        const f32x16 g = res_dact16(act, opaque_tile(h2[hto]));
                        f32x16 dT2 = {};
#pragma unroll
                        for (int j = 0; j < D; ++j) {
                            const f32x16 w3 = load_bias16(s + F.w3 + (j * HT + hto) * 32, h);
#pragma unroll
                            for (int r = 0; r < 16; ++r) dT2[r] = fmaf(w3[r], Gi[j], dT2[r]);
                        }
                        f32x16 T2;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            dg2[hto][r] = fmaf(dT2[r], u[r], dg2[hto][r]);
                            T2[r] = g[r] * u[r];
                            dU[hto][r] = g[r] * dT2[r];
                        }
                        const f32x16 T2T = transpose(T2);
#pragma unroll
                        for (int j = 0; j < D; ++j) aW3[j][hto] += dot_samples(T2T, gs + (j * D + i) * 32);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                // dT1_i = W2^T dU_i; dg1 += dT1_i * W1[:, i]; dW1[:, i] += g1 * dT1_i
#pragma unroll
                for (int jo = 0; jo < HT; ++jo) {
                    const f32x16 m = hxh(s + L.w2t, jo, dU, f32x16{});
                    const f32x16 g = res_dact16(act, opaque_tile(h1[jo]));
                    const f32x16 w = load_bias16(s + F.w1c + (i * HT + jo) * 32, h);
                    f32x16 a;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        dg1[jo][r] = fmaf(m[r], w[r], dg1[jo][r]);
                        a[r] = g[r] * m[r];
                    }
                    const f32x16 aT = transpose(a);
                    g1s[(i * HT + jo) * 64] += sum16(aT);
                    __builtin_amdgcn_sched_barrier(0);
                }
                // dW2 += dU_i T1_i^T (T1_i worked out again: it is not kept over the two products above)
                f32x16 T1T[HT];
#pragma unroll
                for (int jt = 0; jt < HT; ++jt) T1T[jt] = transpose(tangent1(jt));
#pragma unroll
                for (int kt = 0; kt < HT; ++kt) {
                    const f32x16 xT = transpose(dU[kt]);
#pragma unroll
                    for (int jt = 0; jt < HT; ++jt)
#pragma unroll
                        for (int r = 0; r < 16; ++r) aW2[kt * HT + jt] = mfma32(xT[r], T1T[jt][r], aW2[kt * HT + jt]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }

        // ---- the value-chain adjoint. forward: one pass with vb = gy and the folded dg1, dg2.
        // inverse: a pass with vb = 0 gives z_bar; (I + J)^T w = gy + z_bar; a second, value-only
        // pass with vb = -w.
        float vb[D], gx[D];
#pragma unroll
        for (int j = 0; j < D; ++j) {
            vb[j] = inverse ? 0.f : gy[j];
            gx[j] = 0.f;
        }
        const int npass = inverse ? 2 : 1;
#pragma unroll 1
        for (int pass = 0; pass < npass; ++pass) {
            const float* s = sm + opaque_zero();
            wave_lds_sync();
            if (h == 0) {
#pragma unroll
                for (int j = 0; j < D; ++j) vs[j * 32 + col] = vb[j];
            }
            wave_lds_sync();
            // dW3 += vb h2^T
#pragma unroll
            for (int kt = 0; kt < HT; ++kt) {
                const f32x16 xT = transpose(h2[kt]);
#pragma unroll
                for (int j = 0; j < D; ++j) aW3[j][kt] += dot_samples(xT, vs + j * 32);
            }
            // ab2 = g2 * (W3^T vb) + c2 * dg2
            f32x16 a2[HT];
#pragma unroll
            for (int ht = 0; ht < HT; ++ht) {
                f32x16 wv = {};
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const f32x16 w3 = load_bias16(s + F.w3 + (j * HT + ht) * 32, h);
#pragma unroll
                    for (int r = 0; r < 16; ++r) wv[r] = fmaf(w3[r], vb[j], wv[r]);
                }
                const f32x16 g = res_dact16(act, opaque_tile(h2[ht])), c = res_ddact16(act, opaque_tile(h2[ht]));
#pragma unroll
                for (int r = 0; r < 16; ++r) a2[ht][r] = fmaf(g[r], wv[r], c[r] * dg2[ht][r]);
            }
            // dW2 += ab2 h1^T, db2 += ab2
            f32x16 h1T[HT];
#pragma unroll
            for (int ht = 0; ht < HT; ++ht) h1T[ht] = transpose(h1[ht]);
#pragma unroll
            for (int kt = 0; kt < HT; ++kt) {
                const f32x16 xT = transpose(a2[kt]);
#pragma unroll
                for (int jt = 0; jt < HT; ++jt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) aW2[kt * HT + jt] = mfma32(xT[r], h1T[jt][r], aW2[kt * HT + jt]);
                ab2[kt] += sum16(xT);
            }
            __builtin_amdgcn_sched_barrier(0);
            // ab1 = g1 * (W2^T ab2) + c1 * dg1; z_bar = W1^T ab1; dW1 += ab1 z^T, db1 += ab1
            float pz[D];
#pragma unroll
            for (int j = 0; j < D; ++j) pz[j] = 0.f;
#pragma unroll
            for (int jo = 0; jo < HT; ++jo) {
                const f32x16 m = hxh(s + L.w2t, jo, a2, f32x16{});
                const f32x16 g = res_dact16(act, opaque_tile(h1[jo])), c = res_ddact16(act, opaque_tile(h1[jo]));
                f32x16 a1;
#pragma unroll
                for (int r = 0; r < 16; ++r) a1[r] = fmaf(g[r], m[r], c[r] * dg1[jo][r]);
#pragma unroll
                for (int j = 0; j < D; ++j) pz[j] = acc_dot16(s + F.w1c + (j * HT + jo) * 32, h, a1, pz[j]);
                const f32x16 xT = transpose(a1);
                ab1[jo] += sum16(xT);
#pragma unroll
                for (int i = 0; i < D; ++i) g1s[(i * HT + jo) * 64] += dot_samples(xT, zs + i * 32);
                __builtin_amdgcn_sched_barrier(0);
            }
            float zb[D];
#pragma unroll
            for (int j = 0; j < D; ++j) {
                zb[j] = halves_sum(pz[j], pz[j]);
                ab3[j] += vb[j];
            }
            if (!inverse) {
#pragma unroll
                for (int j = 0; j < D; ++j) gx[j] = gy[j] + zb[j];
            } else if (pass == 0) {
                float M[D][D], w[D];
#pragma unroll
                for (int a = 0; a < D; ++a) {
                    w[a] = gy[a] + zb[a];
#pragma unroll
                    for (int b = 0; b < D; ++b) M[a][b] = dead ? (a == b ? 1.f : 0.f) : ms[(a * D + b) * 32 + col];
                }
                res_lu_solve<D>(M, piv, w);
                bool bad = dead;
#pragma unroll
                for (int a = 0; a < D; ++a) bad = bad || nonfinite(w[a]);
#pragma unroll
                for (int a = 0; a < D; ++a) {
                    gx[a] = bad ? 0.f : w[a];
                    vb[a] = -gx[a];
                }
#pragma unroll
                for (int ht = 0; ht < HT; ++ht) dg1[ht] = dg2[ht] = f32x16{};
            }
        }

        if (live && h == 0) {
#pragma unroll
            for (int j = 0; j < D; ++j) A.gx[srow * D + j] = gx[j];
        }
    }

    // The wave's partial sums (every launched wave writes its slot, a wave that had no tile writes
    // zeros).
    float* slot = A.ws + ((int64_t)blockIdx.x * nw + wave) * P.total;
#pragma unroll
    for (int i = 0; i < HT * HT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) slot[P.w2 + (i * 16 + r) * 64 + lane] = aW2[i][r];
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            slot[P.g1 + (j * HT + ht) * 64 + lane] = g1s[(j * HT + ht) * 64];
            slot[P.g3 + (j * HT + ht) * 64 + lane] = aW3[j][ht];
        }
        slot[P.b1 + ht * 64 + lane] = ab1[ht];
        slot[P.b2 + ht * 64 + lane] = ab2[ht];
    }
#pragma unroll
    for (int j = 0; j < D; ++j) slot[P.b3 + j * 64 + lane] = ab3[j];
}

typedef void (*residual_bwd_kernel_t)(ResBwdArgs);

// Defined once per padded width, in nfx_residual_bwd_h{1,2}.hip.
template <int HT>
residual_bwd_kernel_t res_bwd_pick_ht(int d);
template <>
residual_bwd_kernel_t res_bwd_pick_ht<1>(int d);
template <>
residual_bwd_kernel_t res_bwd_pick_ht<2>(int d);

template <int HT>
residual_bwd_kernel_t res_bwd_pick(int d) {
    return pick_range<1, kResMaxD>(d, [](auto D) -> residual_bwd_kernel_t { return residual_bwd_kernel<HT, D()>; });
}

// The pack of nfx_residual.hip: the forward image and, with `backward`, the operands behind it.
int residual_pack_launch(const float* const (&w)[3], const float* const (&b)[3], const float* const (&u)[3],
                         const float* const (&v)[3], const float (&c)[3], int d, int H, float* packed, bool backward,
                         hipStream_t stream);

}  // namespace nfx

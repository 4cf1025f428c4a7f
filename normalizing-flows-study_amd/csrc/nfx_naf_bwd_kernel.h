// Backward of NeuralAutoregressiveFlow's density direction: the gradients of one DeepMADE pass and
// the affine transform with respect to the input and every parameter, one launch (see
// nfx_naf_bwd.hip for the recurrences and the layout).
#pragma once
#include "nfx_naf_kernel.h"

namespace nfx {

constexpr int kNafBwdMaxH = 64;  // widest hidden layer of the backward family (two 32-row tiles)

// Packed image of the backward (floats): the forward image (naf_layout, written by nfx_naf_pack),
// then per layer l = 0 .. nh (nh = the output layer) the A operand of (W o M)^T x,
//   wt  [NTin_l][NT_l][4][64][4]   out tile = a tile of the layer's INPUT rows, k tile = a tile of its
//                                  output rows; NTin_0 = 1 (the 16 input slots), NT_nh = 1 (row j =
//                                  mu_j, row 16 + j = alpha_j, as in the forward image).
// One wave's partial sums (floats), per layer, in the order the finish kernel decodes:
//   gw  [NT_l][NTin_l][16][64]     dW tile (ot, kt): register r of lane l is element
//                                  (32 ot + crow(r, l >> 5), 32 kt + (l & 31))
//   gb, gg, ge [NT_l][64]          db, dgamma, dbeta: lane l holds half (l >> 5) of the sum for row
//                                  32 ot + (l & 31) (gg, ge are written with LayerNorm only)
struct NafBwdLayerDesc {
    int wt;    // float offset of the transposed A operand in the image
    int ntin;  // tiles of the layer's input
    int gw, gb, gg, ge;  // float offsets in a wave's partial sums
};

struct NafBwdLayout {
    NafLayout F;
    NafBwdLayerDesc layer[kNafLayers];
    int total;    // floats of the image
    int partial;  // floats of one wave's partial sums
};

__host__ __device__ inline NafBwdLayout naf_bwd_layout(int d, int nh, const int* widths) {
    NafBwdLayout L{};
    L.F = naf_layout(d, nh, widths);
    int o = L.F.total, p = 0;
    for (int l = 0; l <= nh; ++l) {
        const int nt = L.F.layer[l].nt, ntin = l == 0 ? 1 : L.F.layer[l - 1].nt;
        L.layer[l].wt = o;
        o += ntin * nt * 1024;
        L.layer[l].ntin = ntin;
        L.layer[l].gw = p;
        p += nt * ntin * 1024;
        L.layer[l].gb = p;
        p += nt * 64;
        L.layer[l].gg = p;
        p += nt * 64;
        L.layer[l].ge = p;
        p += nt * 64;
    }
    L.total = o;
    L.partial = p;
    return L;
}

// Wave-private LDS behind the image: one 32 x 32 tile with pitch 33, the transposition between
// "hidden rows x sample lanes" and "sample rows x hidden lanes".
constexpr int kNafBwdPitch = 33;
constexpr int kNafBwdWaveFloats = 32 * kNafBwdPitch;

// What the reverse sweep needs of the recomputed conditioner, kept per wave in a stretch of the
// workspace (written and read back by the same lane, register r of tile t at (16 t + r) 64 + lane):
// per hidden layer the normalised value x^ (without LayerNorm: the pre-activation) [HTM tiles], the
// layer's output [HTM tiles], and rstd [64].
__host__ __device__ constexpr int naf_bwd_keep_layer_floats(int HTM) { return 2 * HTM * 1024 + 64; }

// Launch shape, fixed on the host and independent of the device so that the workspace size is: a
// wave per 32-row tile up to kNafBwdMaxWaves (one wave per SIMD of 256 CUs); one-wave workgroups
// while every tile can have a CU of its own, four waves sharing one staged image beyond.
constexpr int kNafBwdMaxWaves = 1024;
constexpr int kNafBwdWideTiles = 256;
inline int naf_bwd_threads(int64_t ntiles) { return ntiles > kNafBwdWideTiles ? 256 : 64; }
inline int naf_bwd_grid(int64_t ntiles) {
    const int nw = naf_bwd_threads(ntiles) / 64;
    const int64_t g = (ntiles + nw - 1) / nw;
    return (int)(g < kNafBwdMaxWaves / nw ? g : kNafBwdMaxWaves / nw);
}

struct NafBwdArgs {
    NafArgs F;         // packed = the backward image, total4 = all of it; in = x; out, logdet unused
    const float* gz;   // [B][d]
    const float* gld;  // [B]
    float* gx;         // [B][d]
    float* ws;         // [grid * waves][partial]
    float* keep;       // [grid * waves][nh][naf_bwd_keep_layer_floats]
    int partial;
    NafBwdLayerDesc bl[kNafLayers];
};

// d act / d p at the pre-activation p, a tile at a time: g <- g * act'(p).
__device__ __forceinline__ void naf_act_bwd16(int act, const f32x16& p, f32x16& g) {
    switch (act) {
        case NFX_NAF_RELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = p[r] > 0.f ? g[r] : 0.f;
            break;
        case NFX_NAF_ELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = p[r] > 0.f ? g[r] : g[r] * expf(p[r]);
            break;
        case NFX_NAF_LEAKY_RELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = p[r] > 0.f ? g[r] : g[r] * 0.1f;
            break;
        default:  // exact GELU: Phi(p) + p phi(p)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float cdf = 0.5f * (1.f + erff(p[r] * 0.70710678118654752440f));
                const float pdf = expf(-0.5f * p[r] * p[r]) * 0.39894228040143267794f;
                g[r] = g[r] * fmaf(p[r], pdf, cdf);
            }
            break;
    }
}

// naf_norm_act with the values the reverse sweep needs stored on the way: the same operations in
// the same order (the clamp and guard masks of the backward must be those of the forward), x^ =
// dev * rstd rounded once and used for the affine step as there.
template <int HTM>
__device__ __forceinline__ void naf_norm_act_keep(const float* s, const NafArgs& A, const NafLayerDesc& L, float eps,
                                                  int lane, f32x16 (&t)[HTM], float* keep) {
    const int h = lane >> 5;
    if (A.ln) {
        float ts[HTM];
#pragma unroll
        for (int ot = 0; ot < HTM; ++ot) ts[ot] = ot < L.nt ? naf_sum16(t[ot]) : 0.f;
        const float sum = naf_sum_tiles<HTM>(ts);
        const float n = (float)L.width;
        const float mean = halves_sum(sum, sum) / n;
        const int rows_left = L.width - 4 * h;
#pragma unroll
        for (int ot = 0; ot < HTM; ++ot) {
            ts[ot] = 0.f;
            if (ot < L.nt) {
                f32x16 sq;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float dev = 32 * ot + crow(r, 0) < rows_left ? t[ot][r] - mean : 0.f;
                    sq[r] = dev * dev;
                    t[ot][r] = dev;
                }
                ts[ot] = naf_sum16(sq);
            }
        }
        const float ss = naf_sum_tiles<HTM>(ts);
        const float var = halves_sum(ss, ss) / n;
        const float rstd = 1.f / sqrtf(var + eps);
        keep[2 * HTM * 1024 + lane] = rstd;
#pragma unroll
        for (int ot = 0; ot < HTM; ++ot)
            if (ot < L.nt) {
                const f32x16 g = load_bias16(s + L.v + 32 * (L.nt + ot), h);
                const f32x16 b = load_bias16(s + L.v + 32 * (2 * L.nt + ot), h);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float xh = t[ot][r] * rstd;
                    keep[(16 * ot + r) * 64 + lane] = xh;
                    t[ot][r] = fmaf(xh, g[r], b[r]);
                }
            }
    } else {
#pragma unroll
        for (int ot = 0; ot < HTM; ++ot)
            if (ot < L.nt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) keep[(16 * ot + r) * 64 + lane] = t[ot][r];
            }
    }
#pragma unroll
    for (int ot = 0; ot < HTM; ++ot)
        if (ot < L.nt) naf_act16(A.act, t[ot]);
}

// naf_eval for the wave's 32 samples with every layer's values kept: the output tile BEFORE its
// [-2, 2] clamp (the caller needs both sides of it).
template <int HTM>
__device__ __forceinline__ f32x16 naf_eval_keep(const float* sm, const NafArgs& A, int lane, const float (&x)[8],
                                                float* keep) {
    constexpr int KL = naf_bwd_keep_layer_floats(HTM);
    const int h = lane >> 5;
    const float* s = sm + opaque_zero();
    f32x16 cur[HTM];
    {
        const NafLayerDesc L = A.layer[0];
        const f32x4* wl = reinterpret_cast<const f32x4*>(s + L.w) + lane;
#pragma unroll
        for (int ot = 0; ot < HTM; ++ot) {
            f32x16 a = {};
            if (ot < L.nt) {
                f32x16 acc[2] = {};
#pragma unroll
                for (int rq = 0; rq < 2; ++rq)
                    if (rq == 0 || A.d > 8) {
                        const f32x4 w = wl[(2 * ot + rq) * 64];
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) acc[rq] = mfma32(w[rr], x[4 * rq + rr], acc[rq]);
                    }
                a = (acc[0] + acc[1]) + load_bias16(s + L.v + 32 * ot, h);
            }
            cur[ot] = a;
        }
        naf_norm_act_keep<HTM>(s, A, L, s[0], lane, cur, keep);
#pragma unroll
        for (int ot = 0; ot < HTM; ++ot)
            if (ot < L.nt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) keep[HTM * 1024 + (16 * ot + r) * 64 + lane] = cur[ot][r];
            }
    }
#pragma unroll 1
    for (int l = 1; l < A.nh; ++l) {
        const NafLayerDesc L = A.layer[l];
        const int ntin = A.layer[l - 1].nt;
        float* kl = keep + l * KL;
        f32x16 nxt[HTM];
#pragma unroll
        for (int ot = 0; ot < HTM; ++ot) {
            nxt[ot] = f32x16{};
            if (ot < L.nt) nxt[ot] = naf_tile<HTM>(s, L, ot, ntin, lane, cur);
        }
        naf_norm_act_keep<HTM>(s, A, L, s[l], lane, nxt, kl);
        const bool res = (A.resmask >> l) & 1;
#pragma unroll
        for (int ot = 0; ot < HTM; ++ot) {
            cur[ot] = res ? nxt[ot] + cur[ot] : nxt[ot];
            if (ot < L.nt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) kl[HTM * 1024 + (16 * ot + r) * 64 + lane] = cur[ot][r];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    return naf_tile<HTM>(s, A.layer[A.nh], 0, A.layer[A.nh - 1].nt, lane, cur);
}

template <int HTM>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void naf_bwd_kernel(NafBwdArgs A) {
    constexpr int PITCH = kNafBwdPitch;
    constexpr int KL = naf_bwd_keep_layer_floats(HTM);
    extern __shared__ f32x4 lds4[];
    stage_image(lds4, A.F.packed, A.F.total4);
    float* sm = reinterpret_cast<float*>(lds4);

    const int lane = lane_id(), h = lane >> 5, col = lane & 31;
    const int nw = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* tb = sm + 4 * A.F.total4 + wave * kNafBwdWaveFloats;  // transposition tile
    const int64_t slot_id = (int64_t)blockIdx.x * nw + wave;
    float* slot = A.ws + slot_id * A.partial;
    float* keep = A.keep + slot_id * ((int64_t)A.F.nh * KL);
    const int d = A.F.d, nh = A.F.nh;
    const float ca = A.F.clamp_alpha, cl = A.F.clamp_log_scale;

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

    // The wave's sums live in its workspace slot and are advanced once per tile: the first tile
    // writes, the later ones add (a wave has few tiles: at most ntiles / 1024 rounded up).
    bool first = true;
    // g[lane] += the sum over this lane half's 16 samples of hidden unit lane & 31
    auto add_cols = [&](float* g, const f32x16& XT) {
        float p[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) p[i] = XT[2 * i] + XT[2 * i + 1];
        const float sum = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
        g[lane] = first ? sum : g[lane] + sum;
    };
    // the dW tile at g += a^T-operand tile times in^T-operand tile (the contraction over 32 samples)
    auto add_outer = [&](float* g, const f32x16& aT, const f32x16& inT) {
        f32x16 acc = {};
        if (!first) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = g[r * 64 + lane];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc = mfma32(aT[r], inT[r], acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r * 64 + lane] = acc[r];
    };

    for (int64_t tile = (int64_t)blockIdx.x * nw + wave; tile < A.F.ntiles; tile += (int64_t)gridDim.x * nw) {
        const int64_t srow = tile * 32 + col;
        const bool live = srow < A.F.B;
        const float* s = sm + opaque_zero();
        // A row past the batch, or one with a non-finite input element or conditioner output, is a
        // dead column: zero input and zero cotangents, so it adds exact zeros to every sum.
        float x[8], gz[8];
        bool dead = !live;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int j = naf_dim(r, h);
            const bool in = live && j < d;
            x[r] = in ? A.F.in[srow * d + j] : 0.f;
            gz[r] = in ? A.gz[srow * d + j] : 0.f;
            dead = dead || nonfinite(x[r]);
        }
        {
            const float f = dead ? 1.f : 0.f;
            dead = halves_sum(f, f) > 0.f;  // the sample's other eight elements
        }
        const float gld = live ? A.gld[srow] : 0.f;

        // The conditioner, recomputed as naf_eval computes it. A column whose output is not finite
        // dies here and the pass runs once more with its input zeroed (a wave-uniform decision), so
        // that what the sweep reads of it is finite.
        f32x16 o;
#pragma unroll 1
        for (int pass = 0; pass < 2; ++pass) {
            if (dead) {
#pragma unroll
                for (int r = 0; r < 8; ++r) x[r] = 0.f;
            }
            o = naf_eval_keep<HTM>(sm, A.F, lane, x, keep);
            bool bad = false;
#pragma unroll
            for (int r = 0; r < 16; ++r) bad = bad || nonfinite(o[r]);
            const float f = bad ? 1.f : 0.f;
            bad = halves_sum(f, f) > 0.f;
            const bool again = bad && !dead;
            dead = dead || bad;
            if (__builtin_amdgcn_ballot_w64(again) == 0) break;
        }

        // The transform and its cotangents: a[0] is the cotangent of the output tile before its clamp.
        f32x16 a[HTM], g[HTM];
        float direct[8];
#pragma unroll
        for (int ot = 0; ot < HTM; ++ot) a[ot] = g[ot] = f32x16{};
        {
#pragma clang fp contract(off)  // the transform rounds op by op, as the forward kernel's
            float ls[8], nls[8], al[8], e[8], z[8];
            float ldp = 0.f, ldc = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float mu = tclamp(o[r], -2.f, 2.f);
                al[r] = tclamp(o[8 + r], -2.f, 2.f);
                nls[r] = -tclamp(al[r], -ca, ca);
                ls[r] = tclamp(nls[r], -cl, cl);
                e[r] = expf(ls[r]);
                z[r] = (x[r] - mu) * e[r];
                if (naf_dim(r, h) < d) naf_two_sum(ldp, ldc, ls[r]);
            }
            float ld;
            {
                const float op = halves_other(ldp, ldp), oc = halves_other(ldc, ldc);
                float lo = h ? op : ldp, c = ldc + oc;
                naf_two_sum(lo, c, h ? ldp : op);
                ld = lo + c;
            }
            // torch.clamp passes the gradient on the closed interval; a NaN fails both comparisons
            const float gl = (!dead && ld >= -100.f && ld <= 100.f && !nonfinite(ld)) ? gld : 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const bool on = !dead && naf_dim(r, h) < d;
                const bool zf = on && !nonfinite(z[r]);
                const float gzr = zf ? gz[r] : 0.f;
                const float mu_bar = -(gzr * e[r]);
                const float ls_bar = (zf ? gzr * z[r] : 0.f) + gl;
                const bool both = nls[r] >= -cl && nls[r] <= cl && al[r] >= -ca && al[r] <= ca;
                const float alpha_bar = both ? -ls_bar : 0.f;
                direct[r] = on ? gzr * e[r] : 0.f;
                a[0][r] = on && o[r] >= -2.f && o[r] <= 2.f ? mu_bar : 0.f;
                a[0][8 + r] = on && o[8 + r] >= -2.f && o[8 + r] <= 2.f ? alpha_bar : 0.f;
            }
        }

        // The output layer and the hidden layers, top down. Entering layer l < nh, g is the cotangent
        // of the layer's output; leaving it, of its input.
#pragma unroll 1
        for (int l = nh; l >= 0; --l) {
            const NafLayerDesc L = A.F.layer[l];
            const NafBwdLayerDesc BL = A.bl[l];
            if (l < nh) {
                const float* kl = keep + l * KL;
                f32x16 xh[HTM];
#pragma unroll
                for (int ot = 0; ot < HTM; ++ot) {
                    xh[ot] = a[ot] = f32x16{};
                    if (ot < L.nt) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) xh[ot][r] = kl[(16 * ot + r) * 64 + lane];
                    }
                }
                if (A.F.ln) {
                    const float rstd = kl[2 * HTM * 1024 + lane];
                    const float n = (float)L.width;
                    const int rows_left = L.width - 4 * h;
                    float s1[HTM], s2[HTM];
#pragma unroll
                    for (int ot = 0; ot < HTM; ++ot) {
                        s1[ot] = s2[ot] = 0.f;
                        if (ot < L.nt) {
                            const f32x16 gam = load_bias16(s + L.v + 32 * (L.nt + ot), h);
                            const f32x16 bet = load_bias16(s + L.v + 32 * (2 * L.nt + ot), h);
                            f32x16 p, gh = g[ot];
#pragma unroll
                            for (int r = 0; r < 16; ++r) p[r] = fmaf(xh[ot][r], gam[r], bet[r]);
                            naf_act_bwd16(A.F.act, p, gh);
                            add_cols(slot + BL.ge + 64 * ot, transpose(gh));
                            f32x16 gx_;
#pragma unroll
                            for (int r = 0; r < 16; ++r) gx_[r] = gh[r] * xh[ot][r];
                            add_cols(slot + BL.gg + 64 * ot, transpose(gx_));
                            // gamma g^ and its product with x^ (a pad row has gamma = 0 and x^ = 0)
                            f32x16 q;
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                gh[r] = gh[r] * gam[r];
                                q[r] = gh[r] * xh[ot][r];
                            }
                            s1[ot] = naf_sum16(gh);
                            s2[ot] = naf_sum16(q);
                            a[ot] = gh;
                        }
                    }
                    const float t1 = naf_sum_tiles<HTM>(s1), t2 = naf_sum_tiles<HTM>(s2);
                    const float m1 = halves_sum(t1, t1) / n, m2 = halves_sum(t2, t2) / n;
#pragma unroll
                    for (int ot = 0; ot < HTM; ++ot)
                        if (ot < L.nt) {
#pragma unroll
                            for (int r = 0; r < 16; ++r)
                                a[ot][r] = 32 * ot + crow(r, 0) < rows_left
                                               ? rstd * ((a[ot][r] - m1) - xh[ot][r] * m2)
                                               : 0.f;
                        }
                } else {
#pragma unroll
                    for (int ot = 0; ot < HTM; ++ot)
                        if (ot < L.nt) {
                            a[ot] = g[ot];
                            naf_act_bwd16(A.F.act, xh[ot], a[ot]);
                        }
                }
            }
            // dW += a (x) in, db += a: both operands pass through the transposition tile
            f32x16 inT[HTM];
#pragma unroll
            for (int kt = 0; kt < HTM; ++kt) {
                inT[kt] = f32x16{};
                if (kt < BL.ntin) {
                    f32x16 in = {};
                    if (l == 0) {
#pragma unroll
                        for (int r = 0; r < 8; ++r) in[r] = x[r];
                    } else {
                        const float* kc = keep + (l - 1) * KL + HTM * 1024;
#pragma unroll
                        for (int r = 0; r < 16; ++r) in[r] = kc[(16 * kt + r) * 64 + lane];
                    }
                    inT[kt] = transpose(in);
                }
            }
#pragma unroll
            for (int ot = 0; ot < HTM; ++ot)
                if (ot < L.nt) {
                    const f32x16 aT = transpose(a[ot]);
                    add_cols(slot + BL.gb + 64 * ot, aT);
#pragma unroll
                    for (int kt = 0; kt < HTM; ++kt)
                        if (kt < BL.ntin) add_outer(slot + BL.gw + (ot * BL.ntin + kt) * 1024, aT, inT[kt]);
                }
            // in_bar = (W o M)^T a, plus the skip of a residual block
            const f32x4* wl = reinterpret_cast<const f32x4*>(s + BL.wt) + lane;
            const bool res = l < nh && ((A.F.resmask >> l) & 1);
            f32x16 nb[HTM];
#pragma unroll
            for (int jt = 0; jt < HTM; ++jt) {
                nb[jt] = f32x16{};
                if (jt < BL.ntin) {
                    f32x16 acc[2] = {};
#pragma unroll
                    for (int ot = 0; ot < HTM; ++ot)
                        if (ot < L.nt) {
#pragma unroll
                            for (int rq = 0; rq < 4; ++rq) {
                                const f32x4 w = wl[a_quad(a_tile(jt, ot, L.nt), rq) * 64];
#pragma unroll
                                for (int rr = 0; rr < 4; ++rr)
                                    acc[rq & 1] = mfma32(w[rr], a[ot][4 * rq + rr], acc[rq & 1]);
                            }
                        }
                    nb[jt] = acc[0] + acc[1];
                    if (res) nb[jt] = nb[jt] + g[jt];
                }
            }
#pragma unroll
            for (int jt = 0; jt < HTM; ++jt) g[jt] = nb[jt];
            __builtin_amdgcn_sched_barrier(0);
        }

        if (live) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int j = naf_dim(r, h);
                if (j < d) A.gx[srow * d + j] = dead ? 0.f : direct[r] + g[0][r];
            }
        }
        first = false;
    }

    // a launched wave that had no tile still owns a slot: zeros
    if (first)
        for (int i = lane; i < A.partial; i += 64) slot[i] = 0.f;
}

typedef void (*naf_bwd_kernel_t)(NafBwdArgs);

// Defined once per padded width, in nfx_naf_bwd_h{1,2}.hip.
template <int HTM>
naf_bwd_kernel_t naf_bwd_pick_ht();
template <>
naf_bwd_kernel_t naf_bwd_pick_ht<1>();
template <>
naf_bwd_kernel_t naf_bwd_pick_ht<2>();

}  // namespace nfx

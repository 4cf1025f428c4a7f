// Backward of the continuous-flow solve: the reverse sweep of the DISCRETE 3/8-rule steps (the
// gradients of the scheme cnf_kernel runs, not of the ODE), one launch (see nfx_cnf_bwd.hip for
// the recurrences and the cost model).
#pragma once
#include "nfx_cnf_kernel.h"

namespace nfx {

// Packed image of the backward (floats): the forward image (cnf_layout, w2 included: here every
// H x H operand is staged in LDS, the registers hold gradient accumulators), then
//   c2t [HT][HT][4][64][4]  A operand of C^T x: the c2 order with (C^T)[j, k] = C[k, j]
//   w2t [HT][HT][4][64][4]  A operand of W2^T x
//   w1c [d][HT][2][16]      column i of W1 in accumulator order (VALU dots of z_bar = W1[:, :d]^T a1)
struct CnfBwdLayout {
    CnfLayout F;
    int c2t, w2t, w1c, total;
};

__host__ __device__ constexpr CnfBwdLayout cnf_bwd_layout(int d, int HT) {
    CnfBwdLayout L{};
    L.F = cnf_layout(d, HT);
    int o = L.F.total;
    L.c2t = o; o += HT * HT * 1024;
    L.w2t = o; o += HT * HT * 1024;
    L.w1c = o; o += d * HT * 32;
    L.total = (o + 3) & ~3;
    return L;
}

// Wave-private LDS behind the image: one 32 x 32 tile with pitch 33 (the transposition between
// "hidden rows x sample lanes" and "sample rows x hidden lanes"), then three small tables by
// sample: the stage input z [8][33], the cotangent v_bar [8][33], and l_bar [32]; then the wave's
// dW1 and dW3 sums, [2][HT][16][2][16]: accumulator tiles of which only columns 0..15 are kept
// (d + 1 <= 9 are in use). They are read, advanced by 16 MFMAs and written back per evaluation:
// the register file is full with the dW2 and dC sums.
constexpr int kCnfBwdPitch = 33;
constexpr int kCnfBwdSmall = 2 * 8 * kCnfBwdPitch + 32;
__host__ __device__ constexpr int cnf_bwd_wave_floats(int HT) {
    return 32 * kCnfBwdPitch + kCnfBwdSmall + 2 * HT * 512;
}

// One wave's partial sums (floats), dumped in register order and decoded by the finish kernel:
//   w2, c  [HT][HT][16][64]  dW2 / dC tile (kt, jt): register r of lane l is element
//                            (32 kt + crow(r, l >> 5), 32 jt + (l & 31))
//   g1     [HT][16][64]      dW1[32 ht + crow(r, l >> 5)][c = l & 31], c <= d
//   g3     [HT][16][64]      dW3[c = l & 31][32 ht + crow(r, l >> 5)], c < d
//   b1, b2 [HT][64]          lane l: half (l >> 5) of the sum for hidden unit 32 ht + (l & 31)
//   b3     [d][64]           per-lane sums over the lane's samples (lanes 0..31 count)
struct CnfBwdPartial {
    int w2, c, g1, g3, b1, b2, b3, total;
};

__host__ __device__ constexpr CnfBwdPartial cnf_bwd_partial(int d, int HT) {
    CnfBwdPartial P{};
    int o = 0;
    P.w2 = o; o += HT * HT * 1024;
    P.c = o; o += HT * HT * 1024;
    P.g1 = o; o += HT * 1024;
    P.g3 = o; o += HT * 1024;
    P.b1 = o; o += HT * 64;
    P.b2 = o; o += HT * 64;
    P.b3 = o; o += d * 64;
    P.total = o;
    return P;
}

// Launch shape, fixed on the host and independent of the device so that the workspace size is:
// a wave per 32-row tile up to kCnfBwdMaxWaves (one wave per SIMD of 256 CUs); one-wave
// workgroups while every tile can have a CU of its own, four waves sharing one staged image beyond.
constexpr int kCnfBwdMaxWaves = 1024;
constexpr int kCnfBwdWideTiles = 256;
inline int cnf_bwd_threads(int64_t ntiles) { return ntiles > kCnfBwdWideTiles ? 256 : 64; }
inline int cnf_bwd_grid(int64_t ntiles) {
    const int nw = cnf_bwd_threads(ntiles) / 64;
    const int64_t g = (ntiles + nw - 1) / nw;
    return (int)(g < kCnfBwdMaxWaves / nw ? g : kCnfBwdMaxWaves / nw);
}

struct CnfBwdArgs {
    const float* packed;
    const float* x;      // the forward's input [B][d]
    const float* traj;   // cnf_traj_floats of the saving forward
    const float* gy;     // [B][d]
    const float* gld;    // [B]
    float* gx;           // [B][d]
    float* ws;           // [grid * waves][CnfBwdPartial::total]
    int64_t B, ntiles;
    CnfGrid g;           // nsteps >= 1 (equal times never launch)
};

template <int HT, int D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void cnf_bwd_kernel(CnfBwdArgs A) {
    constexpr CnfBwdLayout L = cnf_bwd_layout(D, HT);
    constexpr CnfLayout F = L.F;
    constexpr CnfBwdPartial P = cnf_bwd_partial(D, HT);
    constexpr int PITCH = kCnfBwdPitch;
    extern __shared__ f32x4 lds4[];
    stage_image(lds4, A.packed, L.total / 4);
    float* sm = reinterpret_cast<float*>(lds4);

    const int lane = lane_id(), h = lane >> 5, col = lane & 31;
    const int nw = blockDim.x >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* tb = sm + L.total + wave * cnf_bwd_wave_floats(HT);  // transposition tile
    float* zs = tb + 32 * PITCH;                                // stage input by sample
    float* vs = zs + 8 * PITCH;                                 // v_bar by sample
    float* ls = vs + 8 * PITCH;                                 // l_bar by sample
    float* ga1 = ls + 32 + 16 * h + (col & 15);                 // dW1 sums: [HT][16][32], this lane's column
    float* ga3 = ga1 + HT * 512;                                // dW3 sums
    const bool gcol = col < 16;

    // Gradient accumulators, carried across every step of every tile of the wave.
    f32x16 aW2[HT * HT], aC[HT * HT];
    float ab1[HT], ab2[HT], ab3[D];
#pragma unroll
    for (int i = 0; i < HT * HT; ++i) aW2[i] = aC[i] = f32x16{};
#pragma unroll
    for (int i = 0; i < HT; ++i) ab1[i] = ab2[i] = 0.f;
    if (gcol) {
#pragma unroll
        for (int i = 0; i < HT * 16; ++i) ga1[i * 32] = ga3[i * 32] = 0.f;
    }
    // acc += X^T-operand tile times a 32-column B operand, for an accumulator tile kept in LDS
    auto lds_tile_mfma = [&](float* g, const f32x16& xT, const float (&b)[16]) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = gcol ? g[r * 32] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc = mfma32(xT[r], b[r], acc);
        if (gcol) {
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r * 32] = acc[r];
        }
    };
#pragma unroll
    for (int j = 0; j < D; ++j) ab3[j] = 0.f;

    // One accumulator tile X (32 hidden rows in registers, sample = lane & 31) -> X^T (hidden unit =
    // lane & 31, register r = sample crow(r, h)): the operand form of a product that contracts over
    // the samples. Register r of half h is row crow(r, 0) + 4 h.
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

    // One evaluation of the field at (t, z), the arithmetic of cnf_kernel's field with every h2 tile
    // and its trace companion q = C g1 kept. vjp == false: out = v, tr = the divergence. vjp == true:
    // the cotangents (vb, cl * l_bar) of (v, tr) are pulled back: out = z_bar, and the evaluation's
    // share of every parameter gradient joins the accumulators.
    float lbar = 0.f;  // l_bar of sample col (ls holds it by sample for the transposed layout)
    auto stage = [&](float t, const float (&z)[D], bool vjp, const float (&vb)[D], float cl, float (&out)[D],
                     float& tr) {
        const int oz = opaque_zero();  // no hoisting of the LDS operands out of the step loop
        const float* s = sm + oz;
        constexpr int KS1 = F.KS1;
        float xb[KS1];
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            const int k0 = 2 * ks, k1 = 2 * ks + 1;
            const float a = k0 < D ? z[k0 < D ? k0 : 0] : (k0 == D ? t : 0.f);
            const float b = k1 < D ? z[k1 < D ? k1 : 0] : (k1 == D ? t : 0.f);
            xb[ks] = h ? b : a;
        }
        f32x16 h1[HT], h2[HT], q[HT];
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) {
            f32x16 a = load_bias16(s + F.b1 + ht * 32, h);
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) a = mfma32(s[F.w1 + (ht * KS1 + ks) * 64 + lane], xb[ks], a);
#pragma unroll
            for (int r = 0; r < 16; ++r) h1[ht][r] = tanhf(a[r]);
        }
        __builtin_amdgcn_sched_barrier(0);
        const f32x4* w2l = reinterpret_cast<const f32x4*>(s + F.w2) + lane;
        const f32x4* c2l = reinterpret_cast<const f32x4*>(s + F.c2) + lane;
#pragma unroll
        for (int hto = 0; hto < HT; ++hto) {
            f32x16 a = load_bias16(s + F.b2 + hto * 32, h);
            f32x16 c = {};
#pragma unroll
            for (int kt = 0; kt < HT; ++kt)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const f32x4 w = w2l[a_quad(a_tile(hto, kt, HT), rq) * 64];
                    const f32x4 cw = c2l[a_quad(a_tile(hto, kt, HT), rq) * 64];
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const float hv = h1[kt][4 * rq + rr];
                        a = mfma32(w[rr], hv, a);
                        c = mfma32(cw[rr], fmaf(-hv, hv, 1.f), c);
                    }
                }
#pragma unroll
            for (int r = 0; r < 16; ++r) h2[hto][r] = tanhf(a[r]);
            q[hto] = c;
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!vjp) {
            float ptr = 0.f;
#pragma unroll
            for (int ht = 0; ht < HT; ++ht)
#pragma unroll
                for (int r = 0; r < 16; ++r) ptr = fmaf(fmaf(-h2[ht][r], h2[ht][r], 1.f), q[ht][r], ptr);
#pragma unroll
            for (int j = 0; j < D; ++j) {
                float pv = 0.f;
#pragma unroll
                for (int ht = 0; ht < HT; ++ht) pv = acc_dot16(s + F.w3 + (j * HT + ht) * 32, h, h2[ht], pv);
                out[j] = halves_sum(pv, pv) + s[F.b3 + j];
            }
            tr = halves_sum(ptr, ptr);
            return;
        }

        // The parameter gradients contract over the samples: their operands pass through the
        // wave's LDS tile one hidden tile at a time (h1^T is kept whole: every product below pairs
        // it, or g1^T = 1 - h1^T^2, with one tile of the other operand).
        wave_lds_sync();
        if (h == 0) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                zs[j * PITCH + col] = z[j];
                vs[j * PITCH + col] = vb[j];
            }
        }
        f32x16 h1T[HT];
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) h1T[ht] = transpose(h1[ht]);
        // h2^T: dW3 += vb h2^T, dC += (tb g2) g1^T
#pragma unroll
        for (int kt = 0; kt < HT; ++kt) {
            f32x16 xT = transpose(h2[kt]);
            {
                float vB[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) vB[r] = col < D ? vs[col * PITCH + 4 * h + crow(r, 0)] : 0.f;
                lds_tile_mfma(ga3 + kt * 512, xT, vB);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) xT[r] = (cl * ls[4 * h + crow(r, 0)]) * fmaf(-xT[r], xT[r], 1.f);
#pragma unroll
            for (int jt = 0; jt < HT; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    aC[kt * HT + jt] = mfma32(xT[r], fmaf(-h1T[jt][r], h1T[jt][r], 1.f), aC[kt * HT + jt]);
        }
        __builtin_amdgcn_sched_barrier(0);

        // a2 = g2 * (W3^T vb - 2 h2 * (tb q)),  qb = tb g2,  tb = cl * l_bar  (over h2 and q)
        const float tbar = cl * lbar;
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) {
            f32x16 wv = {};
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const f32x16 w3 = load_bias16(s + F.w3 + (j * HT + ht) * 32, h);
#pragma unroll
                for (int r = 0; r < 16; ++r) wv[r] = fmaf(w3[r], vb[j], wv[r]);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float hv = h2[ht][r], g2 = fmaf(-hv, hv, 1.f);
                h2[ht][r] = g2 * fmaf(-2.f * hv, tbar * q[ht][r], wv[r]);
                q[ht][r] = tbar * g2;
            }
        }
        f32x16(&a2)[HT] = h2;
        f32x16(&qb)[HT] = q;
        // a2^T: dW2 += a2 h1^T, db2 += a2
#pragma unroll
        for (int kt = 0; kt < HT; ++kt) {
            const f32x16 xT = transpose(a2[kt]);
#pragma unroll
            for (int jt = 0; jt < HT; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) aW2[kt * HT + jt] = mfma32(xT[r], h1T[jt][r], aW2[kt * HT + jt]);
            float sum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) sum += xT[r];
            ab2[kt] += sum;
        }
        __builtin_amdgcn_sched_barrier(0);
        // a1 = g1 * (W2^T a2 - 2 h1 * (C^T qb))  (over h1, tile by tile: a2 and qb are needed whole)
        f32x16 a1[HT];
        const f32x4* w2tl = reinterpret_cast<const f32x4*>(s + L.w2t) + lane;
        const f32x4* c2tl = reinterpret_cast<const f32x4*>(s + L.c2t) + lane;
#pragma unroll
        for (int jo = 0; jo < HT; ++jo) {
            f32x16 m = {}, n = {};
#pragma unroll
            for (int kt = 0; kt < HT; ++kt)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const f32x4 w = w2tl[a_quad(a_tile(jo, kt, HT), rq) * 64];
                    const f32x4 cw = c2tl[a_quad(a_tile(jo, kt, HT), rq) * 64];
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        m = mfma32(w[rr], a2[kt][4 * rq + rr], m);
                        n = mfma32(cw[rr], qb[kt][4 * rq + rr], n);
                    }
                }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float hv = h1[jo][r];
                a1[jo][r] = fmaf(-hv, hv, 1.f) * fmaf(-2.f * hv, n[r], m[r]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // z_bar = W1[:, :d]^T a1
#pragma unroll
        for (int j = 0; j < D; ++j) {
            float pz = 0.f;
#pragma unroll
            for (int ht = 0; ht < HT; ++ht) pz = acc_dot16(s + L.w1c + (j * HT + ht) * 32, h, a1[ht], pz);
            out[j] = halves_sum(pz, pz);
            ab3[j] += vb[j];
        }
        tr = 0.f;
        // a1^T: dW1 += a1 [z; t]^T, db1 += a1
#pragma unroll
        for (int ht = 0; ht < HT; ++ht) {
            const f32x16 xT = transpose(a1[ht]);
            float sum = 0.f, uB[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                uB[r] = col < D ? zs[col * PITCH + 4 * h + crow(r, 0)] : (col == D ? t : 0.f);
                sum += xT[r];
            }
            lds_tile_mfma(ga1 + ht * 512, xT, uB);
            ab1[ht] += sum;
        }
    };

    for (int64_t tile = (int64_t)blockIdx.x * nw + wave; tile < A.ntiles; tile += (int64_t)gridDim.x * nw) {
        const int64_t srow = tile * 32 + col;
        const bool live = srow < A.B;
        // A row that is past the batch, or whose input or final state holds a non-finite value, is a
        // dead column: zero state and zero cotangents, so it adds exact zeros to every sum.
        bool dead = !live;
        float ybar[D];
        const float* yfin = A.traj + ((int64_t)(A.g.nsteps - 1) * A.B + srow) * D;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            ybar[j] = live ? yfin[j] : 0.f;  // (the unclamped y_n for now)
            dead = dead || nonfinite(live ? A.x[srow * D + j] : 0.f) || nonfinite(ybar[j]);
        }
        const float ldfin = live ? A.traj[(int64_t)A.g.nsteps * A.B * D + srow] : 0.f;
        // torch.clamp passes the gradient where the input lies in [-10, 10], bounds included
#pragma unroll
        for (int j = 0; j < D; ++j)
            ybar[j] = (!dead && ybar[j] >= -10.f && ybar[j] <= 10.f) ? A.gy[srow * D + j] : 0.f;
        lbar = (!dead && ldfin >= -10.f && ldfin <= 10.f) ? A.gld[srow] : 0.f;  // (a NaN fails both)
        wave_lds_sync();
        if (h == 0) ls[col] = lbar;
        wave_lds_sync();

#pragma unroll 1
        for (int k = A.g.nsteps - 1; k >= 0; --k) {
#pragma clang fp contract(off)  // the cotangents' mul/adds round separately, as the stage inputs'
            const CnfStep S = cnf_step(A.g, k);
            const float dt = S.dt;
            float y[D];
            const float* yk = k == 0 ? A.x + srow * D : A.traj + ((int64_t)(k - 1) * A.B + srow) * D;
#pragma unroll
            for (int j = 0; j < D; ++j) y[j] = dead ? 0.f : yk[j];
            float k1[D], k2[D], k3[D], zb4[D], zb3[D], zb2[D], zb1[D];
#pragma unroll
            for (int j = 0; j < D; ++j) k1[j] = k2[j] = k3[j] = zb4[j] = zb3[j] = zb2[j] = zb1[j] = 0.f;
            // passes 0..2 recompute k1, k2, k3; passes 3..6 pull back through stages 4, 3, 2, 1
#pragma unroll 1
            for (int pass = 0; pass < 7; ++pass) {
                const int sg = pass < 3 ? pass + 1 : 7 - pass;
                float t, zin[D], vb[D], cl;
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    if (sg == 1) {
                        zin[j] = cnf_stage_input(1, dt, y[j], 0.f, 0.f, 0.f);
                        vb[j] = dt * 0.125f * ybar[j] + dt * zb4[j] - dt / 3.f * zb3[j] + dt / 3.f * zb2[j];
                    } else if (sg == 2) {
                        zin[j] = cnf_stage_input(2, dt, y[j], k1[j], k2[j], k3[j]);
                        vb[j] = 3.f * dt * 0.125f * ybar[j] - dt * zb4[j] + dt * zb3[j];
                    } else if (sg == 3) {
                        zin[j] = cnf_stage_input(3, dt, y[j], k1[j], k2[j], k3[j]);
                        vb[j] = 3.f * dt * 0.125f * ybar[j] + dt * zb4[j];
                    } else {
                        zin[j] = cnf_stage_input(4, dt, y[j], k1[j], k2[j], k3[j]);
                        vb[j] = dt * 0.125f * ybar[j];
                    }
                }
                if (sg == 1) {
                    t = cnf_stage_time(1, S);
                    cl = dt * 0.125f;
                } else if (sg == 2) {
                    t = cnf_stage_time(2, S);
                    cl = 3.f * dt * 0.125f;
                } else if (sg == 3) {
                    t = cnf_stage_time(3, S);
                    cl = 3.f * dt * 0.125f;
                } else {
                    t = cnf_stage_time(4, S);
                    cl = dt * 0.125f;
                }
                float o[D], tr;
                stage(t, zin, pass >= 3, vb, cl, o, tr);
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    if (pass == 0) k1[j] = o[j];
                    else if (pass == 1) k2[j] = o[j];
                    else if (pass == 2) k3[j] = o[j];
                    else if (pass == 3) zb4[j] = o[j];
                    else if (pass == 4) zb3[j] = o[j];
                    else if (pass == 5) zb2[j] = o[j];
                    else zb1[j] = o[j];
                }
            }
#pragma unroll
            for (int j = 0; j < D; ++j) ybar[j] = ybar[j] + zb1[j] + zb2[j] + zb3[j] + zb4[j];
        }

        if (live && h == 0) {
#pragma unroll
            for (int j = 0; j < D; ++j) A.gx[srow * D + j] = dead ? A.gy[srow * D + j] : ybar[j];
        }
    }

    // The wave's partial sums, in register order (every launched wave writes its slot, a wave that
    // had no tile writes zeros).
    float* slot = A.ws + ((int64_t)blockIdx.x * nw + wave) * P.total;
#pragma unroll
    for (int i = 0; i < HT * HT; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            slot[P.w2 + (i * 16 + r) * 64 + lane] = aW2[i][r];
            slot[P.c + (i * 16 + r) * 64 + lane] = aC[i][r];
        }
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            slot[P.g1 + (ht * 16 + r) * 64 + lane] = gcol ? ga1[(ht * 16 + r) * 32] : 0.f;
            slot[P.g3 + (ht * 16 + r) * 64 + lane] = gcol ? ga3[(ht * 16 + r) * 32] : 0.f;
        }
        slot[P.b1 + ht * 64 + lane] = ab1[ht];
        slot[P.b2 + ht * 64 + lane] = ab2[ht];
    }
#pragma unroll
    for (int j = 0; j < D; ++j) slot[P.b3 + j * 64 + lane] = ab3[j];
}

typedef void (*cnf_bwd_kernel_t)(CnfBwdArgs);

// Defined once per hidden width, in nfx_cnf_bwd_h{1,2}.hip.
template <int HT>
cnf_bwd_kernel_t cnf_bwd_pick_ht(int d);
template <>
cnf_bwd_kernel_t cnf_bwd_pick_ht<1>(int d);
template <>
cnf_bwd_kernel_t cnf_bwd_pick_ht<2>(int d);

template <int HT>
cnf_bwd_kernel_t cnf_bwd_pick(int d) {
    return pick_range<1, kCnfMaxD>(d, [](auto D) -> cnf_bwd_kernel_t { return cnf_bwd_kernel<HT, D()>; });
}

}  // namespace nfx

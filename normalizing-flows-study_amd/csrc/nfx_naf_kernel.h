// NeuralAutoregressiveFlow: the DeepMADE conditioner (1 to 4 masked hidden layers, LayerNorm,
// residual blocks, four activations) and the affine transform, both directions in ONE launch (see
// nfx_naf.hip for the design notes).
#pragma once
#include <math.h>

#include "nfx_tile_mlp.h"

namespace nfx {

constexpr int kNafMaxD = 16;
constexpr int kNafMaxHidden = 4;
constexpr int kNafMaxH = 128;
constexpr int kNafLayers = kNafMaxHidden + 1;  // the hidden layers and the output layer
constexpr int kNafLdsBytes = 160 * 1024;       // the whole LDS of a CU: the kernel has no other LDS

// Packed weight image (floats), every width padded to whole 32-row tiles (padding rows and columns
// are 0, and so are their bias, gamma and beta: a pad row is exactly 0 after LayerNorm and after
// every activation). All of it is staged in LDS. With NT_l = tiles of hidden layer l:
//   eps  [4]                          LayerNorm eps of hidden layer l
//   per hidden layer l:
//     w  l = 0: [NT_0][2][64][4]      A operand over the 16 input slots, quads 0 and 1 of a tile
//        l > 0: [NT_l][NT_l-1][4][64][4]   A operand, [out tile][k tile][r/4][lane][r%4]
//     v  [3][NT_l][2][16]             bias, gamma, beta in accumulator order
//   output layer:
//     w  [NT_last][4][64][4]          one out tile: row j = mu_j, row 16 + j = alpha_j (j < d)
//     v  [2][16]                      its bias, the same rows
// The input x sits on the first 8 accumulator registers of a tile, x_j in register creg(j) of lane
// half chalf(j) (j < 16), so layer 0 is k-steps 0..7 of an ordinary tile; and the output tile holds
// mu_j in the register and lane half that hold x_j, alpha_j eight registers further.
struct NafLayerDesc {
    int w, v;   // float offsets of the A operand and of the vectors
    int nt;     // out tiles
    int width;  // true width (LayerNorm divides by it)
};

struct NafLayout {
    NafLayerDesc layer[kNafLayers];  // [0, nh): hidden; [nh]: output
    int total;
};

__host__ __device__ inline NafLayout naf_layout(int d, int nh, const int* widths) {
    NafLayout L{};
    int o = 4, prev = 0;
    for (int l = 0; l < nh; ++l) {
        const int nt = (widths[l] + 31) / 32;
        L.layer[l].w = o;
        o += l == 0 ? nt * 512 : nt * prev * 1024;
        L.layer[l].v = o;
        o += 3 * 32 * nt;
        L.layer[l].nt = nt;
        L.layer[l].width = widths[l];
        prev = nt;
    }
    L.layer[nh].w = o;
    o += prev * 1024;
    L.layer[nh].v = o;
    o += 32;
    L.layer[nh].nt = 1;
    L.layer[nh].width = 2 * d;
    L.total = o;
    return L;
}

// Host-side checks shared by the forward and the backward entry points.
inline bool naf_activation(int a) { return a >= NFX_NAF_RELU && a <= NFX_NAF_GELU; }

// A residual flag needs a layer above the first whose width equals the one below it.
inline bool naf_flags_ok(int nh, const int* widths, int flags) {
    if (flags & ~(NFX_NAF_LAYER_NORM | ((2 << kNafMaxHidden) - 2))) return false;
    for (int l = 0; l < kNafMaxHidden; ++l)
        if (flags & NFX_NAF_RESIDUAL(l))
            if (l < 1 || l >= nh || widths[l] != widths[l - 1]) return false;
    return true;
}

// Padded tiles of the widest hidden layer: the instantiation a shape runs.
inline int naf_max_tiles(int nh, const int* widths) {
    int m = 1;
    for (int l = 0; l < nh; ++l) m = widths[l] > m ? widths[l] : m;
    return hidden_tiles(m);
}

struct NafArgs {
    const float* packed;
    const float* in;
    float* out;
    float* logdet;
    int64_t B, ntiles;
    int total4;      // f32x4 words of the image
    int d, nh;
    int act;         // NFX_NAF_*: the same for every wave
    int ln;          // LayerNorm after every hidden Linear
    int resmask;     // bit l: hidden layer l is a residual block
    int inverse;
    int accumulate;
    int tpw;         // sample tiles (waves at work) per workgroup
    float clamp_alpha, clamp_log_scale;
    NafLayerDesc layer[kNafLayers];
};

// Input dimension on register r (< 8) of lane half h: 0..3 and 8..11 in the lower half, 4..7 and
// 12..15 in the upper.
__device__ __forceinline__ int naf_dim(int r, int h) { return crow(r, h); }

// ---- the four activations, a tile of 16 accumulator registers at a time; `act` is uniform over
// the launch: one scalar branch per tile. All of them map 0 to 0.
__device__ __forceinline__ void naf_act16(int act, f32x16& a) {
    switch (act) {
        case NFX_NAF_RELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = trelu(a[r]);
            break;
        case NFX_NAF_ELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = a[r] > 0.f ? a[r] : expm1f(a[r]);
            break;
        case NFX_NAF_LEAKY_RELU:
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = a[r] > 0.f ? a[r] : a[r] * 0.1f;
            break;
        default:  // exact GELU, in torch's order of operations
#pragma unroll
            for (int r = 0; r < 16; ++r) a[r] = a[r] * 0.5f * (1.f + erff(a[r] * 0.70710678118654752440f));
            break;
    }
}

// Pairwise sums, so that the rounding error of a moment grows with the logarithm of the width: the 16
// registers of a tile, and the tiles of a layer (an absent tile adds an exact 0).
__device__ __forceinline__ float naf_sum16(const f32x16& v) {
    float p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = v[2 * i] + v[2 * i + 1];
    return ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
}
template <int HTM>
__device__ __forceinline__ float naf_sum_tiles(const float (&ts)[HTM]) {
    if constexpr (HTM == 1) return ts[0];
    else if constexpr (HTM == 2) return ts[0] + ts[1];
    else return (ts[0] + ts[1]) + (ts[2] + ts[3]);
}

// LayerNorm over the true width (two passes: the mean, then the squared deviations of the true
// rows only: a pad row's deviation is -mean, not 0) and the activation, for the tiles of one layer.
// A sample's rows are this lane's registers over the tiles plus the other lane half's, met in one
// halves_sum per pass.
template <int HTM>
__device__ __forceinline__ void naf_norm_act(const float* s, const NafArgs& A, const NafLayerDesc& L, float eps,
                                             int lane, f32x16 (&t)[HTM]) {
    const int h = lane >> 5;
    if (A.ln) {
        float ts[HTM];
#pragma unroll
        for (int ot = 0; ot < HTM; ++ot) ts[ot] = ot < L.nt ? naf_sum16(t[ot]) : 0.f;
        const float sum = naf_sum_tiles<HTM>(ts);
        const float n = (float)L.width;
        const float mean = halves_sum(sum, sum) / n;
        const int rows_left = L.width - 4 * h;  // row 32 ot + crow(r, 0) + 4 h is a true row below it
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
#pragma unroll
        for (int ot = 0; ot < HTM; ++ot)
            if (ot < L.nt) {
                const f32x16 g = load_bias16(s + L.v + 32 * (L.nt + ot), h);
                const f32x16 b = load_bias16(s + L.v + 32 * (2 * L.nt + ot), h);
#pragma unroll
                for (int r = 0; r < 16; ++r) t[ot][r] = fmaf(t[ot][r] * rstd, g[r], b[r]);
            }
    }
#pragma unroll
    for (int ot = 0; ot < HTM; ++ot)
        if (ot < L.nt) naf_act16(A.act, t[ot]);
}

// One tile of a layer over the k tiles below it: a = W[ot, :] below + bias. The tile below is the B
// operand as it stands (k-step 4 rq + rr reads its register 4 rq + rr). The contraction runs as four
// chains of 8 HTM k-steps each, summed pairwise, then the bias (the order of an addmm): a quarter of
// one chain's rounding error, and four MFMA chains in flight instead of one.
template <int HTM>
__device__ __forceinline__ f32x16 naf_tile(const float* s, const NafLayerDesc& L, int ot, int ntin, int lane,
                                           const f32x16 (&below)[HTM]) {
    f32x16 acc[4] = {};
    const f32x4* wl = reinterpret_cast<const f32x4*>(s + L.w) + lane;
#pragma unroll
    for (int kt = 0; kt < HTM; ++kt)
        if (kt < ntin) {
#pragma unroll
            for (int rq = 0; rq < 4; ++rq) {
                const int c = (4 * kt + rq) / HTM;  // (a constant after unrolling)
                const f32x4 w = wl[a_quad(a_tile(ot, kt, ntin), rq) * 64];
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) acc[c] = mfma32(w[rr], below[kt][4 * rq + rr], acc[c]);
            }
        }
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + load_bias16(s + L.v + 32 * ot, lane >> 5);
}

// The whole conditioner for the wave's 32 samples: the output tile, clamped to [-2, 2]. Register
// r < 8 holds mu of dimension naf_dim(r, h), register 8 + r its alpha.
template <int HTM>
__device__ __forceinline__ f32x16 naf_eval(const float* sm, const NafArgs& A, int lane, const float (&x)[8]) {
    const int h = lane >> 5;
    const float* s = sm + opaque_zero();  // no hoisting of the LDS operands out of the caller's loops
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
        naf_norm_act<HTM>(s, A, L, s[0], lane, cur);
    }
#pragma unroll 1
    for (int l = 1; l < A.nh; ++l) {
        const NafLayerDesc L = A.layer[l];
        const int ntin = A.layer[l - 1].nt;
        f32x16 nxt[HTM];
#pragma unroll
        for (int ot = 0; ot < HTM; ++ot) {
            nxt[ot] = f32x16{};
            if (ot < L.nt) nxt[ot] = naf_tile<HTM>(s, L, ot, ntin, lane, cur);
        }
        naf_norm_act<HTM>(s, A, L, s[l], lane, nxt);
        const bool res = (A.resmask >> l) & 1;
#pragma unroll
        for (int ot = 0; ot < HTM; ++ot) cur[ot] = res ? nxt[ot] + cur[ot] : nxt[ot];
        __builtin_amdgcn_sched_barrier(0);
    }
    f32x16 o = naf_tile<HTM>(s, A.layer[A.nh], 0, A.layer[A.nh - 1].nt, lane, cur);
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = tclamp(o[r], -2.f, 2.f);
    return o;
}

// s + c <- s + c + v with the rounding error of the add carried in c (Knuth's two-sum): the log-det
// keeps the errors of its d adds and folds them in once at the end.
__device__ __forceinline__ void naf_two_sum(float& s, float& c, float v) {
    const float t = s + v;
    const float bp = t - s;
    c += (s - (t - bp)) + (v - bp);
    s = t;
}

template <int HTM>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(tile_waves_per_simd(HTM), tile_waves_per_simd(HTM)))) void naf_kernel(NafArgs A) {
    extern __shared__ f32x4 lds4[];
    stage_image(lds4, A.packed, A.total4);
    const float* sm = reinterpret_cast<const float*>(lds4);

    const int lane = lane_id(), h = lane >> 5, col = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave >= A.tpw) return;  // few tiles: one wave per workgroup computes, all four staged
    const int d = A.d;
    const float ca = A.clamp_alpha, cl = A.clamp_log_scale;

    for (int64_t tile = (int64_t)blockIdx.x * A.tpw + wave; tile < A.ntiles; tile += (int64_t)gridDim.x * A.tpw) {
#pragma clang fp contract(off)  // the transform rounds op by op, as the composite's
        const int64_t srow = tile * 32 + col;
        const bool live = srow < A.B;  // a dead column carries zeros and is never stored
        float in[8], y[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int j = naf_dim(r, h);
            in[r] = live && j < d ? A.in[srow * d + j] : 0.f;
        }
        float ldp = 0.f, ldc = 0.f;  // this lane half's share of the log-det, and its rounding errors
        if (A.inverse) {
            const f32x16 o = naf_eval<HTM>(sm, A, lane, in);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float alpha = tclamp(o[8 + r], -ca, ca);
                const float ls = tclamp(-alpha, -cl, cl);
                y[r] = (in[r] - o[r]) * expf(ls);
                if (naf_dim(r, h) < d) naf_two_sum(ldp, ldc, ls);
            }
        } else {
            // d passes through the whole network from x = 0; pass i writes x_i alone
#pragma unroll
            for (int r = 0; r < 8; ++r) y[r] = 0.f;
#pragma unroll 1
            for (int i = 0; i < d; ++i) {
                const f32x16 o = naf_eval<HTM>(sm, A, lane, y);
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    if (naf_dim(r, h) == i) {
                        const float alpha = tclamp(o[8 + r], -ca, ca);
                        const float ls = tclamp(alpha, -cl, cl);
                        y[r] = in[r] * expf(ls) + o[r];
                        naf_two_sum(ldp, ldc, ls);
                    }
                }
            }
        }
        float ld;
        {
            // the two halves' shares, lower half first in both, so that both compute the same bits
            const float op = halves_other(ldp, ldp), oc = halves_other(ldc, ldc);
            float lo = h ? op : ldp, c = ldc + oc;
            naf_two_sum(lo, c, h ? ldp : op);
            ld = lo + c;
        }
        if (nonfinite(ld)) ld = 0.f;
        ld = tclamp(ld, -100.f, 100.f);
        if (live) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int j = naf_dim(r, h);
                if (j < d) A.out[srow * d + j] = nonfinite(y[r]) ? 0.f : y[r];
            }
            if (h == 0) A.logdet[srow] = A.accumulate ? A.logdet[srow] + ld : ld;
        }
    }
}

typedef void (*naf_kernel_t)(NafArgs);

// Defined once per padded width, in nfx_naf_h{1,2,4}.hip.
template <int HTM>
naf_kernel_t naf_pick_ht();
template <>
naf_kernel_t naf_pick_ht<1>();
template <>
naf_kernel_t naf_pick_ht<2>();
template <>
naf_kernel_t naf_pick_ht<4>();

// Launch the pack kernel of the image (nfx_naf.hip), for a shape the caller has checked: both kernel
// families read the same image. `who` names the entry point in the error text.
int naf_pack_image(const char* who, const NfxNafLayer* layers, int d, int n_hidden, const int* widths, float* packed,
                   hipStream_t stream);

}  // namespace nfx

// NeuralAutoregressiveFlow, the wide family: hidden widths up to 512 (see nfx_naf_wide.hip for the
// design notes). The packed image, its pack kernel, the activations, the LayerNorm rules and the
// transform are those of nfx_naf_kernel.h; what differs is where things live: a four-wave workgroup
// owns a 32-sample tile, a layer's activations sit in LDS, and the weights stream from global memory.
#pragma once
#include "nfx_naf_kernel.h"

namespace nfx {

constexpr int kNafWideMaxH = 512;
constexpr int kNafWideWaves = 4;
constexpr int kNafWideRing = 8;  // weight quads in flight per wave: 32 MFMAs of lead over the loads

// Out tiles a wave owns in a layer of `tiles` tiles (wave w owns tiles w, w + 4, ...): the
// instantiation a shape runs. 1 up to width 128, 2 up to 256, 4 up to 512.
constexpr int naf_wide_tiles_per_wave(int tiles) { return tiles <= 4 ? 1 : tiles <= 8 ? 2 : 4; }

// Tiles of one activation buffer: the widest layer, and at least the four partial tiles of the
// output layer, which the idle buffer holds.
constexpr int naf_wide_buffer_tiles(int max_tiles) { return max_tiles < 4 ? 4 : max_tiles; }

// LDS (floats): two activation buffers, then the LayerNorm partials [2][4 waves][64 lanes].
constexpr int kNafWideRedFloats = 2 * kNafWideWaves * 64;
constexpr size_t naf_wide_lds_bytes(int max_tiles) {
    return ((size_t)2 * naf_wide_buffer_tiles(max_tiles) * 1024 + kNafWideRedFloats) * sizeof(float);
}
static_assert(naf_wide_lds_bytes(kNafWideMaxH / 32) <= (size_t)kNafLdsBytes, "the widest shape fits one workgroup");

struct NafWideArgs {
    const float* packed;
    const float* in;
    float* out;
    float* logdet;
    int64_t B, ntiles;
    int d, nh;
    int act;      // NFX_NAF_*
    int ln;       // LayerNorm after every hidden Linear
    int resmask;  // bit l: hidden layer l is a residual block
    int inverse;
    int accumulate;
    int buf4;     // f32x4 words of one activation buffer
    float clamp_alpha, clamp_log_scale;
    NafLayerDesc layer[kNafLayers];
};

// An activation tile in LDS is the accumulator tile as its lanes hold it, [rq][lane][4]: quad rq of
// tile t is f32x4 word a_quad(t, rq) * 64 + lane, registers 4 rq .. 4 rq + 3. The lane that reads a
// word as a B operand is the lane number that wrote it (in whichever wave), so the k-step order is
// the one the image's A operand was packed for, and 64 lanes read 1 KiB in a row: no bank conflict.
// Quad q = 4 kt + rq of the layer below is word q * 64 + lane, and the A quads of out tile ot over
// that layer are contiguous in the same order:
static_assert(a_quad(a_tile(3, 2, 5), 1) == a_quad(a_tile(3, 0, 5), 0) + 4 * 2 + 1 && a_quad(2, 1) == 4 * 2 + 1,
              "quad q of an [ot][kt] image row and of an activation buffer are q words of 64 lanes on");

__device__ __forceinline__ void naf_wide_store_tile(f32x4* buf, int ot, int lane, const f32x16& t) {
#pragma unroll
    for (int rq = 0; rq < 4; ++rq)
        buf[a_quad(ot, rq) * 64 + lane] = f32x4{t[4 * rq], t[4 * rq + 1], t[4 * rq + 2], t[4 * rq + 3]};
}
__device__ __forceinline__ f32x16 naf_wide_load_tile(const f32x4* buf, int ot, int lane) {
    f32x16 t;
#pragma unroll
    for (int rq = 0; rq < 4; ++rq) {
        const f32x4 q = buf[a_quad(ot, rq) * 64 + lane];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) t[4 * rq + rr] = q[rr];
    }
    return t;
}

// The weight quads of a wave's chains pass through a ring of kNafWideRing register quads, each
// loaded that many quads ahead of its MFMAs: the image streams from L2 with no LDS stop. `wl` is the
// layer's A operand at this lane's word; a chain is named by the number of its first quad, and quad
// q is word wl[q * 64]. Every load of the ring is unconditional and its address a scalar select, so
// the waits on it are counted ones (a load under a branch would make every later wait a full drain).
struct NafWideRing {
    f32x4 w[kNafWideRing];
};
// The first quads of the chain at quad q0 (n quads long; a slot beyond n repeats the last quad).
__device__ __forceinline__ void naf_wide_ring_fill(NafWideRing& R, const f32x4* wl, int q0, int n) {
#pragma unroll
    for (int j = 0; j < kNafWideRing; ++j) R.w[j] = wl[(q0 + (j < n ? j : n - 1)) * 64];
}
// Slot j after quad i of the chain at q0 has used it: quad i + ring of the same chain, or quad j of
// the chain at qnext, which is as long.
__device__ __forceinline__ void naf_wide_ring_next(NafWideRing& R, const f32x4* wl, int q0, int qnext, int n, int i,
                                                   int j) {
    const int q = i + kNafWideRing < n ? q0 + i + kNafWideRing : qnext + (j < n ? j : n - 1);
    R.w[j] = wl[q * 64];
}
// One MFMA chain: the n weight quads from q0 against the n quads of the layer below at `below` (this
// lane's words), in ascending k. The ring holds the chain's first quads on entry and those of the
// chain at qnext (q0 again where nothing follows: the loads are then spare, and in bounds) on exit.
// Whole groups of ring quads run without a branch; the rest of the chain skips the MFMAs it lacks.
__device__ __forceinline__ f32x16 naf_wide_chain(NafWideRing& R, const f32x4* wl, int q0, int qnext,
                                                 const f32x4* below, int n) {
    f32x16 acc = {};
    f32x4 b = below[0];
    int i0 = 0;
    // Each step reads the next quad of the layer below before its own MFMAs and reloads its ring slot
    // after them; the scheduling barriers keep both there (gathered at the end of a group, the loads
    // would lead their first use by nothing; after the MFMAs, the LDS read would be waited for at once).
#pragma unroll 1
    for (; i0 + kNafWideRing <= n; i0 += kNafWideRing) {
#pragma unroll
        for (int j = 0; j < kNafWideRing; ++j) {
            const int i = i0 + j;
            const f32x4 bn = below[(i + 1 < n ? i + 1 : n - 1) * 64];
            __builtin_amdgcn_sched_barrier(0);
            const f32x4 a = R.w[j];
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) acc = mfma32(a[rr], b[rr], acc);
            naf_wide_ring_next(R, wl, q0, qnext, n, i, j);
            __builtin_amdgcn_sched_barrier(0);
            b = bn;
        }
    }
    if (i0 < n) {
#pragma unroll
        for (int j = 0; j < kNafWideRing - 1; ++j) {
            const int i = i0 + j;
            const f32x4 bn = below[(i + 1 < n ? i + 1 : n - 1) * 64];
            if (i < n) {
                const f32x4 a = R.w[j];
#pragma unroll
                for (int rr = 0; rr < 4; ++rr) acc = mfma32(a[rr], b[rr], acc);
            }
            naf_wide_ring_next(R, wl, q0, qnext, n, i, j);
            __builtin_amdgcn_sched_barrier(0);
            b = bn;
        }
    }
    return acc;
}

// The first quad of chain c of out tile ot over ntin k tiles: quads c ntin .. (c + 1) ntin - 1 of the
// tile's 4 ntin, the same four chains as naf_tile's at HTM == ntin.
__device__ __forceinline__ int naf_wide_chain_at(int ot, int c, int ntin) {
    const int q = c * ntin;
    return a_quad(a_tile(ot, q >> 2, ntin), q & 3);
}

// LayerNorm's sum over a sample's row, which spans the four waves: each wave leaves its share (both
// lane halves already summed) in its own slot, and after the barrier every wave adds the four in the
// same pairwise order, so the result is the same in all of them whichever wave arrived first.
__device__ __forceinline__ float naf_wide_row_sum(float* slots, int wave, int lane, float part) {
    slots[wave * 64 + lane] = halves_sum(part, part);
    __syncthreads();
    return (slots[lane] + slots[64 + lane]) + (slots[128 + lane] + slots[192 + lane]);
}

// The whole conditioner for the workgroup's 32 samples: the output tile, clamped to [-2, 2], the
// same in all four waves. Register r < 8 holds mu of dimension naf_dim(r, h), register 8 + r its
// alpha. Every branch around a barrier is uniform over the launch.
template <int TPW>
__device__ __forceinline__ f32x16 naf_wide_eval(const NafWideArgs& A, f32x4* lds4, int lane, int wave,
                                                const float (&x)[8]) {
    const int h = lane >> 5;
    const float* img = A.packed;
    float* red = reinterpret_cast<float*>(lds4 + 2 * A.buf4);
#pragma unroll 1
    for (int l = 0; l < A.nh; ++l) {
        const NafLayerDesc L = A.layer[l];
        f32x4* out = lds4 + (l & 1) * A.buf4;
        const f32x4* inbuf = lds4 + ((l & 1) ^ 1) * A.buf4;
        const f32x4* below = inbuf + lane;
        const f32x4* wl = reinterpret_cast<const f32x4*>(img + L.w) + lane;
        f32x16 t[TPW];
        if (l == 0) {
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const int ot = wave + kNafWideWaves * i;
                t[i] = f32x16{};
                if (ot < L.nt) {
                    f32x16 acc[2] = {};
#pragma unroll
                    for (int rq = 0; rq < 2; ++rq)
                        if (rq == 0 || A.d > 8) {
                            const f32x4 w = wl[(2 * ot + rq) * 64];
#pragma unroll
                            for (int rr = 0; rr < 4; ++rr) acc[rq] = mfma32(w[rr], x[4 * rq + rr], acc[rq]);
                        }
                    t[i] = (acc[0] + acc[1]) + load_bias16(img + L.v + 32 * ot, h);
                }
            }
        } else {
            const int ntin = A.layer[l - 1].nt;
            NafWideRing R;
            if (wave < L.nt) naf_wide_ring_fill(R, wl, naf_wide_chain_at(wave, 0, ntin), ntin);
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const int ot = wave + kNafWideWaves * i;
                t[i] = f32x16{};
                if (ot < L.nt) {
                    f32x16 acc[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int q0 = naf_wide_chain_at(ot, c, ntin);
                        const int qnext = c < 3 ? naf_wide_chain_at(ot, c + 1, ntin)
                                          : i + 1 < TPW && ot + kNafWideWaves < L.nt
                                              ? naf_wide_chain_at(ot + kNafWideWaves, 0, ntin)
                                              : q0;
                        acc[c] = naf_wide_chain(R, wl, q0, qnext, below + c * ntin * 64, ntin);
                    }
                    t[i] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + load_bias16(img + L.v + 32 * ot, h);
                }
            }
        }
        if (A.ln) {
            // two passes over the true width: the mean, then the squared deviations of the true rows
            // only (a pad row's deviation is -mean, not 0)
            float ts[TPW];
#pragma unroll
            for (int i = 0; i < TPW; ++i) ts[i] = wave + kNafWideWaves * i < L.nt ? naf_sum16(t[i]) : 0.f;
            const float n = (float)L.width;
            const float mean = naf_wide_row_sum(red, wave, lane, naf_sum_tiles<TPW>(ts)) / n;
            const int rows_left = L.width - 4 * h;  // row 32 ot + crow(r, 0) + 4 h is a true row below it
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const int ot = wave + kNafWideWaves * i;
                ts[i] = 0.f;
                if (ot < L.nt) {
                    f32x16 sq;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float dev = 32 * ot + crow(r, 0) < rows_left ? t[i][r] - mean : 0.f;
                        sq[r] = dev * dev;
                        t[i][r] = dev;
                    }
                    ts[i] = naf_sum16(sq);
                }
            }
            const float var = naf_wide_row_sum(red + kNafWideWaves * 64, wave, lane, naf_sum_tiles<TPW>(ts)) / n;
            const float rstd = 1.f / sqrtf(var + img[l]);
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                const int ot = wave + kNafWideWaves * i;
                if (ot < L.nt) {
                    const f32x16 g = load_bias16(img + L.v + 32 * (L.nt + ot), h);
                    const f32x16 b = load_bias16(img + L.v + 32 * (2 * L.nt + ot), h);
#pragma unroll
                    for (int r = 0; r < 16; ++r) t[i][r] = fmaf(t[i][r] * rstd, g[r], b[r]);
                }
            }
        }
        const bool res = (A.resmask >> l) & 1;
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int ot = wave + kNafWideWaves * i;
            if (ot < L.nt) {
                naf_act16(A.act, t[i]);
                // (a residual block's input is the other buffer, whole until the barrier below)
                if (res) t[i] = t[i] + naf_wide_load_tile(inbuf, ot, lane);
                naf_wide_store_tile(out, ot, lane, t[i]);
            }
        }
        __syncthreads();
    }
    // The output layer is one tile; its four chains are the four waves', met through the idle buffer
    // and summed pairwise, then the bias: naf_tile's order.
    const NafLayerDesc L = A.layer[A.nh];
    const int ntin = A.layer[A.nh - 1].nt;
    f32x4* part = lds4 + (A.nh & 1) * A.buf4;
    {
        const f32x4* below = lds4 + ((A.nh & 1) ^ 1) * A.buf4 + lane;
        const f32x4* wl = reinterpret_cast<const f32x4*>(img + L.w) + lane;
        const int q0 = naf_wide_chain_at(0, wave, ntin);
        NafWideRing R;
        naf_wide_ring_fill(R, wl, q0, ntin);
        naf_wide_store_tile(part, wave, lane, naf_wide_chain(R, wl, q0, q0, below + wave * ntin * 64, ntin));
    }
    __syncthreads();
    f32x16 o = ((naf_wide_load_tile(part, 0, lane) + naf_wide_load_tile(part, 1, lane)) +
                (naf_wide_load_tile(part, 2, lane) + naf_wide_load_tile(part, 3, lane))) +
               load_bias16(img + L.v, h);
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = tclamp(o[r], -2.f, 2.f);
    __syncthreads();  // the next pass writes the buffers the partial tiles were read from
    return o;
}

template <int TPW>
__global__ __launch_bounds__(64 * kNafWideWaves) void naf_wide_kernel(NafWideArgs A) {
    extern __shared__ f32x4 lds4[];
    const int lane = lane_id(), h = lane >> 5, col = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int d = A.d;
    const float ca = A.clamp_alpha, cl = A.clamp_log_scale;

    // (the tile is the workgroup's: every wave loads the same rows and holds the same results)
    for (int64_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
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
            const f32x16 o = naf_wide_eval<TPW>(A, lds4, lane, wave, in);
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
                const f32x16 o = naf_wide_eval<TPW>(A, lds4, lane, wave, y);
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
        if (live && wave == 0) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int j = naf_dim(r, h);
                if (j < d) A.out[srow * d + j] = nonfinite(y[r]) ? 0.f : y[r];
            }
            if (h == 0) A.logdet[srow] = A.accumulate ? A.logdet[srow] + ld : ld;
        }
    }
}

typedef void (*naf_wide_kernel_t)(NafWideArgs);

// Defined once per tiles-per-wave count, in nfx_naf_wide_t{1,2,4}.hip.
template <int TPW>
naf_wide_kernel_t naf_wide_pick();
template <>
naf_wide_kernel_t naf_wide_pick<1>();
template <>
naf_wide_kernel_t naf_wide_pick<2>();
template <>
naf_wide_kernel_t naf_wide_pick<4>();

}  // namespace nfx

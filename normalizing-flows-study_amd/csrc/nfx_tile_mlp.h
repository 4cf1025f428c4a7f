// The tile-owner MLP core shared by the ContinuousFlow (forward and backward), ResidualFlow and
// NeuralAutoregressiveFlow kernels. In all of them a wave owns a tile of 32 samples from load to
// store; the packed weight image is staged in LDS once per workgroup; hidden units sit on the
// accumulator rows of v_mfma_f32_32x32x2_f32 and samples on its columns, so a layer's accumulator
// tile is the next layer's B operand; both lane halves hold the same sample (column lane & 31), own
// different hidden-unit rows of every tile, and meet in halves_sum; narrow output layers are VALU
// dots across the two halves.
//
// Here: the pieces that are the same code in every family. The hidden x hidden k-step bodies stay
// with their kernels: they differ in chain count, operand transforms and summation order. Two
// kernels whose register allocation is at the limit keep layer 1 written out.
// Nothing below multiplies and adds outside an explicit fmaf, so no contraction mode applies.
#pragma once
#include "nfx_common.h"

namespace nfx {

// Padded hidden tiles of a hidden width: 32 -> 1, 64 -> 2, up to 128 -> 4 (a 96-wide layer runs
// the 4-tile kernels).
constexpr int hidden_tiles(int H) { return H <= 32 ? 1 : H <= 64 ? 2 : 4; }

// Waves per SIMD the launch really reaches: two up to 64 hidden units (<= 256 registers), one at
// 128 (the register file to itself).
constexpr int tile_waves_per_simd(int HT) { return HT <= 2 ? 2 : 1; }

// k-steps of a layer over NIN per-sample inputs: two inputs per step, zero beyond the last.
constexpr int layer1_ksteps(int NIN) { return (NIN + 1) / 2; }

// Copy the n4 16-byte words of the packed image to LDS with the whole workgroup, four loads in
// flight per thread, and wait for it.
__device__ __forceinline__ void stage_image(f32x4* lds4, const float* packed, int n4) {
    const f32x4* src = reinterpret_cast<const f32x4*>(packed);
    const int n = blockDim.x;
    int i = threadIdx.x;
    for (; i + 3 * n < n4; i += 4 * n) {
        const f32x4 a = src[i], b = src[i + n], c = src[i + 2 * n], e = src[i + 3 * n];
        lds4[i] = a;
        lds4[i + n] = b;
        lds4[i + 2 * n] = c;
        lds4[i + 3 * n] = e;
    }
    for (; i < n4; i += n) lds4[i] = src[i];
    __syncthreads();
}

// Layer 1 from per-sample inputs: a[ht] = W1[tile ht, :] in + b1, the pre-activation tiles. w1 is
// the A operand [HT][KS][64] (a1_elem), b1 the bias [HT][2][16]; lane half h feeds input 2 ks + h
// to k-step ks.
template <int HT, int NIN>
__device__ __forceinline__ void layer1_preact(const float* w1, const float* b1, int lane, const float (&in)[NIN],
                                              f32x16 (&a)[HT]) {
    constexpr int KS = layer1_ksteps(NIN);
    const int h = lane >> 5;
    float xb[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int k0 = 2 * ks, k1 = 2 * ks + 1;
        const float lo = in[k0];
        const float hi = k1 < NIN ? in[k1 < NIN ? k1 : 0] : 0.f;
        xb[ks] = h ? hi : lo;
    }
#pragma unroll
    for (int ht = 0; ht < HT; ++ht) {
        a[ht] = load_bias16(b1 + ht * 32, h);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) a[ht] = mfma32(w1[(ht * KS + ks) * 64 + lane], xb[ks], a[ht]);
    }
}

// One tile's worth of a VALU dot: acc + sum_r w[r] x[r] over this lane half's 16 rows, w a row in
// accumulator order ([2][16], acc_vec_row). The caller sums the tiles and the halves (halves_sum).
__device__ __forceinline__ float acc_dot16(const f32x16& w, const f32x16& x, float acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc = fmaf(w[r], x[r], acc);
    return acc;
}
__device__ __forceinline__ float acc_dot16(const float* w, int h, const f32x16& x, float acc) {
    return acc_dot16(load_bias16(w, h), x, acc);
}

}  // namespace nfx

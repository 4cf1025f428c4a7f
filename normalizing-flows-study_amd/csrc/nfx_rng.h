// The on-device N(0, I) base draw of every sampling path, and its generator state.
//
// The base value is a pure function of (seed, offset, row, dim): Philox4x32-10 (Salmon et al.,
// SC'11 — the counter-based generator torch's CUDA/HIP normal_ uses; not its stream: a separate
// generator state) keyed by `seed`, one block per four consecutive dimensions of a sample row,
// Box-Muller on the word pairs (0, 1) and (2, 3). Every kernel that draws — the stand-alone
// base_normal_kernel (nfx_rng.hip), the coupling and spline chains' prologues, the IAF tile
// kernel's SAMPLE variant — evaluates this one function, so their z agree bit for bit.
//
// Counter of block blk = dim / 4 of sample `row` (word = dim % 4 of the block's output):
//   c[0] = row[31:0]
//   c[1] = row[39:32]  |  blk[31:8] << 8  |  blk[7:0] << 24
//   c[2] = offset[31:0],  c[3] = offset[63:32]
// distinct for every (row < 2^40, blk < 2^24), i.e. far beyond dim < 2^16; for dim < 1024
// (blk < 256) it is the counter the coupling / spline chains have always used.
//
// State: device uint64[2]. [0] = the offset (one per launch), [1] = the arrival word of
// rng_commit: [63:16] a tag, [15:0] the count of workgroups that arrived, as logp_commit's word
// (nfx_common.h). Any content of [1] is valid on entry (zeros, a fill, a stale count): a word
// without the tag is claimed by one compare-and-swap, never added to.
#pragma once
#include "nfx_common.h"

namespace nfx {

__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
        const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}
// Two standard normals from two uniform words (u1 in (0, 1], so log never sees 0).
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float u1 = ((float)(a >> 8) + 1.f) * 5.9604645e-8f;  // (0, 1], 2^-24 steps
    const float u2 = (float)(b >> 8) * 5.9604645e-8f;          // [0, 1)
    const float r = sqrtf(-2.f * logf(u1));
    float sn, cs;
    sincospif(2.f * u2, &sn, &cs);
    z0 = r * cs;
    z1 = r * sn;
}

// The four Philox words of block `blk` of sample `row`.
__device__ __forceinline__ void base_words(int64_t row, uint32_t blk, uint64_t seed, uint64_t offset,
                                           uint32_t (&c)[4]) {
    c[0] = (uint32_t)row;
    c[1] = (uint32_t)((uint64_t)row >> 32) ^ ((blk >> 8) << 8) ^ (blk << 24);
    c[2] = (uint32_t)offset;
    c[3] = (uint32_t)(offset >> 32);
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
}
// The base values of dimensions 4 blk .. 4 blk + 3 of sample `row`.
__device__ __forceinline__ void base_block(int64_t row, uint32_t blk, uint64_t seed, uint64_t offset, float (&g)[4]) {
    uint32_t c[4];
    base_words(row, blk, seed, offset, c);
    box_muller(c[0], c[1], g[0], g[1]);
    box_muller(c[2], c[3], g[2], g[3]);
}
// The base value of (row, dim) alone: the block's word pair of dim, one Box-Muller.
__device__ __forceinline__ float base_value(int64_t row, int dim, uint64_t seed, uint64_t offset) {
    uint32_t c[4];
    base_words(row, (uint32_t)dim >> 2, seed, offset, c);
    float z0, z1;
    box_muller((dim & 2) ? c[2] : c[0], (dim & 2) ? c[3] : c[1], z0, z1);
    return (dim & 1) ? z1 : z0;
}
// The D base values of sample `row`.
template <int D>
__device__ __forceinline__ void base_draw(int64_t row, uint64_t seed, uint64_t offset, float (&z)[D]) {
#pragma unroll
    for (int blk = 0; blk < (D + 3) / 4; ++blk) {
        float g[4];
        base_block(row, (uint32_t)blk, seed, offset, g);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (4 * blk + q < D) z[4 * blk + q] = g[q];
    }
}

constexpr uint64_t kRngClean = 0x4E4658524E47ull << 16;  // "NFXRNG", count 0
constexpr int kRngMaxGrid = 1 << 16;                     // launches that commit stay below this

// This launch's offset. Every workgroup reads it before its rng_commit, and only the last
// commit of the launch changes it.
__device__ __forceinline__ uint64_t rng_offset(const uint64_t* rng) {
    return __hip_atomic_load(rng, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// End of a drawing kernel (every thread of every workgroup calls it once, after its last use of
// rng_offset's value; gridDim.x < kRngMaxGrid, one-dimensional grid): the last workgroup to arrive
// adds 1 to the offset and stores the clean arrival word, so the next launch on the stream — a
// replay of a captured graph included — draws fresh values. The arrival protocol is
// logp_commit's: one atomic add per workgroup; an add that met a word without the tag did not
// count, and that workgroup claims the word ("clean tag, count 1") or adds again to the clean one.
__device__ __forceinline__ void rng_commit(uint64_t* rng) {
    __syncthreads();
    if (threadIdx.x != 0) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    uint64_t* cnt = rng + 1;
    uint64_t prev = __hip_atomic_fetch_add(cnt, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while ((prev & ~0xFFFFull) != kRngClean) {
        uint64_t cur = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((cur & ~0xFFFFull) == kRngClean) {
            prev = __hip_atomic_fetch_add(cnt, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (__hip_atomic_compare_exchange_strong(cnt, &cur, kRngClean | 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                        __HIP_MEMORY_SCOPE_AGENT)) {
            prev = kRngClean;
        }
    }
    if ((unsigned)(prev & 0xFFFFu) != gridDim.x - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    __hip_atomic_store(rng, __hip_atomic_load(rng, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(cnt, kRngClean, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace nfx

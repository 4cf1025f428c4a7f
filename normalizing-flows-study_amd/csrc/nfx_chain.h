// Shared pieces of the one-launch coupling chains (nfx_affine_chain.hip: small-batch layout,
// nfx_affine_schain.hip: streaming layout for large batches).
#pragma once
#include "nfx_affine_kernel.h"
#include "nfx_rng.h"

namespace nfx {

constexpr int kChainMax = 64;
struct NfxChainPacks {
    const float* p[kChainMax];
};

// LDS-DMA of 16 bytes per lane: lane l's float4 at `src` (per-lane address) lands at LDS
// lds_dst + 16 l. Issued as inline asm so the compiler does not see an LDS write in flight (the
// builtin would make it wait vmcnt(0) before every later ds_read, which cannot alias the other
// buffer the DMA targets); completion is waited for explicitly (lds_dma_wait) before the
// barrier that publishes the buffer.
// lds_addr: the LDS byte address (lds_addr_of of the shared array + offset).
__device__ __forceinline__ void lds_dma_x4(const float* src, uint32_t lds_addr) {
    const uint32_t m = lds_addr;
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(src), "s"(__builtin_amdgcn_readfirstlane(m))
        : "memory");
}
template <typename T>
__device__ __forceinline__ uint32_t lds_addr_of(T* shared_array) {
    return (uint32_t)(uintptr_t)((__attribute__((address_space(3))) T*)shared_array);
}
__device__ __forceinline__ void lds_dma_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// The on-device base draw of the fused sampling chains (base_draw<D>, rng_offset, rng_commit):
// nfx_rng.h.

// Work of one wave in a slice of nch 64-sample chunks of a streaming chain (NW = 8 or 12 waves;
// waves w, w + 4, w + 8 share a SIMD, and all meet a barrier per layer, so a layer takes as long
// as its busiest SIMD). Every wave takes the F = nch / NW whole chunks w, w + NW, ...; the R
// leftover chunks are 2R 32-sample halves, dealt so that the largest per-SIMD load is the
// smallest possible: SIMD s gets 2R / 4 halves, one more for s < 2R % 4. Within a SIMD they go
// out one half per wave (two waves co-issue better than one wave with twice the work; with
// 2R <= NW this is "the first 2R waves take a half chunk each"), and only when a SIMD's share
// exceeds its waves do its first waves take a whole chunk instead. A wave's extra unit is
// `xtiles` 32-row tiles (0, 1 or 2) at slice row `xbase`: whole chunks lie first in the leftover
// region, so they stay 64-aligned, the halves after them. Only leftovers are cut: a slice dealt
// out entirely as halves measured slower.
struct ChainShare {
    int nfull, xtiles, xbase;
};

__host__ __device__ constexpr int chain_extra_tiles(int R, int NW, int w) {
    const int K = NW / 4, s = w & 3, i = w >> 2;
    const int q = (2 * R) / 4 + (s < (2 * R) % 4 ? 1 : 0);  // the SIMD's share, in halves (<= 2 K)
    if (q <= K) return i < q ? 1 : 0;
    return i < q - K ? 2 : 1;
}

__host__ __device__ constexpr ChainShare chain_share(int nch, int NW, int wave) {
    const int F = nch / NW, R = nch - F * NW;
    const int mine = chain_extra_tiles(R, NW, wave);
    int wholes = 0, wholes_before = 0, halves_before = 0;
    for (int w = 0; w < NW; ++w) {
        const int e = chain_extra_tiles(R, NW, w);
        wholes += e == 2;
        wholes_before += e == 2 && w < wave;
        halves_before += e == 1 && w < wave;
    }
    const int idx = mine == 2 ? 2 * wholes_before : 2 * wholes + halves_before;
    return ChainShare{F, mine, F * NW * 64 + idx * 32};
}

// The deal checks itself for every slice length a workgroup's LDS can hold: each 32-row tile of
// the slice belongs to exactly one wave, and no SIMD carries more than ceil(2 nch / 4) halves.
__host__ __device__ constexpr bool chain_share_ok(int NW, int nch0, int nch1) {
    for (int nch = nch0; nch <= nch1; ++nch) {
        int load[4] = {0, 0, 0, 0};
        unsigned long long seen[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // 2 * 256 tiles
        for (int w = 0; w < NW; ++w) {
            const ChainShare c = chain_share(nch, NW, w);
            load[w & 3] += 2 * c.nfull + c.xtiles;
            for (int u = 0; u <= c.nfull; ++u) {
                const int tiles = u < c.nfull ? 2 : c.xtiles;
                const int base = u < c.nfull ? (w + u * NW) * 64 : c.xbase;
                if (tiles == 2 && base % 64 != 0) return false;
                for (int t = 0; t < tiles; ++t) {
                    const int tile = base / 32 + t;
                    if (base % 32 != 0 || tile >= 2 * nch || (seen[tile >> 6] >> (tile & 63) & 1)) return false;
                    seen[tile >> 6] |= 1ull << (tile & 63);
                }
            }
        }
        for (int t = 0; t < 2 * nch; ++t)
            if (!(seen[t >> 6] >> (t & 63) & 1)) return false;
        for (int s = 0; s < 4; ++s)
            if (load[s] > (2 * nch + 3) / 4) return false;
    }
    return true;
}
// (nch = 1..256 in pieces: each static_assert has the constant evaluator's step budget to itself)
#define NFX_CHAIN_SHARE_CHECK(lo, hi)                                                    \
    static_assert(chain_share_ok(8, lo, hi) && chain_share_ok(12, lo, hi),               \
                  "chain_share: a tile unowned, owned twice, or a SIMD overloaded")
NFX_CHAIN_SHARE_CHECK(1, 64);
NFX_CHAIN_SHARE_CHECK(65, 112);
NFX_CHAIN_SHARE_CHECK(113, 152);
NFX_CHAIN_SHARE_CHECK(153, 184);
NFX_CHAIN_SHARE_CHECK(185, 208);
NFX_CHAIN_SHARE_CHECK(209, 232);
NFX_CHAIN_SHARE_CHECK(233, 256);
#undef NFX_CHAIN_SHARE_CHECK

// Streaming chain (nfx_affine_schain.hip): which (B, d, H) it takes and its launch.
int schain_launch(const NfxChainPacks& P, int nl, const float* in, float* out, float* log_det, int64_t B, int d,
                  int H, int direction, int accumulate, float* logp, double* sums, void* workspace, hipStream_t s);
bool schain_supported(int64_t B, int d, int H);
// The affine kernel policy (nfx_affine_kernel_policy; nfx_affine.hip).
int affine_policy_get();
// AUTO: the small-batch chain up to this batch, the streaming chain above it.
constexpr int64_t kSmallChainMaxB = 1 << 16;

}  // namespace nfx

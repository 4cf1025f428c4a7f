// The stand-alone base draw: z[B, d] ~ N(0, I) by the draw function of nfx_rng.h. It is the
// definition every fused variant (the coupling / spline chains' prologues, the IAF tile kernel's
// SAMPLE variant) matches bit for bit, and the draw of every model without a fused variant.
#include "nfx_rng.h"

namespace nfx {

constexpr int kBaseNormalThreads = 256;
constexpr int kBaseNormalMaxGrid = 4096;  // < kRngMaxGrid
static_assert(kBaseNormalMaxGrid < kRngMaxGrid, "rng_commit's count field");

// One thread per Philox block (four consecutive dimensions of one row), grid-stride: consecutive
// threads write consecutive 16-byte pieces of a row, so stores coalesce along d. (Scalar stores:
// a row's pieces are 16-byte aligned only when d % 4 == 0, and the last piece may be short.)
__global__ __launch_bounds__(kBaseNormalThreads) void base_normal_kernel(uint64_t seed, uint64_t* __restrict__ rng,
                                                                         float* __restrict__ z, int64_t B, int d) {
    const uint64_t off = rng_offset(rng);
    const int nb = (d + 3) / 4;
    const int64_t total = B * nb;
    for (int64_t i = (int64_t)blockIdx.x * kBaseNormalThreads + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * kBaseNormalThreads) {
        const int64_t row = i / nb;
        const int blk = (int)(i - row * nb);
        float g[4];
        base_block(row, (uint32_t)blk, seed, off, g);
        float* p = z + row * d + 4 * blk;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (4 * blk + q < d) p[q] = g[q];
    }
    rng_commit(rng);
}

}  // namespace nfx

using namespace nfx;

extern "C" int nfx_base_normal(uint64_t seed, uint64_t* rng_state, float* z, int64_t B, int d, void* stream) {
    if (B < 0 || d <= 0) return set_error(NFX_EINVAL, "base_normal: bad shape B=%lld d=%d", (long long)B, d);
    if (B == 0) return NFX_OK;
    if (!rng_state || !z) return set_error(NFX_EINVAL, "base_normal: null pointer");
    const int64_t total = B * ((d + 3) / 4);
    int64_t grid = (total + kBaseNormalThreads - 1) / kBaseNormalThreads;
    if (grid > kBaseNormalMaxGrid) grid = kBaseNormalMaxGrid;
    base_normal_kernel<<<(unsigned)grid, kBaseNormalThreads, 0, (hipStream_t)stream>>>(seed, rng_state, z, B, d);
    return check_launch("base_normal_kernel");
}

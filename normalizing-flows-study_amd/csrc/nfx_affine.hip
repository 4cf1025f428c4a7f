// Fused affine-coupling layer (RealNVP CouplingLayer) for gfx950.
//
// Reference: src/flows/coupling/coupling_layer.py
//   forward :40-68   x = z*m + (1-m)*(z*exp(s)+b),  ld = sum((1-m)*s)
//   inverse :70-96   z = x*m + (1-m)*((x-b)*exp(-s)), ld = sum((1-m)*(-s))
//   s = clamp(s_net(x*m), -10, 10), b = clamp(b_net(x*m), -10, 10)   (:50-51, :79-80)
//   s_net/b_net: Linear(d,H) BN ReLU Linear(H,H) BN ReLU Linear(H,d)   (:18-35)
//   guards: non-finite outputs -> 0, non-finite ld -> 0                 (:61-66, :89-94)
//
// One kernel = one layer, fully fused: conditioner MLPs on fp32 MFMA (32x32x2, activations
// kept in accumulator registers between layers, weights staged once per workgroup in LDS),
// the 64->d output layer on VALU with a v_permlane32_swap half-wave combine, the affine
// transform, the NaN/Inf guards and the per-sample log-det accumulate. HBM traffic is the
// x row in, the y row out and the log-det read-modify-write: 8d+8 bytes per sample.
//
// Work decomposition: a wave owns 64-sample chunks (two 32-sample MFMA column tiles);
// after the output layer lane l holds sample (chunk*64 + l) for the epilogue, so x/y/log_det
// accesses are fully coalesced. Waves grid-stride over chunks so the LDS weight image is
// loaded once per workgroup. Small batches go to the latency-oriented variant in
// nfx_affine_small_kernel.h instead (see affine_policy).
#include <atomic>
#include <climits>
#include <cstdlib>

#include "nfx_affine_kernel.h"
#include "nfx_affine_small_kernel.h"
#include "nfx_pack.h"

namespace nfx {


__global__ void affine_pack_kernel(NfxMlpRaw s_net, NfxMlpRaw b_net, const float* mask, int d,
                                   int H, float* packed) {
    const int HT = (H + 31) / 32;
    const AffineLayout L = affine_layout(d, HT);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L.s; i += gridDim.x * blockDim.x) {
        float v = 0.f;
        if (i >= L.mask) {
            int j = i - L.mask;
            v = j < d ? mask[j] : 0.f;
        } else {
            const int net = i / L.net;
            const NfxMlpRaw& P = net ? b_net : s_net;
            const int o = i - net * L.net;
            if (o < L.b1) {
                const RowCol e = a1_elem(o - L.w1, L.KS1);
                v = (e.row < H && e.col < d) ? mlp_weight(P, 0, d, e.row, e.col) : 0.f;
            } else if (o < L.w2) {
                int row = acc_vec_row(o - L.b1);
                v = row < H ? mlp_bias(P, 0, row) : 0.f;
            } else if (o < L.b2) {
                const ATileElem e = a_tile_elem(o - L.w2);
                int row = 32 * (e.tile / HT) + e.row, col = 32 * (e.tile % HT) + e.k;
                v = (row < H && col < H) ? mlp_weight(P, 1, H, row, col) : 0.f;
            } else if (o < L.w3) {
                int row = acc_vec_row(o - L.b2);
                v = row < H ? mlp_bias(P, 1, row) : 0.f;
            } else if (o < L.b3 && d > 8) {  // MFMA A-operand tiles of the output layer
                const ATileElem e = a_tile_elem(o - L.w3);
                int row = 32 * (e.tile / HT) + e.row, col = 32 * (e.tile % HT) + e.k;
                v = (row < d && col < H) ? mlp_weight(P, 2, H, row, col) : 0.f;
            } else if (o < L.b3) {
                int t = o - L.w3, j = t / (32 * HT), col = acc_vec_row(t % (32 * HT));
                v = col < H ? mlp_weight(P, 2, H, j, col) : 0.f;
            } else if (d > 8) {  // output bias in accumulator order
                int row = acc_vec_row(o - L.b3);
                v = row < d ? mlp_bias(P, 2, row) : 0.f;
            } else {
                int j = o - L.b3;
                v = j < d ? mlp_bias(P, 2, j) : 0.f;
            }
        }
        packed[i] = v;
    }
}

// The split tail of an affine image (affine_split, nfx_affine_kernel.h), derived from the fp32
// image written before it on the same stream: copies of w1 b1 b2 w3 b3 and the mask, W2's three
// round-to-nearest bf16 pieces in v_mfma_f32_32x32x16_bf16 A-operand order, and the safety words (W2 finite,
// |w| <= 1e6 and the lower-edge bound below; xsafe = (1e30 - max|b1|) / max_row sum|w1|). One
// workgroup: the maxima are reductions and the tail is ~14k floats.
__global__ __launch_bounds__(1024) void affine_split_pack_kernel(float* packed, int d, int H, int live_fold) {
    const int HT = (H + 31) / 32, KS1 = (d + 1) / 2;
    const AffineLayout L = affine_layout(d, HT);
    const AffineSplit S = affine_split(d, HT);
    float* out = packed + L.s;
    __shared__ int w2_bad;
    __shared__ float rowsum[2 * 64], bmax[2 * 64], w2sum[2 * 64], w3sum[2 * 8];
    if (threadIdx.x == 0) w2_bad = 0;
    __syncthreads();
    bool bad = false;
    for (int i = threadIdx.x; i < S.total; i += blockDim.x) {
        const int net = i < S.mask ? i / S.net : 0;
        const int o = i - net * S.net;
        const float* P = packed + net * L.net;
        uint32_t v = 0;
        if (i >= S.ok) {
            continue;  // the safety words: below, after the reductions
        } else if (i >= S.mask) {
            v = __float_as_uint(packed[L.mask + (i - S.mask)]);
        } else if (o < S.b1) {
            v = __float_as_uint(P[L.w1 + (o - S.w1)]);
        } else if (o < S.b2) {
            v = __float_as_uint(P[L.b1 + (o - S.b1)]);
        } else if (o < S.w3) {
            v = __float_as_uint(P[L.b2 + (o - S.b2)]);
        } else if (o < S.b3) {
            v = __float_as_uint(P[L.w3 + (o - S.w3)]);
        } else if (o < S.w2s) {
            v = __float_as_uint(P[L.b3 + (o - S.b3)]);
        } else {
            // dword t: [out tile hto][k block kb][piece p][lane][q], elements 2q, 2q + 1
            const int t = o - S.w2s, q = t & 3, lane = (t >> 2) & 63, g = t >> 8;
            const int p = g % 3, kb = (g / 3) % (2 * HT), hto = (g / 3) / (2 * HT);
            const int kt = kb >> 1;
            uint32_t half[2];
            for (int e = 0; e < 2; ++e) {
                const int r = 8 * (kb & 1) + 2 * q + e;  // accumulator register of the B operand
                const float w = P[L.w2 + ((hto * HT + kt) * 4 + (r >> 2)) * 256 + lane * 4 + (r & 3)];
                if (!(fabsf(w) <= 1e6f)) bad = true;
                // round-to-nearest pieces (random signs: unbiased dropped products, split_block)
                const uint32_t u0 = __builtin_bit_cast(uint16_t, (__bf16)w);
                const float r1 = w - __uint_as_float(u0 << 16);
                const uint32_t u1 = __builtin_bit_cast(uint16_t, (__bf16)r1);
                const uint32_t u2 = __builtin_bit_cast(uint16_t, (__bf16)(r1 - __uint_as_float(u1 << 16)));
                half[e] = p == 0 ? u0 : p == 1 ? u1 : u2;
            }
            v = half[0] | (half[1] << 16);
        }
        out[i] = __uint_as_float(v);
    }
    if (bad) atomicOr(&w2_bad, 1);
    // layer-1 bound: row sums of |w1| (rows 32 ht + c of net n) and |b1|; for the lower edge
    // below: the row sums of |w2| (same rows) and of |w3| (output j of net n)
    for (int i = threadIdx.x; i < 2 * 64; i += blockDim.x) {
        rowsum[i] = 0.f;
        bmax[i] = 0.f;
        w2sum[i] = 0.f;
        if (i < 2 * 8) w3sum[i] = 0.f;
    }
    __syncthreads();
    if (threadIdx.x < 2 * 32 * HT) {
        const int net = threadIdx.x / (32 * HT), row = threadIdx.x % (32 * HT), ht = row >> 5, c = row & 31;
        const float* P = packed + net * L.net;
        float sum = 0.f;
        for (int ks = 0; ks < KS1; ++ks)
            for (int hh = 0; hh < 2; ++hh) sum += fabsf(P[L.w1 + (ht * KS1 + ks) * 64 + c + 32 * hh]);
        rowsum[net * 64 + row] = sum;
        float b = 0.f;
        for (int r = 0; r < 16; ++r)
            for (int hh = 0; hh < 2; ++hh)
                if (crow(r, hh) == c) b = fabsf(P[L.b1 + ht * 32 + 16 * hh + r]);
        bmax[net * 64 + row] = b;
        float s2 = 0.f;  // row 32 ht + c of w2: lanes c and c + 32 of every (k tile, register) group
        for (int g = 0; g < HT * 4; ++g)
            for (int hh = 0; hh < 2; ++hh)
                for (int rr = 0; rr < 4; ++rr) s2 += fabsf(P[L.w2 + (ht * HT * 4 + g) * 256 + (c + 32 * hh) * 4 + rr]);
        w2sum[net * 64 + row] = s2;
    }
    if (threadIdx.x < 2 * d) {
        const int net = threadIdx.x / d, j = threadIdx.x % d;
        const float* P = packed + net * L.net;
        float s3 = 0.f;
        for (int t = 0; t < HT * 32; ++t) s3 += fabsf(P[L.w3 + j * HT * 32 + t]);
        w3sum[net * 8 + j] = s3;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float n1 = 0.f, c1 = 0.f;
        bool nan = false;
        for (int i = 0; i < 2 * 64; ++i) {
            nan = nan || !(rowsum[i] <= 3e38f) || !(bmax[i] <= 3e38f);
            n1 = fmaxf(n1, rowsum[i]);
            c1 = fmaxf(c1, bmax[i]);
        }
        const float xs = nan ? 0.f : (1e30f - c1) / n1;  // n1 == 0: +inf (no x reaches layer 1)
        // Lower edge: split3's pieces go to the MFMA as bf16, whose smallest subnormal is 2^-133, so
        // an activation below 2^-110 loses the bits of its third piece under 2^-133 (pack_bf16 cuts
        // them). That moves a layer-2 output by less than 2^-133 * row-sum|w2| and s by that times
        // row-sum|w3|: the layer stays on the split only while this stays under 2^-24, the
        // relative rounding of exp(s) in fp32 (NaN or inf sums fail the test).
        bool lost = false;
        for (int net = 0; net < 2; ++net) {
            float r2 = 0.f, r3 = 0.f;
            for (int i = 0; i < 64; ++i) r2 = fmaxf(r2, w2sum[net * 64 + i]);
            for (int j = 0; j < 8; ++j) r3 = fmaxf(r3, w3sum[net * 8 + j]);
            lost = lost || !(0x1p-133 * (double)r2 * (double)r3 < 0x1p-24);
        }
        const bool wok = !(w2_bad || lost);
        out[S.ok] = wok ? 1.f : 0.f;
        out[S.ok + 1] = xs > 0.f ? xs : 0.f;
        // Live outputs (affine_live_unit, nfx_affine_kernel.h): output j with mask[j] == 1.0f exactly
        // is dead, it enters the layer's result only times (1 - m) = +0. A kernel may skip the fold of the dead rows when
        // the live ones fit (D + 1) / 2 slots and no dead s or t can be NaN or inf on a tile that
        // runs the split nets: there every layer-1 activation is <= 1e30 (xsafe), so a layer-2
        // one is at most hmax = 1e30 * max row-sum|w2| + max|b2| (ok[0] holds, so the split's own
        // error is far below the margin), and every partial sum of dead row j stays under
        // row-sum|w3[j]| * hmax + |b3[j]|, required <= 1e37 (NaN or inf sums fail the test).
        int nlive = 0;
        uint32_t idx = 0x88888888u;  // slot jj: nibble jj = the output's index; 8 = unused (reads row 0)
        bool dead_ok = wok && xs > 0.f && live_fold;
        for (int j = 0; j < d; ++j) {
            if (packed[L.mask + j] == 1.0f) {
                for (int net = 0; net < 2; ++net) {
                    const float* P = packed + net * L.net;
                    float r2 = 0.f, b2 = 0.f;
                    for (int i = 0; i < 64; ++i) r2 = fmaxf(r2, w2sum[net * 64 + i]);
                    for (int i = 0; i < HT * 32; ++i) b2 = fmaxf(b2, fabsf(P[L.b2 + i]));
                    const double hmax = 1e30 * (double)r2 + (double)b2;
                    dead_ok = dead_ok && (double)w3sum[net * 8 + j] * hmax + (double)fabsf(P[L.b3 + j]) <= 1e37;
                }
            } else {
                if (nlive < 8) idx = (idx & ~(0xfu << (4 * nlive))) | ((uint32_t)j << (4 * nlive));
                ++nlive;
                // a live s that is zero by construction (a fresh layer's output weights are): the sign of
                // a zero log-det would hang on the dead outputs (affine_nets_split), so no elision
                if (w3sum[j] == 0.f && packed[L.b3 + j] == 0.f) dead_ok = false;
            }
        }
        const bool elide = dead_ok && nlive >= 1 && nlive <= (d + 1) / 2;
        out[S.ok + 2] = __uint_as_float((uint32_t)nlive | (elide ? kAffineLiveElide : 0u));
        out[S.ok + 3] = __uint_as_float(idx);
    }
}

int affine_split_pack(float* packed, int d, int H, hipStream_t s) {
    if (!affine_has_split(d, (H + 31) / 32)) return NFX_OK;
    // NFX_AFFINE_LIVE_FOLD=0 (debugging, tests): no layer packed from now on skips dead outputs
    const char* e = getenv("NFX_AFFINE_LIVE_FOLD");
    affine_split_pack_kernel<<<1, 1024, 0, s>>>(packed, d, H, e && atoi(e) == 0 ? 0 : 1);
    return check_launch("affine_split_pack_kernel");
}

static affine_kernel_t pick_affine(int HT, int d, int dir, bool logp) {
    return pick_range<1, 4>(HT, [=](auto HT_) { return affine_pick_ht<HT_()>(d, dir, logp); });
}

static affine_kernel_t pick_affine_small(int HT, int d, int dir, bool logp) {
    return pick_range<1, 4>(HT, [=](auto HT_) { return affine_small_pick_ht<HT_()>(d, dir, logp); });
}

// Kernel choice (nfx_affine_kernel_policy). AUTO compares MFMA "rounds": the streaming kernel
// runs ceil(chunks / resident waves) 64-sample chunks per wave, each a chain of ~2*HT times the
// MFMAs of one small-kernel 32-sample tile, of which the small kernel runs ceil(tiles /
// resident workgroups) per workgroup. (Measured at RealNVP H=128: small 8 us vs streaming 37 us
// per layer up to 8k samples, break-even near 64k.) Initial policy: $NFX_AFFINE_POLICY or AUTO.
static std::atomic<int>& affine_policy() {
    static std::atomic<int> v{[] {
        const char* e = getenv("NFX_AFFINE_POLICY");
        return e ? atoi(e) : NFX_AFFINE_AUTO;
    }()};
    return v;
}

int affine_policy_get() { return affine_policy().load(std::memory_order_relaxed); }

typedef void (*affine_wide_t)(const float*, const float*, float*, float*, int64_t, int, int, int64_t, float*,
                              double*, double*, float);

template <int HT>
static affine_wide_t wide_pick(int dir, bool logp) {
    if (dir > 0) return affine_wide_kernel<HT, 1, false>;
    return logp ? affine_wide_kernel<HT, -1, true> : affine_wide_kernel<HT, -1, false>;
}

static int affine_wide_launch(const float* packed, const float* in, float* out, float* log_det, int64_t B, int d,
                              int H, int direction, int accumulate, float* logp, double* sums, void* workspace,
                              hipStream_t stream) {
    const bool fused = sums != nullptr;
    const int HT = (H + 31) / 32;
    if (d > 64 || HT > 4)
        return set_error(NFX_EUNSUPPORTED, "affine_coupling: d=%d H=%d outside the compiled family (d<=64, H<=128)", d, H);
    affine_wide_t k = pick_range<1, 4>(HT, [=](auto HT_) { return wide_pick<HT_()>(direction, fused); });
    if (B == 0) return fused ? gauss_finish(reinterpret_cast<double*>(workspace), 0, sums, 0, stream) : NFX_OK;
    if (!packed || !in || !out || !log_det) return set_error(NFX_EINVAL, "affine_coupling: null pointer");
    if (in == out) return set_error(NFX_EINVAL, "affine_coupling: in and out must not alias");
    const size_t lds = (size_t)kWideWaves * 32 * (d | 1) * sizeof(float);
    const int64_t ntiles = (B + 31) / 32;
    int grid = resident_grid((const void*)k, 64 * kWideWaves, lds, (ntiles + kWideWaves - 1) / kWideWaves);
    if (grid > kMaxPartials) grid = kMaxPartials;
    double* partials = reinterpret_cast<double*>(workspace);
    k<<<grid, 64 * kWideWaves, lds, stream>>>(packed, in, out, log_det, B, d, accumulate, ntiles, logp, partials,
                                              sums, gauss_const(d));
    return check_launch("affine_wide_kernel");  // (LOGP: the last workgroup wrote sums)
}

static int affine_launch(const float* packed, const float* in, float* out, float* log_det, int64_t B,
                         int d, int H, int direction, int accumulate, float* logp, double* sums,
                         void* workspace, hipStream_t stream) {
    const bool fused = sums != nullptr;
    if (B < 0 || d <= 0 || H <= 0) return set_error(NFX_EINVAL, "affine_coupling: bad shape B=%lld d=%d H=%d", (long long)B, d, H);
    if (direction != NFX_FORWARD && direction != NFX_INVERSE)
        return set_error(NFX_EINVAL, "affine_coupling: direction must be +1 or -1");
    if (fused && B > 0 && (!logp || !workspace)) return set_error(NFX_EINVAL, "affine_coupling_logprob: null logp/workspace");
    const int HT = (H + 31) / 32;
    if (d > 8) return affine_wide_launch(packed, in, out, log_det, B, d, H, direction, accumulate, logp, sums,
                                         workspace, stream);
    affine_kernel_t k = pick_affine(HT, d, direction, fused);
    if (!k) return set_error(NFX_EUNSUPPORTED, "affine_coupling: d=%d H=%d outside the compiled family (d<=64, H<=128)", d, H);
    if (B == 0) return fused ? gauss_finish(reinterpret_cast<double*>(workspace), 0, sums, 0, stream) : NFX_OK;
    if (!packed || !in || !out || !log_det) return set_error(NFX_EINVAL, "affine_coupling: null pointer");
    if (in == out) return set_error(NFX_EINVAL, "affine_coupling: in and out must not alias");
    const AffineLayout L = affine_layout(d, HT);
    const size_t lds = (size_t)(affine_has_split(d, HT) ? affine_split(d, HT).total : L.total) * sizeof(float);
    int rc = prepare_lds((const void*)k, lds);
    if (rc) return rc;
    double* partials = reinterpret_cast<double*>(workspace);
    const int64_t nchunks = (B + 63) / 64;
    const int64_t ntiles = (B + 31) / 32;
    const int policy = affine_policy().load(std::memory_order_relaxed);
    affine_kernel_t ks = pick_affine_small(HT, d, direction, fused);
    int grid_small = resident_grid((const void*)ks, 128 * HT, 0, ntiles);
    bool small = policy == NFX_AFFINE_SMALL;
    if (policy == NFX_AFFINE_AUTO) {
        const int64_t waves = 4 * (int64_t)resident_grid((const void*)k, 256, lds, INT64_MAX);
        const int64_t rounds_stream = (nchunks + waves - 1) / waves;
        const int64_t rounds_small = (ntiles + grid_small - 1) / grid_small;
        small = rounds_small < 2 * HT * rounds_stream;
    }
    if (small) {
        if (grid_small > kMaxPartials) grid_small = kMaxPartials;
        ks<<<grid_small, 128 * HT, 0, stream>>>(packed, in, out, log_det, B, accumulate, ntiles, logp,
                                                partials, sums, gauss_const(d));
        return check_launch("affine_small_kernel");
    }
    // Up to one 32-sample half chunk per wave: when the resident waves outnumber the 64-sample
    // chunks (small batches, e.g. a strong-scaled 125k shard), the kernel's split gives every wave
    // a half chunk instead of leaving half the waves idle behind full chunks (the layer time is one
    // wave's chain: 64 -> 32 samples halves it)
    int grid = resident_grid((const void*)k, 256, lds, ((B + 31) / 32 + 3) / 4);
    if (grid > kMaxPartials) grid = kMaxPartials;
    k<<<grid, 256, lds, stream>>>(packed, in, out, log_det, B, accumulate, nchunks, logp, partials, sums,
                                  gauss_const(d));
    return check_launch("affine_coupling_kernel");
}

}  // namespace nfx

using namespace nfx;

extern "C" size_t nfx_affine_packed_floats(int d, int H) {
    if (d <= 0 || H <= 0) return 0;
    return (size_t)affine_layout(d, (H + 31) / 32).total;
}

extern "C" int nfx_affine_pack(const NfxMlpRaw* s_net, const NfxMlpRaw* b_net, const float* mask,
                               int d, int H, float* packed, void* stream) {
    if (!s_net || !b_net || !mask || !packed) return set_error(NFX_EINVAL, "affine_pack: null pointer");
    if (d <= 0 || H <= 0) return set_error(NFX_EINVAL, "affine_pack: bad shape d=%d H=%d", d, H);
    const NfxMlpRaw* nets[2] = {s_net, b_net};
    for (int n = 0; n < 2; ++n)
        for (int l = 0; l < 3; ++l)
            if (!nets[n]->w[l]) return set_error(NFX_EINVAL, "affine_pack: net %d layer %d weight is null", n, l);
    const int total = (int)nfx_affine_packed_floats(d, H);
    int blocks = (total + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    affine_pack_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(*s_net, *b_net, mask, d, H, packed);
    const int rc = check_launch("affine_pack_kernel");
    return rc ? rc : affine_split_pack(packed, d, H, (hipStream_t)stream);
}

extern "C" int nfx_affine_coupling(const float* packed, const float* in, float* out, float* log_det,
                                   int64_t B, int d, int H, int direction, int accumulate,
                                   void* stream) {
    return affine_launch(packed, in, out, log_det, B, d, H, direction, accumulate, nullptr, nullptr,
                         nullptr, (hipStream_t)stream);
}

extern "C" int nfx_affine_kernel_policy(int policy) {
    if (policy < 0) return affine_policy().load();
    if (policy > NFX_AFFINE_SMALL) return set_error(NFX_EINVAL, "affine_kernel_policy: unknown policy %d", policy);
    return affine_policy().exchange(policy);
}

extern "C" int nfx_affine_coupling_logprob(const float* packed, const float* in, float* out,
                                           float* log_det, float* logp, double* sums, void* workspace,
                                           int64_t B, int d, int H, int accumulate, void* stream) {
    if (!sums) return set_error(NFX_EINVAL, "affine_coupling_logprob: null sums");
    return affine_launch(packed, in, out, log_det, B, d, H, NFX_INVERSE, accumulate, logp, sums,
                         workspace, (hipStream_t)stream);
}

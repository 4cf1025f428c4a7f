// NeuralAutoregressiveFlow (src/flows/advanced/neural_autoregressive_flow.py): an affine
// autoregressive flow whose conditioner, DeepMADE, is a deep masked MLP: 1 to 4 hidden layers, a
// LayerNorm after every masked Linear, residual blocks between equal widths, relu / elu /
// leaky_relu(0.1) / exact gelu. ONE launch per call and direction.
//
// The reference's sampling direction is `dim` full conditioner calls from Python, about four ATen
// launches per hidden layer each. Here a wave owns a tile of 32 samples from load to store (the
// shared core, nfx_tile_mlp.h): hidden units on the accumulator rows of v_mfma_f32_32x32x2_f32,
// samples on its columns, every layer's A fragments staged once per workgroup in LDS in the order
// that makes a layer's accumulator tile the next layer's B operand. New here:
//   * the input is held like the first 8 registers of an accumulator tile (x_j in register creg(j)
//     of lane half chalf(j)), so the d -> H layer is k-steps of an ordinary tile and needs no
//     per-d instantiation; the H -> 2d layer is one more MFMA tile whose row j is mu_j and row
//     16 + j is alpha_j: mu_j and alpha_j land in the lane that holds x_j;
//   * LayerNorm per sample: a sum over the lane's accumulator registers across the layer's tiles
//     and one exchange between the lane halves, twice (mean, then squared deviations of the true
//     rows);
//   * a residual block keeps the layer's input tiles live beside the new ones;
//   * the forward direction runs its d passes inside the launch with x in registers. LayerNorm
//     mixes every hidden unit, so the conditioner is NOT autoregressive when it is on, and the
//     reference's result is what d full passes give: every pass runs the whole network.
// The number of layers, their widths, the activation, the LayerNorm flag and the residual flags are
// launch-uniform runtime values: three instantiations, one per padded width of the widest layer.
#include <math.h>

#include "nfx_naf_kernel.h"

namespace nfx {

static naf_kernel_t pick_naf(int HTM) {
    return pick_of<1, 2, 4>(HTM, [](auto HT) -> naf_kernel_t { return naf_pick_ht<HT()>(); });
}

static const char* kNafFamily =
    "outside the compiled family (1 <= d <= 16, 1 to 4 hidden layers of width 1..128, image within 160 KiB of LDS)";

// Shape inside the family: 0, or the reason.
static const char* naf_shape_problem(int d, int nh, const int* widths) {
    if (d < 1 || d > kNafMaxD) return "d";
    if (nh < 1 || nh > kNafMaxHidden) return "n_hidden";
    if (!widths) return "widths";
    for (int l = 0; l < nh; ++l)
        if (widths[l] < 1 || widths[l] > kNafMaxH) return "width";
    if ((size_t)naf_layout(d, nh, widths).total * sizeof(float) > (size_t)kNafLdsBytes) return "LDS";
    return nullptr;
}

struct NafPackArgs {
    NfxNafLayer raw[kNafLayers];
    NafLayout lay;
    int d, nh;
    float* packed;
};

constexpr int kNafPackThreads = 256;

__device__ __forceinline__ float naf_weight(const NfxNafLayer& r, int row, int col, int cols) {
    const float w = r.weight[row * cols + col];
    return r.mask ? w * r.mask[row * cols + col] : w;
}

// One thread per image float: which layer and section it lies in, then the nfx_tile.h decode.
__global__ __launch_bounds__(kNafPackThreads) void naf_pack_kernel(NafPackArgs P) {
    const int d = P.d, nh = P.nh;
    for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < P.lay.total; o += gridDim.x * blockDim.x) {
        float v = 0.f;
        if (o < 4) {
            if (o < nh && P.raw[o].ln_weight) v = P.raw[o].ln_eps;
        } else {
            int l = 0;
            while (l < nh && o >= P.lay.layer[l + 1].w) ++l;
            const NafLayerDesc L = P.lay.layer[l];
            const NfxNafLayer& R = P.raw[l];
            const int cols = l == 0 ? d : P.lay.layer[l - 1].width;
            if (l == nh) {  // output layer: row j = mu_j, row 16 + j = alpha_j
                if (o < L.v) {
                    const RowCol e = a_image_elem(o - L.w, P.lay.layer[l - 1].nt);  // (one out tile)
                    const int j = e.row & 15;
                    if (j < d && e.col < cols) v = naf_weight(R, (e.row >> 4) * d + j, e.col, cols);
                } else {
                    const int row = acc_vec_row(o - L.v), j = row & 15;
                    if (j < d) v = R.bias[(row >> 4) * d + j];
                }
            } else if (o < L.v) {
                int row, k;
                if (l == 0) {  // half tiles: quads 0 and 1, the 16 input slots
                    const int t = o - L.w;
                    const ATileElem e = a_tile_elem(t & 511);
                    row = 32 * (t >> 9) + e.row;
                    k = e.k;
                } else {
                    const RowCol e = a_image_elem(o - L.w, P.lay.layer[l - 1].nt);
                    row = e.row;
                    k = e.col;
                }
                if (row < L.width && k < cols) v = naf_weight(R, row, k, cols);
            } else {  // bias, gamma, beta
                const VecRow e = acc_rows_elem(o - L.v, L.nt);
                if (e.row < L.width) {
                    if (e.vec == 0) v = R.bias[e.row];
                    else if (R.ln_weight) v = e.vec == 1 ? R.ln_weight[e.row] : R.ln_bias[e.row];
                }
            }
        }
        P.packed[o] = v;
    }
}

}  // namespace nfx

using namespace nfx;

extern "C" size_t nfx_naf_packed_floats(int d, int n_hidden, const int* widths) {
    if (naf_shape_problem(d, n_hidden, widths)) return 0;
    return (size_t)naf_layout(d, n_hidden, widths).total;
}

extern "C" int nfx_naf_supported(int64_t B, int d, int n_hidden, const int* widths, int activation, int flags) {
    return B >= 1 && !naf_shape_problem(d, n_hidden, widths) && naf_activation(activation) &&
                   naf_flags_ok(n_hidden, widths, flags)
               ? 1
               : 0;
}

int nfx::naf_pack_image(const char* who, const NfxNafLayer* layers, int d, int n_hidden, const int* widths,
                        float* packed, hipStream_t stream) {
    if (int rc = check_pointers(who, {layers, packed})) return rc;
    NafPackArgs P{};
    for (int l = 0; l <= n_hidden; ++l) {
        const NfxNafLayer& r = layers[l];
        if (!r.weight || !r.bias) return set_error(NFX_EINVAL, "%s: layer %d weight or bias is null", who, l);
        if ((r.ln_weight == nullptr) != (r.ln_bias == nullptr))
            return set_error(NFX_EINVAL, "%s: layer %d needs both LayerNorm vectors or neither", who, l);
        if (r.residual && (l < 1 || l >= n_hidden || widths[l] != widths[l - 1]))
            return set_error(NFX_EINVAL, "%s: layer %d cannot be a residual block", who, l);
        if (l == n_hidden && r.ln_weight) return set_error(NFX_EINVAL, "%s: the output layer has no LayerNorm", who);
        P.raw[l] = r;
    }
    P.lay = naf_layout(d, n_hidden, widths);
    P.d = d;
    P.nh = n_hidden;
    P.packed = packed;
    const int per_block = 4 * kNafPackThreads;
    naf_pack_kernel<<<(P.lay.total + per_block - 1) / per_block, kNafPackThreads, 0, stream>>>(P);
    return check_launch("naf_pack_kernel");
}

extern "C" int nfx_naf_pack(const NfxNafLayer* layers, int d, int n_hidden, const int* widths, float* packed,
                            void* stream) {
    if (d <= 0 || n_hidden <= 0 || !widths)
        return set_error(NFX_EINVAL, "naf_pack: bad shape d=%d n_hidden=%d", d, n_hidden);
    if (const char* why = naf_shape_problem(d, n_hidden, widths))
        return set_error(NFX_EUNSUPPORTED, "naf: d=%d n_hidden=%d %s (%s)", d, n_hidden, kNafFamily, why);
    return naf_pack_image("naf_pack", layers, d, n_hidden, widths, packed, (hipStream_t)stream);
}

extern "C" int nfx_naf_flow(const float* packed, const float* in, float* out, float* log_det, int64_t B, int d,
                            int n_hidden, const int* widths, int activation, int flags, float clamp_alpha,
                            float clamp_log_scale, int direction, int accumulate, void* stream) {
    if (B < 0 || d <= 0 || n_hidden <= 0 || !widths)
        return set_error(NFX_EINVAL, "naf: bad shape B=%lld d=%d n_hidden=%d", (long long)B, d, n_hidden);
    if (int rc = check_direction("naf", direction)) return rc;
    if (const char* why = naf_shape_problem(d, n_hidden, widths))
        return set_error(NFX_EUNSUPPORTED, "naf: d=%d n_hidden=%d %s (%s)", d, n_hidden, kNafFamily, why);
    if (!naf_activation(activation))
        return set_error(NFX_EUNSUPPORTED, "naf: activation=%d is not one of NFX_NAF_*", activation);
    if (!naf_flags_ok(n_hidden, widths, flags))
        return set_error(NFX_EINVAL, "naf: flags=0x%x name a residual block between unequal widths or an unknown bit",
                         flags);
    naf_kernel_t k = pick_naf(naf_max_tiles(n_hidden, widths));
    if (!k) return set_error(NFX_EUNSUPPORTED, "naf: no kernel for these widths");
    if (B == 0) return NFX_OK;
    if (int rc = check_io("naf", {packed, in, out, log_det}, in, out)) return rc;
    const NafLayout lay = naf_layout(d, n_hidden, widths);
    NafArgs A{};
    A.packed = packed;
    A.in = in;
    A.out = out;
    A.logdet = log_det;
    A.B = B;
    A.ntiles = (B + 31) / 32;
    A.total4 = lay.total / 4;
    A.d = d;
    A.nh = n_hidden;
    A.act = activation;
    A.ln = flags & NFX_NAF_LAYER_NORM ? 1 : 0;
    A.resmask = (flags >> 1) & ((1 << kNafMaxHidden) - 1);
    A.inverse = direction == NFX_INVERSE ? 1 : 0;
    A.accumulate = accumulate ? 1 : 0;
    A.clamp_alpha = clamp_alpha;
    A.clamp_log_scale = clamp_log_scale;
    for (int l = 0; l <= n_hidden; ++l) A.layer[l] = lay.layer[l];
    const size_t lds = (size_t)lay.total * sizeof(float);
    // Every workgroup is four waves, which stage the image together. How many of them compute
    // follows the load: while every tile finds a resident workgroup slot of its own, one wave per
    // workgroup (the tiles spread over every CU); beyond that 2, 3 or 4 waves share a staged image,
    // as many as it takes for the resident workgroups to cover the tiles in one round, so no CU
    // walks through tiles on one SIMD while the other three idle.
    const int threads = 256;
    int rc = prepare_lds((const void*)k, lds);
    if (rc) return rc;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k, threads, lds) != hipSuccess ||
        per_cu <= 0) {
        (void)hipGetLastError();
        per_cu = 1;
    }
    const int64_t slots = (int64_t)num_cus() * per_cu;
    const int64_t want = (A.ntiles + slots - 1) / slots;
    A.tpw = want < 1 ? 1 : want > 4 ? 4 : (int)want;
    return launch_resident((const void*)k, &A, threads, lds, (A.ntiles + A.tpw - 1) / A.tpw, (hipStream_t)stream,
                           "naf_flow_kernel");
}

// NeuralAutoregressiveFlow, the wide kernel family: hidden widths up to 512, the shapes the
// constructor's default [512, 512, 512] produces. ONE launch per call and direction, as naf_kernel.
//
// naf_kernel (nfx_naf.hip) keeps the whole image in LDS and a layer's activations in a wave's
// accumulator registers; a 512-wide layer would need 256 registers per lane for one layer's output
// and an image of megabytes. Here the roles are swapped:
//   * a four-wave workgroup owns a tile of 32 samples; wave w computes out tiles w, w + 4, ... of
//     every hidden layer (four tiles, 64 accumulator registers, at width 512);
//   * a layer's activations live in LDS, in two buffers of up to 16 tiles (64 KiB) each, "layer
//     input" and "layer output", swapped after every layer: a residual block and the other waves'
//     contractions need the input whole until the layer's closing barrier. A tile is stored as the
//     accumulator registers of its lanes, so reading it back as the B operand needs no index
//     arithmetic beyond nfx_tile.h's quads and is free of bank conflicts;
//   * the weights stay in global memory, in the image nfx_naf_pack writes (A-operand order, W * mask
//     folded in, widths padded to whole tiles with zero weight, bias, gamma and beta). Every
//     workgroup streams the same image through L2, each wave eight quads ahead of its MFMAs;
//   * the contraction of a tile is naf_tile's: four chains over quarters of the k range, summed
//     pairwise, then the bias. The output layer is one tile: each wave runs one of its four chains,
//     and they meet in the idle buffer;
//   * LayerNorm's two row sums (the mean; the squared deviations of the TRUE rows) span the four
//     waves: 64 floats per wave in a small LDS section, a barrier, and the same pairwise sum in every
//     wave, so the result does not depend on which wave arrives first.
// Nothing is read from LDS that the launch did not write, no sample reads another sample's column,
// and a partial tile computes on zeros and stores its true rows only.
// Three instantiations by out tiles per wave (1, 2, 4); everything else is a runtime value.
#include <math.h>

#include "nfx_naf_wide_kernel.h"

namespace nfx {

static naf_wide_kernel_t pick_naf_wide(int TPW) {
    return pick_of<1, 2, 4>(TPW, [](auto T) -> naf_wide_kernel_t { return naf_wide_pick<T()>(); });
}

static const char* kNafWideFamily =
    "outside the wide family (1 <= d <= 16, 1 to 4 hidden layers of width 1..512)";

// Shape inside the family: 0, or the reason.
static const char* naf_wide_shape_problem(int d, int nh, const int* widths) {
    if (d < 1 || d > kNafMaxD) return "d";
    if (nh < 1 || nh > kNafMaxHidden) return "n_hidden";
    if (!widths) return "widths";
    for (int l = 0; l < nh; ++l)
        if (widths[l] < 1 || widths[l] > kNafWideMaxH) return "width";
    return nullptr;
}

// Tiles of the widest hidden layer.
static int naf_wide_max_tiles(int nh, const int* widths) {
    int m = 1;
    for (int l = 0; l < nh; ++l) m = widths[l] > m ? widths[l] : m;
    return (m + 31) / 32;
}

}  // namespace nfx

using namespace nfx;

extern "C" size_t nfx_naf_wide_packed_floats(int d, int n_hidden, const int* widths) {
    if (naf_wide_shape_problem(d, n_hidden, widths)) return 0;
    return (size_t)naf_layout(d, n_hidden, widths).total;
}

extern "C" int nfx_naf_wide_supported(int64_t B, int d, int n_hidden, const int* widths, int activation, int flags) {
    return B >= 1 && !naf_wide_shape_problem(d, n_hidden, widths) && naf_activation(activation) &&
                   naf_flags_ok(n_hidden, widths, flags)
               ? 1
               : 0;
}

extern "C" int nfx_naf_wide_pack(const NfxNafLayer* layers, int d, int n_hidden, const int* widths, float* packed,
                                 void* stream) {
    if (d <= 0 || n_hidden <= 0 || !widths)
        return set_error(NFX_EINVAL, "naf_wide_pack: bad shape d=%d n_hidden=%d", d, n_hidden);
    if (const char* why = naf_wide_shape_problem(d, n_hidden, widths))
        return set_error(NFX_EUNSUPPORTED, "naf_wide: d=%d n_hidden=%d %s (%s)", d, n_hidden, kNafWideFamily, why);
    return naf_pack_image("naf_wide_pack", layers, d, n_hidden, widths, packed, (hipStream_t)stream);
}

extern "C" int nfx_naf_wide_flow(const float* packed, const float* in, float* out, float* log_det, int64_t B, int d,
                                 int n_hidden, const int* widths, int activation, int flags, float clamp_alpha,
                                 float clamp_log_scale, int direction, int accumulate, void* stream) {
    if (B < 0 || d <= 0 || n_hidden <= 0 || !widths)
        return set_error(NFX_EINVAL, "naf_wide: bad shape B=%lld d=%d n_hidden=%d", (long long)B, d, n_hidden);
    if (int rc = check_direction("naf_wide", direction)) return rc;
    if (const char* why = naf_wide_shape_problem(d, n_hidden, widths))
        return set_error(NFX_EUNSUPPORTED, "naf_wide: d=%d n_hidden=%d %s (%s)", d, n_hidden, kNafWideFamily, why);
    if (!naf_activation(activation))
        return set_error(NFX_EUNSUPPORTED, "naf_wide: activation=%d is not one of NFX_NAF_*", activation);
    if (!naf_flags_ok(n_hidden, widths, flags))
        return set_error(NFX_EINVAL,
                         "naf_wide: flags=0x%x name a residual block between unequal widths or an unknown bit", flags);
    const int max_tiles = naf_wide_max_tiles(n_hidden, widths);
    naf_wide_kernel_t k = pick_naf_wide(naf_wide_tiles_per_wave(max_tiles));
    if (!k) return set_error(NFX_EUNSUPPORTED, "naf_wide: no kernel for these widths");
    if (B == 0) return NFX_OK;
    if (int rc = check_io("naf_wide", {packed, in, out, log_det}, in, out)) return rc;
    const NafLayout lay = naf_layout(d, n_hidden, widths);
    NafWideArgs A{};
    A.packed = packed;
    A.in = in;
    A.out = out;
    A.logdet = log_det;
    A.B = B;
    A.ntiles = (B + 31) / 32;
    A.d = d;
    A.nh = n_hidden;
    A.act = activation;
    A.ln = flags & NFX_NAF_LAYER_NORM ? 1 : 0;
    A.resmask = (flags >> 1) & ((1 << kNafMaxHidden) - 1);
    A.inverse = direction == NFX_INVERSE ? 1 : 0;
    A.accumulate = accumulate ? 1 : 0;
    A.buf4 = naf_wide_buffer_tiles(max_tiles) * 256;
    A.clamp_alpha = clamp_alpha;
    A.clamp_log_scale = clamp_log_scale;
    for (int l = 0; l <= n_hidden; ++l) A.layer[l] = lay.layer[l];
    // One workgroup per 32-row tile, as many as are resident at once; beyond that a workgroup walks
    // through its tiles.
    return launch_resident((const void*)k, &A, 64 * kNafWideWaves, naf_wide_lds_bytes(max_tiles), A.ntiles,
                           (hipStream_t)stream, "naf_wide_kernel");
}

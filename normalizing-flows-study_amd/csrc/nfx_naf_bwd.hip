// Backward of NeuralAutoregressiveFlow's density direction (nfx_naf.hip, NFX_INVERSE): the gradients
// autograd gives for the torch composite, with respect to the input and every parameter of the
// DeepMADE conditioner, for 1 <= d <= 16 and 1 to 4 hidden layers of width 1..64.
//
// The density direction is ONE conditioner pass, so nothing is saved by the forward: the backward
// recomputes the conditioner from x exactly as naf_eval does (same contraction order, LayerNorm and
// activations, so the clamp masks are the forward's), keeping per hidden layer the normalised value
// x^ (without LayerNorm: the pre-activation p), rstd and the layer's output. With o the output
// before its [-2, 2] clamp, gz and gld the cotangents of z and of the log-det:
//   guards     gld passes where the summed log-det is finite and within +-100, gz_j where z_j is finite
//   transform  ls_j = clamp(-clamp(alpha_j, +-ca), +-cl), z_j = (x_j - mu_j) exp(ls_j):
//              mu_bar_j = -gz_j exp(ls_j), ls_bar_j = gz_j z_j + gld, alpha_bar_j = -ls_bar_j where both
//              clamps pass (closed intervals), gx_j = gz_j exp(ls_j) + (the conditioner's share)
//   clamp      o_bar = (mu_bar, alpha_bar) where -2 <= o <= 2
//   a layer    in_bar = (W o M)^T a, dW += a (x) in, db += a; a residual block adds its output's
//              cotangent to its input's
//   activation g^ = g * act'(p): relu 1 / 0, leaky 1 / 0.1, elu 1 / exp(p), gelu Phi(p) + p phi(p)
//   LayerNorm  dgamma += g^ x^, dbeta += g^, a = rstd (gamma g^ - mean(gamma g^) - x^ mean(gamma g^ x^)),
//              the means over the true rows
// and MaskedLinear multiplies weight * mask, so the weight gradient is mask o dW (the finish).
//
// A wave owns a tile of 32 samples, as in the forward; the image (the forward image and every
// layer's transposed A operand) is staged once per workgroup. The data path (W x, W^T a) runs on
// MFMA with accumulator tiles as B operands. The parameter products contract over the sample axis,
// which the accumulator layout keeps in lanes: a and the layer's input pass, one 32 x 32 tile at a
// time, through a wave-private LDS tile that returns them with the sample in the register index.
// The kept values go to a per-wave stretch of the workspace and come back to the lane that wrote
// them (plain vector stores and loads, L2-resident: 8 KiB per layer and tile); the layer count is
// a runtime value, so registers could hold them only in a kernel per layer count.
//
// No float atomics: a wave advances its sums in its own workspace slot once per tile,
// naf_bwd_reduce sums the slots in a fixed order in float64, and naf_bwd_finish decodes the register
// order, applies the masks and writes every gradient in nn.Linear / nn.LayerNorm layout. Same
// inputs, same bits.
//
// A row with a non-finite input element or conditioner output adds nothing to any parameter
// gradient and gets gx = 0 (autograd on the composite gives NaN there, through 0 * NaN behind
// torch.where): a deliberate difference, as in the residual flow.
#include <math.h>

#include "nfx_naf_bwd_kernel.h"

namespace nfx {

static naf_bwd_kernel_t pick_naf_bwd(int HTM) {
    return pick_of<1, 2>(HTM, [](auto HT) -> naf_bwd_kernel_t { return naf_bwd_pick_ht<HT()>(); });
}

static const char* kNafBwdFamily =
    "outside the compiled family (1 <= d <= 16, 1 to 4 hidden layers of width 1..64, image and transposition tiles "
    "within 160 KiB of LDS)";

// LDS of a four-wave workgroup: the image and the waves' transposition tiles.
static size_t naf_bwd_lds_bytes(int d, int nh, const int* widths, int nw) {
    return sizeof(float) * ((size_t)naf_bwd_layout(d, nh, widths).total + (size_t)nw * kNafBwdWaveFloats);
}

// Shape inside the family: 0, or the reason.
static const char* naf_bwd_shape_problem(int d, int nh, const int* widths) {
    if (d < 1 || d > kNafMaxD) return "d";
    if (nh < 1 || nh > kNafMaxHidden) return "n_hidden";
    if (!widths) return "widths";
    for (int l = 0; l < nh; ++l)
        if (widths[l] < 1 || widths[l] > kNafBwdMaxH) return "width";
    if (naf_bwd_lds_bytes(d, nh, widths, 4) > (size_t)kNafLdsBytes) return "LDS";
    return nullptr;
}

static bool naf_bwd_family(int64_t B, int d, int nh, const int* widths) {
    return B >= 1 && !naf_bwd_shape_problem(d, nh, widths);
}

static size_t naf_bwd_slots(int64_t ntiles) { return (size_t)naf_bwd_grid(ntiles) * (naf_bwd_threads(ntiles) / 64); }

// Workspace (floats): the slots, the float64 totals of one slot's length, the waves' kept values.
static size_t naf_bwd_keep_floats(int nh, const int* widths) {
    return (size_t)nh * naf_bwd_keep_layer_floats(naf_max_tiles(nh, widths));
}

struct NafBwdPackArgs {
    NfxNafLayer raw[kNafLayers];
    NafBwdLayout lay;
    int d, nh;
    float* packed;
};

// The part of the backward image behind the forward image (which nfx_naf_pack writes): one thread
// per float, (input row i, output row k) of (W o M)^T from the nfx_tile.h decode.
__global__ __launch_bounds__(256) void naf_bwd_pack_kernel(NafBwdPackArgs P) {
    const int d = P.d, nh = P.nh;
    for (int o = P.lay.F.total + blockIdx.x * blockDim.x + threadIdx.x; o < P.lay.total;
         o += gridDim.x * blockDim.x) {
        int l = 0;
        while (l < nh && o >= P.lay.layer[l + 1].wt) ++l;
        const NfxNafLayer& R = P.raw[l];
        const int cols = l == 0 ? d : P.lay.F.layer[l - 1].width;
        const RowCol e = a_image_elem(o - P.lay.layer[l].wt, P.lay.F.layer[l].nt);
        const int i = e.row, k = e.col;
        float v = 0.f;
        if (i < cols) {
            int row = -1;  // the Linear's row on tile row k
            if (l == nh) {
                if (k < 32 && (k & 15) < d) row = (k >> 4) * d + (k & 15);
            } else if (k < P.lay.F.layer[l].width) {
                row = k;
            }
            if (row >= 0) {
                v = R.weight[row * cols + i];
                if (R.mask) v *= R.mask[row * cols + i];
            }
        }
        P.packed[o] = v;
    }
}

// tot[e] = sum over the slots in float64, in an order that depends on nslots alone: the slots are cut
// into kNafBwdReduceSegs runs of consecutive slots, each run is summed in slot order by one thread,
// and the runs' sums are added in run order. A workgroup takes 64 consecutive elements (256-byte
// reads) times the runs: one thread per element would walk 1,024 slots with one load in flight
// (measured 369 us at 65,536 rows, against 80 us for the sweep itself).
constexpr int kNafBwdReduceSegs = 16;

__global__ __launch_bounds__(64 * kNafBwdReduceSegs) void naf_bwd_reduce_kernel(const float* __restrict__ ws, int nslots,
                                                                              int len, double* __restrict__ tot) {
    __shared__ double part[kNafBwdReduceSegs][64];
    const int i = threadIdx.x & 63, seg = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + i;
    const int per = (nslots + kNafBwdReduceSegs - 1) / kNafBwdReduceSegs;
    const int s0 = seg * per, s1 = s0 + per < nslots ? s0 + per : nslots;
    double acc = 0.0;
    if (e < len) {
#pragma unroll 8
        for (int sl = s0; sl < s1; ++sl) acc += (double)ws[(size_t)sl * len + e];
    }
    part[seg][i] = acc;
    __syncthreads();
    if (seg == 0 && e < len) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < kNafBwdReduceSegs; ++k) t += part[k][i];
        tot[e] = t;
    }
}

struct NafBwdFinishArgs {
    const double* tot;
    NfxNafLayer raw[kNafLayers];
    NfxNafLayerGrad grad[kNafLayers];
    NafBwdLayout lay;
    int d, nh;
    int first[kNafLayers + 1];  // first output element of every layer, and the total
};

// One thread per gradient element: decode the register order, apply the mask.
__global__ void naf_bwd_finish_kernel(NafBwdFinishArgs P) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P.first[P.nh + 1]) return;
    int l = 0;
    while (e >= P.first[l + 1]) ++l;
    e -= P.first[l];
    const bool out = l == P.nh;
    const int rows = out ? 2 * P.d : P.lay.F.layer[l].width;
    const int cols = l == 0 ? P.d : P.lay.F.layer[l - 1].width;
    const NafBwdLayerDesc BL = P.lay.layer[l];
    const NfxNafLayer& R = P.raw[l];
    const NfxNafLayerGrad& G = P.grad[l];
    auto tile_row = [&](int row) { return out ? (row / P.d) * 16 + row % P.d : row; };
    auto vec = [&](int base, int row) -> double {
        const int t = tile_row(row), o = base + (t >> 5) * 64 + (t & 31);
        return P.tot[o] + P.tot[o + 32];
    };
    if (e < rows * cols) {
        const int row = e / cols, c = e % cols, t = tile_row(row);
        double v = P.tot[BL.gw + ((t >> 5) * BL.ntin + (c >> 5)) * 1024 + acc_dump_index(t & 31, c & 31)];
        if (R.mask) v *= (double)R.mask[e];
        if (G.weight) G.weight[e] = (float)v;
        return;
    }
    e -= rows * cols;
    if (e < rows) {
        if (G.bias) G.bias[e] = (float)vec(BL.gb, e);
    } else if (e < 2 * rows) {
        if (G.ln_weight) G.ln_weight[e - rows] = (float)vec(BL.gg, e - rows);
    } else {
        if (G.ln_bias) G.ln_bias[e - 2 * rows] = (float)vec(BL.ge, e - 2 * rows);
    }
}

}  // namespace nfx

using namespace nfx;

extern "C" int nfx_naf_backward_supported(int64_t B, int d, int n_hidden, const int* widths, int activation,
                                          int flags) {
    return naf_bwd_family(B, d, n_hidden, widths) && naf_activation(activation) &&
                   naf_flags_ok(n_hidden, widths, flags)
               ? 1
               : 0;
}

extern "C" size_t nfx_naf_backward_packed_floats(int d, int n_hidden, const int* widths) {
    if (naf_bwd_shape_problem(d, n_hidden, widths)) return 0;
    return (size_t)naf_bwd_layout(d, n_hidden, widths).total;
}

extern "C" size_t nfx_naf_backward_slots(int64_t B, int d, int n_hidden, const int* widths) {
    if (!naf_bwd_family(B, d, n_hidden, widths)) return 0;
    return naf_bwd_slots((B + 31) / 32);
}

extern "C" size_t nfx_naf_backward_block_threads(int64_t B, int d, int n_hidden, const int* widths) {
    if (!naf_bwd_family(B, d, n_hidden, widths)) return 0;
    return (size_t)naf_bwd_threads((B + 31) / 32);
}

extern "C" size_t nfx_naf_backward_workspace_floats(int64_t B, int d, int n_hidden, const int* widths) {
    if (!naf_bwd_family(B, d, n_hidden, widths)) return 0;
    const size_t len = (size_t)naf_bwd_layout(d, n_hidden, widths).partial;
    const size_t slots = naf_bwd_slots((B + 31) / 32);
    return slots * len + 2 * len + slots * naf_bwd_keep_floats(n_hidden, widths);
}

static int naf_bwd_check_layers(const char* what, const NfxNafLayer* layers, int n_hidden, const int* widths) {
    for (int l = 0; l <= n_hidden; ++l) {
        const NfxNafLayer& r = layers[l];
        if (!r.weight || !r.bias) return set_error(NFX_EINVAL, "%s: layer %d weight or bias is null", what, l);
        if ((r.ln_weight == nullptr) != (r.ln_bias == nullptr))
            return set_error(NFX_EINVAL, "%s: layer %d needs both LayerNorm vectors or neither", what, l);
        if (r.residual && (l < 1 || l >= n_hidden || widths[l] != widths[l - 1]))
            return set_error(NFX_EINVAL, "%s: layer %d cannot be a residual block", what, l);
        if (l == n_hidden && r.ln_weight) return set_error(NFX_EINVAL, "%s: the output layer has no LayerNorm", what);
    }
    return NFX_OK;
}

extern "C" int nfx_naf_pack_backward(const NfxNafLayer* layers, int d, int n_hidden, const int* widths, float* packed,
                                     void* stream) {
    if (d <= 0 || n_hidden <= 0 || !widths)
        return set_error(NFX_EINVAL, "naf_pack_backward: bad shape d=%d n_hidden=%d", d, n_hidden);
    if (const char* why = naf_bwd_shape_problem(d, n_hidden, widths))
        return set_error(NFX_EUNSUPPORTED, "naf backward: d=%d n_hidden=%d %s (%s)", d, n_hidden, kNafBwdFamily, why);
    if (int rc = check_pointers("naf_pack_backward", {layers, packed})) return rc;
    if (int rc = nfx_naf_pack(layers, d, n_hidden, widths, packed, stream)) return rc;  // (checks the layers)
    NafBwdPackArgs P{};
    for (int l = 0; l <= n_hidden; ++l) P.raw[l] = layers[l];
    P.lay = naf_bwd_layout(d, n_hidden, widths);
    P.d = d;
    P.nh = n_hidden;
    P.packed = packed;
    const int n = P.lay.total - P.lay.F.total;
    naf_bwd_pack_kernel<<<(n + 1023) / 1024, 256, 0, (hipStream_t)stream>>>(P);
    return check_launch("naf_bwd_pack_kernel");
}

extern "C" int nfx_naf_backward(const float* packed, const NfxNafLayer* layers, const float* x, const float* gz,
                                const float* gld, float* gx, const NfxNafLayerGrad* grads, float* workspace,
                                int64_t B, int d, int n_hidden, const int* widths, int activation, int flags,
                                float clamp_alpha, float clamp_log_scale, void* stream) {
    if (B < 0 || d <= 0 || n_hidden <= 0 || !widths)
        return set_error(NFX_EINVAL, "naf backward: bad shape B=%lld d=%d n_hidden=%d", (long long)B, d, n_hidden);
    if (const char* why = naf_bwd_shape_problem(d, n_hidden, widths))
        return set_error(NFX_EUNSUPPORTED, "naf backward: d=%d n_hidden=%d %s (%s)", d, n_hidden, kNafBwdFamily, why);
    if (!naf_activation(activation))
        return set_error(NFX_EUNSUPPORTED, "naf backward: activation=%d is not one of NFX_NAF_*", activation);
    if (!naf_flags_ok(n_hidden, widths, flags))
        return set_error(NFX_EINVAL,
                         "naf backward: flags=0x%x name a residual block between unequal widths or an unknown bit",
                         flags);
    naf_bwd_kernel_t k = pick_naf_bwd(naf_max_tiles(n_hidden, widths));
    if (!k) return set_error(NFX_EUNSUPPORTED, "naf backward: no kernel for these widths");
    if (B == 0) return NFX_OK;
    if (int rc = check_pointers("naf backward", {packed, layers, x, gz, gld, gx, grads, workspace})) return rc;
    if (int rc = check_no_alias("naf backward", x, gx)) return rc;
    if (int rc = check_no_alias("naf backward", gz, gx)) return rc;
    if (int rc = naf_bwd_check_layers("naf backward", layers, n_hidden, widths)) return rc;
    const bool ln = flags & NFX_NAF_LAYER_NORM;
    for (int l = 0; l < n_hidden; ++l)
        if ((layers[l].ln_weight != nullptr) != ln)
            return set_error(NFX_EINVAL, "naf backward: layer %d's LayerNorm vectors do not match the flags", l);

    const NafBwdLayout lay = naf_bwd_layout(d, n_hidden, widths);
    const int64_t ntiles = (B + 31) / 32;
    const int threads = naf_bwd_threads(ntiles), nw = threads / 64, grid = naf_bwd_grid(ntiles);
    const int len = lay.partial, nslots = grid * nw;
    NafBwdArgs A{};
    A.F.packed = packed;
    A.F.in = x;
    A.F.B = B;
    A.F.ntiles = ntiles;
    A.F.total4 = lay.total / 4;
    A.F.d = d;
    A.F.nh = n_hidden;
    A.F.act = activation;
    A.F.ln = ln ? 1 : 0;
    A.F.resmask = (flags >> 1) & ((1 << kNafMaxHidden) - 1);
    A.F.inverse = 1;
    A.F.tpw = nw;
    A.F.clamp_alpha = clamp_alpha;
    A.F.clamp_log_scale = clamp_log_scale;
    for (int l = 0; l <= n_hidden; ++l) {
        A.F.layer[l] = lay.F.layer[l];
        A.bl[l] = lay.layer[l];
    }
    A.gz = gz;
    A.gld = gld;
    A.gx = gx;
    A.ws = workspace;
    A.keep = workspace + (size_t)nslots * len + 2 * (size_t)len;
    A.partial = len;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = naf_bwd_lds_bytes(d, n_hidden, widths, nw);
    int rc = prepare_lds((const void*)k, lds);
    if (rc) return rc;
    k<<<grid, threads, lds, s>>>(A);
    rc = check_launch("naf_bwd_kernel");
    if (rc) return rc;
    double* tot = reinterpret_cast<double*>(workspace + (size_t)nslots * len);
    naf_bwd_reduce_kernel<<<(len + 63) / 64, 64 * kNafBwdReduceSegs, 0, s>>>(workspace, nslots, len, tot);
    rc = check_launch("naf_bwd_reduce_kernel");
    if (rc) return rc;
    NafBwdFinishArgs Fn{};
    Fn.tot = tot;
    Fn.lay = lay;
    Fn.d = d;
    Fn.nh = n_hidden;
    int n = 0;
    for (int l = 0; l <= n_hidden; ++l) {
        Fn.raw[l] = layers[l];
        Fn.grad[l] = grads[l];
        Fn.first[l] = n;
        const int rows = l == n_hidden ? 2 * d : widths[l], cols = l == 0 ? d : widths[l - 1];
        n += rows * cols + rows + (l < n_hidden && ln ? 2 * rows : 0);
    }
    Fn.first[n_hidden + 1] = n;
    naf_bwd_finish_kernel<<<(n + 255) / 256, 256, 0, s>>>(Fn);
    return check_launch("naf_bwd_finish_kernel");
}

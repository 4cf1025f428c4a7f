// ResidualFlow (src/flows/advanced/residual_flow.py): x = z + f(z) with f a three-layer MLP whose
// weights are spectrally normalised, in ONE launch per call and direction.
//
// The reference evaluates the inverse as a fixed-point loop of up to 100 MLP calls with a host sync
// after each, and every log-det from a d x d Jacobian built by d autograd passes. Here a wave owns
// a tile of 32 samples from load to store (the shared core, nfx_tile_mlp.h): the d -> H
// layer is short v_mfma_f32_32x32x2_f32 k-steps, the H x H layer runs on A fragments read from LDS,
// the H -> d layer is VALU dots across the two lane halves. New here:
//   * the full Jacobian, one forward-mode tangent per input dimension,
//       J[:, i] = W3 (g2 * (W2 (g1 * W1[:, i]))),
//     on the same k-steps as layer 2: an A fragment is read once and feeds the value chain and the
//     tangent chains of the pass (tangents in groups of res_tangent_group, so that the accumulator
//     tiles fit the register file; each group recomputes the value chain for g2);
//   * the Neumann traces with the d x d powers in registers;
//   * the fixed-point iteration inside the kernel, with a per-sample stopping rule (include/nfx.h);
//   * the spectral normalisation at pack time, on the device (residual_pack_kernel); the same
//     kernel writes the backward's image (nfx_residual_bwd.hip), which begins with this one.
// The activation is a launch-uniform switch taken once per accumulator tile, not a template
// parameter: 24 instantiations (3 padded widths x 8 dims) instead of 96.
#include <math.h>

#include "nfx_residual_bwd_kernel.h"

namespace nfx {

static residual_kernel_t pick_residual(int d, int HT) {
    return pick_of<1, 2, 4>(HT, [&](auto HT_) -> residual_kernel_t { return res_pick_ht<HT_()>(d); });
}

static bool res_family(int d, int H) { return d >= 1 && d <= kResMaxD && H >= 1 && H <= kResMaxH; }
static bool res_activation(int a) { return a >= NFX_RESIDUAL_RELU && a <= NFX_RESIDUAL_TANH; }

struct ResLayerRaw {
    const float *w, *b, *u, *v;
    float c;
    int rows, cols;
};
struct ResPackArgs {
    ResLayerRaw layer[3];
    int d, H;
    int total;  // the forward image, or the backward's (res_bwd_layout) that begins with it
    float* packed;
};

constexpr int kResPackThreads = 256;

// The factor the reference multiplies a layer's weight by: one power iteration from the stored
// (u, v), sums in float64 and every value the reference holds as an fp32 tensor rounded to fp32.
// Every thread of the block returns the same value. tmp: kResMaxH floats of shared memory twice.
__device__ float res_spectral_scale(const ResLayerRaw& l, float* tv, float* tu) {
    const int R = l.rows, C = l.cols;
    // v <- normalize(W^T u)
    for (int j = threadIdx.x; j < C; j += blockDim.x) {
        double a = 0.0;
        for (int i = 0; i < R; ++i) a += (double)l.w[i * C + j] * (double)l.u[i];
        tv[j] = (float)a;
    }
    __syncthreads();
    double n = 0.0;
    for (int j = 0; j < C; ++j) n += (double)tv[j] * (double)tv[j];
    const float nv = fmaxf((float)sqrt(n), 1e-12f);
    __syncthreads();
    for (int j = threadIdx.x; j < C; j += blockDim.x) tv[j] = tv[j] / nv;
    __syncthreads();
    // W v, then u <- normalize(W v) and sigma = u . (W v)
    for (int i = threadIdx.x; i < R; i += blockDim.x) {
        double a = 0.0;
        for (int j = 0; j < C; ++j) a += (double)l.w[i * C + j] * (double)tv[j];
        tu[i] = (float)a;
    }
    __syncthreads();
    n = 0.0;
    for (int i = 0; i < R; ++i) n += (double)tu[i] * (double)tu[i];
    const float nu = fmaxf((float)sqrt(n), 1e-12f);
    double sg = 0.0;
    for (int i = 0; i < R; ++i) sg += (double)(tu[i] / nu) * (double)tu[i];
    const float sigma = (float)sg;
    __syncthreads();
    return sigma > l.c ? (1.f / sigma) * l.c : 1.f;
}

// Every block works the three factors out for itself (at most 128 x 128 products per layer) and
// then writes its share of the image: one launch, nothing between kernels, nothing on the host.
__global__ __launch_bounds__(kResPackThreads) void residual_pack_kernel(ResPackArgs P) {
    __shared__ float tv[kResMaxH], tu[kResMaxH];
    float sc[3];
    for (int l = 0; l < 3; ++l) sc[l] = res_spectral_scale(P.layer[l], tv, tu);
    const int d = P.d, H = P.H;
    const int HT = hidden_tiles(H);
    const ResLayout L = res_layout(d, HT);
    const float *w1 = P.layer[0].w, *w2 = P.layer[1].w, *w3 = P.layer[2].w;
    for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < P.total; o += gridDim.x * blockDim.x) {
        float v = 0.f;
        if (o < L.b1) {  // w1: layer-1 A operand
            const RowCol e = a1_elem(o - L.w1, L.KS1);
            if (e.row < H && e.col < d) v = w1[e.row * d + e.col] * sc[0];
        } else if (o < L.w1c) {  // b1, b2
            const bool second = o >= L.b2;
            const int row = acc_vec_row(o - (second ? L.b2 : L.b1));
            if (row < H) v = second ? P.layer[1].b[row] : P.layer[0].b[row];
        } else if (o < L.w3) {  // w1c: column i of W1
            const VecRow e = acc_rows_elem(o - L.w1c, HT);
            if (e.row < H) v = w1[e.row * d + e.vec] * sc[0];
        } else if (o < L.b3) {  // w3: row j of W3
            const VecRow e = acc_rows_elem(o - L.w3, HT);
            if (e.row < H) v = w3[e.vec * H + e.row] * sc[2];
        } else if (o < L.w2) {  // b3
            const int j = o - L.b3;
            if (j < d) v = P.layer[2].b[j];
        } else if (o < L.total) {  // w2: A operand over (out row k, hidden input j)
            const RowCol e = a_image_elem(o - L.w2, HT);
            if (e.row < H && e.col < H) v = w2[e.row * H + e.col] * sc[1];
        } else if (o < L.total + HT * HT * 1024) {  // w2t (backward image): A operand of W2^T
            const RowCol e = a_image_elem(o - L.total, HT);
            if (e.row < H && e.col < H) v = w2[e.col * H + e.row] * sc[1];
        }
        P.packed[o] = v;
    }
}

int residual_pack_launch(const float* const (&w)[3], const float* const (&b)[3], const float* const (&u)[3],
                         const float* const (&v)[3], const float (&c)[3], int d, int H, float* packed, bool backward,
                         hipStream_t stream) {
    ResPackArgs P{};
    P.layer[0] = ResLayerRaw{w[0], b[0], u[0], v[0], c[0], H, d};
    P.layer[1] = ResLayerRaw{w[1], b[1], u[1], v[1], c[1], H, H};
    P.layer[2] = ResLayerRaw{w[2], b[2], u[2], v[2], c[2], d, H};
    P.d = d;
    P.H = H;
    const int HT = hidden_tiles(H);
    P.total = backward ? res_bwd_layout(d, HT).total : res_layout(d, HT).total;
    P.packed = packed;
    const int per_block = 4 * kResPackThreads;
    residual_pack_kernel<<<(P.total + per_block - 1) / per_block, kResPackThreads, 0, stream>>>(P);
    return check_launch("residual_pack_kernel");
}

}  // namespace nfx

using namespace nfx;

extern "C" size_t nfx_residual_packed_floats(int d, int H) {
    if (!res_family(d, H)) return 0;
    return (size_t)res_layout(d, hidden_tiles(H)).total;
}

extern "C" int nfx_residual_supported(int64_t B, int d, int H, int activation) {
    return B >= 1 && res_family(d, H) && res_activation(activation) ? 1 : 0;
}

extern "C" int nfx_residual_pack(const float* w1, const float* b1, const float* u1, const float* v1, float c1,
                                 const float* w2, const float* b2, const float* u2, const float* v2, float c2,
                                 const float* w3, const float* b3, const float* u3, const float* v3, float c3, int d,
                                 int H, float* packed, void* stream) {
    if (d <= 0 || H <= 0) return set_error(NFX_EINVAL, "residual_pack: bad shape d=%d H=%d", d, H);
    if (!res_family(d, H))
        return set_error(NFX_EUNSUPPORTED, "residual: d=%d H=%d outside the compiled family (d<=8, H<=128)", d, H);
    if (int rc = check_pointers("residual_pack", {w1, b1, u1, v1, w2, b2, u2, v2, w3, b3, u3, v3, packed})) return rc;
    return residual_pack_launch({w1, w2, w3}, {b1, b2, b3}, {u1, u2, u3}, {v1, v2, v3}, {c1, c2, c3}, d, H, packed, false,
                                (hipStream_t)stream);
}

extern "C" int nfx_residual_flow(const float* packed, const float* in, float* out, float* log_det, int64_t B, int d,
                                 int H, int activation, int direction, int neumann_terms, int max_iter, float tol,
                                 int accumulate, void* stream) {
    if (B < 0 || d <= 0 || H <= 0)
        return set_error(NFX_EINVAL, "residual: bad shape B=%lld d=%d H=%d", (long long)B, d, H);
    if (int rc = check_direction("residual", direction)) return rc;
    if (neumann_terms < 0 || max_iter < 0)
        return set_error(NFX_EINVAL, "residual: neumann_terms=%d and max_iter=%d must not be negative", neumann_terms,
                         max_iter);
    if (!res_family(d, H))
        return set_error(NFX_EUNSUPPORTED, "residual: d=%d H=%d outside the compiled family (d<=8, H<=128)", d, H);
    if (!res_activation(activation))
        return set_error(NFX_EUNSUPPORTED, "residual: activation=%d is not one of NFX_RESIDUAL_*", activation);
    const int HT = hidden_tiles(H);
    residual_kernel_t k = pick_residual(d, HT);
    if (!k) return set_error(NFX_EUNSUPPORTED, "residual: no kernel for d=%d H=%d", d, H);
    if (B == 0) return NFX_OK;
    if (int rc = check_io("residual", {packed, in, out, log_det}, in, out)) return rc;
    ResArgs A{};
    A.packed = packed;
    A.in = in;
    A.out = out;
    A.logdet = log_det;
    A.B = B;
    A.ntiles = (B + 31) / 32;
    A.accumulate = accumulate ? 1 : 0;
    A.act = activation;
    A.inverse = direction == NFX_INVERSE ? 1 : 0;
    A.nterms = neumann_terms;
    A.max_iter = max_iter;
    A.tol = tol;
    const size_t lds = (size_t)res_layout(d, HT).total * sizeof(float);
    const int threads = tile_owner_threads(A.ntiles), nw = threads / 64;
    return launch_resident((const void*)k, &A, threads, lds, (A.ntiles + nw - 1) / nw, (hipStream_t)stream,
                           "residual_flow_kernel");
}

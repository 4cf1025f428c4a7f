// PlanarFlow, RadialFlow (src/flows/advanced/planar_flow.py, radial_flow.py) and SylvesterFlow
// (sylvester_flow.py): the C-ABI of the stack kernel (nfx_lowrank_kernel.h) and the pack kernels.
//
// The reference runs one layer per call, its inverse as a Python loop of up to 50 steps with a
// host sync each, and the Sylvester log-det as one torch.det per row. These layers are used in
// stacks of 8 to 32, a handful of flops per element each, so here a whole stack of any mix of the
// three kinds at one dim is ONE launch, z in registers from load to store; a single layer is the
// same kernel with n_layers = 1.
//
// Each layer is one fixed-size record of the stack's device image. The pack kernels (one launch of
// one 64-thread workgroup per layer, sums in float64, each result rounded to fp32, nothing read
// back) write straight into the record they are given:
//   Planar     u = u_hat + (m - w.u_hat) w / (|w|^2 + 1e-8), m = -1 + log1p(exp(w.u_hat)); u.w
//   Radial     alpha = softplus(alpha_hat), beta = -alpha + softplus(beta_hat) (linear above 20)
//   Sylvester  Qm = H_K ... H_1 (H = I - 2 v v^T / (|v|^2 + 1e-8)), A = R Qm, Bm = Qm R^T, S = R R^T,
//              b; num_transforms padded to 8 with zeros. The layer is then z + Bm tanh(A z + b).
#include <math.h>

#include "nfx_lowrank_kernel.h"

namespace nfx {

static bool lr_family(int dim) { return dim >= 1 && dim <= kLrMaxDim; }
static bool lr_layers(int n) { return n >= 1 && n <= kLrMaxLayers; }

static lowrank_kernel_t pick_lowrank(int DP) { return DP <= 16 ? lowrank_pick_h1(DP) : DP == 32 ? lowrank_pick_h2(DP) : lowrank_pick_h3(DP); }

constexpr int kLrPackThreads = 64;

// Zero the record, then its header. Ends on a barrier: every thread may write values after it.
__device__ void lr_pack_begin(float* rec, int DP, int kind, int max_iter, float tol) {
    const int total = lr_record_floats(DP);
    for (int o = threadIdx.x; o < total; o += blockDim.x) rec[o] = 0.f;
    __syncthreads();
    if (threadIdx.x == 0) {
        rec[kLrKind] = __int_as_float(kind);
        rec[kLrIter] = __int_as_float(max_iter);
        rec[kLrTol] = tol;
    }
}

__device__ double lr_softplus(double x) { return x > 20.0 ? x : log1p(exp(x)); }

__global__ __launch_bounds__(kLrPackThreads) void lowrank_pack_planar_kernel(const float* w, const float* u_hat,
                                                                             const float* b, int dim, int DP,
                                                                             int max_iter, float tol, float* rec) {
    __shared__ float us[kLrMaxDim];
    lr_pack_begin(rec, DP, kLrPlanar, max_iter, tol);
    double wtu = 0.0, nrm = 0.0;
    for (int j = 0; j < dim; ++j) {
        wtu += (double)w[j] * (double)u_hat[j];
        nrm += (double)w[j] * (double)w[j];
    }
    const float wtu_f = (float)wtu, nrm_f = (float)nrm;
    const float m = (float)(-1.0 + log1p(exp((double)wtu_f)));
    const double coef = ((double)m - (double)wtu_f) / ((double)nrm_f + 1e-8);
    const int j = threadIdx.x;
    if (j < dim) {
        us[j] = (float)((double)u_hat[j] + coef * (double)w[j]);
        rec[kLrVec + j] = w[j];
        rec[kLrVec + DP + j] = us[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double utw = 0.0;
        for (int i = 0; i < dim; ++i) utw += (double)us[i] * (double)w[i];
        rec[kLrS0] = b[0];
        rec[kLrS1] = (float)utw;
    }
}

__global__ __launch_bounds__(kLrPackThreads) void lowrank_pack_radial_kernel(const float* z0, const float* alpha_hat,
                                                                             const float* beta_hat, int dim, int DP,
                                                                             int max_iter, float tol, float* rec) {
    lr_pack_begin(rec, DP, kLrRadial, max_iter, tol);
    const int j = threadIdx.x;
    if (j < dim) rec[kLrVec + j] = z0[j];
    if (threadIdx.x == 0) {
        const float alpha = (float)lr_softplus((double)alpha_hat[0]);
        const float sp = (float)lr_softplus((double)beta_hat[0]);
        rec[kLrS0] = alpha;
        rec[kLrS1] = (float)(-(double)alpha + (double)sp);
    }
}

// Thread c owns column c of Qm while the reflections are applied (H_k acts on columns
// independently), then row c of Bm and one entry of S.
__global__ __launch_bounds__(kLrPackThreads) void lowrank_pack_sylvester_kernel(const float* v, const float* R,
                                                                                const float* b, int dim, int K, int M,
                                                                                int DP, int max_iter, float tol,
                                                                                float* rec) {
    __shared__ double q[kLrMaxDim * kLrMaxDim];
    lr_pack_begin(rec, DP, kLrSylvester, max_iter, tol);
    const int c = threadIdx.x;
    if (c < dim) {
        for (int i = 0; i < dim; ++i) q[i * kLrMaxDim + c] = i == c ? 1.0 : 0.0;
        for (int k = 0; k < K; ++k) {
            const float* vk = v + (size_t)k * dim;
            double nsq = 0.0, dot = 0.0;
            for (int i = 0; i < dim; ++i) {
                nsq += (double)vk[i] * (double)vk[i];
                dot += (double)vk[i] * q[i * kLrMaxDim + c];
            }
            const double f = 2.0 * dot / (nsq + 1e-8);
            for (int i = 0; i < dim; ++i) q[i * kLrMaxDim + c] -= f * (double)vk[i];
        }
        for (int m = 0; m < M; ++m) {  // A = R Qm, column c
            double a = 0.0;
            for (int i = 0; i < dim; ++i) a += (double)R[m * dim + i] * q[i * kLrMaxDim + c];
            rec[kLrVec + m * DP + c] = (float)a;
        }
    }
    __syncthreads();
    if (c < dim) {
        for (int m = 0; m < M; ++m) {  // Bm = Qm R^T, row c, stored transposed
            double a = 0.0;
            for (int i = 0; i < dim; ++i) a += q[c * kLrMaxDim + i] * (double)R[m * dim + i];
            rec[kLrVec + kLrMaxTransforms * DP + m * DP + c] = (float)a;
        }
    }
    const int sa = c / kLrMaxTransforms, sb = c % kLrMaxTransforms;
    if (sa < M && sb < M) {
        double a = 0.0;
        for (int i = 0; i < dim; ++i) a += (double)R[sa * dim + i] * (double)R[sb * dim + i];
        rec[kLrS + sa * kLrMaxTransforms + sb] = (float)a;
    }
    if (c < M) rec[kLrBias + c] = b[c];
}

static int lr_check_pack(const char* what, int dim, int max_iter) {
    if (dim <= 0 || max_iter < 0) return set_error(NFX_EINVAL, "%s: bad dim=%d or max_iter=%d", what, dim, max_iter);
    if (!lr_family(dim) || max_iter > kLrMaxIter)
        return set_error(NFX_EUNSUPPORTED, "%s: dim=%d max_iter=%d outside the compiled family (dim<=64, max_iter<=1000)",
                         what, dim, max_iter);
    return NFX_OK;
}

}  // namespace nfx

using namespace nfx;

static_assert(kLrPackThreads == kLrMaxDim && kLrPackThreads == kLrMaxTransforms * kLrMaxTransforms,
              "a pack thread per component and per entry of S");

extern "C" int nfx_lowrank_supported(int64_t B, int dim, int n_layers) {
    return B >= 1 && lr_family(dim) && lr_layers(n_layers) ? 1 : 0;
}

extern "C" size_t nfx_lowrank_record_floats(int dim) {
    return lr_family(dim) ? (size_t)lr_record_floats(lr_padded(dim)) : 0;
}

extern "C" int nfx_lowrank_pack_planar(const float* w, const float* u_hat, const float* b, int dim, int max_iter,
                                       float tol, float* record, void* stream) {
    if (int rc = lr_check_pack("lowrank_pack_planar", dim, max_iter)) return rc;
    if (int rc = check_pointers("lowrank_pack_planar", {w, u_hat, b, record})) return rc;
    lowrank_pack_planar_kernel<<<1, kLrPackThreads, 0, (hipStream_t)stream>>>(w, u_hat, b, dim, lr_padded(dim),
                                                                              max_iter, tol, record);
    return check_launch("lowrank_pack_planar_kernel");
}

extern "C" int nfx_lowrank_pack_radial(const float* z0, const float* alpha_hat, const float* beta_hat, int dim,
                                       int max_iter, float tol, float* record, void* stream) {
    if (int rc = lr_check_pack("lowrank_pack_radial", dim, max_iter)) return rc;
    if (int rc = check_pointers("lowrank_pack_radial", {z0, alpha_hat, beta_hat, record})) return rc;
    lowrank_pack_radial_kernel<<<1, kLrPackThreads, 0, (hipStream_t)stream>>>(z0, alpha_hat, beta_hat, dim,
                                                                              lr_padded(dim), max_iter, tol, record);
    return check_launch("lowrank_pack_radial_kernel");
}

extern "C" int nfx_lowrank_pack_sylvester(const float* v, const float* R, const float* b, int dim,
                                          int num_householder, int num_transforms, int max_iter, float tol,
                                          float* record, void* stream) {
    if (num_householder < 0 || num_transforms <= 0)
        return set_error(NFX_EINVAL, "lowrank_pack_sylvester: bad num_householder=%d or num_transforms=%d",
                         num_householder, num_transforms);
    if (int rc = lr_check_pack("lowrank_pack_sylvester", dim, max_iter)) return rc;
    if (num_transforms > kLrMaxTransforms || num_householder > kLrMaxDim)
        return set_error(NFX_EUNSUPPORTED,
                         "lowrank_pack_sylvester: num_transforms=%d num_householder=%d outside the compiled family "
                         "(num_transforms<=8, num_householder<=64)",
                         num_transforms, num_householder);
    if (int rc = check_pointers("lowrank_pack_sylvester", {R, b, record})) return rc;
    if (num_householder > 0 && !v) return set_error(NFX_EINVAL, "lowrank_pack_sylvester: null pointer");
    lowrank_pack_sylvester_kernel<<<1, kLrPackThreads, 0, (hipStream_t)stream>>>(
        v, R, b, dim, num_householder, num_transforms, lr_padded(dim), max_iter, tol, record);
    return check_launch("lowrank_pack_sylvester_kernel");
}

extern "C" int nfx_lowrank_stack(const float* image, int n_layers, const float* x, float* out, float* log_det,
                                 int64_t B, int dim, int direction, int accumulate, void* stream) {
    if (B < 0 || dim <= 0 || n_layers <= 0)
        return set_error(NFX_EINVAL, "lowrank: bad shape B=%lld dim=%d n_layers=%d", (long long)B, dim, n_layers);
    if (int rc = check_direction("lowrank", direction)) return rc;
    if (!lr_family(dim) || !lr_layers(n_layers))
        return set_error(NFX_EUNSUPPORTED, "lowrank: dim=%d n_layers=%d outside the compiled family (dim<=64, n_layers<=256)",
                         dim, n_layers);
    lowrank_kernel_t k = pick_lowrank(lr_padded(dim));
    if (!k) return set_error(NFX_EUNSUPPORTED, "lowrank: no kernel for dim=%d", dim);
    if (B == 0) return NFX_OK;
    if (int rc = check_io("lowrank", {image, x, out, log_det}, x, out)) return rc;
    LowrankArgs A{};
    A.image = image;
    A.in = x;
    A.out = out;
    A.logdet = log_det;
    A.B = B;
    A.dim = dim;
    A.n_layers = n_layers;
    A.inverse = direction == NFX_INVERSE ? 1 : 0;
    A.accumulate = accumulate ? 1 : 0;
    // few rows: one wave per workgroup, so they spread over the CUs
    const int threads = B <= 64 * 1024 ? 64 : 256;
    const int64_t blocks = (B + threads - 1) / threads;
    if (blocks > 0x7fffffffLL) return set_error(NFX_EUNSUPPORTED, "lowrank: B=%lld too large", (long long)B);
    k<<<dim3((unsigned)blocks), dim3(threads), 0, (hipStream_t)stream>>>(A);
    return check_launch("lowrank_stack_kernel");
}

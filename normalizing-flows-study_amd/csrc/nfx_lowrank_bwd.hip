// Fused backward of the Planar / Radial / Sylvester stack: the C-ABI of lowrank_bwd_kernel
// (nfx_lowrank_bwd_kernel.h: the sweep and the per-workgroup gradient images), the fixed-order sum of
// the workgroups' images, and the record-to-parameter adjoint of the pack kernels (nfx_lowrank.hip).
//
// Workspace: [slots][n_layers * record] floats, one image per workgroup, then n_layers * record
// float64 totals. Its size depends on B only through the slot count, which is capped.
//
// nfx_lrbwd_param_grads: one 64-thread workgroup per call and layer, sums in float64, the adjoint of
//   Planar     u.w, then u = u_hat + (m - w.u_hat) w / (|w|^2 + 1e-8)
//   Radial     alpha = softplus(alpha_hat), beta = -alpha + softplus(beta_hat)
//   Sylvester  A = R Qm, Bm = Qm R^T, S = R R^T, and Qm = H_K ... H_1 down to every v_k: with
//              T = Qm_bar Qm^T the reflections are peeled from the left, each with the exact inverse
//              (I - c v v^T)^-1 = I - c / (c |v|^2 - 1) v v^T, so num_householder up to 64 costs
//              O(K dim^2).
#include <math.h>

#include "nfx_lowrank_bwd_kernel.h"

namespace nfx {

static lowrank_bwd_kernel_t pick_lowrank_bwd(int DP) {
    return DP <= 16 ? lowrank_bwd_pick_h1(DP) : DP == 32 ? lowrank_bwd_pick_h2(DP) : lowrank_bwd_pick_h3(DP);
}

static bool lr_bwd_family(int64_t B, int dim, int n_layers, int direction) {
    if (B < 1 || dim < 1 || dim > kLrMaxDim || n_layers < 1) return false;
    if (direction == NFX_FORWARD) return n_layers == 1;  // a forward stack would need every layer's input
    return direction == NFX_INVERSE && n_layers <= lr_bwd_max_layers(lr_padded(dim));
}

static int64_t lr_bwd_chunks(int64_t B) { return (B + kLrBwdRows - 1) / kLrBwdRows; }
static int lr_bwd_slots(int64_t B) {
    const int64_t n = lr_bwd_chunks(B);
    return (int)(n < kLrBwdMaxSlots ? n : kLrBwdMaxSlots);
}

constexpr int kLrReduceThreads = 256;
__global__ __launch_bounds__(kLrReduceThreads) void lowrank_bwd_reduce_kernel(const float* slots, int nslots, int len,
                                                                              double* totals) {
    const int e = blockIdx.x * kLrReduceThreads + threadIdx.x;
    if (e >= len) return;
    double s = 0.0;
    for (int w = 0; w < nslots; ++w) s += (double)slots[(size_t)w * len + e];
    totals[e] = s;
}

constexpr int kLrGradThreads = 64;
constexpr int kLrQStride = kLrMaxDim + 1;
constexpr size_t kLrGradLdsBytes =
    (2 * kLrMaxDim * kLrQStride + 2 * kLrMaxTransforms * kLrMaxDim + 2 * kLrMaxDim) * sizeof(double);

__device__ double lr_sigmoid(double x) { return x > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-x)); }

struct LowrankGradArgs {
    const double* G;  // the layer's record of totals
    const float *p0, *p1, *p2;
    float *g0, *g1, *g2;
    int kind, dim, DP, K, M;
};

__global__ __launch_bounds__(kLrGradThreads) void lowrank_param_grads_kernel(LowrankGradArgs P) {
    extern __shared__ double sh[];
    const int c = threadIdx.x, dim = P.dim, DP = P.DP;
    const double* G = P.G;
    const double* G0 = G + kLrVec;
    const double* G1 = G + kLrVec + kLrMaxTransforms * DP;
    if (P.kind == kLrPlanar) {
        const float *w = P.p0, *u_hat = P.p1;
        double s = 0.0, n = 0.0;
        for (int j = 0; j < dim; ++j) {
            s += (double)w[j] * (double)u_hat[j];
            n += (double)w[j] * (double)w[j];
        }
        const double m = -1.0 + log1p(exp(s));
        const double coef = (m - s) / (n + 1e-8);
        const double cbar = G[1];
        double coefbar = 0.0;  // sum_j u_bar_j w_j, u_bar the total cotangent of the constrained u
        for (int j = 0; j < dim; ++j) coefbar += (G1[j] + cbar * (double)w[j]) * (double)w[j];
        const double sbar = coefbar * (lr_sigmoid(s) - 1.0) / (n + 1e-8);
        const double nbar = -coefbar * coef / (n + 1e-8);
        if (c < dim) {
            const double wj = w[c], uhj = u_hat[c];
            const double ubar = G1[c] + cbar * wj;
            if (P.g1) P.g1[c] = (float)(ubar + sbar * wj);
            if (P.g0) P.g0[c] = (float)(G0[c] + cbar * (uhj + coef * wj) + coef * ubar + sbar * uhj + 2.0 * nbar * wj);
        }
        if (c == 0 && P.g2) P.g2[0] = (float)G[8];
        return;
    }
    if (P.kind == kLrRadial) {
        if (c < dim && P.g0) P.g0[c] = (float)(-(G1[c] + G0[c] - (double)P.p0[c] * G[8]));
        if (c == 0) {
            const double abar = G[1], bbar = G[2];
            if (P.g1) P.g1[0] = (float)((abar - bbar) * lr_sigmoid((double)P.p1[0]));
            if (P.g2) P.g2[0] = (float)(bbar * lr_sigmoid((double)P.p2[0]));
        }
        return;
    }
    // Sylvester
    const int K = P.K, M = P.M;
    const float *v = P.p0, *R = P.p1;
    double* q = sh;                                    // Qm [dim][dim], stride kLrQStride
    double* T = q + kLrMaxDim * kLrQStride;            // Qm_bar Qm^T, then peeled
    double* aq = T + kLrMaxDim * kLrQStride;           // A_bar Qm^T [M][dim]
    double* rq = aq + kLrMaxTransforms * kLrMaxDim;    // R Qm^T     [M][dim]
    double* mv = rq + kLrMaxTransforms * kLrMaxDim;    // [dim]
    if (c < dim) {
        for (int i = 0; i < dim; ++i) q[i * kLrQStride + c] = i == c ? 1.0 : 0.0;
        for (int k = 0; k < K; ++k) {
            const float* vk = v + (size_t)k * dim;
            double nsq = 0.0, dot = 0.0;
            for (int i = 0; i < dim; ++i) {
                nsq += (double)vk[i] * (double)vk[i];
                dot += (double)vk[i] * q[i * kLrQStride + c];
            }
            const double f = 2.0 * dot / (nsq + 1e-8);
            for (int i = 0; i < dim; ++i) q[i * kLrQStride + c] -= f * (double)vk[i];
        }
    }
    __syncthreads();
    if (c < dim) {
        for (int m = 0; m < M; ++m) {
            double a = 0.0, r = 0.0;
            for (int l = 0; l < dim; ++l) {
                a += G0[m * DP + l] * q[c * kLrQStride + l];
                r += (double)R[m * dim + l] * q[c * kLrQStride + l];
            }
            aq[m * kLrMaxDim + c] = a;
            rq[m * kLrMaxDim + c] = r;
        }
    }
    __syncthreads();
    if (c < dim) {
        if (P.g1) {
            for (int m = 0; m < M; ++m) {  // R_bar = A_bar Qm^T + Bm^T_bar Qm + (S_bar + S_bar^T) R
                double a = aq[m * kLrMaxDim + c];
                for (int l = 0; l < dim; ++l) a += G1[m * DP + l] * q[l * kLrQStride + c];
                for (int n = 0; n < M; ++n)
                    a += (G[kLrS + m * kLrMaxTransforms + n] + G[kLrS + n * kLrMaxTransforms + m]) * (double)R[n * dim + c];
                P.g1[m * dim + c] = (float)a;
            }
        }
        for (int i = 0; i < dim; ++i) {  // T = (R^T A_bar + Bm^T_bar^T R) Qm^T, column c
            double a = 0.0;
            for (int m = 0; m < M; ++m)
                a += (double)R[m * dim + i] * aq[m * kLrMaxDim + c] + G1[m * DP + i] * rq[m * kLrMaxDim + c];
            T[i * kLrQStride + c] = a;
        }
    }
    if (c < M && P.g2) P.g2[c] = (float)G[kLrBias + c];
    __syncthreads();
    for (int k = K - 1; k >= 0; --k) {
        const float* vk = v + (size_t)k * dim;
        double n = 0.0;
        for (int i = 0; i < dim; ++i) n += (double)vk[i] * (double)vk[i];
        const double cc = 2.0 / (n + 1e-8);
        const double gam = cc / (cc * n - 1.0);
        if (c < dim) {  // row c of M = T H_k^-1
            double dot = 0.0;
            for (int j = 0; j < dim; ++j) dot += T[c * kLrQStride + j] * (double)vk[j];
            for (int j = 0; j < dim; ++j) T[c * kLrQStride + j] -= gam * dot * (double)vk[j];
            mv[c] = dot * (1.0 - gam * n);
        }
        __syncthreads();
        if (c < dim) {  // column c: v_bar_k, then T = H_k M
            double d = 0.0, vmv = 0.0;
            for (int i = 0; i < dim; ++i) {
                d += (double)vk[i] * T[i * kLrQStride + c];
                vmv += (double)vk[i] * mv[i];
            }
            if (P.g0) P.g0[(size_t)k * dim + c] = (float)(cc * cc * vmv * (double)vk[c] - cc * (mv[c] + d));
            for (int i = 0; i < dim; ++i) T[i * kLrQStride + c] -= cc * (double)vk[i] * d;
        }
        __syncthreads();
    }
}

}  // namespace nfx

using namespace nfx;

extern "C" int nfx_lrbwd_supported(int64_t B, int dim, int n_layers, int direction) {
    return lr_bwd_family(B, dim, n_layers, direction) ? 1 : 0;
}

extern "C" size_t nfx_lrbwd_max_layers(int dim) {
    return dim >= 1 && dim <= kLrMaxDim ? (size_t)lr_bwd_max_layers(lr_padded(dim)) : 0;
}

extern "C" size_t nfx_lrbwd_chunk_rows(int dim) { return dim >= 1 && dim <= kLrMaxDim ? (size_t)kLrBwdRows : 0; }

extern "C" size_t nfx_lrbwd_slots(int64_t B, int dim, int n_layers) {
    return lr_bwd_family(B, dim, n_layers, NFX_INVERSE) ? (size_t)lr_bwd_slots(B) : 0;
}

extern "C" size_t nfx_lrbwd_workspace_floats(int64_t B, int dim, int n_layers) {
    const size_t slots = nfx_lrbwd_slots(B, dim, n_layers);
    const size_t len = (size_t)n_layers * lr_record_floats(lr_padded(dim));
    return slots ? slots * len + 2 * len : 0;
}

extern "C" int nfx_lrbwd_stack(const float* image, int n_layers, const float* point, const float* gv, const float* gld,
                               float* gx, float* workspace, int64_t B, int dim, int direction, void* stream) {
    if (B < 0 || dim <= 0 || n_layers <= 0)
        return set_error(NFX_EINVAL, "lowrank backward: bad shape B=%lld dim=%d n_layers=%d", (long long)B, dim, n_layers);
    if (int rc = check_direction("lowrank backward", direction)) return rc;
    if (!lr_bwd_family(B > 0 ? B : 1, dim, n_layers, direction))
        return set_error(NFX_EUNSUPPORTED,
                         "lowrank backward: dim=%d n_layers=%d direction=%d outside the compiled family (dim<=64; "
                         "NFX_FORWARD one layer; NFX_INVERSE a stack whose gradient image fits the LDS budget)",
                         dim, n_layers, direction);
    const int DP = lr_padded(dim);
    lowrank_bwd_kernel_t k = pick_lowrank_bwd(DP);
    if (!k) return set_error(NFX_EUNSUPPORTED, "lowrank backward: no kernel for dim=%d", dim);
    if (B == 0) return NFX_OK;
    if (int rc = check_pointers("lowrank backward", {image, point, gv, gld, gx, workspace})) return rc;
    if (int rc = check_no_alias("lowrank backward", point, gx)) return rc;
    if (int rc = check_no_alias("lowrank backward", gv, gx)) return rc;
    if ((uintptr_t)workspace % 8) return set_error(NFX_EINVAL, "lowrank backward: workspace not 8-byte aligned");
    const int slots = lr_bwd_slots(B);
    const int len = n_layers * lr_record_floats(DP);
    const size_t lds = lr_bwd_lds_bytes(DP, n_layers);
    if (int rc = prepare_lds((const void*)k, lds)) return rc;
    LowrankBwdArgs A{};
    A.B = B;
    A.n_chunks = lr_bwd_chunks(B);
    A.dim = dim;
    A.n_layers = n_layers;
    A.inverse = direction == NFX_INVERSE ? 1 : 0;
    k<<<dim3((unsigned)slots), dim3(kLrBwdRows), lds, (hipStream_t)stream>>>(image, point, gv, gld, gx, workspace, A);
    if (int rc = check_launch("lowrank_bwd_kernel")) return rc;
    double* totals = reinterpret_cast<double*>(workspace + (size_t)slots * len);
    lowrank_bwd_reduce_kernel<<<dim3((len + kLrReduceThreads - 1) / kLrReduceThreads), dim3(kLrReduceThreads), 0,
                                (hipStream_t)stream>>>(workspace, slots, len, totals);
    return check_launch("lowrank_bwd_reduce_kernel");
}

extern "C" int nfx_lrbwd_param_grads(const float* workspace, int64_t B, int dim, int n_layers, int layer, int kind,
                                     const float* p0, const float* p1, const float* p2, float* g0, float* g1, float* g2,
                                     int num_householder, int num_transforms, void* stream) {
    if (B < 1 || dim <= 0 || n_layers <= 0 || layer < 0 || layer >= n_layers || kind < kLrPlanar || kind > kLrSylvester)
        return set_error(NFX_EINVAL, "lowrank param grads: bad B=%lld dim=%d n_layers=%d layer=%d kind=%d", (long long)B,
                         dim, n_layers, layer, kind);
    if (dim > kLrMaxDim || n_layers > kLrMaxLayers)
        return set_error(NFX_EUNSUPPORTED, "lowrank param grads: dim=%d n_layers=%d outside the compiled family", dim,
                         n_layers);
    if (kind == kLrSylvester && (num_householder < 0 || num_householder > kLrMaxDim || num_transforms < 1 ||
                                 num_transforms > kLrMaxTransforms))
        return set_error(NFX_EUNSUPPORTED, "lowrank param grads: num_householder=%d num_transforms=%d outside the family",
                         num_householder, num_transforms);
    if (int rc = check_pointers("lowrank param grads", {workspace, p1, p2})) return rc;
    if (!p0 && !(kind == kLrSylvester && num_householder == 0))
        return set_error(NFX_EINVAL, "lowrank param grads: null pointer");
    const int DP = lr_padded(dim);
    const int len = n_layers * lr_record_floats(DP);
    LowrankGradArgs P{};
    P.G = reinterpret_cast<const double*>(workspace + (size_t)lr_bwd_slots(B) * len) + (size_t)layer * lr_record_floats(DP);
    P.p0 = p0, P.p1 = p1, P.p2 = p2;
    P.g0 = g0, P.g1 = g1, P.g2 = g2;
    P.kind = kind, P.dim = dim, P.DP = DP, P.K = num_householder, P.M = num_transforms;
    const size_t lds = kind == kLrSylvester ? kLrGradLdsBytes : 0;
    if (int rc = prepare_lds((const void*)lowrank_param_grads_kernel, lds)) return rc;
    lowrank_param_grads_kernel<<<1, kLrGradThreads, lds, (hipStream_t)stream>>>(P);
    return check_launch("lowrank_param_grads_kernel");
}

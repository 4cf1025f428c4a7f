// C-ABI plumbing of libnfx.so: version, thread-local error string, launch checks.
#include <stdarg.h>
#include <stdio.h>

#include "nfx_common.h"

namespace nfx {

static thread_local char g_err[512] = "";
static thread_local const char* g_last_kernel = "";  // (string literals of the launch sites)

int set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int check_launch(const char* what) {
    g_last_kernel = what;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_error(NFX_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return NFX_OK;
}

int num_cus() {
    static int cache[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (cache[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            n <= 0)
            n = 256;
        cache[dev] = n;
    }
    return cache[dev];
}

// Grid: enough resident workgroups to fill every CU (occupancy from the runtime), never more
// than there are groups of work.
int resident_grid(const void* kernel, int threads, size_t lds_bytes, int64_t work_groups) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds_bytes) != hipSuccess ||
        per_cu <= 0) {
        (void)hipGetLastError();  // do not leave the error sticky for the launch check that follows
        per_cu = 1;
    }
    int64_t g = (int64_t)num_cus() * per_cu;
    if (work_groups < g) g = work_groups;
    return (int)(g < 1 ? 1 : g);
}

int prepare_lds(const void* kernel, size_t bytes) {
    if (bytes > 65536) {
        if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) !=
            hipSuccess) {
            (void)hipGetLastError();  // do not leave the error sticky for the caller's next HIP call
            return set_error(NFX_ELAUNCH, "hipFuncSetAttribute(dynamic LDS %zu B) failed", bytes);
        }
    }
    return NFX_OK;
}

int tile_owner_threads(int64_t ntiles) { return ntiles >= (int64_t)8 * num_cus() ? 256 : 64; }

int launch_resident(const void* kernel, void* args, int threads, size_t lds_bytes, int64_t work_groups,
                    hipStream_t stream, const char* name) {
    int rc = prepare_lds(kernel, lds_bytes);
    if (rc) return rc;
    const int grid = resident_grid(kernel, threads, lds_bytes, work_groups);
    void* argv[1] = {args};
    (void)hipLaunchKernel(kernel, dim3(grid), dim3(threads), argv, lds_bytes, stream);  // (check_launch reads it)
    return check_launch(name);
}

int check_direction(const char* family, int direction) {
    if (direction != NFX_FORWARD && direction != NFX_INVERSE)
        return set_error(NFX_EINVAL, "%s: direction must be NFX_FORWARD or NFX_INVERSE", family);
    return NFX_OK;
}

int check_pointers(const char* family, std::initializer_list<const void*> required) {
    for (const void* p : required)
        if (!p) return set_error(NFX_EINVAL, "%s: null pointer", family);
    return NFX_OK;
}

int check_no_alias(const char* family, const void* in, const void* out) {
    if (in == out) return set_error(NFX_EINVAL, "%s: in and out must not alias", family);
    return NFX_OK;
}

int check_io(const char* family, std::initializer_list<const void*> required, const void* in, const void* out) {
    if (int rc = check_pointers(family, required)) return rc;
    return check_no_alias(family, in, out);
}

}  // namespace nfx

extern "C" int nfx_abi_version(void) { return NFX_ABI_VERSION; }
extern "C" const char* nfx_last_error(void) { return nfx::g_err; }
extern "C" const char* nfx_last_kernel(void) { return nfx::g_last_kernel; }

// Test hook: fill the whole LDS of every CU with the 32-bit pattern `bits` (one 160 KiB workgroup
// per CU, several rounds), so a kernel that read LDS it never wrote would see that pattern
// instead of whatever the previous kernel left behind. No effect on any later result.
__global__ __launch_bounds__(256) void nfx_fill_lds_kernel(uint32_t bits, int nwords) {
    extern __shared__ uint32_t fill[];
    for (int i = threadIdx.x; i < nwords; i += 256) fill[i] = bits;
    __syncthreads();
}

extern "C" int nfx_debug_fill_lds(uint32_t bits, void* stream) {
    const int bytes = 160 * 1024;
    int rc = nfx::prepare_lds((const void*)nfx_fill_lds_kernel, bytes);
    if (rc) return rc;
    nfx_fill_lds_kernel<<<8 * nfx::num_cus(), 256, bytes, (hipStream_t)stream>>>(bits, bytes / 4);
    return nfx::check_launch("nfx_fill_lds_kernel");
}

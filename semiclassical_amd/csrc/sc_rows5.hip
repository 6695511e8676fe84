// Five-sum rows (sc_rows5.h): the reduction over the bands and the limits that sc_hk_cross and
// sc_hk_opcorr share, and the launch helpers of the operator tile kernels (sc_optile.h).
#include <cstdio>
#include "sc_optile.h"

namespace {

// out[e] = sum over the bands of partials[band][e], e < total = 5 count: the bands in 16 contiguous slices, each added in order by
// one thread, then the slices in order
__global__ __launch_bounds__(256) void rows5_reduce_kernel(const double *partials, int64_t bands, int64_t total, double *out,
                                                           const long long *cursor) {
    __shared__ double red[16][16];
    const int sl = threadIdx.x >> 4, el = threadIdx.x & 15;
    const int64_t e = (int64_t)blockIdx.x * 16 + el;
    const int64_t per = (bands + 15) / 16, b0 = sl * per, b1 = min(b0 + per, bands);
    double s = 0.0;
    if (e < total)
        for (int64_t b = b0; b < b1; ++b) s += partials[b * total + e];
    red[sl][el] = s;
    __syncthreads();
    if (sl == 0 && e < total) {
        double t = 0.0;
        for (int g = 0; g < 16; ++g) t += red[g][el];
        if (cursor) out += total * *cursor;
        out[e] = t;
    }
}

}  // namespace

int64_t sc_rows5_bands(int64_t n, int64_t count) {
    if (n <= 0 || count <= 0) return 0;
    return (n + R5_TILE - 1) / R5_TILE;
}

int sc_rows5_limits(const char *who, const char *letter, const char *noun, int64_t n, int D, int count, const char *missing) {
    if (count < 1 || D < 1 || n < 0)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "%s: %s=%d, D=%d, n=%lld", who, letter, count, D, (long long)n);
    if (missing) return sc_fail(SC_ERR_BAD_ARGUMENT, "%s: %s", who, missing);
    if (D > 512) return sc_fail(SC_ERR_UNSUPPORTED, "%s: D=%d outside D <= 512", who, D);
    if (count > 65535) return sc_fail(SC_ERR_UNSUPPORTED, "%s: %s=%d %s outside %s <= 65535", who, letter, count, noun, letter);
    if ((n + R5_TILE - 1) / R5_TILE > 65535)
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: n=%lld trajectories outside n <= %d", who, (long long)n, R5_TILE * 65535);
    return SC_OK;
}

int sc_rows5_reduce(const char *who, const double *partials, int64_t bands, int count, double *out, const int64_t *cursor,
                    hipStream_t stream) {
    const int64_t total = (int64_t)5 * count;
    hipLaunchKernelGGL(rows5_reduce_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, stream, partials, bands, total, out,
                       (const long long *)cursor);
    return sc_check_launch(who);
}

// ---- operator tiles (sc_optile.h) ----
dim3 sc_optile_prepass_grid(int64_t n, int M) {
    const int64_t blocks = (n * M + 255) / 256;
    return dim3((unsigned)(blocks < 65535 ? blocks : 65535));
}

int sc_optile_rows(const char *who, const void *tile, void *args, unsigned columns, int64_t n, int M, const double *partials,
                   double *out, const int64_t *cursor, hipStream_t stream) {
    const int64_t bands = sc_rows5_bands(n, M);
    if (bands > 0) {
        (void)hipLaunchKernel(tile, dim3(columns, (unsigned)bands), dim3(256), &args, 0, stream);
        const int rc = sc_check_launch(who);
        if (rc != SC_OK) return rc;
    }
    char reduction[96];
    snprintf(reduction, sizeof reduction, "%s (reduction)", who);
    return sc_rows5_reduce(reduction, partials, bands, M, out, cursor, stream);
}

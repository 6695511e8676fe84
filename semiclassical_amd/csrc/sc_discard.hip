// Discarding trajectories whose monodromy matrix has left the symplectic condition.
//
// A per-trajectory mask kept[n] (one byte each, 1 = kept) is cleared by sc_discard_mark from the deviations sc_symplectic_deviation
// reports, and honoured by ONE reduction over the exported per-trajectory terms, sc_term_masked_sums: a discarded trajectory is a
// sample of value zero, N does not change.  No state kernel and no correlate kernel knows the mask.
//
//   discard_mark_kernel        elementwise: kept[i] &= max3(dev[i]) <= tol, discarded_at[i] = step where the bit fell, and the
//                              number of bits still set (an INTEGER atomic per wavefront: the order of the adds changes nothing)
//   term_masked_partial_kernel 64 workgroups of 256 threads.  Workgroup w walks the groups of four trajectories g = w (mod 64):
//                              every valid B divides 64, so everything it sees lies in block w mod B (sc_error_block).  Per group:
//                              four 16-byte loads of cq, four of kq, ONE 32-bit load of the four mask bytes.  Ten accumulators per
//                              thread (four sums, six second moments), wave_sum, the four wavefronts in order -> scratch[w][10]
//   term_masked_finish_kernel  one workgroup: slot sums and moments = rows 0 ... 63 in order, block b = rows b, b + B, ... in order
// One writer per output, no floating-point atomics, a summation order that depends on (n, B) alone: the same bits in every run.
// A term of a discarded trajectory is SELECTED away before it touches an accumulator (never multiplied by the mask): such
// trajectories carry inf / NaN terms.
//
// Why this shape and not the three existing passes (reduce, sc_term_moments, sc_term_blocks) with a mask each: it is a per-step
// launch on the path of every masked step, and one pass reads the 32 + 1 bytes per trajectory once instead of three times; the
// partition by w mod 64 makes the block sums a by-product of the partial rows instead of a second kernel shape.
#include "sc_common.h"

namespace {

constexpr int MASKED_WG = 64;          // workgroups of the partial kernel = rows of the scratch
constexpr int MASKED_COLS = 10;        // Re/Im sum cq, Re/Im sum kq, then the six moments of sc_hk_correlate_m
constexpr int MARK_MAX_WG = 32;        // the mark is a few bytes per trajectory: 8192 threads stride over the batch

__global__ __launch_bounds__(256) void discard_mark_kernel(const double *dev, int64_t n, double tol, int step, uint8_t *kept,
                                                           int32_t *discarded_at, unsigned long long *kept_count) {
    unsigned long long alive = 0;           // of this wavefront; complete in lane 0, which leaves the loop last
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        bool keep = kept[i] != 0;
        if (keep) {
            const double d0 = dev[3 * i], d1 = dev[3 * i + 1], d2 = dev[3 * i + 2];
            // !(max3 <= tol), written so that a NaN in any of the three clears the bit as +inf does
            if (!(d0 <= tol && d1 <= tol && d2 <= tol)) {
                keep = false;
                kept[i] = 0;
                discarded_at[i] = step;
            }
        }
        alive += (unsigned long long)__popcll(__ballot(keep));
    }
    if ((threadIdx.x & 63) == 0 && alive != 0) atomicAdd(kept_count, alive);
}

struct MaskedArgs {
    const cplx *cq, *kq;          // kq may be NULL: its sums are 0
    const uint8_t *kept;
    int64_t n;
    double *scratch;              // [MASKED_WG][MASKED_COLS]
};

__device__ __forceinline__ void add_masked(double (&acc)[MASKED_COLS], bool keep, cplx c, cplx k) {
    // selection: nothing of a discarded trajectory reaches the arithmetic
    const double cr = keep ? c.x : 0.0, ci = keep ? c.y : 0.0, kr = keep ? k.x : 0.0, ki = keep ? k.y : 0.0;
    acc[0] += cr; acc[1] += ci; acc[2] += kr; acc[3] += ki;
    acc[4] = fma(cr, cr, acc[4]); acc[5] = fma(ci, ci, acc[5]); acc[6] = fma(cr, ci, acc[6]);
    acc[7] = fma(kr, kr, acc[7]); acc[8] = fma(ki, ki, acc[8]); acc[9] = fma(kr, ki, acc[9]);
}

__global__ __launch_bounds__(256) void term_masked_partial_kernel(MaskedArgs A) {
    __shared__ double wsum[4][MASKED_COLS];
    const int w = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t groups = (A.n + 3) >> 2;
    const bool has_k = A.kq != nullptr;
    const cplx zero = c_make(0.0, 0.0);
    double acc[MASKED_COLS];
#pragma unroll
    for (int i = 0; i < MASKED_COLS; ++i) acc[i] = 0.0;
    for (int64_t g = w + (int64_t)MASKED_WG * tid; g < groups; g += (int64_t)MASKED_WG * 256) {
        const int64_t i0 = g << 2;
        if (A.n - i0 >= 4) {
            const uint32_t m = *(const uint32_t *)(A.kept + i0);      // kept is 4-byte aligned (checked by the entry point)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                add_masked(acc, ((m >> (8 * j)) & 0xffu) != 0, A.cq[i0 + j], has_k ? A.kq[i0 + j] : zero);
        } else {
            // the last group of the batch, partial: byte loads, nothing is read beyond n
            for (int64_t i = i0; i < A.n; ++i) add_masked(acc, A.kept[i] != 0, A.cq[i], has_k ? A.kq[i] : zero);
        }
    }
#pragma unroll
    for (int i = 0; i < MASKED_COLS; ++i) acc[i] = wave_sum(acc[i]);      // fixed order: deterministic
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < MASKED_COLS; ++i) wsum[wave][i] = acc[i];
    }
    __syncthreads();
    if (tid < MASKED_COLS) {
        double s = 0.0;
        for (int v = 0; v < 4; ++v) s += wsum[v][tid];
        A.scratch[(size_t)w * MASKED_COLS + tid] = s;
    }
}

// Thread t < 4 B owns out column j = t & 3 of block b = t >> 2: the rows b, b + B, ... of the scratch in order.  Thread t < 10
// owns a total: rows 0 ... 63 in order, columns 0 ... 3 to the slot, 4 ... 9 to the moments.
__global__ __launch_bounds__(256) void term_masked_finish_kernel(const double *scratch, int B, double *slot, double *moments,
                                                                 double *blocks) {
    const int tid = threadIdx.x;
    if (blocks && tid < 4 * B) {
        const int b = tid >> 2, j = tid & 3;
        double s = 0.0;
        for (int r = b; r < MASKED_WG; r += B) s += scratch[r * MASKED_COLS + j];
        blocks[tid] = s;
    }
    if (tid < MASKED_COLS && (tid < 4 || moments)) {
        double s = 0.0;
        for (int r = 0; r < MASKED_WG; ++r) s += scratch[r * MASKED_COLS + tid];
        if (tid < 4) slot[tid] = s;
        else moments[tid - 4] = s;
    }
}

}  // namespace

extern "C" int sc_discard_mark(const double *dev, int64_t n, double tol, int32_t step, uint8_t *kept, int32_t *discarded_at,
                               int64_t *kept_count, void *stream) {
    if (!dev || !kept || !discarded_at || !kept_count) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_discard_mark: null argument");
    if (!(tol > 0.0)) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_discard_mark: the tolerance has to be positive, got %g", tol);
    if (n < 0) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_discard_mark: n = %lld", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(kept_count, 0, sizeof(int64_t), s) != hipSuccess) return sc_check_launch("sc_discard_mark (counter)");
    if (n == 0) return SC_OK;
    const int64_t want = (n + 255) / 256;
    const int grid = (int)(want < MARK_MAX_WG ? want : MARK_MAX_WG);
    hipLaunchKernelGGL(discard_mark_kernel, dim3(grid), dim3(256), 0, s, dev, n, tol, (int)step, kept, discarded_at,
                       (unsigned long long *)kept_count);
    return sc_check_launch("sc_discard_mark");
}

extern "C" int64_t sc_term_masked_scratch_doubles(void) { return (int64_t)MASKED_WG * MASKED_COLS; }

extern "C" int sc_term_masked_sums(const double *cq, const double *kq, const uint8_t *kept, int64_t n, int32_t B, double *scratch,
                                   double *slot, double *moments, double *blocks, void *stream) {
    if (!cq || !kept || !scratch || !slot) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_term_masked_sums: null argument");
    if (B != 0 && !sc_error_blocks_valid(B))
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_term_masked_sums: the number of blocks has to be a power of two in 2 ... 64 (or 0), "
                       "got %d", (int)B);
    if ((B != 0) != (blocks != nullptr))
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_term_masked_sums: B = %d %s a blocks buffer", (int)B, B ? "needs" : "comes without");
    if (((uintptr_t)cq | (uintptr_t)kq) & 15 || ((uintptr_t)kept & 3))
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_term_masked_sums: cq / kq have to be 16-byte aligned, kept 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    MaskedArgs a{(const cplx *)cq, (const cplx *)kq, kept, n > 0 ? n : 0, scratch};
    hipLaunchKernelGGL(term_masked_partial_kernel, dim3(MASKED_WG), dim3(256), 0, s, a);
    if (const int rc = sc_check_launch("sc_term_masked_sums")) return rc;
    hipLaunchKernelGGL(term_masked_finish_kernel, dim3(1), dim3(256), 0, s, (const double *)scratch, (int)B, slot, moments, blocks);
    return sc_check_launch("sc_term_masked_sums (finish)");
}

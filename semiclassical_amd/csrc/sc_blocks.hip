// Block sums of the correlation terms: the raw material of Monte-Carlo error bars on anything LINEAR in C_auto(t) or k_ic(t),
// the rate k_ic(E) first of all (batch means).
//
// The trajectories of a batch are split into B fixed blocks, sc_error_block(i, B) = (i >> 2) & (B - 1) (sc_common.h): groups of
// four consecutive trajectories are dealt round robin to the blocks.  Per time step the kernels here leave
//     out[b][0..3] = Re sum cq_i, Im sum cq_i, Re sum kq_i, Im sum kq_i   over the trajectories i of block b
// (cq_i, kq_i as sc_hk_correlate defines them, reference propagators.py:784-911: weight included, dynamical phase not), so that
// sum_b out[b] is the slot row of the step.  Two sources:
//   term_blocks_kernel     the exported per-trajectory terms cq[n], kq[n] of sc_hk_correlate(_m), sc_wm_correlate or the caller
//   hk_run_blocks_kernel   the per-wavefront partials of the whole-loop kernels (sc_hk_run*): wavefront `slot` holds the
//                          trajectories with (i >> 2) mod slots == slot, and slots is either 4 ceil(n / 16) (no slot is visited
//                          twice: slot = i >> 2) or 4096 (a multiple of every B), hence block = slot mod B on both branches
// Every output has ONE writer and a summation order that depends on (n, B) alone: no floating-point atomics, the same bits in
// every run.
#include "sc_common.h"

namespace {

struct TermBlocksArgs {
    const cplx *cq, *kq;          // kq may be NULL: the k columns are 0
    int64_t n;
    int B;
    double *out;                  // [B][4], or [.][B][4] with a cursor
    const long long *cursor;      // optional device-resident row counter: read, never advanced here
};

// One workgroup per block b.  Thread t walks the groups g = b + B (t + 256 m) of four trajectories (64 contiguous bytes of cq,
// read as 16-byte loads; the last group of the batch may be partial), then wave_sum and a fixed-order sum over the four
// wavefronts through LDS, as hk_correlate_kernel ends.
__global__ __launch_bounds__(256) void term_blocks_kernel(TermBlocksArgs A) {
    __shared__ double wsum[4][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t groups = (A.n + 3) >> 2;
    const bool has_k = A.kq != nullptr;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t g = b + (int64_t)A.B * tid; g < groups; g += (int64_t)A.B * 256) {
        const int64_t i0 = g << 2;                 // sc_error_block(i0 + j, B) == b for j < 4
        const int cnt = A.n - i0 < 4 ? (int)(A.n - i0) : 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < cnt) {
                const cplx c = A.cq[i0 + j];
                acc[0] += c.x; acc[1] += c.y;
                if (has_k) {
                    const cplx k = A.kq[i0 + j];
                    acc[2] += k.x; acc[3] += k.y;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = wave_sum(acc[i]);      // fixed order: deterministic
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wsum[wave][i] = acc[i];
    }
    __syncthreads();
    if (tid < 4) {
        double s = 0.0;
        for (int w = 0; w < 4; ++w) s += wsum[w][tid];
        double *out = A.out + (A.cursor ? (size_t)*A.cursor * 4 * A.B : (size_t)0);
        out[(size_t)b * 4 + tid] = s;
    }
}

// One workgroup per time step k, as hk_run_reduce_kernel.  Thread t owns column j = t & 3 of block b = (t >> 2) & (B - 1) and
// is part p = t / (4 B) of the P = 256 / (4 B) threads that share this output: it adds the slots b + B (p + P m) in order, then
// the P parts are added in order through LDS by the one thread that writes out[k][b][j].
__global__ __launch_bounds__(256) void hk_run_blocks_kernel(const double *partials, int slots, int B, double *out) {
    __shared__ double part[256];
    const int k = blockIdx.x, tid = threadIdx.x, j = tid & 3, b = (tid >> 2) & (B - 1), nout = 4 * B;
    const int p = tid / nout, P = 256 / nout;
    double s = 0.0;
    for (int slot = b + B * p; slot < slots; slot += B * P) s += partials[((size_t)k * slots + slot) * 5 + j];
    part[tid] = s;
    __syncthreads();
    if (tid < nout) {
        double total = 0.0;
        for (int q = 0; q < P; ++q) total += part[tid + nout * q];
        out[(size_t)k * nout + tid] = total;          // tid = 4 b + j
    }
}

int launch_term_blocks(const char *who, const double *cq, const double *kq, int64_t n, int32_t B, double *out,
                       const int64_t *cursor, void *stream) {
    if (!cq || !out) return sc_fail(SC_ERR_BAD_ARGUMENT, "%s: null argument", who);
    if (!sc_error_blocks_valid(B))
        return sc_fail(SC_ERR_BAD_ARGUMENT, "%s: the number of blocks has to be a power of two in 2 ... 64, got %d", who, (int)B);
    TermBlocksArgs a{(const cplx *)cq, (const cplx *)kq, n > 0 ? n : 0, B, out, (const long long *)cursor};
    hipLaunchKernelGGL(term_blocks_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
    return sc_check_launch(who);
}

}  // namespace

extern "C" int sc_term_blocks(const double *cq, const double *kq, int64_t n, int32_t B, double *out, void *stream) {
    return launch_term_blocks("sc_term_blocks", cq, kq, n, B, out, nullptr, stream);
}

extern "C" int sc_term_blocks_at(const double *cq, const double *kq, int64_t n, int32_t B, double *out_base, const int64_t *cursor,
                                 void *stream) {
    if (!cursor) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_term_blocks_at: null cursor");
    return launch_term_blocks("sc_term_blocks_at", cq, kq, n, B, out_base, cursor, stream);
}

extern "C" int sc_hk_run_blocks(const double *partials, int64_t n, int32_t dim, int32_t nsteps, int32_t B, double *out,
                                void *stream) {
    if (!partials || !out) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_run_blocks: null argument");
    if (!sc_error_blocks_valid(B))
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_run_blocks: the number of blocks has to be a power of two in 2 ... 64, got %d",
                       (int)B);
    if (n <= 0 || nsteps <= 0) return SC_OK;
    const int slots = sc_hk_run_slots(n, dim);
    // block = slot mod B needs slot = i >> 2 (no slot visited twice) or a slot count the blocks divide
    if (!((int64_t)slots * 4 >= n || slots % B == 0))
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_hk_run_blocks: %d wavefront slots for %lld trajectories wrap around and are no "
                       "multiple of %d blocks: the slots do not map to blocks", slots, (long long)n, (int)B);
    hipLaunchKernelGGL(hk_run_blocks_kernel, dim3(nsteps), dim3(256), 0, (hipStream_t)stream, partials, slots, B, out);
    return sc_check_launch("sc_hk_run_blocks");
}

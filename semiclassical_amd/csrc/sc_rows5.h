// Five-sum rows: what sc_cross.hip and sc_opcorr.hip share once a thread holds x for its (trajectory,
// column) pairs.  Row c of the output: sum over the trajectories of  Re x, Im x, (Re x)^2, (Im x)^2, Re x Im x.
//
// The tile mapping: one workgroup of 256 threads owns 64 trajectories (blockIdx.y, a "band") x 64 columns (blockIdx.x); thread
// (ti, tj) = (tid >> 4, tid & 15) owns the 4 x 4 pairs of trajectories 4 ti + a and columns 4 tj + b (the mapping of
// pair_sum_kernel, phase A).  The d-loop is staged through LDS in chunks of R5_CHUNK.  The thread adds its 4 trajectories in
// registers (rows5_add, a = 0 .. 3 in order), the 16 threads of a column add through the reused staging LDS in index order
// (rows5_store_partials): one store of 5 doubles per column into partials[band][count][5].  sc_rows5_reduce adds the bands in 16
// contiguous slices, each in order, then the slices in order, into out or out[*cursor].  No atomics: the order of every sum is a
// function of (n, count) alone, the same bits in every call.
#pragma once
#include "sc_common.h"

#define R5_TILE 64                  // tile edge
#define R5_CHUNK 16                 // d chunk
// Row stride of a staged chunk: 16-byte aligned, so that a thread's four values are two 16-byte LDS reads.  With R5_TILE + 1 they
// are two-address 8-byte reads at half the LDS rate: 0.33 instead of 0.22 ms at n = 1e5, K = 64, D = 60.
#define R5_ROW (R5_TILE + 2)
#define R5_REDUCE_DOUBLES (16 * 5 * R5_TILE)       // [ti][sum][column] of the column reduction: the staging LDS is at least this

// four consecutive doubles of a staged row, from a 16-byte aligned address
__device__ __forceinline__ void load4(const double *p, double (&o)[4]) {
    const double2 lo = ((const double2 *)p)[0], hi = ((const double2 *)p)[1];
    o[0] = lo.x; o[1] = lo.y; o[2] = hi.x; o[3] = hi.y;
}

// one x into the five sums of its column
__device__ __forceinline__ void rows5_add(double (&sum)[5], cplx x) {
    sum[0] += x.x; sum[1] += x.y;
    sum[2] = fma(x.x, x.x, sum[2]); sum[3] = fma(x.y, x.y, sum[3]); sum[4] = fma(x.x, x.y, sum[4]);
}

// The tail of a tile kernel.  sum[b]: the thread's five sums of column 4 tj + b; lds: the staging buffers (free after the first
// barrier); tid, ti, tj: the thread and its place in the tile mapping; kv: the valid columns of the tile; k0: its first column.
__device__ __forceinline__ void rows5_store_partials(const double (&sum)[4][5], void *lds, int tid, int ti, int tj, int kv, int k0,
                                                     int count, double *partials) {
    __syncthreads();                                       // the staging buffers are free
    double (*red)[5][R5_TILE] = (double (*)[5][R5_TILE])lds;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int c = 0; c < 5; ++c) red[ti][c][4 * tj + b] = sum[b][c];
    __syncthreads();
    for (int e = tid; e < 5 * kv; e += 256) {
        const int t = e / 5, c = e - 5 * t;
        double s = 0.0;
        for (int g = 0; g < 16; ++g) s += red[g][c][t];
        partials[((size_t)blockIdx.y * count + k0) * 5 + e] = s;
    }
}

// ---- host side (sc_rows5.hip) ----
// bands of partials for n trajectories and `count` columns: what sc_hk_cross_rows and sc_hk_opcorr_rows return
int64_t sc_rows5_bands(int64_t n, int64_t count);
// The limits of the tile kernels, 0 = inside: count >= 1, D >= 1, n >= 0 (SC_ERR_BAD_ARGUMENT), then `missing` (a further refusal
// of an argument, or NULL), then D <= 512, count <= 65535, bands <= 65535 (SC_ERR_UNSUPPORTED).  letter, noun: "K", "targets".
int sc_rows5_limits(const char *who, const char *letter, const char *noun, int64_t n, int D, int count, const char *missing);
// out[e] (or out[total * *cursor + e]) = sum over the bands of partials[band][e], e < total = 5 count; `who` names the launch
int sc_rows5_reduce(const char *who, const double *partials, int64_t bands, int count, double *out, const int64_t *cursor,
                    hipStream_t stream);

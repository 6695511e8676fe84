// Operator tiles: what the tile and pre-pass kernels of sc_opcorr.hip, sc_opquad.hip,
// sc_thermal_opcorr.hip and sc_thermal_opquad.hip share.  Every operator, or column of an operator, is an affine form of a phase-space point,
//   z = kappa + u.Q + i w.P,
// and a workgroup forms it for a 64 x 64 tile of (trajectory, column) pairs.  The tile mapping is that of sc_rows5.h: thread
// (ti, tj) owns the trajectories 4 ti + a and the columns 4 tj + b.
#pragma once
#include "sc_rows5.h"

// the staged chunk of a tile kernel: Q, P of the trajectories and u, w of the columns (the kernels reuse it after their loops)
struct alignas(16) OpStage {
    typedef double chunk[R5_CHUNK][R5_ROW];
    chunk tq, tp, ku, kw;
};

// the LDS of a linear tile kernel: the staged chunk, and the column reduction of rows5_store_partials, which is the larger
union alignas(16) OpTileLds {
    OpStage S;
    double red[R5_REDUCE_DOUBLES];
};

// The band header: live[r] != 0 and cqs[r] = cq of trajectory i0 + r where it is below n and kept (`kept` may be NULL); else 0, and
// neither cq nor anything else of the trajectory is read later.  No barrier: the first one of the staged loop publishes both.
__device__ __forceinline__ void optile_band_header(int *live, double2 *cqs, int64_t n, int64_t i0, const uint8_t *kept,
                                                   const double *cq, int tid) {
    if (tid < R5_TILE) {
        const int64_t tr = i0 + tid;
        const bool in = tr < n && (!kept || kept[tr]);
        cqs[tid] = in ? ((const cplx *)cq)[tr] : c_make(0.0, 0.0);
        live[tid] = in;
    }
}

// fr += yu (x) xq, fi += yw (x) xp over the staged chunk: the thread's 4 x 4 pairs
__device__ __forceinline__ void optile_chunk_fma(const OpStage &S, int ti, int tj, double (&fr)[4][4], double (&fi)[4][4]) {
#pragma unroll 4
    for (int k = 0; k < R5_CHUNK; ++k) {
        double xq[4], xp[4], yu[4], yw[4];
        load4(&S.tq[k][4 * ti], xq); load4(&S.tp[k][4 * ti], xp);
        load4(&S.ku[k][4 * tj], yu); load4(&S.kw[k][4 * tj], yw);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                fr[a][b] = fma(yu[b], xq[a], fr[a][b]);
                fi[a][b] = fma(yw[b], xp[a], fi[a][b]);
            }
    }
}

// fr[a][b] += u_col.Q_i, fi[a][b] += w_col.P_i of the thread's 4 x 4 pairs over D in staged chunks; the caller zeroes fr, fi.
// qp [n][2 D]: the rows i0 + r with live[r] != 0 are read, the others staged as zeros; u, w [.][D]: the columns k0 ... k0 + kv - 1.
// Column: int where the columns are at most 65 535 operators, int64_t where they are the columns of operators (sc_opquad.hip) --
// with a 64-bit k0 in all of them the staging loop of the linear kernels keeps four 64-bit pointers more in flight.
template <typename Column>
__device__ __forceinline__ void optile_staged_loop(OpStage &S, const int *live, const double *qp, int D, const double *u,
                                                   const double *w, int64_t i0, Column k0, int kv, int tid, int ti, int tj,
                                                   double (&fr)[4][4], double (&fi)[4][4]) {
    for (int d0 = 0; d0 < D; d0 += R5_CHUNK) {
        __syncthreads();                                   // live[] is written; the last readers of the buffers are done
        for (int e = tid; e < R5_CHUNK * R5_TILE; e += 256) {
            const int r = e / R5_CHUNK, k = e - r * R5_CHUNK, d = d0 + k;      // row r of the tile, column k of the chunk
            double q = 0.0, p = 0.0;
            if (d < D && live[r]) {
                const double *row = qp + (i0 + r) * 2 * D;
                q = row[d]; p = row[D + d];
            }
            S.tq[k][r] = q; S.tp[k][r] = p;
            double uv = 0.0, wv = 0.0;
            if (d < D && r < kv) {
                const size_t at = (size_t)(k0 + r) * D + d;
                uv = u[at]; wv = w[at];
            }
            S.ku[k][r] = uv; S.kw[k][r] = wv;
        }
        __syncthreads();
        optile_chunk_fma(S, ti, tj, fr, fi);
    }
}

// The same over the d'' thermal modes of an ensemble with per-trajectory centres: fr[a][b] += ut_col.Qc_i(t),
// fi[a][b] += wt_col.Pc_i(t) with the centres rotated WHILE STAGING,
//   Qc(t) = Qc cos wt + Pc / w sin wt,   Pc(t) = Pc cos wt - w Qc sin wt.
// A staging thread keeps one mode index k through a chunk (256 is a multiple of R5_CHUNK): cos, sin and 1 / w of the chunk's 16 modes
// are formed once per chunk and workgroup into the 48-double table `rot`.  centres [n][2 dm] at t = 0: the rows i0 + r with
// live[r] != 0 are read; ut, wt [.][dm]: the columns k0 ... k0 + kv - 1.  The table of chunk c + 1 is written after the second barrier
// of chunk c, behind which no staging thread of chunk c reads it any more, and before the first barrier of chunk c + 1; that first
// barrier also ends the reads of the buffers by whoever ran before the loop.
typedef double OpRotTable[3][R5_CHUNK];                    // cos w t, sin w t, 1 / w of the chunk's modes
template <typename Column>
__device__ __forceinline__ void optile_rotated_loop(OpStage &S, OpRotTable &rot, const int *live, const double *omega, double time,
                                                    const double *centres, int dm, const double *ut, const double *wt, int64_t i0,
                                                    Column k0, int kv, int tid, int ti, int tj, double (&fr)[4][4],
                                                    double (&fi)[4][4]) {
    for (int m0 = 0; m0 < dm; m0 += R5_CHUNK) {
        if (tid < R5_CHUNK) {
            double c = 1.0, s = 0.0, iw = 0.0;
            if (m0 + tid < dm) {
                const double om = omega[m0 + tid];
                sincos(om * time, &s, &c);
                iw = 1.0 / om;
            }
            rot[0][tid] = c; rot[1][tid] = s; rot[2][tid] = iw;
        }
        __syncthreads();
        const int k = tid & (R5_CHUNK - 1), mode = m0 + k; // the thread's mode through the chunk
        const double c = rot[0][k], s = rot[1][k], iw = rot[2][k];
        const double om = mode < dm ? omega[mode] : 0.0;
        for (int e = tid; e < R5_CHUNK * R5_TILE; e += 256) {
            const int r = e / R5_CHUNK;
            double qt = 0.0, pt = 0.0;
            if (mode < dm && live[r]) {
                const double *row = centres + (i0 + r) * 2 * dm;
                const double qc = row[mode], pc = row[dm + mode];
                qt = fma(pc * iw, s, qc * c);
                pt = fma(-om * qc, s, pc * c);
            }
            S.tq[k][r] = qt; S.tp[k][r] = pt;
            double u = 0.0, w = 0.0;
            if (mode < dm && r < kv) {
                const size_t at = (size_t)(k0 + r) * dm + mode;
                u = ut[at]; w = wt[at];
            }
            S.ku[k][r] = u; S.kw[k][r] = w;
        }
        __syncthreads();
        optile_chunk_fma(S, ti, tj, fr, fi);
    }
}

// The finish of a linear tile kernel: x_ia = (kappa_a + f_ia) g_ia cq_i, x = 0 by selection for a column beyond kv or a row that is
// not live (its g is not read); the thread's four trajectories are added per operator in registers, then the tail of sc_rows5.h.
// kap [M] complex, g [n][M] complex, lds: the staging buffers.
__device__ __forceinline__ void optile_finish_linear(const double (&fr)[4][4], const double (&fi)[4][4], const int *live,
                                                     const double2 *cqs, const double *kap, const double *g, int64_t i0, int k0,
                                                     int kv, int M, void *lds, int tid, int ti, int tj, double *partials) {
    double sum[4][5];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
        for (int c = 0; c < 5; ++c) sum[b][c] = 0.0;
        const int op = 4 * tj + b;
        const cplx ka = op < kv ? ((const cplx *)kap)[k0 + op] : c_make(0.0, 0.0);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int r = 4 * ti + a;
            cplx x = c_make(0.0, 0.0);
            if (op < kv && live[r]) {
                // Im g is read before Re g.  hipcc orders the two products of Im (f g) by where their operands are read and fuses
                // the first, rounding the other: with g read as one cplx inside this function it rounds f.x g.y, where
                // opcorr_tile_kernel and thermal_opcorr_tile_kernel with the same text in their own bodies rounded f.y g.x -- the
                // bits of tests/golden/rows5_parent_bits.npz and optile_parent_bits.npz.  The two reads stay one 16-byte load.
                const double *gp = g + 2 * ((size_t)(i0 + r) * M + k0 + op);
                const double gy = gp[1], gx = gp[0];
                const cplx f = c_make(ka.x + fr[a][b], ka.y + fi[a][b]);
                x = c_mul(c_mul(f, c_make(gx, gy)), cqs[r]);
            }
            rows5_add(sum[b], x);
        }
    }
    rows5_store_partials(sum, lds, tid, ti, tj, kv, k0, M, partials);
}

// re += u.z[:len], im += w.z[len:] of one (point, column) pair of a pre-pass kernel; the caller zeroes re, im
__device__ __forceinline__ void optile_affine_dot(const double *u, const double *w, const double *z, int len, double &re,
                                                  double &im) {
    for (int d = 0; d < len; ++d) {
        re = fma(u[d], z[d], re);
        im = fma(w[d], z[len + d], im);
    }
}

// ---- host side (sc_rows5.hip) ----
// the grid of a pre-pass kernel of 256 threads: one (trajectory, operator) pair per thread, a grid stride beyond 65 535 workgroups
dim3 sc_optile_prepass_grid(int64_t n, int M);
// The five-sum rows of a tile kernel: `tile` (a __global__ function of one argument, the struct at `args`) on a grid of `columns`
// x bands workgroups where there is a band, then sc_rows5_reduce of `partials` into out or out[*cursor].  `who` names the launch
// in an error, "`who` (reduction)" the reduction.
int sc_optile_rows(const char *who, const void *tile, void *args, unsigned columns, int64_t n, int M, const double *partials,
                   double *out, const int64_t *cursor, hipStream_t stream);
// the limits of the quadratic tile kernels (sc_opquad.hip): 0 <= R <= 512 and M (1 + R) < 2^24, after those of sc_rows5_limits
int sc_opquad_limits(const char *who, int64_t n, int D, int M, int R);
// 1 <= d'' <= D of the thermal tile kernels (sc_thermal_opcorr.hip)
int sc_thermal_modes_limit(const char *who, int D, int dm);

// The exponent of the overlap <q_i, p_i, Gamma_t | q_k, p_k, Gamma_0> for a 64 x 64 tile of (trajectory, coherent state) pairs
// (DESIGN.md section 4.13): the staging and the d-loop that cross_tile_kernel (sc_cross.hip) and ta_terms_kernel
// (sc_timeavg.hip) share.  The tile mapping is that of sc_rows5.h: thread (ti, tj) owns the trajectories 4 ti + a and the
// columns 4 tj + b.
#pragma once
#include "sc_rows5.h"

// the LDS of a tile kernel: the d-chunk of both operand sets (sc_cross.hip reuses it for the column reduction)
struct alignas(16) CrossStage {
    typedef double chunk[R5_CHUNK][R5_ROW];
    chunk ta, tb, tq, tc;      // trajectories: La q, Lb p, q, C p
    chunk ka, kb, kq, kg;      // targets: La q_k, Lb p_k, q_k, C p_k - p_k
};

// re[a][b] = |La dq|^2 + |Lb dp|^2 and im[a][b] = sum_d dq_d ((C p_k)_d - (C p_i)_d - p_k,d) of the thread's 4 x 4 pairs: the
// exponent is E = -re / 2 + i im / hbar.  live[r] != 0: row r of the tile is a trajectory whose state is read (every other row is
// staged as zeros); the caller has written live[] and has NOT yet passed a barrier: the first one of the loop publishes it.
// DIAG: the widths are diagonal and q, p are scaled by La, Lb, Cm [D] while they are staged; else the rows [La q | Lb p | q | C p]
// come from `operands` [n][4 D] (cross_operands_kernel).  targets [K][5 D]; kv: the valid columns of the tile from k0 on.
template <bool DIAG>
__device__ __forceinline__ void cross_tile_exponents(CrossStage &S, const int *live, const sc_state &st, const double *La,
                                                     const double *Lb, const double *Cm, const double *operands,
                                                     const double *targets, int64_t i0, int k0, int kv, int tid, int ti, int tj,
                                                     double (&re)[4][4], double (&im)[4][4]) {
    const int D = st.dim;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) { re[a][b] = 0.0; im[a][b] = 0.0; }
    for (int d0 = 0; d0 < D; d0 += R5_CHUNK) {
        __syncthreads();                                   // live[] is written; the last readers of the chunk before are done
        for (int e = tid; e < R5_CHUNK * R5_TILE; e += 256) {
            const int r = e / R5_CHUNK, k = e - r * R5_CHUNK, d = d0 + k;      // row r of the tile, column k of the chunk
            double a = 0.0, b = 0.0, q = 0.0, c = 0.0;
            if (d < D && live[r]) {
                if (DIAG) {
                    const double *qp = st.qp + (i0 + r) * 2 * D;
                    const double p = qp[D + d];
                    q = qp[d];
                    a = La[d] * q; b = Lb[d] * p; c = Cm[d] * p;
                } else {
                    const double *row = operands + (i0 + r) * 4 * D;
                    a = row[d]; b = row[D + d]; q = row[2 * D + d]; c = row[3 * D + d];
                }
            }
            S.ta[k][r] = a; S.tb[k][r] = b; S.tq[k][r] = q; S.tc[k][r] = c;
            a = 0.0; b = 0.0; q = 0.0; c = 0.0;
            if (d < D && r < kv) {
                const double *row = targets + (size_t)(k0 + r) * 5 * D;
                a = row[d]; b = row[D + d]; q = row[2 * D + d]; c = row[3 * D + d] - row[4 * D + d];
            }
            S.ka[k][r] = a; S.kb[k][r] = b; S.kq[k][r] = q; S.kg[k][r] = c;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < R5_CHUNK; ++k) {
            double xa[4], xb[4], xq[4], xc[4], ya[4], yb[4], yq[4], yg[4];
            load4(&S.ta[k][4 * ti], xa); load4(&S.tb[k][4 * ti], xb); load4(&S.tq[k][4 * ti], xq); load4(&S.tc[k][4 * ti], xc);
            load4(&S.ka[k][4 * tj], ya); load4(&S.kb[k][4 * tj], yb); load4(&S.kq[k][4 * tj], yq); load4(&S.kg[k][4 * tj], yg);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const double da = ya[b] - xa[a], db = yb[b] - xb[a], dq = yq[b] - xq[a];
                    re[a][b] = fma(da, da, re[a][b]);
                    re[a][b] = fma(db, db, re[a][b]);
                    im[a][b] = fma(dq, yg[b] - xc[a], im[a][b]);
                }
        }
    }
}

// conj(fac exp(E)) of one pair from its sums
__device__ __forceinline__ cplx cross_tile_overlap_conj(double re, double im, double fac) {
    return c_scale(c_exp(c_make(-0.5 * re, -im * (1.0 / SC_HBAR))), fac);
}

// dense widths: the rows [La q_i | Lb p_i | q_i | C p_i] of every trajectory into operands [n][4 D] (sc_cross.hip); La, Lb [D][D]
// symmetric, Ct the transpose of C.  `who` names the launch in an error.
int sc_cross_operands(const char *who, const sc_state *st, const double *La, const double *Lb, const double *Ct, double *operands,
                      hipStream_t stream);

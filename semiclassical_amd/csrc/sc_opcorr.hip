// Operator correlation functions <phi_0| A_a e^(-iHt) B_a |phi_0> of the Herman-Kluk wavepacket for M pairs of LINEAR operators
// A_a = cA_a + mA_a.x, B_a = cB_a + mB_a.x (not in the reference) -- the O(n M D) kernels behind
// HermanKlukPropagator.operator_correlation() and run(operators=...).  Every trajectory's C_auto term cq_i (what sc_hk_correlate
// exports, the Monte-Carlo weight inside) is multiplied by a bra-side factor at the current (Q_i, P_i) and a ket-side factor at the
// initial (q_i, p_i), the way the reference's ic_correlation (semiclassical/propagators.py:845-911) multiplies it by nacQ and nacq.
// For a linear operator both are closed-form Gaussian matrix elements, which the host folds into one affine form per operator:
//
//   f_ia = bra_k_a + bra_u_a.Q_i + i bra_w_a.P_i          (the tile kernel, every step)
//   g_ia = ket_k_a + ket_u_a.q_i + i ket_w_a.p_i          (affine_kernel, once per ensemble and set of operators)
//   x_ia = f_ia g_ia cq_i
//   row a of the output: the five sums of x_ia over i (sc_rows5.h).
//
// opcorr_tile_kernel: the tile mapping, the column reduction and the reduction over the bands of sc_rows5.h, the columns being the
//   operators.  Per pair and d two FMAs; then one complex product chain -- no exponential.  With M <= 64 there is one tile column:
//   qp is read from HBM exactly once per call.
// Discarded trajectories (`kept`) and the rows beyond n are staged as zero operands, and their cq and g are never loaded (x = 0 by
// selection, not by a product): a non-finite value of a discarded trajectory cannot reach a sum.
#include "sc_rows5.h"

namespace {


constexpr int STAGE_DOUBLES = 4 * R5_CHUNK * R5_ROW;       // the d-chunk of Q, P (trajectories) and u, w (operators)
constexpr int LDS_DOUBLES = STAGE_DOUBLES > R5_REDUCE_DOUBLES ? STAGE_DOUBLES : R5_REDUCE_DOUBLES;   // reused by the reduction

struct OpcorrArgs {
    const double *qp;               // [n][2 D]
    int64_t n;
    int D, M;
    const double *cq;               // [n] complex
    const double *u, *w;            // [M][D]
    const double *kap;              // [M] complex
    const double *g;                // [n][M] complex
    const uint8_t *kept;            // may be NULL
    double *partials;               // [bands][M][5]
};

__global__ __launch_bounds__(256) void opcorr_tile_kernel(OpcorrArgs A) {
    __shared__ alignas(16) double lds[LDS_DOUBLES];
    __shared__ double2 cqs[R5_TILE];// cq_i of the band's trajectories (0: beyond n, or discarded)
    __shared__ int live[R5_TILE];
    typedef double row[R5_ROW];
    row *tq = (row *)lds, *tp = tq + R5_CHUNK, *ku = tp + R5_CHUNK, *kw = ku + R5_CHUNK;
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int D = A.D, M = A.M;
    const int64_t i0 = (int64_t)blockIdx.y * R5_TILE;
    const int k0 = blockIdx.x * R5_TILE;
    const int iv = (int)min((int64_t)R5_TILE, A.n - i0), kv = min(R5_TILE, M - k0);      // valid rows / operators of the tile
    if (tid < R5_TILE) {
        const int64_t tr = i0 + tid;
        const bool in = tid < iv && (!A.kept || A.kept[tr]);
        cqs[tid] = in ? ((const cplx *)A.cq)[tr] : c_make(0.0, 0.0);
        live[tid] = in;
    }
    double fr[4][4], fi[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) { fr[a][b] = 0.0; fi[a][b] = 0.0; }
    for (int d0 = 0; d0 < D; d0 += R5_CHUNK) {
        __syncthreads();                                   // live[] is written; the last readers of the chunk before are done
        for (int e = tid; e < R5_CHUNK * R5_TILE; e += 256) {
            const int r = e / R5_CHUNK, k = e - r * R5_CHUNK, d = d0 + k;      // row r of the tile, column k of the chunk
            double q = 0.0, p = 0.0;
            if (d < D && live[r]) {
                const double *row = A.qp + (i0 + r) * 2 * D;
                q = row[d]; p = row[D + d];
            }
            tq[k][r] = q; tp[k][r] = p;
            double u = 0.0, w = 0.0;
            if (d < D && r < kv) {
                const size_t at = (size_t)(k0 + r) * D + d;
                u = A.u[at]; w = A.w[at];
            }
            ku[k][r] = u; kw[k][r] = w;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < R5_CHUNK; ++k) {
            double xq[4], xp[4], yu[4], yw[4];
            load4(&tq[k][4 * ti], xq); load4(&tp[k][4 * ti], xp);
            load4(&ku[k][4 * tj], yu); load4(&kw[k][4 * tj], yw);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    fr[a][b] = fma(yu[b], xq[a], fr[a][b]);
                    fi[a][b] = fma(yw[b], xp[a], fi[a][b]);
                }
        }
    }
    // x_ia = f_ia g_ia cq_i; the thread's four trajectories are added per operator in registers
    double sum[4][5];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
        for (int c = 0; c < 5; ++c) sum[b][c] = 0.0;
        const int op = 4 * tj + b;
        const cplx kap = op < kv ? ((const cplx *)A.kap)[k0 + op] : c_make(0.0, 0.0);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int r = 4 * ti + a;
            cplx x = c_make(0.0, 0.0);
            if (op < kv && live[r]) {
                const cplx g = ((const cplx *)A.g)[(size_t)(i0 + r) * M + k0 + op];
                const cplx f = c_make(kap.x + fr[a][b], kap.y + fi[a][b]);
                x = c_mul(c_mul(f, g), cqs[r]);
            }
            rows5_add(sum[b], x);
        }
    }
    rows5_store_partials(sum, lds, tid, ti, tj, kv, k0, M, A.partials);
}

// out[i][a] = k_a + u_a.z_i[:D] + i w_a.z_i[D:], one (trajectory, operator) pair per thread, the operator index fastest
__global__ __launch_bounds__(256) void opcorr_affine_kernel(const double *z, int64_t n, int D, const double *u, const double *w,
                                                            const double *kap, int M, double *out) {
    const int64_t total = n * M;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / M;
        const int a = (int)(e - i * M);
        const double *row = z + i * 2 * D, *ua = u + (size_t)a * D, *wa = w + (size_t)a * D;
        double re = 0.0, im = 0.0;
        for (int d = 0; d < D; ++d) {
            re = fma(ua[d], row[d], re);
            im = fma(wa[d], row[D + d], im);
        }
        ((cplx *)out)[e] = c_make(kap[2 * a] + re, kap[2 * a + 1] + im);
    }
}

}  // namespace

extern "C" int64_t sc_hk_opcorr_rows(int64_t n, int64_t M) { return sc_rows5_bands(n, M); }

extern "C" int sc_hk_opcorr_initial(const double *zi, int64_t n, int32_t D, const double *ket_u, const double *ket_w,
                                    const double *ket_k, int32_t M, double *g, void *stream) {
    if (!zi || !ket_u || !ket_w || !ket_k || !g) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opcorr_initial: null argument");
    const int rc = sc_rows5_limits("sc_hk_opcorr_initial", "M", "operators", n, D, M, nullptr);
    if (rc != SC_OK) return rc;
    if (n == 0) return SC_OK;
    const int64_t blocks = (n * M + 255) / 256;
    hipLaunchKernelGGL(opcorr_affine_kernel, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(256), 0, (hipStream_t)stream,
                       zi, n, D, ket_u, ket_w, ket_k, M, g);
    return sc_check_launch("sc_hk_opcorr_initial");
}

extern "C" int sc_hk_opcorr(const sc_state *st, const double *cq, const double *bra_u, const double *bra_w, const double *bra_k,
                            const double *g, int32_t M, const uint8_t *kept, double *partials, double *out,
                            const int64_t *cursor, void *stream) {
    if (!st || !cq || !bra_u || !bra_w || !bra_k || !g || !partials || !out)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opcorr: null argument");
    int rc = sc_rows5_limits("sc_hk_opcorr", "M", "operators", st->n, st->dim, M, nullptr);
    if (rc != SC_OK) return rc;
    if (!st->qp) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opcorr: the state has no qp");
    const int64_t bands = sc_rows5_bands(st->n, M);
    hipStream_t s = (hipStream_t)stream;
    if (bands > 0) {
        OpcorrArgs a{st->qp, st->n, st->dim, M, cq, bra_u, bra_w, bra_k, g, kept, partials};
        hipLaunchKernelGGL(opcorr_tile_kernel, dim3((unsigned)((M + R5_TILE - 1) / R5_TILE), (unsigned)bands), dim3(256), 0, s, a);
        rc = sc_check_launch("sc_hk_opcorr");
        if (rc != SC_OK) return rc;
    }
    return sc_rows5_reduce("sc_hk_opcorr (reduction)", partials, bands, M, out, cursor, s);
}

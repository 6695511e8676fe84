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
//   row a of the output: sum_i of  Re x, Im x, (Re x)^2, (Im x)^2, Re x Im x        (the row of sc_hk_cross).
//
// opcorr_tile_kernel: the mapping of cross_tile_kernel (sc_cross.hip): one workgroup of 256 threads owns 64 trajectories
//   (blockIdx.y, a "band") x 64 operators (blockIdx.x); thread (ti, tj) owns the 4 x 4 pairs of trajectories 4 ti + a and operators
//   4 tj + b.  The d-loop is staged through LDS in chunks of CK, two FMAs per pair and d; then one complex product chain and the
//   three moment products -- no exponential.  With M <= 64 there is one tile column: qp is read from HBM exactly once per call.
//   The thread adds its 4 trajectories in registers, the 16 threads of an operator column add through the reused staging LDS in a
//   fixed order: one store of 5 doubles per operator into partials[band][M][5].
// opcorr_reduce_kernel: adds the bands in the fixed order of cross_reduce_kernel (16 contiguous slices, then the slices).
// No atomics; the order of every sum is a function of (n, M) alone: the same bits in every call.  Discarded trajectories (`kept`)
// and the rows beyond n are staged as zero operands, and their cq and g are never loaded (x = 0 by selection, not by a product):
// a non-finite value of a discarded trajectory cannot reach a sum.
#include "sc_common.h"

namespace {

#define OT 64      // tile edge
#define OK 16      // d chunk
#define OROW (OT + 2)   // row stride of 66 doubles: 16-byte aligned, a thread's four values are two 16-byte LDS reads

constexpr int STAGE_DOUBLES = 4 * OK * OROW;       // the d-chunk of Q, P (trajectories) and u, w (operators)
constexpr int REDUCE_DOUBLES = 16 * 5 * OT;        // [ti][column][operator] of the column reduction
constexpr int LDS_DOUBLES = STAGE_DOUBLES > REDUCE_DOUBLES ? STAGE_DOUBLES : REDUCE_DOUBLES;

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

// four consecutive doubles of a staged row, from a 16-byte aligned address
__device__ __forceinline__ void load4(const double *p, double (&o)[4]) {
    const double2 lo = ((const double2 *)p)[0], hi = ((const double2 *)p)[1];
    o[0] = lo.x; o[1] = lo.y; o[2] = hi.x; o[3] = hi.y;
}

__global__ __launch_bounds__(256) void opcorr_tile_kernel(OpcorrArgs A) {
    __shared__ alignas(16) double lds[LDS_DOUBLES];
    __shared__ double2 cqs[OT];     // cq_i of the band's trajectories (0: beyond n, or discarded)
    __shared__ int live[OT];
    double (*tq)[OROW] = (double (*)[OROW])lds, (*tp)[OROW] = tq + OK, (*ku)[OROW] = tp + OK, (*kw)[OROW] = ku + OK;
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int D = A.D, M = A.M;
    const int64_t i0 = (int64_t)blockIdx.y * OT;
    const int k0 = blockIdx.x * OT;
    const int iv = (int)min((int64_t)OT, A.n - i0), kv = min(OT, M - k0);      // valid trajectories / operators of the tile
    if (tid < OT) {
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
    for (int d0 = 0; d0 < D; d0 += OK) {
        __syncthreads();                                   // live[] is written; the last readers of the chunk before are done
        for (int e = tid; e < OK * OT; e += 256) {
            const int r = e / OK, k = e - r * OK, d = d0 + k;      // row r of the tile, column k of the chunk
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
        for (int k = 0; k < OK; ++k) {
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
            sum[b][0] += x.x; sum[b][1] += x.y;
            sum[b][2] = fma(x.x, x.x, sum[b][2]); sum[b][3] = fma(x.y, x.y, sum[b][3]); sum[b][4] = fma(x.x, x.y, sum[b][4]);
        }
    }
    __syncthreads();                                       // the staging buffers are free
    double (*red)[5][OT] = (double (*)[5][OT])lds;         // [ti][column][operator]
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int c = 0; c < 5; ++c) red[ti][c][4 * tj + b] = sum[b][c];
    __syncthreads();
    for (int e = tid; e < 5 * kv; e += 256) {
        const int t = e / 5, c = e - 5 * t;
        double s = 0.0;
        for (int g = 0; g < 16; ++g) s += red[g][c][t];
        A.partials[((size_t)blockIdx.y * M + k0) * 5 + e] = s;
    }
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

// out[e] = sum over the bands of partials[band][e], e < total = 5 M: the bands in 16 contiguous slices, each added in order by
// one thread, then the slices in order (the order of cross_reduce_kernel)
__global__ __launch_bounds__(256) void opcorr_reduce_kernel(const double *partials, int64_t bands, int64_t total, double *out,
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

// the limits both entry points share; 0 = inside
int opcorr_limits(const char *who, int64_t n, int D, int M) {
    if (M < 1 || D < 1 || n < 0) return sc_fail(SC_ERR_BAD_ARGUMENT, "%s: M=%d, D=%d, n=%lld", who, M, D, (long long)n);
    if (D > 512) return sc_fail(SC_ERR_UNSUPPORTED, "%s: D=%d outside D <= 512", who, D);
    if (M > 65535) return sc_fail(SC_ERR_UNSUPPORTED, "%s: M=%d operators outside M <= 65535", who, M);
    if ((n + OT - 1) / OT > 65535)
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: n=%lld trajectories outside n <= %d", who, (long long)n, OT * 65535);
    return SC_OK;
}

}  // namespace

extern "C" int64_t sc_hk_opcorr_rows(int64_t n, int64_t M) {
    if (n <= 0 || M <= 0) return 0;
    return (n + OT - 1) / OT;
}

extern "C" int sc_hk_opcorr_initial(const double *zi, int64_t n, int32_t D, const double *ket_u, const double *ket_w,
                                    const double *ket_k, int32_t M, double *g, void *stream) {
    if (!zi || !ket_u || !ket_w || !ket_k || !g) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opcorr_initial: null argument");
    const int rc = opcorr_limits("sc_hk_opcorr_initial", n, D, M);
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
    int rc = opcorr_limits("sc_hk_opcorr", st->n, st->dim, M);
    if (rc != SC_OK) return rc;
    if (!st->qp) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opcorr: the state has no qp");
    const int64_t bands = (st->n + OT - 1) / OT;
    hipStream_t s = (hipStream_t)stream;
    if (bands > 0) {
        OpcorrArgs a{st->qp, st->n, st->dim, M, cq, bra_u, bra_w, bra_k, g, kept, partials};
        hipLaunchKernelGGL(opcorr_tile_kernel, dim3((unsigned)((M + OT - 1) / OT), (unsigned)bands), dim3(256), 0, s, a);
        rc = sc_check_launch("sc_hk_opcorr");
        if (rc != SC_OK) return rc;
    }
    const int64_t total = (int64_t)5 * M;
    hipLaunchKernelGGL(opcorr_reduce_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, s, partials, bands, total, out,
                       (const long long *)cursor);
    return sc_check_launch("sc_hk_opcorr (reduction)");
}

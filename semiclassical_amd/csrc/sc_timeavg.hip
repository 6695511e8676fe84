// Time-averaged Herman-Kluk spectra I_k(E) of Kaledin and Miller in the separable-prefactor form (not in the reference; DESIGN.md
// section 4.17) -- the kernels behind HermanKlukPropagator.time_average() and run(time_average=...).  Per trajectory i,
// reference state k and step s of the window
//
//   g_ik(t_s) = conj(O_ik) u_i,   u_i = c_i / |c_i| e^{i S_i/hbar},   c_i = sgn_i sqrt(c2_i)        (u_i = 0 where c_i = 0)
//   A_ik(E_e) = dt sum_s g_ik(t_s) exp(i E_e t_s / hbar),             t_s = t_a + s dt
//   y_ik(e)   = |A_ik(E_e)|^2 / (2 pi hbar mc_norm P_i),   out[k][e] = (sum_i y, sum_i y^2)          (the caller divides by T, T^2)
//
// with O_ik the overlap of sc_cross.hip (bra: trajectory i of width Gamma_t, ket: reference k of width Gamma_0).
//
// ta_terms_kernel: one column of G [TB][n K] complex.  The tile, the staging and the d-loop are cross_tile_kernel's
//   (sc_cross_tile.h; K <= 64: one tile column); the tail multiplies by u_i and stores -- no sums.  Bound by the d-loop like
//   cross_tile_kernel.
// ta_phase_kernel: W [count][NE] complex, W_ce = dt exp(i E_e t_(s0 + c) / hbar): one sincos of the PRODUCT E_e t_s per element,
//   t_s = t_a + s dt formed as a product -- no recurrence in s, so the error does not grow along the window.
// ta_accumulate_kernel: A [n K][NE] += G[0 .. count)^T W, a complex fp64 product of inner length count <= TB.  A workgroup owns
//   64 rows x 64 energies, stages its G and W tiles in LDS (64 KB at TB = 32: two workgroups per CU), every thread holds 4 x 4
//   elements of A in registers, reads them once, adds the columns in ascending s and writes them once.  Bound by that one read and
//   write of A per TB steps (16 n K NE bytes each way); plain vector FMAs.  A += ... starts from the stored value and adds one
//   column after the other: the bits of A do not depend on where the blocks of columns were cut.
// ta_finish_kernel + ta_reduce_kernel: the two sums per (k, e) over the trajectories -- per band of 64 trajectories in order, then
//   the bands in 16 contiguous slices, each in order, then the slices in order (the reduction of sc_rows5.hip).  No atomics: the
//   order of every sum is a function of (n, K, NE) alone.
// Discarded trajectories (`kept`) and the tile rows beyond n are staged as zero operands with u = 0; their column entries are
// exact zeros, their state is never read, and ta_finish_kernel does not read their rows of A.
#include "sc_cross_tile.h"

#define TA_BLOCK 32                 // TB: columns of G between two updates of A

namespace {

struct TaTermsArgs {
    sc_state st;
    const double *La, *Lb, *Cm;     // diagonal widths: [D] each; dense: unused here
    const double *operands;         // dense widths: [n][4 D] from cross_operands_kernel
    const double *refs;             // [K][5 D]
    int K;
    double fac;
    const uint8_t *kept;            // may be NULL
    cplx *column;                   // [n K]
};

template <bool DIAG>
__global__ __launch_bounds__(256) void ta_terms_kernel(TaTermsArgs A) {
    __shared__ CrossStage S;
    __shared__ double2 us[R5_TILE]; // u_i of the band's trajectories (0: beyond n, discarded, or c_i = 0)
    __shared__ int live[R5_TILE];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int64_t n = A.st.n, i0 = (int64_t)blockIdx.y * R5_TILE;
    const int iv = (int)min((int64_t)R5_TILE, n - i0);
    if (tid < R5_TILE) {
        cplx u = c_make(0.0, 0.0);
        const int64_t tr = i0 + tid;
        const bool in = tid < iv && (!A.kept || A.kept[tr]);
        if (in) {
            const cplx c = signed_root(((const cplx *)A.st.c2)[tr], A.st.sgn[tr]);
            const double r = hypot(c.x, c.y);
            if (r > 0.0) u = c_mul(c_scale(c, 1.0 / r), action_phase(A.st.act[tr]));
        }
        us[tid] = u;
        live[tid] = in;
    }
    double re[4][4], im[4][4];
    cross_tile_exponents<DIAG>(S, live, A.st, A.La, A.Lb, A.Cm, A.operands, A.refs, i0, 0, A.K, tid, ti, tj, re, im);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int r = 4 * ti + a;
        if (r >= iv) continue;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int k = 4 * tj + b;
            if (k >= A.K) continue;
            cplx g = c_make(0.0, 0.0);
            if (live[r]) g = c_mul(cross_tile_overlap_conj(re[a][b], im[a][b], A.fac), us[r]);
            A.column[(i0 + r) * A.K + k] = g;
        }
    }
}

__global__ __launch_bounds__(256) void ta_phase_kernel(const double *energies, int NE, double t_a, double dt, long long s0, int count,
                                                       cplx *W) {
    const int64_t at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (at >= (int64_t)count * NE) return;
    const int c = (int)(at / NE), e = (int)(at - (int64_t)c * NE);
    // (__dmul_rn: the products stay products -- a fused t_a + s dt would round differently from the host's grid)
    const double t = t_a + __dmul_rn((double)(s0 + c), dt);
    double sn, cs;
    sincos(__dmul_rn(energies[e], t) * (1.0 / SC_HBAR), &sn, &cs);
    W[at] = c_make(dt * cs, dt * sn);
}

// thread (ti, tj) = (tid >> 4, tid & 15) owns the rows 4 ti + a and the energies tj + 16 b of the tile: its four W values of a
// column are 16 bytes apart from the next lane's (conflict-free 16-byte LDS reads), its elements of A 16 bytes apart likewise
__global__ __launch_bounds__(256) void ta_accumulate_kernel(const cplx *G, int64_t rows, int count, const cplx *W, int NE, cplx *A) {
    __shared__ cplx gs[TA_BLOCK][R5_TILE];
    __shared__ cplx ws[TA_BLOCK][R5_TILE];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int64_t r0 = (int64_t)blockIdx.x * R5_TILE;
    const int e0 = blockIdx.y * R5_TILE;
    for (int at = tid; at < count * R5_TILE; at += 256) {
        const int c = at >> 6, r = at & 63;
        gs[c][r] = r0 + r < rows ? G[(int64_t)c * rows + r0 + r] : c_make(0.0, 0.0);
        ws[c][r] = e0 + r < NE ? W[(int64_t)c * NE + e0 + r] : c_make(0.0, 0.0);
    }
    cplx acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t r = r0 + 4 * ti + a;
            const int e = e0 + tj + 16 * b;
            acc[a][b] = r < rows && e < NE ? A[r * NE + e] : c_make(0.0, 0.0);
        }
    __syncthreads();
    for (int c = 0; c < count; ++c) {                      // ascending s
        cplx g[4], w[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) g[a] = gs[c][4 * ti + a];
#pragma unroll
        for (int b = 0; b < 4; ++b) w[b] = ws[c][tj + 16 * b];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = c_fma(g[a], w[b], acc[a][b]);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t r = r0 + 4 * ti + a;
            const int e = e0 + tj + 16 * b;
            if (r < rows && e < NE) A[r * NE + e] = acc[a][b];
        }
}

// partials[band][k NE + e] = (sum y, sum y^2) over the band's trajectories, in order; one thread per (k, e)
__global__ __launch_bounds__(256) void ta_finish_kernel(const cplx *A, int64_t n, int K, int NE, const double *probi, double mc_norm,
                                                        const uint8_t *kept, double2 *partials) {
    const int64_t cols = (int64_t)K * NE, col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= cols) return;
    const int k = (int)(col / NE), e = (int)(col - (int64_t)k * NE);
    const int64_t i0 = (int64_t)blockIdx.y * R5_TILE, i1 = min(i0 + R5_TILE, n);
    double s1 = 0.0, s2 = 0.0;
    for (int64_t i = i0; i < i1; ++i) {
        if (kept && !kept[i]) continue;                    // y = 0; the row of A is not read
        const cplx a = A[(i * K + k) * NE + e];
        const double y = c_abs2(a) / (2.0 * M_PI * SC_HBAR * mc_norm * probi[i]);
        s1 += y;
        s2 = fma(y, y, s2);
    }
    partials[(int64_t)blockIdx.y * cols + col] = make_double2(s1, s2);
}

// out[x] = sum over the bands of partials[band][x], x < total: the bands in 16 contiguous slices, each added in order by one
// thread, then the slices in order (rows5_reduce_kernel of sc_rows5.hip for a row of any length)
__global__ __launch_bounds__(256) void ta_reduce_kernel(const double *partials, int64_t bands, int64_t total, double *out) {
    __shared__ double red[16][16];
    const int sl = threadIdx.x >> 4, el = threadIdx.x & 15;
    const int64_t x = (int64_t)blockIdx.x * 16 + el;
    const int64_t per = (bands + 15) / 16, b0 = sl * per, b1 = min(b0 + per, bands);
    double s = 0.0;
    if (x < total)
        for (int64_t b = b0; b < b1; ++b) s += partials[b * total + x];
    red[sl][el] = s;
    __syncthreads();
    if (sl == 0 && x < total) {
        double t = 0.0;
        for (int g = 0; g < 16; ++g) t += red[g][el];
        out[x] = t;
    }
}

// the limits every entry point shares: n >= 0, 1 <= K <= 64, n <= 64 * 65535
int ta_limits(const char *who, int64_t n, int K) {
    if (K < 1 || n < 0) return sc_fail(SC_ERR_BAD_ARGUMENT, "%s: K=%d, n=%lld", who, K, (long long)n);
    if (K > R5_TILE) return sc_fail(SC_ERR_UNSUPPORTED, "%s: K=%d reference states outside K <= %d", who, K, R5_TILE);
    if ((n + R5_TILE - 1) / R5_TILE > 65535)
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: n=%lld trajectories outside n <= %d", who, (long long)n, R5_TILE * 65535);
    return SC_OK;
}

int ta_energy_limits(const char *who, int NE) {
    if (NE < 1) return sc_fail(SC_ERR_BAD_ARGUMENT, "%s: NE=%d", who, NE);
    if (NE > 65535) return sc_fail(SC_ERR_UNSUPPORTED, "%s: NE=%d energies outside NE <= 65535", who, NE);
    return SC_OK;
}

}  // namespace

extern "C" int32_t sc_hk_ta_block(void) { return TA_BLOCK; }

extern "C" int sc_hk_ta_terms(const sc_state *st, const double *La, const double *Lb, const double *Ct, int32_t diag, double fac,
                              const double *refs, int32_t K, const uint8_t *kept, double *operands, double *G, int32_t column,
                              void *stream) {
    if (!st || !La || !Lb || !Ct || !refs || !G) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_ta_terms: null argument");
    if (st->dim < 1) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_ta_terms: D=%d", st->dim);
    if (column < 0 || column >= TA_BLOCK)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_ta_terms: column=%d outside 0 ... %d", column, TA_BLOCK - 1);
    int rc = ta_limits("sc_hk_ta_terms", st->n, K);
    if (rc != SC_OK) return rc;
    if (!diag && !operands) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_ta_terms: dense widths need the operand scratch [n][4 D]");
    if (st->dim > 512) return sc_fail(SC_ERR_UNSUPPORTED, "sc_hk_ta_terms: D=%d outside D <= 512", st->dim);
    const int64_t bands = (st->n + R5_TILE - 1) / R5_TILE;
    if (bands == 0) return SC_OK;
    hipStream_t s = (hipStream_t)stream;
    if (!diag) {
        rc = sc_cross_operands("sc_hk_ta_terms (operands)", st, La, Lb, Ct, operands, s);
        if (rc != SC_OK) return rc;
    }
    TaTermsArgs a{*st, La, Lb, Ct, operands, refs, K, fac, kept, (cplx *)G + (int64_t)column * st->n * K};
    const dim3 grid(1, (unsigned)bands);
    if (diag) hipLaunchKernelGGL(ta_terms_kernel<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(ta_terms_kernel<false>, grid, dim3(256), 0, s, a);
    return sc_check_launch("sc_hk_ta_terms");
}

extern "C" int sc_hk_ta_accumulate(const double *G, int64_t n, int32_t K, int32_t count, const double *energies, int32_t NE,
                                   double t_a, double dt, int64_t s0, double *W, double *A, void *stream) {
    if (!G || !energies || !W || !A) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_ta_accumulate: null argument");
    if (count < 1 || count > TA_BLOCK)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_ta_accumulate: count=%d outside 1 ... %d", count, TA_BLOCK);
    int rc = ta_limits("sc_hk_ta_accumulate", n, K);
    if (rc == SC_OK) rc = ta_energy_limits("sc_hk_ta_accumulate", NE);
    if (rc != SC_OK) return rc;
    const int64_t rows = n * K;
    if (rows == 0) return SC_OK;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ta_phase_kernel, dim3((unsigned)(((int64_t)count * NE + 255) / 256)), dim3(256), 0, s, energies, NE, t_a, dt,
                       (long long)s0, count, (cplx *)W);
    rc = sc_check_launch("sc_hk_ta_accumulate (phases)");
    if (rc != SC_OK) return rc;
    const dim3 grid((unsigned)((rows + R5_TILE - 1) / R5_TILE), (unsigned)((NE + R5_TILE - 1) / R5_TILE));
    hipLaunchKernelGGL(ta_accumulate_kernel, grid, dim3(256), 0, s, (const cplx *)G, rows, count, (const cplx *)W, NE, (cplx *)A);
    return sc_check_launch("sc_hk_ta_accumulate");
}

extern "C" int64_t sc_hk_ta_finish_rows(int64_t n) { return n <= 0 ? 0 : (n + R5_TILE - 1) / R5_TILE; }

extern "C" int sc_hk_ta_finish(const double *A, int64_t n, int32_t K, int32_t NE, const double *probi, double mc_norm,
                               const uint8_t *kept, double *partials, double *out, void *stream) {
    if (!A || !probi || !partials || !out) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_ta_finish: null argument");
    int rc = ta_limits("sc_hk_ta_finish", n, K);
    if (rc == SC_OK) rc = ta_energy_limits("sc_hk_ta_finish", NE);
    if (rc != SC_OK) return rc;
    const int64_t bands = sc_hk_ta_finish_rows(n), cols = (int64_t)K * NE;
    hipStream_t s = (hipStream_t)stream;
    if (bands > 0) {
        const dim3 grid((unsigned)((cols + 255) / 256), (unsigned)bands);
        hipLaunchKernelGGL(ta_finish_kernel, grid, dim3(256), 0, s, (const cplx *)A, n, K, NE, probi, mc_norm, kept,
                           (double2 *)partials);
        rc = sc_check_launch("sc_hk_ta_finish");
        if (rc != SC_OK) return rc;
    }
    hipLaunchKernelGGL(ta_reduce_kernel, dim3((unsigned)((2 * cols + 15) / 16)), dim3(256), 0, s, partials, bands, 2 * cols, out);
    return sc_check_launch("sc_hk_ta_finish (reduction)");
}

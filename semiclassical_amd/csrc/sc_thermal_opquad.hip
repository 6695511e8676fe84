// Thermal operator correlation functions X_a(t) = Tr[rho e^(iH_es t) A_a e^(-iH_gs t) B_a] of the Herman-Kluk thermal ensemble for
// M pairs of QUADRATIC operators A_a = c_a + m_a.x + 1/2 x^T K_a x (not in the reference) -- the kernels
// behind HermanKlukPropagator.thermal_quadratic_correlation() and run(thermal_quadratic=...) once a K is given.  The columns of
// sc_opquad.hip with the trajectory's OWN centre of sc_thermal_opcorr.hip in the place of (q0, p0): one side of one operator is a
// list of 1 + R columns, each an affine form of the point and of the centre in mode coordinates (Qc_i, Pc_i) [d''],
//
//   z_col = k_col + u_col.Q_i + i w_col.P_i + ut_col.Qc_i(t) + i wt_col.Pc_i(t)       (the bra; the ket: q_i, p_i and t = 0)
//   f_ia  = l_0 z_0 + sum_{col >= 1} l_col z_col^2
//   x_ia  = f_ia g_ia cq_i,  row a of the output: the five sums of x_ia over i (sc_rows5.h)
//
// (hostmath.fold_thermal_quadratic_operators).  cq_i is the thermal C_auto term sc_hk_correlate_thermal exports.
//
// thermal_opquad_tile_kernel: the text of opquad_tile_kernel (sc_opquad.hip) -- operators per tile, the wide case 1 + R > 64, the
//   powers, the segmented column sum by planes, the finish by quarters -- with optile_rotated_loop of sc_optile.h, the mode loop it
//   shares with thermal_opcorr_tile_kernel, per tile between the staged loop over D and the powers.  (The tile text is a copy: as
//   one definition in sc_optile.h it changed the bits opquad_tile_kernel is pinned to)  The order of every
//   sum is a function of (n, M, R, D, d'') alone.  th->map_q, map_p, q0, n1 are not read; the centres of discarded trajectories and of
//   the rows beyond n are never loaded.
//   The rotation table in the wide case, where it is rewritten for every tile: the last read of tile t's table lies before the second
//   barrier of its last chunk (optile_rotated_loop); the first write of tile t + 1's table comes after the four barriers of tile t's
//   planes and the first barrier of tile t + 1's loop over D.  Every thread passes those, whatever `ov`, `kv` or live[] say: no
//   barrier of the tile loop stands under a condition that differs between threads, so no reader is still behind them.
#include "sc_optile.h"

namespace {

constexpr int STAGE_DOUBLES = sizeof(OpStage) / sizeof(double);
constexpr int PLANE_ROW = R5_TILE + 1;                     // row stride of a plane of t or x: lane = row reads without conflicts
static_assert(R5_TILE * PLANE_ROW <= STAGE_DOUBLES, "a plane of t fits the staging buffers");
static_assert(4 * 5 * R5_TILE <= STAGE_DOUBLES, "the four quarters of the five sums fit the staging buffers");

struct ThermalOpquadArgs {
    const double *qp;               // [n][2 D]
    int64_t n;
    int D, dm, M, C1;               // C1 = 1 + R columns per operator
    double time;
    const double *omega;            // [d'']
    const double *centres;          // [n][2 d''] at t = 0
    const double *cq;               // [n] complex: the thermal terms
    const double *u, *w;            // [M C1][D]
    const double *ut, *wt;          // [M C1][d'']
    const double *kap;              // [M C1] complex
    const double *lam;              // [M C1]
    const double *g;                // [n][M] complex
    const uint8_t *kept;            // may be NULL
    double *partials;               // [bands][M][5]
};

__global__ __launch_bounds__(256, 2) void thermal_opquad_tile_kernel(ThermalOpquadArgs A) {
    __shared__ OpStage S;      // the planes of t and x and the four quarters of the sums reuse it
    __shared__ double2 cqs[R5_TILE];// cq_i of the band's trajectories (0: beyond n, or discarded)
    __shared__ int live[R5_TILE];
    __shared__ OpRotTable rot;
    typedef double prow[PLANE_ROW];
    prow *plane = (prow *)&S;                              // [trajectory][tile column] of t; [operator][trajectory] of x
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int D = A.D, M = A.M, C1 = A.C1;
    const int64_t i0 = (int64_t)blockIdx.y * R5_TILE;
    // the workgroup's operators a0 ... a0 + ov - 1, its tiles, and the columns of an operator inside one tile
    const bool wide = C1 > R5_TILE;
    const int per = wide ? 1 : R5_TILE / C1;
    const int a0 = blockIdx.x * per, ov = min(per, M - a0);
    const int tiles = wide ? (C1 + R5_TILE - 1) / R5_TILE : 1;
    const int64_t c0 = (int64_t)a0 * C1, cend = c0 + (int64_t)ov * C1;       // the workgroup's columns
    const int pr = tid & (R5_TILE - 1), pw = tid >> 6;     // the (trajectory, operator) pairs of the thread: pr, pw + 4 s
    optile_band_header(live, cqs, A.n, i0, A.kept, A.cq, tid);
    double fre[16], fim[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) { fre[s] = 0.0; fim[s] = 0.0; }
    for (int tile = 0; tile < tiles; ++tile) {
        const int64_t k0 = c0 + (int64_t)tile * R5_TILE;
        const int kv = (int)min((int64_t)R5_TILE, cend - k0);                  // valid columns of the tile
        const int seg = wide ? kv : C1;                    // columns of one operator in this tile
        double fr[4][4] = {}, fi[4][4] = {};
        optile_staged_loop(S, live, A.qp, D, A.u, A.w, i0, k0, kv, tid, ti, tj, fr, fi);       // the current points against u, w
        optile_rotated_loop(S, rot, live, A.omega, A.time, A.centres, A.dm, A.ut, A.wt, i0, k0, kv, tid, ti, tj, fr, fi);
        // t = l z^p, z = k + (fr, fi), in place; the columns beyond kv give zero
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int col = 4 * tj + b;
            const bool in = col < kv;
            const cplx kap = in ? ((const cplx *)A.kap)[k0 + col] : c_make(0.0, 0.0);
            const double lam = in ? A.lam[k0 + col] : 0.0;
            const bool first = wide ? tile == 0 && col == 0 : col % C1 == 0;  // column 0 of its operator: the first power
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const cplx z = c_make(kap.x + fr[a][b], kap.y + fi[a][b]);
                const cplx zp = first ? z : c_mul(z, z);
                fr[a][b] = lam * zp.x; fi[a][b] = lam * zp.y;
            }
        }
        // the columns of every operator, in column order, one plane at a time
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            __syncthreads();                               // the buffers (or the plane before) are free
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) plane[4 * ti + a][4 * tj + b] = part == 0 ? fr[a][b] : fi[a][b];
            __syncthreads();
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int o = pw + 4 * s;
                if (o < ov) {
                    double acc = part == 0 ? fre[s] : fim[s];
                    const double *t = &plane[pr][o * seg];
                    for (int j = 0; j < seg; ++j) acc += t[j];
                    if (part == 0) fre[s] = acc; else fim[s] = acc;
                }
            }
        }
    }
    // x_ia = f_ia g_ia cq_i, as planes [operator][trajectory]; thread (operator po, quarter pq) adds its 16 trajectories in order
    const int po = tid & (R5_TILE - 1), pq = tid >> 6;
    double xr[16], sum[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int o = pw + 4 * s;
            if (o < ov) {
                if (part == 0) {
                    cplx x = c_make(0.0, 0.0);
                    if (live[pr]) {
                        const cplx g = ((const cplx *)A.g)[(size_t)(i0 + pr) * M + a0 + o];
                        x = c_mul(c_mul(c_make(fre[s], fim[s]), g), cqs[pr]);
                    }
                    fre[s] = x.x; fim[s] = x.y;
                }
                plane[o][pr] = part == 0 ? fre[s] : fim[s];
            }
        }
        __syncthreads();
        if (po < ov) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const double v = plane[po][16 * pq + i];
                if (part == 0) xr[i] = v;
                else rows5_add(sum, c_make(xr[i], v));
            }
        }
    }
    __syncthreads();
    double (*red)[5][R5_TILE] = (double (*)[5][R5_TILE])&S;
    if (po < ov)
#pragma unroll
        for (int c = 0; c < 5; ++c) red[pq][c][po] = sum[c];
    __syncthreads();
    for (int e = tid; e < 5 * ov; e += 256) {
        const int t = e / 5, c = e - 5 * t;
        double s = 0.0;
        for (int q = 0; q < 4; ++q) s += red[q][c][t];
        A.partials[((size_t)blockIdx.y * M + a0) * 5 + e] = s;
    }
}

// out[i][a] = sum over the columns of operator a of  l z^p,  z = k + u.z_i[:D] + i w.z_i[D:] + ut.c_i[:d''] + i wt.c_i[d'':]  (p = 1
// for column 0, else 2): opquad_initial_kernel with the two dot products of the centre per column
__global__ __launch_bounds__(256) void thermal_opquad_initial_kernel(const double *z, const double *cen, int64_t n, int D, int dm,
                                                                     const double *u, const double *w, const double *ut,
                                                                     const double *wt, const double *kap, const double *lam, int M,
                                                                     int C1, double *out) {
    const int64_t total = n * M;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / M;
        const int a = (int)(e - i * M);
        cplx f = c_make(0.0, 0.0);
        for (int j = 0; j < C1; ++j) {
            const size_t col = (size_t)a * C1 + j;
            double re = 0.0, im = 0.0;
            optile_affine_dot(u + col * D, w + col * D, z + i * 2 * D, D, re, im);
            optile_affine_dot(ut + col * dm, wt + col * dm, cen + i * 2 * dm, dm, re, im);
            const cplx zc = c_make(kap[2 * col] + re, kap[2 * col + 1] + im);
            const cplx zp = j == 0 ? zc : c_mul(zc, zc);
            f.x += lam[col] * zp.x; f.y += lam[col] * zp.y;
        }
        ((cplx *)out)[e] = f;
    }
}

// the limits of sc_hk_opquad, then those of sc_hk_opcorr_thermal
int thermal_opquad_limits(const char *who, int64_t n, int D, int dm, int M, int R) {
    const int rc = sc_opquad_limits(who, n, D, M, R);
    return rc != SC_OK ? rc : sc_thermal_modes_limit(who, D, dm);
}

}  // namespace

extern "C" int64_t sc_hk_opquad_thermal_rows(int64_t n, int64_t M) { return sc_rows5_bands(n, M); }

extern "C" int sc_hk_opquad_thermal_initial(const double *zi, const double *centres, int64_t n, int32_t D, int32_t dmodes,
                                            const double *ket_u, const double *ket_w, const double *ket_ut, const double *ket_wt,
                                            const double *ket_k, const double *ket_l, int32_t M, int32_t RB, double *g, void *stream) {
    if (!zi || !centres || !ket_u || !ket_w || !ket_ut || !ket_wt || !ket_k || !ket_l || !g)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opquad_thermal_initial: null argument");
    const int rc = thermal_opquad_limits("sc_hk_opquad_thermal_initial", n, D, dmodes, M, RB);
    if (rc != SC_OK) return rc;
    if (n == 0) return SC_OK;
    hipLaunchKernelGGL(thermal_opquad_initial_kernel, sc_optile_prepass_grid(n, M), dim3(256), 0, (hipStream_t)stream, zi, centres, n,
                       D, dmodes, ket_u, ket_w, ket_ut, ket_wt, ket_k, ket_l, M, 1 + RB, g);
    return sc_check_launch("sc_hk_opquad_thermal_initial");
}

extern "C" int sc_hk_opquad_thermal(const sc_state *st, double time, const sc_thermal_consts *th, const double *cq,
                                    const double *bra_u, const double *bra_w, const double *bra_ut, const double *bra_wt,
                                    const double *bra_k, const double *bra_l, const double *g, int32_t M, int32_t RA,
                                    const uint8_t *kept, double *partials, double *out, const int64_t *cursor, void *stream) {
    if (!st || !th || !cq || !bra_u || !bra_w || !bra_ut || !bra_wt || !bra_k || !bra_l || !g || !partials || !out)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opquad_thermal: null argument");
    const int rc = thermal_opquad_limits("sc_hk_opquad_thermal", st->n, st->dim, th->dmodes, M, RA);
    if (rc != SC_OK) return rc;
    if (!st->qp) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opquad_thermal: the state has no qp");
    if (!th->omega || !th->centres || th->dim != st->dim)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opquad_thermal: thermal constants for D = %d without omega or centres, state D = %d",
                       th->dim, st->dim);
    const int C1 = 1 + RA, per = C1 > R5_TILE ? 1 : R5_TILE / C1;
    ThermalOpquadArgs a{st->qp, st->n, st->dim, th->dmodes, M, C1, time, th->omega, th->centres, cq, bra_u, bra_w, bra_ut, bra_wt,
                        bra_k, bra_l, g, kept, partials};
    return sc_optile_rows("sc_hk_opquad_thermal", (const void *)thermal_opquad_tile_kernel, &a, (unsigned)((M + per - 1) / per), st->n, M,
                          partials, out, cursor, (hipStream_t)stream);
}

// Thermal operator correlation functions X_a(t) = Tr[rho e^(iH_es t) A_a e^(-iH_gs t) B_a] of the Herman-Kluk thermal ensemble for
// M pairs of LINEAR operators A_a = cA_a + mA_a.x, B_a = cB_a + mB_a.x (not in the reference) -- the kernels
// behind HermanKlukPropagator.thermal_operator_correlation() and run(thermal_operators=...).  Every trajectory's thermal C_auto
// term cq_i (what sc_hk_correlate_thermal exports: phase, both overlaps, prefactor and weight inside) is multiplied by the two
// Gaussian matrix elements of sc_opcorr.hip with the trajectory's OWN centre in the place of (q0, p0), the bra centre rotated to
// the time of the state.  The host folds the Cartesian maps of the centres into the operators (hostmath.
// fold_thermal_linear_operators), so the kernels see dot products with the mode coordinates (Qc_i, Pc_i) [d''] only:
//
//   f_ia = bra_k_a + bra_u_a.Q_i + i bra_w_a.P_i + bra_ut_a.Qc_i(t) + i bra_wt_a.Pc_i(t)      (the tile kernel, every step)
//   g_ia = ket_k_a + ket_u_a.q_i + i ket_w_a.p_i + ket_ut_a.Qc_i    + i ket_wt_a.Pc_i         (affine_kernel, once per ensemble and set)
//   x_ia = f_ia g_ia cq_i,   row a of the output: the five sums of x_ia over i (sc_rows5.h)
//   Qc(t) = Qc cos wt + Pc / w sin wt,   Pc(t) = Pc cos wt - w Qc sin wt
//
// thermal_opcorr_tile_kernel: opcorr_tile_kernel (the pieces of sc_optile.h) with a second staged loop between the loop over D and
//   the finish, over the d'' modes, whose trajectory planes are the centres rotated WHILE STAGING (optile_rotated_loop of
//   sc_optile.h, which sc_thermal_opquad.hip shares).  th->map_q, map_p, q0, n1 are not read.  The centres of discarded trajectories and of the
//   rows beyond n are never loaded either.
#include "sc_optile.h"

namespace {

struct ThermalOpcorrArgs {
    const double *qp;               // [n][2 D]
    int64_t n;
    int D, dm, M;
    double time;
    const double *omega;            // [d'']
    const double *centres;          // [n][2 d''] at t = 0
    const double *cq;               // [n] complex
    const double *u, *w;            // [M][D]
    const double *ut, *wt;          // [M][d'']
    const double *kap;              // [M] complex
    const double *g;                // [n][M] complex
    const uint8_t *kept;            // may be NULL
    double *partials;               // [bands][M][5]
};

__global__ __launch_bounds__(256) void thermal_opcorr_tile_kernel(ThermalOpcorrArgs A) {
    __shared__ OpTileLds lds;
    __shared__ double2 cqs[R5_TILE];// cq_i of the band's trajectories (0: beyond n, or discarded)
    __shared__ int live[R5_TILE];
    __shared__ OpRotTable rot;
    OpStage &S = lds.S;
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int dm = A.dm;
    const int64_t i0 = (int64_t)blockIdx.y * R5_TILE;
    const int k0 = blockIdx.x * R5_TILE, kv = min(R5_TILE, A.M - k0);          // the operators of the tile
    optile_band_header(live, cqs, A.n, i0, A.kept, A.cq, tid);
    double fr[4][4] = {}, fi[4][4] = {};
    optile_staged_loop(S, live, A.qp, A.D, A.u, A.w, i0, k0, kv, tid, ti, tj, fr, fi);       // the current points against u, w
    // the rotated centres against ut, wt
    optile_rotated_loop(S, rot, live, A.omega, A.time, A.centres, dm, A.ut, A.wt, i0, k0, kv, tid, ti, tj, fr, fi);
    optile_finish_linear(fr, fi, live, cqs, A.kap, A.g, i0, k0, kv, A.M, &lds, tid, ti, tj, A.partials);
}

// out[i][a] = k_a + u_a.z_i[:D] + i w_a.z_i[D:] + ut_a.c_i[:d''] + i wt_a.c_i[d'':], one (trajectory, operator) pair per thread,
// the operator index fastest: opcorr_affine_kernel with the two dot products of the centre
__global__ __launch_bounds__(256) void thermal_opcorr_affine_kernel(const double *z, const double *cen, int64_t n, int D, int dm,
                                                                    const double *u, const double *w, const double *ut,
                                                                    const double *wt, const double *kap, int M, double *out) {
    const int64_t total = n * M;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / M;
        const int a = (int)(e - i * M);
        double re = 0.0, im = 0.0;
        optile_affine_dot(u + (size_t)a * D, w + (size_t)a * D, z + i * 2 * D, D, re, im);
        optile_affine_dot(ut + (size_t)a * dm, wt + (size_t)a * dm, cen + i * 2 * dm, dm, re, im);
        ((cplx *)out)[e] = c_make(kap[2 * a] + re, kap[2 * a + 1] + im);
    }
}

// the limits both entry points share: those of the five-sum rows, then 1 <= d'' <= D
int thermal_opcorr_limits(const char *who, int64_t n, int D, int dm, int M) {
    const int rc = sc_rows5_limits(who, "M", "operators", n, D, M, nullptr);
    if (rc != SC_OK) return rc;
    return sc_thermal_modes_limit(who, D, dm);
}

}  // namespace

int sc_thermal_modes_limit(const char *who, int D, int dm) {
    if (dm < 1 || dm > D) return sc_fail(SC_ERR_UNSUPPORTED, "%s: d''=%d outside 1 <= d'' <= D=%d", who, dm, D);
    return SC_OK;
}

extern "C" int64_t sc_hk_opcorr_thermal_rows(int64_t n, int64_t M) { return sc_rows5_bands(n, M); }

extern "C" int sc_hk_opcorr_thermal_initial(const double *zi, const double *centres, int64_t n, int32_t D, int32_t dmodes,
                                            const double *ket_u, const double *ket_w, const double *ket_ut, const double *ket_wt,
                                            const double *ket_k, int32_t M, double *g, void *stream) {
    if (!zi || !centres || !ket_u || !ket_w || !ket_ut || !ket_wt || !ket_k || !g)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opcorr_thermal_initial: null argument");
    const int rc = thermal_opcorr_limits("sc_hk_opcorr_thermal_initial", n, D, dmodes, M);
    if (rc != SC_OK) return rc;
    if (n == 0) return SC_OK;
    hipLaunchKernelGGL(thermal_opcorr_affine_kernel, sc_optile_prepass_grid(n, M), dim3(256), 0, (hipStream_t)stream, zi, centres, n,
                       D, dmodes, ket_u, ket_w, ket_ut, ket_wt, ket_k, M, g);
    return sc_check_launch("sc_hk_opcorr_thermal_initial");
}

extern "C" int sc_hk_opcorr_thermal(const sc_state *st, double time, const sc_thermal_consts *th, const double *cq,
                                    const double *bra_u, const double *bra_w, const double *bra_ut, const double *bra_wt,
                                    const double *bra_k, const double *g, int32_t M, const uint8_t *kept, double *partials,
                                    double *out, const int64_t *cursor, void *stream) {
    if (!st || !th || !cq || !bra_u || !bra_w || !bra_ut || !bra_wt || !bra_k || !g || !partials || !out)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opcorr_thermal: null argument");
    const int rc = thermal_opcorr_limits("sc_hk_opcorr_thermal", st->n, st->dim, th->dmodes, M);
    if (rc != SC_OK) return rc;
    if (!st->qp) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opcorr_thermal: the state has no qp");
    if (!th->omega || !th->centres || th->dim != st->dim)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opcorr_thermal: thermal constants for D = %d without omega or centres, state D = %d",
                       th->dim, st->dim);
    ThermalOpcorrArgs a{st->qp, st->n, st->dim, th->dmodes, M, time, th->omega, th->centres, cq, bra_u, bra_w, bra_ut, bra_wt,
                        bra_k, g, kept, partials};
    return sc_optile_rows("sc_hk_opcorr_thermal", (const void *)thermal_opcorr_tile_kernel, &a, (unsigned)((M + R5_TILE - 1) / R5_TILE),
                          st->n, M, partials, out, cursor, (hipStream_t)stream);
}

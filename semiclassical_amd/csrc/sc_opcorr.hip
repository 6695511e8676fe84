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
// opcorr_tile_kernel: the pieces of sc_optile.h in a row, the columns being the operators.  Per pair and d two FMAs; then one
//   complex product chain -- no exponential.  With M <= 64 there is one tile column: qp is read from HBM exactly once per call.
#include "sc_optile.h"

namespace {

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
    __shared__ OpTileLds lds;
    __shared__ double2 cqs[R5_TILE];// cq_i of the band's trajectories (0: beyond n, or discarded)
    __shared__ int live[R5_TILE];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int64_t i0 = (int64_t)blockIdx.y * R5_TILE;
    const int k0 = blockIdx.x * R5_TILE, kv = min(R5_TILE, A.M - k0);          // the operators of the tile
    optile_band_header(live, cqs, A.n, i0, A.kept, A.cq, tid);
    double fr[4][4] = {}, fi[4][4] = {};
    optile_staged_loop(lds.S, live, A.qp, A.D, A.u, A.w, i0, k0, kv, tid, ti, tj, fr, fi);
    optile_finish_linear(fr, fi, live, cqs, A.kap, A.g, i0, k0, kv, A.M, &lds, tid, ti, tj, A.partials);
}

// out[i][a] = k_a + u_a.z_i[:D] + i w_a.z_i[D:], one (trajectory, operator) pair per thread, the operator index fastest
__global__ __launch_bounds__(256) void opcorr_affine_kernel(const double *z, int64_t n, int D, const double *u, const double *w,
                                                            const double *kap, int M, double *out) {
    const int64_t total = n * M;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / M;
        const int a = (int)(e - i * M);
        double re = 0.0, im = 0.0;
        optile_affine_dot(u + (size_t)a * D, w + (size_t)a * D, z + i * 2 * D, D, re, im);
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
    hipLaunchKernelGGL(opcorr_affine_kernel, sc_optile_prepass_grid(n, M), dim3(256), 0, (hipStream_t)stream, zi, n, D, ket_u, ket_w,
                       ket_k, M, g);
    return sc_check_launch("sc_hk_opcorr_initial");
}

extern "C" int sc_hk_opcorr(const sc_state *st, const double *cq, const double *bra_u, const double *bra_w, const double *bra_k,
                            const double *g, int32_t M, const uint8_t *kept, double *partials, double *out,
                            const int64_t *cursor, void *stream) {
    if (!st || !cq || !bra_u || !bra_w || !bra_k || !g || !partials || !out)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opcorr: null argument");
    const int rc = sc_rows5_limits("sc_hk_opcorr", "M", "operators", st->n, st->dim, M, nullptr);
    if (rc != SC_OK) return rc;
    if (!st->qp) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_opcorr: the state has no qp");
    OpcorrArgs a{st->qp, st->n, st->dim, M, cq, bra_u, bra_w, bra_k, g, kept, partials};
    return sc_optile_rows("sc_hk_opcorr", (const void *)opcorr_tile_kernel, &a, (unsigned)((M + R5_TILE - 1) / R5_TILE), st->n, M,
                          partials, out, cursor, (hipStream_t)stream);
}

// Quartic force field (QFF): a coupled anharmonic Taylor expansion around pos0 with the cubic derivatives t_ijk and the
// semi-diagonal quartic derivatives u_iiii, u_iijj, u_iiij.  With x = r - pos0, y_i = x_i^2,
// z_i = x_i^3 and the constants folded by the host (A_ij = u_iijj / 8, A_ii = u_iiii / 24, B_ij = u_iiij / 6):
//   W_ij   = sum_k t_ijk x_k
//   V      = e0 + g.x + 1/2 x^T H x + 1/6 x^T W x + y^T A y + z^T B x
//   dV_m   = g_m + (Hx)_m + 1/2 (Wx)_m + 4 x_m (Ay)_m + 3 x_m^2 (Bx)_m + (B^T z)_m
//   d2V_mn = H_mn + W_mn + 8 A_mn x_m x_n + 3 B_mn x_m^2 + 3 B_nm x_n^2 + delta_mn [4 (Ay)_m + 6 x_m (Bx)_m]
//
// One kernel.  A workgroup (four wavefronts) owns QFF_TB = 16 QFF_RT trajectories, whose displacements sit in LDS as
// xs[k][trajectory] (rows D .. Dp - 1 are zero: K is padded to a multiple of 4, D to a multiple of 16, in LDS only --
// nothing is read past an array).  Wavefront w walks the Hessian rows i = w, w + 4, ...; for a row it walks the blocks of
// 16 consecutive j.  W = T.X runs on v_mfma_f64_16x16x4_f64 with the TRAJECTORIES as the A operand (rows) and the 16
// consecutive j as the B operand (columns), B[k][j] = t[i][k][j] (= t_ijk: the tensor is fully symmetric) streamed from
// L2 and shared by the QFF_RT accumulator tiles of the wavefront.  C/D map of the f64 instruction: column = lane & 15,
// row = (lane >> 4) + 4 reg -- the 16 lanes of an accumulator row hold 16 consecutive j of ONE trajectory's Hessian row and
// store 128 contiguous bytes, straight into the image the monodromy kernel reads.
// Epilogue per tile, on the accumulators: the constant and quartic parts of the Hessian, and this lane's share of the five
// row sums (Hx)_i, (Wx)_i, (Ay)_i, (Bx)_i, (B^T z)_i.  The block of j that holds the diagonal goes last, so that the
// diagonal term is complete when that element is stored.  Per row, three combinations of the sums are added over the 16
// lanes by DPP rotations (every lane ends with the same bits): the gradient, the row's share of the energy, the diagonal.
//   Order.     Every sum runs in an order fixed by D: k ascending inside the MFMA chain, j blocks ascending with the diagonal
//              block last, the rotation tree over the 16 lanes, rows i = w, w + 4, ... per wavefront, wavefronts 0..3.
//              A trajectory's bits do not depend on n, on its index, on its place in the tile or on the grid.  No atomics.
//   Symmetry.  t, H, A are stored exactly symmetric by the host, so W_ij and W_ji are the same chain of the same products;
//              the remaining terms are formed without contraction into fused multiply-adds from commutative operations
//              (x_i x_j; 3 B_ij y_i + 3 B_ji y_j as a sum of two rounded products).  hess[i][j] == hess[j][i] bit for bit.
//   Parts.     cubic == NULL: no MFMA chain at all; both quartic pointers NULL: no quartic terms (template parameters).
// The stage variant puts sc_stage_point's kernel in front and sc_stage_consume's behind, as sc_gdml_large.hip does.
#include "sc_common.h"
#include "sc_row16.h"

int sc_stage_point_range(const sc_state *st, const sc_dense_scratch *sc, double dt, int stage, double *r_out, int64_t t0,
                         int64_t t1, hipStream_t stream);                                    // sc_dense_mono.hip
int sc_stage_consume_range(const sc_state *st, const sc_dense_scratch *sc, const double *inv_mass, const double *V,
                           const double *grad, double dt, int stage, double *energy_partials, int64_t t0, int64_t t1,
                           int accumulate, hipStream_t stream);

#ifndef SC_QFF_RT
// accumulator tiles (of 16 trajectories) per wavefront.  Measured at D = 24, 60 (n = 1e5) and 96 (n = 1e4), ms per sc_qff_stage
// call: 0.45, 3.23, 1.40 with one tile; 0.70, 4.77, 2.98 with two; 0.69, 4.34, 1.96 with four (profiles/qff_timing.jsonl).  The
// re-read of the cubic tensor from L2 per 16 trajectories is not what bounds the kernel: the per-trajectory row sums of the
// epilogue are held in registers (148 VGPRs with one tile: three wavefronts per SIMD; 260 and 434 with two and four: one), and
// with one wavefront per SIMD nothing overlaps the epilogue's vector work with the next tile's matrix-core chain.  Eight tiles
// spill.  DESIGN.md section 4.18.
#define SC_QFF_RT 1
#endif

namespace {

constexpr int QFF_MAX_DIM = 96;                                  // sc_dense_mono_step's MFMA route ends here
constexpr int QFF_RT = SC_QFF_RT, QFF_TB = 16 * QFF_RT;         // trajectories per workgroup
constexpr int QFF_LD = QFF_TB + 4;                               // row pitch of xs (doubles)
constexpr int QFF_WAVES = 4;
constexpr int64_t QFF_MAX_N = (int64_t)64 * 65535;

typedef double d4 __attribute__((ext_vector_type(4)));

struct QffArgs {
    sc_qff_model M;
    const double *r;       // [n][D]
    int64_t n;
    double *energy;        // [n]
    double *grad;          // [n][D]
    double *hess;          // trajectory b, row i, column j at hess[b * hstride + i * D + j]
    int64_t hstride;
};

inline size_t qff_lds_bytes(int D) {
    const int Dp = (D + 15) & ~15;
    return sizeof(double) * ((size_t)Dp * QFF_LD + QFF_WAVES * QFF_TB);
}

// constant + quartic part of one Hessian element on top of hw = H_ij + W_ij.  No contraction: every product is rounded on its
// own, so that exchanging (i, j) exchanges the operands of commutative operations and nothing else
template <bool QUART>
__device__ __forceinline__ double qff_hess_element(double hw, double a8, double b3ij, double b3ji, double xi, double xj, double yi,
                                                   double yj) {
#pragma clang fp contract(off)
    if constexpr (!QUART) return hw;
    else {
        const double t1 = a8 * (xi * xj);
        const double p = b3ij * yi, q = b3ji * yj;
        return (hw + t1) + (p + q);
    }
}

template <bool CUBIC, bool QUART>
__global__ __launch_bounds__(64 * QFF_WAVES) void qff_kernel(QffArgs a) {
    extern __shared__ double qff_lds[];
    const sc_qff_model &M = a.M;
    const int D = M.dim, Dp = (D + 15) & ~15, K4 = (D + 3) >> 2, njb = Dp >> 4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, rg = lane >> 4;
    const int64_t b0 = (int64_t)blockIdx.x * QFF_TB;
    double *xs = qff_lds, *ep = qff_lds + (size_t)Dp * QFF_LD;

    // displacements of the tile, zero beyond D and beyond n
    for (int idx = tid; idx < Dp * QFF_TB; idx += 64 * QFF_WAVES) {
        const int b = idx / Dp, k = idx - b * Dp;
        double v = 0.0;
        if (k < D && b0 + b < a.n) v = a.r[(size_t)(b0 + b) * D + k] - M.pos0[k];
        xs[k * QFF_LD + b] = v;
    }
    if (li == 0) {
#pragma unroll
        for (int rt = 0; rt < QFF_RT; ++rt)
#pragma unroll
            for (int q = 0; q < 4; ++q) ep[wave * QFF_TB + 16 * rt + rg + 4 * q] = 0.0;      // this lane alone adds to them
    }
    __syncthreads();

    const double *qa = M.quartic_a, *qb = M.quartic_b;
    for (int i = wave; i < D; i += QFF_WAVES) {
        const int jd = i >> 4;
        // this lane's shares of the row sums, per trajectory (16 rt + rg + 4 q)
        double sH[QFF_RT][4], sW[QFF_RT][4], sA[QFF_RT][4], sB[QFF_RT][4], sT[QFF_RT][4];
#pragma unroll
        for (int rt = 0; rt < QFF_RT; ++rt)
#pragma unroll
            for (int q = 0; q < 4; ++q) { sH[rt][q] = 0.0; sW[rt][q] = 0.0; sA[rt][q] = 0.0; sB[rt][q] = 0.0; sT[rt][q] = 0.0; }

        for (int it = 0; it < njb; ++it) {
            const bool last = it == njb - 1;
            const int jb = last ? jd : (it < jd ? it : it + 1), j = 16 * jb + li;
            const bool jin = j < D;
            d4 acc[QFF_RT];
#pragma unroll
            for (int rt = 0; rt < QFF_RT; ++rt) acc[rt] = (d4){0.0, 0.0, 0.0, 0.0};
            if constexpr (CUBIC) {
                // A[trajectory = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]
                const double *trow = M.cubic + (size_t)i * D * D + j;
                for (int kk = 0; kk < K4; ++kk) {
                    const int k = 4 * kk + rg;
                    const double bv = (jin && k < D) ? trow[(size_t)k * D] : 0.0;
                    const double *xk = xs + k * QFF_LD + li;
#pragma unroll
                    for (int rt = 0; rt < QFF_RT; ++rt)
                        acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(xk[16 * rt], bv, acc[rt], 0, 0, 0);
                }
            }
            const double hij = jin ? M.hess0[i * D + j] : 0.0;
            double aij = 0.0, bij = 0.0, bji = 0.0;
            if constexpr (QUART) {
                if (jin && qa) aij = qa[i * D + j];
                if (jin && qb) { bij = qb[i * D + j]; bji = qb[j * D + i]; }
            }
            const double a8 = 8.0 * aij, b3ij = 3.0 * bij, b3ji = 3.0 * bji;
            double val[QFF_RT][4];
#pragma unroll
            for (int rt = 0; rt < QFF_RT; ++rt)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int b = 16 * rt + rg + 4 * q;
                    const double xj = xs[j * QFF_LD + b], xi = xs[i * QFF_LD + b], yj = xj * xj, yi = xi * xi;
                    const double w = acc[rt][q];
                    sH[rt][q] = fma(hij, xj, sH[rt][q]);
                    if constexpr (CUBIC) sW[rt][q] = fma(w, xj, sW[rt][q]);
                    if constexpr (QUART) {
                        sA[rt][q] = fma(aij, yj, sA[rt][q]);
                        sB[rt][q] = fma(bij, xj, sB[rt][q]);
                        sT[rt][q] = fma(bji, yj * xj, sT[rt][q]);
                    }
                    val[rt][q] = qff_hess_element<QUART>(CUBIC ? hij + w : hij, a8, b3ij, b3ji, xi, xj, yi, yj);
                }
            if constexpr (QUART) {
                if (last) {
                    // the diagonal term 4 (Ay)_i + 6 x_i (Bx)_i: the row sums are complete
#pragma unroll
                    for (int rt = 0; rt < QFF_RT; ++rt)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const double xi = xs[i * QFF_LD + 16 * rt + rg + 4 * q];
                            const double d = row_sum(fma(6.0 * xi, sB[rt][q], 4.0 * sA[rt][q]));
                            if (li == (i & 15)) val[rt][q] += d;
                        }
                }
            }
            if (jin) {
#pragma unroll
                for (int rt = 0; rt < QFF_RT; ++rt)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int64_t t = b0 + 16 * rt + rg + 4 * q;
                        // written once, read by the monodromy kernel after the stage: non-temporal (the cubic tensor stays in L2)
                        if (t < a.n) __builtin_nontemporal_store(val[rt][q], &a.hess[(size_t)t * a.hstride + (size_t)i * D + j]);
                    }
            }
        }
        // gradient and the row's share of the energy
        const double gi = M.grad0[i];
#pragma unroll
        for (int rt = 0; rt < QFF_RT; ++rt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int b = 16 * rt + rg + 4 * q;
                const double xi = xs[i * QFF_LD + b], yi = xi * xi, zi = yi * xi;
                double g = sH[rt][q], e = 0.5 * xi * sH[rt][q];
                if constexpr (CUBIC) { g = fma(0.5, sW[rt][q], g); e = fma((1.0 / 6.0) * xi, sW[rt][q], e); }
                if constexpr (QUART) {
                    g = fma(4.0 * xi, sA[rt][q], g); g = fma(3.0 * yi, sB[rt][q], g); g += sT[rt][q];
                    e = fma(yi, sA[rt][q], e); e = fma(zi, sB[rt][q], e);
                }
                g = row_sum(g); e = row_sum(e);
                if (li == 0) {
                    if (b0 + b < a.n) a.grad[(size_t)(b0 + b) * D + i] = gi + g;
                    ep[wave * QFF_TB + b] += fma(gi, xi, e);
                }
            }
    }
    __syncthreads();
    if (tid < QFF_TB && b0 + tid < a.n)
        a.energy[b0 + tid] = M.energy0 + ((ep[tid] + ep[QFF_TB + tid]) + (ep[2 * QFF_TB + tid] + ep[3 * QFF_TB + tid]));
}

template <bool CUBIC, bool QUART>
int qff_launch_as(const QffArgs &a, hipStream_t s) {
    const size_t lds = qff_lds_bytes(a.M.dim);
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute((const void *)qff_kernel<CUBIC, QUART>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return sc_check_launch("sc_qff (LDS size)");
    const int64_t blocks = (a.n + QFF_TB - 1) / QFF_TB;
    hipLaunchKernelGGL((qff_kernel<CUBIC, QUART>), dim3((unsigned)blocks), dim3(64 * QFF_WAVES), lds, s, a);
    return sc_check_launch("sc_qff");
}

int qff_launch(const QffArgs &a, hipStream_t s) {
    const bool cubic = a.M.cubic != nullptr, quart = a.M.quartic_a != nullptr || a.M.quartic_b != nullptr;
    if (cubic) return quart ? qff_launch_as<true, true>(a, s) : qff_launch_as<true, false>(a, s);
    return quart ? qff_launch_as<false, true>(a, s) : qff_launch_as<false, false>(a, s);
}

int qff_check_model(const sc_qff_model *m, int64_t n, const char *who) {
    if (!m->pos0 || !m->grad0 || !m->hess0) return sc_fail(SC_ERR_BAD_ARGUMENT, "%s: null model array", who);
    if (m->dim < 1 || m->dim > QFF_MAX_DIM)
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: D=%d; the quartic force field kernel holds 1 <= D <= %d", who, m->dim, QFF_MAX_DIM);
    if (n > QFF_MAX_N)
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: n=%lld; at most %lld trajectories per call", who, (long long)n, (long long)QFF_MAX_N);
    return SC_OK;
}

}  // namespace

extern "C" int sc_qff_max_dim(void) { return QFF_MAX_DIM; }
extern "C" int sc_qff_tile(void) { return QFF_TB; }

extern "C" int64_t sc_qff_scratch_bytes(int64_t n, int32_t dim) {
    if (n < 0 || dim < 1 || dim > QFF_MAX_DIM) return -1;
    return 8 * (n * dim + n + n * dim);                    // stage positions [n][D], V [n], grad [n][D]
}

extern "C" int sc_qff_eval(const sc_qff_model *m, const double *r, int64_t n, double *energy, double *grad, double *hess,
                           void *stream) {
    if (!m || !r || !energy || !grad || !hess) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_qff_eval: null argument");
    if (int rc = qff_check_model(m, n, "sc_qff_eval")) return rc;
    if (n <= 0) return SC_OK;
    const QffArgs a{*m, r, n, energy, grad, hess, (int64_t)m->dim * m->dim};
    return qff_launch(a, (hipStream_t)stream);
}

extern "C" int sc_qff_stage(const sc_qff_model *m, double *scratch, const sc_state *st, const sc_dense_scratch *sc, double dt,
                            int32_t stage, double *energy_partials, void *stream) {
    if (!m || !scratch || !st || !sc || !sc->hess || !sc->kprev || !sc->ksum || !sc->ssum || !m->inv_mass)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_qff_stage: null argument");
    if (stage < 0 || stage > 3) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_qff_stage: stage %d", stage);
    if (int rc = qff_check_model(m, st->n, "sc_qff_stage")) return rc;
    if (st->dim != m->dim) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_qff_stage: state of D=%d, model of D=%d", st->dim, m->dim);
    const int64_t n = st->n;
    if (n <= 0) return SC_OK;
    const int D = m->dim;
    hipStream_t s = (hipStream_t)stream;
    double *pos = scratch, *V = pos + n * D, *grad = V + n;
    int rc = sc_stage_point_range(st, sc, dt, stage, pos, 0, n, s);
    if (rc) return rc;
    // the stage Hessian goes straight into the image of sc_dense_mono_step (hess[n][4][D][D]); it is symmetric bit for bit
    const QffArgs a{*m, pos, n, V, grad, sc->hess + (size_t)stage * D * D, (int64_t)4 * D * D};
    rc = qff_launch(a, s);
    if (rc) return rc;
    return sc_stage_consume_range(st, sc, m->inv_mass, V, grad, dt, stage, energy_partials, 0, n, 0, s);
}

// What the two register kernels for a CONSTANT dense Hessian at D <= 16 share (DESIGN.md sections 4.2 and 4.3): hk_step_lin_kernel
// (sc_hk_step_lin.hip, one step per launch) and hk_run_lin_kernel (sc_hk_run_lin.hip, the whole loop in one launch).  One
// trajectory per 16-lane DPP row, lane a holds row a of every matrix (sc_row16.h).  Each piece is written here once and called by
// both, so that the two paths run the same arithmetic in the same order: they agree to rounding, their branch trackers bit for bit.
#pragma once
#include "sc_common.h"
#include "sc_row16.h"

namespace {

// ---- the per-lane constants, staged once per workgroup ----
// doubles: H rows [16][D], Phi rows [16][4 D], per-lane vectors [NV][16]; rows of Re L1, Re L2 [16][D] and Re R1, Re R2 [16][d']
// (dense widths).  A kernel's own constants are the vectors from 5 on and what follows behind n_doubles.
// Row pitches: every lane of a 16-lane row reads ITS row of a constant, so the pitch decides the LDS banks the lanes meet on.
// Unpadded, Phi's rows (4 D doubles = 96 dwords at D = 12) put all lanes on one bank: a 12-way conflict on every read of the
// product loop, 87 % of the step kernel's LDS cycles (SQ_LDS_BANK_CONFLICT).  One double more per row spreads the lanes over the
// banks.
// L1, L2, R1, R2 are REAL here: they are products of U and real symmetric square roots of the positive semi-definite width
// matrices; the reference carries them as complex128 with imaginary parts that are zero or rounding dust (1e-24 for methylium).
// sc_hk_consts.real_lr says so (lin16_dispatch); widths with genuinely complex roots take the LDS kernel.
template <int D, int DP, bool DIAG, int NV = 8>
struct Lin16Consts {
    static constexpr int PH = D + 1, PP = 4 * D + 1, PL = D + 1, PR = DP + 1;
    static constexpr int n_doubles = 16 * PH + 16 * PP + NV * 16 + (DIAG ? 0 : 2 * 16 * PL + 2 * 16 * PR);
    double *sH;                          // row a: H[a][:]
    double *sPhi;                        // row a: Phi_qq[a][:], Phi_qp[a][:], Phi_pq[a][:], Phi_pp[a][:]; MODAL: (phi_qq, phi_qp, phi_pq, phi_pp)_a
    double *svec;                        // x0, g0, 1/m, st, 1/st; vectors 5 .. NV - 1 are the kernel's
    double *sL1, *sL2, *sR1, *sR2;       // rows i < d' of Re L1, Re L2; rows b < D of Re R1, Re R2 (dense widths)

    __device__ __forceinline__ explicit Lin16Consts(double *ls)
        : sH(ls), sPhi(sH + 16 * PH), svec(sPhi + 16 * PP), sL1(svec + NV * 16), sL2(sL1 + (DIAG ? 0 : 16 * PL)),
          sR1(sL2 + (DIAG ? 0 : 16 * PL)), sR2(sR1 + (DIAG ? 0 : 16 * PR)) {}

    // Phi = A.pot.lin_prop (absent in a prefactor-only launch: zeros).  The caller's barrier follows.  hk_run_lin_kernel keeps this
    // loop written out, fused with the staging of its own rows and vectors (and of the per-mode step matrices in Phi's place): see there.
    __device__ __forceinline__ void stage(const StepArgs &A, int tid) const {
        constexpr int W = 2 * D;
        for (int e = tid; e < 16 * D; e += 256) {
            const int i = e / D, b = e - i * D;
            sH[i * PH + b] = i < D ? A.pot.par2[i * D + b] : 0.0;
            if (!DIAG) {
                sL1[i * PL + b] = i < DP ? A.hk.L1[2 * (i * D + b)] : 0.0;          // real parts of the interleaved complex arrays
                sL2[i * PL + b] = i < DP ? A.hk.L2[2 * (i * D + b)] : 0.0;
            }
        }
        if (!DIAG) {
            for (int e = tid; e < 16 * DP; e += 256) {
                const int i = e / DP, j = e - i * DP;
                sR1[i * PR + j] = i < D ? A.hk.R1[2 * (i * DP + j)] : 0.0;
                sR2[i * PR + j] = i < D ? A.hk.R2[2 * (i * DP + j)] : 0.0;
            }
        }
        for (int e = tid; e < 16 * 4 * D; e += 256) {
            const int i = e / (4 * D), k = e - i * 4 * D, blk = k / D, g = k - blk * D;      // blk: qq, qp, pq, pp
            const int row = (blk >> 1) * D + i, col = (blk & 1) * D + g;
            sPhi[i * PP + k] = (i < D && A.pot.lin_prop) ? A.pot.lin_prop[row * W + col] : 0.0;
        }
        if (tid < 16) {
            const bool in = tid < D;
            svec[tid] = in ? A.pot.par0[tid] : 0.0;
            svec[16 + tid] = in ? A.pot.par1[tid] : 0.0;
            svec[32 + tid] = in ? A.pot.inv_mass[tid] : 0.0;
            const double st = (DIAG && in) ? A.hk.st[tid] : 1.0;
            svec[48 + tid] = st; svec[64 + tid] = 1.0 / st;
        }
    }
};

// ---- (q, p, S): the explicit RK4 stages for lane r (V = E0 + g.dr + 1/2 dr.H.dr - origin, grad = g + H.dr) ----
// hrow_lds: row r of H in LDS; hh, h6: dt / 2, dt / 6.  Advances q, p of the lanes r < D; out: the lane's shares red5 of T - V at
// the four stages and of T + V at the last.
template <int D>
__device__ __forceinline__ void lin_rk4_row(const double *hrow_lds, int r, double x0, double g0, double im, double dt, double hh,
                                            double h6, double &q, double &p, double (&red5)[5]) {
    double qs = q, ps = p, kqs = 0.0, kps = 0.0, qn = 0.0, pn = 0.0;
#pragma unroll
    for (int s = 0; s < 5; ++s) red5[s] = 0.0;
    double hrow[D];
#pragma unroll
    for (int b = 0; b < D; ++b) hrow[b] = hrow_lds[b];
    sfor<0, 4>([&](auto sc_) {
        constexpr int s = decltype(sc_)::value;
        if (s > 0) { const double c = (s == 3) ? dt : hh; qs = q + c * kqs; ps = p + c * kps; }
        double dr = r < D ? qs - x0 : 0.0;
        double hd = 0.0, hd2 = 0.0;         // two chains: consecutive multiply-adds do not wait for each other
        dpp_guard(dr);
        sfor<0, D>([&](auto bc_) {
            constexpr int b = decltype(bc_)::value;
            if (b & 1) fmac_bc<b>(hd2, dr, hrow[b]); else fmac_bc<b>(hd, dr, hrow[b]);
        });
        hd += hd2;
        const double v = dr * g0 + 0.5 * dr * hd;           // + scalar0 after the reduction
        const double kq = ps * im, kp = -(g0 + hd), t = 0.5 * ps * ps * im;
        red5[s] = t - v;
        if (s == 3) red5[4] = t + v;
        const double w = (s == 0 || s == 3) ? 1.0 : 2.0;
        qn += w * kq; pn += w * kp;
        kqs = kq; kps = kp;
    });
    if (r < D) { q = q + h6 * qn; p = p + h6 * pn; }
}
// ... and their sums over the lanes k < D (fused broadcast multiply-adds with `one`, 1.0 in a register the compiler cannot fold)
template <int D>
__device__ __forceinline__ void lin_rk4_sums(double (&red5)[5], const double &one, double scalar0) {
    sum_rows<D>(red5, one);
#pragma unroll
    for (int s = 0; s < 4; ++s) red5[s] -= scalar0;
    red5[4] += scalar0;
}

// ---- [X; Y] <- Phi [X; Y], one half (Mqq, Mpq | Mqp, Mpp): column c of the result needs column c of the old blocks only ----
// Row g of the old blocks (Tq, Tp) comes from lane g inside the multiply-add, Phi[r][g] from LDS (phi_lds: row r of sPhi).
template <int D>
__device__ __forceinline__ void lin_phi_half(const double *phi_lds, double (&Tq)[D], double (&Tp)[D], double (&Xq)[D], double (&Xp)[D]) {
#pragma unroll
    for (int b = 0; b < D; ++b) { Xq[b] = 0.0; Xp[b] = 0.0; }
    dpp_guard(Tq, Tp);
    sfor<0, D>([&](auto gc) {
        constexpr int g = decltype(gc)::value;
        const double fqq = phi_lds[g], fqp = phi_lds[D + g], fpq = phi_lds[2 * D + g], fpp = phi_lds[3 * D + g];
        // X[r][b] += Phi[r][g] * old[g][b]
#pragma unroll
        for (int b = 0; b < D; ++b) { fmac_bc<g>(Xq[b], Tq[b], fqq); fmac_bc<g>(Xp[b], Tq[b], fpq); }
#pragma unroll
        for (int b = 0; b < D; ++b) { fmac_bc<g>(Xq[b], Tp[b], fqp); fmac_bc<g>(Xp[b], Tp[b], fpp); }
    });
}

// ---- the prefactor, accumulated HALF by half of the monodromy rows (h = 0: columns of [Mqq; Mpq], h = 1: of [Mqp; Mpp]) ----
// diagonal widths: mat_ab = 1/2 [st_a/si_b Mqq + si_b/st_a Mpp - i hbar st_a si_b Mqp + i/hbar Mpq/(st_a si_b)]  (:969-986)
// dense widths:    X1 = Mqq R1 - i hbar Mqp R2, X2 = Mpp R2 + i/hbar Mpq R1 (row r; rows b of R1, R2 come from lane b);
//                  mat' = 1/2 (L1 X1 + L2 X2): rows of X1, X2 from lane a, L1[i][a], L2[i][a] from LDS        (:969-994)
// The sums of dense widths: s1 = Mqq R1, s2 = Mqp R2, t1 = Mpp R2, t2 = Mpq R1 (real: R1, R2 are); diagonal widths: unused.
template <int DP, bool DIAG>
struct Lin16Sums {
    static constexpr int NS = DIAG ? 1 : DP;
    double s1[NS], s2[NS], t1[NS], t2[NS];
};
// element b of the lane's row for diagonal widths (in: r < D): h = 0 sets it from (Mqq, Mpq), h = 1 adds the share of (Mqp, Mpp)
template <int h>
__device__ __forceinline__ void lin_diag_element(cplx &m, bool in, double sib, double sta, double ista, double xq, double xp) {
    const double isib = 1.0 / sib;
    if (h == 0) m = in ? c_make(0.5 * (sta * isib * xq), 0.5 * ((1.0 / SC_HBAR) * ista * isib * xp)) : c_make(0.0, 0.0);
    else m = in ? c_make(m.x + 0.5 * (ista * sib * xp), m.y + 0.5 * (-SC_HBAR * sta * sib * xq)) : c_make(0.0, 0.0);
}
// Xq, Xp: the lane's rows of the half's q and p block; rrow_lds: row r of R1 (h = 0) or R2 (h = 1) in LDS
template <int D, int DP, bool DIAG, int h, int N>
__device__ __forceinline__ void lin_prefactor_half(cplx (&mat)[N], Lin16Sums<DP, DIAG> &u, const double *rrow_lds, kptr ksi,
                                                   double sta, double ista, int r, const double (&Xq)[D], const double (&Xp)[D]) {
    if constexpr (DIAG) {
        WM_BLOCK {
#pragma unroll
            for (int b = 0; b < D; ++b) lin_diag_element<h>(mat[b], r < D, ksi[b], sta, ista, Xq[b], Xp[b]);
        }
    } else {
        double rr[DP];
        double (&uq)[DP] = h ? u.s2 : u.s1, (&up)[DP] = h ? u.t1 : u.t2;
#pragma unroll
        for (int j = 0; j < DP; ++j) { rr[j] = rrow_lds[j]; uq[j] = 0.0; up[j] = 0.0; }
        dpp_guard(rr);
        sfor<0, D>([&](auto bcn) {
            constexpr int b = decltype(bcn)::value;
#pragma unroll
            for (int j = 0; j < DP; ++j) { fmac_bc<b>(uq[j], rr[j], Xq[b]); fmac_bc<b>(up[j], rr[j], Xp[b]); }
        });
    }
}
// dense widths, after both halves: mat = 1/2 (L1 X1 + L2 X2); l1_lds, l2_lds: row r of L1 and of L2 in LDS
template <int D, int DP>
__device__ __forceinline__ void lin_sandwich(cplx (&mat)[DP], const Lin16Sums<DP, false> &u, const double *l1_lds, const double *l2_lds) {
    cplx X1[DP], X2[DP];
#pragma unroll
    for (int j = 0; j < DP; ++j) {
        X1[j] = c_make(u.s1[j], -SC_HBAR * u.s2[j]);                 // Mqq R1 - i hbar Mqp R2
        X2[j] = c_make(u.t1[j], (1.0 / SC_HBAR) * u.t2[j]);          // Mpp R2 + i/hbar Mpq R1
    }
#pragma unroll
    for (int j = 0; j < DP; ++j) mat[j] = c_make(0.0, 0.0);
    dpp_guard(X1, X2);
    sfor<0, D>([&](auto ac) {
        constexpr int a = decltype(ac)::value;
        const double l1 = l1_lds[a], l2 = l2_lds[a];
#pragma unroll
        for (int j = 0; j < DP; ++j) { fmac_bc<a>(mat[j].x, X1[j].x, l1); fmac_bc<a>(mat[j].y, X1[j].y, l1); }
#pragma unroll
        for (int j = 0; j < DP; ++j) { fmac_bc<a>(mat[j].x, X2[j].x, l2); fmac_bc<a>(mat[j].y, X2[j].y, l2); }
    });
#pragma unroll
    for (int j = 0; j < DP; ++j) mat[j] = c_scale(mat[j], 0.5);
}

// ---- lane r's rows of a trajectory's monodromy blocks M (row-major Mqq, Mqp, Mpq, Mpp), straight from and to memory ----
// half h: row r of the q block (Mqq | Mqp) and of the p block (Mpq | Mpp); lanes r >= D hold zeros
template <int D>
__device__ __forceinline__ void lin_load_half(const double *M, int r, int h, double (&Xq)[D], double (&Xp)[D]) {
#pragma unroll
    for (int b = 0; b < D; ++b) {
        Xq[b] = r < D ? M[(h ? D * D : 0) + r * D + b] : 0.0;
        Xp[b] = r < D ? M[(h ? D * D : 0) + 2 * D * D + r * D + b] : 0.0;
    }
}
// for a lane r < D
template <int D>
__device__ __forceinline__ void lin_store_half(double *M, int r, int h, const double (&Xq)[D], const double (&Xp)[D]) {
#pragma unroll
    for (int b = 0; b < D; ++b) {
        M[(h ? D * D : 0) + r * D + b] = Xq[b];
        M[(h ? D * D : 0) + 2 * D * D + r * D + b] = Xp[b];
    }
}

// ---- the instantiated shapes (host) ----
// whole_loop: hk_run_lin_kernel has the shape too (it keeps a trajectory's 4 D registers of monodromy rows across the steps: not D = 15)
struct Lin16Shape { int D, dp; bool diag, whole_loop; };
constexpr Lin16Shape lin16_shapes[] = {
    {12, 6, false, true}, {12, 12, true, true}, {9, 3, false, true}, {9, 9, true, true}, {6, 6, true, true}, {6, 6, false, true},
    {3, 3, true, true},
    // further molecular shapes (D = 3 N Cartesian coordinates, d' = D - 6, or D - 5 for a linear molecule)
    {6, 1, false, true}, {9, 4, false, true}, {12, 7, false, true}, {15, 9, false, false}, {15, 15, true, false}};

// launch(D, d', diagonal widths), as integral constants, of the shape (D, hk.dprime, hk.diag) if it is instantiated (for the
// whole-loop kernel: WHOLE_LOOP) and its result; 0 if not, or if L, R are genuinely complex (indefinite rounding in the widths)
template <bool WHOLE_LOOP, size_t I = 0, class F>
int lin16_dispatch(const sc_hk_consts &hk, int D, F &&launch) {
    if constexpr (I < sizeof(lin16_shapes) / sizeof(lin16_shapes[0])) {
        constexpr Lin16Shape s = lin16_shapes[I];
        if (!hk.diag && !hk.real_lr) return 0;
        if constexpr (!WHOLE_LOOP || s.whole_loop)
            if (D == s.D && hk.dprime == s.dp && (hk.diag != 0) == s.diag)
                return launch(std::integral_constant<int, s.D>{}, std::integral_constant<int, s.dp>{}, std::integral_constant<bool, s.diag>{});
        return lin16_dispatch<WHOLE_LOOP, I + 1>(hk, D, launch);
    }
    return 0;
}

}  // namespace

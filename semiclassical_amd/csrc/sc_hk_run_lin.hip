// The caller loop of the reference (cli.py:401-436: autocorrelation, ic_correlation, step -- nt times) as ONE launch for a
// CONSTANT dense Hessian (MolecularHarmonicPotential, potentials.py:553-593) and small matrices (D <= 16): the methylium
// example of the reference (12 Cartesian coordinates, rank-6 widths) with the Herman-Kluk propagator.
//
// Step by step this loop is hk_correlate_rows16_kernel + reduce + hk_step_lin_kernel + guard per time step, and the step
// kernel is bound by reading and writing the 4 D^2 monodromy doubles of every trajectory (9.6 KB at D = 12) each step.
// Here a trajectory is loaded ONCE into the registers of its 16-lane row -- lane a holds row a of the four monodromy blocks
// (96 registers at D = 12), q_a, p_a -- runs all nsteps steps there and is written back once; per step only five partial
// sums per wavefront leave the chip (the scheme of sc_hk_run_sep16.hip).  This file holds the
// kernel and its launcher; the entry points, the checks and the reductions are in sc_hk_run.hip.
//
// Per step and trajectory, in the order of the caller loop, with the arithmetic (and operation order) of the step-at-a-time
// kernels, so that both paths agree to rounding -- what it shares with hk_step_lin_kernel is written once, in sc_lin16.h:
//   terms of C_auto, k_ic from the CURRENT state    hk_correlate_rows16_kernel: y = A dq, B dp, C dp as fused broadcast
//                                                   multiply-adds, sums over the modes (sum_rows, sc_row16.h), then the scalar
//                                                   tail every route calls (sc_common.h: overlap_value ... corr_k_term)   (:784-911)
//   RK4 stages of (q, p), action, <T+V> at k4       hk_step_lin_kernel                                 (:86-119, 313-383)
//   [X; Y] <- Phi(dt) [X; Y]                        one product with the step matrix (sc_potential.lin_prop), half by half
//   prefactor matrix, determinant, branch tracker   real sandwiches L (M R) (sc_hk_consts.real_lr), fixed pivot order; a weak
//                                                   pivot repeats the elimination with the pivot searched among the lanes
//                                                   (the rows are still in registers)                  (:969-1052)
#include "sc_hk_run.h"
#include "sc_lin16.h"

namespace {

// LDS: the constants of both constant-Hessian kernels (sc_lin16.h) with this kernel's per-lane vectors among them (qk, pk, nq0, np0,
// nrn, ngn, -), then the overlap rows A, B, C at the odd pitch D + 1
template <int D, int DP, bool DIAG> using RunLinConsts = Lin16Consts<D, DP, DIAG, 12>;

#ifndef SC_RUNLIN_OCC
#define SC_RUNLIN_OCC 2
#endif
#ifndef SC_RUNLIN_MODAL_OCC
#define SC_RUNLIN_MODAL_OCC 2
#endif
// MODAL (round 4, sc_hk_run_modal): the monodromy blocks of the state are in NORMAL-MODE coordinates (the caller transformed them and
// the prefactor constants), where the step matrix is 2 x 2 per mode: row a of the blocks is multiplied by (phi_qq, phi_qp; phi_pq,
// phi_pp)_a -- 8 D plain multiply-adds per lane and step instead of the 8 D^2 broadcast multiply-adds of the product with Phi.
template <int D, int DP, bool DIAG, bool MODAL, bool MOM>
__global__ __launch_bounds__(256, MODAL ? SC_RUNLIN_MODAL_OCC : SC_RUNLIN_OCC) void hk_run_lin_kernel(RunArgs R) {
    typedef RunLinConsts<D, DP, DIAG> L;
    constexpr int DD = D * D, N = DIAG ? D : DP, PD = D + 1;
    extern __shared__ double2 smem2[];
    const StepArgs &A = R.step;
    const int tid = threadIdx.x, lane = tid & 63, r = tid & 15, grp = tid >> 4, wave = tid >> 6, rowbase = tid & 48;
    const double dt = A.dt, hh = 0.5 * dt, h6 = dt / 6.0;
    const bool nac = R.has_nac != 0;

    const L C((double *)smem2);
    constexpr int W = 2 * D, PH = L::PH, PP = L::PP, PL = L::PL, PR = L::PR;
    double *sH = C.sH, *sPhi = C.sPhi, *svec = C.svec, *sL1 = C.sL1, *sL2 = C.sL2, *sR1 = C.sR1, *sR2 = C.sR2;
    double *sOA = (double *)smem2 + L::n_doubles, *sOB = sOA + 16 * PD, *sOC = sOB + 16 * PD;
    // (Lin16Consts::stage written out, fused with the own rows: as a call <12, 7, false, false> spills 93 VGPRs; 62 before sc_lin16.h, 41 as built)
    for (int e = tid; e < 16 * D; e += 256) {
        const int i = e / D, b = e - i * D;
        const bool in = i < D;
        sH[i * PH + b] = in ? A.pot.par2[i * D + b] : 0.0;
        if (!DIAG) {
            sL1[i * PL + b] = i < DP ? A.hk.L1[2 * (i * D + b)] : 0.0;          // real parts (sc_hk_consts.real_lr)
            sL2[i * PL + b] = i < DP ? A.hk.L2[2 * (i * D + b)] : 0.0;
        }
        // overlap matrices: dense rows, or the diagonal spread into rows of zeros
        if (R.oc.diag) {
            sOA[i * PD + b] = (in && i == b) ? R.oc.A[i] : 0.0;
            sOB[i * PD + b] = (in && i == b) ? R.oc.B[i] : 0.0;
            sOC[i * PD + b] = (in && i == b) ? R.oc.C[i] : 0.0;
        } else {
            sOA[i * PD + b] = in ? R.oc.A[i * D + b] : 0.0;
            sOB[i * PD + b] = in ? R.oc.B[i * D + b] : 0.0;
            sOC[i * PD + b] = in ? R.oc.C[i * D + b] : 0.0;
        }
    }
    if (!DIAG) {
        for (int e = tid; e < 16 * DP; e += 256) {
            const int i = e / DP, j = e - i * DP;
            sR1[i * PR + j] = i < D ? A.hk.R1[2 * (i * DP + j)] : 0.0;
            sR2[i * PR + j] = i < D ? A.hk.R2[2 * (i * DP + j)] : 0.0;
        }
    }
    if (MODAL) {
        for (int e = tid; e < 16 * 4; e += 256) {
            const int i = e >> 2, k = e & 3;                                              // (phi_qq, phi_qp, phi_pq, phi_pp) of mode i
            sPhi[i * PP + k] = i < D ? R.mode_prop[i * 4 + k] : (k == 0 || k == 3 ? 1.0 : 0.0);
        }
    } else {
        for (int e = tid; e < 16 * 4 * D; e += 256) {
            const int i = e / (4 * D), k = e - i * 4 * D, blk = k / D, g = k - blk * D;      // blk: qq, qp, pq, pp
            const int row = (blk >> 1) * D + i, col = (blk & 1) * D + g;
            sPhi[i * PP + k] = i < D ? A.pot.lin_prop[row * W + col] : 0.0;
        }
    }
    if (tid < 16) {
        const bool in = tid < D;
        svec[tid] = in ? A.pot.par0[tid] : 0.0;
        svec[16 + tid] = in ? A.pot.par1[tid] : 0.0;
        svec[32 + tid] = in ? A.pot.inv_mass[tid] : 0.0;
        const double st = (DIAG && in) ? A.hk.st[tid] : 1.0;
        svec[48 + tid] = st; svec[64 + tid] = 1.0 / st;
        svec[80 + tid] = in ? R.oc.qk[tid] : 0.0;
        svec[96 + tid] = in ? R.oc.pk[tid] : 0.0;
        svec[112 + tid] = (in && nac) ? R.nc.q0[tid] : 0.0;
        svec[128 + tid] = (in && nac) ? R.nc.p0[tid] : 0.0;
        svec[144 + tid] = (in && nac) ? R.nc.rn[tid] : 0.0;
        svec[160 + tid] = (in && nac) ? R.nc.gn[tid] : 0.0;
    }
    __syncthreads();
    const double x0 = svec[r], g0 = svec[16 + r], im = svec[32 + r], sta = svec[48 + r], ista = svec[64 + r];
    const double qk = svec[80 + r], pk = svec[96 + r];
    kptr ksi = (kptr)A.hk.si;

    const int64_t n = A.st.n, stride = (int64_t)gridDim.x * 16;
    const int slot = blockIdx.x * 4 + wave;
    double one = 1.0;
    asm volatile("" : "+v"(one));

    for (int64_t t0 = (int64_t)blockIdx.x * 16; t0 < n; t0 += stride) {
        const bool active = t0 + grp < n, head = active && r == 0;
        const int64_t tr = active ? t0 + grp : n - 1;          // idle rows shadow the last trajectory and contribute nothing
        double *M = A.st.mono + tr * 4 * (int64_t)DD, *qp = A.st.qp + tr * 2 * D;
        // ---- the trajectory: rows of the four blocks as [half][q | p block][column]: half 0 = (Mqq, Mpq), half 1 = (Mqp, Mpp)
        double cur[2][2][D];
        // (load and write-back written out: through lin_load_half / lin_store_half <12, 7, false, false> spills 93 VGPRs; 62 before, 41 as built)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int b = 0; b < D; ++b) {
                cur[h][0][b] = r < D ? M[(h ? DD : 0) + r * D + b] : 0.0;
                cur[h][1][b] = r < D ? M[(h ? DD : 0) + 2 * DD + r * D + b] : 0.0;
            }
        double q = r < D ? qp[r] : 0.0, p = r < D ? qp[D + r] : 0.0;
        double S = A.st.act[tr], sgn = A.st.sgn[tr];
        cplx c2 = ((const cplx *)A.st.c2)[tr];
        const cplx vi = ((const cplx *)R.vi)[tr];
        const cplx nacq = nac ? ((const cplx *)R.nacq)[tr] : c_make(0.0, 0.0);
        const double wgt = 1.0 / (R.mc_norm * R.probi[tr]);

        for (int k = 0; k < R.nsteps; ++k) {
            int lofs = 0;
            asm volatile("" : "+v"(lofs));         // the per-lane constants are re-read from LDS every step, never kept across steps
            const double *cH = sH + lofs + r * PH, *cPhi = sPhi + lofs + r * PP, *cv = svec + lofs;     // the lane's rows of the constants
            double v5[5];
            // ---- terms of the correlation functions from the current state (hk_correlate_rows16_kernel) ----
            {
                const double *cA = sOA + lofs + r * PD, *cB = sOB + lofs + r * PD, *cC = sOC + lofs + r * PD;
                double dq = qk - q, dpp = pk - p;
                if (r >= D) { dq = 0.0; dpp = 0.0; }
                double ya = 0.0, yb = 0.0, yc = 0.0;
                dpp_guard(dq, dpp);
                // one matrix after the other (a row of constants is 2 D registers, and 4 D^2 / 16 * 2 are taken by the trajectory)
                auto times_row = [&](double &y, const double &x, const double *row) {
                    double rw[D];
#pragma unroll
                    for (int b = 0; b < D; ++b) rw[b] = row[b];
                    sfor<0, D>([&](auto bcn) { fmac_bc<decltype(bcn)::value>(y, x, rw[decltype(bcn)::value]); });
                };
                times_row(ya, dq, cA); times_row(yb, dpp, cB); times_row(yc, dpp, cC);
                const double nq0 = cv[112 + r], np0 = cv[128 + r], nrn = cv[144 + r], ngn = cv[160 + r];
                double s[6] = {dq * ya, dpp * yb, pk * dq, dq * yc, (nq0 - q) * nrn, (p - np0) * ngn};
                sum_rows<D>(s, one);
                const cplx cvt = overlap_value_conj(R.oc.fac, s[0], s[1], s[2], s[3]);
                const cplx cq = corr_c_term(cvt, vi, signed_root(c2, sgn), action_phase(S), wgt);
                v5[0] = cq.x; v5[1] = cq.y; v5[2] = 0.0; v5[3] = 0.0;
                if (nac) {
                    const cplx kq = corr_k_term(R.nc.n2, R.nc.p0n1, s[4], s[5], nacq, cq);
                    v5[2] = kq.x; v5[3] = kq.y;
                }
            }
            // ---- (q, p, S): the explicit RK4 stages (lin_rk4_row) ----
            {
                double red5[5];
                lin_rk4_row<D>(cH, r, x0, g0, im, dt, hh, h6, q, p, red5);
                lin_rk4_sums<D>(red5, one, A.pot.scalar0);
                S = S + h6 * (red5[0] + 2.0 * red5[1] + 2.0 * red5[2] + red5[3]);
                v5[4] = red5[4];
            }
            // ---- [X; Y] <- Phi [X; Y], one half (Mqq, Mpq | Mqp, Mpp) at a time (lin_phi_half); MODAL: 2 x 2 per mode ----
            if constexpr (MODAL) {
                const double fqq = cPhi[0], fqp = cPhi[1], fpq = cPhi[2], fpp = cPhi[3];
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int b = 0; b < D; ++b) {
                        const double tq = cur[h][0][b], tp = cur[h][1][b];
                        cur[h][0][b] = fma(fqp, tp, fqq * tq);
                        cur[h][1][b] = fma(fpp, tp, fpq * tq);
                    }
            } else
            sfor<0, 2>([&](auto hc) {
                constexpr int h = decltype(hc)::value;
                double (&Tq)[D] = cur[h][0], (&Tp)[D] = cur[h][1];
                double Xq[D], Xp[D];
                lin_phi_half<D>(cPhi, Tq, Tp, Xq, Xp);
#pragma unroll
                for (int b = 0; b < D; ++b) { Tq[b] = Xq[b]; Tp[b] = Xp[b]; }
            });
            // ---- prefactor matrix from the new rows (lin_prefactor_half, lin_sandwich) ----
            cplx mat[N];
            auto build_mat = [&]() {
                if constexpr (DIAG) {
                    // (both halves of an element together: in two passes of lin_prefactor_half <12, 12, true> takes 324 B of scratch; 232 before, 200 as built)
#pragma unroll
                    for (int b = 0; b < D; ++b) {
                        const double sib = ksi[b];
                        lin_diag_element<0>(mat[b], r < D, sib, sta, ista, cur[0][0][b], cur[0][1][b]);
                        lin_diag_element<1>(mat[b], r < D, sib, sta, ista, cur[1][0][b], cur[1][1][b]);
                    }
                } else {
                    Lin16Sums<DP, DIAG> sums;
                    sfor<0, 2>([&](auto hc) {
                        constexpr int h = decltype(hc)::value;
                        lin_prefactor_half<D, DP, DIAG, h>(mat, sums, (h ? sR2 : sR1) + lofs + r * PR, ksi, sta, ista, r, cur[h][0], cur[h][1]);
                    });
                    lin_sandwich<D, DP>(mat, sums, sL1 + lofs + r * PL, sL2 + lofs + r * PL);
                }
            };
            build_mat();
            int weak = 0;
            cplx det = det_rows_fixed_order<N>(mat, r, weak);
            if (__builtin_amdgcn_readfirstlane(wave_max_i32(weak)) != 0) {
                // a trajectory of this wavefront met a weak pivot: its determinant by elimination with the pivot searched among
                // the lanes (what the fix-up launch of the step-at-a-time path does), from the rows that are still here
                build_mat();
                int myk, src;
                cplx det2, dummy[1] = {c_make(0.0, 0.0)};
                gauss_jordan_rows<N, 1>(mat, dummy, r >= N, r, rowbase, myk, src, det2);
                if (weak) det = det2;
            }
            if (crossed_branch_cut(c2, det)) sgn = -sgn;       // branch tracker (propagators.py:1045-1047)
            c2 = det;
            // ---- this wavefront's share of step k: one writer per slot ----
            if constexpr (MOM) run_moments_share<MOM>(R, v5, head, k, slot, lane);
            // (the hand-over is written out in both whole-loop kernels: as a shared function it moves hk_run_lin_kernel's registers)
#pragma unroll
            for (int i = 0; i < 5; ++i) v5[i] = wave_sum(head ? v5[i] : 0.0);
            if (lane == 0) {
                double *pp = R.partials + ((size_t)k * R.slots + slot) * 5;
#pragma unroll
                for (int i = 0; i < 5; ++i) __builtin_amdgcn_global_atomic_fadd_f64((__attribute__((address_space(1))) double *)(pp + i), v5[i]);
            }
        }
        // ---- the trajectory goes back
        if (active) {
            if (r < D) {
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int b = 0; b < D; ++b) {
                        M[(h ? DD : 0) + r * D + b] = cur[h][0][b];
                        M[(h ? DD : 0) + 2 * DD + r * D + b] = cur[h][1][b];
                    }
                qp[r] = q; qp[D + r] = p;
            }
            if (r == 0) {
                A.st.act[tr] = S; A.st.sgn[tr] = sgn;
                ((cplx *)A.st.c2)[tr] = c2;
            }
        }
    }
}

template <int D, int DP, bool DIAG, bool MODAL, bool MOM>
int launch_one(const RunArgs &a, int grid, hipStream_t s) {
    const size_t lds = (size_t)(RunLinConsts<D, DP, DIAG>::n_doubles + 3 * 16 * (D + 1)) * 8;
    if (hipFuncSetAttribute((const void *)hk_run_lin_kernel<D, DP, DIAG, MODAL, MOM>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess)
        return sc_check_launch("sc_hk_run (LDS attribute)");
    hipLaunchKernelGGL((hk_run_lin_kernel<D, DP, DIAG, MODAL, MOM>), dim3(grid), dim3(256), lds, s, a);
    const int rc = sc_check_launch("sc_hk_run (constant-Hessian whole-loop kernel)");
    return rc == SC_OK ? 1 : rc;
}

// this file is compiled twice: on its own with the kernels of sc_hk_run (MOM = false), and included by sc_hk_run_lin_m.hip with
// SC_RUN_MOMENTS_TU defined for those of sc_hk_run_m (MOM = true) -- a translation unit of their own, so that the instantiations
// without moments are compiled exactly as before
#ifdef SC_RUN_MOMENTS_TU
#define SC_RUNLIN_MOM true
#define SC_RUNLIN_ENTRY sc_launch_run_lin_m
#else
#define SC_RUNLIN_MOM false
#define SC_RUNLIN_ENTRY sc_launch_run_lin_plain
#endif
template <int D, int DP, bool DIAG>
int launch(const RunArgs &a, int grid, hipStream_t s, int do_launch) {
    if (a.mode_prop) {
        if constexpr (DIAG) return 0;            // the transformed prefactor constants are dense: no modal kernel for diagonal widths
        else return do_launch ? launch_one<D, DP, DIAG, true, SC_RUNLIN_MOM>(a, grid, s) : 1;
    }
    return do_launch ? launch_one<D, DP, DIAG, false, SC_RUNLIN_MOM>(a, grid, s) : 1;
}

}  // namespace

int SC_RUNLIN_ENTRY(const RunArgs &a, int grid, hipStream_t s, int do_launch) {
    return lin16_dispatch<true>(a.step.hk, a.step.st.dim, [&](auto d, auto dp, auto diag) {
        return launch<decltype(d)::value, decltype(dp)::value, decltype(diag)::value>(a, grid, s, do_launch);
    });
}

#ifndef SC_RUN_MOMENTS_TU
int sc_launch_run_lin(const RunArgs &a, int grid, hipStream_t s, int do_launch, bool moments) {
    return moments && do_launch ? sc_launch_run_lin_m(a, grid, s, do_launch) : sc_launch_run_lin_plain(a, grid, s, do_launch);
}
#endif

// The caller loop of the reference (cli.py:401-436: autocorrelation, ic_correlation, step -- nt times) as ONE launch, for
// SEPARABLE potentials with diagonal width matrices and D <= 12 (BASELINE.json configs[0]: the 5-mode anharmonic AS model).
//
// Step by step the loop is six launches per time step (correlate, reduce, step, guard, ...): at n = 1000 the kernels need
// 12 us of a 33 us step, and replaying the sequence from a HIP graph is no faster than issuing it.  Here a trajectory is
// loaded ONCE into the registers of its 16-lane row (the layout of hk_step_sep16_kernel: lane a holds mode a and row a of
// the four monodromy blocks), runs all nsteps steps there and is written back once; between steps nothing touches HBM
// but the five partial sums of the step.  Trajectories are independent, so there is no grid-wide synchronisation: every
// wavefront adds its four trajectories' terms of step k into its own slot partials[k][slot] (one writer per slot: the
// sums are deterministic), and hk_run_reduce_kernel (sc_hk_run.hip) adds the slots of a step in a fixed order afterwards.  This file holds the kernel and its launcher; the entry points, the checks and the reductions that serve both
// whole-loop kernels are in sc_hk_run.hip.
//
// Per step and trajectory, in this order (= the order of the caller loop):
//   terms of C_auto and k_ic from the CURRENT state       overlap_sums_diag, nac_sums, overlap_value_conj, signed_root, action_phase,
//                                                         corr_c_term, corr_k_term (sc_common.h: the functions
//                                                         hk_correlate_kernel calls), sums over the modes by a rotate-and-add
//                                                         tree (propagators.py:784-843, 845-911)
//   RK4 of (q_a, p_a), action, <T+V> at the k4 stage,     sep_mode_rk4, sep_row_propagator, sep_propagate_row (sc_common.h: the
//   row propagators P_a applied to the monodromy rows     functions hk_step_sep16_kernel calls; propagators.py:86-119, 313-383)
//   prefactor row, determinant, branch tracker            prefactor_element_diag, crossed_branch_cut (sc_common.h);
//                                                         fixed pivot order; a weak pivot (never for the diagonal blocks a
//                                                         separable potential produces from M(0) = 1) repeats the
//                                                         elimination with the pivot searched among the lanes
//                                                         (propagators.py:969-1052)
#include "sc_hk_run.h"
#include "sc_row16.h"

namespace {

// value of `v` in lane 0 of each 16-lane row, summed over the four rows of the wavefront (result in every lane)
__device__ __forceinline__ double sum_row_heads(double v, bool head) { return wave_sum(head ? v : 0.0); }

#ifndef SC_RUN_OCC
#define SC_RUN_OCC 2
#endif
template <int DP, int KIND, bool MOM>
__global__ __launch_bounds__(256, SC_RUN_OCC) void hk_run_sep16_kernel(RunArgs R) {
    const StepArgs &A = R.step;
    const int D = A.st.dim, DD = D * D, tid = threadIdx.x, lane = tid & 63, r = tid & 15, grp = tid >> 4, wave = tid >> 6;
    const int rowbase = tid & 48;
    const double dt = A.dt, h6 = dt / 6.0;
    const bool mine = r < D;
    const double sta = mine ? A.hk.st[r] : 1.0, ista = 1.0 / sta;
    const double im = mine ? A.pot.inv_mass[r] : 0.0, c0 = mine ? A.pot.par0[r] : 0.0;
    const double c1 = (mine && A.pot.par1) ? A.pot.par1[r] : 0.0;
    const double ocA = mine ? R.oc.A[r] : 0.0, ocB = mine ? R.oc.B[r] : 0.0, ocC = mine ? R.oc.C[r] : 0.0;
    const double qk = mine ? R.oc.qk[r] : 0.0, pk = mine ? R.oc.pk[r] : 0.0;
    const bool nac = R.has_nac != 0;
    const double nq0 = (mine && nac) ? R.nc.q0[r] : 0.0, np0 = (mine && nac) ? R.nc.p0[r] : 0.0;
    const double nrn = (mine && nac) ? R.nc.rn[r] : 0.0, ngn = (mine && nac) ? R.nc.gn[r] : 0.0;
    kptr ksi = (kptr)A.hk.si;
    const int64_t n = A.st.n, stride = (int64_t)gridDim.x * 16;
    const int slot = blockIdx.x * 4 + wave;
    double one = 1.0;
    asm volatile("" : "+v"(one));

    for (int64_t t0 = (int64_t)blockIdx.x * 16; t0 < n; t0 += stride) {
        const bool active = t0 + grp < n, head = active && r == 0;
        const int64_t tr = active ? t0 + grp : n - 1;          // idle rows shadow the last trajectory and contribute nothing
        double *M = A.st.mono + tr * 4 * (int64_t)DD, *qp = A.st.qp + tr * 2 * D;
        // ---- the trajectory: rows of the four blocks, (q_a, p_a), S, c2, sign, and its time-independent factors
        double mqq[DP], mqp[DP], mpq[DP], mpp[DP];
#pragma unroll
        for (int b = 0; b < DP; ++b) {
            const bool ok = mine && b < D;
            mqq[b] = ok ? M[r * D + b] : 0.0; mqp[b] = ok ? M[DD + r * D + b] : 0.0;
            mpq[b] = ok ? M[2 * DD + r * D + b] : 0.0; mpp[b] = ok ? M[3 * DD + r * D + b] : 0.0;
        }
        double q = mine ? qp[r] : 0.0, p = mine ? qp[D + r] : 0.0;
        double S = A.st.act[tr], sgn = A.st.sgn[tr];
        cplx c2 = ((const cplx *)A.st.c2)[tr];
        const cplx vi = ((const cplx *)R.vi)[tr];
        const cplx nacq = nac ? ((const cplx *)R.nacq)[tr] : c_make(0.0, 0.0);
        const double wgt = 1.0 / (R.mc_norm * R.probi[tr]);

        for (int k = 0; k < R.nsteps; ++k) {
            // ---- terms of the correlation functions from the current state (hk_correlate_kernel, diagonal widths) ----
            double v5[5];
            {
                auto sum = [](double v) { return row_sum(v); };
                double sA, sB, sP, sC, sR = 0.0, sG = 0.0;
                overlap_sums_diag(qk, pk, ocA, ocB, ocC, q, p, sum, sA, sB, sP, sC);
                if (nac) nac_sums(nq0, np0, nrn, ngn, q, p, sum, sR, sG);
                const cplx cvt = overlap_value_conj(R.oc.fac, sA, sB, sP, sC);
                const cplx cq = corr_c_term(cvt, vi, signed_root(c2, sgn), action_phase(S), wgt);
                v5[0] = cq.x; v5[1] = cq.y; v5[2] = 0.0; v5[3] = 0.0;
                if (nac) {
                    const cplx kq = corr_k_term(R.nc.n2, R.nc.p0n1, sR, sG, nacq, cq);
                    v5[2] = kq.x; v5[3] = kq.y;
                }
            }
            // ---- RK4 of (q_a, p_a) with the reference's stage formula, action, <T+V> and the row propagator P_a ----
            double red5[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, p11 = 1.0, p12 = 0.0, p21 = 0.0, p22 = 1.0;
            if (mine) {
                double h1, h2, h3, h4;
                sep_mode_rk4(KIND, c0, c1, im, dt, q, p, red5, h1, h2, h3, h4);
                sep_row_propagator(im, h1, h2, h3, h4, dt, p11, p12, p21, p22);
            }
            {
                double s5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
                dpp_guard(red5);
                // sum_rows (sc_row16.h) written out: with the call hipcc spills 2 to 6 VGPRs more at DP = 12
                sfor<0, DP>([&](auto kc) {            // sums over the lanes k < DP (lanes beyond D hold zeros): as hk_step_sep16_kernel
#pragma unroll
                    for (int i = 0; i < 5; ++i) fmac_bc<decltype(kc)::value>(s5[i], red5[i], one);
                });
                S += h6 * (s5[0] + 2.0 * s5[1] + 2.0 * s5[2] + s5[3]);
                v5[4] = s5[4];
            }
            // ---- (Mqq, Mpq)' = P_a (Mqq, Mpq), (Mqp, Mpp)' = P_a (Mqp, Mpp); prefactor row a (rows and columns beyond D: identity)
            cplx mat[DP], keep[DP];
#pragma unroll
            for (int b = 0; b < DP; ++b) {
                // sep_propagate_row written out: with the call hipcc spills 250 bytes per lane more at DP = 12
                const double nqq = fma(p12, mpq[b], p11 * mqq[b]), npq = fma(p22, mpq[b], p21 * mqq[b]);
                const double nqp = fma(p12, mpp[b], p11 * mqp[b]), npp = fma(p22, mpp[b], p21 * mqp[b]);
                mqq[b] = nqq; mpq[b] = npq; mqp[b] = nqp; mpp[b] = npp;
                const double sib = b < D ? ksi[b] : 1.0, isib = 1.0 / sib;
                mat[b] = (mine && b < D) ? prefactor_element_diag(sta, ista, sib, isib, mqq[b], mqp[b], mpq[b], mpp[b])
                                         : c_make(r == b ? 1.0 : 0.0, 0.0);
                keep[b] = mat[b];
            }
            int weak = 0;
            cplx det = det_rows_fixed_order<DP>(mat, r, weak);
            if (__builtin_amdgcn_readfirstlane(wave_max_i32(weak)) != 0) {
                // some trajectory of this wavefront met a weak pivot: its determinant by elimination with the pivot searched among
                // the lanes (ds_bpermute), as round 2 did for every trajectory
                int myk, src;
                cplx det2, dummy[1] = {c_make(0.0, 0.0)};
                gauss_jordan_rows<DP, 1>(keep, dummy, r >= DP, r, rowbase, myk, src, det2);
                if (weak) det = det2;
            }
            if (crossed_branch_cut(c2, det)) sgn = -sgn;       // branch tracker (propagators.py:1045-1047)
            c2 = det;
            // ---- this wavefront's share of step k: one writer per slot ----
            if constexpr (MOM) run_moments_share<MOM>(R, v5, head, k, slot, lane);
            // (the hand-over is written out in both whole-loop kernels: as a shared function it moves hk_run_lin_kernel's registers)
#pragma unroll
            for (int i = 0; i < 5; ++i) v5[i] = sum_row_heads(v5[i], head);
            if (lane == 0) {
                double *pp = R.partials + ((size_t)k * R.slots + slot) * 5;
#pragma unroll
                for (int i = 0; i < 5; ++i) __builtin_amdgcn_global_atomic_fadd_f64((__attribute__((address_space(1))) double *)(pp + i), v5[i]);
            }
        }
        // ---- the trajectory goes back
        if (active) {
            if (mine) {
#pragma unroll
                for (int b = 0; b < DP; ++b) {
                    if (b < D) {
                        M[r * D + b] = mqq[b]; M[DD + r * D + b] = mqp[b];
                        M[2 * DD + r * D + b] = mpq[b]; M[3 * DD + r * D + b] = mpp[b];
                    }
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


}  // namespace

// this file is compiled twice: on its own with the kernels of sc_hk_run (MOM = false), and included by sc_hk_run_sep16_m.hip with
// SC_RUN_MOMENTS_TU defined for those of sc_hk_run_m (MOM = true) -- a translation unit of their own, so that the instantiations
// without moments are compiled exactly as before
#ifdef SC_RUN_MOMENTS_TU
#define SC_RUNSEP_MOM true
#define SC_RUNSEP_ENTRY sc_launch_run_sep16_m
#else
#define SC_RUNSEP_MOM false
#define SC_RUNSEP_ENTRY sc_launch_run_sep16_plain
#endif
int SC_RUNSEP_ENTRY(const RunArgs &a, int grid, hipStream_t s) {
    sc_sep16_dispatch(a.step.pot.kind, a.step.st.dim, [&](auto dp, auto kind) {
        hipLaunchKernelGGL((hk_run_sep16_kernel<decltype(dp)::value, decltype(kind)::value, SC_RUNSEP_MOM>), dim3(grid), dim3(256), 0, s, a);
    });
    const int rc = sc_check_launch(SC_RUNSEP_MOM ? "sc_hk_run_m (fused steps)" : "sc_hk_run (fused steps)");
    return rc == SC_OK ? 1 : rc;
}

#ifndef SC_RUN_MOMENTS_TU
int sc_launch_run_sep16(const RunArgs &a, int grid, hipStream_t s, bool moments) {
    return moments ? sc_launch_run_sep16_m(a, grid, s) : sc_launch_run_sep16_plain(a, grid, s);
}
#endif

// Arguments and launchers shared by the whole-loop kernels behind sc_hk_run (sc_hk_run_sep16.hip: separable
// potentials; sc_hk_run_lin.hip: constant dense Hessian) and their host side (sc_hk_run.hip).
#pragma once
#include "sc_common.h"

struct RunArgs {
    StepArgs step;              // potential, state, prefactor constants, dt
    sc_overlap_consts oc;       // <q_t, p_t, Gamma_t | q0, p0, Gamma_0>
    sc_nac_consts nc;
    int has_nac;
    const double *vi, *probi, *nacq;
    double mc_norm;
    int nsteps;
    double *partials;           // [nsteps][slots][5]: Re C, Im C, Re k, Im k, sum of (T+V) at the k4 stage; zeroed by the caller.
                                // sc_hk_run_m: followed by [nsteps][slots][6], the second moments of the terms (run_moments_share)
    int slots;                  // 4 * gridDim.x
    const double *mode_prop;    // sc_hk_run_modal: [D][4] per-mode step matrices (the blocks are in normal-mode coordinates), else NULL
};

// sc_hk_run_lin.hip: 1 = the shape (D, d', diagonal widths) is instantiated (and, with launch != 0, was launched), 0 = not,
// < 0 on error.  The caller guarantees SC_POT_HARMONIC_DENSE, pot.lin_prop built for a.step.dt, row-major blocks.
// moments: the kernels of sc_hk_run_m (sc_hk_run_lin_m.hip, sc_launch_run_lin_m).
int sc_launch_run_lin(const RunArgs &a, int grid, hipStream_t s, int launch, bool moments = false);
int sc_launch_run_lin_plain(const RunArgs &a, int grid, hipStream_t s, int launch);
int sc_launch_run_lin_m(const RunArgs &a, int grid, hipStream_t s, int launch);
// sc_hk_run_sep16.hip: the separable whole-loop kernel for a.step.pot.kind, D <= 12; 1 = launched, < 0 on error.
// moments: the kernels of sc_hk_run_m (sc_hk_run_sep16_m.hip, sc_launch_run_sep16_m).
int sc_launch_run_sep16(const RunArgs &a, int grid, hipStream_t s, bool moments);
int sc_launch_run_sep16_plain(const RunArgs &a, int grid, hipStream_t s);
int sc_launch_run_sep16_m(const RunArgs &a, int grid, hipStream_t s);

// sc_hk_run_m: the second moments (Re C)^2, (Im C)^2, Re C Im C, (Re k)^2, (Im k)^2, Re k Im k of the trajectories whose terms sit
// in v5[0..3] of the row heads, summed over the wavefront and added to its moment slot of step k -- one writer per slot, as for
// the main partials.  Called before the main sums overwrite v5; the kernels without moments (MOM = false) compile nothing here.
template <bool MOM>
__device__ __forceinline__ void run_moments_share(const RunArgs &R, const double (&v5)[5], bool head, int k, int slot, int lane) {
    if constexpr (MOM) {
        double m[6] = {v5[0] * v5[0], v5[1] * v5[1], v5[0] * v5[1], v5[2] * v5[2], v5[3] * v5[3], v5[2] * v5[3]};
#pragma unroll
        for (int i = 0; i < 6; ++i) m[i] = wave_sum(head ? m[i] : 0.0);
        if (lane == 0) {
            double *pp = R.partials + (size_t)5 * R.slots * R.nsteps + ((size_t)k * R.slots + slot) * 6;
#pragma unroll
            for (int i = 0; i < 6; ++i) __builtin_amdgcn_global_atomic_fadd_f64((__attribute__((address_space(1))) double *)(pp + i), m[i]);
        }
    }
}

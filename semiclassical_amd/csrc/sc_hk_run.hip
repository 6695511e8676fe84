// Host side of the whole loop as one launch (sc_hk_run, sc_hk_run_m, sc_hk_run_modal, sc_hk_run_modal_m): the checks, the RunArgs,
// the choice between the two whole-loop kernels (sc_hk_run_sep16.hip: separable potentials; sc_hk_run_lin.hip: constant dense
// Hessian) and what follows either of them -- the slots of every step added in a fixed order, and the energy guard.
#include "sc_hk_run.h"

namespace {

// slots of one step added in a fixed order -> out[k][0..3], mean <T+V> of the step -> out[k][4]
__global__ __launch_bounds__(256) void hk_run_reduce_kernel(const double *partials, int slots, double n_traj, double *out) {
    __shared__ double red[32];
    const int k = blockIdx.x;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < slots; i += 256) {
        const double *pp = partials + ((size_t)k * slots + i) * 5;
#pragma unroll
        for (int j = 0; j < 5; ++j) v[j] += pp[j];
    }
    block_sum<5>(v, red);
    if (threadIdx.x < 5) out[(size_t)k * 5 + threadIdx.x] = threadIdx.x < 4 ? v[threadIdx.x] : v[4] / n_traj;
}

// moment slots of one step added in a fixed order -> out[k][0..5]
__global__ __launch_bounds__(256) void hk_run_reduce_moments_kernel(const double *mpart, int slots, double *out) {
    __shared__ double red[24];
    const int k = blockIdx.x;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < slots; i += 256) {
        const double *pp = mpart + ((size_t)k * slots + i) * 6;
#pragma unroll
        for (int j = 0; j < 6; ++j) v[j] += pp[j];
    }
    block_sum<6>(v, red);
    if (threadIdx.x < 6) out[(size_t)k * 6 + threadIdx.x] = v[threadIdx.x];
}

// the energy guard over the steps of a fused run, in order (propagators.py:385-398; sc_energy_guard step by step)
__global__ void hk_run_guard_kernel(const double *out, int nsteps, double *elog) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double prev = elog[1], worst = elog[2], count = elog[3], last = elog[0];
    for (int k = 0; k < nsteps; ++k) {
        const double mean = out[(size_t)k * 5 + 4];
        last = prev;
        if (count >= 1.0) { const double change = fabs(mean - prev); if (change > worst) worst = change; }
        prev = mean; count += 1.0;
    }
    elog[0] = last; elog[1] = prev; elog[2] = worst; elog[3] = count;
}

}  // namespace

extern "C" int sc_hk_run_slots(int64_t n, int32_t dim) {
    (void)dim;
    const int64_t groups = (n + 15) / 16;
    return 4 * (int)(groups < 1024 ? (groups > 0 ? groups : 1) : 1024);
}

// constant dense Hessian with its step matrix, D <= 16 at the shapes sc_hk_run_lin.hip instantiates (real L, R)
static bool run_lin_shape(const sc_potential *pot, const sc_hk_consts *hk, bool modal = false) {
    if (pot->kind != SC_POT_HARMONIC_DENSE || (!modal && !pot->lin_prop) || pot->dim > 16 || hk->dim != pot->dim) return false;
    static const double some = 0.0;
    RunArgs probe{};
    probe.step.st.dim = pot->dim;
    probe.step.hk = *hk;
    probe.mode_prop = modal ? &some : nullptr;
    return sc_launch_run_lin(probe, 0, nullptr, 0) == 1;
}

extern "C" int sc_hk_run_supported(const sc_potential *pot, const sc_hk_consts *hk, const sc_overlap_consts *ovl) {
    if (!pot || !hk || !ovl) return 0;
    const bool sep = sc_pot_is_separable(pot->kind);
    if (sep && hk->diag && ovl->diag && pot->dim <= SC_SEP16_MAX_D) return 1;
    return run_lin_shape(pot, hk) ? 1 : 0;
}

extern "C" int64_t sc_hk_run_scratch_doubles(int64_t n, int32_t dim, int32_t nsteps, int32_t moments) {
    if (nsteps <= 0) return 0;
    return (int64_t)(moments ? 11 : 5) * sc_hk_run_slots(n, dim) * (int64_t)nsteps;
}

static int run_whole_loop(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, const sc_overlap_consts *ovl_t0,
                          const sc_nac_consts *nc, const double *vi, const double *probi, const double *nacq, double mc_norm,
                          double dt, int32_t nsteps, const double *mode_prop, double *partials, double *slots_out, double *elog,
                          double *moments_out, void *stream) {
    if (!pot || !st || !hk || !ovl_t0 || !vi || !probi || !partials || !slots_out || !elog)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_run: null argument");
    if (nc && !nacq) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_run: nac constants without nacq");
    if (!mode_prop && !sc_hk_run_supported(pot, hk, ovl_t0))
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_hk_run: needs a separable potential with diagonal width matrices and D <= %d, or a "
                       "constant dense Hessian with its step matrix (sc_potential.lin_prop) at an instantiated shape D <= 16 "
                       "(use the step-by-step entry points)", SC_SEP16_MAX_D);
    const bool lin = pot->kind == SC_POT_HARMONIC_DENSE;
    if (lin && !mode_prop && pot->lin_dt != dt)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_run: the step matrix was built for dt = %g, the call asks for %g", pot->lin_dt, dt);
    if (pot->dim != st->dim || hk->dim != st->dim || ovl_t0->dim != st->dim)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_run: dimension mismatch");
    if (int rq = sc_require_rowmajor(st, "sc_hk_run")) return rq;
    if (st->n <= 0 || nsteps <= 0) return SC_OK;
    hipStream_t s = (hipStream_t)stream;
    RunArgs a;
    a.step = StepArgs{*pot, *st, *hk, dt, 0, nullptr, 0};
    a.oc = *ovl_t0; a.has_nac = nc != nullptr;
    if (nc) a.nc = *nc; else a.nc = sc_nac_consts{};
    a.vi = vi; a.probi = probi; a.nacq = nacq; a.mc_norm = mc_norm; a.nsteps = nsteps; a.partials = partials;
    a.slots = sc_hk_run_slots(st->n, st->dim);
    a.mode_prop = mode_prop;
    const bool mom = moments_out != nullptr;
    if (hipMemsetAsync(partials, 0, sizeof(double) * (size_t)sc_hk_run_scratch_doubles(st->n, st->dim, nsteps, mom), s) != hipSuccess)
        return sc_check_launch("sc_hk_run (partials)");
    const int grid = a.slots / 4;
    const int rc = lin ? sc_launch_run_lin(a, grid, s, 1, mom) : sc_launch_run_sep16(a, grid, s, mom);
    if (rc < 0) return rc;
    if (rc == 0) return sc_fail(SC_ERR_UNSUPPORTED, "sc_hk_run: shape D=%d d'=%d not instantiated", st->dim, hk->dprime);
    hipLaunchKernelGGL(hk_run_reduce_kernel, dim3(nsteps), dim3(256), 0, s, partials, a.slots, (double)st->n, slots_out);
    if (mom)
        hipLaunchKernelGGL(hk_run_reduce_moments_kernel, dim3(nsteps), dim3(256), 0, s, partials + (size_t)5 * a.slots * nsteps,
                           a.slots, moments_out);
    hipLaunchKernelGGL(hk_run_guard_kernel, dim3(1), dim3(64), 0, s, slots_out, nsteps, elog);
    return sc_check_launch("sc_hk_run (reduction)");
}

extern "C" int sc_hk_run(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, const sc_overlap_consts *ovl_t0,
                         const sc_nac_consts *nc, const double *vi, const double *probi, const double *nacq, double mc_norm,
                         double dt, int32_t nsteps, double *partials, double *slots_out, double *elog, void *stream) {
    return run_whole_loop(pot, st, hk, ovl_t0, nc, vi, probi, nacq, mc_norm, dt, nsteps, nullptr, partials, slots_out, elog, nullptr,
                          stream);
}

extern "C" int sc_hk_run_m(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, const sc_overlap_consts *ovl_t0,
                           const sc_nac_consts *nc, const double *vi, const double *probi, const double *nacq, double mc_norm,
                           double dt, int32_t nsteps, double *partials, double *slots_out, double *elog, double *moments_out,
                           void *stream) {
    return run_whole_loop(pot, st, hk, ovl_t0, nc, vi, probi, nacq, mc_norm, dt, nsteps, nullptr, partials, slots_out, elog,
                          moments_out, stream);
}

extern "C" int sc_hk_run_modal_supported(const sc_potential *pot, const sc_hk_consts *hk, const sc_overlap_consts *ovl) {
    if (!pot || !hk || !ovl) return 0;
    return run_lin_shape(pot, hk, true) ? 1 : 0;
}

extern "C" int sc_hk_run_modal_m(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, const sc_overlap_consts *ovl_t0,
                                 const sc_nac_consts *nc, const double *vi, const double *probi, const double *nacq, double mc_norm,
                                 double dt, int32_t nsteps, const double *mode_prop, double *partials, double *slots_out, double *elog,
                                 double *moments_out, void *stream) {
    if (!mode_prop) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_run_modal: null mode_prop");
    if (!pot || !hk || !ovl_t0 || !sc_hk_run_modal_supported(pot, hk, ovl_t0))
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_hk_run_modal: needs a constant dense Hessian and dense real prefactor constants at an "
                       "instantiated shape D <= 16 (use sc_hk_run)");
    return run_whole_loop(pot, st, hk, ovl_t0, nc, vi, probi, nacq, mc_norm, dt, nsteps, mode_prop, partials, slots_out, elog,
                          moments_out, stream);
}

extern "C" int sc_hk_run_modal(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, const sc_overlap_consts *ovl_t0,
                               const sc_nac_consts *nc, const double *vi, const double *probi, const double *nacq, double mc_norm,
                               double dt, int32_t nsteps, const double *mode_prop, double *partials, double *slots_out, double *elog,
                               void *stream) {
    return sc_hk_run_modal_m(pot, st, hk, ovl_t0, nc, vi, probi, nacq, mc_norm, dt, nsteps, mode_prop, partials, slots_out, elog,
                             nullptr, stream);
}

// Shared device helpers of the gfx950 trajectory engine (wave64, fp64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "semiclassical_hip.h"

#define SC_HBAR 1.0   // reference semiclassical/units.py:8

typedef double2 cplx;   // (re, im), same memory layout as torch.complex128

__device__ __forceinline__ cplx c_make(double re, double im) { return make_double2(re, im); }
__device__ __forceinline__ cplx c_add(cplx a, cplx b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cplx c_sub(cplx a, cplx b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ cplx c_mul(cplx a, cplx b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ cplx c_scale(cplx a, double s) { return make_double2(a.x * s, a.y * s); }
__device__ __forceinline__ cplx c_conj(cplx a) { return make_double2(a.x, -a.y); }
__device__ __forceinline__ double c_abs2(cplx a) { return a.x * a.x + a.y * a.y; }
__device__ __forceinline__ cplx c_inv(cplx a) {
    double s = 1.0 / c_abs2(a);
    return make_double2(a.x * s, -a.y * s);
}
// a - l*u
__device__ __forceinline__ cplx c_fnma(cplx l, cplx u, cplx a) {
    a.x = fma(-l.x, u.x, a.x); a.x = fma(l.y, u.y, a.x);
    a.y = fma(-l.x, u.y, a.y); a.y = fma(-l.y, u.x, a.y);
    return a;
}
// a + l*u
__device__ __forceinline__ cplx c_fma(cplx l, cplx u, cplx a) {
    a.x = fma(l.x, u.x, a.x); a.x = fma(-l.y, u.y, a.x);
    a.y = fma(l.x, u.y, a.y); a.y = fma(l.y, u.x, a.y);
    return a;
}
// principal square root (branch cut on the negative real axis, sign of Im follows Im z), as torch.sqrt
__device__ __forceinline__ cplx c_sqrt(cplx z) {
    double r = hypot(z.x, z.y);
    if (r == 0.0) return make_double2(0.0, z.y);
    if (z.x >= 0.0) {
        double t = sqrt(0.5 * (r + z.x));
        return make_double2(t, z.y / (2.0 * t));
    }
    double t = sqrt(0.5 * (r - z.x));
    return make_double2(fabs(z.y) / (2.0 * t), copysign(t, z.y));
}
__device__ __forceinline__ cplx c_exp(cplx z) {
    double s, c;
    sincos(z.y, &s, &c);
    double e = exp(z.x);
    return make_double2(e * c, e * s);
}

// Sum over the wavefront, result in every lane.  DPP rotations inside each 16-lane row (64-bit values move as two
// 32-bit DPP moves), then one v_readlane pair per row: no LDS traffic (`__shfl_xor` is a ds_bpermute, ~100 cycles
// per dependent step, 12 of them for a double).  Fixed order => deterministic.
template <int CTRL>
__device__ __forceinline__ double dpp_mov_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum(double v) {
    v += dpp_mov_f64<0x128>(v);      // row_ror:8
    v += dpp_mov_f64<0x124>(v);      // row_ror:4
    v += dpp_mov_f64<0x122>(v);      // row_ror:2
    v += dpp_mov_f64<0x121>(v);      // row_ror:1
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const double r0 = __hiloint2double(__builtin_amdgcn_readlane(hi, 0), __builtin_amdgcn_readlane(lo, 0));
    const double r1 = __hiloint2double(__builtin_amdgcn_readlane(hi, 16), __builtin_amdgcn_readlane(lo, 16));
    const double r2 = __hiloint2double(__builtin_amdgcn_readlane(hi, 32), __builtin_amdgcn_readlane(lo, 32));
    const double r3 = __hiloint2double(__builtin_amdgcn_readlane(hi, 48), __builtin_amdgcn_readlane(lo, 48));
    return (r0 + r1) + (r2 + r3);
}

// Wave-uniform maximum of a 32-bit integer over the wavefront without LDS traffic: DPP row rotations inside each
// 16-lane row, then one v_readlane per row.  (`__shfl_xor` is a ds_bpermute: ~100 cycles per dependent step.)
__device__ __forceinline__ int wave_max_i32(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x128, 0xF, 0xF, false));      // row_ror:8
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x124, 0xF, 0xF, false));      // row_ror:4
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x122, 0xF, 0xF, false));      // row_ror:2
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x121, 0xF, 0xF, false));      // row_ror:1
    const int a = __builtin_amdgcn_readlane(v, 0), b = __builtin_amdgcn_readlane(v, 16);
    const int c = __builtin_amdgcn_readlane(v, 32), d = __builtin_amdgcn_readlane(v, 48);
    return max(max(a, b), max(c, d));
}

// Partial-pivoting search over one candidate per lane: `mag` = |a|^2 of this lane's candidate row `row` (or any
// value with valid = false).  Returns the row of (nearly) the largest magnitude: the comparison key keeps the sign,
// the exponent and 14 mantissa bits of |a|^2, ties go to the lower lane.  -1 if no lane is valid.
__device__ __forceinline__ int wave_pivot_row(double mag, int row, bool valid) {
    const int lane = threadIdx.x & 63;
    const int key = valid ? ((__double2hiint(mag) & ~63) | (63 - lane)) : -1;
    const int best = wave_max_i32(key);
    if (best < 0) return -1;
    return __builtin_amdgcn_readlane(row, __builtin_amdgcn_readfirstlane(63 - (best & 63)));
}

// Sum NV values over the whole workgroup; every thread receives the totals.
// `red` is LDS scratch of at least NV * (blockDim.x / 64) doubles.  Deterministic order.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    if (nw == 1) return;
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) red[wave * NV + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double s = 0.0;
        for (int w = 0; w < nw; ++w) s += red[w * NV + i];
        v[i] = s;
    }
}

// offset of element (a, b) of block p inside one trajectory's monodromy storage (include/semiclassical_hip.h)
__host__ __device__ __forceinline__ int64_t sc_mono_offset(int layout, int D, int p, int a, int b) {
    if (layout == SC_MONO_ROWMAJOR) return ((int64_t)p * D + a) * D + b;
    const int ra = a >> 4, rb = b >> 4;
    const int nra = D - 16 * ra < 16 ? D - 16 * ra : 16, ncb = D - 16 * rb < 16 ? D - 16 * rb : 16;
    // inside a tile: (Mqq, Mqp) element by element, then (Mpq, Mpp) element by element (a thread of the fast kernel moves the two
    // planes of a pair with ONE 16-byte access; round 4 -- the four planes used to follow one another)
    return 4 * ((int64_t)16 * ra * D + 16 * nra * rb) + (int64_t)(p >> 1) * 2 * nra * ncb + 2 * ((a & 15) * ncb + (b & 15)) + (p & 1);
}

// ---- shared by the step kernels ----
struct StepArgs {
    sc_potential pot;
    sc_state st;
    sc_hk_consts hk;
    double dt;
    int mode;
    double *epart;
    int npart;          // entries of epart the energy guard adds up (sc_step_grid); kernels with fewer workgroups clear the rest
};

// diagonal Hessian: every mode is its own one-dimensional problem (sep_eval below)
__host__ __device__ __forceinline__ bool sc_pot_is_separable(int kind) {
    return kind == SC_POT_MORSE || kind == SC_POT_HARMONIC_SEP || kind == SC_POT_EPS_MORSE;
}

// V, dV/dx, d2V/dx2 of one mode of a separable potential
__device__ __forceinline__ void sep_eval(int kind, double c0, double c1, double x, double &v, double &g, double &h) {
    if (kind == SC_POT_MORSE) {                    // c0 = a, c1 = De
        double e = exp(-c0 * x);
        double om = 1.0 - e;
        v = c1 * om * om;
        g = 2.0 * c0 * c1 * e * om;
        h = 2.0 * c0 * c0 * c1 * e * (2.0 * e - 1.0);
    } else if (kind == SC_POT_HARMONIC_SEP) {      // c0 = omega^2
        v = 0.5 * c0 * x * x;
        g = c0 * x;
        h = c0;
    } else {                                       // SC_POT_EPS_MORSE: c0 = eps, c1 = b
        double e1 = exp(-c1 * x), e2 = exp(-2.0 * c1 * x);
        double om = 1.0 - e1;
        v = c0 / (2.0 * c1 * c1) * om * om + (1.0 - c0) * 0.5 * x * x;
        g = c0 / c1 * (e1 - e2) + (1.0 - c0) * x;
        h = c0 * (2.0 * e2 - e1) + (1.0 - c0);
    }
}

// RK4 of the pair (u, v) with du/dt = v/m, dv/dt = -h(t) u  (diagonal Hessian)
__device__ __forceinline__ void rk4_pair(double &u, double &v, double im, double h1, double h2, double h3, double h4,
                                         double dt) {
    const double hh = 0.5 * dt, h6 = dt / 6.0;
    double k1u = v * im, k1v = -h1 * u;
    double u2 = u + hh * k1u, v2 = v + hh * k1v;
    double k2u = v2 * im, k2v = -h2 * u2;
    double u3 = u + hh * k2u, v3 = v + hh * k2v;
    double k3u = v3 * im, k3v = -h3 * u3;
    double u4 = u + dt * k3u, v4 = v + dt * k3v;
    double k4u = v4 * im, k4v = -h4 * u4;
    u = u + h6 * (k1u + 2.0 * k2u + 2.0 * k3u + k4u);
    v = v + h6 * (k1v + 2.0 * k2v + 2.0 * k3v + k4v);
}

// The physics of one HK step for a separable potential with diagonal width matrices, defined ONCE: every route calls these,
// so the routes agree bit for bit in them by construction.  Do not reorder an operation here: results would change everywhere.
//
// RK4 of one mode (q_a, p_a) with the reference's stage formula (propagators.py:86-119, 313-383): q and p advance in place;
// te[0..3] = T - V at the four stage points, te[4] = T + V at the k4 point (:380, quirk Q2), h1..h4 = d2V/dx2 at the stage points
__device__ __forceinline__ void sep_mode_rk4(int kind, double c0, double c1, double im, double dt, double &q, double &p,
                                             double (&te)[5], double &h1, double &h2, double &h3, double &h4) {
    const double hh = 0.5 * dt, h6 = dt / 6.0;
    double v, g;
    sep_eval(kind, c0, c1, q, v, g, h1);
    const double kq1 = p * im, kp1 = -g;
    te[0] = 0.5 * p * p * im - v;
    const double q2 = q + hh * kq1, p2 = p + hh * kp1;
    sep_eval(kind, c0, c1, q2, v, g, h2);
    const double kq2 = p2 * im, kp2 = -g;
    te[1] = 0.5 * p2 * p2 * im - v;
    const double q3 = q + hh * kq2, p3 = p + hh * kp2;
    sep_eval(kind, c0, c1, q3, v, g, h3);
    const double kq3 = p3 * im, kp3 = -g;
    te[2] = 0.5 * p3 * p3 * im - v;
    const double q4 = q + dt * kq3, p4 = p + dt * kp3;
    sep_eval(kind, c0, c1, q4, v, g, h4);
    const double kq4 = p4 * im, kp4 = -g;
    te[3] = 0.5 * p4 * p4 * im - v;
    te[4] = 0.5 * p4 * p4 * im + v;
    q = q + h6 * (kq1 + 2.0 * kq2 + 2.0 * kq3 + kq4);
    p = p + h6 * (kp1 + 2.0 * kp2 + 2.0 * kp3 + kp4);
}

// 2 x 2 RK4 propagator P_a = [[p11, p12], [p21, p22]] of row a of the monodromy blocks: the unit vectors through rk4_pair
__device__ __forceinline__ void sep_row_propagator(double im, double h1, double h2, double h3, double h4, double dt,
                                                   double &p11, double &p12, double &p21, double &p22) {
    p11 = 1.0; p21 = 0.0; p12 = 0.0; p22 = 1.0;
    rk4_pair(p11, p21, im, h1, h2, h3, h4, dt);       // (u, v) = (1, 0) -> first column of P_a
    rk4_pair(p12, p22, im, h1, h2, h3, h4, dt);       // (0, 1) -> second column
}

// (Mqq, Mpq)' = P_a (Mqq, Mpq), (Mqp, Mpp)' = P_a (Mqp, Mpp) for one element of row a
__device__ __forceinline__ void sep_propagate_row(double p11, double p12, double p21, double p22,
                                                  double &mqq, double &mqp, double &mpq, double &mpp) {
    const double nqq = fma(p12, mpq, p11 * mqq), npq = fma(p22, mpq, p21 * mqq);
    const double nqp = fma(p12, mpp, p11 * mqp), npp = fma(p22, mpp, p21 * mqp);
    mqq = nqq; mpq = npq; mqp = nqp; mpp = npp;
}

// element (a, b) of the HK prefactor matrix for diagonal width matrices (propagators.py:969-986):
//   1/2 (st_a/si_b Mqq + si_b/st_a Mpp) + i/2 (-hbar st_a si_b Mqp + Mpq / (hbar st_a si_b)),  ista = 1/st_a, isib = 1/si_b
__device__ __forceinline__ cplx prefactor_element_diag(double sta, double ista, double sib, double isib,
                                                       double mqq, double mqp, double mpq, double mpp) {
    return c_make(0.5 * (sta * isib * mqq + ista * sib * mpp),
                  0.5 * (-SC_HBAR * sta * sib * mqp + (1.0 / SC_HBAR) * ista * isib * mpq));
}

// branch rule of the sqrt tracker (propagators.py:1045-1047): c2 went from `prev` to `det` across the negative real axis
__device__ __forceinline__ bool crossed_branch_cut(cplx prev, cplx det) {
    return prev.x < 0.0 && det.x < 0.0 && prev.y * det.y < 0.0;
}

// What one trajectory contributes to C_auto(t) and k_ic(t), defined ONCE like the step physics above: every HK route calls
// these.  Do not reorder an operation here, and do not merge or split these functions without comparing the results of every
// caller bit for bit: hipcc contracts products and sums into fused multiply-adds per kernel, and the cut into functions decides
// which ("One definition of the correlation terms").
//
// <q, p, Gamma_t | qk, pk, Gamma_0> from the four exponent sums dq.A.dq, dp.B.dp, pk.dq, dq.C.dp (propagators.py:232-237)
// (fac = sc_overlap_consts.fac.  These helpers take scalars, not the structs of constants: with a reference to a part of the
// kernel's argument block the whole-loop kernels are compiled with other branches and other register counts.)
__device__ __forceinline__ cplx overlap_value(double fac, double sA, double sB, double sP, double sC) {
    const cplx ex = c_make(-0.5 * sA - 0.5 / (SC_HBAR * SC_HBAR) * sB, (-sP + sC) / SC_HBAR);
    return c_scale(c_exp(ex), fac);
}

// those four sums for diagonal width matrices, and the two coupling sums of nacQ: this lane's mode, summed over the lanes by
// `sum` (wave_sum or row_sum) one term after the other -- with all terms formed first hk_correlate_kernel needs 8 VGPRs more
template <class SUM>
__device__ __forceinline__ void overlap_sums_diag(double qk, double pk, double ocA, double ocB, double ocC, double q, double p, SUM sum,
                                                  double &sA, double &sB, double &sP, double &sC) {
    const double dq = qk - q, dpp = pk - p;
    sA = sum(dq * ocA * dq); sB = sum(dpp * ocB * dpp); sP = sum(pk * dq); sC = sum(dq * ocC * dpp);
}
template <class SUM>
__device__ __forceinline__ void nac_sums(double nq0, double np0, double nrn, double ngn, double q, double p, SUM sum, double &sR, double &sG) {
    sR = sum((nq0 - q) * nrn); sG = sum((p - np0) * ngn);
}

// the trajectory's own factors: the signed principal root of the prefactor's square, and the action phase (propagators.py:784-807)
__device__ __forceinline__ cplx signed_root(cplx c2, double sgn) { return c_scale(c_sqrt(c2), sgn); }
__device__ __forceinline__ cplx action_phase(double S) { return c_exp(c_make(0.0, S / SC_HBAR)); }

// conj(vt) = <q0, p0, Gamma_0 | q, p, Gamma_t> as the terms of C_auto take it.  A function of its own next to the product with
// `fac`: hipcc folds the sign into that product and then forms a b + c d of the next complex product as one multiply and one fused
// multiply-add -- WHICH product it fuses, and with it the last bit of the terms, follows from where the sign sits
__device__ __forceinline__ cplx overlap_value_conj(double fac, double sA, double sB, double sP, double sC) {
    const cplx vt = overlap_value(fac, sA, sB, sP, sC);
    return c_conj(vt);
}

// term of C_auto: conj(vt) vi (c ph) w with cvt = overlap_value_conj(...), vi the initial overlap, c = signed_root(...), ph =
// action_phase(...), w the Monte-Carlo weight; the callers form cvt, c, ph, w in this order, between their loads
__device__ __forceinline__ cplx corr_c_term(cplx cvt, cplx vi, cplx c, cplx ph, double w) {
    return c_scale(c_mul(c_mul(cvt, vi), c_mul(c, ph)), w);
}

// term of k_ic from the term of C_auto: nacQ nacq cq / hbar^2 with n2, p0n1 of sc_nac_consts (propagators.py:886-909).  The
// caller keeps its `if (nac)` around the call: with the branch in here hk_run_sep16_kernel needs 80 bytes of scratch per lane more.
__device__ __forceinline__ cplx corr_k_term(double n2, double p0n1, double sR, double sG, cplx nacq, cplx cq) {
    const cplx nacQ = c_make(n2 + sR, -(p0n1 + sG) / SC_HBAR);
    return c_scale(c_mul(c_mul(nacQ, nacq), cq), 1.0 / (SC_HBAR * SC_HBAR));
}

// The partition of a batch into B blocks for the Monte-Carlo error bars (batch means), defined ONCE: the
// block of the trajectory with rank-local index i.  Groups of four consecutive trajectories go round robin to the blocks; B is a
// power of two in 2 ... 64.  The trajectories are independent draws, so any fixed partition is valid; this one is what the
// whole-loop kernels already keep apart (block = wavefront slot mod B, sc_blocks.hip).  hostmath.error_block is the host's copy.
__host__ __device__ __forceinline__ int sc_error_block(int64_t i, int B) { return (int)((i >> 2) & (B - 1)); }
__host__ __device__ __forceinline__ bool sc_error_blocks_valid(int B) { return B >= 2 && B <= 64 && (B & (B - 1)) == 0; }

#define SC_SEP16_MAX_D 12   // D <= 12: hk_step_sep16_kernel (four trajectories per wavefront); 13 .. 16: hk_step_w16_kernel
int sc_launch_step_sep16(const StepArgs &a, int grid_entries, hipStream_t s);   // sc_hk_step_sep16.hip: 1 launched, 0 not taken
// the KIND x DP instantiations of the separable kernels for D <= SC_SEP16_MAX_D, chosen ONCE: f(dp, kind) is called with
// std::integral_constant<int, DP> (D rounded up to 4, 8, 12) and std::integral_constant<int, KIND> (the potential family)
template <class F>
inline void sc_sep16_dispatch(int kind, int D, F &&f) {
    auto with_dp = [&](auto dp) {
        if (kind == SC_POT_MORSE) f(dp, std::integral_constant<int, SC_POT_MORSE>{});
        else if (kind == SC_POT_HARMONIC_SEP) f(dp, std::integral_constant<int, SC_POT_HARMONIC_SEP>{});
        else f(dp, std::integral_constant<int, SC_POT_EPS_MORSE>{});
    };
    if (D <= 4) with_dp(std::integral_constant<int, 4>{});
    else if (D <= 8) with_dp(std::integral_constant<int, 8>{});
    else with_dp(std::integral_constant<int, 12>{});
}
int sc_launch_step_sd_multi(const StepArgs &a, const sc_multi_scratch &ms, int ksteps, hipStream_t s);    // sc_hk_step_sd.hip: ksteps = 2 .. 4 steps per visit
int sc_launch_step_lin(const StepArgs &a, int grid, hipStream_t s);   // sc_hk_step_lin.hip: 1 launched, 0 shape not built
int sc_launch_mono_identity(const sc_state *st, hipStream_t s);       // sc_sample.hip: st->mono = the identity blocks of t = 0

// host-side error plumbing (sc_api.hip)
int sc_fail(int code, const char *fmt, ...);
int sc_check_launch(const char *what);
int sc_require_rowmajor(const sc_state *st, const char *who);     // sc_layout.hip

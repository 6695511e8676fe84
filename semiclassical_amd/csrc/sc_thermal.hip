// Thermal ensembles of a harmonic initial surface: the canonical density operator as a positive mixture
// of coherent states of the width Gamma_0 (Glauber-Sudarshan P function).  Trajectory i carries its own centre (Q_i, P_i) in
// mass-weighted normal coordinates of the initial surface, and the terms of C_auto / k_ic are those of sc_hk_correlate.hip with
// the Cartesian image (a_i(t), b_i(t)) of the centre ROTATED to the time of the state in the place of (q0, p0), times the phase
//     Phi_i(t) = exp(i / (2 hbar) sum_k [Q_ik P_ik - Q_ik(t) P_ik(t)])
// between the displaced vacuum and the code's Gaussian.  Not in the reference, whose expressions the terms restate:
//   <q,p,Gbra|qk,pk,Gket>                         semiclassical/propagators.py:181-240
//   C_qp, Monte-Carlo weight                      semiclassical/propagators.py:784-807, 837
//   nacQ, nacq, k_ic                              semiclassical/propagators.py:886-909
//
// Mapping as hk_correlate_kernel: a wavefront takes 16 consecutive trajectories, reduces their sums one after the other (lane =
// mode) and parks them in lanes 0..15, which then evaluate the scalar tails side by side.  cos / sin of omega_k t: once per
// workgroup, in LDS.  Diagonal Gamma_0 (mode k = coordinate k) with diagonal overlap matrices: no matrix-vector product at all.
#include "sc_common.h"
#include "sc_philox.h"

namespace {

constexpr int TH_MAX_D = 512;
constexpr int64_t TH_MAX_N = (int64_t)64 * 65535;

struct ThermalArgs {
    sc_state st;                // correlate: the state; initial: only n, dim
    sc_overlap_consts oc;
    sc_nac_consts nc;
    sc_thermal_consts th;
    int has_nac;
    double time;
    const double *qp;           // [n][2 D]: st.qp (correlate) or the initial points (initial)
    const double *vi, *probi, *nacq;
    double mc_norm;
    double *cq_out, *kq_out, *partials;      // correlate
    double *vi_out, *nacq_out;               // initial
};

// the eight sums of one trajectory, summed over the wave:
//   sA = dq.A.dq, sB = dp.B.dp, sP = b.dq, sC = dq.C.dp   with dq = a - q, dp = b - p             (the overlap's exponent)
//   sR = (a - q).rn, sG = (p - b).gn, sN = b.n1                                                   (the coupling factors)
//   sF = sum_k [Q_k P_k - Q_k(t) P_k(t)]                                                          (the phase)
// cs, sn: LDS tables of cos / sin omega_k t, NULL = the centre of t = 0.  wv: per-wave LDS scratch [2 d''] + [2 D] (used for the
// dense maps and the dense overlap matrices only).
struct ThermalSums { double sA, sB, sP, sC, sR, sG, sN, sF; };

__device__ __forceinline__ void rotate_centre(double Q, double P, double w, const double *cs, const double *sn, int k,
                                              double &Qt, double &Pt, double &f) {
    if (cs) {
        const double c = cs[k], s = sn[k];
        Qt = fma(P / w, s, Q * c);
        Pt = fma(-w * Q, s, P * c);
        f = fma(-Qt, Pt, Q * P);
    } else {
        Qt = Q; Pt = P; f = 0.0;
    }
}

__device__ __forceinline__ ThermalSums thermal_sums(const ThermalArgs &A, const double *qp, const double *cen, const double *cs,
                                                    const double *sn, double *wv) {
    const int D = A.th.dim, dm = A.th.dmodes, lane = threadIdx.x & 63;
    const bool nac = A.has_nac != 0;
    ThermalSums s = {0, 0, 0, 0, 0, 0, 0, 0};
    double *rot = wv, *dvec = wv + 2 * dm;
    if (!A.th.diag) {
        for (int k = lane; k < dm; k += 64) {
            double Qt, Pt, f;
            rotate_centre(cen[k], cen[dm + k], A.th.omega[k], cs, sn, k, Qt, Pt, f);
            rot[k] = Qt; rot[dm + k] = Pt;
            s.sF += f;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    for (int a = lane; a < D; a += 64) {
        double ca, cb;
        if (A.th.diag) {
            double Qt, Pt, f;
            rotate_centre(cen[a], cen[dm + a], A.th.omega[a], cs, sn, a, Qt, Pt, f);
            s.sF += f;
            ca = fma(A.th.map_q[a], Qt, A.th.q0[a]);
            cb = A.th.map_p[a] * Pt;
        } else {
            ca = A.th.q0[a]; cb = 0.0;
            const double *mq = A.th.map_q + (size_t)a * dm, *mp = A.th.map_p + (size_t)a * dm;
            for (int k = 0; k < dm; ++k) {
                ca = fma(mq[k], rot[k], ca);
                cb = fma(mp[k], rot[dm + k], cb);
            }
        }
        const double dq = ca - qp[a], dpp = cb - qp[D + a];
        s.sP = fma(cb, dq, s.sP);
        if (nac) {
            s.sR = fma(dq, A.nc.rn[a], s.sR);
            s.sG = fma(-dpp, A.nc.gn[a], s.sG);
            s.sN = fma(cb, A.th.n1[a], s.sN);
        }
        if (A.oc.diag) {
            s.sA = fma(dq * A.oc.A[a], dq, s.sA);
            s.sB = fma(dpp * A.oc.B[a], dpp, s.sB);
            s.sC = fma(dq * A.oc.C[a], dpp, s.sC);
        } else {
            dvec[a] = dq; dvec[D + a] = dpp;
        }
    }
    if (!A.oc.diag) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int a = lane; a < D; a += 64) {
            double ya = 0, yb = 0, yc = 0;
            const double *rA = A.oc.A + (size_t)a * D, *rB = A.oc.B + (size_t)a * D, *rC = A.oc.C + (size_t)a * D;
            for (int b = 0; b < D; ++b) {
                ya = fma(rA[b], dvec[b], ya);
                yb = fma(rB[b], dvec[D + b], yb);
                yc = fma(rC[b], dvec[D + b], yc);
            }
            const double dq = dvec[a], dpp = dvec[D + a];
            s.sA = fma(dq, ya, s.sA);
            s.sB = fma(dpp, yb, s.sB);
            s.sC = fma(dq, yc, s.sC);
        }
    }
    // the next trajectory rewrites wv: every lane has read it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    s.sA = wave_sum(s.sA); s.sB = wave_sum(s.sB); s.sP = wave_sum(s.sP); s.sC = wave_sum(s.sC); s.sF = wave_sum(s.sF);
    if (nac) { s.sR = wave_sum(s.sR); s.sG = wave_sum(s.sG); s.sN = wave_sum(s.sN); }
    return s;
}

// doubles of per-wave LDS scratch, and of the whole workgroup with `nw` waves and the cos / sin tables
__host__ __device__ __forceinline__ size_t thermal_wave_doubles(int D, int dm, int th_diag, int oc_diag) {
    return (th_diag && oc_diag) ? 0 : (size_t)2 * dm + 2 * D;
}

template <bool INITIAL>
__global__ __launch_bounds__(256) void hk_thermal_kernel(ThermalArgs A) {
    extern __shared__ double smem[];
    __shared__ double wsum[4][4];
    constexpr int B = 16;
    const int D = A.th.dim, dm = A.th.dmodes, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    double *cs = nullptr, *sn = nullptr, *wv = smem;
    if constexpr (!INITIAL) {
        cs = smem; sn = smem + dm; wv = smem + 2 * dm;
        for (int k = threadIdx.x; k < dm; k += blockDim.x) {
            double s, c;
            sincos(A.th.omega[k] * A.time, &s, &c);
            cs[k] = c; sn[k] = s;
        }
        __syncthreads();
    }
    wv += (size_t)wave * thermal_wave_doubles(D, dm, A.th.diag, A.oc.diag);
    double acc[4] = {0, 0, 0, 0};
    const int64_t n = A.st.n, ntask = (n + B - 1) / B;
    for (int64_t task = (int64_t)blockIdx.x * nw + wave; task < ntask; task += (int64_t)gridDim.x * nw) {
        const int64_t base = task * B;
        const int cnt = (int)(n - base < B ? n - base : B);
        ThermalSums m = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < cnt; ++j) {
            const ThermalSums s = thermal_sums(A, A.qp + (base + j) * 2 * D, A.th.centres + (base + j) * 2 * dm, cs, sn, wv);
            if (lane == j) m = s;
        }
        if (lane < cnt) {
            const int64_t tr = base + lane;
            if constexpr (INITIAL) {
                if (A.vi_out) ((cplx *)A.vi_out)[tr] = overlap_value(A.oc.fac, m.sA, m.sB, m.sP, m.sC);
                if (A.nacq_out) ((cplx *)A.nacq_out)[tr] = c_make(A.nc.n2 + m.sR, (m.sN + m.sG) / SC_HBAR);
            } else {
                const cplx cvt = overlap_value_conj(A.oc.fac, m.sA, m.sB, m.sP, m.sC);
                const cplx c = signed_root(((const cplx *)A.st.c2)[tr], A.st.sgn[tr]);
                const cplx ph = action_phase(A.st.act[tr]);
                const double w = 1.0 / (A.mc_norm * A.probi[tr]);
                const cplx phi = c_exp(c_make(0.0, 0.5 * m.sF / SC_HBAR));
                const cplx cq = c_mul(phi, corr_c_term(cvt, ((const cplx *)A.vi)[tr], c, ph, w));
                acc[0] += cq.x; acc[1] += cq.y;
                ((cplx *)A.cq_out)[tr] = cq;
                if (A.has_nac) {
                    const cplx kq = corr_k_term(A.nc.n2, m.sN, m.sR, m.sG, ((const cplx *)A.nacq)[tr], cq);
                    acc[2] += kq.x; acc[3] += kq.y;
                    ((cplx *)A.kq_out)[tr] = kq;
                }
            }
        }
    }
    if constexpr (!INITIAL) {
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = wave_sum(acc[i]);      // fixed order: deterministic
        if (lane == 0) { for (int i = 0; i < 4; ++i) wsum[wave][i] = acc[i]; }
        __syncthreads();
        if (threadIdx.x < 4) {
            double s = 0;
            for (int w = 0; w < nw; ++w) s += wsum[w][threadIdx.x];
            A.partials[(size_t)blockIdx.x * 4 + threadIdx.x] = s;
        }
    }
}

int check_thermal(const char *who, const sc_thermal_consts *th, int D, int64_t n) {
    if (!th->omega || !th->map_q || !th->map_p || !th->q0 || !th->centres)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "%s: null pointer in sc_thermal_consts", who);
    if (th->dim != D || th->dmodes < 1 || th->dmodes > D || (th->diag && th->dmodes != D))
        return sc_fail(SC_ERR_BAD_ARGUMENT, "%s: D = %d, thermal constants for D = %d with d'' = %d (diag = %d)", who, D, th->dim,
                       th->dmodes, th->diag);
    if (D < 1 || D > TH_MAX_D || n > TH_MAX_N)
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: D = %d, n = %lld (D <= %d and n <= %lld are held)", who, D, (long long)n, TH_MAX_D,
                       (long long)TH_MAX_N);
    return SC_OK;
}

// waves per workgroup: four, two where the per-wave scratch of four would not fit 64 KB of LDS next to the tables
int thermal_waves(int D, int dm, int th_diag, int oc_diag) {
    return (2 * dm + 4 * thermal_wave_doubles(D, dm, th_diag, oc_diag)) * sizeof(double) <= 48 * 1024 ? 4 : 2;
}

constexpr int TH_SAMPLE_MAX_E = 512;     // 2 d' deviates and 2 d'' centre coordinates of one trajectory staged in LDS

struct ThermalSampleArgs {
    sc_state st;
    sc_thermal_consts th;
    const double *ilz;        // [2 d'][2 D] row-major: block_diag(iLq, iLp)
    const double *sigma_q, *sigma_p;      // [d''] standard deviations of Q_k, P_k
    double *centres_out;      // [n][2 d''] out
    double *zi_t, *probi, *xi_out;
    int dprime;
    double prob0;
    uint64_t seed, subsequence;
    int64_t first;
    int init_state;
};

// sample_initial_kernel (sc_sample.hip) with a centre per trajectory: the pairs 0 .. d' - 1 of the trajectory's Philox stream are
// its xi, bit for bit; the pairs d' .. d' + d'' - 1 give (Q_k, P_k) = (sigma_q[k] g, sigma_p[k] g')
__global__ __launch_bounds__(256) void sample_thermal_kernel(ThermalSampleArgs A) {
    __shared__ double xis[4][TH_SAMPLE_MAX_E];
    __shared__ double cens[4][TH_SAMPLE_MAX_E];
    const int D = A.st.dim, D2 = 2 * D, dp = A.dprime, dm = A.th.dmodes, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const PhiloxKey key = {(uint32_t)A.seed, (uint32_t)(A.seed >> 32)};
    const uint32_t sub_lo = (uint32_t)A.subsequence, sub_hi = (uint32_t)(A.subsequence >> 32) << 8;
    for (int64_t tr = (int64_t)blockIdx.x * 4 + wave; tr < A.st.n; tr += (int64_t)gridDim.x * 4) {
        const uint64_t g = (uint64_t)(A.first + tr);
        double half = 0.0;
        for (int p = lane; p < dp; p += 64) {
            double a, b;
            philox_normal_pair(g, (uint32_t)p, sub_hi, sub_lo, key, a, b);
            xis[wave][p] = a; xis[wave][dp + p] = b;
            half += a * a + b * b;
            if (A.xi_out) { A.xi_out[tr * 2 * dp + p] = a; A.xi_out[tr * 2 * dp + dp + p] = b; }
        }
        for (int k = lane; k < dm; k += 64) {
            double a, b;
            philox_normal_pair(g, (uint32_t)(dp + k), sub_hi, sub_lo, key, a, b);
            const double Q = A.sigma_q[k] * a, P = A.sigma_p[k] * b;
            cens[wave][k] = Q; cens[wave][dm + k] = P;
            A.centres_out[tr * 2 * dm + k] = Q; A.centres_out[tr * 2 * dm + dm + k] = P;
        }
        half = wave_sum(half);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int i = lane; i < D2; i += 64) {
            const bool pos = i < D;
            const int j0 = pos ? 0 : dp, a = pos ? i : i - D;
            double dz = 0.0;
            for (int j = 0; j < dp; ++j) dz = fma(A.ilz[(int64_t)(j0 + j) * D2 + i], xis[wave][j0 + j], dz);
            double c = pos ? A.th.q0[a] : 0.0;
            const double *coord = cens[wave] + (pos ? 0 : dm);
            if (A.th.diag) {
                c = fma((pos ? A.th.map_q : A.th.map_p)[a], coord[a], c);
            } else {
                const double *row = (pos ? A.th.map_q : A.th.map_p) + (size_t)a * dm;
                for (int k = 0; k < dm; ++k) c = fma(row[k], coord[k], c);
            }
            const double z = c + dz;
            A.zi_t[tr * D2 + i] = z;
            if (A.init_state) A.st.qp[tr * D2 + i] = z;
        }
        if (lane == 0) {
            A.probi[tr] = A.prob0 * exp(-0.5 * half);
            if (A.init_state) {
                A.st.act[tr] = 0.0;
                ((cplx *)A.st.c2)[tr] = c_make(1.0, 0.0);
                A.st.sgn[tr] = 1.0;
            }
        }
        __builtin_amdgcn_wave_barrier();         // xis[wave], cens[wave] are rewritten by the next trajectory
    }
}

}  // namespace

extern "C" int sc_hk_thermal_initial(const sc_thermal_consts *th, const sc_overlap_consts *ovl_i0, const sc_nac_consts *nc,
                                     const double *zi, int64_t n, double *vi_out, double *nacq_out, void *stream) {
    if (!th || !ovl_i0 || !zi || (!vi_out && !nacq_out)) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_thermal_initial: null argument");
    if (nacq_out && (!nc || !th->n1)) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_thermal_initial: nacq without coupling constants");
    if (n < 0) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_thermal_initial: n = %lld", (long long)n);
    if (int rc = check_thermal("sc_hk_thermal_initial", th, ovl_i0->dim, n)) return rc;
    if (n == 0) return SC_OK;
    ThermalArgs a = {};
    a.st.n = n; a.st.dim = th->dim;
    a.oc = *ovl_i0; a.th = *th; a.has_nac = nacq_out != nullptr;
    if (nc) a.nc = *nc;
    a.qp = zi; a.vi_out = vi_out; a.nacq_out = nacq_out;
    const int nw = thermal_waves(th->dim, th->dmodes, th->diag, ovl_i0->diag);
    const size_t lds = nw * thermal_wave_doubles(th->dim, th->dmodes, th->diag, ovl_i0->diag) * sizeof(double);
    hipLaunchKernelGGL(hk_thermal_kernel<true>, dim3(sc_correlate_grid(n, th->dim)), dim3(64 * nw), lds, (hipStream_t)stream, a);
    return sc_check_launch("sc_hk_thermal_initial");
}

extern "C" int sc_hk_correlate_thermal(const sc_state *st, double time, const sc_overlap_consts *ovl_t0, const sc_nac_consts *nc,
                                       const sc_thermal_consts *th, const double *vi, const double *probi, const double *nacq,
                                       double mc_norm, double *cq_out, double *kq_out, double *partials, void *stream) {
    if (!st || !ovl_t0 || !th || !vi || !probi || !cq_out || !partials || !st->qp || !st->act || !st->c2 || !st->sgn)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_correlate_thermal: null argument");
    if (nc && (!nacq || !kq_out || !th->n1))
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_correlate_thermal: nac constants without nacq, kq_out or n1");
    if (ovl_t0->dim != st->dim || st->n < 0) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_correlate_thermal: dimension mismatch");
    if (int rc = check_thermal("sc_hk_correlate_thermal", th, st->dim, st->n)) return rc;
    ThermalArgs a = {};
    a.st = *st; a.oc = *ovl_t0; a.th = *th; a.has_nac = nc != nullptr;
    if (nc) a.nc = *nc;
    a.time = time; a.qp = st->qp; a.vi = vi; a.probi = probi; a.nacq = nacq; a.mc_norm = mc_norm;
    a.cq_out = cq_out; a.kq_out = kq_out; a.partials = partials;
    const int nw = thermal_waves(th->dim, th->dmodes, th->diag, ovl_t0->diag);
    const size_t lds = (2 * (size_t)th->dmodes + nw * thermal_wave_doubles(th->dim, th->dmodes, th->diag, ovl_t0->diag)) * sizeof(double);
    hipLaunchKernelGGL(hk_thermal_kernel<false>, dim3(sc_correlate_grid(st->n, st->dim)), dim3(64 * nw), lds, (hipStream_t)stream, a);
    return sc_check_launch("sc_hk_correlate_thermal");
}

extern "C" int sc_sample_thermal(const sc_state *st, const double *ilz, const sc_thermal_consts *th, const double *sigma_q,
                                 const double *sigma_p, int32_t dprime, double prob0, uint64_t seed, uint64_t subsequence,
                                 int64_t first, int32_t init_state, double *centres_out, double *zi_t, double *probi,
                                 double *xi_out, void *stream) {
    if (!st || !ilz || !th || !sigma_q || !sigma_p || !centres_out || !zi_t || !probi)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_sample_thermal: null argument");
    if (st->n < 0 || st->dim < 1 || dprime < 1 || dprime > st->dim)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_sample_thermal: n = %lld, D = %d, d' = %d", (long long)st->n, st->dim, dprime);
    if (!th->map_q || !th->map_p || !th->q0 || th->dim != st->dim || th->dmodes < 1 || th->dmodes > st->dim ||
        (th->diag && th->dmodes != st->dim))
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_sample_thermal: thermal constants for D = %d with d'' = %d (diag = %d), state D = %d",
                       th->dim, th->dmodes, th->diag, st->dim);
    if (subsequence >> 56)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_sample_thermal: subsequence %llu does not fit the counter (< 2^56)",
                       (unsigned long long)subsequence);
    if (dprime + th->dmodes > 256 || st->dim > TH_MAX_D || st->n > TH_MAX_N)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_sample_thermal: d' + d'' = %d, D = %d, n = %lld (at most 256 pairs of deviates per "
                       "trajectory are drawn on the device; sample on the host and use set_thermal_initial_conditions)",
                       dprime + th->dmodes, st->dim, (long long)st->n);
    if (init_state && (!st->qp || !st->act || !st->mono || !st->c2 || !st->sgn))
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_sample_thermal: init_state needs the state buffers");
    if (st->n == 0) return SC_OK;
    ThermalSampleArgs a;
    a.st = *st; a.th = *th; a.ilz = ilz; a.sigma_q = sigma_q; a.sigma_p = sigma_p; a.centres_out = centres_out;
    a.zi_t = zi_t; a.probi = probi; a.xi_out = xi_out; a.dprime = dprime; a.prob0 = prob0; a.seed = seed;
    a.subsequence = subsequence; a.first = first; a.init_state = init_state;
    const int64_t quads = (st->n + 3) / 4;
    hipLaunchKernelGGL(sample_thermal_kernel, dim3((int)(quads < 4096 ? quads : 4096)), dim3(256), 0, (hipStream_t)stream, a);
    int rc = sc_check_launch("sc_sample_thermal");
    if (rc != SC_OK || !init_state) return rc;
    return sc_launch_mono_identity(st, (hipStream_t)stream);
}

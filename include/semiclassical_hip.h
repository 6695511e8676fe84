/*
 * semiclassical_hip.h -- C-ABI of the MI355X (gfx950) trajectory engine.
 *
 * The reference (humeniuka/semiclassical) has no FFI boundary: its hot path is a
 * sequence of eager PyTorch ops inside two Python classes.  This header is the
 * boundary the build introduces underneath those classes: every entry point
 * replaces one group of reference ops (cited per function, paths relative to the
 * reference repository).  The Python classes in semiclassical_amd/propagators.py
 * bind these symbols with ctypes (see INTEGRATION.md for the stub).
 *
 * Conventions
 *   - all pointers inside the structs are DEVICE pointers (torch owns every
 *     buffer; nothing is allocated, freed or retained by the library);
 *   - fp64 everywhere; complex numbers are interleaved (re, im) doubles;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream);
 *   - every function returns 0 on success or a negative SC_ERR_* code and never
 *     synchronises the device; sc_last_error() gives the message of the last
 *     failure on the calling thread.
 *
 * Engine-native state layout ("trajectory-major"):
 *     qp   [n][2*D]        q(0..D-1), p(0..D-1) of one trajectory are contiguous
 *     act  [n]             classical action S
 *     mono [n][4][D][D]    monodromy blocks Mqq, Mqp, Mpq, Mpp (row-major a,b)
 *     c2   [n] complex     HK prefactor squared  (the sign tracker's "previous")
 *     sgn  [n]             accumulated branch sign (+1/-1) of sqrt(c2)
 * The reference's (rows, n) tensor `y` is produced from / converted to this
 * layout by sc_state_from_reference / sc_state_to_reference.
 */
#ifndef SEMICLASSICAL_HIP_H
#define SEMICLASSICAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped on every change of a struct layout or a function signature below.  semiclassical_amd/_lib.py refuses a
 * library whose sc_abi_version() or struct sizes differ from its own declarations. */
#define SC_ABI_VERSION        18

#define SC_OK                 0
#define SC_ERR_BAD_ARGUMENT  -1
#define SC_ERR_UNSUPPORTED   -2   /* shape outside what the kernels hold on chip */
#define SC_ERR_LAUNCH        -3   /* hip launch / runtime error */

/* potential kinds: reference semiclassical/potentials.py */
#define SC_POT_MORSE          1   /* MorsePotential, chi != 0           potentials.py:274-327 */
#define SC_POT_HARMONIC_SEP   2   /* MorsePotential, all chi == 0       potentials.py:267-312 */
#define SC_POT_EPS_MORSE      3   /* NonHarmonicPotential               potentials.py:63-134  */
#define SC_POT_HARMONIC_DENSE 4   /* MolecularHarmonicPotential         potentials.py:553-593 */

typedef struct sc_potential {
    int32_t kind;           /* SC_POT_* */
    int32_t dim;            /* D */
    const double *par0;     /* MORSE: a[D]  HARMONIC_SEP: omega^2[D]  EPS_MORSE: eps[D]  DENSE: pos0[D]      */
    const double *par1;     /* MORSE: De[D]                            EPS_MORSE: b[D]    DENSE: grad0[D]     */
    const double *par2;     /*                                                            DENSE: hess0[D][D]  */
    double        scalar0;  /*                                                            DENSE: energy0 - origin */
    const double *inv_mass; /* 1/m [D]                                 potentials.py:261-263, 549 */
    const double *lin_prop; /* DENSE, optional (may be NULL): the RK4 step matrix Phi[2D][2D] = sum_{k<=4} (lin_dt G)^k / k!
                               of the monodromy equations, G = [[0, diag 1/m], [-hess0, 0]] (row-major).  One RK4
                               step of a linear constant-coefficient system is the product with Phi; sc_hk_step
                               uses it for its small-D register kernel when lin_dt equals the step it is called with. */
    double        lin_dt;
} sc_potential;

/* Storage order of the 4 D^2 doubles mono[i] of one trajectory.
 *   SC_MONO_ROWMAJOR  [4][D][D]: Mqq, Mqp, Mpq, Mpp one after the other, each row-major (a, b).  Every entry point
 *                     takes this order.
 *   SC_MONO_TILED16   16 x 16 tiles in the order (ra, rb) of tile rows / columns; tile (ra, rb) stores its nra x ncb
 *                     part (nra = min(16, D - 16 ra), ncb likewise) of the plane PAIR (Mqq, Mqp) element by element
 *                     (row-major inside the tile, the two planes of an element side by side), then the pair (Mpq, Mpp)
 *                     the same way (ABI 16; up to ABI 15 the four planes followed one another):
 *                         offset(p, a, b) = 4 (16 ra D + 16 nra rb) + (p / 2) 2 nra ncb + 2 ((a - 16 ra) ncb + (b - 16 rb)) + p % 2
 *                     A thread of the fast kernel then moves both planes of a pair with one 16-byte access.
 *                     Identical to SC_MONO_ROWMAJOR for D <= 16.  Only sc_hk_step on its separable / diagonal-width
 *                     fast path takes it (the 16 x 16 thread grid of that kernel then walks a trajectory linearly
 *                     through HBM); sc_mono_convert switches a state between the two in place. */
#define SC_MONO_ROWMAJOR 0
#define SC_MONO_TILED16  1

typedef struct sc_state {
    int64_t n;              /* trajectories in this batch (this rank's shard) */
    int32_t dim;            /* D */
    int32_t mono_layout;    /* SC_MONO_ROWMAJOR or SC_MONO_TILED16: storage order inside mono[i], see below */
    double *qp;
    double *act;
    double *mono;
    double *c2;
    double *sgn;
    double *work;           /* [n][4][D] scratch of the separable fast path: RK4 propagators of the monodromy rows */
    int32_t *flags;         /* [n + 2], zero-initialised scratch: flags[i] != 0 marks a trajectory whose determinant
                               the fast path hands to the fully pivoted elimination, flags[n] counts them for the
                               current step, flags[n + 1] is the cursor through which the fast kernel hands out
                               trajectories to its workgroups.  May be NULL: the fixed-pivot-order register kernels
                               (which rely on the fix-up) are then not used at all -- every trajectory takes the fully
                               pivoted LDS kernel, correct but several times slower */
} sc_state;

/* constants of the HK prefactor, reference propagators.py:951-1004.
 * diag != 0: Gamma_i, Gamma_t diagonal and of full rank; st = sqrt(diag Gamma_t),
 *            si = sqrt(diag Gamma_i).
 * diag == 0: L1 = U^T Gt^{1/2}, L2 = U^T Gt^{-1/2} (d' x D complex),
 *            R1 = Gi^{-1/2} U,  R2 = Gi^{1/2} U   (D x d' complex).
 *            real_lr != 0: the caller asserts that the imaginary parts of all four are zero (they are products of real
 *            matrices for positive semi-definite widths; the reference's complex128 copies carry rounding dust at most):
 *            the register kernels then run the sandwiches in real arithmetic.  0 is always correct. */
typedef struct sc_hk_consts {
    int32_t dim, dprime, diag, real_lr;
    const double *st, *si;
    const double *L1, *L2, *R1, *R2;
} sc_hk_consts;

/* constants of <q,p,G_bra | qk,pk,G_ket>, reference propagators.py:124-240.
 * diag != 0: A, B, C hold D diagonal entries, else D x D row-major.
 *   A = Gbra.iG.Gket   B = iG = (Gbra+Gket)^+   C = Gket.iG   fac = sqrt(2^rank sqrt(detGbra detGket)/detG) */
typedef struct sc_overlap_consts {
    int32_t dim, diag;
    const double *A, *B, *C;
    const double *qk, *pk;  /* centre of the ket, [D] each */
    double fac;
} sc_overlap_consts;

/* constants of the non-adiabatic coupling factors, reference propagators.py:886-903
 *   n1 = -hbar^2 nac/m ;  rn = R.n1 with R = G0.iGi0.Gi ;  gn = (G0.iGi0)^T.n1 ;
 *   p0n1 = p0.n1 ;  n2 = -hbar^2/2 sum_k tau2_k/m_k (0 for every reference potential) */
typedef struct sc_nac_consts {
    int32_t dim, _pad;
    const double *rn, *gn;
    const double *q0, *p0;
    double p0n1, n2;
} sc_nac_consts;

/* constants and per-trajectory tracker state of the Walton-Manolopoulos prefactor, reference
 * propagators.py:1102-1130 (_prepare), :1195-1389 (_prefactor).  e = 2 d'.
 *   U     D x d' (real)      eigenvectors of Gamma_0 + Gamma_i with non-zero eigenvalue      :495-498
 *   Gt, G0, iGi0, S = iGi0.G0, Cqq = G0 - G0.iGi0.G0                     D x D real          :1280-1296
 *   Cst   e x e complex = U2^T (2 filinov + Eqz^T Gi Eqz - 2i/hbar Epz^T Eqz) U2            :1227-1238
 *   Bq    D x e complex = [Gi U, -i/hbar U]                                                  :1264
 *   n1 = -hbar^2 tau1/m, s_n1 = S n1, w_n1 = G0 n1 (NULL until the potential is known)       :1693
 *   inv_scale_a = 1/(2 sqrt(alpha beta))   :1328       inv_two_pi = 1/(2 pi)   :1358
 *   pre = detG0^1/2 detGt^1/4 detGi^1/4 / sqrt(detGi0) with the pi-absorbing determinants    :1116-1125, 1598-1599
 *   detA, detM [n] complex + sgnA, sgnM [n]: "previous" values and branch signs of the two trackers :1336, 1389 */
typedef struct sc_wm_consts {
    int32_t dim, dprime;
    const double *U, *Gt, *G0, *iGi0, *S, *Cqq;
    const double *Cst, *Bq;
    const double *q0, *p0;
    const double *n1, *s_n1, *w_n1;
    double inv_scale_a, inv_two_pi, pre, p0n1, n2;
    double *detA, *detM, *sgnA, *sgnM;
    /* optional per-trajectory export behind WaltonManolopoulosPropagator.coefficients() / wavefunction() / norm()
     * (propagators.py:1391-1575); each may be NULL:
     *   coef_out [n] complex   v_n of eqn (75) without the x-dependent part, :1408-1432, with
     *                          pre_coef = detG0^1/4 detGt^1/4 detGi^1/4 / sqrt(detGi0)
     *   cqq_out  [n][D][D] complex   C_QQ of eqn (70)
     *   dvec_out [n][D] complex      C_qQ^T (q0 - q) + i/hbar PI_Q, :1513 */
    double pre_coef;
    double *coef_out, *cqq_out, *dvec_out;
    /* matrix storage for shapes whose per-trajectory matrices exceed the LDS of a compute unit (D >~ 24 at full
     * rank): sc_wm_scratch_bytes(n, D, d') bytes of device memory, 0 / NULL when not needed.  Contents are scratch. */
    double *scratch;
    int64_t scratch_bytes;
    /* [n + 1] int32 scratch, or NULL.  The register-resident kernel eliminates in a fixed pivot order; a trajectory
     * whose pivot falls more than a factor 16 below what partial pivoting would have picked is marked flags[i] = 1
     * (flags[n] counts them) and recomputed with full partial pivoting by the LDS kernel in the same call.  NULL: the
     * register kernel is not used, every trajectory takes the fully pivoted LDS kernel. */
    int32_t *flags;
    /* [n][3 D + 3] or NULL.  Position-dependent derivative couplings (potentials whose derivative_coupling_1st / _2nd
     * depend on r; the reference evaluates them at the initial and the current points of every trajectory,
     * propagators.py:1685-1693): per trajectory n1(q_i)[D], S n1(q_i)[D], G0 n1(Q)[D], p0.n1(Q), n2(q_i), n2(Q), filled by
     * the caller before every call; they replace n1, s_n1, w_n1, p0n1, n2 above and route the call to the LDS / scratch
     * kernels. */
    const double *nac_traj;
} sc_wm_consts;

/* sGDML force field, reference semiclassical/gdml_predictor.py:57-85 (constructor) and :96-250 (forward).
 *   xs_train, jx_alphas [n_train][n_desc]: permutation-expanded training descriptors and Jacobian-contracted
 *   coefficients (16-byte aligned: the kernels copy blocks of rows with 16-byte loads); pair_k/pair_l [n_desc]: atoms (k > l) of descriptor d in torch.tril_indices order;
 *   q = sqrt(5)/sigma; energies are returned relative to `origin` (potentials.py:699). */
typedef struct sc_gdml_model {
    int32_t n_atoms, n_desc, n_train, _pad;
    const double *xs_train, *jx_alphas;
    const int32_t *pair_k, *pair_l;
    double q, c, std, origin;
    const double *inv_mass;     /* [3 n_atoms] */
} sc_gdml_model;

/* per-trajectory scratch of the unfused RK4 step for dense, position-dependent Hessians */
typedef struct sc_dense_scratch {
    double *hess;   /* [n][4][D][D]  stage Hessians */
    double *kprev;  /* [n][2D]       slopes of (q, p) of the previous stage */
    double *ksum;   /* [n][2D]       weighted slope sums k1 + 2 k2 + 2 k3 (+ k4) */
    double *ssum;   /* [n]           weighted sums of T - V */
} sc_dense_scratch;

int         sc_version(void);
const char *sc_last_error(void);
/* ABI guard: SC_ABI_VERSION the library was compiled with; sizeof of the struct called `name` ("sc_state", ...), or
 * -1 for an unknown name; 1 if the library is a tuning build (-DSC_TUNING: reads experiment knobs from the
 * environment), 0 for the product build. */
int sc_abi_version(void);
int sc_struct_size(const char *name);
int sc_tuning_build(void);

/* number of workgroups sc_hk_step / sc_hk_correlate use for n trajectories of dimension D;
 * the caller sizes the `partials` buffers with it. */
int sc_step_grid(int64_t n, int32_t dim);
int sc_correlate_grid(int64_t n, int32_t dim);

/* In-place change of st->mono between the storage orders (the caller updates st->mono_layout afterwards);
 * `to_layout` is the order wanted, st->mono_layout the order the data is in.  D <= 64. */
int sc_mono_convert(const sc_state *st, int32_t to_layout, void *stream);

/* y (rows = 2D+4D^2+1, n) with n fastest  <->  engine layout.   reference propagators.py:329-334, 581 */
int sc_state_from_reference(const double *y, const sc_state *st, void *stream);
int sc_state_to_reference(const sc_state *st, double *y, void *stream);

/* Initial conditions sampled ON THE DEVICE, replaces the sampling half of HermanKlukPropagator.initial_conditions
 * (propagators.py:537-566: xi ~ N(0,1) of shape (2d', n), zi = z0 + iLz^T xi, probi = detLz/(2 pi)^D exp(-|xi|^2/2))
 * and, with init_state != 0, the construction of y(0) (:581-603: q, p = zi, S = 0, Mqq = Mpp = 1; also c2 = 1,
 * sgn = 1; st->mono is written ROW-MAJOR).
 *   ilz   [2d'][2D] row-major = block_diag(iLq, iLp) (:506-528), z0 [2D] = (q0, p0), prob0 = detLz/(2 pi)^D
 *   zi_t  [n][2D] out, probi [n] out, xi_out [n][2d'] out or NULL (the deviates themselves)
 * Deviates: Philox4x32-10 + Box-Muller, key = seed, counter = (trajectory index, pair index, subsequence): deviate j of the
 * trajectory with GLOBAL index first + i depends only on (seed, subsequence, first + i, j) -- not on n, the launch shape or
 * the rank that draws it -- and distinct (seed, subsequence) never share a stream.  d' <= 256, subsequence < 2^56. */
int sc_sample_initial(const sc_state *st, const double *ilz, const double *z0, int32_t dprime, double prob0,
                      uint64_t seed, uint64_t subsequence, int64_t first, int32_t init_state, double *zi_t,
                      double *probi, double *xi_out, void *stream);

/* One RK4 step of (q,p,Mqq,Mqp,Mpq,Mpp,S) followed by the HK prefactor and its sqrt-branch tracking,
 * fused per trajectory.  Replaces _rk4_step + EquationsOfMotion.f + potential.harmonic_approximation
 * (propagators.py:86-119, 313-383) and _prefactor + _track_signs_of_sqrt (propagators.py:951-1052).
 *   energy_partials[sc_step_grid()]: per-workgroup sums of T+V at the k4 stage (propagators.py:380).
 *   mode 0: step + prefactor;  mode 1: prefactor only with tracker initialisation (t = 0, propagators.py:631). */
int sc_hk_step(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk,
               double dt, int32_t mode, double *energy_partials, void *stream);

/* TWO consecutive time steps per visit of a trajectory (round 4): the same arithmetic as two calls of sc_hk_step, for the
 * separable / diagonal-width fast path with 16 < D <= 64 on the tiled storage order (sc_hk_step_multi_supported).  A workgroup
 * streams a trajectory's monodromy blocks M(k), applies step k in registers and eliminates -- for D > 32 WITHOUT storing -- and streams the
 * SAME blocks again: these loads hit the L2 / memory-side cache instead of HBM (profiles/pair_nostore_revisit.txt); it applies
 * step k and then step k + 1 (the same fma sequence: the bits of M(k+1) are those sc_hk_step would have stored), stores M(k+2)
 * and eliminates.  Two of the four HBM transfers of two time steps are gone.  Between the two sub-steps, and until the stores of
 * the second one, the blocks in memory are those of the visit's START, M(k): M(k+1) never exists in memory (D <= 32: the first
 * sub-step stores M(k+1) and the second reloads it, as in round 4; callers must not rely on either).  Results are
 * bit-identical to two sc_hk_step calls (tests/test_hk_multi_gpu.py, tests/test_pair_no_mid_store_gpu.py).  Measured at
 * D = 60, n = 1e5 in round 4, with the intermediate store: 4.38 instead of 4.55 ms per step -- the elimination (FP64 VALU issue)
 * bounds the kernel, not the streaming phase (profiles/r4_sd_phases.txt); without the store: docs/NOTEBOOK.md section 9.2.
 *   ms->work    [2][n][4][D]   row propagators of both sub-steps (scratch)
 *   ms->qp_mid  [n][2D], act_mid [n], c2_mid [n] complex, sgn_mid [n]: the state BETWEEN the two steps -- what sc_hk_correlate of
 *               the second time step reads (pass an sc_state whose qp / act / c2 / sgn point to them)
 *   ms->unrepaired   one int32 on the device, zeroed by the caller.  The fix-up of a weak in-block pivot (sc_state.flags) needs
 *               the blocks the determinant belongs to; those of the FIRST sub-step are not in memory (any more).  The kernel counts such
 *               determinants here: non-zero after the call = the intermediate determinants (and everything derived from them)
 *               are not reliable, redo the two steps from a saved state with sc_hk_step.  Monodromy blocks that are
 *               diagonal (separable potential from M(0) = 1) cannot have weak pivots; HermanKlukPropagator.run() takes this
 *               entry point only then.
 *   energy_partials [2][sc_step_grid()]: sums of T+V at the k4 stage of either step (two sc_energy_guard calls). */
typedef struct sc_multi_scratch {
    double *work, *qp_mid, *act_mid, *c2_mid, *sgn_mid;
    int32_t *unrepaired;
} sc_multi_scratch;
int sc_hk_step_multi_supported(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk);
int sc_hk_step_multi(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, const sc_multi_scratch *ms,
                     double dt, double *energy_partials, void *stream);

/* KS = `ksteps` consecutive time steps per visit of a trajectory, 2 <= ksteps <= 4 (an addition: the ABI number stays): sc_hk_step_multi for a general
 * number of sub-steps, the same arithmetic as ksteps calls of sc_hk_step.  ksteps = 2 IS sc_hk_step_multi (same kernels).
 * ksteps = 3, 4 exist for 32 < D <= 64 only (sc_hk_step_visit_supported), in the store-free scheme: sub-step ks loads the blocks
 * of the visit's start M(k) (the first load allocates in the cache, every later one re-reads the same lines), applies the row
 * propagators P(0) .. P(ks) one after the other with the explicit fma sequence of sc_hk_step, forms its prefactor matrix and
 * determinant, and only the LAST sub-step stores: M(k + ksteps).  Per time step 1 / ksteps of a read pass from HBM and
 * 1 / ksteps of a write pass; until the last sub-step's stores the blocks in memory are M(k).  Bit-identical to ksteps calls
 * of sc_hk_step (tests/test_visit_steps_gpu.py); measurements: docs/NOTEBOOK.md section 9.3.
 *   ms->work    [ksteps][n][4][D]
 *   ms->qp_mid  [ksteps - 1][n][2D], act_mid [ksteps - 1][n], c2_mid [ksteps - 1][n] complex, sgn_mid [ksteps - 1][n]: the
 *               states after sub-step 0 .. ksteps - 2 (one sc_state view per intermediate state for sc_hk_correlate)
 *   ms->unrepaired   as for sc_hk_step_multi: counts weak in-block pivots of ALL intermediate sub-steps; the fix-up launch
 *               repairs the last sub-step's determinant from M(k + ksteps) in memory
 *   energy_partials [ksteps][sc_step_grid()] (ksteps sc_energy_guard calls). */
int sc_hk_step_visit_supported(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, int32_t ksteps);
int sc_hk_step_visit(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, const sc_multi_scratch *ms,
                     double dt, double *energy_partials, int32_t ksteps, void *stream);

/* out[i] = <qp[i] , G_bra | qk,pk,G_ket> for i < n  (complex).  propagators.py:181-240 with a single ket. */
int sc_overlap(const sc_overlap_consts *oc, const double *qp, int64_t n, double *out, void *stream);

/* nac factor of the INITIAL points: nacq = n2 + (q0-q).rn + i/hbar (p0n1 + (p-p0).gn).  propagators.py:902-903 */
int sc_nac_initial(const sc_nac_consts *nc, const double *zi, int64_t n, double *nacq, void *stream);

/* Per-trajectory terms of C_auto and k_ic for the current state and their per-workgroup partial sums.
 * Replaces autocorrelation_qp / autocorrelation / ic_correlation (propagators.py:784-911) up to the
 * phase exp(i t E0/hbar), which the host applies.
 *   w_i      = 1 / (mc_norm * probi_i),  mc_norm = N_total (2 pi hbar)^D      propagators.py:837
 *   cq_i     = conj(vt_i) vi_i sgn_i sqrt(c2_i) exp(i S_i/hbar) w_i           propagators.py:806
 *   kq_i     = nacQ_i nacq_i cq_i / hbar^2  (skipped when nc == NULL)         propagators.py:900-909
 *   partials[sc_correlate_grid()][4] = sums of (cq.re, cq.im, kq.re, kq.im) per workgroup
 *   cq_out / kq_out (complex [n]) may be NULL. */
int sc_hk_correlate(const sc_state *st, const sc_overlap_consts *ovl_t0, const sc_nac_consts *nc,
                    const double *vi, const double *probi, const double *nacq, double mc_norm,
                    double *cq_out, double *kq_out, double *partials, void *stream);

/* ---- Monte-Carlo second moments (standard errors of C_auto and k_ic) -----------------------------------------------------
 * Every entry point with a trailing moments argument does what the one without it does -- same launches, C and k bit for bit --
 * and in addition forms, per time step, the six sums over the trajectories
 *     S_rr(C) = sum (Re cq_i)^2, S_ii(C) = sum (Im cq_i)^2, S_ri(C) = sum Re cq_i Im cq_i, and the same three of kq_i
 * (cq_i, kq_i as defined at sc_hk_correlate: weight included, dynamical phase not), in a fixed summation order.  NULL there
 * gives the old launch.  The host rotates them by the phase and forms the standard errors (propagators.py, finalize_moments).
 *   sc_hk_correlate_m   moment_partials[sc_correlate_grid()][6]
 *   sc_term_moments     the six sums of exported terms cq[n], kq[n] (complex; kq may be NULL: its sums are 0) into
 *                       moment_partials[sc_term_moments_grid(n)][6] -- for the Walton-Manolopoulos terms of sc_wm_correlate
 *                       (a pass of its own, not fused into the WM kernels) and for k_ic terms the caller forms itself
 *                       (position-dependent couplings)
 *   sc_reduce_moments   moments[0..5] = sum of n_rows partial rows
 *   sc_reduce_slot_moments_at   ONE launch: the slot sums of sc_reduce_slot_at into row *cursor of slots[.][5], the moment sums
 *                       into row *cursor of moments[.][6], then *cursor += 1 (the graph-captured loop of run(use_graph=True)) */
int sc_hk_correlate_m(const sc_state *st, const sc_overlap_consts *ovl_t0, const sc_nac_consts *nc,
                      const double *vi, const double *probi, const double *nacq, double mc_norm,
                      double *cq_out, double *kq_out, double *partials, double *moment_partials, void *stream);
int sc_term_moments_grid(int64_t n);
int sc_term_moments(const double *cq, const double *kq, int64_t n, double *moment_partials, void *stream);
int sc_reduce_moments(const double *moment_partials, int32_t n_rows, double *moments, void *stream);
int sc_reduce_slot_moments_at(const double *corr_partials, int32_t n_corr, const double *moment_partials, int32_t n_mom,
                              double *slots, double *moments, int64_t *cursor, void *stream);

/* slot[0..3] = sum of correlate partials, slot[4] = (sum of energy partials)/n_energy.
 * Deterministic (fixed summation order).  Either partial buffer may be NULL (its slots are left untouched). */
int sc_reduce_slot(const double *corr_partials, int32_t n_corr, const double *energy_partials, int32_t n_energy_blocks,
                   double n_energy, double *slot, void *stream);

/* The same sums into ROW *cursor of slots[.][5], then *cursor += 1 (cursor: one int64 in device memory).  With the
 * destination held on the device a launch sequence "correlate, reduce, step" has no argument that changes from step to
 * step: it is captured once in a HIP graph and replayed (HermanKlukPropagator.run(use_graph=True)). */
int sc_reduce_slot_at(const double *corr_partials, int32_t n_corr, double *slots, int64_t *cursor, void *stream);

/* The WHOLE caller loop (cli.py:401-436: nsteps times "autocorrelation, ic_correlation, step") in one launch, for
 *   - separable potentials (SC_POT_MORSE / HARMONIC_SEP / EPS_MORSE) with diagonal width matrices and D <= 12,
 *   - a constant dense Hessian (SC_POT_HARMONIC_DENSE with its step matrix lin_prop built for this dt), any width matrices
 *     (hk->real_lr for dense ones), at the small molecular shapes D <= 12 the library instantiates (methylium: D = 12, d' = 6):
 * a trajectory is loaded once into registers, runs all steps there and is written back once (sc_hk_run_supported says
 * whether the combination qualifies; everything else takes sc_hk_correlate / sc_hk_step step by step).  Arguments as for
 * sc_hk_correlate and sc_hk_step.  partials: scratch of 5 * sc_hk_run_slots(n, D) * nsteps doubles;
 * slots_out [nsteps][5]: row k = Re C, Im C, Re k, Im k summed over the trajectories for the state BEFORE step k (what
 * sc_hk_correlate + sc_reduce_slot give) and the mean <T+V> at the k4 stage of step k; elog: the energy-guard log of
 * sc_energy_guard, advanced by nsteps steps. */
int sc_hk_run_slots(int64_t n, int32_t dim);
int sc_hk_run_supported(const sc_potential *pot, const sc_hk_consts *hk, const sc_overlap_consts *ovl_t0);
int sc_hk_run(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, const sc_overlap_consts *ovl_t0,
              const sc_nac_consts *nc, const double *vi, const double *probi, const double *nacq, double mc_norm,
              double dt, int32_t nsteps, double *partials, double *slots_out, double *elog, void *stream);

/* sc_hk_run / sc_hk_run_modal with the per-step second moments (see sc_hk_correlate_m) in moments_out[nsteps][6]; `partials` then
 * holds sc_hk_run_scratch_doubles(n, D, nsteps, 1) doubles (with moments = 0: the 5 * sc_hk_run_slots * nsteps of sc_hk_run). */
int64_t sc_hk_run_scratch_doubles(int64_t n, int32_t dim, int32_t nsteps, int32_t moments);
int sc_hk_run_m(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, const sc_overlap_consts *ovl_t0,
                const sc_nac_consts *nc, const double *vi, const double *probi, const double *nacq, double mc_norm,
                double dt, int32_t nsteps, double *partials, double *slots_out, double *elog, double *moments_out, void *stream);

/* ---- Block sums (Monte-Carlo error bars of anything linear in C_auto(t), k_ic(t): the rate k_ic(E)) ------------------------
 * A batch is split into B fixed blocks, B a power of two in 2 ... 64 (anything else: SC_ERR_BAD_ARGUMENT): the trajectory with
 * rank-local index i belongs to block (i >> 2) & (B - 1).  Per time step the entry points below ADD NOTHING to the state or to the
 * slot sums; they form, from terms the existing kernels already produce,
 *     out[b][0..3] = Re sum cq_i, Im sum cq_i, Re sum kq_i, Im sum kq_i   over the trajectories i of block b
 * with cq_i, kq_i as defined at sc_hk_correlate (propagators.py:784-911: 806 and 837 for cq_i, 900-909 for kq_i; weight included,
 * dynamical phase not), so that sum_b out[b] is the slot row of the step.  One writer per output, fixed summation order: the same
 * bits in every run.  The host evaluates a linear functional on every block's own estimate out[b] N / n_b and takes the standard
 * error from the spread of the B values (hostmath.block_standard_error, rates.rate_standard_error).
 *   sc_term_blocks      adds the block sums of the EXPORTED per-trajectory terms cq[n], kq[n] (complex; what sc_hk_correlate(_m)
 *                       writes to cq_out / kq_out, sc_wm_correlate to its term arrays, or the caller forms itself for
 *                       position-dependent couplings) into out[B][4].  kq may be NULL: the k columns are 0.
 *   sc_term_blocks_at   the same into ROW *cursor of out_base[.][B][4] (cursor as for sc_reduce_slot_at).  It reads the cursor and
 *                       never advances it: launch it BEFORE the reduction that does.
 *   sc_hk_run_blocks    adds, for the whole-loop entry points (sc_hk_run, sc_hk_run_m, sc_hk_run_modal, sc_hk_run_modal_m), the
 *                       block sums of their per-wavefront `partials` [nsteps][sc_hk_run_slots(n, dim)][5] of the launch that just
 *                       ran into out[nsteps][B][4]: wavefront slot s holds the trajectories with (i >> 2) mod slots == s, and the
 *                       slot count either does not wrap (slot = i >> 2) or is a multiple of B, so block = s mod B; anything else
 *                       is refused (SC_ERR_UNSUPPORTED).  Same stream, before `partials` is reused. */
int sc_term_blocks(const double *cq, const double *kq, int64_t n, int32_t B, double *out, void *stream);
int sc_term_blocks_at(const double *cq, const double *kq, int64_t n, int32_t B, double *out_base, const int64_t *cursor,
                      void *stream);
int sc_hk_run_blocks(const double *partials, int64_t n, int32_t dim, int32_t nsteps, int32_t B, double *out, void *stream);

/* sc_hk_run for a CONSTANT dense Hessian with the monodromy blocks of the state in NORMAL-MODE coordinates (round 4).  RK4 of a
 * linear system commutes with a change of basis: with W = m^-1/2 H m^-1/2 = U diag(lambda) U^T, A = m^-1/2 U, B = m^1/2 U and
 *     Mqq~ = A^-1 Mqq A,  Mqp~ = A^-1 Mqp B,  Mpq~ = B^-1 Mpq A,  Mpp~ = B^-1 Mpp B
 * the step matrix Phi(dt) of sc_potential.lin_prop becomes 2 x 2 per mode, mode_prop[a] = (phi_qq, phi_qp, phi_pq, phi_pp)_a =
 * the RK4 polynomial of dt [[0, 1], [-lambda_a, 0]], and the prefactor is the same expression of the transformed blocks with
 * L1 A, L2 B, A^-1 R1, B^-1 R2 as the prefactor constants -- real, dense: diag = 0.  The CALLER transforms st->mono before the call and back
 * after it (HermanKlukPropagator.run does, with two batched products); (q, p, S), the correlation terms and the energy guard are
 * in the original coordinates as in sc_hk_run.  Per lane and step 8 D multiply-adds replace the 8 D^2 of the product with Phi. */
/* mono[i][p] <- left[p] . mono[i][p] . right[p] for the four blocks p = qq, qp, pq, pp of every trajectory (left, right: [4][D][D],
 * row-major state, D <= 64): the change of basis in front of and behind sc_hk_run_modal / sc_hk_step_modal.  D <= 16 and
 * 16 < D <= 64 are two kernels (ABI 18 widened the range; the results for D <= 16 are those of ABI 17 bit for bit). */
int sc_mono_similarity(const sc_state *st, const double *left, const double *right, void *stream);
int sc_hk_run_modal_supported(const sc_potential *pot, const sc_hk_consts *hk, const sc_overlap_consts *ovl_t0);
int sc_hk_run_modal(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, const sc_overlap_consts *ovl_t0,
                    const sc_nac_consts *nc, const double *vi, const double *probi, const double *nacq, double mc_norm,
                    double dt, int32_t nsteps, const double *mode_prop, double *partials, double *slots_out, double *elog, void *stream);
int sc_hk_run_modal_m(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, const sc_overlap_consts *ovl_t0,
                      const sc_nac_consts *nc, const double *vi, const double *probi, const double *nacq, double mc_norm,
                      double dt, int32_t nsteps, const double *mode_prop, double *partials, double *slots_out, double *elog,
                      double *moments_out, void *stream);

/* One HK time step for a CONSTANT dense Hessian (SC_POT_HARMONIC_DENSE) at 16 < D <= 64 with the monodromy blocks of the state in
 * NORMAL-MODE coordinates (ABI 18).  Same contract as sc_hk_step (replaces _rk4_step + EquationsOfMotion.f, propagators.py:86-119,
 * 313-383, and _prefactor + _track_signs_of_sqrt, propagators.py:951-1052; energy_partials[sc_step_grid()]; mode 0 = step +
 * prefactor, 1 = prefactor only with tracker initialisation), except that
 *   - st->mono holds Mqq~, Mqp~, Mpq~, Mpp~ (row-major, the transformation of sc_hk_run_modal above; the caller converts with
 *     sc_mono_similarity) and the step multiplies row a of the plane pairs (Mqq~, Mpq~), (Mqp~, Mpp~) by the 2 x 2 matrix
 *     mode_prop[a] = (phi_qq, phi_qp, phi_pq, phi_pp)_a;
 *   - hk holds the transformed constants L1 A, L2 B, A^-1 R1, B^-1 R2 (dense: diag = 0, real_lr = 1; d' <= D; diagonal width
 *     matrices are passed as dense diagonal L, R);
 *   - (q, p, S) stay Cartesian.
 * The prefactor is formed from the new blocks on chip by FP64 matrix-core products; the determinant is a pivoted LU.
 * sc_hk_step_modal_supported: 1 if the combination is held (else the call fails with SC_ERR_UNSUPPORTED). */
int sc_hk_step_modal_supported(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk);
int sc_hk_step_modal(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, double dt, int32_t mode,
                     const double *mode_prop, double *energy_partials, void *stream);

/* Walton-Manolopoulos: Filinov matrix A (eqn 50), its inverse and determinant, Gt/Gti/CQQ/M (57-78), the second
 * inverse and determinant, the trackers of sqrt(detA), sqrt(detM) and the per-trajectory terms of eqns (85), (100),
 * fused per trajectory.  Replaces WaltonManolopoulosPropagator._expand_L/_prefactor/autocorrelation_qp/
 * autocorrelation/ic_correlation (propagators.py:1132-1389, 1577-1719) after sc_hk_step has advanced the state.
 *   track: 2 initialise the trackers (t = 0), 1 track against the previous step, 0 recompute with the stored signs
 *   has_nac == 0: k_ic terms are skipped (wc->n1 etc. may be NULL)
 *   cq_out/kq_out complex [n] may be NULL; partials[sc_wm_grid()][4] as in sc_hk_correlate.
 * Three kernels behind it: a register-resident one (D <= 16, e <= 16 at the instantiated shapes), one with every matrix of
 * the trajectory in LDS, and the same with the matrices in wc->scratch for shapes beyond the LDS (no size limit other
 * than memory: sc_wm_scratch_bytes says how much scratch the call needs, 0 if none, -1 for invalid shapes).
 * sc_wm_grid: rows of `partials` the caller provides and sums (the kernels' own slots + those of the pivoted re-run). */
int sc_wm_grid(int64_t n, int32_t dim);
int64_t sc_wm_scratch_bytes(int64_t n, int32_t dim, int32_t dprime);
int sc_wm_correlate(const sc_state *st, const sc_wm_consts *wc, const double *zi, const double *probi,
                    double mc_norm, int32_t track, int32_t has_nac, double *cq_out, double *kq_out,
                    double *partials, void *stream);

/* partner atoms per atom the single-workgroup sGDML kernels (one workgroup per geometry, everything in LDS and registers)
 * instantiated for a molecule of n_atoms atoms hold (8, 16, 20, 24, 32, 40 or 48); -1 beyond 48 atoms, where
 * sc_gdml_eval / sc_gdml_stage take the multi-kernel route with caller-owned scratch instead */
int sc_gdml_row_len(int32_t n_atoms);
/* largest molecule sc_gdml_eval / sc_gdml_stage accept (170 atoms: 3N <= 510); beyond it they return SC_ERR_UNSUPPORTED */
int sc_gdml_max_atoms(void);
/* bytes of the `scratch` sc_gdml_eval_scratch / sc_gdml_stage_scratch need for a model of n_atoms atoms and n_train (permutation-expanded) training
 * points: 0 for n_atoms <= 48; above, a fixed batch of geometries (the calls walk n in batches, so the size does not
 * depend on n); -1 beyond sc_gdml_max_atoms() */
int64_t sc_gdml_scratch_bytes(int32_t n_atoms, int32_t n_train);

/* E - origin [n], dE/dr [n][3N], d2E/drdr [n][3N][3N] of the sGDML model at the geometries r [n][3N].
 * Replaces GDMLPredict.forward / MolecularGDMLPotential.harmonic_approximation (gdml_predictor.py:96-250). */
int sc_gdml_eval(const sc_gdml_model *g, const double *r, int64_t n, double *energy, double *grad, double *hess,
                 void *stream);
/* the same with caller-owned device scratch of sc_gdml_scratch_bytes(n_atoms, n_train) bytes (one buffer per stream: the
 * call writes it), required beyond 48 atoms and NULL allowed where that size is 0; sc_gdml_eval = scratch NULL */
int sc_gdml_eval_scratch(const sc_gdml_model *g, double *scratch, const double *r, int64_t n, double *energy, double *grad,
                         double *hess, void *stream);

/* One RK4 stage (stage = 0..3) of (q, p, S) on the sGDML surface: stage point from the previous slope, potential
 * evaluation, slopes, stage Hessian -> sc->hess; stage 3 also writes the new (q, p, S) and the per-workgroup sums of
 * T+V (energy_partials[sc_dense_grid()]).  With sc_dense_mono_step it replaces _rk4_step / EquationsOfMotion.f
 * (propagators.py:86-119, 313-383) for potentials whose Hessian is dense and position dependent. */
int sc_dense_grid(int64_t n);
/* The same RK4 bookkeeping of (q, p, S) for potentials the CALLER evaluates (any object with the reference's potential
 * protocol, potentials.py:41-204): per stage, sc_stage_point writes the stage positions r_out [n][D], the caller
 * evaluates V [n], grad [n][D] (and copies its Hessians into sc->hess[n][stage][D][D]), sc_stage_consume advances the
 * slopes / sums exactly as sc_gdml_stage does (energy_partials[sc_dense_grid()] at stage 3). */
int sc_stage_point(const sc_state *st, const sc_dense_scratch *sc, double dt, int32_t stage, double *r_out, void *stream);
int sc_stage_consume(const sc_state *st, const sc_dense_scratch *sc, const double *inv_mass, const double *V,
                     const double *grad, double dt, int32_t stage, double *energy_partials, void *stream);
int sc_gdml_stage(const sc_gdml_model *g, const sc_state *st, const sc_dense_scratch *sc, double dt, int32_t stage,
                  double *energy_partials, void *stream);
/* sc_gdml_stage with caller-owned device scratch (as sc_gdml_eval_scratch) */
int sc_gdml_stage_scratch(const sc_gdml_model *g, double *scratch, const sc_state *st, const sc_dense_scratch *sc, double dt,
                          int32_t stage, double *energy_partials, void *stream);

/* RK4 of the four monodromy blocks with the four stage Hessians hess[n][4][D][D] (each used as A[i][k] = hess[k][i];
 * the built-in potentials produce symmetric images), then the HK prefactor (diagonal or dense/rank-deficient width
 * matrices) and its branch tracking.  D <= 96: on the FP64 matrix cores; for 64 < D the RK4 sums do not fit the
 * register file and live in `mono_sums`.  D > 96: no size limit -- every matrix of a trajectory in a per-workgroup block
 * of `mono_sums`, products on the vector ALUs, pivoted LU on global memory (slow, kept for parity with the unbounded
 * reference).  `mono_sums`: sc_dense_mono_scratch_bytes(n, D, d') bytes (0: may be NULL).
 * mode: 0 = step + prefactor, 1 = prefactor and tracker initialisation only. */
int64_t sc_dense_mono_scratch_bytes(int64_t n, int32_t D, int32_t dprime);
int sc_dense_mono_step(const sc_state *st, const sc_hk_consts *hk, const double *inv_mass, const double *hess,
                       double *mono_sums, double dt, int32_t mode, void *stream);

/* Structure-exploiting HK step ("separable shortcut"): same contract as sc_hk_step for a
 * separable potential (SC_POT_MORSE / _HARMONIC_SEP / _EPS_MORSE), diagonal width matrices (hk->diag) and monodromy
 * blocks that are diagonal, held as mono_diag[n][4][D] (diagonals of Mqq, Mqp, Mpq, Mpp) instead of st->mono, which
 * is NOT touched.  Replaces the same reference code as sc_hk_step (propagators.py:86-119, 313-383, 951-1052) for this
 * special case; opt-in on the host, reported separately from the dense-state kernel. */
int sc_hk_step_diag(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, double *mono_diag,
                    double dt, int32_t mode, double *energy_partials, void *stream);

/* O(n^2) pairwise sum  sum_ij wb_i wk_j exp(rs_i + rs_j + X1_i.Y1_j + i (ib_i + ik_j + X2_i.Y2_j))  behind
 * HermanKlukPropagator.norm() (propagators.py:734-782): X1/Y1 [n][K1], X2/Y2 [n][K2] real, rs/ib/ik [n] real,
 * wb/wk [n] complex; partials[sc_pair_sum_tiles(n)][4] (re, im, 0, 0) for sc_reduce_slot. */
int64_t sc_pair_sum_tiles(int64_t n);
/* ... and over bras i of one set of trajectories (X operands, rs_i, ib, wb: ni rows) and kets j of another (Y operands,
 * rs_j, ik, wk: nj rows): a rank's shard against the gathered ensemble, for norm() across ranks. */
int64_t sc_pair_sum_rect_tiles(int64_t ni, int64_t nj);
int sc_pair_sum_rect(const double *X1, const double *Y1, int32_t K1, const double *X2, const double *Y2, int32_t K2,
                     const double *rs_i, const double *rs_j, const double *ib, const double *ik, const double *wb,
                     const double *wk, int64_t ni, int64_t nj, double *partials, void *stream);
int sc_pair_sum(const double *X1, const double *Y1, int32_t K1, const double *X2, const double *Y2, int32_t K2,
                const double *rs, const double *ib, const double *ik, const double *wb, const double *wk,
                int64_t n, double *partials, void *stream);

/* Reduced density of the frozen-Gaussian wavepacket along M directions u_d on a grid s[ns], behind
 * HermanKlukPropagator.reduced_density() (not in the reference):
 *   rho[d][k] = sqrt(h_d / pi) sum_ij wb_i wk_j exp( E_ij + beta^2 h_d - (s_k - m)^2 h_d + i 2 h_d (s_k - m) beta )   (complex),
 * E_ij the pair exponent of sc_pair_sum_rect from the same operands X1 ... wk, m = a_bra[d][i] + a_ket[d][j],
 * beta = b_ket[d][j] - b_bra[d][i], h_d = inv_two_sigma2[d], s_k = s[k] - s_origin[d] (the caller centres the positions on a
 * point c and passes u_d.c).  With a = u_d.q / 2, b = u_d^T (2 Gamma_t)^+ p / hbar and
 * 1 / h_d = 2 u_d^T (2 Gamma_t)^+ u_d its real part is  int |psi(x)|^2 delta(s_k - u_d.x) dx.
 *   a_bra, b_bra [M][ni], a_ket, b_ket [M][nj] (trajectory index fastest), inv_two_sigma2, s_origin [M], s [ns], rho [M][ns] complex;
 *   partials: scratch of sc_density_pair_sum_rows(ni, nj) * M * ns * 2 doubles (bra bands x shares of the kets), free again when
 *   the call's work on `stream` has run.
 * Two launches; one writer per output, no floating-point atomics, summation order a function of the shapes alone: the same bits
 * in every run.  K1 <= 1024, K2 <= 1536 (D <= 512), ni <= 64 * 65535, M * ceil(ns / 256) < 2^24 -- one call takes the whole grid,
 * the caller does not split it; beyond: SC_ERR_UNSUPPORTED.  A null pointer, M < 1, ns < 1 or K < 1: SC_ERR_BAD_ARGUMENT. */
int64_t sc_density_pair_sum_rows(int64_t ni, int64_t nj);
int sc_density_pair_sum(const double *X1, const double *Y1, int32_t K1, const double *X2, const double *Y2, int32_t K2,
                        const double *rs_i, const double *rs_j, const double *ib, const double *ik, const double *wb,
                        const double *wk, int64_t ni, int64_t nj, const double *a_bra, const double *b_bra,
                        const double *a_ket, const double *b_ket, const double *inv_two_sigma2, int32_t M,
                        const double *s, const double *s_origin, int32_t ns, double *partials, double *rho, void *stream);

/* Expectation values of M quadratic operators in the frozen-Gaussian wavepacket, behind HermanKlukPropagator.expectation() (not in
 * the reference):
 *   out[a] = sum_ij T_ij (kap[a] + sum_col lam[col] z_col^p),  a < M,      out[M] = sum_ij T_ij      (complex),
 * T_ij = wb_i wk_j exp(E_ij) the pair term of sc_pair_sum_rect from the same operands X1 ... wk, z_col = za[col][i] + zb[col][j], the
 * sum over the 1 + R columns col = a (1 + R) + r of operator a: r = 0 to the first power (p = 1), r = 1 ... R squared (p = 2).
 *   za [M (1 + R)][ni], zb [M (1 + R)][nj] complex (trajectory index fastest), lam [M (1 + R)] real, kap [M] complex,
 *   out [M + 1] complex; partials: scratch of sc_pair_expect_tiles(ni, nj) * (M + 1) * 2 doubles, free again when the call's work
 *   on `stream` has run.
 * Two launches; one writer per output, no floating-point atomics, nothing skipped by magnitude, summation order a function of
 * (ni, nj, M, R) alone: the same bits in every run.  The limits of sc_pair_sum_rect, 1 <= M <= 65535, 0 <= R <= 512,
 * M (1 + R) < 2^24; beyond: SC_ERR_UNSUPPORTED.  A null pointer, M < 1, R < 0 or K < 0: SC_ERR_BAD_ARGUMENT.  ni <= 0 or nj <= 0:
 * out = 0. */
int64_t sc_pair_expect_tiles(int64_t ni, int64_t nj);
int sc_pair_expect(const double *X1, const double *Y1, int32_t K1, const double *X2, const double *Y2, int32_t K2,
                   const double *rs_i, const double *rs_j, const double *ib, const double *ik, const double *wb,
                   const double *wk, int64_t ni, int64_t nj, const double *za, const double *zb, const double *lam,
                   const double *kap, int32_t M, int32_t R, double *partials, double *out, void *stream);

/* sc_pair_expect with P product columns per operator next to the 1 + R sum columns, behind
 * HermanKlukPropagator.expectation(ex=...) and anharmonic_energy_expectation() (not in the reference):
 *   out[a] = sum_ij T_ij (kap[a] + sum_col lam[col] z_col^p + sum_{e < P} ea[a P + e][i] eb[a P + e][j]),  a < M,   out[M] = sum_ij T_ij.
 * The matrix element of w exp(-a.x) between two Gaussians of one width, divided by their overlap, is such a product (the weight
 * folded into ea by the caller); operators with fewer terms carry columns of zeros.
 *   ea [M P][ni], eb [M P][nj] complex (trajectory index fastest); everything else, the scratch (sc_pair_expect_tiles) and the
 *   shape of partials as in sc_pair_expect.
 * Two launches, the guarantees of sc_pair_expect; summation order a function of (ni, nj, M, R, P) alone.  The limits of
 * sc_pair_expect, 0 <= P <= 1024, M P < 2^24; beyond: SC_ERR_UNSUPPORTED.  P = 0: ea, eb may be NULL.  P > 0 with a NULL ea or eb,
 * P < 0 and what sc_pair_expect refuses: SC_ERR_BAD_ARGUMENT.  ni <= 0 or nj <= 0: out = 0. */
int sc_pair_expect_exp(const double *X1, const double *Y1, int32_t K1, const double *X2, const double *Y2, int32_t K2,
                       const double *rs_i, const double *rs_j, const double *ib, const double *ik, const double *wb,
                       const double *wk, int64_t ni, int64_t nj, const double *za, const double *zb, const double *lam,
                       const double *kap, int32_t M, int32_t R, const double *ea, const double *eb, int32_t P, double *partials,
                       double *out, void *stream);

/* Cross-correlation of the Herman-Kluk wavepacket with K target coherent states |q_k, p_k, Gamma_0>, behind
 * HermanKlukPropagator.cross_correlation() and run(targets=...) (not in the reference, whose CoherentStatesOverlap,
 * propagators.py:181-240, defines the overlap).  With dq = q_k - q_i, dp = p_k - p_i and A, B, C, fac the
 * overlap constants of (Gamma_t, Gamma_0):
 *   x_ik = conj(fac exp(-1/2 dq^T A dq - 1/2 hbar^-2 dp^T B dp - i/hbar p_k.dq + i/hbar dq^T C dp)) v_i,
 *   v_i  = sgn_i sqrt(c2_i) e^{i S_i/hbar} vi_i / (mc_norm probi_i)              (as sc_hk_correlate forms it, from `st`),
 *   out[k] = sum_i (Re x_ik, Im x_ik, (Re x_ik)^2, (Im x_ik)^2, Re x_ik Im x_ik)   -- five doubles per target, no phase.
 * For (q_k, p_k) = (q0, p0), x_ik is the cq_i of sc_hk_correlate.  The exponent is formed from differences in transformed
 * coordinates, La = A^(1/2), Lb = B^(1/2) / hbar:
 *   diag != 0 (diagonal widths): La, Lb, Ct = the diagonals of La, Lb, C, [D] each; `operands` may be NULL (no pre-pass);
 *   diag == 0: La, Lb [D][D] symmetric, Ct [D][D] = the TRANSPOSE of C; operands: scratch of n * 4 D doubles, which a
 *              pre-pass fills with the rows [La q_i | Lb p_i | q_i | C p_i].
 *   targets [K][5 D]: rows [La q_k | Lb p_k | q_k | C p_k | p_k], formed by the caller once per set of targets.
 *   kept: uint8 [n] or NULL; a trajectory with kept == 0 adds zero to all five sums (its state is not read).
 *   partials: scratch of sc_hk_cross_rows(n, K) * K * 5 doubles; operands and partials are free again when the call's work on
 *             `stream` has run.
 *   out [K][5]; with `cursor` (device resident) the row goes to out + 5 K *cursor, and the cursor is NOT advanced (the
 *             reduction of the correlate launch that shares the cursor advances it: launch this one first).
 * `st` may be a view of an intermediate state (sc_hk_step_multi, sc_hk_step_visit): only n, dim, qp, act, c2, sgn are read.
 * Two launches (three for dense widths); no atomics, the order of every sum is a function of (n, K) alone: the same bits in
 * every call.  D <= 512, 1 <= K <= 65535, n <= 64 * 65535; beyond: SC_ERR_UNSUPPORTED.  A null pointer or K < 1:
 * SC_ERR_BAD_ARGUMENT. */
int64_t sc_hk_cross_rows(int64_t n, int64_t K);
int sc_hk_cross(const sc_state *st, const double *La, const double *Lb, const double *Ct, int32_t diag, double fac,
                const double *targets, int32_t K, const double *vi, const double *probi, double mc_norm,
                const uint8_t *kept, double *operands, double *partials, double *out, const int64_t *cursor, void *stream);

/* Operator correlation functions X_a(t) = <phi_0| A_a e^(-iHt) B_a |phi_0> of the Herman-Kluk wavepacket for M pairs of LINEAR
 * operators A_a = cA_a + mA_a.x, B_a = cB_a + mB_a.x, behind HermanKlukPropagator.operator_correlation() and
 * run(operators=...) (not in the reference, whose ic_correlation, propagators.py:845-911, has the structure: a bra-side and a
 * ket-side factor on every trajectory's C_auto term).  The caller folds the Gaussian matrix elements
 *   <a|x|b> / <a|b> = (Gamma_a + Gamma_b)^+ (Gamma_a q_a + Gamma_b q_b + i (p_b - p_a) / hbar)
 * into one affine form per operator and side (diagonal and dense widths alike, no operand pre-pass):
 *   g_ia = ket_k[a] + ket_u[a].q_i + i ket_w[a].p_i      sc_hk_opcorr_initial, from the INITIAL points zi [n][2 D] = [q_i | p_i]:
 *                                                        once per ensemble and set of operators, into g [n][M] complex;
 *   f_ia = bra_k[a] + bra_u[a].Q_i + i bra_w[a].P_i      from the current (Q_i, P_i) of `st`;
 *   x_ia = f_ia g_ia cq_i                                cq [n] complex: the per-trajectory C_auto terms sc_hk_correlate(_m)
 *                                                        exports for the same state (the Monte-Carlo weight is inside);
 *   out[a] = sum_i (Re x_ia, Im x_ia, (Re x_ia)^2, (Im x_ia)^2, Re x_ia Im x_ia)    -- the row of sc_hk_cross, no phase.
 *   *_u, *_w [M][D] real, *_k [M] complex (re, im).  With S = (Gamma_0 + Gamma_t)^+ the bra side of A = c + m.x is
 *   u = Gamma_t S m, w = S m / hbar, k = c + m.S (Gamma_0 q0 - i p0 / hbar); the ket side has S = (Gamma_i + Gamma_0)^+,
 *   u = Gamma_i S m, w = -S m / hbar, k = c + m.S (Gamma_0 q0 + i p0 / hbar).
 *   kept: uint8 [n] or NULL; a trajectory with kept == 0 adds zero to all five sums: its state, cq and g are not read.
 *   partials: scratch of sc_hk_opcorr_rows(n, M) * M * 5 doubles, free again when the call's work on `stream` has run.
 *   out [M][5]; with `cursor` (device resident) the row goes to out + 5 M *cursor, and the cursor is NOT advanced (the
 *             reduction of the correlate launch that shares the cursor advances it: launch this one first).
 * `st` may be a view of an intermediate state (sc_hk_step_multi, sc_hk_step_visit): only n, dim and qp are read.
 * sc_hk_opcorr: two launches; no atomics, the order of every sum is a function of (n, M) alone: the same bits in every call.
 * D <= 512, 1 <= M <= 65535, n <= 64 * 65535; beyond: SC_ERR_UNSUPPORTED.  A null pointer or M < 1: SC_ERR_BAD_ARGUMENT. */
int64_t sc_hk_opcorr_rows(int64_t n, int64_t M);
int sc_hk_opcorr_initial(const double *zi, int64_t n, int32_t D, const double *ket_u, const double *ket_w, const double *ket_k,
                         int32_t M, double *g, void *stream);
int sc_hk_opcorr(const sc_state *st, const double *cq, const double *bra_u, const double *bra_w, const double *bra_k,
                 const double *g, int32_t M, const uint8_t *kept, double *partials, double *out, const int64_t *cursor,
                 void *stream);

/* The same correlation functions for QUADRATIC operators A_a = c_a + m_a.x + 1/2 x^T K_a x (K_a real symmetric), B_a likewise
 * (DESIGN.md section 4.16).  With every width fixed the matrix element is a quadratic form in the complex mean of the linear case,
 *   <a|A|b> / <a|b> = c + m.x + 1/2 x^T K x + 1/2 tr(K S),   S = (Gamma_a + Gamma_b)^+,
 *   x = S (Gamma_a q_a + Gamma_b q_b + i (p_b - p_a) / hbar),
 * and the caller writes K = sum_r lambda_r v_r v_r^T (R eigenpairs kept): one side of one operator is 1 + R COLUMNS, each an affine
 * form of sc_hk_opcorr.  All operators of a side are padded to the same R with columns of zeros.
 *   z_col = k[col] + u[col].Q_i + i w[col].P_i            col = a (1 + R) + j, j = 0 ... R
 *   f_ia  = l[a][0] z_(a,0) + sum_{j >= 1} l[a][j] z_(a,j)^2       column 0 enters to the first power, the others squared; added in
 *                                                        column order.  From the current (Q_i, P_i) of `st` with bra_*, RA;
 *   g_ia  = the same from the INITIAL points zi [n][2 D] = [q_i | p_i] with ket_*, RB: sc_hk_opquad_initial, once per ensemble
 *           and set of operators, into g [n][M] complex;
 *   x_ia  = f_ia g_ia cq_i,  out[a] = the five sums of sc_hk_opcorr.
 *   *_u, *_w [M][1 + R][D] real, *_k [M][1 + R] complex (re, im), *_l [M][1 + R] real.  Column 0: (u, w, k) of sc_hk_opcorr for
 *   (c, m) with 1/2 tr(K S) added to k, l = 1; column j >= 1: (u, w, k) of sc_hk_opcorr for (0, v_j), l = lambda_j / 2.
 *   RA and RB are independent and either may be 0; with both 0 and l = 1 the rows are those of sc_hk_opcorr.
 *   kept, partials (sc_hk_opquad_rows(n, M) * M * 5 doubles), out, cursor, `st`: as for sc_hk_opcorr.
 * sc_hk_opquad: two launches; no atomics, the order of every sum is a function of (n, M, R) alone: the same bits in every call.
 * D <= 512, 1 <= M <= 65535, n <= 64 * 65535, 0 <= R <= 512, M (1 + R) < 2^24; beyond: SC_ERR_UNSUPPORTED.  A null pointer, M < 1
 * or R < 0: SC_ERR_BAD_ARGUMENT. */
int64_t sc_hk_opquad_rows(int64_t n, int64_t M);
int sc_hk_opquad_initial(const double *zi, int64_t n, int32_t D, const double *ket_u, const double *ket_w, const double *ket_k,
                         const double *ket_l, int32_t M, int32_t RB, double *g, void *stream);
int sc_hk_opquad(const sc_state *st, const double *cq, const double *bra_u, const double *bra_w, const double *bra_k,
                 const double *bra_l, const double *g, int32_t M, int32_t RA, const uint8_t *kept, double *partials, double *out,
                 const int64_t *cursor, void *stream);

/* Time-averaged Herman-Kluk spectra I_k(E) (Kaledin and Miller, separable prefactor) behind
 * HermanKlukPropagator.time_average() and run(time_average=...) (not in the reference).  With O_ik the
 * overlap of sc_hk_cross (bra: trajectory i, width Gamma_t; ket: reference state k, width Gamma_0; La, Lb, Ct, diag, fac,
 * operands and the rows refs [K][5 D] exactly as sc_hk_cross takes its targets):
 *   g_ik(t_s) = conj(O_ik) u_i,   u_i = c_i / |c_i| e^{i S_i/hbar},   c_i = sgn_i sqrt(c2_i)   (u_i = 0 where c_i = 0),
 *   A_ik(E_e) = dt sum_s g_ik(t_s) exp(i E_e t_s / hbar),   t_s = t_a + s dt (a product, s an integer),
 *   y_ik(e)   = |A_ik(E_e)|^2 / (2 pi hbar mc_norm probi_i),   out[k][e] = (sum_i y_ik(e), sum_i y_ik(e)^2);
 * the spectrum over a window of ns steps, T = ns dt, is I_k(E_e) = out[k][e][0] / T, its second sum out[k][e][1] / T^2.
 * All buffers are the caller's: G [TB][n K] complex (row index i K + k), W [TB][NE] complex, A [n K][NE] complex (zeroed by the
 * caller before the first column), TB = sc_hk_ta_block().
 *   sc_hk_ta_terms       column `column` (0 ... TB - 1) of G from the state `st`, which may be a view of an intermediate state
 *                        (sc_hk_step_multi, sc_hk_step_visit): only n, dim, qp, act, c2, sgn are read.  kept: uint8 [n] or NULL; a
 *                        trajectory with kept == 0 gets exact zeros and its state is not read.  One launch (two for dense widths).
 *   sc_hk_ta_accumulate  A += sum_{c < count} G[c] (x) W[c],  W[c][e] = dt exp(i E_e (t_a + (s0 + c) dt) / hbar): column c of G holds
 *                        step s0 + c of the window.  Every W is one sincos of the product E_e t_s -- no recurrence; the columns
 *                        are added to the stored A in ascending c, so the bits of A do not depend on where the blocks of columns
 *                        were cut.  Two launches; G and W are free again when they have run.
 *   sc_hk_ta_finish      out [K][NE][2] from A; partials: scratch of sc_hk_ta_finish_rows(n) * K * NE * 2 doubles.  A trajectory
 *                        with kept == 0 counts as y = 0 (its rows of A are not read).  Two launches; no atomics, the order of
 *                        every sum is a function of (n, K, NE) alone: the same bits in every call.  A is not changed.
 * D <= 512, 1 <= K <= 64, 1 <= NE <= 65535, n <= 64 * 65535; beyond: SC_ERR_UNSUPPORTED.  A null pointer, K < 1, NE < 1, a column
 * outside 0 ... TB - 1 or a count outside 1 ... TB: SC_ERR_BAD_ARGUMENT. */
int32_t sc_hk_ta_block(void);
int sc_hk_ta_terms(const sc_state *st, const double *La, const double *Lb, const double *Ct, int32_t diag, double fac,
                   const double *refs, int32_t K, const uint8_t *kept, double *operands, double *G, int32_t column, void *stream);
int sc_hk_ta_accumulate(const double *G, int64_t n, int32_t K, int32_t count, const double *energies, int32_t NE, double t_a,
                        double dt, int64_t s0, double *W, double *A, void *stream);
int64_t sc_hk_ta_finish_rows(int64_t n);
int sc_hk_ta_finish(const double *A, int64_t n, int32_t K, int32_t NE, const double *probi, double mc_norm, const uint8_t *kept,
                    double *partials, double *out, void *stream);

/* Frozen-Gaussian wavefunction on a spatial grid behind HermanKlukPropagator.wavefunction() (propagators.py:252-292,
 * 688-732):  phi[k] = fac sum_n v_n exp(-1/2 |Lx_k - Lq_n|^2 + i (p_n.x_k - pq_n)),  L = Gamma_t^(1/2).
 * LqT, PT [D][n] (trajectory index fastest), pq [n], v [n] complex, Lx, X [nx][D], phi [nx] complex. */
int sc_grid_sum(const double *LqT, const double *PT, const double *pq, const double *v, int64_t n, int32_t D,
                const double *Lx, const double *X, int32_t nx, double fac, double *phi, void *stream);

/* Walton-Manolopoulos wavefunction on a spatial grid (propagators.py:1434-1482):
 *   phi[k] = sum_n v_n exp(-1/2 dx^T CQQ_n dx + dvec_n . dx),  dx = x_k - Q_n
 * with the per-trajectory export of sc_wm_correlate; qp [n][2D] (engine state), X [nx][D], phi [nx] complex. */
int sc_wm_grid_sum(const double *qp, const double *coef, const double *cqq, const double *dvec, int64_t n, int32_t D,
                   const double *X, int32_t nx, double *phi, void *stream);

/* O(n^2) pair sum behind WaltonManolopoulosPropagator.norm() (propagators.py:1484-1575), from the per-trajectory
 * export of sc_wm_correlate and its projections cqqp [n][d'][d'] = U^T CQQ U, dvecp [n][d'] = U^T dvec (complex),
 * U [D][d'] real.  partials [sc_wm_pair_sum_tiles(n)][4] for sc_reduce_slot.  D <= 512, d' <= 96: D <= 64 with d' <= 16
 * takes one thread per pair, every other shape one wavefront per pair (bordered matrix in LDS, partial pivoting,
 * det(D'/2pi) as mantissa x 2^e); larger shapes return SC_ERR_UNSUPPORTED. */
int64_t sc_wm_pair_sum_tiles(int64_t n);
/* The same pair sum over bras i of one set of trajectories and kets j of another (a rank's shard against the gathered
 * ensemble: norm() across ranks); partials [sc_wm_pair_sum_rect_tiles(ni, nj)][4]. */
int64_t sc_wm_pair_sum_rect_tiles(int64_t ni, int64_t nj);
int sc_wm_pair_sum_rect(const double *qp_i, const double *coef_i, const double *cqqp_i, const double *dvecp_i, int64_t ni,
                        const double *qp_j, const double *coef_j, const double *cqq_j, const double *dvec_j,
                        const double *cqqp_j, const double *dvecp_j, int64_t nj, const double *U, int32_t D,
                        int32_t dprime, double *partials, void *stream);
int sc_wm_pair_sum(const double *qp, const double *coef, const double *cqq, const double *dvec, const double *cqqp,
                   const double *dvecp, const double *U, int64_t n, int32_t D, int32_t dprime, double *partials,
                   void *stream);

/* Expectation values of M operators in the Walton-Manolopoulos wavepacket, behind WaltonManolopoulosPropagator.wm_expectation()
 * (not in the reference), on the operands of sc_wm_pair_sum_rect:
 *   out[a] = sum_ij T_ij F_a,ij  (a < M),   out[M] = sum_ij T_ij,   T_ij = conj(v_i) O_ij v_j the pair term of sc_wm_pair_sum_rect,
 *   F_a,ij = kap_a + sum_col lam_col f_col over the 1 + R columns col = a (1 + R) ... of operator a,
 *   f_col  = l_col for column 0 of an operator,  l_col^2 + s_col^T D'^-1 s_col for its columns 1 ... R,
 *   l_col  = za[col][i] + zb[col][j] + g_col . b' + s_col^T D'^-1 b',
 *   s_col  = sfix[col], plus sket[a][j] for column 0 of operator a when sket is not NULL,
 * with D' = conj(C'_i) + C'_j, b' = U^T C_j dQ + conj(d'_i) + d'_j of the norm (Q_i + U D'^-1 b' is the mean of x under the product
 * of the two Gaussians, U D'^-1 U^T its covariance).  za [C][ni], zb [C][nj] complex (trajectory index fastest), g, sfix [C][d']
 * complex, sket NULL or [M][nj][d'] complex, lam [C] real, kap [M] complex, C = M (1 + R); out [M + 1] complex; partials: scratch of
 * sc_wm_pair_expect_tiles(ni, nj) * (M + 1) * 2 doubles.
 * One wavefront per pair for every shape: D' is eliminated once with partial pivoting, b' and the border vectors carried as extra
 * columns and rows, det(D'/2pi) as mantissa x 2^e.  Two launches (tiles, then their sum); no atomics, nothing skipped by magnitude,
 * summation order a function of (ni, nj, D, d', M, R) alone: the same bits in every call.
 * The border columns of a launch share the LDS region of a pair with D': sc_wm_pair_expect_capacity(D, d') is the largest C of one
 * call (4 at d' = 96; 0 for a shape outside the limits); the caller splits larger operator sets into several calls (columns of one
 * operator may go to different calls: F is their sum).
 * Limits: those of sc_wm_pair_sum_rect (D <= 512, d' <= 96, fewer than 2^31 tiles), 1 <= M <= 65535, M (1 + R) <= the capacity;
 * beyond: SC_ERR_UNSUPPORTED, with the capacity in the text.  A NULL pointer other than sket, M < 1, R < 0: SC_ERR_BAD_ARGUMENT.
 * ni <= 0 or nj <= 0: out = 0. */
int64_t sc_wm_pair_expect_tiles(int64_t ni, int64_t nj);
int32_t sc_wm_pair_expect_capacity(int32_t D, int32_t dprime);
int sc_wm_pair_expect(const double *qp_i, const double *coef_i, const double *cqqp_i, const double *dvecp_i, int64_t ni,
                      const double *qp_j, const double *coef_j, const double *cqq_j, const double *dvec_j, const double *cqqp_j,
                      const double *dvecp_j, int64_t nj, const double *U, int32_t D, int32_t dprime, const double *za,
                      const double *zb, const double *g, const double *sfix, const double *sket, const double *lam,
                      const double *kap, int32_t M, int32_t R, double *partials, double *out, void *stream);

/* sc_wm_pair_expect with a kind and a slot of per-ket border vectors per column, behind wm_operator_expectation() and
 * wm_energy_expectation() of the WaltonManolopoulosPropagator (not in the reference).  Operator a owns the
 * columns col = a cols ... a cols + cols - 1, and  F_a,ij = kap_a + sum_col lam_col f_col  with l_col as above and
 *   kind[col] = 0:  f = l,      1:  f = l^2 + s^T D'^-1 s,      2:  f = exp(-l + 1/2 s^T D'^-1 s),
 *   s_col = sfix[col]  if ketcol[col] = -1,   sfix[col] + sket[p][j]  if ketcol[col] = p  (0 <= p < S).
 * A quadratic momentum operator 1/2 p^T W p acting on the ket is a kind-1 column with a per-ket vector per eigenpair of W, the
 * operator exp(-a.x) a kind-2 column with s = U^T a.  kind, ketcol [C] int32 on the device, C = M cols; sket [S][nj][d'] complex, NULL
 * when S = 0; the other operands, partials and out as sc_wm_pair_expect.  A column that pads an operator has kind 0 and lam = 0
 * (never kind 2: 0 x inf).  The entry reads kind and ketcol back to the host once and checks them (it synchronises the stream).
 * Same kernel body, capacity (sc_wm_pair_expect_capacity), tiles, order of the sums and limits as sc_wm_pair_expect: M cols <= the
 * capacity, beyond: SC_ERR_UNSUPPORTED with the capacity in the text.  A NULL pointer other than sket with S = 0, M < 1, cols < 1,
 * S < 0, a kind outside 0 ... 2 and a ketcol outside -1 ... S - 1: SC_ERR_BAD_ARGUMENT. */
int sc_wm_pair_expect_cols(const double *qp_i, const double *coef_i, const double *cqqp_i, const double *dvecp_i, int64_t ni,
                           const double *qp_j, const double *coef_j, const double *cqq_j, const double *dvec_j, const double *cqqp_j,
                           const double *dvecp_j, int64_t nj, const double *U, int32_t D, int32_t dprime, const double *za,
                           const double *zb, const double *g, const double *sfix, const double *sket, int32_t S,
                           const int32_t *ketcol, const int32_t *kind, const double *lam, const double *kap, int32_t M, int32_t cols,
                           double *partials, double *out, void *stream);

/* Energy-conservation guard on the device, reference propagators.py:385-398 (check_energy_conservation).
 * elog[4] = { <T+V>(t-dt), <T+V>(t), largest |change| seen so far, number of steps logged }.
 * The mean of this step is formed from energy_partials; the host raises the reference's RuntimeError when
 * elog[2] > 1e-2 Hartree the next time it synchronises. */
int sc_energy_guard(const double *energy_partials, int32_t n_blocks, double n_traj, double *elog, void *stream);

/* Per-trajectory symplecticity of the monodromy matrix M = [[Mqq, Mqp], [Mpq, Mpp]]: an exact flow has M^T J M = J, the fixed RK4
 * step only nearly (the reference has no such check).  With A = Mqq, B = Mqp, C = Mpq, D = Mpp (Cartesian
 * blocks) the three independent blocks of M^T J M - J are
 *     E1 = A^T C - C^T A,    E2 = A^T D - C^T B - 1,    E3 = B^T D - D^T B,
 * taken in the scaled canonical coordinates q~_a = scale_a q_a, p~_a = p_a / scale_a (scale: [D] positive, NULL = ones):
 *     E1~_ab = E1_ab / (scale_a scale_b),   E2~_ab = E2_ab scale_b / scale_a,   E3~_ab = E3_ab scale_a scale_b.
 *   dev [n][3] = max_ab |E1~|, max_ab |E2~|, max_ab |E3~| per trajectory; the trajectory's deviation is the largest of the three.
 *                A trajectory with a non-finite element in any of its four blocks reports +inf in all three.
 * Reads st->mono in the storage order st->mono_layout says (SC_MONO_ROWMAJOR: 1 <= D <= 510; SC_MONO_TILED16: D <= 64) and
 * never converts or writes it.  No atomics, fixed order of operations: the same bits in every run.  D <= 16 runs on the vector
 * ALUs (one trajectory per 16 lanes), larger D on the FP64 matrix cores (one workgroup per trajectory at a time). */
int sc_symplectic_deviation(const sc_state *st, const double *scale, double *dev, void *stream);

/* ---- Discarding trajectories that fail the symplecticity check -----------------------------------
 * A per-trajectory mask kept[n] (one byte each, 1 = kept, all ones at t = 0) is STICKY: the entry points below only ever clear it.
 * A discarded trajectory is a sample of value ZERO and N does not change: from its mark on, C_auto, k_ic, their second moments and
 * their block sums are the sums of the exported per-trajectory terms (cq_out / kq_out of sc_hk_correlate(_m), the term arrays of
 * sc_wm_correlate) over the kept trajectories with the unchanged weights 1/(N prob_i) -- so the standard errors and the batch-means
 * errors with their unchanged N and n_b are the errors of this estimator.  The state kernels and the correlate kernels do not know
 * the mask: a discarded trajectory is still propagated.  These entry points ADD NOTHING to the state.
 *   sc_discard_mark      clears kept[i] and sets discarded_at[i] = step for every trajectory whose bit is set and whose deviation
 *                        dev[i][0..2] (what sc_symplectic_deviation wrote) is NOT <= tol in all three blocks: +inf and NaN clear
 *                        it.  Bits that are clear stay clear, their discarded_at stays what it is (the caller starts it at -1).
 *                        *kept_count (device; zeroed on the stream first) receives the number of bits set after the mark (integer
 *                        atomic adds: the value does not depend on their order).  tol NaN or <= 0, or a null pointer:
 *                        SC_ERR_BAD_ARGUMENT.
 *   sc_term_masked_sums  ONE pass over cq[n], kq[n] (complex; kq may be NULL: its sums are 0) and kept[n] that leaves, summed over
 *                        the trajectories with kept[i] != 0,
 *                            slot[0..3]    = Re sum cq_i, Im sum cq_i, Re sum kq_i, Im sum kq_i
 *                            moments[0..5] = the six second-moment sums of sc_hk_correlate_m (NULL: not wanted)
 *                            blocks[b][0..3], b < B = the slot sums over block b = (i >> 2) & (B - 1) (B = 0 and NULL: not wanted;
 *                                            B as for sc_term_blocks, anything else SC_ERR_BAD_ARGUMENT)
 *                        moments and blocks are independent options; sum_b blocks[b] is the slot row up to rounding.  A term of a
 *                        discarded trajectory is selected away before any arithmetic (never multiplied by the mask): it may be
 *                        inf or NaN.  One writer per output, no floating-point atomics, summation order a function of (n, B)
 *                        alone: the same bits in every run.  `scratch`: sc_term_masked_scratch_doubles() doubles, free again when
 *                        the call's work on `stream` has run.  cq / kq 16-byte aligned, kept 4-byte aligned.  Two launches:
 *                        64 workgroups (workgroup w takes the groups of four trajectories g = w mod 64, all in block w mod B),
 *                        then one workgroup that adds the 64 partial rows in order. */
int sc_discard_mark(const double *dev, int64_t n, double tol, int32_t step, uint8_t *kept, int32_t *discarded_at,
                    int64_t *kept_count, void *stream);
int64_t sc_term_masked_scratch_doubles(void);
int sc_term_masked_sums(const double *cq, const double *kq, const uint8_t *kept, int64_t n, int32_t B, double *scratch,
                        double *slot, double *moments, double *blocks, void *stream);

/* ---- multi-GPU flush -------------------------------------------------------------------------
 * Trajectories shard over the GPUs of a node, one process per GPU; every term of C_auto / k_ic already carries the weight
 * 1/(N_total P(q_i, p_i)) (propagators.py:837, 909), so the functions of the whole ensemble are the plain SUM of the
 * per-rank slot buffers -- the running mean of cli.py:453-458 over one repetition, taken across ranks.
 * sc_flush_allreduce is that sum: ONE ncclAllReduce(ncclDouble, ncclSum), in place, on `stream` (RCCL over xGMI), of
 * `count` doubles -- the caller passes the packed 4 nt sums, or the whole [nt][5] slot buffer of sc_reduce_slot_at /
 * sc_hk_run (column 4, the per-rank mean <T+V>, then holds the sum of the ranks' means).  Nothing else on the hot path
 * is a collective.
 *
 * librccl is loaded at the first sc_comm_* call (dlopen of librccl.so.1 from the loader's search path): no link-time
 * dependency, single-GPU users never load it.
 *   sc_comm_available   RCCL's version code (ncclGetVersion) if the library can be loaded, 0 otherwise
 *   sc_comm_unique_id   ncclGetUniqueId -> id_out[SC_COMM_ID_BYTES]; ONE rank calls it and hands the bytes to the others by
 *                       whatever host channel the application has (file, socket, MPI, torch's TCPStore)
 *   sc_comm_init        ncclCommInitRank on the CURRENT HIP device; collective over the nranks processes
 *   sc_comm_rank_count  rank and size of a communicator (either output may be NULL)
 *   sc_comm_destroy     ncclCommDestroy (NULL is accepted)
 * Returns SC_ERR_UNSUPPORTED when librccl cannot be loaded, SC_ERR_LAUNCH with RCCL's message on an RCCL error. */
#define SC_COMM_ID_BYTES 128
int sc_comm_available(void);
int sc_comm_unique_id(void *id_out);
int sc_comm_init(const void *id, int32_t nranks, int32_t rank, void **comm_out);
int sc_comm_rank_count(void *comm, int32_t *rank_out, int32_t *nranks_out);
int sc_comm_destroy(void *comm);
int sc_flush_allreduce(double *sums, int64_t count, void *comm, void *stream);

/* ---- Quartic force field (an addition: the ABI number stays) ---------------------------------------------------------------
 * A coupled anharmonic Taylor expansion around pos0, behind potentials.QuarticForceFieldPotential (not in the reference, whose
 * potential protocol, potentials.py:41-204, it implements).  With x = r - pos0, y_i = x_i^2, z_i = x_i^3:
 *   W_ij   = sum_k t_ijk x_k
 *   V      = energy0 + g.x + 1/2 x^T H x + 1/6 x^T W x + y^T A y + z^T B x
 *   dV_m   = g_m + (Hx)_m + 1/2 (Wx)_m + 4 x_m (Ay)_m + 3 x_m^2 (Bx)_m + (B^T z)_m
 *   d2V_mn = H_mn + W_mn + 8 A_mn x_m x_n + 3 B_mn x_m^2 + 3 B_nm x_n^2 + delta_mn [4 (Ay)_m + 6 x_m (Bx)_m]
 * cubic holds the DERIVATIVES t_ijk; quartic_a / quartic_b hold the semi-diagonal quartic derivatives FOLDED by the caller:
 * A_ij = u_iijj / 8 (i != j), A_ii = u_iiii / 24, B_ij = u_iiij / 6 (zero diagonal).  hess0, cubic and quartic_a have to be
 * symmetric bit for bit (the kernel relies on it for an exactly symmetric Hessian image).  A NULL cubic skips the D^2 x D x n
 * product, NULL quartic_a and quartic_b skip the quartic terms; either of the two alone counts as zeros. */
typedef struct sc_qff_model {
    int32_t dim, _pad;
    const double *pos0, *grad0, *hess0;      /* [D], [D], [D][D] */
    const double *cubic;                     /* [D][D][D] derivatives, fully symmetric; NULL = none */
    const double *quartic_a, *quartic_b;     /* folded A, B [D][D]; NULL = none */
    double energy0;                          /* energy0 - origin */
    const double *inv_mass;                  /* [D] */
} sc_qff_model;

/*   sc_qff_max_dim        96: the largest D (the limit of sc_dense_mono_step's matrix-core route)
 *   sc_qff_tile           trajectories per workgroup (the tile edges of the n axis; results do not depend on it)
 *   sc_qff_scratch_bytes  bytes of the `scratch` of sc_qff_stage: stage positions, V and grad of n trajectories; -1 for an
 *                         invalid shape
 *   sc_qff_eval           r [n][D] -> energy [n], grad [n][D], hess [n][D][D] (the contract of sc_gdml_eval)
 *   sc_qff_stage          one RK4 stage of (q, p, S) (the contract of sc_gdml_stage_scratch): stage point, evaluation with the
 *                         stage Hessian written straight into sc->hess[i][stage], slopes; energy_partials[sc_dense_grid()]
 * W = T.X runs on v_mfma_f64_16x16x4_f64.  Every sum runs in an order fixed by D: a trajectory's results do not depend on n,
 * on its index or on the launch shape; no atomics; hess[i][j] == hess[j][i] bit for bit.
 * A null pointer or a stage outside 0..3: SC_ERR_BAD_ARGUMENT.  D < 1, D > sc_qff_max_dim() or n > 64 * 65535:
 * SC_ERR_UNSUPPORTED.  n = 0: SC_OK, nothing is launched. */
int     sc_qff_max_dim(void);
int     sc_qff_tile(void);
int64_t sc_qff_scratch_bytes(int64_t n, int32_t dim);
int sc_qff_eval(const sc_qff_model *m, const double *r, int64_t n, double *energy, double *grad, double *hess, void *stream);
int sc_qff_stage(const sc_qff_model *m, double *scratch, const sc_state *st, const sc_dense_scratch *sc, double dt,
                 int32_t stage, double *energy_partials, void *stream);

/* ---- Thermal ensembles (an addition: the ABI number stays; no existing struct changes) ---------------------------------------
 * C_auto(t) and k_ic(t) of the canonical density operator of a HARMONIC initial surface, behind
 * HermanKlukPropagator.thermal_initial_conditions() (not in the reference).  The density operator is a
 * positive mixture of coherent states of the width Gamma_0 (Glauber-Sudarshan P function): trajectory i carries its own centre,
 * drawn from P, and the Herman-Kluk expression of sc_hk_correlate is evaluated with that centre in the place of (q0, p0).
 * With W = m^-1/2 Gamma_0 m^-1/2 hbar = L diag(omega) L^T and the d'' modes of omega_k > 0 a centre is (Q_i, P_i) in
 * mass-weighted normal coordinates; its Cartesian image is a_i = q0 + map_q Q_i, b_i = map_p P_i.  The bra centre at the time t
 * of the state rotates on the initial surface,
 *     Q_ik(t) = Q_ik cos w_k t + P_ik / w_k sin w_k t,     P_ik(t) = P_ik cos w_k t - w_k Q_ik sin w_k t,
 * and each trajectory carries the phase Phi_i(t) = exp(i / (2 hbar) sum_k [Q_ik P_ik - Q_ik(t) P_ik(t)]).
 *   dmodes   d'' (1 ... D)
 *   diag     != 0: d'' == D and mode k IS coordinate k (diagonal Gamma_0): map_q, map_p hold the D scale factors m_k^-1/2,
 *            m_k^1/2 and no matrix-vector product is formed; 0: map_q = m^-1/2 L, map_p = m^1/2 L, [D][d''] row-major
 *   centres  [n][2 d''] = (Q_i | P_i) at t = 0; never written by the correlate kernel
 *   n1       [D] = -hbar^2 tau1 / m (the vector behind sc_nac_consts.p0n1), NULL without coupling */
typedef struct sc_thermal_consts {
    int32_t dim, dmodes, diag, _pad;
    const double *omega;            /* [d''] */
    const double *map_q, *map_p;
    const double *q0;               /* [D] minimum of the initial surface */
    const double *n1;
    const double *centres;
} sc_thermal_consts;

/*   sc_hk_thermal_initial    once per ensemble (and per coupling): vi_out[i] = <q_i, p_i, Gamma_i | a_i, b_i, Gamma_0> from the
 *                            INITIAL points zi [n][2 D] and ovl_i0 (its qk, pk are not read), and
 *                            nacq_out[i] = n2 + (a_i - q_i).rn + i/hbar [b_i.n1 + (p_i - b_i).gn]  (nc: rn, gn, n2 are read).
 *                            Either output may be NULL; nacq_out needs nc and th->n1.
 *   sc_hk_correlate_thermal  sc_hk_correlate for the state `st` AT THE TIME `time` (the caller's clock of that state: the mid
 *                            states of sc_hk_step_multi / sc_hk_step_visit work through their views; only n, dim, qp, act, c2,
 *                            sgn are read):
 *                                cq_i = Phi_i(t) conj(<q_i(t), p_i(t), Gamma_t | a_i(t), b_i(t), Gamma_0>) vi_i sgn_i sqrt(c2_i)
 *                                       e^{i S_i/hbar} / (mc_norm probi_i)
 *                                kq_i = nacQ_i nacq_i cq_i / hbar^2,
 *                                nacQ_i = n2 + (a_i(t) - q_i(t)).rn - i/hbar [b_i(t).n1 + (p_i(t) - b_i(t)).gn]
 *                            cq_out and kq_out [n] complex are ALWAYS written (kq_out only with nc); partials
 *                            [sc_correlate_grid()][4] as sc_hk_correlate writes them, so sc_reduce_slot*, sc_term_moments,
 *                            sc_term_blocks* and sc_term_masked_sums follow unchanged.  cos / sin of omega_k t are formed once
 *                            per workgroup.  With all centres zero the terms are those of sc_hk_correlate up to rounding.
 *   sc_sample_thermal        sc_sample_initial with per-trajectory centres drawn ON THE DEVICE: Q_ik = sigma_q[k] g, P_ik =
 *                            sigma_p[k] g', (g, g') the Box-Muller pair with pair index d' + k of the trajectory's Philox stream
 *                            (the pairs 0 ... d' - 1 are the xi of sc_sample_initial, bit for bit: with the same seed
 *                            zi - (a_i, b_i) is the zero-temperature draw minus z0 up to rounding); centres_out [n][2 d''],
 *                            zi_t = (a_i, b_i) + iLz^T xi, probi and the state as sc_sample_initial writes them.
 *                            d' + d'' <= 256 (the pair index has eight bits), else SC_ERR_UNSUPPORTED.
 * D <= 512, n <= 64 * 65535; beyond: SC_ERR_UNSUPPORTED.  A null pointer: SC_ERR_BAD_ARGUMENT.  One launch each; no atomics,
 * the order of every sum is a function of the shapes alone: the same bits in every call. */
int sc_hk_thermal_initial(const sc_thermal_consts *th, const sc_overlap_consts *ovl_i0, const sc_nac_consts *nc,
                          const double *zi, int64_t n, double *vi_out, double *nacq_out, void *stream);
int sc_hk_correlate_thermal(const sc_state *st, double time, const sc_overlap_consts *ovl_t0, const sc_nac_consts *nc,
                            const sc_thermal_consts *th, const double *vi, const double *probi, const double *nacq,
                            double mc_norm, double *cq_out, double *kq_out, double *partials, void *stream);
int sc_sample_thermal(const sc_state *st, const double *ilz, const sc_thermal_consts *th, const double *sigma_q,
                      const double *sigma_p, int32_t dprime, double prob0, uint64_t seed, uint64_t subsequence, int64_t first,
                      int32_t init_state, double *centres_out, double *zi_t, double *probi, double *xi_out, void *stream);

/* Thermal operator correlation functions X_a(t) = Tr[rho e^(iH_es t) A_a e^(-iH_gs t) B_a] for M pairs of LINEAR operators
 * A_a = cA_a + mA_a.x, B_a = cB_a + mB_a.x on a thermal ensemble, behind HermanKlukPropagator.thermal_operator_correlation() and
 * run(thermal_operators=...) (not in the reference): sc_hk_opcorr with the trajectory's own centre in the
 * place of (q0, p0), the bra centre rotated to the time of the state.  The caller folds the Cartesian maps of the centres into
 * the operators, so both kernels take dot products with the mode coordinates (Qc_i | Pc_i) = th->centres [n][2 d''] only:
 *   g_ia = ket_k[a] + ket_u[a].q_i + i ket_w[a].p_i + ket_ut[a].Qc_i + i ket_wt[a].Pc_i
 *                                                        sc_hk_opcorr_thermal_initial, from the INITIAL points zi [n][2 D] and the
 *                                                        centres of t = 0: once per ensemble and set of operators, into g [n][M];
 *   f_ia = bra_k[a] + bra_u[a].Q_i + i bra_w[a].P_i + bra_ut[a].Qc_i(t) + i bra_wt[a].Pc_i(t)
 *                                                        from the current (Q_i, P_i) of `st` and the centres rotated to `time`,
 *                                                        Qc(t) = Qc cos wt + Pc / w sin wt, Pc(t) = Pc cos wt - w Qc sin wt;
 *   x_ia = f_ia g_ia cq_i                                cq [n] complex: the terms sc_hk_correlate_thermal exports for the same
 *                                                        state and time (phase, overlaps, prefactor and weight inside);
 *   out[a] = sum_i (Re x_ia, Im x_ia, (Re x_ia)^2, (Im x_ia)^2, Re x_ia Im x_ia)    -- the row of sc_hk_opcorr, no phase.
 *   *_u, *_w [M][D] and *_k [M] complex: those of sc_hk_opcorr with p0 = 0.  *_ut, *_wt [M][d''] real: with S as there,
 *   ut = map_q^T Gamma_0 S m on both sides, wt = -map_p^T S m / hbar (bra), +map_p^T S m / hbar (ket).
 *   Of `th` only dim, dmodes, omega and centres are read: map_q, map_p, q0 and n1 may be NULL.
 *   kept, partials (sc_hk_opcorr_thermal_rows(n, M) * M * 5 doubles), out, cursor, `st`: as for sc_hk_opcorr.
 * sc_hk_opcorr_thermal: two launches; no atomics, the order of every sum is a function of (n, M, D, d'') alone: the same bits in
 * every call.  D <= 512, 1 <= d'' <= D, 1 <= M <= 65535, n <= 64 * 65535; beyond: SC_ERR_UNSUPPORTED.  A null pointer, M < 1 or
 * th->dim != st->dim: SC_ERR_BAD_ARGUMENT. */
int64_t sc_hk_opcorr_thermal_rows(int64_t n, int64_t M);
int sc_hk_opcorr_thermal_initial(const double *zi, const double *centres, int64_t n, int32_t D, int32_t dmodes,
                                 const double *ket_u, const double *ket_w, const double *ket_ut, const double *ket_wt,
                                 const double *ket_k, int32_t M, double *g, void *stream);
int sc_hk_opcorr_thermal(const sc_state *st, double time, const sc_thermal_consts *th, const double *cq, const double *bra_u,
                         const double *bra_w, const double *bra_ut, const double *bra_wt, const double *bra_k, const double *g,
                         int32_t M, const uint8_t *kept, double *partials, double *out, const int64_t *cursor, void *stream);

/* The same with QUADRATIC operators A_a = c_a + m_a.x + 1/2 x^T K_a x on both sides, behind
 * HermanKlukPropagator.thermal_quadratic_correlation() and run(thermal_quadratic=...) (not in the reference; DESIGN.md section
 * 4.22): the columns of sc_hk_opquad with the trajectory's own centre of sc_hk_opcorr_thermal.  One side of an operator is 1 + R
 * columns,
 *   z_col = k[col] + u[col].Q_i + i w[col].P_i + ut[col].Qc_i(t) + i wt[col].Pc_i(t),   f_ia = sum_col l[col] z_col^p
 *   (p = 1 for column 0 of an operator, else 2), the ket from the initial points and the centres of t = 0 into g [n][M]
 *   (sc_hk_opquad_thermal_initial, RB), the bra from `st` and the centres rotated to `time` (RA);  x_ia = f_ia g_ia cq_i and the
 *   row of five sums as above.
 *   *_u, *_w [M (1 + R)][D], *_k [M (1 + R)] complex, *_l [M (1 + R)]: those of sc_hk_opquad with p0 = 0; *_ut, *_wt
 *   [M (1 + R)][d'']: those of sc_hk_opcorr_thermal of every column's vector (zeros in padding columns).
 *   th, cq, kept, partials (sc_hk_opquad_thermal_rows(n, M) * M * 5 doubles), out, cursor, `st`: as for sc_hk_opcorr_thermal.
 * sc_hk_opquad_thermal: two launches; no atomics, the order of every sum is a function of (n, M, R, D, d'') alone: the same bits in
 * every call.  The limits and codes of sc_hk_opquad (R <= 512, M (1 + R) < 2^24) and of sc_hk_opcorr_thermal (1 <= d'' <= D <= 512). */
int64_t sc_hk_opquad_thermal_rows(int64_t n, int64_t M);
int sc_hk_opquad_thermal_initial(const double *zi, const double *centres, int64_t n, int32_t D, int32_t dmodes,
                                 const double *ket_u, const double *ket_w, const double *ket_ut, const double *ket_wt,
                                 const double *ket_k, const double *ket_l, int32_t M, int32_t RB, double *g, void *stream);
int sc_hk_opquad_thermal(const sc_state *st, double time, const sc_thermal_consts *th, const double *cq, const double *bra_u,
                         const double *bra_w, const double *bra_ut, const double *bra_wt, const double *bra_k, const double *bra_l,
                         const double *g, int32_t M, int32_t RA, const uint8_t *kept, double *partials, double *out,
                         const int64_t *cursor, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SEMICLASSICAL_HIP_H */

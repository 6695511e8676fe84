// Fused Herman-Kluk step for a CONSTANT dense Hessian (MolecularHarmonicPotential, reference potentials.py:553-593) and
// small matrices (D <= 16): register-resident, one trajectory per 16-lane DPP row.
//
// With a constant Hessian the equations of motion of the monodromy blocks (reference propagators.py:342-357) are linear
// with constant coefficients,  d/dt [X; Y] = G [X; Y],  X = [Mqq|Mqp], Y = [Mpq|Mpp],  G = [[0, 1/m], [-H, 0]],  and one
// step of the reference's classical RK4 (propagators.py:86-119) IS the multiplication by the fixed 2D x 2D matrix
//     Phi = 1 + h G + (h G)^2 / 2 + (h G)^3 / 6 + (h G)^4 / 24
// (the four stages of RK4 applied to a linear autonomous system; differences to the staged evaluation are re-association
// only, ~1e-16).  The host builds Phi once per (potential, dt) (sc_potential.lin_prop); the kernel then does ONE product
// per step instead of four dependent stages.  (q, p, S) and the guard's <T+V> keep the explicit stages: S' = T - V is
// quadratic in the stage points.  Then the HK prefactor (diagonal widths: D x D, or the projected d' x d' matrix
// L (M R) of propagators.py:969-994), its determinant by lane-pivoted elimination (sc_row16.h) and the branch tracker.
//
// Mapping as in sc_wm_small.hip: lane a of a 16-lane row holds row a of every matrix of its trajectory; Phi and the other
// per-row constants sit in LDS (staged once per workgroup), uniform constants come from scalar registers.
// Replaces hk_step_kernel<true> (every matrix in LDS, one 64-thread workgroup per trajectory) for the instantiated
// shapes: config 3 (methylium, D = 12, d' = 6, n = 1e5) 1.78 -> 0.20 ms (docs/NOTEBOOK.md section 4.2).
#include "sc_lin16.h"

#ifndef SC_LIN_OCC
#define SC_LIN_OCC 2      // waves per SIMD the kernel is compiled for
#endif
#ifndef SC_LIN_FORCE_FIXUP
#define SC_LIN_FORCE_FIXUP 0     // 1: variant library that hands every determinant to the pivoted fix-up launch
#endif

#ifndef SC_LIN_DMA
#define SC_LIN_DMA 1      // 0: variant library without the LDS-DMA row prefetch (every shape on the direct loads)
#endif

namespace {

// Row prefetch through LDS (even D: a 16-byte unit never straddles two matrix rows).  The four trajectories of a wavefront
// are contiguous in memory; per HALF of the product ([Mqq, Mpq], then [Mqp, Mpp]) they are 4 D^2 16-byte units, which the
// wavefront requests with fully coalesced LDS-DMA loads (global_load_lds_dwordx4, 1 KB per instruction, no registers)
// into ITS OWN buffer: no workgroup barrier, the wavefront waits for its own vmcnt.  Lane (g, r) then reads row r of its
// trajectory from LDS.  The direct loads this replaces had every lane fetch its 8 D-byte row with 16-byte loads at a lane
// stride of 8 D bytes: 48 partially used 64-byte requests per instruction, and a memory round trip exposed in every pass.
template <int D>
struct LinDma {
    static constexpr bool on = SC_LIN_DMA && (D % 2 == 0);
    static constexpr int DD = D * D;
    static constexpr int half_units = 4 * DD;                 // 16-byte units per wavefront and half
    static constexpr int ndma = (half_units + 63) / 64;       // requests per half
    static constexpr int wave_units = ndma * 64 + 64;         // + one request of per-trajectory scalars
    static constexpr int zero_units = (DD + D + 1) / 2;       // rows of zeros for the lanes r >= D of a 16-lane row
    static constexpr int units = on ? 4 * wave_units + zero_units : 1;
};

__device__ __forceinline__ void lin_opaque(kptr &p) { asm volatile("" : "+s"(p)); }
__device__ __forceinline__ void lin_opaque(int &v) { asm volatile("" : "+v"(v)); }

// the way back: the lane's new rows of two blocks into the wavefront's buffer (same addresses as lin_lds_rows) ...
template <int D, int I>
__device__ __forceinline__ void lin_lds_put_rows(unsigned addr, const double (&Xq)[D], const double (&Xp)[D]) {
    if constexpr (I < D / 2) {
        const lin_d2v vq = {Xq[2 * I], Xq[2 * I + 1]}, vp = {Xp[2 * I], Xp[2 * I + 1]};
        asm volatile("ds_write_b128 %0, %1 offset:%2" : : "v"(addr), "v"(vq), "n"(16 * I) : "memory");
        asm volatile("ds_write_b128 %0, %1 offset:%2" : : "v"(addr), "v"(vp), "n"(8 * D * D + 16 * I) : "memory");
        lin_lds_put_rows<D, I + 1>(addr, Xq, Xp);
    }
}
// ... and out of it in the order of the requests: unit 64 j + lane
template <int NJ, int J>
__device__ __forceinline__ void lin_lds_unit_reads(unsigned addr, lin_d2v (&v)[NJ]) {
    if constexpr (J < NJ) {
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=&v"(v[J]) : "v"(addr), "n"(1024 * J));
        lin_lds_unit_reads<NJ, J + 1>(addr, v);
    }
}
template <int NJ>
__device__ __forceinline__ void lin_lds_units(unsigned addr, lin_d2v (&v)[NJ]) {
    lin_lds_unit_reads<NJ, 0>(addr, v);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < NJ; ++j) asm volatile("" : "+v"(v[j]));
}

// Waves per SIMD: two for every shape (256 registers per lane).  The loop of the prefetching shapes must not spill: a scratch
// reload is a vector-memory operation, and its vmcnt wait would also wait for every row request in flight (measured with
// the prefactor accumulated from whole rows: 115 spilled registers at two waves, 0.40 ms with one wave and accumulator
// registers as spill space -- no faster than without the prefetch; accumulated half by half the kernel needs 253).
template <int D> constexpr int lin_occ() { return SC_LIN_OCC; }

template <int D, int DP, bool DIAG>
__global__ __launch_bounds__(256, lin_occ<D>()) void hk_step_lin_kernel(StepArgs A) {
    typedef Lin16Consts<D, DP, DIAG> L;
    constexpr int DD = D * D, N = DIAG ? D : DP;
    extern __shared__ double2 smem2[];
    const int tid = threadIdx.x, r = tid & 15, grp = tid >> 4;
    const bool do_step = (A.mode & 0xff) == 0;
    const double dt = A.dt, hh = 0.5 * dt, h6 = dt / 6.0;

    const L C((double *)smem2);
    double *red = (double *)smem2 + L::n_doubles;
    C.stage(A, tid);           // (a prefactor-only launch has no Phi: zeros)
    __syncthreads();
    const double x0 = C.svec[r], g0 = C.svec[16 + r], im = C.svec[32 + r], sta = C.svec[48 + r], ista = C.svec[64 + r];
    kptr ksi = (kptr)A.hk.si;

    // ---- row prefetch (LinDma) ----
    typedef LinDma<D> Dm;
    __shared__ lin_d2v rowbuf[Dm::units];
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), gl = grp & 3;
    lin_d2v *wbuf = rowbuf + (Dm::on ? wave * Dm::wave_units : 0);
    const double *sbuf = (const double *)(wbuf + Dm::ndma * 64);         // the quad's (q, p), S, c2, sign: 8 D + 16 doubles
    // unit u = 64 j + lane of a half: trajectory g = u / DD, block (u / (DD / 2)) & 1, element pair u % (DD / 2); its
    // source, in doubles from the quad's first block of that half: 4 DD g + 2 DD blk + 2 (u % (DD / 2)) = 2 u + DD (u / (DD / 2))
    auto soff = [&](int j) { const int u = 64 * j + lane; return u < Dm::half_units ? 2 * u + DD * (u / (DD / 2)) : -1; };
    unsigned rowaddr = 0;         // LDS byte address of this lane's row in block 0 of the wavefront's buffer
    unsigned unitaddr = 0;        // ... of this lane's 16-byte unit of request 0
    if (Dm::on) {
        for (int e = tid; e < Dm::zero_units; e += 256) rowbuf[4 * Dm::wave_units + e] = (lin_d2v){0.0, 0.0};
        const unsigned base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) lin_d2v *)rowbuf;
        rowaddr = r < D ? base + 16u * (unsigned)(wave * Dm::wave_units) + 8u * (unsigned)((gl * 2) * DD + r * D)
                        : base + 16u * (unsigned)(4 * Dm::wave_units);
        unitaddr = base + 16u * (unsigned)(wave * Dm::wave_units + lane);
        __syncthreads();
    }
    const int64_t n = A.st.n;
    // requests of a COMPLETE quad (tq + 4 <= n): one half of the monodromy rows; the per-trajectory scalars
    auto dma_half = [&](int64_t tq, int h) {
        const double *src = A.st.mono + tq * 4 * (int64_t)DD + (h ? DD : 0);
#pragma unroll
        for (int j = 0; j < Dm::ndma; ++j)
            if (soff(j) >= 0)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + soff(j)),
                                                 (__attribute__((address_space(3))) void *)(wbuf + 64 * j), 16, 0, 0);
    };
    auto dma_scalars = [&](int64_t tq) {
        // 16-byte units of one request: 4 D of (q, p) [4 trajectories x 2 D doubles, contiguous], 2 of S, 4 of c2, 2 of the signs
        const double *src = nullptr;
        if (lane < 4 * D) src = A.st.qp + tq * 2 * D + 2 * lane;
        else if (lane < 4 * D + 2) src = A.st.act + tq + 2 * (lane - 4 * D);
        else if (lane < 4 * D + 6) src = A.st.c2 + 2 * tq + 2 * (lane - 4 * D - 2);
        else if (lane < 4 * D + 8) src = A.st.sgn + tq + 2 * (lane - 4 * D - 6);
        if (src)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(wbuf + Dm::ndma * 64), 16, 0, 0);
    };
    auto prefetch = [&](int64_t t0) { dma_scalars(t0 + 4 * wave); dma_half(t0 + 4 * wave, 0); };

    double esum = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 16;
    // results of the PREVIOUS prefetching pass: their stores wait for the top of the next pass, so that the vmcnt(0) there
    // never waits for a young store
    cplx pend_det = c_make(0.0, 0.0);
    double pend_sgn = 0.0;                 // new branch sign, 0 = unchanged
    int64_t pend_tr = -1;
    int pend_weak = 0;
    auto commit = [&]() {
        if (pend_tr >= 0 && r == 0) {
            if (pend_weak && A.st.flags) {
                A.st.flags[pend_tr] = 1;
                atomicAdd(&A.st.flags[n], 1);
            } else {
                if (pend_sgn != 0.0) A.st.sgn[pend_tr] = pend_sgn;
                ((cplx *)A.st.c2)[pend_tr] = pend_det;
            }
        }
        pend_tr = -1;
    };

    // One pass over the workgroup's 16 trajectories.  FETCHED: all 16 exist and their rows and scalars were requested into
    // LDS by the previous pass (or the prologue); otherwise (ragged last pass, odd D, prefactor-only mode) direct loads.
    auto pass = [&](auto fetched_c, int64_t t0) {
        constexpr bool FETCHED = decltype(fetched_c)::value;
        const bool active = t0 + grp < n;
        const int64_t tr = active ? t0 + grp : n - 1;
        double *qp = A.st.qp + tr * 2 * D;
        double *M = A.st.mono + tr * 4 * (int64_t)DD;
        lin_opaque(ksi);
        int lofs = 0;
        lin_opaque(lofs);
        const double *cH = C.sH + lofs + r * L::PH, *cPhi = C.sPhi + lofs + r * L::PP;        // the lane's rows of the constants

        double q = 0.0, p = 0.0;
        // the read-modify-write operands of the row's first lane (action, previous determinant and branch sign) come with
        // the coordinates: the additions and the tracker at the end of the pass do not wait for memory
        double act_old = 0.0, sgn_old = 1.0;
        cplx prev = c_make(0.0, 0.0);
        if constexpr (FETCHED) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wavefront's scalars and first-half rows have landed
            const int rr = r < D ? r : 0;
            q = sbuf[gl * 2 * D + rr]; p = sbuf[gl * 2 * D + D + rr];
            act_old = sbuf[8 * D + gl]; prev = c_make(sbuf[8 * D + 4 + 2 * gl], sbuf[8 * D + 5 + 2 * gl]); sgn_old = sbuf[8 * D + 12 + gl];
            if (r >= D) { q = 0.0; p = 0.0; }
            commit();                                             // the previous pass's results: behind the reads above
        } else {
            WM_BLOCK {
                if (r < D) { q = qp[r]; p = qp[D + r]; }
                if (do_step && r == 0) { act_old = A.st.act[tr]; prev = ((const cplx *)A.st.c2)[tr]; sgn_old = A.st.sgn[tr]; }
            }
        }

        // ---- prefactor, accumulated HALF by half of the monodromy rows (lin_prefactor_half): a half is consumed as soon as its
        // product is there and never lives next to the other one ----
        cplx mat[N];
        Lin16Sums<DP, DIAG> sums;
        auto accum_half = [&](auto hc, const double (&Xhq)[D], const double (&Xhp)[D]) {
            constexpr int h = decltype(hc)::value;
            lin_prefactor_half<D, DP, DIAG, h>(mat, sums, (h ? C.sR2 : C.sR1) + lofs + r * L::PR, ksi, sta, ista, r, Xhq, Xhp);
        };

        if (FETCHED || do_step) {
            double red5[5];
            lin_rk4_row<D>(cH, r, x0, g0, im, dt, hh, h6, q, p, red5);
            {
                double one = 1.0;
                asm volatile("" : "+v"(one));
                lin_rk4_sums<D>(red5, one, A.pot.scalar0);
            }
            if (active && r < D) { qp[r] = q; qp[D + r] = p; }
            if (active && r == 0) {
                A.st.act[tr] = act_old + h6 * (red5[0] + 2.0 * red5[1] + 2.0 * red5[2] + red5[3]);
                esum += red5[4];
            }

            // ---- [X; Y] <- Phi [X; Y], one half (Mqq, Mpq | Mqp, Mpp) at a time (lin_phi_half) ----
            double Told[2][2][D], Xn[2][2][D];          // old and new rows: [half][q | p][column]
            if constexpr (FETCHED) {
                lin_lds_rows<D>(rowaddr, Told[0][0], Told[0][1]);
                dma_half(t0 + 4 * wave, 1);           // second half into the same buffer, under the first half's product
            } else {
                // BOTH halves requested together: one HBM round trip per trajectory instead of one per half of the product
#pragma unroll
                for (int h = 0; h < 2; ++h) lin_load_half<D>(M, r, h, Told[h][0], Told[h][1]);
            }
            auto product = [&](auto hc) {
                constexpr int h = decltype(hc)::value;
                lin_phi_half<D>(cPhi, Told[h][0], Told[h][1], Xn[h][0], Xn[h][1]);
            };
            auto store_half = [&](int h) {
                if constexpr (FETCHED) {
                    // through the wavefront's buffer (free between the row reads and the next request) and out in 1 KB
                    // instructions: the lanes' own rows are 8 D bytes apart, a store of theirs is 48 quarter-used 64-byte
                    // requests
                    if (r < D) lin_lds_put_rows<D, 0>(rowaddr, Xn[h][0], Xn[h][1]);
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the rows are in LDS before other lanes read them
                    lin_d2v v[Dm::ndma];
                    lin_lds_units<Dm::ndma>(unitaddr, v);
                    double *dst = A.st.mono + (t0 + 4 * wave) * 4 * (int64_t)DD + (h ? DD : 0);
#pragma unroll
                    for (int j = 0; j < Dm::ndma; ++j)
                        if (soff(j) >= 0) *(lin_d2v *)(dst + soff(j)) = v[j];
                    return;
                }
                if (active && r < D) lin_store_half<D>(M, r, h, Xn[h][0], Xn[h][1]);
            };
            product(std::integral_constant<int, 0>{});
            accum_half(std::integral_constant<int, 0>{}, Xn[0][0], Xn[0][1]);
            if constexpr (FETCHED) {
                // only the second half's requests are in flight here (the first half's stores come behind this wait)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                lin_lds_rows<D>(rowaddr, Told[1][0], Told[1][1]);
            }
            store_half(0);
            product(std::integral_constant<int, 1>{});
            store_half(1);
            // operands of the next pass: requested here, they land under the rest of the prefactor
            if constexpr (FETCHED)
                if (t0 + stride + 16 <= n) prefetch(t0 + stride);
            accum_half(std::integral_constant<int, 1>{}, Xn[1][0], Xn[1][1]);
        } else {
            // prefactor only: rows of the stored blocks, half by half
            sfor<0, 2>([&](auto hc) {
                constexpr int h = decltype(hc)::value;
                double Xq[D], Xp[D];
                WM_BLOCK { lin_load_half<D>(M, r, h, Xq, Xp); }
                accum_half(hc, Xq, Xp);
            });
        }
        if constexpr (!DIAG) lin_sandwich<D, DP>(mat, sums, C.sL1 + lofs + r * L::PL, C.sL2 + lofs + r * L::PL);
        // determinant in the fixed pivot order (sc_row16.h); a weak pivot hands the trajectory to the fully pivoted
        // elimination of hk_step_kernel (fix-up launch of sc_hk_step, as on the separable fast path)
        int weak = SC_LIN_FORCE_FIXUP;
        const cplx det = det_rows_fixed_order<N>(mat, r, weak);
        double newsgn = 0.0;
        if (do_step) { if (crossed_branch_cut(prev, det)) newsgn = -sgn_old; }
        else newsgn = 1.0;
        if (active) { pend_tr = tr; pend_det = det; pend_weak = weak; pend_sgn = newsgn; }
        if constexpr (!FETCHED) commit();
    };

    int64_t t0 = (int64_t)blockIdx.x * 16;
    if constexpr (Dm::on) {
        if (do_step) {
            if (t0 + 16 <= n) prefetch(t0);
            for (; t0 + 16 <= n; t0 += stride) pass(std::true_type{}, t0);
            commit();
        }
    }
    for (; t0 < n; t0 += stride) pass(std::false_type{}, t0);
    if (r == 0) red[grp] = esum;
    __syncthreads();
    if (tid == 0 && A.epart && do_step) {
        double s = 0.0;
        for (int g = 0; g < 16; ++g) s += red[g];
        A.epart[blockIdx.x] = s;
    }
    // the energy guard adds sc_step_grid(n, D) partials: workgroup 0 zeroes the ones no workgroup owns
    if (blockIdx.x == 0 && A.epart && do_step)
        for (int i = gridDim.x + tid; i < A.npart; i += 256) A.epart[i] = 0.0;
}

template <int D, int DP, bool DIAG>
int launch(const StepArgs &a, int grid, hipStream_t s) {
    const size_t lds = (size_t)(Lin16Consts<D, DP, DIAG>::n_doubles + 16) * 8;       // + the energy partials of the 16 rows
    if (hipFuncSetAttribute((const void *)hk_step_lin_kernel<D, DP, DIAG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess)
        return sc_check_launch("sc_hk_step (LDS attribute)");
    // persistent grid: one (prefetching shapes) or two workgroups per CU are resident; every further workgroup would stage
    // the constants (12 KB) again for one or two passes over 16 trajectories.  The kernel clears the energy partials it leaves.
    // the row prefetch moves 16-byte units: state arrays that are not 16-byte aligned go to the general kernel
    if (LinDma<D>::on && ((((uintptr_t)a.st.mono | (uintptr_t)a.st.qp | (uintptr_t)a.st.act | (uintptr_t)a.st.c2 | (uintptr_t)a.st.sgn) & 15) != 0))
        return 0;
    static_assert(!LinDma<D>::on || 4 * D + 8 <= 64, "one request holds the scalars of a quad");
    const int resident = lin_occ<D>() * 256;
    hipLaunchKernelGGL((hk_step_lin_kernel<D, DP, DIAG>), dim3(grid < resident ? grid : resident), dim3(256), lds, s, a);
    const int rc = sc_check_launch("sc_hk_step (constant-Hessian register kernel)");
    return rc == SC_OK ? 1 : rc;
}

}  // namespace

// returns 1 and launches if the shape (D, d', diagonal widths) is instantiated, 0 if not, < 0 on error.  The caller
// guarantees: SC_POT_HARMONIC_DENSE, pot.lin_prop built for this dt (mode 0), row-major monodromy blocks.
int sc_launch_step_lin(const StepArgs &a, int grid, hipStream_t s) {
    return lin16_dispatch<false>(a.hk, a.st.dim, [&](auto d, auto dp, auto diag) {
        return launch<decltype(d)::value, decltype(dp)::value, decltype(diag)::value>(a, grid, s);
    });
}

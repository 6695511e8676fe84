// HK time step for a CONSTANT dense Hessian (SC_POT_HARMONIC_DENSE) with 16 < D <= 64, the monodromy blocks held in
// NORMAL-MODE coordinates (include/semiclassical_hip.h: sc_hk_step_modal).
//
// With W = m^-1/2 H m^-1/2 = U diag(lambda) U^T, A = m^-1/2 U, B = m^1/2 U and Mqq~ = A^-1 Mqq A, Mqp~ = A^-1 Mqp B,
// Mpq~ = B^-1 Mpq A, Mpp~ = B^-1 Mpp B, the RK4 step of the monodromy equations is a 2 x 2 matrix per ROW mode a:
//     (Mqq~, Mpq~)[a][b] <- phi_a (Mqq~, Mpq~)[a][b],   (Mqp~, Mpp~)[a][b] <- phi_a (Mqp~, Mpp~)[a][b]
// -- an elementwise stream over the 4 D^2 doubles, the only HBM traffic of any size.  The prefactor matrix is the
// reference's expression (propagators.py:951-1004) with the transformed real constants L1~ = L1 A, L2~ = L2 B,
// R1~ = A^-1 R1, R2~ = B^-1 R2:
//     Re P = 1/2 [L1~ (Mqq~ R1~) + L2~ (Mpp~ R2~)]      Im P = 1/2 [-hbar L1~ (Mqp~ R2~) + 1/hbar L2~ (Mpq~ R1~)]
// Both products run on v_mfma_f64_16x16x4_f64.  One 256-thread workgroup per trajectory at a time:
//   * (q, p, S): RK4 in Cartesian coordinates with the reference's stage order (propagators.py:86-119, 313-383), as the
//     dense branch of hk_step_kernel (sc_hk_step.hip) does;
//   * blocks: row tile ra (16 modes) of all four planes is read from HBM, stepped, written back and parked in LDS;
//   * first product: a wavefront owns a task (part = Re / Im, column tile jt of P) and forms the 16 x 16 tiles
//     Y = M~[ra rows] R~[:, jt] of the two planes of its part (A operand from the LDS panel, B operand R~ in LDS);
//   * second product: the accumulator layout of Y (col = lane & 15, row = (lane >> 4) + 4 reg) IS the B-operand layout
//     of the next product with k = 16 ra + 4 reg + (lane >> 4) (as in sc_dense_mono.hip), so P[:, jt] += L~[:, ra rows] Y
//     follows without moving Y; P stays in registers until all row tiles are done;
//   * determinant: pivoted LU in LDS (lds_lu_det, partial pivoting over the whole column -- no fixed-order elimination,
//     hence no weak pivot to hand to a fix-up pass), then the branch tracker (propagators.py:1005-1052).
#include "sc_common.h"
#include "sc_prefactor.h"

namespace {

struct ModalArgs {
    StepArgs s;
    const double *mode_prop;    // [D][4] (phi_qq, phi_qp, phi_pq, phi_pp) per mode
    int h_lds, l_lds;           // the Hessian / the left constants L~ are staged in LDS (1) or read from global memory (0)
};

typedef double d4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline size_t al2(size_t x) { return (x + 1) & ~size_t(1); }

struct ModalLds {
    size_t red, ipiv, drv, phi, R, L, H, U, total;      // offsets in doubles
};

// LDS carve-up shared by the launcher (size) and the kernel (offsets); every offset even => 16-byte aligned
__host__ __device__ inline ModalLds modal_lds(int D, int dp, int h_lds, int l_lds) {
    const int KP = 4 * ((D + 3) / 4), JP = 16 * ((dp + 15) / 16);
    ModalLds o;
    size_t off = 0;
    o.red = off; off += 32;
    o.ipiv = off; off += 2;
    o.drv = off; off += al2(D);
    o.phi = off; off += al2(4 * D);
    o.R = off; off += al2(2 * (size_t)KP * JP);                     // R1~, R2~ real, [KP][JP], zero padded
    o.L = off; if (l_lds) off += al2(2 * (size_t)dp * D);          // L1~, L2~ real, [dp][D]
    o.H = off; if (h_lds) off += al2((size_t)D * D);
    o.U = off;
    const size_t panel = 4 * 16 * (size_t)KP, mat = 2 * (size_t)dp * dp;
    off += al2(panel > mat ? panel : mat);                           // row panel of the blocks, later the prefactor matrix
    o.total = off;
    return o;
}

__global__ __launch_bounds__(256) void hk_step_modal_kernel(ModalArgs MA) {
    extern __shared__ double2 smem2[];
    double *smem = (double *)smem2;
    const StepArgs &A = MA.s;
    const int D = A.st.dim, DD = D * D, dp = A.hk.dprime, tid = threadIdx.x, nth = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int KT = (D + 3) / 4, KP = 4 * KT, NT = (D + 15) / 16, JT = (dp + 15) / 16, JP = 16 * JT;
    const bool do_step = (A.mode & 0xff) == 0, init_track = (A.mode & 0xff) == 1;
    const double dt = A.dt, hh = 0.5 * dt, h6 = dt / 6.0;
    const ModalLds o = modal_lds(D, dp, MA.h_lds, MA.l_lds);
    double *red = smem + o.red, *drv = smem + o.drv, *phi = smem + o.phi, *Rs = smem + o.R, *Ls = smem + o.L;
    int *ipiv = (int *)(smem + o.ipiv);
    double *panel = smem + o.U;
    cplx *mat = (cplx *)(smem + o.U);
    const double *Hm = MA.h_lds ? smem + o.H : A.pot.par2;
    const double *R1g = A.hk.R1, *R2g = A.hk.R2, *L1g = A.hk.L1, *L2g = A.hk.L2;      // complex, real parts used

    for (int e = tid; e < 4 * D; e += nth) phi[e] = MA.mode_prop[e];
    for (int e = tid; e < KP * JP; e += nth) {
        const int k = e / JP, j = e - k * JP;
        const bool ok = k < D && j < dp;
        Rs[e] = ok ? R1g[2 * (k * dp + j)] : 0.0;
        Rs[KP * JP + e] = ok ? R2g[2 * (k * dp + j)] : 0.0;
    }
    if (MA.l_lds)
        for (int e = tid; e < dp * D; e += nth) { Ls[e] = L1g[2 * e]; Ls[dp * D + e] = L2g[2 * e]; }
    if (MA.h_lds)
        for (int e = tid; e < DD; e += nth) smem[o.H + e] = A.pot.par2[e];
    __syncthreads();

    double esum = 0.0;
    for (int64_t tr = blockIdx.x; tr < A.st.n; tr += gridDim.x) {
        double *qp = A.st.qp + tr * 2 * D;
        double *M = A.st.mono + tr * 4 * (int64_t)DD;

        if (do_step) {
            // ---------------- (q, p, S): V = E0 + g.dr + 1/2 dr.H.dr - origin, grad = g + H.dr   potentials.py:583-590
            double red5[5] = {0, 0, 0, 0, 0};
            double qn = 0, pn = 0;
            const bool own = tid < D;
            double q = 0, p = 0, im = 0;
            if (own) { q = qp[tid]; p = qp[D + tid]; im = A.pot.inv_mass[tid]; }
            double kqs = 0, kps = 0;
            const double g0 = own ? A.pot.par1[tid] : 0.0, x0 = own ? A.pot.par0[tid] : 0.0;
            for (int s = 0; s < 4; ++s) {
                double qs = q, ps = p;
                if (s > 0) { const double c = (s == 3) ? dt : hh; qs = q + c * kqs; ps = p + c * kps; }
                __syncthreads();
                if (own) drv[tid] = qs - x0;
                __syncthreads();
                double kq = 0, kp = 0;
                if (own) {
                    double hd = 0.0;
                    for (int b = 0; b < D; ++b) hd = fma(Hm[tid * D + b], drv[b], hd);
                    const double dr = qs - x0;
                    const double v = dr * g0 + 0.5 * dr * hd;   // + scalar0 added after the reduction
                    kq = ps * im; kp = -(g0 + hd);
                    const double t = 0.5 * ps * ps * im;
                    red5[s] = t - v;
                    if (s == 3) red5[4] = t + v;
                    const double w = (s == 0 || s == 3) ? 1.0 : 2.0;
                    qn += w * kq; pn += w * kp;
                }
                kqs = kq; kps = kp;
            }
            if (own) { qn = q + h6 * qn; pn = p + h6 * pn; }
            block_sum<5>(red5, red);
            for (int s = 0; s < 4; ++s) red5[s] -= A.pot.scalar0;
            red5[4] += A.pot.scalar0;
            if (own) { qp[tid] = qn; qp[D + tid] = pn; }
            if (tid == 0) {
                A.st.act[tr] += h6 * (red5[0] + 2.0 * red5[1] + 2.0 * red5[2] + red5[3]);
                esum += red5[4];
            }
        }

        // ---------------- blocks (stream) + the two products, one row tile of modes at a time ----------------
        // task t = 2 jt + part of this wavefront: t = wave and t = wave + 4 (< 2 JT)
        d4 P[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int it = 0; it < 4; ++it) P[u][it] = (d4){0.0, 0.0, 0.0, 0.0};
        for (int ra = 0; ra < NT; ++ra) {
            __syncthreads();            // previous panel consumed
            for (int e = tid; e < 16 * KP; e += nth) {
                const int rl = e / KP, b = e - rl * KP, a = 16 * ra + rl;
                double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
                if (a < D && b < D) {
                    const int64_t x = (int64_t)a * D + b;
                    const double qq = M[x], qpv = M[DD + x], pq = M[2 * DD + x], pp = M[3 * DD + x];
                    if (do_step) {
                        const double fqq = phi[4 * a], fqp = phi[4 * a + 1], fpq = phi[4 * a + 2], fpp = phi[4 * a + 3];
                        v0 = fma(fqq, qq, fqp * pq); v2 = fma(fpq, qq, fpp * pq);
                        v1 = fma(fqq, qpv, fqp * pp); v3 = fma(fpq, qpv, fpp * pp);
                        M[x] = v0; M[DD + x] = v1; M[2 * DD + x] = v2; M[3 * DD + x] = v3;
                    } else {
                        v0 = qq; v1 = qpv; v2 = pq; v3 = pp;
                    }
                }
                panel[e] = v0; panel[16 * KP + e] = v1; panel[32 * KP + e] = v2; panel[48 * KP + e] = v3;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int t = wave + 4 * u;
                if (t >= 2 * JT) continue;                           // wave-uniform
                const int part = t & 1, jt = t >> 1;
                // part 0 (Re): planes qq (R1, L1) and pp (R2, L2); part 1 (Im): planes qp (R2, L1, -hbar), pq (R1, L2, 1/hbar)
                const int pa = part ? 1 : 0, pb = part ? 2 : 3;
                const double *Ra = Rs + (part ? KP * JP : 0), *Rb = Rs + (part ? 0 : KP * JP);
                const double sa = part ? -SC_HBAR : 1.0, sb = part ? 1.0 / SC_HBAR : 1.0;
                d4 Ya = (d4){0.0, 0.0, 0.0, 0.0}, Yb = (d4){0.0, 0.0, 0.0, 0.0};
                const double *rowa = panel + pa * 16 * KP + (lane & 15) * KP + (lane >> 4);
                const double *rowb = panel + pb * 16 * KP + (lane & 15) * KP + (lane >> 4);
                const int rc = (lane >> 4) * JP + 16 * jt + (lane & 15);
                for (int kt = 0; kt < KT; ++kt) {
                    Ya = __builtin_amdgcn_mfma_f64_16x16x4f64(rowa[4 * kt], Ra[4 * kt * JP + rc], Ya, 0, 0, 0);
                    Yb = __builtin_amdgcn_mfma_f64_16x16x4f64(rowb[4 * kt], Rb[4 * kt * JP + rc], Yb, 0, 0, 0);
                }
                Ya *= sa; Yb *= sb;
                // P[:, jt] += L1~[:, 16 ra ..] Ya + L2~[:, 16 ra ..] Yb ; k-slice r: a = 16 ra + 4 r + (lane >> 4)
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    if (it >= JT) continue;
                    const int i = 16 * it + (lane & 15);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int a = 16 * ra + 4 * r + (lane >> 4);
                        double l1 = 0.0, l2 = 0.0;
                        if (i < dp && a < D) {
                            if (MA.l_lds) { l1 = Ls[i * D + a]; l2 = Ls[dp * D + i * D + a]; }
                            else { l1 = L1g[2 * (i * D + a)]; l2 = L2g[2 * (i * D + a)]; }
                        }
                        P[u][it] = __builtin_amdgcn_mfma_f64_16x16x4f64(l1, Ya[r], P[u][it], 0, 0, 0);
                        P[u][it] = __builtin_amdgcn_mfma_f64_16x16x4f64(l2, Yb[r], P[u][it], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();                // the panel region becomes the prefactor matrix
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = wave + 4 * u;
            if (t >= 2 * JT) continue;
            const int part = t & 1, jt = t >> 1, j = 16 * jt + (lane & 15);
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                if (it >= JT) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * it + (lane >> 4) + 4 * r;
                    if (i < dp && j < dp) ((double *)&mat[i * dp + j])[part] = 0.5 * P[u][it][r];
                }
            }
        }
        __syncthreads();

        // ---------------- c2 = det(mat), branch tracking ----------------
        const cplx det = lds_lu_det(mat, dp, ipiv);
        if (tid == 0) {
            cplx *c2 = (cplx *)A.st.c2;
            if (!init_track) {
                const cplx prev = c2[tr];
                if (crossed_branch_cut(prev, det)) A.st.sgn[tr] = -A.st.sgn[tr];
            } else {
                A.st.sgn[tr] = 1.0;
            }
            c2[tr] = det;
        }
        __syncthreads();
    }
    if (tid == 0 && A.epart && blockIdx.x < (unsigned)A.npart) A.epart[blockIdx.x] = esum;
}

constexpr size_t kModalLdsMax = 160 * 1024;

// which of the shared operands go to LDS next to the per-trajectory buffers.  Two workgroups per CU come first: the pivoted
// elimination of one trajectory is latency bound and overlaps with the stream / products of the other (coumarin: L~ and H in
// LDS = 130 KB, one workgroup per CU; both from L2 = 75 KB, two).  Then L~ (read once per row tile) before H.
bool modal_plan(int D, int dp, int &h_lds, int &l_lds, size_t &bytes) {
    for (size_t cap : {kModalLdsMax / 2, kModalLdsMax})
        for (int l = 1; l >= 0; --l)
            for (int h = 1; h >= 0; --h) {
                const size_t b = modal_lds(D, dp, h, l).total * sizeof(double);
                if (b <= cap) { h_lds = h; l_lds = l; bytes = b; return true; }
            }
    return false;
}

}  // namespace

extern "C" int sc_hk_step_modal_supported(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk) {
    if (!pot || !st || !hk) return 0;
    const int D = st->dim;
    int h, l;
    size_t b;
    return pot->kind == SC_POT_HARMONIC_DENSE && pot->dim == D && hk->dim == D && D > 16 && D <= 64 && hk->diag == 0 &&
           hk->real_lr != 0 && hk->dprime >= 1 && hk->dprime <= D && st->mono_layout == SC_MONO_ROWMAJOR &&
           modal_plan(D, hk->dprime, h, l, b) ? 1 : 0;
}

extern "C" int sc_hk_step_modal(const sc_potential *pot, const sc_state *st, const sc_hk_consts *hk, double dt, int32_t mode,
                                const double *mode_prop, double *energy_partials, void *stream) {
    if (!pot || !st || !hk || !mode_prop) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_step_modal: null argument");
    const int D = st->dim;
    if (pot->dim != D || hk->dim != D) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_step_modal: dimension mismatch");
    if (mode != 0 && mode != 1) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_step_modal: mode %d (0 = step, 1 = prefactor only)", mode);
    if (!sc_hk_step_modal_supported(pot, st, hk))
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_hk_step_modal: needs SC_POT_HARMONIC_DENSE, 16 < D <= 64 (D=%d), 1 <= d' <= D (d'=%d), "
                       "dense real prefactor constants (diag = 0, real_lr = 1) and the row-major storage order", D, hk->dprime);
    if (mode == 0 && (!pot->par0 || !pot->par1 || !pot->par2 || !pot->inv_mass))
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_step_modal: potential descriptor without pos0 / grad0 / hess0 / inv_mass");
    if (st->n <= 0) return SC_OK;
    int h_lds = 0, l_lds = 0;
    size_t lds = 0;
    modal_plan(D, hk->dprime, h_lds, l_lds, lds);
    const int grid = sc_step_grid(st->n, D);
    ModalArgs a{StepArgs{*pot, *st, *hk, dt, mode, energy_partials, grid}, mode_prop, h_lds, l_lds};
    hipStream_t s = (hipStream_t)stream;
    if (hipFuncSetAttribute((const void *)hk_step_modal_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return sc_check_launch("sc_hk_step_modal (LDS attribute)");
    hipLaunchKernelGGL(hk_step_modal_kernel, dim3(grid), dim3(256), lds, s, a);
    return sc_check_launch("sc_hk_step_modal");
}

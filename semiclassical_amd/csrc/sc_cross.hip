// Cross-correlation of the Herman-Kluk wavepacket with K target coherent states |q_k, p_k, Gamma_0> (not in the reference;
// DESIGN.md section 4.13) -- the O(n K D) kernels behind HermanKlukPropagator.cross_correlation() and run(targets=...).  The
// overlap is the reference's CoherentStatesOverlap, semiclassical/propagators.py:181-240 (the formula: 232-237), with the bra
// trajectory i of width Gamma_t and the ket target k of width Gamma_0:
//
//   E_ik = -1/2 dq^T A dq - 1/2 hbar^-2 dp^T B dp - i/hbar p_k.dq + i/hbar dq^T C dp,      dq = q_k - q_i, dp = p_k - p_i
//   x_ik = conj(fac exp(E_ik)) v_i,   v_i = sgn_i sqrt(c2_i) e^{i S_i/hbar} vi_i / (N (2 pi hbar)^D P_i)
//   row k of the output: sum_i of  Re x, Im x, (Re x)^2, (Im x)^2, Re x Im x.
//
// The exponent is formed from DIFFERENCES in transformed coordinates, La = A^(1/2), Lb = B^(1/2) / hbar (the host's):
//   Re E = -1/2 (|La q_k - La q_i|^2 + |Lb p_k - Lb p_i|^2),   Im E = 1/hbar sum_d dq_d ((C p_k)_d - (C p_i)_d - p_k,d)
// -- no cancellation between large q^2 terms, nothing to centre.  Operand rows: trajectory [La q | Lb p | q | C p] (4 D), target
// [La q_k | Lb p_k | q_k | C p_k | p_k] (5 D, formed by the host once per set of targets).
//
// cross_operands_kernel (dense widths only): the trajectory rows into caller-owned scratch, three D x D mat-vecs per trajectory,
//   one trajectory per wavefront pass.  Diagonal widths need no pre-pass: the tile kernel scales q and p while it stages them.
// cross_tile_kernel: the tile mapping, the column reduction and the reduction over the bands of sc_rows5.h, the columns being the
//   targets.  The staging and the d-loop are cross_tile_exponents of sc_cross_tile.h, shared with the terms kernel of the
//   time-averaged spectra (sc_timeavg.hip).  Per pair and d two FMAs for Re E and one for Im E; then one c_exp per pair and the product with v_i (formed once per
//   trajectory by the first 64 threads exactly as hk_correlate_kernel forms it).
// Discarded trajectories (`kept`) and the rows beyond n are staged as zero operands with v = 0: they add exact zeros and never
// meet a non-finite value.
#include "sc_cross_tile.h"

namespace {

struct CrossArgs {
    sc_state st;
    const double *La, *Lb, *Cm;     // diagonal widths: [D] each (the tile kernel scales); dense: unused here
    const double *operands;         // dense widths: [n][4 D] from cross_operands_kernel
    const double *targets;          // [K][5 D]
    int K;
    double fac, mc_norm;
    const double *vi, *probi;
    const uint8_t *kept;            // may be NULL
    double *partials;               // [bands][K][5]
};

template <bool DIAG>
__global__ __launch_bounds__(256) void cross_tile_kernel(CrossArgs A) {
    __shared__ CrossStage S;
    __shared__ double2 vs[R5_TILE]; // v_i of the band's trajectories (0: beyond n, or discarded)
    __shared__ int live[R5_TILE];
    static_assert(sizeof(CrossStage) >= sizeof(double) * R5_REDUCE_DOUBLES, "the column reduction reuses the staging buffers");
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int64_t n = A.st.n, i0 = (int64_t)blockIdx.y * R5_TILE;
    const int k0 = blockIdx.x * R5_TILE;
    const int iv = (int)min((int64_t)R5_TILE, n - i0), kv = min(R5_TILE, A.K - k0);      // valid rows / targets of the tile
    if (tid < R5_TILE) {
        cplx v = c_make(0.0, 0.0);
        const int64_t tr = i0 + tid;
        const bool in = tid < iv && (!A.kept || A.kept[tr]);
        if (in) {
            // signed_root and action_phase (sc_common.h: what hk_correlate_kernel calls), the initial overlap, the Monte-Carlo weight
            const cplx c = signed_root(((const cplx *)A.st.c2)[tr], A.st.sgn[tr]);
            const cplx ph = action_phase(A.st.act[tr]);
            const double w = 1.0 / (A.mc_norm * A.probi[tr]);
            v = c_scale(c_mul(((const cplx *)A.vi)[tr], c_mul(c, ph)), w);
        }
        vs[tid] = v;
        live[tid] = in;
    }
    double re[4][4], im[4][4];
    cross_tile_exponents<DIAG>(S, live, A.st, A.La, A.Lb, A.Cm, A.operands, A.targets, i0, k0, kv, tid, ti, tj, re, im);
    // x_ik = conj(fac exp(E)) v_i; the thread's four trajectories are added per target in registers
    double sum[4][5];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
        for (int c = 0; c < 5; ++c) sum[b][c] = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const cplx o = cross_tile_overlap_conj(re[a][b], im[a][b], A.fac);
            const cplx x = c_mul(o, vs[4 * ti + a]);
            rows5_add(sum[b], x);
        }
    }
    rows5_store_partials(sum, &S, tid, ti, tj, kv, k0, A.K, A.partials);
}

// dense widths: operands[i] = [La q_i | Lb p_i | q_i | C p_i].  La and Lb are symmetric, Ct is the TRANSPOSE of C: element (a, b)
// of all three is read at [b D + a], consecutive lanes consecutive addresses.  One trajectory per wavefront pass.
__global__ __launch_bounds__(256) void cross_operands_kernel(sc_state st, const double *La, const double *Lb, const double *Ct,
                                                             double *operands) {
    extern __shared__ double smem[];
    const int D = st.dim, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *qp = smem + (size_t)wave * 2 * D;
    for (int64_t tr = (int64_t)blockIdx.x * 4 + wave; tr < st.n; tr += (int64_t)gridDim.x * 4) {
        for (int a = lane; a < 2 * D; a += 64) qp[a] = st.qp[tr * 2 * D + a];
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_s_waitcnt(0xC07F);                // lgkmcnt(0): the wave's own LDS writes have landed
        double *row = operands + tr * 4 * D;
        for (int a = lane; a < D; a += 64) {
            double ya = 0.0, yb = 0.0, yc = 0.0;
            for (int b = 0; b < D; ++b) {
                ya = fma(La[(size_t)b * D + a], qp[b], ya);
                yb = fma(Lb[(size_t)b * D + a], qp[D + b], yb);
                yc = fma(Ct[(size_t)b * D + a], qp[D + b], yc);
            }
            row[a] = ya; row[D + a] = yb; row[2 * D + a] = qp[a]; row[3 * D + a] = yc;
        }
        __builtin_amdgcn_wave_barrier();                   // every lane has read qp before the next trajectory overwrites it
    }
}

}  // namespace

int sc_cross_operands(const char *who, const sc_state *st, const double *La, const double *Lb, const double *Ct, double *operands,
                      hipStream_t stream) {
    const int64_t blocks = (st->n + 3) / 4;
    hipLaunchKernelGGL(cross_operands_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256),
                       (size_t)4 * 2 * st->dim * sizeof(double), stream, *st, La, Lb, Ct, operands);
    return sc_check_launch(who);
}

extern "C" int64_t sc_hk_cross_rows(int64_t n, int64_t K) { return sc_rows5_bands(n, K); }

extern "C" int sc_hk_cross(const sc_state *st, const double *La, const double *Lb, const double *Ct, int32_t diag, double fac,
                           const double *targets, int32_t K, const double *vi, const double *probi, double mc_norm,
                           const uint8_t *kept, double *operands, double *partials, double *out, const int64_t *cursor,
                           void *stream) {
    if (!st || !La || !Lb || !Ct || !targets || !vi || !probi || !partials || !out)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_hk_cross: null argument");
    int rc = sc_rows5_limits("sc_hk_cross", "K", "targets", st->n, st->dim, K,
                             !diag && !operands ? "dense widths need the operand scratch [n][4 D]" : nullptr);
    if (rc != SC_OK) return rc;
    const int64_t bands = sc_rows5_bands(st->n, K);
    hipStream_t s = (hipStream_t)stream;
    if (bands > 0) {
        if (!diag) {
            rc = sc_cross_operands("sc_hk_cross (operands)", st, La, Lb, Ct, operands, s);
            if (rc != SC_OK) return rc;
        }
        CrossArgs a{*st, La, Lb, Ct, operands, targets, K, fac, mc_norm, vi, probi, kept, partials};
        const dim3 grid((unsigned)((K + R5_TILE - 1) / R5_TILE), (unsigned)bands);
        if (diag) hipLaunchKernelGGL(cross_tile_kernel<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(cross_tile_kernel<false>, grid, dim3(256), 0, s, a);
        rc = sc_check_launch("sc_hk_cross");
        if (rc != SC_OK) return rc;
    }
    return sc_rows5_reduce("sc_hk_cross (reduction)", partials, bands, K, out, cursor, s);
}

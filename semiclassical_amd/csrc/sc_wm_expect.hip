// Expectation values of x, p and quadratic x operators in the Walton-Manolopoulos wavepacket (not in the reference; DESIGN.md
// section 4.24) -- the O(n^2) kernel behind WaltonManolopoulosPropagator.wm_expectation():
//
//   out[a] = sum_ij T_ij F_a,ij   (a < M),      out[M] = sum_ij T_ij,
//   T_ij   = conj(v_i) O_ij v_j                 the pair term of sc_wm_pair_sum_rect, same operands (the comment in sc_wm.hip),
//   F_a,ij = kap_a + sum_col lam_col f_col,     f_col = l_col for column 0 of an operator, l_col^2 + s_col^T D'^-1 s_col for its
//                                               columns 1 ... R,
//   l_col  = za[col][i] + zb[col][j] + g_col . b' + s_col^T D'^-1 b',
//   s_col  = sfix[col]  (+ sket[a][j] for column 0 of operator a, when sket is given),
//
// D' = conj(C'_i) + C'_j and b' = U^T C_j dQ + conj(d'_i) + d'_j as in the norm: the mean of x under the product of the two Gaussians
// is Q_i + U D'^-1 b', its covariance U D'^-1 U^T.
//
// wm_expect_kernel: one wavefront per pair, NW = blockDim.x / 64 wavefronts per tile of 16 x 16 pairs, for every shape.  Each wavefront
// owns an LDS region with the bordered matrix of nt = d' + 1 + C rows and columns, C = M (1 + R),
//     [ D'    b'   S ]
//     [ b'^T  0    0 ]       S = (s_0 ... s_C-1), row stride odd (in complex elements),
//     [ S^T   0    0 ]
// and eliminates the first d' columns with partial pivoting among the first d' rows (row swaps there leave the Schur complement as
// it is).  Rows up to b'^T carry every column, the row of s_col only the columns of D' and its own diagonal entry: what is left is
//     M[d'][d'] = -b'^T D'^-1 b',   M[d'][d'+1+col] = -b'^T D'^-1 s_col,   M[d'+1+col][d'+1+col] = -s_col^T D'^-1 s_col.
// det(D'/2pi) is kept as mantissa x 2^e, T_ij formed in log space.  Lane col then forms lam_col f_col, lane a adds the columns of
// operator a in order and accumulates T F_a in its registers (operators a and a + 64); the tile's wavefronts are added in order
// through LDS: ONE store per output and tile into partials[tile][M + 1][2].  expect_reduce_kernel adds the tiles.  No atomics,
// nothing skipped by magnitude (a pair whose D' is exactly singular adds nothing, as in the norm); the order of every sum is a
// function of (ni, nj, D, d', M, R) alone: the same bits in every run.
//
// A launch carries the columns that fit: nt <= 128 (two rows per lane) and nt * (nt | 1) complex within the LDS of a workgroup;
// sc_wm_pair_expect_capacity(D, d') is that number (4 at d' = 96).
//
// wm_expect_cols_kernel (sc_wm_pair_expect_cols) is the same pair loop, wme_body<true>, with a kind and a
// slot of per-ket border vectors per column: f_col = l_col (kind 0), l_col^2 + s_col^T D'^-1 s_col (1), exp(-l_col + 1/2 s_col^T
// D'^-1 s_col) (2), s_col = sfix[col] (+ sket[ketcol[col]][j]) -- quadratic momentum operators acting on the ket and exp(-a.x).
// Same region, capacity and order of the sums.
#include <algorithm>

#include "sc_expect_tile.h"

namespace {

#define WME_MAXD 512
#define WME_MAXDP 96
#define WME_MAXROWS 128
#define WME_LDS (160 * 1024 - 64)

struct WmExpectArgs {
    const double *qp_i, *coef_i, *cqqp_i, *dvecp_i;                       // bras i: [ni] ...
    const double *qp, *coef, *cqq, *dvec, *cqqp, *dvecp, *U;               // kets j: [nj] ...
    int64_t ni, n;
    int D, dp;
    const double *za, *zb;              // [C][ni], [C][nj] complex, trajectory index fastest
    const double *g, *sfix;             // [C][d'] complex
    const double *sket;                 // NULL or [M][nj][d'] complex
    const double *lam;                  // [C]
    const double *kap;                  // [M] complex
    int M, R;
    double *partials;                   // [tiles][M + 1][2]
};

struct WmExpectColsArgs {
    WmExpectArgs a;                     // R = cols - 1; sket [S][nj][d'] complex, indexed by ketcol
    const int *kind, *ketcol;           // [C]
};

// LDS operations of one wavefront execute in order; the fences keep the compiler from moving them across the sync
__device__ __forceinline__ void wme_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// T_ij = conj(v_i) v_j det^-1/2 exp(ex), det = mant * 2^expo:  det^-1/2 exp(ex) = exp(ex - e ln2 / 2) / sqrt(mant); 2^e is real positive, so
// the principal branch of sqrt(det) is that of sqrt(mant).  Not inlined: inside the pair loop the constants of exp / sincos / sqrt
// would be hoisted into SGPRs held through the elimination.
__device__ __noinline__ cplx wme_pair_term(cplx ex, cplx mant, int expo, cplx vi, cplx vj) {
    const cplx ol = c_mul(c_inv(c_sqrt(mant)), c_exp(c_make(ex.x - 0.5 * (double)expo * 0.69314718055994530942, ex.y)));
    return c_mul(c_mul(c_conj(vi), vj), ol);
}

// exp(z) of a kind-2 column; not inlined for the reason given at wme_pair_term (inlined, the kernel took 179 VGPRs against 138)
__device__ __noinline__ cplx wme_col_exp(cplx z) { return c_exp(z); }

// The pair loop of both kernels.  COLS = false: the columns of sc_wm_pair_expect (column 0 of an operator linear with the per-ket
// border vector of its operator, the others squared); COLS = true: kind[col] and ketcol[col] of sc_wm_pair_expect_cols.
template <bool COLS>
__device__ __forceinline__ void wme_body(const WmExpectArgs &A, const int *kind, const int *ketcol, int stride, int region) {
    extern __shared__ double2 smem2[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, D = A.D, dp = A.dp;
    const int cols = 1 + A.R, nc = A.M * cols, nt = dp + 1 + nc;
    cplx *M = smem2 + (size_t)wave * region;
    cplx *w = M;
    double *dq = (double *)(M + D);
    const unsigned tiles_j = (unsigned)((A.n + 15) / 16);     // the host keeps the tile count below 2^31
    const int64_t i0 = (int64_t)(blockIdx.x / tiles_j) * 16, j0 = (int64_t)(blockIdx.x % tiles_j) * 16;
    cplx acc[2] = {c_make(0.0, 0.0), c_make(0.0, 0.0)};      // sum T F_a of the operators a = lane, lane + 64
    cplx accn = c_make(0.0, 0.0);                             // sum T
    for (int pr = wave; pr < 256; pr += nw) {
        const int64_t i = i0 + (pr >> 4), j = j0 + (pr & 15);
        if (i >= A.ni || j >= A.n) continue;
        const double *Qi = A.qp_i + i * 2 * D, *Qj = A.qp + j * 2 * D;
        const cplx *Cj = (const cplx *)A.cqq + j * (int64_t)D * D, *dj = (const cplx *)A.dvec + j * D;
        const cplx *Cpi = (const cplx *)A.cqqp_i + i * (int64_t)dp * dp, *Cpj = (const cplx *)A.cqqp + j * (int64_t)dp * dp;
        const cplx *dpi = (const cplx *)A.dvecp_i + i * dp, *dpj = (const cplx *)A.dvecp + j * dp;
        wme_lds_sync();                                       // the previous pair's last reads of the region are done
        for (int a = lane; a < D; a += 64) dq[a] = Qj[a] - Qi[a];
        wme_lds_sync();
        // w = C_j dQ (lane a: rows a, a + 64, ...) and this lane's share of -1/2 dQ^T C_j dQ - d_j . dQ
        cplx exl = c_make(0.0, 0.0);
        for (int a = lane; a < D; a += 64) {
            cplx s = c_make(0.0, 0.0);
            const cplx *row = Cj + (int64_t)a * D;
#pragma unroll 1
            for (int c = 0; c < D; ++c) { const double q = dq[c]; s.x = fma(row[c].x, q, s.x); s.y = fma(row[c].y, q, s.y); }
            w[a] = s;
            const double q = dq[a];
            exl.x = fma(q, -0.5 * s.x - dj[a].x, exl.x); exl.y = fma(q, -0.5 * s.y - dj[a].y, exl.y);
        }
        wme_lds_sync();
        // b'_r = (U^T w)_r + conj(d'_i)_r + (d'_j)_r for rows r = lane, lane + 64
        cplx bq[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = lane + 64 * h;
            cplx s = c_make(0.0, 0.0);
            if (r < dp) {
                s = c_make(dpi[r].x + dpj[r].x, -dpi[r].y + dpj[r].y);
#pragma unroll 1
                for (int a = 0; a < D; ++a) { const double u = A.U[a * dp + r]; s.x = fma(u, w[a].x, s.x); s.y = fma(u, w[a].y, s.y); }
            }
            bq[h] = s;
        }
        wme_lds_sync();                                       // w is overwritten by the matrix from here on
        for (int r = 0; r < dp; ++r)
            for (int l = lane; l < dp; l += 64)
                M[r * stride + l] = c_make(Cpi[r * dp + l].x + Cpj[r * dp + l].x, -Cpi[r * dp + l].y + Cpj[r * dp + l].y);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r = lane + 64 * h;
            if (r < dp) { M[r * stride + dp] = bq[h]; M[dp * stride + r] = bq[h]; }
        }
        for (int c = 0; c < nc; ++c) {                        // the border vectors, as columns and as rows
            int op = c / cols;
            bool perket = A.sket != nullptr && c == op * cols;
            if constexpr (COLS) { op = ketcol[c]; perket = op >= 0; }      // the slot of the column's per-ket vectors
            for (int r = lane; r < dp; r += 64) {
                cplx s = ((const cplx *)A.sfix)[(int64_t)c * dp + r];
                if (perket) s = c_add(s, ((const cplx *)A.sket)[((int64_t)op * A.n + j) * dp + r]);
                M[r * stride + dp + 1 + c] = s;
                M[(dp + 1 + c) * stride + r] = s;
            }
        }
        for (int e = lane; e < (nc + 1) * (nc + 1); e += 64) {
            const int r = e / (nc + 1), c = e - r * (nc + 1);
            M[(dp + r) * stride + dp + c] = c_make(0.0, 0.0);
        }
        wme_lds_sync();
        // g_col . b' of this lane's columns col = lane, lane + 64 (b' read back as a broadcast)
        cplx gb[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = lane + 64 * h;
            cplx s = c_make(0.0, 0.0);
            if (c < nc) {
                const cplx *gc = (const cplx *)A.g + (int64_t)c * dp;
#pragma unroll 1
                for (int r = 0; r < dp; ++r) s = c_fma(gc[r], M[r * stride + dp], s);
            }
            gb[h] = s;
        }
        cplx mant = c_make(1.0, 0.0);                         // det(D'/2pi) = mant * 2^expo
        int expo = 0;
        bool singular = false;
        for (int k = 0; k < dp; ++k) {
            // pivot among rows k..d'-1 (two candidates per lane)
            const int r0 = k + lane, r1 = k + lane + 64;
            const double m0 = r0 < dp ? c_abs2(M[r0 * stride + k]) : -1.0;
            const double m1 = r1 < dp ? c_abs2(M[r1 * stride + k]) : -1.0;
            const bool take1 = m1 > m0;
            const int piv = wave_pivot_row(take1 ? m1 : m0, take1 ? r1 : r0, r0 < dp);
            if (piv != k) {
                for (int l = k + lane; l < nt; l += 64) {
                    const cplx t = M[k * stride + l];
                    M[k * stride + l] = M[piv * stride + l];
                    M[piv * stride + l] = t;
                }
                mant = c_make(-mant.x, -mant.y);
                wme_lds_sync();
            }
            const cplx p = M[k * stride + k];
            if (p.x == 0.0 && p.y == 0.0) { singular = true; break; }
            mant = c_scale(c_mul(mant, p), 1.0 / (2.0 * 3.14159265358979323846));
            int e;
            frexp(fmax(fabs(mant.x), fabs(mant.y)), &e);
            mant = c_make(ldexp(mant.x, -e), ldexp(mant.y, -e));
            expo += e;
            const cplx ip = c_inv(p);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r = k + 1 + lane + 64 * h;          // rows k+1 .. nt-1 (nt <= 128)
                if (r < nt) {
                    const cplx f = c_mul(M[r * stride + k], ip);
                    const int lend = r <= dp ? nt : dp;       // a border row: the columns of D', then its own diagonal entry
#pragma unroll 1
                    for (int l = k + 1; l < lend; ++l) M[r * stride + l] = c_fnma(f, M[k * stride + l], M[r * stride + l]);
                    if (r > dp) M[r * stride + r] = c_fnma(f, M[k * stride + r], M[r * stride + r]);
                }
            }
            wme_lds_sync();
        }
        if (singular) continue;
        const cplx bib = M[dp * stride + dp];                 // -b'^T D'^-1 b'
        const cplx ex = c_make(wave_sum(exl.x) - 0.5 * bib.x, wave_sum(exl.y) - 0.5 * bib.y);
        const cplx T = wme_pair_term(ex, mant, expo, ((const cplx *)A.coef_i)[i], ((const cplx *)A.coef)[j]);
        cplx term[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = lane + 64 * h;
            term[h] = c_make(0.0, 0.0);
            if (c < nc) {
                const cplx sb = M[dp * stride + dp + 1 + c];                  // -b'^T D'^-1 s_c
                const cplx zi = ((const cplx *)A.za)[(int64_t)c * A.ni + i], zj = ((const cplx *)A.zb)[(int64_t)c * A.n + j];
                const cplx l = c_make(zi.x + zj.x + gb[h].x - sb.x, zi.y + zj.y + gb[h].y - sb.y);
                cplx f = l;
                if constexpr (COLS) {
                    const int kd = kind[c];
                    const cplx ss = M[(dp + 1 + c) * stride + dp + 1 + c];          // -s_c^T D'^-1 s_c
                    if (kd == 1) f = c_sub(c_mul(l, l), ss);
                    if (kd == 2) f = wme_col_exp(c_make(-l.x - 0.5 * ss.x, -l.y - 0.5 * ss.y));
                } else {
                    if (c % cols != 0) f = c_sub(c_mul(l, l), M[(dp + 1 + c) * stride + dp + 1 + c]);
                }
                term[h] = c_scale(f, A.lam[c]);
            }
        }
        wme_lds_sync();                                       // the corner has been read; row 0 of the region takes the terms
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int c = lane + 64 * h;
            if (c < nc) M[c] = term[h];
        }
        wme_lds_sync();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int a = lane + 64 * h;
            if (a < A.M) {
                cplx F = ((const cplx *)A.kap)[a];
#pragma unroll 1
                for (int c = 0; c < cols; ++c) F = c_add(F, M[a * cols + c]);
                acc[h] = c_fma(T, F, acc[h]);
            }
        }
        accn = c_add(accn, T);
    }
    // the tile's wavefronts, added in order: every wavefront leaves its sums at the head of its region
    wme_lds_sync();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int a = lane + 64 * h;
        if (a < A.M) M[a] = acc[h];
    }
    if (lane == 0) M[A.M] = accn;
    __syncthreads();
    for (int o = threadIdx.x; o <= A.M; o += blockDim.x) {
        cplx s = c_make(0.0, 0.0);
        for (int v = 0; v < nw; ++v) s = c_add(s, smem2[(size_t)v * region + o]);
        ((double2 *)A.partials)[(size_t)blockIdx.x * (A.M + 1) + o] = s;
    }
}

__global__ __launch_bounds__(256) void wm_expect_kernel(WmExpectArgs A, int stride, int region) {
    wme_body<false>(A, nullptr, nullptr, stride, region);
}

__global__ __launch_bounds__(256) void wm_expect_cols_kernel(WmExpectColsArgs A, int stride, int region) {
    wme_body<true>(A.a, A.kind, A.ketcol, stride, region);
}

// rows of the bordered matrix with C border columns, its odd row stride and the LDS region of one wavefront (complex elements)
int wme_stride(int nt) { return nt | 1; }
int wme_region(int D, int nt) {
    const int mat = nt * wme_stride(nt), vec = D + (D + 1) / 2;
    return mat > vec ? mat : vec;
}
bool wme_shape_ok(int D, int dp) { return D >= 1 && D <= WME_MAXD && dp >= 1 && dp <= WME_MAXDP && dp <= D; }
int wme_capacity(int D, int dp) {
    for (int c = WME_MAXROWS - dp - 1; c >= 1; --c)
        if ((size_t)wme_region(D, dp + 1 + c) * sizeof(cplx) <= WME_LDS) return c;
    return 0;
}

}  // namespace

extern "C" int64_t sc_wm_pair_expect_tiles(int64_t ni, int64_t nj) {
    if (ni <= 0 || nj <= 0) return 0;
    return ((ni + 15) / 16) * ((nj + 15) / 16);
}

extern "C" int32_t sc_wm_pair_expect_capacity(int32_t D, int32_t dprime) { return wme_shape_ok(D, dprime) ? wme_capacity(D, dprime) : 0; }

extern "C" int sc_wm_pair_expect(const double *qp_i, const double *coef_i, const double *cqqp_i, const double *dvecp_i, int64_t ni,
                                 const double *qp_j, const double *coef_j, const double *cqq_j, const double *dvec_j,
                                 const double *cqqp_j, const double *dvecp_j, int64_t nj, const double *U, int32_t D, int32_t dprime,
                                 const double *za, const double *zb, const double *g, const double *sfix, const double *sket,
                                 const double *lam, const double *kap, int32_t M, int32_t R, double *partials, double *out,
                                 void *stream) {
    if (!qp_i || !coef_i || !cqqp_i || !dvecp_i || !qp_j || !coef_j || !cqq_j || !dvec_j || !cqqp_j || !dvecp_j || !U || !za || !zb ||
        !g || !sfix || !lam || !kap || !partials || !out)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_wm_pair_expect: null argument");
    if (M < 1 || R < 0) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_wm_pair_expect: M=%d, R=%d", M, R);
    if (!wme_shape_ok(D, dprime))
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_wm_pair_expect: D=%d d'=%d outside 1 <= d' <= D, D <= %d, d' <= %d", D, dprime, WME_MAXD,
                       WME_MAXDP);
    if (M > 65535) return sc_fail(SC_ERR_UNSUPPORTED, "sc_wm_pair_expect: M=%d operators outside M <= 65535", M);
    const int cap = wme_capacity(D, dprime);
    if ((int64_t)M * (1 + (int64_t)R) > cap)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_wm_pair_expect: M (1 + R) = %lld columns, one launch holds at most %d at D=%d d'=%d",
                       (long long)M * (1 + (long long)R), cap, D, dprime);
    const int64_t tiles = sc_wm_pair_expect_tiles(ni, nj);
    if (tiles > 0x7fffffff)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_wm_pair_expect: %lld x %lld pairs need more than 2^31 tiles", (long long)ni, (long long)nj);
    hipStream_t s = (hipStream_t)stream;
    if (tiles > 0) {
        WmExpectArgs a{qp_i, coef_i, cqqp_i, dvecp_i, qp_j, coef_j, cqq_j, dvec_j, cqqp_j, dvecp_j, U, ni, nj, D, dprime,
                       za, zb, g, sfix, sket, lam, kap, M, R, partials};
        const int nt = dprime + 1 + M * (1 + R), stride = wme_stride(nt), region = wme_region(D, nt);
        const size_t per_wave = (size_t)region * sizeof(cplx);
        const int nw = (int)std::min<size_t>(4, WME_LDS / per_wave);
        const size_t bytes = per_wave * nw;
        if (hipFuncSetAttribute((const void *)wm_expect_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
            return sc_check_launch("sc_wm_pair_expect (LDS attribute)");
        hipLaunchKernelGGL(wm_expect_kernel, dim3((unsigned)tiles), dim3(64 * nw), bytes, s, a, stride, region);
        const int rc = sc_check_launch("sc_wm_pair_expect");
        if (rc != SC_OK) return rc;
    }
    hipLaunchKernelGGL(expect_reduce_kernel, dim3((unsigned)(M + 1)), dim3(256), 0, s, partials, tiles, M + 1, out);
    return sc_check_launch("sc_wm_pair_expect (reduction)");
}

// sc_wm_pair_expect with a kind and a slot of per-ket border vectors per column: kind 0  f = l,  kind 1
// f = l^2 + s^T D'^-1 s,  kind 2  f = exp(-l + 1/2 s^T D'^-1 s);  ketcol[col] = -1 or the slot p of  s_col = sfix[col] + sket[p][j].
// kind and ketcol are read back once and checked here, the kernel indexes sket with them unchecked.
extern "C" int sc_wm_pair_expect_cols(const double *qp_i, const double *coef_i, const double *cqqp_i, const double *dvecp_i, int64_t ni,
                                      const double *qp_j, const double *coef_j, const double *cqq_j, const double *dvec_j,
                                      const double *cqqp_j, const double *dvecp_j, int64_t nj, const double *U, int32_t D,
                                      int32_t dprime, const double *za, const double *zb, const double *g, const double *sfix,
                                      const double *sket, int32_t S, const int32_t *ketcol, const int32_t *kind, const double *lam,
                                      const double *kap, int32_t M, int32_t cols, double *partials, double *out, void *stream) {
    if (!qp_i || !coef_i || !cqqp_i || !dvecp_i || !qp_j || !coef_j || !cqq_j || !dvec_j || !cqqp_j || !dvecp_j || !U || !za || !zb ||
        !g || !sfix || !ketcol || !kind || !lam || !kap || !partials || !out || (!sket && S != 0))
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_wm_pair_expect_cols: null argument");
    if (M < 1 || cols < 1 || S < 0) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_wm_pair_expect_cols: M=%d, cols=%d, S=%d", M, cols, S);
    if (!wme_shape_ok(D, dprime))
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_wm_pair_expect_cols: D=%d d'=%d outside 1 <= d' <= D, D <= %d, d' <= %d", D, dprime,
                       WME_MAXD, WME_MAXDP);
    if (M > 65535) return sc_fail(SC_ERR_UNSUPPORTED, "sc_wm_pair_expect_cols: M=%d operators outside M <= 65535", M);
    const int cap = wme_capacity(D, dprime);
    if ((int64_t)M * cols > cap)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_wm_pair_expect_cols: M cols = %lld columns, one launch holds at most %d at D=%d d'=%d",
                       (long long)M * cols, cap, D, dprime);
    const int64_t tiles = sc_wm_pair_expect_tiles(ni, nj);
    if (tiles > 0x7fffffff)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_wm_pair_expect_cols: %lld x %lld pairs need more than 2^31 tiles", (long long)ni,
                       (long long)nj);
    hipStream_t s = (hipStream_t)stream;
    const int nc = M * cols;                                  // <= WME_MAXROWS
    int32_t meta[2 * WME_MAXROWS];
    if (hipMemcpyAsync(meta, kind, nc * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(meta + nc, ketcol, nc * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return sc_check_launch("sc_wm_pair_expect_cols (host copy of kind and ketcol)");
    for (int c = 0; c < nc; ++c) {
        if (meta[c] < 0 || meta[c] > 2) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_wm_pair_expect_cols: kind[%d]=%d outside 0 ... 2", c, meta[c]);
        if (meta[nc + c] < -1 || meta[nc + c] >= S)
            return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_wm_pair_expect_cols: ketcol[%d]=%d outside -1 ... S-1=%d", c, meta[nc + c], S - 1);
    }
    if (tiles > 0) {
        WmExpectColsArgs a{{qp_i, coef_i, cqqp_i, dvecp_i, qp_j, coef_j, cqq_j, dvec_j, cqqp_j, dvecp_j, U, ni, nj, D, dprime,
                            za, zb, g, sfix, sket, lam, kap, M, cols - 1, partials}, kind, ketcol};
        const int nt = dprime + 1 + nc, stride = wme_stride(nt), region = wme_region(D, nt);
        const size_t per_wave = (size_t)region * sizeof(cplx);
        const int nw = (int)std::min<size_t>(4, WME_LDS / per_wave);
        const size_t bytes = per_wave * nw;
        if (hipFuncSetAttribute((const void *)wm_expect_cols_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
            return sc_check_launch("sc_wm_pair_expect_cols (LDS attribute)");
        hipLaunchKernelGGL(wm_expect_cols_kernel, dim3((unsigned)tiles), dim3(64 * nw), bytes, s, a, stride, region);
        const int rc = sc_check_launch("sc_wm_pair_expect_cols");
        if (rc != SC_OK) return rc;
    }
    hipLaunchKernelGGL(expect_reduce_kernel, dim3((unsigned)(M + 1)), dim3(256), 0, s, partials, tiles, M + 1, out);
    return sc_check_launch("sc_wm_pair_expect_cols (reduction)");
}

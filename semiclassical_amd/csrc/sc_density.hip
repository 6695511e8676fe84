// Reduced (marginal) density of a frozen-Gaussian wavepacket along chosen directions u_d (not in the reference; DESIGN.md
// section 4.12) -- the O(n^2) kernel behind HermanKlukPropagator.reduced_density():
//
//   rho_d(s) = int |psi(x)|^2 delta(s - u_d.x) dx                      (s = grid value - origin of direction d)
//            = sum_ij wb_i wk_j (2 pi sigma_d^2)^-1/2 exp( E_ij + beta^2 h_d - (s - m)^2 h_d + i 2 h_d (s - m) beta ),
//
//   E_ij = rs_i + rs_j + X1_i.Y1_j + i (ib_i + ik_j + X2_i.Y2_j)      the pair exponent of sc_pair_sum_rect, same operands,
//   m = a_i + a_j,  beta = b_j - b_i,  h_d = 1 / (2 sigma_d^2),        a = u_d.q / 2,  b = u_d^T B p / hbar,  sigma_d^2 = u_d^T B u_d.
//
// The product of two Gaussians of one width is a Gaussian in x whose marginal along u is a Gaussian in s with the complex
// centre m + i beta; the whole term is the exponential of ONE exponent, whose real part is <= 0 (Cauchy-Schwarz).
//
// density_kernel: one workgroup of 256 threads owns a band of 64 bras, a share of the ket tiles (blockIdx.z) and up to 256 grid
// points of ONE direction (blockIdx.x), one point per thread.  Per 64 x 64 tile of pairs:
//   phase A  the pair exponents as in pair_sum_kernel (4 x 4 pairs per thread, K staged through LDS in chunks of 16);
//   phase B  in four rounds the threads put 1024 of the tile's pairs into LDS as (Re E + beta^2 h, Im E, m, 2 h beta, w) -- the
//            space of phase A's staging buffers -- and every thread walks over them (all lanes read the same pair: a broadcast)
//            with one c_exp per pair and point, accumulating into its own two registers.
// No cross-thread reduction and no atomics: the registers are stored once, into row (band, share) of partials[rows][M ns][2], and
// density_reduce_kernel adds the rows in order and applies (2 pi sigma^2)^-1/2 = sqrt(h / pi).  The order of every sum is a
// function of the shapes alone: the same bits in every run.  Pairs beyond ni, nj are never visited.  Nothing is skipped by
// magnitude.
//
// Limits: K1 <= 1024 and K2 <= 1536 (D <= 512 as sc_grid_sum), ni <= 64 * 65535, any M >= 1 and ns >= 1 with
// M * ceil(ns / 256) < 2^24: the kernel does not bound the points of a launch below that, the host never has to split M ns.
#include "sc_common.h"

namespace {

#define DT 64      // tile edge
#define DK 16      // K chunk
#define DP 256     // grid points per workgroup (one per thread)
#define DROUND (DT * DT / 4)   // pairs of one phase-B round

struct DensityArgs {
    const double *X1, *Y1, *X2, *Y2;    // [ni][K1], [nj][K1], [ni][K2], [nj][K2]
    int K1, K2;
    const double *rsi, *rsj, *ib, *ik;  // [ni], [nj], [ni], [nj] real
    const double *wb, *wk;              // [ni], [nj] complex
    int64_t ni, nj;
    const double *abra, *bbra;          // [M][ni]
    const double *aket, *bket;          // [M][nj]
    const double *h;                    // [M]  1 / (2 sigma^2)
    const double *s, *s0;               // [ns] grid, [M] origin of direction d: the point is s - s0[d]
    int M, ns, chunks;                  // chunks = ceil(ns / DP)
    int64_t jtiles, jper;               // ket tiles in all, ket tiles per share
    double *partials;                   // [bands * shares][M * ns][2]
};

__global__ __launch_bounds__(256) void density_kernel(DensityArgs A) {
    // phase A: xs[DK][DT + 1], ys[DK][DT + 1]; phase B: pr[DROUND][3] (double2) -- never live at the same time
    __shared__ double2 smem[DROUND * 3];
    __shared__ double bra[DT][6], ket[DT][6];      // rs, ib | ik, Re w, Im w, a, b of the tile's rows
    double (*xs)[DT + 1] = (double (*)[DT + 1])smem;
    double (*ys)[DT + 1] = xs + DK;
    double2 (*pr)[3] = (double2 (*)[3])smem;
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int dir = blockIdx.x / A.chunks, pt = (blockIdx.x - dir * A.chunks) * DP + tid;
    const bool active = pt < A.ns;
    const int64_t i0 = (int64_t)blockIdx.y * DT;
    const int64_t t0 = (int64_t)blockIdx.z * A.jper, t1 = min(t0 + A.jper, A.jtiles);
    const int iv = (int)min((int64_t)DT, A.ni - i0);           // valid bras of the band
    const double h = A.h[dir], sv = active ? A.s[pt] - A.s0[dir] : 0.0;
    if (tid < DT) {
        const bool in = tid < iv;
        const int64_t i = i0 + tid;
        bra[tid][0] = in ? A.rsi[i] : 0.0;
        bra[tid][1] = in ? A.ib[i] : 0.0;
        bra[tid][2] = in ? A.wb[2 * i] : 0.0;
        bra[tid][3] = in ? A.wb[2 * i + 1] : 0.0;
        bra[tid][4] = in ? A.abra[(size_t)dir * A.ni + i] : 0.0;
        bra[tid][5] = in ? A.bbra[(size_t)dir * A.ni + i] : 0.0;
    }
    double acc_re = 0.0, acc_im = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t j0 = t * DT;
        const int jv = (int)min((int64_t)DT, A.nj - j0);       // valid kets of the tile
        double re[4][4], im[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) { re[a][b] = 0.0; im[a][b] = 0.0; }
        for (int part = 0; part < 2; ++part) {
            const double *X = part ? A.X2 : A.X1, *Y = part ? A.Y2 : A.Y1;
            const int K = part ? A.K2 : A.K1;
            for (int k0 = 0; k0 < K; k0 += DK) {
                __syncthreads();                               // the last readers of xs, ys, pr and ket are done
                for (int e = tid; e < DK * DT; e += 256) {
                    const int r = e / DK, k = e - r * DK;      // row r of the tile, column k of the chunk
                    const bool kin = k0 + k < K;
                    xs[k][r] = (kin && r < iv) ? X[(i0 + r) * K + k0 + k] : 0.0;
                    ys[k][r] = (kin && r < jv) ? Y[(j0 + r) * K + k0 + k] : 0.0;
                }
                if (part == 0 && k0 == 0 && tid < DT) {
                    const bool in = tid < jv;
                    const int64_t j = j0 + tid;
                    ket[tid][0] = in ? A.rsj[j] : 0.0;
                    ket[tid][1] = in ? A.ik[j] : 0.0;
                    ket[tid][2] = in ? A.wk[2 * j] : 0.0;
                    ket[tid][3] = in ? A.wk[2 * j + 1] : 0.0;
                    ket[tid][4] = in ? A.aket[(size_t)dir * A.nj + j] : 0.0;
                    ket[tid][5] = in ? A.bket[(size_t)dir * A.nj + j] : 0.0;
                }
                __syncthreads();
#pragma unroll 8                                               // 16 puts the kernel over 256 VGPRs: one workgroup per CU
                for (int k = 0; k < DK; ++k) {
                    double xv[4], yv[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) { xv[a] = xs[k][4 * ti + a]; yv[a] = ys[k][4 * tj + a]; }
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {
                            if (part) im[a][b] = fma(xv[a], yv[b], im[a][b]);
                            else re[a][b] = fma(xv[a], yv[b], re[a][b]);
                        }
                }
            }
        }
        // phase B, round r: the pairs of the ket columns 4 c + r, c = 0 .. 15, at pr[c * DT + bra row]
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            __syncthreads();                                   // phase A, or the round before, has read its LDS
            const double *kj = ket[4 * tj + r];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const double *bi = bra[4 * ti + a];
                const double beta = kj[5] - bi[5];
                const cplx w = c_mul(c_make(bi[2], bi[3]), c_make(kj[2], kj[3]));
                double2 *o = pr[tj * DT + 4 * ti + a];
                o[0] = make_double2(fma(beta * beta, h, bi[0] + kj[0] + re[a][r]), bi[1] + kj[1] + im[a][r]);
                o[1] = make_double2(bi[4] + kj[4], 2.0 * h * beta);
                o[2] = w;
            }
            __syncthreads();
            if (active) {
                for (int c = 0; c < 16 && 4 * c + r < jv; ++c) {
                    double2 (*col)[3] = pr + c * DT;
#pragma unroll 2
                    for (int row = 0; row < iv; ++row) {
                        const double2 z = col[row][0], mb = col[row][1], w = col[row][2];
                        const double d = sv - mb.x;
                        const cplx e = c_exp(c_make(fma(-h * d, d, z.x), fma(d, mb.y, z.y)));
                        const cplx term = c_mul(w, e);
                        acc_re += term.x; acc_im += term.y;
                    }
                }
            }
        }
    }
    if (active) {
        const size_t rowi = (size_t)blockIdx.y * gridDim.z + blockIdx.z;
        const size_t at = (rowi * A.M + dir) * (size_t)A.ns + pt;
        A.partials[2 * at] = acc_re;
        A.partials[2 * at + 1] = acc_im;
    }
}

// out[d][p] = sqrt(h_d / pi) sum_rows partials[row][d][p], rows in order
__global__ __launch_bounds__(256) void density_reduce_kernel(const double *partials, int64_t rows, const double *h, int64_t ns,
                                                             int64_t total, double *out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;      // one complex output
    if (e >= total) return;
    double re = 0.0, im = 0.0;
    for (int64_t r = 0; r < rows; ++r) {
        const double2 v = ((const double2 *)partials)[r * total + e];
        re += v.x; im += v.y;
    }
    const double f = sqrt(h[e / ns] * (1.0 / 3.14159265358979323846));
    ((double2 *)out)[e] = make_double2(f * re, f * im);
}

// ket tiles per share and the number of shares: enough workgroups to fill the device when there are few bra bands
void density_split(int64_t ni, int64_t nj, int64_t &bands, int64_t &jtiles, int64_t &jper, int64_t &shares) {
    bands = (ni + DT - 1) / DT;
    jtiles = (nj + DT - 1) / DT;
    int64_t want = (1024 + bands - 1) / bands;
    if (want > jtiles) want = jtiles;
    if (want > 1024) want = 1024;
    if (want < 1) want = 1;
    jper = (jtiles + want - 1) / want;
    shares = (jtiles + jper - 1) / jper;                         // no share is empty
}

}  // namespace

extern "C" int64_t sc_density_pair_sum_rows(int64_t ni, int64_t nj) {
    if (ni <= 0 || nj <= 0) return 0;
    int64_t bands, jtiles, jper, shares;
    density_split(ni, nj, bands, jtiles, jper, shares);
    return bands * shares;
}

extern "C" int sc_density_pair_sum(const double *X1, const double *Y1, int32_t K1, const double *X2, const double *Y2, int32_t K2,
                                   const double *rs_i, const double *rs_j, const double *ib, const double *ik, const double *wb,
                                   const double *wk, int64_t ni, int64_t nj, const double *a_bra, const double *b_bra,
                                   const double *a_ket, const double *b_ket, const double *inv_two_sigma2, int32_t M,
                                   const double *s, const double *s_origin, int32_t ns, double *partials, double *rho,
                                   void *stream) {
    if (!X1 || !Y1 || !X2 || !Y2 || !rs_i || !rs_j || !ib || !ik || !wb || !wk || !a_bra || !b_bra || !a_ket || !b_ket ||
        !inv_two_sigma2 || !s || !s_origin || !partials || !rho)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_density_pair_sum: null argument");
    if (M < 1 || ns < 1 || K1 < 1 || K2 < 1 || ni < 0 || nj < 0)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_density_pair_sum: M=%d, ns=%d, K1=%d, K2=%d, ni=%lld, nj=%lld", M, ns, K1, K2,
                       (long long)ni, (long long)nj);
    if (K1 > 1024 || K2 > 1536)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_density_pair_sum: K1=%d, K2=%d outside K1 <= 1024, K2 <= 1536 (D <= 512)", K1, K2);
    const int64_t chunks = ((int64_t)ns + DP - 1) / DP, total = (int64_t)M * ns;
    if (chunks * M > 0xffffff)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_density_pair_sum: M=%d directions of ns=%d points need more than 2^24 - 1 chunks of %d",
                       M, ns, DP);
    hipStream_t st = (hipStream_t)stream;
    int64_t rows = 0;
    if (ni > 0 && nj > 0) {
        int64_t bands, jtiles, jper, shares;
        density_split(ni, nj, bands, jtiles, jper, shares);
        if (bands > 65535)
            return sc_fail(SC_ERR_UNSUPPORTED, "sc_density_pair_sum: ni=%lld bras outside ni <= %d", (long long)ni, DT * 65535);
        rows = bands * shares;
        DensityArgs a{X1, Y1, X2, Y2, K1, K2, rs_i, rs_j, ib, ik, wb, wk, ni, nj, a_bra, b_bra, a_ket, b_ket, inv_two_sigma2, s, s_origin,
                      M, ns, (int)chunks, jtiles, jper, partials};
        hipLaunchKernelGGL(density_kernel, dim3((unsigned)(chunks * M), (unsigned)bands, (unsigned)shares), dim3(256), 0, st, a);
        const int rc = sc_check_launch("sc_density_pair_sum");
        if (rc != SC_OK) return rc;
    }
    hipLaunchKernelGGL(density_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, partials, rows,
                       inv_two_sigma2, (int64_t)ns, total, rho);
    return sc_check_launch("sc_density_pair_sum (reduction)");
}

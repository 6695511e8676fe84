// Expectation values of quadratic operators in the frozen-Gaussian wavepacket (not in the reference) --
// the O(n^2) kernel behind HermanKlukPropagator.expectation():
//
//   out[a] = sum_ij T_ij F_a,ij   (a < M),      out[M] = sum_ij T_ij,
//   T_ij   = wb_i wk_j exp( rs_i + rs_j + X1_i.Y1_j + i (ib_i + ik_j + X2_i.Y2_j) )      the pair term of sc_pair_sum_rect, same operands,
//   F_a,ij = kap_a + sum_col lam_col z_col^(p_col),    z_col = za[col][i] + zb[col][j],
//
// with 1 + R columns per operator: column 0 to the first power (the linear part), columns 1 ... R squared (the eigenvectors of the
// quadratic parts; operators of lower rank carry columns of zeros with lam = 0).
//
// expect_kernel: one workgroup of 256 threads owns a 64 x 64 tile of pairs, 4 x 4 pairs per thread (the text: sc_expect_tile.h).
//   phase A  the pair exponents exactly as in pair_sum_kernel (K staged through LDS in chunks of 16), one c_exp per pair, T kept in
//            registers; pairs beyond ni, nj are never visited.
//   phase B  per operator: the columns of za, zb of the tile's 64 bras and 64 kets staged through LDS in chunks of 16 columns -- the
//            space of phase A's staging buffers --, every thread accumulates f = sum_col lam z^p of its 16 pairs, adds kap, forms
//            sum T f over its pairs, and block_sum adds the threads in fixed order: ONE store per operator and tile into
//            partials[tile][M + 1][2].
// expect_reduce_kernel adds the tiles: one workgroup per output, thread t takes the tiles t, t + 256, ... in order, then block_sum.
// No atomics, nothing skipped by magnitude; the order of every sum is a function of (ni, nj, M, R) alone: the same bits in every run.
//
// Limits: those of sc_pair_sum_rect (fewer than 2^31 tiles), 1 <= M <= 65535, 0 <= R <= 512, M (1 + R) < 2^24.
#include "sc_expect_tile.h"

extern "C" int64_t sc_pair_expect_tiles(int64_t ni, int64_t nj) {
    if (ni <= 0 || nj <= 0) return 0;
    return ((ni + ET - 1) / ET) * ((nj + ET - 1) / ET);
}

extern "C" int sc_pair_expect(const double *X1, const double *Y1, int32_t K1, const double *X2, const double *Y2, int32_t K2,
                              const double *rs_i, const double *rs_j, const double *ib, const double *ik, const double *wb,
                              const double *wk, int64_t ni, int64_t nj, const double *za, const double *zb, const double *lam,
                              const double *kap, int32_t M, int32_t R, double *partials, double *out, void *stream) {
    if (!X1 || !Y1 || !X2 || !Y2 || !rs_i || !rs_j || !ib || !ik || !wb || !wk || !za || !zb || !lam || !kap || !partials || !out)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_pair_expect: null argument");
    if (M < 1 || R < 0 || K1 < 0 || K2 < 0)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_pair_expect: M=%d, R=%d, K1=%d, K2=%d", M, R, K1, K2);
    if (M > 65535 || R > 512 || (int64_t)M * (1 + R) >= (1 << 24))
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_pair_expect: M=%d operators of R=%d squared columns outside M <= 65535, R <= 512, "
                                           "M (1 + R) < 2^24", M, R);
    const int64_t tiles = sc_pair_expect_tiles(ni, nj);
    if (tiles > 0x7fffffff)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_pair_expect: %lld x %lld pairs need more than 2^31 tiles", (long long)ni, (long long)nj);
    hipStream_t st = (hipStream_t)stream;
    if (tiles > 0) {
        ExpectArgs a{X1, Y1, X2, Y2, K1, K2, rs_i, rs_j, ib, ik, wb, wk, ni, nj, za, zb, lam, kap, M, R, partials};
        hipLaunchKernelGGL((expect_kernel<false, ExpectArgs>), dim3((unsigned)tiles), dim3(256), 0, st, a);
        const int rc = sc_check_launch("sc_pair_expect");
        if (rc != SC_OK) return rc;
    }
    hipLaunchKernelGGL(expect_reduce_kernel, dim3((unsigned)(M + 1)), dim3(256), 0, st, partials, tiles, M + 1, out);
    return sc_check_launch("sc_pair_expect (reduction)");
}

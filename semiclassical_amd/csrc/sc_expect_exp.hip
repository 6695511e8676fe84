// Expectation values of operators with exp(-a.x) terms in the frozen-Gaussian wavepacket (not in the reference; DESIGN.md section
// 4.23) -- the O(n^2) kernel behind HermanKlukPropagator.expectation(ex=...) and anharmonic_energy_expectation():
//
//   out[a] = sum_ij T_ij F_a,ij   (a < M),      out[M] = sum_ij T_ij,            T_ij the pair term of sc_pair_expect, same operands,
//   F_a,ij = kap_a + sum_col lam_col z_col^(p_col) + sum_{e < P} ea[a P + e][i] eb[a P + e][j]
//
// the 1 + R SUM columns of sc_pair_expect (z = za_i + zb_j, to the first or second power) and P PRODUCT columns per operator: the
// matrix element of exp(-a.x) between two Gaussians of one width factorises over the pair, so a column costs one complex product
// per pair and no exponential.  The caller has folded the weights into ea; operators with fewer terms carry columns of zeros.
//
// The kernel is expect_kernel<true, ExpectExpArgs> of sc_expect_tile.h: the tile, phase A and the sum columns of sc_pair_expect's
// instance, then the product columns of the operator staged through the same LDS buffers in chunks of 16 and accumulated into the
// same registers; one block_sum and ONE store per operator and tile.  expect_reduce_kernel adds the tiles in fixed order.  No
// atomics, nothing skipped by magnitude, pairs beyond ni, nj never visited; the order of every sum is a function of
// (ni, nj, M, R, P) alone.
//
// Limits: those of sc_pair_expect, 0 <= P <= 1024, M P < 2^24.
#include "sc_expect_tile.h"

namespace {

struct ExpectExpArgs : ExpectArgs {
    const double *ea, *eb;              // [M P][ni], [M P][nj] complex, trajectory index fastest
    int P;
};

}  // namespace

extern "C" int sc_pair_expect_exp(const double *X1, const double *Y1, int32_t K1, const double *X2, const double *Y2, int32_t K2,
                                  const double *rs_i, const double *rs_j, const double *ib, const double *ik, const double *wb,
                                  const double *wk, int64_t ni, int64_t nj, const double *za, const double *zb, const double *lam,
                                  const double *kap, int32_t M, int32_t R, const double *ea, const double *eb, int32_t P,
                                  double *partials, double *out, void *stream) {
    if (!X1 || !Y1 || !X2 || !Y2 || !rs_i || !rs_j || !ib || !ik || !wb || !wk || !za || !zb || !lam || !kap || !partials || !out)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_pair_expect_exp: null argument");
    if (M < 1 || R < 0 || P < 0 || K1 < 0 || K2 < 0)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_pair_expect_exp: M=%d, R=%d, P=%d, K1=%d, K2=%d", M, R, P, K1, K2);
    if (P > 0 && (!ea || !eb))
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_pair_expect_exp: null ea or eb with P=%d product columns", P);
    if (M > 65535 || R > 512 || (int64_t)M * (1 + R) >= (1 << 24) || P > 1024 || (int64_t)M * P >= (1 << 24))
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_pair_expect_exp: M=%d operators of R=%d squared and P=%d product columns outside "
                                           "M <= 65535, R <= 512, M (1 + R) < 2^24, P <= 1024, M P < 2^24", M, R, P);
    const int64_t tiles = sc_pair_expect_tiles(ni, nj);
    if (tiles > 0x7fffffff)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_pair_expect_exp: %lld x %lld pairs need more than 2^31 tiles", (long long)ni,
                       (long long)nj);
    hipStream_t st = (hipStream_t)stream;
    if (tiles > 0) {
        ExpectExpArgs a{{X1, Y1, X2, Y2, K1, K2, rs_i, rs_j, ib, ik, wb, wk, ni, nj, za, zb, lam, kap, M, R, partials}, ea, eb, P};
        hipLaunchKernelGGL((expect_kernel<true, ExpectExpArgs>), dim3((unsigned)tiles), dim3(256), 0, st, a);
        const int rc = sc_check_launch("sc_pair_expect_exp");
        if (rc != SC_OK) return rc;
    }
    hipLaunchKernelGGL(expect_reduce_kernel, dim3((unsigned)(M + 1)), dim3(256), 0, st, partials, tiles, M + 1, out);
    return sc_check_launch("sc_pair_expect_exp (reduction)");
}

// Per-trajectory symplecticity check of the monodromy matrix (the reference has no counterpart).
//
// For an exact flow M = d(q_t, p_t)/d(q_0, p_0) satisfies M^T J M = J.  With A = Mqq, B = Mqp, C = Mpq, D = Mpp the defect
// M^T J M - J has three independent blocks
//     E1 = A^T C - C^T A          (antisymmetric)
//     E2 = A^T D - C^T B - 1
//     E3 = B^T D - D^T B          (antisymmetric)
// which are made dimensionless in the scaled canonical coordinates q~_a = s_a q_a, p~_a = p_a / s_a:
//     E1~_ab = E1_ab / (s_a s_b),   E2~_ab = E2_ab s_b / s_a,   E3~_ab = E3_ab s_a s_b.
// The products are formed on the raw blocks, the scaling is an epilogue.  Per trajectory the kernels write
// dev[i][0..2] = max_ab |E1~|, |E2~|, |E3~|; a trajectory with a non-finite element in any of its four blocks (or in a result)
// gets +inf in all three -- explicitly, because fmax drops NaNs and a blown-up trajectory must not look healthy.
//
// Two kernels, both read-only on st->mono, without atomics and with a fixed order of operations (same bits in every run):
//   * D <= 16 (`symplectic_row16_kernel`): one trajectory per 16-lane row, four per wavefront; the four blocks (8 KB at most)
//     are copied to LDS once, lane j forms column j of the three defects row by row on the vector ALUs.
//   * D > 16 (`symplectic_mfma_kernel`): one 256-thread workgroup per trajectory at a time.  The 16 x 16 output tiles -- all of E2,
//     the tiles on and above the diagonal of E1 and E3 (|E_ab| = |E_ba| and the scale factors are symmetric) -- go round robin to
//     the four wavefronts; a tile is two chains of v_mfma_f64_16x16x4_f64 into ONE accumulator, X1^T Y1 + (-X2)^T Y2.
//     Operand layout (sc_gdml_large.hip, sc_dense_mono.hip): A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
//     accumulator register r = element (row (lane >> 4) + 4 r, column lane & 15).  The A operand of X^T Y is
//     A[i][k] = X[k0 + k][a0 + i]: both operands are 16 consecutive elements of a ROW of a block per 16-lane group, 128-byte
//     segments in the row-major order.  Operands come straight from global memory (a trajectory's blocks are 115 KB at D = 60 and
//     are re-read from cache); edges are zero-padded.  Either storage order of st->mono is read through sc_mono_offset.
#include "sc_common.h"

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int non_finite(double x) { return (__double2hiint(x) & 0x7ff00000) == 0x7ff00000; }

// LDS traffic of ONE wavefront executes in issue order: a compiler fence is all a write -> read hand-over between its lanes needs
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// maximum over the 16 lanes of a DPP row, result in every lane of the row (arguments are >= 0 and never NaN here)
__device__ __forceinline__ double row_max_f64(double v) {
    v = fmax(v, dpp_mov_f64<0x128>(v));      // row_ror:8
    v = fmax(v, dpp_mov_f64<0x124>(v));      // row_ror:4
    v = fmax(v, dpp_mov_f64<0x122>(v));      // row_ror:2
    v = fmax(v, dpp_mov_f64<0x121>(v));      // row_ror:1
    return v;
}
__device__ __forceinline__ double wave_max_f64(double v) {
    v = row_max_f64(v);
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const double r0 = __hiloint2double(__builtin_amdgcn_readlane(hi, 0), __builtin_amdgcn_readlane(lo, 0));
    const double r1 = __hiloint2double(__builtin_amdgcn_readlane(hi, 16), __builtin_amdgcn_readlane(lo, 16));
    const double r2 = __hiloint2double(__builtin_amdgcn_readlane(hi, 32), __builtin_amdgcn_readlane(lo, 32));
    const double r3 = __hiloint2double(__builtin_amdgcn_readlane(hi, 48), __builtin_amdgcn_readlane(lo, 48));
    return fmax(fmax(r0, r1), fmax(r2, r3));
}

// |E~_ab| of block blk (0: E1, 1: E2, 2: E3) from the raw element e: two roundings on top of e
__device__ __forceinline__ double scaled_abs(int blk, double e, double sa, double sb) {
    if (blk == 0) return fabs(e / (sa * sb));
    if (blk == 1) return fabs(e * sb / sa);
    return fabs(e * sa * sb);
}

#define SYMP_ROW16_GRID 2048      // workgroups of the D <= 16 kernel: four trajectories each per pass of the stride loop
#define SYMP_MFMA_GRID 2048       // workgroups of the D > 16 kernel: one trajectory each per pass

__global__ __launch_bounds__(64) void symplectic_row16_kernel(const double *mono, int64_t n, int D, const double *scale, double *dev) {
    extern __shared__ double2 smem2[];          // [4 trajectories][4][D][D]
    __shared__ double sg[16];
    const int DD = D * D, lane = threadIdx.x, row = lane >> 4, j = lane & 15;
    double *S = (double *)smem2 + (size_t)row * 4 * DD;
    if (lane < 16) sg[lane] = (lane < D && scale) ? scale[lane] : 1.0;
    wave_fence();
    const double sj = sg[j];
    const int64_t groups = (n + 3) >> 2;
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t tr = 4 * g + row;
        const bool live = tr < n;
        wave_fence();                            // the reads of the previous pass are done
        int bad = 0;
        if (live) {
            const double *M = mono + tr * 4 * (int64_t)DD;      // the two storage orders coincide for D <= 16
            for (int e = j; e < 4 * DD; e += 16) {
                const double v = M[e];
                S[e] = v;
                bad |= non_finite(v);
            }
        }
        wave_fence();
        double m1 = 0.0, m2 = 0.0, m3 = 0.0;
        if (live && j < D) {
            const double *Aj = S + j, *Bj = S + DD + j, *Cj = S + 2 * DD + j, *Dj = S + 3 * DD + j;
            for (int a = 0; a < D; ++a) {
                const double *Aa = S + a, *Ba = S + DD + a, *Ca = S + 2 * DD + a, *Da = S + 3 * DD + a;
                double e1 = 0.0, e2 = 0.0, e3 = 0.0;
                for (int k = 0; k < D; ++k) {
                    const int o = k * D;
                    const double aa = Aa[o], ba = Ba[o], ca = Ca[o], da = Da[o];
                    const double ab = Aj[o], bb = Bj[o], cb = Cj[o], db = Dj[o];
                    e1 = fma(aa, cb, e1); e1 = fma(-ca, ab, e1);
                    e2 = fma(aa, db, e2); e2 = fma(-ca, bb, e2);
                    e3 = fma(ba, db, e3); e3 = fma(-da, bb, e3);
                }
                if (a == j) e2 -= 1.0;
                const double sa = sg[a];
                const double v1 = scaled_abs(0, e1, sa, sj), v2 = scaled_abs(1, e2, sa, sj), v3 = scaled_abs(2, e3, sa, sj);
                bad |= non_finite(v1) | non_finite(v2) | non_finite(v3);
                m1 = fmax(m1, v1); m2 = fmax(m2, v2); m3 = fmax(m3, v3);
            }
        }
        // a non-finite value may have entered fmax: such lanes contribute 0 and the flag decides
        m1 = row_max_f64(bad ? 0.0 : m1); m2 = row_max_f64(bad ? 0.0 : m2); m3 = row_max_f64(bad ? 0.0 : m3);
        const unsigned long long flagged = __ballot(bad != 0);
        const bool row_bad = ((flagged >> (16 * row)) & 0xffffull) != 0ull;
        if (live && j == 0) {
            const double inf = __longlong_as_double(0x7ff0000000000000ll);
            double *out = dev + 3 * tr;
            out[0] = row_bad ? inf : m1; out[1] = row_bad ? inf : m2; out[2] = row_bad ? inf : m3;
        }
    }
}

#define SYMP_KU 4                  // k-slices (of four rows each) whose operands are loaded before their products are issued

template <int LAYOUT>
__global__ __launch_bounds__(256) void symplectic_mfma_kernel(const double *mono, int64_t n, int D, const double *scale, double *dev) {
    __shared__ double sg[512];
    __shared__ double red[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, rg = lane >> 4;
    const int64_t DD4 = 4 * (int64_t)D * D;
    const int NT = (D + 15) >> 4, nup = NT * (NT + 1) / 2, items = NT * NT + 2 * nup;
    for (int e = tid; e < 512; e += 256) sg[e] = (e < D && scale) ? scale[e] : 1.0;
    __syncthreads();
    for (int64_t tr = blockIdx.x; tr < n; tr += gridDim.x) {
        const double *M = mono + tr * DD4;
        double mx[3] = {0.0, 0.0, 0.0};
        int bad = 0;
        for (int item = wave; item < items; item += 4) {          // wave-uniform
            int blk, ta, tb;
            if (item < NT * NT) { blk = 1; ta = item / NT; tb = item - ta * NT; }
            else {
                int u = item - NT * NT;
                blk = u < nup ? 0 : 2;
                if (u >= nup) u -= nup;
                tb = 0;
                while ((tb + 1) * (tb + 2) / 2 <= u) ++tb;         // tile (ta, tb), ta <= tb, index tb (tb + 1) / 2 + ta
                ta = u - tb * (tb + 1) / 2;
            }
            // acc = X1^T Y1 - X2^T Y2 with (X1, Y1, X2, Y2) = E1: (A, C, C, A), E2: (A, D, C, B), E3: (B, D, D, B); planes A B C D = 0 1 2 3
            const int px1 = blk == 2 ? 1 : 0, py1 = blk == 0 ? 2 : 3, px2 = blk == 2 ? 3 : 2, py2 = blk == 0 ? 0 : 1;
            const int ca = 16 * ta + li, cb = 16 * tb + li;
            const bool oka = ca < D, okb = cb < D;
            d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < D; k0 += 4 * SYMP_KU) {
                double x1[SYMP_KU], x2[SYMP_KU], y1[SYMP_KU], y2[SYMP_KU];
#pragma unroll
                for (int u = 0; u < SYMP_KU; ++u) {
                    const int k = k0 + 4 * u + rg;
                    const bool in = k < D;
                    x1[u] = (in && oka) ? M[sc_mono_offset(LAYOUT, D, px1, k, ca)] : 0.0;
                    x2[u] = (in && oka) ? M[sc_mono_offset(LAYOUT, D, px2, k, ca)] : 0.0;
                    y1[u] = (in && okb) ? M[sc_mono_offset(LAYOUT, D, py1, k, cb)] : 0.0;
                    y2[u] = (in && okb) ? M[sc_mono_offset(LAYOUT, D, py2, k, cb)] : 0.0;
                }
                if (blk == 1) {                                   // the E2 tiles together touch every element of the four blocks
#pragma unroll
                    for (int u = 0; u < SYMP_KU; ++u) bad |= non_finite(x1[u]) | non_finite(x2[u]) | non_finite(y1[u]) | non_finite(y2[u]);
                }
#pragma unroll
                for (int u = 0; u < SYMP_KU; ++u) {
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[u], y1[u], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-x2[u], y2[u], acc, 0, 0, 0);
                }
            }
            if (okb) {
                const double sb = sg[cb];
                double m = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ra = 16 * ta + rg + 4 * r;
                    if (ra < D) {
                        double e = acc[r];
                        if (blk == 1 && ra == cb) e -= 1.0;
                        const double v = scaled_abs(blk, e, sg[ra], sb);
                        bad |= non_finite(v);
                        m = fmax(m, v);
                    }
                }
                if (blk == 0) mx[0] = fmax(mx[0], m); else if (blk == 1) mx[1] = fmax(mx[1], m); else mx[2] = fmax(mx[2], m);
            }
        }
        // a non-finite value may have entered fmax: such lanes contribute 0 and the flag decides
#pragma unroll
        for (int i = 0; i < 3; ++i) mx[i] = wave_max_f64(bad ? 0.0 : mx[i]);
        const bool wave_bad = __ballot(bad != 0) != 0ull;
        __syncthreads();                                           // `red` of the previous trajectory has been read
        if (lane == 0) {
            red[wave][0] = mx[0]; red[wave][1] = mx[1]; red[wave][2] = mx[2]; red[wave][3] = wave_bad ? 1.0 : 0.0;
        }
        __syncthreads();
        if (tid < 3) {
            const bool any_bad = (red[0][3] + red[1][3]) + (red[2][3] + red[3][3]) != 0.0;
            const double v = fmax(fmax(red[0][tid], red[1][tid]), fmax(red[2][tid], red[3][tid]));
            dev[3 * tr + tid] = any_bad ? __longlong_as_double(0x7ff0000000000000ll) : v;
        }
    }
}

}  // namespace

extern "C" int sc_symplectic_deviation(const sc_state *st, const double *scale, double *dev, void *stream) {
    if (!st || !st->mono || !dev) return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_symplectic_deviation: null argument");
    const int D = st->dim, layout = st->mono_layout;
    if (layout != SC_MONO_ROWMAJOR && layout != SC_MONO_TILED16)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "sc_symplectic_deviation: unknown monodromy layout %d", layout);
    if (D < 1 || D > 510) return sc_fail(SC_ERR_UNSUPPORTED, "sc_symplectic_deviation: D=%d outside 1..510", D);
    if (layout == SC_MONO_TILED16 && D > 64)
        return sc_fail(SC_ERR_UNSUPPORTED, "sc_symplectic_deviation: the tiled monodromy layout is defined for D <= 64, D=%d", D);
    if (st->n <= 0) return SC_OK;
    hipStream_t s = (hipStream_t)stream;
    if (D <= 16) {
        const int64_t groups = (st->n + 3) >> 2;
        const int grid = (int)(groups < SYMP_ROW16_GRID ? groups : SYMP_ROW16_GRID);
        const size_t lds = (size_t)16 * D * D * sizeof(double);                 // 32 KB at D = 16: no attribute needed
        hipLaunchKernelGGL(symplectic_row16_kernel, dim3(grid), dim3(64), lds, s, (const double *)st->mono, st->n, D, scale, dev);
        return sc_check_launch("sc_symplectic_deviation");
    }
    const int grid = (int)(st->n < SYMP_MFMA_GRID ? st->n : SYMP_MFMA_GRID);
    if (layout == SC_MONO_TILED16)
        hipLaunchKernelGGL(symplectic_mfma_kernel<SC_MONO_TILED16>, dim3(grid), dim3(256), 0, s, (const double *)st->mono, st->n, D, scale, dev);
    else
        hipLaunchKernelGGL(symplectic_mfma_kernel<SC_MONO_ROWMAJOR>, dim3(grid), dim3(256), 0, s, (const double *)st->mono, st->n, D, scale, dev);
    return sc_check_launch("sc_symplectic_deviation");
}

// sGDML force field beyond 48 atoms (49 <= N <= 170): the route of sc_gdml_eval / sc_gdml_stage for molecules whose
// Hessian accumulators, descriptor arrays and staged training rows no longer fit one workgroup (sc_gdml.hip holds N <= 48).
// The algebra is that of sc_gdml.hip's header comment; reference semiclassical/gdml_predictor.py:96-250.
//
// Three kernels per batch of geometries, with everything that crosses a kernel boundary in caller-owned scratch
// (sc_gdml_scratch_bytes: a fixed number of geometries per batch, so the size does not depend on n):
//   scalars  one workgroup per geometry, 512 threads.  Each thread holds a strided slice of the descriptor x_d and of the
//            Neumaier-compensated descriptor-space gradient g_x in registers; the training rows are read straight from
//            global memory (shared by every geometry: they stay in L2 / MALL).  Per chunk of four training points: block
//            reductions of d_m^2 and XA_m, the scalars e_m, f_m, w_m, the gradient terms in training-point order.
//            Writes V, S = sum_m e_m XA_m, e_m, w_m and g_x.
//   operands grid (atom blocks x training-point blocks, geometries).  Lane = atom a, wavefront = four training points:
//            XJ_m[a] = J^T (x - xs_m) and AJ_m[a] = J^T A_m as gathers over the N - 1 partners (coefficients
//            -x^3 (r_a - r_c) recomputed per partner), written as [M][3N] rows.  The first wavefront of the first
//            training-point block also forms grad = std J^T g_x and the diagonal atom blocks of the pair terms.
//   hessian  grid (64 x 64 super-tiles of the upper triangle, geometries), four wavefronts, each a 32 x 32 block of 2 x 2
//            accumulator tiles: [XJ ; -e AJ]^T [Z ; XJ] over all training points on v_mfma_f64_16x16x4_f64 with the
//            operands formed from the XJ / AJ rows as they are loaded, then the atom-pair terms element by element.
//            Each tile goes out in rows, its mirror in rows through a 16 x 17 LDS transpose; the matrix is exactly
//            symmetric (only elements row <= column are computed into the output).
// The stage variant puts sc_stage_point's kernel in front (stage positions of the batch into the scratch) and
// sc_stage_consume's behind (slopes of (q, p, S); energy partial sums over sc_dense_grid(n) rows).
#include "sc_common.h"
#include "sc_row16.h"

int sc_stage_point_range(const sc_state *st, const sc_dense_scratch *sc, double dt, int stage, double *r_out, int64_t t0,
                         int64_t t1, hipStream_t stream);                                    // sc_dense_mono.hip
int sc_stage_consume_range(const sc_state *st, const sc_dense_scratch *sc, const double *inv_mass, const double *V,
                           const double *grad, double dt, int stage, double *energy_partials, int64_t t0, int64_t t1,
                           int accumulate, hipStream_t stream);

namespace {

constexpr int BIG_MIN_ATOMS = 49, BIG_MAX_ATOMS = 170;
constexpr int P1_THREADS = 512, P1_CH = 4;                     // scalars kernel: threads, training points per block reduction
constexpr int FM_MP = 4, FM_MB = 4 * FM_MP;                    // operands kernel: points per wavefront, per workgroup
constexpr int64_t BIG_BATCH_MAX = 512, BIG_SCRATCH_BUDGET = (int64_t)256 << 20;

__device__ __forceinline__ int pair_index(int a, int b) {      // a != b; torch.tril_indices order (i > j)
    return a > b ? a * (a - 1) / 2 + b : b * (b - 1) / 2 + a;
}

// 1 / |r_k - r_l| exactly as the scalars kernel computes the descriptor (same operands, same order)
__device__ __forceinline__ double inv_dist(const double *pos, int a, int c, double *dist_out) {
    const int k = a > c ? a : c, l = a > c ? c : a;
    const double dx = pos[3 * k] - pos[3 * l], dy = pos[3 * k + 1] - pos[3 * l + 1], dz = pos[3 * k + 2] - pos[3 * l + 2];
    const double dist = sqrt(dx * dx + dy * dy + dz * dz);
    *dist_out = dist;
    return 1.0 / dist;
}

// scratch, arrays over the B geometries of a batch (doubles)
struct BigScratch {
    double *pos;    // [B][3N]   geometries of the batch
    double *V;      // [B]       E - origin
    double *S;      // [B]       sum_m e_m XA_m
    double *em;     // [B][M]
    double *wm;     // [B][M]    e_m XA_m q / d_m
    double *gx;     // [B][Dd]   descriptor-space gradient
    double *grad;   // [B][3N]
    double *dg;     // [B][N][9] diagonal atom blocks of the pair terms
    double *xj;     // [B][M][3N]
    double *aj;     // [B][M][3N]
};

inline int64_t big_per_geometry(int N, int M) {                // doubles
    const int64_t X = 3 * N, Dd = (int64_t)N * (N - 1) / 2;
    return X + 2 + 2 * (int64_t)M + Dd + X + 9 * N + 2 * (int64_t)M * X;
}

inline int64_t big_batch(int N, int M) {
    const int64_t b = BIG_SCRATCH_BUDGET / (8 * big_per_geometry(N, M));
    return b < 1 ? 1 : (b > BIG_BATCH_MAX ? BIG_BATCH_MAX : b);
}

BigScratch big_carve(double *base, int N, int M, int64_t B) {
    const int64_t X = 3 * N, Dd = (int64_t)N * (N - 1) / 2;
    BigScratch s;
    double *f = base;
    s.pos = f;  f += B * X;
    s.V = f;    f += B;
    s.S = f;    f += B;
    s.em = f;   f += B * M;
    s.wm = f;   f += B * M;
    s.gx = f;   f += B * Dd;
    s.grad = f; f += B * X;
    s.dg = f;   f += B * 9 * N;
    s.xj = f;   f += B * M * X;
    s.aj = f;
    return s;
}

// descriptor elements per thread of the scalars kernel (Dd <= 512 EPT).  Four instantiations: one per exact EPT kept a
// guard only on the last element but spilled VGPRs from EPT = 20 on (measured with tools/kernel_resources.py); these spill
// only SGPRs (into VGPR lanes, no scratch memory)
inline int big_ept(int Dd) {
    for (int e : {4, 8, 16, 29})
        if (Dd <= P1_THREADS * e) return e;
    return -1;
}

struct BigArgs {
    sc_gdml_model G;
    BigScratch S;
};

// ------------------------------------------------------------------ scalars: V, S, e_m, w_m, g_x of one geometry
template <int EPT>
__global__ __launch_bounds__(P1_THREADS) void gdml_big_scalars_kernel(BigArgs A) {
    __shared__ double pos[3 * BIG_MAX_ATOMS];
    __shared__ double red[(P1_THREADS / 64) * 2 * P1_CH];
    const sc_gdml_model &G = A.G;
    const int g = blockIdx.x, tid = threadIdx.x, N = G.n_atoms, X = 3 * N, Dd = G.n_desc, M = G.n_train;
    for (int i = tid; i < X; i += P1_THREADS) pos[i] = A.S.pos[(size_t)g * X + i];
    __syncthreads();
    double xo[EPT], gacc[EPT], gcomp[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int d = tid + P1_THREADS * j;
        double dist;
        xo[j] = d < Dd ? inv_dist(pos, G.pair_k[d], G.pair_l[d], &dist) : 0.0;
        gacc[j] = 0.0; gcomp[j] = 0.0;
    }
    const double q = G.q, iq2 = 1.0 / (q * q);
    double esum = 0.0, ssum = 0.0;
    for (int m0 = 0; m0 < M; m0 += P1_CH) {
        const int mc = min(P1_CH, M - m0);
        // (1) d_m^2 = |x - xs_m|^2 and XA_m = (x - xs_m) . A_m of the chunk's points (gdml_predictor.py:150-170)
        double v[2 * P1_CH];
#pragma unroll
        for (int i = 0; i < P1_CH; ++i) {
            double s2 = 0.0, sa = 0.0;
            if (i < mc) {
                const double *xs = G.xs_train + (size_t)(m0 + i) * Dd, *al = G.jx_alphas + (size_t)(m0 + i) * Dd;
#pragma unroll
                for (int j = 0; j < EPT; ++j) {
                    const int d = tid + P1_THREADS * j;
                    if (d < Dd) {
                        const double xd = xo[j] - xs[d];
                        s2 = fma(xd, xd, s2); sa = fma(xd, al[d], sa);
                    }
                }
            }
            v[2 * i] = s2; v[2 * i + 1] = sa;
        }
        block_sum<2 * P1_CH>(v, red);
        // (2) scalars of the chunk (every thread, from the same sums: the same values everywhere), as sc_gdml.hip
        double f[P1_CH], ea[P1_CH];
#pragma unroll
        for (int i = 0; i < P1_CH; ++i) {
            const double s2 = i < mc ? v[2 * i] : 1.0, sa = v[2 * i + 1];
            double rd = __builtin_amdgcn_rsq(s2);
            rd = fma(fma(-0.5 * s2 * rd, rd, 0.5), rd, rd);
            rd = fma(fma(-0.5 * s2 * rd, rd, 0.5), rd, rd);
            double dist = s2 * rd;
            dist = fma(fma(-dist, dist, s2), 0.5 * rd, dist);
            const double e = (1.0 / 3.0) * q * q * q * q * exp(-q * dist);
            f[i] = e * (1.0 + q * dist) * iq2;
            ea[i] = e * sa;
            if (i < mc) {
                esum += f[i] * sa; ssum += e * sa;
                if (tid == 0) { A.S.em[(size_t)g * M + m0 + i] = e; A.S.wm[(size_t)g * M + m0 + i] = e * sa * q * rd; }
            }
        }
        // (3) g_x[d] += f_m A_m[d] - e_m XA_m (x[d] - xs_m[d]), training points in order, Neumaier-compensated (the terms
        //     cancel by six to seven orders of magnitude: oracle/gdml_truth.py)
        for (int i = 0; i < mc; ++i) {
            const double *xs = G.xs_train + (size_t)(m0 + i) * Dd, *al = G.jx_alphas + (size_t)(m0 + i) * Dd;
#pragma unroll
            for (int j = 0; j < EPT; ++j) {
                const int d = tid + P1_THREADS * j;
                if (d < Dd) {
                    const double t = fma(f[i], al[d], -ea[i] * (xo[j] - xs[d]));
                    const double sn = gacc[j] + t, bb = sn - gacc[j];
                    gcomp[j] += (gacc[j] - (sn - bb)) + (t - bb);
                    gacc[j] = sn;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int d = tid + P1_THREADS * j;
        if (d < Dd) A.S.gx[(size_t)g * Dd + d] = gacc[j] + gcomp[j];
    }
    if (tid == 0) { A.S.V[g] = esum * G.std + G.c - G.origin; A.S.S[g] = ssum; }
}

// ------------------------------------------------------------------ operands: XJ_m, AJ_m rows; grad and diagonal blocks
__global__ __launch_bounds__(256) void gdml_big_operands_kernel(BigArgs A) {
    __shared__ double pos[3 * BIG_MAX_ATOMS];
    const sc_gdml_model &G = A.G;
    const int N = G.n_atoms, X = 3 * N, Dd = G.n_desc, M = G.n_train, g = blockIdx.y;
    const int nab = (N + 63) / 64, ab = blockIdx.x % nab, mb = blockIdx.x / nab;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, a = 64 * ab + lane;
    for (int i = threadIdx.x; i < X; i += blockDim.x) pos[i] = A.S.pos[(size_t)g * X + i];
    __syncthreads();
    if (a >= N) return;
    const int mf = mb * FM_MB + wave * FM_MP;                      // first training point of the wavefront (wave-uniform)
    const bool extras = mb == 0 && wave == 0;
    const double S = A.S.S[g];
    const double *gx = A.S.gx + (size_t)g * Dd;
    double base[3] = {0.0, 0.0, 0.0}, sx[FM_MP][3], sa[FM_MP][3];
    double g3[3] = {0.0, 0.0, 0.0}, h6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, tr3 = 0.0;
#pragma unroll
    for (int i = 0; i < FM_MP; ++i)
#pragma unroll
        for (int u = 0; u < 3; ++u) { sx[i][u] = 0.0; sa[i][u] = 0.0; }
    for (int c = 0; c < N; ++c) {
        if (c == a) continue;
        const int d = pair_index(a, c);
        double dist;
        const double x = inv_dist(pos, a, c, &dist), x3 = x * x * x;
        double cf[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            cf[u] = -x3 * (pos[3 * a + u] - pos[3 * c + u]);         // d x_(a,c) / d r_a[u]
            base[u] = fma(cf[u], x, base[u]);
        }
#pragma unroll
        for (int i = 0; i < FM_MP; ++i) {
            if (mf + i < M) {
                const double xv = G.xs_train[(size_t)(mf + i) * Dd + d], av = G.jx_alphas[(size_t)(mf + i) * Dd + d];
#pragma unroll
                for (int u = 0; u < 3; ++u) { sx[i][u] = fma(cf[u], xv, sx[i][u]); sa[i][u] = fma(cf[u], av, sa[i][u]); }
            }
        }
        if (extras) {
            // grad = J^T g_x; diagonal block sum_c coef coef^T (3 g r - S) - 1 sum_c g x^3 (sc_gdml.hip)
            const double gv = gx[d], t = fma(3.0 * gv, dist, -S);
            tr3 = fma(gv, x3, tr3);
#pragma unroll
            for (int u = 0; u < 3; ++u) g3[u] = fma(cf[u], gv, g3[u]);
            const double c0 = cf[0] * t, c1 = cf[1] * t, c2 = cf[2] * t;
            h6[0] = fma(c0, cf[0], h6[0]); h6[1] = fma(c0, cf[1], h6[1]); h6[2] = fma(c0, cf[2], h6[2]);
            h6[3] = fma(c1, cf[1], h6[3]); h6[4] = fma(c1, cf[2], h6[4]); h6[5] = fma(c2, cf[2], h6[5]);
        }
    }
#pragma unroll
    for (int i = 0; i < FM_MP; ++i) {
        if (mf + i < M) {
            const size_t row = ((size_t)g * M + mf + i) * X + 3 * a;
#pragma unroll
            for (int u = 0; u < 3; ++u) { A.S.xj[row + u] = base[u] - sx[i][u]; A.S.aj[row + u] = sa[i][u]; }
        }
    }
    if (extras) {
#pragma unroll
        for (int u = 0; u < 3; ++u) A.S.grad[(size_t)g * X + 3 * a + u] = g3[u] * G.std;
        double *dg = A.S.dg + ((size_t)g * N + a) * 9;
        dg[0] = h6[0] - tr3; dg[1] = h6[1]; dg[2] = h6[2];
        dg[3] = h6[1]; dg[4] = h6[3] - tr3; dg[5] = h6[4];
        dg[6] = h6[2]; dg[7] = h6[4]; dg[8] = h6[5] - tr3;
    }
}

// ------------------------------------------------------------------ hessian: rank-M sums on the matrix cores + pair terms
__global__ __launch_bounds__(256) void gdml_big_hessian_kernel(BigArgs A, double *hess, int64_t hstride, int64_t t0) {
    __shared__ double pos[3 * BIG_MAX_ATOMS];
    __shared__ double tbuf[4][16 * 17];
    typedef double d4 __attribute__((ext_vector_type(4)));
    const sc_gdml_model &G = A.G;
    const int N = G.n_atoms, X = 3 * N, Dd = G.n_desc, M = G.n_train, g = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rg = lane >> 4, li = lane & 15;
    int sc = 0;                                                     // super-tile (sr, sc), sr <= sc, index sc (sc + 1) / 2 + sr
    while ((sc + 1) * (sc + 2) / 2 <= (int)blockIdx.x) ++sc;
    const int sr = blockIdx.x - sc * (sc + 1) / 2, wr = wave >> 1, wc = wave & 1;
    for (int i = threadIdx.x; i < X; i += blockDim.x) pos[i] = A.S.pos[(size_t)g * X + i];
    __syncthreads();
    if (sr == sc && wr > wc) return;                                // below the diagonal: the mirror of wave (0, 1)
    const int row0 = 64 * sr + 32 * wr, col0 = 64 * sc + 32 * wc;
    if (row0 >= X || col0 >= X) return;
    const double *xj = A.S.xj + (size_t)g * M * X, *aj = A.S.aj + (size_t)g * M * X;
    const double *em = A.S.em + (size_t)g * M, *wm = A.S.wm + (size_t)g * M;
    d4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
    // operand layout of v_mfma_f64_16x16x4_f64: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]; k is the
    // training point.  Rows: P = XJ, Qn = -e AJ; columns: Z = w XJ - e AJ, P = XJ (rows beyond M / 3N are zero).
    for (int m0 = 0; m0 < M; m0 += 4) {
        const int m = m0 + rg;
        const bool in = m < M;
        const double e = in ? em[m] : 0.0, w = in ? wm[m] : 0.0;
        double pr[2], qr[2], pc[2], zc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = row0 + 16 * i + li, c = col0 + 16 * i + li;
            const bool okr = in && r < X, okc = in && c < X;
            const double xr = okr ? xj[(size_t)m * X + r] : 0.0, ar = okr ? aj[(size_t)m * X + r] : 0.0;
            const double xc = okc ? xj[(size_t)m * X + c] : 0.0, ac = okc ? aj[(size_t)m * X + c] : 0.0;
            pr[i] = xr; qr[i] = -e * ar;
            pc[i] = xc; zc[i] = fma(w, xc, -e * ac);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(pr[i], zc[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(qr[i], pc[j], acc[i][j], 0, 0, 0);
            }
    }
    // atom-pair terms, scale, store: element (xr, y) with xr <= y and its mirror (y, xr)
    const double S = A.S.S[g], std = G.std;
    const double *gx = A.S.gx + (size_t)g * Dd, *dgb = A.S.dg + (size_t)g * N * 9;
    double *H = hess + (size_t)(t0 + g) * hstride, *tb = tbuf[wave];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int R = row0 + 16 * i, C = col0 + 16 * j;
            if (R >= X || C >= X || R > C + 15) continue;              // wave-uniform: nothing of this tile goes out
            const int y = C + li, b = y / 3, v = y - 3 * b;
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const int row = rg + 4 * qq, xr = R + row, a = xr / 3, u = xr - 3 * a;
                double val = 0.0;
                if (xr < X && y < X && xr <= y) {
                    double fin;
                    if (a == b) fin = dgb[9 * a + 3 * u + v];
                    else {
                        double dist;
                        const double x = inv_dist(pos, a, b, &dist), gv = gx[pair_index(a, b)], x3 = x * x * x, x5 = x3 * x * x;
                        const double du = pos[3 * a + u] - pos[3 * b + u], dv = pos[3 * a + v] - pos[3 * b + v];
                        fin = S * (x3 * du) * (x3 * dv) - (3.0 * gv * x5 * du * dv - (u == v ? gv * x3 : 0.0));
                    }
                    val = (acc[i][j][qq] + fin) * std;
                    // written once, read by the monodromy kernel after the stage: non-temporal (the training set stays in L2)
                    __builtin_nontemporal_store(val, &H[(size_t)xr * X + y]);
                }
                tb[row * 17 + li] = val;
            }
            wave_lds_fence();
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                // mirror element (C + row, R + li) = tile value (R + li, C + row)
                const int row = rg + 4 * qq, yy = C + row, xx = R + li;
                const double val = tb[li * 17 + row];
                if (yy < X && xx < X && xx < yy) __builtin_nontemporal_store(val, &H[(size_t)yy * X + xx]);
            }
            wave_lds_fence();
        }
}

// the three kernels on geometries [t0, t0 + nb) of the batch whose positions are in S.pos
int big_launch(const BigArgs &a, int64_t nb, double *hess, int64_t hstride, int64_t t0, hipStream_t s) {
    const sc_gdml_model &G = a.G;
    switch (big_ept(G.n_desc)) {
        case 4: hipLaunchKernelGGL(gdml_big_scalars_kernel<4>, dim3((unsigned)nb), dim3(P1_THREADS), 0, s, a); break;
        case 8: hipLaunchKernelGGL(gdml_big_scalars_kernel<8>, dim3((unsigned)nb), dim3(P1_THREADS), 0, s, a); break;
        case 16: hipLaunchKernelGGL(gdml_big_scalars_kernel<16>, dim3((unsigned)nb), dim3(P1_THREADS), 0, s, a); break;
        case 29: hipLaunchKernelGGL(gdml_big_scalars_kernel<29>, dim3((unsigned)nb), dim3(P1_THREADS), 0, s, a); break;
        default: return sc_fail(SC_ERR_UNSUPPORTED, "sGDML: no scalars kernel for %d descriptors", G.n_desc);
    }
    const int nab = (G.n_atoms + 63) / 64, nmb = (G.n_train + FM_MB - 1) / FM_MB;
    hipLaunchKernelGGL(gdml_big_operands_kernel, dim3((unsigned)(nab * nmb), (unsigned)nb), dim3(256), 0, s, a);
    const int st = (3 * G.n_atoms + 63) / 64;
    hipLaunchKernelGGL(gdml_big_hessian_kernel, dim3((unsigned)(st * (st + 1) / 2), (unsigned)nb), dim3(256), 0, s, a, hess,
                       hstride, t0);
    return sc_check_launch("sGDML (49-170 atoms)");
}

}  // namespace

extern "C" int sc_gdml_max_atoms(void) { return BIG_MAX_ATOMS; }

extern "C" int64_t sc_gdml_scratch_bytes(int32_t n_atoms, int32_t n_train) {
    if (n_atoms < BIG_MIN_ATOMS) return 0;
    if (n_atoms > BIG_MAX_ATOMS || n_train < 1) return -1;
    return 8 * big_batch(n_atoms, n_train) * big_per_geometry(n_atoms, n_train);
}

// checks of the route beyond 48 atoms (before any launch and before the n <= 0 return)
int sc_gdml_large_check(const sc_gdml_model *g, const double *scratch, const char *who) {
    if (g->n_atoms > BIG_MAX_ATOMS)
        return sc_fail(SC_ERR_UNSUPPORTED, "%s: %d atoms; the sGDML kernels hold at most %d atoms (3N <= 510)", who, g->n_atoms,
                       BIG_MAX_ATOMS);
    if (g->n_train < 1) return sc_fail(SC_ERR_BAD_ARGUMENT, "%s: no training points", who);
    if (big_ept(g->n_desc) < 0) return sc_fail(SC_ERR_UNSUPPORTED, "%s: %d descriptors", who, g->n_desc);
    if (!scratch)
        return sc_fail(SC_ERR_BAD_ARGUMENT, "%s: %d atoms need a scratch of sc_gdml_scratch_bytes(%d, %d) = %lld bytes", who,
                       g->n_atoms, g->n_atoms, g->n_train, (long long)sc_gdml_scratch_bytes(g->n_atoms, g->n_train));
    return SC_OK;
}

int sc_gdml_large_eval(const sc_gdml_model *g, double *scratch, const double *r, int64_t n, double *energy, double *grad, double *hess,
                       hipStream_t s) {
    const int N = g->n_atoms, X = 3 * N, M = g->n_train;
    const int64_t B = big_batch(N, M);
    const BigArgs a{*g, big_carve(scratch, N, M, B)};
    for (int64_t t0 = 0; t0 < n; t0 += B) {
        const int64_t nb = n - t0 < B ? n - t0 : B;
        if (hipMemcpyAsync(a.S.pos, r + t0 * X, nb * X * 8, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return sc_check_launch("sc_gdml_eval (positions)");
        const int rc = big_launch(a, nb, hess, (int64_t)X * X, t0, s);
        if (rc) return rc;
        if (hipMemcpyAsync(energy + t0, a.S.V, nb * 8, hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipMemcpyAsync(grad + t0 * X, a.S.grad, nb * X * 8, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return sc_check_launch("sc_gdml_eval (results)");
    }
    return sc_check_launch("sc_gdml_eval");
}

int sc_gdml_large_stage(const sc_gdml_model *g, double *scratch, const sc_state *st, const sc_dense_scratch *sc, double dt, int stage,
                        double *energy_partials, hipStream_t s) {
    const int N = g->n_atoms, D = 3 * N, M = g->n_train;
    const int64_t B = big_batch(N, M), n = st->n;
    const BigArgs a{*g, big_carve(scratch, N, M, B)};
    for (int64_t t0 = 0; t0 < n; t0 += B) {
        const int64_t t1 = n - t0 < B ? n : t0 + B;
        int rc = sc_stage_point_range(st, sc, dt, stage, a.S.pos, t0, t1, s);
        if (!rc) rc = big_launch(a, t1 - t0, sc->hess + (size_t)stage * D * D, (int64_t)4 * D * D, t0, s);
        if (!rc) rc = sc_stage_consume_range(st, sc, g->inv_mass, a.S.V, a.S.grad, dt, stage, energy_partials, t0, t1, t0 > 0, s);
        if (rc) return rc;
    }
    return sc_check_launch("sc_gdml_stage");
}

// The 64 x 64 tile of the expectation kernels (DESIGN.md sections 4.21, 4.23): ONE definition of phase A (the pair terms T), of the
// staged column loop and of the per-operator finish, as a kernel template with two instances: expect_kernel<false, ExpectArgs>
// (csrc/sc_expect.hip: sum columns only) and expect_kernel<true, ExpectExpArgs> (csrc/sc_expect_exp.hip: sum columns, then product
// columns; Args adds ea, eb, P).  PRODUCTS is a compile-time switch: the instance without it holds no trace of the product columns.
// A kernel template, not a device function called by two kernels: the body sits in the kernel itself, so adding the second
// instance left the device code of the first as it was, instruction for instruction (as an inlined function it kept the registers
// but came out with another schedule).
#pragma once
#include "sc_common.h"

namespace {

#define ET 64      // tile edge
#define EK 16      // K chunk of phase A
#define EC 16      // column chunk of phase B

struct ExpectArgs {
    const double *X1, *Y1, *X2, *Y2;    // [ni][K1], [nj][K1], [ni][K2], [nj][K2]
    int K1, K2;
    const double *rsi, *rsj, *ib, *ik;  // [ni], [nj], [ni], [nj] real
    const double *wb, *wk;              // [ni], [nj] complex
    int64_t ni, nj;
    const double *za, *zb;              // [M (1 + R)][ni], [M (1 + R)][nj] complex, trajectory index fastest
    const double *lam;                  // [M (1 + R)]
    const double *kap;                  // [M] complex
    int M, R;
    double *partials;                   // [tiles][M + 1][2]
};

// One workgroup of 256 threads, one tile: partials[tile][a] = sum over the tile's pairs of T_ij F_a,ij (a < M) and [M] = sum T_ij,
//   F_a,ij = kap_a + sum_col lam_col z_col^p  (+ sum_{e < P} ea[a P + e][i] eb[a P + e][j]  with PRODUCTS).
// ea [M P][ni], eb [M P][nj] complex, trajectory index fastest; the product columns pass through the staging buffers of the sum
// columns in chunks of EC and land in the same accumulators.
template <bool PRODUCTS, class Args>
__global__ __launch_bounds__(256) void expect_kernel(Args A) {
    // phase A: xs[EK][ET + 1], ys[EK][ET + 1] (doubles); phase B: zas[EC][ET], zbs[EC][ET] (complex) -- never live at the same time
    __shared__ double2 smem[2 * EC * ET];
    __shared__ double red[32];
    double (*xs)[ET + 1] = (double (*)[ET + 1])smem;
    double (*ys)[ET + 1] = xs + EK;
    cplx (*zas)[ET] = (cplx (*)[ET])smem;
    cplx (*zbs)[ET] = zas + EC;
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    const int64_t tiles = (A.nj + ET - 1) / ET;
    const int64_t bi = blockIdx.x / tiles, bj = blockIdx.x % tiles;
    const int64_t i0 = bi * ET, j0 = bj * ET;
    const int iv = (int)min((int64_t)ET, A.ni - i0), jv = (int)min((int64_t)ET, A.nj - j0);     // valid bras, kets of the tile
    double re[4][4], im[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) { re[a][b] = 0.0; im[a][b] = 0.0; }
    for (int part = 0; part < 2; ++part) {
        const double *X = part ? A.X2 : A.X1, *Y = part ? A.Y2 : A.Y1;
        const int K = part ? A.K2 : A.K1;
        for (int k0 = 0; k0 < K; k0 += EK) {
            __syncthreads();
            for (int e = tid; e < EK * ET; e += 256) {
                const int r = e / EK, k = e - r * EK;            // row r of the tile, column k of the chunk
                const bool kin = k0 + k < K;
                xs[k][r] = (kin && r < iv) ? X[(i0 + r) * K + k0 + k] : 0.0;
                ys[k][r] = (kin && r < jv) ? Y[(j0 + r) * K + k0 + k] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < EK; ++k) {
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
    // T of the thread's pairs, in the registers of the exponents; zero where the pair does not exist
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const bool iin = 4 * ti + a < iv;
        const int64_t i = i0 + 4 * ti + a;
        const cplx wb = iin ? ((const cplx *)A.wb)[i] : c_make(0.0, 0.0);
        const double rsi = iin ? A.rsi[i] : 0.0, ibi = iin ? A.ib[i] : 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t j = j0 + 4 * tj + b;
            cplx t = c_make(0.0, 0.0);
            if (iin && 4 * tj + b < jv) {
                const cplx e = c_exp(c_make(rsi + A.rsj[j] + re[a][b], ibi + A.ik[j] + im[a][b]));
                t = c_mul(c_mul(wb, ((const cplx *)A.wk)[j]), e);
                acc[0] += t.x; acc[1] += t.y;
            }
            re[a][b] = t.x; im[a][b] = t.y;
        }
    }
    const int outs = A.M + 1;
    double *mine = A.partials + (size_t)blockIdx.x * outs * 2;
    block_sum<2>(acc, red);
    if (tid == 0) { mine[2 * A.M] = acc[0]; mine[2 * A.M + 1] = acc[1]; }
    const int cols = 1 + A.R;
    for (int op = 0; op < A.M; ++op) {
        const int64_t cbase = (int64_t)op * cols;
        double fr[4][4], fi[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) { fr[a][b] = 0.0; fi[a][b] = 0.0; }
        for (int c0 = 0; c0 < cols; c0 += EC) {
            const int nc = min(EC, cols - c0);
            __syncthreads();                                     // the last readers of the staging buffers are done
            for (int e = tid; e < nc * ET; e += 256) {
                const int k = e >> 6, r = e & (ET - 1);          // column k of the chunk, row r of the tile: coalesced
                const int64_t col = cbase + c0 + k;
                zas[k][r] = r < iv ? ((const cplx *)A.za)[col * A.ni + i0 + r] : c_make(0.0, 0.0);
                zbs[k][r] = r < jv ? ((const cplx *)A.zb)[col * A.nj + j0 + r] : c_make(0.0, 0.0);
            }
            __syncthreads();
            for (int k = 0; k < nc; ++k) {
                const double l = A.lam[cbase + c0 + k];
                const bool linear = c0 + k == 0;                 // column 0 of the operator: first power
                cplx av[4], bv[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) { av[a] = zas[k][4 * ti + a]; bv[a] = zbs[k][4 * tj + a]; }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const cplx z = c_add(av[a], bv[b]);
                        const cplx zp = linear ? z : c_mul(z, z);
                        fr[a][b] = fma(l, zp.x, fr[a][b]);
                        fi[a][b] = fma(l, zp.y, fi[a][b]);
                    }
            }
        }
        if constexpr (PRODUCTS) {
            const int64_t ebase = (int64_t)op * A.P;
            for (int e0 = 0; e0 < A.P; e0 += EC) {
                const int nc = min(EC, A.P - e0);
                __syncthreads();
                for (int e = tid; e < nc * ET; e += 256) {
                    const int k = e >> 6, r = e & (ET - 1);
                    const int64_t col = ebase + e0 + k;
                    zas[k][r] = r < iv ? ((const cplx *)A.ea)[col * A.ni + i0 + r] : c_make(0.0, 0.0);
                    zbs[k][r] = r < jv ? ((const cplx *)A.eb)[col * A.nj + j0 + r] : c_make(0.0, 0.0);
                }
                __syncthreads();
                for (int k = 0; k < nc; ++k) {
                    cplx av[4], bv[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) { av[a] = zas[k][4 * ti + a]; bv[a] = zbs[k][4 * tj + a]; }
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) {            // f += ea_i eb_j: four FMAs in a fixed order
                            fr[a][b] = fma(av[a].x, bv[b].x, fr[a][b]);
                            fr[a][b] = fma(-av[a].y, bv[b].y, fr[a][b]);
                            fi[a][b] = fma(av[a].x, bv[b].y, fi[a][b]);
                            fi[a][b] = fma(av[a].y, bv[b].x, fi[a][b]);
                        }
                }
            }
        }
        const cplx kap = ((const cplx *)A.kap)[op];
        acc[0] = 0.0; acc[1] = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            if (4 * ti + a >= iv) continue;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (4 * tj + b >= jv) continue;
                const cplx t = c_mul(c_make(re[a][b], im[a][b]), c_make(fr[a][b] + kap.x, fi[a][b] + kap.y));
                acc[0] += t.x; acc[1] += t.y;
            }
        }
        block_sum<2>(acc, red);
        if (tid == 0) { mine[2 * op] = acc[0]; mine[2 * op + 1] = acc[1]; }
    }
}

// out[o] = sum_tiles partials[tile][o]: thread t adds the tiles t, t + 256, ... in order, block_sum adds the threads
__global__ __launch_bounds__(256) void expect_reduce_kernel(const double *partials, int64_t tiles, int outs, double *out) {
    __shared__ double red[32];
    const int o = blockIdx.x;
    double acc[2] = {0.0, 0.0};
    for (int64_t t = threadIdx.x; t < tiles; t += 256) {
        const double2 v = ((const double2 *)partials)[t * outs + o];
        acc[0] += v.x; acc[1] += v.y;
    }
    block_sum<2>(acc, red);
    if (threadIdx.x == 0) ((double2 *)out)[o] = make_double2(acc[0], acc[1]);
}

}  // namespace

// Fast path of the fused Herman-Kluk step for SEPARABLE potentials (diagonal Hessian) with DIAGONAL width
// matrices and D <= 64 -- the anharmonic adiabatic-shift configurations of BASELINE.json.
//
// One 256-thread workgroup per trajectory; 1024 persistent workgroups draw trajectories from a device-side cursor.
// Threads form a 16 x 16 grid; thread (trow, tj) owns the elements (a, b) = (16*ra + trow, 16*rb + tj), ra, rb < NR =
// ceil(D/16), of all four monodromy blocks and of the complex prefactor matrix.  Wave w holds the rows trow = 4w .. 4w+3
// of every 16-row slot (contiguous memory in the tiled storage order: a wave instruction covers 512 bytes), while the
// pivot ORDER inside a slot interleaves the waves (consecutive pivots sit in DIFFERENT waves, which is what lets the
// elimination run as a pipeline).  The whole 4*D*D*8-byte state of the trajectory is read once and written once.
//
//   modes    (hk_modes_kernel, one wavefront per trajectory, lane = mode) RK4 of (q_a, p_a); S and <T+V> by wave
//            reductions.  With a diagonal Hessian the monodromy elements (Mqq,Mpq)_ab and (Mqp,Mpp)_ab obey, for
//            every b, the same linear 2x2 system with the stage Hessians h_s[a]; its RK4 step is the 2x2 matrix
//            P_a, obtained by pushing the unit vectors through the reference's stage formula.  P_a -> st.work.
//                                                               (propagators.py:86-119, 313-383; potentials.py)
//   phase B  every (a,b): (Mqq,Mpq)' = P_a (Mqq,Mpq), (Mqp,Mpp)' = P_a (Mqp,Mpp), store back, and form
//            mat_ab = 1/2[ st_a/si_b Mqq + si_b/st_a Mpp - i hbar st_a si_b Mqp + i/hbar Mpq/(st_a si_b) ]
//            in registers.  Raw buffer instructions: scalar tile / plane offset + ONE per-thread 32-bit offset;
//            threads outside the matrix are cut off by the resource's range check (no branches).
//                                                                            (propagators.py:969-986)
//   phase C  c2 = det(mat) by Gaussian elimination with the matrix held in REGISTERS (NR*NR complex per
//            thread).  Rows are eliminated in a fixed order; the pivot COLUMN of a row is chosen by magnitude
//            among the live columns of the diagonal 16-column block (threshold pivoting: the 16 consecutive
//            lanes that own the row search it with integer keys and DPP rotations).  Because pivots stay inside
//            the diagonal block, finished row AND column blocks drop out statically.  The owner scales the row
//            by 1/pivot and publishes it through LDS; the pivot-column entries a thread needs sit in its own
//            16-lane group and are fetched with DPP row_newbcast.  The four waves are NOT barrier-coupled:
//            consumers poll a tag in the pivot record (see eliminate_block); one barrier in front of the first
//            block and one behind the last.  The last pivot step of a full block updates only the trailing slots
//            (PEEL of eliminate_block, sc_hk_lu.h).  Pivot products (with the signs of the column choices) accumulate in
//            LDS per row group; thread 0 multiplies them while the others stream the next trajectory.
//            If the best in-block pivot is more than 16x smaller than the largest live entry of the row, the
//            trajectory is flagged (sc_state.flags) and its determinant is recomputed by the fully pivoted
//            LDS elimination of sc_hk_step.hip in the same stream (never observed for HK matrices so far; the
//            path is exercised by tests/test_hk_gpu.py::test_weak_pivot_fallback).
//            Then the sqrt branch tracker.                   (torch.det, propagators.py:999, 1006-1052)
#include <algorithm>
#include "sc_common.h"
#include "sc_hk_lu.h"
#include "sc_row16.h"

// test aids of variant libraries (tools/phase_timing.py, the fix-up tests), not schedules
#ifndef SC_SD_ABLATE_LU
#define SC_SD_ABLATE_LU 0  // 1: variant library without the elimination (streaming phase alone)
#endif
#ifndef SC_SD_FORCE_FIXUP
#define SC_SD_FORCE_FIXUP 0
#endif

namespace {

typedef unsigned int sc_v2u __attribute__((ext_vector_type(2)));
typedef unsigned int sc_v4u __attribute__((ext_vector_type(4)));

// cache-policy bits of the block loads / stores (gfx942+: 1 = sc0, 2 = nt, 16 = sc1).  The blocks are touched once per step
// and the state (11.5 GB) is far beyond every cache: non-temporal on BOTH sides is worth 2.6 % (4.69 -> 4.56 ms; loads
// alone: nothing, stores alone: -0.5 %, scope bits: nothing).  TILED layout only: there a wave instruction covers 512
// contiguous bytes; on the 128-byte row segments of the row-major order (unaligned at D = 60) the same hint costs 45 %
// (4.9 -> 7.2 ms), as it does on the 8-byte-per-lane row accesses of the small-D kernels
constexpr int AUX_NT = 2;        // non-temporal: the load of a one-step item, the first load of a visit whose intermediate sub-steps store
                                 // their blocks, the last store of every item or visit
constexpr int AUX_PLAIN = 0;     // stores of an intermediate sub-step (where there are any) and loads of every later sub-step; the first
                                 // load of a visit whose intermediate sub-steps store nothing: the later sub-steps read the SAME lines again,
                                 // so it has to allocate in the L2 / memory-side cache (non-temporal: the re-read comes from HBM)
constexpr int NOSTORE_MIN_NR = 3;   // multi-step visits: smallest NR whose intermediate sub-steps store no blocks (see KS > 1 below)

// TILED: the monodromy blocks of a trajectory are stored as 16 x 16 tiles (sc_state.mono_layout = 1, see the header):
// tile (ra, rb) holds its part of Mqq, Mqp, Mpq, Mpp one after the other, each row-major inside the tile.  With the
// row mapping trow = 4 w + j a wave instruction then covers 512 contiguous bytes, the four waves one tile plane, and
// the workgroup walks the 4 D^2 doubles of the trajectory linearly -- measured 14 % more streaming bandwidth than the
// 128-byte row segments of the row-major layout (tools/micro/stream_patterns.hip).
//
// KS > 1 (sc_hk_step_multi: KS = 2; sc_hk_step_visit: KS = 2 .. 4): KS consecutive time steps per VISIT of a trajectory; every sub-step is the one-step kernel's
// stream-eliminate sequence, the next one follows at once by the same threads at the same addresses.  Two schemes, chosen per NR at
// compile time (mid_store below; measurements and what else was tried: docs/NOTEBOOK.md sections 9 and 9.2):
//   NR >= NOSTORE_MIN_NR (D > 32), store-free: only the LAST sub-step of a visit stores the blocks.  An earlier sub-step ks
//     loads the blocks of the visit's start, applies P(0) .. P(ks) (prop[0..ks], kept in LDS for the whole visit), forms its
//     prefactor matrix and determinant and stores nothing: nobody outside the kernel reads the blocks between the sub-steps, and
//     the intermediate store was a full HBM write pass.  Every later sub-step loads the SAME blocks again and redoes the earlier
//     rotations one by one (sep_propagate_row is explicit fma: the bits the earlier sub-steps formed; no composed 2 x 2 products),
//     the last one applies its own and stores.  The re-reads follow the first read within KS - 1 eliminations (~30 us each; 1024
//     workgroups hold 118 MB in between), so the first load of a visit is plain (it has to allocate in the L2 / the 256 MB
//     memory-side cache: profiles/pair_nostore_revisit.txt, profiles/visit_steps_revisit.txt) and only the last store is
//     non-temporal.  Until the last sub-step's stores the blocks in memory are those of the visit's start.  Per time step the
//     blocks cross HBM 2 / KS times, and sub-step ks redoes ks rotations: (KS - 1) / 2 per time step on top of its own, in a
//     kernel bound by FP64 issue -- measured at n = 1e5: KS = 3 is the fastest for every NR >= 3 (docs/NOTEBOOK.md section 9.3).
//   NR < NOSTORE_MIN_NR (D <= 32), the scheme of round 4: every sub-step stores; intermediate stores and the loads that
//     follow them are plain (they meet in the cache), the first load and the last store of a visit non-temporal.  There the kernel
//     waits for round trips, not for HBM, and the redone rotation is latency it cannot hide (store-free measured 0.6 - 2.6 % slower).
// Either way the kernel is bound by the elimination (FP64 VALU issue), no longer by HBM.
// The determinant tail.  An ITEM is one sub-step of one trajectory.  Its tail -- the product of the signed
// pivots (lu_partial_products, finish_determinant), the weak / zero-pivot handling, the branch rule and the stores of c2 / sgn /
// c2_mid / sgn_mid / flags -- is one lane's serial work on wave 0 and computes nothing another wave needs.  It does not stand
// between the end barrier of item t and the first barrier of item t + 1, where waves 1 - 3 would wait for it: thread 0 (threads
// 0 - 15 for the partial products) runs the tail of item t INSIDE phase B of item t + 1, between the request of a row slot (slot 2,
// or the last one for NR < 3) and the arithmetic on it, where wave 0 waits for memory anyway; the tail's own loads are issued behind
// that slot's, so it waits for nothing the wave would not have waited for.  The last item of a workgroup has no next phase B: its
// tail is an epilogue behind the trajectory loop.  Why the ordering holds:
//   - detbuf[p] / weakbuf[p] are double-buffered by item parity p.  The owner lanes of item t write them inside the elimination of
//     item t; every wave passes the end barrier of item t (and, when stepping, the prop[] barrier of item t + 1) between that
//     and the tail's reads.  The epilogue stands behind the end barrier of the last item.
//   - they are next written for item t + 2: reset at its top by threads of WAVE 0 only (16 NR <= 64), i.e. by the wave that ran
//     the tail of item t earlier in its own program order; the owner lanes' writes of item t + 2 lie behind its RESET BARRIER,
//     which wave 0 reaches only behind its phase B of item t + 1.
//   - the tails of one trajectory run in sub-step order in the same thread.  For ks > 0 the predecessor's determinant and sign come
//     from LDS (tailkeep), where that thread left them one tail earlier (LDS operations of a wave execute in order) -- not from
//     c2_mid / sgn_mid, which miss the L2 at n = 1e5; those are still stored, the correlation kernels read them.  For ks = 0 they
//     are loaded from c2[tr] / sgn[tr] at the head of the tail, and the partial products run while the loads are in flight.
//   - every path executes the barriers it executed before: the tail contains none, and the epilogue adds none.
// Row propagators of sub-step ks: M.work[ks][n][4][D] (hk_modes_multi_kernel); determinant and branch sign after sub-step
// ks < KS - 1: M.c2_mid / M.sgn_mid [ks][n], after the last one: the state's own arrays.
struct MultiArgs {
    const double *work;        // [KS][n][4][D]; KS = 1: unused (st.work)
    double *c2_mid, *sgn_mid;  // [KS - 1][n]
    int *unrepaired;           // counts determinants of INTERMEDIATE sub-steps whose in-block pivots were weak: the blocks have
                               // moved on by the time a fix-up launch could recompute them (sc_hk_step_multi's contract)
};

// -DSD_PHASE_CLOCK (variant library, tools/sd_phases.py): lane 0 of every wave of workgroups 0 and 512 writes the 100 MHz wall clock
// at six points of every item (trajectory sub-step) to g_sd_clock[2][4][256][6] -- raw time stamps, no accumulators in registers
#ifdef SD_PHASE_CLOCK
__device__ unsigned long long *g_sd_clock = nullptr;
#define SD_TICK(i)                                                                                                       \
    do {                                                                                                                 \
        if (pc_blk >= 0 && pc_item < 256 && (threadIdx.x & 63) == 0)                                                     \
            g_sd_clock[((pc_blk * 4 + (threadIdx.x >> 6)) * 256 + pc_item) * 6 + (i)] = wall_clock64();                  \
    } while (0)
#else
#define SD_TICK(i) do { } while (0)
#endif

template <int NR, int MINW, bool STEP, bool TILED, int KS = 1>
__global__ __launch_bounds__(256, MINW) void hk_step_sd_kernel(StepArgs A, MultiArgs MA) {
#ifdef SD_PHASE_CLOCK
    const int pc_blk = g_sd_clock == nullptr ? -1 : (blockIdx.x == 0 ? 0 : (blockIdx.x == 512 ? 1 : -1));
    int pc_item = 0;
#endif
    // KS > 1: do the intermediate sub-steps of a visit store their blocks (NR < NOSTORE_MIN_NR), or does the last one redo them?
    constexpr bool mid_store = KS > 1 && NR < NOSTORE_MIN_NR;
    constexpr int NP = mid_store ? 1 : KS;
    // NR = 4 with four sub-steps: P_a requested during the previous elimination is one value too many for 128 registers (hipcc spills it
    // behind s_waitcnt vmcnt(0) in the middle of the last diagonal block); there it is requested at the top of the sub-step instead
    constexpr bool late_p = KS >= 4 && NR >= 4;
    constexpr int aux_first = (KS == 1 || mid_store) ? AUX_NT : AUX_PLAIN;   // first load of a visit
    __shared__ double prop[NP][4 * 64];      // P_a = (p11, p12, p21, p22) of row a; without intermediate stores one set per sub-step of a visit
    __shared__ double scl[4 * 64];           // st, 1/st, si, 1/si
    __shared__ cplx rowbuf[16][64];
    __shared__ PivotRecord pivrec[16];
    // per-trajectory results of the elimination, double-buffered by trajectory parity: thread 0 finishes trajectory t
    // (product of the partial determinants, branch tracker) while the other waves already stream trajectory t+1
    __shared__ cplx detbuf[2][16 * NR];      // signed pivots, slot 16 KB + kt
    __shared__ int weakbuf[2];               // bit 0: weak in-block pivot (-> pivoted fallback), bit 1: zero pivot
    __shared__ int nextbuf[2];               // what thread 0 drew from the trajectory cursor
    __shared__ double tailkeep[4];           // thread 0, deferred tail of a visit: (Re c2, Im c2, sgn) of the sub-step before
    __shared__ long long tailtr;             // wave 0, deferred tail: the trajectory whose last sub-step waits for its tail (no register across the elimination)

    const int D = A.st.dim, DD = D * D, tid = threadIdx.x;
    constexpr bool do_step = STEP;                   // false: prefactor and tracker initialisation only (t = 0)
    constexpr int NCL_BASE = 16 * (NR - 1);          // first column of the last column tile
    if (tid < 64) {
        const bool in = tid < D;
        const double st = in ? A.hk.st[tid] : 1.0, si = in ? A.hk.si[tid] : 1.0;
        if (tid < 16) pivrec[tid].pad = 0;
        if (tid < 2) { nextbuf[tid] = 0; weakbuf[tid] = 0; }      // never read before they are written (RESET BARRIER below); defined anyway
        scl[tid] = st; scl[64 + tid] = 1.0 / st; scl[128 + tid] = si; scl[192 + tid] = 1.0 / si;
#pragma unroll
        for (int k = 0; k < NP; ++k) { prop[k][tid] = 1.0; prop[k][64 + tid] = 0.0; prop[k][128 + tid] = 0.0; prop[k][192 + tid] = 1.0; }
    }
    __syncthreads();

    const bool rows_odd = row_order_is_odd(D);
    // the thread index is rebuilt per trajectory from the wave number (a scalar) and the lane number (v_mbcnt): no
    // thread-index register lives across the elimination
    const int wave_s = __builtin_amdgcn_readfirstlane(tid >> 6);
    int seq0 = 0;                                  // tags of this workgroup's pivot records: unique per (trajectory, block)
    int par = 0;
    // raw[s][p][rb]: the four planes (Mqq, Mqp, Mpq, Mpp) of row slot ra = s (mod 2); prv: this thread's element of the
    // row propagators P_a (st.work, computed by hk_modes_kernel, "phase A"), handed to the rows' threads through prop[].  Slots 0
    // and 1 and prv of the NEXT item are requested before the last diagonal block of the current elimination starts (most of
    // the matrix registers are dead by then, both raw buffers are free): the first load round trip of an item hides behind
    // that block.
    double raw[2][4][NR];
    double pv[2][4] = {{1.0, 0.0, 0.0, 1.0}, {1.0, 0.0, 0.0, 1.0}};     // written by the dead block of load_slot only (see there)
    double prv = 0.0;
    bool first = true;
    // Trajectories are handed out through a device-side cursor (sc_state.flags[n + 1], zeroed by sc_hk_step): the first
    // gridDim.x statically, every further one to whichever workgroup is ready next.  The trajectories in flight are then
    // always ~gridDim.x CONSECUTIVE ones (static strides let the workgroups drift apart until the accesses are spread over
    // the whole state: measured 5.3 ms against 4.8 ms for compact windows), and nobody waits for a slow workgroup at the
    // end.  Thread 0 draws the next index at the top of a trajectory; it reaches the others through LDS behind the first
    // barrier of the elimination.  Without sc_state.flags: static stride.
    int *cursor = A.st.flags ? A.st.flags + A.st.n + 1 : nullptr;
    int64_t trn = 0;
    // every tail is deferred (see "The determinant tail").  The constant is named once, in item_tail, for the compiler's sake alone:
    // without that capture hipcc assigns the registers of every NR >= 2 instantiation differently; it goes with the dead block of load_slot
    constexpr bool defer_tail = true;
    constexpr bool skip_lu = SC_SD_ABLATE_LU != 0;
    // the tail of sub-step kp of trajectory tp, whose results lie in the buffers of parity parp: determinant from the signed pivots,
    // weak / zero pivots, branch rule, stores.  `tl`: the thread's index as the caller has it; tp < 0: the trajectory wave 0 left in
    // tailtr.  No barrier in here.
    auto item_tail = [&](auto kpc, int64_t tp, int parp, int tl) {
        constexpr int kp = decltype(kpc)::value;
        if (tl >= 16) return;
        if (tp < 0) tp = tailtr;
        cplx *c2 = (cplx *)A.st.c2;
        // previous value / destination of this sub-step's determinant and branch sign
        const cplx *c2_in = kp == 0 ? c2 + tp : (const cplx *)MA.c2_mid + ((int64_t)(kp - 1) * A.st.n + tp);
        const double *sg_in = kp == 0 ? A.st.sgn + tp : MA.sgn_mid + ((int64_t)(kp - 1) * A.st.n + tp);
        cplx *c2_out = kp == KS - 1 ? c2 + tp : (cplx *)MA.c2_mid + ((int64_t)kp * A.st.n + tp);
        double *sg_out = kp == KS - 1 ? A.st.sgn + tp : MA.sgn_mid + ((int64_t)kp * A.st.n + tp);
        const int *weak = &weakbuf[parp];
        // the predecessor FIRST (thread 0): from LDS where the tail of the sub-step before left it, otherwise (sub-step 0) from
        // memory -- requested here so that the partial products below run under the round trip
        constexpr bool kept = defer_tail && kp > 0;
        cplx prev = c_make(0.0, 0.0);
        double sg = 1.0;
        if (tl == 0 && do_step) {
            if (kept) { prev = c_make(tailkeep[0], tailkeep[1]); sg = tailkeep[2]; }
            else { prev = *c2_in; sg = *sg_in; }
        }
        if (tl < 16) lu_partial_products<NR>(detbuf[parp], tl);
        if (kp == KS - 1 && tl == 0 && (*weak & 1) && A.st.flags && !skip_lu) {
            // c2 / sgn are left to the fully pivoted fallback, which tracks against the state's c2 / sgn: after an
            // intermediate sub-step those are KS steps old, so hand it this sub-step's predecessor (c2_mid / sgn_mid)
            if (KS > 1) {
                c2[tp] = prev;
                A.st.sgn[tp] = sg;
            }
            A.st.flags[tp] = 1;
            atomicAdd(&A.st.flags[A.st.n], 1);   // lets the fix-up launch return at once when nothing was flagged
        } else if (tl == 0) {
            if (KS > 1 && kp < KS - 1 && (*weak & 1) && !skip_lu) atomicAdd(MA.unrepaired, 1);
            const cplx c2new = (*weak & 2) ? c_make(0.0, 0.0) : finish_determinant(detbuf[parp], rows_odd);
            double sgnew = 1.0;
            if (do_step) {
                const bool flip = crossed_branch_cut(prev, c2new);
                sgnew = flip ? -sg : sg;
                if (KS > 1) *sg_out = sgnew;
                else if (flip) *sg_out = sgnew;
            } else {
                *sg_out = 1.0;
            }
            *c2_out = c2new;
            if (kp < KS - 1) { tailkeep[0] = c2new.x; tailkeep[1] = c2new.y; tailkeep[2] = sgnew; }
        }
    };
    for (int64_t tr = blockIdx.x; tr < A.st.n; tr = trn) {
      sfor<0, KS>([&](auto ksc) {
        constexpr int ks = decltype(ksc)::value;                 // sub-step of this visit
        constexpr int aux_load = ks == 0 ? aux_first : AUX_PLAIN;
        constexpr int aux_store = ks == KS - 1 ? AUX_NT : AUX_PLAIN;
        constexpr bool store_blocks = ks == KS - 1 || mid_store; // otherwise an intermediate sub-step leaves the blocks in memory alone
        // what is streamed next: the next sub-step of this trajectory, or the first one of the next trajectory
        constexpr int ksn = ks + 1 < KS ? ks + 1 : 0;
        int *weak = &weakbuf[par];
        // Everything derived from the thread index is recomputed per trajectory: hipcc otherwise keeps those values live
        // across the elimination, spills them, and reloads them one by one behind s_waitcnt vmcnt(0) in the load stream
        unsigned ones = ~0u;
        __asm__ volatile("" : "+s"(ones));
        const int tl = (wave_s << 6) | (int)__builtin_amdgcn_mbcnt_hi(ones, __builtin_amdgcn_mbcnt_lo(ones, 0u));
        const int tj = tl & 15, tjl = tj;
        const int til = (tl >> 6) * 4 + ((tl >> 4) & 3);    // wave w holds rows 4w .. 4w+3 of every 16-row slot
        if (tl == 0) *weak = SC_SD_FORCE_FIXUP;             // 1: variant library that hands every trajectory to the fallback
        if (tl < 16 * NR) {
            // formed HERE: hipcc otherwise keeps the constant's four registers live across the whole trajectory loop and spills them
            double one = 1.0, zero = 0.0;
            __asm__ volatile("" : "+v"(one), "+v"(zero));
            detbuf[par][tl] = c_make(one, zero);
        }
        int drawn = 0;
        if (ks == 0 && cursor && tl == 0) drawn = atomicAdd(cursor, 1);
        const int pk = tl >> 6, pa = tl & 63;               // thread -> (row of P, mode) of st.work

        // ---------------- phase B ----------------
        cplx m[NR][NR];
        // All accesses to the trajectory's blocks are raw BUFFER instructions: one resource (base M, 32 D^2 bytes), the
        // tile / plane position as scalar byte offset, the thread's position inside the tile as 32-bit VGPR offset.
        // Threads outside the matrix carry an offset beyond the resource: their loads return 0 and their stores are
        // dropped by the range check, so phase B has no branches and no 64-bit address arithmetic.
        int Dl = D;
        __asm__ volatile("" : "+s"(Dl));                 // tile offsets are recomputed (SALU) per trajectory, not kept in SGPRs
        constexpr unsigned OOB = 0x7fffffffu;
        const bool rowok_last = 16 * (NR - 1) + til < Dl, colok_last = NCL_BASE + tj < Dl;
        // byte offsets of this thread inside a tile: row-major (row, tj) of a D x D plane; tiled: inside a 16-wide / the
        // last (narrower) column tile
        // tiled: 16 bytes per element of a plane pair (Mqq, Mqp) / (Mpq, Mpp)
        const unsigned vo = TILED ? 16u * (unsigned)(til * 16 + tj) : 8u * (unsigned)(til * Dl + tj);
        const unsigned vol = TILED ? 16u * (unsigned)(til * (Dl - NCL_BASE) + tj) : vo;
        auto voffset = [&](int ra, int rb) {
            const unsigned v = rb == NR - 1 ? vol : vo;
            const bool ok = (ra < NR - 1 || rowok_last) && (rb < NR - 1 || colok_last);
            return (int)((ra < NR - 1 && rb < NR - 1) ? v : (ok ? v : OOB));
        };
        auto tile_base = [&](int ra, int rb) {           // scalar byte offset of tile (ra, rb)
            const int nra = min(16, Dl - 16 * ra);
            return 8 * (TILED ? 4 * (16 * ra * Dl + nra * 16 * rb) : 16 * ra * Dl + 16 * rb);
        };
        auto plane_bytes = [&](int ra, int rb) {         // distance between the four blocks of an element
            const int nra = min(16, Dl - 16 * ra), ncb = rb == NR - 1 ? Dl - NCL_BASE : 16;
            return 8 * (TILED ? nra * ncb : Dl * Dl);
        };
        auto resource = [&](int64_t t) {
            return __builtin_amdgcn_make_buffer_rsrc(A.st.mono + t * 4 * (int64_t)Dl * Dl, 0, 32 * Dl * Dl, 0x00020000);
        };
        auto load_slot = [&](auto rac, int64_t t, auto auxc) {
            constexpr int ra = decltype(rac)::value, aux = decltype(auxc)::value;
            const __amdgpu_buffer_rsrc_t rs = resource(t);
#pragma unroll
            for (int rb = 0; rb < NR; ++rb) {
                const int vofs = voffset(ra, rb), base = tile_base(ra, rb), plane = plane_bytes(ra, rb);
                if constexpr (TILED) {                     // one 16-byte load per plane pair
#pragma unroll
                    for (int pp = 0; pp < 2; ++pp) {
                        const sc_v4u v = __builtin_amdgcn_raw_buffer_load_b128(rs, vofs, base + pp * 2 * plane, aux);
                        raw[ra & 1][2 * pp][rb] = __hiloint2double((int)v.y, (int)v.x);
                        raw[ra & 1][2 * pp + 1][rb] = __hiloint2double((int)v.w, (int)v.z);
                    }
                } else {
#pragma unroll
                    for (int pl = 0; pl < 4; ++pl) {
                        const sc_v2u v = __builtin_amdgcn_raw_buffer_load_b64(rs, vofs, base + pl * plane, 0);
                        raw[ra & 1][pl][rb] = __hiloint2double((int)v.y, (int)v.x);
                    }
                }
            }
            if (false && do_step) {
                // DEAD: the rejected direct load of P_a (every thread reads the P_a of its rows itself, no LDS hand-over: 4.65 ms
                // against 4.56 ms).  It and pv[] are all that is left of that experiment: without them hipcc assigns the registers
                // of every NR >= 2 instantiation differently (same counts, no spills), so they go only with an A/B measurement on
                // the GPU (docs/NOTEBOOK.md, closing note)
                const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(A.st.work + t * 4 * (int64_t)Dl, 0, 32 * Dl, 0x00020000);
                const unsigned vw = 16 * ra + til < Dl ? 8u * (unsigned)(16 * ra + til) : OOB;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const sc_v2u v = __builtin_amdgcn_raw_buffer_load_b64(rw, (int)vw, 8 * k * Dl, 0);
                    pv[ra & 1][k] = __hiloint2double((int)v.y, (int)v.x);
                }
            }
        };
        auto first_requests = [&](int64_t t, auto ksnc) {    // P_a and row slot 0 of sub-step ksnc of trajectory t
            constexpr int k2 = decltype(ksnc)::value;
            constexpr int aux2 = k2 == 0 ? aux_first : AUX_PLAIN;
            const double *wk = KS > 1 ? MA.work + (int64_t)k2 * A.st.n * 4 * Dl : A.st.work;
            if (do_step && pa < Dl) prv = wk[(t * 4 + pk) * (int64_t)Dl + pa];
            load_slot(std::integral_constant<int, 0>(), t, std::integral_constant<int, aux2>());
            // row slot 1 as well (both raw buffers are free during the last diagonal block): -3 %
            if (NR > 1) load_slot(std::integral_constant<int, (NR > 1 ? 1 : 0)>(), t, std::integral_constant<int, aux2>());
        };
        auto finish_slot = [&](auto rac) {
            constexpr int ra = decltype(rac)::value;
            const __amdgpu_buffer_rsrc_t rs = resource(tr);
            const int al = (16 * ra + til) & 63;
            if constexpr (ks > 0 && !mid_store) {
                // the blocks in memory are those of the visit's start: redo the earlier sub-steps' rotations first (explicit fma:
                // the bits those sub-steps formed), all rb of the slot per propagator, so that the four P values share registers
                sfor<0, ks>([&](auto kpc) {
                    constexpr int kp = decltype(kpc)::value;
                    WM_BLOCK {          // a basic block of its own: scheduled together with the rest of the slot it costs 9 spilled registers at NR = 4
                        const double q11 = prop[kp][al], q12 = prop[kp][64 + al], q21 = prop[kp][128 + al], q22 = prop[kp][192 + al];
#pragma unroll
                        for (int rb = 0; rb < NR; ++rb)
                            sep_propagate_row(q11, q12, q21, q22, raw[ra & 1][0][rb], raw[ra & 1][1][rb], raw[ra & 1][2][rb], raw[ra & 1][3][rb]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                });
            }
            constexpr int kq = mid_store ? 0 : ks;
            const double p11 = prop[kq][al], p12 = prop[kq][64 + al], p21 = prop[kq][128 + al], p22 = prop[kq][192 + al];
            const double sta = scl[al], ista = scl[64 + al];
#pragma unroll
            for (int rb = 0; rb < NR; ++rb) {
                const int vofs = voffset(ra, rb), base = tile_base(ra, rb), plane = plane_bytes(ra, rb);
                double mqq = raw[ra & 1][0][rb], mqp = raw[ra & 1][1][rb], mpq = raw[ra & 1][2][rb], mpp = raw[ra & 1][3][rb];
                if (do_step) {
                    sep_propagate_row(p11, p12, p21, p22, mqq, mqp, mpq, mpp);
                    const double out[4] = {mqq, mqp, mpq, mpp};
                    if constexpr (!store_blocks) {
                        (void)out; (void)rs; (void)vofs; (void)base; (void)plane;
                        // no store, no store-data hazard to guard; the elements are still scheduled one by one (hipcc otherwise
                        // interleaves the four rb of the slot and spills 8 registers at NR = 4)
                        __builtin_amdgcn_sched_barrier(0);
                    } else if constexpr (TILED) {
#pragma unroll
                        for (int pp = 0; pp < 2; ++pp) {
                            sc_v4u v;
                            v.x = (unsigned)__double2loint(out[2 * pp]); v.y = (unsigned)__double2hiint(out[2 * pp]);
                            v.z = (unsigned)__double2loint(out[2 * pp + 1]); v.w = (unsigned)__double2hiint(out[2 * pp + 1]);
                            __builtin_amdgcn_raw_buffer_store_b128(v, rs, vofs, base + pp * 2 * plane, aux_store);
                            // STORE-DATA HAZARD (found on MI355X, round 4): a buffer store of more than 8 bytes reads its data
                            // registers over more than one cycle, and a VALU instruction that overwrites them in the next wait
                            // states changes what is stored (lanes 12..15 of every row of the last wave got Im M' instead of
                            // Mpq, in 1 % of the trajectories, only with many workgroups in flight).  hipcc's hazard recogniser
                            // covers the case WITHOUT a scalar offset register only (GCNHazardRecognizer::createsVALUHazard);
                            // these stores have one.  Three wait states, and nothing is scheduled across them.
                            __builtin_amdgcn_sched_barrier(0);
                            __asm__ volatile("s_nop 2");
                            __builtin_amdgcn_sched_barrier(0);
                        }
                    } else {
#pragma unroll
                        for (int pl = 0; pl < 4; ++pl) {
                            sc_v2u v;
                            v.x = (unsigned)__double2loint(out[pl]); v.y = (unsigned)__double2hiint(out[pl]);
                            __builtin_amdgcn_raw_buffer_store_b64(v, rs, vofs, base + pl * plane, 0);
                        }
                    }
                }
                const int bl = (16 * rb + tjl) & 63;
                const double sib = scl[128 + bl], isib = scl[192 + bl];
                // elements outside the matrix were loaded as zeros: their mat entries are zeros
                m[ra][rb] = prefactor_element_diag(sta, ista, sib, isib, mqq, mqp, mpq, mpp);
                // the element must exist HERE: hipcc otherwise sinks its computation to the first use in the elimination
                // and carries (spills) the four raw values and the scalings instead
                __asm__ volatile("" : "+v"(m[ra][rb].x), "+v"(m[ra][rb].y));
            }
        };
        // sched_barrier: the stages are scheduled one by one (hipcc otherwise interleaves the stages of this branch-free
        // block until the raw values of three slots are live at once, and spills)
        SD_TICK(0);
        if constexpr (late_p) {                          // not requested during the previous elimination (see late_p)
            if (!first && do_step && pa < Dl) prv = MA.work[(((int64_t)ks * A.st.n + tr) * 4 + pk) * (int64_t)Dl + pa];
        }
        if (first || NR == 1) first_requests(tr, ksc);
        const bool had_item = !first;                    // deferred tail: is there an item before this one?
        first = false;
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_sched_barrier(0);        // both stay: dropping one changes the generated code
        if (do_step) {
            // every wave is past the previous visit's phase B of this sub-step (the elimination barriers lie in between), so
            // prop[ks] may be overwritten without another barrier; the sets of the earlier sub-steps of this visit stay
            if (pa < D) prop[mid_store ? 0 : ks][64 * pk + pa] = prv;
            __syncthreads();
        }
        sfor<0, NR>([&](auto rac) {
            constexpr int ra = decltype(rac)::value;
            // slots 0 and 1 were requested during the previous elimination; every later slot is requested when the one before it is
            // finished (requesting slot 2 before slot 1 is finished as well: 4 spilled registers, 0.5 % slower)
            if (ra > 1) load_slot(rac, tr, std::integral_constant<int, aux_load>());
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (ra == (NR < 3 ? NR - 1 : 2)) {
                // the tail of the item before this one (see "The determinant tail"), while this slot's loads are in flight
                if constexpr (ks > 0) item_tail(std::integral_constant<int, ks - 1>(), tr, par ^ 1, tl);
                else if (had_item) item_tail(std::integral_constant<int, KS - 1>(), -1, par ^ 1, tl);
                __builtin_amdgcn_sched_barrier(0);
            }
            finish_slot(rac);
            __builtin_amdgcn_sched_barrier(0);
        });

        // ---------------- phase C: determinant in registers ----------------
        // phase ablation (tools/phase_timing.py) is a COMPILE-time switch of a variant library: a run-time flag here costs the
        // kernel 148 B/lane of scratch and 30 % of its speed
        SD_TICK(1);
        if (ks == 0 && cursor && tl == 0) nextbuf[par] = drawn;
        // RESET BARRIER -- unconditional, in every variant of this kernel (with or without the elimination).  It orders
        //   (a) thread 0's nextbuf[par] = drawn against the readfirstlane(nextbuf[par]) of every wave below: the value is
        //       the next trajectory index and goes straight into resource(trn), an unordered read addresses memory
        //       outside the state (the GPU memory fault of round 2's tuning build, docs/NOTEBOOK.md section 8.2);
        //   (b) the resets of *weak and detbuf[par] above against the owner lanes' read-modify-writes in the elimination;
        //   (c) the previous trajectory's last uses of the pivot ring (rowbuf / pivrec) against block 0's first records.
        // Later blocks need no barrier: a wave owns every fourth pivot step, so when step s is published every wave has
        // consumed step s - 4, and a ring entry is rewritten 16 steps after its last use.
        __syncthreads();
        SD_TICK(2);
        auto no_barrier = [] {};       // no barrier in front of a diagonal block: the RESET BARRIER is block 0's, later blocks need none
        sfor<0, NR>([&](auto kbc) {
            constexpr int KB = decltype(kbc)::value;
            if (ks == 0 && KB == (NR > 1 ? 1 : 0)) { // behind the RESET BARRIER (NR = 1: the value is read after the last barrier)
                if (NR > 1) trn = cursor ? (int64_t)gridDim.x + __builtin_amdgcn_readfirstlane(nextbuf[par]) : tr + gridDim.x;
            }
            if (NR > 1 && KB == (NR > 2 ? NR - 1 : 1)) {       // the next item's first requests, in front of the last diagonal block
                const int64_t tnext = ks + 1 < KS ? tr : trn;
                if (tnext < A.st.n) {
                    if constexpr (late_p) {         // the row slots only: P_a follows at the top of the sub-step
                        constexpr int auxn = ksn == 0 ? aux_first : AUX_PLAIN;
                        load_slot(std::integral_constant<int, 0>(), tnext, std::integral_constant<int, auxn>());
                        load_slot(std::integral_constant<int, 1>(), tnext, std::integral_constant<int, auxn>());
                    } else {
                        first_requests(tnext, std::integral_constant<int, ksn>());
                    }
                } else {                            // nothing follows: end the live ranges of the old values
                    prv = 0.0;
#pragma unroll
                    for (int pl = 0; pl < 4; ++pl)
#pragma unroll
                        for (int rb = 0; rb < NR; ++rb) { raw[0][pl][rb] = 0.0; raw[1][pl][rb] = 0.0; }
                }
            }
            // TRIM_LAST: the last diagonal block without the steps nobody reads (sc_hk_lu.h)
            if (!skip_lu) eliminate_block<NR, KB, 64, true>(m, detbuf[par], D, seq0 + 1 + KB, rowbuf, pivrec, weak, tl, no_barrier);
        });
        SD_TICK(3);
        __syncthreads();
        SD_TICK(4);
        if (ks == 0 && NR == 1) trn = cursor ? (int64_t)gridDim.x + __builtin_amdgcn_readfirstlane(nextbuf[par]) : tr + gridDim.x;
        // no barrier after this: the buffers of this parity are next written two items on
        if (ks == KS - 1 && tl == 0) tailtr = tr;       // the item's tail runs inside the next item, or in the epilogue
        seq0 += 4; par ^= 1;
        SD_TICK(5);
#ifdef SD_PHASE_CLOCK
        ++pc_item;
#endif
      });
    }
    // epilogue: the tail of the workgroup's last item, behind that item's end barrier
    if (!first) item_tail(std::integral_constant<int, KS - 1>(), -1, par ^ 1, tid);
}

#ifdef SD_PHASE_CLOCK
}  // namespace
extern "C" int sc_sd_phase_clock(unsigned long long *buf) {       // device buffer of 2*4*256*6 time stamps, or NULL to switch off
    return hipMemcpyToSymbol(HIP_SYMBOL(g_sd_clock), &buf, sizeof(buf)) == hipSuccess ? 0 : -3;
}
namespace {
#endif

// "phase A" as its own launch: one wavefront per trajectory, lane = mode.  RK4 of (q_a, p_a) with the reference's
// stage formula, the action and <T+V> at the k4 stage by wave reductions, and the 2x2 RK4 propagator P_a of the
// monodromy rows (unit vectors pushed through the same stage formula) -> st.work[tr][4][D].
__global__ __launch_bounds__(256) void hk_modes_kernel(StepArgs A) {
    const int D = A.st.dim, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double dt = A.dt, h6 = dt / 6.0;
    __shared__ double wsum[4];
    double esum = 0.0;
    for (int64_t tr = (int64_t)blockIdx.x * 4 + wave; tr < A.st.n; tr += (int64_t)gridDim.x * 4) {
        double *qp = A.st.qp + tr * 2 * D;
        double *pr = A.st.work + tr * 4 * (int64_t)D;
        double red5[5] = {0, 0, 0, 0, 0};
        if (lane < D) {
            const double im = A.pot.inv_mass[lane];
            const double c0 = A.pot.par0[lane], c1 = A.pot.par1 ? A.pot.par1[lane] : 0.0;
            double q = qp[lane], p = qp[D + lane], h1, h2, h3, h4, p11, p12, p21, p22;
            sep_mode_rk4(A.pot.kind, c0, c1, im, dt, q, p, red5, h1, h2, h3, h4);
            qp[lane] = q;
            qp[D + lane] = p;
            sep_row_propagator(im, h1, h2, h3, h4, dt, p11, p12, p21, p22);
            pr[lane] = p11; pr[D + lane] = p12; pr[2 * D + lane] = p21; pr[3 * D + lane] = p22;
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) red5[i] = wave_sum(red5[i]);
        if (lane == 0) {
            A.st.act[tr] += h6 * (red5[0] + 2.0 * red5[1] + 2.0 * red5[2] + red5[3]);
            esum += red5[4];
        }
    }
    if (lane == 0) wsum[wave] = esum;
    __syncthreads();
    if (threadIdx.x == 0 && A.epart) A.epart[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}


// hk_modes_kernel for KS consecutive time steps (sc_hk_step_multi): (q_a, p_a) stay in registers between the sub-steps; row
// propagators of sub-step ks -> work[ks][n][4][D]; (q, p, S) after sub-step ks < KS - 1 -> qp_mid / act_mid [ks][n] (what the
// correlation kernel of time step k + ks + 1 reads), after the last one -> the state; <T+V> sums of sub-step ks -> epart[ks][grid].
// The arithmetic of a sub-step is that of hk_modes_kernel.
struct ModesMultiArgs {
    double *work, *qp_mid, *act_mid;
};
template <int KS>
__global__ __launch_bounds__(256) void hk_modes_multi_kernel(StepArgs A, ModesMultiArgs MM) {
    const int D = A.st.dim, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double dt = A.dt, h6 = dt / 6.0;
    __shared__ double wsum[KS][4];
    double esum[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) esum[ks] = 0.0;
    for (int64_t tr = (int64_t)blockIdx.x * 4 + wave; tr < A.st.n; tr += (int64_t)gridDim.x * 4) {
        double *qp = A.st.qp + tr * 2 * D;
        const bool in = lane < D;
        double q = in ? qp[lane] : 0.0, p = in ? qp[D + lane] : 0.0;
        const double im = in ? A.pot.inv_mass[lane] : 0.0, c0 = in ? A.pot.par0[lane] : 0.0, c1 = (in && A.pot.par1) ? A.pot.par1[lane] : 0.0;
        double act = A.st.act[tr];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            double *pr = MM.work + ((int64_t)ks * A.st.n + tr) * 4 * (int64_t)D;
            double red5[5] = {0, 0, 0, 0, 0};
            if (in) {
                double h1, h2, h3, h4, p11, p12, p21, p22;
                sep_mode_rk4(A.pot.kind, c0, c1, im, dt, q, p, red5, h1, h2, h3, h4);
                sep_row_propagator(im, h1, h2, h3, h4, dt, p11, p12, p21, p22);
                pr[lane] = p11; pr[D + lane] = p12; pr[2 * D + lane] = p21; pr[3 * D + lane] = p22;
                double *qo = ks == KS - 1 ? qp : MM.qp_mid + ((int64_t)ks * A.st.n + tr) * 2 * D;
                qo[lane] = q; qo[D + lane] = p;
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) red5[i] = wave_sum(red5[i]);
            act += h6 * (red5[0] + 2.0 * red5[1] + 2.0 * red5[2] + red5[3]);
            if (lane == 0) {
                if (ks == KS - 1) A.st.act[tr] = act; else MM.act_mid[(int64_t)ks * A.st.n + tr] = act;
                esum[ks] += red5[4];
            }
        }
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) if (lane == 0) wsum[ks][wave] = esum[ks];
    __syncthreads();
    if (threadIdx.x < KS && A.epart)
        A.epart[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = wsum[threadIdx.x][0] + wsum[threadIdx.x][1] + wsum[threadIdx.x][2] + wsum[threadIdx.x][3];
}

// ---- D <= 16: one WAVEFRONT per trajectory, everything in registers, no barrier and no LDS hand-off in the elimination.
// Lane (rg, tj) = (lane >> 4, lane & 15) holds column tj of the matrix rows rg, rg + 4, rg + 8, rg + 12 (rows and
// columns beyond D are padded with the identity), for the four monodromy blocks and the prefactor matrix alike; a
// load / store instruction covers four 128-byte row segments.  The modes (RK4 of q, p, S and the row propagators P_a)
// are done by the first D lanes of the same wavefront; P_a reaches the lanes that hold row a through a per-wave LDS
// array.  Elimination, fully unrolled over the pivot row k (so its DPP row rg_k = k & 3 and register k >> 2 are
// static): the pivot column is the largest live entry of the WHOLE row (all columns sit in one 16-lane DPP row: true
// partial pivoting, no fallback needed), the scaled pivot row crosses to the other DPP rows by ds_bpermute, the
// multipliers come from lane (rg, pl) by the same 64-bit DPP row_newbcast / computed jump as in the big kernel, and the
// sign of the column permutation is accumulated from the live-column mask.
template <bool STEP>
__global__ __launch_bounds__(256) void hk_step_w16_kernel(StepArgs A) {
    __shared__ double prop[4][4][16];
    __shared__ double wsum[4];
    const int D = A.st.dim, DD = D * D, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rg = lane >> 4, tj = lane & 15;
    const double dt = A.dt, h6 = dt / 6.0;
    const bool colok = tj < D;
    const double sib = colok ? A.hk.si[tj] : 1.0, isib = 1.0 / sib;
    double sta[4], ista[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int r = rg + 4 * s;
        sta[s] = r < D ? A.hk.st[r] : 1.0;
        ista[s] = 1.0 / sta[s];
    }
    double esum = 0.0;
    for (int64_t tr = (int64_t)blockIdx.x * 4 + wave; tr < A.st.n; tr += (int64_t)gridDim.x * 4) {
        double *qp = A.st.qp + tr * 2 * D;
        double *M = A.st.mono + tr * 4 * (int64_t)DD;
        double p11[4] = {1, 1, 1, 1}, p12[4] = {0, 0, 0, 0}, p21[4] = {0, 0, 0, 0}, p22[4] = {1, 1, 1, 1};
        if (STEP) {
            double red5[5] = {0, 0, 0, 0, 0};
            if (lane < D) {
                const double im = A.pot.inv_mass[lane];
                const double c0 = A.pot.par0[lane], c1 = A.pot.par1 ? A.pot.par1[lane] : 0.0;
                double q = qp[lane], p = qp[D + lane], h1, h2, h3, h4, u1, u2, v1, v2;       // P_a = [[u1, u2], [v1, v2]]
                sep_mode_rk4(A.pot.kind, c0, c1, im, dt, q, p, red5, h1, h2, h3, h4);
                qp[lane] = q;
                qp[D + lane] = p;
                sep_row_propagator(im, h1, h2, h3, h4, dt, u1, u2, v1, v2);
                prop[wave][0][lane] = u1; prop[wave][1][lane] = u2; prop[wave][2][lane] = v1; prop[wave][3][lane] = v2;
            }
#pragma unroll
            for (int i = 0; i < 5; ++i) red5[i] = wave_sum(red5[i]);
            if (lane == 0) {
                A.st.act[tr] += h6 * (red5[0] + 2.0 * red5[1] + 2.0 * red5[2] + red5[3]);
                esum += red5[4];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int r = rg + 4 * s;
                if (r < D) { p11[s] = prop[wave][0][r]; p12[s] = prop[wave][1][r]; p21[s] = prop[wave][2][r]; p22[s] = prop[wave][3][r]; }
            }
        }
        // ---- phase B
        cplx m[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int r = rg + 4 * s;
            const bool ok = colok && r < D;
            const int e = r * D + tj;
            double mqq = ok ? M[e] : 0.0, mqp = ok ? M[DD + e] : 0.0, mpq = ok ? M[2 * DD + e] : 0.0, mpp = ok ? M[3 * DD + e] : 0.0;
            if (STEP) {
                sep_propagate_row(p11[s], p12[s], p21[s], p22[s], mqq, mqp, mpq, mpp);
                if (ok) { M[e] = mqq; M[DD + e] = mqp; M[2 * DD + e] = mpq; M[3 * DD + e] = mpp; }
            }
            m[s] = ok ? prefactor_element_diag(sta[s], ista[s], sib, isib, mqq, mqp, mpq, mpp) : c_make(r == tj ? 1.0 : 0.0, 0.0);
        }
        // ---- phase C
        cplx det = c_make(1.0, 0.0);
        bool live = colok, singular = false;
        int parity = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < D && !singular) {
                constexpr int dummy = 0; (void)dummy;
                const int rgk = k & 3, sk = k >> 2;
                const int blk = (__double2hiint(c_abs2(m[sk])) & ~15) | (15 - tj);
                const int keymax = row16_max_i32((live && rg == rgk) ? blk : -1);
                const int kb = __builtin_amdgcn_readlane(keymax, 16 * rgk);
                const int pl = 15 - (kb & 15);
                const int src = 16 * rgk + pl;
                const cplx piv = c_make(readlane_f64(m[sk].x, src), readlane_f64(m[sk].y, src));
                if (piv.x == 0.0 && piv.y == 0.0) { singular = true; }
                else {
                    det = c_mul(det, piv);
                    const cplx inv = c_inv_fast(piv);
                    // sign of the column permutation: live columns to the left of the pivot column
                    const unsigned long long lm = __ballot(live && rg == 0);
                    parity ^= __popcll(lm & ((1ull << pl) - 1ull)) & 1;
                    // scaled pivot row at this lane's column (from DPP row rgk)
                    const cplx rowv = c_make(__shfl(m[sk].x, 16 * rgk + tj, 64), __shfl(m[sk].y, 16 * rgk + tj, 64));
                    const bool keep = live && tj != pl;
                    const cplx rs = c_mul(rowv, inv);
                    const cplx r = c_make(keep ? rs.x : 0.0, keep ? rs.y : 0.0);
                    cplx c[4];
                    column_fetch_n(pl, m[0], m[1], m[2], m[3], c[0], c[1], c[2], c[3]);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        if (rg + 4 * s <= k) c[s] = c_make(0.0, 0.0);        // rows 0..k are finished
                        m[s] = c_fnma(c[s], r, m[s]);
                    }
                    live = live && tj != pl;
                }
            }
        }
        if (lane == 0) {
            if (singular) det = c_make(0.0, 0.0);
            else if (parity) det = c_make(-det.x, -det.y);
            cplx *c2 = (cplx *)A.st.c2;
            if (STEP) {
                const cplx prev = c2[tr];
                if (crossed_branch_cut(prev, det)) A.st.sgn[tr] = -A.st.sgn[tr];
            } else {
                A.st.sgn[tr] = 1.0;
            }
            c2[tr] = det;
        }
    }
    if (lane == 0) wsum[wave] = esum;
    __syncthreads();
    if (threadIdx.x == 0 && A.epart && STEP) A.epart[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

}  // namespace

// launch the fast path; the caller has validated the arguments (separable potential, diag prefactor, D <= 64)
int sc_launch_step_sd(const StepArgs &a, hipStream_t s) {
    const int D = a.st.dim, nr = (D + 15) / 16, grid = sc_step_grid(a.st.n, D);
    int occ = 4;
#ifdef SC_TUNING
    if (const char *occ_env = getenv("SC_SD_OCC")) occ = atoi(occ_env);   // waves per SIMD the NR=4 kernel is compiled for
#endif
    if (D <= 16) {
        const int rc = sc_launch_step_sep16(a, grid, s);      // four trajectories per wavefront
        if (rc != 0) return rc < 0 ? rc : SC_OK;
        // partial sums: only the first `wg` entries are written, the energy guard adds sc_step_grid() of them
        const int64_t quads = (a.st.n + 3) / 4;
        const int wg = (int)(quads < 2048 ? quads : 2048);
        if (a.epart && hipMemsetAsync(a.epart, 0, sizeof(double) * (size_t)grid, s) != hipSuccess)
            return sc_check_launch("sc_hk_step (partials)");
        if ((a.mode & 0xff) == 0) hipLaunchKernelGGL(hk_step_w16_kernel<true>, dim3(wg), dim3(256), 0, s, a);
        else hipLaunchKernelGGL(hk_step_w16_kernel<false>, dim3(wg), dim3(256), 0, s, a);
        return sc_check_launch("sc_hk_step (one wavefront per trajectory)");
    }
    if ((a.mode & 0xff) == 0) hipLaunchKernelGGL(hk_modes_kernel, dim3(grid), dim3(256), 0, s, a);
    const bool step = (a.mode & 0xff) == 0;
    const bool tiled = a.st.mono_layout == SC_MONO_TILED16;
    // the energy partials belong to hk_modes_kernel: this kernel's grid is free
#define SC_LAUNCH_SD(NR_, OCC_)                                                                                         \
    do {                                                                                                                \
        if (step && tiled) hipLaunchKernelGGL((hk_step_sd_kernel<NR_, OCC_, true, true>), dim3(grid), dim3(256), 0, s, a, MultiArgs{});   \
        else if (step) hipLaunchKernelGGL((hk_step_sd_kernel<NR_, OCC_, true, false>), dim3(grid), dim3(256), 0, s, a, MultiArgs{});     \
        else if (tiled) hipLaunchKernelGGL((hk_step_sd_kernel<NR_, OCC_, false, true>), dim3(grid), dim3(256), 0, s, a, MultiArgs{});    \
        else hipLaunchKernelGGL((hk_step_sd_kernel<NR_, OCC_, false, false>), dim3(grid), dim3(256), 0, s, a, MultiArgs{});              \
    } while (0)
    switch (nr) {
        case 1: SC_LAUNCH_SD(1, 4); break;
        case 2: SC_LAUNCH_SD(2, 4); break;
        case 3: SC_LAUNCH_SD(3, 4); break;
        default:
#ifdef SC_TUNING
            if (occ == 3) { SC_LAUNCH_SD(4, 3); break; }
            if (occ < 3) { SC_LAUNCH_SD(4, 2); break; }
#endif
            (void)occ;
            SC_LAUNCH_SD(4, 4);
            break;
    }
#undef SC_LAUNCH_SD
    return sc_check_launch("sc_hk_step (separable/diagonal fast path)");
}

// KS time steps per visit (the caller has validated: separable potential, diagonal widths, 16 < D <= 64, tiled blocks, flags
// present): hk_modes_multi_kernel<KS>, then the block kernel with KS sub-steps per trajectory.  KS = 2 is sc_hk_step_multi's
// launch, with its own labels and NR = 2 (D <= 32, intermediate stores) as well; KS = 3, 4 exist for the store-free scheme only.
template <int KS>
static int launch_step_sd_visit(const StepArgs &a, const sc_multi_scratch &ms, hipStream_t s) {
    constexpr bool pair = KS == 2;
    const int D = a.st.dim, nr = (D + 15) / 16, grid = sc_step_grid(a.st.n, D);
    ModesMultiArgs mm{ms.work, ms.qp_mid, ms.act_mid};
    hipLaunchKernelGGL(hk_modes_multi_kernel<KS>, dim3(grid), dim3(256), 0, s, a, mm);
    int rc = sc_check_launch(pair ? "sc_hk_step_multi (modes)" : "sc_hk_step_visit (modes)");
    if (rc) return rc;
    MultiArgs ma{ms.work, ms.c2_mid, ms.sgn_mid, ms.unrepaired};
#define SC_LAUNCH_VISIT(NR_, OCC_) hipLaunchKernelGGL((hk_step_sd_kernel<NR_, OCC_, true, true, KS>), dim3(grid), dim3(256), 0, s, a, ma)
    switch (nr < (pair ? 2 : 3) ? 0 : nr) {
        case 2: if constexpr (pair) SC_LAUNCH_VISIT(2, 4); break;
        case 3: SC_LAUNCH_VISIT(3, 4); break;
        case 4:
#ifdef SC_TUNING
            if constexpr (pair) {
                if (const char *occ_env = getenv("SC_SD_OCC")) {
                    if (atoi(occ_env) == 3) { SC_LAUNCH_VISIT(4, 3); break; }
                    if (atoi(occ_env) == 2) { SC_LAUNCH_VISIT(4, 2); break; }
                }
            }
#endif
            SC_LAUNCH_VISIT(4, 4); break;
        default:
            return pair ? sc_fail(SC_ERR_UNSUPPORTED, "sc_hk_step_multi: D = %d", D)
                        : sc_fail(SC_ERR_UNSUPPORTED, "sc_hk_step_visit: %d steps per visit at D = %d", KS, D);
    }
#undef SC_LAUNCH_VISIT
    return sc_check_launch(pair ? "sc_hk_step_multi (two steps per visit)" : "sc_hk_step_visit (KS steps per visit)");
}

// sc_hk_step_multi: ksteps = 2, sc_hk_step_visit: two to four
int sc_launch_step_sd_multi(const StepArgs &a, const sc_multi_scratch &ms, int ksteps, hipStream_t s) {
    switch (ksteps) {
        case 2: return launch_step_sd_visit<2>(a, ms, s);
        case 3: return launch_step_sd_visit<3>(a, ms, s);
        case 4: return launch_step_sd_visit<4>(a, ms, s);
        default: return sc_fail(SC_ERR_UNSUPPORTED, "sc_hk_step_visit: %d steps per visit", ksteps);
    }
}

#ifdef LU_PIVOT_CLOCK
extern "C" int sc_lu_pivot_clock(unsigned long long *buf) {       // device buffer of 64 * 64 * 4 time stamps, or NULL to switch off
    return hipMemcpyToSymbol(HIP_SYMBOL(g_lu_clock), &buf, sizeof(buf)) == hipSuccess ? 0 : -3;
}
#endif

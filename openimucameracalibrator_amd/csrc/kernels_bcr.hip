// Block cyclic reduction (nested dissection in time) of the damped LM system -- the
// O(log n)-depth replacement of the panel-sequential band sweep for the
// SPARSE_NORMAL_CHOLESKY step of ceres::Solve [EXT] (called at
// spline_trajectory_estimator.impl.h:272).
//
// The band (half bandwidth hb <= 64, knots in time order) is cut into n blocks of 64
// columns, which makes it block tridiagonal; the arrow rows (T_i_c, gravity, line delay,
// biases, intrinsics) and the right-hand side ride along as dense border rows.
//
//   level l (stride s = 2^l): the active blocks are o, o + s, o + 2 s, ... (m of them); an ODD m makes every block at an EVEN
//   position a pivot -- both ends included: ceil(m / 2) pivots, an independent set of the chain --, an even m every block at an odd
//   position (bcr_plan below; origin, stride and parity reach the kernels as launch arguments).  All pivots of a level are eliminated
//   concurrently, THROUGH THE EXPLICIT INVERSE of the pivot's 64 x 64 diagonal block (round 3): only that block is factored in one
//   workgroup, the pivot's border rows become matrix products on other CUs and the back substitution a matrix-vector product
//   (bcri_* kernels below).  A pivot at an end has one neighbour only: the Schur groups of the missing side leave at once and the
//   back substitution masks that side's rows of T.
//   After floor(log2 n) levels one block is alone (block 13 of 29; block 0 when n is a power of two): its workgroup also factors the
//   arrow corner, solves it and does the back substitution of the top level's one or two pivots, which then runs two levels per
//   launch in reverse.  (Until the end blocks became pivots only the odd positions were, block 0 stood until the end and the depth
//   was ceil(log2 n) + 1 inversions: one more whenever n is no power of two.  The distributed reduction keeps that order.)
//
// The LAST launch of a whole-band solve -- the back substitution that ends at level 0 -- also retracts: its workgroups hold every entry
// of the step in LDS when they store it, so the candidate parameters x (+) scale .* step and the step's three scalars (LmState) are
// written there, with the functions lm_retract_kernel uses (lm_retract.h), and the step costs one dependent launch fewer
// (launch_bcr_solve's retraction request; bcr_retract_* below).  Plans of fewer than three levels (n < 8 blocks: their last launch is
// the one-level kernel or the last block's), the distributed reduction and scaled steps (line search) keep lm_retract_kernel.
//
// History: rounds 1-2 factored each pivot WITH its 138 + a border rows in one workgroup (solver_algorithm 2) and round 3 added a
// parallel form of that (algorithm 3: every block a pivot at every level); both stayed in the library as independent solvers
// until round 4 removed them (three kernels, ten instantiations: git history) -- the band sweep (kernels_cholesky.hip, algorithm 1)
// is the independent solver the tests compare with.
#include <hip/hip_runtime.h>
#include <mutex>
#include <unordered_map>
#include "oicc_device.h"
#include "lm_decide.h"
#include "lm_launch.h"
#include "lm_retract.h"
#include "bcr_chain_body.h"
#include "../../include/oicc_hip.h"

namespace oicc {


struct BcrArgs {
  double* D;    // [n][64*64]   diagonal blocks, column major (c*64 + r), lower part used
  double* F;    // [n][64*a1]   border rows (arrow + rhs), column major (c*a1 + q)
  double* S;    // couplings, 64*64 each, PIVOT major: Q[c*64 + r] = A(pivot var c, neighbour var r)
  double* Lf;   // [n][Ru*64]   factor rows of each pivot, row major: L_ii (diag slot = 1/L_ii), left, right, border
  double* Mc;   // [a1*a1]      arrow corner (full symmetric), target of the border Schur updates
  double* x;    // [Pb + a]     solution
  int32_t* fail;
  long long* prof;   // optional cycle counters of block 0 / wave 0 (debug)
  int n, a, Pb, rtf, LD;
  int delay;                   // debug: panel waves > 0 sleep this many x ~1000 cycles before they read a panel (makes that hazard deterministic)
  // This level of the plan (bcr_plan): the active blocks are o + k s, k < m; block k is a pivot iff k mod 2 == p.  The couplings the
  // level writes are stored pivot major for the NEXT level, whose parity is pn.  The plan travels in the kernel arguments: a table
  // on the device would put a dependent global load at the head of every launch of a solve.
  int o, s, p, m, pn;
  int64_t offS_in, offS_out;   // first coupling of this level / of the next one
  int carry;                   // distributed reduction: m if the last active block is no pivot at this level (its coupling to the ghost block moves on), else 0
  int last;                    // bcri_invert_kernel<LAST>: the block that is left when every level is done
  // A top level of two pivots (three active blocks): both update the last block's D, F and the corner, and two atomic additions
  // land in either order.  With side != 0 the pivot left of the last block writes its updates with plain stores into the factor rows
  // of the last block (never a pivot: [D part 64*64 | F part 64*a1 | corner part a1*a1] fits its (192 + a1) * 64 doubles) and the
  // last block's workgroup adds them when it loads: a solve of three blocks stays reproducible bit by bit, as it was when every
  // level of it had one pivot.
  int side;
  int top_l, top_r;            // bcri_invert_kernel<LAST>: the pivots of the top level left / right of `last` (-1: none), whose back substitution that workgroup does as well
  // Distributed reduction (round 6, launch_bcr_dist_*): this system is the block range [b0, b0 + n) of a longer band.  `ghost`: the
  // range has a right neighbour outside -- the first block of the next rank's range -- which is never a pivot here: it sits at
  // storage index n (D, F start at zero and collect this range's Schur updates for its owner; x holds its solution for the back
  // substitution), it is the right neighbour of whichever local block is the last active one, and the coupling to it is always
  // stored local-variable major.  b0 = 0, ghost = 0: the whole band, as before.
  int b0, ghost;
  const LmCtl* ctl;            // device-side LM control (oicc_device.h): every kernel returns at once when the loop is done
};
#define BCR_RETURN_IF_DONE(A) do { if ((A).ctl != nullptr && (A).ctl->done != 0) return; } while (0)

__device__ __forceinline__ void bcr_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// (bcr_wave_sync, bcr_readlane: bcr_chain_body.h)
typedef double bcr_v4d __attribute__((ext_vector_type(4)));
typedef double bcr_v2d __attribute__((ext_vector_type(2)));

// lower-triangular tile index 0..9 -> (xt >= yt) in a 4x4 tile grid
__device__ __forceinline__ void tri10(int t, int& xt, int& yt) {
  xt = t < 1 ? 0 : (t < 3 ? 1 : (t < 6 ? 2 : 3));
  yt = t - (xt * (xt + 1)) / 2;
}

// Arrow corner (a x a, with the rhs as row / column a) held as Cq(r, c) = C[c*LD + r]: Cholesky, forward and backward
// substitution; the arrow part of the step lands in da[0..a).  ONE WAVE, lane = row (a + 1 <= 64): per column the pivot comes
// by v_readlane, the rank-1 update of the remaining columns runs over LDS without a workgroup barrier (round 2 spent three
// 1024-thread barriers per column here).  Called by all threads; ends with a workgroup barrier.
// idle: what the other waves do meanwhile (bcri_last_backward_kernel issues loads there: nothing they hold is live in wave 0's branch).
struct BcrNoIdle { __device__ __forceinline__ void operator()() const {} };
template <int LD, class Idle = BcrNoIdle>
__device__ __forceinline__ void bcr_corner_solve(double* C, double* da, int* failp, int a, int tid, int wave, int lane, Idle idle = Idle()) {
  const int a1 = a + 1;
  if (a1 <= 16) {
    // up to 15 arrow columns (T_i_c, gravity, line delay: 9-10): the columns stay in registers -- per column the pivot chain of
    // the panel factorisation and v_readlane broadcasts instead of a read-modify-write of LDS per remaining column; LDS only
    // transposes the factor for the back substitution
    if (wave == 0) {
      double av[16], dinv = 0.0;
#pragma unroll
      for (int c = 0; c < 16; ++c) av[c] = (c < a && lane < a1 && lane >= c) ? C[c * LD + lane] : 0.0;
      bool bad = false;
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        if (c < a) {
          const double piv = bcr_readlane(av[c], c);
          bad |= !(piv > 0.0);
          const double y0 = __builtin_amdgcn_rsq(piv);
          const double g0 = piv * y0, h0 = 0.5 * y0;
          const double r0 = fma(-g0, h0, 0.5);
          const double g1 = fma(g0, r0, g0), h1 = fma(h0, r0, h0);
          const double r1 = fma(-g1, h1, 0.5);
          const double u = (av[c] + av[c]) * h1;
          const double l = fma(u, r1, u);
          av[c] = l;
          if (lane == c) { const double y1 = h1 + h1; dinv = fma(y1, r1, y1); }
#pragma unroll
          for (int c2 = c + 1; c2 < 16; ++c2) {
            const double lc2 = bcr_readlane(l, c2);
            av[c2] = fma(-l, lc2, av[c2]);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < 16; ++c) if (c < a && lane < a1 && lane >= c) C[c * LD + lane] = av[c];
      double lt[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) lt[q] = (q < a && lane < q) ? C[lane * LD + q] : 0.0;      // L(q, lane)
      double z = lane < a ? C[lane * LD + a] : 0.0, xq_mine = 0.0;                               // L(a, lane): the forward-substituted rhs
#pragma unroll
      for (int q = 15; q >= 0; --q) {
        if (q < a) {
          const double xq = bcr_readlane(z * dinv, q);
          if (lane == q) xq_mine = xq;
          z = fma(-lt[q], xq, z);
        }
      }
      if (lane < a) da[lane] = xq_mine;
      if (bad && lane == 0) *failp = 1;
    } else idle();
    __syncthreads();
    return;
  }
  if (wave == 0) {
    bool bad = false;
    for (int c = 0; c < a; ++c) {
      double* col = C + c * LD;
      const double mine = lane < a1 ? col[lane] : 0.0;
      double piv = bcr_readlane(mine, c);
      if (!(piv > 0.0)) { bad = true; piv = 1.0; }
      const double d = sqrt(piv);
      const double l = lane == c ? d : (lane > c ? mine / d : 0.0);
      if (lane >= c && lane < a1) col[lane] = l;
      for (int c2 = c + 1; c2 < a; ++c2) {
        const double l2 = bcr_readlane(l, c2);
        if (lane >= c2 && lane < a1) C[c2 * LD + lane] -= l * l2;
      }
    }
    if (bad && lane == 0) *failp = 1;
    // back substitution of the corner, lane = arrow column: z_q = Cq(a, q), L_c^T x_a = z
    double z = lane < a ? C[lane * LD + a] : 0.0;
    const double dc = lane < a ? 1.0 / C[lane * LD + lane] : 0.0;
    double xq_mine = 0.0;
    for (int q = a - 1; q >= 0; --q) {
      const double xq = bcr_readlane(z * dc, q);
      if (lane == q) xq_mine = xq;
      const double l = lane < q ? C[lane * LD + q] : 0.0;    // L_c(q, lane)
      z = fma(-l, xq, z);
    }
    if (lane < a) da[lane] = xq_mine;
  } else idle();
  __syncthreads();
}

// =====================================================================================================================
// Cyclic reduction through the INVERSE of the pivot blocks (round 3, solver_algorithm 4).
//
// The levels above spend their time in ONE workgroup per pivot that factors D_i with its 128 + a1 border rows hanging
// below the panel (202 rows x 64 columns through one CU's LDS and MFMA pipe, 58 register tiles).  Only the 64 x 64
// diagonal block is inherently serial.  Here a level is
//   bcri_invert_kernel   one workgroup per pivot: right-looking Cholesky of [D_i ; I] (128 rows, 20 tiles), which leaves
//                        X = L^-T below the factor, then Z_i = X X^T = D_i^-1 on MFMA               -> global
//   bcri_schur_kernel    12 + 3 rtf workgroups per pivot: T = B Z_i for one 16-row tile of the border rows B = [S_left ;
//                        S_right ; arrow rows ; rhs] (kept for the back substitution), then the Schur tiles -T B^T onto
//                        the neighbours, their coupling, the arrow rows and the corner
//   bcri_backward_kernel x_i = T_rhs - T_left^T x_il - T_right^T x_ir - T_arrow^T x_arrow: a matrix-vector product, no
//                        triangular solve on the way back
//   bcri_invert_schur_kernel   the first two in ONE launch where a level's Schur workgroups fit the chip at once (bcr_level_joined):
//                        every workgroup of a pivot factors D_i itself and forms its tile T_x = (B_x X) X^T from X = L^-T in LDS, no Z_i
//   bcri_last_backward_kernel  the last block and the back substitution of the level below the top one in ONE launch where the
//                        pairing of levels would leave that level alone (bcr_fold_level): one workgroup per pivot of the level
//                        repeats the last block's work and finds its neighbours' x in its own LDS
// Error: forward errors of B D^-1 B^T through the explicit inverse and through the Cholesky factor are both
// O(cond(D_i) eps); the LM tests hold both to the oracle's steps.
// =====================================================================================================================
constexpr int kBackWaves = 8;   // waves of a back-substitution workgroup (one level alone: bcri_backward_kernel)
constexpr int kInvWaves = 16;   // (measured: 13.3 us per pivot against 14.5 with 8 waves, 17 with 4)
constexpr int kInvLD = 145;   // 128 rows, + 16 (two panels' rows of one wave land in different banks; they hold kInvDgRow's copy), + 1
constexpr int kInvMsDoubles = 3 * kChainStripDoubles;   // multiplier strips of the three panel waves, a strip per column of a panel (bcr_chain_body.h); the tail's x0s (256)
constexpr int kInvDgRow = 128;   // rows 128..143 of the columns j0..j0 + 15: the copy of a panel's diagonal tile the panel waves read (bcri_invert_body)

// Z tile (xt, yt), xt >= yt, of X X^T: X(r, k) = 0 for k < r, the sum starts at the tile of the later rows
template <int XT>
__device__ __forceinline__ bcr_v4d bcri_z_tile(const double* W, int yt, int li, int lq) {
  constexpr int LD = kInvLD, K0 = 4 * XT, NK = 16 - K0;
  const double* py = W + lq * LD + 64 + 16 * yt + li;
  const double* px = W + lq * LD + 64 + 16 * XT + li;
  double vy[NK], vx[NK];
#pragma unroll
  for (int kk = 0; kk < NK; ++kk) { vy[kk] = py[4 * (K0 + kk) * LD]; vx[kk] = px[4 * (K0 + kk) * LD]; }
  asm volatile("" ::: "memory");   // (every load above is issued before the first MFMA)
  bcr_v4d g = {0.0, 0.0, 0.0, 0.0}, g2 = {0.0, 0.0, 0.0, 0.0};   // (two accumulators: the dependent chain is NK / 2 MFMAs)
#pragma unroll
  for (int kk = 0; kk < NK; kk += 2) {
    g = __builtin_amdgcn_mfma_f64_16x16x4f64(vy[kk], vx[kk], g, 0, 0, 0);
    g2 = __builtin_amdgcn_mfma_f64_16x16x4f64(vy[kk + 1], vx[kk + 1], g2, 0, 0, 0);
  }
  g += g2;
  return g;   // g[r] <-> (x row 16 XT + li, y row 16 yt + lq + 4 r)
}

// ---- the back substitution of ONE pivot of a level: x_i = T_rhs - T_left^T x_il - T_right^T x_ir - T_arrow^T x_arrow ----
// Run by bcri_backward_kernel (a level alone in its launch) and by bcri_last_backward_kernel (the level below the top one, inside the
// last block's launch): the same rows, the same eight partial sums over the rows w + 8 k in k order, added in the order w = 0..7 -- the
// same bits from the same inputs.  Only where the neighbours' x and the arrow part are read differs (BcrBackX: LDS either way, staged
// from A.x by the one, left there by the last block's own work in the other).
constexpr int kBackRows = 192 / kBackWaves;   // rows of T per wave
struct BcrBackX {
  const double* xl; const double* xr; const double* xa;   // x of the left / right neighbour (64 each), of the arrow (a)
  bool hasL, hasR;                                         // a missing side reads as zeros
  __device__ __forceinline__ double at(int r, int a) const {
    return r < 64 ? (hasL ? xl[r] : 0.0) : (r < 128 ? (hasR ? xr[r - 64] : 0.0) : (r < 128 + a ? xa[r - 128] : 0.0));
  }
};
// wave w of eight issues its rows of T (Tg: the pivot's rows, behind its Z) and, w == 0, the rhs row
__device__ __forceinline__ void bcri_back_rows(const double* Tg, int a, bool hasL, bool hasR, int w, int lane, double (&lv)[kBackRows], double& yv) {
#pragma unroll
  for (int k = 0; k < kBackRows; ++k) {
    const int r = w + kBackWaves * k;
    const bool ok = r < 128 + a && (hasL || r >= 64) && (hasR || r < 64 || r >= 128);
    lv[k] = ok ? Tg[r * 64 + lane] : 0.0;
  }
  yv = w == 0 ? Tg[(128 + a) * 64 + lane] : 0.0;
}
// Called by every thread of the workgroup (one workgroup barrier inside); `active`: the eight waves w = 0..7 that hold the rows.
// part: [kBackWaves][64] of LDS.  Wave w == 0 returns x_i of column `lane`.
__device__ __forceinline__ double bcri_back_body(const double (&lv)[kBackRows], double yv, const BcrBackX& X, int a, double* part, bool active, int w, int lane) {
  if (active) {
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < kBackRows; ++k) { const int r = w + kBackWaves * k; sum = fma(lv[k], X.at(r, a), sum); }
    part[w * 64 + lane] = sum;
  }
  __syncthreads();
  double acc = 0.0;
  if (active && w == 0) {
#pragma unroll
    for (int ww = 0; ww < kBackWaves; ++ww) acc += part[ww * 64 + lane];
  }
  return yv - acc;
}

// What follows the factorisation of [D_i ; I] (all waves, after a workgroup barrier): Z = X X^T, and for the last block (LAST) the arrow
// corner and the first back substitution.  ZLDS (bcri_invert_schur_kernel): no Z at all -- the workgroup goes on with ONE Schur group
// of its pivot and forms that group's tile T_x = (B_x X) X^T from X, which stays in rows 64..127 of W (bcri_tx_stage); only the
// failure report is left here.
// FOLD (bcri_last_backward_kernel; with LAST): the launch has one workgroup per pivot of the level below the top one, whose plan
// fields are A.o, A.s, A.p, A.m.  Every workgroup does the last block's work with identical bits and then the back substitution of
// its own pivot from LDS; only workgroup 0 stores what they all share and raises A.fail.
template <bool LAST, bool ZLDS, bool FOLD>
__device__ __forceinline__ void bcri_tail(const BcrArgs& A, double* W, double* da, int* failp, const double* Fs, const double* Cs, double* Zg, int tid, int wave, int lane, bool report, double* x0s) {
  static_assert(!FOLD || LAST, "the folded level follows the last block");
  static_assert(!ZLDS || !LAST, "the last block keeps Z");
  if (ZLDS) {   // (failp: final behind the factorisation's last barrier)
    if (report && tid == 0 && *failp) atomicOr(A.fail, 1);
    return;
  }
  constexpr int LD = kInvLD, NW = kInvWaves, NT = 64 * NW, FLD = 65;
  const int li = lane & 15, lq = lane >> 4;
  const int a = A.a, a1 = a + 1;
  const bool shared_writer = !FOLD || blockIdx.x == 0;
  // rows of T of the top level's pivots: [0..4) the rows against the last block and [4..8) the arrow rows of the pivot right of it
  // (whose left neighbour it is: rows 0..63 of T), [8..16) the same of the pivot left of it (rows 64..127); wave 0 / 1 their rhs row.
  // Final since the top level's launch ended.  Issued HERE, ahead of Z = X X^T, which is longer than a global round trip, and not at
  // the head of the kernel: they are 34 registers, which the panel chain needs for the multipliers of its deferred updates.
  double ttop[16], ytop = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) ttop[k] = 0.0;
  if (LAST && (A.top_l >= 0 || A.top_r >= 0)) {
    const int64_t ru64 = (int64_t)(192 + a1) * 64;
    const double* Tr = A.Lf + (A.top_r >= 0 ? A.top_r : 0) * ru64 + 4096;
    const double* Tl = A.Lf + (A.top_l >= 0 ? A.top_l : 0) * ru64 + 4096;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = wave + NW * k;
      if (A.top_r >= 0) { ttop[k] = Tr[r * 64 + lane]; if (r < A.a) ttop[4 + k] = Tr[(128 + r) * 64 + lane]; }
      if (A.top_l >= 0) { ttop[8 + k] = Tl[(64 + r) * 64 + lane]; if (r < A.a) ttop[12 + k] = Tl[(128 + r) * 64 + lane]; }
    }
    if (wave == 0 && A.top_r >= 0) ytop = Tr[(128 + A.a) * 64 + lane];
    if (wave == 1 && A.top_l >= 0) ytop = Tl[(128 + A.a) * 64 + lane];
    asm volatile("" ::: "memory");   // (issued here, used after the corner: the loads must not sink to their use)
  }
  // ---- Z = X X^T (X = L^-T in rows 64..127): to global, or (LAST) into rows 0..63, where the factor is no longer needed
  // (tile t on wave t puts 28 / 24 / 16 / 12 of the 80 MFMAs on the four SIMDs -- the waves w, w + 4, w + 8, w + 12 share one -- and a
  // table that puts 20 on each was measured without gain: DESIGN §8-1)
  for (int t = wave; t < 10; t += NW) {
    int xt, yt; tri10(t, xt, yt);
    const bcr_v4d g = xt == 0 ? bcri_z_tile<0>(W, yt, li, lq) : (xt == 1 ? bcri_z_tile<1>(W, yt, li, lq) : (xt == 2 ? bcri_z_tile<2>(W, yt, li, lq) : bcri_z_tile<3>(W, yt, li, lq)));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int x = 16 * xt + li, y = 16 * yt + lq + 4 * r;
      if (LAST) { W[y * LD + x] = g[r]; if (xt != yt) W[x * LD + y] = g[r]; }
      else { Zg[y * 64 + x] = g[r]; if (xt != yt) Zg[x * 64 + y] = g[r]; }
    }
  }
  __syncthreads();
  if (!LAST) {
    if (report && tid == 0 && *failp) atomicOr(A.fail, 1);
    return;
  }
  // ---------------- LAST: T = F_0 Z into rows 64.. (T(q, c) = W[c*LD + 64 + q]; X is no longer needed)
  const int rtf = A.rtf;
  if (wave < 4 * rtf) {
    const int t = wave >> 2, w = wave & 3;
    const double* pf = Fs + lq * FLD + 16 * t + li;
    const double* pz = W + lq * LD + 16 * w + li;
    double vf[16], vz[16];
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) { vf[kk] = pf[4 * kk * FLD]; vz[kk] = pz[4 * kk * LD]; }
    asm volatile("" ::: "memory");   // (every load above is issued before the first MFMA)
    bcr_v4d tq = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) tq = __builtin_amdgcn_mfma_f64_16x16x4f64(vf[kk], vz[kk], tq, 0, 0, 0);
    // tq[r] <-> (column 16 w + li, border row 16 t + lq + 4 r)
#pragma unroll
    for (int r = 0; r < 4; ++r) W[(16 * w + li) * LD + 64 + 16 * t + lq + 4 * r] = tq[r];
  }
  __syncthreads();
  // corner Cq(r, c) = Mc - T F_0^T at W[c*LD + r] (rows 0..63: the inverse is no longer needed), lower tiles t1 >= t2
  if (wave < (rtf * (rtf + 1)) / 2) {
    int t1 = 0, u = wave; while (u >= t1 + 1) { u -= t1 + 1; ++t1; }
    const int t2 = u;
    const double* pt = W + lq * LD + 64 + 16 * t1 + li;
    const double* pf = Fs + lq * FLD + 16 * t2 + li;
    double vt[16], vf[16];
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) { vt[kk] = pt[4 * kk * LD]; vf[kk] = pf[4 * kk * FLD]; }
    asm volatile("" ::: "memory");   // (every load above is issued before the first MFMA)
    bcr_v4d g = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) g = __builtin_amdgcn_mfma_f64_16x16x4f64(vf[kk], vt[kk], g, 0, 0, 0);
    // g[r] <-> (row q1 = 16 t1 + li, column q2 = 16 t2 + lq + 4 r); Cs: the corner (+ the side buffer's corner part), parked when the kernel started
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int q1 = 16 * t1 + li, q2 = 16 * t2 + lq + 4 * r; if (q1 < a1 && q2 < a1) W[q2 * LD + q1] = Cs[q1 * a1 + q2] - g[r]; }
  }
  // FOLD: this workgroup's pivot of the level below the top one.  Its rows of T (stored two launches ago) are issued when the corner
  // solve starts, by the waves NW - 8 .. NW - 1, which idle through it: the corner solve, x_last and the top level stand between issue
  // and use, and nothing of it is live in wave 0's branch (with the rows in the waves 0..7 the kernel went to scratch there: 24 doubles
  // on top of the 16 of the top level and the corner's own 16 columns).  Wave NW - 8 + w does what wave w of bcri_backward_kernel does.
  double lv[kBackRows], yv = 0.0;
#pragma unroll
  for (int k = 0; k < kBackRows; ++k) lv[k] = 0.0;
  constexpr int BW0 = NW - kBackWaves;
  int fi = 0; bool f_hasL = false, f_hasR = false;
  if (FOLD) {
    const int kp = 2 * (int)blockIdx.x + A.p;
    fi = A.o + kp * A.s; f_hasL = kp > 0; f_hasR = kp < A.m - 1;
  }
  __syncthreads();
  bcr_corner_solve<LD>(W, da, failp, a, tid, wave, lane, [&]() {
    if (FOLD && wave >= BW0) {
      bcri_back_rows(A.Lf + (int64_t)fi * (192 + a1) * 64 + 4096, a, f_hasL, f_hasR, wave - BW0, lane, lv, yv);
      asm volatile("" ::: "memory");   // (issued here: the loads must not sink to their use)
    }
  });
  if (shared_writer) for (int q = tid; q < a; q += NT) A.x[A.Pb + q] = da[q];
  if (wave == 0) {
    const double* tc = W + lane * LD + 64;
    double v = tc[a];
    for (int q = 0; q < a; q += 8) {            // eight loads in flight before the dependent sum
      double t8[8], d8[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) { const bool ok = q + k < a; t8[k] = ok ? tc[q + k] : 0.0; d8[k] = ok ? da[q + k] : 0.0; }
#pragma unroll
      for (int k = 0; k < 8; ++k) v = fma(-t8[k], d8[k], v);
    }
    const int gi = A.last * 64 + lane;
    if (shared_writer && gi < A.Pb) A.x[gi] = v;
    x0s[lane] = gi < A.Pb ? v : 0.0;
  }
  __syncthreads();
  if (shared_writer && tid == 0 && *failp) atomicOr(A.fail, 1);
  if (A.top_l >= 0 || A.top_r >= 0) {
    // the pivots of the top level (one: right of the last block; two: the ends of three active blocks), whose only neighbour is the
    // last block: x = T_rhs - T_nb^T x_last - T_arrow^T x_arrow; their rows of T were loaded when the kernel started
    double sum_r = 0.0, sum_l = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = wave + NW * k;
      const double xn = x0s[r], xa = r < a ? da[r] : 0.0;
      sum_r = fma(ttop[k], xn, sum_r);     sum_r = fma(ttop[4 + k], xa, sum_r);
      sum_l = fma(ttop[8 + k], xn, sum_l); sum_l = fma(ttop[12 + k], xa, sum_l);
    }
    W[wave * 64 + lane] = sum_r;            // (W is free: 2 x NW x 64 partial sums)
    W[(NW + wave) * 64 + lane] = sum_l;
    __syncthreads();
    if (wave < 2) {
      const int blk = wave == 0 ? A.top_r : A.top_l;
      double acc = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) acc += W[(wave * NW + w) * 64 + lane];
      const int gi = blk * 64 + lane;
      const bool ok = blk >= 0 && gi < A.Pb;
      if (shared_writer && ok) A.x[gi] = ytop - acc;
      if (FOLD) x0s[64 * (1 + wave) + lane] = ok ? ytop - acc : 0.0;   // (x0s has 256 doubles: x_last, x of top_r, x of top_l)
    }
    if (FOLD) {
      // every neighbour of a pivot of this level is an active block of the top level: the last block or one of the top pivots
      __syncthreads();
      auto x_of = [&](int blk) -> const double* { return blk == A.last ? x0s : (blk == A.top_r ? x0s + 64 : x0s + 128); };
      BcrBackX X;
      X.hasL = f_hasL; X.hasR = f_hasR; X.xl = x_of(fi - A.s); X.xr = x_of(fi + A.s); X.xa = da;
      const double xv = bcri_back_body(lv, yv, X, a, W + 2 * NW * 64, wave >= BW0, wave - BW0, lane);   // (W: behind the top level's partial sums)
      const int gi = fi * 64 + lane;
      if (wave == BW0 && gi < A.Pb) A.x[gi] = xv;
    }
  }
}


// LAST: the block left after the last level -- the inverse stays in LDS, T = F Z, the arrow corner minus T F^T, its solution and
// x = T_rhs - T_arrow^T x_arrow, all in this workgroup
// park (bcri_invert_schur_kernel): called once by every thread between the LDS fill of D_i and the first barrier -- the global loads
// the caller issued before this function have landed with D_i's by then (one round trip for both), and what it writes behind `Fs`
// is visible after the factorisation
// shadow (bcri_invert_schur_kernel): called with p - 1 by the waves that run no chain while the panel waves run the chain of panel
// p = 1..3 -- the columns of panel p - 1 are final then; it holds no barrier
struct BcrNoPark { __device__ __forceinline__ void operator()(double*) const {} };
struct BcrNoShadow { __device__ __forceinline__ void operator()(int) const {} };
template <bool LAST, bool PROF, bool ZLDS = false, bool FOLD = false, class LoadD, class Park = BcrNoPark, class Shadow = BcrNoShadow>
__device__ __forceinline__ void bcri_invert_body(const BcrArgs& A, const int i, LoadD load_d, const bool report = true, Park park = Park(), Shadow shadow = Shadow()) {
  constexpr int LD = kInvLD, NW = kInvWaves, NT = 64 * NW, NTILE = 20, SLOTS = (NTILE + NW - 1) / NW, RU = 128, NAW = 3, FLD = 65;
  static_assert(NW == 16, "the corner phases of block 0 take one tile per wave");
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  double* const W = lds;                 // [64][LD] column major: rows 0..63 D_i -> L, rows 64..127 I -> L^-T
  double* const da = W + 64 * LD;        // [64] arrow solution (LAST)
  int* const failp = reinterpret_cast<int*>(da + 64);
  double* const ms = da + 64 + 8;        // [NAW][kChainStripDoubles] multiplier strips of the panel waves (below); the tail's x0s (256 doubles); 16-byte aligned
  static_assert(kInvMsDoubles >= NAW * kChainStripDoubles && (kChainStripDoubles * 8) % 16 == 0 && kInvMsDoubles >= 256 && ((64 * LD + 64 + 8) * 8) % 16 == 0, "ms");
  double* const Fs = ms + kInvMsDoubles;           // LAST: [64][FLD] border rows of block 0, Fs[k * FLD + q]; ZLDS: the caller's parked border tiles and Ts
  double* const Cs = Fs + 64 * FLD;      // LAST: [a1][a1] the arrow corner (+ the side buffer's corner part), as A.Mc is laid out
  const int a1 = A.a + 1;
  double* Zg = A.Lf + (int64_t)i * (192 + a1) * 64;
  const double* Fg = A.F + (int64_t)i * 64 * a1;
  const double* Sf = (LAST && A.side != 0) ? Zg + 4096 : nullptr;   // (BcrArgs::side: the F part)
  const double* Sm = (LAST && A.side != 0) ? Zg + 4096 + 64 * a1 : nullptr;   // (the corner part)
  const bool prof = PROF && A.prof != nullptr && blockIdx.x == 0 && wave == 0;
  long long pc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long tprev = prof ? clock64() : 0;
#define BCR_MARK(k) do { if (PROF && prof) { const long long tn_ = clock64(); pc[k] += tn_ - tprev; tprev = tn_; } } while (0)
  if (tid == 0) *failp = 0;
  {
    constexpr int PER = 4096 / NT;
    double gd[PER], gf[PER], gc[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int e = tid + k * NT;
      gd[k] = load_d(e);
      if (LAST) { const int c = e >> 6, q = e & 63; gf[k] = q < a1 ? Fg[c * a1 + q] + (Sf != nullptr ? Sf[c * a1 + q] : 0.0) : 0.0; }
      // the corner: final since the top level's launch ended, so it travels with D and F and no load stands behind the T F^T product
      if (LAST) gc[k] = e < a1 * a1 ? A.Mc[e] + (Sm != nullptr ? Sm[e] : 0.0) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int e = tid + k * NT;
      const int c = e >> 6, r = e & 63;
      W[c * LD + r] = r >= c ? gd[k] : 0.0;
      if (c < 16 && r < 16) W[c * LD + kInvDgRow + r] = r >= c ? gd[k] : 0.0;
      W[c * LD + 64 + r] = r == c ? 1.0 : 0.0;
      if (LAST) Fs[c * FLD + r] = gf[k];
      if (LAST && e < a1 * a1) Cs[e] = gc[k];
    }
    park(Fs);
  }
  __syncthreads();
  // ---- static tile ownership: tiles 0..9 the lower triangle of D_i, 10..19 the upper triangle of X (X(r, c) = 0 for c < r)
  int t_rt[SLOTS], t_ct[SLOTS]; bool t_ok[SLOTS];
  bcr_v4d acc[SLOTS];
#pragma unroll
  for (int k = 0; k < SLOTS; ++k) {
    const int t = wave + NW * k;
    t_ok[k] = t < NTILE;
    int xt, yt; tri10(t < 10 ? t : (t < NTILE ? t - 10 : 0), xt, yt);
    if (t < 10) { t_rt[k] = xt; t_ct[k] = yt; } else { t_rt[k] = 4 + yt; t_ct[k] = xt; }
    const double* src = W + (16 * t_ct[k] + lq) * LD + 16 * t_rt[k] + li;
    acc[k][0] = src[0]; acc[k][1] = src[4 * LD]; acc[k][2] = src[8 * LD]; acc[k][3] = src[12 * LD];
  }
  BCR_MARK(0);
  // Panels of 16 columns = one tile column (four LDS round trips and eight barriers per block instead of eight and sixteen).
  // Panel waves: lanes 0..15 the panel's diagonal rows (redundantly in every panel wave), lanes 16..63 one row each.
  // The diagonal rows are read from a COPY of the diagonal tile (wave 0 overwrites the tile in W while the waves 1, 2 may still read),
  // which lives in the padding rows of the panel's own columns -- DG(c, r) = W[(j0 + c) * LD + kInvDgRow + r] -- so that all lanes
  // load with ONE stride and the sixteen loads take immediate offsets.  Its upper triangle is a zero IN LDS (the fill; the write-back
  // of the trailing update), and the rows of the lanes that are not active are loaded as they are: nothing reads what those lanes
  // compute -- v_readlane takes lanes 0..15 only and the store leaves them out --, so the chain carries no select at all.
  const int prow = 16 + wave * 48 + (lane - 16);
  for (int p = 0; p < 4; ++p) {
    const int j0 = 16 * p;
    if (wave < NAW) {
      const int rho = lane < 16 ? j0 + lane : prow;
      // rows of X below the panel's last column are still zero
      const bool act = lane < 16 || (rho >= j0 + 16 && rho < RU && !(rho >= 64 && rho - 64 > j0 + 15));
      if (A.delay > 0 && wave > 0) for (int k = 0; k < A.delay; ++k) __builtin_amdgcn_s_sleep(16);
      // (the compiler pairs the sixteen loads into eight ds_read2_b64, whose 8-bit offsets take a base address per pair)
      const double* colp = W + j0 * LD + (lane < 16 ? kInvDgRow + lane : (act ? rho : 0));
      double av[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) av[c] = colp[c * LD];
      if (PROF && prof) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
      BCR_MARK(6);
      // The chain: bcr_chain_panel (bcr_chain_body.h) under the table kChainSchedule (bcr_chain_schedule.h).  Per column the dependent
      // sequence pivot -> rsq -> two Goldschmidt steps -> l -> v_readlane hop onto the next column, and in the gaps between its steps
      // seven or eight of the panel's 105 deferred updates av[c2] = fma(-l(k), m(k, c2), av[c2]), whose multipliers m(k, c2) are read
      // back as LDS broadcasts from column k's strip -- every column of a panel has a strip of its own, every lane stores.
      // ONE failure test per panel: a pivot that is not positive makes rsq NaN (negative, NaN) or inf (zero), so g0 = piv * y0, h1 and
      // with them l are NaN in every lane; every later column of the panel takes an update with l and is NaN as well, its pivot
      // included.  So !(pivot of column 15 > 0) is true exactly for the panels in which !(pivot > 0) holds at some column.
      // The arithmetic and its order per entry are unchanged: av[c2] takes the updates of the columns 0 .. c2 - 1 in that order.
      const bool bad = bcr_chain_panel<kChainSchedule>(av, ms + wave * kChainStripDoubles + lane, ms + wave * kChainStripDoubles);
      if (PROF && prof) { asm volatile("s_nop 0" :: "v"(av[15])); }
      BCR_MARK(7);
      if (act && (lane >= 16 || wave == 0)) {
        double* cp = W + j0 * LD + rho;
#pragma unroll
        for (int c = 0; c < 16; ++c) cp[c * LD] = av[c];
      }
      if (bad && lane == 0) *failp = 1;
    } else if (ZLDS && p > 0) {
      shadow(p - 1);
    }
    BCR_MARK(1);
    bcr_lds_barrier();
    BCR_MARK(2);
    if (p < 3) {
#pragma unroll
      for (int k = 0; k < SLOTS; ++k) {
        // tiles right of the panel; an X tile whose rows start below the panel's last column has a zero operand
        if (t_ok[k] && t_ct[k] > p && (t_rt[k] < 4 || t_rt[k] - 4 <= p)) {
          const double* pa = W + (j0 + lq) * LD + 16 * t_ct[k] + li;
          const double* pb = W + (j0 + lq) * LD + 16 * t_rt[k] + li;
          double va[4], vb[4];
#pragma unroll
          for (int kq = 0; kq < 4; ++kq) { va[kq] = pa[4 * kq * LD]; vb[kq] = -pb[4 * kq * LD]; }
#pragma unroll
          for (int kq = 0; kq < 4; ++kq) acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(va[kq], vb[kq], acc[k], 0, 0, 0);
          if (t_ct[k] == p + 1) {   // the next panel's columns go back to LDS
            double* dst = W + (16 * t_ct[k] + lq) * LD + 16 * t_rt[k] + li;
            dst[0] = acc[k][0]; dst[4 * LD] = acc[k][1]; dst[8 * LD] = acc[k][2]; dst[12 * LD] = acc[k][3];
            if (t_rt[k] == t_ct[k]) {   // the panel waves' copy of the diagonal tile: its lower triangle, zeros above (column lq + 4 r, row li)
              double* dd = W + (16 * t_ct[k] + lq) * LD + kInvDgRow + li;
              dd[0] = li >= lq ? acc[k][0] : 0.0; dd[4 * LD] = li >= lq + 4 ? acc[k][1] : 0.0; dd[8 * LD] = li >= lq + 8 ? acc[k][2] : 0.0; dd[12 * LD] = li >= lq + 12 ? acc[k][3] : 0.0;
            }
          }
        }
      }
    }
    BCR_MARK(3);
    bcr_lds_barrier();
    BCR_MARK(4);
  }
  BCR_MARK(4);
  bcri_tail<LAST, ZLDS, FOLD>(A, W, da, failp, Fs, Cs, Zg, tid, wave, lane, report, ms);
  BCR_MARK(5);
  if (PROF && prof && lane == 0) for (int k = 0; k < 8; ++k) A.prof[k] = pc[k];
#undef BCR_MARK
}

template <bool LAST, bool PROF>
__global__ __launch_bounds__(64 * kInvWaves) void bcri_invert_kernel(BcrArgs A) {
  BCR_RETURN_IF_DONE(A);
  const int i = LAST ? A.last : A.o + A.s * (2 * (int)blockIdx.x + A.p);
  const double* Dg = A.D + (int64_t)i * 4096;
  const double* Sd = (LAST && A.side != 0) ? A.Lf + (int64_t)i * (192 + A.a + 1) * 64 : nullptr;   // (BcrArgs::side)
  bcri_invert_body<LAST, PROF>(A, i, [Dg, Sd](int e) { double v = Dg[e]; if (LAST && Sd != nullptr && (e & 63) >= (e >> 6)) v += Sd[e]; return v; });
}

// The last block AND the back substitution of the level below the top one in ONE launch (bcr_fold_level): one workgroup per pivot of
// that level (2 to 4).  Every x such a pivot needs -- the last block's, the top pivots', the arrow part -- is produced by the last
// block's workgroup and sits in its LDS, so every workgroup repeats that work on a compute unit that would idle (identical bits: the
// same loads, the same arithmetic) and goes on with its own pivot.  Nothing is handed from one workgroup to another -- no flag, no
// poll, no wait --, and every global word has one writer: workgroup 0 for what they share, workgroup b for x of pivot b.
// A.o, A.s, A.p, A.m: the folded level; A.last, A.top_l, A.top_r, A.side as for bcri_invert_kernel<true, ...>.
__global__ __launch_bounds__(64 * kInvWaves) void bcri_last_backward_kernel(BcrArgs A) {
  BCR_RETURN_IF_DONE(A);
  const int i = A.last;
  const double* Dg = A.D + (int64_t)i * 4096;
  const double* Sd = A.side != 0 ? A.Lf + (int64_t)i * (192 + A.a + 1) * 64 : nullptr;   // (BcrArgs::side)
  bcri_invert_body<true, false, false, true>(A, i, [Dg, Sd](int e) { double v = Dg[e]; if (Sd != nullptr && (e & 63) >= (e >> 6)) v += Sd[e]; return v; });
}

// ---- one Schur group of a pivot: (16-row tile x of the border rows, up to four column tiles y) ----
// Run by bcri_schur_kernel (one workgroup of 4 waves per group, Z_i read from global memory, where bcri_invert_kernel left it) and by
// bcri_invert_schur_kernel (every workgroup of a pivot factors D_i itself): the same decoding, the same update stage -T_x B_y^T with
// the same stores and atomics.  The tile T_x = B_x Z_i is B_x (X X^T) in the one (the T stage of bcri_schur_body) and (B_x X) X^T in the other
// (bcri_tx_stage): equal up to rounding, not bit for bit.
struct BcrSchurGroup {
  int k, i, irs;                 // position among the active blocks, block, where the right neighbour's D / F live
  bool hasL, hasR, ghostR;       // (a pivot at position 0 -- odd number of active blocks -- has no left neighbour; ghostR: the right neighbour is the next rank's first block)
  int xk, xt, yk, ny;            // row tile (kind xk: 0 left, 1 right, 2 arrow rows / rhs; index xt), column tiles (kind yk, ny of them)
  bool store_t;                  // this group stores its rows of T
  bool leaves;                   // the pivot has no neighbour on a side the group works on
};
__device__ __forceinline__ BcrSchurGroup bcri_schur_group(const BcrArgs& A, int g, int piv) {
  BcrSchurGroup G;
  const int rtf = A.rtf;
  G.k = 2 * piv + A.p;
  G.i = A.o + G.k * A.s;
  G.hasL = G.k > 0;
  G.ghostR = A.ghost != 0 && G.k == A.m - 1;
  G.hasR = G.k < A.m - 1 || G.ghostR;
  G.irs = G.ghostR ? A.n : G.i + A.s;
  if (g < 4) { G.xk = 0; G.xt = g; G.yk = 0; G.ny = g + 1; G.store_t = true; }
  else if (g < 8) { G.xk = 1; G.xt = g - 4; G.yk = 0; G.ny = 4; G.store_t = false; }
  else if (g < 12) { G.xk = 1; G.xt = g - 8; G.yk = 1; G.ny = G.xt + 1; G.store_t = true; }
  else { g -= 12; G.yk = g / rtf; G.xt = g - G.yk * rtf; G.xk = 2; G.ny = G.yk < 2 ? 4 : G.xt + 1; G.store_t = G.yk == (G.hasL ? 0 : 1); }   // (the arrow rows of T: once per pivot)
  G.leaves = ((G.xk == 1 || G.yk == 1) && !G.hasR) || ((G.xk == 0 || G.yk == 0) && !G.hasL);
  return G;
}
// The MFMA operands of a group, element kk of a lane's sixteen: B_x (row 16 xt + li, pivot variable 4 kk + lq), Z (column 16 wave + li,
// the same variable), B_y (row 16 wave + li, the same variable), T_x (row li, the same variable).  kTStage: bcri_schur_body forms
// T_x = B_x Z itself, in Ts.  From global memory ...
struct BcrSchurGlobalOps {
  static constexpr bool kTStage = true;
  static constexpr bool kLateY = false;   // (B_y is in flight with B_x and Z: one global round trip)
  const double *px, *pz, *py; int sx, sy; bool okx, oky;
  __device__ __forceinline__ double x(int kk) const { return px[4 * kk * sx]; }
  __device__ __forceinline__ double z(int kk) const { return pz[4 * kk * 64]; }
  __device__ __forceinline__ double y(int kk) const { return oky ? py[4 * kk * sy] : 0.0; }
  __device__ __forceinline__ double t(const double (*Ts)[68], int kk, int li, int lq) const { return Ts[li][4 * kk + lq]; }
};
// ... or from LDS (bcri_invert_schur_kernel): the border tiles are parked as [pivot variable][16 rows] with zeros where a row lies
// beyond the arrow; T_x was formed by bcri_tx_stage (below), which reads B_x itself and needs no Z, and is read as the sum of its
// partial tiles TP
struct BcrSchurLdsOps {
  static constexpr bool kTStage = false;
  static constexpr bool kLateY = true;    // (an LDS read: B_y is loaded behind T, 32 registers fewer where 1024 threads leave 128)
  const double *py, *TP;
  __device__ __forceinline__ double y(int kk) const { return py[64 * kk]; }
  __device__ __forceinline__ double t(const double (*)[68], int kk, int li, int lq) const;   // (behind bcri_tx_at)
};
__device__ __forceinline__ int bcri_schur_trow0(const BcrSchurGroup& G) { return G.xk == 0 ? 16 * G.xt : (G.xk == 1 ? 64 + 16 * G.xt : 128 + 16 * G.xt); }
// A group runs in two stages with a workgroup barrier between them: the T stage leaves the tile T_x = B_x Z_i in LDS and (store_t) in
// the pivot's rows of T, the update stage forms -T_x B_y^T and adds or stores it.  bcri_schur_kernel runs both here; the joined kernel
// (Ops::kTStage false) has run bcri_tx_stage with its barriers and bcri_tx_store, and runs the update stage alone.
// Called by every thread of the workgroup; `active`: this wave is one of the group's four, `wave` its index among them.
template <class Ops>
__device__ __forceinline__ void bcri_schur_body(const BcrArgs& A, const BcrSchurGroup& G, double (*Ts)[68], const Ops& ops, const bool active, const int wave, const int lane) {
  const int li = lane & 15, lq = lane >> 4;
  const int a1 = A.a + 1, s = A.s;
  const int k = G.k, i = G.i, il = i - s, irs = G.irs, xk = G.xk, xt = G.xt, yk = G.yk, ny = G.ny;
  const bool hasL = G.hasL, ghostR = G.ghostR;
  double vy[16];
  // ---- T stage
  if constexpr (Ops::kTStage) {
    const bool store_t = G.store_t, okx = ops.okx;
    double* Tg = A.Lf + (int64_t)i * (192 + a1) * 64 + 4096;
    double vx[16], vz[16];
    if (active) {
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) { vx[kk] = ops.x(kk); vz[kk] = ops.z(kk); }
      if (!Ops::kLateY) {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) vy[kk] = ops.y(kk);
      }
      asm volatile("" ::: "memory");   // (every load above is issued before the first MFMA)
      // T(x rows, columns 16 wave ..) = B_x Z: two accumulators, the dependent chain is 8 MFMAs
      bcr_v4d tq = {0.0, 0.0, 0.0, 0.0}, tq2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < 16; kk += 2) {
        tq = __builtin_amdgcn_mfma_f64_16x16x4f64(okx ? vx[kk] : 0.0, vz[kk], tq, 0, 0, 0);
        tq2 = __builtin_amdgcn_mfma_f64_16x16x4f64(okx ? vx[kk + 1] : 0.0, vz[kk + 1], tq2, 0, 0, 0);
      }
      tq += tq2;
      // tq[r] <-> (column 16 wave + li, row lq + 4 r of the tile)
      const int trow0 = bcri_schur_trow0(G);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = lq + 4 * r;
        Ts[row][16 * wave + li] = tq[r];
        if (store_t && (xk != 2 || 16 * xt + row < a1)) Tg[(int64_t)(trow0 + row) * 64 + 16 * wave + li] = tq[r];
      }
    }
    __syncthreads();
  }
  // ---- update stage
  if (!active || wave >= ny) return;
  const int yt = wave;
  // orientation of the new coupling (il, ir): il is at position kn of the next level, whose pivots have parity pn
  const int kn = hasL ? (k - 2 + A.p) / 2 : 0;
  const bool il_is_pivot = (kn & 1) == A.pn;
  const bool swap = xk == 1 && yk == 0 && !il_is_pivot && !ghostR;
  double vt[16];
  if (Ops::kLateY) {
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) vy[kk] = ops.y(kk);
  }
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) vt[kk] = ops.t(Ts, kk, li, lq);
  asm volatile("" ::: "memory");   // (every load above is issued before the first MFMA)
  bcr_v4d gq = {0.0, 0.0, 0.0, 0.0}, gq2 = {0.0, 0.0, 0.0, 0.0};
  if (swap) {
#pragma unroll
    for (int kk = 0; kk < 16; kk += 2) {
      gq = __builtin_amdgcn_mfma_f64_16x16x4f64(vt[kk], vy[kk], gq, 0, 0, 0);
      gq2 = __builtin_amdgcn_mfma_f64_16x16x4f64(vt[kk + 1], vy[kk + 1], gq2, 0, 0, 0);
    }
  } else {
#pragma unroll
    for (int kk = 0; kk < 16; kk += 2) {
      gq = __builtin_amdgcn_mfma_f64_16x16x4f64(vy[kk], vt[kk], gq, 0, 0, 0);
      gq2 = __builtin_amdgcn_mfma_f64_16x16x4f64(vy[kk + 1], vt[kk + 1], gq2, 0, 0, 0);
    }
  }
  gq += gq2;
  // not swapped: gq[r] <-> (x row li, y row lq + 4 r); swapped: (y row li, x row lq + 4 r)
  const int ils = hasL ? il : i;
  double* Dl = A.D + (int64_t)ils * 4096; double* Dr = A.D + (int64_t)irs * 4096;
  double* Fl = A.F + (int64_t)ils * 64 * a1; double* Fr = A.F + (int64_t)irs * 64 * a1;
  double* So = A.S + (A.offS_out + kn) * 4096;
  // (two-pivot top level: the updates of the pivot left of the last block go to the side buffer, see BcrArgs::side)
  const bool to_side = A.side != 0 && !hasL;
  double* Sd = A.Lf + (int64_t)irs * (192 + a1) * 64;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double v = -gq[r];
    if (xk == 1 && yk == 0) {
      if (!swap) { const int x = 16 * xt + li, y = 16 * yt + lq + 4 * r; So[y * 64 + x] = v; }    // Q[c = il var][r = ir var]
      else       { const int y = 16 * yt + li, x = 16 * xt + lq + 4 * r; So[x * 64 + y] = v; }    // Q[c = ir var][r = il var]
    } else if (xk < 2) {
      const int x = 16 * xt + li, y = 16 * yt + lq + 4 * r;
      if (to_side) { if (x >= y) Sd[y * 64 + x] = v; }
      else if (x >= y && v != 0.0) unsafeAtomicAdd((xk == 0 ? Dl : Dr) + y * 64 + x, v);
    } else if (yk < 2) {
      const int q = 16 * xt + li, y = 16 * yt + lq + 4 * r;
      if (to_side) { if (q < a1) Sd[4096 + y * a1 + q] = v; }
      else if (q < a1 && v != 0.0) unsafeAtomicAdd((yk == 0 ? Fl : Fr) + y * a1 + q, v);
    } else {
      const int q1 = 16 * xt + li, q2 = 16 * yt + lq + 4 * r;
      if (to_side) { if (q1 < a1 && q2 <= q1) { Sd[4096 + 64 * a1 + q1 * a1 + q2] = v; Sd[4096 + 64 * a1 + q2 * a1 + q1] = v; } }
      else if (q1 < a1 && q2 <= q1 && v != 0.0) {
        unsafeAtomicAdd(A.Mc + q1 * a1 + q2, v);
        if (q1 != q2) unsafeAtomicAdd(A.Mc + q2 * a1 + q1, v);
      }
    }
  }
}

// one workgroup (4 waves) per (pivot, group): Z_i from global memory
__global__ __launch_bounds__(256) void bcri_schur_kernel(BcrArgs A) {
  BCR_RETURN_IF_DONE(A);
  __shared__ double Ts[16][68];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  const int a1 = A.a + 1;
  if ((int)blockIdx.y == (int)gridDim.y - 1 && A.carry > 0) {
    // distributed reduction, odd number of active blocks: the last one is no pivot at this level, its coupling to the ghost block
    // moves on to the next level's table unchanged (the workgroups of this extra row of the grid copy it)
    const int m = A.carry;
    const double* src = A.S + (A.offS_in + (m - 1)) * 4096; double* dst = A.S + (A.offS_out + (m - 1) / 2) * 4096;
    for (int e = (int)blockIdx.x * 256 + tid; e < 4096; e += (int)gridDim.x * 256) dst[e] = src[e];
    return;
  }
  const BcrSchurGroup G = bcri_schur_group(A, (int)blockIdx.x, (int)blockIdx.y);
  if (G.leaves) return;
  const double* SL = A.S + (A.offS_in + (G.hasL ? G.k - 1 : 0)) * 4096;
  const double* SR = A.S + (A.offS_in + G.k) * 4096;
  const double* Fg = A.F + (int64_t)G.i * 64 * a1;
  const double* Zg = A.Lf + (int64_t)G.i * (192 + a1) * 64;
  // border rows as MFMA operands: element (row 16 t + li, pivot variable k = 4 kk + lq)
  auto border_ptr = [&](int kind, int t, int& stride, bool& ok) -> const double* {
    if (kind == 0) { stride = 64; ok = true; return SL + lq * 64 + 16 * t + li; }
    if (kind == 1) { stride = 64; ok = true; return SR + lq * 64 + 16 * t + li; }
    const int q = 16 * t + li; ok = q < a1; stride = a1; return Fg + lq * a1 + (ok ? q : 0);
  };
  BcrSchurGlobalOps ops;
  ops.px = border_ptr(G.xk, G.xt, ops.sx, ops.okx);
  ops.py = border_ptr(G.yk, wave < G.ny ? wave : 0, ops.sy, ops.oky);
  ops.pz = Zg + lq * 64 + 16 * wave + li;
  bcri_schur_body(A, G, Ts, ops, true, wave, lane);
}

// ---- T_x = (B_x X) X^T: the T stage of bcri_invert_schur_kernel, from X = L^-T (upper triangular, rows 64..127 of W), without Z ----
// A workgroup of that kernel needs ONE 16 x 64 tile T_x = B_x Z_i, not Z_i = X X^T (80 MFMAs on every one of a pivot's 15 workgroups, a
// barrier, then 16 dependent-pair MFMAs on each of four waves).  Both factors of (B_x X) X^T fall apart into ten chunks of 4 MFMAs
// (chunk t <-> tri10(t) = (p, q), q <= p).  A chunk of panel p needs the columns of panel p of X only, which are final when that
// panel has left the chain: the chunks of the panels 0..2 are formed while the panel waves run the next chain (bcri_tx_shadow), the
// four of panel 3 behind the factorisation, one per wave and SIMD (bcri_tx_stage):
//   Y chunk (p, q):  YP(p, q) = B_x[:, 16 q .. 16 q + 15] X[16 q .. 16 q + 15, panel p]        (X's tiles below the diagonal are zero: q <= p)
//   T chunk (p, i):  TP(p, i) = Y_p X[16 i .. 16 i + 15, panel p]^T,   Y_p = YP(p, 0) + ... + YP(p, p) summed in that order   (i <= p)
//   T_x[:, tile i] = TP(i, i) + ... + TP(3, i), summed in that order by whoever reads it (bcri_tx_at)
// The orders are fixed, so every workgroup of a pivot has the same bits of T_x.  It is another association of B_x X X^T than the
// two-launch route's B_x (X X^T): the joined kernel is held to the host solve's bounds, not to that route's bits.
// Partial tiles are 16 x 16, element (row, col) at [col * stride + row] with an odd stride (LD = 145 and 17 are both 17 mod 32: the
// stores of rows lq + 4 r at column li and the operand loads of row li at column 4 kk + lq both spread over the banks).  YP lives in
// rows 0..63 of W -- the factor L, which nothing reads behind the factorisation's last barrier --, tile t at columns 16 (t & 3), rows
// 16 (t >> 2); TP in an array of its own.  A non-positive pivot leaves NaN in X, hence in every YP, TP and update.
constexpr int kTxChunks = 10, kTxStride = 17, kTxTileDoubles = 16 * kTxStride;
__device__ __forceinline__ int bcri_tx_chunk(int p, int q) { return (p * (p + 1)) / 2 + q; }   // (tri10's inverse)
__device__ __forceinline__ double* bcri_tx_ytile(double* W, int t) { return W + 16 * (t & 3) * kInvLD + 16 * (t >> 2); }
// Called by every thread of the workgroup; two workgroup barriers inside, the second one behind the TP stores.
// T0: the first chunk that is left to do -- 6: panel 3's four, the others came from bcri_tx_shadow (0: all ten behind the factorisation,
// the form the shadow was measured against: DESIGN §8-1); chunk T0 + w on wave w.
template <int T0>
__device__ __forceinline__ void bcri_tx_stage(double* W, const double* P, double* TP, const int wave, const int lane) {
  constexpr int LD = kInvLD;
  const int li = lane & 15, lq = lane >> 4;
  const int chunk = wave + T0;
  int p, q; tri10(chunk < kTxChunks ? chunk : 0, p, q);
  if (chunk < kTxChunks) {
    const double* pb = P + (16 * q + lq) * 16 + li;               // B_x(row li, variable 16 q + 4 kk + lq)
    const double* px = W + (16 * p + li) * LD + 64 + 16 * q + lq;   // X(16 q + 4 kk + lq, column 16 p + li)
    double vb[4], vx[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) { vb[kk] = pb[64 * kk]; vx[kk] = px[4 * kk]; }
    asm volatile("" ::: "memory");   // (every load above is issued before the first MFMA)
    bcr_v4d y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) y = __builtin_amdgcn_mfma_f64_16x16x4f64(vb[kk], vx[kk], y, 0, 0, 0);
    // y[r] <-> (row lq + 4 r, column li of panel p)
    double* yp = bcri_tx_ytile(W, chunk) + li * LD + lq;
#pragma unroll
    for (int r = 0; r < 4; ++r) yp[4 * r] = y[r];
  }
  bcr_lds_barrier();
  if (chunk < kTxChunks) {
    const int i = q, c0 = bcri_tx_chunk(p, 0);
    const double* px = W + (16 * p + lq) * LD + 64 + 16 * i + li;   // X(row 16 i + li, column 16 p + 4 kk + lq)
    double yv[4][4], vx[4];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) {
      if (qq <= p) {   // (wave uniform)
        const double* yp = bcri_tx_ytile(W, c0 + qq) + lq * LD + li;   // YP(p, qq)(row li, column 4 kk + lq)
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) yv[qq][kk] = yp[4 * kk * LD];
      } else {
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) yv[qq][kk] = 0.0;
      }
    }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) vx[kk] = px[4 * kk * LD];
    asm volatile("" ::: "memory");   // (every load above is issued before the first sum)
    bcr_v4d t = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      double ys = yv[0][kk];
#pragma unroll
      for (int qq = 1; qq < 4; ++qq) if (qq <= p) ys += yv[qq][kk];
      t = __builtin_amdgcn_mfma_f64_16x16x4f64(ys, vx[kk], t, 0, 0, 0);
    }
    // t[r] <-> (row lq + 4 r, column li of tile i)
    double* tp = TP + chunk * kTxTileDoubles + li * kTxStride + lq;
#pragma unroll
    for (int r = 0; r < 4; ++r) tp[4 * r] = t[r];
  }
  bcr_lds_barrier();
}
// The chunks of the panel pp = 0..2 in the shadow of the chain of panel pp + 1 (bcri_invert_body's `shadow`): the columns of panel pp
// are final and thirteen waves wait for the panel waves.  ONE wave does a panel -- wave 3 + 4 pp: the waves 3, 7, 11 sit on the SIMD
// that holds no panel wave -- so Y_pp needs no workgroup barrier: it goes through the wave's own tile of LDS (the MFMA's output layout
// is not its operand layout) behind a wave-local wait.  The same sums in the same order as bcri_tx_stage<0>: YP(pp, q) from zero each,
// added in q order; TP(pp, i) from zero each.  YS: [3] tiles.
__device__ __forceinline__ void bcri_tx_shadow(const double* W, const double* P, double* TP, double* YS, const int pp, const int wave, const int lane) {
  constexpr int LD = kInvLD;
  if (wave != 3 + 4 * pp) return;
  const int li = lane & 15, lq = lane >> 4;
  double* ys = YS + pp * kTxTileDoubles;
  {
    const double* pb = P + lq * 16 + li;                           // B_x(row li, variable 16 q + 4 kk + lq)
    const double* px = W + (16 * pp + li) * LD + 64 + lq;          // X(16 q + 4 kk + lq, column 16 pp + li)
    double vb[3][4], vx[3][4];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) { vb[q][kk] = q <= pp ? pb[256 * q + 64 * kk] : 0.0; vx[q][kk] = q <= pp ? px[16 * q + 4 * kk] : 0.0; }
    }
    asm volatile("" ::: "memory");   // (every load above is issued before the first MFMA)
    bcr_v4d y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      if (q <= pp) {   // (wave uniform)
        bcr_v4d yq = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) yq = __builtin_amdgcn_mfma_f64_16x16x4f64(vb[q][kk], vx[q][kk], yq, 0, 0, 0);
        if (q == 0) y = yq; else y += yq;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) ys[li * kTxStride + lq + 4 * r] = y[r];   // y[r] <-> (row lq + 4 r, column li of panel pp)
  }
  bcr_wave_sync();
  {
    const double* px = W + (16 * pp + lq) * LD + 64 + li;          // X(row 16 i + li, column 16 pp + 4 kk + lq)
    double vy[4], vx[3][4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) vy[kk] = ys[(4 * kk + lq) * kTxStride + li];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) vx[i][kk] = i <= pp ? px[4 * kk * LD + 16 * i] : 0.0;
    }
    asm volatile("" ::: "memory");   // (every load above is issued before the first MFMA)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (i <= pp) {   // (wave uniform)
        bcr_v4d t = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) t = __builtin_amdgcn_mfma_f64_16x16x4f64(vy[kk], vx[i][kk], t, 0, 0, 0);
        double* tp = TP + bcri_tx_chunk(pp, i) * kTxTileDoubles + li * kTxStride + lq;
#pragma unroll
        for (int r = 0; r < 4; ++r) tp[4 * r] = t[r];
      }
    }
  }
}
// T_x(row, column 16 I + cl): the partial tiles of the panels I..3 in panel order
template <int I>
__device__ __forceinline__ double bcri_tx_sum(const double* TP, int row, int cl) {
  const double* tp = TP + cl * kTxStride + row;
  double v = tp[bcri_tx_chunk(I, I) * kTxTileDoubles];
#pragma unroll
  for (int p = I + 1; p < 4; ++p) v += tp[bcri_tx_chunk(p, I) * kTxTileDoubles];
  return v;
}
__device__ __forceinline__ double bcri_tx_at(const double* TP, int i, int row, int cl) {   // (i: uniform)
  return i == 0 ? bcri_tx_sum<0>(TP, row, cl) : (i == 1 ? bcri_tx_sum<1>(TP, row, cl) : (i == 2 ? bcri_tx_sum<2>(TP, row, cl) : bcri_tx_sum<3>(TP, row, cl)));
}
__device__ __forceinline__ double BcrSchurLdsOps::t(const double (*)[68], int kk, int li, int lq) const { return bcri_tx_at(TP, kk >> 2, li, 4 * (kk & 3) + lq); }
// the pivot's rows of T in global memory, as the T stage of bcri_schur_body stores them: wave w of four stores the column tile w
__device__ __forceinline__ void bcri_tx_store(const BcrArgs& A, const BcrSchurGroup& G, const double* TP, const int w, const int lane) {
  const int li = lane & 15, lq = lane >> 4;
  const int a1 = A.a + 1;
  double* Tg = A.Lf + (int64_t)G.i * (192 + a1) * 64 + 4096;
  const int trow0 = bcri_schur_trow0(G);
  double v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = bcri_tx_at(TP, w, lq + 4 * r, li);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = lq + 4 * r;
    if (G.xk != 2 || 16 * G.xt + row < a1) Tg[(int64_t)(trow0 + row) * 64 + 16 * w + li] = v[r];
  }
}

// A level in ONE launch: grid (12 + 3 rtf groups, pivots of the level), 16 waves.  EVERY workgroup of a pivot factors D_i itself --
// the factorisation is deterministic, all copies of X = L^-T are the same bits -- and then runs its Schur group on T_x = (B_x X) X^T
// from X in its own LDS (bcri_tx_stage): Z_i is never formed, no second launch, nothing handed from one workgroup to another (no flag,
// no poll, no wait).  The group's border tiles
// (one of B_x, up to four of B_y) do not depend on Z_i: their loads are issued with D_i's and parked in LDS behind the inversion's
// arrays, so no global round trip stands behind the inversion.  Groups of a side the pivot has no neighbour on leave at once.  For
// levels whose workgroups fit the chip at once (bcr_level_joined); level 0 is not among them while its inversions ride in the build
// launch, whose workgroups still write the blocks the Schur updates land on -- it is behind a plain build launch
// (bcr_level0_behind_build), where the reporting workgroup of a level-0 pivot raises the failure flag that build's thread 0 reset.
constexpr int kInvLdsDoubles = 64 * kInvLD + 64 + 8 + kInvMsDoubles;                 // W, da, failp, ms of bcri_invert_body
constexpr int kJoinLdsDoubles = kInvLdsDoubles + 5 * 1024 + (kTxChunks + 3) * kTxTileDoubles;       // + B_x tile, four B_y tiles ([64][16] each), the ten partial tiles of T_x, the shadow waves' Y tiles
__global__ __launch_bounds__(64 * kInvWaves) void bcri_invert_schur_kernel(BcrArgs A) {
  BCR_RETURN_IF_DONE(A);
  const BcrSchurGroup G = bcri_schur_group(A, (int)blockIdx.x, (int)blockIdx.y);
  if (G.leaves) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  const int a1 = A.a + 1;
  const double* SL = A.S + (A.offS_in + (G.hasL ? G.k - 1 : 0)) * 4096;
  const double* SR = A.S + (A.offS_in + G.k) * 4096;
  const double* Fg = A.F + (int64_t)G.i * 64 * a1;
  // thread -> element (pivot variable kv, row l of a 16-row tile) of each parked tile
  const int kv = tid >> 4, l = tid & 15;
  auto border_at = [&](int kind, int t) -> double {
    if (kind == 0) return SL[kv * 64 + 16 * t + l];
    if (kind == 1) return SR[kv * 64 + 16 * t + l];
    const int q = 16 * t + l; return q < a1 ? Fg[kv * a1 + q] : 0.0;
  };
  double bx = border_at(G.xk, G.xt), by[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) by[t] = t < G.ny ? border_at(G.yk, t) : 0.0;
  asm volatile("" ::: "memory");   // (issued here, with D_i's loads; parked in LDS before the first barrier of the inversion)
  const double* Dg = A.D + (int64_t)G.i * 4096;
  extern __shared__ __attribute__((aligned(16))) double lds_[];   // (bcri_invert_body's `lds`: W first; the parked tiles, TP and the shadow's Y tiles behind kInvLdsDoubles)
  const bool report = (int)blockIdx.x == (G.hasL ? 0 : 8);   // the pivot's first group that does not leave (left x left, or right x right)
  bcri_invert_body<false, false, true>(A, G.i, [Dg](int e) { return Dg[e]; }, report,
    [&](double* P) {
      P[tid] = bx;
#pragma unroll
      for (int t = 0; t < 4; ++t) P[1024 * (1 + t) + tid] = by[t];
    },
    [&](int pp) { bcri_tx_shadow(lds_, lds_ + kInvLdsDoubles, lds_ + kInvLdsDoubles + 5 * 1024, lds_ + kInvLdsDoubles + 5 * 1024 + kTxChunks * kTxTileDoubles, pp, wave, lane); });
  // (the factorisation ended with a workgroup barrier: X is in rows 64..127 of W, the parked tiles are visible)
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* W = lds;
  const double* P = lds + kInvLdsDoubles;
  double* TP = lds + kInvLdsDoubles + 5 * 1024;
  bcri_tx_stage<6>(W, P, TP, wave, lane);   // (panel 3's chunks: the panels 0..2 came in the shadow of the chains)
  // the waves 4..7 store the group's rows of T while the waves 0 .. ny - 1 run the update stage
  if (G.store_t && wave >= 4 && wave < 8) bcri_tx_store(A, G, TP, wave - 4, lane);
  const bool active = wave < 4;
  BcrSchurLdsOps ops;
  ops.TP = TP;
  ops.py = P + 1024 * (1 + (active && wave < G.ny ? wave : 0)) + lq * 16 + li;
  bcri_schur_body(A, G, nullptr, ops, active, wave, lane);
}

// ---- the retraction inside the LAST launch of a whole-band solve (lm_retract.h; used by the two-level back-substitution kernel) ----
// The workgroups that produce the step also retract with it: lm_retract_kernel's work without its launch.  Every tangent entry of the
// band has exactly one owner among the workgroups of the last launch (the ranges are stated at the two kernels); a parameter block
// belongs to the owner of its FIRST tangent entry, its other entries lie at most two further, inside a block whose solution an
// EARLIER launch wrote and the workgroup holds in LDS anyway.  So every step entry a workgroup retracts with is one it computed itself
// or one an earlier launch wrote: nothing another workgroup of the same launch writes is read -- no flag, no wait.  Workgroup 0 also
// owns the arrow entries (x_arrow is final since the last block's kernel).  The owned parameter blocks are found through the entry
// map (oicc_device.h: RetractReq); map, scale, D2, gradient and parameters are loaded before the first barrier, with the T rows.  One
// block reduction and one atomic per scalar and workgroup.
struct BcrOwn {
  int e = -1, code = -1;                 // this thread's tangent entry; kind and parameter offset of the block that starts there (lm_rmap_code), or -1
  double sc0 = 0.0, d2 = 0.0, g = 0.0;   // scale, D2, gradient of the entry
  const double* x = nullptr; double* xc = nullptr;
};
constexpr int kRetractPark = 12;         // doubles parked in LDS per owner: parameters [7], further scales [5]
// Thread tid < 64 NB takes entry 64 b_lo + tid of the blocks [b_lo, b_hi); in the arrow workgroup the next `a` threads take the arrow entries.
template <int NB>
__device__ __forceinline__ BcrOwn bcr_retract_claim(const BcrArgs& A, const RetractReq& R, const SolveBuffers& sb, int b_lo, int b_hi, bool arrow_wg, int tid) {
  BcrOwn o; o.x = R.x; o.xc = R.xc;
  NormalEq ne = R.ne;
  if (A.ctl != nullptr) { o.x = A.ctl->xp[0]; o.xc = A.ctl->xp[1]; ne.base = A.ctl->nep[0]; }
  const int e_hi = b_hi * 64 < A.Pb ? b_hi * 64 : A.Pb;
  if (tid < 64 * NB) { const int e = b_lo * 64 + tid; if (e < e_hi) o.e = e; }
  else if (tid < 64 * NB + A.a && arrow_wg) o.e = A.Pb + (tid - 64 * NB);
  if (o.e >= 0) { o.code = R.rmap[o.e]; o.sc0 = sb.scale[o.e]; o.d2 = sb.D2[o.e]; o.g = ne.g()[o.e]; }
  return o;
}
__device__ __forceinline__ int bcr_rm_steps(int kind) { return kind == kRmEucl ? 1 : (kind == kRmTic ? 6 : 3); }
__device__ __forceinline__ int bcr_rm_params(int kind) { return kind == kRmEucl ? 1 : (kind == kRmTic ? 7 : (kind == kRmSo3 || kind == kRmPt ? 4 : 3)); }
// the parameters and the further scales of the owned block: into LDS (rpark[c * stride + tid]), not into registers, until the step is there
__device__ __forceinline__ void bcr_retract_park(const SolveBuffers& sb, const BcrOwn& o, double* rpark, int stride, int tid) {
  if (o.code < 0) return;
  const int kind = o.code & 7; const int64_t po = o.code >> 3;
  const int nd = bcr_rm_steps(kind), np = bcr_rm_params(kind);
  for (int c = 0; c < np; ++c) rpark[c * stride + tid] = o.x[po + c];
  for (int c = 1; c < nd; ++c) rpark[(6 + c) * stride + tid] = sb.scale[o.e + c];
}
// Behind the workgroup's last store of the step.  xflat: the band part of the step in LDS, entry e at xflat[e - e_base]; xarrow: the
// arrow part.  red: 3 x 64 doubles of LDS nobody reads any more.  OW: the waves that hold owners.  Called by all threads.
template <int OW>
__device__ __forceinline__ void bcr_retract_finish(const BcrArgs& A, const RetractReq& R, const SolveBuffers& sb, const BcrOwn& o, const double* xflat, int e_base,
                                                   const double* xarrow, const double* rpark, int stride, double* red, int tid, int wave, int lane) {
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) {
    // "the solve is done" of the device-side loop: behind the barrier, so every wave of this workgroup has issued its stores of the
    // step -- the end of ONE workgroup's solve, no launch boundary any more (the others finish within the same launch)
    if (A.ctl != nullptr) { if (A.ctl->stamps != nullptr && A.ctl->seq < A.ctl->trace_cap) A.ctl->stamps[3 * A.ctl->seq + 1] = wall_clock64(); }
    else *R.ne.cost() = 0.0;   // (the host-driven loop: the cost slot is cleared for the candidate cost pass)
  }
  double step_sq = 0.0, x_sq = 0.0, model = 0.0;
  if (o.e >= 0) {
    auto step_at = [&](int e) { return e >= A.Pb ? xarrow[e - A.Pb] : xflat[e - e_base]; };
    model = lm_model_term(step_at(o.e), o.d2, o.g, o.sc0);
    if (o.code >= 0) {
      const int kind = o.code & 7;
      const double alpha = R.alpha;
      const int nd = bcr_rm_steps(kind), np = bcr_rm_params(kind);
      double d[6], sc[6], pv[7];
#pragma unroll
      for (int c = 0; c < 6; ++c) { d[c] = c < nd ? step_at(o.e + c) : 0.0; sc[c] = c == 0 ? o.sc0 : (c < nd ? rpark[(6 + c) * stride + tid] : 0.0); }
#pragma unroll
      for (int c = 0; c < 7; ++c) pv[c] = c < np ? rpark[c * stride + tid] : 0.0;
      double* out = o.xc + (o.code >> 3);
      if (kind == kRmSo3) lm_store_so3(lm_retract_so3(Quat{pv[0], pv[1], pv[2], pv[3]}, d, sc, alpha), pv, out, step_sq, x_sq);
      else if (kind == kRmEucl) lm_retract_eucl(pv[0], d[0], sc[0], alpha, out, step_sq, x_sq);
      else if (kind == kRmAb || kind == kRmGb) { const double bound = kind == kRmAb ? R.max_ab : R.max_gb; for (int c = 0; c < 3; ++c) lm_retract_box(pv[c], d[c], sc[c], alpha, bound, out + c, step_sq, x_sq); }
      else if (kind == kRmPt) lm_retract_point(pv, d, sc, alpha, out, step_sq, x_sq);
      else if (kind == kRmTic) lm_retract_tic(pv, d, sc, alpha, out, step_sq, x_sq);
    }
  }
  if (wave < OW) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { step_sq += __shfl_xor(step_sq, off); x_sq += __shfl_xor(x_sq, off); model += __shfl_xor(model, off); }
    if (lane == 0) { red[wave] = step_sq; red[64 + wave] = x_sq; red[128 + wave] = model; }
  }
  __syncthreads();
  if (tid < 3) {
    double acc = 0.0;
    for (int w = 0; w < OW; ++w) acc += red[64 * tid + w];
    unsafeAtomicAdd(tid == 0 ? &sb.st->step_norm_sq : (tid == 1 ? &sb.st->x_norm_sq : &sb.st->model_cost_change), acc);
  }
}

// back substitution of the pivots of one level: lane = column of T, the 128 + a rows spread over the waves
__global__ __launch_bounds__(64 * kBackWaves) void bcri_backward_kernel(BcrArgs A) {
  BCR_RETURN_IF_DONE(A);
  __shared__ double xs[192];
  __shared__ double part[kBackWaves][64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int a = A.a, a1 = a + 1, s = A.s;
  const int kp = 2 * (int)blockIdx.x + A.p;         // position among the active blocks
  const int i = A.o + kp * s, il = i - s;
  const bool hasL = kp > 0;
  const bool hasR = kp < A.m - 1 || A.ghost != 0;
  const int ir = kp < A.m - 1 ? i + s : A.n;        // (distributed reduction: the ghost block's solution sits behind the local blocks)
  double lv[kBackRows], yv;
  bcri_back_rows(A.Lf + (int64_t)i * (192 + a1) * 64 + 4096, a, hasL, hasR, wave, lane, lv, yv);
  double xin = 0.0;
  if (tid < 64) { const int gi = il * 64 + tid; xin = (hasL && gi < A.Pb) ? A.x[gi] : 0.0; }
  else if (tid < 128) { const int gi = ir * 64 + (tid - 64); xin = (hasR && gi < A.Pb) ? A.x[gi] : 0.0; }
  else if (tid < 128 + a) xin = A.x[A.Pb + (tid - 128)];
  if (tid < 192) xs[tid] = xin;
  __syncthreads();
  BcrBackX X;
  X.xl = xs; X.xr = xs + 64; X.xa = xs + 128; X.hasL = true; X.hasR = true;   // (a missing side was staged as zeros)
  const double xv = bcri_back_body(lv, yv, X, a, &part[0][0], true, wave, lane);
  const int gi = i * 64 + lane;
  if (wave == 0 && gi < A.Pb) A.x[gi] = xv;
}

// Two levels of the back substitution in one launch: a workgroup takes a pivot j of the upper level (stride 2 s) and then, eight
// waves each, its two neighbours j - s and j + s, which are pivots of the lower level (stride s) and need x_j -- it stays in LDS.
// Every row of T the three products read is in flight before the first barrier.  A (the plan fields o, s, p, m) describes the lower
// level; ou, pu, mu the upper one.  An upper pivot at an end may lack the child on that side.  An orphan -- a lower pivot at an end of
// the active blocks whose only neighbour is no pivot of the upper level (at most one per end) -- gets a workgroup of its own behind
// the others: orphan_l / orphan_r, its block, or -1.
//
// RETRACT (the levels (1, 0) as the last launch of a whole-band solve, s = 1; see the helpers above): the workgroup of the upper pivot j
// owns the blocks j - 2 .. j + 1 (upper pivots are four blocks apart), clipped to the band; the last upper pivot also takes block
// j + 2 when no right-end orphan stands there; an orphan's workgroup takes the orphan (left end) or the orphan and the block left of it
// (right end).  The children's solutions go to LDS as well as to global memory, for their owners.
template <bool RETRACT>
__device__ __forceinline__ void bcri_backward2_body(const BcrArgs& A, int ou, int pu, int mu, int npiv_upper, int orphan_l, int orphan_r, const RetractReq& R, const SolveBuffers& sb) {
  constexpr int NW = 16, RW1 = 192 / NW, RW2 = 192 / (NW / 2);
  __shared__ double xw[6][64];            // x of the blocks j - 2 s, j - s, j, j + s, j + 2 s (the children's rows only under RETRACT), the arrow part
  __shared__ double part[NW][64];
  double* const xs0 = xw[0]; double* const xs1 = xw[2]; double* const xs2 = xw[4]; double* const xs3 = xw[5];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int a = A.a, a1 = a + 1, s = A.s, n = A.n;
  const int64_t ru64 = (int64_t)(192 + a1) * 64;
  // an orphan's workgroup stands where the missing upper pivot j would be: right of the left-end orphan (its "right child"), left
  // of the right-end one (its "left child")
  const int lone_ix = (int)blockIdx.x - npiv_upper;
  const bool lone = lone_ix >= 0;
  const bool lone_l = lone && orphan_l >= 0 && lone_ix == 0, lone_r = lone && !lone_l;
  const int ku = 2 * (int)blockIdx.x + pu;                          // position of j among the upper level's active blocks
  const int j = lone_l ? orphan_l - s : (lone_r ? orphan_r + s : ou + ku * 2 * s);
  const int jl = j - 2 * s, jr = j + 2 * s;
  // (distributed reduction: a right neighbour beyond the local blocks is the ghost block, whose solution sits behind them)
  const bool ghost = A.ghost != 0;
  const bool has_jl = lone_r || (!lone && ku > 0);
  const bool has_jr = lone_l || (!lone && (ku < mu - 1 || ghost));
  const int jrs = (!lone && ku == mu - 1) ? n : jr;
  // lower pivots: half 0 = j - s (neighbours jl, j), half 1 = j + s (neighbours j, jr)
  const int half = wave >> 3, hw = wave & 7;
  const int ci = half == 0 ? j - s : j + s;
  const bool child = lone ? (half == 0 ? lone_r : lone_l) : (half == 0 ? ci >= A.o : ci <= A.o + (A.m - 1) * s);
  const bool child_hasL = half == 0 ? has_jl : !lone;
  const bool child_hasR = half == 0 ? (!lone || ghost) : has_jr;
  auto xin = [&](int blk, int r) { const int gi = blk * 64 + r; return gi < A.Pb ? A.x[gi] : 0.0; };
  if (tid < 64) xs0[tid] = has_jl ? xin(jl, tid) : 0.0;
  else if (tid < 128) xs2[tid - 64] = has_jr ? xin(jrs, tid - 64) : 0.0;
  else if (tid < 192) xs3[tid - 128] = tid - 128 < a ? A.x[A.Pb + (tid - 128)] : 0.0;
  else if (tid < 256 && lone) xs1[tid - 192] = (lone_r && ghost) ? xin(n, tid - 192) : 0.0;   // (in place of x_j: nothing, or the right-end orphan's ghost block)
  // ---- RETRACT: what this thread owns; its entry of the map, scale, D2 and gradient are loaded here, the parameters of the block
  // that starts at the entry behind the T rows (they need the map's answer), all of it before the first barrier
  __shared__ double rpark[RETRACT ? kRetractPark : 1][384];
  BcrOwn own;
  if (RETRACT) {
    // (j is virtual for an orphan's workgroup: -1 left of the band (owns block 0), n right of it (owns n - 2, n - 1); with it or an
    // upper pivot j = 0 the window's base (j - 2) * 64 is negative: only owned entries, all >= b_lo * 64, are ever looked up in xw[])
    const int b_lo = j - 2 > 0 ? j - 2 : 0;
    int b_hi = j + 2 < n ? j + 2 : n;
    if (!lone && (int)blockIdx.x == npiv_upper - 1 && orphan_r < 0) b_hi = n;   // (then n <= j + 3)
    own = bcr_retract_claim<5>(A, R, sb, b_lo, b_hi, blockIdx.x == 0, tid);
  }
  double l1[RW1], l2[RW2], y1 = 0.0, y2 = 0.0;
  {
    const double* T1 = A.Lf + (lone ? 0 : j) * ru64 + 4096;
#pragma unroll
    for (int k = 0; k < RW1; ++k) {
      const int r = wave + NW * k;
      const bool ok = !lone && r < 128 + a && (has_jl || r >= 64) && (has_jr || r < 64 || r >= 128);
      l1[k] = ok ? T1[r * 64 + lane] : 0.0;
    }
    if (wave == 0 && !lone) y1 = T1[(128 + a) * 64 + lane];
    const double* T2 = A.Lf + (child ? ci : 0) * ru64 + 4096;
#pragma unroll
    for (int k = 0; k < RW2; ++k) {
      const int r = hw + 8 * k;
      const bool ok = child && r < 128 + a && (child_hasL || r >= 64) && (child_hasR || r < 64 || r >= 128);
      l2[k] = ok ? T2[r * 64 + lane] : 0.0;
    }
    if (hw == 0 && child) y2 = T2[(128 + a) * 64 + lane];
  }
  if (RETRACT) bcr_retract_park(sb, own, &rpark[0][0], 384, tid);
  __syncthreads();
  if (!lone) {
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < RW1; ++k) {
      const int r = wave + NW * k;
      const double xv = r < 64 ? xs0[r] : (r < 128 ? xs2[r - 64] : (r < 128 + a ? xs3[r - 128] : 0.0));
      sum = fma(l1[k], xv, sum);
    }
    part[wave][lane] = sum;
    __syncthreads();
    if (wave == 0) {
      double acc = 0.0;
#pragma unroll
      for (int w = 0; w < NW; ++w) acc += part[w][lane];
      const double xv = y1 - acc;
      const int gi = j * 64 + lane;
      xs1[lane] = gi < A.Pb ? xv : 0.0;
      if (gi < A.Pb) A.x[gi] = xv;
    }
    __syncthreads();
  }
  {
    const double* xl = half == 0 ? xs0 : xs1;
    const double* xr = half == 0 ? xs1 : xs2;
    double sum = 0.0;
#pragma unroll
    for (int k = 0; k < RW2; ++k) {
      const int r = hw + 8 * k;
      const double xv = r < 64 ? xl[r] : (r < 128 ? xr[r - 64] : (r < 128 + a ? xs3[r - 128] : 0.0));
      sum = fma(l2[k], xv, sum);
    }
    part[wave][lane] = sum;
    __syncthreads();
    if (hw == 0 && child) {
      double acc = 0.0;
#pragma unroll
      for (int w = 0; w < 8; ++w) acc += part[8 * half + w][lane];
      const int gi = ci * 64 + lane;
      const double xv = y2 - acc;
      if (gi < A.Pb) A.x[gi] = xv;
      if (RETRACT) xw[half == 0 ? 1 : 3][lane] = gi < A.Pb ? xv : 0.0;
    }
  }
  if (RETRACT) bcr_retract_finish<6>(A, R, sb, own, &xw[0][0], (j - 2) * 64, xs3, &rpark[0][0], 384, &part[0][0], tid, wave, lane);
}
__global__ __launch_bounds__(1024) void bcri_backward2_kernel(BcrArgs A, int ou, int pu, int mu, int npiv_upper, int orphan_l, int orphan_r) {
  BCR_RETURN_IF_DONE(A);
  bcri_backward2_body<false>(A, ou, pu, mu, npiv_upper, orphan_l, orphan_r, RetractReq{}, SolveBuffers{});
}
__global__ __launch_bounds__(1024) void bcri_backward2_retract_kernel(BcrArgs A, int ou, int pu, int mu, int npiv_upper, int orphan_l, int orphan_r, RetractReq R, SolveBuffers sb) {
  BCR_RETURN_IF_DONE(A);
  bcri_backward2_body<true>(A, ou, pu, mu, npiv_upper, orphan_l, orphan_r, R, sb);
}

// ---- damped, scaled system in block form:  M = S H S + clamp(diag)/radius, rhs = -S g -----
__device__ __forceinline__ void bcr_build_body(const NormalEq& ne, const TangentLayout& tl, const SolveBuffers& sb, int reuse_diagonal, double min_diag,
                                               double max_diag, const BcrArgs& A, const int64_t tid, const int64_t nthreads) {
  const int Pb = tl.Pb, a = tl.a, W = tl.W, a1 = a + 1, hb = tl.hb, n = A.n;
  const int64_t r0 = (int64_t)A.b0 * 64;             // first band row of this system (distributed reduction: the rank's block range)
  const double radius = sb.radius;
  if (tid == 0) {   // results of the step that starts here
    sb.st->radius = radius; sb.st->model_cost_change = 0.0; sb.st->step_norm_sq = 0.0; sb.st->x_norm_sq = 0.0; sb.st->cand_cost = 0.0; sb.st->chol_failed = 0;
    if (sb.ctl != nullptr && sb.ctl->stamps != nullptr && sb.ctl->seq < sb.ctl->trace_cap) sb.ctl->stamps[3 * sb.ctl->seq] = wall_clock64();
  }
  auto damp = [&](int64_t i, double hii) -> double {
    const double sc = sb.scale[i];
    return (reuse_diagonal ? sb.diag[i] : fmin(fmax(hii * sc * sc, min_diag), max_diag)) / radius;
  };
  for (int64_t i = tid; i < tl.P; i += nthreads) {
    const double hii = i < Pb ? ne.band()[i * W] : ne.C()[(i - Pb) * a + (i - Pb)];
    const double sc = sb.scale[i];
    double d;
    if (!reuse_diagonal) { d = fmin(fmax(hii * sc * sc, min_diag), max_diag); sb.diag[i] = d; }
    else d = sb.diag[i];
    sb.D2[i] = d / radius;
  }
  // diagonal blocks (lower part) and level-0 couplings
  for (int64_t e = tid; e < (int64_t)n * 4096; e += nthreads) {
    const int blk = int(e >> 12), c = int(e >> 6) & 63, r = int(e) & 63;
    {
      const int64_t gc = r0 + (int64_t)blk * 64 + c, gr = r0 + (int64_t)blk * 64 + r;
      double v = 0.0;
      if (r >= c) {
        const int k = r - c;
        if (gr < Pb) {
          if (k <= hb) v = ne.band()[gc * W + k] * sb.scale[gc] * sb.scale[gr];
          if (k == 0) v += damp(gc, ne.band()[gc * W]);
        } else if (gc >= Pb && k == 0) v = 1.0;    // identity padding of the last block
      }
      A.D[e] = v;
    }
    if (blk < n - 1 || A.ghost != 0) {
      // coupling (blk, blk+1): the pivot of level 0 is the one of parity A.p (the ghost block behind the last local one never is)
      const bool right = (blk & 1) == A.p || blk == n - 1;   // pivot = blk, neighbour = blk+1 (its right)
      const int64_t gr = r0 + (int64_t)(blk + 1) * 64 + (right ? r : c);
      const int64_t gc = r0 + (int64_t)blk * 64 + (right ? c : r);
      const int64_t k = gr - gc;
      double v = 0.0;
      if (gr < Pb && k <= hb) v = ne.band()[gc * W + k] * sb.scale[gc] * sb.scale[gr];
      A.S[e] = v;
    }
  }
  // border rows: arrow + rhs
  for (int64_t e = tid; e < (int64_t)n * 64 * a1; e += nthreads) {
    const int64_t li = e / a1; const int q = int(e - li * a1); const int64_t gi = r0 + li;
    double v = 0.0;
    if (gi < Pb) v = q < a ? ne.Et()[(int64_t)q * Pb + gi] * sb.scale[gi] * sb.scale[Pb + q] : -ne.g()[gi] * sb.scale[gi];
    A.F[e] = v;
  }
  if (A.ghost != 0) {   // the ghost block collects this range's Schur updates for its owner: starts at zero
    for (int64_t e = tid; e < 4096; e += nthreads) A.D[(int64_t)n * 4096 + e] = 0.0;
    for (int64_t e = tid; e < (int64_t)64 * a1; e += nthreads) A.F[(int64_t)n * 64 * a1 + e] = 0.0;
  }
  // corner (same format as lm_build_kernel's Mc)
  for (int64_t e = tid; e < (int64_t)a1 * a1; e += nthreads) {
    const int r = int(e / a1), c = int(e - (int64_t)r * a1);
    double v = 0.0;
    if (A.b0 != 0) { sb.Mc[e] = 0.0; continue; }   // (distributed reduction: the corner itself enters on the rank of block 0, the others hold their Schur updates only)
    if (r < a && c < a) {
      v = ne.C()[r * a + c] * sb.scale[Pb + r] * sb.scale[Pb + c];
      if (r == c) v += damp(Pb + r, ne.C()[r * a + r]);
    } else if (r == a && c < a) v = -ne.g()[Pb + c] * sb.scale[Pb + c];
    else if (c == a && r < a) v = -ne.g()[Pb + r] * sb.scale[Pb + r];
    sb.Mc[e] = v;
  }
}

// device-side LM control: the system to build, its radius and the reuse-diagonal flag come from the control block -- as the host
// or an earlier kernel left it, or derived here from the previous iteration's state and results (lm_decide.h)
__device__ __forceinline__ bool lm_ctl_build_inputs(NormalEq& ne, SolveBuffers& sb, int& reuse_diagonal, bool writer) {
  if (sb.ctl == nullptr) return true;
  __shared__ LmCtl s_c;
  if (!lm_ctl_next_state(sb, writer, &s_c)) return false;
  ne.base = s_c.nep[0]; sb.radius = s_c.radius; reuse_diagonal = s_c.reuse_diagonal;
  return true;
}

__global__ void bcr_build_kernel(NormalEq ne, TangentLayout tl, SolveBuffers sb, int reuse_diagonal, double min_diag,
                                 double max_diag, BcrArgs A) {
  if (!lm_ctl_build_inputs(ne, sb, reuse_diagonal, blockIdx.x == 0 && threadIdx.x == 0)) return;
  bcr_build_body(ne, tl, sb, reuse_diagonal, min_diag, max_diag, A, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// The build and the first level's inversions in ONE launch (cyclic reduction through the inverses): the workgroups of the
// pivots of level 0 (parity A.p: floor or ceil of n / 2 blocks) take their D_i straight from the band of the normal equations -- same expressions as
// the build, which still writes every block for the later levels -- while the other workgroups build the system.
__global__ __launch_bounds__(64 * kInvWaves) void bcri_build_invert_kernel(NormalEq ne, TangentLayout tl, SolveBuffers sb, int reuse_diagonal,
                                                                           double min_diag, double max_diag, BcrArgs A) {
  const int npiv = (A.n + 1 - A.p) / 2;
  if (!lm_ctl_build_inputs(ne, sb, reuse_diagonal, (int)blockIdx.x == npiv && threadIdx.x == 0)) return;   // (the writer: thread 0 of the first build workgroup, which also resets LmState for this step)
  if ((int)blockIdx.x >= npiv) {
    bcr_build_body(ne, tl, sb, reuse_diagonal, min_diag, max_diag, A, (int64_t)((int)blockIdx.x - npiv) * blockDim.x + threadIdx.x, (int64_t)((int)gridDim.x - npiv) * blockDim.x);
    return;
  }
  const int i = 2 * (int)blockIdx.x + A.p;
  const int Pb = tl.Pb, Wd = tl.W, hb = tl.hb;
  const double radius = sb.radius;
  const double* band = ne.band();
  bcri_invert_body<false, false>(A, i, [&](int e) -> double {
    const int c = e >> 6, r = e & 63, k = r - c;
    const int64_t gc = (int64_t)(A.b0 + i) * 64 + c, gr = (int64_t)(A.b0 + i) * 64 + r;
    if (k < 0) return 0.0;
    if (gr >= Pb) return (gc >= Pb && k == 0) ? 1.0 : 0.0;   // identity padding of the last block
    const double sc = sb.scale[gc];
    double v = k <= hb ? band[gc * Wd + k] * sc * sb.scale[gr] : 0.0;
    if (k == 0) v += (reuse_diagonal ? sb.diag[gc] : fmin(fmax(band[gc * Wd] * sc * sc, min_diag), max_diag)) / radius;
    return v;
  }, false);   // the build workgroups of this launch reset the failure flag: a non-positive pivot here is not reported but poisons
               // (NaN) the inverse, the Schur complements of every later level and finally block 0, whose kernel reports it
}

// ---- host ------------------------------------------------------------------
// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (function, device): set once per pair, not once per solve
// (a solve is a dozen launches of ~10 us; the attribute calls were a measurable part of its host time)
static void bcr_allow_lds(const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::unordered_map<const void*, uint64_t> done;
  int dev = 0; (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  {
    std::lock_guard<std::mutex> lock(mu);
    uint64_t& mask = done[fn];
    if (dev < 64 && (mask & bit)) return;
    mask |= bit;
  }
  (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}


static inline int bcr_blocks(int Pb) { return (Pb + 63) / 64; }
static size_t bcr_lds_inv() { return (size_t)kInvLdsDoubles * sizeof(double); }
static int64_t bcr_coupling_slots(int nblk) { return 2 * (int64_t)nblk + 40; }   // the coupling tables of all levels (sum of active - 1 + ghost < 2 nblk) and of the one behind them
static void bcr_carve(BcrArgs& A, double* w, int nblk, int a1) {   // nblk: blocks incl. a ghost
  A.D = w; w += (int64_t)nblk * 4096;
  A.F = w; w += (int64_t)nblk * 64 * a1;
  A.S = w; w += bcr_coupling_slots(nblk) * 4096;
  A.Lf = w;
}
static int64_t bcr_carve_doubles(int nblk, int a1) { return (int64_t)nblk * 4096 + (int64_t)nblk * 64 * a1 + bcr_coupling_slots(nblk) * 4096 + (int64_t)nblk * (192 + a1) * 64 + 64; }
// Arrow limit: the kernels take up to 63 arrow columns (four 16-row border tiles).  Round 2 saw sporadic NaN pivots with more than
// two border tiles; the cause was the in-place read of the panel's diagonal block by waves that start a panel late (see the panel
// factorisation and tests/test_gpu_parity.py::test_bcr_wide_borders_and_the_panel_hazard, which makes it deterministic); with the
// copy of the diagonal tile (kInvDgRow) the limit is the kernels' own.
// (the limit travels with the problem: SolveBuffers::bcr_max_border, option bcr_max_border; the workspace is sized for the kernels' own limit)
bool bcr_applicable(const TangentLayout& tl) { return tl.Pb >= 1 && tl.hb <= 64 && tl.a + 1 <= 64; }
int64_t bcr_workspace_doubles(const TangentLayout& tl) {
  if (!bcr_applicable(tl)) return 0;
  const int64_t n = bcr_blocks(tl.Pb), a1 = tl.a + 1;
  return bcr_carve_doubles(int(n), int(a1));
}

// ---- the launch sequence in pieces (shared by the one-GPU solve and the distributed one) ----
// The elimination plan.  Level l: active blocks origin + k stride, k < active; the pivots are the positions of parity `parity` (an
// independent set of the block-tridiagonal chain).  An ODD number of active blocks takes the even positions, both ends included --
// ceil(m / 2) pivots, where the odd positions give (m - 1) / 2 and leave block 0 standing until the very end; an even number takes
// the odd positions.  The depth is floor(log2 n) + 1 inversions instead of ceil(log2 n) + 1 (the same for n a power of two, whose
// plan has parity 1 throughout).  odd_only: the odd positions at every level -- the order of the distributed reduction, whose ghost
// block is a right neighbour that is never a pivot and whose message layout describes that order.
struct BcrLevels {
  int origin[40], strides[40], parity[40], active[40], npivs[40];
  int64_t offS[41];        // first coupling of each level (active - 1 + ghost of them); [nlev]: the table behind the last level (distributed: the final coupling (block 0, ghost))
  int nlev = 0, last = 0;  // last: the block that is left
  int64_t off_end = 0;     // = offS[nlev]
};
static BcrLevels bcr_plan(int n, int ghost, bool odd_only) {
  BcrLevels L;
  const int g = ghost != 0 ? 1 : 0;
  int o = 0, s = 1, m = n; int64_t off = 0;
  while (m > 1) {
    const int p = (odd_only || (m & 1) == 0) ? 1 : 0;
    const int npiv = (m + 1 - p) / 2, l = L.nlev++;
    L.origin[l] = o; L.strides[l] = s; L.parity[l] = p; L.active[l] = m; L.npivs[l] = npiv; L.offS[l] = off;
    off += m - 1 + g; o += (1 - p) * s; s *= 2; m -= npiv;
  }
  L.offS[L.nlev] = off; L.off_end = off; L.last = o;
  return L;
}
static void bcr_set_level(BcrArgs& A, const BcrLevels& L, int l) {
  A.o = L.origin[l]; A.s = L.strides[l]; A.p = L.parity[l]; A.m = L.active[l];
  A.pn = l + 1 < L.nlev ? L.parity[l + 1] : 1;
  A.offS_in = L.offS[l]; A.offS_out = L.offS[l + 1];
}
// build + the inversions of level 0 in one launch (while the level-0 pivots fit on the chip at once)
static bool bcr_fused_build(int n, const long long* prof) { return n >= 2 && n <= 512 && prof == nullptr; }
// option bcr_join_levels (0: no level joined; 2: the levels above level 0 only; any other value: level 0 as well, where
// bcr_level0_behind_build says so) and the workgroup budget of a joined level
struct BcrJoin { int on = 0; int budget = 0; };
// Level 0 as ONE launch (bcri_invert_schur_kernel) behind a PLAIN build launch (bcr_build_kernel) instead of the build launch with
// level 0's inversions (bcri_build_invert_kernel, which forms and stores Z) and a Schur launch that loads Z again: THE rule, host
// arithmetic only (exported as oicc_debug_bcr_level0_plan).  It holds when joining is on and not held to the upper levels, no phase
// clocks are asked for, the solve is the whole band, 8 <= n <= 512 -- below eight blocks nothing of the timed plans runs and the
// recorded bits of the two- and three-block solves are those of B (X X^T); above 512 the build is plain anyway and bcr_level_joined
// alone decides -- and level 0's pivots x groups fit the workgroup budget.
static bool bcr_level0_behind_build(const BcrJoin& J, bool prof, int ghost, int b0, int n, int npiv0, int rtf) {
  return J.on != 0 && J.on != 2 && !prof && ghost == 0 && b0 == 0 && n >= 8 && n <= 512 && (int64_t)npiv0 * (12 + 3 * rtf) <= (int64_t)J.budget;
}
// the damped system in block form (+ the inversions of level 0 in the same launch when they fit the chip at once and level 0 does not
// join behind a plain build: level0_joins, bcr_level0_behind_build's answer); returns whether level 0 is inverted
static bool bcr_launch_build(const NormalEq& ne, const TangentLayout& tl, const SolveBuffers& sb, int reuse_diagonal, double min_diag, double max_diag, BcrArgs A, const BcrLevels& L, hipStream_t st, bool level0_joins = false) {
  const int n = A.n;
  const bool fused_build = bcr_fused_build(n, A.prof) && !level0_joins;
  const int64_t work = (int64_t)(n + A.ghost) * 4096;
  A.o = 0; A.s = 1; A.p = 1; A.m = n; A.pn = 1; A.offS_in = 0; A.offS_out = 0;
  if (L.nlev > 0) bcr_set_level(A, L, 0);
  if (fused_build) {
    int grid = int((work + 1023) / 1024); if (grid > 1024) grid = 1024;
    bcr_allow_lds(reinterpret_cast<const void*>(bcri_build_invert_kernel), bcr_lds_inv());
    hipLaunchKernelGGL(bcri_build_invert_kernel, dim3(L.npivs[0] + grid), dim3(64 * kInvWaves), bcr_lds_inv(), st, ne, tl, sb, reuse_diagonal, min_diag, max_diag, A);
  } else {
    int grid = int((work + 255) / 256); if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(bcr_build_kernel, dim3(grid), dim3(256), 0, st, ne, tl, sb, reuse_diagonal, min_diag, max_diag, A);
  }
  return fused_build;
}
// Which levels run as ONE launch (bcri_invert_schur_kernel) instead of an inversion launch and a Schur launch: THE rule, host
// arithmetic only (exported as oicc_debug_bcr_join_plan).  A level is joined when the option is on, no phase clocks are asked for,
// the solve is the whole band (the distributed reduction -- ghost block, block offset, carried coupling -- keeps its launches), the
// level's inversions are not already part of the build launch, and its pivots x groups fit the workgroup budget (default: one per
// compute unit): every workgroup of a pivot repeats the inversion, which costs nothing on compute units that would idle and
// everything on a level that is throughput bound.
static bool bcr_level_joined(const BcrJoin& J, bool prof, int ghost, int b0, bool carry, bool in_build, int npiv, int rtf) {
  return J.on != 0 && !prof && ghost == 0 && b0 == 0 && !carry && !in_build && (int64_t)npiv * (12 + 3 * rtf) <= (int64_t)J.budget;
}
// forward levels while more than one (local) block is active: inversions of the pivots, Schur complements onto their neighbours;
// returns the number of joined levels; *joined0 (optional): whether level 0 is one of them
static int bcr_launch_forward(BcrArgs A, bool level0_inverted, const BcrLevels& L, hipStream_t st, const BcrJoin& J = BcrJoin(), int* joined0 = nullptr) {
  using KernelFn = void (*)(BcrArgs);
  KernelFn k_inv = A.prof ? bcri_invert_kernel<false, true> : bcri_invert_kernel<false, false>;
  bcr_allow_lds(reinterpret_cast<const void*>(k_inv), bcr_lds_inv());
  const int g = A.ghost != 0 ? 1 : 0;
  int joined = 0;
  for (int l = 0; l < L.nlev; ++l) {
    const int m = L.active[l], npiv = L.npivs[l];
    bcr_set_level(A, L, l);
    A.side = (l == L.nlev - 1 && L.parity[l] == 0) ? 1 : 0;   // (the top level with two pivots)
    const bool carry = g != 0 && (m & 1) != 0;   // the last active block is no pivot: its coupling to the ghost block moves on unchanged
    A.carry = carry ? m : 0;
    if (bcr_level_joined(J, A.prof != nullptr, A.ghost, A.b0, carry, level0_inverted && l == 0, npiv, A.rtf)) {
      const size_t lds_join = (size_t)kJoinLdsDoubles * sizeof(double);
      bcr_allow_lds(reinterpret_cast<const void*>(bcri_invert_schur_kernel), lds_join);
      hipLaunchKernelGGL(bcri_invert_schur_kernel, dim3(12 + 3 * A.rtf, npiv), dim3(64 * kInvWaves), lds_join, st, A);
      ++joined;
      if (l == 0 && joined0 != nullptr) *joined0 = 1;
      continue;
    }
    BcrArgs Ai = A; if (l != 0) Ai.prof = nullptr;
    if (!(level0_inverted && l == 0)) hipLaunchKernelGGL(k_inv, dim3(npiv), dim3(64 * kInvWaves), bcr_lds_inv(), st, Ai);
    hipLaunchKernelGGL(bcri_schur_kernel, dim3(12 + 3 * A.rtf, npiv + (carry ? 1 : 0)), dim3(256), 0, st, A);
  }
  return joined;
}
// the back substitution of the levels top, top - 1, ..., 0: two levels per launch from the bottom up (an odd count: the uppermost alone, first)
// R (optional): the retraction request of a whole-band solve -- honoured by the two-level launch on the levels (1, 0), the last one of
// the solve (bcri_backward2_retract_kernel); returns whether it was
static bool bcr_launch_back(BcrArgs A, const BcrLevels& L, int top, hipStream_t st, const RetractReq* R = nullptr, const SolveBuffers* sb = nullptr) {
  int l = top;
  bool fused = false;
  if (l >= 0 && !(l & 1)) { bcr_set_level(A, L, l); hipLaunchKernelGGL(bcri_backward_kernel, dim3(L.npivs[l]), dim3(64 * kBackWaves), 0, st, A); --l; }
  for (; l >= 1; l -= 2) {
    const int lo = l - 1;   // the lower level of the pair
    // orphans: a lower pivot at an end of the active blocks whose one neighbour is no pivot of the upper level
    const int orphan_l = (L.parity[lo] == 0 && L.parity[l] == 1) ? L.origin[lo] : -1;
    const int orphan_r = (((L.active[lo] - 1) & 1) == L.parity[lo] && ((L.active[l] - 1) & 1) != L.parity[l]) ? L.origin[lo] + (L.active[lo] - 1) * L.strides[lo] : -1;
    bcr_set_level(A, L, lo);
    const dim3 grid(L.npivs[l] + (orphan_l >= 0 ? 1 : 0) + (orphan_r >= 0 ? 1 : 0));
    if (lo == 0 && R != nullptr) {   // (R: launch_bcr_solve decided; it hands a request down only where it is to be honoured)
      hipLaunchKernelGGL(bcri_backward2_retract_kernel, grid, dim3(1024), 0, st, A, L.origin[l], L.parity[l], L.active[l], L.npivs[l], orphan_l, orphan_r, *R, *sb);
      fused = true;
    } else hipLaunchKernelGGL(bcri_backward2_kernel, grid, dim3(1024), 0, st, A, L.origin[l], L.parity[l], L.active[l], L.npivs[l], orphan_l, orphan_r);
  }
  return fused;
}
// Which level's back substitution rides in the last block's launch (bcri_last_backward_kernel) instead of a launch of its own: THE
// rule, host arithmetic only (exported as oicc_debug_bcr_fold_plan); -1: none.  The back substitution pairs the levels from the bottom
// up, so an even number of levels leaves the uppermost one below the top level, nlev - 2, alone in a launch; its 2 to 4 pivots have
// only the last block and the top pivots as neighbours.  It is folded when the option is on, no phase clocks are asked for and the
// solve is the whole band (the distributed reduction -- ghost block, block offset -- keeps its launches).
static int bcr_fold_level(int on, bool prof, int ghost, int b0, const BcrLevels& L) {
  return (on != 0 && !prof && ghost == 0 && b0 == 0 && L.nlev >= 2 && (L.nlev & 1) == 0) ? L.nlev - 2 : -1;
}
// the last block with the arrow corner and the top level's back substitution (one or two pivots, whose only neighbour is the last
// block), then the levels below.  fold: bcr_fold_level's answer (launch_bcr_solve alone hands one down) -- that level goes with the
// last block and the launches below start under it.
static bool bcr_launch_last_and_back(BcrArgs A, const BcrLevels& L, hipStream_t st, const RetractReq* R = nullptr, const SolveBuffers* sb = nullptr, int fold = -1) {
  using KernelFn = void (*)(BcrArgs);
  KernelFn k_inv_last = fold >= 0 ? bcri_last_backward_kernel : bcri_invert_kernel<true, false>;
  const int a1 = A.a + 1;
  const size_t lds_inv_last = bcr_lds_inv() + (size_t)(64 * 65 + a1 * a1) * sizeof(double);           // + Fs, the parked corner
  bcr_allow_lds(reinterpret_cast<const void*>(k_inv_last), bcr_lds_inv() + (size_t)(64 * 65 + 64 * 64) * sizeof(double));   // (set once per function: the widest arrow)
  const int nlev = L.nlev;
  A.o = 0; A.s = 0; A.p = 1; A.m = 1; A.pn = 1; A.offS_in = 0; A.offS_out = 0; A.carry = 0;
  if (fold >= 0) bcr_set_level(A, L, fold);
  A.last = L.last; A.top_l = -1; A.top_r = -1; A.side = (nlev >= 1 && L.parity[nlev - 1] == 0) ? 1 : 0;
  if (nlev >= 1) {   // two active blocks: the pivot right of the last block; three: the two ends
    const int t = nlev - 1;
    A.top_r = L.last + L.strides[t];
    if (L.parity[t] == 0) A.top_l = L.last - L.strides[t];
  }
  hipLaunchKernelGGL(k_inv_last, dim3(fold >= 0 ? L.npivs[fold] : 1), dim3(64 * kInvWaves), lds_inv_last, st, A);
  return bcr_launch_back(A, L, fold >= 0 ? fold - 1 : nlev - 2, st, R, sb);        // (the top level went with the last block)
}

// the route of one cyclic-reduction solve (lm_solve_route): fused or separate build, or kRouteNone where it does not apply.
// kRouteBcrFused ("bcr_fused") names the family of 2..512 blocks without phase clocks, whichever launch inverts level 0: the build
// launch, or -- where bcr_level0_behind_build says so -- the joined level-0 launch behind a plain build.
int bcr_route(const TangentLayout& tl, const SolveBuffers& sb) {
  if (!bcr_applicable(tl) || tl.a + 1 > sb.bcr_max_border || sb.ws == nullptr || sb.ws_doubles < bcr_workspace_doubles(tl)) return kRouteNone;
  if (sb.algo != 0 && sb.algo != 4) return kRouteNone;   // (algorithms 2 and 3 -- the factor-based levels of rounds 1-2 and their parallel form -- left the library in round 4)
  return bcr_fused_build(bcr_blocks(tl.Pb), sb.prof) ? kRouteBcrFused : kRouteBcrUnfused;
}
// build + factor + solve; the solution lands in sb.step_s.  Returns 0, or -1 if not applicable.
// retract (optional): also the retraction x_cand = x (+) scale .* step and the step's three scalars, inside the last launch -- where
// the plan has at least three levels (n >= 8 blocks: the last launch is then the two-level back substitution of the levels (1, 0)),
// the unscaled step is asked for (alpha = 1) and no segment tables are (the request carries none); *fused tells whether it was done,
// and the caller launches lm_retract_kernel exactly when it was not.
int launch_bcr_solve(const NormalEq& ne, const TangentLayout& tl, const SolveBuffers& sb, int reuse_diagonal,
                     double min_diag, double max_diag, hipStream_t st, const RetractReq* retract, bool* fused) {
  if (fused) *fused = false;
  if (bcr_route(tl, sb) == kRouteNone) return -1;
  const int n = bcr_blocks(tl.Pb), a1 = tl.a + 1;
  BcrArgs A{};
  bcr_carve(A, sb.ws, n, a1);
  A.Mc = sb.Mc; A.x = sb.step_s; A.fail = &sb.st->chol_failed; A.prof = sb.prof;
  A.n = n; A.a = tl.a; A.Pb = tl.Pb; A.delay = sb.bcr_delay;
  A.rtf = (a1 + 15) / 16; A.ctl = sb.ctl;
  const BcrLevels L = bcr_plan(n, 0, false);
  BcrJoin J; J.on = sb.bcr_join; J.budget = sb.bcr_join_budget;
  const bool level0_joins = L.nlev > 0 && bcr_level0_behind_build(J, A.prof != nullptr, A.ghost, A.b0, n, L.npivs[0], A.rtf);
  const bool inverted = bcr_launch_build(ne, tl, sb, reuse_diagonal, min_diag, max_diag, A, L, st, level0_joins);
  int joined0 = 0;
  int joined = bcr_launch_forward(A, inverted, L, st, J, &joined0);
  // (a level 0 that joins behind the plain build of 8..512 blocks has counters of its own: [0..1] count what oicc_debug_bcr_join_plan says)
  joined0 = level0_joins ? joined0 : 0; joined -= joined0;
  if (sb.bcr_joined != nullptr) { sb.bcr_joined[0] = joined; sb.bcr_joined[1] += joined; sb.bcr_joined[2] = joined0; sb.bcr_joined[3] += joined0; }
  // the ONE place that decides: a request that is on, for the unscaled step, and a plan whose last launch is the two-level back
  // substitution on the levels (1, 0); this entry always solves the whole band (b0 = 0, no ghost block)
  const bool honour = retract != nullptr && retract->on != 0 && retract->rmap != nullptr && retract->alpha == 1.0 && L.nlev >= 3 && A.ghost == 0 && A.b0 == 0;
  RetractReq R{}; if (honour) { R = *retract; R.ne = ne; }
  const int fold = bcr_fold_level(sb.bcr_fold, A.prof != nullptr, A.ghost, A.b0, L);
  if (sb.bcr_folded != nullptr) { sb.bcr_folded[0] = fold >= 0 ? 1 : 0; sb.bcr_folded[1] += fold >= 0 ? 1 : 0; }
  const bool did = bcr_launch_last_and_back(A, L, st, honour ? &R : nullptr, &sb, fold);
  if (fused) *fused = did;
  return 0;
}

// =================================================================================================================================
// Distributed block cyclic reduction (round 6; SURVEY 8(e) "v2 ... Solve: partitioned"; the reference's solve is one
// SPARSE_NORMAL_CHOLESKY on one host, spline_trajectory_estimator.impl.h:257-272).  N ranks, rank k owns the blocks [b_k, b_k+1) of
// the band (the cuts of the owner-computes exchange lie on multiples of 64 rows) and holds the complete rows of its range only.
//   forward, no communication: rank k reduces ITS blocks with the kernels above down to its first block (the range's separator);
//     the pivots at the right end of the range have the next rank's first block as their right neighbour -- the ghost block, never a
//     pivot, whose D / F start at zero and collect this rank's Schur updates for their owner.
//   ONE all-gather of [D_sep, F_sep, coupling (sep, ghost), D_ghost, F_ghost, this rank's Schur updates of the arrow corner]
//     (3 x 4096 + 2 x 64 (a + 1) + (a + 1)^2 doubles per rank: 0.11 MB) -- the band itself never travels;
//   the top system -- the N separators, block tridiagonal again, + the corner -- is assembled and solved by EVERY rank (log2 N levels
//     + block 0: the same kernels), which leaves x of all separators and of the arrow on every rank;
//   backward, no communication: the local levels in reverse; then ONE all-gather of the ranks' solutions (<= 0.72 MB in all at
//     BASELINE config 5) puts the step on every rank.
// Per-rank depth: ceil(log2(n / N)) + ceil(log2 N) + 1 inversions instead of floor(log2 n) + 1, each over 1 / N of the pivots.
// Both the local range and the top system keep the odd-positions-only order (bcr_plan's odd_only).
// =================================================================================================================================
__global__ void bcr_dist_pack_kernel(BcrArgs A, int64_t off_final, double* msg) {   // this rank's slot of the first gather
  const int a1 = A.a + 1; const int64_t fsz = (int64_t)64 * a1;
  const int64_t total = 3 * 4096 + 2 * fsz + (int64_t)a1 * a1;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    double v;
    if (e < 4096) v = A.D[e];
    else if (e < 4096 + fsz) v = A.F[e - 4096];
    else if (e < 2 * 4096 + fsz) v = A.ghost ? A.S[off_final * 4096 + (e - 4096 - fsz)] : 0.0;
    else if (e < 3 * 4096 + fsz) v = A.ghost ? A.D[(int64_t)A.n * 4096 + (e - 2 * 4096 - fsz)] : 0.0;
    else if (e < 3 * 4096 + 2 * fsz) v = A.ghost ? A.F[(int64_t)A.n * fsz + (e - 3 * 4096 - fsz)] : 0.0;
    else v = A.Mc[e - 3 * 4096 - 2 * fsz];
    msg[e] = v;
  }
}
// the top system from the gathered slots: T.D[k] = D_sep(k) + D_ghost(k - 1) (lower part), T.F likewise, the level-0 couplings in the
// orientation the build gives them (pivot-variable major, the pivot is the odd block), the corner = the sum of the ranks' parts in rank order
__global__ void bcr_dist_top_kernel(BcrArgs T, const double* msgs, int64_t piece) {
  const int N = T.n, a1 = T.a + 1; const int64_t fsz = (int64_t)64 * a1;
  const int64_t nD = (int64_t)N * 4096, nF = (int64_t)N * fsz, nS = (int64_t)(N - 1) * 4096, nC = (int64_t)a1 * a1;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nD + nF + nS + nC; e += (int64_t)gridDim.x * blockDim.x) {
    if (e < nD) {
      const int k = int(e >> 12); const int64_t o = e & 4095;
      T.D[e] = msgs[k * piece + o] + (k > 0 ? msgs[(k - 1) * piece + 2 * 4096 + fsz + o] : 0.0);
    } else if (e < nD + nF) {
      const int64_t f = e - nD; const int k = int(f / fsz); const int64_t o = f - k * fsz;
      T.F[f] = msgs[k * piece + 4096 + o] + (k > 0 ? msgs[(k - 1) * piece + 3 * 4096 + fsz + o] : 0.0);
    } else if (e < nD + nF + nS) {
      const int64_t f = e - nD - nF; const int k = int(f >> 12), c = int(f >> 6) & 63, r = int(f) & 63;
      const double* src = msgs + k * piece + 4096 + fsz;       // Q[c = separator k variable][r = separator k + 1 variable]
      T.S[f] = (k & 1) ? src[c * 64 + r] : src[r * 64 + c];    // (pivot = k + 1 when k is even: transposed)
    } else {
      const int64_t f = e - nD - nF - nS;
      double v = 0.0;
      for (int k = 0; k < N; ++k) v += msgs[k * piece + 3 * 4096 + 2 * fsz + f];
      T.Mc[f] = v;
    }
  }
}
// the separators' and the arrow's solution into the local system: x of block 0, of the ghost block, the arrow part
__global__ void bcr_dist_scatter_kernel(BcrArgs A, const double* xt, int N, int rank) {
  const int t = threadIdx.x;
  if (t < 64) A.x[t] = xt[rank * 64 + t];
  else if (t < 128) { if (A.ghost) A.x[(int64_t)A.n * 64 + (t - 64)] = xt[(rank + 1) * 64 + (t - 64)]; }
  else if (t < 128 + A.a) A.x[A.Pb + (t - 128)] = xt[N * 64 + (t - 128)];
}
__global__ void bcr_dist_pack_x_kernel(BcrArgs A, double* slot, int64_t arrow_at) {   // this rank's slot of the second gather: [its blocks' solution | arrow]
  const int64_t nx = (int64_t)A.n * 64;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nx + A.a; e += (int64_t)gridDim.x * blockDim.x) {
    if (e < nx) slot[e] = A.x[e]; else slot[arrow_at + (e - nx)] = A.x[A.Pb + (e - nx)];
  }
}
__global__ void bcr_dist_unpack_x_kernel(const double* slots, int64_t piece, const int32_t* b0s, int N, int Pb, int a, int64_t arrow_at, double* x) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)Pb + a; i += (int64_t)gridDim.x * blockDim.x) {
    if (i >= Pb) { x[i] = slots[arrow_at + (i - Pb)]; continue; }     // (the arrow part: rank 0's -- every rank solved the same top system, up to the order of its atomics)
    const int blk = int(i >> 6); int k = 0; while (k + 1 < N && blk >= b0s[k + 1]) ++k;
    x[i] = slots[k * piece + (i - (int64_t)b0s[k] * 64)];
  }
}

int64_t bcr_dist_workspace_doubles(const TangentLayout& tl, int n_loc, int nranks) {
  const int a1 = tl.a + 1;
  return bcr_carve_doubles(n_loc + 1, a1) + ((int64_t)(n_loc + 1) * 64 + tl.a + 8) + bcr_carve_doubles(nranks, a1) + ((int64_t)nranks * 64 + tl.a + 8) + 2 * (int64_t)a1 * a1 + 64;
}
int64_t bcr_dist_msg_doubles(const TangentLayout& tl) { const int a1 = tl.a + 1; return 3 * 4096 + 2 * (int64_t)64 * a1 + (int64_t)a1 * a1; }

namespace {
struct DistViews { BcrArgs A, T; double* xt; };
DistViews bcr_dist_views(const TangentLayout& tl, const SolveBuffers& sb, const BcrDist& d) {
  const int a1 = tl.a + 1, ghost = d.rank + 1 < d.nranks ? 1 : 0;
  DistViews v{};
  double* w = d.ws;
  BcrArgs& A = v.A;
  bcr_carve(A, w, d.n_loc + 1, a1); w += bcr_carve_doubles(d.n_loc + 1, a1);
  A.x = w; w += (int64_t)(d.n_loc + 1) * 64 + tl.a + 8;
  A.Mc = w; w += (int64_t)a1 * a1;
  A.fail = &sb.st->chol_failed; A.prof = nullptr; A.n = d.n_loc; A.a = tl.a; A.Pb = (d.n_loc + ghost) * 64; A.delay = sb.bcr_delay;
  A.rtf = (a1 + 15) / 16; A.ctl = nullptr; A.b0 = d.b0; A.ghost = ghost;
  BcrArgs& T = v.T;
  bcr_carve(T, w, d.nranks, a1); w += bcr_carve_doubles(d.nranks, a1);
  T.x = w; w += (int64_t)d.nranks * 64 + tl.a + 8;
  T.Mc = w; w += (int64_t)a1 * a1;
  T.fail = A.fail; T.prof = nullptr; T.n = d.nranks; T.a = tl.a; T.Pb = d.nranks * 64; T.delay = sb.bcr_delay; T.rtf = A.rtf; T.ctl = nullptr; T.b0 = 0; T.ghost = 0;
  v.xt = T.x;
  return v;
}
}  // namespace

// rank-local part of the forward reduction; leaves this rank's slot of the first gather in d.msg
int launch_bcr_dist_forward(const NormalEq& ne, const TangentLayout& tl, const SolveBuffers& sb_in, int reuse_diagonal, double min_diag, double max_diag, const BcrDist& d, hipStream_t st) {
  if (!bcr_applicable(tl) || tl.a + 1 > sb_in.bcr_max_border || d.ws == nullptr || d.n_loc < 1 || d.nranks < 2 || d.ws_doubles < bcr_dist_workspace_doubles(tl, d.n_loc, d.nranks)) return -1;
  DistViews v = bcr_dist_views(tl, sb_in, d);
  SolveBuffers sb = sb_in; sb.Mc = v.A.Mc; sb.ctl = nullptr;   // (the build writes the corner where the Schur kernels add to it)
  const BcrLevels L = bcr_plan(v.A.n, v.A.ghost, true);
  const bool inverted = bcr_launch_build(ne, tl, sb, reuse_diagonal, min_diag, max_diag, v.A, L, st);
  bcr_launch_forward(v.A, inverted, L, st);
  const int64_t total = bcr_dist_msg_doubles(tl);
  hipLaunchKernelGGL(bcr_dist_pack_kernel, dim3(int((total + 255) / 256)), dim3(256), 0, st, v.A, L.off_end, d.msg + (int64_t)d.rank * d.msg_piece);
  return 0;
}
// between the gathers: the top system and its solution (replicated), the local back substitution, this rank's slot of the second gather
int launch_bcr_dist_middle(const TangentLayout& tl, const SolveBuffers& sb, const BcrDist& d, hipStream_t st) {
  DistViews v = bcr_dist_views(tl, sb, d);
  const int a1 = tl.a + 1, N = d.nranks;
  const int64_t work = (int64_t)N * 4096 + (int64_t)N * 64 * a1 + (int64_t)(N - 1) * 4096 + (int64_t)a1 * a1;
  hipLaunchKernelGGL(bcr_dist_top_kernel, dim3(int(std::min<int64_t>(1024, (work + 255) / 256))), dim3(256), 0, st, v.T, d.msg, d.msg_piece);
  const BcrLevels LT = bcr_plan(N, 0, true);   // (the top system's level-0 couplings come from bcr_dist_top_kernel, which orients them for odd pivots)
  bcr_launch_forward(v.T, false, LT, st);
  bcr_launch_last_and_back(v.T, LT, st);
  hipLaunchKernelGGL(bcr_dist_scatter_kernel, dim3(1), dim3(256), 0, st, v.A, v.xt, N, d.rank);
  // the local levels in reverse (the plan follows from the block count alone)
  BcrArgs A = v.A;
  const BcrLevels L = bcr_plan(A.n, A.ghost, true);
  bcr_launch_back(A, L, L.nlev - 1, st);
  const int64_t nx = (int64_t)A.n * 64 + A.a;
  hipLaunchKernelGGL(bcr_dist_pack_x_kernel, dim3(int((nx + 255) / 256)), dim3(256), 0, st, v.A, d.xg + (int64_t)d.rank * d.x_piece, (int64_t)d.max_loc * 64);
  return 0;
}
// behind the second gather: the step of every rank's range -> sb.step_s
void launch_bcr_dist_finish(const TangentLayout& tl, const SolveBuffers& sb, const BcrDist& d, hipStream_t st) {
  const int64_t n = (int64_t)tl.Pb + tl.a;
  hipLaunchKernelGGL(bcr_dist_unpack_x_kernel, dim3(int(std::min<int64_t>(1024, (n + 255) / 256))), dim3(256), 0, st, d.xg, d.x_piece, d.d_b0, d.nranks, tl.Pb, tl.a, (int64_t)d.max_loc * 64, sb.step_s);
}

}  // namespace oicc

extern "C" int oicc_debug_bcr_plan(int32_t n, int32_t ghost, int32_t odd_only, int64_t* levels, int32_t cap_levels, int64_t info[3]) {
  if (n < 1 || levels == nullptr || info == nullptr) return OICC_ERR_INVALID_ARG;
  const oicc::BcrLevels L = oicc::bcr_plan(n, ghost, odd_only != 0);
  if (L.nlev > cap_levels) return OICC_ERR_INVALID_ARG;
  for (int l = 0; l < L.nlev; ++l) {
    int64_t* o = levels + 6 * l;
    o[0] = L.origin[l]; o[1] = L.strides[l]; o[2] = L.parity[l]; o[3] = L.active[l]; o[4] = L.npivs[l]; o[5] = L.offS[l];
  }
  info[0] = L.last; info[1] = L.off_end; info[2] = oicc::bcr_coupling_slots(n + (ghost != 0 ? 1 : 0));
  return L.nlev;
}

extern "C" int oicc_debug_bcr_join_plan(int32_t n, int32_t ghost, int32_t odd_only, int32_t b0, int32_t rtf, int32_t join_levels, int32_t budget,
                                        int32_t build_inverts, int32_t* joined, int32_t cap_levels) {
  if (n < 1 || joined == nullptr || rtf < 1 || rtf > 4 || budget < 0 || b0 < 0) return OICC_ERR_INVALID_ARG;
  const oicc::BcrLevels L = oicc::bcr_plan(n, ghost, odd_only != 0);
  if (L.nlev > cap_levels) return OICC_ERR_INVALID_ARG;
  oicc::BcrJoin J; J.on = join_levels; J.budget = budget;
  const bool in_build0 = build_inverts < 0 ? oicc::bcr_fused_build(n, nullptr) : build_inverts != 0;
  for (int l = 0; l < L.nlev; ++l) {
    const bool carry = ghost != 0 && (L.active[l] & 1) != 0;   // (as bcr_launch_forward)
    joined[l] = oicc::bcr_level_joined(J, false, ghost, b0, carry, in_build0 && l == 0, L.npivs[l], rtf) ? 1 : 0;
  }
  return L.nlev;
}

extern "C" int oicc_debug_bcr_level0_plan(int32_t n, int32_t ghost, int32_t odd_only, int32_t b0, int32_t rtf, int32_t join_levels, int32_t budget) {
  if (n < 1 || rtf < 1 || rtf > 4 || budget < 0 || b0 < 0) return OICC_ERR_INVALID_ARG;
  const oicc::BcrLevels L = oicc::bcr_plan(n, ghost, odd_only != 0);
  oicc::BcrJoin J; J.on = join_levels; J.budget = budget;
  return L.nlev > 0 && oicc::bcr_level0_behind_build(J, false, ghost, b0, n, L.npivs[0], rtf) ? 1 : 0;
}

extern "C" int oicc_debug_bcr_fold_plan(int32_t n, int32_t ghost, int32_t odd_only, int32_t b0, int32_t on) {
  if (n < 1 || b0 < 0 || ghost < 0 || ghost > 1) return INT32_MIN;   // (-1 is an answer here: no level folds)
  const oicc::BcrLevels L = oicc::bcr_plan(n, ghost, odd_only != 0);
  return oicc::bcr_fold_level(on, false, ghost, b0, L);
}

// The panel chain of bcri_invert_body as a list of events in PROGRAM order (host arithmetic only; tests): what bcr_chain_column
// (bcr_chain_body.h) expands from the table kChainSchedule, restated step by step.  One row of six per event:
//   {type, column, gap, k, c2, aux}
//   type 0  pivot read of `column` (v_readlane)                         type 3  deferred update av[c2] = fma(-l(k), m(k, c2), av[c2])
//   type 1  strip store of `column` = k; every lane stores: the doubles  type 4  the v_readlane hop: update (column, column + 1)
//           [aux, c2) of the wave's strips, of which [aux, aux + 16) are strip k
//   type 2  LDS read of m(k, c2) = double aux of the wave's strips, issued in `column` for an update of column + 1
// gap: where in the column (bcr_chain_schedule.h); -1 for the types 0, 1, 4.  Returns the number of events; rows beyond `cap` are
// not written.
extern "C" int oicc_debug_bcr_chain_schedule(int32_t* rows, int32_t cap) {
  const oicc::BcrChainSchedule& S = oicc::kChainSchedule;
  int n = 0;
  auto put = [&](int type, int column, int gap, int k, int c2, int aux) {
    if (rows != nullptr && n < cap) { int32_t* r = rows + 6 * (int64_t)n; r[0] = type; r[1] = column; r[2] = gap; r[3] = k; r[4] = c2; r[5] = aux; }
    ++n;
  };
  auto gap = [&](int c, int g) {
    const int first = oicc::bcr_chain_gap_first(S, c, g);
    for (int q = 0; q < S.gap_n[c][g]; ++q) put(3, c, g, S.k[c][first + q], S.c2[c][first + q], 0);
  };
  auto loads = [&](int c, bool fresh) {   // issued in column c for the updates of column c + 1
    for (int u = 0; u < S.total[c + 1]; ++u)
      if ((S.k[c + 1][u] == c) == fresh) put(2, c, fresh ? 7 : 1, S.k[c + 1][u], S.c2[c + 1][u], 16 * S.k[c + 1][u] + S.c2[c + 1][u]);
  };
  for (int c = 0; c < 16; ++c) {
    put(0, c, -1, c, c, 0);
    gap(c, 0);
    if (c < 14) loads(c, false);
    for (int g = 1; g <= 6; ++g) gap(c, g);
    if (c < 15) {
      if (c < 14) { put(1, c, -1, c, 16 * c + 64, 16 * c); loads(c, true); }
      gap(c, 7);
      put(4, c, -1, c, c + 1, 0);
    }
  }
  return n;
}

// The 16-column panel chain of bcri_invert_body (kernels_bcr.hip) with its deferred updates issued where a BcrChainSchedule puts them
// (bcr_chain_schedule.h).  Device code; included by kernels_bcr.hip and by scripts/micro/chain_issue.hip, which measures this very body.
#pragma once
#include <hip/hip_runtime.h>
#include <utility>
#include "bcr_chain_schedule.h"

namespace oicc {

// The LDS stores of this wave's lanes are visible to the loads of its other lanes behind this: LDS operations of ONE wave execute in
// issue order, so this orders the compiler (wavefront-scope fences) and issues nothing -- no workgroup barrier, no wait.
__device__ __forceinline__ void bcr_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ double bcr_readlane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// Strips: column k of a panel stores l(k) at strip_w[16 k] -- EVERY lane stores (a store under `lane < 16` is a branch per column) --
// with strip_w = base + lane: lanes 0..15 fill the strip [16 k, 16 k + 16), lanes 16..63 land in the strips k + 1 .. k + 3, which their
// own columns overwrite before anything reads them (LDS operations of a wave execute in issue order); column 13's, the last store,
// reach 16 * 13 + 64 = kChainStripDoubles.  m(k, c2) = strip_r[16 k + c2], the same address in every lane (a broadcast).
constexpr int kChainStripDoubles = 272;

// nothing crosses: the order of the source is the order of the instructions
#define BCR_CHAIN_PIN() __builtin_amdgcn_sched_barrier(0)

template <const BcrChainSchedule& S, int C, int U>
__device__ __forceinline__ void bcr_chain_update(double (&av)[16], const double (&mc)[kChainColMax]) {
  constexpr int k = S.k[C][U], c2 = S.c2[C][U];
  av[c2] = fma(-av[k], mc[U], av[c2]);
}
template <const BcrChainSchedule& S, int C, int G>
__device__ __forceinline__ void bcr_chain_gap(double (&av)[16], const double (&mc)[kChainColMax]) {
  constexpr int first = bcr_chain_gap_first(S, C, G), n = S.gap_n[C][G];
  static_assert(n <= 4 && kChainGapMax == 4, "a gap expands up to four updates");
  BCR_CHAIN_PIN();
  if constexpr (n > 0) bcr_chain_update<S, C, first>(av, mc);
  if constexpr (n > 1) bcr_chain_update<S, C, first + 1>(av, mc);
  if constexpr (n > 2) bcr_chain_update<S, C, first + 2>(av, mc);
  if constexpr (n > 3) bcr_chain_update<S, C, first + 3>(av, mc);
  BCR_CHAIN_PIN();
}
// the multipliers of column C's updates, in issue order: FRESH those of column C - 1's strip, else those of the older strips
template <const BcrChainSchedule& S, int C, bool FRESH, int U = 0>
__device__ __forceinline__ void bcr_chain_loads(double (&mn)[kChainColMax], const double* strip_r) {
  if constexpr (U < S.total[C]) {
    constexpr int at = 16 * S.k[C][U] + S.c2[C][U];   // (a constant of the instruction, whatever storage S has)
    if constexpr ((S.k[C][U] == C - 1) == FRESH) mn[U] = strip_r[at];
    bcr_chain_loads<S, C, FRESH, U + 1>(mn, strip_r);
  }
}

template <const BcrChainSchedule& S, int C>
__device__ __forceinline__ void bcr_chain_column(double (&av)[16], double (&mq)[2][kChainColMax], double* strip_w, const double* strip_r, bool& bad) {
  const double (&mc)[kChainColMax] = mq[C & 1];     // the multipliers of this column's updates, loaded during column C - 1
  double (&mn)[kChainColMax] = mq[(C + 1) & 1];     // those of the next column's
  const double piv = bcr_readlane(av[C], C);
  if (C == 15) bad = !(piv > 0.0);
  bcr_chain_gap<S, C, 0>(av, mc);
  const double y0 = __builtin_amdgcn_rsq(piv);
  BCR_CHAIN_PIN();
  if constexpr (C < 14) bcr_chain_loads<S, C + 1, false>(mn, strip_r);
  bcr_chain_gap<S, C, 1>(av, mc);
  const double g0 = piv * y0, h0 = 0.5 * y0;
  const double a2 = av[C] + av[C];
  bcr_chain_gap<S, C, 2>(av, mc);
  const double r0 = fma(-g0, h0, 0.5);
  bcr_chain_gap<S, C, 3>(av, mc);
  const double g1 = fma(g0, r0, g0), h1 = fma(h0, r0, h0);
  bcr_chain_gap<S, C, 4>(av, mc);
  const double r1 = fma(-g1, h1, 0.5);
  const double u = a2 * h1;
  bcr_chain_gap<S, C, 5>(av, mc);
  const double l = fma(u, r1, u);
  av[C] = l;
  bcr_chain_gap<S, C, 6>(av, mc);
  if constexpr (C < 15) {
    const double m1 = bcr_readlane(l, C + 1);
    if constexpr (C < 14) {
      strip_w[16 * C] = l;
      bcr_wave_sync();
      bcr_chain_loads<S, C + 1, true>(mn, strip_r);
    }
    bcr_chain_gap<S, C, 7>(av, mc);
    av[C + 1] = fma(-l, m1, av[C + 1]);
  }
}

template <const BcrChainSchedule& S, int... Cs>
__device__ __forceinline__ void bcr_chain_columns(double (&av)[16], double (&mq)[2][kChainColMax], double* strip_w, const double* strip_r, bool& bad, std::integer_sequence<int, Cs...>) {
  (bcr_chain_column<S, Cs>(av, mq, strip_w, strip_r, bad), ...);
}

// One panel: av[c] = this lane's row of column c on entry, the factor's on return.  strip_w = the wave's strips + lane, strip_r = the
// wave's strips (kChainStripDoubles doubles, 16-byte aligned).  Returns !(pivot of column 15 > 0): true exactly for the panels in which
// a pivot was not positive (a pivot that is not positive makes rsq NaN or inf, l NaN in every lane, and with it every later pivot).
// The arithmetic and its order per entry are those of the plain column loop: av[c2] takes the updates of the columns 0 .. c2 - 1 in
// that order, the last of them by the v_readlane hop.
template <const BcrChainSchedule& S>
__device__ __forceinline__ bool bcr_chain_panel(double (&av)[16], double* strip_w, const double* strip_r) {
  double mq[2][kChainColMax];
  bool bad = false;
  bcr_chain_columns<S>(av, mq, strip_w, strip_r, bad, std::make_integer_sequence<int, 16>());
  return bad;
}

}  // namespace oicc

// Where the deferred updates of a 16-column panel chain are issued (kernels_bcr.hip, bcri_invert_body).  Host and device; no HIP.
//
// Column c of a panel is a dependent sequence -- v_readlane pivot, v_rsq_f64, two Goldschmidt steps, l, the v_readlane hop of l(c + 1)
// onto column c + 1 -- whose every instruction waits out its predecessor with an empty issue slot.  The 105 updates
//     av[c2] = fma(-l(k), m(k, c2), av[c2]),  c2 >= k + 2,  m(k, c2) = l(k) of lane c2, read back from column k's strip in LDS
// are independent of it.  An update (k, c2) may be issued anywhere behind column k's strip store and ahead of column c2's pivot read,
// as long as av[c2] takes its updates in the order k = 0, 1, ...: the table below spreads them, 7 or 8 per column over the columns
// 1 .. 14, into the GAPS between the dependent steps:
//     gap 0  pivot readlane .. rsq          gap 4  g1, h1 .. r1, u
//     gap 1  rsq .. g0, h0                  gap 5  r1, u .. l
//     gap 2  g0, h0 .. r0                   gap 6  l .. readlane of l(c + 1), strip store
//     gap 3  r0 .. g1, h1                   gap 7  readlane, strip store .. the hop's fma onto column c + 1
// The multipliers of column c's updates are loaded one column ahead: those of the columns k <= c - 2 behind the rsq of column c - 1,
// those of column k = c - 1 ("fresh") behind its strip store.
#pragma once

namespace oicc {

constexpr int kChainGaps = 8;       // gaps of a column
constexpr int kChainGapMax = 4;     // updates a gap can hold in the table
constexpr int kChainColMax = 16;    // updates a column can hold in the table

struct BcrChainSchedule {
  signed char total[16];                           // updates issued in column c
  signed char fresh[16];                           // of them those of column k = c - 1, whose strip is stored last
  signed char k[16][kChainColMax], c2[16][kChainColMax];   // in issue order
  signed char gap_n[16][kChainGaps];               // how many of them gap g takes, in order
  bool ok;
};

// weight[g]: the updates gap g takes of a column that has as many as the weights' sum.
// previous_column_only: column c issues exactly the updates of column c - 1 (14 in column 1, none in column 15) -- the order measured
// once before ("item (3), the schedule"), kept for scripts/micro/chain_issue.hip to measure the table against.
constexpr BcrChainSchedule bcr_chain_schedule(const int (&weight)[kChainGaps], int hop_clear = 2, bool previous_column_only = false) {
  BcrChainSchedule S{};
  S.ok = true;
  bool done[16][16] = {};
  int left = 105;
  for (int c = 1; c <= 14; ++c) {
    // this column's share of what is left, at least what column c + 1's pivot needs
    int mand = 0;
    for (int k = 0; k <= c - 1; ++k) if (c + 1 >= k + 2 && !done[k][c + 1]) ++mand;
    int quota = (left + (14 - c)) / (15 - c);
    if (quota < mand) quota = mand;
    if (previous_column_only) quota = 15 - c;
    // selection: the updates onto column c + 1, then the oldest columns' first
    bool sel[16][16] = {};
    int n = 0;
    for (int k = 0; k <= c - 1 && n < quota; ++k) if (c + 1 >= k + 2 && !done[k][c + 1]) { sel[k][c + 1] = true; ++n; }
    for (int k = 0; k <= c - 1; ++k) for (int t = c + 1; t < 16 && n < quota; ++t) if (t >= k + 2 && !done[k][t] && !sel[k][t]) { sel[k][t] = true; ++n; }
    if (n > kChainColMax) { S.ok = false; n = kChainColMax; }
    // issue order: the updates onto column c + 1 of the older columns, the others by (k, c2) -- column c - 1's last --, and the one
    // of column c - 1 onto column c + 1 ahead of the last `hop_clear` others: the hop's fma onto column c + 1 waits for it, and its
    // multiplier is the last to arrive
    signed char bk[kChainColMax] = {}, bt[kChainColMax] = {};
    int nb = 0, i = 0;
    for (int k = 0; k <= c - 2; ++k) if (sel[k][c + 1] && i < kChainColMax) { S.k[c][i] = (signed char)k; S.c2[c][i] = (signed char)(c + 1); ++i; }
    for (int k = 0; k <= c - 1; ++k) for (int t = c + 2; t < 16; ++t) if (sel[k][t] && nb < kChainColMax) { bk[nb] = (signed char)k; bt[nb] = (signed char)t; ++nb; }
    const int tail = nb < hop_clear ? nb : hop_clear;
    for (int b = 0; b < nb - tail && i < kChainColMax; ++b, ++i) { S.k[c][i] = bk[b]; S.c2[c][i] = bt[b]; }
    if (sel[c - 1][c + 1] && i < kChainColMax) { S.k[c][i] = (signed char)(c - 1); S.c2[c][i] = (signed char)(c + 1); ++i; }
    for (int b = nb - tail; b < nb && i < kChainColMax; ++b, ++i) { S.k[c][i] = bk[b]; S.c2[c][i] = bt[b]; }
    int nf = 0;
    for (int q = 0; q < i; ++q) { done[S.k[c][q]][S.c2[c][q]] = true; if (S.k[c][q] == c - 1) ++nf; }
    S.total[c] = (signed char)i; S.fresh[c] = (signed char)nf; left -= i;
    // the gaps take their weights; a column of fewer updates than the weights' sum spares the gaps 6, 5, .. 1 in turn, not the two
    // v_readlane shadows at its ends
    int w[kChainGaps] = {}, sum = 0;
    for (int g = 0; g < kChainGaps; ++g) { w[g] = weight[g] < kChainGapMax ? weight[g] : kChainGapMax; sum += w[g]; }
    for (int g = 6; sum > i; g = g > 1 ? g - 1 : 6) {
      if (w[g] > 0) { --w[g]; --sum; }
      else if (w[1] + w[2] + w[3] + w[4] + w[5] + w[6] == 0) { g = w[7] > 0 ? 7 : 0; --w[g]; --sum; g = 6; }
    }
    int put = 0;
    for (int g = 0; g < kChainGaps; ++g) { S.gap_n[c][g] = (signed char)w[g]; put += w[g]; }
    if (put < i) S.ok = false;
  }
  if (left != 0) S.ok = false;
  return S;
}

// the placement bcri_invert_body runs (scripts/micro/chain_issue.hip measured the candidates)
// two updates in each of the two v_readlane shadows (a v_readlane -> VALU hop is 24.6 cycles, a dependent fp64 instruction's latency
// one or two issue slots), one behind each of the first four steps
constexpr int kChainWeights[kChainGaps] = {2, 1, 1, 1, 1, 0, 0, 2};
constexpr BcrChainSchedule kChainSchedule = bcr_chain_schedule(kChainWeights, 4);
static_assert(kChainSchedule.ok, "every update has a gap");

// first update of gap g of column c in the column's issue order
constexpr int bcr_chain_gap_first(const BcrChainSchedule& S, int c, int g) {
  int s = 0;
  for (int q = 0; q < g; ++q) s += S.gap_n[c][q];
  return s;
}

}  // namespace oicc

// Host walk of the K-best candidate lists (vvc-mip-gpu_amd/csrc/candidates_plan.h) as a
// stand-alone program: tests/test_candidates_plan.py writes the families' tables to a file, this
// program runs candidates_frames_host (the keys, the selection step and the row layout the kernel
// uses) on arrays of exactly the contract's sizes and writes both outputs back; the test compares
// them with tests/candidates_ref.py.  Before that it checks the rank and code mapping, the
// "absent entry" rules, the selection step on hand-made rows and the argument rules of both entry
// points.  Built with -fsanitize=address,undefined as well.
//
//   test_candidates_plan run IN OUT
//   IN : int32 width, height, nframes, k, kin, families (1 MIP | 2 Planar/DC | 4 angular),
//        outputs (1 modes | 2 costs), bias_given, intra_bias[2], ang_bias;
//        then, for the families given, uint8 mip_mode[cus][kin]; int32 mip_cost[cus][kin];
//        int32 intra_cost[cus][2]; int32 ang_cost[cus][65]
//   OUT: uint8 modes[cus][k] (if asked for); int32 costs[cus][k] (if asked for)
#include <cstdio>
#include <cstring>
#include <vector>

#include "candidates_plan.h"

template <class T>
static bool rd(FILE *f, std::vector<T> &v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <class T>
static bool wr(FILE *f, const std::vector<T> &v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "candidates_plan: line %d: %s\n", __LINE__, #cond); \
      return false;                                                       \
    }                                                                     \
  } while (0)

static bool mapping_ok() {
  using namespace mipgpu;
  bool seen[256] = {};
  for (int rank = 0; rank < kCandRanks; rank++) {  // 99 distinct codes
    const uint8_t code = cand_code(rank);
    CHECK(!seen[code] && code != 0xff);
    seen[code] = true;
  }
  for (int v = 0; v < 32; v++) CHECK(cand_rank_mip(v) == v && cand_code(v) == v);
  CHECK(cand_rank_intra(0) == 32 && cand_code(32) == MIP_MODE_PLANAR && cand_rank_intra(1) == 33 && cand_code(33) == MIP_MODE_DC);
  for (int m = MIP_ANGULAR_FIRST; m <= MIP_ANGULAR_LAST; m++)
    CHECK(cand_rank_ang(m - 2) == 32 + m && cand_code(32 + m) == MIP_MODE_ANGULAR(m));
  // keys order by (value, rank); value and rank come back; the top of the domain fits
  const int32_t top = (1 << 24) - 1 - (1 << 20);
  CHECK(cand_key(5, 0, 98) < cand_key(6, 0, 0) && cand_key(5, 0, 3) < cand_key(5, 0, 4) && cand_key(4, 1, 7) == cand_key(5, 0, 7));
  CHECK(cand_key(top, kCandMaxBias, 98) < kCandNone && cand_key_value(cand_key(top, kCandMaxBias, 98)) == (1 << 24) - 1);
  CHECK(cand_key_code(cand_key(top, kCandMaxBias, 98)) == MIP_MODE_ANGULAR(66));
  CHECK(cand_key_code(kCandNone) == 0xff && cand_key_value(kCandNone) == MIP_COST_UNAVAILABLE);
  // absent entries: a MIP mode above 31, 0xff, MIP_COST_UNAVAILABLE in any family
  CHECK(cand_key_mip(32, 5) == kCandNone && cand_key_mip(0xff, 5) == kCandNone && cand_key_mip(200, 0) == kCandNone);
  CHECK(cand_key_mip(31, MIP_COST_UNAVAILABLE) == kCandNone && cand_key_mip(31, 5) == cand_key(5, 0, 31) && cand_key_mip(0, 0) == 0u);
  CHECK(cand_key_intra(0, MIP_COST_UNAVAILABLE, 9) == kCandNone && cand_key_intra(1, 7, 2) == cand_key(9, 0, 33));
  CHECK(cand_key_ang(64, MIP_COST_UNAVAILABLE, 9) == kCandNone && cand_key_ang(0, 7, 2) == cand_key(9, 0, 34));
  // values outside the domain wrap without touching the rank: the code stays the entry's own
  for (int32_t wild : {-1, -(1 << 30), 0x7ffffffe, 1 << 25}) {
    CHECK(cand_key_code(cand_key_ang(64, wild, kCandMaxBias)) == MIP_MODE_ANGULAR(66) && cand_key_ang(64, wild, kCandMaxBias) != kCandNone);
    CHECK(cand_key_code(cand_key_mip(31, wild)) == 31 && cand_key_code(cand_key_intra(1, wild, 0)) == MIP_MODE_DC);
  }
  // the rounds on a hand-made row: a three-way tie across the families goes MIP, Planar, angular;
  // absent entries are never taken; after the last candidate every round gives none
  const uint32_t row[6] = {cand_key_ang(0, 4, 0), kCandNone, cand_key_intra(0, 3, 1), cand_key_mip(7, 4), cand_key_mip(40, 0), cand_key_mip(2, 9)};
  const uint8_t want_mode[5] = {7, MIP_MODE_PLANAR, MIP_MODE_ANGULAR(2), 2, 0xff};
  const int32_t want_cost[5] = {4, 4, 4, 9, MIP_COST_UNAVAILABLE};
  uint32_t floor = 0;
  for (int r = 0; r < 6; r++) {
    uint32_t best = kCandNone;
    for (uint32_t key : row) best = cand_take(best, key, floor);
    floor = cand_floor(best);
    CHECK(cand_key_code(best) == want_mode[r < 4 ? r : 4] && cand_key_value(best) == want_cost[r < 4 ? r : 4]);
  }
  // rows: the families given side by side, an odd stride, at most 99 keys
  for (int fam = 1; fam < 8; fam++)
    for (int kin = 1; kin <= kCandMaxKin; kin++) {
      const CandRow w = cand_row(fam & 4, fam & 2, fam & 1 ? kin : 0);
      CHECK(w.n == (fam & 4 ? 65 : 0) + (fam & 2 ? 2 : 0) + (fam & 1 ? kin : 0) && w.n <= kCandMaxRow && w.stride >= w.n && w.stride % 2 == 1);
      CHECK(w.ang == 0 && w.intra == (fam & 4 ? 65 : 0) && w.mip == w.intra + (fam & 2 ? 2 : 0));
    }
  return true;
}

static bool rules_ok() {
  using namespace mipgpu;
  // one frame of 60x36: one CTU
  static uint8_t mm[5380 * 32], om[5380 * 32];
  static int32_t mc[5380 * 32], ic[5380 * 2], ac[5380 * 65], oc[5380 * 32];
  const int32_t zero[2] = {0, 0}, neg[2] = {0, -1}, big[2] = {kCandMaxBias + 1, 0}, top[2] = {kCandMaxBias, kCandMaxBias};
  auto rule = [&](int w, int h, int n, int k, const void *m, const void *c, int kin, const void *i, const int32_t *ib, const void *a,
                  int32_t ab, const void *o1, const void *o2) { return cand_args(w, h, n, k, m, c, kin, i, ib, a, ab, o1, o2); };
  CHECK(rule(60, 36, 1, 3, mm, mc, 3, ic, zero, ac, 0, om, oc) == kCandOk);
  CHECK(rule(60, 36, 1, 32, mm, mc, 32, ic, top, ac, kCandMaxBias, om, oc) == kCandOk);
  CHECK(rule(60, 36, 1, 1, nullptr, nullptr, 99, ic, nullptr, nullptr, -5, nullptr, oc) == kCandOk);  // kin, ang_bias not looked at
  CHECK(rule(60, 36, 1, 1, nullptr, nullptr, 0, nullptr, neg, ac, 0, om, nullptr) == kCandOk);        // intra_bias not looked at
  CHECK(rule(62, 36, 1, 3, mm, mc, 3, ic, zero, ac, 0, om, oc) == kCandGeometry && rule(60, 0, 1, 3, mm, mc, 3, ic, zero, ac, 0, om, oc) == kCandGeometry);
  CHECK(rule(60, 36, 0, 3, mm, mc, 3, ic, zero, ac, 0, om, oc) == kCandGeometry);
  CHECK(rule(60, 36, 1, 0, mm, mc, 3, ic, zero, ac, 0, om, oc) == kCandK && rule(60, 36, 1, 33, mm, mc, 3, ic, zero, ac, 0, om, oc) == kCandK);
  CHECK(rule(60, 36, 1, 3, mm, nullptr, 3, ic, zero, ac, 0, om, oc) == kCandMipPair && rule(60, 36, 1, 3, nullptr, mc, 3, ic, zero, ac, 0, om, oc) == kCandMipPair);
  CHECK(rule(60, 36, 1, 3, mm, mc, 0, ic, zero, ac, 0, om, oc) == kCandKin && rule(60, 36, 1, 3, mm, mc, 33, ic, zero, ac, 0, om, oc) == kCandKin);
  CHECK(rule(60, 36, 1, 3, nullptr, nullptr, 3, nullptr, zero, nullptr, 0, om, oc) == kCandNoFamily);
  CHECK(rule(60, 36, 1, 3, mm, mc, 3, ic, zero, ac, 0, nullptr, nullptr) == kCandNoOutput);
  CHECK(rule(60, 36, 1, 3, mm, mc, 3, ic, neg, ac, 0, om, oc) == kCandIntraBias && rule(60, 36, 1, 3, mm, mc, 3, ic, big, ac, 0, om, oc) == kCandIntraBias);
  CHECK(rule(60, 36, 1, 3, mm, mc, 3, ic, zero, ac, -1, om, oc) == kCandAngBias && rule(60, 36, 1, 3, mm, mc, 3, ic, zero, ac, kCandMaxBias + 1, om, oc) == kCandAngBias);
  CHECK(rule(60, 36, 1, 3, mm, mc, 3, ic, zero, (const char *)ac + 2, 0, om, oc) == kCandAlign && rule(60, 36, 1, 3, mm, mc, 3, ic, zero, ac, 0, om, (char *)oc + 1) == kCandAlign);
  CHECK(rule(60, 36, 1, 3, mm, mc, 3, ic, zero, (const char *)ac + 4, 0, om, oc) == kCandOk);  // 4-byte alignment is enough
  CHECK(rule(60, 36, 1, 3, mm, mc, 3, ic, zero, ac, 0, mm, oc) == kCandOverlap && rule(60, 36, 1, 3, mm, mc, 3, ic, zero, ac, 0, om, ac + 5380 * 65 - 1) == kCandOverlap);
  CHECK(rule(60, 36, 1, 3, mm, mc, 3, ic, zero, ac, 0, (uint8_t *)oc + 4, oc) == kCandOverlap);
  CHECK(rule(7680, 4320, 196, 3, mm, mc, 3, ic, zero, ac, 0, om, oc) == kCandTooMany);
  for (int c = kCandOk; c <= kCandTooMany; c++) CHECK(strlen(cand_args_text((CandArgs)c)) > 1);
  // a refused call writes nothing
  memset(om, 0x5a, sizeof om);
  CHECK(candidates_frames_host(60, 36, 1, 33, mm, mc, 3, ic, zero, ac, 0, om, oc) == -1 && om[0] == 0x5a && om[sizeof om - 1] == 0x5a);
  // the host chain: flags, k, and the arguments that are looked at only with their bit
  const uint8_t good[3] = {18, 34, 50}, bad[2] = {20, 20};
  CHECK(cand_chain_args(0, 3, neg, bad, 2, 9, -1) == kCandChainOk);
  CHECK(cand_chain_args(MIP_CAND_REGULAR | MIP_CAND_ANGULAR, 32, top, good, 3, 3, kCandMaxBias) == kCandChainOk);
  CHECK(cand_chain_args(MIP_CAND_ANGULAR, 1, neg, nullptr, 0, 0, 0) == kCandChainOk);
  CHECK(cand_chain_args(4u, 3, zero, good, 3, 0, 0) == kCandChainFlags && cand_chain_args(0x80000001u, 3, zero, good, 3, 0, 0) == kCandChainFlags);
  CHECK(cand_chain_args(0, 0, zero, good, 3, 0, 0) == kCandChainK && cand_chain_args(3, 33, zero, good, 3, 0, 0) == kCandChainK);
  CHECK(cand_chain_args(MIP_CAND_REGULAR, 3, neg, good, 3, 0, 0) == kCandChainIntraBias && cand_chain_args(1, 3, big, good, 3, 0, 0) == kCandChainIntraBias);
  CHECK(cand_chain_args(MIP_CAND_ANGULAR, 3, zero, bad, 2, 0, 0) == kCandChainModes && cand_chain_args(2, 3, zero, good, 0, 0, 0) == kCandChainModes);
  CHECK(cand_chain_args(MIP_CAND_ANGULAR, 3, zero, good, 3, 4, 0) == kCandChainSeeds && cand_chain_args(2, 3, zero, good, 3, -1, 0) == kCandChainSeeds);
  CHECK(cand_chain_args(MIP_CAND_ANGULAR, 3, zero, good, 3, 1, -1) == kCandChainAngBias && cand_chain_args(2, 3, zero, good, 3, 1, kCandMaxBias + 1) == kCandChainAngBias);
  return true;
}

int main(int argc, char **argv) {
  using namespace mipgpu;
  if (argc != 4 || strcmp(argv[1], "run")) {
    fprintf(stderr, "usage: test_candidates_plan run IN OUT\n");
    return 2;
  }
  if (!mapping_ok() || !rules_ok()) return 1;
  FILE *in = fopen(argv[2], "rb");
  int32_t hd[11];
  if (!in || fread(hd, sizeof(int32_t), 11, in) != 11) return 2;
  const int w = hd[0], h = hd[1], nf = hd[2], k = hd[3], kin = hd[4], fam = hd[5], outs = hd[6];
  const int32_t bias[2] = {hd[8], hd[9]};
  const size_t cus = (size_t)cand_cus(w, h, nf);
  // exactly-sized arrays: an index past a family's table or an output is a sanitizer report
  std::vector<uint8_t> mip_mode(fam & 1 ? cus * kin : 0), modes(outs & 1 ? cus * k : 0);
  std::vector<int32_t> mip_cost(fam & 1 ? cus * kin : 0), intra(fam & 2 ? cus * 2 : 0), ang(fam & 4 ? cus * 65 : 0), costs(outs & 2 ? cus * k : 0);
  if (!rd(in, mip_mode) || !rd(in, mip_cost) || !rd(in, intra) || !rd(in, ang) || fgetc(in) != EOF) return 2;
  fclose(in);
  if (candidates_frames_host(w, h, nf, k, fam & 1 ? mip_mode.data() : nullptr, fam & 1 ? mip_cost.data() : nullptr, kin,
                             fam & 2 ? intra.data() : nullptr, hd[7] ? bias : nullptr, fam & 4 ? ang.data() : nullptr, hd[10],
                             outs & 1 ? modes.data() : nullptr, outs & 2 ? costs.data() : nullptr) != 0)
    return 3;
  FILE *out = fopen(argv[3], "wb");
  if (!out || !wr(out, modes) || !wr(out, costs) || fclose(out) != 0) return 2;
  printf("candidates_plan: ok\n");
  return 0;
}

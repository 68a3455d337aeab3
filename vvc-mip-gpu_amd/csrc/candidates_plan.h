// candidates_plan.h -- the K-best candidate lists over MIP, Planar / DC and angular modes
// (include/mipgpu.h, mip_candidates_device) as arithmetic shared by the kernel
// (mip_candidates.hip: one lane per CU, its keys in one LDS row) and by the host walk below
// (candidates_frames_host: the same steps, one CU at a time): the rank and code mapping, the
// candidate predicate of every family, the 32-bit (value, rank) key, the selection step, the row
// layout, and the argument rules of both entry points.  No HIP dependency on the host side;
// unit-tested by tests/cpp/test_candidates_plan.cpp.
#pragma once
#include "angular_plan.h"

namespace mipgpu {

constexpr int kCandMaxK = MIP_CAND_MAX_K;
constexpr int kCandMaxKin = 32;
constexpr int32_t kCandMaxBias = 1 << 20;
constexpr int kCandRanks = 99;  // 32 MIP modes, Planar, DC, 65 angular modes

// ---- ranks and codes.  MIP mode v: rank v, code v.  Planar: rank 32; DC: rank 33.  Angular mode
// m (2..66): rank 32 + m, code MIP_MODE_ANGULAR(m).
MIP_INTRA_HD int cand_rank_mip(int mode) { return mode; }
MIP_INTRA_HD int cand_rank_intra(int slot) { return 32 + slot; }
MIP_INTRA_HD int cand_rank_ang(int slot) { return 32 + MIP_ANGULAR_FIRST + slot; }
MIP_INTRA_HD uint8_t cand_code(int rank) {
  return (uint8_t)(rank < 32 ? rank : rank == 32 ? MIP_MODE_PLANAR : rank == 33 ? MIP_MODE_DC : MIP_MODE_ANGULAR(rank - 32));
}

// ---- keys.  A candidate is value << 7 | rank: values stay below 1 << 24 (table values at most
// (1 << 24) - 1 - (1 << 20), biases at most 1 << 20) and ranks below 99, so keys of one CU are
// unique 31-bit numbers ordered by (value, rank); an absent entry is kCandNone.  The rank bits are
// never touched by the value (unsigned arithmetic: a value outside the domain wraps, the code
// stays one of the 99), and the low seven bits of a key are never all ones, so no key is kCandNone.
constexpr uint32_t kCandNone = 0xffffffffu;
MIP_INTRA_HD uint32_t cand_key(int32_t value, int32_t bias, int rank) { return ((uint32_t)value + (uint32_t)bias) << 7 | (uint32_t)rank; }
// the predicates: what makes an entry of a family's input a candidate
MIP_INTRA_HD uint32_t cand_key_mip(uint8_t mode, int32_t cost) {
  return mode <= 31 && cost != MIP_COST_UNAVAILABLE ? cand_key(cost, 0, cand_rank_mip(mode)) : kCandNone;
}
MIP_INTRA_HD uint32_t cand_key_intra(int slot, int32_t cost, int32_t bias) {
  return cost != MIP_COST_UNAVAILABLE ? cand_key(cost, bias, cand_rank_intra(slot)) : kCandNone;
}
MIP_INTRA_HD uint32_t cand_key_ang(int slot, int32_t cost, int32_t bias) {
  return cost != MIP_COST_UNAVAILABLE ? cand_key(cost, bias, cand_rank_ang(slot)) : kCandNone;
}
MIP_INTRA_HD uint8_t cand_key_code(uint32_t key) { return key == kCandNone ? (uint8_t)0xff : cand_code((int)(key & 127u)); }
MIP_INTRA_HD int32_t cand_key_value(uint32_t key) { return key == kCandNone ? MIP_COST_UNAVAILABLE : (int32_t)(key >> 7); }

// ---- selection.  Keys are unique, so round r takes the lowest key that is >= floor, where floor
// is one above the key of round r - 1 (0 in round 0): no used-mask, no array indexed by the round.
// cand_take folds one key into the round's minimum; cand_floor gives the next round's floor, and
// stays at kCandNone once a round has found nothing (only absent entries are left).
MIP_INTRA_HD uint32_t cand_take(uint32_t best, uint32_t key, uint32_t floor) {
  const uint32_t c = key >= floor ? key : kCandNone;
  return c < best ? c : best;
}
MIP_INTRA_HD uint32_t cand_floor(uint32_t taken) { return taken == kCandNone ? kCandNone : taken + 1u; }

// ---- the key row of one CU: the families that are given, side by side -- angular slots, Planar /
// DC, the MIP list -- n keys at a stride that is odd, so that the rows of 64 consecutive CUs start
// in 64 different LDS banks.
struct CandRow {
  int ang, intra, mip;  // first key of the family's part (the part is empty if the family is not given)
  int n, stride;
};
MIP_INTRA_HD CandRow cand_row(bool has_ang, bool has_intra, int kin_or_0) {
  CandRow r;
  r.ang = 0;
  r.intra = has_ang ? kAngModes : 0;
  r.mip = r.intra + (has_intra ? kIntraModes : 0);
  r.n = r.mip + kin_or_0;
  r.stride = r.n | 1;
  return r;
}
constexpr int kCandMaxRow = kAngModes + kIntraModes + kCandMaxKin;  // 99 keys

// ---- argument rules of mip_candidates_device (before any launch; nothing is written)
enum CandArgs {
  kCandOk = 0,
  kCandGeometry,   // width, height, nframes
  kCandK,          // k outside 1..MIP_CAND_MAX_K
  kCandMipPair,    // d_mip_mode / d_mip_cost not given together
  kCandKin,        // kin outside 1..32 with a MIP list
  kCandNoFamily,
  kCandNoOutput,
  kCandIntraBias,  // outside 0..1<<20 with a Planar / DC table
  kCandAngBias,    // outside 0..1<<20 with an angular table
  kCandAlign,      // an int32 pointer that is not 4-byte aligned
  kCandOverlap,    // an output overlaps an input
  kCandTooMany,    // more CUs than one launch takes
};
inline const char *cand_args_text(CandArgs c) {
  switch (c) {
    case kCandOk: return "ok";
    case kCandGeometry: return "bad candidates arguments: width, height (multiples of 4) or nframes";
    case kCandK: return "candidates: k must be 1..32";
    case kCandMipPair: return "candidates: d_mip_mode and d_mip_cost are given together";
    case kCandKin: return "candidates: kin must be 1..32";
    case kCandNoFamily: return "candidates: no family given";
    case kCandNoOutput: return "candidates: no output given";
    case kCandIntraBias: return "candidates: an intra bias is outside 0..1048576";
    case kCandAngBias: return "candidates: the angular bias is outside 0..1048576";
    case kCandAlign: return "candidates: int32 arrays must be 4-byte aligned";
    case kCandOverlap: return "candidates: an output overlaps an input";
    case kCandTooMany: return "candidates: too many CUs for one call";
  }
  return "candidates: bad arguments";
}
inline bool cand_bias_ok(int32_t bias) { return bias >= 0 && bias <= kCandMaxBias; }
inline long long cand_cus(int width, int height, int nframes) {
  return (long long)nframes * ((width + 127) / 128) * ((height + 127) / 128) * MIP_CUS_PER_CTU;
}
inline CandArgs cand_args(int width, int height, int nframes, int k, const void *mip_mode, const void *mip_cost, int kin,
                          const void *intra_cost, const int32_t *intra_bias, const void *ang_cost, int32_t ang_bias, const void *modes,
                          const void *costs) {
  if (width <= 0 || height <= 0 || width % 4 || height % 4 || nframes < 1) return kCandGeometry;
  if (k < 1 || k > kCandMaxK) return kCandK;
  if (!mip_mode != !mip_cost) return kCandMipPair;
  if (mip_mode && (kin < 1 || kin > kCandMaxKin)) return kCandKin;
  if (!mip_mode && !intra_cost && !ang_cost) return kCandNoFamily;
  if (!modes && !costs) return kCandNoOutput;
  if (intra_cost && intra_bias && !(cand_bias_ok(intra_bias[0]) && cand_bias_ok(intra_bias[1]))) return kCandIntraBias;
  if (ang_cost && !cand_bias_ok(ang_bias)) return kCandAngBias;
  for (const void *p : {mip_cost, intra_cost, ang_cost, costs})
    if (reinterpret_cast<uintptr_t>(p) & 3) return kCandAlign;
  const long long cus = cand_cus(width, height, nframes);
  if (cus > (1LL << 31) - 256) return kCandTooMany;
  // byte ranges: an output may not share a byte with an input, nor with the other output
  struct Range {
    uintptr_t at;
    unsigned long long bytes;
  };
  const Range in[4] = {{reinterpret_cast<uintptr_t>(mip_mode), mip_mode ? (unsigned long long)cus * kin : 0},
                       {reinterpret_cast<uintptr_t>(mip_cost), mip_cost ? (unsigned long long)cus * kin * 4 : 0},
                       {reinterpret_cast<uintptr_t>(intra_cost), intra_cost ? (unsigned long long)cus * kIntraModes * 4 : 0},
                       {reinterpret_cast<uintptr_t>(ang_cost), ang_cost ? (unsigned long long)cus * kAngModes * 4 : 0}};
  const Range out[2] = {{reinterpret_cast<uintptr_t>(modes), modes ? (unsigned long long)cus * k : 0},
                        {reinterpret_cast<uintptr_t>(costs), costs ? (unsigned long long)cus * k * 4 : 0}};
  auto meet = [](const Range &a, const Range &b) { return a.bytes && b.bytes && a.at < b.at + b.bytes && b.at < a.at + a.bytes; };
  for (const Range &o : out)
    for (const Range &i : in)
      if (meet(o, i)) return kCandOverlap;
  if (meet(out[0], out[1])) return kCandOverlap;
  return kCandOk;
}

// ---- argument rules of mip_candidates_frames beyond the device call's (before any launch).
// The angular arguments are looked at only with MIP_CAND_ANGULAR; *refine: ang_seeds != 0.
enum CandChainArgs { kCandChainOk = 0, kCandChainFlags, kCandChainK, kCandChainIntraBias, kCandChainModes, kCandChainSeeds, kCandChainAngBias };
inline CandChainArgs cand_chain_args(unsigned flags, int k, const int32_t *intra_bias, const uint8_t *ang_modes, int ang_nmodes,
                                     int ang_seeds, int32_t ang_bias) {
  if (flags & ~(MIP_CAND_REGULAR | MIP_CAND_ANGULAR)) return kCandChainFlags;
  if (k < 1 || k > kCandMaxK) return kCandChainK;
  if ((flags & MIP_CAND_REGULAR) && intra_bias && !(cand_bias_ok(intra_bias[0]) && cand_bias_ok(intra_bias[1]))) return kCandChainIntraBias;
  if (flags & MIP_CAND_ANGULAR) {
    AngList list;
    if (!ang_list(ang_modes, ang_nmodes, &list)) return kCandChainModes;
    if (ang_seeds != 0 && !ang_seeds_ok(ang_seeds)) return kCandChainSeeds;
    if (!cand_bias_ok(ang_bias)) return kCandChainAngBias;
  }
  return kCandChainOk;
}

// ---- host side: the keys of one CU (the row the kernel stages in LDS), the rounds, the walk.
// Everything mip_candidates_device writes, on host arrays of exactly the contract's sizes.
// Returns 0, or -1 for arguments the entry point rejects (nothing written).
inline int candidates_frames_host(int width, int height, int nframes, int k, const uint8_t *mip_mode, const int32_t *mip_cost, int kin,
                                  const int32_t *intra_cost, const int32_t *intra_bias, const int32_t *ang_cost, int32_t ang_bias,
                                  uint8_t *modes, int32_t *costs) {
  if (cand_args(width, height, nframes, k, mip_mode, mip_cost, kin, intra_cost, intra_bias, ang_cost, ang_bias, modes, costs) != kCandOk)
    return -1;
  const CandRow row = cand_row(ang_cost != nullptr, intra_cost != nullptr, mip_mode ? kin : 0);
  const size_t cus = (size_t)cand_cus(width, height, nframes);
  for (size_t g = 0; g < cus; g++) {
    uint32_t key[kCandMaxRow];
    if (ang_cost)
      for (int slot = 0; slot < kAngModes; slot++) key[row.ang + slot] = cand_key_ang(slot, ang_cost[g * kAngModes + slot], ang_bias);
    if (intra_cost)
      for (int slot = 0; slot < kIntraModes; slot++)
        key[row.intra + slot] = cand_key_intra(slot, intra_cost[g * kIntraModes + slot], intra_bias ? intra_bias[slot] : 0);
    if (mip_mode)
      for (int r = 0; r < kin; r++) key[row.mip + r] = cand_key_mip(mip_mode[g * kin + r], mip_cost[g * kin + r]);
    uint32_t floor = 0;
    for (int r = 0; r < k; r++) {
      uint32_t best = kCandNone;
      for (int j = 0; j < row.n; j++) best = cand_take(best, key[j], floor);
      floor = cand_floor(best);
      if (modes) modes[g * k + r] = cand_key_code(best);
      if (costs) costs[g * k + r] = cand_key_value(best);
    }
  }
  return 0;
}

}  // namespace mipgpu

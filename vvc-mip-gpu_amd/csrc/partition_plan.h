// partition_plan.h -- the CTU partition search (include/mipgpu.h, mip_partition_device) as a
// walk over the generated state graph (partition_tables.h): the per-state steps, shared by
// the kernel (mip_partition.hip runs the states of one level in parallel) and by the host
// restatement below (partition_ctu / partition_frames: the same steps, one state at a time).
// No HIP dependency on the host side; unit-tested by tests/cpp/test_partition_plan.cpp.
//
// One CTU has 16 * 640 binary/ternary states (block * 640 + local, block = 4*by + bx of the
// 32x32 block, local = index in the block template), four 64x64 nodes and the root.  The
// bottom-up pass gives every state its best cost and the candidate that reached it; the
// top-down pass marks the states of the chosen tree; marked states whose choice is "leaf" are
// the partition.
#pragma once
#include <stdint.h>

#include "mipgpu.h"
#include "partition_tables.h"

#if defined(__HIPCC__)
#define MIP_PART_HD __host__ __device__ inline
#else
#define MIP_PART_HD inline
#endif

namespace mipgpu {

constexpr int kPartBlockStates = MIP_PART_BLOCK_STATES;
constexpr int kPartBtStates = MIP_PART_BLOCKS * MIP_PART_BLOCK_STATES;  // 10240
constexpr int kPartNode64 = kPartBtStates;                              // + quadrant (2*qy + qx)
constexpr int kPartRoot = kPartBtStates + 4;
constexpr int kPartStates = kPartBtStates + 5;
constexpr int kPartLevels[MIP_PART_NUM_LEVELS + 1] = MIP_PART_LEVELS;
constexpr int kPartShapes = 47;
constexpr int32_t kPartMaxPenalty = 1 << 20;
// Infinity is a value of its own (== MIP_COST_UNAVAILABLE, which is also what a CTU without a
// partition reports): sums test their terms for it, they never reach it by overflow.
constexpr int32_t kPartInf = MIP_COST_UNAVAILABLE;
// choice byte of a state: the candidate taken (candidate order of the contract) | kPartMark
enum : uint8_t { kPartLeaf = 0, kPartBtH = 1, kPartBtV = 2, kPartTtH = 3, kPartTtV = 4, kPartQt = 5, kPartNone = 7, kPartMark = 0x80 };

// The tables as the walk reads them: the host's constexpr copies (part_host_tables) or the
// kernel's copies in LDS.
struct PartTables {
  const mip_part_state *state;                 // [640]
  const uint16_t (*child)[10];                 // [366]
  const uint16_t (*qt)[4];                     // [5]
  const mip_part_step *step;                   // [47]
};

// The frame and the CTU's place in it.
struct PartCtu {
  int width, height, cx, cy;
};

// The CU of a state: index inside the CTU, shape, CTU-relative position.
struct PartCu {
  int cu, shape, x, y, w, h;
};

MIP_PART_HD PartCu part_state_cu(const PartTables &t, int block, int local) {
  const mip_part_state &s = t.state[local];
  const mip_part_step &p = t.step[s.shape];
  const int bx = block & 3, by = block >> 2;
  return PartCu{s.cu0 + bx * p.dx + p.dy[by], s.shape + (by >= 2 ? p.hi : 0), 32 * bx + s.x, 32 * by + s.y, s.w, s.h};
}

MIP_PART_HD bool part_outside(const PartCtu &f, int x, int y) { return f.cx + x >= f.width || f.cy + y >= f.height; }

// Leaf candidate of a region that is a CU: eligible only wholly inside the frame and available.
MIP_PART_HD int32_t part_leaf_cost(const PartCtu &f, const int32_t *best_cost, const int32_t *penalty, const PartCu &g) {
  if (f.cx + g.x + g.w > f.width || f.cy + g.y + g.h > f.height) return kPartInf;
  const int32_t c = best_cost[g.cu];
  if (c == MIP_COST_UNAVAILABLE) return kPartInf;
  return (int32_t)((uint32_t)c + (uint32_t)penalty[g.shape]);  // (wraps for costs past the contract: defined)
}

// Cost of a split: the sum of its children's costs, infinite if any child is.
MIP_PART_HD int32_t part_split_cost(const int32_t *cost, int base, const uint16_t *child, int n) {
  uint32_t sum = 0;
  bool inf = false;
  for (int i = 0; i < n; i++) {
    const int32_t c = cost[base + child[i]];
    inf |= c == kPartInf;
    sum += (uint32_t)c;
  }
  return inf ? kPartInf : (int32_t)sum;
}

// A later candidate replaces the current one only if it is strictly cheaper.
MIP_PART_HD void part_take(int32_t c, uint8_t k, int32_t &best, uint8_t &choice) {
  if (c != kPartInf && c < best) best = c, choice = k;
}

// Bottom-up step of binary/ternary state (block, local); its children (deeper levels, and for
// the quad split the smaller nodes of depth 0) are done.
MIP_PART_HD void part_eval_state(const PartTables &t, const PartCtu &f, const int32_t *best_cost, const int32_t *penalty,
                                 int32_t *cost, uint8_t *choice, int block, int local) {
  const int base = block * kPartBlockStates, id = base + local;
  const PartCu g = part_state_cu(t, block, local);
  if (part_outside(f, g.x, g.y)) {  // costs nothing, holds no leaf
    cost[id] = 0;
    choice[id] = kPartNone;
    return;
  }
  int32_t best = part_leaf_cost(f, best_cost, penalty, g);
  uint8_t ch = best != kPartInf ? kPartLeaf : kPartNone;
  if (local < MIP_PART_SPLIT_STATES) {
    const uint16_t *c = t.child[local];
    if (c[0] != 0xffff) part_take(part_split_cost(cost, base, c, 2), kPartBtH, best, ch);
    if (c[2] != 0xffff) part_take(part_split_cost(cost, base, c + 2, 2), kPartBtV, best, ch);
    if (c[4] != 0xffff) part_take(part_split_cost(cost, base, c + 4, 3), kPartTtH, best, ch);
    if (c[7] != 0xffff) part_take(part_split_cost(cost, base, c + 7, 3), kPartTtV, best, ch);
    if (local < MIP_PART_QT_STATES) part_take(part_split_cost(cost, base, t.qt[local], 4), kPartQt, best, ch);
  }
  cost[id] = best;
  choice[id] = ch;
}

// The 32x32 nodes (state 0 of their blocks) under 64x64 node q, relative to state 0.
MIP_PART_HD void part_node64_children(int q, uint16_t *child) {
  for (int i = 0; i < 4; i++) child[i] = (uint16_t)(((2 * (q >> 1) + (i >> 1)) * 4 + 2 * (q & 1) + (i & 1)) * kPartBlockStates);
}

// Bottom-up step of 64x64 node q: the 64x64 CU (CU q of the CTU, shape 0) or a quad split.
MIP_PART_HD void part_eval_node64(const PartCtu &f, const int32_t *best_cost, const int32_t *penalty, int32_t *cost,
                                  uint8_t *choice, int q) {
  const PartCu g{q, 0, 64 * (q & 1), 64 * (q >> 1), 64, 64};
  if (part_outside(f, g.x, g.y)) {
    cost[kPartNode64 + q] = 0;
    choice[kPartNode64 + q] = kPartNone;
    return;
  }
  int32_t best = part_leaf_cost(f, best_cost, penalty, g);
  uint8_t ch = best != kPartInf ? kPartLeaf : kPartNone;
  uint16_t child[4];
  part_node64_children(q, child);
  part_take(part_split_cost(cost, 0, child, 4), kPartQt, best, ch);
  cost[kPartNode64 + q] = best;
  choice[kPartNode64 + q] = ch;
}

// The root is never a leaf; it is marked when it has a partition.
MIP_PART_HD void part_eval_root(int32_t *cost, uint8_t *choice) {
  const uint16_t child[4] = {0, 1, 2, 3};
  const int32_t c = part_split_cost(cost, kPartNode64, child, 4);
  cost[kPartRoot] = c;
  choice[kPartRoot] = c != kPartInf ? (uint8_t)(kPartQt | kPartMark) : (uint8_t)kPartNone;
}

MIP_PART_HD void part_mark(uint8_t *choice, int base, const uint16_t *child, int n) {
  for (int i = 0; i < n; i++) choice[base + child[i]] |= kPartMark;
}

// Top-down steps: a marked node that split marks its children.
MIP_PART_HD void part_mark_root(uint8_t *choice) {
  const uint16_t child[4] = {0, 1, 2, 3};
  if (choice[kPartRoot] & kPartMark) part_mark(choice, kPartNode64, child, 4);
}
MIP_PART_HD void part_mark_node64(uint8_t *choice, int q) {
  if (choice[kPartNode64 + q] != (kPartQt | kPartMark)) return;
  uint16_t child[4];
  part_node64_children(q, child);
  part_mark(choice, 0, child, 4);
}
MIP_PART_HD void part_mark_state(const PartTables &t, uint8_t *choice, int block, int local) {
  const int base = block * kPartBlockStates;
  const uint8_t c = choice[base + local];
  if (!(c & kPartMark) || local >= MIP_PART_SPLIT_STATES) return;
  const uint16_t *ch = t.child[local];
  switch (c & 7) {
    case kPartBtH: part_mark(choice, base, ch, 2); break;
    case kPartBtV: part_mark(choice, base, ch + 2, 2); break;
    case kPartTtH: part_mark(choice, base, ch + 4, 3); break;
    case kPartTtV: part_mark(choice, base, ch + 7, 3); break;
    case kPartQt: part_mark(choice, base, t.qt[local < MIP_PART_QT_STATES ? local : 0], 4); break;
    default: break;
  }
}

// Leaves are kept per CU as 1 + the CU's position in 4-sample units (x/4 + 32*(y/4)); 0 = not
// a leaf.
MIP_PART_HD uint16_t part_leaf_word(int x, int y) { return (uint16_t)(1 + (x >> 2) + 32 * (y >> 2)); }
MIP_PART_HD void part_collect_state(const PartTables &t, const uint8_t *choice, uint16_t *leaf, int block, int local) {
  if (choice[block * kPartBlockStates + local] != (kPartLeaf | kPartMark)) return;
  const PartCu g = part_state_cu(t, block, local);
  leaf[g.cu] = part_leaf_word(g.x, g.y);
}
MIP_PART_HD void part_collect_node64(const uint8_t *choice, uint16_t *leaf, int q) {
  if (choice[kPartNode64 + q] == (kPartLeaf | kPartMark)) leaf[q] = part_leaf_word(64 * (q & 1), 64 * (q >> 1));
}

// The list entry of leaf CU k of CTU `ctu` (MIP_PRED_FRAME layout), and the padding entry.
MIP_PART_HD mip_pred_item part_item(const PartCtu &f, int frame, int ctu, int k, uint16_t leaf_word, int mode) {
  const int p = leaf_word - 1, x = f.cx + 4 * (p & 31), y = f.cy + 4 * (p >> 5);
  return mip_pred_item{frame, ctu * MIP_CUS_PER_CTU_ABI + k, mode, f.width,
                       (int64_t)frame * f.width * f.height + (int64_t)y * f.width + x};
}
MIP_PART_HD mip_pred_item part_pad_item() { return mip_pred_item{-1, -1, -1, 0, 0}; }

// ---- host side: the tables and the walk, one state at a time
inline constexpr mip_part_state kPartStateTable[MIP_PART_BLOCK_STATES] = MIP_PART_STATE_TABLE;
inline constexpr uint16_t kPartChildTable[MIP_PART_SPLIT_STATES][10] = MIP_PART_CHILD_TABLE;
inline constexpr uint16_t kPartQtTable[MIP_PART_QT_STATES][4] = MIP_PART_QT_TABLE;
inline constexpr mip_part_step kPartStepTable[kPartShapes] = MIP_PART_STEP_TABLE;
inline PartTables part_host_tables() { return PartTables{kPartStateTable, kPartChildTable, kPartQtTable, kPartStepTable}; }

inline bool part_penalty_ok(const int32_t *penalty) {
  for (int s = 0; penalty && s < kPartShapes; s++)
    if (penalty[s] < 0 || penalty[s] > kPartMaxPenalty) return false;
  return true;
}

// Scratch of one CTU's walk (host).
struct PartScratch {
  int32_t cost[kPartStates];
  uint8_t choice[kPartStates];
  uint16_t leaf[MIP_CUS_PER_CTU_ABI];
};

// One CTU: best_cost = the CTU's 5380 costs, penalty[47].  leaf[k] (see part_leaf_word) for the
// CTU's 5380 CUs; returns the CTU's cost (kPartInf: no partition) and the number of leaves.
inline int32_t partition_ctu(const PartCtu &f, const int32_t *best_cost, const int32_t *penalty, PartScratch &w,
                             int *nleaves) {
  const PartTables t = part_host_tables();
  // bottom-up: depth 3 -> 1, then the quad-tree levels 8 -> 128
  for (int lv = MIP_PART_NUM_LEVELS - 1; lv >= 0; lv--)
    for (int b = 0; b < MIP_PART_BLOCKS; b++)
      for (int s = kPartLevels[lv]; s < kPartLevels[lv + 1]; s++) part_eval_state(t, f, best_cost, penalty, w.cost, w.choice, b, s);
  for (int q = 0; q < 4; q++) part_eval_node64(f, best_cost, penalty, w.cost, w.choice, q);
  part_eval_root(w.cost, w.choice);
  // top-down: 128, 64, 32, 16, 8, then depth 1, 2 (depth 3 has no children)
  part_mark_root(w.choice);
  for (int q = 0; q < 4; q++) part_mark_node64(w.choice, q);
  for (int lv = 0; lv < MIP_PART_NUM_LEVELS - 1; lv++)
    for (int b = 0; b < MIP_PART_BLOCKS; b++)
      for (int s = kPartLevels[lv]; s < kPartLevels[lv + 1]; s++) part_mark_state(t, w.choice, b, s);
  for (int k = 0; k < MIP_CUS_PER_CTU_ABI; k++) w.leaf[k] = 0;
  for (int q = 0; q < 4; q++) part_collect_node64(w.choice, w.leaf, q);
  for (int b = 0; b < MIP_PART_BLOCKS; b++)
    for (int s = 0; s < kPartBlockStates; s++) part_collect_state(t, w.choice, w.leaf, b, s);
  int n = 0;
  for (int k = 0; k < MIP_CUS_PER_CTU_ABI; k++) n += w.leaf[k] != 0;
  *nleaves = n;
  return w.cost[kPartRoot];
}

// mip_partition_device on host arrays (same outputs, each optional).  Returns 0, or -1 for
// arguments the entry point rejects.
inline int partition_frames(const int32_t *best_cost, const uint8_t *best_mode, int width, int height, int nframes,
                            const int32_t *penalty, uint8_t *leaf, int32_t *ctu_cost, int32_t *ctu_leaves,
                            mip_pred_item *items) {
  if (!best_cost || width <= 0 || height <= 0 || width % 4 || height % 4 || nframes < 1) return -1;
  if ((!leaf && !ctu_cost && !ctu_leaves && !items) || (items && !best_mode) || !part_penalty_ok(penalty)) return -1;
  const int32_t zero[kPartShapes] = {};
  const int cols = (width + 127) / 128, nctus = cols * ((height + 127) / 128);
  PartScratch *w = new PartScratch;
  for (int fr = 0; fr < nframes; fr++)
    for (int c = 0; c < nctus; c++) {
      const size_t g = (size_t)fr * nctus + c;
      const PartCtu f{width, height, 128 * (c % cols), 128 * (c / cols)};
      int n = 0;
      const int32_t total = partition_ctu(f, best_cost + g * MIP_CUS_PER_CTU_ABI, penalty ? penalty : zero, *w, &n);
      if (ctu_cost) ctu_cost[g] = total;
      if (ctu_leaves) ctu_leaves[g] = n;
      int at = 0;
      for (int k = 0; k < MIP_CUS_PER_CTU_ABI; k++) {
        if (leaf) leaf[g * MIP_CUS_PER_CTU_ABI + k] = w->leaf[k] != 0;
        if (items && w->leaf[k] && at < MIP_PART_MAX_LEAVES)
          items[g * MIP_PART_MAX_LEAVES + at++] = part_item(f, fr, c, k, w->leaf[k], best_mode[g * MIP_CUS_PER_CTU_ABI + k]);
      }
      for (; items && at < MIP_PART_MAX_LEAVES; at++) items[g * MIP_PART_MAX_LEAVES + at] = part_pad_item();
    }
  delete w;
  return 0;
}

}  // namespace mipgpu

// mip_angular_dev.h -- device helpers shared by the two angular cost kernels (mip_angular.hip,
// mip_angular_refine.hip) on top of mip_window_dev.h (items, window staging, LdsRef, group_sum,
// load_org, launch rules): the two boundary lines of a CU in the staged window, the steps of the
// 64x64 CU's path through s_sum and s_tab, the steps of a lane slot of a 32x32 block, and the finish
// of a CU.  As there, the helpers take pointers and scalars, never a kernel's argument struct by
// reference.  Internal linkage: each kernel file has its own copies.  DESIGN.md sections 5.7, 5.9.
#pragma once
#include "angular_plan.h"
#include "mip_window_dev.h"

namespace mipgpu {
namespace {

// The two boundary lines of a CU as a Bound of angular_plan.h: top[t] and left[t] each lie on a
// line of the staged window, at s_ref index base + t * stride (stride 0 for the substitutes of
// the first frame row and column; the 512 of the frame's corner sits in a cell of its own).  The
// bases and strides come from intra_plan.h's own rules, evaluated on a Ref that returns a
// sample's window index instead of its value.
constexpr int kConstAt = kLeftAt + 66;  // the cell that holds 512
constexpr int kIndexBias = 4096;        // (keeps a window index apart from the literal 512)
struct IndexRef {
  int x0, y0, lp;
  __device__ __forceinline__ int operator()(int row, int col) const {
    const int r = row - y0 + 1;
    return kIndexBias + (col >= x0 ? (r << lp) + col - x0 : kLeftAt + r);
  }
};
struct LdsBound {
  const uint16_t *ref;
  int w, h, tb, ts, lb, ls, corner_value;
  __device__ __forceinline__ LdsBound(const LdsRef &win, int x, int y, int w_, int h_) : ref(win.ref), w(w_), h(h_) {
    const IndexRef ir{win.x0, win.y0, win.lp};
    const int t0 = intra_top(ir, x, y, 0), l0 = intra_left(ir, x, y, 0);
    ts = intra_top(ir, x, y, 1) - t0;
    ls = intra_left(ir, x, y, 1) - l0;
    tb = t0 == 512 ? kConstAt : t0 - kIndexBias;
    lb = l0 == 512 ? kConstAt : l0 - kIndexBias;
    corner_value = x > 0 && y > 0 ? win(y - 1, x - 1) : ref[tb];
  }
  __device__ __forceinline__ int sample(bool top_line, int t) const { return ref[(top_line ? tb : lb) + t * (top_line ? ts : ls)]; }
  __device__ __forceinline__ int corner() const { return corner_value; }
};
static_assert(kConstAt > kLeftAt + 64 && kConstAt < kRefCells, "the constant's cell lies behind s_left");

// ---- the 64x64 CU: 256 lanes, one CU.  The waves leave their (sad, satd) per list entry (then per
// candidate) in s_sum; finish_slot adds the four waves' into s_tab (cost, sad, satd per table slot),
// which one lane per slot then writes out.
using WaveSums = int[kAngModes][2];  // s_sum[kThreads / 64]
using CuTable = int[kAngModes];      // s_tab[3]
__device__ __forceinline__ void finish_slot(const WaveSums *s_sum, CuTable *s_tab, int q, int slot) {
  const int sad = s_sum[0][q][0] + s_sum[1][q][0] + s_sum[2][q][0] + s_sum[3][q][0];
  const int satd = s_sum[0][q][1] + s_sum[1][q][1] + s_sum[2][q][1] + s_sum[3][q][1];
  s_tab[0][slot] = intra_cost(sad, satd);
  s_tab[1][slot] = sad;
  s_tab[2][slot] = satd;
}
__device__ __forceinline__ void reset_table(CuTable *s_tab, bool big, int tid) {
  if (big && tid < kAngModes) s_tab[0][tid] = s_tab[1][tid] = s_tab[2][tid] = MIP_COST_UNAVAILABLE;
}
__device__ __forceinline__ void flush_table(const CuTable *s_tab, int tid, size_t cu, int32_t *cost, int32_t *sad, int32_t *satd) {
  if (tid < kAngModes) {
    if (cost) cost[cu * kAngModes + tid] = s_tab[0][tid];
    if (sad) sad[cu * kAngModes + tid] = s_tab[1][tid];
    if (satd) satd[cu * kAngModes + tid] = s_tab[2][tid];
  }
}

// ---- a 32x32 block: one lane per 4x4 block of a CU.  The lane's slot: its block, the lanes of
// its group, whether it is the lane that writes the CU (first), whether that CU is available (on:
// false in every other lane) and the CU's index in the batch.
struct SlotCu {
  IntraSlot c;  // (no slot: fields of CU 0 at the window's corner, nothing written)
  int n;
  bool first, on;
  size_t cu;
};
__device__ __forceinline__ SlotCu slot_cu(uint32_t word, const uint8_t *unavail, int ctu, size_t cu_base) {
  SlotCu s;
  s.c = intra_slot_decode(word);
  s.n = 1 << (s.c.lw + s.c.lh - 4);
  s.first = !(word & kIntraNoSlot) && (s.c.bi | s.c.bj) == 0;
  s.on = s.first && !unavail[(size_t)ctu * MIP_CUS_PER_CTU + s.c.cu];
  s.cu = cu_base + s.c.cu;
  return s;
}
// One mode's table entries of a CU; returns its cost.
__device__ __forceinline__ int32_t write_slot(int32_t *cost, int32_t *sad, int32_t *satd, size_t cu, int m, int sad_m, int satd_m) {
  const int32_t c = intra_cost(sad_m, satd_m);
  const size_t to = cu * kAngModes + m - MIP_ANGULAR_FIRST;
  if (cost) cost[to] = c;
  if (sad) sad[to] = sad_m;
  if (satd) satd[to] = satd_m;
  return c;
}
// The slots of modes not in the list, every slot of an unavailable CU.
__device__ __forceinline__ void clear_unlisted(int32_t *cost, int32_t *sad, int32_t *satd, size_t cu, bool on, const uint32_t *listed) {
  for (int slot = 0; slot < kAngModes; slot++)
    if (!on || !ang_listed(listed, slot)) {
      if (cost) cost[cu * kAngModes + slot] = MIP_COST_UNAVAILABLE;
      if (sad) sad[cu * kAngModes + slot] = MIP_COST_UNAVAILABLE;
      if (satd) satd[cu * kAngModes + slot] = MIP_COST_UNAVAILABLE;
    }
}
// The CU's ang pair and its decision.  One lane per CU; on = the CU is available.
__device__ __forceinline__ void write_best(const AngularArgs &a, size_t cu, bool on, uint8_t mode, int32_t cost) {
  if (a.ang_cost) {
    a.ang_mode[cu] = mode;
    a.ang_cost[cu] = cost;
  }
  if (a.best_cost && on) {
    uint8_t bm = a.best_mode[cu];
    int32_t bc = a.best_cost[cu];
    const int32_t before = bc;
    ang_merge(bm, bc, mode, cost, a.bias);
    if (bc != before) {
      a.best_mode[cu] = bm;
      a.best_cost[cu] = bc;
    }
  }
}

}  // namespace
}  // namespace mipgpu

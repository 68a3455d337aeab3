// mip_angular_dev.h -- device helpers of the six angular cost kernels (mip_angular.hip: one body,
// a policy per variant) on top of mip_window_dev.h (items, window staging, LdsRef, group_sum,
// load_org, launch rules): the two boundary lines of a CU in the staged window, plain (LdsBound) and
// with the two line extensions staged behind it (stage_extensions, ExtLdsBound), the 4-tap
// coefficient words in LDS (LdsCoef), the clamp of a mode chosen on the device (mode_word), the
// steps of the 64x64 CU's path through s_sum and s_tab, the steps of a lane slot of a 32x32 block,
// and the finish of a CU.  The staging helpers take pointers and scalars (mip_window_dev.h says
// why); a helper that is inlined into the kernel may take the kernel's argument struct by const
// reference, as write_best and the kernels' shared body do: the struct stays in the kernel
// argument segment.  Handing it over by value copies it to private memory (688 bytes of scratch per
// lane in the kernels with a length table).  Internal linkage.  DESIGN.md sections 5.7, 5.9, 5.11,
// 5.12.
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

// ---- extended reference lines (mip_angular_refs MIP_ANG_REFS_EXTENDED, and every 4-tap kernel).
// s_ref of these kernels: the window's reference array, its s_left lengthened to 2S + 1 rows, the
// long copy of row y0-1 and the cell that holds 512.
//
// Staging.  Behind stage_window a workgroup stages the two line extensions of its window of side S,
// by linear index with the window's guard idx < W*H:
//   row y0-1 for 2S columns from x0, in cells of its own (kExtTopAt): the window's copy of that row
//     is followed by row y0, this one by its extension;
//   column x0-1 for S more rows, directly behind s_left (rows y0-1 .. y0+S-1 at kLeftAt).
// A top line on another row of the window is followed in s_ref by its own extension already, and
// so is a left line on a column inside it: angular_plan.h's length rule never lets those leave the
// window (tests/test_angular_ext_cpu.py asserts it at every size of the sweep).
constexpr int kExtTopAt = kLeftAt + 136;      // row y0-1, 2S <= 128 columns
constexpr int kExtConstAt = kExtTopAt + 128;  // the cell that holds 512
constexpr int kExtRefCells = kExtConstAt + 8;
static_assert(kLeftAt + 2 * 64 + 1 <= kExtTopAt && kExtTopAt % 8 == 0, "s_left with its extension ends before the long row");

// The two extensions of the window at (x0, y0), side 1 << lp; the barriers are stage_window's.
__device__ __forceinline__ void stage_extensions(const uint16_t *R, int width, long long frame_samples, int x0, int y0, int lp, int tid,
                                                 uint16_t *s_ref) {
  const int side = 1 << lp;
  if (tid < 2 * side) {  // row y0-1, columns x0 .. x0+2S-1
    const long long idx = (long long)(y0 - 1) * width + x0 + tid;
    s_ref[kExtTopAt + tid] = idx >= 0 && idx < frame_samples ? R[idx] : (uint16_t)0;
  }
  if (tid < side) {  // column x0-1, rows y0+S .. y0+2S-1
    const long long idx = (long long)(y0 + side + tid) * width + x0 - 1;
    s_ref[kLeftAt + side + 1 + tid] = idx >= 0 && idx < frame_samples ? R[idx] : (uint16_t)0;
  }
}

// IndexRef with row y0-1 taken from its long copy.
struct ExtIndexRef {
  int x0, y0, lp;
  __device__ __forceinline__ int operator()(int row, int col) const {
    const int r = row - y0 + 1;
    return kIndexBias + (col < x0 ? kLeftAt + r : r == 0 ? kExtTopAt + col - x0 : (r << lp) + col - x0);
  }
};
// LdsBound over that index rule, plus the CU's two lengths.  A lane reads them from the engine's
// table (E_top | E_left << 8 per CU, mip_extended_refs for the call's availability set) and cuts
// each to what is staged behind its line -- 2S columns of row y0-1 and S of any other row, 2S + 1
// rows of column x0-1 and S + 1 of any other column.  The lengths are data, and with the cut no
// table can move an address out of the window.  They apply as angular_plan.h's AngExtView: a larger
// clamp bound for the reads of the main line, per class.
struct ExtLdsBound {
  const uint16_t *ref;
  int w, h, tb, ts, lb, ls;
  uint32_t ce;  // corner | E_top << 16 | E_left << 24 after the cut (one register: the kernels have none to spare)
  __device__ __forceinline__ ExtLdsBound(const LdsRef &win, int x, int y, int w_, int h_, uint32_t ext) : ref(win.ref), w(w_), h(h_) {
    const ExtIndexRef ir{win.x0, win.y0, win.lp};
    const int t0 = intra_top(ir, x, y, 0), l0 = intra_left(ir, x, y, 0);
    ts = intra_top(ir, x, y, 1) - t0;
    ls = intra_left(ir, x, y, 1) - l0;
    tb = t0 == 512 ? kExtConstAt : t0 - kIndexBias;
    lb = l0 == 512 ? kExtConstAt : l0 - kIndexBias;
    const int corner_value = x > 0 && y > 0 ? win(y - 1, x - 1) : ref[tb];
    const int side = 1 << win.lp;
    const int top_room = (y == win.y0 ? 2 * side : side) - (x - win.x0) - w_;
    const int left_room = (x == win.x0 ? 2 * side : side) - (y - win.y0) - h_;
    ce = (uint32_t)corner_value | (uint32_t)min(min((int)(ext & 0xffu), h_), max(top_room, 0)) << 16 |
         (uint32_t)min(min((int)(ext >> 8 & 0xffu), w_), max(left_room, 0)) << 24;
  }
  __device__ __forceinline__ int e_top() const { return (int)(ce >> 16 & 0xffu); }
  __device__ __forceinline__ int e_left() const { return (int)(ce >> 24); }
  __device__ __forceinline__ int sample(bool top_line, int t) const { return ref[(top_line ? tb : lb) + t * (top_line ? ts : ls)]; }
  __device__ __forceinline__ int corner() const { return (int)(ce & 0xffffu); }
};
// The CU's entry of the length table; no table is MIP_ANG_REFS_SUBSTITUTED: 0 / 0 (wave-uniform).
__device__ __forceinline__ uint32_t ext_word(const uint16_t *ext, size_t cu) { return ext ? ext[cu] : 0u; }

// ---- 4-tap interpolation (mip_angular_interp MIP_ANG_INTERP_4TAP): a Coef of angular_plan.h over
// the 64 coefficient words a workgroup has staged in LDS.
struct LdsCoef {
  const uint32_t *word;
  __device__ __forceinline__ uint32_t operator()(bool gauss, int f) const { return word[(gauss ? 32 : 0) + f]; }
};

// ---- the refinement pass.  The packed (mode, angle, inverse) word of a mode chosen on the device.
// The mode is clamped into 2..66 before the lookup, so the table index is 0..64 whatever the sample
// values made of the costs; the word is then one of the host's ang_pack values, whose angle and
// inverse belong to its mode.  With any such word a Bound's reads stay inside the staged window:
// ang_ref and ang_ref_main clamp the line position t into 0 .. M-1 (or S-1) before base + t *
// stride, for every k, and base and stride come from the slot alone.
constexpr int kMaxCand = 2 * kAngMaxSeeds;
__device__ __forceinline__ uint32_t mode_word(const uint32_t *s_pack, int m) {
  m = m < MIP_ANGULAR_FIRST ? MIP_ANGULAR_FIRST : m > MIP_ANGULAR_LAST ? MIP_ANGULAR_LAST : m;
  return s_pack[m - MIP_ANGULAR_FIRST];
}

// The lane index as a value the compiler takes as new per item (the kernels' body forms tid through
// it at the top of the item loop): per-lane addresses -- the staging's, a.modes[tid], the tables'
// a.cost + tid -- are otherwise hoisted out of the item loop into registers held across the whole
// item, which at three waves per SIMD has none to spare.
__device__ __forceinline__ int opaque(int tid) {
  asm volatile("" : "+v"(tid));
  return tid;
}

// ---- the 64x64 CU: 256 lanes, one CU.  The waves leave their (sad, satd) per list entry (then per
// candidate: kMaxCand <= kAngModes) in s_sum; finish_slot adds the four waves' into s_tab (cost, sad, satd per table slot),
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

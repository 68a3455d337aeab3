// mip_angular_dev.h -- device helpers shared by the two angular cost kernels (mip_angular.hip,
// mip_angular_refine.hip): the staged window as a Ref and as the two boundary lines of a CU, the
// group sum, the block's originals and the finish of a CU.  Internal linkage: each kernel file
// has its own copies.  DESIGN.md sections 5.7 and 5.9.
#pragma once
#include "angular_plan.h"
#include "mip_kernels.h"

namespace mipgpu {
namespace {

constexpr int kThreads = 256;
constexpr int kRefRows32 = 33, kRefRows64 = 2;
constexpr int kLeftAt = kRefRows32 * 32;  // s_left inside the reference array

// The staged window as a Ref of intra_plan.h (as in mip_intra.hip).
struct LdsRef {
  const uint16_t *ref;  // s_ref, with s_left at kLeftAt (one array: one index, no pointer select)
  int x0, y0, lp;       // the window's frame position, log2 of its side
  __device__ __forceinline__ int operator()(int row, int col) const {
    const int r = row - y0 + 1;
    return ref[col >= x0 ? (r << lp) + col - x0 : kLeftAt + r];
  }
};

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

// Sums of K values over the lane's group of n lanes (a power of two, the group aligned), as in
// mip_intra.hip: branch-free, the K chains of a step independent.
template <int K>
__device__ __forceinline__ void group_sum(int (&v)[K], int n) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
    for (int k = 0; k < K; k++) {
      const int o = __shfl_xor(v[k], m, 64);
      v[k] += m < n ? o : 0;
    }
  }
}

// The 16 originals of the 4x4 block at window position (4 cx + 4 bi, 4 cy + 4 bj).
__device__ __forceinline__ void load_org(const uint16_t *s_org, int lp, const IntraSlot &c, int *org) {
  const uint16_t *o = s_org + ((4 * c.cy + 4 * c.bj) << lp) + 4 * c.cx + 4 * c.bi;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint2 v = *reinterpret_cast<const uint2 *>(o + (r << lp));
    org[4 * r] = (int)(v.x & 0xffffu);
    org[4 * r + 1] = (int)(v.x >> 16);
    org[4 * r + 2] = (int)(v.y & 0xffffu);
    org[4 * r + 3] = (int)(v.y >> 16);
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

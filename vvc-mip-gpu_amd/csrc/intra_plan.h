// intra_plan.h -- the Planar / DC baseline costs (include/mipgpu.h, mip_intra_device) as
// per-sample and per-4x4-block arithmetic, shared by the kernel (mip_intra.hip: one lane per
// 4x4 block) and by the host restatement below (intra_frames_host: the same steps, one CU at
// a time), plus the lane-slot lists the kernel walks and the decision merge.  The per-sample
// functions also build the Planar / DC blocks that the prediction kernel emits (mip_predict.hip)
// and their host restatement (intra_predict_cu_host).  No HIP dependency on the host side;
// unit-tested by tests/cpp/test_intra_plan.cpp and tests/cpp/test_intra_predict.cpp.
//
// A "Ref" is any callable ref(row, col) -> reference sample at frame row / column, read by
// linear index row * W + col like everything else here: global memory on the host, the staged
// LDS window in the kernel.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "mip_tables.h"
#include "mipgpu.h"

#if defined(__HIPCC__)
#define MIP_INTRA_HD __host__ __device__ inline __attribute__((always_inline))
#define MIP_INTRA_UNROLL _Pragma("unroll")
#else
#define MIP_INTRA_HD inline
#define MIP_INTRA_UNROLL
#endif

namespace mipgpu {

constexpr int kIntraModes = 2;  // slot 0 Planar, slot 1 DC
constexpr int32_t kIntraMaxBias = 1 << 20;

// ---- reference samples: the MIP path's complete boundaries (oracle mipo_cu_boundaries)
template <class Ref>
MIP_INTRA_HD int intra_top(const Ref &ref, int x, int y, int i) {
  return y > 0 ? ref(y - 1, x + i) : x == 0 ? 512 : ref(0, x - 1);
}
template <class Ref>
MIP_INTRA_HD int intra_left(const Ref &ref, int x, int y, int j) {
  return x > 0 ? ref(y + j, x - 1) : y == 0 ? 512 : ref(y - 1, 0);
}

// ---- the two predictions before PDPC
MIP_INTRA_HD int intra_dc(int sum_top, int sum_left, int lw, int lh) {
  if (lw == lh) return (sum_top + sum_left + (1 << lw)) >> (lw + 1);
  return lw > lh ? (sum_top + ((1 << lw) >> 1)) >> lw : (sum_left + ((1 << lh) >> 1)) >> lh;
}
// top_i = top[i], left_j = left[j], tr = top[w-1] (above-right substitute), bl = left[h-1]
MIP_INTRA_HD int intra_planar(int top_i, int left_j, int tr, int bl, int i, int j, int lw, int lh) {
  const int w = 1 << lw, h = 1 << lh;
  const int pred_v = ((h - 1 - j) * top_i + (j + 1) * bl) << lw;
  const int pred_h = ((w - 1 - i) * left_j + (i + 1) * tr) << lh;
  return (pred_v + pred_h + w * h) >> (lw + lh + 1);
}

// ---- PDPC: weight of the boundary sample at distance d (column or row index), and the blend
MIP_INTRA_HD int intra_pdpc_weight(int d, int scale) {
  const int s = (2 * d) >> scale;
  return s <= 5 ? 32 >> s : 0;  // (a 4x64 CU reaches shift 63)
}
MIP_INTRA_HD int intra_pdpc(int p, int top_i, int left_j, int wt, int wl) {
  const int v = (left_j * wl + top_i * wt + (64 - wl - wt) * p + 32) >> 6;
  return v < 0 ? 0 : v > 1023 ? 1023 : v;
}

// ---- SAD and the engine's 4x4 Hadamard SATD (oracle satd4x4: DC term >> 2, (s + 1) >> 1)
MIP_INTRA_HD int intra_abs(int v) { return v < 0 ? -v : v; }
MIP_INTRA_HD int intra_sad16(const int *d) {
  int s = 0;
  MIP_INTRA_UNROLL
  for (int k = 0; k < 16; k++) s += intra_abs(d[k]);
  return s;
}
MIP_INTRA_HD int intra_satd4x4(const int *d) {
  int m[16], e[16];
  MIP_INTRA_UNROLL
  for (int i = 0; i < 4; i++) {
    m[i] = d[i] + d[12 + i];
    m[4 + i] = d[4 + i] + d[8 + i];
    m[8 + i] = d[4 + i] - d[8 + i];
    m[12 + i] = d[i] - d[12 + i];
  }
  MIP_INTRA_UNROLL
  for (int i = 0; i < 4; i++) {
    e[i] = m[i] + m[4 + i];
    e[4 + i] = m[8 + i] + m[12 + i];
    e[8 + i] = m[i] - m[4 + i];
    e[12 + i] = m[12 + i] - m[8 + i];
  }
  int satd = 0, dc = 0;
  MIP_INTRA_UNROLL
  for (int row = 0; row < 4; row++) {
    const int *s = e + 4 * row;
    const int t0 = s[0] + s[3], t1 = s[1] + s[2], t2 = s[1] - s[2], t3 = s[0] - s[3];
    if (row == 0) dc = intra_abs(t0 + t1);
    else satd += intra_abs(t0 + t1);
    satd += intra_abs(t0 - t1) + intra_abs(t2 + t3) + intra_abs(t3 - t2);
  }
  return (satd + (dc >> 2) + 1) >> 1;
}

// ---- one 4x4 block of a CU, both modes: what one lane of the kernel computes
struct IntraBlock {
  int top[4], left[4];  // top[i0 .. i0+4), left[j0 .. j0+4)
  int tr, bl, dc;       // top[w-1], left[h-1], the CU's DC value
  int i0, j0, lw, lh;   // the block's place inside the CU, the CU's size
};
struct IntraSums {
  int sad[kIntraModes], satd[kIntraModes];
};
// org: the block's 16 original samples, row-major
MIP_INTRA_HD IntraSums intra_block(const IntraBlock &b, const int *org) {
  const int scale = (b.lw + b.lh - 2) >> 2;
  int dp[16], dd[16];
  MIP_INTRA_UNROLL
  for (int r = 0; r < 4; r++) {
    const int wt = intra_pdpc_weight(b.j0 + r, scale);
    MIP_INTRA_UNROLL
    for (int c = 0; c < 4; c++) {
      const int wl = intra_pdpc_weight(b.i0 + c, scale);
      const int p = intra_planar(b.top[c], b.left[r], b.tr, b.bl, b.i0 + c, b.j0 + r, b.lw, b.lh);
      dp[4 * r + c] = org[4 * r + c] - intra_pdpc(p, b.top[c], b.left[r], wt, wl);
      dd[4 * r + c] = org[4 * r + c] - intra_pdpc(b.dc, b.top[c], b.left[r], wt, wl);
    }
  }
  return IntraSums{{intra_sad16(dp), intra_sad16(dd)}, {intra_satd4x4(dp), intra_satd4x4(dd)}};
}

MIP_INTRA_HD int32_t intra_cost(int sad, int satd) { return 2 * sad < satd ? 2 * sad : satd; }

// ---- decision merge: candidates MIP, Planar, DC; a later one replaces the current one only if
// its biased cost is strictly lower.  Unavailable CUs (either side) stay as they are.
MIP_INTRA_HD void intra_merge(uint8_t &mode, int32_t &cost, int32_t planar, int32_t dc, int32_t bias_planar, int32_t bias_dc) {
  if (cost == MIP_COST_UNAVAILABLE || planar == MIP_COST_UNAVAILABLE) return;
  if (planar + bias_planar < cost) cost = planar + bias_planar, mode = MIP_MODE_PLANAR;
  if (dc + bias_dc < cost) cost = dc + bias_dc, mode = MIP_MODE_DC;
}

inline bool intra_bias_ok(const int32_t *bias) {
  for (int k = 0; bias && k < kIntraModes; k++)
    if (bias[k] < 0 || bias[k] > kIntraMaxBias) return false;
  return true;
}

// ---- lane slots of the kernel.  Every shape other than 64x64 lies inside one 32x32 block of
// the CTU.  A block's CUs are listed largest first, each as one slot per 4x4 block of the CU
// (row-major), so a CU of n 4x4 blocks (n a power of two, <= 64) owns n consecutive slots
// starting at a multiple of n: lane l of pass p takes slot 64 p + l, and a CU's lanes are an
// aligned group of one wave.  The list is padded to whole waves with kIntraNoSlot.
//   bits 0-12 CU inside the CTU, 13-15 / 16-18 the 4x4 block's column / row inside the CU,
//   19-21 / 22-24 the CU's x / y inside the 32x32 block in 4-sample units,
//   25-27 / 28-30 log2 w - 2 / log2 h - 2, bit 31 no slot.
constexpr uint32_t kIntraNoSlot = 0x80000000u;
constexpr int kIntraBlocks = 16;  // 32x32 blocks per CTU, block = 4 * (y / 32) + x / 32
struct IntraSlot {
  int cu, bi, bj, cx, cy, lw, lh;
};
MIP_INTRA_HD IntraSlot intra_slot_decode(uint32_t s) {
  return IntraSlot{(int)(s & 0x1fffu),      (int)(s >> 13 & 7u),      (int)(s >> 16 & 7u), (int)(s >> 19 & 7u),
                   (int)(s >> 22 & 7u), (int)(s >> 25 & 7u) + 2, (int)(s >> 28 & 7u) + 2};
}

inline constexpr mip_shape_desc kIntraShapes[MIP_NUM_SHAPES] = MIP_SHAPE_TABLE;
inline int intra_axis(int base, int step, int dual, int i) { return dual ? base + (i / 2) * step + (i % 2) * dual : base + i * step; }
inline int intra_log2(int v) {
  int l = 0;
  while ((1 << l) < v) l++;
  return l;
}

// The slot lists of the 16 blocks, [16][*per_block] (per_block a multiple of 64, the same for
// every block).  Empty if the shape table breaks the assumptions above.
inline std::vector<uint32_t> intra_build_slots(int *per_block) {
  struct Cu {
    int cu, n, x, y, lw, lh;
  };
  std::vector<Cu> list[kIntraBlocks];
  int k = 0;
  for (int s = 0; s < MIP_NUM_SHAPES; s++) {
    const mip_shape_desc &sd = kIntraShapes[s];
    const int lw = intra_log2(sd.w), lh = intra_log2(sd.h);
    if ((1 << lw) != sd.w || (1 << lh) != sd.h || lw < 2 || lh < 2) return {};
    for (int cu = 0; cu < sd.ncu; cu++, k++) {
      if (sd.w == 64 && sd.h == 64) continue;  // (the kernel's own work items)
      const int x = intra_axis(sd.xb, sd.xs, sd.xd, cu % sd.ncols), y = intra_axis(sd.yb, sd.ys, sd.yd, cu / sd.ncols);
      if (x % 4 || y % 4 || x % 32 + sd.w > 32 || y % 32 + sd.h > 32 || x + sd.w > 128 || y + sd.h > 128) return {};
      list[4 * (y / 32) + x / 32].push_back(Cu{k, (sd.w / 4) * (sd.h / 4), x % 32, y % 32, lw, lh});
    }
  }
  size_t slots = 0;
  for (const Cu &c : list[0]) slots += c.n;
  const int padded = (int)((slots + 63) / 64 * 64);
  std::vector<uint32_t> out((size_t)kIntraBlocks * padded, kIntraNoSlot);
  for (int b = 0; b < kIntraBlocks; b++) {
    std::stable_sort(list[b].begin(), list[b].end(), [](const Cu &p, const Cu &q) { return p.n > q.n; });
    size_t at = 0;
    for (const Cu &c : list[b])
      for (int t = 0; t < c.n; t++, at++) {
        if (at >= (size_t)padded) return {};
        const int bw = 1 << (c.lw - 2);
        out[(size_t)b * padded + at] = (uint32_t)c.cu | (uint32_t)(t % bw) << 13 | (uint32_t)(t / bw) << 16 | (uint32_t)(c.x / 4) << 19 |
                                       (uint32_t)(c.y / 4) << 22 | (uint32_t)(c.lw - 2) << 25 | (uint32_t)(c.lh - 2) << 28;
      }
    if (at != slots) return {};
  }
  *per_block = padded;
  return out;
}

// ---- host side: one CU, then the whole table
struct IntraHostRef {
  const uint16_t *r;
  int width;
  int operator()(int row, int col) const { return r[(size_t)row * width + col]; }
};

// Both modes of the w x h CU at frame position (x, y): refs / orig are one frame each.
inline void intra_cu_host(const uint16_t *orig, const uint16_t *refs, int width, int x, int y, int lw, int lh, int32_t *sad,
                          int32_t *satd) {
  const IntraHostRef ref{refs, width};
  const int w = 1 << lw, h = 1 << lh;
  int top[64], left[64], sum_top = 0, sum_left = 0;
  for (int i = 0; i < w; i++) sum_top += top[i] = intra_top(ref, x, y, i);
  for (int j = 0; j < h; j++) sum_left += left[j] = intra_left(ref, x, y, j);
  IntraBlock b;
  b.tr = top[w - 1];
  b.bl = left[h - 1];
  b.dc = intra_dc(sum_top, sum_left, lw, lh);
  b.lw = lw;
  b.lh = lh;
  sad[0] = sad[1] = satd[0] = satd[1] = 0;
  for (b.j0 = 0; b.j0 < h; b.j0 += 4)
    for (b.i0 = 0; b.i0 < w; b.i0 += 4) {
      int org[16];
      for (int k = 0; k < 4; k++) {
        b.top[k] = top[b.i0 + k];
        b.left[k] = left[b.j0 + k];
        for (int c = 0; c < 4; c++) org[4 * k + c] = orig[(size_t)(y + b.j0 + k) * width + x + b.i0 + c];
      }
      const IntraSums s = intra_block(b, org);
      for (int m = 0; m < kIntraModes; m++) sad[m] += s.sad[m], satd[m] += s.satd[m];
    }
}

// The samples of one CU (mip_predict_device_ex with MIP_PRED_REGULAR): the Planar
// (MIP_MODE_PLANAR) or DC (MIP_MODE_DC) block of the w x h CU at frame position (x, y) after PDPC,
// row r at out[r * pitch .. + w).  refs is one frame; the steps are the prediction kernel's
// (mip_predict.hip store_regular).  Returns 0, or -1 for any other mode (nothing written).
inline int intra_predict_cu_host(const uint16_t *refs, int width, int x, int y, int lw, int lh, int mode, uint16_t *out,
                                 int pitch) {
  if (mode != MIP_MODE_PLANAR && mode != MIP_MODE_DC) return -1;
  const IntraHostRef ref{refs, width};
  const int w = 1 << lw, h = 1 << lh, scale = (lw + lh - 2) >> 2;
  int top[64], left[64], sum_top = 0, sum_left = 0;
  for (int i = 0; i < w; i++) sum_top += top[i] = intra_top(ref, x, y, i);
  for (int j = 0; j < h; j++) sum_left += left[j] = intra_left(ref, x, y, j);
  const int tr = top[w - 1], bl = left[h - 1], dc = intra_dc(sum_top, sum_left, lw, lh);
  for (int j = 0; j < h; j++) {
    const int wt = intra_pdpc_weight(j, scale);
    for (int i = 0; i < w; i++) {
      const int p = mode == MIP_MODE_PLANAR ? intra_planar(top[i], left[j], tr, bl, i, j, lw, lh) : dc;
      out[(size_t)j * pitch + i] = (uint16_t)intra_pdpc(p, top[i], left[j], wt, intra_pdpc_weight(i, scale));
    }
  }
  return 0;
}

// The tables of mip_intra_device on host arrays (each optional): frames / refs
// [nframes][height][width] (refs already resolved: the originals, the filtered or the caller's
// frames), unavail [nctus*5380] the availability set that goes with refs.  Returns 0, or -1 for
// arguments the entry point rejects.
inline int intra_frames_host(const uint16_t *frames, const uint16_t *refs, const uint8_t *unavail, int width, int height,
                             int nframes, int32_t *cost, int32_t *sad, int32_t *satd) {
  if (!frames || !refs || !unavail || width <= 0 || height <= 0 || width % 4 || height % 4 || nframes < 1) return -1;
  if (!cost && !sad && !satd) return -1;
  const int cols = (width + 127) / 128, nctus = cols * ((height + 127) / 128);
  const size_t fs = (size_t)width * height;
  for (int f = 0; f < nframes; f++)
    for (int c = 0; c < nctus; c++) {
      size_t k = (size_t)c * MIP_CUS_PER_CTU;
      for (int s = 0; s < MIP_NUM_SHAPES; s++) {
        const mip_shape_desc &sd = kIntraShapes[s];
        for (int cu = 0; cu < sd.ncu; cu++, k++) {
          int32_t a[kIntraModes], b[kIntraModes];
          const bool on = !unavail[k];
          if (on)
            intra_cu_host(frames + f * fs, refs + f * fs, width, 128 * (c % cols) + intra_axis(sd.xb, sd.xs, sd.xd, cu % sd.ncols),
                          128 * (c / cols) + intra_axis(sd.yb, sd.ys, sd.yd, cu / sd.ncols), intra_log2(sd.w), intra_log2(sd.h), a, b);
          for (int m = 0; m < kIntraModes; m++) {
            const size_t at = ((size_t)f * nctus * MIP_CUS_PER_CTU + k) * kIntraModes + m;
            if (cost) cost[at] = on ? intra_cost(a[m], b[m]) : MIP_COST_UNAVAILABLE;
            if (sad) sad[at] = on ? a[m] : MIP_COST_UNAVAILABLE;
            if (satd) satd[at] = on ? b[m] : MIP_COST_UNAVAILABLE;
          }
        }
      }
    }
  return 0;
}

// The merge of mip_intra_device on host arrays: cost [n][2] as above, best_mode / best_cost [n].
inline void intra_merge_host(const int32_t *cost, size_t n, const int32_t *bias, uint8_t *best_mode, int32_t *best_cost) {
  for (size_t k = 0; k < n; k++)
    intra_merge(best_mode[k], best_cost[k], cost[2 * k], cost[2 * k + 1], bias ? bias[0] : 0, bias ? bias[1] : 0);
}

}  // namespace mipgpu

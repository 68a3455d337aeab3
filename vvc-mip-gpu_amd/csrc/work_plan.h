// work_plan.h -- everything the host decides about what the search kernel computes: the MFMA
// tables, which CUs of which CTU are searched, the wave tasks and their lists, the item order
// of small launches and the choice among the lists (mipgpu.cpp mip_engine_create / pick_work
// upload and use the result; no HIP dependency and no environment reads, unit-tested by
// tests/cpp/test_work_plan.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <utility>
#include <vector>

#include "mip_tables.h"
#include "mip_work.h"
#include "mipgpu.h"

namespace mipgpu {

inline constexpr mip_shape_desc kShapes[MIP_NUM_SHAPES] = MIP_SHAPE_TABLE;
inline constexpr uint8_t kW0[16 * 16 * 4] = MIP_WEIGHTS_S0;
inline constexpr uint8_t kW1[8 * 16 * 8] = MIP_WEIGHTS_S1;
inline constexpr uint8_t kW2[6 * 64 * 7] = MIP_WEIGHTS_S2;

// The planner's knobs, as data: mipgpu.cpp fills them once per engine from the environment
// (plan_knobs_from_env); the defaults are the shipped configuration.
struct PlanKnobs {
  double cut_factor = 2.0;      // task size cap = a wave's fair share / cut_factor
  bool transpose_wide = true;   // wide CUs (32x4, 16x4, 8x4, 32x8, 16x8) searched as their tall
                                // transposes (transposed classes, mip_work.h)
  bool no_pairs = false;        // profiling: tasks keep their prologue but search no mode pair
  uint64_t shapes = (1ull << MIP_NUM_SHAPES) - 1;  // profiling: bit s = shape s is searched
};

inline int axis_pos(int base, int step, int dual, int i) {
  return dual ? base + (i / 2) * step + (i % 2) * dual : base + i * step;
}

// f32 -> f16 bits, exact for the table's values: multiples of 1/64 of magnitude below 32 have
// at most 11 significant bits and an exponent in f16's normal range, so the conversion is a
// re-biased exponent and the top 10 mantissa bits (the 13 dropped ones are zero).
inline uint16_t to_half(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint32_t sign = (u >> 16) & 0x8000u, exp = (u >> 23) & 0xffu;
  if (exp == 0) return (uint16_t)sign;
  return (uint16_t)(sign | (exp - 127 + 15) << 10 | (u & 0x7fffffu) >> 13);
}

// MIP coefficient tables for the MFMA (layout documented in mip_work.h).
inline std::vector<uint8_t> build_tables() {
  std::vector<uint8_t> t(kTableBytes, 0);
  uint16_t *w = reinterpret_cast<uint16_t *>(t.data());
  float *ctab = reinterpret_cast<float *>(t.data() + kWeightRows * 16);
  // one matrix row: a0 and w'_1..w'_{nin-1} -> A_j (see mip_work.h); returns sum_k A_jk
  auto put = [&](int row, double a0, const double *wp, int nin) {
    double sum_w = 0, sum_a = 0;
    for (int k = 1; k < nin; k++) sum_w += wp[k];
    double a[8] = {a0 - sum_w, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 1; k < nin; k++) a[k] = wp[k];
    for (int k = 0; k < 8; k++) {
      w[row * 8 + k] = to_half((float)a[k]);
      sum_a += a[k];
    }
    return sum_a;
  };
  // sizeId 2: inputs 1..7 use matrix columns 0..6 (p_0 == 0, mip_matrix.cl:441, intra.cl:459-463)
  for (int m = 0; m < 6; m++)
    for (int j = 0; j < 64; j++) {
      double wp[8] = {0};
      for (int k = 1; k < 8; k++) wp[k] = (kW2[(m * 64 + j) * 7 + k - 1] - 32) / 64.0;
      const double sa = put(m * 64 + j, 1.0, wp, 8);
      (void)sa;  // == 1: C' is the constant kAccInitS2
    }
  auto small = [&](int base, int modes, int nin, const uint8_t *src) {
    for (int m = 0; m < modes; m++)
      for (int j = 0; j < 16; j++) {
        const uint8_t *wr = src + (m * 16 + j) * nin;
        double wp[8] = {0};
        for (int k = 1; k < nin; k++) wp[k] = (wr[k] - 32) / 64.0;
        const double sa = put(base + m * 16 + j, (96 - wr[0]) / 64.0, wp, nin);
        ctab[base - kWeightRowOffS1 + m * 16 + j] = (float)(8.0 * (wr[0] - 32) + 0.5 - 1024.0 * sa);
      }
  };
  small(kWeightRowOffS1, 8, 8, kW1);
  small(kWeightRowOffS0, 16, 4, kW0);
  for (int i = 0; i < 4; i++) ctab[384 + i] = kAccInitS2;
  return t;
}

// Is the cost of the CU at frame position (x, y) defined (mipgpu.layout.cu_defined,
// oracle mipo_cu_defined)?
inline bool cu_defined(int width, int height, int x, int y, int w, int h) {
  return y + h <= height && (long long)(y + h - 1) * width + x + w - 1 < (long long)width * height;
}

// CU inside the CTU (reference order, 0..5379) -> its shape and CTU-relative position
// (prediction lists name CUs by this index, like the decision lists).
struct CuGeo {
  uint8_t shape, x, y;
};
inline const std::vector<CuGeo> &cu_geo_table() {
  static const std::vector<CuGeo> table = [] {
    std::vector<CuGeo> t;
    t.reserve(MIP_CUS_PER_CTU);
    for (int s = 0; s < MIP_NUM_SHAPES; s++) {
      const mip_shape_desc &sd = kShapes[s];
      for (int cu = 0; cu < sd.ncu; cu++)
        t.push_back(CuGeo{(uint8_t)s, (uint8_t)axis_pos(sd.xb, sd.xs, sd.xd, cu % sd.ncols),
                          (uint8_t)axis_pos(sd.yb, sd.ys, sd.yd, cu / sd.ncols)});
    }
    return t;
  }();
  return table;
}

// Reference samples above 10 bits.  At widths that are not multiples of 128 the reference's
// separable filters give the last one or two frame columns values up to ~1.7 x 1023: the
// horizontal pass there sums the wrapped next-row samples while the scale is the frame-edge
// class (intra.cl:3446-3458, 3771-3788).  The search kernel's arithmetic is sized for 10-bit
// samples, so with alternative references the CUs that read columns W-2 or W-1 (their top
// row, left column or padding sample) are left to the exact per-CU kernel (fixup_kernel).
inline bool reads_last_columns(int width, int height, int x, int y, int w, int h) {
  (void)height;
  auto col_hit = [&](long long li) { const long long c = li % width; return c >= width - 2; };
  if (y > 0) {
    for (int i = 0; i < w; i++)
      if (col_hit((long long)(y - 1) * width + x + i)) return true;
  } else if (x > 0 && col_hit(x - 1)) {
    return true;
  }
  if (x > 0) {
    for (int i = 0; i < h; i++)
      if (col_hit((long long)(y + i) * width + x - 1)) return true;
  } else if (y > 0 && col_hit((long long)(y - 1) * width)) {
    return true;
  }
  return false;
}

// Filtered reference samples the reference leaves undefined because the filter reads memory
// past the frame's end ("poison"; the oracle's mipo_filter_frame_ex models the same and
// tests/test_gpu_parity.py compares the two).  The reference's filters work on 128x32 tiles
// (intra.cl:2873-2879) and address the frame by linear index; halo cells are gated by
// index < W*H (2D intra.cl:2913-2966 / 3103-3189 and float twins; separable 3336-3366,
// 3606-3688), so only interior cells can read past the end:
//   2-D and separable 5-tap: rows inside the frame are read (2904-2909, 3595-3598), so only
//     the last row right of the frame (wrapping past the end) -- at widths that are not
//     multiples of 128;
//   separable 3-tap: interior rows are read unguarded (3330-3332), so every row below the
//     frame (last tile band when H % 32 != 0) too.
// An output depends on the cells of its window (2-D: (2R+1)^2; separable: horizontal taps of
// the vertical taps' rows, 3377-3478 / 3705-3788).  Tiles store all their 128 columns by
// linear index (3027-3038, 3489-3505): the last tile column's columns right of the frame land
// on the next row, so their poison counts there too (where the two stores race with defined
// values, the engine keeps the owning tile's value: one of the reference's outcomes).
// Only the last tile band (rows [y0, H)) holds such cells; returned as a mask over it.
struct Poison {
  int y0 = 0;                  // first frame row of the mask
  std::vector<uint8_t> mask;   // [(H - y0) * W]: 1 = undefined (linear index - y0 * W)
  bool any = false;
  bool at(long long li, int width) const {
    const long long o = li - (long long)y0 * width;
    return o >= 0 && o < (long long)mask.size() && mask[(size_t)o];
  }
};

inline Poison filter_poison(int width, int height, int filter) {
  Poison ps;
  if (filter < 0) return ps;
  const bool sep = filter == MIP_FILTER_1D_INT || filter == MIP_FILTER_1D_FLOAT || filter == MIP_FILTER_1D_INT_5x5 ||
                   filter == MIP_FILTER_1D_FLOAT_5x5;
  const bool five = filter >= MIP_FILTER_1D_INT_5x5;
  const long long W = width, H = height, WH = W * H;
  ps.y0 = 32 * ((height - 1) / 32);
  ps.mask.assign((size_t)(H - ps.y0) * W, 0);
  const int qy = ps.y0, rows = std::min(32, height - qy);
  // cell poison of tile rows ty (interior 0..31) at tile column tc (0..127)
  auto cell = [&](int qx, int ty, int tc) -> bool {
    if (ty < 0 || ty >= 32 || tc < 0 || tc >= 128) return false;  // halo: gated, never poison
    const long long y = qy + ty;
    if (!(sep && !five) && y >= H) return false;  // 2-D / 5-tap separable: rows below not read
    return y * W + qx + tc >= WH;
  };
  const int R = five ? 2 : 1;
  for (int qx = 0; qx < width; qx += 128) {
    uint8_t out[32][128] = {};
    bool tile_any = false;
    for (int r = 0; r < rows; r++)
      for (int c = 0; c < 128; c++) {
        bool p = false;
        if (!sep) {
          for (int dy = -R; dy <= R && !p; dy++)
            for (int dx = -R; dx <= R && !p; dx++) p = cell(qx, r + dy, c + dx);
        } else {
          // vertical taps over rows r-R..r+R (5-tap: only rows with a horizontal pass,
          // i.e. frame rows, intra.cl:3705-3726), horizontal taps c-R..c+R of each
          for (int dy = -R; dy <= R && !p; dy++) {
            if (five && (qy + r + dy < 0 || qy + r + dy >= height)) continue;
            for (int dx = -R; dx <= R && !p; dx++) p = cell(qx, r + dy, c + dx);
          }
        }
        out[r][c] = p;
        tile_any |= p;
      }
    if (!tile_any) continue;
    for (int r = 0; r < rows; r++)
      for (int c = 0; c < 128; c++) {
        const long long li = (long long)(qy + r) * W + qx + c;  // owning or wrapped store
        if (out[r][c] && li < WH) {
          ps.mask[(size_t)(li - (long long)qy * W)] = 1;
          ps.any = true;
        }
      }
  }
  return ps;
}

// Does the CU at frame position (x, y) read a poisoned reference sample (its top row or the
// top-edge padding sample, its left column or the left-edge padding sample, by linear index
// as the reference's initBoundaries does, intra.cl:96-107, 232-243)?
inline bool reads_poison(const Poison &ps, int width, int x, int y, int w, int h) {
  if (!ps.any) return false;
  if (y > 0) {
    for (int i = 0; i < w; i++)
      if (ps.at((long long)(y - 1) * width + x + i, width)) return true;
  } else if (x > 0 && ps.at(x - 1, width)) {
    return true;
  }
  if (x > 0) {
    for (int i = 0; i < h; i++)
      if (ps.at((long long)(y + i) * width + x - 1, width)) return true;
  } else if (y > 0 && ps.at((long long)(y - 1) * width, width)) {
    return true;
  }
  return false;
}

// CTU -> variant = index of the CTU's set of CUs the search kernel computes (the others get
// MIP_COST_UNAVAILABLE from the fill lists; the fixup kernel overwrites its CUs after).
// Three maps share the variants (kMapOrig / kMapAltCaller / kMapAltEngine): original
// references (every defined CU); caller-supplied alternative references (minus the fixup CUs
// when the width is not a multiple of 128); the engine filter's references (minus the fixup
// CUs and minus the CUs that read a sample the reference's filter leaves undefined,
// filter_poison -- those are MIP_COST_UNAVAILABLE).
constexpr int kMapOrig = 0, kMapAltCaller = 1, kMapAltEngine = 2, kMaps = 3;
struct CtuVariants {
  std::vector<uint8_t> of_ctu[kMaps];
  std::vector<std::vector<bool>> pattern;  // [variant][CU in CTU order]
  std::vector<FixupCu> fixup[kMaps];       // ALT: CUs computed by the fixup kernel
};

inline CtuVariants ctu_variants(int width, int height, int filter) {
  CtuVariants v;
  const int cols = (width + 127) / 128, n = cols * ((height + 127) / 128);
  const Poison ps = filter_poison(width, height, filter);
  for (int map = 0; map < kMaps; map++)
    for (int c = 0; c < n; c++) {
      const int cx = 128 * (c % cols), cy = 128 * (c / cols);
      // only CTUs whose CUs reach the last columns can hold fixup CUs (wraps: W < 256)
      const bool near_edge = map != kMapOrig && width % 128 && (cx + 256 >= width || width < 256);
      // only CTUs whose CUs reach the poisoned band (one CTU row up: left columns wrap)
      const bool near_poison = map == kMapAltEngine && ps.any && cy + 256 > ps.y0;
      std::vector<bool> pat;
      pat.reserve(MIP_CUS_PER_CTU);
      int k = 0;
      for (int s = 0; s < MIP_NUM_SHAPES; s++) {
        const mip_shape_desc &sd = kShapes[s];
        for (int cu = 0; cu < sd.ncu; cu++, k++) {
          const int lx = axis_pos(sd.xb, sd.xs, sd.xd, cu % sd.ncols), ly = axis_pos(sd.yb, sd.ys, sd.yd, cu / sd.ncols);
          bool on = cu_defined(width, height, cx + lx, cy + ly, sd.w, sd.h);
          if (on && near_poison && reads_poison(ps, width, cx + lx, cy + ly, sd.w, sd.h)) on = false;
          if (on && near_edge && reads_last_columns(width, height, cx + lx, cy + ly, sd.w, sd.h)) {
            on = false;
            v.fixup[map].push_back(FixupCu{(uint32_t)c, (uint16_t)k, (uint8_t)s, 0});
          }
          pat.push_back(on);
        }
      }
      size_t var = 0;
      while (var < v.pattern.size() && v.pattern[var] != pat) var++;
      if (var == v.pattern.size()) v.pattern.push_back(pat);
      v.of_ctu[map].push_back((uint8_t)std::min<size_t>(var, 255));
    }
  return v;
}

// Per-quadrant work lists.  The CUs of one size class inside quadrant q (several shapes
// share a class) are split into groups of at most class_slots() CUs; a group and a range
// of its mode pairs form a wave task.  Tasks are cut so that none exceeds half of a wave's
// fair share, then assigned longest-first to the least-loaded of the quadrant's `slices`
// lists (one per workgroup); each list stays in decreasing cost order, and the waves of a
// workgroup take its tasks dynamically.  Costs are VALU-instruction estimates per lane.
// Edge CTUs: the reference reads samples by linear index (intra.cl:100, 236, 718), so CUs
// right of the frame read the next row (defined costs, searched here too) and only two
// kinds of CU are undefined (MIP_COST_UNAVAILABLE here): CUs below the frame (y + h > H:
// stale LDS, intra.cl:96-98) and CUs whose bottom-right sample's linear index
// (y + h - 1) * W + x + w - 1 is past the frame end (in practice: touching the bottom row
// and reaching past the right edge).  Such CUs get no task.  CTUs with the same set of
// defined CUs share a *variant* (ctu_variants: usually the interior, the last CTU row and
// the last CTU); each variant has its own lists and a fill list of the unavailable cost
// entries (16-byte units inside the CTU's cost block).
// One WorkPlan is everything the engine uploads for one (slices, wide) pair.
struct WorkPlan {
  int slices = 1;
  bool wide = false;  // lists for one 16-wave workgroup per CU (small launches, pick_work)
  std::vector<WaveTask> tasks;
  std::vector<Job> jobs;
  std::vector<int> list_begin;   // [variant][quadrant][slice] + 1
  std::vector<double> list_cost; // [variant][quadrant][slice]: estimated time of the list on one
                                 // workgroup (VALU instructions per lane, waves share its tasks)
  std::vector<uint32_t> fill;    // unavailable cost entries, uint4 index inside the CTU block
  std::vector<int> fill_begin;   // [variant][quadrant] + 1
  // decisions only: undefined CUs (CU index inside the CTU) per [variant][quadrant], and the
  // CUs whose mode pairs are cut over several tasks per [variant]
  std::vector<uint16_t> dfill, split;
  std::vector<int> dfill_begin, split_begin;
  int max_split = 0;
  // Small launches: the frame's items longest first (SearchArgs::order), their estimated
  // costs in that order (the makespan model of shortest_makespan), and the items of a frame
  // with tasks (original references): the first `nonempty` of `order`.
  std::vector<uint32_t> order;
  std::vector<double> order_cost;
  uint32_t nonempty = 0;
};

// Estimated VALU instructions per lane for one mode pair of a task of `ncu` CUs.
inline double pair_cost(int cls, int ncu) {
  const int w = kClassW[cls], h = kClassH[cls];
  const int sid = class_size_id(w, h), v = kClassV[cls];
  const int nout = sid == 2 ? 64 : 16;
  const double blocks = (double)h / 4 / v;
  const double mfma = ((ncu + 7) / 8) * (nout / 16);
  return blocks * 200.0 + mfma * 12.0 + 40.0;
}

// The lists of `wp` (every field but the item order) for workgroups of `waves` waves.
inline void build_work(WorkPlan &wl, int waves, const CtuVariants &cv, const PlanKnobs &knobs) {
  const int slices = wl.slices;
  for (int vq = 0; vq < 4 * (int)cv.pattern.size(); vq++) {
    const int var = vq / 4, q = vq % 4;
    wl.fill_begin.push_back((int)wl.fill.size());
    wl.dfill_begin.push_back((int)wl.dfill.size());
    if (q == 0) {
      if (var > 0) wl.max_split = std::max(wl.max_split, (int)wl.split.size() - wl.split_begin.back());
      wl.split_begin.push_back((int)wl.split.size());
    }
    struct Piece { WaveTask t; double cost; };
    std::vector<Piece> pieces;
    std::vector<std::vector<Job>> cls_cus(kNumClasses);
    int shape_cu0 = 0;  // first CU of the shape inside the CTU (reference order)
    for (int s = 0; s < MIP_NUM_SHAPES; shape_cu0 += kShapes[s].ncu, s++) {
      if (!((knobs.shapes >> s) & 1)) continue;
      const mip_shape_desc &sd = kShapes[s];
      int cls = size_class(sd.w, sd.h);
      if (knobs.transpose_wide && kClassTransposed[cls] >= 0) cls = kClassTransposed[cls];
      for (int cu = 0; cu < sd.ncu; cu++) {
        const int x = axis_pos(sd.xb, sd.xs, sd.xd, cu % sd.ncols), y = axis_pos(sd.yb, sd.ys, sd.yd, cu / sd.ncols);
        if (x / 64 != (q & 1) || y / 64 != (q >> 1)) continue;
        if (!cv.pattern[var][shape_cu0 + cu]) {
          const uint32_t off = sd.cost_offset + cu * 2 * sd.modes;  // multiple of 4 entries
          for (uint32_t u = 0; u < (uint32_t)(2 * sd.modes) / 4; u++) wl.fill.push_back(off / 4 + u);
          wl.dfill.push_back((uint16_t)(shape_cu0 + cu));
          continue;
        }
        cls_cus[cls].push_back(Job{(uint32_t)(sd.cost_offset + cu * 2 * sd.modes), (uint8_t)(x % 64), (uint8_t)(y % 64),
                                   (uint16_t)(shape_cu0 + cu)});
      }
    }
    double total = 0;
    for (int cls = 0; cls < kNumClasses; cls++) {
      const std::vector<Job> &v = cls_cus[cls];
      if (v.empty()) continue;
      const int nv = (int)v.size(), slots = class_slots(cls);
      const int sid = class_size_id(kClassW[cls], kClassH[cls]);
      const int modes = sid == 2 ? 6 : (sid == 1 ? 8 : 16);
      // groups (class, CUs): full tasks plus a remainder task of the class's row-part variant
      // when the remainder fits it; otherwise equal-sized groups
      // (variant tasks replace one base task when they occupy fewer lane-blocks: a task of
      // V row parts gives every lane H / (4 V) blocks per mode pair)
      std::vector<std::pair<int, int>> groups;
      const int var = kClassVariant[cls], rem = nv % slots;
      const int nvar = var >= 0 ? (rem + class_slots(var) - 1) / class_slots(var) : 0;
      if (rem > 0 && var >= 0 && nvar * kClassV[cls] < kClassV[var]) {
        for (int g = 0; g < nv / slots; g++) groups.push_back({cls, slots});
        for (int g = 0, at = 0; g < nvar; g++) {
          const int n = (rem - at) / (nvar - g);
          groups.push_back({var, n});
          at += n;
        }
      } else {
        const int ng = (nv + slots - 1) / slots;
        for (int g = 0, at = 0; g < ng; g++) {
          const int n = (nv - at) / (ng - g);
          groups.push_back({cls, n});
          at += n;
        }
      }
      for (int g = 0, at = 0; g < (int)groups.size(); g++) {
        const int gc = groups[g].first, n = groups[g].second;
        const uint32_t first = (uint32_t)wl.jobs.size();
        wl.jobs.insert(wl.jobs.end(), v.begin() + at, v.begin() + at + n);
        at += n;
        const double c = pair_cost(gc, n);
        pieces.push_back({WaveTask{(uint8_t)gc, (uint8_t)n, 0, (uint8_t)modes, first}, c});
        total += c * modes;
      }
    }
    // cut long tasks into pair ranges
    const double cap = std::max(1.0, total / (slices * waves) / knobs.cut_factor);
    std::vector<Piece> cut;
    for (const Piece &p : pieces) {
      const int np = p.t.q1 - p.t.q0;
      const int parts = std::max(1, std::min(np, (int)std::ceil(p.cost * np / cap)));
      if (parts > 1)
        for (uint32_t j = 0; j < p.t.ncu; j++) wl.split.push_back(wl.jobs[p.t.cu0 + j].cu);
      for (int i = 0; i < parts; i++) {
        Piece c = p;
        c.t.q0 = (uint8_t)(p.t.q0 + np * i / parts);
        c.t.q1 = (uint8_t)(p.t.q0 + np * (i + 1) / parts);
        c.cost = p.cost * (c.t.q1 - c.t.q0) + 150.0;
        if (knobs.no_pairs) c.t.q1 = c.t.q0;  // profiling: task prologues only
        cut.push_back(c);
      }
    }
    std::stable_sort(cut.begin(), cut.end(), [](const Piece &a, const Piece &b) { return a.cost > b.cost; });
    const int bins = slices;
    std::vector<double> load(bins, 0.0);
    std::vector<std::vector<WaveTask>> lists(bins);
    for (const Piece &p : cut) {
      const int b = (int)(std::min_element(load.begin(), load.end()) - load.begin());
      load[b] += p.cost;
      lists[b].push_back(p.t);
    }
    for (int b = 0; b < bins; b++) {
      wl.list_begin.push_back((int)wl.tasks.size());
      wl.tasks.insert(wl.tasks.end(), lists[b].begin(), lists[b].end());
      wl.list_cost.push_back(load[b] / waves);
    }
  }
  wl.list_begin.push_back((int)wl.tasks.size());
  wl.fill_begin.push_back((int)wl.fill.size());
  wl.dfill_begin.push_back((int)wl.dfill.size());
  if (!wl.split_begin.empty())
    wl.max_split = std::max(wl.max_split, (int)wl.split.size() - wl.split_begin.back());
  wl.split_begin.push_back((int)wl.split.size());
}

// Per-item cost beyond its tasks (window staging, barriers, fills), in the task cost
// model's units (pair_cost: VALU instructions per lane).
constexpr double kItemOverhead = 600.0;

// Small launches: the frame's items (CTU, quadrant, slice) longest first, by the costs of
// the original-reference lists.
inline void order_items(WorkPlan &wp, const std::vector<uint8_t> &ctu_var) {
  const int sl = wp.slices, per_ctu = 4 * sl, nctus = (int)ctu_var.size();
  auto list_of = [&](uint32_t item) {
    const int c = (int)(item / per_ctu), g = (int)(item % per_ctu), q = g / sl, slc = g % sl;
    return (ctu_var[c] * 4 + q) * sl + slc;
  };
  auto empty = [&](int l) { return wp.list_begin[l + 1] == wp.list_begin[l]; };
  std::vector<double> cost((size_t)nctus * per_ctu);
  for (size_t i = 0; i < cost.size(); i++) {
    const int l = list_of((uint32_t)i);
    cost[i] = wp.list_cost[l] + (empty(l) ? kItemOverhead / 8 : kItemOverhead);
  }
  wp.order.resize(cost.size());
  for (size_t i = 0; i < wp.order.size(); i++) wp.order[i] = (uint32_t)i;
  std::stable_sort(wp.order.begin(), wp.order.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
  wp.order_cost.resize(wp.order.size());
  for (size_t i = 0; i < wp.order.size(); i++) wp.order_cost[i] = cost[wp.order[i]];
  for (uint32_t it : wp.order) {  // (the empty items cost kItemOverhead / 8: they come last)
    if (empty(list_of(it))) break;
    wp.nonempty++;
  }
}

// Everything an engine uploads: the CTU variants and one WorkPlan per (slices, wide) pair --
// the non-wide lists of every slice count of `slice_set`, in its order, then the wide ones.
// (More than kMaxCtuVariants variants: no lists; mip_engine_create refuses the frame size.)
struct EnginePlan {
  CtuVariants cv;
  std::vector<WorkPlan> work;
};

inline EnginePlan plan_engine(int width, int height, int filter, const std::vector<int> &slice_set,
                              const PlanKnobs &knobs = PlanKnobs()) {
  EnginePlan p;
  p.cv = ctu_variants(width, height, filter);
  if (p.cv.pattern.size() > (size_t)kMaxCtuVariants) return p;
  for (int wide = 0; wide < 2; wide++)
    for (int sl : slice_set) {
      p.work.emplace_back();
      WorkPlan &wp = p.work.back();
      wp.slices = sl;
      wp.wide = wide != 0;
      build_work(wp, wide ? kWideWaves : kSearchWaves, p.cv, knobs);
      order_items(wp, p.cv.of_ctu[kMapOrig]);
    }
  return p;
}

// Makespan of `nframes` frames' items taken longest first (SearchArgs::order) by `groups`
// persistent workgroups: greedy list scheduling of the queue order.
inline double lpt_makespan(const std::vector<double> &order_cost, int nframes, int groups) {
  std::vector<double> fin(groups, 0.0);  // min-heap of finish times
  for (double c : order_cost)
    for (int f = 0; f < nframes; f++) {
      std::pop_heap(fin.begin(), fin.end(), std::greater<double>());
      fin.back() += c;
      std::push_heap(fin.begin(), fin.end(), std::greater<double>());
    }
  return *std::max_element(fin.begin(), fin.end());
}

// Large and CTU-range launches: the non-wide lists whose slice count is the closest to
// `want` (the first of equals); index into `work`, -1 when there is none.
inline int closest_slices(const std::vector<WorkPlan> &work, int want) {
  int best = -1;
  for (size_t i = 0; i < work.size(); i++)
    if (!work[i].wide && (best < 0 || std::abs(work[i].slices - want) < std::abs(work[best].slices - want))) best = (int)i;
  return best;
}

// Small launches: the lists (wide or not) whose predicted makespan for `nframes` frames on
// `groups` workgroups is the shortest (the first of equals); index into `work`, -1 when
// there is none.
inline int shortest_makespan(const std::vector<WorkPlan> &work, bool wide, int nframes, int groups) {
  int best = -1;
  double best_m = 0;
  for (size_t i = 0; i < work.size(); i++) {
    if (work[i].wide != wide) continue;
    const double m = lpt_makespan(work[i].order_cost, nframes, groups);
    if (best < 0 || m < best_m) best = (int)i, best_m = m;
  }
  return best;
}

// Small launches on 16-wave workgroups, one per CU: by default below kWideItemsPerGroup items
// per CU at one slice.  Two 8-wave workgroups (round 4)
// on a CU progress at very different rates when both run an item (the SIMD arbiter serves the
// older waves first: 98 vs 170 us for the two items of a CU in a 1080p frame,
// profiles/r04_item_timeline_1frame.csv), so a launch of ~2 items per CU ends with one
// workgroup running alone; a 16-wave workgroup has all its waves on one item's tasks.
// Measured (profiles/r04_small_batch_wide.jsonl): 1 frame 0.185 -> 0.175 ms, 2 frames
// 0.293 -> 0.314 ms (without a second workgroup the item tails and window stagings idle the
// CU), 8-16 frames -9 %.
// Round 6 (six-wave 12-wave workgroups, tools/experiments/r06/small_ab.sh): 2-frame launches
// (3.98 items per CU) 0.2905 ms on 12-wave workgroups vs 0.2967 wide, 1 frame 0.1758 vs 0.1743
// -- the threshold moved from 4 to 3 items per CU (only one-frame 1080p launches go wide).
constexpr int kWideItemsPerGroup = 3;
inline bool few_items_per_cu(long long items1, int cus) { return items1 < (long long)kWideItemsPerGroup * cus; }

}  // namespace mipgpu

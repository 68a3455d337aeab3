// angular_plan.h -- the directional (angular) intra costs (include/mipgpu.h, mip_angular_device)
// as per-sample and per-4x4-block arithmetic, shared by the kernels (mip_angular.hip: one lane per
// 4x4 block, a wave-uniform loop over the mode list) and by the host restatement below
// (angular_frames_host: the same steps, one CU at a time), plus the argmin over the list and the
// decision merge.  Reference samples, SAD, SATD and cost are intra_plan.h's.  No HIP dependency
// on the host side; unit-tested by tests/cpp/test_angular_plan.cpp.
// The coarse-to-fine search (mip_angular_refine_device, the same file's refinement pass) adds the running
// top three of the list, the seed and candidate step, and its own host walk
// (angular_refine_frames_host); unit-tested by tests/cpp/test_angular_refine.cpp.
//
// A "Ref" is intra_plan.h's: any callable ref(row, col) -> reference sample.
#pragma once
#include "intra_plan.h"

namespace mipgpu {

constexpr int kAngModes = MIP_ANGULAR_MODES;  // table slot = mode - 2
constexpr int32_t kAngMaxBias = 1 << 20;

// ---- angle and inverse angle of mode m (2..66): |A| by distance from the pure mode of the class
MIP_INTRA_HD int ang_abs_angle(int k) {
  constexpr int t[17] = {0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 23, 26, 29, 32};
  return t[k];
}
MIP_INTRA_HD int ang_abs_inverse(int k) {  // round(16384 / |A|), 0 for A = 0
  constexpr int t[17] = {0, 16384, 8192, 5461, 4096, 2731, 2048, 1638, 1365, 1170, 1024, 910, 819, 712, 630, 565, 512};
  return t[k];
}
MIP_INTRA_HD int ang_angle(int m) {
  const int k = m < 34 ? 18 - m : m - 50;  // horizontal class: positive towards mode 2
  return k < 0 ? -ang_abs_angle(-k) : ang_abs_angle(k);
}
MIP_INTRA_HD int ang_inverse(int m) {
  const int k = m < 34 ? 18 - m : m - 50;
  return ang_abs_inverse(k < 0 ? -k : k);
}

// One mode of a list as the kernel takes it: mode | (A + 32) << 8 | inv << 16.
struct AngMode {
  int m, angle, inv;
};
MIP_INTRA_HD uint32_t ang_pack(int m) { return (uint32_t)m | (uint32_t)(ang_angle(m) + 32) << 8 | (uint32_t)ang_inverse(m) << 16; }
MIP_INTRA_HD AngMode ang_unpack(uint32_t v) { return AngMode{(int)(v & 0xffu), (int)(v >> 8 & 0xffu) - 32, (int)(v >> 16)}; }

// The mode list of a call: NULL with nmodes == 0 is all 65 modes, else 1..65 strictly increasing
// mode numbers in 2..66.  packed[q] (q < n) in list order, listed: bit (m - 2) of the slots.
struct AngList {
  uint32_t packed[kAngModes];
  uint32_t listed[3];
  int n;
};
inline bool ang_list(const uint8_t *modes, int nmodes, AngList *out) {
  if (!modes ? nmodes != 0 : (nmodes < 1 || nmodes > kAngModes)) return false;
  AngList l{};
  l.n = modes ? nmodes : kAngModes;
  for (int q = 0, before = 0; q < l.n; q++) {
    const int m = modes ? modes[q] : MIP_ANGULAR_FIRST + q;
    if (m < MIP_ANGULAR_FIRST || m > MIP_ANGULAR_LAST || m <= before) return false;
    before = m;
    l.packed[q] = ang_pack(m);
    l.listed[(m - 2) >> 5] |= 1u << ((m - 2) & 31);
  }
  *out = l;
  return true;
}
MIP_INTRA_HD bool ang_listed(const uint32_t *listed, int slot) { return listed[slot >> 5] >> (slot & 31) & 1u; }
inline bool ang_bias_ok(int32_t bias) { return bias >= 0 && bias <= kAngMaxBias; }

// ---- the extended reference of the w x h CU at (x, y): top / left are the MIP path's complete
// boundaries, the corner is R[(y-1)*W + x-1] or top[0]; samples past either end repeat the last.
// A "Bound" gives the two boundary lines: w, h, sample(top_line, t) = top[t] or left[t], and
// corner().  AngBound is the one over a Ref; the kernel has its own over the staged window.
template <class Ref>
struct AngBound {
  const Ref &ref;
  int x, y, w, h;
  MIP_INTRA_HD int sample(bool top_line, int t) const { return top_line ? intra_top(ref, x, y, t) : intra_left(ref, x, y, t); }
  MIP_INTRA_HD int corner() const { return x > 0 && y > 0 ? ref(y - 1, x - 1) : intra_top(ref, x, y, 0); }
};
// ref[k] of the class: VERT main = top, side = left; else the transpose.  One boundary read:
// k <= 0 is side'[min(p, S)] with p = (-k*inv + 256) >> 9, and p == 0 (k == 0 too) is the corner.
template <bool VERT, class Bound>
MIP_INTRA_HD int ang_ref(const Bound &b, int k, int inv, int corner) {
  const int M = VERT ? b.w : b.h, S = VERT ? b.h : b.w;
  const bool main = k > 0;
  const int p = (-k * inv + 256) >> 9;  // (used for k <= 0, reached only with A < 0)
  const int t = main ? (k < M ? k : M) - 1 : (p < S ? p : S) - 1;
  const int v = b.sample(main == VERT, t < 0 ? 0 : t);
  return t < 0 ? corner : v;
}
// the same for A >= 0, where every k is >= 1
template <bool VERT, class Bound>
MIP_INTRA_HD int ang_ref_main(const Bound &b, int k) {
  const int M = VERT ? b.w : b.h;
  return b.sample(VERT, (k < M ? k : M) - 1);
}

MIP_INTRA_HD int ang_clip(int v) { return v < 0 ? 0 : v > 1023 ? 1023 : v; }

// ---- one sample: the predictor as the contract writes it (the block step below computes the
// same values with the per-row terms hoisted).
template <class Bound>
MIP_INTRA_HD int ang_sample(const Bound &b, const AngMode &md, int lw, int lh, int i, int j) {
  const bool vert = md.m >= 34;
  const int a = vert ? i : j, bb = vert ? j : i;
  const int d = (bb + 1) * md.angle, idx = d >> 5, f = d & 31, c = b.corner();
  const int r0 = vert ? ang_ref<true>(b, a + idx + 1, md.inv, c) : ang_ref<false>(b, a + idx + 1, md.inv, c);
  int p = r0;
  if (f) {
    const int r1 = vert ? ang_ref<true>(b, a + idx + 2, md.inv, c) : ang_ref<false>(b, a + idx + 2, md.inv, c);
    p = ((32 - f) * r0 + f * r1 + 16) >> 5;
  }
  if (md.m == 18 || md.m == 50) {
    const int wgt = intra_pdpc_weight(a, (lw + lh - 2) >> 2);
    const int side = b.sample(!vert, bb) - c + p;
    p = (side * wgt + (64 - wgt) * p + 32) >> 6;
  }
  return ang_clip(p);
}

// ---- one 4x4 block of a CU, one mode: what one lane of the kernel computes per mode.  Along the
// side direction (rows of the vertical class, columns of the horizontal one) idx and f are
// constant, so the four samples of such a line need the five consecutive ref[a0+idx+1 .. +5].
// (f == 0 needs no case of its own: ((32 - 0) * r + 16) >> 5 == r for r >= 0.)
// org: the block's 16 original samples, row-major; (i0, j0) the block's place inside the CU.
template <bool VERT, class Bound>
MIP_INTRA_HD void ang_block_class(const Bound &b, const AngMode &md, int corner, int lw, int lh, int i0, int j0,
                                  const int *org, int &sad, int &satd) {
  const int a0 = VERT ? i0 : j0, b0 = VERT ? j0 : i0;
  const bool pdpc = md.m == 18 || md.m == 50;
  const int scale = (lw + lh - 2) >> 2;
  int wgt[4] = {0, 0, 0, 0};
  if (pdpc) {
    MIP_INTRA_UNROLL
    for (int c = 0; c < 4; c++) wgt[c] = intra_pdpc_weight(a0 + c, scale);
  }
  int d[16];
  MIP_INTRA_UNROLL
  for (int r = 0; r < 4; r++) {
    const int dd = (b0 + r + 1) * md.angle, idx = dd >> 5, f = dd & 31;
    int s[5];
    if (md.angle >= 0) {
      MIP_INTRA_UNROLL
      for (int t = 0; t < 5; t++) s[t] = ang_ref_main<VERT>(b, a0 + idx + 1 + t);
    } else {
      MIP_INTRA_UNROLL
      for (int t = 0; t < 5; t++) s[t] = ang_ref<VERT>(b, a0 + idx + 1 + t, md.inv, corner);
    }
    const int side = pdpc ? b.sample(!VERT, b0 + r) - corner : 0;
    MIP_INTRA_UNROLL
    for (int c = 0; c < 4; c++) {
      int p = ((32 - f) * s[c] + f * s[c + 1] + 16) >> 5;
      if (pdpc) p = ((side + p) * wgt[c] + (64 - wgt[c]) * p + 32) >> 6;
      const int at = VERT ? 4 * r + c : 4 * c + r;
      d[at] = org[at] - ang_clip(p);
    }
  }
  sad = intra_sad16(d);
  satd = intra_satd4x4(d);
}
template <class Bound>
MIP_INTRA_HD void ang_block(const Bound &b, const AngMode &md, int corner, int lw, int lh, int i0, int j0, const int *org,
                            int &sad, int &satd) {
  if (md.m >= 34) ang_block_class<true>(b, md, corner, lw, lh, i0, j0, org, sad, satd);
  else ang_block_class<false>(b, md, corner, lw, lh, i0, j0, org, sad, satd);
}

// ---- extended reference lines (include/mipgpu.h, mip_angular_refs): the real above-right and
// below-left samples.  The order key of the sample at frame position (sx, sy): the raster index
// of its CTU, then the Morton code of its 4x4 block inside the CTU (x the even bits, y the odd
// ones) -- z-scan of 4x4 blocks inside CTU raster order.
MIP_INTRA_HD uint32_t ang_spread5(uint32_t v) {  // bit k of v (k < 5) to bit 2k
  v = (v | v << 8) & 0x00ffu;
  v = (v | v << 4) & 0x0f0fu;
  v = (v | v << 2) & 0x3333u;
  return (v | v << 1) & 0x5555u;
}
MIP_INTRA_HD uint32_t ang_order_key(int sx, int sy, int ctu_cols) {
  const uint32_t ctu = (uint32_t)((sy >> 7) * ctu_cols + (sx >> 7));
  return ctu << 10 | ang_spread5((uint32_t)(sx & 127) >> 2) | ang_spread5((uint32_t)(sy & 127) >> 2) << 1;
}
// The two lengths of the w x h CU at (x, y): how many real samples extend its top line (0..h) and
// its left line (0..w).  undefined(linear index): the reference sample is one an engine filter
// leaves undefined (work_plan.h filter_poison; never, without one).
struct AngExt {
  int top, left;
};
template <class Undefined>
inline AngExt ang_ext_lengths(int W, int H, int x, int y, int w, int h, bool unavailable, const Undefined &undefined) {
  AngExt e{0, 0};
  if (unavailable || x + w > W || y + h > H) return e;
  const int cols = (W + 127) / 128;
  const uint32_t own = ang_order_key(x, y, cols);
  while (e.top < h && y > 0 && x + w + e.top < W && ang_order_key(x + w + e.top, y - 1, cols) < own &&
         !undefined((long long)(y - 1) * W + x + w + e.top))
    e.top++;
  while (e.left < w && x > 0 && y + h + e.left < H && ang_order_key(x - 1, y + h + e.left, cols) < own &&
         !undefined((long long)(y + h + e.left) * W + x - 1))
    e.left++;
  return e;
}
// A Bound as one class sees it with its main line extended: w (vertical class) or h (horizontal
// class) is M' = M + E(main), the other length stays the side's cap S.  Over it ang_ref,
// ang_ref_main, ang_sample and ang_block_class are the extended predictor: a larger clamp bound
// for reads of the main line, nothing else.  The Bound's sample(line, t) must reach t < M'.
template <class Bound>
struct AngExtView {
  const Bound &b;
  int w, h;
  MIP_INTRA_HD int sample(bool top_line, int t) const { return b.sample(top_line, t); }
  MIP_INTRA_HD int corner() const { return b.corner(); }
};
template <class Bound>
MIP_INTRA_HD AngExtView<Bound> ang_ext_view(const Bound &b, bool vert, int e_top, int e_left) {
  return AngExtView<Bound>{b, b.w + (vert ? e_top : 0), b.h + (vert ? 0 : e_left)};
}
template <class Bound>
MIP_INTRA_HD int ang_sample_ext(const Bound &b, int e_top, int e_left, const AngMode &md, int lw, int lh, int i, int j) {
  return ang_sample(ang_ext_view(b, md.m >= 34, e_top, e_left), md, lw, lh, i, j);
}
template <class Bound>
MIP_INTRA_HD void ang_block_ext(const Bound &b, int e_top, int e_left, const AngMode &md, int corner, int lw, int lh, int i0, int j0,
                                const int *org, int &sad, int &satd) {
  if (md.m >= 34) ang_block_class<true>(ang_ext_view(b, true, e_top, e_left), md, corner, lw, lh, i0, j0, org, sad, satd);
  else ang_block_class<false>(ang_ext_view(b, false, e_top, e_left), md, corner, lw, lh, i0, j0, org, sad, satd);
}

// ---- VVC's 4-tap luma interpolation (include/mipgpu.h, mip_angular_interp, MIP_ANG_INTERP_4TAP):
// only the line P = ... of the predictor changes.  The cubic table fC for f = 0..16 (fC[32 - f] is
// fC[f] reversed), the Gaussian fG[f] = {16 - (f>>1), 32 - (f>>1), 16 + (f>>1), f>>1}, and which of
// the two a (CU shape, mode) takes.
MIP_INTRA_HD int ang_cubic(int f, int t) {  // fC[f][t], f in 0..31, t in 0..3
  constexpr signed char c[17][4] = {{0, 64, 0, 0},   {-1, 63, 2, 0},  {-2, 62, 4, 0},   {-2, 60, 7, -1},  {-2, 58, 10, -2}, {-3, 57, 12, -2},
                                    {-4, 56, 14, -2}, {-4, 55, 15, -2}, {-4, 54, 16, -2}, {-5, 53, 18, -2}, {-6, 52, 20, -2}, {-6, 49, 24, -3},
                                    {-6, 46, 28, -4}, {-5, 44, 29, -4}, {-4, 42, 30, -4}, {-4, 39, 33, -4}, {-4, 36, 36, -4}};
  return f <= 16 ? c[f][t] : c[32 - f][3 - t];
}
MIP_INTRA_HD int ang_gauss(int f, int t) {  // fG[f][t]
  const int h = f >> 1;
  return t == 0 ? 16 - h : t == 1 ? 32 - h : t == 2 ? 16 + h : h;
}
// G of the contract: the Gaussian filter where the mode's distance from the nearer pure mode
// exceeds the threshold of the CU's size class (lw + lh) >> 1 = 2..6.
MIP_INTRA_HD int ang_gauss_threshold(int lw, int lh) {
  const int n = (lw + lh) >> 1;
  return n <= 2 ? 24 : n == 3 ? 14 : n == 4 ? 2 : 0;
}
MIP_INTRA_HD bool ang_filter_gauss(int m, int lw, int lh) {
  const int dv = m > 50 ? m - 50 : 50 - m, dh = m > 18 ? m - 18 : 18 - m;
  return (dv < dh ? dv : dh) > ang_gauss_threshold(lw, lh);
}
// The four coefficients of (G, f) as one word of signed bytes, c[0] lowest: every coefficient of
// both tables lies in -6 .. 64.  The kernels keep the 64 words in LDS at index G << 5 | f.
constexpr int kAngCoefWords = 64;
MIP_INTRA_HD uint32_t ang_coef_word(bool gauss, int f) {
  uint32_t w = 0;
  for (int t = 0; t < 4; t++) w |= (uint32_t)((gauss ? ang_gauss(f, t) : ang_cubic(f, t)) & 0xff) << (8 * t);
  return w;
}
MIP_INTRA_HD int ang_coef(uint32_t word, int t) { return (int)(word << (24 - 8 * t)) >> 24; }
// A "Coef" is any callable coef(gauss, f) -> that word: AngCoefTable computes it; the kernels
// have their own over the staged words.
struct AngCoefTable {
  MIP_INTRA_HD uint32_t operator()(bool gauss, int f) const { return ang_coef_word(gauss, f); }
};
// ref[k] for A >= 0 under the 4-tap filter, whose first tap reaches k = 0: the corner.
template <bool VERT, class Bound>
MIP_INTRA_HD int ang_ref_main0(const Bound &b, int k, int corner) {
  const int M = VERT ? b.w : b.h;
  const int v = b.sample(VERT, (k < 1 ? 1 : k < M ? k : M) - 1);
  return k < 1 ? corner : v;
}
MIP_INTRA_HD int ang_tap4(uint32_t word, int r0, int r1, int r2, int r3) {
  return (ang_coef(word, 0) * r0 + ang_coef(word, 1) * r1 + ang_coef(word, 2) * r2 + ang_coef(word, 3) * r3 + 32) >> 6;
}
// ang_sample with the 4-tap line: the taps are ref[k-1 .. k+2] (ang_ref gives the corner at 0 for
// every angle), for every f including 0.
template <class Bound>
MIP_INTRA_HD int ang_sample_tap4(const Bound &b, const AngMode &md, int lw, int lh, int i, int j) {
  const bool vert = md.m >= 34;
  const int a = vert ? i : j, bb = vert ? j : i;
  const int d = (bb + 1) * md.angle, idx = d >> 5, f = d & 31, c = b.corner(), k = a + idx + 1;
  int r[4];
  for (int t = 0; t < 4; t++) r[t] = vert ? ang_ref<true>(b, k - 1 + t, md.inv, c) : ang_ref<false>(b, k - 1 + t, md.inv, c);
  int p = ang_tap4(ang_coef_word(ang_filter_gauss(md.m, lw, lh), f), r[0], r[1], r[2], r[3]);
  if (md.m == 18 || md.m == 50) {
    const int wgt = intra_pdpc_weight(a, (lw + lh - 2) >> 2);
    const int side = b.sample(!vert, bb) - c + p;
    p = (side * wgt + (64 - wgt) * p + 32) >> 6;
  }
  return ang_clip(p);
}
// ang_block_class with the 4-tap line: the four samples of a line along the side direction need the
// seven consecutive ref[a0+idx .. a0+idx+6]; one coefficient word per line.
template <bool VERT, class Bound, class Coef>
MIP_INTRA_HD void ang_block_tap4_class(const Bound &b, const AngMode &md, int corner, int lw, int lh, int i0, int j0, const int *org,
                                       const Coef &coef, int &sad, int &satd) {
  const int a0 = VERT ? i0 : j0, b0 = VERT ? j0 : i0;
  const bool pdpc = md.m == 18 || md.m == 50;
  const bool gauss = ang_filter_gauss(md.m, lw, lh);
  const int scale = (lw + lh - 2) >> 2;
  int wgt[4] = {0, 0, 0, 0};
  if (pdpc) {
    MIP_INTRA_UNROLL
    for (int c = 0; c < 4; c++) wgt[c] = intra_pdpc_weight(a0 + c, scale);
  }
  int d[16];
  MIP_INTRA_UNROLL
  for (int r = 0; r < 4; r++) {
    const int dd = (b0 + r + 1) * md.angle, idx = dd >> 5, f = dd & 31;
    const uint32_t word = coef(gauss, f);
    int s[7];
    if (md.angle >= 0) {
      s[0] = ang_ref_main0<VERT>(b, a0 + idx, corner);
      MIP_INTRA_UNROLL
      for (int t = 1; t < 7; t++) s[t] = ang_ref_main<VERT>(b, a0 + idx + t);
    } else {
      MIP_INTRA_UNROLL
      for (int t = 0; t < 7; t++) s[t] = ang_ref<VERT>(b, a0 + idx + t, md.inv, corner);
    }
    const int side = pdpc ? b.sample(!VERT, b0 + r) - corner : 0;
    MIP_INTRA_UNROLL
    for (int c = 0; c < 4; c++) {
      int p = ang_tap4(word, s[c], s[c + 1], s[c + 2], s[c + 3]);
      if (pdpc) p = ((side + p) * wgt[c] + (64 - wgt[c]) * p + 32) >> 6;
      const int at = VERT ? 4 * r + c : 4 * c + r;
      d[at] = org[at] - ang_clip(p);
    }
  }
  sad = intra_sad16(d);
  satd = intra_satd4x4(d);
}
template <class Bound>
MIP_INTRA_HD int ang_sample_tap4_ext(const Bound &b, int e_top, int e_left, const AngMode &md, int lw, int lh, int i, int j) {
  return ang_sample_tap4(ang_ext_view(b, md.m >= 34, e_top, e_left), md, lw, lh, i, j);
}
template <class Bound, class Coef>
MIP_INTRA_HD void ang_block_tap4_ext(const Bound &b, int e_top, int e_left, const AngMode &md, int corner, int lw, int lh, int i0, int j0,
                                     const int *org, const Coef &coef, int &sad, int &satd) {
  if (md.m >= 34) ang_block_tap4_class<true>(ang_ext_view(b, true, e_top, e_left), md, corner, lw, lh, i0, j0, org, coef, sad, satd);
  else ang_block_tap4_class<false>(ang_ext_view(b, false, e_top, e_left), md, corner, lw, lh, i0, j0, org, coef, sad, satd);
}

// ---- argmin over the list (in list order, i.e. increasing mode: ties keep the lower mode) and
// the merge: the best angular mode replaces the current decision only if its biased cost is
// strictly lower.  Unavailable CUs (either side) stay as they are.
MIP_INTRA_HD void ang_best_step(uint8_t &mode, int32_t &cost, int m, int32_t c) {
  if (c < cost) cost = c, mode = (uint8_t)MIP_MODE_ANGULAR(m);
}
MIP_INTRA_HD void ang_merge(uint8_t &mode, int32_t &cost, uint8_t ang_mode, int32_t ang_cost, int32_t bias) {
  if (cost == MIP_COST_UNAVAILABLE || ang_cost == MIP_COST_UNAVAILABLE) return;
  if (ang_cost + bias < cost) cost = ang_cost + bias, mode = ang_mode;
}

// ---- coarse-to-fine (mip_angular_refine_device): the running top three of the list, the
// candidate step and the argmin over modes that arrive in any order.
constexpr int kAngMaxSeeds = MIP_ANGULAR_MAX_SEEDS;
inline bool ang_seeds_ok(int seeds) { return seeds >= 1 && seeds <= kAngMaxSeeds; }

// The three lowest (cost, mode) of the modes seen so far, lowest first; mode 0 = no entry.  The
// list arrives in increasing mode order and only a strictly lower cost moves an entry down, so
// ties keep the lower mode in front.
struct AngTop {
  int32_t c0, c1, c2;
  int m0, m1, m2;
};
MIP_INTRA_HD AngTop ang_top_none() { return AngTop{MIP_COST_UNAVAILABLE, MIP_COST_UNAVAILABLE, MIP_COST_UNAVAILABLE, 0, 0, 0}; }
MIP_INTRA_HD void ang_top_step(AngTop &t, int m, int32_t c) {
  const bool b0 = c < t.c0, b1 = c < t.c1, b2 = c < t.c2;
  t.c2 = b1 ? t.c1 : b2 ? c : t.c2;
  t.m2 = b1 ? t.m1 : b2 ? m : t.m2;
  t.c1 = b0 ? t.c0 : b1 ? c : t.c1;
  t.m1 = b0 ? t.m0 : b1 ? m : t.m1;
  t.c0 = b0 ? c : t.c0;
  t.m0 = b0 ? m : t.m0;
}

// A set of modes as the listed-slot mask: bit (m - 2).
struct AngSet {
  uint32_t w0, w1, w2;
};
MIP_INTRA_HD void ang_set_add(AngSet &s, int m, bool on) {  // m in 2..66 where `on`
  const int slot = m - MIP_ANGULAR_FIRST;
  const uint32_t bit = on ? 1u << (slot & 31) : 0u;
  s.w0 |= (slot >> 5) == 0 ? bit : 0u;
  s.w1 |= (slot >> 5) == 1 ? bit : 0u;
  s.w2 |= (slot >> 5) == 2 ? bit : 0u;
}
MIP_INTRA_HD int ang_set_count(const AngSet &s) { return __builtin_popcount(s.w0) + __builtin_popcount(s.w1) + __builtin_popcount(s.w2); }
// Takes the lowest mode out of the set and returns it; 0 if the set is empty.
MIP_INTRA_HD int ang_set_pop(AngSet &s) {
  const int w = s.w0 ? 0 : s.w1 ? 1 : 2;
  const uint32_t v = s.w0 ? s.w0 : s.w1 ? s.w1 : s.w2;
  const int bit = v ? __builtin_ctz(v) : 0;
  const uint32_t rest = v & (v - 1u);
  s.w0 = w == 0 ? rest : s.w0;
  s.w1 = w == 1 ? rest : s.w1;
  s.w2 = w == 2 ? rest : s.w2;
  return v ? MIP_ANGULAR_FIRST + 32 * w + bit : 0;
}
// The seed and candidate step: the first min(nseeds, entries) entries of the CU's top list are
// its seeds; the candidates are their +-1 neighbours inside 2..66 (no wrap) that the list does
// not hold, as a set -- a neighbour of two seeds counts once -- which ang_set_pop hands out in
// increasing mode order.
MIP_INTRA_HD AngSet ang_candidates(const AngTop &t, int nseeds, const uint32_t *listed) {
  AngSet s{0u, 0u, 0u};
  const int seed[kAngMaxSeeds] = {t.m0, t.m1, t.m2};
  MIP_INTRA_UNROLL
  for (int q = 0; q < kAngMaxSeeds; q++) {
    const bool is = q < nseeds && seed[q] != 0;
    ang_set_add(s, seed[q] - 1, is && seed[q] > MIP_ANGULAR_FIRST);
    ang_set_add(s, seed[q] + 1, is && seed[q] < MIP_ANGULAR_LAST);
  }
  s.w0 &= ~listed[0];
  s.w1 &= ~listed[1];
  s.w2 &= ~listed[2];
  return s;
}
// argmin of (cost, mode) over modes in any order
MIP_INTRA_HD void ang_best_step_any(uint8_t &mode, int32_t &cost, int m, int32_t c) {
  const uint8_t code = (uint8_t)MIP_MODE_ANGULAR(m);
  if (c < cost || (c == cost && code < mode)) cost = c, mode = code;
}

// ---- host side: one CU (every mode of the list), then the whole walk
// (e_top / e_left: the CU's extended lengths, 0 / 0 the substituted lines; interp: the engine's
// mip_angular_interp setting, MIP_ANG_INTERP_2TAP or MIP_ANG_INTERP_4TAP)
inline void angular_cu_host(const uint16_t *orig, const uint16_t *refs, int width, int x, int y, int lw, int lh, const AngList &list,
                            int32_t *sad, int32_t *satd, int e_top = 0, int e_left = 0, int interp = MIP_ANG_INTERP_2TAP) {
  const IntraHostRef ref{refs, width};
  const int w = 1 << lw, h = 1 << lh;
  const AngBound<IntraHostRef> b{ref, x, y, w, h};
  const int corner = b.corner();
  for (int q = 0; q < list.n; q++) sad[q] = satd[q] = 0;
  for (int j0 = 0; j0 < h; j0 += 4)
    for (int i0 = 0; i0 < w; i0 += 4) {
      int org[16];
      for (int r = 0; r < 4; r++)
        for (int c = 0; c < 4; c++) org[4 * r + c] = orig[(size_t)(y + j0 + r) * width + x + i0 + c];
      for (int q = 0; q < list.n; q++) {
        int s, t;
        if (interp == MIP_ANG_INTERP_4TAP)
          ang_block_tap4_ext(b, e_top, e_left, ang_unpack(list.packed[q]), corner, lw, lh, i0, j0, org, AngCoefTable{}, s, t);
        else
          ang_block_ext(b, e_top, e_left, ang_unpack(list.packed[q]), corner, lw, lh, i0, j0, org, s, t);
        sad[q] += s;
        satd[q] += t;
      }
    }
}

// The predicted block of one CU and mode, sample by sample (ang_sample, or ang_sample_tap4 with
// interp == MIP_ANG_INTERP_4TAP): row r at out[r * pitch].
inline void angular_predict_cu_host(const uint16_t *refs, int width, int x, int y, int lw, int lh, int mode, uint16_t *out, int pitch,
                                    int e_top = 0, int e_left = 0, int interp = MIP_ANG_INTERP_2TAP) {
  const IntraHostRef ref{refs, width};
  const AngBound<IntraHostRef> b{ref, x, y, 1 << lw, 1 << lh};
  const AngMode md = ang_unpack(ang_pack(mode));
  for (int j = 0; j < (1 << lh); j++)
    for (int i = 0; i < (1 << lw); i++)
      out[(size_t)j * pitch + i] = (uint16_t)(interp == MIP_ANG_INTERP_4TAP ? ang_sample_tap4_ext(b, e_top, e_left, md, lw, lh, i, j)
                                                                            : ang_sample_ext(b, e_top, e_left, md, lw, lh, i, j));
}

// Everything mip_angular_device writes, on host arrays (each output optional, the pairs given
// together): frames / refs [nframes][height][width] (refs already resolved), unavail
// [nctus*5380] the availability set that goes with refs, modes / nmodes the call's list; cost /
// sad / satd [nframes][nctus*5380][65], ang_mode / ang_cost and best_mode / best_cost
// [nframes][nctus*5380].  Returns 0, or -1 for arguments the entry point rejects (nothing
// written).  ext_top / ext_left [nctus*5380] (both or neither): the extended lengths of
// mip_extended_refs for the same availability set; NULL is the substituted lines.  interp: the
// mip_angular_interp setting (anything but the two values is rejected).
inline int angular_frames_host(const uint16_t *frames, const uint16_t *refs, const uint8_t *unavail, int width, int height,
                               int nframes, const uint8_t *modes, int nmodes, int32_t *cost, int32_t *sad, int32_t *satd,
                               uint8_t *ang_mode, int32_t *ang_cost, int32_t bias, uint8_t *best_mode, int32_t *best_cost,
                               const uint8_t *ext_top = nullptr, const uint8_t *ext_left = nullptr, int interp = MIP_ANG_INTERP_2TAP) {
  if (!ext_top != !ext_left || (interp != MIP_ANG_INTERP_2TAP && interp != MIP_ANG_INTERP_4TAP)) return -1;
  if (!frames || !refs || !unavail || width <= 0 || height <= 0 || width % 4 || height % 4 || nframes < 1) return -1;
  if (!ang_mode != !ang_cost || !best_mode != !best_cost) return -1;
  if (!cost && !sad && !satd && !ang_cost && !best_cost) return -1;
  AngList list;
  if (!ang_list(modes, nmodes, &list) || !ang_bias_ok(bias)) return -1;
  const int cols = (width + 127) / 128, nctus = cols * ((height + 127) / 128);
  const size_t fs = (size_t)width * height;
  const int32_t none = MIP_COST_UNAVAILABLE;
  for (int f = 0; f < nframes; f++)
    for (int c = 0; c < nctus; c++) {
      size_t k = (size_t)c * MIP_CUS_PER_CTU;
      for (int s = 0; s < MIP_NUM_SHAPES; s++) {
        const mip_shape_desc &sd = kIntraShapes[s];
        for (int cu = 0; cu < sd.ncu; cu++, k++) {
          int32_t a[kAngModes], b[kAngModes];
          const bool on = !unavail[k];
          if (on)
            angular_cu_host(frames + f * fs, refs + f * fs, width, 128 * (c % cols) + intra_axis(sd.xb, sd.xs, sd.xd, cu % sd.ncols),
                            128 * (c / cols) + intra_axis(sd.yb, sd.ys, sd.yd, cu / sd.ncols), intra_log2(sd.w), intra_log2(sd.h), list,
                            a, b, ext_top ? ext_top[k] : 0, ext_left ? ext_left[k] : 0, interp);
          const size_t at = (size_t)f * nctus * MIP_CUS_PER_CTU + k;
          for (int slot = 0; slot < kAngModes; slot++) {
            if (cost) cost[at * kAngModes + slot] = none;
            if (sad) sad[at * kAngModes + slot] = none;
            if (satd) satd[at * kAngModes + slot] = none;
          }
          uint8_t bm = 0xff;
          int32_t bc = none;
          for (int q = 0; on && q < list.n; q++) {
            const int m = ang_unpack(list.packed[q]).m;
            const int32_t v = intra_cost(a[q], b[q]);
            if (cost) cost[at * kAngModes + m - 2] = v;
            if (sad) sad[at * kAngModes + m - 2] = a[q];
            if (satd) satd[at * kAngModes + m - 2] = b[q];
            ang_best_step(bm, bc, m, v);
          }
          if (ang_cost) ang_mode[at] = bm, ang_cost[at] = bc;
          if (best_cost) ang_merge(best_mode[at], best_cost[at], bm, bc, bias);
        }
      }
    }
  return 0;
}

// Everything mip_angular_refine_device writes, on host arrays: angular_frames_host's arguments
// plus seeds and the optional tried [nframes][nctus*5380] (and its ext_top / ext_left).  Per available CU the list's costs, the
// running top three, the candidate step, the candidates' costs, then the pair over both.
inline int angular_refine_frames_host(const uint16_t *frames, const uint16_t *refs, const uint8_t *unavail, int width, int height,
                                      int nframes, const uint8_t *modes, int nmodes, int seeds, int32_t *cost, int32_t *sad,
                                      int32_t *satd, uint8_t *ang_mode, int32_t *ang_cost, uint8_t *tried, int32_t bias,
                                      uint8_t *best_mode, int32_t *best_cost, const uint8_t *ext_top = nullptr,
                                      const uint8_t *ext_left = nullptr, int interp = MIP_ANG_INTERP_2TAP) {
  if (!ext_top != !ext_left || (interp != MIP_ANG_INTERP_2TAP && interp != MIP_ANG_INTERP_4TAP)) return -1;
  if (!frames || !refs || !unavail || width <= 0 || height <= 0 || width % 4 || height % 4 || nframes < 1) return -1;
  if (!ang_mode != !ang_cost || !best_mode != !best_cost) return -1;
  if (!cost && !sad && !satd && !ang_cost && !best_cost && !tried) return -1;
  AngList list;
  if (!ang_list(modes, nmodes, &list) || !ang_bias_ok(bias) || !ang_seeds_ok(seeds)) return -1;
  const int nseeds = seeds < list.n ? seeds : list.n;
  const int cols = (width + 127) / 128, nctus = cols * ((height + 127) / 128);
  const size_t fs = (size_t)width * height;
  const int32_t none = MIP_COST_UNAVAILABLE;
  for (int f = 0; f < nframes; f++)
    for (int c = 0; c < nctus; c++) {
      size_t k = (size_t)c * MIP_CUS_PER_CTU;
      for (int s = 0; s < MIP_NUM_SHAPES; s++) {
        const mip_shape_desc &sd = kIntraShapes[s];
        for (int cu = 0; cu < sd.ncu; cu++, k++) {
          const size_t at = (size_t)f * nctus * MIP_CUS_PER_CTU + k;
          for (int slot = 0; slot < kAngModes; slot++) {
            if (cost) cost[at * kAngModes + slot] = none;
            if (sad) sad[at * kAngModes + slot] = none;
            if (satd) satd[at * kAngModes + slot] = none;
          }
          uint8_t bm = 0xff;
          int32_t bc = none;
          int evaluated = 0;
          if (!unavail[k]) {
            const int x = 128 * (c % cols) + intra_axis(sd.xb, sd.xs, sd.xd, cu % sd.ncols);
            const int y = 128 * (c / cols) + intra_axis(sd.yb, sd.ys, sd.yd, cu / sd.ncols);
            const int lw = intra_log2(sd.w), lh = intra_log2(sd.h);
            int32_t a[kAngModes], b[kAngModes];
            auto take = [&](const AngList &l) {
              angular_cu_host(frames + f * fs, refs + f * fs, width, x, y, lw, lh, l, a, b, ext_top ? ext_top[k] : 0, ext_left ? ext_left[k] : 0, interp);
              for (int q = 0; q < l.n; q++) {
                const int m = ang_unpack(l.packed[q]).m;
                if (cost) cost[at * kAngModes + m - 2] = intra_cost(a[q], b[q]);
                if (sad) sad[at * kAngModes + m - 2] = a[q];
                if (satd) satd[at * kAngModes + m - 2] = b[q];
                ang_best_step_any(bm, bc, m, intra_cost(a[q], b[q]));
              }
              evaluated += l.n;
            };
            take(list);
            AngTop top = ang_top_none();
            for (int q = 0; q < list.n; q++) ang_top_step(top, ang_unpack(list.packed[q]).m, intra_cost(a[q], b[q]));
            AngSet cand = ang_candidates(top, nseeds, list.listed);
            AngList fine{};
            for (int m = ang_set_pop(cand); m; m = ang_set_pop(cand)) fine.packed[fine.n++] = ang_pack(m);
            if (fine.n) take(fine);
          }
          if (ang_cost) ang_mode[at] = bm, ang_cost[at] = bc;
          if (tried) tried[at] = (uint8_t)evaluated;
          if (best_cost) ang_merge(best_mode[at], best_cost[at], bm, bc, bias);
        }
      }
    }
  return 0;
}

}  // namespace mipgpu

// mip_angular_tap4.hip -- the two angular cost kernels with VVC's 4-tap cubic / Gaussian luma
// interpolation (gfx950), contract in include/mipgpu.h (mip_angular_interp, MIP_ANG_INTERP_4TAP).
// No reference counterpart.  angular_tap4_kernel is angular_ext_kernel and angular_tap4_refine_kernel
// is angular_ext_refine_kernel (mip_angular_ext.hip), which both stay as they are: the same work
// items, slot lists, window and extension staging, length clamps, grid rule, mode loops and
// finishing steps, read there and in mip_angular_dev.h / mip_window_dev.h.  One kernel per role
// serves both mip_angular_refs settings: without a length table (a.ext == NULL, the substituted
// lines) every CU's lengths are 0 / 0, which is the substituted predictor bit for bit.  What is new:
//
// The line.  A mode's line of a lane's 4x4 block takes the seven ref[a0+idx .. a0+idx+6] instead of
// five and four multiplies per sample instead of two (angular_plan.h ang_block_tap4_class).
//
// No new staging: every tap index is clamped onto the lines that are staged already.
//   k+2 at M'.  A tap k >= 1 reads main[min(k, M') - 1], the very clamp of the 2-tap predictor: k + 2
//     past M' reads the cell of main[M' - 1] that k and k + 1 read there, and M' is the length
//     ExtLdsBound has cut to the staged extent of the line.
//   k-1 at the side's cap.  A tap k <= 0 reads side'[min((-k*inv + 256) >> 9, S)]: one step further
//     along the side than the 2-tap predictor's lowest tap, but capped at S like it, so it reads
//     side[S - 1] at most -- a cell of the CU's own side line.
//   k-1 = 0 for A >= 0.  The corner, which the lane holds in a register (ExtLdsBound::ce): no read.
//
// Coefficients.  The filter G depends on the lane's CU shape and the wave-uniform mode, the
// fraction f on the lane's row, so the index is divergent.  The 64 coefficient quadruples (G << 5 | f,
// angular_plan.h ang_coef_word: four signed bytes in one word) are staged in LDS once per workgroup
// from the kernel arguments; a lane fetches one word per line of its block (one ds_read_b32, 64
// consecutive words: at most a two-way bank conflict) and unpacks it with four sign-extending
// bit-field extracts -- no select between the tables, no table in constant memory, whose divergent
// index would serialise into one load per distinct address.  The products are 32-bit: references
// are uint16 and an engine filter's can exceed 15 bits, so packed signed 16-bit dot products would
// misread them.  No atomics, no scratch.  DESIGN.md section
// 5.12.
#include "mip_angular_dev.h"

namespace mipgpu {
namespace {

// (the staging, the index rule and the Bound are mip_angular_ext.hip's, copied: the shared headers
// stay as the existing kernels compiled them)
// s_ref of these kernels: the window's reference array, its s_left lengthened to 2S + 1 rows, the
// long copy of row y0-1 and the cell that holds 512.
constexpr int kExtTopAt = kLeftAt + 136;      // row y0-1, 2S <= 128 columns
constexpr int kExtConstAt = kExtTopAt + 128;  // the cell that holds 512
constexpr int kExtRefCells = kExtConstAt + 8;
static_assert(kLeftAt + 2 * 64 + 1 <= kExtTopAt && kExtTopAt % 8 == 0, "s_left with its extension ends before the long row");

// The lane index as a value the compiler takes as new per item (the kernels form tid through it at
// the top of the item loop): per-lane addresses -- the staging's, a.modes[tid], the tables' a.cost +
// tid -- are otherwise hoisted out of the item loop into registers held across the whole item, which
// at three waves per SIMD has none to spare (angular_refine_kernel does the same for its 64x64 path).
__device__ __forceinline__ int opaque(int tid) {
  asm volatile("" : "+v"(tid));
  return tid;
}
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

// IndexRef (mip_angular_dev.h) with row y0-1 taken from its long copy.
struct ExtIndexRef {
  int x0, y0, lp;
  __device__ __forceinline__ int operator()(int row, int col) const {
    const int r = row - y0 + 1;
    return kIndexBias + (col < x0 ? kLeftAt + r : r == 0 ? kExtTopAt + col - x0 : (r << lp) + col - x0);
  }
};
// LdsBound (mip_angular_dev.h) over that index rule, plus the CU's two lengths: the table's, each
// cut to what is staged behind its line -- 2S columns of row y0-1 and S of any other row, 2S + 1
// rows of column x0-1 and S + 1 of any other column.
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
// A Coef of angular_plan.h over the staged words.
struct LdsCoef {
  const uint32_t *word;
  __device__ __forceinline__ uint32_t operator()(bool gauss, int f) const { return word[(gauss ? 32 : 0) + f]; }
};

// (mode_word is angular_refine_kernel's: the clamp of a mode chosen on the device)
constexpr int kMaxCand = 2 * kAngMaxSeeds;
__device__ __forceinline__ uint32_t mode_word(const uint32_t *s_pack, int m) {
  m = m < MIP_ANGULAR_FIRST ? MIP_ANGULAR_FIRST : m > MIP_ANGULAR_LAST ? MIP_ANGULAR_LAST : m;
  return s_pack[m - MIP_ANGULAR_FIRST];
}

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void angular_tap4_kernel(AngularTap4Args a) {
  __shared__ __attribute__((aligned(16))) uint16_t s_org[64 * 64];
  __shared__ __attribute__((aligned(16))) uint16_t s_ref[kExtRefCells];
  __shared__ WaveSums s_sum[kThreads / 64];
  __shared__ CuTable s_tab[3];
  __shared__ uint32_t s_coef[kAngCoefWords];
  const long long frame_samples = (long long)a.width * a.height;
  const long long items = (long long)a.nframes * a.nctus * kItemsPerCtu;
  const bool tables = a.cost || a.sad || a.satd;
  const int32_t none = MIP_COST_UNAVAILABLE;
  if (threadIdx.x < kAngCoefWords) s_coef[threadIdx.x] = a.coef[threadIdx.x];  // (the first item's barriers order it before its readers)
  const LdsCoef coef{s_coef};
  for (long long g = blockIdx.x; g < items; g += gridDim.x) {
    const int tid = opaque((int)threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const WindowItem it = window_item(g, a.nctus, a.ctu_cols, frame_samples, a.orig, a.refs);
    __syncthreads();  // (the previous item's last reads of the window and of s_tab)
    stage_window(it.F, it.R, a.width, frame_samples, it.x0, it.y0, it.lp, it.big, tid, s_org, s_ref);
    stage_extensions(it.R, a.width, frame_samples, it.x0, it.y0, it.lp, tid, s_ref);
    if (tid == 0) s_ref[kExtConstAt] = 512;
    reset_table(s_tab, it.big, tid);
    __syncthreads();
    const LdsRef ref{s_ref, it.x0, it.y0, it.lp};
    const size_t cu_base = (size_t)it.fc * MIP_CUS_PER_CTU;
    int org[16];
    if (it.big) {
      const int k = it.k;
      const IntraSlot c{k, tid & 15, tid >> 4, 0, 0, 6, 6};
      load_org(s_org, it.lp, c, org);
      const ExtLdsBound b(ref, it.x0, it.y0, 64, 64, ext_word(a.ext, (size_t)it.ctu * MIP_CUS_PER_CTU + k));
      const int corner = b.corner();
      for (int q = 0; q < a.nmodes; q++) {
        int v[2];
        ang_block_tap4_ext(b, b.e_top(), b.e_left(), ang_unpack(a.modes[q]), corner, 6, 6, 4 * c.bi, 4 * c.bj, org, coef, v[0], v[1]);
        group_sum(v, 64);
        if (lane == 0) s_sum[wave][q][0] = v[0], s_sum[wave][q][1] = v[1];
      }
      __syncthreads();
      const bool on = !a.unavail[(size_t)it.ctu * MIP_CUS_PER_CTU + k];
      if (tid < a.nmodes && on) finish_slot(s_sum, s_tab, tid, ang_unpack(a.modes[tid]).m - MIP_ANGULAR_FIRST);
      __syncthreads();
      const size_t cu = cu_base + k;
      flush_table(s_tab, tid, cu, a.cost, a.sad, a.satd);
      if (tid == 0) {
        uint8_t mode = 0xff;
        int32_t cost = none;
        for (int q = 0; q < a.nmodes; q++) {
          const int m = ang_unpack(a.modes[q]).m;
          ang_best_step(mode, cost, m, s_tab[0][m - MIP_ANGULAR_FIRST]);
        }
        write_best(a, cu, on, mode, cost);
      }
    } else {
      const uint32_t *slots = a.slots + (size_t)(it.k - 4) * a.slots_per_block;
      for (int at = 64 * wave; at < a.slots_per_block; at += kThreads) {
        const SlotCu s = slot_cu(slots[at + lane], a.unavail, it.ctu, cu_base);
        load_org(s_org, it.lp, s.c, org);
        const ExtLdsBound b(ref, it.x0 + 4 * s.c.cx, it.y0 + 4 * s.c.cy, 1 << s.c.lw, 1 << s.c.lh,
                            ext_word(a.ext, (size_t)it.ctu * MIP_CUS_PER_CTU + s.c.cu));
        const int corner = b.corner();
        if (tables && s.first) clear_unlisted(a.cost, a.sad, a.satd, s.cu, s.on, a.listed);
        uint8_t best_mode = 0xff;
        int32_t best_cost = none;
        for (int q = 0; q < a.nmodes; q += 2) {
          const bool two = q + 1 < a.nmodes;
          const AngMode m0 = ang_unpack(a.modes[q]), m1 = ang_unpack(a.modes[two ? q + 1 : q]);
          int v[4] = {0, 0, 0, 0};
          ang_block_tap4_ext(b, b.e_top(), b.e_left(), m0, corner, s.c.lw, s.c.lh, 4 * s.c.bi, 4 * s.c.bj, org, coef, v[0], v[1]);
          if (two) ang_block_tap4_ext(b, b.e_top(), b.e_left(), m1, corner, s.c.lw, s.c.lh, 4 * s.c.bi, 4 * s.c.bj, org, coef, v[2], v[3]);
          group_sum(v, s.n);
          if (s.on) {
            ang_best_step(best_mode, best_cost, m0.m, write_slot(a.cost, a.sad, a.satd, s.cu, m0.m, v[0], v[1]));
            if (two) ang_best_step(best_mode, best_cost, m1.m, write_slot(a.cost, a.sad, a.satd, s.cu, m1.m, v[2], v[3]));
          }
        }
        if (s.first) write_best(a, s.cu, s.on, best_mode, best_cost);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void angular_tap4_refine_kernel(AngularTap4Args a) {
  __shared__ __attribute__((aligned(16))) uint16_t s_org[64 * 64];
  __shared__ __attribute__((aligned(16))) uint16_t s_ref[kExtRefCells];
  __shared__ WaveSums s_sum[kThreads / 64];
  __shared__ CuTable s_tab[3];
  __shared__ uint32_t s_pack[kAngModes];
  __shared__ int s_cand[kMaxCand + 1];
  __shared__ uint32_t s_coef[kAngCoefWords];
  static_assert(kMaxCand <= kAngModes, "the candidates' sums fit s_sum");
  const long long frame_samples = (long long)a.width * a.height;
  const long long items = (long long)a.nframes * a.nctus * kItemsPerCtu;
  const bool tables = a.cost || a.sad || a.satd;
  const int32_t none = MIP_COST_UNAVAILABLE;
  const int rounds = 2 * a.nseeds;  // (uniform over the grid)
  if (threadIdx.x < kAngModes) s_pack[threadIdx.x] = a.all[threadIdx.x];  // (the first item's barriers order it before its readers)
  if (threadIdx.x < kAngCoefWords) s_coef[threadIdx.x] = a.coef[threadIdx.x];
  const LdsCoef coef{s_coef};
  for (long long g = blockIdx.x; g < items; g += gridDim.x) {
    const int tid = opaque((int)threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const WindowItem it = window_item(g, a.nctus, a.ctu_cols, frame_samples, a.orig, a.refs);
    __syncthreads();  // (the previous item's last reads of the window, of s_tab and of s_cand)
    stage_window(it.F, it.R, a.width, frame_samples, it.x0, it.y0, it.lp, it.big, tid, s_org, s_ref);
    stage_extensions(it.R, a.width, frame_samples, it.x0, it.y0, it.lp, tid, s_ref);
    if (tid == 0) s_ref[kExtConstAt] = 512;
    reset_table(s_tab, it.big, tid);
    __syncthreads();
    const LdsRef ref{s_ref, it.x0, it.y0, it.lp};
    const size_t cu_base = (size_t)it.fc * MIP_CUS_PER_CTU;
    int org[16];
    if (it.big) {
      const int k = it.k;
      const IntraSlot c{k, tid & 15, tid >> 4, 0, 0, 6, 6};
      load_org(s_org, it.lp, c, org);
      const ExtLdsBound b(ref, it.x0, it.y0, 64, 64, ext_word(a.ext, (size_t)it.ctu * MIP_CUS_PER_CTU + k));
      const int corner = b.corner();
      for (int q = 0; q < a.nmodes; q++) {
        int v[2];
        ang_block_tap4_ext(b, b.e_top(), b.e_left(), ang_unpack(a.modes[q]), corner, 6, 6, 4 * c.bi, 4 * c.bj, org, coef, v[0], v[1]);
        group_sum(v, 64);
        if (lane == 0) s_sum[wave][q][0] = v[0], s_sum[wave][q][1] = v[1];
      }
      __syncthreads();
      const bool on = !a.unavail[(size_t)it.ctu * MIP_CUS_PER_CTU + k];
      if (tid < a.nmodes && on) finish_slot(s_sum, s_tab, tid, ang_unpack(a.modes[tid]).m - MIP_ANGULAR_FIRST);
      __syncthreads();
      AngTop top = ang_top_none();
      if (tid == 0) {
        for (int q = 0; q < a.nmodes; q++) {
          const int m = ang_unpack(a.modes[q]).m;
          ang_top_step(top, m, s_tab[0][m - MIP_ANGULAR_FIRST]);
        }
        AngSet cand = ang_candidates(top, a.nseeds, a.listed);
        s_cand[kMaxCand] = ang_set_count(cand);
        for (int r = 0; r < rounds; r++) {
          const int m = ang_set_pop(cand);
          s_cand[r] = m ? m : top.m0;
        }
      }
      __syncthreads();
      const int ncand = s_cand[kMaxCand];
      for (int r = 0; r < rounds; r++) {  // (no barrier inside; the same modes in every lane)
        const uint32_t word = __builtin_amdgcn_readfirstlane(mode_word(s_pack, s_cand[r]));
        int v[2];
        ang_block_tap4_ext(b, b.e_top(), b.e_left(), ang_unpack(word), corner, 6, 6, 4 * c.bi, 4 * c.bj, org, coef, v[0], v[1]);
        group_sum(v, 64);
        if (lane == 0) s_sum[wave][r][0] = v[0], s_sum[wave][r][1] = v[1];
      }
      __syncthreads();
      if (tid < ncand && on) finish_slot(s_sum, s_tab, tid, (int)(mode_word(s_pack, s_cand[tid]) & 0xffu) - MIP_ANGULAR_FIRST);
      __syncthreads();
      const size_t cu = cu_base + k;
      flush_table(s_tab, tid, cu, a.cost, a.sad, a.satd);
      if (tid == 0) {
        uint8_t mode = 0xff;
        int32_t cost = none;
        if (on) {
          ang_best_step(mode, cost, top.m0, top.c0);
          for (int r = 0; r < ncand; r++) {
            const int m = (int)(mode_word(s_pack, s_cand[r]) & 0xffu);
            ang_best_step_any(mode, cost, m, s_tab[0][m - MIP_ANGULAR_FIRST]);
          }
        }
        write_best(a, cu, on, mode, cost);
        if (a.tried) a.tried[cu] = (uint8_t)(on ? a.nmodes + ncand : 0);
      }
    } else {
      const uint32_t *slots = a.slots + (size_t)(it.k - 4) * a.slots_per_block;
      for (int at = 64 * wave; at < a.slots_per_block; at += kThreads) {
        const SlotCu s = slot_cu(slots[at + lane], a.unavail, it.ctu, cu_base);
        const uint32_t cu = (uint32_t)cu_base + (uint32_t)s.c.cu;  // (one register: window_args_ok keeps the batch's CUs below 2^31)
        load_org(s_org, it.lp, s.c, org);
        const ExtLdsBound b(ref, it.x0 + 4 * s.c.cx, it.y0 + 4 * s.c.cy, 1 << s.c.lw, 1 << s.c.lh,
                            ext_word(a.ext, (size_t)it.ctu * MIP_CUS_PER_CTU + s.c.cu));
        const int corner = b.corner();
        if (tables && s.first) clear_unlisted(a.cost, a.sad, a.satd, cu, s.on, a.listed);  // (a candidate's slot is written again below)
        AngTop top = ang_top_none();  // (every lane of the group: the sums are the group's in each)
        for (int q = 0; q < a.nmodes; q += 2) {
          const bool two = q + 1 < a.nmodes;
          const AngMode m0 = ang_unpack(a.modes[q]), m1 = ang_unpack(a.modes[two ? q + 1 : q]);
          int v[4] = {0, 0, 0, 0};
          ang_block_tap4_ext(b, b.e_top(), b.e_left(), m0, corner, s.c.lw, s.c.lh, 4 * s.c.bi, 4 * s.c.bj, org, coef, v[0], v[1]);
          if (two) ang_block_tap4_ext(b, b.e_top(), b.e_left(), m1, corner, s.c.lw, s.c.lh, 4 * s.c.bi, 4 * s.c.bj, org, coef, v[2], v[3]);
          group_sum(v, s.n);
          ang_top_step(top, m0.m, intra_cost(v[0], v[1]));
          if (two) ang_top_step(top, m1.m, intra_cost(v[2], v[3]));
          if (s.on) {
            write_slot(a.cost, a.sad, a.satd, cu, m0.m, v[0], v[1]);
            if (two) write_slot(a.cost, a.sad, a.satd, cu, m1.m, v[2], v[3]);
          }
        }
        AngSet cand = ang_candidates(top, a.nseeds, a.listed);
        if (s.first && a.tried) a.tried[cu] = (uint8_t)(s.on ? a.nmodes + ang_set_count(cand) : 0);
        const int seed = top.m0;
        uint8_t best_mode = (uint8_t)MIP_MODE_ANGULAR(seed);
        int32_t best_cost = top.c0;
        for (int r = 0; r < rounds; r++) {  // wave-uniform; the mode is the group's own
          const int next = ang_set_pop(cand);
          const AngMode md = ang_unpack(mode_word(s_pack, next ? next : seed));
          int v[2] = {0, 0};
          ang_block_tap4_ext(b, b.e_top(), b.e_left(), md, corner, s.c.lw, s.c.lh, 4 * s.c.bi, 4 * s.c.bj, org, coef, v[0], v[1]);
          group_sum(v, s.n);
          if (next) ang_best_step_any(best_mode, best_cost, md.m, intra_cost(v[0], v[1]));
          if (s.on && next) write_slot(a.cost, a.sad, a.satd, cu, md.m, v[0], v[1]);
        }
        if (s.first) write_best(a, cu, s.on, s.on ? best_mode : (uint8_t)0xff, s.on ? best_cost : none);
      }
    }
  }
}

}  // namespace

hipError_t launch_angular_tap4(const AngularTap4Args &a, hipStream_t s) {
  if (!window_args_ok(a) || a.nmodes < 1 || a.nmodes > kAngModes || !a.ang_cost != !a.ang_mode ||
      (!a.cost && !a.sad && !a.satd && !a.best_cost && !a.ang_cost))
    return hipErrorInvalidValue;
  return launch_window_kernel(angular_tap4_kernel, a, s);
}

hipError_t launch_angular_tap4_refine(const AngularTap4Args &a, hipStream_t s) {
  if (!window_args_ok(a) || a.nmodes < 1 || a.nmodes > kAngModes || a.nseeds < 1 || a.nseeds > kAngMaxSeeds ||
      a.nseeds > a.nmodes || !a.ang_cost != !a.ang_mode ||
      (!a.cost && !a.sad && !a.satd && !a.best_cost && !a.ang_cost && !a.tried))
    return hipErrorInvalidValue;
  return launch_window_kernel(angular_tap4_refine_kernel, a, s);
}

}  // namespace mipgpu

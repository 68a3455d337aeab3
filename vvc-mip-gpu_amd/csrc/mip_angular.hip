// mip_angular.hip -- the six angular cost kernels (gfx950): directional intra costs of every CU,
// the best angular mode and its merge into the decisions, contracts in include/mipgpu.h
// (mip_angular_device, mip_angular_refine_device, mip_angular_refs, mip_angular_interp).  No
// reference counterpart.  The arithmetic is angular_plan.h's, shared with the host walk.
//
// One body (angular_items) holds the item loop; a kernel is that body with a policy for its
// reference lines and interpolation (PlainLines, ExtLines, Tap4Lines below) and a compile-time flag
// for the refinement pass:
//   angular_kernel         angular_refine_kernel        substituted lines, 2-tap
//   angular_ext_kernel *   angular_ext_refine_kernel    extended lines (a.ext), 2-tap
//   angular_tap4_kernel *  angular_tap4_refine_kernel   either (a.ext or NULL), 4-tap
// (* these two keep the same walk as a body of their own, behind the wrappers: as instances of
// the one body they were measured slower)
//
// Work items, window staging and lane slots are the intra kernel's (mip_window_dev.h).  The CU's
// corner sample is already in that window: row y0-1 of s_ref, or s_left, through the LdsRef index
// rule.  The steps are mip_angular_dev.h's.
//
// Coarse pass.  Per slot pass a lane loads its block's 16 originals once, finds where its CU's top
// and left lines lie in the window (the policy's Bound: a base and a stride each, so that a
// reference sample is one LDS read at an index computed from k alone) and then runs a wave-uniform
// loop over the mode list (kernel arguments: mode, angle and inverse angle are scalars), two modes
// per round: per mode the block's 16 residuals in registers -- five consecutive ref[] samples per
// line of the block (seven with four taps), the side projection only in the modes with a negative
// angle -- the in-lane Hadamard, and one xor-shuffle reduction of both modes' (sad, satd) pairs
// inside the group.  The group's first lane writes the table entries per mode.  Without refinement
// it keeps the running best and, after the loop, writes the ang pair and merges the decision.  The
// 64x64 CU's 256 lanes leave their waves' sums per mode in LDS and finish after one barrier.  Side
// projection and substitution are index arithmetic on slot-table and mode values: there, sample
// values are only ever values.  DESIGN.md section 5.7.
//
// Refinement pass (the refine flag).  After the xor butterfly every lane of a group holds the
// group's sums, so in the coarse pass every lane keeps the running top three (angular_plan.h
// ang_top_step) itself: no broadcast.
// 32x32 blocks: every lane forms its CU's candidate set (ang_candidates: the +-1 neighbours of the
// CU's seeds that the list does not hold) and a wave-uniform loop of 2 * nseeds rounds takes one
// candidate per round, lowest mode first -- each group its own mode.  Mode, angle and inverse are
// one per-lane read of a 65-word table staged in LDS once per workgroup; the class, angle-sign and
// pure-mode branches of the block step are divergent between the groups of a wave and reconverge
// before the group sum.  A group whose set has run out computes on its first seed and drops the
// result.
// 64x64 CU: after the coarse sums one lane forms seeds and candidates and leaves them in LDS; all
// 256 lanes run those modes uniformly (the mode made scalar), the waves' sums go through s_sum to
// the finish.  Every loop around a workgroup barrier has a trip count from the kernel arguments
// alone.  This is the one place in the family where sample values reach an address, through the
// chosen mode: see mode_word (mip_angular_dev.h).  DESIGN.md section 5.9.
//
// Extended lines (ExtLines, Tap4Lines): the staging of the two line extensions and the cut of a
// CU's lengths to the staged extent are mip_angular_dev.h's stage_extensions and ExtLdsBound;
// everything else of a mode's arithmetic is ang_block_class as before.  DESIGN.md section 5.11.
//
// Four taps (Tap4Lines).  One kernel per role serves both mip_angular_refs settings: without a
// length table (a.ext == NULL, the substituted lines) every CU's lengths are 0 / 0, which is the
// substituted predictor bit for bit.
// The line.  A mode's line of a lane's 4x4 block takes the seven ref[a0+idx .. a0+idx+6] instead of
// five and four multiplies per sample instead of two (angular_plan.h ang_block_tap4_class).
// No new staging: every tap index is clamped onto the lines that are staged already.
//   k+2 at M'.  A tap k >= 1 reads main[min(k, M') - 1], the very clamp of the 2-tap predictor: k + 2
//     past M' reads the cell of main[M' - 1] that k and k + 1 read there, and M' is the length
//     ExtLdsBound has cut to the staged extent of the line.
//   k-1 at the side's cap.  A tap k <= 0 reads side'[min((-k*inv + 256) >> 9, S)]: one step further
//     along the side than the 2-tap predictor's lowest tap, but capped at S like it, so it reads
//     side[S - 1] at most -- a cell of the CU's own side line.
//   k-1 = 0 for A >= 0.  The corner, which the lane holds in a register (ExtLdsBound::ce): no read.
// Coefficients.  The filter G depends on the lane's CU shape and the wave-uniform mode, the
// fraction f on the lane's row, so the index is divergent.  The 64 coefficient quadruples (G << 5 | f,
// angular_plan.h ang_coef_word: four signed bytes in one word) are staged in LDS once per workgroup
// from the kernel arguments; a lane fetches one word per line of its block (one ds_read_b32, 64
// consecutive words: at most a two-way bank conflict) and unpacks it with four sign-extending
// bit-field extracts -- no select between the tables, no table in constant memory, whose divergent
// index would serialise into one load per distinct address.  The products are 32-bit: references
// are uint16 and an engine filter's can exceed 15 bits, so packed signed 16-bit dot products would
// misread them.  DESIGN.md section 5.12.
//
// No atomics, no scratch in any of the six.
#include "mip_angular_dev.h"

namespace mipgpu {
namespace {

// ---- what differs between the variants: the layout of s_ref, the staging behind stage_window, the
// Bound of a CU and how it is made, the block step, and whether the coefficient words are staged.
struct PlainLines {
  static constexpr int kCells = kRefCells, kConst = kConstAt;
  static constexpr bool kCoef = false;
  using Bound = LdsBound;
  __device__ static __forceinline__ void stage(const WindowItem &, int, long long, int, uint16_t *) {}
  __device__ static __forceinline__ Bound bound(const AngularArgs &, const LdsRef &win, int x, int y, int w, int h, size_t) {
    return Bound(win, x, y, w, h);
  }
  __device__ static __forceinline__ void block(const Bound &b, const AngMode &md, int corner, const IntraSlot &c, const int *org,
                                               const uint32_t *, int &sad, int &satd) {
    ang_block(b, md, corner, c.lw, c.lh, 4 * c.bi, 4 * c.bj, org, sad, satd);
  }
};
struct ExtLines {
  static constexpr int kCells = kExtRefCells, kConst = kExtConstAt;
  static constexpr bool kCoef = false;
  using Bound = ExtLdsBound;
  __device__ static __forceinline__ void stage(const WindowItem &it, int width, long long frame_samples, int tid, uint16_t *s_ref) {
    stage_extensions(it.R, width, frame_samples, it.x0, it.y0, it.lp, tid, s_ref);
  }
  __device__ static __forceinline__ Bound bound(const AngularExtArgs &a, const LdsRef &win, int x, int y, int w, int h, size_t cu) {
    return Bound(win, x, y, w, h, a.ext[cu]);  // (the launchers require the table)
  }
  __device__ static __forceinline__ void block(const Bound &b, const AngMode &md, int corner, const IntraSlot &c, const int *org,
                                               const uint32_t *, int &sad, int &satd) {
    ang_block_ext(b, b.e_top(), b.e_left(), md, corner, c.lw, c.lh, 4 * c.bi, 4 * c.bj, org, sad, satd);
  }
};
struct Tap4Lines : ExtLines {
  static constexpr bool kCoef = true;
  __device__ static __forceinline__ Bound bound(const AngularTap4Args &a, const LdsRef &win, int x, int y, int w, int h, size_t cu) {
    return Bound(win, x, y, w, h, ext_word(a.ext, cu));
  }
  __device__ static __forceinline__ void block(const Bound &b, const AngMode &md, int corner, const IntraSlot &c, const int *org,
                                               const uint32_t *coef, int &sad, int &satd) {
    ang_block_tap4_ext(b, b.e_top(), b.e_left(), md, corner, c.lw, c.lh, 4 * c.bi, 4 * c.bj, org, LdsCoef{coef}, sad, satd);
  }
};

// The body of the kernels: four are its instances, two keep the same walk written out (below).
// The argument struct comes by const reference (mip_angular_dev.h says why).  An instantiation that does not name an LDS array does not have it: s_pack and s_cand are
// the refinement's, s_coef the four taps'.
template <class Lines, bool kRefine, class Args>
__device__ __forceinline__ void angular_items(const Args &a) {
  __shared__ __attribute__((aligned(16))) uint16_t s_org[64 * 64];
  __shared__ __attribute__((aligned(16))) uint16_t s_ref[Lines::kCells];
  __shared__ WaveSums s_sum[kThreads / 64];  // 64x64 CU: the waves' (sad, satd) per list entry, then per candidate
  __shared__ CuTable s_tab[3];               // 64x64 CU: cost, sad, satd per table slot
  __shared__ uint32_t s_pack[kAngModes];     // ang_pack of every mode, slot = mode - 2
  __shared__ int s_cand[kMaxCand + 1];       // 64x64 CU: the modes of the refinement rounds, then their count
  __shared__ uint32_t s_coef[kAngCoefWords];
  static_assert(kMaxCand <= kAngModes, "the candidates' sums fit s_sum");
  const long long frame_samples = (long long)a.width * a.height;
  const long long items = (long long)a.nframes * a.nctus * kItemsPerCtu;
  const bool tables = a.cost || a.sad || a.satd;
  const int32_t none = MIP_COST_UNAVAILABLE;
  int rounds = 0;
  const uint32_t *coef = nullptr;
  if constexpr (kRefine) {
    rounds = 2 * a.nseeds;  // (uniform over the grid)
    if (threadIdx.x < kAngModes) s_pack[threadIdx.x] = a.all[threadIdx.x];  // (the first item's barriers order it before its readers)
  }
  if constexpr (Lines::kCoef) {
    if (threadIdx.x < kAngCoefWords) s_coef[threadIdx.x] = a.coef[threadIdx.x];  // (likewise)
    coef = s_coef;
  }
  for (long long g = blockIdx.x; g < items; g += gridDim.x) {
    const int tid = opaque((int)threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const WindowItem it = window_item(g, a.nctus, a.ctu_cols, frame_samples, a.orig, a.refs);
    __syncthreads();  // (the previous item's last reads of the window, of s_tab and of s_cand)
    stage_window(it.F, it.R, a.width, frame_samples, it.x0, it.y0, it.lp, it.big, tid, s_org, s_ref);
    Lines::stage(it, a.width, frame_samples, tid, s_ref);
    if (tid == 0) s_ref[Lines::kConst] = 512;
    reset_table(s_tab, it.big, tid);
    __syncthreads();
    const LdsRef ref{s_ref, it.x0, it.y0, it.lp};
    const size_t cu_base = (size_t)it.fc * MIP_CUS_PER_CTU, ctu_base = (size_t)it.ctu * MIP_CUS_PER_CTU;
    int org[16];
    if (it.big) {  // 256 lanes, one CU: wave sums per mode, then the four waves' through LDS
      const int k = it.k;
      const IntraSlot c{k, tid & 15, tid >> 4, 0, 0, 6, 6};
      load_org(s_org, it.lp, c, org);
      const typename Lines::Bound b = Lines::bound(a, ref, it.x0, it.y0, 64, 64, ctu_base + k);
      const int corner = b.corner();
      for (int q = 0; q < a.nmodes; q++) {
        int v[2];
        Lines::block(b, ang_unpack(a.modes[q]), corner, c, org, coef, v[0], v[1]);
        group_sum(v, 64);
        if (lane == 0) s_sum[wave][q][0] = v[0], s_sum[wave][q][1] = v[1];
      }
      __syncthreads();
      const bool on = !a.unavail[ctu_base + k];
      if (tid < a.nmodes && on) finish_slot(s_sum, s_tab, tid, ang_unpack(a.modes[tid]).m - MIP_ANGULAR_FIRST);
      __syncthreads();
      const size_t cu = cu_base + k;
      if constexpr (!kRefine) {
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
        // one lane: the seeds and the candidates of the CU (none if it is unavailable: every cost is
        // then MIP_COST_UNAVAILABLE and the top list stays empty); rounds past the set's end get
        // the first seed as a valid substitute
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
          Lines::block(b, ang_unpack(word), corner, c, org, coef, v[0], v[1]);
          group_sum(v, 64);
          if (lane == 0) s_sum[wave][r][0] = v[0], s_sum[wave][r][1] = v[1];
        }
        __syncthreads();
        if (tid < ncand && on) finish_slot(s_sum, s_tab, tid, (int)(mode_word(s_pack, s_cand[tid]) & 0xffu) - MIP_ANGULAR_FIRST);
        __syncthreads();
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
      }
    } else {
      const uint32_t *slots = a.slots + (size_t)(it.k - 4) * a.slots_per_block;
      for (int at = 64 * wave; at < a.slots_per_block; at += kThreads) {
        const SlotCu s = slot_cu(slots[at + lane], a.unavail, it.ctu, cu_base);
        const uint32_t cu = (uint32_t)cu_base + (uint32_t)s.c.cu;  // (one register: window_args_ok keeps the batch's CUs below 2^31)
        load_org(s_org, it.lp, s.c, org);
        const typename Lines::Bound b =
            Lines::bound(a, ref, it.x0 + 4 * s.c.cx, it.y0 + 4 * s.c.cy, 1 << s.c.lw, 1 << s.c.lh, ctu_base + s.c.cu);
        const int corner = b.corner();
        if (tables && s.first) clear_unlisted(a.cost, a.sad, a.satd, cu, s.on, a.listed);  // (a candidate's slot is written again below)
        uint8_t best_mode = 0xff;
        int32_t best_cost = none;
        AngTop top = ang_top_none();  // (refinement, every lane of the group: the sums are the group's in each)
        for (int q = 0; q < a.nmodes; q += 2) {
          const bool two = q + 1 < a.nmodes;
          const AngMode m0 = ang_unpack(a.modes[q]), m1 = ang_unpack(a.modes[two ? q + 1 : q]);
          int v[4] = {0, 0, 0, 0};
          Lines::block(b, m0, corner, s.c, org, coef, v[0], v[1]);
          if (two) Lines::block(b, m1, corner, s.c, org, coef, v[2], v[3]);
          group_sum(v, s.n);
          if constexpr (kRefine) {
            ang_top_step(top, m0.m, intra_cost(v[0], v[1]));
            if (two) ang_top_step(top, m1.m, intra_cost(v[2], v[3]));
          }
          if (s.on) {
            const int32_t c0 = write_slot(a.cost, a.sad, a.satd, cu, m0.m, v[0], v[1]);
            if constexpr (!kRefine) ang_best_step(best_mode, best_cost, m0.m, c0);
            if (two) {
              const int32_t c1 = write_slot(a.cost, a.sad, a.satd, cu, m1.m, v[2], v[3]);
              if constexpr (!kRefine) ang_best_step(best_mode, best_cost, m1.m, c1);
            }
          }
        }
        if constexpr (kRefine) {
          // the best of the list is the top list's first entry; the other entries end in the set
          AngSet cand = ang_candidates(top, a.nseeds, a.listed);
          if (s.first && a.tried) a.tried[cu] = (uint8_t)(s.on ? a.nmodes + ang_set_count(cand) : 0);
          const int seed = top.m0;
          best_mode = (uint8_t)MIP_MODE_ANGULAR(seed);
          best_cost = top.c0;
          for (int r = 0; r < rounds; r++) {  // wave-uniform; the mode is the group's own
            const int next = ang_set_pop(cand);
            const AngMode md = ang_unpack(mode_word(s_pack, next ? next : seed));
            int v[2] = {0, 0};
            Lines::block(b, md, corner, s.c, org, coef, v[0], v[1]);
            group_sum(v, s.n);
            if (next) ang_best_step_any(best_mode, best_cost, md.m, intra_cost(v[0], v[1]));
            if (s.on && next) write_slot(a.cost, a.sad, a.satd, cu, md.m, v[0], v[1]);
          }
          if (!s.on) best_mode = 0xff, best_cost = none;
        }
        if (s.first) write_best(a, cu, s.on, best_mode, best_cost);
      }
    }
  }
}

#define MIP_THREE_WAVES __attribute__((amdgpu_waves_per_eu(3, 3)))
__global__ __launch_bounds__(kThreads) void angular_kernel(AngularArgs a) { angular_items<PlainLines, false>(a); }
__global__ __launch_bounds__(kThreads) MIP_THREE_WAVES void angular_refine_kernel(AngularRefineArgs a) { angular_items<PlainLines, true>(a); }
__global__ __launch_bounds__(kThreads) MIP_THREE_WAVES void angular_ext_refine_kernel(AngularExtArgs a) { angular_items<ExtLines, true>(a); }
__global__ __launch_bounds__(kThreads) MIP_THREE_WAVES void angular_tap4_refine_kernel(AngularTap4Args a) { angular_items<Tap4Lines, true>(a); }
#undef MIP_THREE_WAVES

// Two kernels keep a body of their own: as instances of angular_items (ExtLines / Tap4Lines without
// the refinement) they were measured 3.3 to 3.6 % and 2.2 to 2.8 % slower than this text, which is
// the one body's list path with the policy written out -- also with every value formed as here, and
// also with tid formed outside the item loop ("One body, six kernels").  Any
// change to angular_items' coarse pass belongs here too.
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void angular_ext_kernel(AngularExtArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t s_org[64 * 64];
  __shared__ __attribute__((aligned(16))) uint16_t s_ref[kExtRefCells];
  __shared__ WaveSums s_sum[kThreads / 64];
  __shared__ CuTable s_tab[3];
  const long long frame_samples = (long long)a.width * a.height;
  const long long items = (long long)a.nframes * a.nctus * kItemsPerCtu;
  const bool tables = a.cost || a.sad || a.satd;
  const int32_t none = MIP_COST_UNAVAILABLE;
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
      const ExtLdsBound b(ref, it.x0, it.y0, 64, 64, a.ext[(size_t)it.ctu * MIP_CUS_PER_CTU + k]);
      const int corner = b.corner();
      for (int q = 0; q < a.nmodes; q++) {
        int v[2];
        ang_block_ext(b, b.e_top(), b.e_left(), ang_unpack(a.modes[q]), corner, 6, 6, 4 * c.bi, 4 * c.bj, org, v[0], v[1]);
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
                            a.ext[(size_t)it.ctu * MIP_CUS_PER_CTU + s.c.cu]);
        const int corner = b.corner();
        if (tables && s.first) clear_unlisted(a.cost, a.sad, a.satd, s.cu, s.on, a.listed);
        uint8_t best_mode = 0xff;
        int32_t best_cost = none;
        for (int q = 0; q < a.nmodes; q += 2) {
          const bool two = q + 1 < a.nmodes;
          const AngMode m0 = ang_unpack(a.modes[q]), m1 = ang_unpack(a.modes[two ? q + 1 : q]);
          int v[4] = {0, 0, 0, 0};
          ang_block_ext(b, b.e_top(), b.e_left(), m0, corner, s.c.lw, s.c.lh, 4 * s.c.bi, 4 * s.c.bj, org, v[0], v[1]);
          if (two) ang_block_ext(b, b.e_top(), b.e_left(), m1, corner, s.c.lw, s.c.lh, 4 * s.c.bi, 4 * s.c.bj, org, v[2], v[3]);
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

// The launchers' rules behind window_args_ok: the mode list, the ang pair, at least one output;
// with `seeds` (the refining launches) the seed count, and `tried` counts as an output.  ext_ok:
// the length table is there where the kernel needs it.
bool angular_args_ok(const AngularArgs &a, const AngularRefineArgs *seeds, bool ext_ok) {
  if (a.nmodes < 1 || a.nmodes > kAngModes || !a.ang_cost != !a.ang_mode || !ext_ok) return false;
  if (seeds && (seeds->nseeds < 1 || seeds->nseeds > kAngMaxSeeds || seeds->nseeds > a.nmodes)) return false;
  return a.cost || a.sad || a.satd || a.best_cost || a.ang_cost || (seeds && seeds->tried);
}

}  // namespace

hipError_t launch_angular(const AngularArgs &a, hipStream_t s) {
  if (!window_args_ok(a) || !angular_args_ok(a, nullptr, true)) return hipErrorInvalidValue;
  return launch_window_kernel(angular_kernel, a, s);
}

hipError_t launch_angular_refine(const AngularRefineArgs &a, hipStream_t s) {
  if (!window_args_ok(a) || !angular_args_ok(a, &a, true)) return hipErrorInvalidValue;
  return launch_window_kernel(angular_refine_kernel, a, s);
}

hipError_t launch_angular_ext(const AngularExtArgs &a, hipStream_t s) {
  if (!window_args_ok(a) || !angular_args_ok(a, nullptr, a.ext != nullptr)) return hipErrorInvalidValue;
  return launch_window_kernel(angular_ext_kernel, a, s);
}

hipError_t launch_angular_ext_refine(const AngularExtArgs &a, hipStream_t s) {
  if (!window_args_ok(a) || !angular_args_ok(a, &a, a.ext != nullptr)) return hipErrorInvalidValue;
  return launch_window_kernel(angular_ext_refine_kernel, a, s);
}

hipError_t launch_angular_tap4(const AngularTap4Args &a, hipStream_t s) {  // (no table: the substituted lines)
  if (!window_args_ok(a) || !angular_args_ok(a, nullptr, true)) return hipErrorInvalidValue;
  return launch_window_kernel(angular_tap4_kernel, a, s);
}

hipError_t launch_angular_tap4_refine(const AngularTap4Args &a, hipStream_t s) {
  if (!window_args_ok(a) || !angular_args_ok(a, &a, true)) return hipErrorInvalidValue;
  return launch_window_kernel(angular_tap4_refine_kernel, a, s);
}

}  // namespace mipgpu

// mip_angular_refine.hip -- coarse-to-fine angular mode search in one launch (gfx950), contract in
// include/mipgpu.h (mip_angular_refine_device).  No reference counterpart.  A second kernel beside
// angular_kernel (mip_angular.hip), which stays as it is: the same items, window staging, lane
// slots and grid cap (mip_window_dev.h) and the same steps of the two paths (mip_angular_dev.h), so
// one staging of a window serves both passes.
//
// Coarse pass: angular_kernel's loop over the caller's list (scalar modes from the kernel
// arguments, two per round).  After the xor butterfly every lane of a group holds the group's
// sums, so every lane keeps the running top three (angular_plan.h ang_top_step) itself: no
// broadcast.
// Refinement pass, 32x32 blocks: every lane forms its CU's candidate set (ang_candidates: the
// +-1 neighbours of the CU's seeds that the list does not hold) and a wave-uniform loop of
// 2 * nseeds rounds takes one candidate per round, lowest mode first -- each group its own mode.
// Mode, angle and inverse are one per-lane read of a 65-word table staged in LDS once per
// workgroup; the class, angle-sign and pure-mode branches of ang_block are divergent between the
// groups of a wave and reconverge before the group sum.  A group whose set has run out computes
// on its first seed and drops the result.
// Refinement pass, 64x64 CU: after the coarse sums one lane forms seeds and candidates and leaves
// them in LDS; all 256 lanes run those modes uniformly (the mode made scalar), the waves' sums go
// through s_sum to the finish.  Every loop around a workgroup barrier has a trip count from the
// kernel arguments alone.
// This is the one place in the kernel family where sample values reach an address, through the
// chosen mode: see mode_word below.  No atomics, no scratch.  DESIGN.md section 5.9.
#include "mip_angular_dev.h"

namespace mipgpu {
namespace {

constexpr int kMaxCand = 2 * kAngMaxSeeds;

// The packed (mode, angle, inverse) word of a mode chosen on the device.  The mode is clamped
// into 2..66 before the lookup, so the table index is 0..64 whatever the sample values made of the
// costs; the word is then one of the host's ang_pack values, whose angle and inverse belong to
// its mode.  With any such word LdsBound's reads stay inside the staged window: ang_ref and
// ang_ref_main clamp the line position t into 0 .. M-1 (or S-1) before base + t * stride, for
// every k, and base and stride come from the slot alone.
__device__ __forceinline__ uint32_t mode_word(const uint32_t *s_pack, int m) {
  m = m < MIP_ANGULAR_FIRST ? MIP_ANGULAR_FIRST : m > MIP_ANGULAR_LAST ? MIP_ANGULAR_LAST : m;
  return s_pack[m - MIP_ANGULAR_FIRST];
}

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3, 3))) void angular_refine_kernel(AngularRefineArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t s_org[64 * 64];
  __shared__ __attribute__((aligned(16))) uint16_t s_ref[kRefCells];
  __shared__ WaveSums s_sum[kThreads / 64];           // 64x64 CU: the waves' (sad, satd) per list entry, then per candidate
  __shared__ CuTable s_tab[3];                        // 64x64 CU: cost, sad, satd per table slot
  __shared__ uint32_t s_pack[kAngModes];              // ang_pack of every mode, slot = mode - 2
  __shared__ int s_cand[kMaxCand + 1];                // 64x64 CU: the modes of the refinement rounds, then their count
  static_assert(kMaxCand <= kAngModes, "the candidates' sums fit s_sum");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long frame_samples = (long long)a.width * a.height;
  const long long items = (long long)a.nframes * a.nctus * kItemsPerCtu;
  const bool tables = a.cost || a.sad || a.satd;
  const int32_t none = MIP_COST_UNAVAILABLE;
  const int rounds = 2 * a.nseeds;  // (uniform over the grid)
  if (tid < kAngModes) s_pack[tid] = a.all[tid];  // (the first item's barriers order it before its readers)
  for (long long g = blockIdx.x; g < items; g += gridDim.x) {
    const WindowItem it = window_item(g, a.nctus, a.ctu_cols, frame_samples, a.orig, a.refs);
    __syncthreads();  // (the previous item's last reads of the window, of s_tab and of s_cand)
    stage_window(it.F, it.R, a.width, frame_samples, it.x0, it.y0, it.lp, it.big, tid, s_org, s_ref);
    if (tid == 0) s_ref[kConstAt] = 512;
    reset_table(s_tab, it.big, tid);
    __syncthreads();
    const LdsRef ref{s_ref, it.x0, it.y0, it.lp};
    const size_t cu_base = (size_t)it.fc * MIP_CUS_PER_CTU;
    int org[16];
    if (it.big) {  // 256 lanes, one CU: wave sums per mode, then the four waves' through LDS
      const int k = it.k;
      const IntraSlot c{k, tid & 15, tid >> 4, 0, 0, 6, 6};
      load_org(s_org, it.lp, c, org);
      const LdsBound b(ref, it.x0, it.y0, 64, 64);
      const int corner = b.corner();
      for (int q = 0; q < a.nmodes; q++) {
        int v[2];
        ang_block(b, ang_unpack(a.modes[q]), corner, 6, 6, 4 * c.bi, 4 * c.bj, org, v[0], v[1]);
        group_sum(v, 64);
        if (lane == 0) s_sum[wave][q][0] = v[0], s_sum[wave][q][1] = v[1];
      }
      __syncthreads();
      const bool on = !a.unavail[(size_t)it.ctu * MIP_CUS_PER_CTU + k];
      // (t is tid, opaque per item: the per-lane addresses of this path -- a.modes[t], the tables'
      // a.cost + t -- are otherwise hoisted out of the item loop into registers held across the
      // 32x32 path, which at three waves per SIMD has none to spare)
      int t = tid;
      asm volatile("" : "+v"(t));
      if (t < a.nmodes && on) finish_slot(s_sum, s_tab, t, ang_unpack(a.modes[t]).m - MIP_ANGULAR_FIRST);
      __syncthreads();
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
        ang_block(b, ang_unpack(word), corner, 6, 6, 4 * c.bi, 4 * c.bj, org, v[0], v[1]);
        group_sum(v, 64);
        if (lane == 0) s_sum[wave][r][0] = v[0], s_sum[wave][r][1] = v[1];
      }
      __syncthreads();
      if (tid < ncand && on) finish_slot(s_sum, s_tab, tid, (int)(mode_word(s_pack, s_cand[tid]) & 0xffu) - MIP_ANGULAR_FIRST);
      __syncthreads();
      const size_t cu = cu_base + k;
      flush_table(s_tab, t, cu, a.cost, a.sad, a.satd);
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
        load_org(s_org, it.lp, s.c, org);
        const LdsBound b(ref, it.x0 + 4 * s.c.cx, it.y0 + 4 * s.c.cy, 1 << s.c.lw, 1 << s.c.lh);
        const int corner = b.corner();
        if (tables && s.first) clear_unlisted(a.cost, a.sad, a.satd, s.cu, s.on, a.listed);  // (a candidate's slot is written again below)
        AngTop top = ang_top_none();  // (every lane of the group: the sums are the group's in each)
        for (int q = 0; q < a.nmodes; q += 2) {
          const bool two = q + 1 < a.nmodes;
          const AngMode m0 = ang_unpack(a.modes[q]), m1 = ang_unpack(a.modes[two ? q + 1 : q]);
          int v[4] = {0, 0, 0, 0};
          ang_block(b, m0, corner, s.c.lw, s.c.lh, 4 * s.c.bi, 4 * s.c.bj, org, v[0], v[1]);
          if (two) ang_block(b, m1, corner, s.c.lw, s.c.lh, 4 * s.c.bi, 4 * s.c.bj, org, v[2], v[3]);
          group_sum(v, s.n);
          ang_top_step(top, m0.m, intra_cost(v[0], v[1]));
          if (two) ang_top_step(top, m1.m, intra_cost(v[2], v[3]));
          if (s.on) {
            write_slot(a.cost, a.sad, a.satd, s.cu, m0.m, v[0], v[1]);
            if (two) write_slot(a.cost, a.sad, a.satd, s.cu, m1.m, v[2], v[3]);
          }
        }
        // the best of the list is the top list's first entry; the other entries end in the set
        AngSet cand = ang_candidates(top, a.nseeds, a.listed);
        if (s.first && a.tried) a.tried[s.cu] = (uint8_t)(s.on ? a.nmodes + ang_set_count(cand) : 0);
        const int seed = top.m0;
        uint8_t best_mode = (uint8_t)MIP_MODE_ANGULAR(seed);
        int32_t best_cost = top.c0;
        for (int r = 0; r < rounds; r++) {  // wave-uniform; the mode is the group's own
          const int next = ang_set_pop(cand);
          const AngMode md = ang_unpack(mode_word(s_pack, next ? next : seed));
          int v[2] = {0, 0};
          ang_block(b, md, corner, s.c.lw, s.c.lh, 4 * s.c.bi, 4 * s.c.bj, org, v[0], v[1]);
          group_sum(v, s.n);
          if (next) ang_best_step_any(best_mode, best_cost, md.m, intra_cost(v[0], v[1]));
          if (s.on && next) write_slot(a.cost, a.sad, a.satd, s.cu, md.m, v[0], v[1]);
        }
        if (s.first) write_best(a, s.cu, s.on, s.on ? best_mode : (uint8_t)0xff, s.on ? best_cost : none);
      }
    }
  }
}

}  // namespace

hipError_t launch_angular_refine(const AngularRefineArgs &a, hipStream_t s) {
  if (!window_args_ok(a) || a.nmodes < 1 || a.nmodes > kAngModes || a.nseeds < 1 || a.nseeds > kAngMaxSeeds || a.nseeds > a.nmodes ||
      !a.ang_cost != !a.ang_mode || (!a.cost && !a.sad && !a.satd && !a.best_cost && !a.ang_cost && !a.tried))
    return hipErrorInvalidValue;
  return launch_window_kernel(angular_refine_kernel, a, s);
}

}  // namespace mipgpu

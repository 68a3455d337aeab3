// mip_angular.hip -- directional (angular) intra costs of every CU, the best angular mode and
// its merge into the decisions (gfx950), contract in include/mipgpu.h (mip_angular_device).  No
// reference counterpart.  The arithmetic is angular_plan.h's, shared with the host walk.
//
// Work items, window staging and lane slots are the intra kernel's (mip_window_dev.h).  The CU's
// corner sample is already in that window: row y0-1 of s_ref, or s_left, through the LdsRef index
// rule.  The steps below are mip_angular_dev.h's, shared with angular_refine_kernel.
//
// Per slot pass a lane loads its block's 16 originals once, finds where its CU's top and left
// lines lie in the window (LdsBound: a base and a stride each, so that a reference sample is one
// LDS read at an index computed from k alone) and then runs a wave-uniform loop over the mode
// list (kernel arguments: mode, angle and inverse angle are scalars), two modes per round: per
// mode the block's 16 residuals in registers -- five consecutive ref[] samples per line of the
// block, 20 LDS reads, the side projection only in the modes with a negative angle -- the in-lane
// Hadamard, and one xor-shuffle reduction of both modes' (sad, satd) pairs inside the group.  The
// group's first lane writes the table entries per mode, keeps the running best and, after the
// loop, writes the ang pair and merges the decision.
// The 64x64 CU's 256 lanes leave their waves' sums per mode in LDS and finish after one barrier.
// Side projection and substitution are index arithmetic on slot-table and mode values: sample
// values are only ever values.  No atomics.  DESIGN.md section 5.7.
#include "mip_angular_dev.h"

namespace mipgpu {
namespace {

__global__ __launch_bounds__(kThreads) void angular_kernel(AngularArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t s_org[64 * 64];
  __shared__ __attribute__((aligned(16))) uint16_t s_ref[kRefCells];
  __shared__ WaveSums s_sum[kThreads / 64];  // 64x64 CU: the waves' (sad, satd) per list entry
  __shared__ CuTable s_tab[3];               // 64x64 CU: cost, sad, satd per table slot
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long frame_samples = (long long)a.width * a.height;
  const long long items = (long long)a.nframes * a.nctus * kItemsPerCtu;
  const bool tables = a.cost || a.sad || a.satd;
  const int32_t none = MIP_COST_UNAVAILABLE;
  for (long long g = blockIdx.x; g < items; g += gridDim.x) {
    const WindowItem it = window_item(g, a.nctus, a.ctu_cols, frame_samples, a.orig, a.refs);
    __syncthreads();  // (the previous item's last reads of the window and of s_tab)
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
        const LdsBound b(ref, it.x0 + 4 * s.c.cx, it.y0 + 4 * s.c.cy, 1 << s.c.lw, 1 << s.c.lh);
        const int corner = b.corner();
        if (tables && s.first) clear_unlisted(a.cost, a.sad, a.satd, s.cu, s.on, a.listed);
        uint8_t best_mode = 0xff;
        int32_t best_cost = none;
        for (int q = 0; q < a.nmodes; q += 2) {
          const bool two = q + 1 < a.nmodes;
          const AngMode m0 = ang_unpack(a.modes[q]), m1 = ang_unpack(a.modes[two ? q + 1 : q]);
          int v[4] = {0, 0, 0, 0};
          ang_block(b, m0, corner, s.c.lw, s.c.lh, 4 * s.c.bi, 4 * s.c.bj, org, v[0], v[1]);
          if (two) ang_block(b, m1, corner, s.c.lw, s.c.lh, 4 * s.c.bi, 4 * s.c.bj, org, v[2], v[3]);
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

}  // namespace

hipError_t launch_angular(const AngularArgs &a, hipStream_t s) {
  if (!window_args_ok(a) || a.nmodes < 1 || a.nmodes > kAngModes || !a.ang_cost != !a.ang_mode ||
      (!a.cost && !a.sad && !a.satd && !a.best_cost && !a.ang_cost))
    return hipErrorInvalidValue;
  return launch_window_kernel(angular_kernel, a, s);
}

}  // namespace mipgpu

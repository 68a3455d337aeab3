// mip_angular.hip -- directional (angular) intra costs of every CU, the best angular mode and
// its merge into the decisions (gfx950), contract in include/mipgpu.h (mip_angular_device).  No
// reference counterpart.  The arithmetic is angular_plan.h's, shared with the host walk.
//
// Work items, window staging and lane slots are the intra kernel's (mip_intra.hip): items
// (frame, CTU, k), k < 4 the 64x64 CU of quadrant k, else the 32x32 block k - 4; a workgroup
// (4 waves) takes items blockIdx.x, + gridDim.x, ...; per item it stages the window's originals
// and reference samples once by linear index with the guard idx < W*H (2-byte loads), as uint16
// in LDS (s_org, s_ref with s_left behind it), and walks the block's lane slots: one lane per 4x4
// block of a CU, a CU's lanes an aligned power-of-two group of one wave.  The CU's corner sample
// is already in that window: row y0-1 of s_ref, or s_left, through the LdsRef index rule.
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

constexpr int kItemsPerCtu = 4 + kIntraBlocks;

__global__ __launch_bounds__(kThreads) void angular_kernel(AngularArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t s_org[64 * 64];
  __shared__ __attribute__((aligned(16))) uint16_t s_ref[kLeftAt + 65 + 7];
  static_assert(kConstAt > kLeftAt + 64 && kConstAt < kLeftAt + 65 + 7, "the constant's cell lies behind s_left");
  uint16_t *const s_left = s_ref + kLeftAt;
  __shared__ int s_sum[kThreads / 64][kAngModes][2];  // 64x64 CU: the waves' (sad, satd) per list entry
  __shared__ int s_tab[3][kAngModes];                 // 64x64 CU: cost, sad, satd per table slot
  static_assert(kRefRows64 * 64 <= kRefRows32 * 32, "the 64x64 CU's reference rows fit");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long frame_samples = (long long)a.width * a.height;
  const long long items = (long long)a.nframes * a.nctus * kItemsPerCtu;
  const bool tables = a.cost || a.sad || a.satd;
  const int32_t none = MIP_COST_UNAVAILABLE;
  for (long long g = blockIdx.x; g < items; g += gridDim.x) {
    const long long fc = g / kItemsPerCtu;  // frame * nctus + ctu
    const int k = (int)(g - fc * kItemsPerCtu), frame = (int)(fc / a.nctus), ctu = (int)(fc - (long long)frame * a.nctus);
    const bool big = k < 4;
    const int lp = big ? 6 : 5, side = 1 << lp;
    const int x0 = 128 * (ctu % a.ctu_cols) + (big ? 64 * (k & 1) : 32 * ((k - 4) & 3));
    const int y0 = 128 * (ctu / a.ctu_cols) + (big ? 64 * (k >> 1) : 32 * ((k - 4) >> 2));
    const uint16_t *F = a.orig + (size_t)frame * frame_samples, *R = a.refs + (size_t)frame * frame_samples;
    __syncthreads();  // (the previous item's last reads of the window and of s_tab)
    for (int i = tid; i < side * side; i += kThreads) {
      const long long idx = (long long)(y0 + (i >> lp)) * a.width + x0 + (i & (side - 1));
      s_org[i] = idx < frame_samples ? F[idx] : (uint16_t)0;
    }
    const int rows = big ? kRefRows64 : kRefRows32;
    for (int i = tid; i < rows * side; i += kThreads) {
      const int r = i >> lp;
      const long long idx = (long long)(y0 - 1 + r) * a.width + x0 + (i & (side - 1));
      s_ref[i] = idx >= 0 && idx < frame_samples ? R[idx] : (uint16_t)0;
    }
    if (tid <= side) {  // rows y0-1 .. y0+side-1 of column x0-1
      const long long idx = (long long)(y0 - 1 + tid) * a.width + x0 - 1;
      s_left[tid] = idx >= 0 && idx < frame_samples ? R[idx] : (uint16_t)0;
    }
    if (tid == 0) s_ref[kConstAt] = 512;
    if (big && tid < kAngModes) s_tab[0][tid] = s_tab[1][tid] = s_tab[2][tid] = none;
    __syncthreads();
    const LdsRef ref{s_ref, x0, y0, lp};
    const size_t cu_base = (size_t)fc * MIP_CUS_PER_CTU;
    int org[16];
    if (big) {  // 256 lanes, one CU: wave sums per mode, then the four waves' through LDS
      const IntraSlot c{k, tid & 15, tid >> 4, 0, 0, 6, 6};
      load_org(s_org, lp, c, org);
      const LdsBound b(ref, x0, y0, 64, 64);
      const int corner = b.corner();
      for (int q = 0; q < a.nmodes; q++) {
        int v[2];
        ang_block(b, ang_unpack(a.modes[q]), corner, 6, 6, 4 * c.bi, 4 * c.bj, org, v[0], v[1]);
        group_sum(v, 64);
        if (lane == 0) s_sum[wave][q][0] = v[0], s_sum[wave][q][1] = v[1];
      }
      __syncthreads();
      const bool on = !a.unavail[(size_t)ctu * MIP_CUS_PER_CTU + k];
      if (tid < a.nmodes && on) {
        const int slot = ang_unpack(a.modes[tid]).m - MIP_ANGULAR_FIRST;
        const int sad = s_sum[0][tid][0] + s_sum[1][tid][0] + s_sum[2][tid][0] + s_sum[3][tid][0];
        const int satd = s_sum[0][tid][1] + s_sum[1][tid][1] + s_sum[2][tid][1] + s_sum[3][tid][1];
        s_tab[0][slot] = intra_cost(sad, satd);
        s_tab[1][slot] = sad;
        s_tab[2][slot] = satd;
      }
      __syncthreads();
      const size_t cu = cu_base + k;
      if (tid < kAngModes) {
        if (a.cost) a.cost[cu * kAngModes + tid] = s_tab[0][tid];
        if (a.sad) a.sad[cu * kAngModes + tid] = s_tab[1][tid];
        if (a.satd) a.satd[cu * kAngModes + tid] = s_tab[2][tid];
      }
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
      const uint32_t *slots = a.slots + (size_t)(k - 4) * a.slots_per_block;
      for (int at = 64 * wave; at < a.slots_per_block; at += kThreads) {
        const uint32_t word = slots[at + lane];
        const IntraSlot c = intra_slot_decode(word);  // (no slot: fields of CU 0 at the window's corner, nothing written)
        const int n = 1 << (c.lw + c.lh - 4);
        load_org(s_org, lp, c, org);
        const LdsBound b(ref, x0 + 4 * c.cx, y0 + 4 * c.cy, 1 << c.lw, 1 << c.lh);
        const int corner = b.corner();
        const bool first = !(word & kIntraNoSlot) && (c.bi | c.bj) == 0;  // the lane that writes the CU
        const bool on = first && !a.unavail[(size_t)ctu * MIP_CUS_PER_CTU + c.cu];
        const size_t cu = cu_base + c.cu;
        if (tables && first) {  // slots of modes not in the list, every slot of an unavailable CU
          for (int slot = 0; slot < kAngModes; slot++)
            if (!on || !ang_listed(a.listed, slot)) {
              if (a.cost) a.cost[cu * kAngModes + slot] = none;
              if (a.sad) a.sad[cu * kAngModes + slot] = none;
              if (a.satd) a.satd[cu * kAngModes + slot] = none;
            }
        }
        uint8_t best_mode = 0xff;
        int32_t best_cost = none;
        for (int q = 0; q < a.nmodes; q += 2) {
          const bool two = q + 1 < a.nmodes;
          const AngMode m0 = ang_unpack(a.modes[q]), m1 = ang_unpack(a.modes[two ? q + 1 : q]);
          int v[4] = {0, 0, 0, 0};
          ang_block(b, m0, corner, c.lw, c.lh, 4 * c.bi, 4 * c.bj, org, v[0], v[1]);
          if (two) ang_block(b, m1, corner, c.lw, c.lh, 4 * c.bi, 4 * c.bj, org, v[2], v[3]);
          group_sum(v, n);
          auto take = [&](int m, int sad, int satd) {
            const int32_t cost = intra_cost(sad, satd);
            const size_t to = cu * kAngModes + m - MIP_ANGULAR_FIRST;
            if (a.cost) a.cost[to] = cost;
            if (a.sad) a.sad[to] = sad;
            if (a.satd) a.satd[to] = satd;
            ang_best_step(best_mode, best_cost, m, cost);
          };
          if (on) {
            take(m0.m, v[0], v[1]);
            if (two) take(m1.m, v[2], v[3]);
          }
        }
        if (first) write_best(a, cu, on, best_mode, best_cost);
      }
    }
  }
}

}  // namespace

hipError_t launch_angular(const AngularArgs &a, hipStream_t s) {
  const long long groups = (long long)a.nframes * a.nctus * kItemsPerCtu;
  if (!a.orig || !a.refs || !a.unavail || !a.slots || a.nframes < 1 || a.nctus < 1 || a.ctu_cols < 1 || a.slots_per_block < 64 ||
      a.slots_per_block % 64 || (long long)a.nframes * a.nctus * MIP_CUS_PER_CTU > (1LL << 31) - 256 || a.nmodes < 1 ||
      a.nmodes > kAngModes || !a.best_cost != !a.best_mode || !a.ang_cost != !a.ang_mode ||
      (!a.cost && !a.sad && !a.satd && !a.best_cost && !a.ang_cost))
    return hipErrorInvalidValue;
  // a few rounds of resident workgroups, each striding over the items
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
    return hipErrorInvalidDevice;
  const long long grid = groups < 32LL * cus ? groups : 32LL * cus;
  hipLaunchKernelGGL(angular_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace mipgpu

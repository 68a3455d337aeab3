// mip_intra.hip -- Planar / DC baseline costs of every CU and the MIP-vs-regular decision merge
// (gfx950), contract in include/mipgpu.h (mip_intra_device).  No reference counterpart: the
// reference ranks MIP modes only.  The arithmetic is intra_plan.h's, shared with the host walk.
//
// Work items, window staging, the window Ref and the group sum are mip_window_dev.h's, shared with
// the angular kernels.  Per lane slot a lane builds both modes' 16 residuals in registers and runs
// the Hadamard in-lane; the DC sums and the four per-CU sums are xor-shuffle reductions inside the
// group (the 64x64 CU's 256 lanes finish through LDS).  The group's first lane writes the CU's
// two costs per table with one 8-byte store and merges the CU's decision.  No atomics; every
// index comes from the slot table and the work-item index, sample values are only ever values.
// DESIGN.md section 5.6.
#include "mip_window_dev.h"

namespace mipgpu {
namespace {

// One lane's 4x4 block of the CU at window position (4 cx, 4 cy): the block's inputs but the DC
// value, and the lane's share of the boundary sums.
__device__ __forceinline__ void load_block(const LdsRef &ref, const uint16_t *s_org, const IntraSlot &c, IntraBlock &b, int *org,
                                           int &sum_top, int &sum_left) {
  const int x = ref.x0 + 4 * c.cx, y = ref.y0 + 4 * c.cy;
  b.i0 = 4 * c.bi;
  b.j0 = 4 * c.bj;
  b.lw = c.lw;
  b.lh = c.lh;
  sum_top = sum_left = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    sum_top += b.top[k] = intra_top(ref, x, y, b.i0 + k);
    sum_left += b.left[k] = intra_left(ref, x, y, b.j0 + k);
  }
  b.tr = intra_top(ref, x, y, (1 << c.lw) - 1);
  b.bl = intra_left(ref, x, y, (1 << c.lh) - 1);
  if (c.bj) sum_top = 0;   // the top row of blocks carries the top boundary,
  if (c.bi) sum_left = 0;  // the left column the left one
  load_org(s_org + ((4 * c.cy + b.j0) << ref.lp) + 4 * c.cx + b.i0, ref.lp, org);
}

// The CU's results: its table entries and its decision.  One lane per CU.
__device__ __forceinline__ void write_cu(const IntraArgs &a, size_t cu, bool on, const int *sad, const int *satd) {
  const int32_t none = MIP_COST_UNAVAILABLE;
  const int32_t c0 = on ? intra_cost(sad[0], satd[0]) : none, c1 = on ? intra_cost(sad[1], satd[1]) : none;
  if (a.cost) reinterpret_cast<int2 *>(a.cost)[cu] = make_int2(c0, c1);
  if (a.sad) reinterpret_cast<int2 *>(a.sad)[cu] = on ? make_int2(sad[0], sad[1]) : make_int2(none, none);
  if (a.satd) reinterpret_cast<int2 *>(a.satd)[cu] = on ? make_int2(satd[0], satd[1]) : make_int2(none, none);
  if (a.best_cost) {
    uint8_t mode = a.best_mode[cu];
    int32_t cost = a.best_cost[cu];
    const int32_t before = cost;
    intra_merge(mode, cost, c0, c1, a.bias[0], a.bias[1]);
    if (cost != before) {
      a.best_mode[cu] = mode;
      a.best_cost[cu] = cost;
    }
  }
}

__global__ __launch_bounds__(kThreads) void intra_kernel(IntraArgs a) {
  __shared__ __attribute__((aligned(16))) uint16_t s_org[64 * 64];
  __shared__ __attribute__((aligned(16))) uint16_t s_ref[kRefCells];
  __shared__ int s_part[kThreads / 64][6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long frame_samples = (long long)a.width * a.height;
  const long long items = (long long)a.nframes * a.nctus * kItemsPerCtu;
  for (long long g = blockIdx.x; g < items; g += gridDim.x) {
    const WindowItem it = window_item(g, a.nctus, a.ctu_cols, frame_samples, a.orig, a.refs);
    const int k = it.k, ctu = it.ctu;
    __syncthreads();  // (the previous item's last reads of the window)
    stage_window(it.F, it.R, a.width, frame_samples, it.x0, it.y0, it.lp, it.big, tid, s_org, s_ref);
    __syncthreads();
    const LdsRef ref{s_ref, it.x0, it.y0, it.lp};
    const size_t cu_base = (size_t)it.fc * MIP_CUS_PER_CTU;
    IntraBlock b;
    int org[16], st, sl;
    if (it.big) {  // 256 lanes, one CU: wave sums, then the four waves' through LDS
      const IntraSlot c{k, tid & 15, tid >> 4, 0, 0, 6, 6};
      load_block(ref, s_org, c, b, org, st, sl);
      int bs[2] = {st, sl};
      group_sum(bs, 64);
      if (lane == 0) s_part[wave][0] = bs[0], s_part[wave][1] = bs[1];
      __syncthreads();
      b.dc = intra_dc(s_part[0][0] + s_part[1][0] + s_part[2][0] + s_part[3][0], s_part[0][1] + s_part[1][1] + s_part[2][1] + s_part[3][1], 6, 6);
      const IntraSums s = intra_block(b, org);
      int v[4] = {s.sad[0], s.sad[1], s.satd[0], s.satd[1]};
      group_sum(v, 64);
      if (lane == 0) {
#pragma unroll
        for (int q = 0; q < 4; q++) s_part[wave][2 + q] = v[q];
      }
      __syncthreads();
      if (tid == 0) {
        int t[4];
#pragma unroll
        for (int q = 0; q < 4; q++) t[q] = s_part[0][2 + q] + s_part[1][2 + q] + s_part[2][2 + q] + s_part[3][2 + q];
        write_cu(a, cu_base + k, !a.unavail[(size_t)ctu * MIP_CUS_PER_CTU + k], t, t + 2);
      }
    } else {
      const uint32_t *slots = a.slots + (size_t)(k - 4) * a.slots_per_block;
      for (int at = 64 * wave; at < a.slots_per_block; at += kThreads) {
        const uint32_t word = slots[at + lane];
        const IntraSlot c = intra_slot_decode(word);  // (no slot: fields of CU 0 at the window's corner, nothing written)
        const int n = 1 << (c.lw + c.lh - 4);
        load_block(ref, s_org, c, b, org, st, sl);
        int bs[2] = {st, sl};
        group_sum(bs, n);
        b.dc = intra_dc(bs[0], bs[1], c.lw, c.lh);
        const IntraSums s = intra_block(b, org);
        int v[4] = {s.sad[0], s.sad[1], s.satd[0], s.satd[1]};
        group_sum(v, n);
        if (!(word & kIntraNoSlot) && (c.bi | c.bj) == 0)
          write_cu(a, cu_base + c.cu, !a.unavail[(size_t)ctu * MIP_CUS_PER_CTU + c.cu], v, v + 2);
      }
    }
  }
}

}  // namespace

hipError_t launch_intra(const IntraArgs &a, hipStream_t s) {
  if (!window_args_ok(a) || (!a.cost && !a.sad && !a.satd && !a.best_cost)) return hipErrorInvalidValue;
  return launch_window_kernel(intra_kernel, a, s);
}

}  // namespace mipgpu

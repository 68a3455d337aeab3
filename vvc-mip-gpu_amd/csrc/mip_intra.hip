// mip_intra.hip -- Planar / DC baseline costs of every CU and the MIP-vs-regular decision merge
// (gfx950), contract in include/mipgpu.h (mip_intra_device).  No reference counterpart: the
// reference ranks MIP modes only.  The arithmetic is intra_plan.h's, shared with the host walk.
//
// Work items are (frame, CTU, k): k < 4 the 64x64 CU of quadrant k, else the 32x32 block
// k - 4, which holds 336 CUs of the other 46 shapes.  A workgroup (4 waves) takes items
// blockIdx.x, + gridDim.x, ...; per item it stages the window's originals and reference
// samples once, by linear index with the guard idx < W*H (2-byte loads: no alignment demand on
// the caller's frames), as uint16 in LDS:
//   s_org   S x S originals                        (S = 32 or 64)
//   s_ref   rows y0-1 .. y0+S-1 of columns x0 .. x0+S-1   (64x64: rows y0-1 and y0 only)
//   s_left  column x0-1 of the same rows
// and then walks the block's lane slots (intra_plan.h intra_build_slots): one lane per 4x4
// block of a CU, a CU's lanes an aligned power-of-two group of one wave.  A lane builds both
// modes' 16 residuals in registers and runs the Hadamard in-lane; the DC sums and the four
// per-CU sums are xor-shuffle reductions inside the group (the 64x64 CU's 256 lanes finish
// through LDS).  The group's first lane writes the CU's two costs per table with one 8-byte
// store and merges the CU's decision.  No atomics; every index comes from the slot table and
// the work-item index, sample values are only ever values.  DESIGN.md section 5.6.
#include "intra_plan.h"
#include "mip_kernels.h"

namespace mipgpu {
namespace {

constexpr int kThreads = 256;
constexpr int kItemsPerCtu = 4 + kIntraBlocks;
constexpr int kRefRows32 = 33, kRefRows64 = 2;
constexpr int kLeftAt = kRefRows32 * 32;  // s_left inside the reference array

// The staged window as a Ref of intra_plan.h.
struct LdsRef {
  const uint16_t *ref;  // s_ref, with s_left at kLeftAt (one array: one index, no pointer select)
  int x0, y0, lp;       // the window's frame position, log2 of its side
  __device__ __forceinline__ int operator()(int row, int col) const {
    const int r = row - y0 + 1;
    return ref[col >= x0 ? (r << lp) + col - x0 : kLeftAt + r];
  }
};

// Sums of K values over the lane's group of n lanes (a power of two, the group aligned): every
// lane runs all six steps and keeps only those inside its group -- branch-free, the K chains of a
// step independent.  (Skipping the steps no lane of the wave needs, by a wave-uniform bound, was
// not faster: DESIGN.md section 5.6.)
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
  const uint16_t *o = s_org + ((4 * c.cy + b.j0) << ref.lp) + 4 * c.cx + b.i0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint2 v = *reinterpret_cast<const uint2 *>(o + (r << ref.lp));
    org[4 * r] = (int)(v.x & 0xffffu);
    org[4 * r + 1] = (int)(v.x >> 16);
    org[4 * r + 2] = (int)(v.y & 0xffffu);
    org[4 * r + 3] = (int)(v.y >> 16);
  }
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
  __shared__ __attribute__((aligned(16))) uint16_t s_ref[kLeftAt + 65 + 7];
  uint16_t *const s_left = s_ref + kLeftAt;
  __shared__ int s_part[kThreads / 64][6];
  static_assert(kRefRows64 * 64 <= kRefRows32 * 32, "the 64x64 CU's reference rows fit");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long frame_samples = (long long)a.width * a.height;
  const long long items = (long long)a.nframes * a.nctus * kItemsPerCtu;
  for (long long g = blockIdx.x; g < items; g += gridDim.x) {
    const long long fc = g / kItemsPerCtu;  // frame * nctus + ctu
    const int k = (int)(g - fc * kItemsPerCtu), frame = (int)(fc / a.nctus), ctu = (int)(fc - (long long)frame * a.nctus);
    const bool big = k < 4;
    const int lp = big ? 6 : 5, side = 1 << lp;
    const int x0 = 128 * (ctu % a.ctu_cols) + (big ? 64 * (k & 1) : 32 * ((k - 4) & 3));
    const int y0 = 128 * (ctu / a.ctu_cols) + (big ? 64 * (k >> 1) : 32 * ((k - 4) >> 2));
    const uint16_t *F = a.orig + (size_t)frame * frame_samples, *R = a.refs + (size_t)frame * frame_samples;
    __syncthreads();  // (the previous item's last reads of the window)
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
    __syncthreads();
    const LdsRef ref{s_ref, x0, y0, lp};
    const size_t cu_base = (size_t)fc * MIP_CUS_PER_CTU;
    IntraBlock b;
    int org[16], st, sl;
    if (big) {  // 256 lanes, one CU: wave sums, then the four waves' through LDS
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
  const long long groups = (long long)a.nframes * a.nctus * kItemsPerCtu;
  if (!a.orig || !a.refs || !a.unavail || !a.slots || a.nframes < 1 || a.nctus < 1 || a.ctu_cols < 1 || a.slots_per_block < 64 ||
      a.slots_per_block % 64 || (long long)a.nframes * a.nctus * MIP_CUS_PER_CTU > (1LL << 31) - 256 || !a.best_cost != !a.best_mode ||
      (!a.cost && !a.sad && !a.satd && !a.best_cost))
    return hipErrorInvalidValue;
  // a few rounds of resident workgroups, each striding over the items
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
    return hipErrorInvalidDevice;
  const long long grid = groups < 32LL * cus ? groups : 32LL * cus;
  hipLaunchKernelGGL(intra_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace mipgpu

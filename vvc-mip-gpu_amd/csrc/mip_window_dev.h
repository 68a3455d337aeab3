// mip_window_dev.h -- what the kernels that cost every CU of a frame from a staged window share
// (intra_kernel in mip_intra.hip; the six angular cost kernels of mip_angular.hip, one body, through
// mip_angular_dev.h): the work items, the window staging, the window as a Ref, the group sum, a
// lane's originals, and the launchers' common argument and grid rules.  Internal linkage: each
// kernel file has its own copies.  DESIGN.md section 5.6.
//
// Work items are (frame, CTU, k): k < 4 the 64x64 CU of quadrant k, else the 32x32 block k - 4,
// which holds 336 CUs of the other 46 shapes.  A workgroup (4 waves) takes items blockIdx.x,
// + gridDim.x, ...; per item it stages the window's originals and reference samples once, by
// linear index with the guard idx < W*H (2-byte loads: no alignment demand on the caller's
// frames), as uint16 in LDS:
//   s_org   S x S originals                        (S = 32 or 64)
//   s_ref   rows y0-1 .. y0+S-1 of columns x0 .. x0+S-1   (64x64: rows y0-1 and y0 only)
//   s_left  column x0-1 of the same rows, inside s_ref's array at kLeftAt
// and then walks the block's lane slots (intra_plan.h intra_build_slots): one lane per 4x4 block
// of a CU, a CU's lanes an aligned power-of-two group of one wave.
//
// The device helpers here take pointers and scalars, not a reference to a kernel's argument struct
// (a staging helper that took one left the angular kernels with 20 bytes of private segment per
// lane), and their form is the one in which the kernels keep their registers and the code of
// their loops: DESIGN.md section 5.6, "One copy".  (The angular kernels' shared body, inlined into
// each one-line kernel, does take the struct by const reference: mip_angular_dev.h.)
#pragma once
#include "intra_plan.h"
#include "mip_kernels.h"

namespace mipgpu {
namespace {

constexpr int kThreads = 256;
constexpr int kItemsPerCtu = 4 + kIntraBlocks;
constexpr int kRefRows32 = 33, kRefRows64 = 2;
constexpr int kLeftAt = kRefRows32 * 32;     // s_left inside the reference array
constexpr int kRefCells = kLeftAt + 65 + 7;  // s_ref's array: the rows, s_left, padding to 16 bytes
static_assert(kRefRows64 * 64 <= kRefRows32 * 32, "the 64x64 CU's reference rows fit");

// One work item: its place in the batch and its window.
struct WindowItem {
  long long fc;  // frame * nctus + ctu
  int k, ctu;
  bool big;            // the 64x64 CU of quadrant k (else the 32x32 block k - 4)
  int lp, x0, y0;      // log2 of the window's side, its frame position
  const uint16_t *F, *R;  // the frame's originals and reference source
};
__device__ __forceinline__ WindowItem window_item(long long g, int nctus, int ctu_cols, long long frame_samples, const uint16_t *orig,
                                                  const uint16_t *refs) {
  WindowItem it;
  it.fc = g / kItemsPerCtu;
  const int k = (int)(g - it.fc * kItemsPerCtu), frame = (int)(it.fc / nctus), ctu = (int)(it.fc - (long long)frame * nctus);
  const bool big = k < 4;
  it.k = k, it.ctu = ctu, it.big = big;
  it.lp = big ? 6 : 5;
  it.x0 = 128 * (ctu % ctu_cols) + (big ? 64 * (k & 1) : 32 * ((k - 4) & 3));
  it.y0 = 128 * (ctu / ctu_cols) + (big ? 64 * (k >> 1) : 32 * ((k - 4) >> 2));
  it.F = orig + (size_t)frame * frame_samples, it.R = refs + (size_t)frame * frame_samples;
  return it;
}

// Stages the item's window; s_ref is the whole reference array of kRefCells.  The caller has a
// barrier before it (the previous item's last reads) and one behind it.
__device__ __forceinline__ void stage_window(const uint16_t *F, const uint16_t *R, int width, long long frame_samples, int x0, int y0, int lp,
                                             bool big, int tid, uint16_t *s_org, uint16_t *s_ref) {
  const int side = 1 << lp;
  for (int i = tid; i < side * side; i += kThreads) {
    const long long idx = (long long)(y0 + (i >> lp)) * width + x0 + (i & (side - 1));
    s_org[i] = idx < frame_samples ? F[idx] : (uint16_t)0;
  }
  const int rows = big ? kRefRows64 : kRefRows32;
  for (int i = tid; i < rows * side; i += kThreads) {
    const int r = i >> lp;
    const long long idx = (long long)(y0 - 1 + r) * width + x0 + (i & (side - 1));
    s_ref[i] = idx >= 0 && idx < frame_samples ? R[idx] : (uint16_t)0;
  }
  if (tid <= side) {  // rows y0-1 .. y0+side-1 of column x0-1
    const long long idx = (long long)(y0 - 1 + tid) * width + x0 - 1;
    s_ref[kLeftAt + tid] = idx >= 0 && idx < frame_samples ? R[idx] : (uint16_t)0;
  }
}

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

// The 16 originals of the 4x4 block whose first sample is o, in a window of side 1 << lp; of the
// slot's block, at window position (4 cx + 4 bi, 4 cy + 4 bj).
__device__ __forceinline__ void load_org(const uint16_t *o, int lp, int *org) {
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const uint2 v = *reinterpret_cast<const uint2 *>(o + (r << lp));
    org[4 * r] = (int)(v.x & 0xffffu);
    org[4 * r + 1] = (int)(v.x >> 16);
    org[4 * r + 2] = (int)(v.y & 0xffffu);
    org[4 * r + 3] = (int)(v.y >> 16);
  }
}
__device__ __forceinline__ void load_org(const uint16_t *s_org, int lp, const IntraSlot &c, int *org) {
  load_org(s_org + ((4 * c.cy + 4 * c.bj) << lp) + 4 * c.cx + 4 * c.bi, lp, org);
}

// ---- host side: what the launchers share.  The argument rules every one of them has; each
// adds its own (its mode list, its seeds, "at least one output").
template <class Args>
inline bool window_args_ok(const Args &a) {
  return a.orig && a.refs && a.unavail && a.slots && a.nframes >= 1 && a.nctus >= 1 && a.ctu_cols >= 1 && a.slots_per_block >= 64 &&
         a.slots_per_block % 64 == 0 && (long long)a.nframes * a.nctus * MIP_CUS_PER_CTU <= (1LL << 31) - 256 && !a.best_cost == !a.best_mode;
}
// The launch: a few rounds of resident workgroups, each striding over the items.
template <class Args>
inline hipError_t launch_window_kernel(void (*kernel)(Args), const Args &a, hipStream_t s) {
  const long long groups = (long long)a.nframes * a.nctus * kItemsPerCtu;
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
    return hipErrorInvalidDevice;
  const long long grid = groups < 32LL * cus ? groups : 32LL * cus;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace
}  // namespace mipgpu

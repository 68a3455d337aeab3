// mip_partition.hip -- CTU partition decision from the per-CU best costs (gfx950), contract in
// include/mipgpu.h (mip_partition_device).  A workgroup takes one (frame, CTU) at a time and
// walks the state graph of partition_tables.h with the per-state steps of partition_plan.h:
// the states of one level in parallel, a barrier between levels -- bottom-up for the costs and
// choices (LDS), top-down for the marks, then the leaves are compacted in CU order by a
// workgroup prefix sum (no atomic append: the list order is deterministic).
//
// LDS: int32 cost + uint8 choice per state, 10245 states (51.3 KB), and the 13 KB block
// template: 63 KB, two workgroups per CU.  After the bottom-up pass only the root's cost is
// still needed, so the leaf words (uint16 per CU) and the scan buffers live in the cost array.
// Indices come from the tables and the workgroup index alone; the input arrays are only ever
// values.  DESIGN.md section 5.5.
#include "mip_kernels.h"
#include "partition_plan.h"

namespace mipgpu {
namespace {

// The block template: 13 KB, copied into LDS once per workgroup (every state reads its entries
// in each of the three passes, and the entries head the chain table -> CU index -> cost).
struct Tables {
  alignas(16) mip_part_state state[MIP_PART_BLOCK_STATES];
  alignas(16) uint16_t child[MIP_PART_SPLIT_STATES][10];
  alignas(16) mip_part_step step[kPartShapes];
  alignas(16) uint16_t qt[MIP_PART_QT_STATES][4];
};
static_assert(sizeof(Tables) % 16 == 0, "copied 16 bytes per lane");
__constant__ Tables c_tables = {MIP_PART_STATE_TABLE, MIP_PART_CHILD_TABLE, MIP_PART_STEP_TABLE, MIP_PART_QT_TABLE};
__constant__ int c_levels[MIP_PART_NUM_LEVELS + 1] = MIP_PART_LEVELS;

constexpr int kThreads = 512;
constexpr int kCus = MIP_CUS_PER_CTU_ABI;
constexpr int kChunk = (kCus + kThreads - 1) / kThreads;  // CUs per thread in the compaction
constexpr int kCostWords = (kPartStates + 3) & ~3;
constexpr int kScanAt = 4096;  // int32 offset of the scan buffers in the cost array, past the leaf words
static_assert(kCus * 2 <= kScanAt * 4 && kScanAt + 2 * kThreads <= kCostWords, "LDS reuse");

__global__ __launch_bounds__(kThreads) void partition_kernel(PartitionArgs a) {
  __shared__ int32_t s_cost[kCostWords];
  __shared__ uint8_t s_choice[kCostWords];
  __shared__ int32_t s_pen[kPartShapes + 1];
  __shared__ Tables s_tables;
  const int tid = threadIdx.x;
  for (int i = tid; i < (int)(sizeof(Tables) / 16); i += kThreads)
    reinterpret_cast<uint4 *>(&s_tables)[i] = reinterpret_cast<const uint4 *>(&c_tables)[i];
  const PartTables t{s_tables.state, s_tables.child, s_tables.qt, s_tables.step};
  if (tid < kPartShapes) s_pen[tid] = a.penalty.v[tid];
  // a workgroup takes (frame, CTU) pairs blockIdx.x, + gridDim.x, ...
  for (int g = blockIdx.x; g < a.nframes * a.nctus; g += gridDim.x) {
    __syncthreads();  // (the tables; the previous pair's last reads of the LDS arrays)
    const int frame = g / a.nctus, ctu = g - frame * a.nctus;
    const PartCtu f{a.width, a.height, 128 * (ctu % a.ctu_cols), 128 * (ctu / a.ctu_cols)};
    const int32_t *best_cost = a.best_cost + (size_t)g * kCus;

    // bottom-up: depth 3 -> 1, the nodes of side 8, 16, 32, then 64 and the root
    for (int lv = MIP_PART_NUM_LEVELS - 1; lv >= 0; lv--) {
      const int begin = c_levels[lv], n = c_levels[lv + 1] - begin;
      for (int i = tid; i < MIP_PART_BLOCKS * n; i += kThreads) {
        const int block = i / n;
        part_eval_state(t, f, best_cost, s_pen, s_cost, s_choice, block, begin + i - block * n);
      }
      __syncthreads();
    }
    if (tid < 4) part_eval_node64(f, best_cost, s_pen, s_cost, s_choice, tid);
    __syncthreads();
    if (tid == 0) part_eval_root(s_cost, s_choice);
    __syncthreads();
    const int32_t total_cost = s_cost[kPartRoot];

    // top-down: the chosen tree's states
    if (tid == 0) part_mark_root(s_choice);
    __syncthreads();
    if (tid < 4) part_mark_node64(s_choice, tid);
    __syncthreads();
    for (int lv = 0; lv < MIP_PART_NUM_LEVELS - 1; lv++) {
      const int begin = c_levels[lv], n = c_levels[lv + 1] - begin;
      for (int i = tid; i < MIP_PART_BLOCKS * n; i += kThreads) {
        const int block = i / n;
        part_mark_state(t, s_choice, block, begin + i - block * n);
      }
      __syncthreads();
    }

    // leaves per CU (the cost array is free now)
    uint16_t *s_leaf = reinterpret_cast<uint16_t *>(s_cost);
    int32_t *s_scan = s_cost + kScanAt;
    for (int k = tid; k < kCus; k += kThreads) s_leaf[k] = 0;
    __syncthreads();
    if (tid < 4) part_collect_node64(s_choice, s_leaf, tid);
    for (int i = tid; i < kPartBtStates; i += kThreads) {
      const int block = i / kPartBlockStates;
      part_collect_state(t, s_choice, s_leaf, block, i - block * kPartBlockStates);
    }
    __syncthreads();

    // compaction in CU order: thread tid owns CUs [tid * kChunk, (tid + 1) * kChunk)
    int cnt = 0;
    for (int j = 0; j < kChunk; j++) {
      const int k = tid * kChunk + j;
      cnt += k < kCus && s_leaf[k] != 0;
    }
    s_scan[tid] = cnt;
    __syncthreads();
    int src = 0;
    for (int d = 1; d < kThreads; d <<= 1) {  // inclusive scan, two buffers
      int v = s_scan[src * kThreads + tid];
      if (tid >= d) v += s_scan[src * kThreads + tid - d];
      src ^= 1;
      s_scan[src * kThreads + tid] = v;
      __syncthreads();
    }
    const int nleaves = s_scan[src * kThreads + kThreads - 1];

    if (a.items) {
      mip_pred_item *items = a.items + (size_t)g * MIP_PART_MAX_LEAVES;
      const uint8_t *best_mode = a.best_mode + (size_t)g * kCus;
      int at = s_scan[src * kThreads + tid] - cnt;
      for (int j = 0; j < kChunk; j++) {
        const int k = tid * kChunk + j;
        if (k < kCus && s_leaf[k] != 0 && at < MIP_PART_MAX_LEAVES) items[at++] = part_item(f, frame, ctu, k, s_leaf[k], best_mode[k]);
      }
      for (int i = nleaves + tid; i < MIP_PART_MAX_LEAVES; i += kThreads) items[i] = part_pad_item();
    }
    if (a.leaf) {
      uint8_t *leaf = a.leaf + (size_t)g * kCus;
      for (int k = tid; k < kCus; k += kThreads) leaf[k] = s_leaf[k] != 0;
    }
    if (tid == 0) {
      if (a.ctu_cost) a.ctu_cost[g] = total_cost;  // (kPartInf == MIP_COST_UNAVAILABLE: no partition)
      if (a.ctu_leaves) a.ctu_leaves[g] = nleaves;
    }
  }
}

}  // namespace

hipError_t launch_partition(const PartitionArgs &a, hipStream_t s) {
  const long long groups = (long long)a.nframes * a.nctus;
  if (!a.best_cost || a.nframes < 1 || a.nctus < 1 || a.ctu_cols < 1 || groups * kCus >= (1LL << 31) || (a.items && !a.best_mode))
    return hipErrorInvalidValue;
  // two workgroups fit a CU (LDS); a few rounds of them, each striding over the pairs
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
    return hipErrorInvalidDevice;
  const long long grid = groups < 8LL * cus ? groups : 8LL * cus;
  hipLaunchKernelGGL(partition_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace mipgpu

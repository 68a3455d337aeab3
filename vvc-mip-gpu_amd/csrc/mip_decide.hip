// mip_decide.hip -- per-CU decisions from the search's outputs (gfx950): the decision lists
// of a cost table (best_mode_kernel) and the split CUs of a decisions-only search
// (dec_split_kernel, see SearchArgs::best_cost in mip_kernels.h).
#include "mip_kernels.h"
#include "mip_tables.h"

namespace mipgpu {
namespace {

constexpr int kUnavailable = MIP_COST_UNAVAILABLE;

__constant__ mip_shape_desc c_shapes[MIP_NUM_SHAPES] = MIP_SHAPE_TABLE;
// first CU (reference order inside a CTU) of every shape, for the decision-list kernel
struct ShapeStarts {
  uint16_t v[MIP_NUM_SHAPES + 1];
};
constexpr mip_shape_desc kShapesC[MIP_NUM_SHAPES] = MIP_SHAPE_TABLE;
constexpr ShapeStarts make_shape_starts() {
  ShapeStarts st{};
  for (int i = 0; i < MIP_NUM_SHAPES; i++) st.v[i + 1] = (uint16_t)(st.v[i] + kShapesC[i].ncu);
  return st;
}
static_assert(make_shape_starts().v[MIP_NUM_SHAPES] == MIP_CUS_PER_CTU, "shape table");
__constant__ ShapeStarts c_shape_start = make_shape_starts();

// Decision list of one CU: the k lowest-cost of its M modes (ties to the lower mode), by
// repeated selection over the row held in registers; 0xff / kUnavailable past the M modes
// and for unavailable CUs (every entry of such a row is kUnavailable).
template <int M>
__device__ __forceinline__ void topk_row(const int32_t *row, int k, uint8_t *mo, int32_t *co) {
  int v[M];
#pragma unroll
  for (int m = 0; m < M; m += 4) {  // rows start 16-byte aligned (12, 16 or 32 entries per CU)
    const int4 q = *reinterpret_cast<const int4 *>(row + m);
    v[m] = q.x, v[m + 1] = q.y, v[m + 2] = q.z, v[m + 3] = q.w;
  }
  const bool unavailable = v[0] == kUnavailable;
  uint32_t used = 0;
  for (int r = 0; r < k; r++) {
    int best = 0, bc = 0;
    bool found = false;
#pragma unroll
    for (int m = 0; m < M; m++)
      if (!((used >> m) & 1) && (!found || v[m] < bc)) best = m, bc = v[m], found = true;
    const bool ok = found && !unavailable;
    if (ok) used |= 1u << best;
    if (mo) mo[r] = ok ? (uint8_t)best : 0xff;
    if (co) co[r] = ok ? bc : kUnavailable;
  }
}

// Per-CU decision lists (k = 1: the argmin).
__global__ __launch_bounds__(256) void best_mode_kernel(BestArgs a) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.total_cus) return;
  const int ctu = g / MIP_CUS_PER_CTU;
  int r = g - ctu * MIP_CUS_PER_CTU, s = 0;
#pragma unroll
  for (int step = 32; step; step >>= 1)  // last shape whose first CU is <= r
    if (s + step < MIP_NUM_SHAPES && c_shape_start.v[s + step] <= r) s += step;
  r -= c_shape_start.v[s];
  const mip_shape_desc sd = c_shapes[s];
  const int32_t *row = a.cost + (size_t)ctu * MIP_COSTS_PER_CTU + sd.cost_offset + (size_t)r * 2 * sd.modes;
  uint8_t *mo = a.best_mode ? a.best_mode + (size_t)g * a.k : nullptr;
  int32_t *co = a.best_cost ? a.best_cost + (size_t)g * a.k : nullptr;
  switch (sd.modes) {
    case 6: topk_row<12>(row, a.k, mo, co); break;
    case 8: topk_row<16>(row, a.k, mo, co); break;
    default: topk_row<32>(row, a.k, mo, co); break;
  }
}

// Split CUs of decisions-only searches: all ones before the search (init), packed argmin ->
// decision list of length 1 after it (the layout of best_mode_kernel with k = 1).
template <bool INIT>
__global__ __launch_bounds__(256) void dec_split_kernel(SplitArgs a, int total) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int j = t % a.max_split, r = t / a.max_split, ctu = a.ctu0 + r % a.nrange, frame = r / a.nrange;
  const int v = a.ctu_var[ctu], b = a.split_begin[v];
  if (j >= a.split_begin[v + 1] - b) return;
  const size_t g = ((size_t)frame * a.nctus + ctu) * MIP_CUS_PER_CTU + a.split[b + j];
  if (INIT) {
    if (a.acc) a.acc[g] = ~0u;
    else a.best_cost[g] = -1;
  } else {
    uint32_t p;
    if (a.acc) {
      p = a.acc[g];
      a.acc[g] = ~0u;  // initialised for the next launch
    } else {
      p = (uint32_t)a.best_cost[g];
    }
    const bool ok = p != 0xffffffffu;
    if (a.best_mode) a.best_mode[g] = ok ? (uint8_t)(p & 31) : (uint8_t)0xff;
    a.best_cost[g] = ok ? (int32_t)(p >> 5) : kUnavailable;
  }
}

}  // namespace

hipError_t launch_dec_split(const SplitArgs &a, int nframes, bool init, hipStream_t s) {
  if (a.max_split < 1) return hipSuccess;  // no split CUs
  const long long total = (long long)nframes * a.nrange * a.max_split;
  if (!a.best_cost || !a.split || total >= (1LL << 31)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (init) hipLaunchKernelGGL(dec_split_kernel<true>, grid, dim3(256), 0, s, a, (int)total);
  else hipLaunchKernelGGL(dec_split_kernel<false>, grid, dim3(256), 0, s, a, (int)total);
  return hipGetLastError();
}

hipError_t launch_best_modes(const BestArgs &a, hipStream_t s) {
  if (a.k < 1 || a.k > kMaxBestK) return hipErrorInvalidValue;
  hipLaunchKernelGGL(best_mode_kernel, dim3((a.total_cus + 255) / 256), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace mipgpu

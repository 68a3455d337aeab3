// mip_candidates.hip -- K-best candidate lists over MIP, Planar / DC and angular modes (gfx950):
// include/mipgpu.h mip_candidates_device, arithmetic in candidates_plan.h.
//
// One lane per CU, one wave per workgroup: a workgroup takes 64 consecutive CUs.  Every lane keeps
// its CU's 32-bit (value, rank) keys in one LDS row (candidates_plan.h CandRow) -- an array in
// registers indexed by a run-time k would spill -- at an odd stride, so the 64 lanes' rows are in
// different banks.  No lane reads another lane's row: there is no barrier.
//   * Staging.  Every lane reads its own CU's entries -- 65 angular slots, Planar / DC, the MIP
//     list -- turns each into its key and stores it in its row.  A lane's angular row is 260
//     contiguous bytes, so one load instruction of the wave touches 64 cache lines, all of whose
//     bytes the following slots use: 8 KB of the table are in flight per instruction.  (Staging
//     the wave's 16 640 contiguous bytes with coalesced 256-byte steps through LDS was measured
//     and lost, 0.200 against 0.081 ms per 1080p frame: with 256 bytes per instruction the
//     launch is bound by the loads in flight)
//   * Selection.  Keys are unique, so round r is the lowest key of the row at or above one plus
//     the key of round r - 1: k passes over the row in LDS, no used-mask.
// The trip counts (65, kin, k, the row length) come from the kernel arguments.
#include "candidates_plan.h"
#include "mip_kernels.h"

namespace mipgpu {
namespace {

constexpr int kCandLanes = 64;  // CUs per workgroup

__global__ __launch_bounds__(kCandLanes) void candidates_kernel(CandidatesArgs a) {
  extern __shared__ uint32_t s_key[];  // [kCandLanes][row.stride]
  const int lane = threadIdx.x;
  const long long first = (long long)blockIdx.x * kCandLanes;  // the workgroup's first CU
  const long long left = a.total_cus - first;
  const int ncu = left < kCandLanes ? (int)left : kCandLanes;  // (the last workgroup may be short)
  const CandRow row = cand_row(a.ang_cost != nullptr, a.intra_cost != nullptr, a.mip_mode ? a.kin : 0);

  if (lane >= ncu) return;
  const size_t g = (size_t)first + lane;
  uint32_t *mine = s_key + lane * row.stride;
  if (a.ang_cost) {
    const int32_t *src = a.ang_cost + g * kAngModes;
#pragma unroll 13
    for (int slot = 0; slot < kAngModes; slot++) mine[row.ang + slot] = cand_key_ang(slot, src[slot], a.ang_bias);
  }
  if (a.intra_cost) {
    mine[row.intra] = cand_key_intra(0, a.intra_cost[g * kIntraModes], a.intra_bias[0]);
    mine[row.intra + 1] = cand_key_intra(1, a.intra_cost[g * kIntraModes + 1], a.intra_bias[1]);
  }
  if (a.mip_mode) {
    const uint8_t *mode = a.mip_mode + g * a.kin;
    const int32_t *cost = a.mip_cost + g * a.kin;
    for (int r = 0; r < a.kin; r++) mine[row.mip + r] = cand_key_mip(mode[r], cost[r]);
  }

  uint8_t *mo = a.modes ? a.modes + g * a.k : nullptr;
  int32_t *co = a.costs ? a.costs + g * a.k : nullptr;
  uint32_t floor = 0;
  for (int r = 0; r < a.k; r++) {
    uint32_t best = kCandNone;
    for (int j = 0; j < row.n; j++) best = cand_take(best, mine[j], floor);
    floor = cand_floor(best);
    if (mo) mo[r] = cand_key_code(best);
    if (co) co[r] = cand_key_value(best);
  }
}

}  // namespace

hipError_t launch_candidates(const CandidatesArgs &a, hipStream_t s) {
  if (a.total_cus < 1 || a.total_cus > (1LL << 31) - 256 || a.k < 1 || a.k > kCandMaxK || !a.mip_mode != !a.mip_cost ||
      (a.mip_mode && (a.kin < 1 || a.kin > kCandMaxKin)) || (!a.mip_mode && !a.intra_cost && !a.ang_cost) || (!a.modes && !a.costs))
    return hipErrorInvalidValue;
  // one workgroup of one wave per 64 CUs; its LDS is the 64 key rows
  const CandRow row = cand_row(a.ang_cost != nullptr, a.intra_cost != nullptr, a.mip_mode ? a.kin : 0);
  const long long grid = (a.total_cus + kCandLanes - 1) / kCandLanes;
  hipLaunchKernelGGL(candidates_kernel, dim3((unsigned)grid), dim3(kCandLanes), (size_t)kCandLanes * row.stride * sizeof(uint32_t), s, a);
  return hipGetLastError();
}

}  // namespace mipgpu

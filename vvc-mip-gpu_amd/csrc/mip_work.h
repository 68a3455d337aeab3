// mip_work.h -- the types and constants the host's work planner (work_plan.h) and the gfx950
// kernels share: work-list records, size classes, table layout.  No HIP dependency, so the
// planner compiles with any host compiler; mip_kernels.h includes it for the kernels.
#pragma once
#include <stdint.h>

namespace mipgpu {

// Work is organised per 64x64 quadrant of a CTU (no CU of the 47 shapes straddles a
// quadrant).  CUs of one size class (W x H; several shapes share a class) are grouped into
// wave *tasks*: up to 64/(S*V) CUs (S = W/4 column strips, V = row parts, see
// mip_search.hip) and a range of mode pairs; one lane per (CU, strip, row part) walks
// the pairs one after another.
struct Job {      // one CU of a task (geometry resolved on the host: no division in kernels)
  uint32_t cost;  // entry of mode 0 inside the CTU's cost block: shape offset + cu*2*modes
                  // (CU index in reference order, constants.h:1235-1354 / 1558-1631)
  uint8_t lx, ly; // CU origin inside the 64x64 quadrant
  uint16_t cu;    // CU index inside the CTU (reference order, 0..5379): decision entries
};
struct WaveTask {
  uint8_t cls;    // size class, kClassW/kClassH
  uint8_t ncu;    // CUs in the task
  uint8_t q0, q1; // mode pairs [q0, q1): pair q = modes 2q, 2q+1 (transposed when 2q >= modes)
  uint32_t cu0;   // first CU in the job array
};

// Size classes: W x H with V row parts per CU.  Classes 0-16 are the base class of each CU
// size (row parts: classes with few CUs per quadrant split each CU's rows over V lanes per
// strip so that a task still fills the wave); 17-20 are variants with more row parts, used
// for the remainder group of a class whose CU count per quadrant is not a multiple of its
// task size (e.g. 28 CUs of 32x8 = 3 tasks of 8 + one task of 4 CUs with V = 2; 84 CUs of
// 8x16 = 2 tasks of 32 + three tasks of 7, 7, 6 CUs with V = 4; 12 CUs of 32x16 = one task of
// 8 + one task of 4 with V = 2, classes 27-28).  21-26 are *transposed*
// classes (kClassTR): tasks of wide CUs (32x4, 16x4, 8x4, 32x8, 16x8 -- one upsampling
// direction only) searched as their tall transposes W x H listed here (mip_search.hip
// run_task; the CU position sets of a size and its transpose are transposes of each other).
constexpr int kNumClasses = 29;
constexpr int kNumBaseClasses = 17;
constexpr int kClassW[kNumClasses] = {64, 32, 32, 16, 32, 8, 16, 16, 8, 32, 4, 16, 4, 8, 8, 4, 4, 32, 16, 16, 8,
                                      4, 4, 4, 8, 8, 8, 32, 16};
constexpr int kClassH[kNumClasses] = {64, 32, 16, 32, 8, 32, 16, 8, 16, 4, 32, 4, 16, 8, 4, 8, 4, 8, 16, 8, 16,
                                      32, 16, 8, 32, 16, 16, 16, 32};
// MIP_SIX_WAVES: the search kernel's occupancy design.
//   3 (default since round 6): 12-wave workgroups, two per CU -- six waves per SIMD (80 VGPRs)
//     -- with the MIP tables and the next item's window in LDS beside a 768-word per-wave
//     scratch: 16x16 / 16x8 and the 64-slot 4x4 / 4x8 tasks produce their reduced predictions
//     in halves, 8xH tasks in quarters (mip_search.hip Geo, phase_a_half, walk_pairs_chunked).
//   0: 8-wave workgroups, two per CU, four waves per SIMD, 1280-word scratch (rounds 1-5): the
//     four-wave twin, or a whole four-wave library as an A/B baseline.
#ifndef MIP_SIX_WAVES
#define MIP_SIX_WAVES 3
#endif
#if MIP_SIX_WAVES != 3 && MIP_SIX_WAVES != 0
#error "MIP_SIX_WAVES must be 3 (12-wave workgroups, the default) or 0 (the four-wave design)"
#endif
constexpr int kClassV[kNumClasses] = {4, 2, 1, 2, 1, 1, 1, 1, 1, 1, 2, 1, 2, 1, 1, 1, 1, 2, 4, 2, 4,
                                      2, 2, 1, 1, 1, 4, 2, 4};
constexpr bool kClassTR[kNumClasses] = {false, false, false, false, false, false, false, false, false, false, false,
                                        false, false, false, false, false, false, false, false, false, false,
                                        true, true, true, true, true, true, false, false};
constexpr int kClassVariant[kNumClasses] = {-1, -1, 27, 28, 17, -1, 18, 19, 20, -1, -1, -1, -1, -1, -1, -1, -1,
                                            -1, -1, -1, -1, -1, -1, -1, -1, 26, -1, -1, -1};  // remainder-task class
// base class -> its transposed class (-1: searched as it is)
constexpr int kClassTransposed[kNumBaseClasses] = {-1, -1, -1, -1, 24, -1, -1, 25, -1, 21, -1, 22, -1, -1, 23, -1, -1};
constexpr int size_class(int w, int h) {  // base class of a CU size
  for (int i = 0; i < kNumBaseClasses; i++)
    if (kClassW[i] == w && kClassH[i] == h) return i;
  return -1;
}
constexpr int class_size_id(int w, int h) { return (w == 4 && h == 4) ? 0 : ((w == 4 || h == 4 || (w == 8 && h == 8)) ? 1 : 2); }
constexpr int class_slots(int cls) { return 64 / ((kClassW[cls] / 4) * kClassV[cls]); }

// Waves per search workgroup: two 12-wave workgroups share a CU in batched launches (MIP_SIX_WAVES
// 3; 8-wave ones with MIP_SIX_WAVES 0); small launches can run one 16-wave workgroup per CU
// instead ("wide"), whose waves share one item's tasks (launch_search).
constexpr int kSearchWaves = MIP_SIX_WAVES == 3 ? 12 : 8, kWideWaves = 16;
// Items per workgroup from which a launch is "large": it prefetches the next item's window and
// cuts the item queue into XCD chunks (launch_search); below it the host orders the items
// longest first and picks the slice count (mipgpu.cpp pick_work, work_plan.h), and alternating
// pipeline chunks run the four-wave twin (pipe_small).  One constant, so the host and the
// launcher never disagree about which launches are small.
constexpr int kPrefetchMinItems = 32;

// CTU variants (work_plan.h ctu_variants): CTUs with the same set of defined CUs share work /
// fill lists; the lists omit the CUs whose cost the reference leaves undefined.
constexpr int kMaxCtuVariants = 255;

// MIP matrices, restated for an exact f16 MFMA (mip_search.hip, phase A).  The reference
// computes pred_j = clamp(((32 - 32*sum_k p_k + sum_k p_k*w_jk) >> 6) + b0, 0, 1023) with
// p_k = b_k - b0 (p_0 = 0 for sizeId 2, 512 - b0 otherwise; intra.cl:415-482).  With
// w'_k = (w_jk - 32)/64 and a0 = 1 (sizeId 2; its matrix has no column for input 0) or
// (96 - w_j0)/64 (sizeId 1/0: p_0 = 512 - b0 folded), that is
//     pred_j = clamp(floor(C_j + a0*b0 + sum_{k>=1} w'_k (b_k - b0)))
// with C_j = 0.5 (sizeId 2) or 8*(w_j0 - 32) + 0.5.  The MFMA is fed x_k = 1024 + b_k (f16
// bit pattern 0x6400 | b_k, no conversion), so the stored coefficients are
//     A_j0 = a0 - sum_{k>=1} w'_k,   A_jk = w'_k (k >= 1),   C'_j = C_j - 1024 * sum_k A_jk.
// All values are multiples of 1/64 below 2^5 (f16-exact); every partial sum stays below
// 2^18 in units of 1/64, so the f32 accumulation is exact.
//   f16 rows [768][8], row = base(sizeId) + mode*R*R + j, base = 0 / 384 / 512 for sizeId
//   2 / 1 / 0 (sizeId 0: 4 inputs, halves 4..7 zero).
//   f32 rows [388] (sizeId 1 and 0, from row 384): C'_j; then 4 x kAccInitS2, the sizeId 2
//   C' = 0.5 - 1024 of every row (read from LDS so it stays in registers).
constexpr float kAccInitS2 = 0.5f - 1024.0f;
constexpr int kWeightRows = 768, kWeightRowOffS1 = 384, kWeightRowOffS0 = 512;
constexpr int kCtabRows = 384 + 4;  // + 4 copies of kAccInitS2 (row 384..387)
constexpr int kTableBytes = kWeightRows * 16 + kCtabRows * 4;

// One CU searched by the exact per-CU kernel (fixup_kernel): alternative references whose
// samples may exceed 10 bits (work_plan.h reads_last_columns).
struct FixupCu {
  uint32_t ctu;
  uint16_t cu;     // CU index inside the CTU (reference order, 0..5379)
  uint8_t shape;
  uint8_t pad;
};

}  // namespace mipgpu

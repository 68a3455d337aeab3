// pknorm_probe.hip -- can the search kernel's phase A clip its reduced predictions while it
// converts them?  v_cvt_pknorm_u16_f32 turns two f32 values x in [0, 1] into two u16 values
// x * 65535, saturating at both ends, so with the MFMA delivering x = (D + beta) / 1024 (D the
// unclipped reduced sample, a multiple of 1/64) a packed shift right by 6 would leave
// min(max(floor(D), 0), 1023) in both halves: two instructions for two samples, like the two
// v_cvt_u32_f32 of today, and no clip on any read.  Two things have to hold on the hardware:
//
//  1. Conversion.  For every f32 x = j * 2^-17, j in [-2^23, 2^23), both halves of
//     pknorm(x, x') >> 6 are compared with clip(floor(1024 x - beta), 0, 1023), for
//     beta = 2^-7 and beta = 2^-6.  1024 x - beta is a multiple of 1/64 -- a value the kernel can
//     produce -- exactly for the odd j with beta = 2^-7 and for the even j with beta = 2^-6; on
//     the other half of the grid x * 65535 sits a hair below an integer or a half-integer
//     (j = 128 k is x = k / 1024, x * 65535 = 64 k - k / 1024), where no rounding rule can
//     return floor(1024 x - beta), so a zero count over the whole grid is impossible for any
//     hardware.  The probe prints both counts per beta; the verdict is the count over the
//     kernel's values.
//  2. MFMA.  v_mfma_f32_16x16x16f16 with the real table rows, B = 1 + b / 1024 (f16 bits
//     0x3C00 | b) and C = (C' + beta) * 2^-10, in phase A's block-diagonal operand layout (mode
//     X in K rows 0..7, mode Y in K rows 8..15), must return (D + beta) / 1024 bit for bit, D
//     from integer arithmetic on the host (mip_work.h).  All three size ids, 65 536 random
//     boundary vectors per K half, and the all-0 and all-1023 vectors against every table row.
//
// Exit status 0: some beta passes both.  Built by the engine's Makefile to bin/pknorm_probe.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "work_plan.h"

#define CHECK(x)                                                                \
  do {                                                                          \
    hipError_t e_ = (x);                                                        \
    if (e_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(2);                                                                  \
    }                                                                           \
  } while (0)

typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned short u2 __attribute__((ext_vector_type(2)));

using namespace mipgpu;

__host__ __device__ inline uint32_t hash32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// ---- 1. conversion --------------------------------------------------------------------------
constexpr int kGridBits = 24;  // j + 2^23 in [0, 2^24)
__host__ __device__ inline int clip10(int v) { return v < 0 ? 0 : v > 1023 ? 1023 : v; }
// clip(floor(1024 x - beta)) for x = j * 2^-17: 1024 x = j / 128, beta = bu / 128
__host__ __device__ inline int want_of(int j, int bu) { return clip10((j - bu) >> 7); }

// counts[4 * b + 0 / 1]: mismatches over the whole grid / over the kernel's values, beta index b
// (0: 2^-7, values = odd j; 1: 2^-6, values = even j); first[b]: one mismatching j of the latter
__global__ __launch_bounds__(256) void convert_probe(unsigned *counts, int *first) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  const int j0 = (int)t - (1 << 23), j1 = (int)(t ^ 0x2a5u) - (1 << 23);  // the pair's other value
  const float x0 = ldexpf((float)j0, -17), x1 = ldexpf((float)j1, -17);
  const u2 pk = __builtin_bit_cast(u2, __builtin_amdgcn_cvt_pknorm_u16(x0, x1)) >> (u2){6, 6};
#pragma unroll
  for (int b = 0; b < 2; b++) {
    const int bu = b + 1;  // beta in units of 2^-7
    const bool bad0 = pk.x != want_of(j0, bu), bad1 = pk.y != want_of(j1, bu);
    // each j is the low half of exactly one thread and the high half of exactly one
    if (bad0) atomicAdd(counts + 4 * b, 1u);
    if (bad1) atomicAdd(counts + 4 * b + 2, 1u);
    const bool mine0 = (j0 & 1) == (b == 0), mine1 = (j1 & 1) == (b == 0);
    if (bad0 && mine0) atomicAdd(counts + 4 * b + 1, 1u), first[b] = j0;
    if (bad1 && mine1) atomicAdd(counts + 4 * b + 3, 1u), first[b] = j1;
  }
}

// ---- 2. MFMA --------------------------------------------------------------------------------
struct SizeId {
  int sid, wbase, modes, nout, nin;
};
constexpr SizeId kSizes[3] = {{2, 0, 6, 64, 8}, {1, kWeightRowOffS1, 8, 16, 8}, {0, kWeightRowOffS0, 16, 16, 4}};
constexpr int kRandomWaves = 65536 / 8;  // 8 columns per K half and wave

// boundary sample `k` of column n of wave w; the last `nblk` waves carry the all-0 (columns
// 0..7) and all-1023 (8..15) vectors against row block w - kRandomWaves of both K halves
__host__ __device__ inline int sample(uint32_t seed, int w, int n, int k) {
  if (w >= kRandomWaves) return n < 8 ? 0 : 1023;
  return (int)(hash32(seed ^ (uint32_t)((w * 16 + n) * 8 + k)) & 1023u);
}
__host__ __device__ inline void row_blocks(uint32_t seed, int w, int nblk, int &bx, int &by) {
  if (w >= kRandomWaves) {
    bx = by = w - kRandomWaves;
  } else {
    bx = (int)(hash32(seed + 0x9e3779b9u * (uint32_t)w) % (uint32_t)nblk);
    by = (int)(hash32(seed + 0x85ebca6bu * (uint32_t)w + 1u) % (uint32_t)nblk);
  }
}

// one wave = one product: lane l holds A[l & 15][4 (l >> 4)..+3], B[4 (l >> 4)..+3][l & 15] and
// gets D[4 (l >> 4)..+3][l & 15].  Column n belongs to K half n & 1 (phase A: mode 2q + (n & 1)).
__global__ __launch_bounds__(64) void mfma_probe(const uint8_t *tab, SizeId s, uint32_t seed, int bu, float *out) {
  const int l = threadIdx.x, w = blockIdx.x, r = l & 15, h = l >> 4;
  const int nblk = s.modes * s.nout / 16;
  int bx, by;
  row_blocks(seed, w, nblk, bx, by);
  const int blk = h >> 1 ? by : bx;  // K rows 4h..4h+3: half h >> 1, inputs 4 (h & 1)..+3
  const h4 a = *reinterpret_cast<const h4 *>(tab + ((s.wbase + blk * 16 + r) * 8 + 4 * (h & 1)) * 2);
  h4 b;
  for (int i = 0; i < 4; i++) {
    const uint16_t bits = (h >> 1) == (r & 1) ? (uint16_t)(0x3C00 | sample(seed, w, r, 4 * (h & 1) + i)) : 0;
    b[i] = __builtin_bit_cast(_Float16, bits);
  }
  const float *ctab = reinterpret_cast<const float *>(tab + kWeightRows * 16);
  const float beta = (float)bu * (1.0f / 128.0f);
  f4 c;
  for (int i = 0; i < 4; i++) {
    const float cp = s.sid == 2 ? ctab[384] : ctab[s.wbase - kWeightRowOffS1 + (r & 1 ? by : bx) * 16 + 4 * h + i];
    c[i] = (cp + beta) * (1.0f / 1024.0f);
  }
  const f4 d = __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0);
  for (int i = 0; i < 4; i++) out[((size_t)w * 64 + l) * 4 + i] = d[i];
}

static float half_to_float(uint16_t v) {  // the tables' values: normal or zero
  const uint32_t e = (v >> 10) & 31, m = v & 1023;
  if (e == 0) return 0.0f;
  const float f = ldexpf((float)(1024 + m), (int)e - 25);
  return v & 0x8000 ? -f : f;
}

int main() {
  // ---- 1
  unsigned *d_counts;
  int *d_first;
  CHECK(hipMalloc(&d_counts, 8 * sizeof(unsigned)));
  CHECK(hipMalloc(&d_first, 2 * sizeof(int)));
  CHECK(hipMemset(d_counts, 0, 8 * sizeof(unsigned)));
  CHECK(hipMemset(d_first, 0, 2 * sizeof(int)));
  hipLaunchKernelGGL(convert_probe, dim3((1u << kGridBits) / 256), dim3(256), 0, 0, d_counts, d_first);
  CHECK(hipGetLastError());
  unsigned counts[8];
  int first[2];
  CHECK(hipMemcpy(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(first, d_first, sizeof first, hipMemcpyDeviceToHost));
  bool conv_ok[2];
  for (int b = 0; b < 2; b++) {
    const unsigned grid = counts[4 * b] + counts[4 * b + 2], mine = counts[4 * b + 1] + counts[4 * b + 3];
    conv_ok[b] = mine == 0;
    printf("convert beta=2^-%d: %u mismatches over the kernel's values (%s j, 2 x %d), %u over the whole grid (2 x %d)",
           7 - b, mine, b == 0 ? "odd" : "even", 1 << (kGridBits - 1), grid, 1 << kGridBits);
    if (mine) printf("; e.g. j = %d", first[b]);
    printf("\n");
  }

  // ---- 2
  const std::vector<uint8_t> tab = build_tables();
  const uint16_t *wt = reinterpret_cast<const uint16_t *>(tab.data());
  const float *ctab = reinterpret_cast<const float *>(tab.data() + kWeightRows * 16);
  uint8_t *d_tab;
  CHECK(hipMalloc(&d_tab, tab.size()));
  CHECK(hipMemcpy(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice));
  const int max_waves = kRandomWaves + 24;
  float *d_out;
  CHECK(hipMalloc(&d_out, (size_t)max_waves * 64 * 4 * sizeof(float)));
  std::vector<float> out((size_t)max_waves * 64 * 4);
  bool mfma_ok[2] = {true, true};
  for (int b = 0; b < 2; b++) {
    const int bu = b + 1;
    for (const SizeId &s : kSizes) {
      const int nblk = s.modes * s.nout / 16, waves = kRandomWaves + nblk;
      const uint32_t seed = 0x5eed0000u + (uint32_t)s.sid * 16 + (uint32_t)b;
      hipLaunchKernelGGL(mfma_probe, dim3(waves), dim3(64), 0, 0, d_tab, s, seed, bu, d_out);
      CHECK(hipGetLastError());
      CHECK(hipMemcpy(out.data(), d_out, (size_t)waves * 64 * 4 * sizeof(float), hipMemcpyDeviceToHost));
      long long bad[2] = {0, 0}, total[2] = {0, 0}, above = 0, below = 0;
      for (int w = 0; w < waves; w++) {
        int bx, by;
        row_blocks(seed, w, nblk, bx, by);
        for (int n = 0; n < 16; n++) {
          const int half = n & 1, blk = half ? by : bx;
          for (int j = 0; j < 16; j++) {
            const int row = s.wbase + blk * 16 + j;
            // D in units of 1/64: C' + sum_k A_jk (1024 + b_k), integers throughout
            const float cp = s.sid == 2 ? ctab[384] : ctab[s.wbase - kWeightRowOffS1 + blk * 16 + j];
            long long d64 = llrintf(cp * 64.0f);
            for (int k = 0; k < 8; k++)
              d64 += (long long)lrintf(half_to_float(wt[row * 8 + k]) * 64.0f) * (1024 + sample(seed, w, n, k));
            const float want = ldexpf((float)(2 * d64 + bu), -17);  // (D + beta) / 1024; |2 d64 + bu| < 2^24
            const float got = out[((size_t)w * 64 + (j >> 2) * 16 + n) * 4 + (j & 3)];
            total[half]++;
            above += d64 >= 1024 * 64;
            below += d64 < 0;
            if (memcmp(&got, &want, 4) != 0) {
              if (bad[0] + bad[1] < 3)
                printf("  sizeId %d wave %d row %d column %d: got %.9g want %.9g\n", s.sid, w, row, n, got, want);
              bad[half]++;
            }
          }
        }
      }
      if (bad[0] + bad[1]) mfma_ok[b] = false;
      printf("mfma beta=2^-%d sizeId %d: %lld of %lld (K rows 0..7) and %lld of %lld (K rows 8..15) results differ "
             "from (D + beta) / 1024; D > 1023 in %lld, D < 0 in %lld\n",
             7 - b, s.sid, bad[0], total[0], bad[1], total[1], above, below);
    }
  }
  int pick = -1;
  for (int b = 0; b < 2; b++)
    if (pick < 0 && conv_ok[b] && mfma_ok[b]) pick = b;
  if (pick < 0) {
    printf("verdict: no beta is exact\n");
    return 1;
  }
  printf("verdict: beta=2^-%d is exact\n", 7 - pick);
  return 0;
}

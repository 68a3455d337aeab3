// mip_predict_angular_tap4.hip -- angular block output with VVC's 4-tap cubic / Gaussian luma
// interpolation (gfx950), contract in include/mipgpu.h (mip_angular_interp, MIP_ANG_INTERP_4TAP).
// No reference counterpart.  angular_tap4_predict_kernel is angular_ext_predict_kernel
// (mip_predict_angular_ext.hip), which stays as it is: the same scan of the list, the same
// compaction, the same write rule (predict_rule.h, the same function), the same split into small
// and large blocks, the same per-item line ref[-S .. M + E] and the same stores, read there.  It
// serves both mip_angular_refs settings: without a length table (a.ext == NULL, the substituted
// lines) every E is 0.
//
// What is new is the sample: the four taps line[S + k-1 .. S + k+2] with the coefficient word of
// (G, f), G the item's (wave- or group-uniform), f the sample's, from 64 words staged in LDS once
// per workgroup (angular_plan.h ang_coef_word).  No longer line is needed: k >= 1 - S (|A| <= 32,
// so idx >= -S), hence k - 1 >= -S is line[0], which the line step already fills with ref[-S] -- the
// side projection at its cap for A < 0 -- and line[S] is ref[0], the corner, for every angle; taps
// past M + E are clamped to line[S + M + E] like the 2-tap predictor's.  DESIGN.md section 5.12.
#include <algorithm>

#include "angular_plan.h"
#include "mip_kernels.h"
#include "mip_tables.h"
#include "predict_rule.h"

namespace mipgpu {
namespace {

__constant__ mip_shape_desc x_shapes[MIP_NUM_SHAPES] = MIP_SHAPE_TABLE;

constexpr int kExtPredWaves = 4;             // waves per workgroup
constexpr int kExtPredEntriesPerWave = 64;   // list entries a wave scans per pass (one per lane)
constexpr int kExtPredGroupsCap = 1024;      // workgroups, whatever the device
// Wave-private LDS words.  A group of G lanes keeps
//   top[G] left[G] line[3G + 4]      (line[S + k] = ref[k], k = -S .. M + E, M + S <= 2G, E <= S <= G)
constexpr int ext_lds_words(int g) { return 5 * g + 4; }
constexpr int kExtGroupWords = ext_lds_words(16);                                 // 84
constexpr int kExtWaveWords = std::max(ext_lds_words(64), 4 * kExtGroupWords);    // 336
static_assert(kExtWaveWords % 4 == 0 && kExtGroupWords % 4 == 0, "LDS layout");

// LDS fence for data handed between lanes of ONE wave.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int ilog2i(int v) { return 31 - __clz(v); }

struct ExtShapes {
  __device__ __forceinline__ mip_shape_desc operator()(int s) const { return x_shapes[s]; }
};

struct FrameRef {
  const uint16_t *f;
  int width;
  __device__ __forceinline__ int operator()(int row, int col) const { return f[(size_t)row * width + col]; }
};

struct StagedBound {
  const int *top, *left;
  int w, h, c;
  __device__ __forceinline__ int sample(bool top_line, int t) const { return top_line ? top[t] : left[t]; }
  __device__ __forceinline__ int corner() const { return c; }
};

// V consecutive samples of output row yy from column xx (multiple of V), from the mode's line of
// main length M1 = M + E.
template <int V>
__device__ __forceinline__ void store_angular(const Item &c, const AngMode &md, const int *top, const int *left, const int *line,
                                              int corner, int M1, const uint32_t *coef, int t, int step, uint16_t *out) {
  const int w = c.w, lw = ilog2i(w), lh = ilog2i(c.h);
  const int lu = lw - (V == 8 ? 3 : 2);  // log2 of the lane units per row
  const int units = (c.h * w) >> (V == 8 ? 3 : 2);
  const bool vert = md.m >= 34, pdpc = md.m == 18 || md.m == 50;
  const int S = vert ? c.h : w, scale = (lw + lh - 2) >> 2;
  coef += ang_filter_gauss(md.m, lw, lh) ? 32 : 0;  // (the item's table)
  for (int u = t; u < units; u += step) {
    const int yy = u >> lu, xx = (u & ((1 << lu) - 1)) * V;
    int v[V];
#pragma unroll
    for (int q = 0; q < V; q++) {
      const int i = xx + q, a = vert ? i : yy, bb = vert ? yy : i;
      const int d = (bb + 1) * md.angle, idx = d >> 5, f = d & 31, k = a + idx + 1;  // k >= 1 - S: k - 1 is line[0] at least
      const int r0 = line[S + (k - 1 < M1 ? k - 1 : M1)], r1 = line[S + (k < M1 ? k : M1)];
      const int r2 = line[S + (k + 1 < M1 ? k + 1 : M1)], r3 = line[S + (k + 2 < M1 ? k + 2 : M1)];
      int p = ang_tap4(coef[f], r0, r1, r2, r3);
      if (pdpc) {
        const int wgt = intra_pdpc_weight(a, scale);
        const int side = (vert ? left[bb] : top[bb]) - corner + p;
        p = (side * wgt + (64 - wgt) * p + 32) >> 6;
      }
      v[q] = ang_clip(p);
    }
    uint16_t *dst = out + c.offset + (long long)yy * c.pitch + xx;
    if constexpr (V == 8) {
      *reinterpret_cast<uint4 *>(dst) = make_uint4((uint32_t)v[0] | (uint32_t)v[1] << 16, (uint32_t)v[2] | (uint32_t)v[3] << 16,
                                                   (uint32_t)v[4] | (uint32_t)v[5] << 16, (uint32_t)v[6] | (uint32_t)v[7] << 16);
    } else {
      *reinterpret_cast<uint2 *>(dst) = make_uint2((uint32_t)v[0] | (uint32_t)v[1] << 16, (uint32_t)v[2] | (uint32_t)v[3] << 16);
    }
  }
}

// Prediction of one angular item by a group of G lanes (t = lane inside the group, L = the
// group's LDS words, ext = the CU's E_top | E_left << 8).  Called by whole waves: lanes of groups
// without an item run it with c.on = false (no memory access).
template <int G>
__device__ __forceinline__ void predict_angular_cu(const PredictTap4Args &a, const Item &c, uint32_t ext, const uint32_t *coef, int t, int *L) {
  int *top = L, *left = L + G, *line = L + 2 * G;
  const int w = c.w, h = c.h;
  const AngMode md = ang_unpack(ang_pack(c.on ? c.mode - MIP_MODE_ANGULAR(0) : MIP_ANGULAR_LAST));
  const bool vert = md.m >= 34;
  const int M = vert ? w : h, S = vert ? h : w;
  // the main line's extension: at most S samples, all inside the frame's row y-1 / column x-1
  const int room = vert ? (c.y > 0 ? a.width - (c.x + w) : 0) : (c.x > 0 ? a.height - (c.y + h) : 0);
  const int E = c.on ? min(min((int)(vert ? ext & 0xffu : ext >> 8 & 0xffu), S), max(room, 0)) : 0;
  int corner = 0;
  if (c.on) {  // complete boundaries and the corner, by linear index (the CU is available: all inside the frame)
    const FrameRef ref{a.refs + (size_t)c.frame * a.width * a.height, a.width};
    if (t < w) top[t] = intra_top(ref, c.x, c.y, t);
    if (t < h) left[t] = intra_left(ref, c.x, c.y, t);
    corner = AngBound<FrameRef>{ref, c.x, c.y, w, h}.corner();
    // line[S + M + 1 + e] = ref[M + 1 + e] = main[M + e], e < E (E > 0 only with y > 0 / x > 0)
    for (int e = t; e < E; e += G) line[S + M + 1 + e] = vert ? ref(c.y - 1, c.x + M + e) : ref(c.y + M + e, c.x - 1);
  }
  wave_lds_sync();
  if (c.on) {  // line[S + k] = ref[k], k = -S .. M
    const StagedBound b{top, left, w, h, corner};
    for (int e = t; e <= M + S; e += G)
      line[e] = vert ? ang_ref<true>(b, e - S, md.inv, corner) : ang_ref<false>(b, e - S, md.inv, corner);
  }
  wave_lds_sync();
  if (c.on) {
    // 16-byte stores where every row segment of the block is 16-byte aligned
    const bool wide = w >= 8 && (c.pitch & 7) == 0 && ((reinterpret_cast<uintptr_t>(a.out + c.offset) & 15) == 0);
    if (wide) store_angular<8>(c, md, top, left, line, corner, M + E, coef, t, G, a.out);
    else store_angular<4>(c, md, top, left, line, corner, M + E, coef, t, G, a.out);
  }
  wave_lds_sync();  // the next item rewrites the group's words
}

// The fields of lane src's item that the prediction needs (sid, modes and reg are predict_kernel's).
__device__ __forceinline__ Item take_item(const Item &c, int src) {
  Item u{};
  u.reg = false;
  u.frame = __shfl(c.frame, src, 64);
  u.x = __shfl(c.x, src, 64);
  u.y = __shfl(c.y, src, 64);
  const int wh = __shfl(c.w | c.h << 8, src, 64);
  u.w = wh & 0xff;
  u.h = wh >> 8;
  u.mode = __shfl(c.mode, src, 64);
  u.pitch = __shfl(c.pitch, src, 64);
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)c.offset, src, 64), hi = (uint32_t)__shfl((int)(c.offset >> 32), src, 64);
  u.offset = (long long)(((unsigned long long)hi << 32) | lo);
  return u;
}

__global__ __launch_bounds__(64 * kExtPredWaves) void angular_tap4_predict_kernel(PredictTap4Args a) {
  __shared__ __attribute__((aligned(16))) int lds[kExtPredWaves * kExtWaveWords];
  __shared__ uint32_t s_coef[kAngCoefWords];
  if (threadIdx.x < kAngCoefWords) s_coef[threadIdx.x] = a.coef[threadIdx.x];
  __syncthreads();  // (the only workgroup barrier: the waves go their own ways below)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, grp = lane >> 4;
  int *wl = lds + wv * kExtWaveWords;
  const long long rows = (a.n + kExtPredEntriesPerWave - 1) / kExtPredEntriesPerWave;
  for (long long r = (long long)blockIdx.x * kExtPredWaves + wv; r < rows; r += (long long)gridDim.x * kExtPredWaves) {
    const long long idx = r * kExtPredEntriesPerWave + lane;  // the lane's entry
    Item c{};
    c.on = c.reg = false;
    int ext = 0;
    if (idx < a.n && pred_mode_is_angular(a.items[idx].mode)) {  // (padding: this one load)
      const mip_pred_item it = a.items[idx];  // (one reading of the entry: its cu names the table's)
      c = pred_decode<false, true>(a, it, ExtShapes{});
      if (c.on && a.ext) ext = a.ext[it.cu];  // (the write rule has checked it.cu; no table: the substituted lines)
    }
    const unsigned long long emit = __ballot(c.on);
    if (!emit) continue;  // wave-uniform
    // predict_kernel counted these items as not written; they are written below
    if (lane == 0 && a.skipped) atomicSub(a.skipped, (unsigned)__popcll(emit));
    unsigned long long large = __ballot(c.on && c.w * c.h > 64), small = emit & ~large;
    while (small) {  // up to four small blocks, one per 16-lane group
      int src = -1;
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int s = small ? __ffsll((long long)small) - 1 : -1;
        small &= small - (small != 0);
        if (grp == g) src = s;
      }
      Item u = take_item(c, src < 0 ? 0 : src);
      u.on = src >= 0;
      predict_angular_cu<16>(a, u, (uint32_t)__shfl(ext, src < 0 ? 0 : src, 64), s_coef, lane & 15, wl + grp * kExtGroupWords);
    }
    while (large) {  // larger blocks, one per wave
      const int src = __ffsll((long long)large) - 1;
      large &= large - 1;
      Item u = take_item(c, src);
      u.on = true;
      predict_angular_cu<64>(a, u, (uint32_t)__shfl(ext, src, 64), s_coef, lane, wl);
    }
  }
}

}  // namespace

hipError_t launch_predict_angular_tap4(const PredictTap4Args &a, hipStream_t s) {
  if (a.n < 1) return hipSuccess;
  if (!a.refs || !a.items || !a.out || !a.unavail || !a.geo || a.n > (1LL << 31) - 256) return hipErrorInvalidValue;
  // grid-stride over the list: 256 entries per workgroup pass, a fixed cap on the workgroups
  const long long per_group = (long long)kExtPredWaves * kExtPredEntriesPerWave;
  const long long groups = std::min<long long>((a.n + per_group - 1) / per_group, kExtPredGroupsCap);
  hipLaunchKernelGGL(angular_tap4_predict_kernel, dim3((unsigned)groups), dim3(64 * kExtPredWaves), 0, s, a);
  return hipGetLastError();
}

}  // namespace mipgpu

// mip_predict_angular.hip -- angular block output: the predicted samples of the list items whose
// mode is an angular code MIP_MODE_ANGULAR(2..66) (gfx950), contract in include/mipgpu.h
// (mip_predict_device_ex, MIP_PRED_ANGULAR; mip_angular_refs; mip_angular_interp).  No reference
// counterpart.  The second kernel of a prediction call with that flag: predict_kernel
// (mip_predict.hip) has already run over the same list on the same stream, has emitted the MIP /
// Planar / DC items and has counted every angular item as skipped; this kernel emits the angular
// items and takes them off the count again, so that in stream order the word ends as "items not
// written".
//
// One body (angular_predict_items) holds the scan; a kernel is that body with a policy for the
// item's line and sample (Line2, ExtLine2, ExtLine4 below):
//   angular_predict_kernel        substituted lines, 2-tap
//   angular_ext_predict_kernel    extended lines (a.ext), 2-tap
//   angular_tap4_predict_kernel   either (a.ext or NULL: every E is 0), 4-tap
//
// Scan and compact.  The list a partition writes is mostly padding, so a wave reads 64 entries
// per pass, one lane each and only the 4-byte `mode` word; a lane whose word is an angular code
// loads the whole entry once and checks it against the write rule (predict_rule.h, the function
// predict_kernel runs).  A ballot of the accepted lanes gives the pass's work; padding costs its
// one load and nothing else.  The wave then works through the set bits with predict_kernel's
// wave-uniform split: blocks of at most 64 samples four at a time, one per 16-lane group, larger
// blocks one per wave, the item's fields handed over by lane shuffles.
//
// Per item, in the group's wave-private LDS words (wave-level fences only, all in wave-uniform
// control flow): top[w] and left[h] with intra_plan.h's boundary rules and the corner with
// AngBound's; then the mode's projected extended reference line ref[-S .. M] (angular_plan.h
// ang_ref over the staged boundaries, at most 129 words), built once; then every lane builds 8 (or
// 4) consecutive samples of an output row -- two LDS reads and the 2-tap blend per sample, PDPC for
// modes 18 and 50, the clip -- and stores them with one 16-byte (8-byte) store, as predict_kernel
// does.  The values are ang_sample's: the line holds ref[k] for every k a sample can ask for, a
// read past M is clamped to ref[M] as ang_ref clamps it, and the blend with f = 0 is ref itself.
//
// Extended lines.  A lane that has accepted its entry reads its CU's two lengths from the engine's
// table (a.ext, mip_extended_refs for the call's availability set) and hands them over with the
// item.  The group builds ref[-S .. M] as before and then ref[M+1 .. M+E] from the item's frame by
// linear index -- the main line's E real samples past its end -- so the line is ref[-S .. M + E], at
// most 3G + 4 words behind top[G] and left[G]: 5G + 4 words per group.  A sample's read past M + E
// is clamped to ref[M + E].  The lengths are data: E is cut to the side's length S (the line's
// room) and to the frame's right or bottom edge (the reads' room) before use.  DESIGN.md section
// 5.11.
//
// Four taps.  The sample takes line[S + k-1 .. S + k+2] with the coefficient word of (G, f), G the
// item's (wave- or group-uniform), f the sample's, from 64 words staged in LDS once per workgroup
// (angular_plan.h ang_coef_word) behind the file's only workgroup barrier, before the scan: the
// waves go their own ways after it.  No longer line is needed: k >= 1 - S (|A| <= 32, so idx >= -S),
// hence k - 1 >= -S is line[0], which the line step already fills with ref[-S] -- the side
// projection at its cap for A < 0 -- and line[S] is ref[0], the corner, for every angle; taps past
// M + E are clamped to line[S + M + E] like the 2-tap predictor's.  DESIGN.md section 5.12.
//
// LDS banks: a vertical-class lane reads line[S + i + idx(j) + 1 ..] at consecutive words for
// consecutive columns.  In the horizontal class the index is S + j + idx(i) + 1 with idx(i) =
// ((i + 1) * A) >> 5: for one read of the wave the lanes cover a few rows j and eight (or four)
// column phases, so the addresses span at most 8 + 64 words of a 129-word line -- two of them
// share a bank only across that span's end, equal addresses are broadcast.  No padding is needed.
//
// The list is data in device memory: every index below comes from an item that passed the write
// rule; a bad entry reads no sample and writes nothing.  DESIGN.md section 5.8.
#include <algorithm>

#include "angular_plan.h"
#include "mip_kernels.h"
#include "mip_tables.h"
#include "predict_rule.h"

namespace mipgpu {
namespace {

__constant__ mip_shape_desc a_shapes[MIP_NUM_SHAPES] = MIP_SHAPE_TABLE;

constexpr int kAngPredWaves = 4;             // waves per workgroup
constexpr int kAngPredEntriesPerWave = 64;   // list entries a wave scans per pass (one per lane)
constexpr int kAngPredGroupsCap = 1024;      // workgroups, whatever the device: one round is 262 144 entries

// LDS fence for data handed between lanes of ONE wave.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int ilog2i(int v) { return 31 - __clz(v); }

struct AngShapes {
  __device__ __forceinline__ mip_shape_desc operator()(int s) const { return a_shapes[s]; }
};

// One frame of the reference source as a Ref of intra_plan.h.
struct FrameRef {
  const uint16_t *f;
  int width;
  __device__ __forceinline__ int operator()(int row, int col) const { return f[(size_t)row * width + col]; }
};

// The staged boundaries as a Bound of angular_plan.h.
struct StagedBound {
  const int *top, *left;
  int w, h, c;
  __device__ __forceinline__ int sample(bool top_line, int t) const { return top_line ? top[t] : left[t]; }
  __device__ __forceinline__ int corner() const { return c; }
};

// ---- what differs between the variants: the wave-private words of a group of G lanes (64: the
// wave, 16: a quarter), the length table, and the sample from the mode's line.  A group keeps
//   top[G] left[G] line[2G + 4]      (line[S + k] = ref[k], k = -S .. M, M + S <= 2G)
//   top[G] left[G] line[3G + 4]      with the extension: k = -S .. M + E, E <= S <= G
// sample(): line points at ref[0], last is the line's last k (M + E), coef the item's 32 words.
enum class ExtTable { none, required, optional };
struct Line2 {
  static constexpr int words(int g) { return 4 * g + 4; }
  static constexpr ExtTable kExt = ExtTable::none;
  static constexpr bool kCoef = false;
  __device__ static __forceinline__ int sample(const int *line, int k, int last, int f, const uint32_t *) {
    const int r0 = line[k < last ? k : last], r1 = line[k + 1 < last ? k + 1 : last];
    return ((32 - f) * r0 + f * r1 + 16) >> 5;  // (f == 0: r0, the samples are not negative)
  }
};
struct ExtLine2 : Line2 {
  static constexpr int words(int g) { return 5 * g + 4; }
  static constexpr ExtTable kExt = ExtTable::required;
};
struct ExtLine4 : ExtLine2 {
  static constexpr ExtTable kExt = ExtTable::optional;
  static constexpr bool kCoef = true;
  __device__ static __forceinline__ int sample(const int *line, int k, int last, int f, const uint32_t *coef) {  // k >= 1 - S: k - 1 is line[-S] at least
    const int r0 = line[k - 1 < last ? k - 1 : last], r1 = line[k < last ? k : last];
    const int r2 = line[k + 1 < last ? k + 1 : last], r3 = line[k + 2 < last ? k + 2 : last];
    return ang_tap4(coef[f], r0, r1, r2, r3);
  }
};
template <class Line>
constexpr int group_words() { return Line::words(16); }  // 68, 84
template <class Line>
constexpr int wave_words() { return std::max(Line::words(64), 4 * group_words<Line>()); }  // 272, 336

// V consecutive samples of output row yy from column xx (multiple of V), from the mode's line of
// main length M1 = M + E.
template <int V, class Line>
__device__ __forceinline__ void store_angular(const Item &c, const AngMode &md, const int *top, const int *left, const int *line,
                                              int corner, int M1, const uint32_t *coef, int t, int step, uint16_t *out) {
  const int w = c.w, lw = ilog2i(w), lh = ilog2i(c.h);
  const int lu = lw - (V == 8 ? 3 : 2);  // log2 of the lane units per row
  const int units = (c.h * w) >> (V == 8 ? 3 : 2);
  const bool vert = md.m >= 34, pdpc = md.m == 18 || md.m == 50;
  const int S = vert ? c.h : w, scale = (lw + lh - 2) >> 2;
  if constexpr (Line::kCoef) coef += ang_filter_gauss(md.m, lw, lh) ? 32 : 0;  // (the item's table)
  for (int u = t; u < units; u += step) {
    const int yy = u >> lu, xx = (u & ((1 << lu) - 1)) * V;
    int v[V];
#pragma unroll
    for (int q = 0; q < V; q++) {
      const int i = xx + q, a = vert ? i : yy, bb = vert ? yy : i;
      const int d = (bb + 1) * md.angle, idx = d >> 5, f = d & 31, k = a + idx + 1;  // k >= 1 - S
      int p = Line::sample(line + S, k, M1, f, coef);
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
// without an item run it with c.on = false (no memory access), so that the fences sit in
// wave-uniform control flow.
template <int G, class Line, class Args>
__device__ __forceinline__ void predict_angular_cu(const Args &a, const Item &c, uint32_t ext, const uint32_t *coef, int t, int *L) {
  int *top = L, *left = L + G, *line = L + 2 * G;
  const int w = c.w, h = c.h;
  const AngMode md = ang_unpack(ang_pack(c.on ? c.mode - MIP_MODE_ANGULAR(0) : MIP_ANGULAR_LAST));
  const bool vert = md.m >= 34;
  const int M = vert ? w : h, S = vert ? h : w;
  int E = 0;
  if constexpr (Line::kExt != ExtTable::none) {
    // the main line's extension: at most S samples, all inside the frame's row y-1 / column x-1
    const int room = vert ? (c.y > 0 ? a.width - (c.x + w) : 0) : (c.x > 0 ? a.height - (c.y + h) : 0);
    E = c.on ? min(min((int)(vert ? ext & 0xffu : ext >> 8 & 0xffu), S), max(room, 0)) : 0;
  }
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
    if (wide) store_angular<8, Line>(c, md, top, left, line, corner, M + E, coef, t, G, a.out);
    else store_angular<4, Line>(c, md, top, left, line, corner, M + E, coef, t, G, a.out);
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

// The body of the three kernels.  The argument struct comes by const reference (by value it would
// be copied to private memory).  An instantiation that does not name s_coef does not have it.
template <class Line, class Args>
__device__ __forceinline__ void angular_predict_items(const Args &a) {
  constexpr int kWaveWords = wave_words<Line>(), kGroupWords = group_words<Line>();
  static_assert(kWaveWords % 4 == 0 && kGroupWords % 4 == 0, "LDS layout");
  __shared__ __attribute__((aligned(16))) int lds[kAngPredWaves * kWaveWords];
  __shared__ uint32_t s_coef[kAngCoefWords];
  const uint32_t *coef = nullptr;
  if constexpr (Line::kCoef) {
    if (threadIdx.x < kAngCoefWords) s_coef[threadIdx.x] = a.coef[threadIdx.x];
    __syncthreads();  // (the only workgroup barrier: the waves go their own ways below)
    coef = s_coef;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, grp = lane >> 4;
  int *wl = lds + wv * kWaveWords;
  const long long rows = (a.n + kAngPredEntriesPerWave - 1) / kAngPredEntriesPerWave;
  for (long long r = (long long)blockIdx.x * kAngPredWaves + wv; r < rows; r += (long long)gridDim.x * kAngPredWaves) {
    const long long idx = r * kAngPredEntriesPerWave + lane;  // the lane's entry
    Item c{};
    c.on = c.reg = false;
    int ext = 0;
    if (idx < a.n && pred_mode_is_angular(a.items[idx].mode)) {  // (padding: this one load)
      const mip_pred_item it = a.items[idx];  // (one reading of the entry: its mode is the one emitted, its cu names the table's)
      c = pred_decode<false, true>(a, it, AngShapes{});
      c.on = c.on && pred_mode_is_angular(c.mode);  // (the mode word was read twice; only this reading counts)
      if constexpr (Line::kExt == ExtTable::required) {
        if (c.on) ext = a.ext[it.cu];  // (the write rule has checked it.cu)
      } else if constexpr (Line::kExt == ExtTable::optional) {
        if (c.on && a.ext) ext = a.ext[it.cu];  // (no table: the substituted lines)
      }
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
      predict_angular_cu<16, Line>(a, u, (uint32_t)__shfl(ext, src < 0 ? 0 : src, 64), coef, lane & 15, wl + grp * kGroupWords);
    }
    while (large) {  // larger blocks, one per wave
      const int src = __ffsll((long long)large) - 1;
      large &= large - 1;
      Item u = take_item(c, src);
      u.on = true;
      predict_angular_cu<64, Line>(a, u, (uint32_t)__shfl(ext, src, 64), coef, lane, wl);
    }
  }
}

__global__ __launch_bounds__(64 * kAngPredWaves) void angular_predict_kernel(PredictArgs a) { angular_predict_items<Line2>(a); }
__global__ __launch_bounds__(64 * kAngPredWaves) void angular_ext_predict_kernel(PredictExtArgs a) { angular_predict_items<ExtLine2>(a); }
__global__ __launch_bounds__(64 * kAngPredWaves) void angular_tap4_predict_kernel(PredictTap4Args a) { angular_predict_items<ExtLine4>(a); }

// The launch of all three.  ext_ok: the length table is there where the kernel needs it.
template <class Args>
hipError_t launch_angular_predict(void (*kernel)(Args), const Args &a, bool ext_ok, hipStream_t s) {
  if (a.n < 1) return hipSuccess;
  if (!a.refs || !a.items || !a.out || !a.unavail || !a.geo || !ext_ok || a.n > (1LL << 31) - 256) return hipErrorInvalidValue;
  // grid-stride over the list: 256 entries per workgroup pass, a fixed cap on the workgroups
  const long long per_group = (long long)kAngPredWaves * kAngPredEntriesPerWave;
  const long long groups = std::min<long long>((a.n + per_group - 1) / per_group, kAngPredGroupsCap);
  hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(64 * kAngPredWaves), 0, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_predict_angular(const PredictArgs &a, hipStream_t s) { return launch_angular_predict(angular_predict_kernel, a, true, s); }
hipError_t launch_predict_angular_ext(const PredictExtArgs &a, hipStream_t s) {
  return launch_angular_predict(angular_ext_predict_kernel, a, a.ext != nullptr, s);
}
hipError_t launch_predict_angular_tap4(const PredictTap4Args &a, hipStream_t s) {  // (no table: the substituted lines)
  return launch_angular_predict(angular_tap4_predict_kernel, a, true, s);
}

}  // namespace mipgpu

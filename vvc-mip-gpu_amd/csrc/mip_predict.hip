// mip_predict.hip -- MIP prediction output: the predicted samples of chosen (CU, mode) pairs
// (gfx950).  No reference counterpart: the reference's upsampleDistortion builds these
// samples in LDS, measures them against the originals and drops them (intra.cl:545-1166);
// an encoder that takes the decision next needs the block itself (residual, full RD).
//
// Plain 32-bit integer arithmetic like mip_fixup.hip -- engine-filtered references exceed 10
// bits in the last frame columns at widths that are not multiples of 128 -- in the
// reference's own semantics:
//   boundaries   intra.cl:96-107, 232-243 (linear indexes, padding), 127-141, 259-279
//   GEMV         intra.cl:415-485 (p_0, offset, shift 6, clip to 10 bits, transposition)
//   upsampling   intra.cl:815-912 (horizontal on the anchor rows, then vertical)
//
// Work split: a wave takes four consecutive list items at a time.  When none of them has more
// than 64 samples (4x4, 8x4, 4x8, 8x8, 16x4, 4x16: at most a 4x4 reduced prediction), each
// 16-lane group predicts its own item; otherwise the whole wave predicts them one after
// another, so that the shape is wave-uniform.  Per item: boundaries -> LDS (the top row
// with 8-byte loads), reduced boundaries, one GEMV output per lane, the horizontal pass on
// the anchor rows -> LDS, then every lane builds 8 (or 4) consecutive samples of an output
// row from the anchor rows (the vertical pass needs no second buffer) and stores them with
// one 16-byte (8-byte) store.  All LDS traffic is wave-private: no workgroup barrier.
//
// Regular items (the kernel's second instance, MIP_PRED_REGULAR): an item whose mode is
// MIP_MODE_PLANAR / MIP_MODE_DC needs the boundaries and, for DC, their two sums (eight partial
// sums in red[], where a MIP item keeps its reduced boundaries); it idles through the GEMV and
// anchor-row phases of its MIP neighbours and builds its samples in the store phase with the
// per-sample functions of intra_plan.h -- the text the cost kernel (mip_intra.hip) and the host
// restatement run, so an emitted block is the one whose SAD / SATD mip_intra_device reports.
//
// Every item is checked here against the write rule of include/mipgpu.h (the list is data
// in device memory): a bad entry writes nothing, reads no sample and is counted.
#include <algorithm>

#include "intra_plan.h"
#include "mip_kernels.h"
#include "mip_tables.h"
#include "predict_rule.h"

namespace mipgpu {
namespace {

__constant__ mip_shape_desc p_shapes[MIP_NUM_SHAPES] = MIP_SHAPE_TABLE;
__constant__ uint8_t p_w0[16 * 16 * 4] = MIP_WEIGHTS_S0;
__constant__ uint8_t p_w1[8 * 16 * 8] = MIP_WEIGHTS_S1;
__constant__ uint8_t p_w2[6 * 64 * 7] = MIP_WEIGHTS_S2;

constexpr int kPredWaves = 4;          // waves per workgroup
constexpr int kPredItemsPerWave = 4;   // list items a wave takes at a time (one per 16 lanes)
// Wave-private LDS words.  A group of G lanes (64: the wave, 16: a quarter) keeps
//   top[G] left[G] red[8] rpred[G] anchor[r x w]
// (anchor rows: r x w <= 8 x 64 for the wave, 4 x 16 for a quarter); every array starts on a
// 16-byte boundary.  A regular item uses top, left and red only.
constexpr int lds_words(int g) { return 3 * g + 8 + (g == 64 ? 8 * 64 : 4 * 16); }
constexpr int kWaveWords = lds_words(64);  // 712
constexpr int kGroupWords = 176;           // a quarter's words (120 used), 16-byte aligned
static_assert(kWaveWords % 4 == 0 && kGroupWords % 4 == 0 && kGroupWords >= lds_words(16) &&
                  kPredItemsPerWave * kGroupWords <= kWaveWords,
              "LDS layout");

// LDS fence for data handed between lanes of ONE wave.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int ilog2i(int v) { return 31 - __clz(v); }

// V consecutive samples of output row yy from column xx (multiple of V): the vertical pass
// between the anchor rows (intra.cl:871-912); anchor rows keep their values.
template <int V>
__device__ __forceinline__ void store_rows(const Item &c, const int *top, const int *anc, int t, int step,
                                           uint16_t *out) {
  const int w = c.w, uv = c.sid == 2 ? c.h >> 3 : c.h >> 2, lv = ilog2i(uv);
  const int lu = ilog2i(w) - (V == 8 ? 3 : 2);  // log2 of the lane units per row
  const int units = (c.h * w) >> (V == 8 ? 3 : 2);
  for (int u = t; u < units; u += step) {
    const int yy = u >> lu, xx = (u & ((1 << lu) - 1)) * V;
    const int kk = yy >> lv, o = (yy & (uv - 1)) + 1;
    int v[V];
#pragma unroll
    for (int q = 0; q < V; q += 4) {
      const int4 af = *reinterpret_cast<const int4 *>(anc + kk * w + xx + q);
      int4 r = af;
      if (o != uv) {
        const int4 bf = *reinterpret_cast<const int4 *>(kk == 0 ? top + xx + q : anc + (kk - 1) * w + xx + q);
        const int rnd = 1 << (lv - 1);
        r.x = ((uv - o) * bf.x + o * af.x + rnd) >> lv;
        r.y = ((uv - o) * bf.y + o * af.y + rnd) >> lv;
        r.z = ((uv - o) * bf.z + o * af.z + rnd) >> lv;
        r.w = ((uv - o) * bf.w + o * af.w + rnd) >> lv;
      }
      v[q] = r.x;
      v[q + 1] = r.y;
      v[q + 2] = r.z;
      v[q + 3] = r.w;
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

// The same lane units for a regular item: Planar or DC, then PDPC (include/mipgpu.h,
// mip_intra_device), from the boundaries and the eight partial sums in red[].
template <int V>
__device__ __forceinline__ void store_regular(const Item &c, const int *top, const int *left, const int *red, int t, int step,
                                              uint16_t *out) {
  const int w = c.w, lw = ilog2i(w), lh = ilog2i(c.h), scale = (lw + lh - 2) >> 2;
  const int lu = lw - (V == 8 ? 3 : 2);
  const int units = (c.h * w) >> (V == 8 ? 3 : 2);
  const bool planar = c.mode == MIP_MODE_PLANAR;
  const int4 st = *reinterpret_cast<const int4 *>(red), sl = *reinterpret_cast<const int4 *>(red + 4);
  const int dc = intra_dc(st.x + st.y + st.z + st.w, sl.x + sl.y + sl.z + sl.w, lw, lh);
  const int tr = top[w - 1], bl = left[c.h - 1];
  for (int u = t; u < units; u += step) {
    const int yy = u >> lu, xx = (u & ((1 << lu) - 1)) * V;
    const int lj = left[yy], wt = intra_pdpc_weight(yy, scale);
    int v[V];
#pragma unroll
    for (int q = 0; q < V; q += 4) {
      const int4 tf = *reinterpret_cast<const int4 *>(top + xx + q);
      const int ti[4] = {tf.x, tf.y, tf.z, tf.w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int i = xx + q + k;
        const int p = planar ? intra_planar(ti[k], lj, tr, bl, i, yy, lw, lh) : dc;
        v[q + k] = intra_pdpc(p, ti[k], lj, wt, intra_pdpc_weight(i, scale));
      }
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

// Prediction of one item by a group of G lanes (t = lane inside the group, L = the group's
// LDS words).  Called by whole waves: lanes of groups without an item to write run it with
// c.on = false (no memory access), so that the fences sit in wave-uniform control flow.  For the
// same reason a regular item's group runs every phase: mip = false predicates the MIP steps.
template <int G, bool REGULAR>
__device__ __forceinline__ void predict_cu(const PredictArgs &a, const Item &c, int t, int *L) {
  int *top = L, *left = L + G, *red = L + 2 * G, *rpred = L + 2 * G + 8, *anc = L + 3 * G + 8;
  const int W = a.width, w = c.w, h = c.h, x = c.x, y = c.y, sid = c.sid;
  const bool reg = REGULAR && c.reg, mip = c.on && !reg;
  const uint16_t *F = a.refs + (size_t)c.frame * W * a.height;
  // complete boundaries (linear indexes, intra.cl:100, 106, 236, 242)
  if (c.on) {
    if (y > 0) {
      const uint16_t *row = F + (size_t)(y - 1) * W + x;  // a multiple of 4 samples into the frame
      if (a.refs_vec) {
        if (4 * t < w) {
          const uint2 v = *reinterpret_cast<const uint2 *>(row + 4 * t);
          *reinterpret_cast<int4 *>(top + 4 * t) =
              make_int4((int)(v.x & 0xffffu), (int)(v.x >> 16), (int)(v.y & 0xffffu), (int)(v.y >> 16));
        }
      } else if (t < w) {
        top[t] = row[t];
      }
    } else if (t < w) {
      top[t] = x == 0 ? 512 : F[x - 1];
    }
    if (t < h) left[t] = x > 0 ? F[(size_t)(y + t) * W + x - 1] : (y == 0 ? 512 : F[(size_t)(y - 1) * W]);
  }
  wave_lds_sync();
  const int rbs = sid == 0 && !reg ? 2 : 4;
  if (c.on && t < 2 * rbs) {  // reduced boundaries: box averages; a factor of 1 is a copy
    const int side = t >= rbs, i = t - side * rbs, len = side ? h : w, df = len / rbs, l2 = ilog2i(df);
    const int rnd = df > 1 ? 1 << (l2 - 1) : 0;
    const int *src = side ? left : top;
    int s = 0;
    for (int k = 0; k < df; k++) s += src[i * df + k];
    red[side * 4 + i] = reg ? s : (s + rnd) >> l2;  // (a regular item: quarter sums for DC)
  }
  wave_lds_sync();
  const int r = sid == 2 ? 8 : 4, lr = sid == 2 ? 3 : 2;
  if (mip && t < r * r) {  // reduced prediction (intra.cl:415-485), one output per lane
    const bool tr = c.mode >= c.modes;
    const int mode = tr ? c.mode - c.modes : c.mode;
    const int4 rt = *reinterpret_cast<const int4 *>(red), rl = *reinterpret_cast<const int4 *>(red + 4);
    const int4 f = tr ? rl : rt, s = tr ? rt : rl;  // first / second half of the input vector
    const int b0 = f.x;
    int p[8];  // p_k = b_k - b_0; sizeId 0 has four inputs (the others stay 0)
    p[0] = sid == 2 ? 0 : 512 - b0;
    p[1] = f.y - b0;
    p[2] = (sid == 0 ? s.x : f.z) - b0;
    p[3] = (sid == 0 ? s.y : f.w) - b0;
    p[4] = sid == 0 ? 0 : s.x - b0;
    p[5] = sid == 0 ? 0 : s.y - b0;
    p[6] = sid == 0 ? 0 : s.z - b0;
    p[7] = sid == 0 ? 0 : s.w - b0;
    int psum = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) psum += p[i];
    int acc = 32 - 32 * psum;
    if (sid == 2) {
      const uint8_t *wp = p_w2 + (mode * 64 + t) * 7;
#pragma unroll
      for (int i = 1; i < 8; i++) acc += p[i] * wp[i - 1];
    } else if (sid == 1) {
      const uint8_t *wp = p_w1 + (mode * 16 + t) * 8;
#pragma unroll
      for (int i = 0; i < 8; i++) acc += p[i] * wp[i];
    } else {
      const uint8_t *wp = p_w0 + (mode * 16 + t) * 4;
#pragma unroll
      for (int i = 0; i < 4; i++) acc += p[i] * wp[i];
    }
    const int v = min(max((acc >> 6) + b0, 0), 1023);
    rpred[tr ? ((t & (r - 1)) << lr) + (t >> lr) : t] = v;
  }
  wave_lds_sync();
  if (mip) {  // horizontal pass on the anchor rows (a factor of 1 is a copy): anc[k][xx]
    const int uh = w >> lr, uv = h >> lr, lh = ilog2i(uh), lw = ilog2i(w);
    for (int i = t; i < r * w; i += G) {
      const int k = i >> lw, xx = i & (w - 1);
      int v;
      if (uh == 1) {
        v = rpred[k * r + xx];
      } else {
        const int o = (xx & (uh - 1)) + 1, j = xx >> lh;
        const int before = j == 0 ? left[k * uv + uv - 1] : rpred[k * r + j - 1];
        v = ((uh - o) * before + o * rpred[k * r + j] + (1 << (lh - 1))) >> lh;
      }
      anc[i] = v;
    }
  }
  wave_lds_sync();
  if (c.on) {
    // 16-byte stores where every row segment of the block is 16-byte aligned
    const bool wide = w >= 8 && (c.pitch & 7) == 0 && ((reinterpret_cast<uintptr_t>(a.out + c.offset) & 15) == 0);
    if (reg) {
      if (wide) store_regular<8>(c, top, left, red, t, G, a.out);
      else store_regular<4>(c, top, left, red, t, G, a.out);
    } else if (wide) {
      store_rows<8>(c, top, anc, t, G, a.out);
    } else {
      store_rows<4>(c, top, anc, t, G, a.out);
    }
  }
  wave_lds_sync();  // the next item rewrites the group's words
}

// The write rule of include/mipgpu.h, item by item (predict_rule.h, shared with the angular kernel).
struct PredShapes {
  __device__ __forceinline__ mip_shape_desc operator()(int s) const { return p_shapes[s]; }
};
template <bool REGULAR>
__device__ __forceinline__ Item decode(const PredictArgs &a, const mip_pred_item &it) {
  return pred_decode<REGULAR, false>(a, it, PredShapes{});
}

__device__ __forceinline__ int bcast(int v, int src) { return __builtin_amdgcn_readfirstlane(__shfl(v, src, 64)); }

template <bool REGULAR>
__global__ __launch_bounds__(64 * kPredWaves) void predict_kernel(PredictArgs a) {
  __shared__ __attribute__((aligned(16))) int lds[kPredWaves * kWaveWords];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, grp = lane >> 4;
  int *wl = lds + wv * kWaveWords;
  const long long quads = (a.n + kPredItemsPerWave - 1) / kPredItemsPerWave;
  for (long long q = (long long)blockIdx.x * kPredWaves + wv; q < quads; q += (long long)gridDim.x * kPredWaves) {
    const long long idx = q * kPredItemsPerWave + grp;  // the 16-lane group's item
    Item c{};
    c.on = c.reg = false;
    if (idx < a.n) {
      c = decode<REGULAR>(a, a.items[idx]);
      if (!c.on && (lane & 15) == 0 && a.skipped) atomicAdd(a.skipped, 1u);
    }
    const bool large = c.on && c.w * c.h > 64;
    if (!__any(large)) {
      predict_cu<16, REGULAR>(a, c, lane & 15, wl + grp * kGroupWords);
    } else {
      for (int j = 0; j < kPredItemsPerWave; j++) {
        const int src = 16 * j;
        if (!bcast(c.on, src)) continue;  // wave-uniform
        Item u;
        u.on = true;
        u.reg = REGULAR && bcast(c.reg, src);
        u.frame = bcast(c.frame, src);
        u.x = bcast(c.x, src);
        u.y = bcast(c.y, src);
        u.w = bcast(c.w, src);
        u.h = bcast(c.h, src);
        u.sid = bcast(c.sid, src);
        u.modes = bcast(c.modes, src);
        u.mode = bcast(c.mode, src);
        u.pitch = bcast(c.pitch, src);
        const uint32_t lo = (uint32_t)bcast((int)(uint32_t)c.offset, src), hi = (uint32_t)bcast((int)(c.offset >> 32), src);
        u.offset = (long long)(((unsigned long long)hi << 32) | lo);
        predict_cu<64, REGULAR>(a, u, lane, wl);
      }
    }
  }
}

}  // namespace

hipError_t launch_predict(const PredictArgs &a, hipStream_t s) {
  if (a.n < 1) return hipSuccess;
  if (!a.refs || !a.items || !a.out || !a.unavail || !a.geo || a.n > (1LL << 31) - 256) return hipErrorInvalidValue;
  // grid-stride over the list: 16 items per workgroup pass, at most 16 workgroups per CU's worth
  const long long per_group = (long long)kPredWaves * kPredItemsPerWave;
  const long long groups = std::min<long long>((a.n + per_group - 1) / per_group, 256 * 16);
  // (flags 0 runs the MIP-only instance: no regular-item code in it)
  if (a.regular) hipLaunchKernelGGL(predict_kernel<true>, dim3((unsigned)groups), dim3(64 * kPredWaves), 0, s, a);
  else hipLaunchKernelGGL(predict_kernel<false>, dim3((unsigned)groups), dim3(64 * kPredWaves), 0, s, a);
  return hipGetLastError();
}

}  // namespace mipgpu

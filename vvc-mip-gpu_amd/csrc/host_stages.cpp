// host_stages.cpp -- the stages behind the search (include/mipgpu.h): prediction output, the
// partition decision, the Planar / DC and angular intra costs, the candidate lists and the chains
// of them.  Each has a device entry point (the caller's buffers and stream) and a host wrapper that
// walks the call's frames through the engine buffers in chunks (walk_chunks).
#include "engine.h"

#include <algorithm>

#include "angular_plan.h"
#include "candidates_plan.h"
#include "intra_plan.h"
#include "partition_plan.h"
#include "predict_rule.h"

using mipgpu::kShapes;

// One chunk at a time through e->d_frames on e->stream: upload, body, download, synchronise.
// Caller references go into the engine's reference buffer, or -- on an engine without one --
// into a block of the walk's own, sized to the chunk.
int walk_chunks(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes, int chunk,
                std::initializer_list<ChunkOut> outs, const std::function<int(int, const uint16_t *)> &body) {
  const size_t fs = (size_t)e->width * e->height;
  DevScratch staging(e->device);
  uint16_t *d_refs = refs_or_null ? e->d_refs : nullptr;
  if (refs_or_null && !d_refs) HIP_TRY(staging.take(d_refs, (size_t)chunk * fs * 2));
  hipStream_t s = e->stream;
  for (int f0 = 0; f0 < nframes; f0 += chunk) {
    const size_t nb = (size_t)std::min(chunk, nframes - f0);
    HIP_TRY(hipMemcpyAsync(e->d_frames, frames + f0 * fs, nb * fs * 2, hipMemcpyHostToDevice, s));
    if (d_refs) HIP_TRY(hipMemcpyAsync(d_refs, refs_or_null + f0 * fs, nb * fs * 2, hipMemcpyHostToDevice, s));
    if (body((int)nb, d_refs) != 0) return -1;
    for (const ChunkOut &o : outs)
      if (o.host) HIP_TRY(hipMemcpyAsync((char *)o.host + f0 * o.bytes, o.dev, nb * o.bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  e->refs_pending = false;
  return 0;
}

extern "C" {

// ---------------------------------------------------------------- prediction output
int mip_pred_layout(int width, int height, int nframes, int layout, mip_pred_item *items, int64_t n,
                    int64_t *out_samples) {
  if (width <= 0 || height <= 0 || width % 4 || height % 4 || nframes < 1 || n < 0 || (n && !items) || !out_samples)
    return fail("bad prediction-layout arguments");
  if (layout != MIP_PRED_PACKED && layout != MIP_PRED_FRAME) return fail("unknown prediction layout %d", layout);
  const std::vector<mipgpu::CuGeo> &geo = mipgpu::cu_geo_table();
  const int cols = (width + 127) / 128, ncus = mip_num_ctus(width, height) * MIP_CUS_PER_CTU;
  const int64_t fs = (int64_t)width * height;
  int64_t next = 0;
  for (int64_t i = 0; i < n; i++) {
    mip_pred_item &it = items[i];
    if (it.frame < 0 || it.frame >= nframes)
      return fail("prediction item %lld: frame %d outside 0..%d", (long long)i, it.frame, nframes - 1);
    if (it.cu < 0 || it.cu >= ncus) return fail("prediction item %lld: cu %d outside 0..%d", (long long)i, it.cu, ncus - 1);
    const int ctu = it.cu / MIP_CUS_PER_CTU;
    const mipgpu::CuGeo &g = geo[(size_t)(it.cu % MIP_CUS_PER_CTU)];
    const mip_shape_desc &sd = kShapes[g.shape];
    if (layout == MIP_PRED_PACKED) {
      it.pitch = sd.w;
      it.offset = next;
      next += (int64_t)sd.w * sd.h;
    } else {
      it.pitch = width;
      it.offset = it.frame * fs + (int64_t)(128 * (ctu / cols) + g.y) * width + 128 * (ctu % cols) + g.x;
    }
  }
  *out_samples = layout == MIP_PRED_PACKED ? next : (int64_t)nframes * fs;
  return 0;
}

// The engine's prediction tables (mip_engine::d_pred_unavail, d_pred_geo), uploaded once.
static int ensure_pred_tables(mip_engine *e) {
  if (e->d_pred_geo) return 0;
  const size_t ncus = (size_t)e->nctus * MIP_CUS_PER_CTU;
  std::vector<uint8_t> un(ncus);
  for (int m = 0; m < 2; m++) {
    if (m == 1 && e->opts.filter == MIP_FILTER_NONE) {
      e->d_pred_unavail[1] = e->d_pred_unavail[0];
      break;
    }
    if (mip_unavailable_cus(e->width, e->height, m ? e->opts.filter : MIP_FILTER_NONE, un.data()) != 0) return -1;
    HIP_TRY(dev_malloc(e->device, (void **)&e->d_pred_unavail[m], ncus));
    HIP_TRY(hipMemcpy(e->d_pred_unavail[m], un.data(), ncus, hipMemcpyHostToDevice));
  }
  const std::vector<mipgpu::CuGeo> &geo = mipgpu::cu_geo_table();
  std::vector<uint32_t> packed(geo.size());
  for (size_t i = 0; i < geo.size(); i++) packed[i] = geo[i].shape | (uint32_t)geo[i].x << 8 | (uint32_t)geo[i].y << 16;
  uint32_t *d = nullptr;
  HIP_TRY(dev_malloc(e->device, (void **)&d, packed.size() * sizeof(uint32_t)));
  if (hipMemcpy(d, packed.data(), packed.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
    dev_free(d);
    return fail("uploading the CU geometry failed");
  }
  e->d_pred_geo = d;  // (set last: the tables are complete)
  return 0;
}

// The engine's extended-line lengths (mip_engine::d_ang_ext), uploaded at the first call with
// MIP_ANG_REFS_EXTENDED: mip_extended_refs for the two sets of d_pred_unavail.
static int ensure_ext_tables(mip_engine *e) {
  if (e->d_ang_ext[1]) return 0;
  const size_t ncus = (size_t)e->nctus * MIP_CUS_PER_CTU;
  std::vector<uint8_t> top(ncus), left(ncus);
  std::vector<uint16_t> both(ncus);
  for (int m = 0; m < 2; m++) {
    if (m == 1 && e->opts.filter == MIP_FILTER_NONE) {
      e->d_ang_ext[1] = e->d_ang_ext[0];
      break;
    }
    if (!e->d_ang_ext[m]) {  // (kept from a call that failed half-way)
      if (mip_extended_refs(e->width, e->height, m ? e->opts.filter : MIP_FILTER_NONE, top.data(), left.data()) != 0) return -1;
      for (size_t k = 0; k < ncus; k++) both[k] = (uint16_t)(top[k] | left[k] << 8);
      uint16_t *d = nullptr;
      HIP_TRY(dev_malloc(e->device, (void **)&d, ncus * sizeof(uint16_t)));
      if (hipMemcpy(d, both.data(), ncus * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess) {
        dev_free(d);
        return fail("uploading the extended reference lengths failed");
      }
      e->d_ang_ext[m] = d;
    }
  }
  return 0;
}

// The 64 coefficient words of the 4-tap kernels (mip_kernels.h AngularTap4Args::coef).
static void tap4_coefficients(uint32_t (&coef)[mipgpu::kAngCoefWords]) {
  for (int k = 0; k < mipgpu::kAngCoefWords; k++) coef[k] = mipgpu::ang_coef_word(k >> 5, k & 31);
}

// refs: the reference frames to predict from (already resolved); engine_refs: they are the
// engine filter's output (its unavailable set applies).
static int predict_launch(mip_engine *e, const uint16_t *refs, bool engine_refs, int nframes, const mip_pred_item *d_items,
                          int64_t n, uint16_t *d_out, int64_t out_samples, uint32_t *d_skipped, unsigned flags, hipStream_t s) {
  mipgpu::PredictArgs a{};
  a.refs = refs;
  a.items = d_items;
  a.n = n;
  a.unavail = e->d_pred_unavail[engine_refs ? 1 : 0];
  a.geo = e->d_pred_geo;
  a.out = d_out;
  a.out_samples = out_samples;
  a.skipped = d_skipped;
  a.width = e->width;
  a.height = e->height;
  a.ctu_cols = e->ctu_cols;
  a.nctus = e->nctus;
  a.nframes = nframes;
  a.refs_vec = (reinterpret_cast<uintptr_t>(refs) & 7) == 0;
  a.regular = (flags & MIP_PRED_REGULAR) != 0;
  HIP_TRY(mipgpu::launch_predict(a, s));
  // MIP_PRED_ANGULAR: the kernel above has rejected and counted the angular items; the angular
  // kernel emits them behind it and takes them off the count (final in stream order)
  if (flags & MIP_PRED_ANGULAR) {
    const bool extended = e->ang_refs.load() == MIP_ANG_REFS_EXTENDED;       // (the two settings of this launch)
    const bool tap4 = e->ang_interp.load() == MIP_ANG_INTERP_4TAP;
    if (extended && ensure_ext_tables(e) != 0) return -1;
    if (tap4) {  // one kernel for both reference settings: no table is the substituted lines
      mipgpu::PredictTap4Args x{};
      static_cast<mipgpu::PredictArgs &>(x) = a;
      x.ext = extended ? e->d_ang_ext[engine_refs ? 1 : 0] : nullptr;
      tap4_coefficients(x.coef);
      HIP_TRY(mipgpu::launch_predict_angular_tap4(x, s));
    } else if (extended) {
      mipgpu::PredictExtArgs x{};
      static_cast<mipgpu::PredictArgs &>(x) = a;
      x.ext = e->d_ang_ext[engine_refs ? 1 : 0];
      HIP_TRY(mipgpu::launch_predict_angular_ext(x, s));
    } else {
      HIP_TRY(mipgpu::launch_predict_angular(a, s));
    }
  }
  return 0;
}

static int predict_args_ok(const mip_engine *e, int nframes, const void *items, int64_t n, const void *out,
                           int64_t out_samples, unsigned flags) {
  if (!mipgpu::pred_flags_ok(flags)) return fail("unknown prediction flags 0x%x", flags);
  if (nframes < 1 || n < 0 || out_samples < 0 || (n && (!items || !out))) return fail("bad prediction arguments");
  if (n > kMaxCus) return fail("%lld prediction items exceed %lld per call", (long long)n, kMaxCus);
  if ((long long)nframes * e->nctus * MIP_CUS_PER_CTU > kMaxCus) return fail("%d frames exceed %lld CUs per call", nframes, kMaxCus);
  return 0;
}

int mip_predict_device(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes,
                       const mip_pred_item *d_items, int64_t n, uint16_t *d_out, int64_t out_samples,
                       uint32_t *d_skipped, void *stream) {
  return mip_predict_device_ex(e, d_frames, d_refs, nframes, d_items, n, d_out, out_samples, d_skipped, 0, stream);
}

int mip_predict_device_ex(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes,
                          const mip_pred_item *d_items, int64_t n, uint16_t *d_out, int64_t out_samples,
                          uint32_t *d_skipped, unsigned flags, void *stream) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!d_frames && !d_refs) return fail("bad prediction arguments: no frames");
  if (predict_args_ok(e, nframes, d_items, n, d_out, out_samples, flags) != 0) return -1;
  if ((reinterpret_cast<uintptr_t>(d_out) & 7) || (reinterpret_cast<uintptr_t>(d_items) & 7))
    return fail("d_out and d_items must be 8-byte aligned");
  if (n == 0) return 0;
  HIP_TRY(hipSetDevice(e->device));
  if (flush_open(e) != 0) return -1;  // (device-API work orders itself after the host calls)
  if (ensure_pred_tables(e) != 0) return -1;
  hipStream_t s = (hipStream_t)stream;
  const uint16_t *refs = nullptr;
  bool engine_refs = false;
  if (engine_refs_begin(e, d_frames, d_refs, nframes, s, &refs, &engine_refs) != 0) return -1;
  if (predict_launch(e, refs, engine_refs, nframes, d_items, n, d_out, out_samples, d_skipped, flags, s) != 0) return -1;
  return engine_refs_end(e, engine_refs, s);
}

int mip_predict_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                       const mip_pred_item *items, int64_t n, uint16_t *out, int64_t out_samples, int64_t *skipped) {
  return mip_predict_frames_ex(e, frames, refs_or_null, nframes, items, n, out, out_samples, 0, skipped);
}

int mip_predict_frames_ex(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                          const mip_pred_item *items, int64_t n, uint16_t *out, int64_t out_samples, unsigned flags,
                          int64_t *skipped) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!frames && !refs_or_null) return fail("bad prediction arguments: no frames");
  if (predict_args_ok(e, nframes, items, n, out, out_samples, flags) != 0) return -1;
  if (out_samples && !out) return fail("bad prediction arguments: out is NULL");
  // the list on the host: names outside the call's frames / the frame's CUs are the caller's bug
  for (int64_t i = 0; i < n; i++) {
    if (items[i].frame < 0 || items[i].frame >= nframes)
      return fail("prediction item %lld: frame %d outside 0..%d", (long long)i, items[i].frame, nframes - 1);
    if (items[i].cu < 0 || items[i].cu >= e->nctus * MIP_CUS_PER_CTU)
      return fail("prediction item %lld: cu %d outside 0..%d", (long long)i, items[i].cu, e->nctus * MIP_CUS_PER_CTU - 1);
  }
  if (skipped) *skipped = 0;
  if (out_samples == 0) {
    if (skipped) *skipped = n;
    return 0;
  }
  HIP_TRY(hipSetDevice(e->device));
  if (quiesce(e) != 0) return -1;  // (host searches in flight use d_frames / d_refs)
  if (ensure_pred_tables(e) != 0) return -1;
  const size_t fs = (size_t)e->width * e->height, fbytes = fs * (size_t)nframes * 2;
  const bool engine_refs = !refs_or_null && e->opts.filter != MIP_FILTER_NONE;
  // the call's own device buffers (through the device block cache); the engine's frame buffers
  // serve when the call's frames fit them
  DevScratch scratch(e->device);
  uint16_t *d_in = e->d_frames, *d_refs = e->d_refs, *d_out = nullptr;
  mip_pred_item *d_items = nullptr;
  uint32_t *d_skip = nullptr;
  if (nframes > e->hp_frames) HIP_TRY(scratch.take(d_in, fbytes));
  if (engine_refs && (nframes > e->hp_frames || !d_refs)) HIP_TRY(scratch.take(d_refs, fbytes));
  HIP_TRY(scratch.take(d_out, (size_t)out_samples * 2));
  HIP_TRY(scratch.take(d_items, std::max<size_t>(1, (size_t)n) * sizeof(mip_pred_item)));
  HIP_TRY(scratch.take(d_skip, sizeof(uint32_t)));
  hipStream_t s = e->stream;
  HIP_TRY(hipMemcpyAsync(d_in, refs_or_null ? refs_or_null : frames, fbytes, hipMemcpyHostToDevice, s));
  if (n) HIP_TRY(hipMemcpyAsync(d_items, items, (size_t)n * sizeof(mip_pred_item), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(d_out, 0xff, (size_t)out_samples * 2, s));  // MIP_PRED_NONE
  HIP_TRY(hipMemsetAsync(d_skip, 0, sizeof(uint32_t), s));
  const uint16_t *refs = d_in;
  if (engine_refs) {
    // (in batches of max_batch frames like mip_filter_frames: the filter kernel's launch limit)
    for (int f0 = 0; f0 < nframes; f0 += e->opts.max_batch) {
      const int nb = std::min(e->opts.max_batch, nframes - f0);
      if (mip_filter_device(d_in + f0 * fs, d_refs + f0 * fs, e->width, e->height, nb, e->opts.filter, e->opts.kernel_idx,
                            s) != 0)
        return -1;
    }
    refs = d_refs;
  }
  if (predict_launch(e, refs, engine_refs, nframes, d_items, n, d_out, out_samples, d_skip, flags, s) != 0) return -1;
  uint32_t nskip = 0;
  HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)out_samples * 2, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&nskip, d_skip, sizeof nskip, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  e->refs_pending = false;
  if (skipped) *skipped = nskip;
  return 0;
}

// ---------------------------------------------------------------- partition decision
// The argument rules of both partition entry points (before any launch).
static int partition_args_ok(int width, int height, int nframes, const int32_t *penalty, bool any_output) {
  if (width <= 0 || height <= 0 || width % 4 || height % 4 || nframes < 1) return fail("bad partition arguments");
  if (!any_output) return fail("partition: no output given");
  if (!mipgpu::part_penalty_ok(penalty))
    return fail("partition: a shape penalty is outside 0..%d", (int)mipgpu::kPartMaxPenalty);
  if ((long long)nframes * mip_num_ctus(width, height) * MIP_CUS_PER_CTU > kMaxCus)
    return fail("%d frames exceed %lld CUs per call", nframes, kMaxCus);
  return 0;
}

int mip_partition_device(const int32_t *d_best_cost, const uint8_t *d_best_mode, int width, int height, int nframes,
                         const int32_t *penalty, uint8_t *d_leaf, int32_t *d_ctu_cost, int32_t *d_ctu_leaves,
                         mip_pred_item *d_items, void *stream) {
  if (!d_best_cost) return fail("bad partition arguments: d_best_cost is NULL");
  if (partition_args_ok(width, height, nframes, penalty, d_leaf || d_ctu_cost || d_ctu_leaves || d_items) != 0) return -1;
  if (d_items && !d_best_mode) return fail("partition: d_items needs d_best_mode");
  if (reinterpret_cast<uintptr_t>(d_items) & 7) return fail("partition: d_items must be 8-byte aligned");
  mipgpu::PartitionArgs a{};
  a.best_cost = d_best_cost;
  a.best_mode = d_best_mode;
  a.leaf = d_leaf;
  a.ctu_cost = d_ctu_cost;
  a.ctu_leaves = d_ctu_leaves;
  a.items = d_items;
  a.width = width;
  a.height = height;
  a.ctu_cols = (width + 127) / 128;
  a.nctus = mip_num_ctus(width, height);
  a.nframes = nframes;
  for (int s = 0; s < MIP_NUM_SHAPES; s++) a.penalty.v[s] = penalty ? penalty[s] : 0;
  HIP_TRY(mipgpu::launch_partition(a, (hipStream_t)stream));
  return 0;
}

// The device chain on host frames, chunk by chunk: decisions, (Planar / DC merge,) (angular
// merge,) partition and, with pred_out, the partition's predicted frames with the merged leaves.
// The entry points have checked their arguments and hold e->mu; `name` is theirs, for the error
// texts.
struct ChainStages {
  const char *name;
  bool intra, angular;  // the merges that run between the search and the partition
};
static int chain_frames(mip_engine *e, const ChainStages &st, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                        const int32_t *penalty, const int32_t *bias, const uint8_t *ang_modes, int ang_nmodes, int32_t ang_bias,
                        uint8_t *best_mode_out, int32_t *best_cost_out, uint8_t *leaf_out, int32_t *ctu_cost_out,
                        int32_t *ctu_leaves_out, uint16_t *pred_out) {
  if (e->opts.best_k != 1) return fail("%s needs best_k <= 1 (got %d)", st.name, e->opts.best_k);
  HIP_TRY(hipSetDevice(e->device));
  if (quiesce(e) != 0) return -1;  // (host searches in flight use the engine buffers)
  if (check_device_status(e) != 0) return -1;  // (an earlier device-API search's violation)
  if (st.intra && ensure_pred_tables(e) != 0) return -1;
  const size_t fs = (size_t)e->width * e->height, ncu = (size_t)e->nctus * MIP_CUS_PER_CTU, mb = (size_t)e->opts.max_batch;
  const size_t nctus = (size_t)e->nctus, per_frame = nctus * MIP_PART_MAX_LEAVES;  // list entries
  const int chunk = mipgpu::stage_chunk_frames(e->opts.max_batch, nframes, 0);
  // the partition outputs' device buffers, for max_batch frames: allocated at their first use,
  // released with the engine
  if (!e->d_part_leaf) HIP_TRY(dev_malloc(e->device, (void **)&e->d_part_leaf, mb * ncu));
  if (!e->d_part_ctu) HIP_TRY(dev_malloc(e->device, (void **)&e->d_part_ctu, mb * nctus * 2 * sizeof(int32_t)));
  int32_t *d_ctu_cost = e->d_part_ctu, *d_ctu_leaves = e->d_part_ctu + mb * nctus;
  // the call's own device buffers (through the device block cache): one chunk's item list and
  // its frame canvases
  DevScratch scratch(e->device);
  uint16_t *d_pred = nullptr;
  mip_pred_item *d_items = nullptr;
  if (pred_out) {
    HIP_TRY(scratch.take(d_items, chunk * per_frame * sizeof(mip_pred_item)));
    HIP_TRY(scratch.take(d_pred, chunk * fs * 2));
  }
  const bool engine_refs = !refs_or_null && e->opts.filter != MIP_FILTER_NONE;
  hipStream_t s = e->stream;
  auto stages = [&](int nb, const uint16_t *d_refs) {
    // (without references the search filters the frames into e->d_refs when the engine has a
    // filter; the merges and the prediction below read that buffer)
    if (search_device_impl(e, e->d_frames, d_refs, nb, nullptr, nullptr, nullptr, e->d_best, e->d_best_cost, s,
                           d_refs != nullptr, device_status(e)) != 0)
      return -1;
    if (st.intra && mip_intra_device(e, e->d_frames, d_refs, nb, nullptr, nullptr, nullptr, bias, e->d_best, e->d_best_cost, s) != 0)
      return -1;
    if (st.angular && mip_angular_device(e, e->d_frames, d_refs, nb, ang_modes, ang_nmodes, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, ang_bias, e->d_best, e->d_best_cost, s) != 0)
      return -1;
    // the list's frame indexes and offsets are the chunk's own: 0 .. nb-1 into d_pred
    if (mip_partition_device(e->d_best_cost, e->d_best, e->width, e->height, nb, penalty, e->d_part_leaf, d_ctu_cost,
                             d_ctu_leaves, d_items, s) != 0)
      return -1;
    if (!pred_out) return 0;
    HIP_TRY(hipMemsetAsync(d_pred, 0xff, nb * fs * 2, s));  // MIP_PRED_NONE
    const uint16_t *refs = d_refs ? d_refs : engine_refs ? e->d_refs : e->d_frames;
    return predict_launch(e, refs, engine_refs, nb, d_items, (int64_t)(nb * per_frame), d_pred, (int64_t)(nb * fs), nullptr,
                          st.angular ? MIP_PRED_REGULAR | MIP_PRED_ANGULAR : MIP_PRED_REGULAR, s);
  };
  if (walk_chunks(e, frames, refs_or_null, nframes, chunk,
                  {{pred_out, d_pred, fs * 2},
                   {best_mode_out, e->d_best, ncu},
                   {best_cost_out, e->d_best_cost, ncu * 4},
                   {leaf_out, e->d_part_leaf, ncu},
                   {ctu_cost_out, d_ctu_cost, nctus * 4},
                   {ctu_leaves_out, d_ctu_leaves, nctus * 4}},
                  stages) != 0)
    return -1;
  if (const uint32_t f = take_status(e, mip_engine::kCallRing)) return contract_error(f, st.name);
  return 0;
}

int mip_partition_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                         const int32_t *penalty, uint8_t *best_mode_out, int32_t *best_cost_out, uint8_t *leaf_out,
                         int32_t *ctu_cost_out, int32_t *ctu_leaves_out) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!frames) return fail("bad partition arguments: no frames");
  if (partition_args_ok(e->width, e->height, nframes, penalty,
                        best_mode_out || best_cost_out || leaf_out || ctu_cost_out || ctu_leaves_out) != 0)
    return -1;
  return chain_frames(e, {"mip_partition_frames", false, false}, frames, refs_or_null, nframes, penalty, nullptr, nullptr, 0, 0,
                      best_mode_out, best_cost_out, leaf_out, ctu_cost_out, ctu_leaves_out, nullptr);
}

int mip_predicted_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                         const int32_t *penalty, const int32_t *bias, uint8_t *best_mode_out, int32_t *best_cost_out,
                         uint8_t *leaf_out, int32_t *ctu_cost_out, int32_t *ctu_leaves_out, uint16_t *pred_out) {
  return mip_predicted_frames_ex(e, frames, refs_or_null, nframes, penalty, bias, nullptr, 0, 0, 0, best_mode_out, best_cost_out,
                                 leaf_out, ctu_cost_out, ctu_leaves_out, pred_out);
}

// With MIP_CHAIN_ANGULAR the angular merge runs between the Planar / DC merge and the partition,
// and the prediction emits the angular leaves too.
int mip_predicted_frames_ex(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                            const int32_t *penalty, const int32_t *bias, const uint8_t *ang_modes, int ang_nmodes,
                            int32_t ang_bias, unsigned flags, uint8_t *best_mode_out, int32_t *best_cost_out, uint8_t *leaf_out,
                            int32_t *ctu_cost_out, int32_t *ctu_leaves_out, uint16_t *pred_out) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!frames) return fail("bad partition arguments: no frames");
  if (partition_args_ok(e->width, e->height, nframes, penalty,
                        best_mode_out || best_cost_out || leaf_out || ctu_cost_out || ctu_leaves_out || pred_out) != 0)
    return -1;
  if (!mipgpu::intra_bias_ok(bias)) return fail("intra: a bias is outside 0..%d", (int)mipgpu::kIntraMaxBias);
  mipgpu::AngList ang_list_checked;  // (mip_angular_device checks the caller's list again, chunk by chunk)
  switch (mipgpu::predicted_ex_args(flags, ang_modes, ang_nmodes, ang_bias, &ang_list_checked)) {
    case mipgpu::kPredictedExOk: break;
    case mipgpu::kPredictedExFlags: return fail("unknown chain flags 0x%x", flags);
    case mipgpu::kPredictedExModes:
      return fail("angular: modes must be 1..%d strictly increasing mode numbers in %d..%d (or NULL, 0 for all)", MIP_ANGULAR_MODES,
                  MIP_ANGULAR_FIRST, MIP_ANGULAR_LAST);
    case mipgpu::kPredictedExBias: return fail("angular: the bias is outside 0..%d", (int)mipgpu::kAngMaxBias);
  }
  return chain_frames(e, {"mip_predicted_frames", true, (flags & MIP_CHAIN_ANGULAR) != 0}, frames, refs_or_null, nframes, penalty,
                      bias, ang_modes, ang_nmodes, ang_bias, best_mode_out, best_cost_out, leaf_out, ctu_cost_out, ctu_leaves_out,
                      pred_out);
}

// ---------------------------------------------------------------- Planar / DC baseline costs
// The engine's lane-slot table (mip_engine::d_intra_slots), uploaded once, and the prediction
// tables' availability sets.
static int ensure_intra_tables(mip_engine *e) {
  if (ensure_pred_tables(e) != 0) return -1;
  if (e->d_intra_slots) return 0;
  int per_block = 0;
  const std::vector<uint32_t> slots = mipgpu::intra_build_slots(&per_block);
  if (slots.empty()) return fail("intra: the CU shapes do not fit the 32x32 blocks");
  uint32_t *d = nullptr;
  HIP_TRY(dev_malloc(e->device, (void **)&d, slots.size() * sizeof(uint32_t)));
  if (hipMemcpy(d, slots.data(), slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
    dev_free(d);
    return fail("uploading the intra lane slots failed");
  }
  e->intra_slots_per_block = per_block;
  e->d_intra_slots = d;  // (set last: the table is complete)
  return 0;
}

// The argument rules of both intra entry points (before any launch).
static int intra_args_ok(const mip_engine *e, int nframes, bool any_output) {
  if (nframes < 1) return fail("bad intra arguments");
  if (!any_output) return fail("intra: no output given");
  if ((long long)nframes * e->nctus * MIP_CUS_PER_CTU > kMaxCus) return fail("%d frames exceed %lld CUs per call", nframes, kMaxCus);
  return 0;
}

int mip_intra_device(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes, int32_t *d_cost,
                     int32_t *d_sad, int32_t *d_satd, const int32_t *bias, uint8_t *d_best_mode, int32_t *d_best_cost,
                     void *stream) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!d_frames) return fail("bad intra arguments: no frames");
  if (intra_args_ok(e, nframes, d_cost || d_sad || d_satd || d_best_mode || d_best_cost) != 0) return -1;
  if (!d_best_mode != !d_best_cost) return fail("intra: d_best_mode and d_best_cost are given together");
  if (!mipgpu::intra_bias_ok(bias)) return fail("intra: a bias is outside 0..%d", (int)mipgpu::kIntraMaxBias);
  for (const void *p : {(const void *)d_cost, (const void *)d_sad, (const void *)d_satd})
    if (reinterpret_cast<uintptr_t>(p) & 7) return fail("intra: the tables must be 8-byte aligned");
  HIP_TRY(hipSetDevice(e->device));
  if (flush_open(e) != 0) return -1;  // (device-API work orders itself after the host calls)
  if (ensure_intra_tables(e) != 0) return -1;
  hipStream_t s = (hipStream_t)stream;
  const uint16_t *refs = nullptr;
  bool engine_refs = false;
  if (engine_refs_begin(e, d_frames, d_refs, nframes, s, &refs, &engine_refs) != 0) return -1;
  mipgpu::IntraArgs a{};
  a.orig = d_frames;
  a.refs = refs;
  a.unavail = e->d_pred_unavail[engine_refs ? 1 : 0];
  a.slots = e->d_intra_slots;
  a.slots_per_block = e->intra_slots_per_block;
  a.cost = d_cost;
  a.sad = d_sad;
  a.satd = d_satd;
  a.best_mode = d_best_mode;
  a.best_cost = d_best_cost;
  for (int k = 0; k < mipgpu::kIntraModes; k++) a.bias[k] = bias ? bias[k] : 0;
  a.width = e->width;
  a.height = e->height;
  a.ctu_cols = e->ctu_cols;
  a.nctus = e->nctus;
  a.nframes = nframes;
  HIP_TRY(mipgpu::launch_intra(a, s));
  return engine_refs_end(e, engine_refs, s);
}

int mip_intra_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes, int32_t *cost_out,
                     int32_t *sad_out, int32_t *satd_out) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!frames) return fail("bad intra arguments: no frames");
  if (intra_args_ok(e, nframes, cost_out || sad_out || satd_out) != 0) return -1;
  HIP_TRY(hipSetDevice(e->device));
  if (quiesce(e) != 0) return -1;  // (host searches in flight use the engine buffers)
  const size_t table = (size_t)e->nctus * MIP_CUS_PER_CTU * mipgpu::kIntraModes * sizeof(int32_t);  // per frame
  const int chunk = mipgpu::stage_chunk_frames(e->opts.max_batch, nframes, 0);
  // the call's own device buffers (through the device block cache): one table of a chunk's
  // frames per output asked for
  int32_t *const host_out[3] = {cost_out, sad_out, satd_out};
  DevScratch scratch(e->device);
  int32_t *d_out[3] = {nullptr, nullptr, nullptr};
  for (int t = 0; t < 3; t++)
    if (host_out[t]) HIP_TRY(scratch.take(d_out[t], chunk * table));
  // (without references the device entry point filters the frames itself when the engine has a filter)
  return walk_chunks(e, frames, refs_or_null, nframes, chunk,
                     {{cost_out, d_out[0], table}, {sad_out, d_out[1], table}, {satd_out, d_out[2], table}},
                     [&](int nb, const uint16_t *d_refs) {
                       return mip_intra_device(e, e->d_frames, d_refs, nb, d_out[0], d_out[1], d_out[2], nullptr, nullptr, nullptr,
                                               e->stream);
                     });
}

// ---------------------------------------------------------------- angular intra costs
// The argument rules of both angular entry points (before any launch).
static int angular_args_ok(const mip_engine *e, int nframes, const uint8_t *modes, int nmodes, bool any_output,
                           mipgpu::AngList *list) {
  if (intra_args_ok(e, nframes, any_output) != 0) return -1;
  if (!mipgpu::ang_list(modes, nmodes, list))
    return fail("angular: modes must be 1..%d strictly increasing mode numbers in %d..%d (or NULL, 0 for all)", MIP_ANGULAR_MODES,
                MIP_ANGULAR_FIRST, MIP_ANGULAR_LAST);
  return 0;
}

// Both device entry points: refine == false is mip_angular_device (seeds and d_tried not looked
// at), refine == true mip_angular_refine_device.
static int angular_device_impl(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes, const uint8_t *modes,
                               int nmodes, bool refine, int seeds, int32_t *d_cost, int32_t *d_sad, int32_t *d_satd,
                               uint8_t *d_ang_mode, int32_t *d_ang_cost, uint8_t *d_tried, int32_t bias, uint8_t *d_best_mode,
                               int32_t *d_best_cost, void *stream) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!d_frames) return fail("bad angular arguments: no frames");
  mipgpu::AngList list;
  if (angular_args_ok(e, nframes, modes, nmodes,
                      d_cost || d_sad || d_satd || d_ang_mode || d_ang_cost || d_best_mode || d_best_cost || (refine && d_tried),
                      &list) != 0)
    return -1;
  if (refine && !mipgpu::ang_seeds_ok(seeds)) return fail("angular: seeds must be 1..%d", MIP_ANGULAR_MAX_SEEDS);
  if (!d_ang_mode != !d_ang_cost) return fail("angular: d_ang_mode and d_ang_cost are given together");
  if (!d_best_mode != !d_best_cost) return fail("angular: d_best_mode and d_best_cost are given together");
  if (!mipgpu::ang_bias_ok(bias)) return fail("angular: the bias is outside 0..%d", (int)mipgpu::kAngMaxBias);
  for (const void *p : {(const void *)d_cost, (const void *)d_sad, (const void *)d_satd, (const void *)d_ang_cost, (const void *)d_best_cost})
    if (reinterpret_cast<uintptr_t>(p) & 3) return fail("angular: int32 outputs must be 4-byte aligned");
  HIP_TRY(hipSetDevice(e->device));
  if (flush_open(e) != 0) return -1;  // (device-API work orders itself after the host calls)
  if (ensure_intra_tables(e) != 0) return -1;
  const bool extended = e->ang_refs.load() == MIP_ANG_REFS_EXTENDED;  // (the two settings of this launch)
  const bool tap4 = e->ang_interp.load() == MIP_ANG_INTERP_4TAP;
  if (extended && ensure_ext_tables(e) != 0) return -1;
  hipStream_t s = (hipStream_t)stream;
  const uint16_t *refs = nullptr;
  bool engine_refs = false;
  if (engine_refs_begin(e, d_frames, d_refs, nframes, s, &refs, &engine_refs) != 0) return -1;
  mipgpu::AngularTap4Args a{};  // (the 2-tap launches take their AngularExtArgs / AngularRefineArgs / AngularArgs part)
  if (tap4) tap4_coefficients(a.coef);  // (one 4-tap kernel per role: no table is the substituted lines)
  a.ext = extended ? e->d_ang_ext[engine_refs ? 1 : 0] : nullptr;
  a.orig = d_frames;
  a.refs = refs;
  a.unavail = e->d_pred_unavail[engine_refs ? 1 : 0];
  a.slots = e->d_intra_slots;
  a.slots_per_block = e->intra_slots_per_block;
  a.cost = d_cost;
  a.sad = d_sad;
  a.satd = d_satd;
  a.ang_mode = d_ang_mode;
  a.ang_cost = d_ang_cost;
  a.best_mode = d_best_mode;
  a.best_cost = d_best_cost;
  a.bias = bias;
  a.width = e->width;
  a.height = e->height;
  a.ctu_cols = e->ctu_cols;
  a.nctus = e->nctus;
  a.nframes = nframes;
  a.nmodes = list.n;
  for (int k = 0; k < 3; k++) a.listed[k] = list.listed[k];
  for (int q = 0; q < list.n; q++) a.modes[q] = list.packed[q];
  if (refine) {
    a.tried = d_tried;
    a.nseeds = std::min(seeds, list.n);
    for (int m = MIP_ANGULAR_FIRST; m <= MIP_ANGULAR_LAST; m++) a.all[m - MIP_ANGULAR_FIRST] = mipgpu::ang_pack(m);
    HIP_TRY(tap4 ? mipgpu::launch_angular_tap4_refine(a, s)
                 : extended ? mipgpu::launch_angular_ext_refine(a, s) : mipgpu::launch_angular_refine(a, s));
  } else {
    HIP_TRY(tap4 ? mipgpu::launch_angular_tap4(a, s) : extended ? mipgpu::launch_angular_ext(a, s) : mipgpu::launch_angular(a, s));
  }
  return engine_refs_end(e, engine_refs, s);
}

int mip_angular_device(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes, const uint8_t *modes,
                       int nmodes, int32_t *d_cost, int32_t *d_sad, int32_t *d_satd, uint8_t *d_ang_mode, int32_t *d_ang_cost,
                       int32_t bias, uint8_t *d_best_mode, int32_t *d_best_cost, void *stream) {
  return angular_device_impl(e, d_frames, d_refs, nframes, modes, nmodes, false, 0, d_cost, d_sad, d_satd, d_ang_mode, d_ang_cost,
                             nullptr, bias, d_best_mode, d_best_cost, stream);
}

int mip_angular_refine_device(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes, const uint8_t *modes,
                              int nmodes, int seeds, int32_t *d_cost, int32_t *d_sad, int32_t *d_satd, uint8_t *d_ang_mode,
                              int32_t *d_ang_cost, uint8_t *d_ang_tried, int32_t bias, uint8_t *d_best_mode, int32_t *d_best_cost,
                              void *stream) {
  return angular_device_impl(e, d_frames, d_refs, nframes, modes, nmodes, true, seeds, d_cost, d_sad, d_satd, d_ang_mode, d_ang_cost,
                             d_ang_tried, bias, d_best_mode, d_best_cost, stream);
}

// Both host calls (refine as in angular_device_impl).  With cost_out the chunk is cut so that
// the call's device table stays within mipgpu::kAngularTableBytes (host_policy.h).
static int angular_frames_impl(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes, const uint8_t *modes,
                               int nmodes, bool refine, int seeds, int32_t *cost_out, uint8_t *ang_mode_out, int32_t *ang_cost_out,
                               uint8_t *tried_out) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!frames) return fail("bad angular arguments: no frames");
  mipgpu::AngList list;
  if (angular_args_ok(e, nframes, modes, nmodes, cost_out || ang_mode_out || ang_cost_out || (refine && tried_out), &list) != 0) return -1;
  if (!ang_mode_out != !ang_cost_out) return fail("angular: ang_mode_out and ang_cost_out are given together");
  if (refine && !mipgpu::ang_seeds_ok(seeds)) return fail("angular: seeds must be 1..%d", MIP_ANGULAR_MAX_SEEDS);
  if (!refine) tried_out = nullptr;
  HIP_TRY(hipSetDevice(e->device));
  if (quiesce(e) != 0) return -1;  // (host searches in flight use the engine buffers)
  const size_t ncu = (size_t)e->nctus * MIP_CUS_PER_CTU, table = ncu * mipgpu::kAngModes * sizeof(int32_t);  // per frame
  const int chunk = mipgpu::stage_chunk_frames(e->opts.max_batch, nframes, cost_out ? table : 0);
  // the call's own device buffers (through the device block cache)
  DevScratch scratch(e->device);
  int32_t *d_cost = nullptr, *d_ang_cost = nullptr;
  uint8_t *d_ang_mode = nullptr, *d_tried = nullptr;
  if (cost_out) HIP_TRY(scratch.take(d_cost, chunk * table));
  if (ang_cost_out) {
    HIP_TRY(scratch.take(d_ang_cost, chunk * ncu * sizeof(int32_t)));
    HIP_TRY(scratch.take(d_ang_mode, chunk * ncu));
  }
  if (tried_out) HIP_TRY(scratch.take(d_tried, chunk * ncu));
  // (without references the device entry point filters the frames itself when the engine has a filter)
  return walk_chunks(e, frames, refs_or_null, nframes, chunk,
                     {{tried_out, d_tried, ncu},
                      {cost_out, d_cost, table},
                      {ang_cost_out, d_ang_cost, ncu * sizeof(int32_t)},
                      {ang_mode_out, d_ang_mode, ncu}},
                     [&](int nb, const uint16_t *d_refs) {
                       return angular_device_impl(e, e->d_frames, d_refs, nb, modes, nmodes, refine, seeds, d_cost, nullptr, nullptr,
                                                  d_ang_mode, d_ang_cost, d_tried, 0, nullptr, nullptr, e->stream);
                     });
}

int mip_angular_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes, const uint8_t *modes,
                       int nmodes, int32_t *cost_out, uint8_t *ang_mode_out, int32_t *ang_cost_out) {
  return angular_frames_impl(e, frames, refs_or_null, nframes, modes, nmodes, false, 0, cost_out, ang_mode_out, ang_cost_out, nullptr);
}

int mip_angular_refine_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes, const uint8_t *modes,
                              int nmodes, int seeds, int32_t *cost_out, uint8_t *ang_mode_out, int32_t *ang_cost_out,
                              uint8_t *tried_out) {
  return angular_frames_impl(e, frames, refs_or_null, nframes, modes, nmodes, true, seeds, cost_out, ang_mode_out, ang_cost_out,
                             tried_out);
}

// ---------------------------------------------------------------- K-best candidate lists
int mip_candidates_device(int width, int height, int nframes, int k, const uint8_t *d_mip_mode, const int32_t *d_mip_cost, int kin,
                          const int32_t *d_intra_cost, const int32_t *intra_bias, const int32_t *d_ang_cost, int32_t ang_bias,
                          uint8_t *d_modes, int32_t *d_costs, void *stream) {
  const mipgpu::CandArgs rule = mipgpu::cand_args(width, height, nframes, k, d_mip_mode, d_mip_cost, kin, d_intra_cost, intra_bias,
                                                  d_ang_cost, ang_bias, d_modes, d_costs);
  if (rule != mipgpu::kCandOk) return fail("%s", mipgpu::cand_args_text(rule));
  mipgpu::CandidatesArgs a{};
  a.mip_mode = d_mip_mode;
  a.mip_cost = d_mip_cost;
  a.kin = d_mip_mode ? kin : 0;
  a.intra_cost = d_intra_cost;
  for (int s = 0; s < mipgpu::kIntraModes; s++) a.intra_bias[s] = d_intra_cost && intra_bias ? intra_bias[s] : 0;
  a.ang_cost = d_ang_cost;
  a.ang_bias = d_ang_cost ? ang_bias : 0;
  a.modes = d_modes;
  a.costs = d_costs;
  a.total_cus = mipgpu::cand_cus(width, height, nframes);
  a.k = k;
  HIP_TRY(mipgpu::launch_candidates(a, (hipStream_t)stream));
  return 0;
}

int mip_candidates_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes, int k, unsigned flags,
                          const int32_t *intra_bias, const uint8_t *ang_modes, int ang_nmodes, int ang_seeds, int32_t ang_bias,
                          uint8_t *modes_out, int32_t *costs_out) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!frames) return fail("bad candidates arguments: no frames");
  if (intra_args_ok(e, nframes, modes_out || costs_out) != 0) return -1;
  switch (mipgpu::cand_chain_args(flags, k, intra_bias, ang_modes, ang_nmodes, ang_seeds, ang_bias)) {
    case mipgpu::kCandChainOk: break;
    case mipgpu::kCandChainFlags: return fail("unknown candidates flags 0x%x", flags);
    case mipgpu::kCandChainK: return fail("%s", mipgpu::cand_args_text(mipgpu::kCandK));
    case mipgpu::kCandChainIntraBias: return fail("%s", mipgpu::cand_args_text(mipgpu::kCandIntraBias));
    case mipgpu::kCandChainModes:
      return fail("angular: modes must be 1..%d strictly increasing mode numbers in %d..%d (or NULL, 0 for all)", MIP_ANGULAR_MODES,
                  MIP_ANGULAR_FIRST, MIP_ANGULAR_LAST);
    case mipgpu::kCandChainSeeds: return fail("angular: seeds must be 0..%d", MIP_ANGULAR_MAX_SEEDS);
    case mipgpu::kCandChainAngBias: return fail("%s", mipgpu::cand_args_text(mipgpu::kCandAngBias));
  }
  const bool regular = (flags & MIP_CAND_REGULAR) != 0, angular = (flags & MIP_CAND_ANGULAR) != 0;
  HIP_TRY(hipSetDevice(e->device));
  if (quiesce(e) != 0) return -1;  // (host searches in flight use the engine buffers)
  if (check_device_status(e) != 0) return -1;  // (an earlier device-API search's violation)
  // the MIP lists: the search's own decisions when one entry is asked for and the engine keeps
  // argmins (best_k 1), else a cost table and the decision lists of length kin from it
  const int kin = std::min(k, mipgpu::kCandMaxKin);
  const bool mip_table = !(kin == 1 && e->opts.best_k == 1);
  const size_t ncu = (size_t)e->nctus * MIP_CUS_PER_CTU;
  const size_t mip_bytes = mip_table ? (size_t)e->nctus * MIP_COSTS_PER_CTU_ABI * sizeof(int32_t) : 0;  // per frame
  const size_t intra_bytes = regular ? ncu * mipgpu::kIntraModes * sizeof(int32_t) : 0;
  const size_t ang_bytes = angular ? ncu * mipgpu::kAngModes * sizeof(int32_t) : 0;
  const int chunk = mipgpu::stage_chunk_frames(e->opts.max_batch, nframes, mip_bytes + intra_bytes + ang_bytes);
  // the call's own device buffers (through the device block cache)
  DevScratch scratch(e->device);
  int32_t *d_table = nullptr, *d_intra = nullptr, *d_ang = nullptr, *d_mip_cost = nullptr, *d_costs = nullptr;
  uint8_t *d_mip_mode = nullptr, *d_modes = nullptr;
  if (mip_table) HIP_TRY(scratch.take(d_table, chunk * mip_bytes));
  if (regular) HIP_TRY(scratch.take(d_intra, chunk * intra_bytes));
  if (angular) HIP_TRY(scratch.take(d_ang, chunk * ang_bytes));
  HIP_TRY(scratch.take(d_mip_cost, chunk * ncu * kin * sizeof(int32_t)));
  HIP_TRY(scratch.take(d_mip_mode, chunk * ncu * kin));
  if (costs_out) HIP_TRY(scratch.take(d_costs, chunk * ncu * k * sizeof(int32_t)));
  if (modes_out) HIP_TRY(scratch.take(d_modes, chunk * ncu * k));
  hipStream_t s = e->stream;
  auto stages = [&](int nb, const uint16_t *d_refs) {
    // (without references every stage filters the frames into e->d_refs itself when the engine has a filter)
    if (search_device_impl(e, e->d_frames, d_refs, nb, d_table, nullptr, nullptr, mip_table ? nullptr : d_mip_mode,
                           mip_table ? nullptr : d_mip_cost, s, d_refs != nullptr, device_status(e)) != 0)
      return -1;
    if (mip_table) {
      const mipgpu::BestArgs b{d_table, d_mip_mode, d_mip_cost, (int)(nb * ncu), kin};
      HIP_TRY(mipgpu::launch_best_modes(b, s));
    }
    if (regular && mip_intra_device(e, e->d_frames, d_refs, nb, d_intra, nullptr, nullptr, nullptr, nullptr, nullptr, s) != 0) return -1;
    if (angular && angular_device_impl(e, e->d_frames, d_refs, nb, ang_modes, ang_nmodes, ang_seeds != 0, ang_seeds, d_ang, nullptr,
                                       nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, s) != 0)
      return -1;
    return mip_candidates_device(e->width, e->height, nb, k, d_mip_mode, d_mip_cost, kin, d_intra, intra_bias, d_ang, ang_bias, d_modes,
                                 d_costs, s);
  };
  if (walk_chunks(e, frames, refs_or_null, nframes, chunk, {{modes_out, d_modes, ncu * k}, {costs_out, d_costs, ncu * k * sizeof(int32_t)}},
                  stages) != 0)
    return -1;
  if (const uint32_t f = take_status(e, mip_engine::kCallRing)) return contract_error(f, "mip_candidates_frames");
  return 0;
}

}  // extern "C"

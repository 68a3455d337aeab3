// mipgpu.cpp -- C-ABI engine (include/mipgpu.h): device set-up, buffers, the upload of the
// planned work lists (work_plan.h), the search's device API with its launch sequence, and the
// filter.
// The host API's pipeline, which replaces main.cpp's OpenCL host loop: host_pipeline.cpp; the
// stages behind the search (prediction, partition, intra costs): host_stages.cpp.
#include "engine.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstring>

#include "angular_plan.h"
#include "mip_tables.h"

thread_local std::string g_err;

int fail(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return -1;
}

namespace {

// the planner's geometry (work_plan.h), shared with the public table queries below
using mipgpu::axis_pos;
using mipgpu::cu_defined;
using mipgpu::kMapAltCaller;
using mipgpu::kMapAltEngine;
using mipgpu::kMapOrig;
using mipgpu::kMaps;
using mipgpu::kShapes;

const char *const kShapeNames[MIP_NUM_SHAPES] = MIP_SHAPE_NAMES;

// Profiling knobs that give wrong tables by design (MIPGPU_SHAPE_FILTER, MIPGPU_NO_PAIRS) are
// honoured only by A/B builds made with KNOBS=-DMIPGPU_PROFILING_KNOBS (the option enters the
// build ID, mip_build_id()); a release build refuses to create an engine while they are set
// (mip_engine_create), so no caller -- CLI, C ABI, Python -- gets a silently wrong table.
#ifdef MIPGPU_PROFILING_KNOBS
constexpr bool kProfilingKnobs = true;
#else
constexpr bool kProfilingKnobs = false;
#endif
const char *const kWrongResultKnobs[] = {"MIPGPU_SHAPE_FILTER", "MIPGPU_NO_PAIRS"};

// The planner's knobs (work_plan.h PlanKnobs), read once per engine (mip_engine_create):
//   MIPGPU_CUT_FACTOR (tuning knob): task size cap = a wave's fair share / factor;
//   MIPGPU_TRANSPOSE=0 (A/B knob): wide CUs are searched as they are;
//   MIPGPU_SHAPE_FILTER="i,j,..." (profiling knob): the search is restricted to those shapes;
//   MIPGPU_NO_PAIRS=1 (profiling knob): tasks keep their prologue but search no mode pair.
mipgpu::PlanKnobs plan_knobs_from_env() {
  mipgpu::PlanKnobs k;
  if (const char *e = getenv("MIPGPU_CUT_FACTOR"); e && atof(e) > 0) k.cut_factor = atof(e);
  if (const char *e = getenv("MIPGPU_TRANSPOSE")) k.transpose_wide = *e != '0';
  if (!kProfilingKnobs) return k;
  if (const char *e = getenv("MIPGPU_NO_PAIRS")) k.no_pairs = *e == '1';
  if (const char *flt = getenv("MIPGPU_SHAPE_FILTER"); flt && *flt) {
    k.shapes = 0;
    for (const char *p = flt; *p;) {
      char *end;
      const long v = strtol(p, &end, 10);
      if (end == p) break;
      if (v >= 0 && v < MIP_NUM_SHAPES) k.shapes |= 1ull << v;
      p = *end ? end + 1 : end;
    }
  }
  return k;
}

bool filter_valid(int f, int k) {
  if (f < 0 || f > 7) return false;
  const bool five = f >= 4;
  return k >= 0 && k < (five ? 3 : 5);
}

// MIPGPU_PIPE_KERNEL (A/B knob) for the host pipeline's chunks: 4 (default) = the four-wave
// twin for small alternating chunks and for decisions-only chunks, 8 = the twin for every
// chunk, 6 = the six-wave kernel on one workgroup per CU for small alternating chunks, 0 = the
// six-wave kernel's full grid throughout.
int pipe_kernel() {
  const char *e = getenv("MIPGPU_PIPE_KERNEL");
  return e && (*e == '0' || *e == '6' || *e == '8') ? *e - '0' : 4;
}

// MIPGPU_EXT_DONE=0 (A/B knob): record the host pipeline's per-chunk completion event as a
// separate marker instead of on the search kernel's dispatch.
bool ext_done_enabled() {
  const char *e = getenv("MIPGPU_EXT_DONE");
  return !(e && *e == '0');
}

bool lpt_order_enabled() {
  const char *e = getenv("MIPGPU_ORDER");  // A/B knob: 0 = raster item order in small launches
  return !(e && *e == '0');
}

// Small launches on 16-wave workgroups, one per CU (MIPGPU_WIDE: 0 = never, 1 = every small
// launch; default: work_plan.h few_items_per_cu).
bool wide_launch(long long items1, int cus) {
  if (cus < 1) return false;  // no 16-wave workgroup fits a CU of this device
  const char *e = getenv("MIPGPU_WIDE");
  if (e && *e == '0') return false;
  if (e && *e == '1') return true;
  return mipgpu::few_items_per_cu(items1, cus);
}

// Work lists for a launch of `nframes`: items (quadrant x slice) for the persistent grid.
// Large launches (>= kPrefetchMinItems items per workgroup at one slice): one slice.
// Small ones take their items longest first, on 8- or 16-wave workgroups (wide_launch); the
// slice count is the one whose predicted makespan (work_plan.h shortest_makespan, per frame
// count, cached) is the shortest.  (Before the LPT order: 1 frame -> 2 slices 5076 frames/s
// at 1080p (1: 4842, 4: 4770).)
const mip_engine::Work &pick_work(mip_engine *e, int nframes, int nrange, bool alt) {
  const int groups = e->resident[alt ? 1 : 0];
  const long long items1 = 4LL * nrange * nframes;  // items at one slice
  if (nrange != e->nctus || items1 >= (long long)mipgpu::kPrefetchMinItems * groups || !lpt_order_enabled())
    return e->work[mipgpu::closest_slices(e->plan.work, items1 < 1000 && nrange != e->nctus ? 2 : 1)];
  const bool wide = wide_launch(items1, e->resident_wide[alt ? 1 : 0]);
  std::vector<int> &cache = e->small_choice[alt ? 1 : 0][wide ? 1 : 0];
  if ((int)cache.size() <= nframes) cache.resize(nframes + 1, -1);
  int &ch = cache[nframes];
  if (ch < 0) ch = mipgpu::shortest_makespan(e->plan.work, wide, nframes, wide ? e->resident_wide[alt ? 1 : 0] : groups);
  return e->work[ch];
}

}  // namespace

// Samples above 10 bits seen by a search launched before this point (the kernels mark
// SearchArgs::status): the costs of that search are not the reference's, so the call that
// notices reports it (sticky until reported, then cleared).  The reference reads the CSV
// samples into unsigned short and its kernels take short* (main.cpp:364-384, intra.cl:17,
// 545), with 10-bit constants throughout (constants.cl:22-23, valueDC = 512, clip 1023);
// this engine's packed 16-bit / f16 arithmetic is exact for 10-bit samples only.
static uint32_t *status_set(mip_engine *e, int set) { return e->h_status + (size_t)set * mipgpu::kStatusWords; }

// Read and clear a status set: 0, or 1 (frame samples) | 2 (reference samples).
uint32_t take_status(mip_engine *e, int set) {
  volatile uint32_t *st = status_set(e, set);
  const uint32_t f = (st[mipgpu::kStatusOrig] ? 1u : 0u) | (st[mipgpu::kStatusRefs] ? 2u : 0u);
  if (f) {
    st[mipgpu::kStatusOrig] = 0;
    st[mipgpu::kStatusRefs] = 0;
  }
  return f;
}

int contract_error(uint32_t flags, const char *what) {
  return fail("input contract: %s samples above 10 bits (> 1023) in a frame searched by %s; its costs are not valid "
              "(samples must be 10-bit values)", (flags & 1) ? "frame" : "reference", what);
}

// Device API: the searches issued since the last check (asynchronous: reported by
// mip_check_input or the next device-API search call).
int check_device_status(mip_engine *e) {
  const uint32_t f = take_status(e, mip_engine::kCallRing);
  return f ? contract_error(f, "a device-API search of this engine") : 0;
}

// Device pointers of the status sets the kernels mark.
uint32_t *device_status(mip_engine *e) { return e->d_status + (size_t)mip_engine::kCallRing * mipgpu::kStatusWords; }

// Device block cache (round 6).  Freeing a large device allocation halves every later
// host <-> device copy of the process on this platform -- 56.4 -> 28.7 GB/s, SDMA and blit
// copies alike, old and new buffers, whatever the NUMA placement or the number of streams
// (tools/free_repro.hip, profiles/r06_free_repro.txt: a standalone HIP program, no engine) --
// until some later page-locked allocation churn restores it, on some boxes only.  Engines are
// created and destroyed by serving processes (a resolution change), so engine buffers of at
// least kCacheMin bytes are not freed: mip_engine_destroy parks them in a process-wide cache,
// and later engines on the same device take the smallest parked block that fits (blocks are
// not split: the process holds at most its largest engine set).  hipMalloc failing for lack of
// memory releases the device's parked blocks and retries; mip_device_cache(device, 1, ...)
// releases them explicitly.  MIPGPU_DEVICE_CACHE=0 (A/B knob): plain hipMalloc / hipFree.
namespace {
constexpr size_t kCacheMin = 16u << 20;
struct BlockCache {
  std::mutex mu;
  std::map<void *, std::pair<int, size_t>> live;      // blocks handed out: (device, bytes)
  std::multimap<std::pair<int, size_t>, void *> idle;  // parked blocks by (device, bytes)
  uint64_t reused = 0;
};
BlockCache &block_cache() {
  static BlockCache *c = new BlockCache();  // (never destroyed: no hipFree at process exit)
  return *c;
}
bool device_cache_enabled() {
  const char *e = getenv("MIPGPU_DEVICE_CACHE");
  return !(e && *e == '0');
}
}  // namespace
// hipMalloc on `device` (the current device) through the cache.
hipError_t dev_malloc(int device, void **p, size_t bytes) {
  if (bytes < kCacheMin || !device_cache_enabled()) return hipMalloc(p, bytes);
  BlockCache &c = block_cache();
  {
    std::lock_guard<std::mutex> lk(c.mu);
    auto it = c.idle.lower_bound({device, bytes});
    if (it != c.idle.end() && it->first.first == device) {
      *p = it->second;
      c.live[*p] = it->first;
      c.idle.erase(it);
      c.reused++;
      return hipSuccess;
    }
  }
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) {  // release the parked blocks, retry
    (void)hipGetLastError();
    std::lock_guard<std::mutex> lk(c.mu);
    for (auto it = c.idle.begin(); it != c.idle.end();)
      if (it->first.first == device) {
        (void)hipFree(it->second);
        it = c.idle.erase(it);
      } else {
        ++it;
      }
    e = hipMalloc(p, bytes);
  }
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> lk(c.mu);
    c.live[*p] = {device, bytes};
  }
  return e;
}
void dev_free(void *p) {
  if (!p) return;
  BlockCache &c = block_cache();
  {
    std::lock_guard<std::mutex> lk(c.mu);
    auto it = c.live.find(p);
    if (it != c.live.end()) {
      c.idle.insert({it->second, p});
      c.live.erase(it);
      return;
    }
  }
  (void)hipFree(p);
}

namespace {
// One planned array (work_plan.h) on the device: a block from dev_malloc -- at least one
// element, so that no list pointer is null -- holding a copy of `v`.
template <class T>
int upload(int device, T *&d, const std::vector<T> &v, const char *what) {
  const size_t bytes = v.size() * sizeof(T);
  hipError_t err = dev_malloc(device, (void **)&d, std::max(bytes, sizeof(T)));
  if (err == hipSuccess && bytes) err = hipMemcpy(d, v.data(), bytes, hipMemcpyHostToDevice);
  return err == hipSuccess ? 0 : fail("uploading %s (%zu bytes) failed: %s", what, bytes, hipGetErrorString(err));
}
}  // namespace

// NUMA placement of a device (numa_place.h; none when the bus id or its node is unknown).
static mipgpu::NumaPlace device_place(int device) {
  char bus[64] = {};
  if (hipDeviceGetPCIBusId(bus, sizeof bus, device) != hipSuccess) {
    (void)hipGetLastError();
    return mipgpu::NumaPlace();
  }
  return mipgpu::numa_place_of_pci(bus);
}

extern "C" {

void mip_opts_default(mip_opts *o) {
  if (!o) return;
  o->filter = MIP_FILTER_NONE;
  o->kernel_idx = 0;
  o->max_batch = 1;
  o->want_sad_satd = 0;
  o->slices_per_ctu = 0;
  o->best_k = 1;
}

const char *mip_last_error(void) { return g_err.c_str(); }
int mip_abi_version(void) { return MIPGPU_ABI_VERSION; }
#ifndef MIPGPU_BUILD_ID
#define MIPGPU_BUILD_ID "src:unversioned"
#endif
const char *mip_build_id(void) { return MIPGPU_BUILD_ID; }

int mip_num_ctus(int width, int height) { return ((width + 127) / 128) * ((height + 127) / 128); }
int64_t mip_costs_per_frame(int width, int height) { return (int64_t)mip_num_ctus(width, height) * MIP_COSTS_PER_CTU; }
int64_t mip_cus_per_frame(int width, int height) { return (int64_t)mip_num_ctus(width, height) * MIP_CUS_PER_CTU; }

const char *mip_shape_name(int shape) {
  return shape >= 0 && shape < MIP_NUM_SHAPES ? kShapeNames[shape] : "ERROR";
}

int mip_shape_info(int shape, int *w, int *h, int *modes, int *ncu, int *cost_offset) {
  if (shape < 0 || shape >= MIP_NUM_SHAPES) return fail("bad shape index %d", shape);
  const mip_shape_desc &s = kShapes[shape];
  if (w) *w = s.w;
  if (h) *h = s.h;
  if (modes) *modes = s.modes;
  if (ncu) *ncu = s.ncu;
  if (cost_offset) *cost_offset = (int)s.cost_offset;
  return 0;
}

int mip_unavailable_cus(int width, int height, int filter, uint8_t *cu_out) {
  if (!cu_out || width <= 0 || height <= 0 || width % 4 || height % 4) return fail("bad unavailable-CU arguments");
  if (filter < MIP_FILTER_NONE || filter > MIP_FILTER_2D_FLOAT_5x5) return fail("invalid filter %d", filter);
  const mipgpu::Poison ps = mipgpu::filter_poison(width, height, filter);
  const int cols = (width + 127) / 128, n = mip_num_ctus(width, height);
  size_t k = 0;
  for (int c = 0; c < n; c++) {
    const int cx = 128 * (c % cols), cy = 128 * (c / cols);
    for (int s = 0; s < MIP_NUM_SHAPES; s++) {
      const mip_shape_desc &sd = kShapes[s];
      for (int cu = 0; cu < sd.ncu; cu++, k++) {
        const int x = cx + axis_pos(sd.xb, sd.xs, sd.xd, cu % sd.ncols), y = cy + axis_pos(sd.yb, sd.ys, sd.yd, cu / sd.ncols);
        cu_out[k] = !cu_defined(width, height, x, y, sd.w, sd.h) || mipgpu::reads_poison(ps, width, x, y, sd.w, sd.h);
      }
    }
  }
  return 0;
}

int mip_extended_refs(int width, int height, int filter, uint8_t *top_out, uint8_t *left_out) {
  if ((!top_out && !left_out) || width <= 0 || height <= 0 || width % 4 || height % 4) return fail("bad extended-reference arguments");
  if (filter < MIP_FILTER_NONE || filter > MIP_FILTER_2D_FLOAT_5x5) return fail("invalid filter %d", filter);
  const mipgpu::Poison ps = mipgpu::filter_poison(width, height, filter);
  const auto undefined = [&](long long li) { return ps.any && ps.at(li, width); };
  const int cols = (width + 127) / 128, n = mip_num_ctus(width, height);
  size_t k = 0;
  for (int c = 0; c < n; c++) {
    const int cx = 128 * (c % cols), cy = 128 * (c / cols);
    for (int s = 0; s < MIP_NUM_SHAPES; s++) {
      const mip_shape_desc &sd = kShapes[s];
      for (int cu = 0; cu < sd.ncu; cu++, k++) {
        const int x = cx + axis_pos(sd.xb, sd.xs, sd.xd, cu % sd.ncols), y = cy + axis_pos(sd.yb, sd.ys, sd.yd, cu / sd.ncols);
        const bool off = !cu_defined(width, height, x, y, sd.w, sd.h) || mipgpu::reads_poison(ps, width, x, y, sd.w, sd.h);
        const mipgpu::AngExt e = mipgpu::ang_ext_lengths(width, height, x, y, sd.w, sd.h, off, undefined);
        if (top_out) top_out[k] = (uint8_t)e.top;
        if (left_out) left_out[k] = (uint8_t)e.left;
      }
    }
  }
  return 0;
}

int mip_angular_refs(mip_engine *e, int refs) {
  if (!e) return fail("engine is NULL");
  if (refs != MIP_ANG_REFS_SUBSTITUTED && refs != MIP_ANG_REFS_EXTENDED) return fail("unknown angular reference setting %d", refs);
  std::lock_guard<std::recursive_mutex> lk(e->mu);  // (a call in progress on another thread keeps one setting throughout)
  e->ang_refs.store(refs);
  return 0;
}

int mip_angular_refs_get(const mip_engine *e) {
  if (!e) return fail("engine is NULL");
  return e->ang_refs.load();
}

int mip_angular_interp(mip_engine *e, int interp) {
  if (!e) return fail("engine is NULL");
  if (interp != MIP_ANG_INTERP_2TAP && interp != MIP_ANG_INTERP_4TAP) return fail("unknown angular interpolation setting %d", interp);
  std::lock_guard<std::recursive_mutex> lk(e->mu);  // (a call in progress on another thread keeps one setting throughout)
  e->ang_interp.store(interp);
  return 0;
}

int mip_angular_interp_get(const mip_engine *e) {
  if (!e) return fail("engine is NULL");
  return e->ang_interp.load();
}

int mip_angular_filter(int lw, int lh, int mode) {
  if (lw < 2 || lw > 6 || lh < 2 || lh > 6 || mode < MIP_ANGULAR_FIRST || mode > MIP_ANGULAR_LAST)
    return fail("angular filter: lw and lh are 2..6, the mode %d..%d", MIP_ANGULAR_FIRST, MIP_ANGULAR_LAST);
  return mipgpu::ang_filter_gauss(mode, lw, lh) ? 1 : 0;
}

int mip_cu_position(int shape, int cu, int *x, int *y) {
  if (shape < 0 || shape >= MIP_NUM_SHAPES) return fail("bad shape index %d", shape);
  const mip_shape_desc &s = kShapes[shape];
  if (cu < 0 || cu >= s.ncu) return fail("bad cu index %d for shape %d", cu, shape);
  if (x) *x = axis_pos(s.xb, s.xs, s.xd, cu % s.ncols);
  if (y) *y = axis_pos(s.yb, s.ys, s.yd, cu / s.ncols);
  return 0;
}

int mip_engine_destroy(mip_engine *e) {
  if (!e) return 0;
  {  // the open chunk is launched (its calls were accepted)
    std::lock_guard<std::recursive_mutex> lk(e->mu);
    (void)hipSetDevice(e->device);
    (void)flush_open(e);
  }
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->stream2) (void)hipStreamSynchronize(e->stream2);
  if (e->stream3) (void)hipStreamSynchronize(e->stream3);
  if (e->stream4) (void)hipStreamSynchronize(e->stream4);
  e->stage.abandon();
  for (void *p : {(void *)e->d_frames, (void *)e->d_refs, (void *)e->d_costs, (void *)e->d_sad,
                  (void *)e->d_satd, (void *)e->d_best, (void *)e->d_best_cost, (void *)e->d_split_acc,
                  (void *)e->d_tables})
    dev_free(p);
  for (int m = 0; m < kMaps; m++) {
    dev_free(e->d_ctu_var[m]);
    dev_free(e->d_fixup[m]);
  }
  if (e->d_pred_unavail[1] != e->d_pred_unavail[0]) dev_free(e->d_pred_unavail[1]);
  dev_free(e->d_pred_unavail[0]);
  dev_free(e->d_pred_geo);
  if (e->d_ang_ext[1] != e->d_ang_ext[0]) dev_free(e->d_ang_ext[1]);
  dev_free(e->d_ang_ext[0]);
  dev_free(e->d_part_leaf);
  dev_free(e->d_part_ctu);
  dev_free(e->d_intra_slots);
  dev_free(e->d_queue);
  if (e->h_status) (void)hipHostFree(e->h_status);
  if (e->h_frame_status) (void)hipHostFree(e->h_frame_status);
  for (hipEvent_t ev : e->queue_done)
    if (ev) (void)hipEventDestroy(ev);
  if (e->refs_done) (void)hipEventDestroy(e->refs_done);
  for (int i = 0; i < mip_engine::kHostSlots; i++)
    for (hipEvent_t ev : {e->slot_up[i], e->slot_comp[i], e->slot_down[i]})
      if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : e->call_done)
    if (ev) (void)hipEventDestroy(ev);
  for (auto &evs : e->tr_ev)
    for (hipEvent_t ev : evs)
      if (ev) (void)hipEventDestroy(ev);
  for (const mip_engine::Work &w : e->work)
    for (void *p : {(void *)w.d_tasks, (void *)w.d_jobs, (void *)w.d_lists, (void *)w.d_fill, (void *)w.d_fill_begin,
                    (void *)w.d_dfill, (void *)w.d_dfill_begin, (void *)w.d_split, (void *)w.d_split_begin,
                    (void *)w.d_order})
      dev_free(p);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  if (e->stream2) (void)hipStreamDestroy(e->stream2);
  if (e->stream3) (void)hipStreamDestroy(e->stream3);
  if (e->stream4) (void)hipStreamDestroy(e->stream4);
  delete e;
  return 0;
}

int mip_engine_create(int device, int width, int height, const mip_opts *opts, mip_engine **out) {
  if (!out) return fail("out is NULL");
  *out = nullptr;
  if (width <= 0 || height <= 0 || width % 4 || height % 4)
    return fail("frame size %dx%d must be positive multiples of 4", width, height);
  // 32-bit linear sample indexes in the kernels (the window reaches 128 columns and 64 rows
  // past the frame)
  if ((long long)(width + 128) * (height + 128) >= (1LL << 31))
    return fail("frame size %dx%d too large (linear sample index beyond 2^31)", width, height);
  mip_opts o;
  mip_opts_default(&o);
  if (opts) o = *opts;
  if (o.max_batch < 1) return fail("max_batch must be >= 1");
  if ((long long)o.max_batch * mip_num_ctus(width, height) * MIP_CUS_PER_CTU > kMaxCus)
    return fail("max_batch %d x %d CTUs exceeds %lld CUs per launch", o.max_batch, mip_num_ctus(width, height), kMaxCus);
  if (o.best_k == 0) o.best_k = 1;
  if (o.best_k < 1 || o.best_k > mipgpu::kMaxBestK) return fail("best_k %d out of range 1..%d", o.best_k, mipgpu::kMaxBestK);
  if (o.filter != MIP_FILTER_NONE) {
    if (!filter_valid(o.filter, o.kernel_idx)) return fail("invalid filter %d / kernel_idx %d", o.filter, o.kernel_idx);
  }
  if (!kProfilingKnobs)
    for (const char *k : kWrongResultKnobs)
      if (const char *v = getenv(k); v && *v)
        return fail("%s is set: a profiling knob that makes wrong cost tables by design, honoured only by A/B builds "
                    "(make KNOBS=-DMIPGPU_PROFILING_KNOBS); this release build refuses to run with it -- unset it", k);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail("device %d out of range (%d devices)", device, ndev);
  HIP_TRY(hipSetDevice(device));

  mip_engine *e = new mip_engine();
  e->device = device;
  e->place = device_place(device);
  e->stage.set_device(device);  // (the bounce ring's completion thread)
  e->stage.set_place(e->place);
  e->width = width;
  e->height = height;
  e->nctus = mip_num_ctus(width, height);
  e->ctu_cols = (width + 127) / 128;
  e->opts = o;
  // host pipeline slots (see mip_engine::hp_slots); the engine buffers hold all of them
  e->hp_slots = o.max_batch >= 16 ? 4 : 3;
  e->hp_cap = o.max_batch >= 16 ? o.max_batch / 4 : o.max_batch;
  e->hp_frames = std::max(o.max_batch, e->hp_slots * e->hp_cap);
  const size_t fs = (size_t)width * height, nb = (size_t)e->hp_frames;
  const size_t ncost = nb * e->nctus * MIP_COSTS_PER_CTU, ncu = nb * e->nctus * MIP_CUS_PER_CTU;
  auto cleanup = [&](int rc) { mip_engine_destroy(e); return rc; };
#define ALLOC(ptr, bytes)                                                               \
  do {                                                                                  \
    hipError_t _e = dev_malloc(device, (void **)&(ptr), (bytes));                       \
    if (_e != hipSuccess) return cleanup(fail("hipMalloc(%zu): %s", (size_t)(bytes), hipGetErrorString(_e))); \
  } while (0)
  {
    // The engine's streams are created with the device's greatest priority.  HIP maps streams
    // onto a few hardware queues per priority (GPU_MAX_HW_QUEUES, 4 on the MI355X boxes); a
    // process that already holds many streams of the default priority -- torch creates a pool
    // of 32 per priority level at its first torch.cuda.Stream() -- then shares those queues
    // with the engine's streams, and the host pipeline's downloads -- blit kernels on the
    // runtime torch's wheel bundles, which then serves the engine (DESIGN.md section 6,
    // pageable host buffers, round 5) -- queued behind the searches on a shared queue:
    // 8 queued 1-frame 1080p full-table calls 830 instead of 1000 frames/s,
    // the configs[2] shape 570-894 instead of 1026 (tools/e2e_probe.py --torch stream,
    // gpurun_out/r05l).  With an explicit priority both rates are restored (high or low alike;
    // high, so that a serving engine is not starved by other work).  MIPGPU_STREAM_PRIO
    // (A/B knob): "low" / "normal" (the plain default streams).
    int lo = 0, hi = 0, prio = 0;
    bool with_prio = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess;
    prio = hi;
    if (const char *sp = getenv("MIPGPU_STREAM_PRIO")) {
      if (!strcmp(sp, "low")) prio = lo;
      else if (!strcmp(sp, "normal")) with_prio = false;
    }
    for (hipStream_t *st : {&e->stream, &e->stream2, &e->stream3, &e->stream4})
      if ((with_prio ? hipStreamCreateWithPriority(st, hipStreamNonBlocking, prio)
                     : hipStreamCreateWithFlags(st, hipStreamNonBlocking)) != hipSuccess)
        return cleanup(fail("hipStreamCreate failed"));
  }
  // The slot events order the engine's own streams on this device only (uploads -> search ->
  // downloads; the kernels' dispatch packets carry the device-scope cache fences).
  // MIPGPU_SLOT_EVENTS (A/B knob): "nofence" drops their system-scope fences
  // (hipEventDisableSystemFence), "device" releases to device scope (hipEventReleaseToDevice).
  unsigned slot_flags = hipEventDisableTiming;
  if (const char *se = getenv("MIPGPU_SLOT_EVENTS")) {
    if (!strcmp(se, "nofence")) slot_flags |= hipEventDisableSystemFence;
    else if (!strcmp(se, "device")) slot_flags |= hipEventReleaseToDevice;
  }
  for (int i = 0; i < mip_engine::kHostSlots; i++)
    for (hipEvent_t *ev : {&e->slot_up[i], &e->slot_comp[i], &e->slot_down[i]})
      if (hipEventCreateWithFlags(ev, slot_flags) != hipSuccess) return cleanup(fail("hipEventCreate failed"));
  for (hipEvent_t &ev : e->call_done)
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return cleanup(fail("hipEventCreate failed"));
  ALLOC(e->d_frames, fs * nb * 2);  // (through the device block cache, dev_malloc)
  if (o.filter != MIP_FILTER_NONE) ALLOC(e->d_refs, fs * nb * 2);
  ALLOC(e->d_costs, ncost * 4);
  if (o.want_sad_satd) {
    ALLOC(e->d_sad, ncost * 4);
    ALLOC(e->d_satd, ncost * 4);
  }
  ALLOC(e->d_best, ncu * o.best_k);
  ALLOC(e->d_queue, mipgpu::kQueueWords * 3 * mip_engine::kQueueSlots * sizeof(uint32_t));
  if (hipMemset(e->d_queue, 0, mipgpu::kQueueWords * 3 * mip_engine::kQueueSlots * sizeof(uint32_t)) != hipSuccess)
    return cleanup(fail("hipMemset failed"));
  // Every engine stream takes its hardware queue now, and the copy streams their copy
  // engines (1 MiB each way through a page-locked buffer): HIP sets these up at their first
  // use (tools/experiments/r05/_r05ao.sh: the CLI's first download started 8-9 ms after the search it
  // waited for).  (The counters are zero: rewriting one is harmless.)
  {
    void *h = nullptr;
    const size_t nbytes = std::min<size_t>(1u << 20, fs * nb * 2);  // (d_frames' size)
    bool ok = hipHostMalloc(&h, nbytes, hipHostMallocDefault) == hipSuccess;
    for (hipStream_t st : {e->stream, e->stream4})
      ok = ok && hipMemsetAsync(e->d_queue, 0, sizeof(uint32_t), st) == hipSuccess;
    ok = ok && hipMemcpyAsync(e->d_frames, h, nbytes, hipMemcpyHostToDevice, e->stream2) == hipSuccess &&
         hipStreamSynchronize(e->stream2) == hipSuccess &&
         hipMemcpyAsync(h, e->d_frames, nbytes, hipMemcpyDeviceToHost, e->stream3) == hipSuccess;
    for (hipStream_t st : {e->stream, e->stream2, e->stream3, e->stream4})
      ok = ok && hipStreamSynchronize(st) == hipSuccess;
    if (h) (void)hipHostFree(h);
    if (!ok) return cleanup(fail("initialising the engine streams failed"));
  }
  for (hipEvent_t &ev : e->queue_done)
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return cleanup(fail("hipEventCreate failed"));
  const size_t status_bytes = (size_t)(mip_engine::kCallRing + 1) * mipgpu::kStatusWords * sizeof(uint32_t);
  const mipgpu::ScopedNodePolicy pol(e->place);  // (the engine's page-locked words on its node)
  const unsigned numa_flag = pol.applied() ? hipHostMallocNumaUser : 0u;
  if (hipHostMalloc((void **)&e->h_status, status_bytes, hipHostMallocMapped | hipHostMallocCoherent | numa_flag) !=
      hipSuccess)
    return cleanup(fail("hipHostMalloc (status words) failed"));
  memset(e->h_status, 0, status_bytes);
  if (hipHostGetDevicePointer((void **)&e->d_status, e->h_status, 0) != hipSuccess || !e->d_status)
    return cleanup(fail("hipHostGetDevicePointer (status words) failed"));
  {  // merged chunks' per-frame status pointers (mip_engine::h_frame_status)
    const size_t bytes = (size_t)mip_engine::kCallRing * e->hp_cap * sizeof(uint32_t *);
    if (hipHostMalloc((void **)&e->h_frame_status, bytes, hipHostMallocMapped | hipHostMallocCoherent | numa_flag) !=
        hipSuccess)
      return cleanup(fail("hipHostMalloc (frame status) failed"));
    memset(e->h_frame_status, 0, bytes);
    if (hipHostGetDevicePointer((void **)&e->d_frame_status, e->h_frame_status, 0) != hipSuccess || !e->d_frame_status)
      return cleanup(fail("hipHostGetDevicePointer (frame status) failed"));
  }
  if (hipEventCreateWithFlags(&e->refs_done, hipEventDisableTiming) != hipSuccess)
    return cleanup(fail("hipEventCreate failed"));
  for (int alt = 0; alt < 2; alt++) {
    if ((e->resident[alt] = mipgpu::search_resident_groups(alt != 0, false)) < 1)
      return cleanup(fail("cannot size the persistent search grid on device %d", device));
    // 16-wave workgroups (small launches) are optional: 0 when one does not fit a CU
    e->resident_wide[alt] = mipgpu::search_resident_groups(alt != 0, true);
    e->resident_four[alt] = mipgpu::search_resident_groups_four(alt != 0, false);
  }
  ALLOC(e->d_best_cost, ncu * o.best_k * 4);
  ALLOC(e->d_split_acc, ncu * 4);
  if (hipMemset(e->d_split_acc, 0xff, ncu * 4) != hipSuccess) return cleanup(fail("hipMemset failed"));
#undef ALLOC
  // What the search computes (work_plan.h), planned once; the device blocks are taken in a
  // fixed order (the block cache hands out blocks by size).
  e->plan = mipgpu::plan_engine(width, height, o.filter,
                                o.slices_per_ctu > 0 ? std::vector<int>{o.slices_per_ctu} : std::vector<int>{1, 2, 4},
                                plan_knobs_from_env());
  const mipgpu::CtuVariants &cv = e->plan.cv;
  if (cv.pattern.size() > (size_t)mipgpu::kMaxCtuVariants)
    return cleanup(fail("too many CTU variants (%zu)", cv.pattern.size()));
  for (int m = 0; m < kMaps; m++) {
    if (upload(device, e->d_ctu_var[m], cv.of_ctu[m], "CTU variants") != 0) return cleanup(-1);
    e->nfixup[m] = (int)cv.fixup[m].size();
    if (e->nfixup[m] && upload(device, e->d_fixup[m], cv.fixup[m], "fixup CUs") != 0) return cleanup(-1);
  }
  for (const mipgpu::WorkPlan &wp : e->plan.work) {
    e->work.emplace_back();
    mip_engine::Work &ew = e->work.back();
    ew.host = &wp;
    if (upload(device, ew.d_tasks, wp.tasks, "tasks") != 0 || upload(device, ew.d_jobs, wp.jobs, "jobs") != 0 ||
        upload(device, ew.d_lists, wp.list_begin, "task lists") != 0 || upload(device, ew.d_fill, wp.fill, "fill entries") != 0 ||
        upload(device, ew.d_fill_begin, wp.fill_begin, "fill lists") != 0 ||
        upload(device, ew.d_order, wp.order, "the item order") != 0 ||
        upload(device, ew.d_dfill, wp.dfill, "undefined CUs") != 0 ||
        upload(device, ew.d_dfill_begin, wp.dfill_begin, "undefined-CU lists") != 0 ||
        upload(device, ew.d_split, wp.split, "split CUs") != 0 ||
        upload(device, ew.d_split_begin, wp.split_begin, "split-CU lists") != 0)
      return cleanup(-1);
    if (getenv("MIPGPU_WORK_STATS"))  // diagnostic: list sizes per slice count
      fprintf(stderr, "mipgpu work %dx%d slices %d: %zu tasks, %zu jobs, %zu fill, %zu undefined CUs, %zu split CUs (max %d per CTU)\n",
              width, height, wp.slices, wp.tasks.size(), wp.jobs.size(), wp.fill.size(), wp.dfill.size(), wp.split.size(),
              wp.max_split);
  }
  if (upload(device, e->d_tables, mipgpu::build_tables(), "static tables") != 0) return cleanup(-1);
  *out = e;
  return 0;
}

int mip_topk_device(const int32_t *d_costs, int width, int height, int nframes, int k, uint8_t *d_modes,
                    int32_t *d_costs_k, void *stream) {
  if (!d_costs || nframes < 1 || width <= 0 || height <= 0) return fail("bad top-k arguments");
  if (k < 1 || k > mipgpu::kMaxBestK) return fail("k %d out of range 1..%d", k, mipgpu::kMaxBestK);
  if (!d_modes && !d_costs_k) return 0;
  const long long cus = (long long)nframes * mip_num_ctus(width, height) * MIP_CUS_PER_CTU;
  if (cus > kMaxCus) return fail("too many CUs");
  mipgpu::BestArgs b{d_costs, d_modes, d_costs_k, (int)cus, k};
  HIP_TRY(mipgpu::launch_best_modes(b, (hipStream_t)stream));
  return 0;
}

int mip_copy_device(const void *d_src, void *d_dst, size_t bytes, void *stream) {
  if (!d_src || !d_dst) return fail("bad copy arguments");
  HIP_TRY(mipgpu::launch_copy(d_src, d_dst, bytes, (hipStream_t)stream));
  return 0;
}

int mip_filter_device(const uint16_t *d_in, uint16_t *d_out, int width, int height, int nframes,
                      int filter, int kernel_idx, void *stream) {
  if (!d_in || !d_out || nframes < 1) return fail("bad filter arguments");
  if (!filter_valid(filter, kernel_idx)) return fail("invalid filter %d / kernel_idx %d", filter, kernel_idx);
  mipgpu::FilterArgs a{d_in, d_out, width, height, nframes, filter, kernel_idx};
  HIP_TRY(mipgpu::launch_filter(a, (hipStream_t)stream));
  return 0;
}

}  // extern "C"

// The reference frames of a device-API stage (search, prediction, intra costs): the caller's,
// the originals, or -- *engine_refs -- the engine's filter applied into the engine's reference
// scratch, ordered after that scratch's previous users: this is the rule that keeps two writers
// of d_refs on different streams apart (mip_engine::refs_done).  The stage then records refs_done
// behind its last kernel that reads the scratch (engine_refs_end).
int engine_refs_begin(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes, hipStream_t s,
                      const uint16_t **refs, bool *engine_refs) {
  *refs = d_refs ? d_refs : d_frames;
  *engine_refs = !d_refs && e->opts.filter != MIP_FILTER_NONE;
  if (!*engine_refs) return 0;
  if (nframes > e->opts.max_batch) return fail("nframes %d > max_batch %d", nframes, e->opts.max_batch);
  if (e->refs_pending) HIP_TRY(hipStreamWaitEvent(s, e->refs_done, 0));  // last reader of d_refs
  if (e->host_pending)  // host calls in flight (calls complete in order: the last one)
    HIP_TRY(hipStreamWaitEvent(s, e->call_done[(e->host_calls - 1) % mip_engine::kCallRing], 0));
  if (mip_filter_device(d_frames, e->d_refs, e->width, e->height, nframes, e->opts.filter, e->opts.kernel_idx, s) != 0)
    return -1;
  *refs = e->d_refs;
  return 0;
}
int engine_refs_end(mip_engine *e, bool engine_refs, hipStream_t s) {
  if (engine_refs) {
    HIP_TRY(hipEventRecord(e->refs_done, s));
    e->refs_pending = true;
  }
  return 0;
}

int search_device_impl(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes, int32_t *d_costs,
                       int32_t *d_sad, int32_t *d_satd, uint8_t *d_best, int32_t *d_best_cost, hipStream_t s,
                       bool caller_refs, uint32_t *d_status, int ctu0, int nrange, uint32_t *split_acc,
                       mipgpu::SplitArgs *defer_split, hipEvent_t *done, uint32_t *const *frame_status,
                       bool alternating) {
  if (!e || !d_frames || nframes < 1) return fail("bad search arguments");
  // Decisions only (no cost table): the search writes each CU's decision into d_best /
  // d_best_cost; CUs whose mode pairs are cut over several tasks keep a packed running argmin
  // (cost << 5 | mode) in d_best_cost, set to all ones before and unpacked after the search.
  const bool decisions_only = d_costs == nullptr;
  if (decisions_only) {
    if (!d_best_cost) return fail("a search without d_costs needs d_best_cost (decisions only)");
    if (e->opts.best_k != 1) return fail("a search without d_costs needs best_k == 1 (got %d)", e->opts.best_k);
    if (d_sad || d_satd) return fail("a search without d_costs cannot produce SAD / SATD tables");
  }
  if (nrange < 0) nrange = e->nctus - ctu0;
  if (ctu0 < 0 || nrange < 1 || ctu0 + nrange > e->nctus)
    return fail("CTU range [%d, %d) outside the frame's %d CTUs", ctu0, ctu0 + nrange, e->nctus);
  const long long total_cus = (long long)nframes * e->nctus * MIP_CUS_PER_CTU;
  if (total_cus > kMaxCus) return fail("%d frames x %d CTUs exceed %lld CUs per launch", nframes, e->nctus, kMaxCus);
  const uint16_t *refs = nullptr;
  bool engine_refs = false;
  if (engine_refs_begin(e, d_frames, d_refs, nframes, s, &refs, &engine_refs) != 0) return -1;
  const bool alt = refs != d_frames;
  mipgpu::SearchArgs a{};
  a.orig = d_frames;
  a.refs = refs;
  a.cost = d_costs;
  a.best_mode = decisions_only ? d_best : nullptr;
  a.best_cost = decisions_only ? d_best_cost : nullptr;
  a.sad = d_sad;
  a.satd = d_satd;
  const mip_engine::Work &work = pick_work(e, nframes, nrange, alt);
  const mipgpu::WorkPlan &wp = *work.host;
  int resident = wp.wide ? e->resident_wide[alt ? 1 : 0] : e->resident[alt ? 1 : 0];
  // Host-pipeline chunks whose searches alternate between the two search streams and are too
  // small to prefetch (round 6).  At six waves per SIMD a full grid of the batched kernel
  // leaves no room on a CU for the next chunk's workgroups nor for the download stream's
  // unpacking / copy kernels, which wait for the search to drain (a kernel trace of 8 merged
  // one-frame calls: dec_split busy 1.3 ms instead of 28 us).  Such chunks run the four-wave
  // twin (8-wave workgroups, two per CU: the occupancy rounds 1-5 ran the whole pipeline at),
  // or -- MIPGPU_PIPE_KERNEL=6 -- one 12-wave workgroup per CU (8 queued one-frame
  // decisions-only calls 4740 -> 5100 frames/s, 32 calls 5550 -> 6340).
  const bool pipe_small = alternating && !wp.wide &&
                          (long long)4 * wp.slices * nrange * nframes < (long long)mipgpu::kPrefetchMinItems * resident;
  const int pk = pipe_kernel();
  // (decisions-only pipeline chunks of any size too: their downloads -- blit kernels on torch's
  // runtime -- and split unpacking run beside the next chunk's search; 8 queued 128-frame
  // calls 7097-7121 -> 7191-7247 frames/s, tools/experiments/r06/e2e_twin.sh; full-table
  // chunks are PCIe-bound either way and keep the six-wave kernel)
  const bool four = ((pk == 4 && (pipe_small || (decisions_only && done))) || (pk == 8 && done)) && !wp.wide &&
                    e->resident_four[alt ? 1 : 0] > 0;
  if (four) resident = e->resident_four[alt ? 1 : 0];
  else if (pipe_small && pk == 6) resident = std::max(1, resident / 2);
  a.tasks = work.d_tasks;
  a.jobs = work.d_jobs;
  a.list_begin = work.d_lists;
  a.fill = work.d_fill;
  a.fill_begin = work.d_fill_begin;
  a.dfill = work.d_dfill;
  a.dfill_begin = work.d_dfill_begin;
  a.tables = reinterpret_cast<const uint4 *>(e->d_tables);
  // engine-filtered references (here or in the host pipeline) leave the CUs that read the
  // filter's undefined samples unavailable; caller-supplied references are taken as they are
  const int map = !alt ? kMapOrig : (caller_refs ? kMapAltCaller : kMapAltEngine);
  a.ctu_var = e->d_ctu_var[map];
  a.width = e->width;
  a.height = e->height;
  a.ctu_cols = e->ctu_cols;
  a.nctus = e->nctus;
  a.ctu0 = ctu0;
  a.nrange = nrange;
  a.slices = wp.slices;
  a.status = d_status;  // the calling API's status set (mip_engine::h_status)
  a.frame_status = frame_status;  // merged chunks: each frame's own call's set
  a.check_refs = alt && caller_refs;
  a.order = lpt_order_enabled() ? work.d_order : nullptr;  // launch_search drops it for large / range launches
  // pair mode of 16-wave launches (original references; launch_search checks the rest)
  const char *pv = getenv("MIPGPU_PAIR");  // A/B knob: 0 = 16-wave launches take items one at a time
  a.nonempty = wp.wide && !alt && a.order && !(pv && *pv == '0') ? wp.nonempty * (uint32_t)nframes : 0;
  // MIPGPU_WAVE_TIMING=file (profiling): per-task cycles appended to `file` (synchronous;
  // one binary record of uint64 [workgroup][wave][kClockSlots] per launch), and the task
  // lists to `file`.tasks once.
  static const char *timing = getenv("MIPGPU_WAVE_TIMING");
  std::vector<uint64_t> clocks;
  if (timing) {
    const size_t n = (size_t)4 * wp.slices * nrange * nframes * mipgpu::kClockSlots;
    HIP_TRY(hipMalloc((void **)&a.wave_clock, n * 8));
    HIP_TRY(hipMemsetAsync(a.wave_clock, 0, n * 8, s));
    clocks.resize(n);
    static std::atomic<bool> dumped{false};
    if (!dumped.exchange(true)) {
      if (FILE *f = fopen((std::string(timing) + ".tasks").c_str(), "w")) {
        fprintf(f, "{\"slices\": %d, \"list_begin\": [", wp.slices);
        for (size_t i = 0; i < wp.list_begin.size(); i++) fprintf(f, "%s%d", i ? ", " : "", wp.list_begin[i]);
        fprintf(f, "], \"tasks\": [");
        for (size_t i = 0; i < wp.tasks.size(); i++)
          fprintf(f, "%s[%d, %d, %d, %d]", i ? ", " : "", wp.tasks[i].cls, wp.tasks[i].ncu, wp.tasks[i].q0, wp.tasks[i].q1);
        fprintf(f, "]}\n");
        fclose(f);
      }
    }
  }
  // split_acc + defer_split (host pipeline): the split CUs meet in split_acc, which holds all
  // ones outside the launches in flight, and the caller unpacks (and re-initialises) it on
  // its download stream -- no kernel but the search on the search stream
  if (decisions_only && split_acc && defer_split) a.split_acc = split_acc;
  else defer_split = nullptr;
  const mipgpu::SplitArgs sa{work.d_split, work.d_split_begin, a.ctu_var, d_best, d_best_cost,
                             e->nctus, ctu0, nrange, wp.max_split, a.split_acc};
  if (defer_split) *defer_split = sa;
  if (decisions_only && !defer_split) HIP_TRY(mipgpu::launch_dec_split(sa, nframes, true, s));
  // the host pipeline's launches (on the engine's search streams) use their own rings
  auto &ring = s == e->stream ? e->hp_queue : s == e->stream4 ? e->hp_queue2 : e->queue;
  const int qbase = s == e->stream ? mip_engine::kQueueSlots : s == e->stream4 ? 2 * mip_engine::kQueueSlots : 0;
  const int slot = ring.acquire(s);
  if (slot < 0) return fail("ordering the search's item counter failed: %s", hipGetErrorString(hipGetLastError()));
  a.queue = e->d_queue + mipgpu::kQueueWords * (qbase + slot);
  // done (host pipeline): the chunk's completion event, recorded by the search kernel's own
  // dispatch when nothing follows it on s (saves a marker packet between two chunks'
  // searches); *done = nullptr tells the caller it was recorded
  const bool last = !(alt && e->nfixup[map]) && !engine_refs && !timing &&
                    (decisions_only ? defer_split != nullptr : !(d_best || d_best_cost)) && ext_done_enabled();
  hipEvent_t stop = done && last ? *done : nullptr;
  mipgpu::SearchLaunchInfo li{};
  const hipError_t le = four ? SLOW_CALL(mipgpu::launch_search_four(a, nframes, alt, resident, false, s, stop, &li))
                             : SLOW_CALL(mipgpu::launch_search(a, nframes, alt, resident, wp.wide, s, stop, &li));
  if (le == hipSuccess && stop) *done = nullptr;
  if (le == hipSuccess) {  // mip_search_census (every caller holds e->mu)
    const int w = li.waves == 12 ? 0 : li.waves == 16 ? 1 : 2;
    e->census[8 * w + 4 * li.alt + 2 * li.dec + li.pf]++;
    e->census[MIP_CENSUS_PAIR] += li.pair;
    e->census[MIP_CENSUS_CHUNKED] += li.chunked;
    e->census[MIP_CENSUS_ORDERED] += li.ordered;
  }
  if (le != hipSuccess) {
    ring.failed(slot);  // the pair is cleared before its next use
    return fail("search launch failed: %s", hipGetErrorString(le));
  }
  if (ring.launched(slot, s) != 0) return fail("hipEventRecord failed");
  if (alt && e->nfixup[map]) HIP_TRY(mipgpu::launch_fixup(a, e->d_fixup[map], e->nfixup[map], nframes, s));
  if (engine_refs_end(e, engine_refs, s) != 0) return -1;
  if (timing) {
    HIP_TRY(hipMemcpyAsync(clocks.data(), a.wave_clock, clocks.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    (void)hipFree(a.wave_clock);
    if (FILE *f = fopen(timing, "ab")) {
      fwrite(clocks.data(), 8, clocks.size(), f);
      fclose(f);
    }
  }
  if (decisions_only) {
    if (!defer_split) HIP_TRY(mipgpu::launch_dec_split(sa, nframes, false, s));
  } else if (d_best || d_best_cost) {
    mipgpu::BestArgs b{d_costs, d_best, d_best_cost, (int)total_cus, e->opts.best_k};
    HIP_TRY(mipgpu::launch_best_modes(b, s));
  }
  return 0;
}

extern "C" {

int mip_search_device(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes,
                      int32_t *d_costs, int32_t *d_sad, int32_t *d_satd, uint8_t *d_best_mode,
                      int32_t *d_best_cost, void *stream) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (check_device_status(e) != 0) return -1;
  HIP_TRY(hipSetDevice(e->device));
  if (flush_open(e) != 0) return -1;  // (device-API work orders itself after the host calls)
  return search_device_impl(e, d_frames, d_refs, nframes, d_costs, d_sad, d_satd, d_best_mode, d_best_cost,
                            (hipStream_t)stream, d_refs != nullptr && d_refs != d_frames, device_status(e));
}

int mip_check_input(mip_engine *e, void *stream) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return check_device_status(e);
}

int mip_search_device_range(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes,
                            int ctu_begin, int ctu_end, int32_t *d_costs, int32_t *d_sad, int32_t *d_satd,
                            void *stream) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (!d_costs) return fail("d_costs is NULL");
  // an empty range (more CTU-row bands than CTU rows, mipgpu.split) is a successful no-op
  if (ctu_begin == ctu_end && ctu_begin >= 0 && ctu_end <= e->nctus) return 0;
  if (check_device_status(e) != 0) return -1;
  HIP_TRY(hipSetDevice(e->device));
  if (flush_open(e) != 0) return -1;
  return search_device_impl(e, d_frames, d_refs, nframes, d_costs, d_sad, d_satd, nullptr, nullptr,
                            (hipStream_t)stream, d_refs != nullptr && d_refs != d_frames, device_status(e), ctu_begin,
                            ctu_end - ctu_begin);
}

int mip_device_cache(int device, int release, uint64_t *idle_bytes, uint64_t *reused_blocks) {
  BlockCache &c = block_cache();
  std::lock_guard<std::mutex> lk(c.mu);
  uint64_t idle = 0;
  for (auto it = c.idle.begin(); it != c.idle.end();) {
    if (it->first.first == device && release) {
      int cur = 0;
      (void)hipGetDevice(&cur);
      (void)hipSetDevice(device);
      (void)hipFree(it->second);
      (void)hipSetDevice(cur);
      it = c.idle.erase(it);
      continue;
    }
    if (it->first.first == device) idle += it->first.second;
    ++it;
  }
  if (idle_bytes) *idle_bytes = idle;
  if (reused_blocks) *reused_blocks = c.reused;
  return 0;
}

int mip_search_census(mip_engine *e, uint64_t *out, int n) {
  if (!e || !out || n < 0 || n > MIP_CENSUS_ENTRIES) return fail("bad arguments");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  for (int i = 0; i < n; i++) out[i] = e->census[i];
  return 0;
}

int mip_host_alloc(size_t bytes, void **out) {
  if (!out) return fail("out is NULL");
  *out = nullptr;
  HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
  return 0;
}

int mip_host_alloc_near(int device, size_t bytes, void **out) {
  if (!out) return fail("out is NULL");
  *out = nullptr;
  const mipgpu::NumaPlace p = device_place(device);
  const mipgpu::ScopedNodePolicy pol(p);
  HIP_TRY(hipHostMalloc(out, bytes ? bytes : 1, pol.applied() ? hipHostMallocNumaUser : hipHostMallocDefault));
  return 0;
}

int mip_numa_node_of_pci(const char *pci_bus_id) {
  if (!pci_bus_id) return fail("pci_bus_id is NULL");
  return mipgpu::numa_place_of_pci(pci_bus_id).node;
}

int mip_numa_node(int device) { return device_place(device).node; }

int mip_bind_thread(int device) { return mipgpu::bind_current_thread(device_place(device)) ? 1 : 0; }

int mip_host_free(void *p) {
  if (p) HIP_TRY(hipHostFree(p));
  return 0;
}

int mip_filter_frames(mip_engine *e, const uint16_t *frames, int nframes, int filter, int kernel_idx,
                      uint16_t *out) {
  if (!e || !frames || !out || nframes < 1) return fail("bad filter arguments");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  if (quiesce(e) != 0) return -1;  // (host searches in flight use d_frames / d_refs)
  const size_t fs = (size_t)e->width * e->height;
  if (!e->d_refs) HIP_TRY(dev_malloc(e->device, (void **)&e->d_refs, fs * e->hp_frames * 2));
  const int chunk = mipgpu::stage_chunk_frames(e->opts.max_batch, nframes, 0);
  auto filter_chunk = [&](int nb, const uint16_t *) {
    return mip_filter_device(e->d_frames, e->d_refs, e->width, e->height, nb, filter, kernel_idx, e->stream);
  };
  if (walk_chunks(e, frames, nullptr, nframes, chunk, {{out, e->d_refs, fs * 2}}, filter_chunk) != 0) return -1;
  HIP_TRY(hipStreamSynchronize(e->stream2));
  return 0;
}

double mip_time_search_device(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes,
                              int32_t *d_costs, int reps) {
  if (!e || reps < 1) return fail("bad timing arguments");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (hipSetDevice(e->device) != hipSuccess) return fail("hipSetDevice");
  if (flush_open(e) != 0) return -1;
  hipEvent_t t0, t1;
  if (hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess) return fail("hipEventCreate");
  (void)hipEventRecord(t0, e->stream);
  for (int r = 0; r < reps; r++)
    if (search_device_impl(e, d_frames, d_refs, nframes, d_costs, nullptr, nullptr, nullptr, nullptr, e->stream,
                           d_refs != nullptr && d_refs != d_frames, device_status(e)) != 0) {
      (void)hipEventDestroy(t0);
      (void)hipEventDestroy(t1);
      return -1;
    }
  (void)hipEventRecord(t1, e->stream);
  (void)hipEventSynchronize(t1);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, t0, t1);
  (void)hipEventDestroy(t0);
  (void)hipEventDestroy(t1);
  if (check_device_status(e) != 0) return -1;
  return ms / reps;
}

}  // extern "C"

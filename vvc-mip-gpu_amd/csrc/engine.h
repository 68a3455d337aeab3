// engine.h -- private to the library: the engine's state and what its three translation units
// share (mipgpu.cpp: create / destroy, block cache, the search's device API, the filter;
// host_pipeline.cpp: the host API's pipeline; host_stages.cpp: prediction, partition and intra
// costs, device entry points and chunked host wrappers).
#pragma once
#include "mipgpu.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <initializer_list>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "mip_kernels.h"
#include "host_policy.h"
#include "host_stage_hip.h"
#include "numa_place.h"
#include "queue_ring.h"
#include "work_plan.h"

#pragma GCC visibility push(hidden)  // (none of this is part of the C ABI)

// mip_last_error's text (per thread) and the way every failure sets it: returns -1.
extern thread_local std::string g_err;
int fail(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

// MIPGPU_SLOW_CALLS=MS (diagnostic): every HIP call made through HIP_TRY / SLOW_CALL that
// blocks the calling thread longer than MS milliseconds is reported on stderr.
inline double slow_call_ms() {
  static const double v = getenv("MIPGPU_SLOW_CALLS") ? atof(getenv("MIPGPU_SLOW_CALLS")) : 0.0;
  return v;
}
struct SlowCall {
  const char *what;
  std::chrono::steady_clock::time_point t0;
  explicit SlowCall(const char *w) : what(w) {
    if (slow_call_ms() > 0) t0 = std::chrono::steady_clock::now();
  }
  ~SlowCall() {
    if (slow_call_ms() <= 0) return;
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ms > slow_call_ms()) fprintf(stderr, "mipgpu slow call: %.3f ms %s\n", ms, what);
  }
};
#define SLOW_CALL(expr) ([&] { SlowCall _sc(#expr); return (expr); }())

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t _e = SLOW_CALL(expr);                                               \
    if (_e != hipSuccess) return fail("%s: %s", #expr, hipGetErrorString(_e));     \
  } while (0)

struct mip_engine {
  int device = 0, width = 0, height = 0, nctus = 0, ctu_cols = 0;
  // NUMA placement of the engine's host side (numa_place.h): its GPU's node, whose memory
  // holds the engine's page-locked buffers and whose CPUs run its host threads.
  mipgpu::NumaPlace place;
  mip_opts opts{};
  // Host API pipeline (mip_search_frames): `stream` and `stream4` compute (chunks alternate
  // between them, so that one chunk's search takes the CUs its predecessor's drains), `stream2`
  // uploads, `stream3` downloads; per buffer slot, events order upload -> compute -> download
  // and a slot's reuse after its previous chunk (see mip_search_frames).
  hipStream_t stream = nullptr, stream2 = nullptr, stream3 = nullptr, stream4 = nullptr;
  // Buffer slots of the host pipeline: hp_slots regions of hp_cap frames each in the engine
  // buffers (d_frames, d_refs, d_costs, ...).  Large engines (max_batch >= 16): 4 slots of a
  // quarter of max_batch; small ones: 3 slots of max_batch frames (triple buffering, so that a
  // caller searching one frame per call -- the reference's per-frame loop with BUFFER_SLOTS 2,
  // main.cpp:886-898, main_aux_functions.h:5, 617 -- overlaps frame k+1's upload and frame
  // k-1's download with frame k's search).
  static constexpr int kHostSlots = 4;
  int hp_slots = 0, hp_cap = 0, hp_frames = 0;  // hp_frames: frames of the engine buffers
  // Decisions-only chunks: the packed running argmins of the CUs whose mode pairs are cut
  // over several tasks ([hp_frames][nCTUs][5380]); all ones outside the chunks in flight
  // (the unpacking kernel resets the entries it reads), so no initialising kernel runs.
  uint32_t *d_split_acc = nullptr;
  hipEvent_t slot_up[kHostSlots] = {}, slot_comp[kHostSlots] = {}, slot_down[kHostSlots] = {};
  // Chunks run through the slots in one global sequence across host-API calls, so that
  // asynchronous calls (mip_search_frames_async) keep the pipeline full; call k completes
  // at call_done[(k - 1) % kCallRing] (tickets are 1-based call numbers).
  uint64_t host_chunks = 0, host_calls = 0;
  static constexpr int kCallRing = 64;
  hipEvent_t call_done[kCallRing] = {};
  // A host-API call was made: device-API searches that filter into the engine's reference
  // scratch wait for the last call's completion, call_done[(host_calls - 1) % kCallRing]
  // (the host pipeline uses the same buffer; no extra event on the search stream).
  bool host_pending = false;
  // mip_trace_times: per-slot timing events around the chunk's upload and filter launch,
  // the chunk (sequence number, frames) whose events are pending, and the per-frame times
  // read so far.
  bool trace = false;
  hipEvent_t tr_ev[kHostSlots][4] = {};  // upload start / end, filter start / end
  uint64_t tr_chunk[kHostSlots] = {};
  int tr_frames[kHostSlots] = {}, tr_filter[kHostSlots] = {};
  std::vector<std::pair<double, double>> tr_times;
  // Page-locked bounce ring for pageable caller buffers of the host pipeline (host_stage.h).
  mipgpu::HostStage stage;
  uint16_t *d_frames = nullptr, *d_refs = nullptr;
  int32_t *d_costs = nullptr, *d_sad = nullptr, *d_satd = nullptr, *d_best_cost = nullptr;
  uint8_t *d_best = nullptr;
  // Work lists, one set per slice count (workgroups per CTU quadrant): small batches need
  // more, smaller workgroups to fill the chip (see pick_work).
  // `plan` (work_plan.h) is the host's copy of everything planned; work[i] holds the device
  // copies of plan.work[i]'s lists.
  mipgpu::EnginePlan plan;
  struct Work {
    const mipgpu::WorkPlan *host = nullptr;  // slices, wide, max_split, order_cost, nonempty
    mipgpu::WaveTask *d_tasks = nullptr;
    mipgpu::Job *d_jobs = nullptr;
    int *d_lists = nullptr;
    uint32_t *d_fill = nullptr;
    int *d_fill_begin = nullptr;
    uint16_t *d_dfill = nullptr, *d_split = nullptr;  // decisions only (WorkPlan)
    int *d_dfill_begin = nullptr, *d_split_begin = nullptr;
    uint32_t *d_order = nullptr;  // small launches: the frame's items longest first
  };
  std::vector<Work> work;
  // pick_work's choice per frame count for small launches (index into `work`), [alt][wide]
  // (the two reference modes have their own resident grids)
  std::vector<int> small_choice[2][2];
  uint8_t *d_tables = nullptr;
  uint8_t *d_ctu_var[mipgpu::kMaps] = {};           // [map][nctus] CTU variant (ctu_variants: orig /
                                            // caller refs / engine-filtered refs)
  mipgpu::FixupCu *d_fixup[mipgpu::kMaps] = {};     // alt refs: CUs of the exact per-CU kernel, per map
  int nfixup[mipgpu::kMaps] = {};
  // Prediction output (mip_predict_device), uploaded at its first use: the CUs that are not
  // predicted, [0] with caller-supplied or original references (the MIP_FILTER_NONE set of
  // mip_unavailable_cus), [1] with the engine filter's references (== [0] without a filter);
  // and the CU geometry inside a CTU (PredictArgs::geo).
  uint8_t *d_pred_unavail[2] = {};
  uint32_t *d_pred_geo = nullptr;
  // Partition decision of host frames (mip_partition_frames), allocated at its first use, for
  // max_batch frames: the leaf flags, and the CTU costs followed by the CTU leaf counts.
  uint8_t *d_part_leaf = nullptr;
  int32_t *d_part_ctu = nullptr;
  // Planar / DC baseline costs (mip_intra_device), uploaded at its first use: the lane slots of
  // the 16 32x32 blocks of a CTU (intra_plan.h intra_build_slots).
  uint32_t *d_intra_slots = nullptr;
  int intra_slots_per_block = 0;
  // Extended angular reference lines (mip_angular_refs): the setting, read when a call builds its
  // launch, and -- uploaded at the first extended call -- the lengths of mip_extended_refs per CU
  // [nctus * 5380] as top | left << 8, [0] / [1] for the sets of d_pred_unavail [0] / [1].
  std::atomic<int> ang_refs{MIP_ANG_REFS_SUBSTITUTED};
  uint16_t *d_ang_ext[2] = {};
  // The angular interpolation filter (mip_angular_interp): the setting, read when a call builds its
  // launch, like ang_refs.
  std::atomic<int> ang_interp{MIP_ANG_INTERP_2TAP};
  int resident[2] = {0, 0};  // persistent search grid (workgroups resident on this device), [alt]
  int resident_wide[2] = {0, 0};  // the same for 16-wave workgroups
  int resident_four[2] = {0, 0};  // the four-wave twin's (8-wave workgroups; 0: not available)
  // Engine-owned reference scratch d_refs, written by the engine filter when a device-API
  // search has no caller references: every such search records refs_done on its stream, and
  // the next writer of d_refs (another device-API search, on any stream, or a host-API call)
  // waits for it first.
  hipEvent_t refs_done = nullptr;
  bool refs_pending = false;
  // Item-counter pairs of the persistent search kernel, used round robin; a pair is reused
  // only after the launch that last used it has completed (stream wait on its event), so
  // launches on different streams never share one.
  static constexpr int kQueueSlots = 16;
  uint32_t *d_queue = nullptr;
  hipEvent_t queue_done[kQueueSlots] = {};
  // Three rings: `queue` for device-API launches (any caller stream: reuse ordered by the
  // slot's event) and `hp_queue` / `hp_queue2` for the host pipeline, whose searches run on
  // the engine's own search streams `stream` / `stream4`, one ring each: launches on one
  // in-order stream never overlap, so such a ring needs neither the event record nor the
  // wait (two fewer queue packets per chunk on the search stream's critical path).  The pairs
  // are distinct memory (hp_queue: slots kQueueSlots..2 kQueueSlots-1 of d_queue, hp_queue2
  // the next kQueueSlots).
  struct QueueOps {
    mip_engine *e;
    int base;           // first counter pair of the ring in d_queue
    bool one_stream;    // every launch of the ring is on one stream: no events needed
    int wait(int slot, hipStream_t s) const {
      return one_stream ? 0 : hipStreamWaitEvent(s, e->queue_done[slot], 0) != hipSuccess;
    }
    int record(int slot, hipStream_t s) const {
      return one_stream ? 0 : hipEventRecord(e->queue_done[slot], s) != hipSuccess;
    }
    int clear(int slot, hipStream_t s) const {
      return hipMemsetAsync(e->d_queue + mipgpu::kQueueWords * (base + slot), 0, mipgpu::kQueueWords * sizeof(uint32_t),
                            s) != hipSuccess;
    }
    int sync(hipStream_t s) const { return hipStreamSynchronize(s) != hipSuccess; }
  };
  QueueRing<QueueOps, kQueueSlots> queue{QueueOps{this, 0, false}};
  QueueRing<QueueOps, kQueueSlots> hp_queue{QueueOps{this, kQueueSlots, true}};
  QueueRing<QueueOps, kQueueSlots> hp_queue2{QueueOps{this, 2 * kQueueSlots, true}};  // (stream4)
  // Input contract (10-bit samples): status words the search kernel sets when it stages a
  // sample above 1023 (SearchArgs::status), in page-locked host memory mapped into the
  // device.  One set of kStatusWords per host-API call (call c: set (c - 1) % kCallRing) and
  // one for the device API (set kCallRing), so that a violation is reported for the call
  // that searched the frame: mip_wait(c) reads call c's set (harvest_status), the device API
  // its own set (check_device_status).  status_harvested: calls <= it have had their set
  // read and cleared; call_errors: the flags of harvested calls not yet reported (ticket ->
  // 1 = frame samples, 2 = reference samples).
  uint32_t *h_status = nullptr, *d_status = nullptr;
  uint64_t status_harvested = 0;
  std::map<uint64_t, uint32_t> call_errors;  // (4: the call's merged launch failed)

  // Merged chunks (round 6).  A small host-API call (page-locked buffers, fewer frames than a
  // slot) that arrives while the pipeline is busy is not launched on its own: it opens -- or
  // joins -- the *open chunk*, whose frames are uploaded into one slot's region at the
  // calls' offsets as they arrive, and the chunk is searched by ONE launch of all its frames
  // (merge_call / flush_open).  One-frame launches run at 0.177 ms against 0.13 ms per frame
  // in 4-frame launches (profiles/r05_small_batch_final.jsonl), so per-frame callers (the
  // reference's loop, main.cpp:678-1241) queueing calls get the multi-frame rate.  The chunk
  // is launched when it is full (merge_cap frames or kMergeCalls calls), when a call that
  // cannot join it arrives, when the next call finds the search launched before it completed
  // (the GPU would idle), at any mip_wait / mip_flush / synchronous call, and before any
  // device-API work of the engine.  (A first version also had a flusher thread that waited
  // for that search with hipEventSynchronize: beside the caller's submissions it made 8 queued
  // calls erratic, 2600-3000 frames/s against 5430 without it, profiles/r06_merge_rates.txt --
  // so there is none.)  MIPGPU_MERGE=0 (A/B knob): off.
  mipgpu::OpenChunk open;  // (host_policy.h, with the rules as merge_decision)
  int last_slot = -1;  // slot of the last launched host-pipeline chunk (its slot_comp event)
  int last_frames = 0;  // frames of the last launched host-pipeline chunk (merge_cap)
  uint64_t stat_launches = 0, stat_merged_calls = 0, stat_merged_launches = 0;  // mip_host_stats
  uint64_t census[MIP_CENSUS_ENTRIES] = {};  // mip_search_census (search_device_impl)
  // per-frame status pointers of merged launches ([kCallRing][hp_cap], page-locked, mapped;
  // row (first call - 1) % kCallRing), SearchArgs::frame_status
  uint32_t **h_frame_status = nullptr, **d_frame_status = nullptr;
  // Every public entry point that uses the engine holds `mu`: an engine is used by one thread
  // at a time (include/mipgpu.h); calls from several threads are serialised, not undefined.
  std::recursive_mutex mu;
};

// CU count limit of one launch (int32 indices in the decision-list kernel).
constexpr long long kMaxCus = (1LL << 31) - 256;

// ---- mipgpu.cpp ----
// hipMalloc / hipFree through the device block cache.
hipError_t dev_malloc(int device, void **p, size_t bytes);
void dev_free(void *p);
// The device blocks of one call: taken from dev_malloc, given back when the call returns,
// whichever way.  (Blocks that outlive the call -- the engine's buffers and tables -- are not
// taken through it.)
struct DevScratch {
  const int device;
  std::vector<void *> blocks;
  explicit DevScratch(int d) : device(d) {}
  DevScratch(const DevScratch &) = delete;
  ~DevScratch() {
    for (void *p : blocks) dev_free(p);
  }
  template <class T>
  hipError_t take(T *&p, size_t bytes) {  // p is set only on success
    void *b = nullptr;
    const hipError_t err = dev_malloc(device, &b, bytes);
    if (err == hipSuccess) blocks.push_back(p = static_cast<T *>(b));
    return err;
  }
};
// Engine-filtered references of a device-API stage: before its kernels (*refs: what they read;
// *engine_refs: the engine's reference scratch, filtered from d_frames on s) and after them.
int engine_refs_begin(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes, hipStream_t s,
                      const uint16_t **refs, bool *engine_refs);
int engine_refs_end(mip_engine *e, bool engine_refs, hipStream_t s);
// caller_refs: d_refs holds caller-supplied reference frames (checked against the 10-bit
// contract like the frames; engine-filtered references are not: the separable filters'
// defined > 10-bit outputs at the last columns go to the fixup kernel).
int search_device_impl(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes, int32_t *d_costs,
                       int32_t *d_sad, int32_t *d_satd, uint8_t *d_best, int32_t *d_best_cost, hipStream_t s,
                       bool caller_refs, uint32_t *d_status, int ctu0 = 0, int nrange = -1, uint32_t *split_acc = nullptr,
                       mipgpu::SplitArgs *defer_split = nullptr, hipEvent_t *done = nullptr,
                       uint32_t *const *frame_status = nullptr, bool alternating = false);
// Status sets (mip_engine::h_status).  take_status: read and clear a set: 0, or 1 (frame
// samples) | 2 (reference samples); contract_error: fail() with the violation's text;
// check_device_status: the device API's set; device_status: its device pointer.
uint32_t take_status(mip_engine *e, int set);
int contract_error(uint32_t flags, const char *what);
int check_device_status(mip_engine *e);
uint32_t *device_status(mip_engine *e);

// ---- host_stages.cpp ----
// A host call's frames through the engine buffers, `chunk` frames (host_policy.h
// stage_chunk_frames) at a time on e->stream: the chunk's frames are uploaded into e->d_frames --
// and its caller references, if any, into a device buffer handed to the body -- then
// body(frames of the chunk, d_refs or null) launches the device stage, the outputs asked for
// are downloaded and the stream is synchronised.  Clears refs_pending: nothing reads d_refs
// after the last synchronise.
struct ChunkOut {
  void *host;       // the call's output buffer for all its frames; null: not asked for
  const void *dev;  // the device buffer the body fills for a chunk
  size_t bytes;     // per frame
};
int walk_chunks(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes, int chunk,
                std::initializer_list<ChunkOut> outs, const std::function<int(int, const uint16_t *)> &body);

// ---- host_pipeline.cpp ----
// Launch the engine's open (merged) chunk, if any.
int flush_open(mip_engine *e);
// Order the engine streams after the device-API searches still reading d_refs.
int wait_refs_readers(mip_engine *e);
// Before engine buffers are used outside the pipeline: launch the open chunk and wait until
// every host search in flight (and every reader of d_refs) is over.
int quiesce(mip_engine *e);

#pragma GCC visibility pop

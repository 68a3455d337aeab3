// host_pipeline.cpp -- the host API (mip_search_frames[_async], mip_wait, mip_flush): chunks of
// host frames through the engine's buffer slots on four streams, merged chunks of small calls,
// per-call status and completion, upload / filter tracing.  What it decides -- merge or not,
// chunk sizes -- is host_policy.h's arithmetic; this file makes the HIP calls.
#include "engine.h"

#include <algorithm>
#include <cstring>

namespace {

using namespace mipgpu;  // host_policy.h: HostOutputs, kSig*, Member, OpenChunk, ...

// ---- The host pipeline's knobs, read at every call (tests set them per test) ----
// MIPGPU_MERGE (A/B / test knob): 0 = every call launches on its own; "hold" = small calls
// open a chunk even into an idle pipeline and only a full chunk, an incompatible call, a wait
// or a device-API call launch it (deterministic merges for tests).
int merge_mode() {
  const char *e = getenv("MIPGPU_MERGE");
  if (e && *e == '0') return kMergeOff;
  return e && !strcmp(e, "hold") ? kMergeHold : kMergeOn;
}
// MIPGPU_GATHER_DOWN=0 (A/B knob): merged decisions-only chunks download member by member.
bool gather_down() {
  const char *e = getenv("MIPGPU_GATHER_DOWN");
  return !(e && *e == '0');
}
// MIPGPU_DEC_INLINE=1 (A/B knob): decisions-only chunks of the host pipeline initialise and
// unpack their split entries on the search stream (before round 5) instead of the download
// stream.
bool dec_inline() {
  const char *e = getenv("MIPGPU_DEC_INLINE");
  return e && *e == '1';
}
// Host pipeline search streams: 2 (chunks alternate between `stream` and `stream4`) or 1
// (MIPGPU_SEARCH_STREAMS=1, A/B knob: every search on `stream`).
int search_streams() {
  const char *e = getenv("MIPGPU_SEARCH_STREAMS");
  return e && *e == '1' ? 1 : 2;
}
// MIPGPU_MAX_INFLIGHT=D (A/B knob): a call waits on the host until the call D before it has
// completed (bounds the commands queued in the HIP runtime); 0: no bound.
int max_inflight() {
  const char *e = getenv("MIPGPU_MAX_INFLIGHT");
  return e ? atoi(e) : 0;
}
// MIPGPU_CHUNK_MB (tuning knob): download bytes per chunk of full tables (host_policy.h
// chunk_frames; 0: its default).
int chunk_mb() {
  const char *e = getenv("MIPGPU_CHUNK_MB");
  return e ? atoi(e) : 0;
}
// MIPGPU_RAMP=0 (A/B knob): no ramps; MIPGPU_RAMP=up: no ramp-down (host_policy.h call_chunks).
int ramp_mode() {
  const char *e = getenv("MIPGPU_RAMP");
  return e && !strcmp(e, "0") ? kRampOff : e && !strcmp(e, "up") ? kRampUp : kRampBoth;
}

// Device pointer of the status set a host-API call's searches mark (mip_engine::h_status).
uint32_t *call_status(mip_engine *e, uint64_t call) {
  return e->d_status + (size_t)((call - 1) % mip_engine::kCallRing) * kStatusWords;
}

// Host API: move the status sets of the completed calls (status_harvested, upto] into
// call_errors (only calls that saw a violation are kept, until mip_wait reports them: an
// entry is never dropped, so a call that searched samples above 1023 can never be waited for
// as a success; memory is bounded by the failed calls nobody waits for -- the Python
// binding's tickets wait when dropped).  Every call <= upto must have completed.
void harvest_status(mip_engine *e, uint64_t upto) {
  for (uint64_t c = e->status_harvested + 1; c <= upto; c++) {
    const uint32_t f = take_status(e, (int)((c - 1) % mip_engine::kCallRing));
    if (f) e->call_errors[c] = f;
  }
  if (upto > e->status_harvested) e->status_harvested = upto;
}

// mip_trace_times: read the pending chunk times of slot `sl` (waits for its events).
int drain_trace(mip_engine *e, int sl) {
  if (!e->tr_frames[sl]) return 0;
  float up = 0, fl = 0;
  HIP_TRY(hipEventSynchronize(e->tr_ev[sl][1]));
  HIP_TRY(hipEventElapsedTime(&up, e->tr_ev[sl][0], e->tr_ev[sl][1]));
  if (e->tr_filter[sl]) {
    HIP_TRY(hipEventSynchronize(e->tr_ev[sl][3]));
    HIP_TRY(hipEventElapsedTime(&fl, e->tr_ev[sl][2], e->tr_ev[sl][3]));
  }
  const int n = e->tr_frames[sl];
  for (int i = 0; i < n; i++) e->tr_times.push_back({(double)up / n, (double)fl / n});
  e->tr_frames[sl] = 0;
  return 0;
}

// After a failure part-way through a chunk: wait for what was queued, and restore the split
// accumulator -- a decisions-only chunk may have been searched without its unpacking, which
// resets its split_acc entries -- to all ones (the streams are idle then).  The failure's
// text stays the last error.
void recover_after_failure(mip_engine *e) {
  const std::string err = g_err;
  for (hipStream_t st : {e->stream2, e->stream, e->stream4, e->stream3}) (void)hipStreamSynchronize(st);
  (void)hipMemset(e->d_split_acc, 0xff, (size_t)e->hp_frames * e->nctus * MIP_CUS_PER_CTU * 4);
  g_err = err;
}

// Sizes per frame of the engine's buffers, in elements: samples, cost-table entries, decision
// entries.
struct FrameSizes {
  size_t fs, cpf, upf;
  explicit FrameSizes(const mip_engine *e)
      : fs((size_t)e->width * e->height), cpf((size_t)e->nctus * MIP_COSTS_PER_CTU),
        upf((size_t)e->nctus * MIP_CUS_PER_CTU * e->opts.best_k) {}
};

// The engine buffers a host-API call needs before its first upload, and the order of the
// engine streams after the device-API searches that read d_refs.
int begin_uploads(mip_engine *e, bool refs) {
  if ((refs || e->opts.filter != MIP_FILTER_NONE) && !e->d_refs)
    HIP_TRY(dev_malloc(e->device, (void **)&e->d_refs, FrameSizes(e).fs * e->hp_frames * 2));
  if (wait_refs_readers(e) != 0) return -1;
  e->refs_pending = false;  // the waits above order every later use of the engine streams
  return 0;
}

// Chunk k, whose nb frames (and caller references, sig & kSigRefs) are queued on the upload
// stream into slot k % hp_slots: everything from there to the start of its downloads.  The
// engine filter (engine references) runs on the upload stream behind the upload: it overlaps
// the previous chunk's search (its workgroups take CUs as the persistent search grid drains),
// and the slot's refs region is free once the slot's previous search is.  The search waits
// for the upload stream (one cross-stream wait on the search stream per chunk) and runs on
// `stream`, or -- alternating, odd chunks -- on `stream4`; the download stream waits for it
// (also without outputs: slot_down ends the chunk).  Decisions only: the split CUs' packed
// running minima live in d_split_acc, which holds all ones outside the chunks in flight (the
// unpacking resets what it reads), so the search stream runs the search kernel alone and the
// unpacking runs on the download stream before the downloads -- the initialising and
// unpacking kernels and their launch gaps leave the search stream's critical path (one-frame
// calls: ~20 us of ~190 us).  status: the call's status set; frame_status (merged chunks):
// each frame's own call's.  *d: the slot's device outputs; the caller queues their downloads
// and records slot_down.
int launch_chunk(mip_engine *e, uint64_t k, int nb, unsigned sig, uint32_t *status, uint32_t *const *frame_status,
                 bool alternating, bool trace, HostOutputs *d) {
  const int sl = (int)(k % e->hp_slots);
  const FrameSizes z(e);
  const size_t fo = (size_t)sl * e->hp_cap;  // first engine frame of this chunk's slot
  const hipStream_t up = e->stream2, down = e->stream3, comp = alternating && (k & 1) ? e->stream4 : e->stream;
  const bool dec = (sig & kSigDec) != 0;
  uint16_t *d_frames = e->d_frames + fo * z.fs;
  const uint16_t *d_refs = (sig & kSigRefs) ? e->d_refs + fo * z.fs : nullptr;
  const bool filt = !(sig & kSigRefs) && e->opts.filter != MIP_FILTER_NONE;
  if (filt) {
    if (trace) HIP_TRY(hipEventRecord(e->tr_ev[sl][2], up));
    if (mip_filter_device(d_frames, e->d_refs + fo * z.fs, e->width, e->height, nb, e->opts.filter, e->opts.kernel_idx,
                          up) != 0)
      return -1;
    if (trace) HIP_TRY(hipEventRecord(e->tr_ev[sl][3], up));
    d_refs = e->d_refs + fo * z.fs;
  }
  HIP_TRY(hipEventRecord(e->slot_up[sl], up));
  HIP_TRY(hipStreamWaitEvent(comp, e->slot_up[sl], 0));
  if (trace) {
    e->tr_frames[sl] = nb;
    e->tr_filter[sl] = filt;
    e->tr_chunk[sl] = k;
  }
  d->costs = dec ? nullptr : e->d_costs + fo * z.cpf;
  d->sad = (sig & kSigSad) ? e->d_sad + fo * z.cpf : nullptr;
  d->satd = (sig & kSigSatd) ? e->d_satd + fo * z.cpf : nullptr;
  d->best_mode = (sig & kSigBestMode) ? e->d_best + fo * z.upf : nullptr;
  d->best_cost = (sig & kSigBestCost) || dec ? e->d_best_cost + fo * z.upf : nullptr;
  SplitArgs split{};
  const bool defer = dec && !dec_inline();
  hipEvent_t comp_done = e->slot_comp[sl];  // (nullptr after the call: the search recorded it)
  if (search_device_impl(e, d_frames, d_refs, nb, d->costs, d->sad, d->satd, d->best_mode, d->best_cost, comp,
                         (sig & kSigRefs) != 0, status, 0, -1,
                         defer ? e->d_split_acc + fo * e->nctus * MIP_CUS_PER_CTU : nullptr, defer ? &split : nullptr,
                         &comp_done, frame_status, alternating) != 0)
    return -1;
  if (comp_done) HIP_TRY(hipEventRecord(e->slot_comp[sl], comp));
  e->last_slot = sl;
  e->last_frames = nb;
  e->stat_launches++;
  HIP_TRY(hipStreamWaitEvent(down, e->slot_comp[sl], 0));
  if (defer) HIP_TRY(launch_dec_split(split, nb, false, down));
  return 0;
}

// The downloads of a merged chunk's members from the slot's outputs `d`.
int download_members(mip_engine *e, const OpenChunk &o, const HostOutputs &d) {
  const FrameSizes z(e);
  const size_t cpf = z.cpf, upf = z.upf;
  const hipStream_t down = e->stream3;
  // Decisions-only members' downloads as one copy kernel writing straight into their
  // device-mapped page-locked buffers: one dispatch per chunk instead of two copies per
  // member.  Fewer queued commands, fewer of the runtime's host stalls (section 6 of
  // DESIGN.md): 32 queued one-frame calls' rounds 6397-6419 frames/s at the 25th percentile
  // instead of 4033-6187 (medians 6451-6477 vs 6423-6628; tools/experiments/r06/gather.sh).
  if ((o.sig & kSigDec) && gather_down() && 2 * o.members.size() <= (size_t)kMaxCopyPieces) {
    CopyPieces cp{};
    bool gathered = true;
    for (const Member &m : o.members) {
      const size_t f = (size_t)m.f0, n = (size_t)m.n;
      auto add = [&](void *host, const void *dev, size_t bytes) {
        void *dp = nullptr;
        if (!host) return;
        if (hipHostGetDevicePointer(&dp, host, 0) != hipSuccess || !dp) {
          (void)hipGetLastError();
          gathered = false;
          return;
        }
        cp.p[cp.n++] = CopyPiece{static_cast<const uint8_t *>(dev), static_cast<uint8_t *>(dp), bytes};
      };
      add(m.out.best_mode, d.best_mode + f * upf, n * upf);
      add(m.out.best_cost, d.best_cost + f * upf, n * upf * 4);
    }
    if (gathered) {
      HIP_TRY(launch_gather_copy(cp, down));
      return 0;
    }
  }
  for (const Member &m : o.members) {
    const size_t f = (size_t)m.f0, n = (size_t)m.n;
    const HostOutputs &h = m.out;
    if (h.costs) HIP_TRY(hipMemcpyAsync(h.costs, d.costs + f * cpf, n * cpf * 4, hipMemcpyDeviceToHost, down));
    if (h.sad) HIP_TRY(hipMemcpyAsync(h.sad, d.sad + f * cpf, n * cpf * 4, hipMemcpyDeviceToHost, down));
    if (h.satd) HIP_TRY(hipMemcpyAsync(h.satd, d.satd + f * cpf, n * cpf * 4, hipMemcpyDeviceToHost, down));
    if (h.best_mode) HIP_TRY(hipMemcpyAsync(h.best_mode, d.best_mode + f * upf, n * upf, hipMemcpyDeviceToHost, down));
    if (h.best_cost)
      HIP_TRY(hipMemcpyAsync(h.best_cost, d.best_cost + f * upf, n * upf * 4, hipMemcpyDeviceToHost, down));
  }
  return 0;
}

// Add a call to the open chunk (opening one, of at most `cap` frames, if there is none): its
// frames (and caller references) are uploaded into the chunk's slot region at the chunk's
// next frame.
int merge_call(mip_engine *e, const uint16_t *frames, const uint16_t *refs, int nframes, const HostOutputs &out,
               unsigned sig, int cap, uint64_t call) {
  OpenChunk &o = e->open;
  const size_t fs = FrameSizes(e).fs;
  const hipStream_t up = e->stream2;
  if (!o.active) {
    if (begin_uploads(e, refs != nullptr) != 0) return -1;
    o.k = e->host_chunks++;
    const int sl = (int)(o.k % e->hp_slots);
    o.active = true;
    o.nb = 0;
    o.cap = cap;
    o.sig = sig;
    o.members.clear();
    // the slot's previous chunk is over once its downloads are (as search_frames_chunks)
    if (o.k >= (uint64_t)e->hp_slots) HIP_TRY(hipStreamWaitEvent(up, e->slot_down[sl], 0));
  }
  const size_t f = (size_t)(o.k % e->hp_slots) * e->hp_cap + o.nb;
  HIP_TRY(hipMemcpyAsync(e->d_frames + f * fs, frames, nframes * fs * 2, hipMemcpyHostToDevice, up));
  if (refs) HIP_TRY(hipMemcpyAsync(e->d_refs + f * fs, refs, nframes * fs * 2, hipMemcpyHostToDevice, up));
  o.members.push_back(Member{call, o.nb, nframes, out});
  o.nb += nframes;
  return 0;
}

// A call that is not merged: chunks of its frames rotate over the engine's hp_slots buffer
// slots (mip_engine::hp_slots: 4 slots of a quarter of max_batch, or 3 slots of max_batch for
// engines below 16 frames) through a three-stream pipeline: stream2 uploads chunk k+1 while
// `stream` searches chunk k and stream3 downloads chunk k-1, so the copy engines (H2D and
// D2H) and the compute run concurrently and the search kernels keep the whole GPU.  Per slot:
// the upload waits until the previous chunk of the slot has been searched (its frames / refs
// are free), the search waits for the upload and for the previous download of the slot's
// outputs, the download waits for the search.  The chunk sequence (and so the slot rotation
// and these waits) continues across calls, so asynchronous calls queue behind each other
// without draining the pipeline -- with three slots even one-frame calls overlap (the
// reference's BUFFER_SLOTS 2 loop: frame curr+1's upload during frame curr's kernels,
// main.cpp:886-898, and a non-blocking read-back of slot curr % 2, main_aux_functions.h:617).
// A slot is a fixed region of hp_cap frames of the engine buffers (chunk sizes differ between
// calls -- outputs requested, call length -- but a slot's region never moves, so the per-slot
// events order every reuse of it).  Transfers run at DMA rate from page-locked host memory
// (mip_host_alloc); `pageable` buffers go through the engine's page-locked bounce ring
// (host_stage.h), their downloads finished by mip_wait.
int search_frames_chunks(mip_engine *e, const uint16_t *frames, const uint16_t *refs, int nframes, const HostOutputs &out,
                         unsigned sig, unsigned pageable, uint64_t call, bool sync) {
  if (begin_uploads(e, refs != nullptr) != 0) return -1;
  const FrameSizes z(e);
  const size_t fs = z.fs, cpf = z.cpf, upf = z.upf;
  const FrameBytes fb{fs * 2, cpf * 4, upf};
  const int nslots = e->hp_slots, slot_cap = e->hp_cap;
  const bool idle = e->host_calls == 0 ||
                    SLOW_CALL(hipEventQuery(e->call_done[(e->host_calls - 1) % mip_engine::kCallRing])) == hipSuccess;
  const ChunkCall cc{nframes, sig, pageable, idle, sync};
  if (pageable) HIP_TRY(e->stage.reserve(ring_piece_bytes(sig, slot_cap, fb)));
  const int sb = chunk_frames(cc, slot_cap, nslots, fb, chunk_mb(), e->stage.piece(),
                              [&](size_t bytes) { return e->stage.footprint(bytes); });
  int nhead = 0, ntail = 0;
  const std::vector<int> plan = call_chunks(cc, sb, nslots, fb, ramp_mode(), &nhead, &ntail);
  // Searches of consecutive chunks alternate between two search streams, so that a chunk's
  // search takes the CUs as its predecessor's persistent grid drains -- except in ramped
  // calls, whose short chunks are sized to run one after the other (device API, 1080p,
  // tools/overlap_probe.py: one-frame launches +10 % decisions-only / +5 % full tables on
  // two streams; host pipeline: 8 queued one-frame calls decisions-only +5 %, 4-frame +4 %,
  // one synchronous ramped 128-frame call -2 %, so ramped calls keep one stream).
  const bool alt_streams = search_streams() == 2 && nhead + ntail == 0;
  for (const int nb : plan)  // (chunk_plan never exceeds sb <= slot_cap: a slot's region)
    if (nb < 1 || nb > slot_cap) return fail("internal: a chunk of %d frames for a slot of %d", nb, slot_cap);
  const hipStream_t up = e->stream2, down = e->stream3;
  // host <-> device copy: DMA from / to page-locked memory, else the bounce ring
  auto to_dev = [&](void *d, const void *h, size_t n) {
    return pageable & kPageIn ? e->stage.upload(d, h, n, up, call) : hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, up);
  };
  auto to_host = [&](void *h, const void *d, size_t n, unsigned buffer) {
    return pageable & buffer ? e->stage.download(h, d, n, down, call) : hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, down);
  };
  int f0 = 0;
  for (const int nb : plan) {
    const uint64_t k = e->host_chunks++;
    const int sl = (int)(k % nslots);
    const size_t fo = (size_t)sl * slot_cap;
    // the slot's previous chunk (k - nslots, of this or an earlier call) is over once its
    // downloads are (they wait for its search): then its frames / refs may be overwritten
    // here, and -- through this upload -- its outputs by this chunk's search
    if (k >= (uint64_t)nslots) HIP_TRY(hipStreamWaitEvent(up, e->slot_down[sl], 0));
    if (e->trace) {
      if (drain_trace(e, sl) != 0) return -1;
      HIP_TRY(hipEventRecord(e->tr_ev[sl][0], up));
    }
    HIP_TRY(to_dev(e->d_frames + fo * fs, frames + f0 * fs, nb * fs * 2));
    if (e->trace) HIP_TRY(hipEventRecord(e->tr_ev[sl][1], up));
    if (refs) HIP_TRY(to_dev(e->d_refs + fo * fs, refs + f0 * fs, nb * fs * 2));
    HostOutputs d;
    if (launch_chunk(e, k, nb, sig, call_status(e, call), nullptr, alt_streams, e->trace, &d) != 0) return -1;
    if (out.costs) HIP_TRY(to_host(out.costs + f0 * cpf, d.costs, nb * cpf * 4, kSigCost));
    if (out.sad) HIP_TRY(to_host(out.sad + f0 * cpf, d.sad, nb * cpf * 4, kSigSad));
    if (out.satd) HIP_TRY(to_host(out.satd + f0 * cpf, d.satd, nb * cpf * 4, kSigSatd));
    if (out.best_mode) HIP_TRY(to_host(out.best_mode + f0 * upf, d.best_mode, nb * upf, kSigBestMode));
    if (out.best_cost) HIP_TRY(to_host(out.best_cost + f0 * upf, d.best_cost, nb * upf * 4, kSigBestCost));
    HIP_TRY(hipEventRecord(e->slot_down[sl], down));
    f0 += nb;
  }
  return 0;
}

// One host-API call (mip_search_frames_async; mip_search_frames with sync = true: it waits for
// the call before returning, so no later call can queue behind its last chunks).
int search_frames_call(mip_engine *e, const uint16_t *frames, const uint16_t *refs, int nframes, const HostOutputs &out,
                       uint64_t *ticket, bool sync) {
  if (!e || !frames || nframes < 1 || !ticket) return fail("bad search arguments");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  *ticket = 0;
  if ((out.sad || out.satd) && !e->opts.want_sad_satd) return fail("engine created without want_sad_satd");
  HIP_TRY(hipSetDevice(e->device));
  const uint64_t next = e->host_calls + 1;
  // call `next` waits on the host until call `c` has completed (an open chunk that holds it
  // is launched first)
  auto wait_for = [&](uint64_t c) -> int {
    if (e->open.active && e->open.first_call() <= c && flush_open(e) != 0) return -1;
    HIP_TRY(hipEventSynchronize(e->call_done[(c - 1) % mip_engine::kCallRing]));
    return 0;
  };
  if (const int mi = max_inflight(); mi > 0 && next > (uint64_t)mi && wait_for(next - (uint64_t)mi) != 0) return -1;
  // call `next` marks status set (next - 1) % kCallRing: the call that used it before (more
  // than kCallRing calls in flight) must have completed and been harvested first
  if (next > (uint64_t)mip_engine::kCallRing && e->status_harvested < next - mip_engine::kCallRing) {
    if (wait_for(next - mip_engine::kCallRing) != 0) return -1;
    harvest_status(e, next - mip_engine::kCallRing);
  }
  // Merged chunks (mip_engine::open, host_policy.h merge_decision): a call with page-locked
  // buffers and fewer frames than a slot joins the open chunk (same outputs, room left), or
  // opens one while the pipeline is busy; anything else launches the open chunk first and
  // takes the chunked path.
  auto unpinned = [](const void *p, unsigned bit) { return p && !host_pinned(p) ? bit : 0u; };
  const unsigned pageable = (host_pinned(frames) && (!refs || host_pinned(refs)) ? 0u : kPageIn) |
                            unpinned(out.costs, kSigCost) | unpinned(out.sad, kSigSad) | unpinned(out.satd, kSigSatd) |
                            unpinned(out.best_mode, kSigBestMode) | unpinned(out.best_cost, kSigBestCost);
  const unsigned sig = call_sig(out, refs != nullptr, e->opts.best_k);
  const OpenChunk &o = e->open;
  const MergeState ms{o.active, o.sig, o.nb, o.cap, (int)o.members.size(), e->last_frames, e->last_slot >= 0,
                      e->host_calls > 0};
  const MergeCall mc{sig, nframes, !pageable && !e->trace && nframes < e->hp_cap, sync};
  const MergeDecision md = merge_decision(
      ms, mc, merge_mode(), e->hp_cap,
      [&] { return SLOW_CALL(hipEventQuery(e->slot_comp[e->last_slot])) == hipSuccess; },
      [&] { return SLOW_CALL(hipEventQuery(e->call_done[(e->host_calls - 1) % mip_engine::kCallRing])) == hipErrorNotReady; });
  if (md.flush_first && flush_open(e) != 0) return -1;
  if (md.take != Take::kChunks) {
    if (merge_call(e, frames, refs, nframes, out, sig, md.cap, next) != 0) return -1;
    *ticket = ++e->host_calls;
    e->host_pending = true;
    if (md.flush_after && flush_open(e) != 0) return -1;
    return 0;
  }
  const int rc = search_frames_chunks(e, frames, refs, nframes, out, sig, pageable, next, sync);
  // After a failure part-way through the chunks, the chunks already queued are waited for
  // here (no ticket covers them).
  if (rc != 0) {
    recover_after_failure(e);
    // staged downloads of the calls before this one complete normally; this call's are dropped
    (void)e->stage.drain(e->host_calls);
    e->stage.abandon();
    (void)take_status(e, (int)((next - 1) % mip_engine::kCallRing));  // the failed call's chunks: no ticket
    return rc;
  }
  // completion on the download stream (every chunk ends there, after its search and
  // downloads, outputs or not): calls complete in order
  const uint64_t call = ++e->host_calls;
  HIP_TRY(hipEventRecord(e->call_done[(call - 1) % mip_engine::kCallRing], e->stream3));
  e->host_pending = true;
  *ticket = call;
  return 0;
}

}  // namespace

// Host-API calls overwrite engine scratch: order them after the device-API searches still
// reading d_refs; once the call has synchronised the engine streams, those searches are
// complete too.
int wait_refs_readers(mip_engine *e) {
  if (!e->refs_pending) return 0;
  HIP_TRY(hipStreamWaitEvent(e->stream, e->refs_done, 0));
  HIP_TRY(hipStreamWaitEvent(e->stream4, e->refs_done, 0));
  HIP_TRY(hipStreamWaitEvent(e->stream2, e->refs_done, 0));
  return 0;
}

int quiesce(mip_engine *e) {
  if (flush_open(e) != 0 || wait_refs_readers(e) != 0) return -1;
  // asynchronous host searches still in flight use the engine buffers: let them finish
  HIP_TRY(hipStreamSynchronize(e->stream2));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream4));
  HIP_TRY(hipStreamSynchronize(e->stream3));
  return 0;
}

// Launch the open chunk: the engine filter over its frames (engine references), ONE search
// of all its frames -- each frame marking its own call's status set (SearchArgs::frame_status)
// -- each member call's downloads from its own frames, and each member call's completion
// event.  After a failure the members' tickets report it (call_errors flag 4).
int flush_open(mip_engine *e) {
  OpenChunk &o = e->open;
  if (!o.active) return 0;
  o.active = false;  // (whatever happens below, the chunk is over)
  if (o.members.empty()) return 0;
  const uint64_t first = o.first_call();
  // row (first - 1) % kCallRing: its previous user, the chunk of call first - kCallRing, has
  // completed (search_frames_call waits for that call before accepting call `first`)
  const size_t row = (size_t)((first - 1) % mip_engine::kCallRing) * e->hp_cap;
  for (const Member &m : o.members)
    for (int i = 0; i < m.n; i++) e->h_frame_status[row + m.f0 + i] = call_status(e, m.call);
  HostOutputs d;
  int rc = launch_chunk(e, o.k, o.nb, o.sig, call_status(e, first), e->d_frame_status + row, search_streams() == 2, false, &d);
  if (rc == 0) {
    e->stat_merged_launches++;
    e->stat_merged_calls += o.members.size();
    rc = download_members(e, o, d);
  }
  if (rc == 0 && hipEventRecord(e->slot_down[o.k % e->hp_slots], e->stream3) != hipSuccess) rc = fail("hipEventRecord failed");
  if (rc != 0) recover_after_failure(e);  // (as a failed call)
  for (const Member &m : o.members) {  // completion of every member (its ticket)
    if (rc != 0) e->call_errors[m.call] |= 4u;
    (void)hipEventRecord(e->call_done[(m.call - 1) % mip_engine::kCallRing], e->stream3);
  }
  o.members.clear();
  o.nb = 0;
  return rc;
}

extern "C" {

int mip_search_frames_async(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                            int32_t *costs_out, uint8_t *best_mode_out, int32_t *best_cost_out, int32_t *sad_out,
                            int32_t *satd_out, uint64_t *ticket) {
  return search_frames_call(e, frames, refs_or_null, nframes, {costs_out, best_mode_out, best_cost_out, sad_out, satd_out},
                            ticket, false);
}

int mip_wait(mip_engine *e, uint64_t ticket) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  if (ticket == 0 || ticket > e->host_calls) return fail("unknown ticket %llu", (unsigned long long)ticket);
  HIP_TRY(hipSetDevice(e->device));
  // the caller is about to block: an open chunk can gain no more calls from it (launched now,
  // behind the searches in flight; a failure is reported by its members' tickets)
  (void)flush_open(e);
  // a ticket older than the ring shares its event with a later call: waiting for that one
  // is later than needed, never too early
  HIP_TRY(hipEventSynchronize(e->call_done[(ticket - 1) % mip_engine::kCallRing]));
  // pageable outputs: copy the call's staged downloads out (and everything queued before)
  HIP_TRY(e->stage.drain(ticket));
  // input contract of this call only (every call <= ticket has completed: calls complete in
  // order); the flags of earlier calls stay with their own tickets
  harvest_status(e, ticket);
  const auto it = e->call_errors.find(ticket);
  if (it == e->call_errors.end()) return 0;
  const uint32_t f = it->second;
  e->call_errors.erase(it);
  if (f & 4u)
    return fail("host-API call %llu of this engine: its merged launch failed", (unsigned long long)ticket);
  char what[64];
  snprintf(what, sizeof what, "host-API call %llu of this engine", (unsigned long long)ticket);
  return contract_error(f, what);
}

int mip_search_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                      int32_t *costs_out, uint8_t *best_mode_out, int32_t *best_cost_out, int32_t *sad_out,
                      int32_t *satd_out) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  uint64_t ticket = 0;
  if (search_frames_call(e, frames, refs_or_null, nframes, {costs_out, best_mode_out, best_cost_out, sad_out, satd_out},
                         &ticket, true) != 0)
    return -1;
  return mip_wait(e, ticket);
}

int mip_flush(mip_engine *e) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  return flush_open(e);
}

int mip_host_stats(mip_engine *e, uint64_t *out, int n) {
  if (!e || !out || n < 0 || n > 4) return fail("bad arguments");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  const uint64_t v[4] = {e->host_calls, e->stat_launches, e->stat_merged_calls, e->stat_merged_launches};
  for (int i = 0; i < n; i++) out[i] = v[i];
  return 0;
}

int mip_trace_times(mip_engine *e, int enable) {
  if (!e) return fail("engine is NULL");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  if (flush_open(e) != 0) return -1;  // (merged chunks are not traced)
  if (enable && !e->tr_ev[0][0]) {
    // all events or none: a partial set would turn tracing on with null events
    hipEvent_t ev[mip_engine::kHostSlots][4] = {};
    for (auto &row : ev)
      for (hipEvent_t &x : row)
        if (hipEventCreate(&x) != hipSuccess) {
          for (auto &r2 : ev)
            for (hipEvent_t y : r2)
              if (y) (void)hipEventDestroy(y);
          return fail("hipEventCreate failed (tracing stays off)");
        }
    memcpy(e->tr_ev, ev, sizeof ev);
  }
  e->trace = enable != 0;
  return 0;
}

int mip_pop_times(mip_engine *e, double *upload_ms, double *filter_ms, int max, int *n) {
  if (!e || !n || max < 0) return fail("bad arguments");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  HIP_TRY(hipSetDevice(e->device));
  // pending chunks in sequence order (frame order)
  std::vector<int> order;
  for (int sl = 0; sl < mip_engine::kHostSlots; sl++)
    if (e->tr_frames[sl]) order.push_back(sl);
  std::sort(order.begin(), order.end(), [&](int a, int b) { return e->tr_chunk[a] < e->tr_chunk[b]; });
  for (int sl : order)
    if (drain_trace(e, sl) != 0) return -1;
  const int k = std::min<int>(max, (int)e->tr_times.size());
  for (int i = 0; i < k; i++) {
    if (upload_ms) upload_ms[i] = e->tr_times[i].first;
    if (filter_ms) filter_ms[i] = e->tr_times[i].second;
  }
  e->tr_times.erase(e->tr_times.begin(), e->tr_times.begin() + k);
  *n = k;
  return 0;
}

}  // extern "C"

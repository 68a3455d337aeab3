// host_policy.h -- what the host pipeline (host_pipeline.cpp) decides, as arithmetic: a call's
// signature, whether it joins or opens a merged chunk, and the chunk sizes of a chunked call --
// and the chunk size of the stage wrappers' walk (host_stages.cpp).
// No HIP dependency and no environment reads (knob values are arguments); unit-tested by
// tests/cpp/test_host_policy.cpp.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <vector>

#include "chunk_plan.h"
#include "host_stage.h"  // the bounce ring's limits

namespace mipgpu {

// The host output buffers of one host-API call (include/mipgpu.h mip_search_frames); null:
// not requested.
struct HostOutputs {
  int32_t *costs = nullptr;
  uint8_t *best_mode = nullptr;
  int32_t *best_cost = nullptr, *sad = nullptr, *satd = nullptr;
};

// Outputs and reference source of a host-API call: calls merge into one launch only when
// these agree (one kernel variant, one set of output tables for the chunk).  kSigDec:
// decisions only -- no cost, SAD or SATD table, K = 1, and a decision list -- the fused
// argmin, no table.
enum : unsigned { kSigCost = 1, kSigSad = 2, kSigSatd = 4, kSigBestMode = 8, kSigBestCost = 16, kSigRefs = 32, kSigDec = 64 };
// With the output bits above: the call's buffers in pageable memory (kPageIn: frames / refs).
enum : unsigned { kPageIn = 128 };

inline unsigned call_sig(const HostOutputs &o, bool caller_refs, int best_k) {
  const unsigned sig = (o.costs ? kSigCost : 0) | (o.sad ? kSigSad : 0) | (o.satd ? kSigSatd : 0) |
                       (o.best_mode ? kSigBestMode : 0) | (o.best_cost ? kSigBestCost : 0) | (caller_refs ? kSigRefs : 0);
  const bool dec = !(sig & (kSigCost | kSigSad | kSigSatd)) && best_k == 1 && (sig & (kSigBestMode | kSigBestCost));
  return sig | (dec ? kSigDec : 0);
}

// ---- Merged chunks (mip_engine::open) ----
constexpr int kMergeCalls = 32;  // calls of one merged chunk
enum { kMergeOff = 0, kMergeOn = 1, kMergeHold = 2 };  // MIPGPU_MERGE (host_pipeline.cpp merge_mode)

struct Member {
  uint64_t call;
  int f0, n;  // frames [f0, f0 + n) of the chunk
  HostOutputs out;
};
struct OpenChunk {
  bool active = false;
  uint64_t k = 0;       // chunk sequence number (slot k % hp_slots)
  int nb = 0;           // frames so far
  int cap = 0;          // frames it may take (merge_cap)
  unsigned sig = 0;     // outputs and reference source of its calls (call_sig)
  std::vector<Member> members;
  // The first member's call number; later than any call when there is none (a chunk whose
  // first upload failed is active without members).
  uint64_t first_call() const { return members.empty() ? ~0ull : members.front().call; }
};

// Frames an open chunk may take: its search can start only when all of its frames are
// uploaded, and the uploads run during the search launched before it -- one 1080p frame
// uploads in ~80 us, a launch of n frames searches in ~130 n + 47 us --
// so a chunk after one of n frames takes at most 1.625 n + 0.6 frames (1, 2, 3, 5, 8, 13, ...:
// a chunk of a whole slot right after a one-frame launch left the GPU idle for six uploads).
// hold (MIPGPU_MERGE=hold): up to a slot.
inline int merge_cap(int last_frames, int slot_cap, bool hold) {
  if (hold) return slot_cap;
  return std::max(2, std::min(slot_cap, (13 * std::max(1, last_frames) + 5) / 8));
}

// What a host-API call does about the open chunk (the rules at mip_engine::open).
struct MergeState {  // the open chunk and the pipeline before the call
  bool active;
  unsigned sig;
  int nb, cap, members;
  int last_frames;  // frames of the last launched chunk
  bool launched;    // a chunk has been launched (its completion can be asked for)
  bool called;      // a call has been accepted (its completion can be asked for)
};
struct MergeCall {
  unsigned sig;
  int nframes;
  bool small;  // page-locked buffers, fewer frames than a slot, no tracing
  bool sync;
};
enum class Take { kChunks, kJoin, kOpen };
struct MergeDecision {
  bool flush_first = false;    // launch the open chunk before anything else
  Take take = Take::kChunks;   // join the open chunk, open one, or take the chunked path
  int cap = 0;                 // kOpen: the new chunk's cap
  bool flush_after = false;    // kJoin / kOpen: launch the chunk once the call is in it
};
// search_done(): the search launched before the open chunk has completed (the GPU would idle);
// last_call_running(): the last accepted call has not completed (the pipeline is busy).  Each
// is one event query, asked only where its answer decides.
template <class SearchDone, class LastCallRunning>
MergeDecision merge_decision(const MergeState &s, const MergeCall &c, int mode, int slot_cap, SearchDone &&search_done,
                             LastCallRunning &&last_call_running) {
  MergeDecision d;
  const bool small = c.small && mode != kMergeOff;
  bool active = s.active;
  int last_frames = s.last_frames;
  auto flush = [&] {
    d.flush_first = true;
    active = false;
    if (s.members) last_frames = s.nb;  // (a chunk without members launches nothing)
  };
  if (active && mode == kMergeOn && s.launched && search_done()) flush();  // this call then opens the next chunk
  if (active) {
    if (small && s.sig == c.sig && s.nb + c.nframes <= s.cap && s.members < kMergeCalls) d.take = Take::kJoin;
    else flush();
  }
  if (!active && small && !c.sync) {
    const int cap = merge_cap(last_frames, slot_cap, mode == kMergeHold);
    if (c.nframes <= cap && (mode == kMergeHold || (s.called && last_call_running()))) {
      d.take = Take::kOpen;
      d.cap = cap;
    }
  }
  if (d.take == Take::kChunks) return d;
  const bool join = d.take == Take::kJoin;
  d.flush_after = (join ? s.nb : 0) + c.nframes >= (join ? s.cap : d.cap) || (join ? s.members : 0) + 1 >= kMergeCalls || c.sync;
  return d;
}

// ---- Chunked calls ----
struct FrameBytes {  // bytes per frame of a call's buffers
  size_t frame;      // samples (frames, references)
  size_t table;      // one cost / SAD / SATD table
  size_t decisions;  // the best-mode list (the best-cost list: four times as much)
};
struct ChunkCall {
  int nframes;
  unsigned sig;       // call_sig
  unsigned pageable;  // the sig's output bits and kPageIn: buffers that go through the bounce ring
  bool idle;          // nothing is queued before the call
  bool sync;
};

inline size_t download_bytes(unsigned sig, const FrameBytes &b) {  // full tables only
  return (size_t)(((sig & kSigCost) ? 1 : 0) + ((sig & kSigSad) ? 1 : 0) + ((sig & kSigSatd) ? 1 : 0)) * b.table;
}

// Piece size to reserve in the bounce ring for a call with pageable buffers: a whole slot of
// the largest buffer this call moves (not this call's chunk: a call into an idle pipeline is
// cut in two, and growing the ring later drains it and pins new memory).
inline size_t ring_piece_bytes(unsigned sig, int slot_cap, const FrameBytes &b) {
  const size_t per_frame = std::max({b.frame, download_bytes(sig, b) ? b.table : 0,
                                     (sig & kSigBestCost) ? b.decisions * 4 : ((sig & kSigBestMode) ? b.decisions : 0)});
  return std::min<size_t>((size_t)slot_cap * per_frame, kMaxRingPiece);
}

// Frames per chunk of a chunked call (at most; chunk_plan cuts the call).
//  - A call into an idle pipeline (nothing queued before it) is cut in two (at most a slot's
//    frames each), so that its own upload, search and download overlap; calls queued behind
//    others keep whole-slot chunks (call_chunk_cap).
//  - Full tables to the host (PCIe-bound): chunks of at most chunk_mb MiB (MIPGPU_CHUNK_MB;
//    <= 0: 1024) of downloads, so the first download starts early and, for pageable outputs,
//    the bounce ring's copy-out keeps up (1080p, 8 calls of 128 frames: 96-frame chunks 831
//    frames/s pageable, 32-frame 892, 16-frame 1018; page-locked 990 / 963 / 1036).  Decisions
//    only keeps the larger chunks (its rate is the search's, whose launches are more efficient
//    with more frames).
//  - Equal chunks: a short last chunk would leave the search waiting for the next upload.
//  - Pageable transfers take ring bytes per buffer (footprint(bytes), pieces of `piece` bytes):
//    a chunk's downloads must fit the ring beside the next chunk's uploads (host_stage.h
//    kMaxChunkPieces), else enqueueing them waits on the host for the chunk's own search.
template <class Footprint>
int chunk_frames(const ChunkCall &c, int slot_cap, int nslots, const FrameBytes &b, int chunk_mb, size_t piece,
                 Footprint &&footprint) {
  int sb = call_chunk_cap(c.nframes, slot_cap, nslots, c.idle);
  if (const size_t down = download_bytes(c.sig, b)) {
    const size_t cap = (size_t)(chunk_mb > 0 ? chunk_mb : 1024) << 20;
    sb = std::max(1, std::min<int>(sb, (int)(cap / down)));
  }
  auto equal_chunks = [&] {
    const int nch = (c.nframes + sb - 1) / sb;
    sb = (c.nframes + nch - 1) / nch;
  };
  equal_chunks();
  if (!c.pageable) return sb;
  auto bytes = [&](unsigned bit, size_t per_frame) -> size_t {
    return (c.pageable & c.sig & bit) ? footprint((size_t)sb * per_frame) : 0;
  };
  auto fits = [&] {
    const size_t down_b = bytes(kSigCost, b.table) + bytes(kSigSad, b.table) + bytes(kSigSatd, b.table) +
                          bytes(kSigBestMode, b.decisions) + bytes(kSigBestCost, b.decisions * 4);
    const size_t up_b = ((c.pageable & kPageIn) ? footprint((size_t)sb * b.frame) : 0) * ((c.sig & kSigRefs) ? 2 : 1);
    return down_b <= kMaxChunkPieces * piece && up_b <= kMaxChunkUploadPieces * piece;
  };
  while (sb > 1 && !fits()) sb--;
  equal_chunks();
  return sb;
}

// The chunks of a chunked call, each at most sb = chunk_frames(...) frames.  A longer call into
// an idle pipeline ramps its first chunks up from a few frames: the search starts after one
// small upload instead of a whole chunk's (64 frames: 4.7 ms at 56 GB/s), and each chunk's
// upload still fits under the previous chunk's search (upload 74 us per 1080p frame, search
// ~131 us: growth x1.75).  A synchronous decisions-only call (mip_search_frames: nothing can
// queue behind it) ramps its last chunks down the same way, so the download left after the
// last search is a few frames' (decision lists: 67 us per frame, under the next chunk's
// search; full tables are download-bound throughout, where a ramp-down changes nothing).  The
// rest of the call keeps equal chunks of at most sb.  ramp (MIPGPU_RAMP): kRampOff no ramps,
// kRampUp no ramp-down.
enum { kRampOff = 0, kRampUp = 1, kRampBoth = 2 };
inline std::vector<int> call_chunks(const ChunkCall &c, int sb, int nslots, const FrameBytes &b, int ramp, int *nhead,
                                    int *ntail) {
  const bool ramps = nslots == 4 && sb >= 16 && ramp != kRampOff;
  return chunk_plan(c.nframes, sb, ramps && c.idle && c.nframes >= 2 * sb,
                    ramps && c.sync && !download_bytes(c.sig, b) && ramp != kRampUp, nhead, ntail);
}

// ---- Stage wrappers (host_stages.cpp walk_chunks) ----
// Frames per chunk of a stage wrapper's walk: what the engine buffers hold (max_batch), and for
// a call with a per-frame device table of table_bytes_per_frame (0: none) as many frames as keep
// that table within kAngularTableBytes, one at least: a 1080p frame's angular cost table is
// 189 MB.
constexpr size_t kAngularTableBytes = (size_t)256 << 20;
inline int stage_chunk_frames(int max_batch, int nframes, size_t table_bytes_per_frame) {
  const int chunk = std::min(max_batch, nframes);
  if (!table_bytes_per_frame) return chunk;
  return (int)std::max<size_t>(1, std::min((size_t)chunk, kAngularTableBytes / table_bytes_per_frame));
}

}  // namespace mipgpu

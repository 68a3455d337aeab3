// CPU unit test of the host pipeline's policy (csrc/host_policy.h).  Built and run by
// tests/test_host_policy.py (g++, plain and with ASan / UBSan; no GPU).
//  a. call_sig: all 32 output combinations x caller references x best_k 1 / 3 against the rule
//     written out here; merge_cap: its chains written out by hand.
//  b. merge_decision: a table of (open chunk, pipeline, call, mode) -> action that covers every
//     rule in the comment at mip_engine::open (engine.h), with counting callables that pin how
//     often each of the two event queries is asked; OpenChunk::first_call without members.
//  c. chunk_frames / call_chunks for 3888 cases -- call lengths x slot layouts x idle x sync x
//     outputs x page-locked / pageable with 1 MiB and 64 MiB ring pieces x two frame sizes, and
//     the knobs -- as digests (FNV-1a 64 of the rows `line` renders, per call length) and 41
//     rows in full.  Both were recorded from the arithmetic as it stood inside mipgpu.cpp
//     search_frames_chunks (commit e387e3c, lines 1395-1478) by a scratch program that held
//     those lines with the HIP calls and getenv replaced by arguments (the ring's footprint:
//     bytes rounded up to 4096, its default alignment) and printed the same rows in the same
//     order.
//  d. stage_chunk_frames (the stage wrappers' walk): max_batch, the call's frames and the
//     angular table bound, each where it decides, from the rule written out by hand.
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_policy.h"
#include "mip_tables.h"

using namespace mipgpu;

static int fails = 0;
#define CHECK(c, ...)                                 \
  do {                                                \
    if (!(c)) {                                       \
      if (fails++ < 20) {                             \
        std::printf("FAIL %s: ", #c);                 \
        std::printf(__VA_ARGS__);                     \
        std::printf("\n");                            \
      }                                               \
    }                                                 \
  } while (0)

static void test_call_sig() {
  int32_t i32 = 0;
  uint8_t u8 = 0;
  for (int m = 0; m < 32; m++)
    for (int refs = 0; refs < 2; refs++)
      for (int k : {1, 3}) {
        HostOutputs o;
        if (m & 1) o.costs = &i32;
        if (m & 2) o.best_mode = &u8;
        if (m & 4) o.best_cost = &i32;
        if (m & 8) o.sad = &i32;
        if (m & 16) o.satd = &i32;
        unsigned want = (m & 1 ? 1u : 0) | (m & 8 ? 2u : 0) | (m & 16 ? 4u : 0) | (m & 2 ? 8u : 0) | (m & 4 ? 16u : 0) |
                        (refs ? 32u : 0);
        // decisions only: no cost, SAD or SATD table, best_k == 1, best mode or best cost
        if (!(m & (1 | 8 | 16)) && k == 1 && (m & (2 | 4))) want |= 64u;
        CHECK(call_sig(o, refs, k) == want, "outputs %d refs %d k %d: %u, want %u", m, refs, k, call_sig(o, refs, k), want);
      }
  static_assert(kSigCost == 1 && kSigSad == 2 && kSigSatd == 4 && kSigBestMode == 8 && kSigBestCost == 16 &&
                kSigRefs == 32 && kSigDec == 64, "the bits call_sig's expectations are written in");
  HostOutputs dec;
  dec.best_mode = &u8;
  CHECK(call_sig(dec, false, 1) == (kSigBestMode | kSigDec), "best mode alone is decisions only");
  CHECK(call_sig(dec, true, 3) == (kSigBestMode | kSigRefs), "K = 3 needs the table");
  CHECK(call_sig(HostOutputs{}, false, 1) == 0, "no output: not decisions only");
}

static void test_merge_cap() {
  // from a one-frame launch, each cap launched in turn
  const std::vector<int> chain96 = {2, 3, 5, 8, 13, 21, 34, 55, 90, 96, 96};
  const std::vector<int> chain8 = {2, 3, 5, 8, 8}, chain4 = {2, 3, 4, 4};
  const std::vector<int> chain1 = {2, 2};  // (never below 2; no call is small on a one-frame slot)
  for (const auto &[slot, chain] : {std::pair<int, std::vector<int>>{96, chain96}, {8, chain8}, {4, chain4}, {1, chain1}}) {
    int last = 1;
    for (size_t i = 0; i < chain.size(); i++) {
      const int c = merge_cap(last, slot, false);
      CHECK(c == chain[i], "slot %d step %zu after %d frames: %d, want %d", slot, i, last, c, chain[i]);
      last = c;
    }
    for (int lf : {0, 1, 7, 500}) CHECK(merge_cap(lf, slot, true) == slot, "hold: slot %d", slot);
    CHECK(merge_cap(0, slot, false) == 2, "before any launch: slot %d", slot);
  }
}

struct Row {
  const char *name;
  MergeState s;
  MergeCall c;
  int mode;
  bool done, running;  // the queries' answers
  MergeDecision want;
  int want_done_q, want_running_q;
};

static void test_merge_decision() {
  const unsigned D = kSigBestMode | kSigBestCost | kSigDec, F = kSigCost;
  const int slot = 8;
  // states: {active, sig, nb, cap, members, last_frames, launched, called}
  const MergeState none{false, 0, 0, 0, 0, 1, true, true};
  const MergeState never{false, 0, 0, 0, 0, 0, false, false};
  const MergeState open3{true, D, 3, 5, 3, 1, true, true};   // three one-frame calls, room for two frames
  const MergeState open4{true, D, 4, 5, 2, 1, true, true};
  const MergeState first{true, D, 1, 2, 1, 0, false, true};  // opened before any launch (hold)
  const MergeState many{true, D, 4, 8, kMergeCalls, 1, true, true};
  const MergeState almost{true, D, 4, 8, kMergeCalls - 1, 1, true, true};
  const MergeState empty{true, D, 0, 5, 0, 5, true, true};   // its first upload failed
  // calls: {sig, nframes, small, sync}
  const MergeCall d1{D, 1, true, false}, d2{D, 2, true, false}, d3{D, 3, true, false}, f1{F, 1, true, false};
  const MergeCall big{D, 8, false, false}, d1sync{D, 1, true, true}, f1sync{F, 1, true, true};
  const Take C = Take::kChunks, J = Take::kJoin, O = Take::kOpen;
  // want: {flush_first, take, cap, flush_after}
  const Row rows[] = {
      {"busy pipeline: a small call opens a chunk", none, d1, kMergeOn, false, true, {false, O, 2, false}, 0, 1},
      {"idle pipeline: launches on its own", none, d1, kMergeOn, false, false, {false, C, 0, false}, 0, 1},
      {"first call of the engine: nothing to ask", never, d1, kMergeOn, false, true, {false, C, 0, false}, 0, 0},
      {"hold: opens into an idle pipeline, unasked", none, d1, kMergeHold, false, false, {false, O, slot, false}, 0, 0},
      {"hold: the engine's first call opens too", never, d1, kMergeHold, false, false, {false, O, slot, false}, 0, 0},
      {"mode 0: never", none, d1, kMergeOff, false, true, {false, C, 0, false}, 0, 0},
      {"synchronous call: never opens", none, d1sync, kMergeOn, false, true, {false, C, 0, false}, 0, 0},
      {"not small: chunked path", none, big, kMergeHold, false, true, {false, C, 0, false}, 0, 0},
      {"more frames than merge_cap: chunked path", none, d3, kMergeOn, false, true, {false, C, 0, false}, 0, 0},
      {"a call that fills its new chunk launches it", none, d2, kMergeOn, false, true, {false, O, 2, true}, 0, 1},
      {"joins: same outputs, room left, predecessor still searching", open3, d1, kMergeOn, false, true, {false, J, 0, false}, 1, 0},
      {"predecessor's search completed: launch, open the next", open3, d1, kMergeOn, true, true, {true, O, 5, false}, 1, 1},
      {"predecessor's search completed, pipeline idle after it", open3, d1, kMergeOn, true, false, {true, C, 0, false}, 1, 1},
      {"hold: the predecessor is not asked about", open3, d1, kMergeHold, true, true, {false, J, 0, false}, 0, 0},
      {"nothing launched yet: no search to ask about", first, d1, kMergeOn, true, true, {false, J, 0, true}, 0, 0},
      {"full by frames: launch, open the next (7 after 4)", open4, d2, kMergeOn, false, true, {true, O, 7, false}, 1, 1},
      {"full by frames, hold: launch, open the next", open4, d2, kMergeHold, false, true, {true, O, slot, false}, 0, 0},
      {"the call that fills the chunk launches it", open4, d1, kMergeOn, false, true, {false, J, 0, true}, 1, 0},
      {"full by kMergeCalls: launch, open the next", many, d1, kMergeHold, false, true, {true, O, slot, false}, 0, 0},
      {"the kMergeCalls-th call launches the chunk", almost, d1, kMergeHold, false, true, {false, J, 0, true}, 0, 0},
      {"other outputs: launch, open the next", open3, f1, kMergeOn, false, true, {true, O, 5, false}, 1, 1},
      {"not small: launch, chunked path", open3, big, kMergeOn, false, true, {true, C, 0, false}, 1, 0},
      {"synchronous call joins and launches", open3, d1sync, kMergeOn, false, true, {false, J, 0, true}, 1, 0},
      {"synchronous call that cannot join: launch, chunked path", open3, f1sync, kMergeHold, false, true, {true, C, 0, false}, 0, 0},
      {"mode 0 with a chunk open: launch, chunked path", open3, d1, kMergeOff, true, true, {true, C, 0, false}, 0, 0},
      {"a chunk without members launches nothing: the last launch still counts", empty, f1, kMergeOn, false, true,
       {true, O, 8, false}, 1, 1},
  };
  for (const Row &r : rows) {
    int nd = 0, nr = 0;
    const MergeDecision d = merge_decision(
        r.s, r.c, r.mode, slot, [&] { return nd++, r.done; }, [&] { return nr++, r.running; });
    CHECK(d.flush_first == r.want.flush_first && d.take == r.want.take && d.flush_after == r.want.flush_after,
          "%s: flush_first %d take %d flush_after %d", r.name, d.flush_first, (int)d.take, d.flush_after);
    if (r.want.take == Take::kOpen) CHECK(d.cap == r.want.cap, "%s: cap %d, want %d", r.name, d.cap, r.want.cap);
    CHECK(nd == r.want_done_q && nr == r.want_running_q, "%s: %d search-done and %d last-call queries, want %d and %d", r.name,
          nd, nr, r.want_done_q, r.want_running_q);
  }
  OpenChunk oc;
  oc.active = true;  // (its first upload failed)
  CHECK(oc.first_call() == ~0ull && !(oc.first_call() <= 1000), "an active chunk without members holds no call");
  oc.members.push_back(Member{41, 0, 1, HostOutputs{}});
  oc.members.push_back(Member{42, 1, 1, HostOutputs{}});
  CHECK(oc.first_call() == 41, "first member's call");
}

static std::string line(int n, int nslots, int cap, int idle, int sync, int out, int host, int res, int refs, int mb, int ramp) {
  const int w = res ? 264 : 1920, h = res ? 136 : 1080;
  const size_t nctus = (size_t)((w + 127) / 128) * ((h + 127) / 128);
  const FrameBytes fb{(size_t)w * h * 2, nctus * MIP_COSTS_PER_CTU * 4, nctus * MIP_CUS_PER_CTU};
  const unsigned outs = out == 0 ? (kSigBestMode | kSigBestCost | kSigDec) : out == 1 ? kSigCost : (kSigCost | kSigSad | kSigSatd);
  const unsigned sig = outs | (refs ? kSigRefs : 0);
  const ChunkCall c{n, sig, host ? (outs & ~kSigDec) | kPageIn : 0u, idle != 0, sync != 0};
  const size_t piece = host == 2 ? (64u << 20) : (1u << 20);
  const int sb = chunk_frames(c, cap, nslots, fb, mb, piece, [](size_t b) { return (b + 4095) / 4096 * 4096; });
  int nhead = -1, ntail = -1;
  const std::vector<int> plan = call_chunks(c, sb, nslots, fb, ramp, &nhead, &ntail);
  char buf[160];
  std::snprintf(buf, sizeof buf, "%d %d %d %d %d %d %d %d %d %d %d : %d %d %d :", n, nslots, cap, idle, sync, out, host, res,
                refs, mb, ramp, sb, nhead, ntail);
  std::string s = buf;
  for (size_t i = 0; i < plan.size();) {  // run-length: count x frames
    size_t j = i;
    while (j < plan.size() && plan[j] == plan[i]) j++;
    std::snprintf(buf, sizeof buf, " %zux%d", j - i, plan[i]);
    s += buf;
    i = j;
  }
  return s;
}

// FNV-1a 64 over the rows of a group, each followed by a newline.
struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void row(const std::string &s) {
    for (const char ch : s + "\n") h = (h ^ (unsigned char)ch) * 1099511628211ull;
  }
};

static void test_chunks() {
  const int frames[] = {1, 2, 3, 5, 8, 9, 13, 64, 128, 384};
  const int slots[][2] = {{3, 1}, {3, 4}, {3, 8}, {4, 16}, {4, 96}};
  // recorded digests: one per call length (360 rows each), then the knob / caller-reference rows
  const uint64_t want[11] = {0x88ca213f5cf67aa3ull, 0x6b466c9cb49959a3ull, 0xa15907d25720df73ull, 0x0b7b7399b294f4fbull,
                             0x6dd88be747df8613ull, 0x8b6f5560f888b94bull, 0xacf6549851408acbull, 0x50c524ec377474f5ull,
                             0x5e0cce1aa2b13377ull, 0x58ec781276bc61b1ull, 0x0a4d92427d8e2ffbull};
  int rows = 0;
  for (int g = 0; g < 10; g++) {
    Fnv f;
    for (auto &s : slots)
      for (int idle = 0; idle < 2; idle++)
        for (int sync = 0; sync < 2; sync++)
          for (int out = 0; out < 3; out++)
            for (int host = 0; host < 3; host++)
              for (int res = 0; res < 2; res++, rows++) f.row(line(frames[g], s[0], s[1], idle, sync, out, host, res, 0, 0, 2));
    CHECK(f.h == want[g], "calls of %d frames: digest %llx, recorded %llx", frames[g], (unsigned long long)f.h,
          (unsigned long long)want[g]);
  }
  Fnv k;  // MIPGPU_CHUNK_MB=64, MIPGPU_RAMP=0 / up, pageable with caller references; 1080p
  for (int n : {64, 128, 384})
    for (int si = 3; si < 5; si++)
      for (int idle = 0; idle < 2; idle++)
        for (int sync = 0; sync < 2; sync++)
          for (int out = 0; out < 3; out++, rows += 4) {
            k.row(line(n, slots[si][0], slots[si][1], idle, sync, out, 0, 0, 0, 64, 2));
            k.row(line(n, slots[si][0], slots[si][1], idle, sync, out, 0, 0, 0, 0, 0));
            k.row(line(n, slots[si][0], slots[si][1], idle, sync, out, 0, 0, 0, 0, 1));
            k.row(line(n, slots[si][0], slots[si][1], idle, sync, out, 1, 0, 1, 0, 2));
          }
  CHECK(k.h == want[10], "knob rows: digest %llx, recorded %llx", (unsigned long long)k.h, (unsigned long long)want[10]);
  CHECK(rows == 3888, "%d rows", rows);
  // recorded rows in full, the first with each (chunk frames, head ramp, tail ramp) among the 3888: columns frames, slots,
  // slot cap, idle, sync, outputs (0 dec, 1 cost, 2 cost + SAD + SATD), host (0 page-locked, 1 pageable with 1 MiB ring
  // pieces, 2 with 64 MiB pieces), size (0 1920x1080, 1 264x136), caller refs, chunk_mb (0 default), ramp (0 off, 1 up,
  // 2 both) : chunk frames, head ramp chunks, tail ramp chunks : the call's chunks, run-length (count x frames)
  const char *const recorded[] = {
      "1 3 1 0 0 0 0 0 0 0 2 : 1 0 0 : 1x1",
      "2 3 4 0 0 0 0 0 0 0 2 : 2 0 0 : 1x2",
      "3 3 4 0 0 0 0 0 0 0 2 : 3 0 0 : 1x3",
      "5 3 8 0 0 0 0 0 0 0 2 : 5 0 0 : 1x5",
      "8 3 4 0 0 0 0 0 0 0 2 : 4 0 0 : 2x4",
      "8 3 8 0 0 0 0 0 0 0 2 : 8 0 0 : 1x8",
      "9 4 16 0 0 0 0 0 0 0 2 : 9 0 0 : 1x9",
      "13 3 8 0 0 0 0 0 0 0 2 : 7 0 0 : 1x7 1x6",
      "13 4 16 0 0 0 0 0 0 0 2 : 13 0 0 : 1x13",
      "64 3 8 0 0 2 0 0 0 0 2 : 6 0 0 : 9x6 2x5",
      "64 4 16 0 0 0 0 0 0 0 2 : 16 0 0 : 4x16",
      "64 4 16 0 1 0 0 0 0 0 2 : 16 0 3 : 2x14 1x13 1x12 1x7 1x4",
      "64 4 16 1 0 0 0 0 0 0 2 : 16 3 0 : 1x4 1x7 1x12 2x14 1x13",
      "64 4 16 1 1 0 0 0 0 0 2 : 16 3 3 : 1x4 1x7 1x12 2x9 1x12 1x7 1x4",
      "64 4 96 0 0 0 0 0 0 0 2 : 64 0 0 : 1x64",
      "64 4 96 0 0 0 1 1 0 0 2 : 32 0 0 : 2x32",
      "64 4 96 0 1 0 1 1 0 0 2 : 32 0 3 : 1x21 1x20 1x12 1x7 1x4",
      "64 4 96 1 0 0 1 1 0 0 2 : 32 3 0 : 1x4 1x7 1x12 1x21 1x20",
      "64 4 96 1 1 0 1 1 0 0 2 : 32 3 1 : 1x4 1x7 1x12 1x19 1x18 1x4",
      "128 4 96 0 0 0 1 1 0 0 2 : 43 0 0 : 2x43 1x42",
      "128 4 96 0 0 1 0 0 0 0 2 : 19 0 0 : 2x19 5x18",
      "128 4 96 0 1 0 0 0 0 0 2 : 64 0 4 : 2x42 1x21 1x12 1x7 1x4",
      "128 4 96 0 1 0 1 1 0 0 2 : 43 0 5 : 2x24 1x36 1x21 1x12 1x7 1x4",
      "128 4 96 1 0 0 0 0 0 0 2 : 64 4 0 : 1x4 1x7 1x12 1x21 2x42",
      "128 4 96 1 0 0 1 1 0 0 2 : 43 5 0 : 1x4 1x7 1x12 1x21 1x36 2x24",
      "128 4 96 1 0 1 0 0 0 0 2 : 19 3 0 : 1x4 1x7 1x12 3x18 3x17",
      "128 4 96 1 1 0 0 0 0 0 2 : 64 4 2 : 1x4 1x7 1x12 1x21 1x37 1x36 1x7 1x4",
      "128 4 96 1 1 0 1 1 0 0 2 : 43 5 1 : 1x4 1x7 1x12 1x21 1x36 2x22 1x4",
      "384 4 96 0 0 0 0 0 0 0 2 : 96 0 0 : 4x96",
      "384 4 96 0 0 0 1 1 0 0 2 : 55 0 0 : 6x55 1x54",
      "384 4 96 0 0 1 0 0 0 0 2 : 20 0 0 : 4x20 16x19",
      "384 4 96 0 1 0 0 0 0 0 2 : 96 0 6 : 1x81 2x80 1x63 1x36 1x21 1x12 1x7 1x4",
      "384 4 96 0 1 0 1 1 0 0 2 : 55 0 5 : 4x51 2x50 1x36 1x21 1x12 1x7 1x4",
      "384 4 96 0 1 0 2 0 0 0 2 : 64 0 6 : 1x61 3x60 1x63 1x36 1x21 1x12 1x7 1x4",
      "384 4 96 1 0 0 0 0 0 0 2 : 96 6 0 : 1x4 1x7 1x12 1x21 1x36 1x63 1x81 2x80",
      "384 4 96 1 0 0 1 1 0 0 2 : 55 5 0 : 1x4 1x7 1x12 1x21 1x36 4x51 2x50",
      "384 4 96 1 0 0 2 0 0 0 2 : 64 6 0 : 1x4 1x7 1x12 1x21 1x36 1x63 1x61 3x60",
      "384 4 96 1 0 1 0 0 0 0 2 : 20 3 0 : 1x4 1x7 1x12 19x19",
      "384 4 96 1 1 0 0 0 0 0 2 : 96 6 6 : 1x4 1x7 1x12 1x21 1x36 1x63 2x49 1x63 1x36 1x21 1x12 1x7 1x4",
      "384 4 96 1 1 0 1 1 0 0 2 : 55 5 5 : 1x4 1x7 1x12 1x21 1x36 4x45 1x44 1x36 1x21 1x12 1x7 1x4",
      "384 4 96 1 1 0 2 0 0 0 2 : 64 6 6 : 1x4 1x7 1x12 1x21 1x36 1x63 2x49 1x63 1x36 1x21 1x12 1x7 1x4",
  };
  for (const char *want_row : recorded) {
    int v[11];
    const int got = std::sscanf(want_row, "%d %d %d %d %d %d %d %d %d %d %d", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6],
                                &v[7], &v[8], &v[9], &v[10]);
    CHECK(got == 11, "malformed row: %s", want_row);
    if (got != 11) break;
    const std::string have = line(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10]);
    CHECK(have == want_row, "recorded %s\n     now      %s", want_row, have.c_str());
  }
  // the ring's piece: a slot of the call's largest buffer, at most 64 MiB
  const FrameBytes hd{1920 * 1080 * 2, (size_t)135 * MIP_COSTS_PER_CTU * 4, (size_t)135 * MIP_CUS_PER_CTU};
  CHECK(ring_piece_bytes(kSigBestMode | kSigDec, 1, hd) == hd.frame, "decisions: the frame is the largest buffer");
  CHECK(ring_piece_bytes(kSigCost, 1, hd) == hd.table, "full table, one frame: the table (52.8 MB)");
  CHECK(ring_piece_bytes(kSigCost, 4, hd) == (64u << 20), "capped at 64 MiB");
  const FrameBytes tiny{8 * 8 * 2, (size_t)MIP_COSTS_PER_CTU * 4, MIP_CUS_PER_CTU};
  CHECK(ring_piece_bytes(kSigBestCost | kSigDec, 3, tiny) == (size_t)3 * MIP_CUS_PER_CTU * 4, "best costs: four bytes per CU");
}

static void test_stage_chunk_frames() {
  CHECK(stage_chunk_frames(200, 3, 0) == 3, "fewer frames than max_batch: the call's frames");
  CHECK(stage_chunk_frames(2, 3, 0) == 2, "more frames than max_batch: max_batch");
  CHECK(stage_chunk_frames(2, 2, 0) == 2 && stage_chunk_frames(1, 1, 0) == 1, "no bound");
  CHECK(stage_chunk_frames(8, 5, kAngularTableBytes / 5) == 5 && stage_chunk_frames(8, 5, kAngularTableBytes / 4) == 4,
        "the table bound cuts only where it is the smaller");
  CHECK(stage_chunk_frames(4, 3, kAngularTableBytes + 1) == 1 && stage_chunk_frames(4, 3, (size_t)1 << 40) == 1,
        "a bound below one frame's table: one frame");
  // one CTU's angular cost table: 5380 CUs x 65 modes x int32; 268435456 / 1398800 = 191.9
  static_assert(MIP_CUS_PER_CTU == 5380 && kAngularTableBytes == 268435456, "the figures of this case");
  const size_t table = (size_t)MIP_CUS_PER_CTU * 65 * 4;
  CHECK(table == 1398800, "%zu", table);
  for (int n : {191, 192, 200, 1000})
    CHECK(stage_chunk_frames(200, n, table) == 191, "%d frames on max_batch 200: %d, want 191", n,
          stage_chunk_frames(200, n, table));
  CHECK(stage_chunk_frames(200, 190, table) == 190 && stage_chunk_frames(100, 200, table) == 100, "below the bound");
}

int main() {
  test_call_sig();
  test_merge_cap();
  test_merge_decision();
  test_chunks();
  test_stage_chunk_frames();
  if (fails) return 1;
  std::printf("host_policy: ok\n");
  return 0;
}

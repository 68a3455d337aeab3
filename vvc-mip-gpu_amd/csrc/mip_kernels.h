// mip_kernels.h -- launch interface between the C-ABI host code (mipgpu.cpp, host_pipeline.cpp)
// and the gfx950 kernels (mip_search.hip, mip_decide.hip, mip_filter.hip, mip_fixup.hip,
// mip_predict.hip, mip_predict_angular.hip, mip_partition.hip, mip_intra.hip, mip_angular.hip,
// mip_candidates.hip).  The angular family is nine kernels from two bodies: six cost kernels in
// mip_angular.hip and three block outputs in mip_predict_angular.hip, each a body with a policy for
// the reference lines and the interpolation; the argument structs below grow by derivation.
// Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mipgpu.h"  // mip_pred_item
#include "mip_work.h"  // work-list records, size classes, table layout (shared with work_plan.h)

namespace mipgpu {

struct SearchArgs {
  const uint16_t *orig;   // [frames][height][width] original samples (distortion)
  const uint16_t *refs;   // reference-sample source: == orig, or the filtered frames
  int32_t *cost;          // [frames][nctus][97840]  min(2*SAD, SATD); null: decisions only
  // Decisions only ([frames][nctus][5380] per-CU best mode / cost): a task that searches
  // all of a CU's mode pairs writes the CU's decision directly; CUs whose pairs are cut over
  // several tasks (the `split` lists) meet in best_cost as a packed running argmin
  // (cost << 5 | mode, all ones before the launch, atomicMin), unpacked after it
  // (launch_dec_split); CUs the reference leaves undefined get 0xff / kUnavailable from the
  // `dfill` lists.
  uint8_t *best_mode;     // optional
  int32_t *best_cost;
  // optional: the split CUs' packed running argmins go here instead of best_cost (same CU
  // indexing; all ones before the launch, reset to all ones by the unpacking launch_dec_split
  // -- the host pipeline keeps it initialised across launches, so no init kernel runs)
  uint32_t *split_acc;
  const uint16_t *dfill;  // undefined CUs of (v, q): CU indices inside the CTU,
  const int *dfill_begin; // [dfill_begin[4v+q], dfill_begin[4v+q+1])
  int32_t *sad;           // optional, same layout
  int32_t *satd;          // optional, same layout
  const WaveTask *tasks;  // per (quadrant, wave) task lists, concatenated
  const Job *jobs;
  const int *list_begin;  // task list of (CTU variant v, quadrant q, slice s), index l = (4v+q)*slices+s:
                          // [list_begin[l], list_begin[l+1])
  const uint32_t *fill;   // unavailable cost entries of (v, q) (uint4 units inside the CTU's cost
  const int *fill_begin;  // block): [fill_begin[4v+q], fill_begin[4v+q+1])
  const uint8_t *ctu_var; // [nctus] CTU variant (work_plan.h ctu_variants): which CUs are defined
  const uint4 *tables;    // kTableBytes: MIP matrices for the MFMA (mip_work.h)
  int width, height;
  int ctu_cols, nctus;
  int ctu0, nrange;       // CTUs searched: [ctu0, ctu0 + nrange) of every frame (whole frame:
                          // 0, nctus); cost entries of the other CTUs are not written
  int slices;             // workgroups (task lists) per CTU quadrant
  uint32_t *queue;        // kQueueWords counters, zero at launch (the kernel leaves them zero
                          // again): [c] next item of chunk c (c < kQueueChunks), then
                          // [kQueueChunks] workgroups done
  uint32_t nitems;        // frames * nrange * 4 * slices (set by launch_search)
  // Small launches (one queue chunk): item order longest first (LPT).  order[i] = the i-th
  // (CTU, quadrant, slice) item of a frame, index ctu * 4 * slices + quadrant * slices +
  // slice, by decreasing estimated cost; queue index q -> item order[q / nframes] of frame
  // q % nframes.  Null: raster order (frame-major).  Whole-frame launches only.
  const uint32_t *order;
  uint32_t nframes;
  uint32_t chunks;        // queue chunks, 1..kQueueChunks (set by launch_search)
  uint64_t *wave_clock;   // profiling (MIPGPU_WAVE_TIMING): [workgroup][kClockSlots] cycles per
                          // task of the workgroup's list; else null
  // Input contract (samples are 10-bit): a workgroup that stages an original sample above
  // 1023 stores 1 to status[kStatusOrig], a caller-supplied reference sample above 1023
  // (check_refs) 1 to status[kStatusRefs].  status is engine-owned page-locked host memory
  // (read by the host after the search; only ever written when the contract is broken).
  uint32_t *status;
  // Merged host-pipeline chunks (several host-API calls in one launch, host_pipeline.cpp
  // flush_open): frame f of the launch marks frame_status[f] (its own call's status set)
  // instead of status; null otherwise.  Read only when the contract is broken.
  uint32_t *const *frame_status;
  int check_refs;
  // 16-wave launches with the longest-first order and original references (pair mode,
  // mip_search.hip pair_loop): the first `nonempty` queue positions hold the items with
  // tasks, the rest only fills.  0: items one at a time.
  uint32_t nonempty;
};
constexpr int kStatusOrig = 0, kStatusRefs = 1, kStatusWords = 4;
constexpr uint32_t kAbove10Bits = 0xfc00fc00u;  // any of bits 10..15 in either half
constexpr int kClockSlots = 128;
// Item queue of one launch: the items are cut into kQueueChunks contiguous chunks, one per
// XCD (workgroups b and b + 8 share an XCD), each with its own counter (mip_search.hip
// take_item).
constexpr int kQueueChunks = 8;
constexpr int kQueueWords = 16;  // 8 chunk counters, the done counter, padding to 64 bytes

struct BestArgs {
  const int32_t *cost;
  uint8_t *best_mode;     // [total_cus][k]
  int32_t *best_cost;     // [total_cus][k]
  int total_cus;          // frames * nctus * 5380
  int k;                  // decision list length, 1..kMaxBestK
};
constexpr int kMaxBestK = 32;

struct FilterArgs {
  const uint16_t *in;
  uint16_t *out;
  int width, height, nframes;
  int filter;             // reference whitelist index (constants.h:25-34)
  int kernel_idx;
};

// Workgroups of the search kernel resident on the current device at once (persistent grid
// size); computed once per engine (mip_engine_create), 0 on error.
int search_resident_groups(bool alt_refs, bool wide);
// The four-wave twin (mip_search.hip compiled again with -DMIP_SIX_WAVES=0
// -DMIP_FOUR_WAVE_TWIN=1): 8-wave workgroups, two per CU, for the host pipeline's small
// alternating chunks; same arguments, no wide launches (0 / hipErrorInvalidValue).
#if !defined(MIP_FOUR_WAVE_TWIN) || !MIP_FOUR_WAVE_TWIN  // (in the twin the names above are these)
int search_resident_groups_four(bool alt_refs, bool wide);
#endif
// What a launch_search call launched (diagnostics: mip_search_census): the kernel instance
// mip_search_kernel<alt, dec, pf, waves> and its launch modes after launch_search's own
// filtering of the arguments.
struct SearchLaunchInfo {
  int waves;     // per workgroup: 12, 16 or 8
  bool alt;      // alternative references
  bool dec;      // decisions only
  bool pf;       // the prefetching instance
  bool pair;     // pair mode (SearchArgs::nonempty > 0)
  bool chunked;  // more than one queue chunk
  bool ordered;  // longest-first item order (SearchArgs::order)
};
// done: optional event recorded by the kernel's own dispatch (hipExtLaunchKernel's stop
// event) instead of a separate marker packet behind it.  info: optional, filled for every
// launch that was attempted.
hipError_t launch_search(const SearchArgs &a, int nframes, bool alt_refs, int resident, bool wide, hipStream_t s,
                         hipEvent_t done = nullptr, SearchLaunchInfo *info = nullptr);
#if !defined(MIP_FOUR_WAVE_TWIN) || !MIP_FOUR_WAVE_TWIN
hipError_t launch_search_four(const SearchArgs &a, int nframes, bool alt_refs, int resident, bool wide, hipStream_t s,
                         hipEvent_t done = nullptr, SearchLaunchInfo *info = nullptr);
#endif
hipError_t launch_best_modes(const BestArgs &a, hipStream_t s);
// Decisions only, CUs whose mode pairs are cut over several tasks (split CUs of the CTU's
// variant: [split_begin[v], split_begin[v+1]) of `split`, at most max_split per variant):
// init = true sets their best_cost entries to all ones (before the search); init = false
// unpacks the packed argmin in place into best_mode / best_cost (after it).  With `acc`
// (SearchArgs::split_acc) the packed argmins are read from acc, which the unpacking resets
// to all ones (init is then never needed).
struct SplitArgs {
  const uint16_t *split;
  const int *split_begin;
  const uint8_t *ctu_var;
  uint8_t *best_mode;
  int32_t *best_cost;
  int nctus, ctu0, nrange, max_split;
  uint32_t *acc;
};
hipError_t launch_dec_split(const SplitArgs &a, int nframes, bool init, hipStream_t s);
hipError_t launch_filter(const FilterArgs &a, hipStream_t s);
// Streaming device-to-device copy (16-byte aligned, multiple of 16 bytes): HBM calibration.
hipError_t launch_copy(const void *src, void *dst, size_t bytes, hipStream_t s);
// Several copies in one launch (the merged chunks' downloads into the members' page-locked,
// device-mapped host buffers: one dispatch instead of one per buffer).
struct CopyPiece {
  const uint8_t *src;
  uint8_t *dst;
  uint64_t bytes;
};
constexpr int kMaxCopyPieces = 64;
struct CopyPieces {
  CopyPiece p[kMaxCopyPieces];
  int n;
};
hipError_t launch_gather_copy(const CopyPieces &a, hipStream_t s);
// Exact per-CU search of `n` CUs of every frame (same outputs as the search kernel: cost /
// SAD / SATD tables or, decisions only, the decision in a.best_mode / a.best_cost).
hipError_t launch_fixup(const SearchArgs &a, const FixupCu *cus, int n, int nframes, hipStream_t s);

// Prediction output (predict_kernel): the samples of `n` list items, each checked by the
// kernel against the write rule of include/mipgpu.h.
struct PredictArgs {
  const uint16_t *refs;       // [nframes][height][width] reference-sample source
  const mip_pred_item *items; // device list
  long long n;                // items, <= 2^31 - 256
  const uint8_t *unavail;     // [nctus * 5380] 1 = the CU is not predicted (mip_unavailable_cus)
  const uint32_t *geo;        // [5380] CU inside the CTU: shape | x << 8 | y << 16
  uint16_t *out;              // 8-byte aligned
  long long out_samples;
  uint32_t *skipped;          // optional: items that were not written are counted here
  int width, height, ctu_cols, nctus, nframes;
  int refs_vec;               // refs is 8-byte aligned: top rows are read 4 samples per load
  int regular;                // MIP_PRED_REGULAR: items with mode MIP_MODE_PLANAR / MIP_MODE_DC are emitted
                              // (launches the kernel's second instance; 0: the MIP-only one)
};
hipError_t launch_predict(const PredictArgs &a, hipStream_t s);
// MIP_PRED_ANGULAR (angular_predict_kernel, mip_predict_angular.hip: the block-output body with
// substituted lines and two taps): the items of the same list
// whose mode is an angular code.  Launched behind launch_predict on the same stream: it emits what
// that kernel rejected and counted, and takes one off a.skipped for every item it emits
// (refs_vec and regular are not used).
hipError_t launch_predict_angular(const PredictArgs &a, hipStream_t s);

// CTU partition decision (partition_kernel, mip_partition.hip): one workgroup per (frame, CTU).
struct PartitionPenalty {
  int32_t v[47];              // per shape, 0 .. 1 << 20 (checked by the caller)
};
struct PartitionArgs {
  const int32_t *best_cost;   // [nframes][nctus][5380]
  const uint8_t *best_mode;   // same shape; needed for items only
  uint8_t *leaf;              // optional outputs (include/mipgpu.h)
  int32_t *ctu_cost, *ctu_leaves;
  mip_pred_item *items;
  int width, height, ctu_cols, nctus, nframes;
  PartitionPenalty penalty;
};
hipError_t launch_partition(const PartitionArgs &a, hipStream_t s);

// Planar / DC baseline costs and the decision merge (intra_kernel, mip_intra.hip): workgroups
// stride over the (frame, CTU, 64x64 CU or 32x32 block) items.
struct IntraArgs {
  const uint16_t *orig;       // [nframes][height][width] original samples (distortion)
  const uint16_t *refs;       // reference-sample source: == orig, the filtered or the caller's frames
  const uint8_t *unavail;     // [nctus * 5380] 1 = the CU's entries are MIP_COST_UNAVAILABLE
  const uint32_t *slots;      // [16][slots_per_block] lane slots (intra_plan.h intra_build_slots)
  int slots_per_block;        // a multiple of 64
  int32_t *cost, *sad, *satd; // optional tables [nframes][nctus * 5380][2], 8-byte aligned
  uint8_t *best_mode;         // optional merge, both or neither: [nframes][nctus * 5380]
  int32_t *best_cost;
  int32_t bias[2];            // Planar, DC: 0 .. 1 << 20 (checked by the caller)
  int width, height, ctu_cols, nctus, nframes;
};
hipError_t launch_intra(const IntraArgs &a, hipStream_t s);

// Angular intra costs, the best angular mode and its merge into the decisions (angular_kernel,
// mip_angular.hip: the cost body with substituted lines and two taps, no refinement): the work
// items, window and lane slots of the intra kernel, a wave-uniform loop over the mode list.
struct AngularArgs {
  const uint16_t *orig;       // as IntraArgs
  const uint16_t *refs;
  const uint8_t *unavail;
  const uint32_t *slots;
  int slots_per_block;
  int32_t *cost, *sad, *satd; // optional tables [nframes][nctus * 5380][65], slot = mode - 2
  uint8_t *ang_mode;          // optional, both or neither: [nframes][nctus * 5380]
  int32_t *ang_cost;
  uint8_t *best_mode;         // optional merge, both or neither
  int32_t *best_cost;
  int32_t bias;               // 0 .. 1 << 20 (checked by the caller)
  int width, height, ctu_cols, nctus, nframes;
  int nmodes;                 // 1..65
  uint32_t listed[3];         // bit (mode - 2): the mode is in the list
  uint32_t modes[65];         // the list in increasing mode order (angular_plan.h ang_pack)
};
hipError_t launch_angular(const AngularArgs &a, hipStream_t s);

// Coarse-to-fine angular search (angular_refine_kernel: the same body with its refinement pass):
// angular_kernel's items, window and coarse loop, then per CU the +-1 neighbours of its own best
// `nseeds` modes.
struct AngularRefineArgs : AngularArgs {
  uint8_t *tried;             // optional: [nframes][nctus * 5380] modes evaluated per CU
  int nseeds;                 // min(seeds, nmodes): 1..3
  uint32_t all[65];           // ang_pack of every mode 2..66 (staged in LDS: a per-lane lookup)
};
hipError_t launch_angular_refine(const AngularRefineArgs &a, hipStream_t s);

// The angular family with extended reference lines (mip_angular_refs MIP_ANG_REFS_EXTENDED):
// angular_ext_kernel and angular_ext_refine_kernel are the cost body with the policy that stages
// the two line extensions and lengthens each CU's main line by its entry of `ext`;
// angular_ext_predict_kernel is the block-output body with the longer per-item line.  The launch
// rules are the family's; `ext` is required.  (angular_ext_kernel and angular_tap4_kernel have that
// walk and policy written out as a body of their own: mip_angular.hip says why.)
struct AngularExtArgs : AngularRefineArgs {  // (the plain launch does not look at tried, nseeds, all)
  const uint16_t *ext;        // [nctus * 5380] E_top | E_left << 8 (mip_extended_refs, the set of unavail)
};
hipError_t launch_angular_ext(const AngularExtArgs &a, hipStream_t s);
hipError_t launch_angular_ext_refine(const AngularExtArgs &a, hipStream_t s);
struct PredictExtArgs : PredictArgs {
  const uint16_t *ext;        // as AngularExtArgs::ext
};
hipError_t launch_predict_angular_ext(const PredictExtArgs &a, hipStream_t s);

// The angular family with VVC's 4-tap luma interpolation (mip_angular_interp MIP_ANG_INTERP_4TAP):
// angular_tap4_kernel and angular_tap4_refine_kernel are the cost body and
// angular_tap4_predict_kernel the block-output body with the _ext policies' lines and the line
// P = ... of the predictor replaced.  One kernel per role serves both mip_angular_refs settings:
// ext == NULL is MIP_ANG_REFS_SUBSTITUTED (every length 0).  The launch rules are the family's.
struct AngularTap4Args : AngularExtArgs {  // (ext may be NULL)
  uint32_t coef[64];          // angular_plan.h ang_coef_word at G << 5 | f (staged in LDS: a per-lane lookup)
};
hipError_t launch_angular_tap4(const AngularTap4Args &a, hipStream_t s);
hipError_t launch_angular_tap4_refine(const AngularTap4Args &a, hipStream_t s);
struct PredictTap4Args : PredictExtArgs {  // (ext may be NULL)
  uint32_t coef[64];          // as AngularTap4Args::coef
};
hipError_t launch_predict_angular_tap4(const PredictTap4Args &a, hipStream_t s);

// K-best candidate lists over the mode families (candidates_kernel, mip_candidates.hip): one lane
// per CU, one wave per workgroup, the CU's keys (candidates_plan.h) in one LDS row.
struct CandidatesArgs {
  const uint8_t *mip_mode;    // optional family, both or neither: [total_cus][kin]
  const int32_t *mip_cost;
  int kin;                    // 1..32 with a MIP list
  const int32_t *intra_cost;  // optional family: [total_cus][2]
  int32_t intra_bias[2];      // 0 .. 1 << 20 (checked by the caller)
  const int32_t *ang_cost;    // optional family: [total_cus][65]
  int32_t ang_bias;
  uint8_t *modes;             // outputs, at least one: [total_cus][k]
  int32_t *costs;
  long long total_cus;        // frames * nctus * 5380, <= 2^31 - 256
  int k;                      // 1..32
};
hipError_t launch_candidates(const CandidatesArgs &a, hipStream_t s);

}  // namespace mipgpu

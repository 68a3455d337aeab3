/* mipgpu.h -- C ABI of the MI355X-native VVC MIP search engine (libmipgpu.so).
 *
 * Drop-in boundary for the hot path of iagostorch/VVC-MIP-GPU.  The reference has no
 * FFI layer: its path is main.cpp's OpenCL dispatch of
 *     filterFrame_<type>  (intra.cl:1639-3823, dispatched main.cpp:700-761)
 *     initBoundaries      (intra.cl:17,   main.cpp:802-843)
 *     MIP_ReducedPred     (intra.cl:349,  main.cpp:909-945)
 *     upsampleDistortion  (intra.cl:545,  main.cpp:995-1199, built 3x with -DSIZEID)
 * plus the cost read-back readMemobjsIntoArray_Distortion (main_aux_functions.h:585-630).
 * Each entry point below replaces one of those steps (cited per function); the C++ CLI
 * (vvc-mip-gpu_amd/cli/mipgpu_cli.cpp) replaces main.cpp on top of it.
 *
 * Conventions: plain pointers and sizes, int status (0 = ok, <0 = error, message via
 * mip_last_error()), no exceptions cross the boundary.  Host buffers are owned by the
 * caller; device buffers of the engine are owned by the engine.  One engine per device;
 * an engine must be used by one host thread at a time.  Samples are 10-bit values in
 * uint16; frames are row-major, consecutive frames are concatenated.
 *
 * Input contract: every sample of a frame (and of caller-supplied reference frames) is at
 * most 1023, like the reference's 10-bit constants (valueDC 512, clip 1023,
 * constants.cl:22-23).  The search kernel detects a staged sample above 1023 and the engine
 * reports it as an error (costs of such a frame are not valid): mip_search_frames /
 * mip_wait fail for the call that searched it; device-API searches are asynchronous, so
 * their violation is reported by mip_check_input or by the engine's next search call.
 *
 * Cost layout (identical to the reference's ALL_stridedDistortionsPerCtu,
 * constants.h:1558-1631): int32 [frames][nCTUs][97840], entry
 *     ctu*97840 + shape_offset + cu*2*modes + mode
 * with the 47 CU shapes in reference order.  Samples are addressed like the reference does,
 * by linear index y * width + x, so CUs right of the frame (widths that are not multiples
 * of 128) read the next row's samples and get the reference's costs.  CUs whose cost the
 * reference leaves undefined -- below the frame (stale LDS, intra.cl:96-98), reading past
 * the frame's end, or (engine filter) reading a filtered sample computed from past the
 * frame's end -- are reported as MIP_COST_UNAVAILABLE (mip_unavailable_cus lists them).
 */
#ifndef MIPGPU_H
#define MIPGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPGPU_ABI_VERSION 7
#define MIP_COSTS_PER_CTU_ABI 97840
#define MIP_CUS_PER_CTU_ABI 5380
#define MIP_COST_UNAVAILABLE 0x7fffffff

/* Reference filter whitelist order, constants.h:25-34. */
typedef enum {
  MIP_FILTER_NONE = -1,               /* USE_ALTERNATIVE_SAMPLES=0: references = originals */
  MIP_FILTER_1D_INT = 0,              /* filterFrame_1d_int            intra.cl:3267 */
  MIP_FILTER_1D_FLOAT = 1,            /* filterFrame_1d_float          intra.cl:1828 */
  MIP_FILTER_2D_INT = 2,              /* filterFrame_2d_int_quarterCtu intra.cl:2856 */
  MIP_FILTER_2D_FLOAT = 3,            /* filterFrame_2d_float_quarterCtu intra.cl:1639 */
  MIP_FILTER_1D_INT_5x5 = 4,          /* filterFrame_1d_int_5x5        intra.cl:3508 */
  MIP_FILTER_1D_FLOAT_5x5 = 5,        /* filterFrame_1d_float_5x5      intra.cl:2539 */
  MIP_FILTER_2D_INT_5x5 = 6,          /* filterFrame_2d_int_5x5_quarterCtu intra.cl:3042 */
  MIP_FILTER_2D_FLOAT_5x5 = 7         /* filterFrame_2d_float_5x5_quarterCtu intra.cl:2311 */
} mip_filter_type;

typedef struct {
  int filter;          /* mip_filter_type; MIP_FILTER_NONE for original references */
  int kernel_idx;      /* --KernelIdx: tap set index (0..4 for 3x3, 0..2 for 5x5) */
  int max_batch;       /* frames per device batch (device buffers sized for this); >= 1 */
  int want_sad_satd;   /* also produce the SAD / SATD tables (MAX_PERFORMANCE_DIST=0) */
  int slices_per_ctu;  /* workgroups per 64x64 CTU quadrant in the search kernel; 0 = auto
                          (chosen per launch: more, smaller workgroups for small batches) */
  int best_k;          /* decision list length K of best_mode_out / best_cost_out (1..32;
                          0 = 1): the K lowest-cost modes of every CU, see mip_topk_device */
} mip_opts;

typedef struct mip_engine mip_engine;

/* Defaults: no filter, kernel_idx 0, max_batch 1, no SAD/SATD, auto slicing. */
void mip_opts_default(mip_opts *opts);

/* Create an engine on HIP device `device` for width x height frames (width, height
 * multiples of 4).  Replaces main.cpp:90-598 (device/context/queue/buffer/program set-up).
 * Returns 0 and *out, or <0. */
int mip_engine_create(int device, int width, int height, const mip_opts *opts, mip_engine **out);
int mip_engine_destroy(mip_engine *e);

/* Geometry helpers. */
int mip_num_ctus(int width, int height);                     /* intra.cl:31-33 */
int64_t mip_costs_per_frame(int width, int height);          /* nCTUs * 97840 */
int64_t mip_cus_per_frame(int width, int height);            /* nCTUs * 5380 */
const char *mip_shape_name(int shape);                       /* main_aux_functions.h:296-401 */
/* Geometry of CU shape `shape` (0..46): w, h, modes (without transposition), CU count per
 * CTU, cost offset inside the CTU block.  Returns 0 or <0 for a bad index. */
int mip_shape_info(int shape, int *w, int *h, int *modes, int *ncu, int *cost_offset);
/* CTU-relative position of CU `cu` of `shape` (ALL_X_POS / ALL_Y_POS, constants.h:1235-1354). */
int mip_cu_position(int shape, int cu, int *x, int *y);

/* CUs whose costs this engine reports as MIP_COST_UNAVAILABLE for width x height frames,
 * with references from the engine's own filter `filter` (MIP_FILTER_NONE: original
 * references): 1 per CU in the order ctu*5380 + shape CU prefix + cu, for nCTUs*5380 CUs.
 * They are the CUs the reference leaves undefined geometrically (below the frame, stale LDS
 * intra.cl:96-98; reading past the frame's end) and, with a filter, the CUs that read a
 * filtered sample the reference's filter computes from memory past the frame's end (its
 * linear tile addressing, intra.cl:2904-2909 / 3330-3332; e.g. the last frame row of the
 * separable 3-tap filters when the height is not a multiple of 32).  Filtered samples that
 * two of the reference's tiles store with different values (widths that are not multiples
 * of 128, intra.cl:3037) are not undefined here: the engine uses the owning tile's value,
 * one of the reference's two outcomes.  Host only; returns 0 or <0. */
int mip_unavailable_cus(int width, int height, int filter, uint8_t *cu_out);

/* Low-pass filter of `nframes` host frames (filterFrame_<type>, main.cpp:700-761).
 * out must hold nframes frames.  Synchronous. */
int mip_filter_frames(mip_engine *e, const uint16_t *frames, int nframes, int filter,
                      int kernel_idx, uint16_t *out);

/* Full MIP search of `nframes` host frames: H2D, [filter], search, D2H, in chunks through
 * the engine's three streams (uploads, search, downloads) and buffer slots -- 4 slots of
 * max_batch/4 frames (max_batch >= 16), else 3 slots of max_batch frames (the engine's
 * buffers hold 3 x max_batch frames then) -- so that one chunk's upload, the previous
 * chunk's search and the one before's download run at the same time, also across calls:
 * an engine searching one frame per call (max_batch 1, the reference's per-frame loop with
 * BUFFER_SLOTS 2, main.cpp:886-898, main_aux_functions.h:5, 617) overlaps frame k+1's
 * upload and frame k-1's download with frame k's search when the calls are queued with
 * mip_search_frames_async.  A call into an idle pipeline is cut into two chunks.
 * Replaces the per-frame loop main.cpp:678-1241 + readMemobjsIntoArray_Distortion.
 * refs_or_null: caller-provided reference-sample frames (alternative samples computed
 * elsewhere); NULL = originals, or the engine's filter when opts.filter != NONE.
 * costs_out: int32 [nframes][nCTUs*97840] (may be NULL if only best modes are wanted).
 * best_mode_out / best_cost_out: optional per-CU decision lists, [nframes][nCTUs*5380][K]
 * with K = opts.best_k (K = 1: the argmin; mip_topk_device gives the ordering rules;
 * 0xff / MIP_COST_UNAVAILABLE for unavailable CUs).
 * sad_out / satd_out: optional (need opts.want_sad_satd).  Synchronous.
 * Host buffers: page-locked memory (mip_host_alloc, hipHostRegister) is transferred by DMA
 * directly; pageable memory (malloc, the reference's return_minSadHad, main.cpp:656-668)
 * goes through the engine's page-locked bounce ring (one arena of 16 pieces of up to 64 MB,
 * parallel host copies), allocated at its first use. */
int mip_search_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null,
                      int nframes, int32_t *costs_out, uint8_t *best_mode_out,
                      int32_t *best_cost_out, int32_t *sad_out, int32_t *satd_out);

/* mip_search_frames without the final wait: enqueues the call's chunks behind the calls
 * still in flight (the upload / search / download pipeline stays full from one call to the
 * next) and returns a ticket (> 0) in *ticket.  The host buffers must stay valid and
 * unmodified (inputs) / unread (outputs) until mip_wait(e, ticket) returns.  Calls complete
 * in order.  mip_filter_frames waits for every call in flight.
 * Merged launches (ABI 7): a call with page-locked buffers and fewer frames than one buffer
 * slot (opts.max_batch below 16, else max_batch / 4) that arrives while the pipeline is busy
 * joins the engine's open chunk -- calls with the same outputs and reference source share ONE
 * search launch (one-frame calls then run at the multi-frame launch rate).  The chunk is
 * launched when full, when an incompatible call arrives, when a later call finds the GPU idle,
 * at any mip_wait / mip_flush / synchronous call / device-API call of the engine.  Every call
 * keeps its own ticket, outputs and input-contract status.  A caller that queues a call and
 * then neither waits nor calls again should call mip_flush (launches the open chunk now). */
int mip_search_frames_async(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null,
                            int nframes, int32_t *costs_out, uint8_t *best_mode_out,
                            int32_t *best_cost_out, int32_t *sad_out, int32_t *satd_out,
                            uint64_t *ticket);

/* Block until the call with this ticket (and every earlier one) has completed: its outputs
 * are in host memory.  Pageable output buffers are complete (copied out of the bounce ring by
 * its completion thread) when this returns -- an asynchronous call with pageable outputs
 * must be waited for.  Fails
 * if THIS call's search staged a sample above 1023 (input contract; every call has its own
 * status, so an earlier or later call's violation is reported by that call's own wait). */
int mip_wait(mip_engine *e, uint64_t ticket);

/* Launch the engine's open (merged) chunk now, if any (see mip_search_frames_async); no wait. */
int mip_flush(mip_engine *e);

/* Device block cache (ABI 7).  Freeing a large device allocation halves every later host <->
 * device copy of the process on the MI355X platform (profiles/r06_free_repro.txt), so
 * mip_engine_destroy parks its buffers of >= 16 MB in a process-wide cache that later engines
 * on the same device reuse (the smallest block that fits).  mip_device_cache reports the
 * parked bytes of `device` and the blocks reused so far; release = 1 frees the parked blocks
 * first (hipFree: the copies of the process may slow down afterwards). */
int mip_device_cache(int device, int release, uint64_t *idle_bytes, uint64_t *reused_blocks);

/* Device-resident variant (inputs already in HBM; all pointers are device pointers,
 * `stream` is a hipStream_t; NULL means the default (null) stream, as in HIP).
 * Asynchronous on `stream`.
 * d_refs NULL: originals, or the engine filter applied into engine scratch.
 * d_costs NULL = decisions only (no cost table is written): needs d_best_cost and
 * opts.best_k == 1, no SAD / SATD; the search kernel keeps every CU's argmin itself (packed
 * in d_best_cost, unpacked in place).  mip_search_frames takes this path whenever no table
 * (costs / SAD / SATD) is requested and best_k == 1.  The optional outputs may be NULL. */
int mip_search_device(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs,
                      int nframes, int32_t *d_costs, int32_t *d_sad, int32_t *d_satd,
                      uint8_t *d_best_mode, int32_t *d_best_cost, void *stream);

/* Input-contract check of the device-API searches issued on `stream` (a hipStream_t, NULL =
 * the null stream): synchronises the stream, returns <0 (mip_last_error names it) if a
 * search of this engine staged a sample above 1023 since the last check, else 0. */
int mip_check_input(mip_engine *e, void *stream);

/* mip_search_device restricted to the CTUs [ctu_begin, ctu_end) (raster order) of every
 * frame: writes exactly those CTUs' blocks of the full-size cost / SAD / SATD tables and
 * leaves the others untouched.  The frames are complete (CUs at the range's top and left
 * edge read their reference samples from the rows / columns outside the range, the filter
 * runs over whole frames), so ranges that tile the frame give the full table: one large
 * frame split into CTU-row bands over several GPUs.  No decision
 * lists (run mip_topk_device on the assembled table). */
int mip_search_device_range(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs,
                            int nframes, int ctu_begin, int ctu_end, int32_t *d_costs,
                            int32_t *d_sad, int32_t *d_satd, void *stream);

/* Per-CU decision lists (no reference counterpart; what an encoder's full-RD stage takes
 * from the cost table, e.g. VTM's numModesForFullRD MIP candidates): for every CU of
 * `nframes` device cost tables (reference layout), the k lowest-cost modes in increasing
 * cost order, ties to the lower mode index.  Modes are numbered as the log's Mode column
 * (0..2*modes-1, transposed modes >= modes).  Entries past the CU's 2*modes modes and all
 * entries of unavailable CUs are 0xff / MIP_COST_UNAVAILABLE.  k in 1..32.
 * d_modes: uint8 [nframes][nCTUs*5380][k]; d_costs_k: int32, same shape (either may be
 * NULL).  Asynchronous on `stream`. */
int mip_topk_device(const int32_t *d_costs, int width, int height, int nframes, int k,
                    uint8_t *d_modes, int32_t *d_costs_k, void *stream);

/* Prediction output (additive to ABI 7; no reference counterpart -- the reference's
 * upsampleDistortion builds the predicted samples in local memory, measures them and drops
 * them, intra.cl:545-1166): the predicted samples of chosen (CU, mode) pairs, what an encoder
 * needs after the decision (residual, the full-RD stage on mip_topk_device's candidates, a
 * predicted frame).  The stages are the reference's: boundaries with linear indexes and padding
 * (intra.cl:96-107, 232-243, 127-141, 259-279), the matrix product with transposition
 * (intra.cl:415-485), horizontal then vertical upsampling (intra.cl:815-912) -- so the SAD /
 * SATD of an emitted block against the original samples are the entries of the SAD / SATD
 * tables.
 *
 * A list item names a frame of the call, a CU and a mode, and says where its w x h samples go
 * in the output buffer `out` of out_samples uint16: row r of the block at
 * out[offset + r*pitch .. + w).  mip_pred_layout fills pitch / offset for the two usual
 * layouts; callers may set their own.
 *
 * Write rule.  An item is written only when ALL of these hold:
 *   - 0 <= frame < nframes and 0 <= cu < nCTUs*5380;
 *   - the CU is available for this engine, i.e. not in mip_unavailable_cus(width, height,
 *     filter) (with caller-supplied references: the MIP_FILTER_NONE set);
 *   - 0 <= mode < 2*modes of the CU's shape;
 *   - pitch >= w; pitch and offset are multiples of 4 samples; offset >= 0;
 *   - offset + (h-1)*pitch + w <= out_samples.
 * Any other item writes nothing and reads no sample; it is counted in the skipped counter.
 * The device kernel checks every item itself: a device-side list is data, and a bad entry
 * never becomes an out-of-bounds access.  Items whose blocks overlap in `out` (a frame layout
 * with CUs of several shapes, wrapped CUs) are the caller's business: which one wins is
 * unspecified. */
typedef struct {
  int32_t frame;   /* 0 .. nframes-1 */
  int32_t cu;      /* ctu*5380 + shape CU prefix + cu: the index used by best_mode_out */
  int32_t mode;    /* 0 .. 2*modes-1, numbered as the log's Mode column; anything else (0xff) = none */
  int32_t pitch;   /* samples between consecutive rows of the block in `out` */
  int64_t offset;  /* sample index in `out` of the block's top-left sample */
} mip_pred_item;   /* 24 bytes */

#define MIP_PRED_PACKED 0   /* blocks back to back, row-major w x h, list order (pitch = w) */
#define MIP_PRED_FRAME  1   /* blocks at their place in frame-shaped canvases: pitch = width,
                               offset = frame*W*H + y*W + x, the reference's linear addressing
                               (CUs right of the frame wrap into the next row; every available
                               CU stays inside its frame) */
#define MIP_PRED_NONE 0xffff

/* Fill pitch and offset of `n` items (frame, cu set by the caller) for `layout` and return the
 * output size in *out_samples.  Packed: offset = exclusive prefix sum of w*h in list order
 * (items with mode "none" and unavailable CUs reserve their block too).  Frame: out_samples =
 * nframes*W*H.  Host only (no HIP call).  <0 for a frame or cu out of range. */
int mip_pred_layout(int width, int height, int nframes, int layout,
                    mip_pred_item *items, int64_t n, int64_t *out_samples);

/* Predict the items of a device list into d_out (8-byte aligned, as d_items), asynchronous on
 * `stream`.  Reference source as in mip_search_device: d_refs NULL = the originals, or the
 * engine's filter applied into engine scratch (nframes <= max_batch then); otherwise the
 * caller's frames.  Samples of d_out that no item writes are left as they were.  d_skipped:
 * optional device word, zeroed by the caller; it holds the number of items not written when the
 * call's work on `stream` has completed (before that its value is unspecified: the call may run
 * more than one kernel over the list, and they settle the count between them). */
int mip_predict_device(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes,
                       const mip_pred_item *d_items, int64_t n, uint16_t *d_out, int64_t out_samples,
                       uint32_t *d_skipped, void *stream);

/* Synchronous host variant: uploads, filters if the engine has a filter and no references are
 * given, predicts, downloads (no pipelining).  Like mip_filter_frames it first waits for every
 * call in flight (an open merged chunk is launched).  The list is validated on the host: a
 * frame or cu out of range fails the call; items the write rule excludes otherwise are skipped.
 * Samples of `out` that no item writes are MIP_PRED_NONE; *skipped (optional) receives the
 * number of items not written.  With refs the originals are not read (frames may be NULL). */
int mip_predict_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                       const mip_pred_item *items, int64_t n, uint16_t *out, int64_t out_samples,
                       int64_t *skipped);

/* Prediction with flags (additive to ABI 7).  flags == 0: exactly mip_predict_device /
 * mip_predict_frames -- outputs, skipped count and errors (those entry points are flags == 0 calls
 * of these).  Any bit other than MIP_PRED_REGULAR and MIP_PRED_ANGULAR (bit 2 included) is an
 * error before any launch.
 *
 * MIP_PRED_REGULAR: the mode condition of the write rule gains one alternative -- mode ==
 * MIP_MODE_PLANAR or mode == MIP_MODE_DC (defined with mip_intra_device below) is valid for every
 * shape, 64x64 included; every other condition is unchanged.  Such an item's samples are exactly
 * the `out` of the Planar / DC / PDPC definition under mip_intra_device: top and left are the MIP
 * path's complete boundaries, topRight = top[w-1], bottomLeft = left[h-1], 32-bit arithmetic,
 * clipped to 0..1023, the reference frame read by linear index.  Reference source and availability
 * set are those of mip_predict_device; the originals are not read (with d_refs / refs given the
 * frames may be NULL).  So the SAD, SATD and min(2*SAD, SATD) of an emitted block against the
 * original samples are the mip_intra_device table entries of that CU and slot (0 Planar, 1 DC),
 * and the device list of mip_partition_device on merged decisions gives whole predicted frames.
 *
 * MIP_PRED_ANGULAR: the mode condition gains one more alternative -- MIP_MODE_ANGULAR(2) <= mode <=
 * MIP_MODE_ANGULAR(66) (defined with mip_angular_device below) is valid for every shape; every
 * other condition is unchanged, and codes 0x80, 0x81, 0xc3 and above stay invalid.  Such an item's
 * samples are exactly the `out` of the predictor under mip_angular_device for mode m = mode - 0x80,
 * sample for sample, with the reference source and availability set of mip_predict_device; the
 * originals are not read.  So the SAD, SATD and cost of an emitted block against the original
 * samples are the mip_angular_device table entries of that CU and slot m - 2.  The two bits are
 * independent: with MIP_PRED_ANGULAR alone Planar / DC items are skipped and counted.  Without the
 * bit a call does what it did before the bit existed: same outputs, same count, same launches. */
#define MIP_PRED_REGULAR 1u   /* flags bit: items with mode MIP_MODE_PLANAR / MIP_MODE_DC are emitted */
#define MIP_PRED_ANGULAR 4u   /* flags bit: items with mode MIP_MODE_ANGULAR(2..66) are emitted */
int mip_predict_device_ex(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes,
                          const mip_pred_item *d_items, int64_t n, uint16_t *d_out, int64_t out_samples,
                          uint32_t *d_skipped, unsigned flags, void *stream);
int mip_predict_frames_ex(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                          const mip_pred_item *items, int64_t n, uint16_t *out, int64_t out_samples,
                          unsigned flags, int64_t *skipped);

/* CTU partition decision (additive to ABI 7; no reference counterpart -- the reference stops at
 * the cost table): which CUs to use.  The 47 CU shapes are closed under VTM's intra partition
 * defaults for a 128x128 CTU -- quad-tree splits down to 8x8, binary and ternary splits only
 * below 64, at most three of them under a quad-tree leaf, minimum side 4 -- which reach exactly
 * the 5376 CUs of the 46 shapes other than 64x64 (the four 64x64 CUs are the quad-tree nodes one
 * level up).  mip_partition_device finds, per CTU, the minimum-cost partition over that CU set
 * from the per-CU best costs.
 *
 * Input, per CU of a frame: best_cost, int32 [nframes][nCTUs*5380], the K = 1 list of
 * mip_search_device / mip_topk_device (MIP_COST_UNAVAILABLE marks unavailable CUs); best_mode
 * (optional, same shape, uint8); penalty, an optional HOST array of one int32 per shape in
 * 0 .. 1<<20 (NULL = zeros; anything else is an error before any launch).
 *
 * Leaf cost of CU c of shape s: best_cost[c] + penalty[s].  A CU is eligible as a leaf only if
 * best_cost[c] != MIP_COST_UNAVAILABLE and it lies wholly inside the frame (x + w <= W,
 * y + h <= H in frame coordinates): CUs right of the frame, whose costs come from wrapped
 * samples, are never leaves.  The penalty is the caller's rate term, lambda * bits of a leaf of
 * that shape; with zero penalties the sum of distortions favours small blocks.
 *
 * Regions.  A region whose top-left sample is outside the frame (x >= W or y >= H) costs 0 and
 * has no leaves.  Any other region that is not an eligible CU must split, or is infinite.
 * Quad-tree nodes are the aligned squares of side 128, 64, 32, 16, 8 reached by quad splits
 * only: 128 is never a leaf; 64 may be a leaf (the 64x64 CU) or quad-split; a node of side <= 32
 * is also the root of a binary/ternary subtree at depth 0; a node of side >= 16 may quad-split
 * into four nodes of half the side.  A binary/ternary state (rectangle, d), d in 0..3, is a leaf
 * if eligible and, if d < 3, may split into children at depth d + 1:
 *     BT-H  top and bottom halves           needs h >= 8
 *     BT-V  left and right halves           needs w >= 8
 *     TT-H  h/4, h/2, h/4 stacked           needs h >= 16
 *     TT-V  w/4, w/2, w/4 side by side      needs w >= 16
 * No quad split happens below a binary/ternary split.  VVC's redundant-split bans (e.g. a
 * binary split of a ternary split's middle part in the same direction) are NOT modelled.
 *
 * The cost of a split is the sum of its children's best costs, infinite if any child is infinite
 * (infinity is a state of its own, never reached through overflow).  Candidates are taken in
 * the order leaf, BT-H, BT-V, TT-H, TT-V, QT; a later one replaces the current one only if it
 * is strictly cheaper.  Sums are int32: for costs the search produces (<= 2*w*h*1023) and
 * penalties <= 1<<20 a CTU's total is below 1.11e9; larger input costs give an unspecified
 * result (memory-safe and deterministic).  A CTU whose root is infinite has no partition: its
 * ctu_cost is MIP_COST_UNAVAILABLE and it has no leaves.
 *
 * Outputs (device pointers, each optional, at least one given; asynchronous on `stream`, no
 * engine needed):
 *   d_leaf        uint8 [nframes][nCTUs*5380]: 1 where the CU is a leaf of the chosen partition,
 *                 else 0; every byte is written.
 *   d_ctu_cost, d_ctu_leaves   int32 [nframes][nCTUs].
 *   d_items       mip_pred_item [nframes][nCTUs][MIP_PART_MAX_LEAVES] (8-byte aligned; needs
 *                 d_best_mode): the first ctu_leaves entries of a CTU are its leaves in
 *                 increasing CU index, {frame, cu = ctu*5380 + k, mode = best_mode[cu], pitch = W,
 *                 offset = frame*W*H + y*W + x} (MIP_PRED_FRAME); the others are {-1, -1, -1, 0, 0},
 *                 which mip_predict_device skips and counts.  The whole array is a valid device
 *                 list: passed to mip_predict_device it gives the predicted frames with no host
 *                 round trip. */
#define MIP_PART_MAX_LEAVES 1024   /* 4x4 tiling of a CTU */
int mip_partition_device(const int32_t *d_best_cost, const uint8_t *d_best_mode, int width, int height,
                         int nframes, const int32_t *penalty, uint8_t *d_leaf, int32_t *d_ctu_cost,
                         int32_t *d_ctu_leaves, mip_pred_item *d_items, void *stream);

/* Decisions and partition of host frames, synchronous like mip_predict_frames (it first waits
 * for every call in flight; an open merged chunk is launched): in chunks of at most max_batch
 * frames -- upload, filter if the engine has one and no references are given, decisions-only
 * search, partition, download.  Needs opts.best_k <= 1.  best_mode_out / best_cost_out:
 * [nframes][nCTUs*5380]; leaf_out, ctu_cost_out, ctu_leaves_out as d_leaf, d_ctu_cost,
 * d_ctu_leaves above.  Every output is optional, at least one must be given. */
int mip_partition_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                         const int32_t *penalty, uint8_t *best_mode_out, int32_t *best_cost_out,
                         uint8_t *leaf_out, int32_t *ctu_cost_out, int32_t *ctu_leaves_out);

/* Planar / DC baseline costs and the MIP-vs-regular decision merge (additive to ABI 7; no
 * reference counterpart -- the reference ranks MIP modes only).  VTM keeps MIP modes in one
 * candidate list with the regular intra modes and ranks them by the same min(2*SAD, SATD);
 * Planar and DC are the regular modes it always tries.  mip_intra_device gives every CU those
 * two costs with the engine's own measure, so that "where does MIP win" and a partition that is
 * not MIP-only need no host round trip.
 *
 * Definition, for the CU at frame position (x, y) of size w x h (lw = log2 w, lh = log2 h).  R
 * is the reference frame with the source rule of mip_predict_device (d_refs NULL: the originals,
 * or the engine's filter applied into engine scratch, nframes <= max_batch then; otherwise the
 * caller's frames), F the original frame; both are read by linear index.
 *
 * Reference samples.  top[0..w) and left[0..h) are exactly the complete boundaries of the MIP
 * path: top[i] = R[(y-1)*W + x+i], or on the first frame row R[x-1] (512 at x = 0); left[j] =
 * R[(y+j)*W + x-1], or in the first frame column R[(y-1)*W] (512 at y = 0).  Above-right and
 * below-left samples are treated as unavailable (their causal availability depends on the
 * partition, which is not known here) and take VVC's substitution: topRight = top[w-1],
 * bottomLeft = left[h-1].  The corner sample is never read.  So a CU reads no sample that its
 * MIP search does not read, and the availability set is the search's: mip_unavailable_cus(width,
 * height, filter), or the MIP_FILTER_NONE set with caller references.
 *
 * Planar (mode slot 0), sample (i, j):
 *     predV = ((h-1-j)*top[i] + (j+1)*bottomLeft) << lw
 *     predH = ((w-1-i)*left[j] + (i+1)*topRight) << lh
 *     P     = (predV + predH + w*h) >> (lw + lh + 1)
 * DC (mode slot 1), every sample:
 *     w == h: P = (sum top + sum left + w) >> (lw+1)
 *     w >  h: P = (sum top + (w>>1)) >> lw          h > w: P = (sum left + (h>>1)) >> lh
 * PDPC, both modes:
 *     scale = (lw + lh - 2) >> 2
 *     sT = (2*j) >> scale, wT = sT <= 5 ? 32 >> sT : 0;  sL = (2*i) >> scale, wL likewise
 *     out = clip(0, 1023, (left[j]*wL + top[i]*wT + (64 - wL - wT)*P + 32) >> 6)
 * in 32-bit arithmetic throughout (engine-filtered references exceed 10 bits in the last columns
 * at widths that are not multiples of 128; that is the only way the clip can fire).
 *
 * NOT modelled: VVC's [1 2 1] smoothing of Planar's reference samples for blocks of more than 32
 * samples (it needs the corner and samples beyond w and h), multi-reference lines and ISP.  The
 * angular modes have their own entry point, mip_angular_device below.
 *
 * Cost.  SAD and SATD of `out` against the CU's originals F[(y+j)*W + x+i] (CUs right of the
 * frame wrap as in the cost tables), SATD the engine's: the 4x4 Hadamard per 4x4 block with the
 * DC term >> 2 and (s + 1) >> 1 per block.  cost = min(2*SAD, SATD).
 *
 * Tables (device pointers, 8-byte aligned, each optional): d_cost, d_sad, d_satd are int32
 * [nframes][nCTUs*5380][2] in the CU order of best_mode_out (ctu*5380 + shape CU prefix + cu),
 * slot 0 Planar, slot 1 DC.  Every entry of a given table is written; unavailable CUs get
 * MIP_COST_UNAVAILABLE in all three.
 *
 * Merge (optional; d_best_mode and d_best_cost are given together).  On entry d_best_mode /
 * d_best_cost [nframes][nCTUs*5380] hold the K = 1 MIP decisions of mip_search_device or
 * mip_topk_device.  bias is a HOST array of two int32 in 0 .. 1<<20 (NULL = zeros; anything else
 * is an error before any launch): the caller's rate difference for signalling Planar / DC instead
 * of a MIP mode.  Candidates are taken in the order MIP, Planar, DC; a later one replaces the
 * current one only if cost + bias is strictly lower, and then writes mode MIP_MODE_PLANAR or
 * MIP_MODE_DC and the biased cost.  Unavailable CUs (MIP_COST_UNAVAILABLE, mode 0xff) stay as
 * they are.  Both mode constants are >= 2*modes of every shape, so mip_predict_device skips and
 * counts such items under its write rule; mip_predict_device_ex with MIP_PRED_REGULAR emits their
 * Planar / DC blocks.  The merged arrays feed mip_partition_device unchanged.
 *
 * At least one table or the merge pair must be given.  Asynchronous on `stream`; argument errors
 * are reported before any launch. */
#define MIP_MODE_PLANAR 0xf0
#define MIP_MODE_DC 0xf1
int mip_intra_device(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes,
                     int32_t *d_cost, int32_t *d_sad, int32_t *d_satd, const int32_t *bias,
                     uint8_t *d_best_mode, int32_t *d_best_cost, void *stream);

/* The tables of host frames, synchronous like mip_predict_frames (it first waits for every call
 * in flight; an open merged chunk is launched): in chunks of at most max_batch frames -- upload,
 * filter if the engine has one and no references are given, kernel, download (no pipelining).
 * cost_out / sad_out / satd_out: int32 [nframes][nCTUs*5380][2], each optional, at least one. */
int mip_intra_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                     int32_t *cost_out, int32_t *sad_out, int32_t *satd_out);

/* Directional (angular) intra costs and their merge into the decisions (additive to ABI 7; no
 * reference counterpart).  The angular modes 2..66 are 65 of VVC's 67 regular intra modes; VTM
 * ranks them in the same candidate list as Planar, DC and the MIP modes by the same
 * min(2*SAD, SATD).  mip_angular_device gives every CU the cost of each mode of a caller's list
 * with the engine's own measure, the best of them, and merges that into the decisions.
 *
 * Mode codes.  MIP_MODE_ANGULAR(m) = 0x80 + m (0x82 .. 0xc2) is the best_mode value of angular
 * mode m.  Every such code is >= 2*modes of every shape and is neither MIP_MODE_PLANAR nor
 * MIP_MODE_DC, so mip_predict_device, and mip_predict_device_ex without MIP_PRED_ANGULAR, skip
 * and count such items under the write rule; mip_predict_device_ex with MIP_PRED_ANGULAR emits
 * their blocks -- the `out` of the predictor below -- so that the device list of
 * mip_partition_device on decisions merged here predicts whole frames with both flag bits.
 *
 * Definition, for the w x h CU at frame position (x, y), lw = log2 w, lh = log2 h.  R, F and
 * the reference source rule are exactly those of mip_intra_device.
 *
 * Reference samples.  top[0..w) and left[0..h) are the MIP path's complete boundaries as under
 * mip_intra_device.  The corner is one more sample: corner = R[(y-1)*W + x-1] if x > 0 and
 * y > 0, else top[0] (that is R[(y-1)*W] in the first frame column, R[x-1] in the first frame
 * row and 512 at (0, 0): the substitution the boundaries already make).  Above-right and
 * below-left samples stay unavailable, with VVC's substitution as in Planar: every sample past
 * top[w-1] equals top[w-1], every sample past left[h-1] equals left[h-1].
 *
 * Availability.  The corner's linear index is non-negative and below the indexes the search
 * already reads, and no otherwise-available CU has its corner among the samples an engine filter
 * leaves undefined, so the set is unchanged: mip_unavailable_cus(width, height, filter), or the
 * MIP_FILTER_NONE set with caller references.
 *
 * Angle A(m) of mode m:
 *     m =  2..18:   32  29  26  23  20  18  16  14  12  10   8   6   4   3   2   1   0
 *     m = 19..34:   -1  -2  -3  -4  -6  -8 -10 -12 -14 -16 -18 -20 -23 -26 -29 -32
 *     m = 35..50:  -29 -26 -23 -20 -18 -16 -14 -12 -10  -8  -6  -4  -3  -2  -1   0
 *     m = 51..66:    1   2   3   4   6   8  10  12  14  16  18  20  23  26  29  32
 * inv(A) = round(16384 / |A|) for A != 0:
 *     |A|   1     2    3    4    6    8   10   12   14   16  18  20  23  26  29  32
 *     inv 16384 8192 5461 4096 2731 2048 1638 1365 1170 1024 910 819 712 630 565 512
 *
 * Predictor.  Modes m >= 34 are the vertical class: main = top (length M = w), side = left
 * (length S = h), (a, b) = (i, j).  Modes m < 34 are the horizontal class, the same computation
 * transposed: main = left (M = h), side = top (S = w), (a, b) = (j, i).  The extended reference:
 *     ref[0]  = corner
 *     ref[k]  = main[min(k, M) - 1]                         k >= 1
 *     ref[-k] = side'[min((k*inv + 256) >> 9, S)]           k >= 1 (reached only with A < 0),
 *               side'[0] = corner, side'[t] = side[t-1]
 * Sample (i, j), with d = (b+1)*A, idx = d >> 5 (arithmetic shift), f = d & 31:
 *     P = f ? ((32 - f)*ref[a + idx + 1] + f*ref[a + idx + 2] + 16) >> 5 : ref[a + idx + 1]
 * PDPC applies to the two pure modes only, with the weight of mip_intra_device (w(d) = 32 >> s
 * for s = (2*d) >> scale <= 5, else 0; scale = (lw + lh - 2) >> 2):
 *     m = 50: wL = w(i), wT = 0, refL = left[j] - corner + P
 *     m = 18: wT = w(j), wL = 0, refT = top[i] - corner + P
 *     P' = (refL*wL + refT*wT + (64 - wL - wT)*P + 32) >> 6
 * For every mode out = clip(0, 1023, P or P'), in 32-bit arithmetic throughout (engine-filtered
 * references can exceed 10 bits).
 *
 * NOT modelled: wide-angle remapping for non-square blocks; PDPC of modes 2..17 and 51..66;
 * multi-reference lines and ISP; with mip_angular_refs(MIP_ANG_REFS_EXTENDED) availability below
 * binary / ternary splits is z-order (without it, the default, the above-right / below-left samples
 * are the substitutes above).  The 2-tap filter above is VVC's chroma filter and the default;
 * mip_angular_interp(MIP_ANG_INTERP_4TAP) replaces it by VVC's luma filters, with one difference:
 * VVC leaves the last sample of its 2M-long line unsmoothed, here the [1 2 1] smoothing of the
 * integer-slope modes runs over this engine's line with its clamp.
 *
 * Cost.  Exactly mip_intra_device's: SAD and the engine's 4x4-Hadamard SATD of `out` against
 * F[(y+j)*W + x+i] (CUs right of the frame wrap as in the cost tables), cost = min(2*SAD, SATD).
 *
 * modes / nmodes: a HOST list of VVC mode numbers, strictly increasing, each in 2..66, nmodes in
 * 1..65; NULL with nmodes == 0 means all 65.  Anything else is an error before any launch.  (A
 * caller's first pass would usually be the 33 even modes.)
 *
 * Tables (device pointers, each optional): d_cost, d_sad, d_satd are int32
 * [nframes][nCTUs*5380][65], slot m - 2 for mode m.  Every entry of a given table is written:
 * slots of modes not in the list, and all slots of unavailable CUs, are MIP_COST_UNAVAILABLE.
 * 4-byte alignment is enough (65 is odd: there is no 8-byte demand here).
 *
 * Best angular mode (optional; d_ang_mode and d_ang_cost are given together), uint8 / int32
 * [nframes][nCTUs*5380]: the lowest cost over the list, ties to the lower mode number, as the
 * MIP_MODE_ANGULAR code and the unbiased cost; 0xff / MIP_COST_UNAVAILABLE for unavailable CUs.
 *
 * Merge (optional; d_best_mode and d_best_cost are given together).  On entry they hold the
 * K = 1 decisions -- MIP, or already merged by mip_intra_device.  The decision is replaced by the
 * best angular mode of the list only if ang_cost + bias is strictly lower; it then holds the
 * MIP_MODE_ANGULAR code and the biased cost.  bias is in 0 .. 1<<20, else an error before any
 * launch.  CUs whose best_cost is MIP_COST_UNAVAILABLE, and unavailable CUs, stay as they are.
 * The merged arrays feed mip_partition_device unchanged.
 *
 * At least one table, the ang pair or the merge pair must be given.  Asynchronous on `stream`;
 * reference source, the nframes <= max_batch rule with an engine filter, and the ordering on the
 * engine's filter scratch are those of mip_intra_device.  Argument errors are reported before
 * any launch. */
#define MIP_ANGULAR_FIRST 2
#define MIP_ANGULAR_LAST  66
#define MIP_ANGULAR_MODES 65          /* table slot = m - 2 */
#define MIP_MODE_ANGULAR(m) (0x80 + (m))   /* 0x82 .. 0xc2 */
int mip_angular_device(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes,
                       const uint8_t *modes, int nmodes,
                       int32_t *d_cost, int32_t *d_sad, int32_t *d_satd,
                       uint8_t *d_ang_mode, int32_t *d_ang_cost,
                       int32_t bias, uint8_t *d_best_mode, int32_t *d_best_cost, void *stream);

/* The best angular modes and, optionally, the cost table of host frames, synchronous like
 * mip_intra_frames (it first waits for every call in flight; an open merged chunk is launched):
 * upload, filter if the engine has one and no references are given, kernel, download, in chunks
 * of at most max_batch frames.  cost_out: int32 [nframes][nCTUs*5380][65]; ang_mode_out /
 * ang_cost_out (given together): [nframes][nCTUs*5380]; at least one output.  The table is
 * 1.4 MB per CTU (about 189 MB per 1080p frame), so with cost_out the chunk is further cut so
 * that the call's device table stays within 256 MiB (always at least one frame).  Results do not
 * depend on the chunking. */
int mip_angular_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                       const uint8_t *modes, int nmodes,
                       int32_t *cost_out, uint8_t *ang_mode_out, int32_t *ang_cost_out);

/* Coarse-to-fine angular mode search in one launch (additive to ABI 7; no reference counterpart):
 * every CU ranks the caller's list, then also evaluates the +-1 neighbours of its own best few
 * modes -- the second pass of an encoder's mode search, per CU, on the windows the first pass
 * staged.  Everything not said here is mip_angular_device's, word for word: reference source,
 * corner, availability set, predictor, cost, list rules, bias range, table layout, merge rule, the
 * "at least one output" rule (d_ang_tried counts as an output), asynchrony, and argument errors
 * reported before any launch.
 *
 * seeds is in 1 .. MIP_ANGULAR_MAX_SEEDS, anything else is an error before any launch.  For every
 * available CU, with L the caller's list:
 *   Seeds.       The min(seeds, nmodes) modes of L with the lowest cost, ties to the lower mode
 *                number: the first entries of L sorted by (cost, mode).
 *   Candidates.  C = { s - 1, s + 1 : s a seed } within [2, 66] and not in L, as a set: no wrap
 *                between 2 and 66, a neighbour reached from two seeds counts once.
 *   Evaluated.   E = L u C.  The ang pair is the minimum of (cost, mode) over E, as the
 *                MIP_MODE_ANGULAR code and the unbiased cost; the merge uses that pair exactly as
 *                mip_angular_device merges its own.
 *   Tables.      For this CU the slots of E hold their values, every other slot
 *                MIP_COST_UNAVAILABLE.  Unavailable CUs are MIP_COST_UNAVAILABLE in every slot.
 *   d_ang_tried  (optional) uint8 [nframes][nCTUs*5380]: |E|, and 0 for unavailable CUs -- how
 *                many modes were evaluated per CU, without downloading a table.
 * Consequences: with all 65 modes listed C is empty and every output equals mip_angular_device's
 * (d_ang_tried is 65); the refined cost is never above the list's best and never below the
 * 65-mode best. */
#define MIP_ANGULAR_MAX_SEEDS 3
int mip_angular_refine_device(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs, int nframes,
                              const uint8_t *modes, int nmodes, int seeds,
                              int32_t *d_cost, int32_t *d_sad, int32_t *d_satd,
                              uint8_t *d_ang_mode, int32_t *d_ang_cost, uint8_t *d_ang_tried,
                              int32_t bias, uint8_t *d_best_mode, int32_t *d_best_cost, void *stream);

/* mip_angular_refine_device on host frames, synchronous and chunked like mip_angular_frames (the
 * same 256 MiB cut of the device table with cost_out).  tried_out: uint8 [nframes][nCTUs*5380],
 * optional; ang_mode_out / ang_cost_out given together; at least one output.  Results do not
 * depend on the chunking. */
int mip_angular_refine_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                              const uint8_t *modes, int nmodes, int seeds,
                              int32_t *cost_out, uint8_t *ang_mode_out, int32_t *ang_cost_out, uint8_t *tried_out);

/* Real above-right and below-left reference samples for the angular family (additive to ABI 7; no
 * reference counterpart).  An engine-level switch: with MIP_ANG_REFS_EXTENDED every angular entry
 * point of that engine -- mip_angular_device / _frames, mip_angular_refine_device / _frames, the
 * MIP_PRED_ANGULAR items of mip_predict_device_ex / mip_predict_frames_ex, mip_predicted_frames_ex
 * with MIP_CHAIN_ANGULAR and mip_candidates_frames with MIP_CAND_ANGULAR -- extends the two reference
 * lines by the real samples past top[w-1] and left[h-1] where they exist and precede the CU in coding
 * order.  The default, MIP_ANG_REFS_SUBSTITUTED, is the contract of mip_angular_device as written
 * above, unchanged.  MIP, Planar / DC, the partition and mip_candidates_device do not look at the
 * switch.  The setting is read when a call builds its launch: work already enqueued keeps the
 * setting it was enqueued with, no synchronisation is needed, and the cost kernels and the block
 * output of one engine always agree (the SAD / SATD of an emitted block are the table entries).
 *
 * The engine predicts from original (or filtered) samples, not from reconstructed ones, so the real
 * samples exist whenever they lie inside the frame; only their causal order is modelled.
 *
 * Everything of mip_angular_device stays word for word, except the lengths of the two lines.
 *
 * Order key.  The key of the sample at frame position (sx, sy) is the pair (raster index of the CTU
 * that holds it, Morton code of ((sx % 128) >> 2, (sy % 128) >> 2) with x in the even bits and y in
 * the odd bits), compared lexicographically: z-scan order of 4x4 blocks inside CTU raster order.
 * This is THE MODEL: it is exact for quad-tree splits and an approximation below binary / ternary
 * splits.
 *
 * A CU that is unavailable, or not wholly inside the frame (x + w > W or y + h > H: the wrapped
 * CUs), has E_top = E_left = 0.
 *
 * Top line of any other CU: extended by E_top, the largest n in 0..h such that every t in
 * [w, w + n) meets all of: y > 0; x + t < W; key(x + t, y - 1) < key(x, y); with an engine filter,
 * R[(y-1)*W + x + t] is not among the samples the filter leaves undefined (with caller references
 * the MIP_FILTER_NONE set applies: none).  Then top[t] = R[(y-1)*W + x + t] for t in [w, w + E_top).
 *
 * Left line: extended by E_left, the largest n in 0..w such that every t in [h, h + n) meets all of:
 * x > 0; y + t < H; key(x - 1, y + t) < key(x, y); the same undefined-sample condition on
 * R[(y+t)*W + x - 1].  Then left[t] = R[(y+t)*W + x - 1] for t in [h, h + E_left).
 *
 * Predictor.  The main line has length M' = M + E(main) (E_top in the vertical class, E_left in the
 * horizontal one): ref[k] = main[min(k, M') - 1] for k >= 1.  The side projection keeps its cap S:
 * negative angles never reach past the side's end.  PDPC of modes 18 and 50, the corner, the clip,
 * SAD / SATD / cost, the tables, the ang pair, the merge and `tried` are unchanged.
 *
 * Consequences: every output of modes 18..50 equals the substituted one; so does every output of a
 * CU with E_top = E_left = 0; a CU with E_top = h predicts mode 66 as top[i + j + 1] exactly.
 *
 * mip_angular_refs: 0, or <0 for a NULL engine ("engine is NULL") or a value other than the two
 * below.  mip_angular_refs_get: the current setting, <0 for NULL.
 * mip_extended_refs (host only, like mip_unavailable_cus): per CU [nCTUs*5380] the number of real
 * samples that extend its top line (0..h) and its left line (0..w) under the rule above, with the
 * availability / undefined-sample set of `filter`.  Either output may be NULL, not both. */
#define MIP_ANG_REFS_SUBSTITUTED 0   /* default: the lines of mip_angular_device */
#define MIP_ANG_REFS_EXTENDED    1
int mip_angular_refs(mip_engine *e, int refs);
int mip_angular_refs_get(const mip_engine *e);
int mip_extended_refs(int width, int height, int filter, uint8_t *top_out, uint8_t *left_out);

/* VVC's 4-tap cubic / Gaussian luma interpolation for the angular family (additive to ABI 7; no
 * reference counterpart).  An engine-level switch in the shape of mip_angular_refs: with
 * MIP_ANG_INTERP_4TAP every angular entry point of that engine -- the list of mip_angular_refs above
 * -- predicts with VVC's luma filters.  The default, MIP_ANG_INTERP_2TAP, is the predictor of
 * mip_angular_device as written above, unchanged.  MIP, Planar / DC, the partition and
 * mip_candidates_device do not look at the switch.  The setting is read when a call builds its
 * launch, next to the mip_angular_refs setting and under the same rules: work already enqueued keeps
 * the setting it was enqueued with, and the cost kernels and the block output of one engine always
 * agree.  The two switches are independent: all four combinations are defined.
 *
 * Everything of mip_angular_device and of mip_angular_refs stays word for word, except the line
 * P = ... of the predictor: the reference source, the corner, ref[k] with its clamps, the extended
 * length M' under MIP_ANG_REFS_EXTENDED, the side projection and its cap S, PDPC of modes 18 and 50,
 * the clip, SAD / SATD / cost, the tables, the ang pair, the merge, `tried`, the list and bias rules.
 *
 * With MIP_ANG_INTERP_4TAP, for sample (i, j) of a CU with w = 1 << lw, h = 1 << lh and mode m, take
 * d, idx, f and k = a + idx + 1 as above:
 *     G = min(|m - 50|, |m - 18|) > T[(lw + lh) >> 1],   T[0..6] = {24, 24, 24, 14, 2, 0, 0}
 *     c = G ? fG[f] : fC[f]
 *     P = (c[0]*ref[k-1] + c[1]*ref[k] + c[2]*ref[k+1] + c[3]*ref[k+2] + 32) >> 6
 * The sum can be negative: the shift is arithmetic and the arithmetic 32-bit throughout.  The same
 * expression applies for every f, f = 0 included.  ref[] is the class's reference exactly as the
 * engine's mip_angular_refs setting resolves it (ref[k] = main[min(k, M') - 1] for k >= 1, the side
 * projection for k < 0); ref[0] is the corner, also for A >= 0, where the 2-tap predictor never
 * reads it.
 *
 * fG[f] = {16 - (f>>1), 32 - (f>>1), 16 + (f>>1), f>>1}; fG[0] = {16, 32, 16, 0} is VVC's [1 2 1]
 * reference smoothing of the integer-slope modes.  fC[f] for f = 0..16:
 *     { 0,64, 0, 0} {-1,63, 2, 0} {-2,62, 4, 0} {-2,60, 7,-1} {-2,58,10,-2} {-3,57,12,-2}
 *     {-4,56,14,-2} {-4,55,15,-2} {-4,54,16,-2} {-5,53,18,-2} {-6,52,20,-2} {-6,49,24,-3}
 *     {-6,46,28,-4} {-5,44,29,-4} {-4,42,30,-4} {-4,39,33,-4} {-4,36,36,-4}
 * and fC[32 - f] is fC[f] reversed.  fC[0] is the identity; every row of both tables sums to 64.
 * (VVC's intra luma filters and its intraHorVerDistThres; these tables are the contract.)
 *
 * Consequences: modes 18 and 50 equal the 2-tap outputs everywhere (f = 0 and G is false: the
 * identity); modes 2, 34 and 66 equal the 2-tap outputs on CUs with (lw + lh) >> 1 == 2 (4x4, 4x8,
 * 8x4; on every larger CU they are smoothed by fG[0]); a constant reference line predicts that
 * constant in every mode; a line that is v everywhere but v + 64 at one sample predicts v + c at the
 * samples whose window covers it, c the coefficient of the tap that lands on it (v in 6 .. 959: no
 * clip).
 * With MIP_ANG_REFS_EXTENDED the tap k+2 of a negative-angle mode reaches ref[M+1], the first sample
 * of the extension, so of the consequences listed under mip_angular_refs "modes 18..50 equal the
 * substituted outputs" holds for modes 18 and 50 only; a CU with E_top = E_left = 0 still equals its
 * substituted outputs in every mode.
 *
 * mip_angular_interp: 0, or <0 for a NULL engine ("engine is NULL") or a value other than the two
 * below.  mip_angular_interp_get: the current setting, <0 for NULL.
 * mip_angular_filter (host only): which table a w x h = (1 << lw) x (1 << lh) CU takes for `mode`
 * under MIP_ANG_INTERP_4TAP -- 0 the cubic fC, 1 the Gaussian fG (G above); <0 for lw or lh outside
 * 2..6 or a mode outside 2..66. */
#define MIP_ANG_INTERP_2TAP 0   /* default: the predictor of mip_angular_device as written */
#define MIP_ANG_INTERP_4TAP 1
int mip_angular_interp(mip_engine *e, int interp);
int mip_angular_interp_get(const mip_engine *e);
int mip_angular_filter(int lw, int lh, int mode);

/* The whole chain on host frames, synchronous like mip_partition_frames (it first waits for every
 * call in flight; an open merged chunk is launched): in chunks of at most max_batch frames --
 * upload, filter if the engine has one and no references are given, decisions-only search, the
 * merge of mip_intra_device with `bias` (NULL = zeros), mip_partition_device with `penalty`,
 * MIP_PRED_REGULAR prediction of the partition's own device list into frame canvases preset to
 * MIP_PRED_NONE, download.  Needs opts.best_k <= 1.  best_mode_out / best_cost_out (the merged
 * decisions), leaf_out, ctu_cost_out, ctu_leaves_out as in mip_partition_frames; pred_out: uint16
 * [nframes][H][W], the leaves' predicted samples at their place -- samples no leaf covers (CTUs
 * without a partition) stay MIP_PRED_NONE.  Every output is optional, at least one must be given.
 * A penalty or bias out of range is an error before any launch. */
int mip_predicted_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                         const int32_t *penalty, const int32_t *bias,
                         uint8_t *best_mode_out, int32_t *best_cost_out, uint8_t *leaf_out,
                         int32_t *ctu_cost_out, int32_t *ctu_leaves_out, uint16_t *pred_out);

/* The chain with an optional angular stage (additive to ABI 7).  flags == 0 is mip_predicted_frames
 * exactly (that entry point is the flags == 0 call of this one; ang_modes, ang_nmodes and ang_bias
 * are then not looked at).  Any bit other than MIP_CHAIN_ANGULAR is an error before any launch.
 *
 * MIP_CHAIN_ANGULAR: per chunk -- decisions-only search, the merge of mip_intra_device with `bias`,
 * the merge of mip_angular_device over the list ang_modes / ang_nmodes with ang_bias (the merge
 * pair only, no tables), mip_partition_device with `penalty`, prediction of the partition's own
 * device list with MIP_PRED_REGULAR | MIP_PRED_ANGULAR.  The list and the bias follow
 * mip_angular_device's rules (NULL with 0: all 65 modes; bias in 0 .. 1<<20); a bad list or bias is
 * an error before any launch.  The outputs are mip_predicted_frames': best_mode_out / best_cost_out
 * hold the decisions after both merges, pred_out every leaf's MIP, Planar, DC or angular block. */
#define MIP_CHAIN_ANGULAR 1u   /* flags bit of mip_predicted_frames_ex: the angular stage is on */
int mip_predicted_frames_ex(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                            const int32_t *penalty, const int32_t *bias,
                            const uint8_t *ang_modes, int ang_nmodes, int32_t ang_bias, unsigned flags,
                            uint8_t *best_mode_out, int32_t *best_cost_out, uint8_t *leaf_out,
                            int32_t *ctu_cost_out, int32_t *ctu_leaves_out, uint16_t *pred_out);

/* K-best candidate lists over every mode family (additive to ABI 7; no reference counterpart):
 * for every CU the k lowest-cost modes among its MIP modes, Planar, DC and the angular modes, in
 * one list -- what an encoder's rough mode decision hands to full RD (VTM takes two or three per
 * block, MIP and regular modes together).  mip_candidates_device merges the families' per-CU
 * costs, which the other entry points leave in device memory; no table goes to the host.  No
 * engine is needed.  Asynchronous on `stream`.  Argument errors are reported before any launch
 * and nothing is written.
 *
 * CUs are indexed as in best_mode_out: [nframes][nCTUs*5380].  Each family is optional (a NULL
 * pointer: not given), at least one must be given.
 *
 * MIP.  d_mip_mode / d_mip_cost (given together): uint8 / int32 [nframes][nCTUs*5380][kin], kin in
 *   1..32 (kin is not looked at without them) -- the decision lists of mip_search_device on an
 *   engine with best_k = kin, or of mip_topk_device.  Entry r of a CU is a candidate iff
 *   mode <= 31 and cost != MIP_COST_UNAVAILABLE; its code is the mode, its value the cost.  Any
 *   other entry (0xff, a mode above 31, MIP_COST_UNAVAILABLE) is simply absent.  The list is
 *   data: no entry ever moves an address.
 * Planar / DC.  d_intra_cost: int32 [nframes][nCTUs*5380][2], the d_cost table of
 *   mip_intra_device.  A slot that is not MIP_COST_UNAVAILABLE is a candidate; its code is
 *   MIP_MODE_PLANAR (slot 0) / MIP_MODE_DC (slot 1), its value cost + intra_bias[slot].
 *   intra_bias is a HOST array of two int32 in 0 .. 1<<20, NULL = zeros (checked only with
 *   d_intra_cost).
 * Angular.  d_ang_cost: int32 [nframes][nCTUs*5380][65], the d_cost table of mip_angular_device
 *   or mip_angular_refine_device.  Every slot that is not MIP_COST_UNAVAILABLE is a candidate;
 *   its code is MIP_MODE_ANGULAR(slot + 2), its value cost + ang_bias, ang_bias in 0 .. 1<<20
 *   (checked only with d_ang_cost).  Slots of modes that were not listed or not evaluated drop
 *   out by themselves: a refined table contributes exactly the CU's set E.
 * int32 arrays need 4-byte alignment only.
 *
 * Order.  The candidates of a CU are sorted by (value, rank), lowest first.  The rank of MIP mode
 * v is v (0..31), of Planar 32, of DC 33, of angular mode m 32 + m (34..98).  This is the order
 * of the existing merges -- MIP, Planar, DC, angular; the lower mode first inside a family; a
 * later candidate wins only if strictly cheaper -- so with the same biases entry 0 is, bit for
 * bit, the decision that the search's argmin, mip_intra_device's merge and
 * mip_angular_device's / mip_angular_refine_device's merge leave.
 *
 * Outputs.  d_modes uint8 and d_costs int32, [nframes][nCTUs*5380][k], k in 1..MIP_CAND_MAX_K;
 * either may be NULL, not both.  No output may overlap an input or the other output (an error
 * before any launch).  The first min(k, number of candidates) entries of a CU are the sorted
 * candidates' codes and values (biased, as the merges write them); every later entry is 0xff /
 * MIP_COST_UNAVAILABLE.  Every entry of a given output is written.  A CU without a candidate is
 * 0xff / MIP_COST_UNAVAILABLE throughout (an unavailable CU is MIP_COST_UNAVAILABLE in every
 * family).
 *
 * Domain.  Costs the engine produces are at most 2*64*64*1023 = 8 380 416, so cost plus bias stays
 * below 1<<24.  A table or list value other than MIP_COST_UNAVAILABLE outside
 * 0 .. (1<<24) - 1 - (1<<20), or a MIP list that names a mode twice, gives an unspecified result:
 * memory-safe (every code written is still one of the 99 codes or 0xff) and deterministic. */
#define MIP_CAND_MAX_K 32
int mip_candidates_device(int width, int height, int nframes, int k,
                          const uint8_t *d_mip_mode, const int32_t *d_mip_cost, int kin,
                          const int32_t *d_intra_cost, const int32_t *intra_bias,
                          const int32_t *d_ang_cost, int32_t ang_bias,
                          uint8_t *d_modes, int32_t *d_costs, void *stream);

/* The candidate lists of host frames, synchronous like mip_partition_frames (it first waits for
 * every call in flight; an open merged chunk is launched).  Per chunk: upload; filter, if the
 * engine has one and no references are given; the search, with MIP lists of length min(k, 32)
 * whatever opts.best_k is; with MIP_CAND_REGULAR the Planar / DC table of mip_intra_device; with
 * MIP_CAND_ANGULAR the angular table over the list ang_modes / ang_nmodes (mip_angular_device's
 * rules: NULL with 0 = all 65) -- ang_seeds == 0 runs mip_angular_device, 1 ..
 * MIP_ANGULAR_MAX_SEEDS mip_angular_refine_device with that many seeds; then
 * mip_candidates_device over the families that ran, with intra_bias (NULL = zeros) and ang_bias;
 * download.  flags == 0 gives the MIP lists alone.  Without MIP_CAND_ANGULAR the angular
 * arguments are not looked at, without MIP_CAND_REGULAR intra_bias is not.  Any other flag bit, a
 * bad list, bias, seeds or k is an error before any launch.
 * modes_out uint8 / costs_out int32: [nframes][nCTUs*5380][k], either may be NULL, not both.
 * Chunks hold at most max_batch frames and are cut further, as in mip_angular_frames, so that the
 * chunk's device tables -- the MIP cost table (the search writes one unless k == 1 on an engine
 * with best_k <= 1), the Planar / DC table, the angular table -- stay within 256 MiB together,
 * always at least one frame.  Results do not depend on the chunking. */
#define MIP_CAND_REGULAR 1u   /* flags bit: Planar and DC are candidates */
#define MIP_CAND_ANGULAR 2u   /* flags bit: the angular modes of the list are candidates */
int mip_candidates_frames(mip_engine *e, const uint16_t *frames, const uint16_t *refs_or_null, int nframes,
                          int k, unsigned flags, const int32_t *intra_bias,
                          const uint8_t *ang_modes, int ang_nmodes, int ang_seeds, int32_t ang_bias,
                          uint8_t *modes_out, int32_t *costs_out);

/* Streaming device-to-device copy of `bytes` (a multiple of 16, 16-byte aligned pointers),
 * asynchronous on `stream`: 16 bytes per lane, four loads in flight per lane -- the HBM copy
 * rate bench.py prices the filter kernel against (no reference counterpart). */
int mip_copy_device(const void *d_src, void *d_dst, size_t bytes, void *stream);

/* Device-resident filter (asynchronous on `stream`). */
int mip_filter_device(const uint16_t *d_in, uint16_t *d_out, int width, int height,
                      int nframes, int filter, int kernel_idx, void *stream);

/* Kernel-only timing of the search on resident buffers: runs `reps` launches of the
 * fused search for `nframes` device frames on the engine's own stream, returns the mean
 * device time per launch in milliseconds (HIP events on that stream), or <0. */
double mip_time_search_device(mip_engine *e, const uint16_t *d_frames, const uint16_t *d_refs,
                              int nframes, int32_t *d_costs, int reps);

/* Per-frame device times of the host pipeline, for the reference's stdout report
 * ("FilterSamples took %f ms" and the filter TIMING REPORT, main.cpp:749-775; the frame
 * write time, main.cpp:580-595).  mip_trace_times(e, 1): mip_search_frames[_async] brackets
 * every chunk's upload and filter launch with HIP timing events (a buffer slot is then reused
 * only after its times were read: tracing costs some overlap).  mip_pop_times returns the
 * per-frame times (the chunk's time / its frames, frame order) of the calls completed so
 * far: up to `max` frames into upload_ms / filter_ms (either may be NULL; filter 0 without
 * a filter), the count in *n. */
int mip_trace_times(mip_engine *e, int enable);
int mip_pop_times(mip_engine *e, double *upload_ms, double *filter_ms, int max, int *n);

/* Host-pipeline counters of the engine (diagnostics, tests): out[0] host-API calls, out[1]
 * search launches of the host pipeline (chunks), out[2] calls that went through merged
 * chunks, out[3] merged launches (n entries of out are written, n <= 4). */
int mip_host_stats(mip_engine *e, uint64_t *out, int n);

/* Search-launch census of the engine (diagnostics, tests; additive to ABI 7): which instance
 * of the search kernel every search launch of the engine ran -- host pipeline chunks, device-API
 * searches and mip_time_search_device alike -- counted since the engine was created.
 *   out[8*w + 4*alt + 2*dec + pf]  launches of the instance with
 *       w    0: 12-wave workgroups, 1: 16-wave ("wide", small launches), 2: 8-wave (the
 *            four-wave twin of the host pipeline),
 *       alt  1: alternative (filtered or caller-supplied) references,
 *       dec  1: decisions only (no cost table),
 *       pf   1: the instance that prefetches the next item's window (as launched, not as asked);
 *   out[MIP_CENSUS_PAIR]     launches in pair mode (16-wave workgroups taking two items at once),
 *   out[MIP_CENSUS_CHUNKED]  launches whose item queue was cut into per-XCD chunks,
 *   out[MIP_CENSUS_ORDERED]  launches that took their items longest first (else raster order).
 * n entries of out are written, n <= MIP_CENSUS_ENTRIES.  Launches that failed are not counted. */
#define MIP_CENSUS_INSTANCES 24
#define MIP_CENSUS_PAIR 24
#define MIP_CENSUS_CHUNKED 25
#define MIP_CENSUS_ORDERED 26
#define MIP_CENSUS_ENTRIES 27
int mip_search_census(mip_engine *e, uint64_t *out, int n);

/* Page-locked host memory (hipHostMalloc): host buffers for mip_search_frames /
 * mip_filter_frames allocated here are transferred by DMA at full PCIe rate (pageable
 * buffers are staged through the runtime -- the cost table is 52.8 MB per 1080p frame).
 * Replaces the reference's malloc'd return_minSadHad etc. (main.cpp:656-668). */
int mip_host_alloc(size_t bytes, void **out);
int mip_host_free(void *p);

/* NUMA placement (ABI 7).  Each GPU hangs off one socket of a multi-socket host; an engine
 * keeps its page-locked buffers on that GPU's NUMA node and runs its host threads (bounce-ring
 * copies, completion) on the node's CPUs.  mip_host_alloc_near allocates the
 * caller's page-locked buffers on `device`'s node (else as mip_host_alloc);
 * mip_bind_thread runs the calling thread on the node's CPUs (1 bound, 0 nothing to do: one
 * node or unknown); mip_numa_node gives the node (-1 unknown / one node);
 * mip_numa_node_of_pci the node of a PCI bus id ("0000:c1:00.0"), read from sysfs
 * (MIPGPU_SYSFS_ROOT overrides /sys). */
int mip_host_alloc_near(int device, size_t bytes, void **out);
int mip_bind_thread(int device);
int mip_numa_node(int device);
int mip_numa_node_of_pci(const char *pci_bus_id);

/* Last error message of the calling thread ("" if none). */
const char *mip_last_error(void);
int mip_abi_version(void);
/* Build ID of this library: "src:<hash of the sources and compiler flags> git:<commit>"
 * (+ "knobs:<-D options>" for A/B variants).  bench.py prints it and ties profiles/ to it. */
const char *mip_build_id(void);

#ifdef __cplusplus
}
#endif
#endif

#!/usr/bin/env python3
"""Device time of the angular family with extended reference lines (mip_angular_refs,
MIP_ANG_REFS_EXTENDED) beside the substituted kernels, 1080p, resident buffers, original
references: the cost kernel (best + merge, all 65 modes and the 33 even modes), the refined search
(even list, two seeds) and the block output (every 8x8 CU inside the frame, one angular item each,
frame layout).  One process, one engine: the two settings alternate round by round, so both see
the same clocks; the yardstick of an extended kernel is its substituted sibling in the same round.
HIP events per launch, warm-up first, median of REPS launches per round.

It also records, on the synthetic frames of mipgpu.synth (kinds 0 and 1 -- synthetic content, not
video), the share of available CUs whose best angular cost differs between the settings, and in
which direction.  Writes the record (with mip_build_id()) to --out, default
profiles/angular_ext_rate.txt."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vvc-mip-gpu_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mipgpu  # noqa: E402
from mipgpu import MipEngine, layout  # noqa: E402
from mipgpu.synth import synth_frames_torch  # noqa: E402

W, H, B, REPS, WARMUP, ROUNDS = 1920, 1080, 48, 10, 2, 3
EVEN = tuple(range(2, 67, 2))
ITEM_MODES = (2, 66, 10, 58, 18, 50, 34, 17, 51)
SETTINGS = (("substituted", mipgpu.ANG_REFS_SUBSTITUTED), ("extended", mipgpu.ANG_REFS_EXTENDED))


def median_ms(fn, stream):
    for _ in range(WARMUP):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for e0, e1 in ev:
        e0.record(stream)
        fn()
        e1.record(stream)
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "angular_ext_rate.txt"))
    ap.add_argument("--frames", type=int, default=B)
    args = ap.parse_args()
    nf = args.frames
    dev = torch.device("cuda:0")
    frames = synth_frames_torch(W, H, nf, 0x1080, 0, device=dev)
    nct = layout.num_ctus(W, H)
    ncu = nct * layout.CUS_PER_CTU
    stream = torch.cuda.Stream()
    lines = ["angular family with extended reference lines, %dx%d x %d resident frames, original references," % (W, H, nf),
             "median of %d launches per round (HIP events), %d rounds, the two settings alternating in one process" % (REPS, ROUNDS),
             "build: " + mipgpu.build_id(), "device: " + torch.cuda.get_device_name(0), ""]
    best_mode = torch.empty((nf, ncu), dtype=torch.uint8, device=dev)
    best_cost = torch.empty((nf, ncu), dtype=torch.int32, device=dev)
    ang_mode = torch.empty((nf, ncu), dtype=torch.uint8, device=dev)
    ang_cost = torch.empty((nf, ncu), dtype=torch.int32, device=dev)
    tried = torch.empty((nf, ncu), dtype=torch.uint8, device=dev)
    # the block-output list: every available 8x8 CU wholly inside the frame, every frame
    un = mipgpu.unavailable_cus(W, H)
    shape, x, _, bw, _ = layout.cu_geometry(W, H, np.arange(ncu))
    cus = np.nonzero(~un & (shape == layout.SHAPE_BY_NAME["ALL_AL_8x8"].index) & (x + bw <= W))[0]
    cu = np.tile(cus, nf)
    frame_of = np.repeat(np.arange(nf), cus.size)
    mode = mipgpu.MODE_ANGULAR_BASE + np.array(ITEM_MODES)[np.arange(cu.size) % len(ITEM_MODES)]
    items, total = mipgpu.pred_items(W, H, frame_of, cu, mode, layout="frame", nframes=nf)
    d_items = torch.from_numpy(items.view(np.uint8).copy()).to(dev)
    canvas = torch.empty(total, dtype=torch.int16, device=dev)
    with MipEngine(W, H, max_batch=nf) as eng:
        stream.wait_stream(torch.cuda.current_stream(dev))
        eng.search_device(frames, costs=False, best_mode=best_mode, best_cost=best_cost, stream=stream)
        eng.check_input(stream)
        jobs = (("cost kernel, 65 modes, best + merge",
                 lambda: eng.angular_device(frames, ang_mode=ang_mode, ang_cost=ang_cost, best_mode=best_mode, best_cost=best_cost, stream=stream)),
                ("cost kernel, 33 even modes, best + merge",
                 lambda: eng.angular_device(frames, modes=EVEN, ang_mode=ang_mode, ang_cost=ang_cost, best_mode=best_mode, best_cost=best_cost,
                                            stream=stream)),
                ("refined search, even list, 2 seeds",
                 lambda: eng.angular_refine_device(frames, modes=EVEN, seeds=2, ang_mode=ang_mode, ang_cost=ang_cost, tried=tried,
                                                   best_mode=best_mode, best_cost=best_cost, stream=stream)),
                ("block output, %d items per frame" % cus.size,
                 lambda: eng.predict_device(frames, d_items, canvas, stream=stream, angular=True)))
        lines.append("%-44s %-8s %s   %s" % ("ms per frame", "round", "   ".join("%11s" % n for n, _ in SETTINGS), "extended / substituted"))
        for name, fn in jobs:
            ratios = []
            for r in range(ROUNDS):
                ms = []
                for _, value in SETTINGS:
                    eng.angular_refs = value
                    ms.append(median_ms(fn, stream) / nf)
                ratios.append(ms[1] / ms[0])
                lines.append("%-44s %-8d %s   %.3f" % (name, r, "   ".join("%11.4f" % v for v in ms), ratios[-1]))
            lines.append("%-44s %-8s %s   %.3f" % ("", "median", " " * (14 * len(SETTINGS) - 3), statistics.median(ratios)))
        # the decisions: synthetic frames only
        lines += ["", "best angular cost, all 65 modes, extended against substituted lines, SYNTHETIC frames (mipgpu.synth; not video):",
                  "%-8s %10s %10s %10s %12s" % ("kind", "changed", "lower", "higher", "mean change")]
        for kind in (0, 1):
            few = synth_frames_torch(W, H, 4, 0x1080 + kind, kind, device=dev)
            got = []
            for _, value in SETTINGS:
                eng.angular_refs = value
                c = torch.empty((4, ncu), dtype=torch.int32, device=dev)
                m = torch.empty((4, ncu), dtype=torch.uint8, device=dev)
                eng.angular_device(few, ang_mode=m, ang_cost=c, stream=stream)
                stream.synchronize()
                got.append(c.cpu().numpy().astype(np.int64))
            on = got[0] != layout.UNAVAILABLE
            sub, ext = got[0][on], got[1][on]
            lines.append("%-8d %9.1f%% %9.1f%% %9.1f%% %11.2f%%" % (kind, 100 * (ext != sub).mean(), 100 * (ext < sub).mean(),
                                                                 100 * (ext > sub).mean(), 100 * (ext.sum() - sub.sum()) / sub.sum()))
        eng.angular_refs = mipgpu.ANG_REFS_SUBSTITUTED
    lines += ["", "changed / lower / higher: share of the available CUs whose best angular cost over all 65 modes differs, falls, rises;",
              "mean change: the sum of those best costs, extended over substituted.  A real sample in place of a",
              "replicated one can predict a block worse as well as better: both directions occur on synthetic content,",
              "and nothing here says what the change is worth on video."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

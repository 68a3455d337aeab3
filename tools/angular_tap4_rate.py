#!/usr/bin/env python3
"""Device time of the angular family with VVC's 4-tap luma interpolation (mip_angular_interp,
MIP_ANG_INTERP_4TAP) beside the 2-tap kernels, 1080p, resident buffers, original references: the
cost kernel (best + merge, all 65 modes and the 33 even modes), the refined search (even list, one
seed, and two seeds as in profiles/angular_ext_rate.txt) and the block output (every 8x8 CU inside
the frame, one angular item each, frame layout), under both mip_angular_refs settings.  One process,
one engine: the two interpolation settings alternate round by round, so both see the same clocks;
the yardstick of a 4-tap kernel is the 2-tap kernel of the same reference setting in the same round.
HIP events per launch, warm-up first, median of REPS launches per round.

It then holds this run's 2-tap timings against profiles/angular_ext_rate.txt (the same jobs, the
same frames): the difference of the medians beside that record's own spread over its rounds.
Writes the record (with mip_build_id()) to --out, default profiles/angular_tap4_rate.txt."""
import argparse
import os
import re
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
REFS = (("substituted", mipgpu.ANG_REFS_SUBSTITUTED), ("extended", mipgpu.ANG_REFS_EXTENDED))
INTERP = (("2-tap", mipgpu.ANG_INTERP_2TAP), ("4-tap", mipgpu.ANG_INTERP_4TAP))


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


def earlier_record(path):
    """{job name: ([substituted ms per round], [extended ms per round])} of profiles/angular_ext_rate.txt."""
    out = {}
    if not os.path.exists(path):
        return out
    for line in open(path):
        m = re.match(r"(.+?)\s+(\d)\s+([\d.]+)\s+([\d.]+)\s+[\d.]+\s*$", line)
        if m:
            sub, ext = out.setdefault(m.group(1).strip(), ([], []))
            sub.append(float(m.group(3)))
            ext.append(float(m.group(4)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "angular_tap4_rate.txt"))
    ap.add_argument("--frames", type=int, default=B)
    args = ap.parse_args()
    nf = args.frames
    dev = torch.device("cuda:0")
    frames = synth_frames_torch(W, H, nf, 0x1080, 0, device=dev)
    nct = layout.num_ctus(W, H)
    ncu = nct * layout.CUS_PER_CTU
    stream = torch.cuda.Stream()
    lines = ["angular family with 4-tap luma interpolation, %dx%d x %d resident frames, original references," % (W, H, nf),
             "median of %d launches per round (HIP events), %d rounds, the two interpolation settings alternating in one process" % (REPS, ROUNDS),
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
    two_tap = {}
    with MipEngine(W, H, max_batch=nf) as eng:
        stream.wait_stream(torch.cuda.current_stream(dev))
        eng.search_device(frames, costs=False, best_mode=best_mode, best_cost=best_cost, stream=stream)
        eng.check_input(stream)
        refine = lambda seeds: (lambda: eng.angular_refine_device(frames, modes=EVEN, seeds=seeds, ang_mode=ang_mode, ang_cost=ang_cost,
                                                                  tried=tried, best_mode=best_mode, best_cost=best_cost, stream=stream))
        jobs = (("cost kernel, 65 modes, best + merge",
                 lambda: eng.angular_device(frames, ang_mode=ang_mode, ang_cost=ang_cost, best_mode=best_mode, best_cost=best_cost, stream=stream)),
                ("cost kernel, 33 even modes, best + merge",
                 lambda: eng.angular_device(frames, modes=EVEN, ang_mode=ang_mode, ang_cost=ang_cost, best_mode=best_mode, best_cost=best_cost,
                                            stream=stream)),
                ("refined search, even list, 1 seed", refine(1)),
                ("refined search, even list, 2 seeds", refine(2)),
                ("block output, %d items per frame" % cus.size,
                 lambda: eng.predict_device(frames, d_items, canvas, stream=stream, angular=True)))
        for refs_name, refs_value in REFS:
            eng.angular_refs = refs_value
            lines.append("%s reference lines" % refs_name)
            lines.append("%-44s %-8s %s   %s" % ("ms per frame", "round", "   ".join("%11s" % n for n, _ in INTERP), "4-tap / 2-tap"))
            for name, fn in jobs:
                ratios = []
                for r in range(ROUNDS):
                    ms = []
                    for _, value in INTERP:
                        eng.angular_interp = value
                        ms.append(median_ms(fn, stream) / nf)
                    ratios.append(ms[1] / ms[0])
                    two_tap.setdefault((refs_name, name), []).append(ms[0])
                    lines.append("%-44s %-8d %s   %.3f" % (name, r, "   ".join("%11.4f" % v for v in ms), ratios[-1]))
                lines.append("%-44s %-8s %s   %.3f" % ("", "median", " " * (14 * len(INTERP) - 3), statistics.median(ratios)))
            lines.append("")
        eng.angular_interp = mipgpu.ANG_INTERP_2TAP
        eng.angular_refs = mipgpu.ANG_REFS_SUBSTITUTED
    # this run's 2-tap timings beside the earlier record of the same jobs
    path = os.path.join(REPO, "profiles", "angular_ext_rate.txt")
    before = earlier_record(path)
    lines += ["2-tap timings of this run against profiles/angular_ext_rate.txt (median ms per frame; spread: max - min over a record's rounds):",
              "%-44s %-12s %10s %10s %10s %10s %10s" % ("", "lines", "this run", "spread", "record", "spread", "difference")]
    for name, _ in jobs:
        if name not in before:
            continue
        for col, (refs_name, _) in enumerate(REFS):
            now, old = two_tap[(refs_name, name)], before[name][col]
            lines.append("%-44s %-12s %10.4f %10.4f %10.4f %10.4f %+9.2f%%" % (name, refs_name, statistics.median(now), max(now) - min(now),
                                                                                statistics.median(old), max(old) - min(old),
                                                                                100 * (statistics.median(now) / statistics.median(old) - 1)))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

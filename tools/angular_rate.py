#!/usr/bin/env python3
"""Device time of the angular intra costs (mip_angular_device) on resident buffers, 1080p,
original references: best angular mode and merge only (no table), for all 65 modes, for the 32
modes of either class alone and for the 33 even modes, beside two unchanged kernels timed in the
same process -- mip_intra_device (cost table only: Planar and DC, two modes) and the
decisions-only search whose outputs the merge takes.  The yardstick for the angular kernel is the intra kernel's time per mode.

96 frames per launch by default (259 200 work items, 32 rounds of the launcher's capped grid of
a 256-CU device; 384 frames of 65-mode work would add nothing to a median but time).  HIP events
per launch, warm-up first, median of REPS launches.  Writes the record (with mip_build_id()) to
--out, default profiles/angular_rate.txt."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vvc-mip-gpu_amd"))
import torch  # noqa: E402

import mipgpu  # noqa: E402
from mipgpu import MipEngine, layout  # noqa: E402
from mipgpu.synth import synth_frames_torch  # noqa: E402

W, H, B, REPS, WARMUP = 1920, 1080, 96, 20, 3


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "angular_rate.txt"))
    ap.add_argument("--frames", type=int, default=B)
    args = ap.parse_args()
    nf = args.frames
    dev = torch.device("cuda:0")
    frames = synth_frames_torch(W, H, nf, 0x1080, 0, device=dev)
    ncu = layout.num_ctus(W, H) * layout.CUS_PER_CTU
    stream = torch.cuda.Stream()
    lines = ["angular intra cost rate, %dx%d x %d resident frames, original references, median of %d launches (HIP events)"
             % (W, H, nf, REPS), "build: " + mipgpu.build_id(), "device: " + torch.cuda.get_device_name(0), ""]
    best_mode = torch.empty((nf, ncu), dtype=torch.uint8, device=dev)
    best_cost = torch.empty((nf, ncu), dtype=torch.int32, device=dev)
    ang_mode = torch.empty((nf, ncu), dtype=torch.uint8, device=dev)
    ang_cost = torch.empty((nf, ncu), dtype=torch.int32, device=dev)
    cost2 = torch.empty((nf, ncu, 2), dtype=torch.int32, device=dev)
    with MipEngine(W, H, max_batch=nf) as eng:
        def search():
            eng.search_device(frames, costs=False, best_mode=best_mode, best_cost=best_cost, stream=stream)
        stream.wait_stream(torch.cuda.current_stream(dev))
        search_ms = median_ms(search, stream)
        eng.check_input(stream)
        intra_ms = median_ms(lambda: eng.intra_device(frames, cost=cost2, stream=stream), stream)
        per_mode = intra_ms / nf / 2
        lines += ["search: %.4f ms per frame (decisions-only mip_search_device, unchanged kernel)" % (search_ms / nf),
                  "intra:  %.4f ms per frame (mip_intra_device, cost table only, unchanged kernel) = %.4f ms per frame and mode"
                  % (intra_ms / nf, per_mode), "",
                  "%-28s %6s %12s %14s %12s %10s %12s" % ("variant", "modes", "ms / frame", "ms / fr / mode", "x intra/mode", "x search", "frames / s")]
        for name, modes in (("all modes, best + merge", None), ("horizontal class 2..33", tuple(range(2, 34))),
                            ("vertical class 35..66", tuple(range(35, 67))), ("even modes, best + merge", tuple(range(2, 67, 2)))):
            n = 65 if modes is None else len(modes)
            search()                                             # (the merge rewrites the decisions: start from the search's)
            ms = median_ms(lambda: eng.angular_device(frames, modes=modes, ang_mode=ang_mode, ang_cost=ang_cost, best_mode=best_mode,
                                                      best_cost=best_cost, stream=stream), stream)
            lines.append("%-28s %6d %12.4f %14.4f %12.2f %10.2f %12.0f"
                         % (name, n, ms / nf, ms / nf / n, ms / nf / n / per_mode, ms / search_ms, nf / ms * 1e3))
        stream.synchronize()
        taken = int(((best_mode >= 0x82) & (best_mode <= 0xC2)).sum().item())
        assert int((ang_cost == layout.UNAVAILABLE).sum().item()) == int((best_mode == 0xFF).sum().item())
    lines += ["", "merged decisions: %.1f %% of the available CUs took an even angular mode over their MIP mode (zero bias)"
              % (100.0 * taken / max(1, int((best_mode != 0xFF).sum().item()))),
              "(launches after the first find the decisions merged -- same reads and arithmetic, no rewrites);",
              "ms / fr / mode: time per frame divided by the modes of the list;",
              "x intra/mode: that over the intra kernel's time per frame and mode (its table time / 2) in this run;",
              "x search: time / decisions-only search time of the same frames."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

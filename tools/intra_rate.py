#!/usr/bin/env python3
"""Device time of the Planar / DC baseline costs (mip_intra_device) on resident buffers, 1080p x
384 frames, original references: (a) the cost table only, (b) the merge only, against two
yardsticks measured in the same process: the decisions-only search (mip_search_device without a
cost table) of the same frames, whose outputs the merge takes, and mip_copy_device of the bytes
each variant reads and writes.

HIP events per launch, warm-up first, median of REPS launches.  Writes the record (with
mip_build_id()) to --out, default profiles/intra_rate.txt."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vvc-mip-gpu_amd"))
import torch  # noqa: E402

import mipgpu  # noqa: E402
from mipgpu import MipEngine, copy_device, layout  # noqa: E402
from mipgpu.synth import synth_frames_torch  # noqa: E402

W, H, B, REPS, WARMUP = 1920, 1080, 384, 20, 3


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "intra_rate.txt"))
    ap.add_argument("--frames", type=int, default=B)
    args = ap.parse_args()
    nf = args.frames
    dev = torch.device("cuda:0")
    frames = synth_frames_torch(W, H, nf, 0x1080, 0, device=dev)
    ncu = layout.num_ctus(W, H) * layout.CUS_PER_CTU
    stream = torch.cuda.Stream()
    lines = ["Planar / DC baseline cost rate, %dx%d x %d resident frames, original references, median of %d launches (HIP events)"
             % (W, H, nf, REPS), "build: " + mipgpu.build_id(), "device: " + torch.cuda.get_device_name(0), ""]
    best_mode = torch.empty((nf, ncu), dtype=torch.uint8, device=dev)
    best_cost = torch.empty((nf, ncu), dtype=torch.int32, device=dev)
    cost = torch.empty((nf, ncu, 2), dtype=torch.int32, device=dev)
    frame_bytes = frames.numel() * 2
    # (a) reads the frames, writes the table; (b) reads the frames and the decisions, rewrites at most all of them
    variants = (("cost table only", dict(cost=cost), frame_bytes + cost.numel() * 4),
                ("merge only", dict(best_mode=best_mode, best_cost=best_cost), frame_bytes + 2 * (best_cost.numel() * 4 + best_mode.numel())))
    with MipEngine(W, H, max_batch=nf) as eng:
        def search():
            eng.search_device(frames, costs=False, best_mode=best_mode, best_cost=best_cost, stream=stream)
        stream.wait_stream(torch.cuda.current_stream(dev))
        search_ms = median_ms(search, stream)
        eng.check_input(stream)
        lines.append("search yardstick: %.4f ms per frame (decisions-only mip_search_device, %d frames per launch)" % (search_ms / nf, nf))
        lines.append("")
        lines.append("%-16s %12s %12s %12s %10s %10s %12s" % ("variant", "ms / frame", "MB / frame", "copy ms / fr", "x copy", "x search", "frames / s"))
        for name, outs, nbytes in variants:
            half = (nbytes // 2 + 15) // 16 * 16                 # a copy reads and writes: half the bytes each way
            src = torch.zeros(half, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copy_ms = median_ms(lambda: copy_device(src, dst, stream=stream), stream)
            del src, dst
            search()                                             # (the merge rewrites the decisions: start from the search's)
            ms = median_ms(lambda: eng.intra_device(frames, stream=stream, **outs), stream)
            lines.append("%-16s %12.4f %12.1f %12.4f %10.2f %10.3f %12.0f"
                         % (name, ms / nf, nbytes / nf / 1e6, copy_ms / nf, ms / copy_ms, ms / search_ms, nf / ms * 1e3))
        stream.synchronize()
        replaced = int((best_mode >= mipgpu.MODE_PLANAR).logical_and(best_mode != 0xFF).sum().item())
        assert int((cost[..., 0] == layout.UNAVAILABLE).sum().item()) == int((best_mode == 0xFF).sum().item())
    lines += ["", "merged decisions: %.1f %% of the available CUs took Planar or DC (zero bias)" % (100.0 * replaced / max(1, int((best_mode != 0xFF).sum().item()))),
              "(merge only: launches after the first find the decisions merged -- same reads and arithmetic, no rewrites);",
              "x copy: time / mip_copy_device of the bytes the variant reads and writes;",
              "x search: time / decisions-only search time of the same frames."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

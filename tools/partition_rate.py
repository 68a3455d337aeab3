#!/usr/bin/env python3
"""Device time of the CTU partition decision (mip_partition_device) on resident buffers, 1080p x
384 frames, all four outputs, against two yardsticks measured in the same process:
mip_copy_device of the bytes the kernel reads and writes, and the decisions-only search
(mip_search_device without a cost table) of the same frames, whose outputs are its inputs.

The penalty is the same for every shape; one row per penalty (0: the all-small tiling, a middle
value, 1<<20: four 64x64 leaves).  HIP events per launch, warm-up first, median of REPS
launches.  Writes the record (with mip_build_id()) to --out, default
profiles/partition_rate.txt."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vvc-mip-gpu_amd"))
import torch  # noqa: E402

import mipgpu  # noqa: E402
from mipgpu import MipEngine, copy_device, layout, partition_device  # noqa: E402
from mipgpu.synth import synth_frames_torch  # noqa: E402

W, H, B, REPS, WARMUP = 1920, 1080, 384, 20, 3
PENALTIES = (0, 1000, 1 << 20)


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "partition_rate.txt"))
    ap.add_argument("--frames", type=int, default=B)
    args = ap.parse_args()
    nf = args.frames
    dev = torch.device("cuda:0")
    frames = synth_frames_torch(W, H, nf, 0x1080, 0, device=dev)
    nct = layout.num_ctus(W, H)
    ncu = nct * layout.CUS_PER_CTU
    stream = torch.cuda.Stream()
    lines = ["partition decision rate, %dx%d x %d resident frames, all outputs, median of %d launches (HIP events)" % (W, H, nf, REPS),
             "build: " + mipgpu.build_id(), "device: " + torch.cuda.get_device_name(0), ""]
    best_mode = torch.empty((nf, ncu), dtype=torch.uint8, device=dev)
    best_cost = torch.empty((nf, ncu), dtype=torch.int32, device=dev)
    with MipEngine(W, H, max_batch=nf) as eng:
        def search():
            eng.search_device(frames, costs=False, best_mode=best_mode, best_cost=best_cost, stream=stream)
        stream.wait_stream(torch.cuda.current_stream(dev))
        search_ms = median_ms(search, stream)
        eng.check_input(stream)
    leaf = torch.empty((nf, ncu), dtype=torch.uint8, device=dev)
    ctu_cost = torch.empty((nf, nct), dtype=torch.int32, device=dev)
    ctu_leaves = torch.empty((nf, nct), dtype=torch.int32, device=dev)
    items = torch.empty((nf, nct, mipgpu.PART_MAX_LEAVES * mipgpu.PRED_ITEM.itemsize), dtype=torch.uint8, device=dev)
    # bytes in: best_cost, best_mode; out: leaf, the two CTU arrays, the item lists
    nbytes = best_cost.numel() * 4 + best_mode.numel() + leaf.numel() + 8 * ctu_cost.numel() + items.numel()
    half = (nbytes // 2 + 15) // 16 * 16                     # a copy reads and writes: half the bytes each way
    src = torch.zeros(half, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy_ms = median_ms(lambda: copy_device(src, dst, stream=stream), stream)
    lines.append("search yardstick: %.4f ms per frame (decisions-only mip_search_device, %d frames per launch)" % (search_ms / nf, nf))
    lines.append("copy yardstick:   %.4f ms per frame (mip_copy_device, %.1f MB read + written per frame)" % (copy_ms / nf, nbytes / nf / 1e6))
    lines.append("")
    lines.append("%-10s %12s %12s %10s %10s %12s" % ("penalty", "ms / frame", "leaves / fr", "x copy", "x search", "frames / s"))
    for pen in PENALTIES:
        def run():
            partition_device(best_cost, W, H, penalty=pen, best_mode=best_mode, leaf=leaf, ctu_cost=ctu_cost,
                             ctu_leaves=ctu_leaves, items=items, stream=stream)
        ms = median_ms(run, stream)
        nleaves = int(ctu_leaves.sum().item())
        assert int(leaf.sum().item()) == nleaves and int((ctu_cost == layout.UNAVAILABLE).sum().item()) == 0
        lines.append("%-10d %12.4f %12.1f %10.2f %10.3f %12.0f" % (pen, ms / nf, nleaves / nf, ms / copy_ms, ms / search_ms, nf / ms * 1e3))
    lines += ["", "x copy: partition time / mip_copy_device of the bytes the kernel reads and writes;",
              "x search: partition time / decisions-only search time of the same frames."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of the prediction output (mip_predict_device) on resident buffers, 1080p x 16
frames, against two yardsticks measured in the same process: mip_copy_device of the same number
of output bytes, and the search (mip_time_search_device) per frame at the same batch.

Tilings, frame layout, best mode of every available CU of one shape: 64x64, 16x16, 4x4.  Packed:
every mode of every 16x16 CU of one frame.  Those four go through mip_predict_device (the MIP-only
kernel instance).  Two more go through mip_predict_device_ex with MIP_PRED_REGULAR: Planar for every
available 16x16 CU, and the item list mip_partition_device writes for the 16 frames after the
Planar / DC merge (bias CHAIN_BIAS, penalty CHAIN_PENALTY; padding entries included, as a caller
that makes no host round trip passes it).  With MIP_PRED_ANGULAR (the second kernel behind the
first: mip_predict_angular.hip's one block-output body, the instance the engine's mip_angular_refs
and mip_angular_interp settings select): every available 16x16 CU with one angular mode of each
class and sign in turn (modes 6, 27, 41, 60), frame layout; the list the partition writes after the
Planar / DC merge and the merge of all 65 angular modes (bias 0), predicted with both flags; and a
list of the same entry count that is padding only, with MIP_PRED_REGULAR alone and with both flags
-- the difference is what the angular kernel's scan of the padding costs.  HIP events per launch,
warm-up first, median of REPS launches.  Writes the record (with mip_build_id()) to --out, default
profiles/predict_rate.txt."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vvc-mip-gpu_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mipgpu  # noqa: E402
from mipgpu import MipEngine, copy_device, layout  # noqa: E402
from mipgpu.synth import synth_frames_torch  # noqa: E402

W, H, B, REPS, WARMUP = 1920, 1080, 16, 30, 5
CHAIN_BIAS, CHAIN_PENALTY = (30, 30), 600


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "predict_rate.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    frames = synth_frames_torch(W, H, B, 0x1080, 0, device=dev)
    nct = layout.num_ctus(W, H)
    prefix = np.cumsum([0] + [s.ncu for s in layout.SHAPES])
    un = mipgpu.unavailable_cus(W, H).reshape(nct, layout.CUS_PER_CTU)
    stream = torch.cuda.Stream()
    lines = ["prediction output rate, %dx%d x %d frames, median of %d launches (HIP events)" % (W, H, B, REPS),
             "build: " + mipgpu.build_id(), "device: " + torch.cuda.get_device_name(0), ""]
    with MipEngine(W, H, max_batch=B) as eng:
        best = torch.empty((B, eng.cus_per_frame), dtype=torch.uint8, device=dev)
        best_cost = torch.empty((B, eng.cus_per_frame), dtype=torch.int32, device=dev)
        eng.search_device(frames, costs=False, best_mode=best, best_cost=best_cost)
        torch.cuda.synchronize()
        best = best.cpu().numpy()
        costs = torch.empty((B, eng.costs_per_frame), dtype=torch.int32, device=dev)
        search_ms = eng.time_search_device(frames, costs, reps=5)           # warm-up
        search_ms = eng.time_search_device(frames, costs, reps=20) / B
        del costs
        lines.append("search yardstick: %.4f ms per frame (mip_time_search_device, %d frames per launch)" % (search_ms, B))
        lines.append("")
        lines.append("%-28s %9s %10s %9s %9s %10s %11s" % ("case", "items", "out MB", "ms", "copy ms", "x copy", "x search/fr"))
        canvas = torch.zeros(B * H * W, dtype=torch.int16, device=dev)
        scratch = torch.empty_like(canvas)

        def run(name, items, out, nframes_of_case, regular=False, angular=False):
            # (a flag that is off passes no keyword: the four MIP cases run on older libraries too)
            kw = dict({"regular": True} if regular else {}, **({"angular": True} if angular else {}))
            d_items = torch.from_numpy(items.view(np.uint8)).to(dev)
            sk = torch.zeros(1, dtype=torch.int32, device=dev)
            eng.predict_device(frames, d_items, out, skipped=sk, stream=stream, **kw)
            torch.cuda.synchronize()
            padding = items["frame"] < 0                      # (a partition list's unused entries)
            assert int(sk.item()) == int(padding.sum()), (name, int(sk.item()))
            ms = median_ms(lambda: eng.predict_device(frames, d_items, out, stream=stream, **kw), stream)
            items = items[~padding]
            shape = layout.cu_geometry(W, H, items["cu"])
            nbytes = int((shape[3].astype(np.int64) * shape[4]).sum()) * 2
            if nbytes == 0:                                   # (a list of padding only: nothing to copy)
                lines.append("%-28s %9d %10.2f %9.4f %9s %10s %11.3f" % (
                    name, d_items.numel() // mipgpu.PRED_ITEM.itemsize, 0.0, ms, "-", "-", ms / nframes_of_case / search_ms))
                return
            nbytes16 = (nbytes + 15) // 16 * 16
            src, dst = canvas.view(torch.uint8)[:nbytes16], scratch.view(torch.uint8)[:nbytes16]
            copy_ms = median_ms(lambda: copy_device(src, dst, stream=stream), stream)
            lines.append("%-28s %9d %10.2f %9.4f %9.4f %10.2f %11.3f" % (
                name, d_items.numel() // mipgpu.PRED_ITEM.itemsize, nbytes / 1e6, ms, copy_ms, ms / copy_ms,
                ms / nframes_of_case / search_ms))

        for sname in ("ALL_AL_64x64", "ALL_AL_16x16", "ALL_AL_4x4"):
            s = layout.SHAPE_BY_NAME[sname]
            ctu, c = np.nonzero(~un[:, prefix[s.index]:prefix[s.index + 1]])
            cu = ctu * layout.CUS_PER_CTU + prefix[s.index] + c
            frame = np.repeat(np.arange(B), cu.size)
            cu_all = np.tile(cu, B)
            items, total = mipgpu.pred_items(W, H, frame, cu_all, best[frame, cu_all], layout="frame", nframes=B)
            assert total == canvas.numel()
            run("frame, best mode, %s" % sname[7:], items, canvas, B)
        s = layout.SHAPE_BY_NAME["ALL_AL_16x16"]
        ctu, c = np.nonzero(~un[:, prefix[s.index]:prefix[s.index + 1]])
        cu = np.repeat(ctu * layout.CUS_PER_CTU + prefix[s.index] + c, s.total_modes)
        mode = np.tile(np.arange(s.total_modes), ctu.size)
        items, total = mipgpu.pred_items(W, H, 0, cu, mode, nframes=B)
        run("packed, all modes, 16x16, 1 fr", items, canvas[:total], 1)
        # regular items (MIP_PRED_REGULAR)
        frame = np.repeat(np.arange(B), ctu.size)
        cu_all = np.tile(ctu * layout.CUS_PER_CTU + prefix[s.index] + c, B)
        items, total = mipgpu.pred_items(W, H, frame, cu_all, mipgpu.MODE_PLANAR, layout="frame", nframes=B)
        run("frame, Planar, 16x16", items, canvas, B, regular=True)
        d_best = torch.empty((B, eng.cus_per_frame), dtype=torch.uint8, device=dev)
        eng.search_device(frames, costs=False, best_mode=d_best, best_cost=best_cost)
        eng.intra_device(frames, bias=CHAIN_BIAS, best_mode=d_best, best_cost=best_cost)
        d_list = torch.zeros((B, nct, mipgpu.PART_MAX_LEAVES * mipgpu.PRED_ITEM.itemsize), dtype=torch.uint8, device=dev)
        mipgpu.partition_device(best_cost, W, H, penalty=CHAIN_PENALTY, best_mode=d_best, items=d_list)
        torch.cuda.synchronize()
        items = d_list.cpu().numpy().reshape(-1).view(mipgpu.PRED_ITEM)
        leaves = items[items["frame"] >= 0]
        n_regular = int(np.isin(leaves["mode"], (mipgpu.MODE_PLANAR, mipgpu.MODE_DC)).sum())
        run("frame, merged partition list", items, canvas, B, regular=True)
        lines.append("merged partition list: %d leaves (%d Planar / DC) in %d entries" % (leaves.size, n_regular, items.size))
        # angular items (MIP_PRED_ANGULAR): one mode of each class and sign in turn
        turn = mipgpu.MODE_ANGULAR_BASE + np.array([6, 27, 41, 60])
        items, total = mipgpu.pred_items(W, H, frame, cu_all, turn[np.arange(cu_all.size) % 4], layout="frame", nframes=B)
        run("frame, angular x4, 16x16", items, canvas, B, angular=True)
        eng.angular_device(frames, bias=0, best_mode=d_best, best_cost=best_cost)
        mipgpu.partition_device(best_cost, W, H, penalty=CHAIN_PENALTY, best_mode=d_best, items=d_list)
        torch.cuda.synchronize()
        items = d_list.cpu().numpy().reshape(-1).view(mipgpu.PRED_ITEM)
        leaves = items[items["frame"] >= 0]
        n_regular = int(np.isin(leaves["mode"], (mipgpu.MODE_PLANAR, mipgpu.MODE_DC)).sum())
        n_angular = int(((leaves["mode"] >= mipgpu.MODE_ANGULAR_BASE + 2) & (leaves["mode"] <= mipgpu.MODE_ANGULAR_BASE + 66)).sum())
        run("frame, angular partition list", items, canvas, B, regular=True, angular=True)
        lines.append("angular partition list: %d leaves (%d Planar / DC, %d angular) in %d entries" % (
            leaves.size, n_regular, n_angular, items.size))
        padding = np.zeros(items.size, mipgpu.PRED_ITEM)
        padding[:] = (-1, -1, -1, 0, 0)
        run("padding only, regular", padding, canvas, B, regular=True)
        run("padding only, both flags", padding, canvas, B, regular=True, angular=True)
    lines += ["", "x copy: prediction time / mip_copy_device of the same number of output bytes;",
              "x search/fr: prediction time per frame of the case / search time per frame."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time of the K-best candidate lists (mip_candidates_device) and of what feeds it, with the
method of tools/angular_refine_rate.py: 1080p resident frames, original references, HIP events per
launch, warm-up first, median of 20 launches.

  kernel rate: candidates_kernel at k = 3, kin = 3, all three families, --frames frames per launch
      (217 MB of tables and lists per frame): ms per frame and bytes read plus written per second,
      beside mip_copy_device moving the same total bytes (half read, half written) in the same
      process; then the families alone and k = 1 / 8 / 32, to see what the rounds cost;
  angular table path: mip_angular_device (65 modes, 33 even) and mip_angular_refine_device (even
      list, one seed) with the ang pair only and with the cost table as well -- the difference is
      what the table-driven design pays over a top-K fused into the angular kernels;
  host chain: mip_candidates_frames (k = 3, Planar / DC, even list, one seed) on pageable host
      frames, ms per frame, beside the sum of its stages' device times at the chunk size the
      256 MiB rule gives at 1080p (one frame): table search + decision lists, Planar / DC table,
      refined angular table, candidates.

Writes the record (with mip_build_id()) to --out, default profiles/candidates_rate.txt."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "vvc-mip-gpu_amd"))
W, H, REPS, WARMUP = 1920, 1080, 20, 3
EVEN = tuple(range(2, 67, 2))


def median_ms(fn, stream):
    import torch
    for _ in range(WARMUP):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for e0, e1 in ev:
        e0.record(stream)
        fn()
        e1.record(stream)
    torch.cuda.synchronize()
    return statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)


def finish(out, lines):
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "candidates_rate.txt"))
    ap.add_argument("--frames", type=int, default=16, help="resident frames of the kernel-rate launches")
    ap.add_argument("--table-frames", type=int, default=8, help="resident frames of the angular launches")
    ap.add_argument("--host-frames", type=int, default=8, help="frames of the host call")
    ap.add_argument("--kernel-only", action="store_true", help="the kernel rate only (A/B of a variant library through MIPGPU_LIB)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import mipgpu
    from mipgpu import MipEngine, layout
    from mipgpu.synth import synth_frames_torch
    dev = torch.device("cuda:0")
    ncu = layout.num_ctus(W, H) * layout.CUS_PER_CTU
    stream = torch.cuda.Stream()
    bid = mipgpu.build_id()
    lines = ["candidate-list rate, %dx%d, original references, median of %d launches (HIP events)" % (W, H, REPS),
             "device: " + torch.cuda.get_device_name(0), "build: " + bid, ""]

    # ---- kernel rate on tables that look like the stages' own: real tables of one frame, repeated
    nf, kin = args.frames, 3
    frames = synth_frames_torch(W, H, max(args.table_frames, 1), 0x1080, 0, device=dev)
    with MipEngine(W, H, max_batch=args.table_frames, best_k=kin) as eng, torch.cuda.stream(stream):
        one = frames[:1]
        mm = torch.empty((1, ncu, kin), dtype=torch.uint8, device=dev)
        mc = torch.empty((1, ncu, kin), dtype=torch.int32, device=dev)
        eng.search_device(one, best_mode=mm, best_cost=mc, stream=stream)
        ic = torch.empty((1, ncu, 2), dtype=torch.int32, device=dev)
        eng.intra_device(one, cost=ic, stream=stream)
        ac = torch.empty((1, ncu, 65), dtype=torch.int32, device=dev)
        eng.angular_refine_device(one, modes=EVEN, seeds=1, cost=ac, stream=stream)
        eng.check_input(stream)
        tabs = {"mip_mode": mm.repeat(nf, 1, 1), "mip_cost": mc.repeat(nf, 1, 1), "intra_cost": ic.repeat(nf, 1, 1), "ang_cost": ac.repeat(nf, 1, 1)}
        del mm, mc, ic, ac
    per_cu = {"mip": 5 * kin, "intra": 8, "ang": 260}
    fams = {"all three": ("mip", "intra", "ang"), "MIP + Planar/DC": ("mip", "intra"), "angular alone": ("ang",), "MIP alone": ("mip",)}
    keys = {"mip": ("mip_mode", "mip_cost"), "intra": ("intra_cost",), "ang": ("ang_cost",)}
    lines += ["candidates_kernel, %d frames per launch, kin = %d, refined even-list angular table (about 35 live slots per CU)" % (nf, kin),
              "%-18s %4s %12s %12s %14s" % ("families", "k", "ms / frame", "bytes / CU", "GB/s (r + w)")]
    rate_all = None
    with torch.cuda.stream(stream):
        for name, fam in fams.items():
            for k in ((1, 3, 8, 32) if name == "all three" else (3,)):
                modes = torch.empty((nf, ncu, k), dtype=torch.uint8, device=dev)
                costs = torch.empty((nf, ncu, k), dtype=torch.int32, device=dev)
                part = {key: tabs[key] for f in fam for key in keys[f]}
                ms = median_ms(lambda: mipgpu.candidates_device(W, H, k, modes=modes, costs=costs, stream=stream, **part), stream)
                nbytes = sum(per_cu[f] for f in fam) + 5 * k
                gbs = nbytes * ncu * nf / ms / 1e6
                if name == "all three" and k == 3:
                    rate_all, total = gbs, nbytes * ncu * nf
                lines.append("%-18s %4d %12.4f %12d %14.1f" % (name, k, ms / nf, nbytes, gbs))
                del modes, costs
        half = total // 2 // 16 * 16
        src = torch.empty(half, dtype=torch.uint8, device=dev)
        dst = torch.empty(half, dtype=torch.uint8, device=dev)
        ms = median_ms(lambda: mipgpu.copy_device(src, dst, stream=stream), stream)
        copy_rate = 2 * half / ms / 1e6
        lines += ["%-18s %4s %12.4f %12s %14.1f" % ("mip_copy_device", "-", ms / nf, "-", copy_rate),
                  "candidates_kernel (all three, k = 3) runs at %.2f of the copy's rate" % (rate_all / copy_rate), ""]
        del src, dst, tabs
    torch.cuda.synchronize()
    if args.kernel_only:
        finish(args.out, lines)
        return

    # ---- the angular table path
    tf = args.table_frames
    lines += ["angular kernels with and without the cost table, %d frames per launch, ms per frame" % tf,
              "%-34s %12s %12s %12s" % ("call", "pair only", "pair + table", "difference")]
    stage = {}
    with MipEngine(W, H, max_batch=tf, best_k=kin) as eng, torch.cuda.stream(stream):
        fr = frames[:tf]
        am = torch.empty((tf, ncu), dtype=torch.uint8, device=dev)
        ag = torch.empty((tf, ncu), dtype=torch.int32, device=dev)
        table = torch.empty((tf, ncu, 65), dtype=torch.int32, device=dev)
        calls = (("mip_angular_device, 65 modes", lambda **o: eng.angular_device(fr, ang_mode=am, ang_cost=ag, stream=stream, **o)),
                 ("mip_angular_device, 33 even", lambda **o: eng.angular_device(fr, modes=EVEN, ang_mode=am, ang_cost=ag, stream=stream, **o)),
                 ("mip_angular_refine_device, even, 1", lambda **o: eng.angular_refine_device(fr, modes=EVEN, seeds=1, ang_mode=am, ang_cost=ag,
                                                                                              stream=stream, **o)))
        for name, call in calls:
            bare = median_ms(lambda: call(), stream) / tf
            full = median_ms(lambda: call(cost=table), stream) / tf
            lines.append("%-34s %12.4f %12.4f %12.4f" % (name, bare, full, full - bare))
        lines.append("")
        # ---- the stages of the host chain at its chunk size (one 1080p frame)
        one = frames[:1]
        costs = torch.empty((1, eng.costs_per_frame), dtype=torch.int32, device=dev)
        mm = torch.empty((1, ncu, kin), dtype=torch.uint8, device=dev)
        mc = torch.empty((1, ncu, kin), dtype=torch.int32, device=dev)
        ic = torch.empty((1, ncu, 2), dtype=torch.int32, device=dev)
        om = torch.empty((1, ncu, 3), dtype=torch.uint8, device=dev)
        oc = torch.empty((1, ncu, 3), dtype=torch.int32, device=dev)
        stage["search, table + lists of 3"] = median_ms(lambda: eng.search_device(one, costs=costs, best_mode=mm, best_cost=mc, stream=stream), stream)
        stage["Planar / DC table"] = median_ms(lambda: eng.intra_device(one, cost=ic, stream=stream), stream)
        stage["refined angular table"] = median_ms(lambda: eng.angular_refine_device(one, modes=EVEN, seeds=1, cost=table[:1], stream=stream), stream)
        stage["candidates, k = 3"] = median_ms(lambda: mipgpu.candidates_device(W, H, 3, mm, mc, ic, None, table[:1], 0, om, oc, stream=stream), stream)
        eng.check_input(stream)
    torch.cuda.synchronize()
    del table, costs

    # ---- the host chain
    hf = args.host_frames
    host = np.ascontiguousarray(frames[:1].cpu().numpy().view(np.uint16).repeat(hf, axis=0))
    with MipEngine(W, H, max_batch=hf) as eng:
        import time
        eng.candidates(host[:2], k=3, angular=EVEN, seeds=1)            # warm-up: scratch blocks, tables
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            eng.candidates(host, k=3, angular=EVEN, seeds=1)
            times.append((time.perf_counter() - t0) * 1e3 / hf)
    lines += ["mip_candidates_frames, k = 3, Planar / DC + even list with one seed, %d pageable frames, chunks of one frame" % hf,
              "wall time per frame, median of 3 calls: %.3f ms" % statistics.median(times),
              "device time of the stages of a one-frame chunk:"]
    lines += ["  %-30s %8.3f ms" % kv for kv in stage.items()]
    lines += ["  %-30s %8.3f ms" % ("sum", sum(stage.values())),
              "(the rest is the chunk's upload of 4.1 MB, the download of the 10.9 MB of lists and the synchronisation per chunk)"]
    finish(args.out, lines)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Device time and decision quality of the coarse-to-fine angular search
(mip_angular_refine_device) beside mip_angular_device, with the method of tools/angular_rate.py:
1080p x 96 resident frames, original references, HIP events per launch, warm-up first, median of
20 launches, best + merge, no tables.

  mip_angular_device, all 65 modes and the 33 even modes: this library and, with --parent DIR (the
      vvc-mip-gpu_amd directory of a built checkout of the parent commit), that library too, each
      in child processes of this one, alternating, ROUNDS times -- the spread between rounds of one
      library is the yardstick for a difference between the two;
  mip_angular_refine_device, even list, seeds 1..3: ms per frame, the mean of `tried` per available
      CU, and the time per evaluated candidate mode -- (time - even-list time) / mean candidates --
      as a ratio to the list mode's time (even-list time / 33) of the same process;
  quality, from the outputs of the same frames: the share of available CUs whose refined cost
      equals the 65-mode best cost, and the share whose merged decision (bias 0, onto the
      decisions-only search) differs from the 65-mode merge.

Writes the record (with mip_build_id()) to --out, default profiles/angular_refine_rate.txt."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, B, REPS, WARMUP, ROUNDS = 1920, 1080, 96, 20, 3, 2
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


def measure(package, nf, refine):
    """One process's figures as a dict (printed as JSON by a child)."""
    sys.path.insert(0, package)
    import torch
    import mipgpu
    from mipgpu import MipEngine, layout
    from mipgpu.synth import synth_frames_torch
    dev = torch.device("cuda:0")
    frames = synth_frames_torch(W, H, nf, 0x1080, 0, device=dev)
    ncu = layout.num_ctus(W, H) * layout.CUS_PER_CTU
    stream = torch.cuda.Stream()
    new = lambda dt: torch.empty((nf, ncu), dtype=dt, device=dev)
    best_mode, best_cost, ang_mode, ang_cost = new(torch.uint8), new(torch.int32), new(torch.uint8), new(torch.int32)
    res = {"build": mipgpu.build_id(), "device": torch.cuda.get_device_name(0)}
    with MipEngine(W, H, max_batch=nf) as eng:
        def search():
            eng.search_device(frames, costs=False, best_mode=best_mode, best_cost=best_cost, stream=stream)
        stream.wait_stream(torch.cuda.current_stream(dev))
        search()
        eng.check_input(stream)
        for key, modes in (("all65", None), ("even33", EVEN)):
            search()                                             # (the merge rewrites the decisions: start from the search's)
            res[key] = median_ms(lambda: eng.angular_device(frames, modes=modes, ang_mode=ang_mode, ang_cost=ang_cost, best_mode=best_mode,
                                                            best_cost=best_cost, stream=stream), stream) / nf
        if refine:
            def merged(call):
                search()
                call()
                stream.synchronize()
                return best_mode.clone(), ang_cost.clone()
            m65, c65 = merged(lambda: eng.angular_device(frames, ang_mode=ang_mode, ang_cost=ang_cost, best_mode=best_mode, best_cost=best_cost,
                                                         stream=stream))
            on = c65 != layout.UNAVAILABLE
            n_on = int(on.sum().item())
            m33, c33 = merged(lambda: eng.angular_device(frames, modes=EVEN, ang_mode=ang_mode, ang_cost=ang_cost, best_mode=best_mode,
                                                         best_cost=best_cost, stream=stream))
            res["even33_same_cost"] = int(((c33 == c65) & on).sum().item()) / n_on
            res["even33_other_decision"] = int(((m33 != m65) & on).sum().item()) / n_on
            tried = new(torch.uint8)
            for seeds in (1, 2, 3):
                def call():
                    eng.angular_refine_device(frames, modes=EVEN, seeds=seeds, ang_mode=ang_mode, ang_cost=ang_cost, tried=tried,
                                              best_mode=best_mode, best_cost=best_cost, stream=stream)
                search()
                ms = median_ms(call, stream) / nf
                m, c = merged(call)
                assert bool(((c <= c33) & (c >= c65)).all().item())   # never above the list's best, never below the 65-mode best
                assert int((tried[~on] != 0).sum().item()) == 0
                res["refine%d" % seeds] = {"ms": ms, "tried": float(tried[on].float().mean().item()),
                                           "same_cost": int(((c == c65) & on).sum().item()) / n_on,
                                           "other_decision": int(((m != m65) & on).sum().item()) / n_on}
    return res


def child(package, nf, refine):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", package, "--frames", str(nf)] + (["--refine"] if refine else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit("child failed (%d):\n%s" % (out.returncode, out.stdout[-2000:] + out.stderr[-2000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "angular_refine_rate.txt"))
    ap.add_argument("--frames", type=int, default=B)
    ap.add_argument("--parent", help="vvc-mip-gpu_amd directory of a built checkout of the parent commit")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--refine", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.child, args.frames, args.refine)))
        return
    nf, here = args.frames, os.path.join(REPO, "vvc-mip-gpu_amd")
    runs = []                                                    # (label, figures), alternating
    for r in range(ROUNDS):
        if args.parent:
            runs.append(("parent", child(args.parent, nf, False)))
        runs.append(("this", child(here, nf, r == ROUNDS - 1)))
    last = runs[-1][1]
    lines = ["coarse-to-fine angular search rate, %dx%d x %d resident frames, original references, median of %d launches (HIP events)"
             % (W, H, nf, REPS), "device: " + last["device"]]
    for label in ("parent", "this"):
        ids = {f["build"] for l, f in runs if l == label}
        lines += ["build (%s): %s" % (label, b) for b in sorted(ids)]
    lines += ["", "mip_angular_device, best + merge, ms per frame (one process per line, in the order run)",
              "%-8s %12s %12s" % ("library", "65 modes", "33 even")]
    lines += ["%-8s %12.4f %12.4f" % (l, f["all65"], f["even33"]) for l, f in runs]
    for key in ("all65", "even33"):
        by = {label: [f[key] for l, f in runs if l == label] for label in ("parent", "this")}
        spread = max(max(v) - min(v) for v in by.values() if v)
        text = "%s: spread between rounds of one library at most %.4f ms" % (key, spread)
        if by["parent"]:
            text += "; this - parent, means: %+.4f ms" % (statistics.mean(by["this"]) - statistics.mean(by["parent"]))
        lines.append(text)
    per_list_mode = last["even33"] / 33
    lines += ["", "mip_angular_refine_device, even list, best + merge + tried (the last process above; list mode = %.4f ms per frame, even / 33)"
              % per_list_mode,
              "%-8s %12s %12s %14s %16s %14s %16s" % ("seeds", "ms / frame", "mean tried", "x 65-mode call", "x list mode/cand", "= 65-mode cost", "other decision")]
    lines.append("%-8s %12.4f %12.2f %14.3f %16s %13.2f%% %15.2f%%" % ("(even)", last["even33"], 33, last["even33"] / last["all65"], "-",
                                                                       100 * last["even33_same_cost"], 100 * last["even33_other_decision"]))
    for seeds in (1, 2, 3):
        f = last["refine%d" % seeds]
        per_cand = (f["ms"] - last["even33"]) / (f["tried"] - 33)
        lines.append("%-8d %12.4f %12.2f %14.3f %16.2f %13.2f%% %15.2f%%" % (seeds, f["ms"], f["tried"], f["ms"] / last["all65"],
                                                                           per_cand / per_list_mode, 100 * f["same_cost"], 100 * f["other_decision"]))
    lines += ["", "mean tried: modes evaluated per available CU (list + candidates);",
              "x 65-mode call: time / the 65-mode mip_angular_device time of the same process;",
              "x list mode/cand: (time - even-list time) / (mean tried - 33), over the even-list time / 33;",
              "= 65-mode cost: available CUs whose best cost equals the best over all 65 modes;",
              "other decision: available CUs whose merged decision (bias 0, onto the decisions-only search) is not the 65-mode merge's."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

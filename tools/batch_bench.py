"""R doMotifSampling repetitions: a loop of gs_motif_sampling over the seeds against one
gs_motif_sampling_batch call over the same seeds.

    python tools/batch_bench.py                      # the three shapes -> profiles/batch/batch_bench.json
    python tools/batch_bench.py --shapes small --out /tmp/x.json
    python tools/batch_bench.py --loop-lib PATH      # the loop through another build of the library

Per shape: a warm-up of both sides (code objects, allocations), then `--reps` timed
repetitions of each side, wall clock around the call(s) that return host results; the
median counts, the spread (min, max) is recorded.  Every repetition asserts that the
batch's positions and pass counts equal the loop's, row by row.  The batch's two device
stages (the chains' first stages back to back, the one greedy launch) come from
gs_batch_last_ms; the loop's greedy time from gs_run_greedy on the same chains' states.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

from conftest import make_dataset  # noqa: E402
from pmc_traffic import _code_only  # noqa: E402

# name: (N, L, W, R)
SHAPES = {"small": (200, 200, 12, 64), "medium": (2_000, 200, 12, 32),
          "cfg2": (10_000, 200, 12, 8)}
PC, CUTOFF, SEED0 = 1e-4, 1.0, 7
SOURCES = ["gibbssampling_amd/csrc/gs_greedy.hip", "gibbssampling_amd/csrc/gs_api.cpp",
           "gibbssampling_amd/csrc/gs_batch.cpp",
           "gibbssampling_amd/csrc/gs_engine.cpp", "gibbssampling_amd/csrc/gs_starts.hip",
           "gibbssampling_amd/csrc/gs_sweep.hip", "gibbssampling_amd/csrc/gs_common.h",
           "gibbssampling_amd/csrc/gs_ctx.h", "gibbssampling_amd/csrc/Makefile"]


def source_hash(root: Path = ROOT) -> str:
    h = hashlib.sha256()
    for s in SOURCES:
        h.update(s.encode())
        h.update(_code_only((root / s).read_text()).encode())
    return h.hexdigest()


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs),
            "runs_ms": list(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--init-mode", type=int, default=0)
    ap.add_argument("--loop-lib", default=None,
                    help="library the sequential loop runs through (default: the built one)")
    ap.add_argument("--batch-lib", default=None,
                    help="library the batch call runs through (default: the built one)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch" / "batch_bench.json"))
    args = ap.parse_args()
    from gibbssampling_amd import Context

    rec = {"tool": "tools/batch_bench.py", "source_sha256": source_hash(),
           "pc": PC, "cutoff": CUTOFF, "init_mode": args.init_mode, "reps": args.reps,
           "loop_lib": args.loop_lib or "built", "batch_lib": args.batch_lib or "built", "shapes": {}}
    for name in args.shapes:
        N, L, W, R = SHAPES[name]
        codes, offsets = make_dataset(N, L, W, b"ACGT", seed=5)
        seeds = [SEED0 + r for r in range(R)]
        loop_ctx = Context(0, lib_path=args.loop_lib)
        batch_ctx = Context(0, lib_path=args.batch_lib)
        for c in (loop_ctx, batch_ctx):
            c.set_sequences(codes, offsets, b"ACGT")
        loop_ctx.motif_sampling(W, PC, CUTOFF, seeds[0], args.init_mode)  # warm-up
        batch_ctx.motif_sampling_batch(W, PC, CUTOFF, seeds[:2], args.init_mode)
        loop_ms, batch_ms, stage1_ms, greedy_ms = [], [], [], []
        passes = None
        for _ in range(args.reps):
            t = time.perf_counter()
            rows = [loop_ctx.motif_sampling(W, PC, CUTOFF, s, args.init_mode) for s in seeds]
            loop_ms.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            pos, pwms, bpass, status = batch_ctx.motif_sampling_batch(W, PC, CUTOFF, seeds,
                                                                      args.init_mode)
            batch_ms.append((time.perf_counter() - t) * 1e3)
            s1, s2 = batch_ctx.batch_last_ms()
            stage1_ms.append(s1)
            greedy_ms.append(s2)
            assert not status.any(), status
            for r, (p, w, k) in enumerate(rows):
                assert np.array_equal(pos[r], p), f"{name}: positions of chain {r} differ"
                assert bpass[r] == k, f"{name}: passes of chain {r} differ"
            passes = [int(k) for k in bpass]
        # the loop's greedy stage alone: the chains' states after their sweep, then
        # gs_run_greedy's own device time (star engine + hand-over, as the loop runs it)
        loop_greedy = []
        for s in seeds:
            sc, p0 = loop_ctx.random_starts(W, PC, s, args.init_mode)
            loop_ctx.set_positions(W, p0)
            loop_ctx.run_sweeps(PC, CUTOFF, 1, s)
            loop_greedy.append(loop_ctx.run_greedy(PC, CUTOFF)[1])
        lm, bm = statistics.median(loop_ms), statistics.median(batch_ms)
        rec["shapes"][name] = {
            "N": N, "L": L, "W": W, "chains": R, "passes": passes,
            "loop": spread(loop_ms), "batch": spread(batch_ms),
            "speedup_median": lm / bm,
            "batch_stage1_device_ms": spread(stage1_ms),
            "batch_greedy_launch_device_ms": spread(greedy_ms),
            "loop_greedy_device_ms_sum": float(sum(loop_greedy)),
            "loop_greedy_device_ms_per_chain": [float(x) for x in loop_greedy],
            "positions_identical": True,
        }
        print(f"{name}: loop {lm:.2f} ms, batch {bm:.2f} ms, x{lm / bm:.2f} "
              f"(stage 1 {statistics.median(stage1_ms):.2f} ms, greedy launch "
              f"{statistics.median(greedy_ms):.2f} ms; loop greedy {sum(loop_greedy):.2f} ms)",
              file=sys.stderr, flush=True)
        loop_ctx.close()
        batch_ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"loop_ms": v["loop"]["median_ms"], "batch_ms": v["batch"]["median_ms"],
                          "speedup": v["speedup_median"]} for k, v in rec["shapes"].items()}))


if __name__ == "__main__":
    main()

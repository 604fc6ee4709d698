"""R getPWMOfRandomStarts runs: a loop of gs_random_starts over the seeds against one
gs_random_starts_batch call over the same seeds.

    python tools/starts_batch_bench.py                      # the four shapes, modes 0 and 1
    python tools/starts_batch_bench.py --shapes dna200 --modes 1 --out /tmp/x.json

Both sides run through this tree's library on a context of their own.  Per shape and mode:
a warm-up of both sides (code objects, allocations), then `--reps` timed repetitions of each
side, wall clock around the call(s) that return host results; the median counts, the spread
(min, max) is recorded.  Every repetition asserts that the batch's rows equal the loop's:
positions and score bits.  The batch's device stages (counts or aggregates, scans) come from
gs_starts_batch_last_ms.
"""
import argparse
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

from multi_batch_bench import dataset as fsx_dataset, source_hash, spread  # noqa: E402
from conftest import make_dataset  # noqa: E402

# name: (N, L, W, R); fsx: bioTestsWithMultipleSamples of the reference's script (.fsx:407)
SHAPES = {"fsx": (5, 27, 6, 64), "dna200": (200, 200, 12, 64), "dna2000": (2_000, 200, 12, 32),
          "dna10k": (10_000, 200, 12, 8)}
PC, SEED0 = 1e-4, 7


def dataset(name):
    if name == "fsx":
        return fsx_dataset(name)
    N, L, W, _ = SHAPES[name]
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=5)
    return codes, offsets, b"ACGT"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--modes", nargs="*", type=int, default=[0, 1])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch" / "starts_batch_bench.json"))
    args = ap.parse_args()
    from gibbssampling_amd import Context

    rec = {"tool": "tools/starts_batch_bench.py", "source_sha256": source_hash(), "pc": PC,
           "reps": args.reps, "shapes": {}}
    for name in args.shapes:
        N, L, W, R = SHAPES[name]
        codes, offsets, alpha = dataset(name)
        seeds = [SEED0 + r for r in range(R)]
        loop_ctx, batch_ctx = Context(0), Context(0)
        for c in (loop_ctx, batch_ctx):
            c.set_sequences(codes, offsets, alpha)
        for mode in args.modes:
            loop_ctx.random_starts(W, PC, seeds[0], mode)  # warm-up
            batch_ctx.random_starts_batch(W, PC, seeds[:2], mode)
            loop_ms, batch_ms, stages = [], [], []
            for _ in range(args.reps):
                t = time.perf_counter()
                rows = [loop_ctx.random_starts(W, PC, s, mode) for s in seeds]
                loop_ms.append((time.perf_counter() - t) * 1e3)
                t = time.perf_counter()
                score, pos, status = batch_ctx.random_starts_batch(W, PC, seeds, mode)
                batch_ms.append((time.perf_counter() - t) * 1e3)
                stages.append(batch_ctx.starts_batch_last_ms())
                assert not status.any(), status
                for r, (s1, p1) in enumerate(rows):
                    assert np.array_equal(pos[r], p1), f"{name} mode {mode}: starts of chain {r} differ"
                    assert np.array_equal(score[r].view(np.uint64), s1.view(np.uint64)), \
                        f"{name} mode {mode}: scores of chain {r} differ"
            lm, bm = statistics.median(loop_ms), statistics.median(batch_ms)
            rec["shapes"][f"{name}-mode{mode}"] = {
                "N": N, "L": L, "W": W, "chains": R, "mode": mode,
                "loop": spread(loop_ms), "batch": spread(batch_ms), "speedup_median": lm / bm,
                "batch_slowest_below_loop_fastest": max(batch_ms) < min(loop_ms),
                "loop_slowest_below_batch_fastest": max(loop_ms) < min(batch_ms),
                "batch_counts_device_ms": spread([s[0] for s in stages]),
                "batch_scans_device_ms": spread([s[1] for s in stages]),
                "loop_us_per_chain": lm * 1e3 / R,
                "rows_identical": True,
            }
            print(f"{name} mode {mode}: loop {lm:.2f} ({min(loop_ms):.2f} - {max(loop_ms):.2f}) ms, "
                  f"batch {bm:.2f} ({min(batch_ms):.2f} - {max(batch_ms):.2f}) ms, x{lm / bm:.2f}; "
                  f"stages {[round(statistics.median(s[i] for s in stages), 3) for i in range(2)]} ms",
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

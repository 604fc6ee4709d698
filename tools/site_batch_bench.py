"""R doSiteSampling repetitions: a loop of gs_site_sampling over the seeds against one
gs_site_sampling_batch call over the same seeds.

    python tools/site_batch_bench.py                  # the three shapes -> profiles/batch/site_batch_bench.json
    python tools/site_batch_bench.py --shapes small --init-mode 1 --out /tmp/x.json
    python tools/site_batch_bench.py --loop-lib PATH  # the loop through another build of the library

Per shape: a warm-up of both sides (code objects, allocations), then `--reps` timed
repetitions of each side, wall clock around the call(s) that return host results; the
median counts, the spread (min, max) is recorded.  Every repetition asserts that the
batch's positions and pass triples equal the loop's, row by row.  The batch's three device
stages (the chains' starts back to back, the one Gauss–Seidel launch, the shifted passes)
come from gs_site_batch_last_ms.
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

from batch_bench import SHAPES, source_hash, spread  # noqa: E402
from conftest import make_dataset  # noqa: E402

PC, SEED0 = 1e-4, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--init-mode", type=int, default=0)
    ap.add_argument("--loop-lib", default=None,
                    help="library the sequential loop runs through (default: the built one)")
    ap.add_argument("--batch-lib", default=None,
                    help="library the batch call runs through (default: the built one)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch" / "site_batch_bench.json"))
    args = ap.parse_args()
    from gibbssampling_amd import Context

    rec = {"tool": "tools/site_batch_bench.py", "source_sha256": source_hash(),
           "pc": PC, "init_mode": args.init_mode, "reps": args.reps,
           "loop_lib": args.loop_lib or "built", "batch_lib": args.batch_lib or "built", "shapes": {}}
    for name in args.shapes:
        N, L, W, R = SHAPES[name]
        codes, offsets = make_dataset(N, L, W, b"ACGT", seed=5)
        seeds = [SEED0 + r for r in range(R)]
        loop_ctx = Context(0, lib_path=args.loop_lib)
        batch_ctx = Context(0, lib_path=args.batch_lib)
        for c in (loop_ctx, batch_ctx):
            c.set_sequences(codes, offsets, b"ACGT")
        loop_ctx.site_sampling(W, PC, seeds[0], args.init_mode)  # warm-up
        batch_ctx.site_sampling_batch(W, PC, seeds[:2], args.init_mode)
        loop_ms, batch_ms, stages = [], [], [[], [], []]
        passes = None
        for _ in range(args.reps):
            t = time.perf_counter()
            rows = [loop_ctx.site_sampling(W, PC, s, args.init_mode) for s in seeds]
            loop_ms.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            pos, score, bpass, status = batch_ctx.site_sampling_batch(W, PC, seeds, args.init_mode)
            batch_ms.append((time.perf_counter() - t) * 1e3)
            for xs, ms in zip(stages, batch_ctx.site_batch_last_ms()):
                xs.append(ms)
            assert not status.any(), status
            for r, (p, sc, k) in enumerate(rows):
                assert np.array_equal(pos[r], p), f"{name}: positions of chain {r} differ"
                assert np.array_equal(bpass[r], k), f"{name}: passes of chain {r} differ"
            passes = [[int(x) for x in k] for k in bpass]
        lm, bm = statistics.median(loop_ms), statistics.median(batch_ms)
        rec["shapes"][name] = {
            "N": N, "L": L, "W": W, "chains": R, "passes": passes,
            "loop": spread(loop_ms), "batch": spread(batch_ms),
            "speedup_median": lm / bm,
            "batch_faster_than_loop_spread": max(batch_ms) < min(loop_ms),
            "batch_starts_device_ms": spread(stages[0]),
            "batch_gauss_seidel_launch_device_ms": spread(stages[1]),
            "batch_shifted_passes_device_ms": spread(stages[2]),
            "positions_identical": True,
        }
        print(f"{name}: loop {lm:.2f} ms, batch {bm:.2f} ms, x{lm / bm:.2f} (starts "
              f"{statistics.median(stages[0]):.2f} ms, Gauss-Seidel launch "
              f"{statistics.median(stages[1]):.2f} ms, shifted passes "
              f"{statistics.median(stages[2]):.2f} ms)", file=sys.stderr, flush=True)
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

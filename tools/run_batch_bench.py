"""R independent chains of T sweeps: a loop of gs_motif_run over the seeds against one
gs_motif_run_batch call over the same seeds.

    python tools/run_batch_bench.py --loop-lib PATH                 # the three shapes, T = 20 and 200
    python tools/run_batch_bench.py --loop-lib PATH --shapes dna200 --clear 1 --out /tmp/x.json

The loop runs through the parent commit's build of the library (--loop-lib, required), never
this tree's own.  Both sides start from the same uploaded rows (init_mode -1): the positions
of random_starts mode 1 per seed, computed outside the timed region.  Per shape and T: a
warm-up of both sides (code objects, allocations), then `--reps` timed repetitions of each
side, wall clock around the call(s) that return host results; the median counts, the spread
(min, max) is recorded.  Every repetition asserts that the batch's rows equal the loop's:
positions exactly, PWMS within 1e-12 relative.  The batch's device stages (starts and first
aggregates, sweeps) come from gs_run_batch_last_ms.  --clear sets run_batch_clear (0: a
memset of the next aggregate rows before each sweep, 1: a third row cleared in-kernel),
--blocks run_batch_blocks (workgroups per CU) on the batch side.
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
SHAPES = {"dna200": (200, 200, 12, 64), "dna2000": (2_000, 200, 12, 16),
          "dna10k": (10_000, 200, 12, 8)}
PC, CUTOFF, SEED0 = 1e-4, 1.0, 7
SOURCES = ["gibbssampling_amd/csrc/gs_multi.hip", "gibbssampling_amd/csrc/gs_api.cpp",
           "gibbssampling_amd/csrc/gs_batch.cpp",
           "gibbssampling_amd/csrc/gs_engine.cpp", "gibbssampling_amd/csrc/gs_starts.hip",
           "gibbssampling_amd/csrc/gs_common.h", "gibbssampling_amd/csrc/gs_ctx.h",
           "gibbssampling_amd/csrc/Makefile"]


def source_hash(root: Path = ROOT) -> str:
    h = hashlib.sha256()
    for s in SOURCES:
        h.update(s.encode())
        h.update(_code_only((root / s).read_text()).encode())
    return h.hexdigest()


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs),
            "runs_ms": list(xs)}


def close(g, o):
    rel = np.abs(g - o) / np.maximum(np.abs(o), 1e-300)
    return bool(np.all((g == o) | (rel <= 1e-12)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--sweeps", nargs="*", type=int, default=[20, 200])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-lib", required=True,
                    help="the parent commit's build of the library, for the sequential loop")
    ap.add_argument("--clear", type=int, default=None, help="run_batch_clear of the batch side")
    ap.add_argument("--blocks", type=int, default=None, help="run_batch_blocks of the batch side")
    ap.add_argument("--batch-lib", default=None,
                    help="library the batch call runs through (default: the built one)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch" / "run_batch_bench.json"))
    args = ap.parse_args()
    from gibbssampling_amd import Context

    tuning = {k: v for k, v in (("run_batch_clear", args.clear), ("run_batch_blocks", args.blocks))
              if v is not None}
    rec = {"tool": "tools/run_batch_bench.py", "source_sha256": source_hash(), "pc": PC,
           "cutoff": CUTOFF, "reps": args.reps, "loop_lib": "parent commit's build",
           "starts": "random_starts mode 1 per seed, uploaded (init_mode -1)", "tuning": tuning,
           "batch_lib": args.batch_lib or "built", "shapes": {}}
    for name in args.shapes:
        N, L, W, R = SHAPES[name]
        codes, offsets = make_dataset(N, L, W, b"ACGT", seed=5)
        seeds = [SEED0 + r for r in range(R)]
        loop_ctx = Context(0, lib_path=args.loop_lib)
        batch_ctx = Context(0, lib_path=args.batch_lib, tuning=tuning or None)
        for c in (loop_ctx, batch_ctx):
            c.set_sequences(codes, offsets, b"ACGT")
        starts = np.array([loop_ctx.random_starts(W, PC, s, 1)[1] for s in seeds], np.int32)
        for T in args.sweeps:
            loop_ctx.motif_run(W, PC, CUTOFF, T, seeds[0], starts[0])  # warm-up
            batch_ctx.motif_run_batch(W, PC, CUTOFF, T, seeds[:2], pos=starts[:2])
            loop_ms, batch_ms, stages, kept = [], [], [], None
            for _ in range(args.reps):
                t = time.perf_counter()
                rows = [loop_ctx.motif_run(W, PC, CUTOFF, T, s, starts[r])
                        for r, s in enumerate(seeds)]
                loop_ms.append((time.perf_counter() - t) * 1e3)
                t = time.perf_counter()
                pos, pwms, status = batch_ctx.motif_run_batch(W, PC, CUTOFF, T, seeds, pos=starts)
                batch_ms.append((time.perf_counter() - t) * 1e3)
                stages.append(batch_ctx.run_batch_last_ms())
                assert not status.any(), status
                for r, (p1, w1) in enumerate(rows):
                    assert np.array_equal(pos[r], p1), f"{name} T={T}: positions of chain {r} differ"
                    assert close(pwms[r], w1), f"{name} T={T}: PWMS of chain {r} differ"
                kept = [int((p >= 0).sum()) for p in pos]
            lm, bm = statistics.median(loop_ms), statistics.median(batch_ms)
            rec["shapes"][f"{name}-T{T}"] = {
                "N": N, "L": L, "W": W, "chains": R, "sweeps": T, "motifs_kept": kept,
                "loop": spread(loop_ms), "batch": spread(batch_ms),
                "speedup_median": lm / bm,
                "batch_slowest_below_loop_fastest": max(batch_ms) < min(loop_ms),
                "loop_fastest_below_batch_slowest": max(loop_ms) < min(batch_ms),
                "batch_starts_device_ms": spread([s[0] for s in stages]),
                "batch_sweeps_device_ms": spread([s[1] for s in stages]),
                "batch_us_per_sweep_launch": statistics.median(s[1] for s in stages) * 1e3 / T,
                "loop_us_per_chain_sweep": lm * 1e3 / (R * T),
                "rows_identical": True,
            }
            print(f"{name} T={T}: loop {lm:.2f} ({min(loop_ms):.2f} - {max(loop_ms):.2f}) ms, "
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

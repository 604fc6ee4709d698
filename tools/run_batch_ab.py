"""gs_motif_run_batch's two launch choices, A/B in one process: how the next
aggregate rows are zeroed (run_batch_clear 0: a memset before each sweep, 1: a third row
cleared in-kernel) and how many one-wavefront workgroups a CU the sweep launches
(run_batch_blocks).

    python tools/run_batch_ab.py [--out profiles/batch/run_batch_ab.json]

One context per variant on the same data and starts; the variants take turns, `--rounds`
times after a warm-up of each, so that drift of the machine falls on all alike.  Per call:
wall clock and the device time of the sweeps (gs_run_batch_last_ms).  Every call's rows
must equal the first variant's.
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

from conftest import make_dataset  # noqa: E402

# name: (N, L, W, R, T)
SHAPES = {"dna200": (200, 200, 12, 64, 200), "dna2000": (2_000, 200, 12, 16, 200),
          "dna10k": (10_000, 200, 12, 8, 20)}
VARIANTS = [(0, 8), (1, 8), (0, 16), (1, 16), (0, 32), (1, 32)]  # (clear, blocks)
PC, CUTOFF, SEED0 = 1e-4, 1.0, 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch" / "run_batch_ab.json"))
    args = ap.parse_args()
    from gibbssampling_amd import Context

    rec = {"tool": "tools/run_batch_ab.py", "rounds": args.rounds, "shapes": {}}
    for name, (N, L, W, R, T) in SHAPES.items():
        codes, offsets = make_dataset(N, L, W, b"ACGT", seed=5)
        seeds = [SEED0 + r for r in range(R)]
        ctxs = []
        for clear, blocks in VARIANTS:
            c = Context(0, tuning={"run_batch_clear": clear, "run_batch_blocks": blocks})
            c.set_sequences(codes, offsets, b"ACGT")
            ctxs.append(c)
        starts = np.array([ctxs[0].random_starts(W, PC, s, 1)[1] for s in seeds], np.int32)
        want = ctxs[0].motif_run_batch(W, PC, CUTOFF, T, seeds, pos=starts)
        for c in ctxs[1:]:
            c.motif_run_batch(W, PC, CUTOFF, T, seeds, pos=starts)  # warm-up
        wall = [[] for _ in VARIANTS]
        dev = [[] for _ in VARIANTS]
        for _ in range(args.rounds):
            for i, c in enumerate(ctxs):
                t = time.perf_counter()
                pos, pwms, status = c.motif_run_batch(W, PC, CUTOFF, T, seeds, pos=starts)
                wall[i].append((time.perf_counter() - t) * 1e3)
                dev[i].append(c.run_batch_last_ms()[1])
                assert not status.any() and np.array_equal(pos, want[0])
                assert np.array_equal(pwms.view(np.uint64), want[1].view(np.uint64))
        rows = {}
        for i, (clear, blocks) in enumerate(VARIANTS):
            rows[f"clear{clear}-blocks{blocks}"] = {
                "wall_ms": {"median": statistics.median(wall[i]), "min": min(wall[i]),
                            "max": max(wall[i])},
                "sweeps_device_ms": {"median": statistics.median(dev[i]), "min": min(dev[i]),
                                     "max": max(dev[i])}}
            print(f"{name} clear {clear} blocks {blocks}: wall {statistics.median(wall[i]):.3f} "
                  f"({min(wall[i]):.3f} - {max(wall[i]):.3f}) ms, sweeps on the device "
                  f"{statistics.median(dev[i]):.3f} ({min(dev[i]):.3f} - {max(dev[i]):.3f}) ms",
                  file=sys.stderr, flush=True)
        rec["shapes"][name] = {"N": N, "L": L, "W": W, "chains": R, "sweeps": T, "variants": rows}
        for c in ctxs:
            c.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

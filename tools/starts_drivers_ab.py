"""The four batched drivers with their starts chain after chain or batched.

    python tools/starts_drivers_ab.py --config parent --lib PATH --out a.json   # one process
    python tools/starts_drivers_ab.py --config loop --out b.json                # batch_starts 0
    python tools/starts_drivers_ab.py --config batched --out c.json             # batch_starts 1
    python tools/starts_drivers_ab.py --merge a.json b.json c.json ... --out profiles/batch/starts/drivers_ab.json

One process measures one configuration: the parent commit's build of the library (--lib),
or this tree's with batch_starts 0 / 1.  The processes take turns (the caller's loop), so
that no configuration owns a stretch of the machine's time.  Per driver, shape (those of the
drivers' own bench tools) and init_mode: a warm-up call, then `--reps` timed calls, wall
clock around the call, and the device time of stage 1 (gs_*_last_ms out[0]).  Only the batch
side runs: the loops over the single-chain entry points are in the drivers' own records.
Every call's arrays are hashed; --merge refuses configurations whose hashes differ, pools the
processes' runs per configuration and reports median (min - max).
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

from starts_batch_bench import dataset  # noqa: E402

PC, CUTOFF, SEED0, SWEEPS = 1e-4, 1.0, 7, 20
# driver: [(shape of starts_batch_bench.SHAPES, W, chains)]
CELLS = {
    "motif_batch": [("dna200", 12, 64), ("dna2000", 12, 32), ("dna10k", 12, 8)],
    "site_batch": [("dna200", 12, 64), ("dna2000", 12, 32), ("dna10k", 12, 8)],
    "multi_batch": [("fsx", 6, 64), ("dna200", 12, 64), ("dna2000", 12, 16)],
    "run_batch": [("dna200", 12, 64), ("dna2000", 12, 16), ("dna10k", 12, 8)],
}


def call(ctx, driver, W, seeds, mode):
    """(arrays of the result, device ms of the call's stages)."""
    if driver == "motif_batch":
        out = ctx.motif_sampling_batch(W, PC, CUTOFF, seeds, mode)
        return out, ctx.batch_last_ms()
    if driver == "site_batch":
        out = ctx.site_sampling_batch(W, PC, seeds, mode)
        return out, ctx.site_batch_last_ms()
    if driver == "multi_batch":
        cnt, pos, pwms, passes, status = ctx.motif_sampling_multi_batch(2, W, PC, CUTOFF, seeds, mode)
        live = np.arange(pos.shape[2])[None, None, :] < cnt[:, :, None]
        return (cnt, np.where(live, pos, -1), pwms, passes, status), ctx.multi_batch_last_ms()
    out = ctx.motif_run_batch(W, PC, CUTOFF, SWEEPS, seeds, init_mode=mode)
    return out, ctx.run_batch_last_ms()


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def measure(args):
    from gibbssampling_amd import Context
    tuning = None if args.config == "parent" else {"batch_starts": int(args.config == "batched")}
    rec = {"config": args.config, "reps": args.reps, "cells": {}}
    for driver in args.drivers:
        for name, W, R in CELLS[driver]:
            codes, offsets, alpha = dataset(name)
            seeds = [SEED0 + r for r in range(R)]
            ctx = Context(0, lib_path=args.lib, tuning=tuning)
            ctx.set_sequences(codes, offsets, alpha)
            for mode in (0, 1):
                call(ctx, driver, W, seeds[:2], mode)  # warm-up
                wall, stage1, later, dig = [], [], [], None
                for _ in range(args.reps):
                    t = time.perf_counter()
                    out, stages = call(ctx, driver, W, seeds, mode)
                    wall.append((time.perf_counter() - t) * 1e3)
                    stage1.append(stages[0])
                    later.append(sum(stages[1:]))
                    dig = digest(out)
                rec["cells"][f"{driver}/{name}/mode{mode}"] = {
                    "chains": R, "wall_ms": wall, "stage1_device_ms": stage1,
                    "later_stages_device_ms": later, "sha256": dig}
                print(f"{args.config} {driver} {name} mode {mode}: wall "
                      f"{statistics.median(wall):.2f} ms, stage 1 {statistics.median(stage1):.2f} ms",
                      file=sys.stderr, flush=True)
            ctx.close()
    return rec


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs),
            "runs_ms": list(xs)}


def merge(args):
    pooled = {}
    for path in args.merge:
        r = json.loads(Path(path).read_text())
        for cell, v in r["cells"].items():
            p = pooled.setdefault(cell, {}).setdefault(
                r["config"], {"wall": [], "stage1": [], "later": [], "sha256": v["sha256"]})
            assert p["sha256"] == v["sha256"], f"{cell}: rows differ between runs of {r['config']}"
            p["wall"] += v["wall_ms"]
            p["stage1"] += v["stage1_device_ms"]
            p["later"] += v["later_stages_device_ms"]
    rec = {"tool": "tools/starts_drivers_ab.py", "pc": PC, "sweeps_run_batch": SWEEPS,
           "processes": len(args.merge), "cells": {}}
    for cell, cfgs in pooled.items():
        assert len({c["sha256"] for c in cfgs.values()}) == 1, f"{cell}: rows differ"
        out = {k: {"wall": spread(c["wall"]), "stage1_device": spread(c["stage1"]),
                   "later_stages_device": spread(c["later"])}
               for k, c in cfgs.items()}
        if {"parent", "loop", "batched"} <= set(cfgs):
            pw = out["parent"]["wall"]
            out["loop_within_parent_spread"] = \
                pw["min_ms"] <= out["loop"]["wall"]["median_ms"] <= pw["max_ms"]
            out["batched_median_below_parent_min"] = \
                out["batched"]["wall"]["median_ms"] < pw["min_ms"]
        out["rows_identical"] = True
        rec["cells"][cell] = out
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["parent", "loop", "batched"])
    ap.add_argument("--lib", default=None, help="--config parent: the parent commit's build")
    ap.add_argument("--drivers", nargs="*", default=list(CELLS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--merge", nargs="*", default=None)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.merge is None and (args.config is None or (args.config == "parent") != bool(args.lib)):
        ap.error("--config parent needs --lib, the other configurations take none")
    rec = merge(args) if args.merge is not None else measure(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""R repetitions of the ByPCV / WithBPV / OfPPM pipelines: a loop of the single-chain entry
point (gs_motif_sampling, gs_site_sampling, gs_motif_sampling_multi) on a context that has
the caller's PCV or PPM set, against one call of the batched entry point that takes the
values as arguments (gs_*_batch_fixed).

    python tools/fixed_batch_bench.py --loop-lib PATH            # -> profiles/batch/fixed_batch_bench.json
    python tools/fixed_batch_bench.py --loop-lib PATH --cases motif-small-pcv --processes 1

--loop-lib names the build of the library the loop runs through (the parent commit's: the
loop's entry points did not change, the batched ones did not exist there).  The
measurement of every case is taken in `--processes` fresh processes, one after the other;
a process warms both sides up, then times `--reps` alternating repetitions of the loop
and of the batch call, wall clock around the call(s) that return host results, and
reports the median of each side.  The record holds the median (min - max) of the
processes' medians.  Every repetition asserts that the batch's positions and pass counts
equal the loop's, row by row.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from conftest import make_dataset  # noqa: E402

# shape: (alphabet, N, L, W, chains); fsx: bioTestsWithMultipleSamples of the reference's
# script (.fsx:407), the motifAmount 2 case
SHAPES = {"small": (b"ACGT", 200, 200, 12, 64), "medium": (b"ACGT", 2_000, 200, 12, 32),
          "fsx": (b"ATGC-", 5, 27, 6, 64)}
# case: (driver, shape); each under a PCV and under a PPM
CASES = {f"{d}-{s}-{k}": (d, s, k)
         for d, s in (("motif", "small"), ("motif", "medium"), ("site", "small"),
                      ("site", "medium"), ("multi", "fsx"))
         for k in ("pcv", "ppm")}
PC, CUTOFF, SEED0 = 1e-4, 1.0, 7
CHILD_LIMIT_S = 900


def data(shape):
    alpha, N, L, W, R = SHAPES[shape]
    if shape == "fsx":
        sets = json.loads((ROOT / "tests" / "golden" / "fsx_sets.json").read_text())
        seqs = sets["bioTestsWithMultipleSamples"]["seqs"]
        codes = np.frombuffer("".join(seqs).encode(), np.uint8).copy()
        offsets = np.zeros(len(seqs) + 1, np.int64)
        np.cumsum([len(s) for s in seqs], out=offsets[1:])
        return codes, offsets
    return make_dataset(N, L, W, alpha, seed=5)


def values(alpha, W, kind):
    """The caller's PCV (non-uniform, strictly positive, a value at every slot) or PPM."""
    rng = np.random.default_rng(11)
    pcv = rng.uniform(0.05, 0.6, 49)
    pcv[[c - 42 for c in alpha]] = rng.dirichlet(np.ones(len(alpha)))
    ppm = rng.uniform(0.01, 1.0, (49, W))
    return (pcv, None) if kind == "pcv" else (None, ppm)


def sides(driver, W, seeds):
    """(loop(ctx) -> rows, batch(ctx, pcv, ppm) -> rows) with rows of (positions, passes)."""
    if driver == "motif":
        def loop(c):
            return [(p, k) for p, _, k in (c.motif_sampling(W, PC, CUTOFF, s) for s in seeds)]

        def batch(c, pcv, ppm):
            pos, _, passes, status = c.motif_sampling_batch(W, PC, CUTOFF, seeds, pcv=pcv, ppm=ppm)
            assert not status.any(), status
            return list(zip(pos, passes))
    elif driver == "site":
        def loop(c):
            return [(p, tuple(k)) for p, _, k in (c.site_sampling(W, PC, s) for s in seeds)]

        def batch(c, pcv, ppm):
            pos, _, passes, status = c.site_sampling_batch(W, PC, seeds, pcv=pcv, ppm=ppm)
            assert not status.any(), status
            return [(p, tuple(k)) for p, k in zip(pos, passes)]
    else:
        def live(cnt, pos):
            return np.where(np.arange(pos.shape[-1])[None, :] < cnt[:, None], pos, -1)

        def loop(c):
            return [(live(cn, p), k) for cn, p, _, k in
                    (c.motif_sampling_multi(2, W, PC, CUTOFF, s) for s in seeds)]

        def batch(c, pcv, ppm):
            cnt, pos, _, passes, status = c.motif_sampling_multi_batch(2, W, PC, CUTOFF, seeds,
                                                                       pcv=pcv, ppm=ppm)
            assert not status.any(), status
            return [(live(cn, p), k) for cn, p, k in zip(cnt, pos, passes)]
    return loop, batch


def child(args):
    """One process's medians of every case, as one JSON line."""
    from gibbssampling_amd import Context
    out = {}
    for name in args.cases:
        driver, shape, kind = CASES[name]
        alpha, N, L, W, R = SHAPES[shape]
        codes, offsets = data(shape)
        seeds = [SEED0 + r for r in range(R)]
        pcv, ppm = values(alpha, W, kind)
        loop_ctx = Context(0, lib_path=args.loop_lib)
        batch_ctx = Context(0)
        for c in (loop_ctx, batch_ctx):
            c.set_sequences(codes, offsets, alpha)
        loop_ctx.set_fixed_pcv(pcv)
        loop_ctx.set_fixed_ppm(ppm)
        loop, batch = sides(driver, W, seeds)
        loop(loop_ctx)  # warm-up: code objects, allocations
        batch(batch_ctx, pcv, ppm)
        loop_ms, batch_ms = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            rows = loop(loop_ctx)
            loop_ms.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            got = batch(batch_ctx, pcv, ppm)
            batch_ms.append((time.perf_counter() - t) * 1e3)
            for r, ((p, k), (bp, bk)) in enumerate(zip(rows, got)):
                assert np.array_equal(bp, p), f"{name}: positions of chain {r} differ"
                assert bk == k, f"{name}: passes of chain {r} differ"
        out[name] = {"loop_ms": statistics.median(loop_ms), "batch_ms": statistics.median(batch_ms)}
        print(f"{name}: loop {out[name]['loop_ms']:.2f} ms, batch {out[name]['batch_ms']:.2f} ms",
              file=sys.stderr, flush=True)
        loop_ctx.close()
        batch_ctx.close()
    print(json.dumps(out))


def spread(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs),
            "processes_ms": list(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--loop-lib", required=True,
                    help="library the sequential loop runs through (the parent commit's build)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch" / "fixed_batch_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = []
    for _ in range(args.processes):  # fresh processes, one at a time
        r = subprocess.run([sys.executable, __file__, "--child", "--loop-lib", args.loop_lib,
                            "--reps", str(args.reps), "--cases", *args.cases],
                           stdout=subprocess.PIPE, text=True, timeout=CHILD_LIMIT_S)
        if r.returncode != 0:  # nothing more on the GPU after a failure
            sys.exit(f"a measuring process ended with status {r.returncode}")
        runs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    rec = {"tool": "tools/fixed_batch_bench.py", "pc": PC, "cutoff": CUTOFF, "init_mode": 0,
           "reps": args.reps, "processes": args.processes, "loop_lib": args.loop_lib,
           "batch_lib": "built", "cases": {}}
    for name in args.cases:
        driver, shape, kind = CASES[name]
        alpha, N, L, W, R = SHAPES[shape]
        lo = spread([r[name]["loop_ms"] for r in runs])
        ba = spread([r[name]["batch_ms"] for r in runs])
        rec["cases"][name] = {"driver": driver, "values": kind, "N": N, "L": L, "W": W,
                              "chains": R, "motif_amount": 2 if driver == "multi" else 1,
                              "loop": lo, "batch": ba,
                              "speedup_median": lo["median_ms"] / ba["median_ms"],
                              "positions_identical": True}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"loop_ms": v["loop"]["median_ms"], "batch_ms": v["batch"]["median_ms"],
                          "speedup": v["speedup_median"]} for k, v in rec["cases"].items()}))


if __name__ == "__main__":
    main()

"""R doMotifSampling repetitions with motifAmount 2: a loop of gs_motif_sampling_multi over
the seeds against one gs_motif_sampling_multi_batch call over the same seeds (DESIGN.md
§9.12).

    python tools/multi_batch_bench.py --loop-lib PATH        # the three shapes
    python tools/multi_batch_bench.py --loop-lib PATH --init-mode 1 --out profiles/batch/multi_batch_bench_mode1.json
    python tools/multi_batch_bench.py --loop-lib PATH --shapes dna200 --fill 1 --out /tmp/x.json

The loop runs through the parent commit's build of the library (--loop-lib, required), never
this tree's own.  Per shape: a warm-up of both sides (code objects, allocations), then
`--reps` timed repetitions of each side, wall clock around the call(s) that return host
results; the median counts, the spread (min, max) is recorded.  Every repetition asserts
that the batch's lists and pass counts equal the loop's, row by row.  The batch's three
device stages (starts, sweep, greedy passes) come from gs_multi_batch_last_ms, its rounds
and slots per chain from gs_multi_batch_last_info.  --fill sets the slot rule's
multi_batch_fill (scoring workgroups per CU over all chains) on the batch side.
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

# name: (N, L, W, R); fsx: bioTestsWithMultipleSamples of the reference's script (.fsx:407)
SHAPES = {"fsx": (5, 27, 6, 64), "dna200": (200, 200, 12, 64), "dna2000": (2_000, 200, 12, 16)}
M, PC, CUTOFF, SEED0 = 2, 1e-4, 1.0, 7
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


def dataset(name):
    N, L, W, R = SHAPES[name]
    if name == "fsx":
        sets = json.loads((ROOT / "tests" / "golden" / "fsx_sets.json").read_text())
        seqs = sets["bioTestsWithMultipleSamples"]["seqs"]
        codes = np.frombuffer("".join(seqs).encode(), np.uint8).copy()
        offsets = np.zeros(len(seqs) + 1, np.int64)
        np.cumsum([len(s) for s in seqs], out=offsets[1:])
        return codes, offsets, b"ATGC-"
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=5)
    return codes, offsets, b"ACGT"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--init-mode", type=int, default=0)
    ap.add_argument("--loop-lib", required=True,
                    help="the parent commit's build of the library, for the sequential loop")
    ap.add_argument("--fill", type=int, default=None, help="multi_batch_fill of the batch side")
    ap.add_argument("--batch-lib", default=None,
                    help="library the batch call runs through (default: the built one)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch" / "multi_batch_bench.json"))
    args = ap.parse_args()
    from gibbssampling_amd import Context

    rec = {"tool": "tools/multi_batch_bench.py", "source_sha256": source_hash(),
           "motif_amount": M, "pc": PC, "cutoff": CUTOFF, "init_mode": args.init_mode,
           "reps": args.reps, "loop_lib": "parent commit's build", "multi_batch_fill": args.fill,
           "batch_lib": args.batch_lib or "built", "shapes": {}}
    for name in args.shapes:
        N, L, W, R = SHAPES[name]
        codes, offsets, alpha = dataset(name)
        seeds = [SEED0 + r for r in range(R)]
        loop_ctx = Context(0, lib_path=args.loop_lib)
        batch_ctx = Context(0, lib_path=args.batch_lib, tuning=None if args.fill is None else {"multi_batch_fill": args.fill})
        for c in (loop_ctx, batch_ctx):
            c.set_sequences(codes, offsets, alpha)
        loop_ctx.motif_sampling_multi(M, W, PC, CUTOFF, seeds[0], args.init_mode)  # warm-up
        batch_ctx.motif_sampling_multi_batch(M, W, PC, CUTOFF, seeds[:2], args.init_mode)
        loop_ms, batch_ms, stages, info, passes = [], [], [], None, None
        for _ in range(args.reps):
            t = time.perf_counter()
            rows = [loop_ctx.motif_sampling_multi(M, W, PC, CUTOFF, s, args.init_mode)
                    for s in seeds]
            loop_ms.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            cnt, pos, pwms, bpass, status = batch_ctx.motif_sampling_multi_batch(
                M, W, PC, CUTOFF, seeds, args.init_mode)
            batch_ms.append((time.perf_counter() - t) * 1e3)
            stages.append(batch_ctx.multi_batch_last_ms())
            info = batch_ctx.multi_batch_last_info()
            assert not status.any(), status
            for r, (c1, p1, w1, k) in enumerate(rows):
                assert np.array_equal(cnt[r], c1), f"{name}: list lengths of chain {r} differ"
                assert all(np.array_equal(pos[r, n, :c1[n]], p1[n, :c1[n]]) for n in range(N)), \
                    f"{name}: positions of chain {r} differ"
                assert bpass[r] == k, f"{name}: passes of chain {r} differ"
            passes = [int(k) for k in bpass]
        lm, bm = statistics.median(loop_ms), statistics.median(batch_ms)
        rec["shapes"][name] = {
            "N": N, "L": L, "W": W, "chains": R, "passes": passes,
            "loop": spread(loop_ms), "batch": spread(batch_ms),
            "speedup_median": lm / bm,
            "batch_slowest_below_loop_fastest": max(batch_ms) < min(loop_ms),
            "batch_starts_device_ms": spread([s[0] for s in stages]),
            "batch_sweep_device_ms": spread([s[1] for s in stages]),
            "batch_greedy_device_ms": spread([s[2] for s in stages]),
            "batch_info": info,
            "lists_identical": True,
        }
        print(f"{name}: loop {lm:.2f} ({min(loop_ms):.2f} - {max(loop_ms):.2f}) ms, batch {bm:.2f} "
              f"({min(batch_ms):.2f} - {max(batch_ms):.2f}) ms, x{lm / bm:.2f}; stages "
              f"{[round(statistics.median(s[i] for s in stages), 2) for i in range(3)]} ms, {info}",
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

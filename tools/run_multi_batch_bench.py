"""R independent chains of T sweeps with Positions lists: a loop of gs_motif_sweep_multi over
the seeds and sweeps against one gs_motif_run_multi_batch call over the same seeds
(DESIGN.md §9.19).

    python tools/run_multi_batch_bench.py --loop-lib PATH            # the four shapes, T = 20
    python tools/run_multi_batch_bench.py --loop-lib PATH --shapes dna200 --out /tmp/x.json

The loop runs through the parent commit's build of the library (--loop-lib, required), never
this tree's own: per seed and per sweep one gs_motif_sweep_multi call fed the previous output,
its uniforms the counter RNG's row made on the host (vectorised; inside the timed region, as a
caller of the loop pays for it).  Both sides start from the same uploaded lists (init_mode
-1): the positions of random_starts mode 1 per seed as one-position lists, computed outside
the timed region.  Per shape: a warm-up of both sides (code objects, allocations), then
`--reps` timed repetitions of each side, wall clock around the call(s) that return host
results; the median counts, the spread (min, max) is recorded.  Every repetition asserts that
the batch's rows equal the loop's: lists exactly, PWMS within 1e-12 relative.  The batch's
device stages (starts and first aggregates, sweeps) come from gs_run_multi_batch_last_ms, its
overflow handling from gs_run_multi_batch_last_info.  --blocks sets run_batch_blocks
(workgroups per CU) on the batch side.
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

from conftest import make_dataset, uniforms  # noqa: E402
from pmc_traffic import _code_only  # noqa: E402

# name: (N, L, W, M, cut-off, R); fsx407 is the reference script's own set (N 5, L 27)
SHAPES = {"fsx407": (5, 27, 6, 2, 1.0, 64), "dna200": (200, 200, 12, 2, 1.0, 64),
          "dna2000": (2_000, 200, 12, 2, 1.0, 16), "m3-overflow": (12, 120, 2, 3, -1000.0, 16)}
PC, SEED0 = 1e-4, 7
STREAM_SWEEP = 1 << 40  # gs_stream_sweep(t) = STREAM_SWEEP | t
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


def dataset(name):
    N, L, W, M, cutoff, R = SHAPES[name]
    if name == "fsx407":
        sets = json.loads((ROOT / "tests" / "golden" / "fsx_sets.json").read_text())
        seqs = sets["bioTestsWithMultipleSamples"]["seqs"]
        codes = np.frombuffer("".join(seqs).encode(), np.uint8).copy()
        offsets = np.zeros(len(seqs) + 1, np.int64)
        np.cumsum([len(s) for s in seqs], out=offsets[1:])
        return codes, offsets, b"ATGC-"
    codes, offsets = make_dataset(N, L, W, b"ACGT", seed=5, mut=0.0 if M >= 3 else 0.25)
    return codes, offsets, b"ACGT"


def loop_chain(ctx, M, W, cutoff, T, seed, cnt, pos):
    pw = None
    for t in range(T):
        u = uniforms(seed, STREAM_SWEEP | t, len(cnt))
        cnt, pos, pw = ctx.motif_sweep_multi(M, W, PC, cutoff, cnt, pos, u)
    return cnt, pos, pw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--sweeps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-lib", required=True,
                    help="the parent commit's build of the library, for the sequential loop")
    ap.add_argument("--blocks", type=int, default=None, help="run_batch_blocks of the batch side")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch" / "run_multi_batch_bench.json"))
    args = ap.parse_args()
    from gibbssampling_amd import Context

    T = args.sweeps
    tuning = {"run_batch_blocks": args.blocks} if args.blocks is not None else {}
    rec = {"tool": "tools/run_multi_batch_bench.py", "source_sha256": source_hash(), "pc": PC,
           "sweeps": T, "reps": args.reps, "loop_lib": "parent commit's build",
           "loop": "gs_motif_sweep_multi per seed and sweep, uniforms made on the host (timed)",
           "starts": "random_starts mode 1 per seed as one-position lists, uploaded (init_mode -1)",
           "tuning": tuning, "shapes": {}}
    for name in args.shapes:
        N, L, W, M, cutoff, R = SHAPES[name]
        codes, offsets, alpha = dataset(name)
        seeds = [SEED0 + r for r in range(R)]
        loop_ctx = Context(0, lib_path=args.loop_lib)
        batch_ctx = Context(0, tuning=tuning or None)
        for c in (loop_ctx, batch_ctx):
            c.set_sequences(codes, offsets, alpha)
        cnt0 = np.ones((R, N), np.int32)
        pos0 = np.full((R, N, M), -1, np.int32)
        for r, s in enumerate(seeds):
            pos0[r, :, 0] = loop_ctx.random_starts(W, PC, s, 1)[1]
        loop_chain(loop_ctx, M, W, cutoff, T, seeds[0], cnt0[0], pos0[0])  # warm-up
        batch_ctx.motif_run_multi_batch(M, W, PC, cutoff, T, seeds[:2], cnt0[:2], pos0[:2])
        loop_ms, batch_ms, stages, info, lens = [], [], [], None, None
        for _ in range(args.reps):
            t = time.perf_counter()
            rows = [loop_chain(loop_ctx, M, W, cutoff, T, s, cnt0[r], pos0[r])
                    for r, s in enumerate(seeds)]
            loop_ms.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            cnt, pos, pwms, status = batch_ctx.motif_run_multi_batch(M, W, PC, cutoff, T, seeds,
                                                                     cnt0, pos0)
            batch_ms.append((time.perf_counter() - t) * 1e3)
            stages.append(batch_ctx.run_multi_batch_last_ms())
            info = batch_ctx.run_multi_batch_last_info()
            assert not status.any(), status
            for r, (c1, p1, w1) in enumerate(rows):
                assert np.array_equal(cnt[r], c1), f"{name}: list lengths of chain {r} differ"
                assert np.array_equal(pos[r], p1), f"{name}: lists of chain {r} differ"
                assert close(pwms[r], w1), f"{name}: PWMS of chain {r} differ"
            lens = np.bincount(cnt.ravel(), minlength=M + 1).tolist()
        lm, bm = statistics.median(loop_ms), statistics.median(batch_ms)
        rec["shapes"][name] = {
            "N": N, "L": L, "W": W, "motif_amount": M, "cutoff": cutoff, "chains": R, "sweeps": T,
            "lists_by_length": lens, "loop": spread(loop_ms), "batch": spread(batch_ms),
            "speedup_median": lm / bm,
            "batch_slowest_below_loop_fastest": max(batch_ms) < min(loop_ms),
            "loop_fastest_below_batch_slowest": max(loop_ms) < min(batch_ms),
            "batch_starts_device_ms": spread([s[0] for s in stages]),
            "batch_sweeps_device_ms": spread([s[1] for s in stages]),
            "batch_us_per_sweep": statistics.median(s[1] for s in stages) * 1e3 / T,
            "loop_us_per_chain_sweep": lm * 1e3 / (R * T),
            "overflow": info, "rows_identical": True,
        }
        print(f"{name}: loop {lm:.2f} ({min(loop_ms):.2f} - {max(loop_ms):.2f}) ms, "
              f"batch {bm:.2f} ({min(batch_ms):.2f} - {max(batch_ms):.2f}) ms, x{lm / bm:.2f}; "
              f"stages {[round(statistics.median(s[i] for s in stages), 3) for i in range(2)]} ms; "
              f"{info}", file=sys.stderr, flush=True)
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

"""R chains of T sweeps and whether pooling them was justified: one
gs_motif_run_batch_agreement call that asks for no bins against what a caller had to do before
it, every chain's bins downloaded and compared with the pool in numpy.

    python tools/run_agreement_bench.py --loop-lib PATH                  # the three shapes
    python tools/run_agreement_bench.py --loop-lib PATH --shapes dna10k

Three sides from the same uploaded starts (init_mode -1: the positions of random_starts mode 1
per seed, computed outside the timed region), T = 200, burn_in = 50, thin = 1:
  (a) gs_motif_run_batch_stats with the bins through the parent commit's build (--loop-lib,
      required), then ChainStats.agreement() on the host; the call and the host reduction are
      timed separately;
  (b) one gs_motif_run_batch_agreement call without the bins through this tree's library: the
      summary and the agreement;
  (s) gs_motif_run_batch_summary without the bins through the parent's build: (b) - (s) is what
      the agreement adds to a summary call;
  (s') the same summary call through this tree's library on (b)'s context, as a control: (s)
      and (b) run the same sweeps on different slabs, which alone moves a call's time.
Per shape a warm-up of every side, then `--reps` timed repetitions, the sides interleaved, wall
clock around the call(s) that return host results; the median counts, the spread (min, max) is
recorded.  Every repetition asserts that (b)'s agreement equals (a)'s and (b)'s summary equals
(s)'s exactly, before any time is reported.  The reductions' own device times
(gs_agreement_last_ms, gs_summary_last_ms) are recorded next to the time of a device-to-device
copy of a slab of the bins' size in the same process.
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

from conftest import make_dataset  # noqa: E402
from run_batch_stats_bench import spread  # noqa: E402
from run_summary_bench import copy_ms  # noqa: E402

# name: (N, L, W, R): the shapes of tools/run_batch_stats_bench.py
SHAPES = {"dna200": (200, 200, 12, 64), "dna2000": (2_000, 200, 12, 16),
          "dna10k": (10_000, 200, 12, 8)}
PC, CUTOFF, SEED0 = 1e-4, 1.0, 7
T, BURN_IN, THIN = 200, 50, 1
ALPHA = b"ACGT"
AGREEMENT = ("agree", "spread", "spread_chain", "chain_agree", "chain_dist")
SUMMARY = ("mode_pos", "mode_count", "counts", "pooled_pos", "pooled_count", "pooled_counts",
           "n_pooled")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-lib", required=True,
                    help="the parent commit's build of the library: sides (a) and (s)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch" / "run_agreement_bench.json"))
    args = ap.parse_args()
    from gibbssampling_amd import ChainStats, Context

    rec = {"tool": "tools/run_agreement_bench.py", "pc": PC, "cutoff": CUTOFF, "reps": args.reps,
           "sweeps": T, "burn_in": BURN_IN, "thin": THIN, "loop_lib": "parent commit's build",
           "starts": "random_starts mode 1 per seed, uploaded", "shapes": {}}
    n_counted = len(range(BURN_IN, T, THIN))
    for name in args.shapes:
        N, L, W, R = SHAPES[name]
        codes, offsets = make_dataset(N, L, W, ALPHA, seed=5)
        seeds = [SEED0 + 1000 * r for r in range(R)]
        parent_stats, parent_summary = (Context(0, lib_path=args.loop_lib) for _ in range(2))
        mine = Context(0)
        ctxs = (parent_stats, parent_summary, mine)
        for c in ctxs:
            c.set_sequences(codes, offsets, ALPHA)
        starts = np.stack([parent_summary.random_starts(W, PC, s, 1)[1] for s in seeds])
        kw = dict(pos=starts, init_mode=-1, burn_in=BURN_IN, thin=THIN)

        def side_a():
            t0 = time.perf_counter()
            pos, pw, status, st = parent_stats.motif_run_batch_stats(W, PC, CUTOFF, T, seeds, **kw)
            t1 = time.perf_counter()
            ag = ChainStats(st["occupancy"], st["offsets"], st["ic"], st["best_sweep"],
                            [[]] * R).agreement()
            t2 = time.perf_counter()
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, pos, ag

        def side_b():
            t0 = time.perf_counter()
            pos, pw, status, s = mine.motif_run_batch_agreement(W, PC, CUTOFF, T, seeds, **kw)
            return (time.perf_counter() - t0) * 1e3, pos, s

        def side_s():
            t0 = time.perf_counter()
            pos, pw, status, s = parent_summary.motif_run_batch_summary(W, PC, CUTOFF, T, seeds, **kw)
            return (time.perf_counter() - t0) * 1e3, pos, s

        def side_s_mine():
            t0 = time.perf_counter()
            mine.motif_run_batch_summary(W, PC, CUTOFF, T, seeds, **kw)
            return (time.perf_counter() - t0) * 1e3

        side_a(), side_b(), side_s(), side_s_mine()  # warm-up: code objects, allocations
        ms = {k: [] for k in ("a_call", "a_host", "a", "b", "s", "s_mine")}
        dev_a, dev_s = [], []
        for rep in range(args.reps):
            call, host, pos_a, ag = side_a()
            ms["a_call"].append(call)
            ms["a_host"].append(host)
            ms["a"].append(call + host)
            t, pos_b, b = side_b()
            ms["b"].append(t)
            dev_a.append(mine.agreement_last_ms())
            dev_s.append(mine.summary_last_ms())
            t, pos_s, s = side_s()
            ms["s"].append(t)
            ms["s_mine"].append(side_s_mine())
            assert np.array_equal(pos_a, pos_b) and np.array_equal(pos_b, pos_s), name
            for k in AGREEMENT:
                assert np.array_equal(getattr(ag, k), b[k]), f"{name}: {k} differs"
            assert ag.n_pooled == int(b["agree_n_pooled"][0]) == R, name
            for k in SUMMARY:
                assert np.array_equal(s[k], b[k]), f"{name}: the summary's {k} differs"
        H = int(mine.occupancy_offsets(W)[-1])
        cp = copy_ms(R * H * 4)
        med = {k: statistics.median(v) for k, v in ms.items()}
        dist = b["spread"] / (2.0 * R * n_counted)
        entry = {"N": N, "L": L, "W": W, "chains": R, "counted": n_counted, "bins_a_chain": H,
                 "bin_bytes": R * H * 4,
                 "a_stats_call_parent": spread(ms["a_call"]), "a_host_agreement": spread(ms["a_host"]),
                 "a_total": spread(ms["a"]), "b_agreement_call": spread(ms["b"]),
                 "s_summary_call_parent": spread(ms["s"]),
                 "a_over_b": med["a"] / med["b"], "a_call_alone_over_b": med["a_call"] / med["b"],
                 "agreement_cost_ms_b_minus_s": med["b"] - med["s"],
                 "s_summary_call_this_tree_same_context": spread(ms["s_mine"]),
                 "agreement_cost_ms_b_minus_s_same_context": med["b"] - med["s_mine"],
                 "b_slowest_below_a_fastest": max(ms["b"]) < min(ms["a"]),
                 "agreement_device_ms": spread(dev_a), "summary_device_ms": spread(dev_s),
                 "d2d_copy_of_the_bins_ms": cp,
                 "agreement_over_copy": statistics.median(dev_a) / cp if cp > 0 else None,
                 "results_equal": True,
                 "largest_distance": float(dist.max()), "median_distance": float(np.median(dist)),
                 "sequences_where_every_chain_agrees": int((b["agree"] == R).sum())}
        rec["shapes"][name] = entry
        print(f"{name}: (a) {med['a']:.2f} = call {med['a_call']:.2f} + host {med['a_host']:.2f}, "
              f"(b) {med['b']:.2f} ({min(ms['b']):.2f} - {max(ms['b']):.2f}), (s) {med['s']:.2f}, (s') {med['s_mine']:.2f} ms; "
              f"a / b x{entry['a_over_b']:.2f}, b - s {entry['agreement_cost_ms_b_minus_s']:.2f} ms; "
              f"agreement {statistics.median(dev_a):.3f} ms and summary {statistics.median(dev_s):.3f} "
              f"ms on the device, copy of {R * H * 4} B {cp:.3f} ms", file=sys.stderr, flush=True)
        for c in ctxs:
            c.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"a_ms": v["a_total"]["median_ms"], "b_ms": v["b_agreement_call"]["median_ms"],
                          "s_ms": v["s_summary_call_parent"]["median_ms"]}
                      for k, v in rec["shapes"].items()}))


if __name__ == "__main__":
    main()

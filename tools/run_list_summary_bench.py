"""R chains of T sweeps of Positions lists reduced to what a caller keeps of them (per sequence
the modal list of the pooled chains, and the count matrix over the counted states): one
gs_motif_run_multi_batch_summary call against the statistics call with the host reduction it
needed before.

    python tools/run_list_summary_bench.py --loop-lib PATH                 # the three shapes
    python tools/run_list_summary_bench.py --loop-lib PATH --shapes dna200

The shapes, starts and sweeps are those of tools/run_multi_batch_stats_bench.py (§9.26).  Three
sides from the same uploaded lists:
  (a) gs_motif_run_multi_batch_stats with the bins and site counts through the parent commit's
      build (--loop-lib, required), then on the host ListChainStats.mode() and the pooled count
      matrix by numpy (tools/run_summary_bench.py's); the call and the host part timed apart;
  (b) one gs_motif_run_multi_batch_summary call without bins through this tree's library;
  (c) plain gs_motif_run_multi_batch through the parent's build;
and as a control (a') the statistics call of (a) through this tree's library on a context of
its own.  The sweeps stage by events (gs_run_multi_batch_last_ms) is recorded for every side.
Per shape a warm-up of every side, then `--reps` timed repetitions, the sides interleaved, wall
clock around the call(s) that return host results; the median counts, the spread (min, max) is
recorded.  Every repetition asserts that (b)'s lists, pooled modes and pooled cells equal (a)'s
exactly.  The reduction's own device time (gs_summary_last_ms) is recorded too.
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

from run_batch_stats_bench import bits, spread  # noqa: E402
from run_multi_batch_bench import PC, SEED0, SHAPES as LIST_SHAPES, dataset  # noqa: E402
from run_multi_batch_stats_bench import BURN_IN, SHAPES, T, THIN  # noqa: E402
import run_summary_bench as single  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=SHAPES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-lib", required=True,
                    help="the parent commit's build of the library: sides (a) and (c)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch" /
                                         "run_multi_batch_summary_bench.json"))
    args = ap.parse_args()
    from gibbssampling_amd import Context, ListChainStats, ListChainSummary

    rec = {"tool": "tools/run_list_summary_bench.py", "pc": PC, "reps": args.reps, "sweeps": T,
           "burn_in": BURN_IN, "thin": THIN, "loop_lib": "parent commit's build",
           "starts": "random_starts mode 1 per seed as one-position lists, uploaded (init_mode -1)",
           "shapes": {}}
    n_counted = len(range(BURN_IN, T, THIN))
    for name in args.shapes:
        N, L, W, M, cutoff, R = LIST_SHAPES[name]
        codes, offsets, alpha = dataset(name)
        seeds = [SEED0 + r for r in range(R)]
        parent_stats, parent_plain = (Context(0, lib_path=args.loop_lib) for _ in range(2))
        mine, mine_stats = Context(0), Context(0)
        ctxs = (parent_stats, parent_plain, mine, mine_stats)
        for c in ctxs:
            c.set_sequences(codes, offsets, alpha)
        cnt0 = np.ones((R, N), np.int32)
        pos0 = np.full((R, N, M), -1, np.int32)
        for r, s in enumerate(seeds):
            pos0[r, :, 0] = parent_plain.random_starts(W, PC, s, 1)[1]
        single.ALPHA = alpha  # (the host count matrix reads the alphabet from its module)
        sym, comp = single.host_static(codes, offsets)
        A = len(alpha)

        def side_a(ctx=parent_stats):
            t0 = time.perf_counter()
            cnt, pos, pw, status, st = ctx.motif_run_multi_batch_stats(
                M, W, PC, cutoff, T, seeds, cnt0, pos0, burn_in=BURN_IN, thin=THIN)
            t1 = time.perf_counter()
            if ctx is not parent_stats:
                return (t1 - t0) * 1e3
            cs = ListChainStats(st["occupancy"], st["offsets"], st["ic"], st["best_sweep"], [],
                                st["sites"], W)
            mode = cs.mode()
            pooled = st["occupancy"][cs.finished()].astype(np.int64).sum(axis=0)
            cells = single.host_count_matrix(pooled, st["offsets"], sym, comp, offsets, W)
            t2 = time.perf_counter()
            return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (cnt, pos, pw), mode, cells

        def side_b():
            t0 = time.perf_counter()
            cnt, pos, pw, status, s = mine.motif_run_multi_batch_summary(
                M, W, PC, cutoff, T, seeds, cnt0, pos0, burn_in=BURN_IN, thin=THIN)
            return (time.perf_counter() - t0) * 1e3, (cnt, pos, pw), s

        def side_c():
            t0 = time.perf_counter()
            cnt, pos, pw, status = parent_plain.motif_run_multi_batch(M, W, PC, cutoff, T, seeds,
                                                                      cnt0, pos0)
            return (time.perf_counter() - t0) * 1e3, (cnt, pos, pw)

        side_a(), side_a(mine_stats), side_b(), side_c()  # warm-up: code objects, allocations
        ms = {k: [] for k in ("a_call", "a_host", "a", "a_call_tree", "b", "c")}
        dev = []
        sweeps = {k: [] for k in ("a", "a_tree", "b", "c")}
        for rep in range(args.reps):
            call, host, rows_a, mode_a, cells_a = side_a()
            ms["a_call"].append(call)
            ms["a_host"].append(host)
            ms["a"].append(call + host)
            sweeps["a"].append(parent_stats.run_multi_batch_last_ms()[1])
            ms["a_call_tree"].append(side_a(mine_stats))
            sweeps["a_tree"].append(mine_stats.run_multi_batch_last_ms()[1])
            t, rows_b, s = side_b()
            ms["b"].append(t)
            dev.append(mine.summary_last_ms())
            sweeps["b"].append(mine.run_multi_batch_last_ms()[1])
            t, rows_c = side_c()
            ms["c"].append(t)
            sweeps["c"].append(parent_plain.run_multi_batch_last_ms()[1])
            for x, y, z in zip(rows_a, rows_b, rows_c):
                same = np.array_equal(bits(x), bits(y)) if x.dtype == np.float64 else \
                    np.array_equal(x, y)
                assert same and np.array_equal(y, z, equal_nan=True), f"{name}: chains differ"
            mode_b = ListChainSummary(
                *(s[k] for k in Context._LIST_SUMMARY_KEYS[:12]), int(s["n_pooled"][0]),
                s["n_counted"], s["ic"], s["best_sweep"], [], W, A).mode()
            assert [m.Positions for m in mode_a] == [m.Positions for m in mode_b], \
                f"{name}: modes differ"
            assert np.array_equal(bits([m.PWMS for m in mode_a]), bits([m.PWMS for m in mode_b])), \
                f"{name}: frequencies differ"
            assert np.array_equal(cells_a, s["pooled_counts"]), f"{name}: cells differ"
        med = {k: statistics.median(v) for k, v in ms.items()}
        H = int(mine.occupancy_offsets(W)[-1])
        entry = {"N": N, "L": L, "W": W, "motif_amount": M, "chains": R, "counted": n_counted,
                 "bins_a_chain": H, "slab_bytes": R * (H + N * (M + 1)) * 4,
                 "a_stats_call_parent": spread(ms["a_call"]), "a_host_reduction": spread(ms["a_host"]),
                 "a_total": spread(ms["a"]), "a_stats_call_this_tree": spread(ms["a_call_tree"]),
                 "b_summary_call": spread(ms["b"]),
                 "sweeps_stage_device_ms": {k: spread(v) for k, v in sweeps.items()},
                 "c_plain_parent": spread(ms["c"]),
                 "a_over_b": med["a"] / med["b"], "a_call_alone_over_b": med["a_call"] / med["b"],
                 "summary_cost_ms_b_minus_c": med["b"] - med["c"],
                 "b_slowest_below_a_fastest": max(ms["b"]) < min(ms["a"]),
                 "reduction_device_ms": spread(dev), "modes_and_cells_equal": True}
        rec["shapes"][name] = entry
        print(f"{name}: (a) {med['a']:.2f} = call {med['a_call']:.2f} + host {med['a_host']:.2f}, "
              f"(b) {med['b']:.2f} ({min(ms['b']):.2f} - {max(ms['b']):.2f}), (c) {med['c']:.2f} ms; "
              f"a / b x{entry['a_over_b']:.2f}, b - c {entry['summary_cost_ms_b_minus_c']:.2f} ms; "
              f"reduction {statistics.median(dev):.3f} ms on the device; (a') "
              f"{med['a_call_tree']:.2f} ms; sweeps stage "
              + ", ".join(f"{k} {statistics.median(v):.2f}" for k, v in sweeps.items()),
              file=sys.stderr, flush=True)
        for c in ctxs:
            c.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"a_ms": v["a_total"]["median_ms"], "b_ms": v["b_summary_call"]["median_ms"],
                          "c_ms": v["c_plain_parent"]["median_ms"]}
                      for k, v in rec["shapes"].items()}))


if __name__ == "__main__":
    main()

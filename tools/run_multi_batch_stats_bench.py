"""R chains of T sweeps of Positions lists with their statistics (occupancy, site counts, trace
of the summed PWMS, best state): one gs_motif_run_multi_batch_stats call against what a
caller had to do before it.

    python tools/run_multi_batch_stats_bench.py --loop-lib PATH            # the three shapes
    python tools/run_multi_batch_stats_bench.py --loop-lib PATH --shapes dna200 --choices

The shapes are those of tools/run_multi_batch_bench.py at motifAmount 2.  All sides start from
the same uploaded lists (init_mode -1: the positions of random_starts mode 1 per seed as
one-position lists, computed outside the timed region), T = 20, burn_in = 5, thin = 1:
  (a) one plain gs_motif_run_multi_batch call through the parent commit's build (--loop-lib,
      required), the same call through this tree's library (a'), and as a control through a
      second context of the parent's build (a2: the same code on other slabs);
  (b) one gs_motif_run_multi_batch_stats call through this tree's library;
  (c) T one-sweep gs_motif_run_multi_batch calls through the parent's build, each fed the
      previous lists, with the tally in numpy: bins, site counts, the ordered sum of every
      chain's PWMS row, the first-maximum best state.
Per shape a warm-up of every side, then `--reps` timed repetitions, the sides interleaved (the
plain calls rotating every repetition), wall clock around the call(s) that return host
results; the median counts, the spread (min, max) is recorded, and so is the sweeps stage by
events (gs_run_multi_batch_last_ms) of every single-call side.  Every repetition asserts
(b) == (c) exactly: counts, sweep numbers and lists equal, binary64 values bit for bit.
Reported: (b) - (a), what the statistics cost, and (c) / (b), what the call saves.  --choices
also times (b) under the launch choices of the statistics kernel.
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

from run_batch_stats_bench import bits, ic_rows, source_hash, spread  # noqa: E402
from run_multi_batch_bench import PC, SEED0, SHAPES as LIST_SHAPES, dataset  # noqa: E402

SHAPES = ["fsx407", "dna200", "dna2000"]
T, BURN_IN, THIN = 20, 5, 1
CHOICES = [{"run_stats_blocks": 1, "run_stats_atomic": 1}, {"run_stats_blocks": 1, "run_stats_atomic": 0},
           {"run_stats_blocks": 0, "run_stats_atomic": 1}, {"run_stats_blocks": 0, "run_stats_atomic": 0}]
KEYS = ("occupancy", "sites", "ic", "best_sweep", "best_cnt", "best_pos", "best_pwms")


def stepwise(ctx, M, W, cutoff, seeds, cnt, pos, off):
    """Side (c): T one-sweep calls and the host tally."""
    R, N = cnt.shape
    H = int(off[-1])
    occ = np.zeros(R * H, np.int32)
    sites = np.zeros(R * N * (M + 1), np.int32)
    chain = (np.arange(R, dtype=np.int64) * H)[:, None]
    empty_bin = chain + off[None, :-1]                                   # [R, N]
    site_base = np.arange(R * N, dtype=np.int64).reshape(R, N) * (M + 1)
    ic = np.zeros((R, len(range(BURN_IN, T, THIN))), np.float64)
    best_sweep = np.full(R, -1, np.int64)
    best_ic = np.zeros(R, np.float64)
    best_cnt = np.zeros((R, N), np.int32)
    best_pos = np.full(pos.shape, -1, np.int32)
    best_pwms = np.zeros((R, N), np.float64)
    pwms = None
    for t in range(T):
        cnt, pos, pwms, status = ctx.motif_run_multi_batch(M, W, PC, cutoff, 1, seeds, cnt, pos,
                                                           first_sweep=t)
        assert not status.any(), status
        if t < BURN_IN or (t - BURN_IN) % THIN:
            continue
        # a chain's bins and site counts of one sweep are distinct
        sites[(site_base + cnt).ravel()] += 1
        occ[empty_bin[cnt == 0]] += 1
        held = np.arange(pos.shape[2])[None, None, :] < cnt[:, :, None]
        occ[(empty_bin[:, :, None] + 1 + pos)[held]] += 1
        v = ic_rows(pwms)
        ic[:, (t - BURN_IN) // THIN] = v
        win = (best_sweep < 0) | (v > best_ic)
        best_sweep[win], best_ic[win] = t, v[win]
        best_cnt[win], best_pos[win], best_pwms[win] = cnt[win], pos[win], pwms[win]
    return cnt, pos, pwms, {"occupancy": occ.reshape(R, H), "sites": sites.reshape(R, N, M + 1),
                            "ic": ic, "best_sweep": best_sweep, "best_cnt": best_cnt,
                            "best_pos": best_pos, "best_pwms": best_pwms}


def same(b, c, what):
    for k in KEYS:
        eq = (np.array_equal(bits(b[k]), bits(c[k])) if b[k].dtype == np.float64
              else np.array_equal(b[k], c[k]))
        assert eq, f"{what}: {k} differs"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=SHAPES)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-lib", required=True,
                    help="the parent commit's build of the library: sides (a) and (c)")
    ap.add_argument("--choices", action="store_true",
                    help="also time (b) under the statistics kernel's launch choices")
    ap.add_argument("--out",
                    default=str(ROOT / "profiles" / "batch" / "run_multi_batch_stats_bench.json"))
    args = ap.parse_args()
    from gibbssampling_amd import Context

    rec = {"tool": "tools/run_multi_batch_stats_bench.py", "source_sha256": source_hash(),
           "pc": PC, "reps": args.reps, "sweeps": T, "burn_in": BURN_IN, "thin": THIN,
           "loop_lib": "parent commit's build",
           "starts": "random_starts mode 1 per seed as one-position lists, uploaded (init_mode -1)",
           "shapes": {}}
    for name in args.shapes:
        N, L, W, M, cutoff, R = LIST_SHAPES[name]
        codes, offsets, alpha = dataset(name)
        seeds = [SEED0 + r for r in range(R)]
        # one context a side, so that each plain call's context has seen plain calls only (a
        # second one through the parent's library is the control: the same code on other
        # slabs, (a2))
        parent, parent_step, parent2 = (Context(0, lib_path=args.loop_lib) for _ in range(3))
        mine, mine_stats = Context(0), Context(0)
        ctxs = (parent, parent_step, parent2, mine, mine_stats)
        for c in ctxs:
            c.set_sequences(codes, offsets, alpha)
        off = mine.occupancy_offsets(W)
        cnt0 = np.ones((R, N), np.int32)
        pos0 = np.full((R, N, M), -1, np.int32)
        for r, s in enumerate(seeds):
            pos0[r, :, 0] = parent.random_starts(W, PC, s, 1)[1]

        def plain(ctx):
            return ctx.motif_run_multi_batch(M, W, PC, cutoff, T, seeds, cnt0, pos0)

        def stats(ctx):
            return ctx.motif_run_multi_batch_stats(M, W, PC, cutoff, T, seeds, cnt0, pos0,
                                                   burn_in=BURN_IN, thin=THIN)

        plain(parent), plain(parent2), plain(mine), stats(mine_stats)  # warm-up
        parent_step.motif_run_multi_batch(M, W, PC, cutoff, 1, seeds, cnt0, pos0)
        ms = {k: [] for k in ("a", "a2", "a_tree", "b", "c")}
        dev = {k: [] for k in ("a", "a2", "a_tree", "b")}
        plain_ctx = {"a": parent, "a2": parent2, "a_tree": mine}
        b = None
        for rep in range(args.reps):
            res = {}
            # the plain calls rotate every repetition, so that no side is always the first
            # call after the stepwise side's host waits
            for k in (("a", "a2", "a_tree") * 2)[rep % 3:rep % 3 + 3]:
                ctx = plain_ctx[k]
                t0 = time.perf_counter()
                res[k] = plain(ctx)
                ms[k].append((time.perf_counter() - t0) * 1e3)
                dev[k].append(ctx.run_multi_batch_last_ms()[1])
            t0 = time.perf_counter()
            cnt_b, pos_b, pw_b, st_b, b = stats(mine_stats)
            ms["b"].append((time.perf_counter() - t0) * 1e3)
            dev["b"].append(mine_stats.run_multi_batch_last_ms()[1])
            t0 = time.perf_counter()
            cnt_c, pos_c, pw_c, c = stepwise(parent_step, M, W, cutoff, seeds, cnt0, pos0, off)
            ms["c"].append((time.perf_counter() - t0) * 1e3)
            assert not st_b.any(), st_b
            same(b, c, name)
            for q in (res["a"], res["a_tree"], (cnt_c, pos_c, pw_c)):
                assert np.array_equal(cnt_b, q[0]) and np.array_equal(pos_b, q[1]), name
                assert np.array_equal(bits(pw_b), bits(q[2])), name
        med = {k: statistics.median(v) for k, v in ms.items()}
        entry = {"N": N, "L": L, "W": W, "motif_amount": M, "cutoff": cutoff, "chains": R,
                 "bins_per_chain": int(off[-1]),
                 "a_plain_parent": spread(ms["a"]), "a_plain_this_tree": spread(ms["a_tree"]),
                 "a2_plain_parent_second_context": spread(ms["a2"]),
                 "b_stats_call": spread(ms["b"]), "c_stepwise_numpy": spread(ms["c"]),
                 "a_parent_sweeps_device_ms": spread(dev["a"]),
                 "a2_parent_second_context_sweeps_device_ms": spread(dev["a2"]),
                 "a_this_tree_sweeps_device_ms": spread(dev["a_tree"]),
                 "b_sweeps_device_ms": spread(dev["b"]),
                 "stats_cost_ms_b_minus_a": med["b"] - med["a"],
                 "saving_c_over_b": med["c"] / med["b"],
                 "b_slowest_below_c_fastest": max(ms["b"]) < min(ms["c"]),
                 # against the parent's runs of both its contexts: wall clock, device stage
                 "plain_this_tree_within_parent_spread":
                     min(ms["a"] + ms["a2"]) <= med["a_tree"] <= max(ms["a"] + ms["a2"]),
                 "plain_this_tree_device_within_parent_spread":
                     min(dev["a"] + dev["a2"]) <= statistics.median(dev["a_tree"])
                     <= max(dev["a"] + dev["a2"]),
                 "b_equals_c": True}
        if args.choices:
            entry["launch_choices"] = []
            for tuning in CHOICES:
                ctx = Context(0, tuning=tuning)
                ctx.set_sequences(codes, offsets, alpha)
                stats(ctx)
                wall, sweeps = [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    out = stats(ctx)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    sweeps.append(ctx.run_multi_batch_last_ms()[1])
                    same(out[4], b, f"{name} {tuning}")
                ctx.close()
                entry["launch_choices"].append({"tuning": tuning, "wall": spread(wall),
                                                "sweeps_device_ms": spread(sweeps)})
                print(f"  {tuning}: {statistics.median(wall):.2f} ms, sweeps stage "
                      f"{statistics.median(sweeps):.2f} ms", file=sys.stderr, flush=True)
        rec["shapes"][name] = entry
        print(f"{name}: " + ", ".join(
            f"({k}) {med[k]:.2f} ({min(ms[k]):.2f} - {max(ms[k]):.2f})" for k in ms) +
              f" ms; b - a {med['b'] - med['a']:.2f} ms, c / b x{med['c'] / med['b']:.2f}; sweeps "
              "stage " + ", ".join(f"({k}) {statistics.median(v):.2f}" for k, v in dev.items()),
              file=sys.stderr, flush=True)
        for c in ctxs:
            c.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {"a_ms": v["a_plain_parent"]["median_ms"],
                          "b_ms": v["b_stats_call"]["median_ms"],
                          "c_ms": v["c_stepwise_numpy"]["median_ms"],
                          "c_over_b": v["saving_c_over_b"]} for k, v in rec["shapes"].items()}))


if __name__ == "__main__":
    main()

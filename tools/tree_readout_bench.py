#!/usr/bin/env python3
"""Time of reading search trees back (gaz_engine_read_trees / gaz_engine_read_pv) on the two shapes they were built for:

  gomoku_64_trees     64 Gomoku games (hash evaluator), one 695-iteration move, then read_trees over all 64 slots (both calls: count + fill)
  connect4_4096_trees 4096 Connect4 games, one 200-iteration move, then read_trees over all 4096 slots
  connect4_4096_pvs   principal_variations(16) of those 4096 games

Protocol: one warm-up call, then --repeats (5) timed calls each (host wall clock around the whole Python call: both C calls, the device
walks, the copies to the host and the split into SearchTree objects); median and range in milliseconds, with the size of what came back.
Writes profiles/tree_readout_times.json.

usage: python tools/tree_readout_bench.py [--repeats 5] [--out profiles/tree_readout_times.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, repeats):
    out = fn()                                          # warm-up
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter(); out = fn(); ms.append((time.perf_counter() - t0) * 1e3)
    return out, dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), repeats=repeats, all_ms=ms)


def searched_engine(game, n_games, iters, max_actions, alpha):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine(game, n_games, iters, max_actions, 0, 0, 2.5, alpha, seed=11, hash_salt=3, sync_moves=True, single_tree=True, ring_capacity=0, tau=0.0)
    eng.start_search(); eng.run_move()
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tree_readout_times.json"))
    args = ap.parse_args()
    res = {"protocol": f"one warm-up call, then {args.repeats} timed calls; host wall clock of the whole Python call, milliseconds"}
    eng = searched_engine("Gomoku", 64, 695, 225, 0.05)
    trees, t = timed(lambda: eng.read_trees(range(64)), args.repeats)
    res["gomoku_64_trees"] = dict(t, nodes=sum(len(x) for x in trees), edges=sum(len(x.edges) for x in trees), config="64 Gomoku games, hash evaluator, after one 695-iteration move")
    eng.close()
    eng = searched_engine("Connect4", 4096, 200, 42, 0.5)
    trees, t = timed(lambda: eng.read_trees(range(4096)), args.repeats)
    res["connect4_4096_trees"] = dict(t, nodes=sum(len(x) for x in trees), edges=sum(len(x.edges) for x in trees), config="4096 Connect4 games, hash evaluator, after one 200-iteration move")
    chosen = eng.root_stats()["chosen"]
    pv, t = timed(lambda: eng.principal_variations(16, first_action=chosen), args.repeats)
    res["connect4_4096_pvs"] = dict(t, mean_len=float(pv["len"].mean()), max_len=16, config="principal_variations(16) of the same 4096 games")
    eng.close()
    for k, v in res.items():
        print(json.dumps({k: v}))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

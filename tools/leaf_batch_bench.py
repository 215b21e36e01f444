#!/usr/bin/env python3
"""Time per move of a deep search of few games, by gaz_engine_config.leaf_batch: SelfPlayEngine in sync mode with the ResNet
evaluator, `--iterations` simulations per move, K in --leaf-batch, --games games at once.  K = 1 is the search without leaf batching.

Per configuration: one engine; a warm-up pass over the timed moves (every launch shape loaded), then --repeats passes of --moves
moves from the empty board, each timed with the host clock around run_move (which ends in a device synchronise).  Reported: median and
min / max ms per move over all timed moves, and launches per move (stats()["waves"]: run_move looks at the games every 4 launches with
leaf batching, every 16 without, so the count is rounded up to that).  One JSON line per configuration; --out writes the list.

    python tools/leaf_batch_bench.py --out profiles/leaf_batch_time_per_move.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"gomoku": ("Gomoku", 10, 225, 4.5, 0.05), "connect4": ("Connect4", 6, 42, 2.5, 0.5)}


def measure(workload, n_games, K, iterations, moves, repeats, seed=11):
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
    from grok_alpha_zero_amd.net import NETS
    game, blocks, max_actions, c_init, alpha = WORKLOADS[workload]
    eng = SelfPlayEngine(game, n_games, iterations, max_actions, 0, 0, c_init, alpha, seed=seed, evaluator=EVAL_RESNET, net_blocks=blocks,
                         net_filters=128, sync_moves=True, single_tree=True, ring_capacity=0, tau=0.0, leaf_batch=K)
    eng.load_weights(NETS[game](blocks, seed=0).eval().export_engine_weights())
    ms, waves = [], []
    for rep in range(repeats + 1):                  # pass 0 = warm-up
        eng.reset_games()
        for _ in range(moves):
            w0 = eng.stats()["waves"]
            eng.start_search()
            t0 = time.perf_counter()
            eng.run_move()
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                ms.append(dt); waves.append(eng.stats()["waves"] - w0)
            eng.apply_moves()
    eng.close()
    return dict(workload=workload, game=game, net_blocks=blocks, n_games=n_games, leaf_batch=K, iterations=iterations, moves_timed=len(ms),
                ms_per_move_median=round(statistics.median(ms), 3), ms_per_move_min=round(min(ms), 3), ms_per_move_max=round(max(ms), 3),
                launches_per_move_median=statistics.median(waves))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="gomoku,connect4")
    ap.add_argument("--games", default="1,16")
    ap.add_argument("--leaf-batch", default="1,8,16,32,64")
    ap.add_argument("--iterations", type=int, default=800)
    ap.add_argument("--moves", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for wl in a.workloads.split(","):
        for g in (int(x) for x in a.games.split(",")):
            for K in (int(x) for x in a.leaf_batch.split(",")):
                rows.append(measure(wl, g, K, a.iterations, a.moves, a.repeats))
                print(json.dumps(rows[-1]), flush=True)
                if a.out:
                    json.dump(rows, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Time per move of the Gumbel search of few games, by gaz_engine_config.gumbel_batch: SelfPlayEngine in sync mode with the ResNet
evaluator (raw-logit policy head), K in --gumbel-batch, --games games at once.  K = 1 is one candidate of sequential halving per game
and wave; every K plays the same moves bit for bit, so only the time and the launches differ.

Workloads: Gomoku 10 blocks x 128 at n = 400, m = 16; Connect4 6 blocks x 128 at n = 200, m = 16 (seven legal moves: m is 7 there).

Per configuration: one engine; a warm-up pass over the timed moves (every launch shape loaded), then --repeats passes of --moves
moves from the empty board, each timed with the host clock around run_move (which ends in a device synchronise).  Reported: median and
min / max ms per move over all timed moves, and launches per move (stats()["waves"]: run_move looks at the games every 4 launches with
gumbel_batch > 1, every 16 without, so the count is rounded up to that).  One JSON line per configuration; --out writes the list.

    python tools/gumbel_batch_bench.py --out profiles/gumbel_batch_time_per_move.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"gomoku": ("Gomoku", 10, 225, 400, 16), "connect4": ("Connect4", 6, 42, 200, 16)}   # game, blocks, max_actions, n, m


def measure(workload, n_games, K, moves, repeats, seed=11):
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SEARCH_GUMBEL, SelfPlayEngine
    from grok_alpha_zero_amd.net import NETS
    game, blocks, max_actions, iterations, m = WORKLOADS[workload]
    eng = SelfPlayEngine(game, n_games, iterations, max_actions, 0, 0, 0.0, 0.0, seed=seed, evaluator=EVAL_RESNET, net_blocks=blocks, net_filters=128,
                         policy_is_logits=1, sync_moves=True, ring_capacity=0, search=SEARCH_GUMBEL, gumbel_m=m, c_visit=50.0, c_scale=1.0, gumbel_batch=K)
    eng.load_weights(NETS[game](blocks, seed=0).eval().export_engine_weights())
    ms, waves, chosen = [], [], []
    for rep in range(repeats + 1):                  # pass 0 = warm-up
        eng.reset_games()
        for _ in range(moves):
            w0 = eng.stats()["waves"]
            t0 = time.perf_counter()
            eng.run_move()
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                ms.append(dt); waves.append(eng.stats()["waves"] - w0)
            if rep == 1:
                chosen.append([int(c) for c in eng.root_stats()["chosen"]])
            eng.apply_moves()
    eng.close()
    return dict(workload=workload, game=game, net_blocks=blocks, n_games=n_games, gumbel_batch=K, iterations=iterations, m=m, moves_timed=len(ms),
                ms_per_move_median=round(statistics.median(ms), 3), ms_per_move_min=round(min(ms), 3), ms_per_move_max=round(max(ms), 3),
                launches_per_move_median=statistics.median(waves), moves_played=chosen)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="gomoku,connect4")
    ap.add_argument("--games", default="1,16")
    ap.add_argument("--gumbel-batch", default="1,4,16")
    ap.add_argument("--moves", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for wl in a.workloads.split(","):
        for g in (int(x) for x in a.games.split(",")):
            for K in (int(x) for x in a.gumbel_batch.split(",")):
                rows.append(measure(wl, g, K, a.moves, a.repeats))
                print(json.dumps(rows[-1]), flush=True)
                if a.out:
                    json.dump(rows, open(a.out, "w"), indent=1)
            played = {json.dumps(r["moves_played"]) for r in rows if r["workload"] == wl and r["n_games"] == g}
            if len(played) != 1:
                print(f"{wl}, {g} games: the moves differ between the gumbel_batch values", file=sys.stderr)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Rates of continuous self-play with and without playout cap randomisation (gaz_engine_config.fast_iterations / full_search_prob), on
the headline configuration: Connect4, 4096 games, the 6-block x 128 network, run_iterations = 300 (Self_Play's int(1.5 x 200)).

Two engines in one process — cap off, and full_search_prob = 0.25 with fast_iterations = 50 — each burnt in to its own stationary ply
mix, then timed ALTERNATELY, --rounds times each, on the same box (the order of the two swaps every round).  A timed segment is
--segments x --waves launches with the finished games drained as training samples (drain_samples: the path run_self_play takes)
between them, bracketed by a device synchronise and the host clock.  Both engines (2 x --games games, each with its own copy of the network)
stay alive for the whole run, so the two settings share the device's memory and clocks; only one of them launches at a time.
Reported per setting, as the median over the rounds and per round:
    plies_per_s         plies played (positions searched) per second, fast and full
    rows_per_s          training sample rows handed out per second (plies of finished games that were searched at the full limit)
    sims_per_move       simulations / plies of the segment
    evals_per_ply       evaluator calls / plies of the segment
    full_fraction       rows / plies of the games drained in the segment
No figure is a threshold; the tool measures.  One JSON object; --out writes it.

    python tools/playout_cap_bench.py --out profiles/playout_cap_rates.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = {"cap_off": dict(fast_iterations=0, full_search_prob=0.0), "cap_on": dict(fast_iterations=50, full_search_prob=0.25)}


def make_engine(a, weights, cap):
    from grok_alpha_zero_amd.engine import EVAL_HASH, EVAL_RESNET, SelfPlayEngine
    net = a.evaluator == "resnet"
    eng = SelfPlayEngine("Connect4", a.games, a.iterations, 42, 8, 7, 2.5, 0.5, seed=1234, evaluator=EVAL_RESNET if net else EVAL_HASH, hash_salt=7,
                         net_blocks=a.blocks if net else 0, ring_capacity=2 * a.games, lib_path=a.emu_lib or None, **cap)
    if net:
        eng.load_weights(weights)
    return eng


def drain(eng):
    b = eng.drain_samples()
    return int(b.games[:, 0].sum()), int(b.rows)


def segment(eng, a):
    """-> dict of the counters' deltas over --segments x --waves launches, and the seconds they took"""
    eng.synchronize(); drain(eng)
    s0, plies_done, rows, t0 = eng.stats(), 0, 0, time.perf_counter()
    for _ in range(a.segments):
        eng.run_waves(a.waves)
        eng.synchronize()
        p, r = drain(eng)
        plies_done += p; rows += r
    dt = time.perf_counter() - t0
    s1 = eng.stats()
    plies = s1["plies"] - s0["plies"]
    return dict(seconds=round(dt, 4), plies=plies, rows=rows, plies_per_s=plies / dt, rows_per_s=rows / dt, sims_per_move=(s1["sims"] - s0["sims"]) / max(plies, 1),
                evals_per_ply=(s1["evals"] - s0["evals"]) / max(plies, 1), full_fraction=rows / max(plies_done, 1), games_drained_plies=plies_done)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--burn-in-waves", type=int, default=12000, help="untimed launches per engine before the first timed segment (about two game lengths with the cap off)")
    ap.add_argument("--waves", type=int, default=400)
    ap.add_argument("--segments", type=int, default=10, help="timed launches per round = segments x waves")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--evaluator", default="resnet", choices=["resnet", "hash"])
    ap.add_argument("--emu-lib", default="", help="rehearsal on the one-lane CPU emulation build (hash evaluator, tiny sizes): no rate it prints means anything")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    weights = None
    if a.evaluator == "resnet":
        from grok_alpha_zero_amd.net import NETS
        weights = NETS["Connect4"](a.blocks, seed=0).eval().export_engine_weights()
    engines = {k: make_engine(a, weights, cap) for k, cap in SETTINGS.items()}
    for k, eng in engines.items():
        for i in range(0, a.burn_in_waves, 500):
            eng.run_waves(min(500, a.burn_in_waves - i)); eng.synchronize(); drain(eng)
    rounds = {k: [] for k in engines}
    for r in range(a.rounds):
        for k in (list(engines) if r % 2 == 0 else list(engines)[::-1]):
            rounds[k].append(segment(engines[k], a))
            print(json.dumps(dict(round=r, setting=k, **rounds[k][-1])), file=sys.stderr, flush=True)
    out = dict(what="tools/playout_cap_bench.py: continuous Connect4 self-play, cap off vs cap on, alternated on one box", games=a.games, run_iterations=a.iterations,
               net_blocks=a.blocks if a.evaluator == "resnet" else 0, evaluator=a.evaluator, burn_in_waves=a.burn_in_waves, waves_per_round=a.waves * a.segments,
               rounds=a.rounds, game_groups={k: e.stats()["game_groups"] for k, e in engines.items()}, fused_wave={k: e.stats()["fused_wave"] for k, e in engines.items()},
               settings={})
    for k, eng in engines.items():
        med = {f: statistics.median(x[f] for x in rounds[k]) for f in ("plies_per_s", "rows_per_s", "sims_per_move", "evals_per_ply", "full_fraction")}
        out["settings"][k] = dict(SETTINGS[k], median=med, per_round=rounds[k])
        eng.close()
    off, on = out["settings"]["cap_off"]["median"], out["settings"]["cap_on"]["median"]
    out["cap_on_over_cap_off"] = {f: on[f] / off[f] for f in ("plies_per_s", "rows_per_s", "sims_per_move", "evals_per_ply")}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

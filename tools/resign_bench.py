#!/usr/bin/env python3
"""Rates of continuous self-play with resignation off and on (SelfPlayEngine.set_resignation), on the headline configuration: Connect4,
4096 games, the 6-block x 128 network, run_iterations = 300 (Self_Play's int(1.5 x 200)).

ONE engine per process, the processes alternated (off, on, off, on ... --rounds times each, one at a time, the order of the two swapping
every round), as tools/ab_lib.sh alternates two builds: with both engines in one process the engine created second ran a quarter slower
whatever its setting, which measured the position and not the feature.  Every child (this file with --setting) creates its engine, burns
it in to its stationary ply mix, then times --segments x --waves launches with the finished games drained as records between them,
bracketed by a device synchronise and the host clock, and prints one JSON line.  Reported per setting, as the median over its processes
and per process:
    plies_per_s           plies played (positions searched) per second
    games_per_s           games finished per second
    mean_game_length      plies per game of the games drained in the segment
    resigned_share        games ended by resignation / games drained
    false_positive_rate   of the play-out games with a would-have-resigned ply that finished in the segment, the share whose would-be
                          resigner drew or won (resign_stats() deltas; 0 when there was none)
    evals_per_ply         evaluator calls / plies of the segment
The network has RANDOM weights: its q carries no game knowledge, so the shares and the false-positive rate say nothing about a trained
network.  Only the rates and the cost of the check are measured.  No figure is a threshold.  One JSON object; --out writes it.

    python tools/resign_bench.py --out profiles/resign_rates.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = {"off": dict(), "on": dict(resign_threshold=0.9, resign_consecutive=2, resign_min_ply=0, no_resign_prob=0.1)}
FIELDS = ("plies_per_s", "games_per_s", "mean_game_length", "resigned_share", "false_positive_rate", "evals_per_ply")


def make_engine(a, weights, kw):
    from grok_alpha_zero_amd.engine import EVAL_HASH, EVAL_RESNET, SelfPlayEngine
    net = a.evaluator == "resnet"
    eng = SelfPlayEngine("Connect4", a.games, a.iterations, 42, 8, 7, 2.5, 0.5, seed=1234, evaluator=EVAL_RESNET if net else EVAL_HASH, hash_salt=7,
                         net_blocks=a.blocks if net else 0, ring_capacity=2 * a.games, lib_path=a.emu_lib or None, **kw)
    if net:
        eng.load_weights(weights)
    return eng


def segment(eng, a):
    """-> dict of the counters' deltas over --segments x --waves launches, and the seconds they took"""
    eng.synchronize(); eng.drain_finished()
    s0, r0, recs, t0 = eng.stats(), eng.resign_stats(), [], time.perf_counter()
    for _ in range(a.segments):
        eng.run_waves(a.waves)
        eng.synchronize()
        recs += eng.drain_finished()
    dt = time.perf_counter() - t0
    s1, r1 = eng.stats(), eng.resign_stats()
    plies = s1["plies"] - s0["plies"]
    would = r1["would_resign"] - r0["would_resign"]
    return dict(seconds=round(dt, 4), plies=plies, games_drained=len(recs), plies_per_s=plies / dt, games_per_s=len(recs) / dt,
                mean_game_length=sum(r["T"] for r in recs) / max(len(recs), 1), resigned_share=sum(r["resigned"] for r in recs) / max(len(recs), 1),
                playout_games=r1["playout_games"] - r0["playout_games"], would_resign=would,
                false_positive_rate=(r1["false_positives"] - r0["false_positives"]) / would if would else 0.0,
                evals_per_ply=(s1["evals"] - s0["evals"]) / max(plies, 1))


def child(a):
    """one engine, one setting: burn in, time one segment, print its figures"""
    weights = None
    if a.evaluator == "resnet":
        from grok_alpha_zero_amd.net import NETS
        weights = NETS["Connect4"](a.blocks, seed=0).eval().export_engine_weights()
    eng = make_engine(a, weights, SETTINGS[a.setting])
    for i in range(0, a.burn_in_waves, 500):
        eng.run_waves(min(500, a.burn_in_waves - i)); eng.synchronize(); eng.drain_finished()
    out = segment(eng, a)
    st = eng.stats()
    out.update(game_groups=st["game_groups"], fused_wave=st["fused_wave"], resign_stats=eng.resign_stats())
    eng.close()
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--burn-in-waves", type=int, default=12000, help="untimed launches before the timed segment (about two game lengths)")
    ap.add_argument("--waves", type=int, default=400)
    ap.add_argument("--segments", type=int, default=10, help="timed launches per process = segments x waves")
    ap.add_argument("--rounds", type=int, default=3, help="processes per setting")
    ap.add_argument("--evaluator", default="resnet", choices=["resnet", "hash"])
    ap.add_argument("--emu-lib", default="", help="rehearsal on the one-lane CPU emulation build (hash evaluator, tiny sizes): no rate it prints means anything")
    ap.add_argument("--setting", default="", choices=["", "off", "on"], help="(the child processes) measure this one setting and print its figures")
    ap.add_argument("--child-timeout", type=float, default=150.0, help="seconds a child process may take; after one that failed or ran out of time none is started")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.setting:
        return child(a)
    rounds = {k: [] for k in SETTINGS}
    passed = [x for x in sys.argv[1:]]
    if "--out" in passed:
        i = passed.index("--out"); del passed[i:i + 2]
    for r in range(a.rounds):
        for k in (list(SETTINGS) if r % 2 == 0 else list(SETTINGS)[::-1]):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--setting", k] + passed, capture_output=True, text=True, timeout=a.child_timeout)
            if p.returncode != 0:
                print(p.stderr[-2000:], file=sys.stderr)
                return 1
            rounds[k].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(dict(round=r, setting=k, **rounds[k][-1])), file=sys.stderr, flush=True)
    out = dict(what="tools/resign_bench.py: continuous Connect4 self-play, resignation off vs on (threshold 0.9, consecutive 2, no_resign_prob 0.1), one engine per process, "
                    "the processes alternated on one box",
               note="random network weights: q carries no game knowledge, so resigned_share and false_positive_rate say nothing about a trained network; "
                    "only the rates and the cost of the check are measured",
               games=a.games, run_iterations=a.iterations, net_blocks=a.blocks if a.evaluator == "resnet" else 0, evaluator=a.evaluator, burn_in_waves=a.burn_in_waves,
               waves_per_process=a.waves * a.segments, processes_per_setting=a.rounds, settings={})
    for k in SETTINGS:
        med = {f: statistics.median(x[f] for x in rounds[k]) for f in FIELDS}
        out["settings"][k] = dict(SETTINGS[k], median=med, per_process=rounds[k])
    off, on = out["settings"]["off"]["median"], out["settings"]["on"]["median"]
    out["on_over_off"] = {f: on[f] / off[f] for f in ("plies_per_s", "games_per_s", "mean_game_length", "evals_per_ply")}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Rates of continuous self-play with the search's random evaluation symmetry off and on (SelfPlayEngine.set_eval_symmetry), on two
configurations of Connect4 with 4096 games, the 6-block x 128 network and run_iterations = 300 (Self_Play's int(1.5 x 200)):
    headline   the fused tree + trunk launch, no evaluation cache
    cache      eval_cache_log2 = 20 (separate launches)

ONE engine per process, the processes alternated (off, on, off, on ... --rounds times each per configuration, one at a time, the order of
the two swapping every round), as tools/ab_lib.sh alternates two builds.  Every child (this file with --setting) creates its engine, burns
it in to its stationary ply mix, then times --segments x --waves launches with the finished games drained as records between them,
bracketed by a device synchronise and the host clock, and prints one JSON line.  Reported per configuration and setting, as the median
over its processes and per process:
    plies_per_s           plies played (positions searched) per second
    evals_per_ply         evaluator requests / plies of the segment (cache hits included)
    cache_hit_rate        requests answered by the evaluation cache / requests (0 without a cache)
    mean_game_length      plies per game of the games drained in the segment
The symmetry is part of the cache key's row — and its draw is keyed by the game —, so across games the hit rate is expected to fall with it
on; it is reported beside the off figure and no bar is set on it.  The network has RANDOM weights.  No figure is a threshold.  One JSON
object; --out writes it.

    python tools/eval_symmetry_bench.py --out profiles/eval_symmetry_rates.json
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

SETTINGS = {"off": dict(), "on": dict(eval_symmetry=True)}
CONFIGS = {"headline": dict(), "cache": dict(eval_cache_log2=20)}
FIELDS = ("plies_per_s", "evals_per_ply", "cache_hit_rate", "mean_game_length")


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
    s0, recs, t0 = eng.stats(), [], time.perf_counter()
    for _ in range(a.segments):
        eng.run_waves(a.waves)
        eng.synchronize()
        recs += eng.drain_finished()
    dt = time.perf_counter() - t0
    s1 = eng.stats()
    plies, evals = s1["plies"] - s0["plies"], s1["evals"] - s0["evals"]
    return dict(seconds=round(dt, 4), plies=plies, games_drained=len(recs), plies_per_s=plies / dt,
                mean_game_length=sum(r["T"] for r in recs) / max(len(recs), 1),
                evals_per_ply=evals / max(plies, 1), cache_hit_rate=(s1["cache_hits"] - s0["cache_hits"]) / max(evals, 1))


def child(a):
    """one engine, one configuration, one setting: burn in, time one segment, print its figures"""
    weights = None
    if a.evaluator == "resnet":
        from grok_alpha_zero_amd.net import NETS
        weights = NETS["Connect4"](a.blocks, seed=0).eval().export_engine_weights()
    eng = make_engine(a, weights, dict(CONFIGS[a.config], **SETTINGS[a.setting]))
    assert eng.eval_symmetry == (a.setting == "on")
    for i in range(0, a.burn_in_waves, 500):
        eng.run_waves(min(500, a.burn_in_waves - i)); eng.synchronize(); eng.drain_finished()
    out = segment(eng, a)
    st = eng.stats()
    out.update(game_groups=st["game_groups"], fused_wave=st["fused_wave"])
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
    ap.add_argument("--rounds", type=int, default=3, help="processes per configuration and setting")
    ap.add_argument("--configs", default="headline,cache")
    ap.add_argument("--evaluator", default="resnet", choices=["resnet", "hash"])
    ap.add_argument("--emu-lib", default="", help="rehearsal on the one-lane CPU emulation build (hash evaluator, tiny sizes): no rate it prints means anything")
    ap.add_argument("--setting", default="", choices=["", "off", "on"], help="(the child processes) measure this one setting and print its figures")
    ap.add_argument("--config", default="headline", choices=sorted(CONFIGS), help="(the child processes) the configuration")
    ap.add_argument("--child-timeout", type=float, default=150.0, help="seconds a child process may take; after one that failed or ran out of time none is started")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.setting:
        return child(a)
    passed = [x for x in sys.argv[1:]]
    for flag in ("--out", "--configs"):
        if flag in passed:
            i = passed.index(flag); del passed[i:i + 2]
    out = dict(what="tools/eval_symmetry_bench.py: continuous Connect4 self-play, random evaluation symmetry off vs on, one engine per process, the processes "
                    "alternated on one box",
               note="random network weights; the evaluation cache's hit rate is expected to fall with the symmetry on (the draw is keyed by the game): reported, no bar",
               games=a.games, run_iterations=a.iterations, net_blocks=a.blocks if a.evaluator == "resnet" else 0, evaluator=a.evaluator, burn_in_waves=a.burn_in_waves,
               waves_per_process=a.waves * a.segments, processes_per_setting=a.rounds, configs={})
    for cfg in a.configs.split(","):
        rounds = {k: [] for k in SETTINGS}
        for r in range(a.rounds):
            for k in (list(SETTINGS) if r % 2 == 0 else list(SETTINGS)[::-1]):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--setting", k, "--config", cfg] + passed, capture_output=True, text=True, timeout=a.child_timeout)
                if p.returncode != 0:
                    print(p.stderr[-2000:], file=sys.stderr)
                    return 1
                rounds[k].append(json.loads(p.stdout.strip().splitlines()[-1]))
                print(json.dumps(dict(config=cfg, round=r, setting=k, **rounds[k][-1])), file=sys.stderr, flush=True)
        res = {k: dict(median={f: statistics.median(x[f] for x in rounds[k]) for f in FIELDS}, per_process=rounds[k]) for k in SETTINGS}
        off, on = res["off"]["median"], res["on"]["median"]
        res["on_over_off"] = {f: on[f] / off[f] for f in FIELDS if off[f]}
        out["configs"][cfg] = dict(engine=CONFIGS[cfg], **res)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What match play costs (SelfPlayEngine.set_match): Connect4, the 6-block x 128 network, run_iterations = 200, at 512
and 4096 slots.  Two settings of the SAME engine shape — game_groups = 1 and set_fused_wave(0), the launches match play runs — are compared:
    off     match off: one evaluator pass over all rows per wave
    match   match on with network B = network A's weights: route + partition + copy, the host's wait for the two row counts, two evaluator
            passes over the rows that carry a request, scatter
ONE engine per process, the processes alternated (off, match, off, match ... --rounds times each per slot count, one at a time on one box, the
order swapping every round).  Every child (this file with --setting) runs under `timeout -k 10`, and after one that failed or ran out of
time none is started.  A child burns its engine in to a stationary ply mix, times --segments x --waves launches with the finished games
drained between them (device synchronise + host clock), then brackets a short stretch with HIP events for the per-wave times.  Reported per
slot count and setting, as the median over its processes and per process:
    positions_per_s, games_per_s     plies played / games finished per second
    ms_tree, ms_eval                 per bracketed wave: the tree step; everything from its end to the end of the wave's evaluator work
    (match) ms_route_copy, ms_sync_gap, ms_scatter, ms_host_wait     SelfPlayEngine.match_timing(), per bracketed wave
The network has RANDOM weights.  No figure is a threshold: nobody had measured the ratio, and the file records it next to the baseline it was
measured against.  One JSON object; --out writes it.

    python tools/match_bench.py --out profiles/match_rates.json
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

SETTINGS = ("off", "match")
FIELDS = ("positions_per_s", "games_per_s", "ms_tree", "ms_eval", "ms_route_copy", "ms_sync_gap", "ms_scatter", "ms_host_wait")


def child(a):
    from grok_alpha_zero_amd.engine import EVAL_HASH, EVAL_RESNET, SelfPlayEngine
    net = a.evaluator == "resnet"
    eng = SelfPlayEngine("Connect4", a.slots, a.iterations, 42, 8, 7, 2.5, 0.5, seed=1234, evaluator=EVAL_RESNET if net else EVAL_HASH, hash_salt=7,
                         net_blocks=a.blocks if net else 0, ring_capacity=2 * a.slots, game_groups=1, lib_path=a.emu_lib or None)
    eng.set_fused_wave(False)
    if net:
        from grok_alpha_zero_amd.net import NETS
        w = NETS["Connect4"](a.blocks, seed=0).eval().export_engine_weights()
        eng.load_weights(w)
        if a.setting == "match":
            eng.load_weights_b(w)
    if a.setting == "match":
        eng.set_match(True, hash_salt_b=7)
    for i in range(0, a.burn_in_waves, 500):
        eng.run_waves(min(500, a.burn_in_waves - i)); eng.synchronize(); eng.drain_finished()
    eng.synchronize(); eng.drain_finished()
    s0, games, t0 = eng.stats(), 0, time.perf_counter()
    for _ in range(a.segments):
        eng.run_waves(a.waves)
        eng.synchronize()
        games += len(eng.drain_finished())
    dt = time.perf_counter() - t0
    s1 = eng.stats()
    out = dict(seconds=round(dt, 4), positions_per_s=(s1["plies"] - s0["plies"]) / dt, games_per_s=games / dt, evals_per_wave=(s1["evals"] - s0["evals"]) / (a.segments * a.waves),
               fused_wave=s1["fused_wave"], game_groups=s1["game_groups"])
    eng.timing_reset(True)                           # the per-wave times, on a stretch of their own (an event record is a packet on the stream)
    eng.run_waves(a.timed_waves); eng.synchronize()
    t = eng.timing()
    n = max(t["n_waves"], 1)
    out.update(ms_tree=t["ms_tree"] / n, ms_eval=t["ms_eval"] / n, waves_bracketed=t["n_waves"])
    mt = eng.match_timing()
    out.update({k: (mt[k] if a.setting == "match" else 0.0) for k in ("ms_route_copy", "ms_sync_gap", "ms_scatter", "ms_host_wait")})
    out["match_stats"] = eng.match_stats()
    eng.close()
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slot-counts", default="512,4096")
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--burn-in-waves", type=int, default=8000, help="untimed launches before the timed segment (about two game lengths)")
    ap.add_argument("--waves", type=int, default=400)
    ap.add_argument("--segments", type=int, default=5, help="timed launches per process = segments x waves")
    ap.add_argument("--timed-waves", type=int, default=800, help="launches of the bracketed stretch (every 8th is bracketed)")
    ap.add_argument("--rounds", type=int, default=2, help="processes per slot count and setting")
    ap.add_argument("--evaluator", default="resnet", choices=["resnet", "hash"])
    ap.add_argument("--emu-lib", default="", help="rehearsal on the one-lane CPU emulation build (hash evaluator, tiny sizes): no rate it prints means anything")
    ap.add_argument("--setting", default="", choices=["", "off", "match"], help="(the child processes) measure this one setting and print its figures")
    ap.add_argument("--slots", type=int, default=4096, help="(the child processes) the slot count")
    ap.add_argument("--child-timeout", type=int, default=150, help="seconds a child process may take; after one that failed or ran out of time none is started")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.setting:
        return child(a)
    passed = list(sys.argv[1:])
    for flag in ("--out", "--slot-counts"):
        if flag in passed:
            i = passed.index(flag); del passed[i:i + 2]
    out = dict(what="tools/match_bench.py: continuous Connect4 self-play, match play (network B = network A's weights) against the same engine with match off, "
                    "separate launches (set_fused_wave(0)) and game_groups = 1; one engine per process, the processes alternated on one box",
               note="random network weights; no figure is a threshold", run_iterations=a.iterations, net_blocks=a.blocks if a.evaluator == "resnet" else 0,
               evaluator=a.evaluator, burn_in_waves=a.burn_in_waves, waves_per_process=a.waves * a.segments, processes_per_setting=a.rounds, slots={})
    for slots in (int(x) for x in a.slot_counts.split(",")):
        rounds = {k: [] for k in SETTINGS}
        for r in range(a.rounds):
            for k in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
                p = subprocess.run(["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--setting", k, "--slots", str(slots)] + passed,
                                   capture_output=True, text=True)
                if p.returncode != 0:                # failed, or killed at its time limit (124 / 137): nothing more is started
                    print(f"child {k} at {slots} slots: exit status {p.returncode}\n{p.stderr[-2000:]}", file=sys.stderr)
                    return 1
                rounds[k].append(json.loads(p.stdout.strip().splitlines()[-1]))
                print(json.dumps(dict(slots=slots, round=r, setting=k, **rounds[k][-1])), file=sys.stderr, flush=True)
        res = {k: dict(median={f: statistics.median(x[f] for x in rounds[k]) for f in FIELDS}, per_process=rounds[k]) for k in SETTINGS}
        off, on = res["off"]["median"], res["match"]["median"]
        res["match_over_off"] = {f: on[f] / off[f] for f in ("positions_per_s", "games_per_s", "ms_tree", "ms_eval") if off[f]}
        out["slots"][str(slots)] = res
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

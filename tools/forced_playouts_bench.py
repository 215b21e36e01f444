#!/usr/bin/env python3
"""Rates of continuous self-play with and without forced playouts and policy target pruning (gaz_engine_config.forced_playouts_k), on
the headline configuration: Connect4, 4096 games, the 6-block x 128 network, run_iterations = 300 (Self_Play's int(1.5 x 200)).

Two engines in one process — k = 0 and k = 2 (KataGo's value) — each burnt in to its own stationary ply mix, then timed ALTERNATELY,
--rounds times each, on the same box (the order of the two swaps every round).  A timed segment is --segments x --waves launches with
the finished games drained as records (drain_finished: the pruned share is computed from them) between them, bracketed by a device
synchronise and the host clock.  Both engines stay alive for the whole run, so the two settings share the device's memory and clocks;
only one of them launches at a time.  Reported per setting, as the median over the rounds and per round:
    plies_per_s         plies played (positions searched) per second
    evals_per_ply       evaluator calls / plies of the segment
    sims_per_move       simulations / plies of the segment
    pruned_share        1 - sum(pruned visits) / sum(root_N) over the searched plies of the records drained in the segment; the pruned
                        visits of a ply are root_N[c*] / policy[c*] (c*, the most visited child, keeps its visits)
    pruned_rows         the share of those plies whose policy row differs from N / sum(N)
No figure is a threshold; the tool measures.  Whether the trade pays in playing strength is a training question.  One JSON object;
--out writes it.

    python tools/forced_playouts_bench.py --out profiles/forced_playouts_rates.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = {"k_0": dict(forced_playouts_k=0.0), "k_2": dict(forced_playouts_k=2.0)}
FIELDS = ("plies_per_s", "evals_per_ply", "sims_per_move", "pruned_share", "pruned_rows")


def make_engine(a, weights, kw):
    from grok_alpha_zero_amd.engine import EVAL_HASH, EVAL_RESNET, SelfPlayEngine
    net = a.evaluator == "resnet"
    eng = SelfPlayEngine("Connect4", a.games, a.iterations, 42, 8, 7, 2.5, 0.5, seed=1234, evaluator=EVAL_RESNET if net else EVAL_HASH, hash_salt=7,
                         net_blocks=a.blocks if net else 0, ring_capacity=2 * a.games, lib_path=a.emu_lib or None, **kw)
    if net:
        eng.load_weights(weights)
    return eng


def pruned_visits(recs):
    """-> (sum of root_N, sum of the pruned visit counts, plies, plies whose row differs from N / sum(N)) over the searched plies.
    The pruned sum of a ply is recovered as rint(N* / policy[c*]) from the float32 policy row: policy[c*] = f32(N* / sum) carries a relative
    error of at most 2^-24, so the quotient is off by at most sum x 2^-24 and the rounding is exact for sums below 2^23 — run_iterations is a
    few hundred.  policy[c*] > 0 wherever sum(root_N) > 0 (c* keeps its visits), so the division is defined on every ply counted."""
    raw = kept = 0.0
    plies = changed = 0
    for r in recs:
        N, pol = r["root_N"].astype(np.float64), r["policies"].astype(np.float64)
        tot = N.sum(axis=1)
        ok = tot > 0
        if not ok.any():
            continue
        N, pol, tot = N[ok], pol[ok], tot[ok]
        top = N.max(axis=1)
        p_star = np.where(N == top[:, None], pol, 0.0).max(axis=1)
        left = np.rint(top / p_star)
        raw += float(tot.sum()); kept += float(left.sum())
        plies += int(ok.sum()); changed += int((left != tot).sum())
    return raw, kept, plies, changed


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
    plies = s1["plies"] - s0["plies"]
    raw, kept, n, changed = pruned_visits(recs)
    return dict(seconds=round(dt, 4), plies=plies, games_drained=len(recs), plies_per_s=plies / dt, evals_per_ply=(s1["evals"] - s0["evals"]) / max(plies, 1),
                sims_per_move=(s1["sims"] - s0["sims"]) / max(plies, 1), pruned_share=1.0 - kept / max(raw, 1.0), pruned_rows=changed / max(n, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=300)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--burn-in-waves", type=int, default=12000, help="untimed launches per engine before the first timed segment (about two game lengths)")
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
    engines = {k: make_engine(a, weights, kw) for k, kw in SETTINGS.items()}
    for k, eng in engines.items():
        for i in range(0, a.burn_in_waves, 500):
            eng.run_waves(min(500, a.burn_in_waves - i)); eng.synchronize(); eng.drain_finished()
    rounds = {k: [] for k in engines}
    for r in range(a.rounds):
        for k in (list(engines) if r % 2 == 0 else list(engines)[::-1]):
            rounds[k].append(segment(engines[k], a))
            print(json.dumps(dict(round=r, setting=k, **rounds[k][-1])), file=sys.stderr, flush=True)
    out = dict(what="tools/forced_playouts_bench.py: continuous Connect4 self-play, forced_playouts_k = 0 vs 2, alternated on one box", games=a.games,
               run_iterations=a.iterations, net_blocks=a.blocks if a.evaluator == "resnet" else 0, evaluator=a.evaluator, burn_in_waves=a.burn_in_waves,
               waves_per_round=a.waves * a.segments, rounds=a.rounds, game_groups={k: e.stats()["game_groups"] for k, e in engines.items()},
               fused_wave={k: e.stats()["fused_wave"] for k, e in engines.items()}, settings={})
    for k, eng in engines.items():
        med = {f: statistics.median(x[f] for x in rounds[k]) for f in FIELDS}
        out["settings"][k] = dict(SETTINGS[k], median=med, per_round=rounds[k])
        eng.close()
    off, on = out["settings"]["k_0"]["median"], out["settings"]["k_2"]["median"]
    out["k_2_over_k_0"] = {f: on[f] / off[f] for f in ("plies_per_s", "evals_per_ply", "sims_per_move")}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

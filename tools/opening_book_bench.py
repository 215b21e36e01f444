#!/usr/bin/env python3
"""What the opening book costs and what it changes (SelfPlayEngine.set_opening_book): the headline configuration —
Connect4, 4096 slots, the 6-block x 128 network, run_iterations = 200, the library's own launch shape (fused launch, game groups) — with
    off     no book
    book    a book of 1024 entries of 8 plies each (random legal unfinished Connect4 positions, a fixed seed), mode 1
ONE engine per process, the processes alternated (off, book, off, book ... --rounds times each, one at a time on one box, the order swapping
every round).  Every child (this file with --setting) runs under `timeout -k 10`, and after one that failed or ran out of time none is
started.  A child burns its engine in to a stationary ply mix, then times --segments x --waves launches with the finished games drained
between them (device synchronise + host clock).  Reported per setting, as the median over its processes and per process:
    positions_per_s      SEARCHED plies per second (the engine's ply counter counts the plies it played; a book prefix is placed, not played)
    games_per_s          games finished per second
    searched_plies_per_game   mean searched plies of the games that finished in the timed stretch (T minus the book plies)
The network has RANDOM weights.  No figure is a threshold.  One JSON object; --out writes it.

    python tools/opening_book_bench.py --out profiles/opening_book_rates.json
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

SETTINGS = ("off", "book")
FIELDS = ("positions_per_s", "games_per_s", "searched_plies_per_game")


def connect4_book(n_entries, plies, seed=20240):
    """n_entries distinct legal unfinished Connect4 positions of `plies` moves, as action-index sequences: random playouts, a fixed seed"""
    import numpy as np
    from grok_alpha_zero_amd.games import Connect4
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    while len(out) < n_entries:
        g, seq = Connect4(), []
        while len(seq) < plies and (not seq or g.check_win() == -2):
            legal = g.get_legal_actions()
            a = legal[int(rng.integers(len(legal)))]
            g.do_action(a); seq.append(int(Connect4.action_to_index(a)) if hasattr(Connect4, "action_to_index") else int(a))
        if len(seq) == plies and g.check_win() == -2 and tuple(seq) not in seen:
            seen.add(tuple(seq)); out.append(seq)
    return out


def child(a):
    from grok_alpha_zero_amd.engine import EVAL_HASH, EVAL_RESNET, SelfPlayEngine
    net = a.evaluator == "resnet"
    eng = SelfPlayEngine("Connect4", a.slots, a.iterations, 42, 8, 7, 2.5, 0.5, seed=1234, evaluator=EVAL_RESNET if net else EVAL_HASH, hash_salt=7,
                         net_blocks=a.blocks if net else 0, ring_capacity=2 * a.slots, lib_path=a.emu_lib or None)
    if net:
        from grok_alpha_zero_amd.net import NETS
        eng.load_weights(NETS["Connect4"](a.blocks, seed=0).eval().export_engine_weights())
    if a.setting == "book":
        eng.set_opening_book(connect4_book(a.entries, a.plies), "game")
    for i in range(0, a.burn_in_waves, 500):
        eng.run_waves(min(500, a.burn_in_waves - i)); eng.synchronize(); eng.drain_finished()
    eng.synchronize(); eng.drain_finished()
    s0, games, searched, t0 = eng.stats(), 0, 0, time.perf_counter()
    for _ in range(a.segments):
        eng.run_waves(a.waves)
        eng.synchronize()
        for r in eng.drain_finished():
            games += 1; searched += int((r["move_kind"] != 3).sum())
    dt = time.perf_counter() - t0
    s1 = eng.stats()
    out = dict(seconds=round(dt, 4), positions_per_s=(s1["plies"] - s0["plies"]) / dt, games_per_s=games / dt, searched_plies_per_game=searched / max(games, 1),
               games=games, evals_per_wave=(s1["evals"] - s0["evals"]) / (a.segments * a.waves), fused_wave=s1["fused_wave"], game_groups=s1["game_groups"])
    if a.setting == "book":
        bc = eng.book_counts()
        out.update(book_started=bc["started"], book_prefix_plies=bc["prefix_plies"], entries_drawn=int((bc["counts"] > 0).sum()))
    eng.close()
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--entries", type=int, default=1024)
    ap.add_argument("--plies", type=int, default=8)
    ap.add_argument("--burn-in-waves", type=int, default=8000, help="untimed launches before the timed segment (about two game lengths)")
    ap.add_argument("--waves", type=int, default=400)
    ap.add_argument("--segments", type=int, default=5, help="timed launches per process = segments x waves")
    ap.add_argument("--rounds", type=int, default=2, help="processes per setting")
    ap.add_argument("--evaluator", default="resnet", choices=["resnet", "hash"])
    ap.add_argument("--emu-lib", default="", help="rehearsal on the one-lane CPU emulation build (hash evaluator, tiny sizes): no rate it prints means anything")
    ap.add_argument("--setting", default="", choices=["", "off", "book"], help="(the child processes) measure this one setting and print its figures")
    ap.add_argument("--child-timeout", type=int, default=150, help="seconds a child process may take; after one that failed or ran out of time none is started")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.setting:
        return child(a)
    passed = list(sys.argv[1:])
    if "--out" in passed:
        i = passed.index("--out"); del passed[i:i + 2]
    out = dict(what="tools/opening_book_bench.py: continuous Connect4 self-play in the library's own launch shape, without a book and with a book of "
                    f"{a.entries} entries of {a.plies} plies (mode 1); one engine per process, the processes alternated on one box",
               note="random network weights; no figure is a threshold; positions_per_s counts searched plies", slots=a.slots, run_iterations=a.iterations,
               net_blocks=a.blocks if a.evaluator == "resnet" else 0, evaluator=a.evaluator, burn_in_waves=a.burn_in_waves, waves_per_process=a.waves * a.segments,
               processes_per_setting=a.rounds)
    rounds = {k: [] for k in SETTINGS}
    for r in range(a.rounds):
        for k in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
            p = subprocess.run(["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--setting", k] + passed, capture_output=True, text=True)
            if p.returncode != 0:                    # failed, or killed at its time limit (124 / 137): nothing more is started
                print(f"child {k}: exit status {p.returncode}\n{p.stderr[-2000:]}", file=sys.stderr)
                return 1
            rounds[k].append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(dict(round=r, setting=k, **rounds[k][-1])), file=sys.stderr, flush=True)
    for k in SETTINGS:
        out[k] = dict(median={f: statistics.median(x[f] for x in rounds[k]) for f in FIELDS}, per_process=rounds[k])
    out["book_over_off"] = {f: out["book"]["median"][f] / out["off"]["median"][f] for f in FIELDS if out["off"]["median"][f]}
    out["off_spread"] = {f: max(x[f] for x in rounds["off"]) - min(x[f] for x in rounds["off"]) for f in FIELDS}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

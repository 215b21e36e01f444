#!/usr/bin/env python3
"""What policy surprise weighting (SelfPlayEngine.set_sample_weighting) costs at the drain and what it writes.

Per case — 4096 finished Connect4 games, 64 finished Gomoku games, hash evaluator, playout cap on — ms per drain_samples() of the whole
ring with the mode off and on (lambda 0.5), and the same off-path on another build of the library (--parent-lib: the parent commit's
libgaz_engine.so), every measurement a process of its own, the processes alternating on one box: parent-off, off, on, parent-off, ...
A process fills the ring three times; its first drain allocates the staging buffers.  The three drains of a process differ from each other
by more than the builds do (the third runs in about a fifth of the second's time), so times are compared per drain position: first with
first, second with second, third with third, the median and the range over the processes of each.  One more
process per case takes the same games as records and counts, with self_play.sample_row_counts, the rows out per full ply and the share
of fast plies that got a row.

usage: python tools/surprise_bench.py [--parent-lib PATH] [--reps 5] [--out profiles/surprise_drain_times.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {   # name -> game, games per fill, run_iterations, fast_iterations, max_actions
    "connect4-4096": ("Connect4", 4096, 40, 8, 42), "gomoku-64": ("Gomoku", 64, 48, 12, 225),
}
LAMBDA, FAST_FACTOR, SEED, FILLS = 0.5, 1.5, 7, 3


def engine(case, lib, fills):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    game, n, R, F, max_actions = CASES[case]
    return SelfPlayEngine(game, n, R, max_actions, 3, 2, 2.5, 0.5, seed=SEED, hash_salt=6, ring_capacity=fills * n, games_budget=fills * n, fast_iterations=F,
                          full_search_prob=0.25, lib_path=lib)


def fill(eng, n):
    """run until n games have finished since the engine was created (the ring holds every game of the process)"""
    for _ in range(200000):
        eng.run_waves(64); eng.synchronize()
        if int(eng.stats()["game_stats"][2]) >= n:
            return
    raise RuntimeError("the ring did not fill")


def child(case, lib, mode):
    n = CASES[case][1]
    if mode == "stats":
        from grok_alpha_zero_amd.self_play import sample_row_counts
        eng = engine(case, lib, 1)
        fill(eng, n)
        recs = eng.drain_finished()
        eng.close()
        rows = n_full = n_fast = fast_written = plies = 0
        for r in recs:
            c = sample_row_counts(r, LAMBDA, FAST_FACTOR, SEED)
            fast = r["move_kind"] == 2
            rows += int(c.sum()); n_full += int((r["move_kind"] == 1).sum()); n_fast += int(fast.sum()); fast_written += int((c[fast] > 0).sum()); plies += r["T"]
        print(json.dumps(dict(games=len(recs), plies=plies, full_plies=n_full, fast_plies=n_fast, rows_out=rows, rows_per_full_ply=rows / max(n_full, 1),
                              fast_plies_written=fast_written, share_of_fast_plies_written=fast_written / max(n_fast, 1))))
        return
    eng = engine(case, lib, FILLS)
    if mode == "on":
        eng.set_sample_weighting(LAMBDA, FAST_FACTOR)
    ms, rows = [], []
    for k in range(FILLS):
        fill(eng, (k + 1) * n)
        t0 = time.perf_counter()
        b = eng.drain_samples(max_games=n)
        ms.append((time.perf_counter() - t0) * 1e3)
        assert b.n == n, (b.n, n)
        rows.append(b.rows)
    eng.close()
    print(json.dumps(dict(ms=ms, rows=rows)))


def run_child(case, lib, mode):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, lib or "", mode], capture_output=True, text=True, timeout=600)
    if r.returncode:
        raise SystemExit(f"{case} {mode}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def summary(samples):
    """per drain position (first, second, third drain of a process): median, min and max over the processes"""
    pos = [[smp["ms"][k] for smp in samples] for k in range(FILLS)]
    return dict(ms_median=[statistics.median(p) for p in pos], ms_min=[min(p) for p in pos], ms_max=[max(p) for p in pos], ms=pos, rows=samples[0]["rows"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surprise_drain_times.json"))
    a = ap.parse_args()
    out = dict(what="ms per drain_samples() of a full ring, hash-evaluator games with the playout cap on (full_search_prob 0.25); processes alternate on one box; "
                    "every list is [first, second, third drain of a process]; the first allocates the staging buffers",
               lambda_=LAMBDA, fast_factor=FAST_FACTOR, reps=a.reps, parent_lib=bool(a.parent_lib), cases={})
    for case in CASES:
        modes = ([("parent_off", a.parent_lib, "off")] if a.parent_lib else []) + [("off", None, "off"), ("on", None, "on")]
        got = {m[0]: [] for m in modes}
        for _ in range(a.reps):
            for key, lib, mode in modes:
                got[key].append(run_child(case, lib, mode))
        res = {k: summary(v) for k, v in got.items()}
        res["weighting"] = run_child(case, None, "stats")
        if a.parent_lib:
            p, o = res["parent_off"], res["off"]
            res["off_vs_parent"] = dict(delta_ms=[a - b for a, b in zip(o["ms_median"], p["ms_median"])],
                                        parent_spread_ms=[a - b for a, b in zip(p["ms_max"], p["ms_min"])])
        res["on_vs_off_ms"] = [a - b for a, b in zip(res["on"]["ms_median"], res["off"]["ms_median"])]
        out["cases"][case] = res
        print(case, json.dumps({k: (v if not isinstance(v, dict) else {x: y for x, y in v.items() if not isinstance(y, list)}) for k, v in res.items()}), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3] or None, sys.argv[4])
    else:
        main()

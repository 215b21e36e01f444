#!/usr/bin/env python3
"""Measures the held-out loss (SelfPlayEngine.score_replay) on an MI355X: a replay window of a few hundred thousand Connect4
rows (random stones, valid policy rows) scored by the 6-block network.

  rows per second of score_replay at batch_rows 1024 and 4096 (host clock around the call, which ends in a synchronise; three repeats after a
      warm-up), and the device time of the pass from HIP events (`ms`)
  ms of k_score_rows per batch from HIP events (gaz_engine_score_rows_timed: the launch of a score_outputs call, 200 times between two events)
  the time of gaz_engine_evaluate(repeats = the number of batches) of the same batch size: the forward passes alone
  the ratio scoring / evaluation and k_score_rows' share of a batch

    python tools/score_bench.py [--rows 262144] [--out profiles/score_rates.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_rates.json"))
    a = ap.parse_args()
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
    from grok_alpha_zero_amd.net import Connect4Net
    from grok_alpha_zero_amd.replay import ReplayWindow
    rng = np.random.default_rng(0)
    R, A = a.rows, 7
    w = ReplayWindow("Connect4", R, seed=1, test_fraction=0.0, target_ratio=None)
    y = rng.random((R, A), dtype=np.float32); y[rng.random((R, A)) < 0.3] = 0; y[np.arange(R), rng.integers(0, A, R)] += np.float32(0.5)
    y = (y / y.sum(1, keepdims=True)).astype(np.float32)
    games = np.zeros((R // 32, 6), np.int32); games[:, 0] = 32; games[:, 4] = np.arange(R // 32) * 32
    w.append_arrays(0, games, rng.integers(-1, 2, (R, 6, 7, 4)).astype(np.int8), y, rng.integers(-1, 2, R).astype(np.float32))
    assert w.begin_epoch("train", 0, percent=1.0, decay=0.0) == R
    weights = Connect4Net(a.blocks, seed=0).eval().export_engine_weights()
    out = dict(what="tools/score_bench.py on an MI355X: score_replay of a Connect4 window by the %d-block network" % a.blocks, rows=R, blocks=a.blocks, cases=[])
    for B in a.batches:
        eng = SelfPlayEngine("Connect4", B, 8, 42, 0, 0, 2.5, 0.5, seed=1, evaluator=EVAL_RESNET, net_blocks=a.blocks, ring_capacity=0, game_groups=1, nodes_per_tree=64)
        eng.load_weights(weights)
        n_batches = (R + B - 1) // B
        first = eng.score_replay(w, batch_rows=B, augment=True)                            # warm-up: code objects, buffers
        wall, dev = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            d = eng.score_replay(w, batch_rows=B, augment=True)
            wall.append(time.perf_counter() - t0); dev.append(d["ms"])
            assert d["ce_sum"] == first["ce_sum"] and d["rows"] == R
        boards, pol, val = w.batch(0, B, augment=True)
        P, V, _ = eng.evaluate(boards)
        eng.score_outputs(P, V, pol, val)
        ms_rows = C.c_double()
        eng._ck(eng.L.gaz_engine_score_rows_timed(eng.h, 200, C.byref(ms_rows)))
        gather_ms = w.sample_timed(0, B, True, repeats=200)
        _, _, ms_eval = eng.evaluate(boards, repeats=n_batches)
        case = dict(batch_rows=B, batches=n_batches, wall_seconds=wall, device_ms=dev, rows_per_second=R / min(wall), ms_per_batch=min(dev) / n_batches,
                    k_score_rows_ms_per_batch=ms_rows.value, gather_ms_per_batch=gather_ms, evaluate_ms_per_batch=ms_eval, evaluate_ms_total=ms_eval * n_batches,
                    scoring_over_evaluation=min(dev) / (ms_eval * n_batches), k_score_rows_share_of_a_batch=ms_rows.value / (min(dev) / n_batches),
                    val_loss=first["val_loss"], top1=first["top1"], bad_rows=first["bad_rows"])
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
        eng.close()
    w.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

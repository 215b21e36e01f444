#!/usr/bin/env python3
"""What the replay window (grok_alpha_zero_amd/replay.py) costs: per game, one window per process,

  * rows/s of append() (host arrays -> the device store, 65536 rows per call),
  * ms per begin_epoch() at 1 M and 8 M live rows (train split, test_fraction 0.1, target_ratio 0.5, four generations, decay 0.25),
  * rows/s and bytes/s (read + written: 2 x (state + policy + value) per row) of the gather at n = 256 and n = 4096 on the 1 M window, HIP
    events around 100 launches after a warm-up (gaz_replay_sample_timed), and its share of the HBM bandwidth figure,
  * the same batch by a PyTorch restatement on the same device and the same window contents: index_select of the three arrays by the same
    source rows, plus a gather through a precomputed [n_aug][state] / [n_aug][A] index table chosen per row by the same symmetries (torch
    events around 100 repetitions).  It gets the rows and symmetries for free; the kernel computes them.  The two alternate in one process,
    five rounds, medians reported; the restatement's bytes are checked against the kernel's once.

usage: python tools/replay_bench.py [--out profiles/replay_rates.json] [--games TicTacToe Connect4 Gomoku] [--rows 1000000 8000000]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBS = 8.0                                   # the spec figure of the MI355X (about 6.3 TB/s is achievable by streaming kernels)
CHUNK, GENERATIONS, REPS, ROUNDS = 65536, 4, 100, 5
GAME_LEN = {"TicTacToe": 7, "Connect4": 30, "Gomoku": 60}


def chunk_of(game, rng):
    from grok_alpha_zero_amd.engine import GAME_DIMS, GAME_IDS
    H, W, Cc, A = GAME_DIMS[GAME_IDS[game]]
    lengths = []
    while sum(lengths) < CHUNK:
        lengths.append(min(int(rng.integers(GAME_LEN[game] - 3, GAME_LEN[game] + 4)), CHUNK - sum(lengths)))
    games = np.zeros((len(lengths), 6), np.int32)
    games[:, 0] = lengths; games[:, 4] = np.cumsum([0] + lengths[:-1])
    return games, rng.integers(-1, 2, (CHUNK, H, W, Cc)).astype(np.int8), rng.random((CHUNK, A), dtype=np.float32), rng.random(CHUNK, dtype=np.float32)


def index_tables(game):
    """[n_aug][state bytes] and [n_aug][A] source indices of the plugin's augment_sample, from an arange pushed through it"""
    from grok_alpha_zero_amd.engine import GAME_DIMS, GAME_IDS
    from grok_alpha_zero_amd.games import GAMES
    H, W, Cc, A = GAME_DIMS[GAME_IDS[game]]
    cls = GAMES[game]
    aug = cls.augment_sample if game == "Connect4" else cls().augment_sample
    st = np.arange(H * W * Cc, dtype=np.int64).reshape(1, H, W, Cc)
    pol = np.arange(A, dtype=np.float32).reshape(1, A)
    hi, p = aug((st // 100).astype(np.int8), pol)                                     # (the plugins return states as int8: two digits of the index)
    lo, _ = aug((st % 100).astype(np.int8), pol)
    b = np.asarray(hi).astype(np.int64) * 100 + np.asarray(lo).astype(np.int64)
    return b.reshape(len(b), -1), np.asarray(p).reshape(len(p), -1).astype(np.int64)


def child(game, rows):
    if rows <= 2_000_000:
        import torch  # noqa: F401 — before the engine library: the two then share one HIP runtime (ReplayWindow.batch_torch)
    from grok_alpha_zero_amd.replay import ReplayWindow
    rng = np.random.default_rng(1)
    games, b, p, v = chunk_of(game, rng)
    n_chunks = rows // CHUNK
    w = ReplayWindow(game, n_chunks * CHUNK, seed=3, test_fraction=0.1, target_ratio=0.5)
    w.append_arrays(0, games, b, p, v); w.evict(1)                                    # warm-up of the copy path
    t0 = time.perf_counter()
    for k in range(n_chunks):
        w.append_arrays(k * GENERATIONS // n_chunks, games, b, p, v)
    t_append = time.perf_counter() - t0
    live = w.info()["rows"]
    assert live == n_chunks * CHUNK
    out = dict(game=game, rows=live, games=w.info()["games"], append_rows_per_s=live / t_append)
    M = w.begin_epoch("train", epoch=0, percent=1.0, decay=0.25)
    ms = []
    for e in range(1, 6):
        t0 = time.perf_counter()
        M = w.begin_epoch("train", epoch=e, percent=1.0, decay=0.25)
        ms.append((time.perf_counter() - t0) * 1e3)
    out.update(begin_epoch_ms=statistics.median(ms), begin_epoch_ms_all=ms, plan_rows=M)
    if rows > 2_000_000:
        w.close()
        print(json.dumps(out))
        return
    import torch
    dev = torch.device("cuda", 0)
    reps = -(-live // CHUNK)
    t_state = torch.from_numpy(np.tile(b.reshape(CHUNK, -1), (reps, 1))[:live]).to(dev)
    t_pol = torch.from_numpy(np.tile(p, (reps, 1))[:live]).to(dev)
    t_val = torch.from_numpy(np.tile(v, reps)[:live]).to(dev)
    si, pi = (torch.from_numpy(x).to(dev) for x in index_tables(game))
    row_bytes = 2 * (w.SB + 4 * w.A + 4)
    out["gather"] = {}
    for n in (256, 4096):
        first = 12345
        kb, kp, kv, kr, ks = w.batch(first, n, with_index=True)
        rows_t, sym_t = torch.from_numpy(kr.astype(np.int64)).to(dev), torch.from_numpy(ks.astype(np.int64)).to(dev)

        def restatement():
            bb = t_state.index_select(0, rows_t).gather(1, si.index_select(0, sym_t))
            pp = t_pol.index_select(0, rows_t).gather(1, pi.index_select(0, sym_t))
            return bb, pp, t_val.index_select(0, rows_t)
        bb, pp, vv = restatement()
        same = bb.cpu().numpy().tobytes() == kb.tobytes() and pp.cpu().numpy().tobytes() == kp.tobytes() and vv.cpu().numpy().tobytes() == kv.tobytes()
        for _ in range(10):
            restatement()
        torch.cuda.synchronize()
        ours, theirs = [], []
        for _ in range(ROUNDS):
            ours.append(w.sample_timed(first, n, True, REPS))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                restatement()
            e1.record(); torch.cuda.synchronize()
            theirs.append(e0.elapsed_time(e1) / REPS)
        k_ms, t_ms = statistics.median(ours), statistics.median(theirs)
        out["gather"][str(n)] = dict(kernel_ms=k_ms, kernel_ms_all=ours, torch_ms=t_ms, torch_ms_all=theirs, restatement_equals_kernel=bool(same),
                                     kernel_rows_per_s=n / k_ms * 1e3, kernel_bytes_per_s=n * row_bytes / k_ms * 1e3,
                                     hbm_share_of_8_TBs=n * row_bytes / k_ms * 1e3 / (HBM_PEAK_TBS * 1e12), torch_rows_per_s=n / t_ms * 1e3)
    w.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_rates.json"))
    ap.add_argument("--games", nargs="+", default=["TicTacToe", "Connect4", "Gomoku"])
    ap.add_argument("--rows", nargs="+", type=int, default=[1_000_000, 8_000_000])
    a = ap.parse_args()
    out = dict(what="replay window: append rows/s, ms per begin_epoch, the gather kernel against a PyTorch restatement (alternated in one process, medians of "
                    f"{ROUNDS} rounds of {REPS} launches); one window per process", hbm_peak_TBs=HBM_PEAK_TBS, results=[])
    for game in a.games:
        for rows in a.rows:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", game, str(rows)], capture_output=True, text=True, timeout=900)
            if r.returncode:
                raise SystemExit(f"{game} {rows}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            res = json.loads(r.stdout.strip().splitlines()[-1])
            out["results"].append(res)
            print(json.dumps({k: v for k, v in res.items() if not k.endswith("_all")}), flush=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()

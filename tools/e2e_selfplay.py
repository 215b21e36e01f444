"""End to end through run_self_play on the GPU: one generation of Connect4 (4096 slots, 201 simulations per move, the 6-block network,
20 000 games), from engine creation to the last game handed out or written.  A measurement tool, not a test and not part of bench.py.

    python tools/e2e_selfplay.py --mode MODE [--cache 0|1] [--games N] [--slots G] [--package-root DIR] [--json FILE]

  off      run_self_play(device_samples=False): records drained one by one, converted by record_to_samples, written to the HDF5 file
  on       run_self_play(device_samples=True): samples built on the device, one call per drain, written by the writer thread
  samples  the same loop with drain_samples and NO file: the rate an integrator with a store of their own gets
  dropped  the same loop with the raw gaz_engine_drain_finished call into a reused buffer, nothing decoded: what the generation costs
           with no host work at all (start-up, tail and repack included) — the yardstick of the other three

Prints one JSON line: positions/s = rows handed out or written / wall clock, and the seconds the thread that queues the waves spent
waiting for the GPU (`main_gpu_wait_s`), obtaining samples (`main_sample_s`) and blocked by the writer (`main_queue_wait_s`), and the
seconds spent writing (`writer_s`; on the writer thread, or on the main thread where the tree has none).  `--package-root` points at
another checkout of this repository (built), e.g. the parent commit for a baseline: a tree whose run_self_play has no `device_samples`
is run as it is (mode off) and timed from outside.  Run every invocation as a process of its own, under its own time limit, and chain
them with && :

    timeout -k 10 300 python tools/e2e_selfplay.py --mode dropped --cache 1 && timeout -k 10 300 python tools/e2e_selfplay.py --mode on --cache 1
"""
import argparse
import inspect
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["off", "on", "samples", "dropped"], required=True)
ap.add_argument("--cache", type=int, default=1, help="1 = evaluation cache on (eval_cache_log2 = 22, run_self_play's default), 0 = off")
ap.add_argument("--games", type=int, default=20000)
ap.add_argument("--slots", type=int, default=4096)
ap.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--json", default=None, help="append the result line to this file as well")
ap.add_argument("--tag", default="")
ap.add_argument("--synthetic", action="store_true", help="the synthetic hash evaluator instead of the network (to try the tool itself)")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.package_root))

from grok_alpha_zero_amd import engine as E                                      # noqa: E402
from grok_alpha_zero_amd import self_play as SP                                  # noqa: E402
from grok_alpha_zero_amd.games import GAMES                                      # noqa: E402
from grok_alpha_zero_amd.net import Connect4Net                                  # noqa: E402

N, G, LOG2 = args.games, args.slots, 22 if args.cache else 0
train = dict(games_per_generation=N, MCTS_iteration_limit=134, max_actions=42, num_explore_actions_first=8, num_explore_actions_second=7,
             c_puct_init=2.5, dirichlet_alpha=0.5, use_gumbel=False)          # int(1.5 * 134) = 201 simulations per move
build = dict(num_resnet_layers=6, num_filters=128)
weights = None if args.synthetic else Connect4Net(6).eval().export_engine_weights()
clock = time.perf_counter
res = dict(mode=args.mode, cache=args.cache, games=N, slots=G, tag=args.tag, main_gpu_wait_s=0.0, main_sample_s=0.0, main_queue_wait_s=0.0, writer_s=0.0)


def through_the_file():
    has_flag = "device_samples" in inspect.signature(SP.run_self_play).parameters
    if not has_flag and args.mode != "off":
        raise SystemExit("this tree's run_self_play has no device_samples: only --mode off")
    root = tempfile.mkdtemp()
    folder = os.path.join(root, "1")
    SP.ReplayStore(folder).create()
    kw, stats = {}, {}
    if has_flag:
        kw = dict(device_samples=args.mode == "on")
    else:                                            # a tree without the writer thread: time its main thread from outside
        depth = [0]

        def timed(fn, key):
            def wrapper(*a, **k):
                depth[0] += 1
                t0 = clock()
                try:
                    return fn(*a, **k)
                finally:
                    depth[0] -= 1
                    if depth[0] == 0:
                        res[key] += clock() - t0
            return wrapper
        drain = E.SelfPlayEngine.drain_finished

        def drain_timed(self, *a, **k):
            t0 = clock()
            self.synchronize()
            t1 = clock()
            out = drain(self, *a, **k)
            res["main_gpu_wait_s"] += t1 - t0; res["main_sample_s"] += clock() - t1
            return out
        E.SelfPlayEngine.drain_finished = drain_timed
        SP.record_to_samples = timed(SP.record_to_samples, "main_sample_s")
        SP.ReplayStore.append_game = timed(SP.ReplayStore.append_game, "writer_s")
        SP.ReplayStore._flush = timed(SP.ReplayStore._flush, "writer_s")
    t0 = clock()
    played = SP.run_self_play(GAMES["Connect4"], (build, train), folder, n_games=G, seed=1, weights=weights, allow_synthetic=args.synthetic, eval_cache_log2=LOG2,
                               engine_stats=stats, **kw)
    dt = clock() - t0
    gs = SP.ReplayStore(folder).game_stats()
    res.update(played=int(played), rows=int(gs[1]), seconds=dt, file_mb=os.path.getsize(os.path.join(folder, "Self_Play_Data.h5")) / 1e6,
               waves=stats.get("waves"), writer_thread=has_flag)
    if has_flag:
        res.update(main_gpu_wait_s=stats["gpu_wait_seconds"], main_sample_s=stats["sample_seconds"], main_queue_wait_s=stats["queue_wait_seconds"],
                   writer_s=stats["writer_seconds"])
    shutil.rmtree(root, ignore_errors=True)


def without_a_file():
    """run_self_play's loop (same engine, same waves per drain, same repack rule) with nothing behind the drain"""
    import ctypes as C
    t_start = clock()
    eng = E.SelfPlayEngine("Connect4", G, 201, 42, 8, 7, 2.5, 0.5, 1, evaluator=E.EVAL_HASH if args.synthetic else E.EVAL_RESNET,
                           net_blocks=0 if args.synthetic else 6, net_filters=128, ring_capacity=max(4 * G, 64), eval_cache_log2=LOG2, games_budget=N, first_game_seq=0)
    if weights is not None:
        eng.load_weights(weights)
    lay = eng.layout
    if args.mode == "dropped":
        cap = max(eng.cfg.ring_capacity, 1)
        buf = np.empty((cap, lay.record_bytes), np.uint8)
        n_out = C.c_int32()
    done = rows = 0
    launch, idle = G, 0
    eng.run_waves(64)
    while done < N:
        t0 = clock()
        eng.synchronize()
        t1 = clock()
        if args.mode == "samples":
            batch = eng.drain_samples()
            got, r = batch.n, batch.rows
        else:
            eng._ck(eng.L.gaz_engine_drain_finished(eng.h, buf.ctypes.data, cap, C.byref(n_out)))
            got = n_out.value
            r = int(buf[:got, lay.off_hdr:lay.off_hdr + 4].copy().view(np.int32).sum())
        res["main_gpu_wait_s"] += t1 - t0; res["main_sample_s"] += clock() - t1
        remaining = N - done - got
        if 0 < remaining and remaining * 2 <= launch and launch > 16:
            _, launch = eng.repack()
        eng.run_waves(64)
        done += got; rows += r
        idle = 0 if got else idle + 1
        if idle > 100000:
            raise RuntimeError("self-play made no progress")
    waves = eng.stats()["waves"]
    eng.close()
    res.update(played=done, rows=rows, seconds=clock() - t_start, waves=waves)


through_the_file() if args.mode in ("off", "on") else without_a_file()
res["positions_per_s"] = res["rows"] / res["seconds"]
line = json.dumps(res)
print(line, flush=True)
if args.json:
    with open(args.json, "a") as f:
        f.write(line + "\n")

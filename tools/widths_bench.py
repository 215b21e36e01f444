#!/usr/bin/env python3
"""Self-play throughput of the Connect4 network at each residual width (build_config["num_filters"] in {64, 128, 192, 256}) on the
headline composition: 4096 games, 200 simulations per move, 6 blocks.  bench.py's conventions: engine set-up, burn-in waves from the
lockstep start, W warm-up steps, then K timed steps of --waves-per-step waves; one JSON result line per width.

  positions/s  plies played in the timed steps / seconds;   evals/s  evaluator rows in the timed steps / seconds.

The convolution kernels' share of the 2.5 PF bf16 peak needs kernel durations that no in-process event can give at F = 128 (the trunk
there runs inside the fused tree + trunk launch), so it comes from a rocprofv3 run of its own over a pure evaluator loop (--profile-evals:
R forwards of 4096 positions, exactly known FLOPs), read back by --parse-trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/widths_bench.py --profile-evals 20
  python tools/widths_bench.py --parse-trace OUT --profile-evals 20

usage: python tools/widths_bench.py [--widths 64,128,192,256] [--steps 8] [--warmup 1] [--burn-in-waves 8000]"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BF16_FLOPS = 2.5e15
G, SIMS, BLOCKS, HW = 4096, 200, 6, 42


def conv_flops_per_position(F, blocks=BLOCKS):
    """the trunk convolutions and the heads' first convolution (the work of the conv kernels; stem and dense layers excluded)"""
    from grok_alpha_zero_amd.net import flops_per_position
    f = flops_per_position(blocks, F)
    return f["trunk"] + 2 * HW * 9 * F * 32            # heads' conv: 16 real channels padded to 32 on the matrix cores


def measure(F, args):
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
    from grok_alpha_zero_amd.net import Connect4Net
    w = Connect4Net(BLOCKS, num_filters=F, seed=0).eval().export_engine_weights()
    eng = SelfPlayEngine("Connect4", G, SIMS, 42, 8, 7, 2.5, 0.5, seed=1234, evaluator=EVAL_RESNET, net_blocks=BLOCKS, net_filters=F,
                         hash_salt=7, ring_capacity=0)
    eng.load_weights(w)
    for i in range(0, args.burn_in_waves, 500):
        eng.run_waves(min(500, args.burn_in_waves - i)); eng.synchronize()
    for _ in range(args.warmup):
        eng.run_waves(args.waves_per_step); eng.synchronize()
    s0 = eng.stats()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        eng.run_waves(args.waves_per_step)
    eng.synchronize()
    dt = time.perf_counter() - t0
    s1 = eng.stats()
    kname, _ = eng.dominant_kernel()
    eng.close()
    plies, evals = int(s1["plies"] - s0["plies"]), int(s1["evals"] - s0["evals"])
    return dict(metric="self-play positions/sec by residual width", num_filters=F, value=plies / dt, unit="positions/s", evals_per_s=evals / dt,
                steps=args.steps, warmup=args.warmup, burn_in_waves=args.burn_in_waves, waves_per_step=args.waves_per_step, ms_per_step=dt / args.steps * 1e3,
                fused_wave=int(s1.get("fused_wave", 0)), game_groups=int(s1.get("game_groups", 1)), dominant_kernel=kname,
                config=f"Connect4 6x7, {G} games, {SIMS} sims/move, {BLOCKS} blocks x {F} filters, bf16, PUCT, random-init weights")


def profile_evals(widths, reps):
    """the kernels to profile: `reps` forwards of G random positions per width, in the order of `widths`"""
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
    from grok_alpha_zero_amd.net import Connect4Net
    x = np.random.default_rng(0).integers(-1, 2, size=(G, 6, 7, 4)).astype(np.int8)
    for F in widths:
        eng = SelfPlayEngine("Connect4", G, SIMS, 42, 8, 7, 2.5, 0.5, seed=1, evaluator=EVAL_RESNET, net_blocks=BLOCKS, net_filters=F, ring_capacity=0)
        eng.load_weights(Connect4Net(BLOCKS, num_filters=F, seed=0).eval().export_engine_weights())
        eng.evaluate(x)                                 # warm-up
        eng.evaluate(x, repeats=reps)
        eng.close()


def parse_trace(out_dir, widths, reps):
    """kernel trace of --profile-evals -> per width: conv kernel time per forward and its share of the bf16 peak.  The widths ran one after
    the other, each with one warm-up forward and `reps` timed ones; a width's launches are told apart by their template arguments and
    column tiles (width_of); F = 128 runs k_trunk (stem, trunk and heads' conv in one kernel: its time is charged to the conv FLOPs alone)."""
    path = sorted(glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True))
    assert path, f"no kernel trace under {out_dir}"
    rows = list(csv.DictReader(open(path[0])))
    for F in widths:
        per = {}
        for r in rows:
            n = r["Kernel_Name"]
            if (F == 128 and "k_trunk" in n) or (F != 128 and "k_conv_wide" in n and width_of(n, int(r["Grid_Size_Y"])) == F):
                per.setdefault(n, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        if not per:
            continue
        forwards = reps + 2                             # evaluate(x) once, then evaluate(x, repeats = R): 1 + R forwards
        ns = sum(sum(d) for d in per.values())
        flops = conv_flops_per_position(F) * G * forwards
        print(json.dumps(dict(metric="conv kernels' share of the bf16 peak", num_filters=F, kernels=len(per), launches=sum(len(d) for d in per.values()),
                              conv_us_per_forward=ns / 1e3 / forwards, flops_per_forward=flops / forwards, tflops=flops / (ns * 1e-9) / 1e12,
                              share_of_peak=flops / (ns * 1e-9) / PEAK_BF16_FLOPS,
                              note="heads' conv counted with its 32 padded channels; stem and dense layers excluded")), flush=True)


def width_of(name, grid_y):
    """F of a k_conv_wide launch from its template arguments <CIN, BN, ..., CIN2, ...> and its column tiles (grid y = F / BN)"""
    args = [int(a) for a in name.split("k_conv_wide<")[1].split(">")[0].split(",")]
    cin, bn, cin2 = args[0], args[1], args[8]
    if bn == 32 or cin2:                                # heads' conv F -> 32, block 0's conv2 + projection: CIN = F
        return cin
    return bn * grid_y                                  # the 3x3 convs F' -> F


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", default="64,128,192,256")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--waves-per-step", type=int, default=400)
    ap.add_argument("--burn-in-waves", type=int, default=8000)
    ap.add_argument("--profile-evals", type=int, default=0, help="R > 0: only run R forwards of 4096 positions per width (for rocprofv3)")
    ap.add_argument("--parse-trace", default="", help="rocprofv3 output directory of a --profile-evals run -> share-of-peak lines")
    args = ap.parse_args()
    widths = [int(f) for f in args.widths.split(",")]
    if args.parse_trace:
        parse_trace(args.parse_trace, widths, args.profile_evals)
    elif args.profile_evals:
        profile_evals(widths, args.profile_evals)
    else:
        for F in widths:
            print(json.dumps(measure(F, args)), flush=True)

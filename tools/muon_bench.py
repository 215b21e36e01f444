#!/usr/bin/env python3
"""Measures the fused Muon step (optim.FusedOptimizer(muon=...); csrc/muon.hpp) on an MI355X against the same chain written
tensor by tensor in torch ops ON THE SAME ARENAS — muon.py as a caller would write it today, the Newton-Schulz products as bf16 torch.matmul — for
the parameter lists of the 10-block Gomoku and the 6-block Connect4 network, classified as train.muon_classification does with the reference's
exclude_layers, under Muon alone and Muon + Grokfast + Orthograd.  For scale: the fused Nadam step of the same list, and a Muon optimizer that holds
Gomoku's largest matrix alone (p_d1, 1800 x 512: 5 iterations x (2 P P Q + P P P + P P Q) x 2 = 10.8 GFLOP of f32 MFMA work a step), from which
the share of the step spent on it and the f32 MFMA rate reached against the chip's peak follow.

  ms per step of both sides from HIP events (gaz_optim_step_timed; torch.cuda.Event around the same number of steps), after a warm-up, the two
      sides alternated in one process, the median over the rounds

    python tools/muon_bench.py [--steps 20] [--rounds 5] [--out profiles/muon_step_times.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B1, B2, EPS, ALPHA, BETA, LAMB = 0.9, 0.995, 1e-8, 0.99, 0.95, 5.0
NS = (3.4445, -4.7750, 2.0315)
PEAK_F32_MFMA_TFLOPS = 157.3                        # MI355X, v_mfma_f32_32x32x2_f32 (AMD's specification)
CONFIGS = [("muon", dict()), ("muon+grokfast+orthograd", dict(grokfast=True, lamb=LAMB, orthograd=True))]
WHAT = ("tools/muon_bench.py on one MI355X: ms per optimizer step from HIP events, `steps` steps a round after a warm-up, the fused Muon step "
        "(optim.FusedOptimizer(muon=...), gaz_optim_step_timed) and muon.py's chain written per tensor in torch ops on the same arenas (bf16 torch.matmul) "
        "alternated in one process, the median over `rounds` rounds; nadam_ms_per_step: the fused Nadam step of the same parameter list; p_d1: a Muon "
        "optimizer holding the 1800 x 512 matrix alone")


def torch_step(tensors, cfg, lr, t):
    """Orthograd(Grokfast_EMA(Muon)) per tensor, as Net/Optimizers/*.py state it"""
    c1, c2 = 1.0 - B1 ** t, 1.0 - B2 ** t
    for w, g, m, v, e, shape, is_muon, scale in tensors:
        if cfg.get("orthograd"):
            proj = torch.dot(w, g) / (torch.dot(w, w) + 1e-30)
            go = g - proj * w
            g = go * (torch.linalg.vector_norm(g) / (torch.linalg.vector_norm(go) + 1e-30))
        if cfg.get("grokfast"):
            e.mul_(ALPHA).add_(g, alpha=1.0 - ALPHA)
            g = g + e * cfg["lamb"]
        if not is_muon:
            m.mul_(B1).add_(g, alpha=1.0 - B1)
            v.mul_(B2).addcmul_(g, g, value=1.0 - B2)
            nesterov = (m / c1) * B1 + (g * (1.0 - B1)) / c1
            w.sub_(nesterov / ((v / c2).sqrt() + EPS) * lr)
            continue
        m.mul_(BETA).add_(g, alpha=1.0 - BETA)
        X = (g + m * BETA).view(shape[0], -1).to(torch.bfloat16)
        tr = X.shape[0] > X.shape[1]
        if tr:
            X = X.T
        X = X / (X.norm() + 1e-7)
        for _ in range(5):
            A = X @ X.T
            B = NS[1] * A + NS[2] * (A @ A)
            X = NS[0] * X + B @ X
        if tr:
            X = X.T
        w.sub_(X.to(torch.float32).reshape(-1) * (scale * lr))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "muon_step_times.json"))
    a = ap.parse_args()
    from grok_alpha_zero_amd import train as T
    from grok_alpha_zero_amd.net import Connect4Net, GomokuNet
    from grok_alpha_zero_amd.optim import FusedOptimizer
    nets = [("Gomoku, 10 blocks", "Gomoku", GomokuNet(10)), ("Connect4, 6 blocks", "Connect4", Connect4Net(6))]
    results = []

    def fill(opt, sizes, params=None):
        rng = np.random.default_rng(0)
        for k, n in enumerate(sizes):
            opt.set("params", k, params[k] if params else rng.standard_normal(n).astype(np.float32) * 0.05)
            opt.set("grads", k, rng.standard_normal(n).astype(np.float32) * 1e-2)

    for net_name, game, net in nets:
        rows = T.muon_classification(game, net, ["policy_2", "value_3"])
        shapes = [tuple(r["shape"]) for r in rows]
        sizes = [int(np.prod(s)) for s in shapes]
        is_muon = [r["path"] == "muon" for r in rows]
        adam_2d = [k for k, r in enumerate(rows) if not is_muon[k] and len(shapes[k]) >= 2]
        params = [p.detach().numpy().reshape(-1) for p in net.parameters()]
        plain = FusedOptimizer(sizes, kind="nadam", beta_1=B1, beta_2=B2, epsilon=EPS)
        fill(plain, sizes, params)
        nadam = statistics.median(plain.step_timed(a.lr, 2, zero_grads=False, repeats=a.steps) for _ in range(a.rounds))
        plain.close()
        for cfg_name, cfg in CONFIGS:
            opt = FusedOptimizer(sizes, kind="nadam", beta_1=B1, beta_2=B2, epsilon=EPS, alpha=ALPHA, muon=dict(adam_tensors=adam_2d), shapes=shapes, **cfg)
            fill(opt, sizes, params)
            arenas = [opt._tensors(i) for i in range(4)] + [opt._tensors(4) if cfg.get("grokfast") else [None] * len(sizes)]
            tensors = [tuple(x) + (shapes[k], is_muon[k], float(rows[k].get("scale", 0.0))) for k, x in enumerate(zip(*arenas))]
            opt.step(a.lr, 1, zero_grads=False)
            torch_step(tensors, cfg, a.lr, 1)
            torch.cuda.synchronize()
            fused, eager = [], []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(a.rounds):                                    # the two sides alternated
                fused.append(opt.step_timed(a.lr, 2, zero_grads=False, repeats=a.steps))
                torch_step(tensors, cfg, a.lr, 2)
                e0.record()
                for i in range(a.steps):
                    torch_step(tensors, cfg, a.lr, 2 + i)
                e1.record()
                e1.synchronize()
                eager.append(e0.elapsed_time(e1) / a.steps)
            r = dict(network=net_name, tensors=len(sizes), muon_tensors=sum(is_muon), elements=int(sum(sizes)), config=cfg_name, fused_ms_per_step=statistics.median(fused),
                     torch_ms_per_step=statistics.median(eager), fused_ms_rounds=fused, torch_ms_rounds=eager, fused_launches_per_step=opt.launches_per_step,
                     nadam_ms_per_step=nadam)
            r["speedup"] = r["torch_ms_per_step"] / r["fused_ms_per_step"]
            print(json.dumps({k: v for k, v in r.items() if not k.endswith("_rounds")}), flush=True)
            results.append(r)
            del tensors, arenas
            opt.close()
    # Gomoku's largest matrix alone
    P, Q = 512, 1800
    opt = FusedOptimizer([P * Q], kind="nadam", beta_1=B1, beta_2=B2, epsilon=EPS, muon=dict(), shapes=[(Q, P)])
    fill(opt, [P * Q])
    ms = statistics.median(opt.step_timed(a.lr, 2, zero_grads=False, repeats=a.steps) for _ in range(a.rounds))
    opt.close()
    flop = 5 * 2 * (P * P * Q + P * P * P + P * P * Q)
    gomoku = next(r for r in results if r["network"].startswith("Gomoku") and r["config"] == "muon")
    p_d1 = dict(rows=Q, cols=P, ms_per_step=ms, gflop_per_step=flop / 1e9, f32_mfma_tflops=flop / (ms * 1e-3) / 1e12, peak_f32_mfma_tflops=PEAK_F32_MFMA_TFLOPS,
                share_of_peak=flop / (ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, share_of_the_gomoku_muon_step=ms / gomoku["fused_ms_per_step"])
    print(json.dumps(p_d1), flush=True)
    out = dict(what=WHAT, device=torch.cuda.get_device_name(0), steps=a.steps, rounds=a.rounds, lr=a.lr, results=results, p_d1=p_d1)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

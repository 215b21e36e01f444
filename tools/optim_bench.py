#!/usr/bin/env python3
"""Measures the fused optimizer step (optim.FusedOptimizer) on an MI355X against the same chain written tensor by tensor in
torch ops ON THE SAME ARENAS — what a caller would write today — for the parameter lists of the 6-block Connect4 and the 10-block Gomoku network
under Nadam, Nadam + Grokfast and Nadam + Grokfast + Orthograd.

  ms per step of both sides from HIP events (gaz_optim_step_timed; torch.cuda.Event around the same number of steps), after a warm-up, the two
      sides alternated in one process, the median over the rounds
  launches per step: the fused side's from gaz_optim_layout; the torch side's as the aten operations one step dispatches (counted on the host by a
      TorchDispatchMode; every one of them is at least one kernel launch)

    python tools/optim_bench.py [--steps 200] [--rounds 5] [--out profiles/optim_step_times.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("nadam", dict(kind="nadam")), ("nadam+grokfast", dict(kind="nadam", grokfast=True, lamb=4.5)),
           ("nadam+grokfast+orthograd", dict(kind="nadam", grokfast=True, lamb=4.5, orthograd=True))]
B1, B2, EPS, ALPHA = 0.9, 0.995, 1e-7, 0.99
WHAT = ("tools/optim_bench.py on one MI355X: ms per optimizer step from HIP events, `steps` steps a round after a warm-up, the fused step "
        "(optim.FusedOptimizer, gaz_optim_step_timed) and the same chain written per tensor in torch ops on the same arenas alternated in one process, "
        "the median over `rounds` rounds. fused_launches_per_step: from gaz_optim_layout; torch_ops_per_step: aten operations one step dispatches, "
        "each at least one kernel launch")


class CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def torch_step(tensors, cfg, lr, t):
    """Orthograd(Grokfast_EMA(Nadam)) per tensor, as Net/Optimizers/*.py state it, with in-place torch ops where the state allows"""
    c1, c2 = 1.0 - B1 ** t, 1.0 - B2 ** t
    lamb = cfg.get("lamb", 0.0)
    for w, g, m, v, e in tensors:
        if cfg.get("orthograd"):
            proj = torch.dot(w, g) / (torch.dot(w, w) + 1e-30)
            go = g - proj * w
            g = go * (torch.linalg.vector_norm(g) / (torch.linalg.vector_norm(go) + 1e-30))
        if cfg.get("grokfast"):
            e.mul_(ALPHA).add_(g, alpha=1.0 - ALPHA)
            g = g + e * lamb
        m.mul_(B1).add_(g, alpha=1.0 - B1)
        v.mul_(B2).addcmul_(g, g, value=1.0 - B2)
        nesterov = (m / c1) * B1 + (g * (1.0 - B1)) / c1
        w.sub_(nesterov / ((v / c2).sqrt() + EPS) * lr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_step_times.json"))
    a = ap.parse_args()
    from grok_alpha_zero_amd.net import Connect4Net, GomokuNet
    from grok_alpha_zero_amd.optim import FusedOptimizer
    nets = [("Connect4, 6 blocks", Connect4Net(6)), ("Gomoku, 10 blocks", GomokuNet(10))]
    results = []
    for net_name, net in nets:
        sizes = [p.numel() for p in net.parameters()]
        for cfg_name, cfg in CONFIGS:
            rng = np.random.default_rng(0)
            opt = FusedOptimizer(sizes, beta_1=B1, beta_2=B2, epsilon=EPS, alpha=ALPHA, **cfg)
            for k, p in enumerate(net.parameters()):
                opt.set("params", k, p.detach().numpy())
                opt.set("grads", k, rng.standard_normal(sizes[k]).astype(np.float32) * 1e-2)
            arenas = [opt._tensors(i) for i in range(4)] + [opt._tensors(4) if cfg.get("grokfast") else [None] * len(sizes)]
            tensors = list(zip(*arenas))
            with CountOps() as counter:
                torch_step(tensors, cfg, a.lr, 1)
            torch_ops = counter.n
            opt.step(a.lr, 1, zero_grads=False)
            torch.cuda.synchronize()
            fused, eager = [], []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(a.rounds):                                    # the two sides alternated
                fused.append(opt.step_timed(a.lr, 2, zero_grads=False, repeats=a.steps))
                torch_step(tensors, cfg, a.lr, 2)                        # warm-up, as step_timed's
                e0.record()
                for i in range(a.steps):
                    torch_step(tensors, cfg, a.lr, 2 + i)
                e1.record()
                e1.synchronize()
                eager.append(e0.elapsed_time(e1) / a.steps)
            r = dict(network=net_name, tensors=len(sizes), elements=int(sum(sizes)), chunks=opt.n_chunks, config=cfg_name, fused_ms_per_step=statistics.median(fused),
                     torch_ms_per_step=statistics.median(eager), fused_ms_rounds=fused, torch_ms_rounds=eager, fused_launches_per_step=opt.launches_per_step,
                     torch_ops_per_step=torch_ops)
            r["speedup"] = r["torch_ms_per_step"] / r["fused_ms_per_step"]
            print(json.dumps({k: v for k, v in r.items() if not k.endswith("_rounds")}), flush=True)
            results.append(r)
            del tensors, arenas
            opt.close()
    out = dict(what=WHAT, device=torch.cuda.get_device_name(0), steps=a.steps, rounds=a.rounds, lr=a.lr, beta_1=B1, beta_2=B2, results=results)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

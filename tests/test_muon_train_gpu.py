"""-m gpu: training with Muon (grok_alpha_zero_amd/train.py with optimizer = "muon") on the HIP build with torch on the
device — the cases of tests/muon_train_cases.py: three Muon steps on the 1-block TicTacToe network with autograd writing straight into the grads
arena, train_generation, and Run(train=dict()) end to end.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py; as in tests/test_train_gpu.py the limit of 90 s is a kill guard: the
first torch convolution of a process loads its library."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_case(name):
    import tempfile
    import time
    import torch  # noqa: F401 — before the library: one HIP runtime in the process
    import muon_train_cases as cases
    t0 = time.time()
    if name == "steps":
        print("muon tensors", cases.steps_case(None), flush=True)
    elif name == "generation":
        with tempfile.TemporaryDirectory() as tmp:
            s = cases.generation_case(tmp, None)
            print({k: s[k] for k in ("generation", "lr", "best_epoch", "steps", "launches_per_step")}, [(e["train_loss"], e["val_loss"]) for e in s["epochs"]], flush=True)
    elif name == "run":
        with tempfile.TemporaryDirectory() as tmp:
            for st in cases.run_case(tmp, None):
                print(st["generation"], st["games"], st["score"]["new"]["val_loss"], st["score"]["current"]["val_loss"], flush=True)
    else:
        raise SystemExit(f"unknown case {name}")
    print(f"{name}: {time.time() - t0:.1f} s", flush=True)


def test_three_muon_steps_on_the_network_equal_the_model_in_every_bit():
    STEPS.run(__file__, "steps", 90)


def test_train_generation_with_muon_records_the_classification():
    STEPS.run(__file__, "generation", 90)


def test_run_trains_with_muon_and_plays_with_the_trained_network():
    STEPS.run(__file__, "run", 90)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

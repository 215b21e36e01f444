"""-m gpu: the fused optimizer step (optim.FusedOptimizer; the "OPTIMIZER" section of include/gaz_engine.h; csrc/optim.hpp) on the HIP build — the
cases of tests/optim_cases.py against tests/optim_model.py, where the launch shapes matter: 16-byte groups and scalar tails, tensors that start
behind pad elements, partial wavefronts, the wavefront butterfly and the LDS stage of a chunk's sums, the ascending sum of a tensor's chunks by
v_readlane, the hardware's f32 division, square root and denormals.  Raw bits everywhere.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py; a step takes a few seconds, its limit is a kill guard."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_case(name):
    import torch  # noqa: F401 — before the library: the views of the arenas need one HIP runtime in the process
    import optim_cases as cases
    kind, _, arg = name.partition(":")
    if kind == "bits":
        combos = [c for c in cases.COMBOS if c["kind"] == int(arg)]
        print("bits", cases.bits_case(None, combos), flush=True)
    elif kind == "edges":
        print("witnesses", cases.witness_case(None), flush=True)
        print("accumulation", cases.accumulation_case(None), flush=True)
        print("round trip", cases.round_trip_case(None), flush=True)
        print(cases.refusal_case(None), flush=True)
    else:
        raise SystemExit(f"unknown case {name}")


@pytest.mark.parametrize("kind", [0, 1])
def test_every_arena_equals_the_model_in_every_bit(kind):
    STEPS.run(__file__, f"bits:{kind}", 60)


def test_witnesses_accumulation_round_trip_and_refusals():
    STEPS.run(__file__, "edges", 60)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

"""-m gpu: Muon in the fused optimizer step (optim.FusedOptimizer(muon=...); the "MUON" part of include/gaz_engine.h; csrc/muon.hpp) on the HIP build —
the cases of tests/muon_cases.py against tests/muon_model.py, where the launch shapes matter: the operand and result layout of
v_mfma_f32_32x32x2_f32 and its accumulation order, the LDS stages, partial tiles at every edge, both orientations, the thin path's float64 sums
over chunks of columns, tensors behind pads.  Raw bits everywhere.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py; a step takes a few seconds, its limit is a kill guard."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_case(name):
    import torch  # noqa: F401 — before the library: one HIP runtime in the process
    import muon_cases as cases
    kind, _, arg = name.partition(":")
    if kind == "bits":
        combos = [c for c in cases.COMBOS if c["ns_steps"] == int(arg)]
        print("bits", cases.bits_case(None, combos), flush=True)
    elif kind == "edges":
        print("witnesses", cases.witness_case(None), flush=True)
        print("round trip", cases.round_trip_case(None), flush=True)
        print(cases.refusal_case(None), flush=True)
    else:
        raise SystemExit(f"unknown case {name}")


@pytest.mark.parametrize("ns_steps", [0, 1, 5])
def test_every_arena_and_every_matrix_equals_the_model_in_every_bit(ns_steps):
    STEPS.run(__file__, f"bits:{ns_steps}", 60)


def test_witnesses_round_trip_and_refusals():
    STEPS.run(__file__, "edges", 60)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

"""-m gpu: batched sequential halving (gaz_engine_config.gumbel_batch = K) of the HIP build against the reference's fixtures, the
oracle, and — with the ResNet evaluator — an engine with gumbel_batch = 1.  The cases are those of tests/gumbel_batch_cases.py.
Bit-equal: no tolerance.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# G = 64: the first and last game of a wavefront's four teams and both ends of the batch; every slot is checked
CONCURRENT_G = {"c4-k7": 64, "c4-k2": 64, "ttt-k4": 64, "gmk-k16": 8, "gmk-k5": 8, "c4-k7-stablemax": 64, "ttt-k4-nonoise": 64}


def test_reference_fixtures():
    STEPS.run(__file__, "fixtures", 120)


@pytest.mark.parametrize("name", sorted(CONCURRENT_G))
def test_concurrent_games_equal_oracle(name):
    STEPS.run(__file__, "concurrent:" + name, 120)


def test_first_move_launch_counts():
    STEPS.run(__file__, "launch-bounds", 120)


@pytest.mark.parametrize("name", ["resnet-c4", "resnet-gmk"])
def test_resnet_evaluator_equals_gumbel_batch_1(name):
    STEPS.run(__file__, name, 180)


def test_mcts_gumbel_class():
    STEPS.run(__file__, "class", 120)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import gumbel_batch_cases as GB
    from oracle import gaz_oracle as O
    name = sys.argv[1]
    if name == "fixtures":
        for fx in GB.GUMBEL_FIXTURES:
            for K in ("m", 3):
                GB.fixture_case(fx, K, None)
            print(f"{fx}: ok", flush=True)
        GB.net_fixture_case(None, K=7)
    elif name.startswith("concurrent:"):
        O.build()
        GB.concurrent_case(O, name.split(":")[1], CONCURRENT_G[name.split(":")[1]], None)
    elif name == "launch-bounds":
        GB.launch_bound_case("Connect4", 32, 7, 7, 13, None)
        GB.launch_bound_case("Gomoku", 64, 16, 16, 21, None)
    elif name in GB.RESNET:
        GB.resnet_case(name)
    elif name == "class":
        O.build()
        for fx in GB.CLASS_FIXTURES:
            GB.class_case(O, fx, None, K=4)
    else:
        raise SystemExit(f"unknown case {name}")
    print("ok", flush=True)

"""-m gpu: batched sequential halving (gaz_engine_config.gumbel_batch = K) of the HIP build against the reference's fixtures, the
oracle, and — with the ResNet evaluator — an engine with gumbel_batch = 1.  The cases are those of tests/gumbel_batch_cases.py.
Bit-equal: no tolerance.

Every GPU step is a child process of its own under a time limit (this file run as a script with the case's name); after a child that
was killed, faulted or ran out of time nothing more is started."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dead = []


def _step(case, seconds):
    if _dead:
        pytest.fail(f"not started: the GPU step {_dead[0]} was killed or ran out of time")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), case], cwd=ROOT, timeout=seconds, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _dead.append(case)
        pytest.fail(f"{case}: no result within {seconds} s")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stderr:
        _dead.append(case)
    print(r.stdout[-4000:])
    assert r.returncode == 0, f"{case}: exit status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"


# G = 64: the first and last game of a wavefront's four teams and both ends of the batch; every slot is checked
CONCURRENT_G = {"c4-k7": 64, "c4-k2": 64, "ttt-k4": 64, "gmk-k16": 8, "gmk-k5": 8, "c4-k7-stablemax": 64, "ttt-k4-nonoise": 64}


def test_reference_fixtures():
    _step("fixtures", 120)


@pytest.mark.parametrize("name", sorted(CONCURRENT_G))
def test_concurrent_games_equal_oracle(name):
    _step("concurrent:" + name, 120)


def test_first_move_launch_counts():
    _step("launch-bounds", 120)


@pytest.mark.parametrize("name", ["resnet-c4", "resnet-gmk"])
def test_resnet_evaluator_equals_gumbel_batch_1(name):
    _step(name, 180)


def test_mcts_gumbel_class():
    _step("class", 120)


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

"""-m gpu: forced playouts and policy target pruning (gaz_engine_config.forced_playouts_k) on the HIP build — the cases of
tests/forced_playouts_cases.py with 64 games at once (four games per wavefront, each forcing and pruning on its own statistics;
Gomoku's 225-child root spread four children to a lane), and the scheduling equalities with the network.  Exact equality
everywhere: no tolerance.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the cases (run in the child)
def _run_case(name):
    import tempfile
    import forced_playouts_cases as cases
    from oracle import gaz_oracle as O
    O.build()
    kind, _, arg = name.partition(":")
    if kind == "hash":
        cases.hash_case(O, arg, 64, None)
    elif kind == "selfplay":
        cases.selfplay_case(O, 64, None, cap=arg == "cap")
    elif kind == "anchors":
        cases.k0_anchor_case(64, None)
        cases.terminal_root_case(O, 64, None)
    elif kind == "samples":
        print(f"samples {arg}: {cases.samples_case(arg, None)} pruned rows", flush=True)
    elif kind == "run_self_play":
        with tempfile.TemporaryDirectory() as tmp:
            cases.run_self_play_case(tmp, None, games=150, G=64)
    elif kind == "refusals":
        for n in sorted(cases.REFUSALS):
            print(n, "->", cases.refusal_case(n, None), flush=True)
    elif kind == "scheduling":
        cases.scheduling_case(arg)
    else:
        raise SystemExit(f"unknown case {name}")


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", ["ttt", "c4-k1", "c4-k4", "gmk"])
def test_sync_searches_equal_the_model_and_policy_is_the_pruned_target(name):
    STEPS.run(__file__, "hash:" + name, 120)


@pytest.mark.parametrize("cap", ["plain", "cap"])
def test_continuous_selfplay_two_trees_equal_the_model(cap):
    STEPS.run(__file__, "selfplay:" + cap, 120)


def test_k_0_anchor_and_terminal_parent_root():
    STEPS.run(__file__, "anchors", 120)


@pytest.mark.parametrize("name", ["c4", "gmk"])
def test_samples_carry_the_pruned_target(name):
    STEPS.run(__file__, "samples:" + name, 120)


def test_run_self_play_reads_the_train_config_key():
    STEPS.run(__file__, "run_self_play", 120)


def test_refusals():
    STEPS.run(__file__, "refusals", 60)


@pytest.mark.parametrize("which", ["fused", "groups", "cache"])
def test_records_do_not_depend_on_scheduling(which):
    STEPS.run(__file__, "scheduling:" + which, 180)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

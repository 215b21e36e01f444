"""-m gpu: the search's random evaluation symmetry (gaz_engine_set_eval_symmetry) on the HIP build — the cases of
tests/eval_symmetry_cases.py at the sizes where the launch shapes matter: 64 games, so that four Connect4 / TicTacToe games with
different k share a wavefront.  Gomoku's 225 cells stride the 64 lanes at any count, so its self-play cases play 4 (PUCT) and 16 (Gumbel)
slots, and the lock-step Connect4 games are capped at 16 plies: both keep the host's side (the oracle's evaluator call-backs, the
row-by-row answers) to seconds.  Then the scheduling equalities with a 1-block network, and whole games with that network against the
oracle.  Exact equality everywhere: no tolerance.

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
    import eval_symmetry_cases as cases
    from oracle import gaz_oracle as O
    O.build()
    kind, _, arg = name.partition(":")
    if kind == "selfplay":
        cases.selfplay_case(O, arg, {"gmk": 4, "gmk-gumbel": 16}.get(arg, 64), None)
    elif kind == "model":
        game, K, forced = arg.split(",")
        widest = cases.model_case(O, game, None, K=int(K), forced_k=float(forced))
        assert int(K) == 1 or widest > 1
    elif kind == "switch":
        game, K = arg.split(",")
        cases.model_case(O, game, None, K=int(K), switch_off_at=2)
    elif kind == "gumbel_batch":
        cases.gumbel_batch_case(arg, 64, None)
    elif kind == "lockstep":
        args = {"ttt": ("TicTacToe", 64, None, 24, 9, 1.25, 1.0), "c4": ("Connect4", 64, None, 40, 16, 2.5, 0.5), "gmk": ("Gomoku", 8, None, 48, 3, 2.5, 0.05)}[arg]
        assert cases.lockstep_case(O, *args) >= 3
    elif kind == "lockstep-gumbel":
        assert cases.lockstep_case(O, "Connect4", 64, None, 32, 16, 0.0, 0.0, gumbel_m=7) >= 3
    elif kind == "equivariant":
        cases.equivariant_case("Connect4", 64, None, 40, 42, 2.5, 0.5)
    elif kind == "samples":
        cases.samples_case(arg, 64, None)
    elif kind == "run_self_play":
        with tempfile.TemporaryDirectory() as tmp:
            cases.run_self_play_case(O, tmp, None, games=96, G=64, game="Connect4")
    elif kind == "mcts":
        cases.mcts_class_case(O, "Connect4", None, 60)
        cases.mcts_gumbel_class_case(O, None)
    elif kind == "refusals":
        cases.abi_case(None)
        for k, m in cases.refusal_case(None).items():
            print(k, "->", m, flush=True)
    elif kind == "scheduling":
        cases.scheduling_case(arg)
    elif kind == "network":
        cases.network_case(O)
    else:
        raise SystemExit(f"unknown case {name}")


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", ["ttt", "c4", "gmk", "c4-gumbel", "gmk-gumbel"])
def test_selfplay_equals_the_oracle_with_the_wrapped_evaluator(name):
    STEPS.run(__file__, "selfplay:" + name, 180)


@pytest.mark.parametrize("arg", ["Connect4,4,0", "Connect4,16,0", "Connect4,1,2", "Gomoku,4,0", "TicTacToe,16,0"])
def test_engine_equals_the_models_with_the_wrapped_evaluator(arg):
    STEPS.run(__file__, "model:" + arg, 120)


def test_mode_0_after_mode_1_between_moves():
    STEPS.run(__file__, "switch:Connect4,4", 120)


@pytest.mark.parametrize("name", ["c4-gumbel", "gmk-gumbel"])
def test_gumbel_batch_4_equals_1(name):
    STEPS.run(__file__, "gumbel_batch:" + name, 120)


@pytest.mark.parametrize("name", ["ttt", "c4", "gmk"])
def test_lockstep_through_the_external_evaluator(name):
    STEPS.run(__file__, "lockstep:" + name, 180)


def test_lockstep_through_the_external_evaluator_gumbel():
    STEPS.run(__file__, "lockstep-gumbel", 180)


def test_an_equivariant_evaluator_gives_the_off_records():
    STEPS.run(__file__, "equivariant", 120)


@pytest.mark.parametrize("name", ["c4", "c4-gumbel"])
def test_drain_samples_equals_record_to_samples(name):
    STEPS.run(__file__, "samples:" + name, 120)


def test_run_self_play_reads_the_key():
    STEPS.run(__file__, "run_self_play", 120)


def test_mcts_classes():
    STEPS.run(__file__, "mcts", 120)


def test_refusals():
    STEPS.run(__file__, "refusals", 120)


@pytest.mark.parametrize("which", ["fused", "groups", "cache"])
def test_records_do_not_depend_on_scheduling(which):
    STEPS.run(__file__, "scheduling:" + which, 180)


def test_the_real_network_against_the_oracle():
    STEPS.run(__file__, "network", 180)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

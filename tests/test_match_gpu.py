"""-m gpu: match play (gaz_engine_set_match) on the HIP build — the cases of tests/match_cases.py at the sizes where
the launch shapes matter: 64 games (one full block of the routing kernels, four Connect4 / TicTacToe games per tree wavefront), the ragged
counts 1, 3, 67 and 9 (blocks that are not full, a second block of three rows; Gomoku's 450-byte rows are copied in 2-byte units), then two
real 1-block networks against the evaluators of two ordinary engines, and play_match end to end.  Exact equality everywhere.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the cases (run in the child)
def _run_case(name):
    import match_cases as cases
    from oracle import gaz_oracle as O
    O.build()
    kind, _, arg = name.partition(":")
    if kind == "selfplay":                           # 64 games, SLOTS64 against the model; Gomoku one game per slot (the model's searches are the host's time)
        cases.selfplay_case(O, arg, 64, None, per_slot=1 if arg == "gmk" else 2)
    elif kind == "anchor":
        cases.anchor_case(arg, 64, None, **(cases.ANCHOR_ALL if arg == "c4" else {}))
    elif kind == "ragged":
        game, G = arg.split(",")
        cases.selfplay_case(O, game, int(G), None, per_slot=2 if int(G) <= 3 else 1, slots=range(int(G)))
    elif kind == "network":
        game, G = arg.split(",")
        cases.network_case(O, game, int(G), slots={64: None, 9: (0, 1, 8)}.get(int(G), range(int(G))))   # (Gomoku: the model's searches are the host's time)
    elif kind == "play_match":
        cases.play_match_case()
    elif kind == "refusals":
        for k, m in cases.refusal_case(None).items():
            print(k, "->", m, flush=True)
        print(cases.weights_b_refusal_case(), flush=True)
    else:
        raise SystemExit(f"unknown case {name}")


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", ["ttt", "c4", "gmk", "ttt-gumbel", "c4-gumbel"])
def test_match_games_are_the_models(name):
    STEPS.run(__file__, "selfplay:" + name, 180)


@pytest.mark.parametrize("name", ["c4", "c4-gumbel", "gmk"])
def test_same_network_twice_is_match_off(name):
    STEPS.run(__file__, "anchor:" + name, 180)


@pytest.mark.parametrize("arg", ["c4,1", "c4,3", "c4,67", "gmk,1", "gmk,9"])
def test_ragged_game_counts(arg):
    STEPS.run(__file__, "ragged:" + arg, 180)


@pytest.mark.parametrize("arg", ["Connect4,64", "Connect4,67", "Gomoku,9"])
def test_two_networks_against_two_ordinary_engines(arg):
    STEPS.run(__file__, "network:" + arg, 240)


def test_play_match_end_to_end():
    STEPS.run(__file__, "play_match", 180)


def test_refusals():
    STEPS.run(__file__, "refusals", 120)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

"""-m gpu: the held-out loss (SelfPlayEngine.score_outputs / score_replay; the "HELD-OUT LOSS" section of include/gaz_engine.h; csrc/score.hpp)
on the HIP build — the cases of tests/score_cases.py against tests/score_model.py, where the launch shapes matter: k_score_rows at 1 .. 257 rows
for all three games (four rows per wavefront with partial teams and partial waves for TicTacToe and Connect4, one row per wavefront for Gomoku,
a second block of 128 for k_score_blocks), score_replay with the hash evaluator (Gomoku at 9 and 129 rows, Connect4 at 300) and with the 1-block
Connect4 network, whose predictions the model takes from engine.evaluate() of the same boards, so that the comparison is exact; a logits head
with softmax and with Stablemax.  Raw bits everywhere; batch_torch is not needed.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py; a step takes a few seconds, its limit is a kill guard."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_case(name):
    import tempfile
    import score_cases as cases
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL
    kind, _, arg = name.partition(":")
    if kind == "outputs":
        print(arg, cases.outputs_case(arg, None), flush=True)
        if arg == "TicTacToe":
            print("two game groups", cases.outputs_case(arg, None, grouped=True), flush=True)
            cases.own_mode_case(None)
    elif kind == "replay":
        sizes = {"Gomoku": (9, 129), "Connect4": (300,), "TicTacToe": cases.REPLAY_SIZES}[arg]
        print(arg, cases.replay_case(arg, None, sizes=sizes), flush=True)
        if arg == "Connect4":
            print("splits", cases.split_case(arg, None), flush=True)
        if arg == "TicTacToe":
            print("untouched", cases.untouched_case(None), flush=True)
            print(cases.refusal_case(None), flush=True)
            with tempfile.TemporaryDirectory() as tmp:
                print("drained", cases.drained_case(tmp, None), flush=True)
    elif kind == "net":
        kw, mode = {"probabilities": (None, 0), "softmax": (dict(policy_is_logits=1, search=SEARCH_GUMBEL, gumbel_m=4), 1),
                    "stablemax": (dict(policy_is_logits=1, search=SEARCH_GUMBEL, gumbel_m=4, gumbel_stablemax=True), 3)}[arg]
        sizes = (1, 3, 129, 257) if arg == "probabilities" else (3, 129)
        for M_rows, (val_loss, top1, ms) in cases.net_case(kw, mode, sizes=sizes).items():
            print(f"{arg}: M {M_rows} val_loss {val_loss!r} top1 {top1!r} ms {ms:.3f}", flush=True)
    else:
        raise SystemExit(f"unknown case {name}")


@pytest.mark.parametrize("game", ["TicTacToe", "Connect4", "Gomoku"])
def test_score_outputs_equals_the_model_in_every_bit(game):
    STEPS.run(__file__, "outputs:" + game, 60)


@pytest.mark.parametrize("game", ["TicTacToe", "Connect4", "Gomoku"])
def test_score_replay_with_the_hash_evaluator(game):
    STEPS.run(__file__, "replay:" + game, 60)


def test_score_replay_with_the_one_block_network():
    STEPS.run(__file__, "net:probabilities", 60)


@pytest.mark.parametrize("head", ["softmax", "stablemax"])
def test_score_replay_of_a_logits_head(head):
    STEPS.run(__file__, "net:" + head, 60)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

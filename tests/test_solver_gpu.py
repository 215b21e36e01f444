"""-m gpu: the solver (gaz_engine_set_solver) on the HIP build — the cases of tests/solver_cases.py at the sizes
where the launch shapes matter: 64 TicTacToe / Connect4 games, so that the four games of a wavefront sit in different proof states, and
Gomoku on 4 slots.  The Python model replays the four games of the first wavefront plus one game of every other wavefront (whole Connect4
games from the empty board: the first wavefront and two more slots, which keeps the model's side to seconds); the minimax check runs on
those slots.  Then the scheduling equalities with a 1-block network, and games with that network against the model.  Exact equality
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
    import solver_cases as cases
    from oracle import gaz_oracle as O
    O.build()
    kind, _, arg = name.partition(":")
    if kind == "sync":
        gmk = arg.startswith("gmk")
        G = 4 if gmk else 64
        w, _, stats = cases.sync_case(O, arg, G, None, slots=None if gmk else cases.gpu_slots(G))
        if arg.startswith("ttt"):
            assert w.proven_nodes > 0 and w.proven_hits > 0 and w.masked_levels > 0 and w.root_draw > 0 and w.zero_sim_moves > 0
            assert w.minimax_checked == w.statuses_checked > 0
        elif arg.startswith("c4"):
            assert w.proven_nodes > 0 and w.masked_levels > 0 and w.root_win > 0 and w.root_loss > 0 and w.zero_sim_moves > 0 and w.short_moves > 0
            assert w.restricted_rows > 0 and w.minimax_checked > 100
        elif arg == "gmk-four-one-end":
            assert w.masked_levels > 0 and w.restricted_rows == G
        else:
            assert w.zero_sim_moves >= 1 and w.root_win >= 1
        assert stats["proven_moves"] > 0 or gmk
    elif kind == "switch":
        w, _, _ = cases.sync_case(O, "c4-16", 64, None, slots=cases.gpu_slots(), switch={16: False, 19: True, 24: False, 26: True})
        assert w.statuses_checked > 0 and w.root_win + w.root_loss > 0
    elif kind == "selfplay":
        w, _ = cases.selfplay_case(O, arg, 64, None, slots=cases.gpu_slots() if arg == "ttt" else (0, 1, 2, 3, 32, 63))
        assert w.proven_nodes > 0 and w.masked_levels > 0 and w.zero_sim_moves > 0 and w.restricted_rows > 0
    elif kind == "forced":
        w, _ = cases.selfplay_case(O, "c4", 64, None, slots=(0, 1, 2, 3, 63), forced_k=2.0)
        assert w.restricted_rows > 0 and w.masked_levels > 0
    elif kind == "cap":
        w, _ = cases.selfplay_case(O, "c4", 64, None, slots=(0, 1, 2, 3, 16, 32, 48, 63), cap=(40, 0.4))
        assert getattr(w, "fast_proven", 0) > 0, w
    elif kind == "quiet":
        cases.quiet_anchor_case(64, None)
        cases.differs_from_off_case("ttt", 64, None)
    elif kind == "resign":
        assert cases.resign_case(O, "c4", 64, None) >= 1
    elif kind == "samples":
        cases.samples_case("ttt", 64, None)
    elif kind == "run_self_play":
        with tempfile.TemporaryDirectory() as tmp:
            cases.run_self_play_case(tmp, None, games=96, G=64)
    elif kind == "mcts":
        assert cases.mcts_class_case(O, None) > 0
    elif kind == "refusals":
        msgs = {n: cases.refusal_case(n, None) for n in cases.REFUSALS}
        msgs.update(cases.abi_case(None))
        assert len(set(msgs.values())) == len(msgs), msgs
    elif kind == "scheduling":
        cases.scheduling_case(arg)
    elif kind == "network":
        cases.network_case(O)
    else:
        raise SystemExit(f"unknown case {name}")


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", ["ttt", "ttt-two-trees-tau", "c4-20-two-trees", "c4-24-compact-no-noise", "gmk-open-four", "gmk-four-one-end"])
def test_sync_games_equal_the_model_and_minimax(name):
    STEPS.run(__file__, "sync:" + name, 180)


def test_switching_between_moves():
    STEPS.run(__file__, "switch", 180)


@pytest.mark.parametrize("name", ["ttt", "c4"])
def test_continuous_selfplay_equals_the_model(name):
    STEPS.run(__file__, "selfplay:" + name, 180)


def test_forced_playouts():
    STEPS.run(__file__, "forced", 180)


def test_playout_cap():
    STEPS.run(__file__, "cap", 180)


def test_quiet_anchor_and_records_that_differ():
    STEPS.run(__file__, "quiet", 120)


def test_resignation():
    STEPS.run(__file__, "resign", 120)


def test_drain_samples_equals_record_to_samples():
    STEPS.run(__file__, "samples", 120)


def test_run_self_play_reads_the_key():
    STEPS.run(__file__, "run_self_play", 120)


def test_mcts_class():
    STEPS.run(__file__, "mcts", 120)


def test_refusals_and_abi():
    STEPS.run(__file__, "refusals", 120)


@pytest.mark.parametrize("which", ["fused", "groups", "cache"])
def test_records_do_not_depend_on_scheduling(which):
    STEPS.run(__file__, "scheduling:" + which, 180)


def test_the_real_network_against_the_model():
    STEPS.run(__file__, "network", 180)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

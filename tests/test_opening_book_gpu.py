"""-m gpu: the opening book (gaz_engine_set_opening_book; csrc/book.hpp, csrc/book_start.hpp) on the HIP build — the cases of
tests/opening_book_cases.py at the sizes where the launch shapes matter: 64 Connect4 and TicTacToe games (four 16-lane teams per wavefront
start from the book side by side), 9 Gomoku games, 67 Connect4 games (a partial team row), and the 1-block network with the fused launch,
two game groups and the evaluation cache against separate launches with one group.  Exact equality everywhere.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py; a step takes a few seconds, its limit is a kill guard."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = (0, 1, 15, 16, 31, 32, 62, 63)             # both ends of a wavefront's four teams, both ends of the batch


# ------------------------------------------------------------------------------------------------ the cases (run in the child)
def _run_case(name):
    import tempfile
    import opening_book_cases as cases
    from oracle import gaz_oracle as O
    O.build()
    kind, _, arg = name.partition(":")
    if kind == "oracle":
        case, _, g = arg.partition("@")
        G = int(g)
        cases.oracle_case(O, case, None, G=G, slots=SLOTS + (64, 66) if G > 16 else None)
    elif kind == "pairs":
        cases.pairs_case(None, G=64)
        cases.match_owner_case(None)
        cases.match_result_case()
        print({k: v for k, v in cases.play_match_case(None, games=256, n_slots=64).items() if k != "match_stats"}, flush=True)
    elif kind == "anchors":
        for case, feature in (("c4-puct", "plain"), ("c4-gumbel", "plain"), ("ttt-puct", "opening"), ("ttt-puct", "solver"), ("ttt-puct", "symmetry"), ("ttt-puct", "forced"),
                              ("ttt-puct", "cap"), ("ttt-puct", "resign"), ("ttt-puct", "match"), ("ttt-gumbel", "match")):
            print(case, feature, cases.empty_book_case(None, case, feature), flush=True)
        cases.removal_case(None)
        for case, prefix in (("c4-puct", cases.C4_LONG), ("c4-gumbel", [2, 4, 4]), ("ttt-puct", cases.TTT_ALMOST_FULL)):
            cases.set_position_anchor_case(None, case, prefix)
    elif kind == "composition":
        cases.leaf_batch_case(O, None, G=16)
        cases.single_tree_case(O, None, G=16)
        cases.same_records_case(None, "c4-gumbel", dict(gumbel_batch=4), dict(gumbel_batch=1), G=16)
        cases.same_records_case(None, "c4-puct", dict(game_groups=5), dict(game_groups=1), G=5)
        cases.same_records_case(None, "c4-puct", dict(game_groups=2), dict(game_groups=1), G=67)
        cases.same_records_case(None, "c4-puct", dict(game_groups=1), dict(game_groups=1), G=67, repack=True)
    elif kind == "samples":
        print(cases.samples_case(None, G=64), cases.samples_case(None, G=64, fast_iterations=6, full_search_prob=0.5), flush=True)
        print(cases.samples_case(None, name="gmk-puct", G=9, games_per_slot=2), flush=True)
        print(cases.surprise_case(O, None, G=64), cases.resign_case(None, G=64), flush=True)
    elif kind == "run":
        msgs = cases.refusal_case(None)
        print(len(msgs), "refusals", flush=True)
        cases.helpers_case()
        with tempfile.TemporaryDirectory() as tmp:
            print(cases.run_self_play_case(O, tmp, None, games=150, G=64), flush=True)
    elif kind == "network":
        cases.scheduling_case(arg)
    else:
        raise SystemExit(f"unknown case {name}")


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("arg", ["c4-puct@64", "c4-gumbel@64", "c4-cap@64", "ttt-puct@64", "ttt-gumbel@64", "gmk-puct@9", "gmk-gumbel@9", "c4-puct@67"])
def test_games_from_the_book_equal_the_oracle(arg):
    """four games per slot; 64 games fill a wavefront's four teams sixteen times over, 67 leave a partial team row, 9 Gomoku games are nine
    wavefronts; the sampled slots are the oracle's games from the entry the restated draw names, every game carries its entry's prefix"""
    STEPS.run(__file__, "oracle:" + arg, 60)


def test_pairs_match_owners_match_result_and_play_match():
    STEPS.run(__file__, "pairs", 60)


def test_anchors_empty_book_removal_and_set_position():
    STEPS.run(__file__, "anchors", 60)


def test_leaf_batch_gumbel_batch_single_tree_groups_and_repack():
    STEPS.run(__file__, "composition", 60)


def test_samples_surprise_weighting_and_resignation():
    STEPS.run(__file__, "samples", 60)


def test_refusals_helpers_and_run_self_play():
    STEPS.run(__file__, "run", 60)


@pytest.mark.parametrize("which", ["fused", "groups", "cache"])
def test_network_scheduling_does_not_change_the_games(which):
    """1-block Connect4 network, 64 games from a five-entry book: the fused launch / two game groups / the evaluation cache give the records
    of separate launches with one group; stats()["fused_wave"] is non-zero where it is without a book (selfplay_support asserts it)"""
    STEPS.run(__file__, "network:" + which, 60)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

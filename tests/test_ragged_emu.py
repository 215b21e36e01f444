"""CPU suite: the tree kernels at game counts that fill no wave, block or tile (tests/ragged_cases.py) on the
emulation build of the device code.  The one-lane emulation has no teams, tree blocks or tiles: what it checks here is the host side of
a ragged count (launch sizes, the budget rule, the game groups' split, repack) and the case bodies themselves; the launch shapes are the
-m gpu suite's (tests/test_ragged_gpu.py).  Exact equality everywhere."""
import pytest

import degenerate_cases
import gumbel_batch_cases
import ragged_cases as cases
from selfplay_support import emu_lib  # noqa: F401

SELFPLAY = [("Connect4", "puct", {}), ("TicTacToe", "puct", {}), ("Gomoku", "puct", {}), ("Connect4", "puct", dict(compact_trees=1)),
            ("Connect4", "gumbel", {}), ("TicTacToe", "gumbel", {})]


# ------------------------------------------------------------------------------------------------ A.1
@pytest.mark.parametrize("game,search,kw,n", [(g, s, kw, n) for g, s, kw in SELFPLAY for n in cases.sizes_of(g)])
def test_selfplay_of_a_ragged_count_equals_the_oracle(emu_lib, oracle, game, search, kw, n):
    cases.selfplay_case(oracle, game, search, n, emu_lib, **kw)


# ------------------------------------------------------------------------------------------------ A.2
@pytest.mark.parametrize("G", (1, 3, 5))
@pytest.mark.parametrize("game,K", [("TicTacToe", 4), ("TicTacToe", 16), ("Connect4", 4), ("Connect4", 16)])
def test_leaf_batched_search_of_a_ragged_count_equals_the_model(emu_lib, oracle, game, K, G):
    degenerate_cases.leaf_batch_case(oracle, game, "uniform", K, G, emu_lib)


@pytest.mark.parametrize("G", (1, 3, 5))
@pytest.mark.parametrize("name", ("c4-k7", "c4-k2", "ttt-k4"))
def test_batched_gumbel_search_of_a_ragged_count_equals_the_oracle(emu_lib, oracle, name, G):
    gumbel_batch_cases.concurrent_case(oracle, name, G, emu_lib)


# ------------------------------------------------------------------------------------------------ A.3
@pytest.mark.parametrize("n,k", cases.GROUPS)
@pytest.mark.parametrize("search", ("puct", "gumbel"))
def test_game_groups_of_a_ragged_count_play_exactly_the_budget(emu_lib, oracle, search, n, k):
    cases.groups_case(oracle, search, n, k, emu_lib)


# ------------------------------------------------------------------------------------------------ A.4
def test_repack_to_one_slot_keeps_every_tictactoe_game(emu_lib, oracle):
    cases.repack_case(oracle, "puct-ttt", emu_lib)


def test_repack_to_one_slot_keeps_every_gomoku_game_with_staggered_starts(emu_lib, oracle):
    """(nine slots: the body of the -m gpu case, whose starts are staggered because capped Gomoku games all finish together)"""
    cases.repack_case(oracle, "puct-gmk", emu_lib)

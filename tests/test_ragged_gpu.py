"""-m gpu: every launch shape of the HIP build at game counts that fill no wave, block or tile — the cases of tests/ragged_cases.py
(DESIGN.md section 20).  A: the tree kernels with the hash evaluator against the oracle (four 16-lane teams per wavefront for Connect4 and
TicTacToe, one game per wavefront for Gomoku).  B: the one-launch wave (tree blocks + trunk workgroups, completion queue) with a real
network against a regular engine of 128 slots that runs separate launches, and against the oracle.  Bit-equal: no tolerance.  Every case
of B prints its witnesses (fused_wave, fused_faults, game_groups, records) and asserts them.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ A.1
@pytest.mark.parametrize("game", ("Connect4", "TicTacToe", "Gomoku"))
def test_puct_selfplay_of_ragged_counts_equals_the_oracle(game):
    STEPS.run(__file__, f"selfplay:puct:{game}", 240, tail=6000)


def test_puct_selfplay_of_ragged_counts_with_reroot_compaction():
    STEPS.run(__file__, "selfplay:compact:Connect4", 240, tail=6000)


@pytest.mark.parametrize("game", ("Connect4", "TicTacToe"))
def test_gumbel_selfplay_of_ragged_counts_equals_the_oracle(game):
    STEPS.run(__file__, f"selfplay:gumbel:{game}", 240, tail=6000)


@pytest.mark.parametrize("game", ("Connect4", "TicTacToe"))
def test_gumbel_selfplay_of_ragged_counts_four_games_per_wavefront(game):
    """GAZ_TREE_TEAMS=1: k_wave_gumbel_teams (16-lane teams) instead of one game per wavefront"""
    STEPS.run(__file__, f"selfplay:gumbel:{game}", 240, env={"GAZ_TREE_TEAMS": "1"}, tail=6000)


# ------------------------------------------------------------------------------------------------ A.2
@pytest.mark.parametrize("game,K", [("TicTacToe", 4), ("TicTacToe", 16), ("Connect4", 4), ("Connect4", 16)])
def test_leaf_batched_search_of_ragged_counts_equals_the_model(game, K):
    STEPS.run(__file__, f"leaf:{game}:{K}", 240, tail=6000)


@pytest.mark.parametrize("name", ("c4-k7", "c4-k2", "ttt-k4", "gmk-k16"))
def test_batched_gumbel_search_of_ragged_counts_equals_the_oracle(name):
    STEPS.run(__file__, f"gumbel-batch:{name}", 240, tail=6000)


# ------------------------------------------------------------------------------------------------ A.3
@pytest.mark.parametrize("search", ("puct", "gumbel"))
def test_game_groups_of_ragged_counts_play_exactly_the_budget(search):
    STEPS.run(__file__, f"groups:{search}", 240, tail=6000)


# ------------------------------------------------------------------------------------------------ A.4
@pytest.mark.parametrize("name", ("gumbel-c4", "puct-ttt", "puct-gmk"))
def test_repack_to_one_slot_keeps_every_game(name):
    STEPS.run(__file__, f"repack:{name}", 240, tail=6000)


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("case", ["puct", "puct-cache", "gumbel", "gumbel-one-game-per-wave", "gomoku", "gomoku2"])
def test_one_launch_wave_of_ragged_counts_equals_the_regular_engine_and_the_oracle(case):
    """gomoku: the 1-block network, for which the evaluator declines the one-launch form at every size (resnet.hip fusable(): blocks > 1) —
    asserted as fused_wave == 0; gomoku2: the 2-block network, fused_wave == 1"""
    STEPS.run(__file__, f"net:{case}", 240, env={"GAZ_FUSE_GUMBEL_TEAMS": "0"} if case == "gumbel-one-game-per-wave" else None, tail=6000)


@pytest.mark.parametrize("kind", ("puct", "gumbel"))
def test_one_launch_wave_of_ragged_game_groups(kind):
    STEPS.run(__file__, f"net-groups:{kind}", 240, tail=6000)


@pytest.mark.parametrize("kind", ("gumbel", "gomoku2"))
def test_one_launch_wave_repacked_to_one_slot(kind):
    STEPS.run(__file__, f"net-repack:{kind}", 240, tail=6000)


@pytest.mark.parametrize("n", (5, 17))
def test_bounded_wait_gives_up_on_a_partial_tile_without_changing_games(n):
    STEPS.run(__file__, f"net-giveup:{n}", 240, tail=6000)


# ------------------------------------------------------------------------------------------------ the steps (run in the child)
def _run(name):
    import degenerate_cases
    import gumbel_batch_cases
    import ragged_cases as cases
    from oracle import gaz_oracle as O
    O.build()
    what, _, rest = name.partition(":")
    if what == "selfplay":
        search, game = rest.split(":")
        kw = dict(compact_trees=1) if search == "compact" else {}
        for n in cases.sizes_of(game):
            cases.selfplay_case(O, game, "gumbel" if search == "gumbel" else "puct", n, None, **kw)
    elif what == "leaf":
        game, K = rest.split(":")
        for G in (1, 3, 5):
            degenerate_cases.leaf_batch_case(O, game, "uniform", int(K), G, None)
    elif what == "gumbel-batch":
        for G in (1, 3, 5):
            gumbel_batch_cases.concurrent_case(O, rest, G, None)
    elif what == "groups":
        for n, k in cases.GROUPS:
            cases.groups_case(O, rest, n, k, None)
    elif what == "repack":
        cases.repack_case(O, rest, None, G=67, budget=200)
    elif what == "net":
        kind = "gumbel" if rest.startswith("gumbel") else ("puct" if rest.startswith("puct") else rest)
        cases.net_sizes_case(O, kind, **(dict(eval_cache_log2=12) if rest == "puct-cache" else {}))
    elif what == "net-groups":
        cases.net_groups_case(rest)
    elif what == "net-repack":
        cases.net_repack_case(rest, gpb=64)          # queue_gpb of one batch: Gumbel 4 rounds x 16 games, Gomoku 8 rounds x 8 (engine.hip one_wave)
    elif what == "net-giveup":
        cases.net_giveup_case(int(rest))
    else:
        raise SystemExit(f"unknown step {name}")


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run(sys.argv[1])
    print("ok", flush=True)

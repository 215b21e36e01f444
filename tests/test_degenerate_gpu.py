"""-m gpu: the searches of the HIP build on tied, zero and saturated evaluator outputs (tests/degenerate_eval.py) — the cases of
tests/degenerate_cases.py with 64 games at once (four 16-lane teams per wavefront for TicTacToe and Connect4, one game per wavefront
for Gomoku), where the tie rules are cross-lane butterflies (wave.hpp) and not the serial loops of the emulation build.  Bit-equal: no
tolerance.  Every step prints its witness counts (tied plies, collisions, zero-mass rows) and asserts them.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES3 = ("TicTacToe", "Connect4", "Gomoku")


# ------------------------------------------------------------------------------------------------ a.
@pytest.mark.parametrize("game", GAMES3)
def test_puct_selfplay_on_tied_priors_equals_the_oracle(game):
    STEPS.run(__file__, f"puct-ties:{game}", 240)


@pytest.mark.parametrize("game", GAMES3)
def test_puct_selfplay_on_zero_mass_rows_equals_the_oracle(game):
    STEPS.run(__file__, f"puct-zeromass:{game}", 240)


# ------------------------------------------------------------------------------------------------ b.
@pytest.mark.parametrize("game", GAMES3)
def test_gumbel_selfplay_equals_the_oracle_at_both_batch_sizes(game):
    STEPS.run(__file__, f"gumbel:{game}", 240)


def test_gumbel_connect4_four_games_per_wavefront():
    """GAZ_TREE_TEAMS=1: k_wave_gumbel_teams (16-lane teams) instead of one game per wavefront; the batched step is a team kernel either way"""
    STEPS.run(__file__, "gumbel:Connect4", 240, env={"GAZ_TREE_TEAMS": "1"})


# ------------------------------------------------------------------------------------------------ c.
@pytest.mark.parametrize("game,K", [("TicTacToe", 4), ("TicTacToe", 16), ("Connect4", 4), ("Connect4", 16), ("Gomoku", 16)])
def test_leaf_batched_search_equals_the_model(game, K):
    STEPS.run(__file__, f"leaf:{game}:{K}", 240)


@pytest.mark.parametrize("game", ("TicTacToe", "Connect4"))
def test_forced_playouts_equal_the_model(game):
    STEPS.run(__file__, f"forced:{game}", 240)


@pytest.mark.parametrize("game", ("TicTacToe", "Connect4"))
def test_leaf_batched_search_without_noise_sees_tied_priors(game):
    STEPS.run(__file__, f"leaf-no-noise:{game}", 240)


# ------------------------------------------------------------------------------------------------ d.
@pytest.mark.parametrize("game", ("TicTacToe", "Connect4"))
def test_tree_readout_after_a_uniform_search(game):
    STEPS.run(__file__, f"readout:{game}", 240)


# ------------------------------------------------------------------------------------------------ e.
@pytest.mark.parametrize("case", ["groups1", "groups2", "groups1-cache", "groups2-cache", "gumbel", "gumbel-one-game-per-wave", "gomoku"])
def test_constant_network_in_the_production_launch_shape(case):
    STEPS.run(__file__, f"net:{case}", 240, env={"GAZ_FUSE_GUMBEL_TEAMS": "0"} if case == "gumbel-one-game-per-wave" else None)


# ------------------------------------------------------------------------------------------------ the steps (run in the child)
def _run(name):
    import degenerate_cases as cases
    from oracle import gaz_oracle as O
    O.build()
    what, _, rest = name.partition(":")
    if what == "puct-ties":
        cases.puct_ties_case(O, rest, 64, None, cases.HIP_SLOTS[rest])
    elif what == "puct-zeromass":
        cases.puct_selfplay_case(O, rest, "zeromass", 64, None, cases.HIP_SLOTS[rest])
    elif what == "gumbel":
        for config in cases.GUMBEL_CONFIGS:
            cases.gumbel_selfplay_case(O, rest, config, 64, None)
    elif what == "leaf":
        game, K = rest.split(":")
        for kind in ("dups", "zeromass") if game == "Gomoku" else ("uniform", "dups", "zeromass"):
            cases.leaf_batch_case(O, game, kind, int(K), 8 if game == "Gomoku" else 64, None)     # (Gomoku: one game per wavefront)
    elif what == "forced":
        for K in (1, 16):
            for kind in ("uniform", "dups", "zeromass"):
                cases.leaf_batch_case(O, rest, kind, K, 64, None, forced_k=2.0)
    elif what == "leaf-no-noise":
        for kind in ("uniform", "dups"):
            for forced_k in (0.0, 2.0):
                cases.leaf_batch_case(O, rest, kind, 16, 64, None, forced_k=forced_k, dirichlet=False)
    elif what == "readout":
        for K in (1, 4):
            cases.leaf_batch_case(O, rest, "uniform", K, 64, None, readout=True)
        cases.leaf_batch_case(O, rest, "uniform", 16, 64, None, readout=True, dirichlet=False)
    elif what == "net":
        if rest.startswith("groups"):
            st, tied = cases.network_case(O, "Connect4", game_groups=int(rest[6]), eval_cache_log2=14 if rest.endswith("cache") else 0)
            assert st["game_groups"] == int(rest[6]) and (st["cache_hits"] > 0) == rest.endswith("cache"), st
            assert st["fused_wave"] == 1, st
            assert tied >= 1, "no ply with a tied maximum of root_N in the compared games"
        elif rest.startswith("gumbel"):
            st, _ = cases.network_case(O, "Connect4", gumbel=True, game_groups=1)
            assert st["fused_wave"] == 1, st
        else:
            cases.network_case(O, "Gomoku", G=256, game_groups=1)
    else:
        raise SystemExit(f"unknown step {name}")


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run(sys.argv[1])
    print("ok", flush=True)

"""CPU suite: the search's random evaluation symmetry (gaz_engine_set_eval_symmetry) on the emulation build of the device code — the
cases of tests/eval_symmetry_cases.py at sizes the one-lane emulation plays in seconds.  Exact equality everywhere.  Every test switches
the symmetry on, so none of them passes on a library without the entry points."""
import numpy as np
import pytest

import eval_symmetry_cases as cases
import eval_symmetry_model as M
from selfplay_support import emu_lib  # noqa: F401


# ------------------------------------------------------------------------------------------------ the restated rule and the shipped helpers
def test_model_transforms_are_the_augmentation_list_and_games_py_agrees(emu_lib):
    """the model's index arithmetic == numpy's flips and rotations in the order of games._GridGame.augment_sample; the helpers of games.py
    == the model; T_k^-1(T_k) is the identity and the inverse table is [0, 1, 2, 7, 4, 5, 6, 3]"""
    from grok_alpha_zero_amd.games import GAMES
    cases.abi_case(emu_lib)
    rng = np.random.default_rng(1)
    for game, (H, W, Cc, A) in (("TicTacToe", (3, 3, 2, 9)), ("Gomoku", (15, 15, 2, 225)), ("Connect4", (6, 7, 4, 7))):
        s = rng.integers(-1, 2, size=(H, W, Cc)).astype(np.int8)
        p = rng.random(A).astype(np.float32)
        if game != "Connect4":
            aug_s, aug_p = GAMES[game]().augment_sample(s[None], p[None])
        for k in range(M.NSYM[game]):
            t = M.transform(game, s, k)
            np.testing.assert_array_equal(GAMES[game].symmetry_transform(s, k), t)
            np.testing.assert_array_equal(GAMES[game].symmetry_untransform_policy(p, k), M.untransform_policy(game, p, k, H, W))
            if game != "Connect4":
                np.testing.assert_array_equal(t, aug_s[k, 0])
                np.testing.assert_array_equal(M.untransform_policy(game, aug_p[k, 0], k, H, W), p)         # T_k^-1 of T_k(policy)
                np.testing.assert_array_equal(M.transform(game, M.transform(game, s, k), M.INVERSE[k]), s)
            else:
                np.testing.assert_array_equal(t, s[:, ::-1] if k else s)                                   # the column mirror, all four planes
                np.testing.assert_array_equal(M.untransform_policy(game, p, k, H, W), p[::-1] if k else p)


def test_the_draw_is_a_variate_of_its_own_keyed_by_the_position(oracle):
    b = np.zeros((3, 3), np.int8)
    assert M.mix64(1) == 0x5692161D100B05E5 and M.position_event(b) == M.mix64(sum(M.mix64((c + 1) << 32) for c in range(9)) & ((1 << 64) - 1)) >> 32
    c = b.copy(); c[1, 1] = -1                        # int8 -1 enters the key as the byte 0xff
    assert M.position_event(c) == M.mix64((sum(M.mix64((i + 1) << 32) for i in range(9) if i != 4) + M.mix64((5 << 32) | 0xFF)) & ((1 << 64) - 1)) >> 32
    n = 4000
    rng = np.random.default_rng(2)
    ks = np.array([M.draw(oracle, "TicTacToe", 7, 3, 1, rng.integers(-1, 2, size=(3, 3)).astype(np.int8)) for _ in range(n)])
    share = np.bincount(ks, minlength=8) / n
    assert np.all(np.abs(share - 0.125) < 4 * np.sqrt(0.125 * 0.875 / n)), share      # four standard deviations of a binomial rate
    e = M.position_event(c)
    assert len({oracle.uniform(7, 3, 1, 2, e, p) for p in (4, 5, 6, 7)}) == 4
    assert M.draw(oracle, "TicTacToe", 7, 3, 1, c) == min(7, int(oracle.uniform(7, 3, 1, 2, e, 7) * 8))


# ------------------------------------------------------------------------------------------------ 1.
@pytest.mark.parametrize("name,G", [("ttt", 16), ("c4", 16), ("gmk", 1), ("c4-gumbel", 16), ("gmk-gumbel", 2)])
def test_selfplay_equals_the_oracle_with_the_wrapped_evaluator(emu_lib, oracle, name, G):
    cases.selfplay_case(oracle, name, G, emu_lib)


# ------------------------------------------------------------------------------------------------ 2.
@pytest.mark.parametrize("K,forced_k", [(1, 0.0), (4, 0.0), (16, 0.0), (1, 2.0)], ids=["plain", "leaf4", "leaf16", "forced"])
@pytest.mark.parametrize("game", ["TicTacToe", "Connect4", "Gomoku"])
def test_engine_equals_the_models_with_the_wrapped_evaluator(emu_lib, oracle, game, K, forced_k):
    widest = cases.model_case(oracle, game, emu_lib, K=K, forced_k=forced_k)
    assert K == 1 or widest > 1, "no launch carried more than one leaf"


# ------------------------------------------------------------------------------------------------ 3.
@pytest.mark.parametrize("name,G", [("c4-gumbel", 8), ("gmk-gumbel", 2)])
def test_gumbel_batch_4_equals_1(emu_lib, name, G):
    cases.gumbel_batch_case(name, G, emu_lib)


# ------------------------------------------------------------------------------------------------ 4.
@pytest.mark.parametrize("game,G,iters,max_actions,c_init,alpha,m", [
    ("TicTacToe", 8, 24, 9, 1.25, 1.0, None), ("Connect4", 8, 40, 42, 2.5, 0.5, None), ("Gomoku", 2, 48, 3, 2.5, 0.05, None),
    ("Connect4", 4, 32, 42, 0.0, 0.0, 7)], ids=["ttt", "c4", "gmk", "c4-gumbel"])
def test_lockstep_through_the_external_evaluator(emu_lib, oracle, game, G, iters, max_actions, c_init, alpha, m):
    assert cases.lockstep_case(oracle, game, G, emu_lib, iters, max_actions, c_init, alpha, gumbel_m=m) >= 3


# ------------------------------------------------------------------------------------------------ 5.
@pytest.mark.parametrize("game,args", [("TicTacToe", (24, 9, 1.25, 1.0)), ("Connect4", (40, 42, 2.5, 0.5))])
def test_an_equivariant_evaluator_gives_the_off_records(emu_lib, game, args):
    cases.equivariant_case(game, 8, emu_lib, *args)


@pytest.mark.parametrize("game,K", [("TicTacToe", 1), ("Connect4", 1), ("Connect4", 4)])
def test_mode_0_after_mode_1_between_moves(emu_lib, oracle, game, K):
    cases.model_case(oracle, game, emu_lib, K=K, switch_off_at=2)


# ------------------------------------------------------------------------------------------------ 6.
@pytest.mark.parametrize("name", ["ttt", "c4", "c4-gumbel"])
def test_drain_samples_equals_record_to_samples(emu_lib, name):
    cases.samples_case(name, 8, emu_lib)


def test_run_self_play_reads_the_key(emu_lib, oracle, tmp_path):
    cases.run_self_play_case(oracle, tmp_path, emu_lib)


@pytest.mark.parametrize("game,iters", [("TicTacToe", 30), ("Connect4", 60)])
def test_mcts_class_equals_the_model(emu_lib, oracle, game, iters):
    cases.mcts_class_case(oracle, game, emu_lib, iters)


def test_mcts_gumbel_class_shows_the_session_permuted_rows(emu_lib, oracle):
    cases.mcts_gumbel_class_case(oracle, emu_lib)


# ------------------------------------------------------------------------------------------------ 7.
def test_refusals(emu_lib):
    cases.refusal_case(emu_lib)

"""CPU suite: the searches on tied, zero and saturated evaluator outputs (tests/degenerate_eval.py) on the emulation build of the device
code — the cases of tests/degenerate_cases.py at sizes the one-lane emulation plays in seconds.  Exact equality everywhere; the tie and
zero-mass witnesses are asserted on the oracle's / the model's side."""
import numpy as np
import pytest

import degenerate_cases as cases
import degenerate_eval as E
from selfplay_support import emu_lib  # noqa: F401

f32 = np.float32
GAMES3 = ("TicTacToe", "Connect4", "Gomoku")


# ------------------------------------------------------------------------------------------------ the evaluators
@pytest.mark.parametrize("game", GAMES3)
def test_evaluators_are_pure_and_see_the_legal_moves(game):
    """legal_mask == the rules of grok_alpha_zero_amd.games on positions played out at random; every kind gives the same row for the same
    state whenever it is asked, sums to 1 (or is all zero), and keeps its promise about the legal entries"""
    from grok_alpha_zero_amd.games import GAMES
    G, A = GAMES[game], cases.A_OF[game]
    rng = np.random.default_rng(3)
    n_zeromass = 0
    for _ in range(6):
        board, player, hist = np.zeros((G.H, G.W), np.int8), -1, []
        for ply in range(cases.MAXT[game]):
            legal = sorted(G.action_to_index(a) for a in G.get_legal_actions_MCTS(board, 0, None))
            state = np.ascontiguousarray(G.get_input_state_MCTS(board, -player, np.array([G.index_to_action(h) for h in hist])), np.int8)
            mask = E.legal_mask(state, A)
            assert np.flatnonzero(mask).tolist() == legal, (game, ply)
            for kind in E.KINDS:
                p, v, m = E.evaluate(kind, state, A)
                p2, v2, _ = E.evaluate(kind, state.copy(), A)
                assert p.dtype == f32 and p.shape == (A,) and np.array_equal(p, p2) and v == v2 and (p >= 0).all()
                total = float(p.sum(dtype=np.float64))
                assert abs(total - 1.0) < 1e-5 or total == 0.0, (kind, total)
                if kind in ("uniform", "dups", "saturated"):
                    assert (p[m] > 0).all() and (len(legal) < 2 or np.unique(p[m]).size < len(legal))
                if kind == "zeros":
                    assert (p[m] > 0).any()
                if kind == "saturated":
                    assert float(v) in (-1.0, 0.0, 1.0)
                if kind == "zeromass" and not (p[m] > 0).any():
                    n_zeromass += 1
                    assert (p[m] == 0).all() and (total == 0.0 or (p[~m] > 0).any())
            a = int(rng.choice(legal))
            G.do_action_MCTS(board, G.index_to_action(a), player); hist.append(a)
            if G.check_win_MCTS(board, player, np.array([G.index_to_action(h) for h in hist])) != -2:
                break
            player = -player
    assert n_zeromass >= 3, n_zeromass


def test_evaluator_counts_distinct_rows_and_batches_do_not_matter():
    ev = E.Evaluator("zeromass", 9)
    s = np.zeros((3, 3, 2), np.int8)
    a, b = ev(s), ev(s.copy())
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and ev.witness()["rows"] == 1
    states = np.random.default_rng(1).integers(-1, 2, size=(40, 3, 3, 2)).astype(np.int8)
    for kind in E.KINDS:
        p, v = E.Evaluator(kind, 9).many(states)
        for i in (0, 7, 39):
            q, w, _ = E.evaluate(kind, states[i], 9)
            assert np.array_equal(p[i], q) and v[i] == w, kind


# ------------------------------------------------------------------------------------------------ the zero-mass rule in the model
# (the oracle's and the engine's make_priors are held against the model's by the zeromass cases below)
def test_zero_mass_rule_in_the_model(oracle):
    """a root whose legal entries sum to 0, NaN or inf gets 1 / n_legal for every legal action (no Dirichlet noise: the priors themselves);
    a positive finite sum is divided through as before"""
    from leaf_batch_model import Tree
    for bad in (0.0, np.nan, np.inf, -1.0):
        pol = np.full(9, bad, f32)
        t = Tree(oracle, "TicTacToe", 1, 1, use_dirichlet=False, evaluator=lambda s: (pol, f32(0.0)))
        np.testing.assert_array_equal(t.root.P, np.full(9, f32(1.0) / f32(9.0), f32))
        assert t.root.act == list(range(8, -1, -1))                       # all tied: the higher action first
    pol = np.arange(1, 10, dtype=f32)
    t = Tree(oracle, "TicTacToe", 1, 1, use_dirichlet=False, evaluator=lambda s: (pol, f32(0.0)))
    np.testing.assert_array_equal(t.root.P, (pol / f32(45.0))[::-1])


# ------------------------------------------------------------------------------------------------ a.
@pytest.mark.parametrize("game", GAMES3)
def test_puct_selfplay_on_tied_priors_equals_the_oracle(emu_lib, oracle, game):
    cases.puct_ties_case(oracle, game, cases.EMU_GAMES[game], emu_lib)


@pytest.mark.parametrize("game", GAMES3)
def test_puct_selfplay_on_zero_mass_rows_equals_the_oracle(emu_lib, oracle, game):
    cases.puct_selfplay_case(oracle, game, "zeromass", cases.EMU_GAMES[game], emu_lib)


# ------------------------------------------------------------------------------------------------ b.
@pytest.mark.parametrize("config", cases.GUMBEL_CONFIGS, ids=lambda c: f"{c[0]}-noise{int(c[1])}-stablemax{int(c[2])}")
@pytest.mark.parametrize("game", GAMES3)
def test_gumbel_selfplay_equals_the_oracle_at_both_batch_sizes(emu_lib, oracle, game, config):
    cases.gumbel_selfplay_case(oracle, game, config, cases.GUMBEL_EMU_GAMES[game], emu_lib)


# ------------------------------------------------------------------------------------------------ c.
# (Gomoku: two games at K = 16 — see degenerate_cases.LEAF — and the model's 695-iteration searches are the slow side)
LEAF_EMU = [(g, K, kind) for g in ("TicTacToe", "Connect4") for K in (4, 16) for kind in ("uniform", "dups", "zeromass")] + \
           [("Gomoku", 16, "dups"), ("Gomoku", 16, "zeromass")]


@pytest.mark.parametrize("game,K,kind", LEAF_EMU)
def test_leaf_batched_search_equals_the_model(emu_lib, oracle, game, K, kind):
    cases.leaf_batch_case(oracle, game, kind, K, 2 if game == "Gomoku" else 8, emu_lib)


@pytest.mark.parametrize("kind", ["uniform", "dups", "zeromass"])
@pytest.mark.parametrize("game,K", [("TicTacToe", 1), ("TicTacToe", 4), ("Connect4", 1), ("Connect4", 16)])
def test_forced_playouts_equal_the_model(emu_lib, oracle, game, K, kind):
    cases.leaf_batch_case(oracle, game, kind, K, 8, emu_lib, forced_k=2.0)


@pytest.mark.parametrize("forced_k", [0.0, 2.0])
@pytest.mark.parametrize("kind", ["uniform", "dups"])
@pytest.mark.parametrize("game", ["TicTacToe", "Connect4"])
def test_leaf_batched_search_without_noise_sees_tied_priors(emu_lib, oracle, game, kind, forced_k):
    """no Dirichlet noise: every node's priors are the evaluator's, ties included (asserted on the model)"""
    cases.leaf_batch_case(oracle, game, kind, 16, 4, emu_lib, forced_k=forced_k, dirichlet=False)


# ------------------------------------------------------------------------------------------------ d.
@pytest.mark.parametrize("game,K", [("TicTacToe", 1), ("Connect4", 1), ("Connect4", 4)])
def test_tree_readout_after_a_uniform_search(emu_lib, oracle, game, K):
    cases.leaf_batch_case(oracle, game, "uniform", K, 8, emu_lib, readout=True)


@pytest.mark.parametrize("game", ["TicTacToe", "Connect4"])
def test_tree_readout_without_noise(emu_lib, oracle, game):
    cases.leaf_batch_case(oracle, game, "uniform", 16, 4, emu_lib, readout=True, dirichlet=False)

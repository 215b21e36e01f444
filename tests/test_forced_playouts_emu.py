"""CPU suite: forced playouts and policy target pruning (gaz_engine_config.forced_playouts_k) on the emulation build of the device
code — the model's own anchors, then the cases of tests/forced_playouts_cases.py at sizes the one-lane emulation plays in seconds.
Exact equality everywhere."""
import numpy as np
import pytest

import forced_playouts_cases as cases
import forced_playouts_model as model
from selfplay_support import emu_lib  # noqa: F401

f32 = np.float32


# ------------------------------------------------------------------------------------------------ the model (no engine)
def test_restated_score_has_the_argmax_of_the_oracle_on_every_root_selection(oracle):
    """the score prune_target uses is the oracle's: on every root selection of forced and plain searches (the forced ones visit
    statistics PUCT alone never produces) the argmax of the restated score == oracle.best_puct_index"""
    n = 0
    for game, R, moves, k, c_init, alpha in (("Connect4", 40, [3, 3, 2, 4], 2.0, 2.5, 0.5), ("TicTacToe", 24, [4, 0, 8], 2.0, 1.25, 1.0),
                                             ("Connect4", 120, [3], 0.0, 2.5, 0.5)):
        for slot in (0, 1):
            t = model.ForcedTree(oracle, game, 1, cases.SEED, slot=slot, c_puct_init=c_init, dirichlet_alpha=alpha, hash_salt=cases.SALT, forced_k=k,
                                 keep_rows=True)
            for m in moves + [None]:
                t.run(R)
                for P, W, N, pv, best in t.rows:
                    assert model.restated_best(P, W, N, pv, c_init, 19652.0) == best, (game, slot, N, pv)
                n += len(t.rows)
                if m is not None:
                    t.play(m)
    assert n > 500, n


def test_prune_target_by_hand():
    """rule 3 on rows small enough to follow by hand (c_init = 2.5, root visits 40, k = 2)"""
    s, c = model.puct_factors(40, 2.5, 19652.0)
    assert s == np.sqrt(40.0) and 2.5 < c < 2.51
    # slot order = priors descending: actions 3, 1, 5.  c* = action 3 (N 30).  Action 5: N 4, P 0.1 -> floor(sqrt(2 * 0.1 * 40)) = 2 forced
    # visits at most; q = -0.5 is so low that both go.  Action 1: q equal to c*'s and a higher U at 5 visits -> PUCT would have chosen it: stays.
    N = np.zeros(7, np.uint32); W = np.zeros(7, f32); P = np.zeros(7, f32)
    N[[3, 1, 5]] = [30, 6, 4]; P[[3, 1, 5]] = [0.6, 0.3, 0.1]; W[[3, 1, 5]] = [15.0, 3.0, -2.0]
    star = model.score(P[3], f32(0.5), 30, s, c)
    assert model.score(P[5], f32(-0.5), 3, s, c) < star and model.score(P[5], f32(-0.5), 2, s, c) < star
    assert model.score(P[1], f32(0.5), 5, s, c) > star
    pol = model.prune_target(N, W, P, 40, 2.0)
    want = np.zeros(7, f32); want[[3, 1, 5]] = [f32(30 / 38), f32(6 / 38), f32(2 / 38)]
    np.testing.assert_array_equal(pol, want)
    # a child pruned down to one visit loses that one too
    N[5], W[5] = 3, -1.5
    pol = model.prune_target(N, W, P, 40, 2.0)
    want = np.zeros(7, f32); want[[3, 1]] = [f32(30 / 36), f32(6 / 36)]
    np.testing.assert_array_equal(pol, want)                             # 3 -> 1 by two steps, then 1 -> 0
    # k = 0: nothing is forced, nothing is pruned
    np.testing.assert_array_equal(model.prune_target(N, W, P, 40, 0.0), model.raw_target(N))
    # ties in N: c* is the LOWEST slot = the higher prior
    N[[3, 1, 5]] = [10, 10, 1]; W[[3, 1, 5]] = [5.0, 5.0, 0.0]
    assert model.prune_slots([10, 10, 1], [5.0, 5.0, 0.0], [0.6, 0.3, 0.1], 40, 2.0, 2.5, 19652.0)[0] == 10


def test_owed_slots_by_hand():
    """rule 2 on priors that float32 holds exactly: root visits 50, k = 2 -> thresholds sqrt(100 P) = 7.07 (P 0.5), 5 exactly (P 0.25), 2.5 (P 0.0625)"""
    P = np.array([0.5, 0.25, 0.125, 0.0625], f32)
    assert model.owed_slots(np.array([7, 4, 0, 1], np.uint32), P, 4, 50, 2.0) == [0, 1, 3]      # an unvisited child is never owed
    assert model.owed_slots(np.array([8, 5, 3, 3], np.uint32), P, 4, 50, 2.0) == [2]            # N < threshold is strict: 5 < 5 is not owed
    assert model.owed_slots(np.array([7, 4, 0, 1], np.uint32), P, 2, 50, 2.0) == [0, 1]         # slots past n_children (reserved) are never owed
    assert model.owed_slots(np.array([7, 4, 0, 1], np.uint32), P, 4, 50, 0.0) == []
    assert model.forced_floor(4, f32(0.25), 50, 2.0) == 4 and model.forced_floor(9, f32(0.25), 50, 2.0) == 5
    assert model.forced_floor(9, f32(0.0625), 50, 2.0) == 2


# ------------------------------------------------------------------------------------------------ (a) + (b)
@pytest.mark.parametrize("name", ["ttt", "c4-k1", "c4-k4", "gmk"])
def test_sync_searches_equal_the_model_and_policy_is_the_pruned_target(emu_lib, oracle, name):
    cases.hash_case(oracle, name, 2 if name == "gmk" else 8, emu_lib)      # (the model's 480-iteration Gomoku searches are the slow side)


# ------------------------------------------------------------------------------------------------ (c), (d)
@pytest.mark.parametrize("cap", [False, True], ids=["cap-off", "cap-on"])
def test_continuous_selfplay_two_trees_equal_the_model(emu_lib, oracle, cap):
    cases.selfplay_case(oracle, 8, emu_lib, cap=cap)


# ------------------------------------------------------------------------------------------------ (e)
def test_k_0_is_the_engine_without_the_field(emu_lib):
    cases.k0_anchor_case(16, emu_lib)


def test_terminal_parent_root_keeps_raw_target(emu_lib, oracle):
    cases.terminal_root_case(oracle, 8, emu_lib)


# ------------------------------------------------------------------------------------------------ (f)
@pytest.mark.parametrize("name,G", [("c4", 16), ("gmk", 2)])
def test_samples_carry_the_pruned_target(emu_lib, name, G):
    cases.samples_case(name, emu_lib, G)


# ------------------------------------------------------------------------------------------------ (g)
def test_run_self_play_reads_the_train_config_key(emu_lib, tmp_path):
    cases.run_self_play_case(tmp_path, emu_lib)


def test_run_self_play_without_the_key_is_unchanged(emu_lib, tmp_path):
    """absent, 0 and None mean off: the same file"""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import ReplayStore, run_self_play
    from samples_util import assert_same_file, file_contents
    train = dict(games_per_generation=12, MCTS_iteration_limit=16, max_actions=9, num_explore_actions_first=2, num_explore_actions_second=1,
                 c_puct_init=1.25, dirichlet_alpha=1.0, use_gumbel=False)
    out = []
    for extra in ({}, dict(forced_playouts_k=0), dict(forced_playouts_k=None), dict(forced_playouts_k=2.0)):
        folder = str(tmp_path / str(len(out)) / "0")
        store = ReplayStore(folder); store.create()
        assert run_self_play(GAMES["TicTacToe"], ({}, dict(train, **extra)), folder, n_games=8, seed=11, hash_salt=4, lib_path=emu_lib) == 12
        out.append(file_contents(store))
    assert_same_file(out[0], out[1]); assert_same_file(out[0], out[2])
    assert any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(out[0].values(), out[3].values())) or list(out[0]) != list(out[3])


# ------------------------------------------------------------------------------------------------ (h)
@pytest.mark.parametrize("name", sorted(cases.REFUSALS))
def test_refusals(emu_lib, name):
    cases.refusal_case(name, emu_lib)


def test_refusal_messages_are_distinct_and_the_abi_moved(emu_lib):
    from grok_alpha_zero_amd import engine
    msgs = {n: cases.refusal_case(n, emu_lib) for n in cases.REFUSALS}
    assert len(set(msgs.values())) == len(msgs), msgs
    assert engine.ABI_VERSION == 10 and engine.EngineConfig._fields_[-1][0] == "forced_playouts_k"
    assert engine.load_library(emu_lib).gaz_engine_abi_version() == 10

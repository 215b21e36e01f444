"""CPU suite: playout cap randomisation (gaz_engine_config.fast_iterations / full_search_prob) on the emulation build of the device
code — the cases of tests/playout_cap_cases.py at sizes the one-lane emulation plays in seconds.  Exact equality everywhere."""
import numpy as np
import pytest

import playout_cap_cases as cases
from selfplay_support import emu_lib  # noqa: F401


# ------------------------------------------------------------------------------------------------ the draws themselves (no engine)
@pytest.mark.parametrize("G", [4, 8, 64])
@pytest.mark.parametrize("name", sorted(cases.HASH_CASES))
def test_seed_gives_both_kinds_after_move_0(oracle, name, G):
    """the seed of the hash cases, for the slots the emulation (4 or 8 games) and the GPU (64 games) compare: fast and full moves both
    occur after move 0, and move 0 is full everywhere"""
    kinds = cases.hash_case_kinds(oracle, name, G)
    assert all(k[0] == 1 for k in kinds.values())
    assert {int(k[t]) for k in kinds.values() for t in range(1, len(next(iter(kinds.values()))))} == {1, 2}


def test_kinds_follow_the_uniform_stream(oracle):
    """kinds_of restated: ply t of game (slot, seq) is fast iff it is not the first searched ply and uniform(seed, slot, seq, tree 2,
    event t, purpose 5) >= p; the rate over many plies is p"""
    p, n = 0.25, 4000
    k = cases.kinds_of(oracle, 7, 3, 2, n, p)
    u = np.array([oracle.uniform(7, 3, 2, 2, t, 5) for t in range(n)])
    assert k[0] == 1 and np.array_equal(k[1:] == 1, u[1:] < p)
    assert abs(float((k == 1).mean()) - p) < 4 * np.sqrt(p * (1 - p) / n)            # four standard deviations of a binomial rate
    assert (u >= 0).all() and (u < 1).all()
    # another purpose of the same event is another variate: the cap does not reuse the opening / move-sampling draws
    assert oracle.uniform(7, 3, 2, 2, 0, 5) != oracle.uniform(7, 3, 2, 2, 0, 4)


# ------------------------------------------------------------------------------------------------ 1.
@pytest.mark.parametrize("name", sorted(cases.HASH_CASES))
def test_limits_per_move_equal_the_model(emu_lib, oracle, name):
    cases.hash_case(oracle, name, 4 if name == "gmk" else 8, emu_lib)          # (the model's 720-iteration Gomoku searches are the slow side)


# ------------------------------------------------------------------------------------------------ 2.
@pytest.mark.parametrize("name", sorted(cases.SELFPLAY_CASES))
def test_continuous_selfplay_two_trees_equal_the_model(emu_lib, oracle, name):
    cases.selfplay_case(oracle, name, 8, emu_lib)


# ------------------------------------------------------------------------------------------------ 3.
def test_anchors_p1_and_fast_equal_full(emu_lib):
    cases.anchor_case(16, emu_lib)


def test_cap_off_writes_move_kind_1_and_set_position_prefix_0(emu_lib):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine("Connect4", 2, 20, 42, 0, 0, 2.5, 0.5, seed=3, hash_salt=2, ring_capacity=8, games_budget=2, lib_path=emu_lib)
    assert eng.layout.off_move_kind == eng.layout.off_P + 4 * eng.layout.max_T * eng.layout.A and eng.layout.record_bytes % 16 == 0
    assert eng.layout.record_bytes >= eng.layout.off_move_kind + eng.layout.t_pad
    eng.set_position(1, [3, 3, 2])
    first = cases.first_games(eng, 2)
    eng.close()
    assert (first[0]["move_kind"] == 1).all() and first[0]["move_kind"].dtype == np.uint8 and first[0]["move_kind"].shape == (first[0]["T"],)
    assert first[1]["move_kind"][:3].tolist() == [0, 0, 0] and (first[1]["move_kind"][3:] == 1).all()


def test_first_searched_move_after_set_position_is_full_and_reset_clears_the_bit(emu_lib, oracle):
    """the 'had a full move' bit is cleared by set_position and reset_games: the first searched ply is full whatever its draw says, and
    the draws stay keyed by the absolute ply"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    p = 0.05                                                                          # nearly every drawn move is fast
    eng = SelfPlayEngine("Connect4", 4, 30, 42, 0, 0, 2.5, 0.5, seed=cases.SEED, hash_salt=2, ring_capacity=16, fast_iterations=6, full_search_prob=p,
                         lib_path=emu_lib)
    eng.run_waves(40)                                                                 # every game is past its first move
    eng.set_position(1, [3, 3, 2]); eng.reset_games([2])
    recs = []
    for _ in range(4000):
        eng.run_waves(16); recs += eng.drain_finished()
        if {(r["slot"], r["game_seq"]) for r in recs} >= {(0, 0), (1, 0), (2, 1), (3, 0)}:
            break
    eng.close()
    by = {(r["slot"], r["game_seq"]): r for r in recs}
    r = by[(1, 0)]
    np.testing.assert_array_equal(r["move_kind"][3:], cases.kinds_of(oracle, cases.SEED, 1, 0, r["T"], p, start=3))
    assert r["move_kind"][:4].tolist() == [0, 0, 0, 1] and r["root_visits"][3] >= 30
    for key in ((0, 0), (2, 1), (3, 0)):
        r = by[key]
        np.testing.assert_array_equal(r["move_kind"], cases.kinds_of(oracle, cases.SEED, key[0], key[1], r["T"], p), err_msg=str(key))
    assert any((r["move_kind"] == 2).any() for r in by.values())


# ------------------------------------------------------------------------------------------------ 4.
def test_gumbel_comparator_holds_without_the_cap(emu_lib, oracle):
    cases.gumbel_case(oracle, 8, emu_lib, cap=False, slots=(0, 3, 7))


def test_gumbel_with_the_cap_equals_host_set_limits(emu_lib, oracle):
    cases.gumbel_case(oracle, 8, emu_lib)


def test_gumbel_batch_4_with_the_cap_equals_gumbel_batch_1(emu_lib):
    cases.gumbel_batch_case(8, emu_lib)


# ------------------------------------------------------------------------------------------------ 5.
@pytest.mark.parametrize("name,G", [("ttt", 16), ("c4", 16), ("gmk", 2), ("c4-groups", 16), ("gmk-long", 8)])
def test_samples_device_path_equals_host_path_and_the_kept_rows(emu_lib, name, G):
    cases.samples_case(name, emu_lib, G)


def test_drain_samples_counts_kept_rows(emu_lib):
    cases.row_accounting_case(emu_lib)


# ------------------------------------------------------------------------------------------------ 6.
@pytest.mark.parametrize("gumbel", [False, True], ids=["puct", "gumbel"])
def test_run_self_play_reads_the_train_config_keys(emu_lib, tmp_path, gumbel):
    cases.run_self_play_case(tmp_path, emu_lib, gumbel=gumbel)


def test_run_self_play_without_the_keys_is_unchanged(emu_lib, tmp_path):
    """absent keys, and MCTS_fast_iteration_limit = 0 next to a probability, mean off: the same file as before"""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import ReplayStore, run_self_play
    from samples_util import assert_same_file, file_contents
    train = dict(games_per_generation=12, MCTS_iteration_limit=16, max_actions=9, num_explore_actions_first=2, num_explore_actions_second=1,
                 c_puct_init=1.25, dirichlet_alpha=1.0, use_gumbel=False)
    out = []
    for extra in ({}, dict(MCTS_fast_iteration_limit=0, full_search_prob=0.25)):
        folder = str(tmp_path / str(len(out)) / "0")
        store = ReplayStore(folder); store.create()
        assert run_self_play(GAMES["TicTacToe"], ({}, dict(train, **extra)), folder, n_games=8, seed=11, hash_salt=4, lib_path=emu_lib) == 12
        out.append(file_contents(store))
    assert_same_file(out[0], out[1])
    assert sum(out[0][f"values_{8 * k}"].shape[0] for k in range(12)) == int(out[0]["game_stats"][1])


# ------------------------------------------------------------------------------------------------ 7.
@pytest.mark.parametrize("name", sorted(cases.REFUSALS))
def test_refusals(emu_lib, name):
    cases.refusal_case(name, emu_lib)


def test_refusal_messages_are_distinct(emu_lib):
    msgs = {n: cases.refusal_case(n, emu_lib) for n in ("negative", "above-run-iterations", "prob-zero", "prob-without-cap", "time-limit")}
    assert len(set(msgs.values())) == 5, msgs


def test_lowering_run_iterations_below_the_fast_limit(emu_lib, oracle):
    cases.lower_run_iterations_case(oracle, emu_lib)

"""CPU suite: the solver (gaz_engine_set_solver) on the emulation build of the device code — the model's own anchors,
then the cases of tests/solver_cases.py at sizes the one-lane emulation plays in seconds.  Exact equality everywhere; every case asserts
the witnesses it is there for, so that it cannot pass vacuously."""
import numpy as np
import pytest

import solver_cases as cases
import solver_model as model
from selfplay_support import emu_lib  # noqa: F401

f32 = np.float32
U, WIN, DRAW, LOSS = model.U, model.WIN, model.DRAW, model.LOSS


# ------------------------------------------------------------------------------------------------ the model (no engine)
def test_move_end_row_by_hand():
    """rule 5 on rows small enough to follow by hand (slot order)"""
    N = [10, 6, 4, 0]
    # no status: the -1 slot and the unvisited slot are out; the row is renormalised over the other two
    row, C, move = model.move_end_row(N, N, [U, LOSS, U, U], U)
    assert C == [0, 2] and move is None
    np.testing.assert_array_equal(row, np.array([f32(10 / 14), 0, f32(4 / 14), 0], f32))
    # no status, every visited slot is -1: all slots are candidates again, the row is N / sum(N)
    row, C, _ = model.move_end_row(N, N, [LOSS, LOSS, LOSS, U], U)
    assert C == [0, 1, 2, 3]
    np.testing.assert_array_equal(row, np.array([f32(0.5), f32(0.3), f32(0.2), 0], f32))
    # WIN: only the +1 slots, the move is the most visited of them whatever the others have
    row, C, move = model.move_end_row(N, N, [U, WIN, WIN, LOSS], WIN)
    assert C == [1, 2] and move == 1
    np.testing.assert_array_equal(row, np.array([0, f32(0.6), f32(0.4), 0], f32))
    # DRAW: the 0 slots; ties in N go to the lowest slot
    row, C, move = model.move_end_row([5, 5, 5, 5], [5, 5, 5, 5], [LOSS, DRAW, DRAW, LOSS], DRAW)
    assert C == [1, 2] and move == 1 and row[1] == f32(0.5)
    # LOSS: all slots, N / sum(N), no forced move
    row, C, move = model.move_end_row(N, N, [LOSS] * 4, LOSS)
    assert C == [0, 1, 2, 3] and move is None and row[0] == f32(0.5)
    # the pruned counts of a forced-playouts move are what is restricted; candidates with no count left leave the row as it was
    row, C, _ = model.move_end_row([10, 0, 2, 0], N, [U, U, U, U], U)
    np.testing.assert_array_equal(row, np.array([f32(10 / 12), 0, f32(2 / 12), 0], f32))
    assert model.move_end_row([0, 0, 0, 0], [0, 0, 0, 0], [U] * 4, U)[0] is None


def test_minimax_on_known_positions():
    """the brute force is independent of the search: TicTacToe is a draw, a fork wins, an open three on Connect4's bottom row"""
    e = np.zeros((3, 3), np.int8)
    assert model.minimax("TicTacToe", e, [], -1) == DRAW
    b, mover = cases.replay("TicTacToe", [0, 4, 8, 2])            # X corners 0, 8; O centre and 2: X takes 6 and forks 3 / 7
    assert mover == -1 and model.minimax("TicTacToe", b, [0, 4, 8, 2], mover) == WIN
    b, mover = cases.replay("TicTacToe", [0, 4, 8, 2, 6])         # the same from O's side
    assert model.minimax("TicTacToe", b, [0, 4, 8, 2, 6], mover) == LOSS
    # Connect4: X holds 1, 2, 3 of the bottom row with both ends open — O to move has lost, and X to move wins
    h = [1, 1, 2, 2, 3]
    b, mover = cases.replay("Connect4", h)
    assert mover == 1 and model.minimax("Connect4", b, h, mover) == LOSS
    b, mover = cases.replay("Connect4", h + [6])
    assert mover == -1 and model.minimax("Connect4", b, h + [6], mover) == WIN


# ------------------------------------------------------------------------------------------------ engine == model, soundness, witnesses
@pytest.mark.parametrize("name,G", [("ttt", 4), ("ttt-two-trees-tau", 4), ("ttt-no-noise-compact", 2), ("ttt-new-root", 2)])
def test_tictactoe_games_equal_the_model_and_minimax(emu_lib, oracle, name, G):
    w, _, stats = cases.sync_case(oracle, name, G, emu_lib)
    assert w.proven_nodes > 0 and w.deep_proofs > 0 and stats["proven_nodes"] == w.proven_nodes
    assert w.proven_hits > 0 and w.masked_levels > 0 and w.root_draw > 0
    assert w.zero_sim_moves > 0 and w.restricted_rows > 0
    assert w.minimax_checked == w.statuses_checked > 0                  # TicTacToe: every exported status is the game's value
    if name == "ttt-new-root":
        assert w.short_moves > 0                                         # a fresh tree per move: proofs are found again, mid-move


@pytest.mark.parametrize("name", ["c4-16", "c4-20-two-trees", "c4-24-compact-no-noise", "c4-whole"])
def test_connect4_games_equal_the_model_and_minimax(emu_lib, oracle, name):
    w, _, _ = cases.sync_case(oracle, name, 2, emu_lib)
    assert w.proven_nodes > 0 and w.deep_proofs > 0 and w.masked_levels > 0
    assert w.root_win > 0 and w.root_loss > 0
    assert w.zero_sim_moves > 0 and w.short_moves > 0 and w.restricted_rows > 0
    assert w.proven_early > 0                                            # a root proven WIN before every child had a visit
    assert w.minimax_checked > 100


@pytest.mark.parametrize("name,G", [("gmk-open-four", 2), ("gmk-four-one-end", 2), ("gmk-open-four-defender", 1)])
def test_gomoku_positions_with_a_four(emu_lib, oracle, name, G):
    w, _, _ = cases.sync_case(oracle, name, G, emu_lib)
    if name == "gmk-open-four":
        assert w.zero_sim_moves == G and w.root_win == G                 # a terminal-parent root ends its move with 0 simulations
    elif name == "gmk-four-one-end":
        assert w.masked_levels > 0 and w.restricted_rows == G            # every move but the block is left out, of the descent and of the row
    else:
        assert w.root_loss == 1 and w.short_moves == 1 and w.zero_sim_moves == 1 and w.proven_nodes == 1


@pytest.mark.parametrize("name,G", [("ttt", 4), ("c4", 2)])
def test_continuous_selfplay_two_trees_equal_the_model(emu_lib, oracle, name, G):
    w, _ = cases.selfplay_case(oracle, name, G, emu_lib)
    assert w.proven_nodes > 0 and w.masked_levels > 0 and w.zero_sim_moves > 0 and w.restricted_rows > 0
    assert (w.root_draw > 0 and w.proven_hits > 0) if name == "ttt" else (w.root_win > 0 and w.root_loss > 0)


def test_records_differ_from_the_solver_off_engine(emu_lib):
    cases.differs_from_off_case("ttt", 4, emu_lib)


# ------------------------------------------------------------------------------------------------ anchors
def test_solver_on_without_a_terminal_parent_gives_the_off_records(emu_lib):
    cases.quiet_anchor_case(8, emu_lib)


@pytest.mark.parametrize("name,switch", [("ttt", {0: False, 4: True}), ("ttt", {5: False}), ("ttt-two-trees-tau", {0: False, 3: True, 6: False}),
                                         ("ttt-two-trees-tau", {0: False, 2: True}), ("c4-20-two-trees", {20: False, 23: True}),
                                         ("c4-24-compact-no-noise", {24: False, 27: True}), ("c4-16", {16: False, 19: True, 24: False, 26: True})])
def test_switching_between_moves_equals_the_model_switching_at_the_same_ply(emu_lib, oracle, name, switch):
    """Terminal parents made before a switch-on count as proven; switching off and on again follows the model"""
    w, _, _ = cases.sync_case(oracle, name, 2, emu_lib, switch=switch)
    assert w.statuses_checked > 0 and (w.root_win + w.root_draw + w.root_loss) > 0


# ------------------------------------------------------------------------------------------------ compositions
def test_forced_playouts(emu_lib, oracle):
    w, _ = cases.selfplay_case(oracle, "c4", 2, emu_lib, forced_k=2.0)
    assert w.restricted_rows > 0 and w.masked_levels > 0 and w.root_win > 0


def test_forced_playouts_sync_tictactoe(emu_lib, oracle):
    w, rows, _ = cases.sync_case(oracle, "ttt", 2, emu_lib, forced_k=2.0)
    assert w.proven_hits > 0 and sum(r["n_differ"] for rr in rows.values() for r in rr) > 0


def test_playout_cap_a_fast_move_ended_by_a_proof(emu_lib, oracle):
    w, _ = cases.selfplay_case(oracle, "c4", 4, emu_lib, cap=(40, 0.4))
    assert getattr(w, "fast_proven", 0) > 0, w


def test_resignation_reads_the_exact_q(emu_lib, oracle):
    assert cases.resign_case(oracle, "c4", 4, emu_lib) >= 1


def test_evaluation_symmetry(emu_lib, oracle):
    w, _, _ = cases.sync_case(oracle, "ttt", 2, emu_lib, eval_symmetry=True)
    assert w.proven_hits > 0 and w.root_draw > 0


def test_drain_samples_equals_record_to_samples(emu_lib):
    cases.samples_case("ttt", 4, emu_lib)


def test_run_self_play_reads_the_train_config_key(emu_lib, tmp_path):
    cases.run_self_play_case(tmp_path, emu_lib)


def test_mcts_class(emu_lib, oracle):
    assert cases.mcts_class_case(oracle, emu_lib) > 0


# ------------------------------------------------------------------------------------------------ refusals and ABI
@pytest.mark.parametrize("which", sorted(cases.REFUSALS))
def test_refusals(emu_lib, which):
    cases.refusal_case(which, emu_lib)


def test_refusal_messages_are_distinct_and_the_abi_did_not_move(emu_lib):
    msgs = {n: cases.refusal_case(n, emu_lib) for n in cases.REFUSALS}
    msgs.update(cases.abi_case(emu_lib))
    assert len(set(msgs.values())) == len(msgs), msgs

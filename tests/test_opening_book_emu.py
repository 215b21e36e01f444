"""CPU suite: the opening book (gaz_engine_set_opening_book, gaz_engine_get_opening_book, gaz_engine_read_book_counts; csrc/book.hpp,
csrc/book_start.hpp) on the one-lane emulation build — the cases of tests/opening_book_cases.py against the oracle's games from
start_history and the restated draw — and the stand-alone sanitizer driver (tests/emu/book_main.cpp).  Exact equality everywhere."""
import pytest

import opening_book_cases as cases
from selfplay_support import emu_lib  # noqa: F401


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_games_from_the_book_equal_the_oracle(oracle, emu_lib, name):
    """all three games, PUCT with two trees and Gumbel, continuous mode, four games per slot: game (slot, seq) is the oracle's game from
    the entry the restated draw names; books of 3 and 5 entries, lengths 0, 1 and max_actions - 1, a full Connect4 column, an entry longer
    than a 16-lane team, Gomoku entries longer than a wavefront, a TicTacToe board one move from full"""
    cases.oracle_case(oracle, name, emu_lib)


# ------------------------------------------------------------------------------------------------ 2. pairs
def test_mode_two_shares_the_prefix_within_every_pair_and_mode_one_does_not(emu_lib):
    cases.pairs_case(emu_lib)


def test_the_two_games_of_a_match_pair_are_answered_by_opposite_networks(emu_lib):
    cases.match_owner_case(emu_lib)


def test_match_result_paired_against_the_closed_form():
    cases.match_result_case()


def test_play_match_with_a_book_end_to_end(emu_lib):
    cases.play_match_case(emu_lib)


# ------------------------------------------------------------------------------------------------ 3. anchors
@pytest.mark.parametrize("name,feature", [("c4-puct", "plain"), ("c4-gumbel", "plain"), ("ttt-puct", "opening"), ("ttt-puct", "solver"), ("ttt-puct", "symmetry"),
                                          ("ttt-puct", "forced"), ("ttt-puct", "cap"), ("ttt-puct", "resign"), ("ttt-puct", "match"), ("ttt-gumbel", "match")])
def test_a_book_of_empty_entries_is_no_book_byte_for_byte(emu_lib, name, feature):
    cases.empty_book_case(emu_lib, name, feature)


def test_removing_the_book_between_games_restores_empty_starts(emu_lib):
    cases.removal_case(emu_lib)


@pytest.mark.parametrize("name,prefix", [("c4-puct", cases.C4_LONG), ("c4-gumbel", [2, 4, 4]), ("ttt-puct", cases.TTT_ALMOST_FULL)])
def test_a_one_entry_book_is_set_position_but_for_the_kind(emu_lib, name, prefix):
    cases.set_position_anchor_case(emu_lib, name, prefix)


# ------------------------------------------------------------------------------------------------ 4. composition
def test_leaf_batch_four_against_the_model_from_the_prefix(oracle, emu_lib):
    cases.leaf_batch_case(oracle, emu_lib)


def test_gumbel_batch_four_equals_gumbel_batch_one(emu_lib):
    cases.same_records_case(emu_lib, "c4-gumbel", dict(gumbel_batch=4), dict(gumbel_batch=1))


def test_single_tree_against_the_model_from_the_prefix(oracle, emu_lib):
    cases.single_tree_case(oracle, emu_lib)


def test_game_groups_down_to_one_game_each(emu_lib):
    cases.same_records_case(emu_lib, "c4-puct", dict(game_groups=4), dict(game_groups=1))


def test_repack_to_one_slot(emu_lib):
    cases.same_records_case(emu_lib, "c4-puct", dict(game_groups=1), dict(game_groups=1), repack=True)


# ------------------------------------------------------------------------------------------------ 5. samples
@pytest.mark.parametrize("kw", [{}, dict(fast_iterations=6, full_search_prob=0.5)], ids=["cap-off", "cap-on"])
def test_drain_samples_leaves_the_book_plies_out(emu_lib, kw):
    cases.samples_case(emu_lib, **kw)


def test_gomoku_samples_behind_a_long_prefix(emu_lib):
    cases.samples_case(emu_lib, name="gmk-puct", G=2, games_per_slot=2)


def test_surprise_weighting_takes_no_notice_of_book_plies(oracle, emu_lib):
    cases.surprise_case(oracle, emu_lib)


def test_a_book_prefix_breaks_a_resignation_run(emu_lib):
    cases.resign_case(emu_lib)


# ------------------------------------------------------------------------------------------------ 6. refusals, helpers, run level
def test_every_refusal_by_its_text_and_the_book_in_force_stays(emu_lib):
    cases.refusal_case(emu_lib)


def test_book_from_records_enumerate_openings_and_the_book_files():
    cases.helpers_case()


def test_run_self_play_reads_the_two_train_config_keys(oracle, emu_lib, tmp_path):
    cases.run_self_play_case(oracle, tmp_path, emu_lib)


# ------------------------------------------------------------------------------------------------ 7. the sanitizer driver
@pytest.fixture(scope="module")
def driver():
    return cases.build_driver()


@pytest.mark.parametrize("name", sorted(cases.DRIVER_CASES))
def test_set_start_drain_and_refusals_under_the_sanitizers(driver, name):
    """the engine's host code and the one-lane build of its device code, linked into a program of their own with
    -fsanitize=address,undefined -fno-sanitize-recover=all, driven through the C ABI: set a book, start three games per slot, drain
    records and samples, and walk the refusal paths"""
    rc, out = cases.run_driver(driver, name)
    assert rc == 0, f"{name}: exit status {rc}\n{out[-3000:]}"

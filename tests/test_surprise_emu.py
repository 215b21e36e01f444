"""CPU suite: policy surprise weighting of the training rows (gaz_engine_set_sample_weighting, gaz_engine_drain_samples2; csrc/samples.hpp)
on the one-lane emulation build — the cases of tests/surprise_cases.py against tests/surprise_model.py — and the stand-alone sanitizer
driver of the weighted drain (tests/emu/surprise_main.cpp).  Exact equality everywhere: no tolerance."""
import pytest

import surprise_cases as cases
from selfplay_support import emu_lib  # noqa: F401


# ------------------------------------------------------------------------------------------------ 1. the weighted drain against the model
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_weighted_drain_equals_the_model(oracle, emu_lib, name):
    """all three games, two games per slot, the cap off and on, lambda 0.5 and 1: bytes, row_ply, games columns and n_rows of drain_samples,
    and record_to_samples(weighting=...), all against the model; the cap-on cases assert their five witnesses"""
    cases.weighted_case(oracle, name, emu_lib)


@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_weighted_drain_with_leaf_batch_single_tree_and_match_play(oracle, emu_lib, shape):
    cases.shape_case(oracle, shape, emu_lib)


# ------------------------------------------------------------------------------------------------ 2. anchors
@pytest.mark.parametrize("name,feature", [("c4-off", "plain"), ("c4-on", "plain"), ("ttt-on", "solver"), ("ttt-on", "forced"), ("ttt-on", "symmetry"),
                                          ("ttt-on", "resign")])
def test_lambda_zero_is_the_mode_off_byte_for_byte(emu_lib, name, feature):
    cases.lambda_zero_case(name, feature, emu_lib)


def test_switching_the_mode_between_two_drains(oracle, emu_lib):
    cases.switch_case(oracle, "ttt-on", emu_lib)


def test_conservation_over_256_games(oracle, emu_lib):
    total, n_full = cases.conservation_case(oracle, emu_lib)
    assert total > 0 and n_full > 0


# ------------------------------------------------------------------------------------------------ 3. degenerate records
@pytest.mark.parametrize("kind", ["first-legal", "zeros"])
def test_degenerate_evaluators(oracle, emu_lib, kind):
    """tied search: pi == P, S == 0, w = w0; exact zero priors under visited moves: the term is left out"""
    cases.degenerate_case(oracle, kind, emu_lib)


def test_one_ply_games_fast_tails_and_a_set_position_prefix(oracle, emu_lib):
    cases.short_games_case(oracle, emu_lib)


# ------------------------------------------------------------------------------------------------ 4. capacity
def test_max_rows_and_max_games_limits_and_mixed_drains(oracle, emu_lib):
    cases.capacity_case(oracle, emu_lib)


def test_game_groups_rings_in_turn(oracle, emu_lib):
    cases.groups_case(oracle, emu_lib)


# ------------------------------------------------------------------------------------------------ 5. run level
def test_every_refusal_by_its_text(emu_lib):
    cases.refusal_case(emu_lib)


def test_run_self_play_reads_the_two_train_config_keys(oracle, emu_lib, tmp_path):
    cases.run_self_play_case(oracle, tmp_path, emu_lib)


# ------------------------------------------------------------------------------------------------ 6. the sanitizer driver
@pytest.fixture(scope="module")
def driver():
    return cases.build_driver()


@pytest.mark.parametrize("name", sorted(cases.DRIVER_CASES))
def test_weighted_drain_at_the_buffer_limits_under_the_sanitizers(driver, name):
    """the engine's host code and the one-lane build of its device code, linked into a program of their own with
    -fsanitize=address,undefined -fno-sanitize-recover=all, driven through the C ABI with caller buffers of exactly the documented sizes"""
    rc, out = cases.run_driver(driver, name)
    assert rc == 0, f"{name}: exit status {rc}\n{out[-3000:]}"

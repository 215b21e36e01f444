"""CPU suite: the tree arena and the record ring at their capacity limits, on the emulation build of the device code — the cases of
tests/capacity_cases.py — and the stand-alone sanitizer driver of the error path (tests/emu/capacity_main.cpp).  Exact equality everywhere."""
import pytest

import capacity_cases as cases
from selfplay_support import emu_lib  # noqa: F401


# ------------------------------------------------------------------------------------------------ 1. the arena at exact fit and one below
@pytest.mark.parametrize("name", sorted(cases.ARENA_CASES))
def test_exact_fit_plays_the_roomy_games(emu_lib, name):
    cases.exact_fit_case(name, cases.smallest_fit(name, emu_lib), emu_lib)


@pytest.mark.parametrize("name", sorted(cases.ARENA_CASES))
def test_one_node_below_is_a_clean_sticky_error(emu_lib, name):
    cases.one_below_case(name, cases.smallest_fit(name, emu_lib), emu_lib)


@pytest.mark.parametrize("case", sorted(cases.ROOT_CHILD_CASES))
def test_gumbel_arena_without_room_for_the_root_children(emu_lib, case):
    cases.root_child_case(case, emu_lib)


# ------------------------------------------------------------------------------------------------ 2. the sanitizer driver
@pytest.fixture(scope="module")
def driver():
    return cases.build_driver()


@pytest.mark.parametrize("name", sorted(cases.ARENA_CASES))
def test_error_path_under_address_and_undefined_behaviour_sanitizers(emu_lib, driver, name):
    """The engine's host code and the one-lane build of its device code, linked into a program of their own with
    -fsanitize=address,undefined -fno-sanitize-recover=all, driven through the C ABI at c* - 1: run_waves(1) until the arena-full error
    appears, 64 more launches with the error standing, close.  Exit status 0 = the message was seen and no sanitizer report ended the run.
    Known limit: all trees live in ONE allocation, so the sanitizer sees a write outside the arena, not a write into the neighbouring
    tree's slice of it; the record equality at c* (test_exact_fit_plays_the_roomy_games) is what guards that."""
    c_star = cases.smallest_fit(name, emu_lib)
    rc, out = cases.run_driver(name, c_star - 1)
    assert rc == 0, f"{name} at c* - 1 = {c_star - 1}: exit status {rc}\n{out[-3000:]}"
    assert cases.ARENA_FULL in out, out[-3000:]


@pytest.mark.parametrize("case", sorted(cases.ROOT_CHILD_CASES))
def test_root_child_error_path_under_the_sanitizers(driver, case):
    """the same program where a Gumbel game stops at the expansion of a root child (capacity_cases.ROOT_CHILD_CASES)"""
    name, nodes = cases.ROOT_CHILD_CASES[case]
    rc, out = cases.run_driver(name, nodes)
    assert rc == 0, f"{case}: exit status {rc}\n{out[-3000:]}"
    assert cases.ARENA_FULL in out, out[-3000:]


def test_sanitizer_driver_plays_through_at_exact_fit(emu_lib, driver):
    c_star = cases.smallest_fit("c4-compact", emu_lib)
    rc, out = cases.run_driver("c4-compact", c_star)
    assert rc == 3, f"exit status {rc}\n{out[-3000:]}"               # 3 = every game finished and no error was raised


# ------------------------------------------------------------------------------------------------ 4. the default sizing
@pytest.mark.parametrize("name", sorted(cases.DEFAULT_CASES))
def test_default_arena_holds_full_length_games(emu_lib, name):
    cases.default_sizing_case(name, emu_lib)


def test_set_hyperparams_holds_values_against_the_arena(emu_lib):
    cases.hyperparams_boundary_case(emu_lib)


# ------------------------------------------------------------------------------------------------ 5. the record ring
@pytest.mark.parametrize("name", sorted(cases.RING_CASES))
def test_tight_ring_hands_out_every_game_once(emu_lib, name):
    cases.ring_case(name, emu_lib)


def test_tight_ring_through_drain_samples(emu_lib):
    cases.ring_samples_case(emu_lib)

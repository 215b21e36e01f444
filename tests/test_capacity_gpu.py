"""-m gpu: the tree arena and the record ring at their capacity limits on the HIP build — the cases of tests/capacity_cases.py.  What the
one-lane emulation cannot show is here: a game that stops shares its wavefront with three that go on, many teams finish in one launch and
race for ring_head, and in the one-launch wave the trunk workgroups wait for games that may have stopped.  Exact equality everywhere.

The smallest arena that fits a case, c*, is found by bisection on the emulation build (on the CPU, in this process, once per case) and
handed to the child: no bisection runs on the GPU.  The "device error" of these cases is the engine's own error word, a return value; a
c* - 1 case runs once, in a child of its own.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py."""
import os
import sys

import pytest

from gpu_step import STEPS
from selfplay_support import emu_lib  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARENA = ("c4-compact", "c4-gumbel", "c4-gumbel-batch7", "c4-leaf8", "c4-puct", "c4-solver", "c4-symmetry", "gmk-compact", "ttt-single")
ROOT_CHILD = ("c4-gumbel-1", "c4-gumbel-5", "c4-gumbel-batch7-1", "c4-gumbel-batch7-5")
RINGS = ("ring1-drain1", "ring2-drain1", "ring3-drain2", "ring3-groups2", "ring5-drain5")


def _c_star(name, emu):
    import capacity_cases as cases
    return cases.smallest_fit(name, emu)


@pytest.mark.parametrize("name", ARENA)
def test_exact_fit_plays_the_roomy_games(emu_lib, name):
    STEPS.run(__file__, f"fit:{name}:{_c_star(name, emu_lib)}", 180)


@pytest.mark.parametrize("name", ARENA)
def test_one_node_below_is_a_clean_sticky_error(emu_lib, name):
    STEPS.run(__file__, f"below:{name}:{_c_star(name, emu_lib)}", 180)


@pytest.mark.parametrize("case", ROOT_CHILD)
def test_gumbel_arena_without_room_for_the_root_children(case):
    STEPS.run(__file__, "root-child:" + case, 180)


@pytest.mark.parametrize("launch", ["fused", "separate"])
def test_network_games_that_stop_do_not_hold_the_wave(launch):
    STEPS.run(__file__, "net-arena:" + launch, 180)


@pytest.mark.parametrize("name", RINGS)
def test_tight_ring_hands_out_every_game_once(name):
    STEPS.run(__file__, "ring:" + name, 180)


def test_tight_ring_through_drain_samples():
    STEPS.run(__file__, "ring-samples", 180)


def test_tight_ring_in_the_one_launch_wave():
    STEPS.run(__file__, "net-ring", 180)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import capacity_cases as cases
    assert sorted(ARENA) == sorted(cases.ARENA_CASES) and sorted(RINGS) == sorted(cases.RING_CASES) and sorted(ROOT_CHILD) == sorted(cases.ROOT_CHILD_CASES)
    kind, _, rest = sys.argv[1].partition(":")
    if kind == "fit":
        cases.exact_fit_case(rest.split(":")[0], int(rest.split(":")[1]), None)
    elif kind == "below":
        cases.one_below_case(rest.split(":")[0], int(rest.split(":")[1]), None)
    elif kind == "root-child":
        cases.root_child_case(rest, None)
    elif kind == "net-arena":
        cases.net_arena_case(rest == "fused")
    elif kind == "ring":
        cases.ring_case(rest, None)
    elif kind == "ring-samples":
        cases.ring_samples_case(None)
    elif kind == "net-ring":
        cases.net_ring_case()
    else:
        raise SystemExit(f"unknown case {sys.argv[1]}")
    print("ok", flush=True)

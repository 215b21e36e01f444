"""-m gpu: resignation in self-play (gaz_engine_set_resignation) on the HIP build — the cases of tests/resign_cases.py at the sizes where
the launch shapes matter (64 games: four games per wavefront, of which some resign while their neighbours play on; Gomoku's PUCT search
with compacted trees; two game groups), and the scheduling equalities with the network.  Exact equality everywhere: no tolerance.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the cases (run in the child)
def _run_case(name):
    import tempfile
    import resign_cases as cases
    from oracle import gaz_oracle as O
    O.build()
    both = cases.MINIMUM + ("false_positive", "true_positive")
    kind, _, arg = name.partition(":")
    if kind == "prefix":
        need = {"c4": both, "ttt": both, "ttt-min4": cases.MINIMUM + ("true_positive",), "gmk-gumbel": ("resigned", "would", "false_positive"),
                "gmk-puct": ("resigned", "natural", "quiet_playout", "would", "false_positive")}.get(arg, cases.MINIMUM)
        G = 8 if arg == "gmk-gumbel" else 64
        cases.prefix_case(O, arg, G, None, need=need)                                  # two games per slot: game_seq 1 too, Gomoku included
    elif kind == "fast":
        print("games that resign after a fast ply:", cases.fast_resign_case(O, 64, None), flush=True)
    elif kind == "anchors":
        print(f"anchors: {cases.anchor_case(64, None)} games with a would-have-resigned ply", flush=True)
    elif kind == "samples":
        n, n_fast = cases.samples_case(O, arg, 64, None)
        assert arg != "c4-cap-forced" or n_fast > 0
    elif kind == "sync":
        cases.sync_case(O, 64, None, prefix=[3, 3, 2] if arg == "prefix" else None)
    elif kind == "run_self_play":
        with tempfile.TemporaryDirectory() as tmp:
            print(cases.run_self_play_case(tmp, None, games=150, G=64, game="Connect4"), flush=True)
    elif kind == "curve":
        cases.curve_case(64, None)
    elif kind == "refusals":
        msgs = {n: cases.refusal_case(n, None) for n in sorted(cases.REFUSALS) + ["struct-size"]}
        for n, m in msgs.items():
            print(n, "->", m, flush=True)
        assert len({msgs[n] for n in ("struct-size", "threshold-nan", "threshold-inf", "threshold-negative", "threshold-one", "consecutive-zero",
                                      "min-ply-negative", "prob-nan")}) == 8
    elif kind == "scheduling":
        cases.scheduling_case(arg)
    else:
        raise SystemExit(f"unknown case {name}")


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", ["c4", "ttt", "ttt-min4", "c4-gumbel", "gmk-gumbel", "gmk-puct", "c4-leaf4", "c4-single"])
def test_records_are_prefixes_and_the_counters_follow(name):
    STEPS.run(__file__, "prefix:" + name, 180 if name == "gmk-puct" else 120)


def test_a_game_resigns_after_a_fast_ply():
    STEPS.run(__file__, "fast", 120)


def test_anchors_late_min_ply_all_playout_and_threshold_0():
    STEPS.run(__file__, "anchors", 120)


@pytest.mark.parametrize("name", ["c4", "c4-cap-forced", "ttt", "c4-gumbel"])
def test_drain_samples_equals_record_to_samples(name):
    STEPS.run(__file__, "samples:" + name, 120)


@pytest.mark.parametrize("which", ["plain", "prefix"])
def test_sync_engine_halts_after_the_resigning_ply(which):
    STEPS.run(__file__, "sync:" + which, 120)


def test_run_self_play_reads_the_four_keys():
    STEPS.run(__file__, "run_self_play", 120)


def test_resign_curve_equals_the_restated_rule():
    STEPS.run(__file__, "curve", 120)


def test_refusals():
    STEPS.run(__file__, "refusals", 120)


@pytest.mark.parametrize("which", ["fused", "groups", "cache"])
def test_records_do_not_depend_on_scheduling(which):
    STEPS.run(__file__, "scheduling:" + which, 180)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

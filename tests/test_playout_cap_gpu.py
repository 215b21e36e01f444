"""-m gpu: playout cap randomisation (gaz_engine_config.fast_iterations / full_search_prob) on the HIP build — the cases of
tests/playout_cap_cases.py at the sizes where the launch shapes matter (64 games: four games per wavefront running different limits;
128 games in two game groups; Gomoku games longer than 128 plies through the sample kernel's compaction), and the scheduling
equalities with the network.  Exact equality everywhere: no tolerance.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the cases (run in the child)
def _long_gomoku_case():
    """Gomoku games of more than 128 plies: the kept-row table of k_build_samples is filled by more than two wavefronts' ballots"""
    import playout_cap_cases as cases
    recs = cases.samples_case("gmk-long", None)
    print(f"gmk-long: (plies, kept rows) {sorted((r['T'], int((r['move_kind'] != 2).sum())) for r in recs.values())}", flush=True)
    # a game whose third wavefront of plies (128 ...) holds kept rows behind plies left out of the second one (64 .. 127)
    assert any(r["T"] > 128 and (r["move_kind"][64:128] == 2).any() and (r["move_kind"][128:] != 2).any() for r in recs.values())


def _run_case(name):
    import tempfile
    import playout_cap_cases as cases
    from oracle import gaz_oracle as O
    O.build()
    kind, _, arg = name.partition(":")
    if kind == "hash":
        cases.hash_case(O, arg, 64, None)
    elif kind == "selfplay":
        cases.selfplay_case(O, arg, 64, None)
    elif kind == "anchors":
        print(f"anchors: {cases.anchor_case(64, None)} rows left out", flush=True)
    elif kind == "gumbel":
        if arg == "batch":
            cases.gumbel_batch_case(64, None)
        else:
            cases.gumbel_case(O, 64, None, cap=arg == "cap")
    elif kind == "samples":
        if arg == "gmk-long":
            _long_gomoku_case()
        elif arg == "rows":
            cases.row_accounting_case(None)
        else:
            cases.samples_case(arg, None)
    elif kind == "run_self_play":
        with tempfile.TemporaryDirectory() as tmp:
            cases.run_self_play_case(tmp, None, gumbel=arg == "gumbel", games=150, G=64)
    elif kind == "refusals":
        for n in sorted(cases.REFUSALS):
            print(n, "->", cases.refusal_case(n, None), flush=True)
        cases.lower_run_iterations_case(O, None)
    elif kind == "scheduling":
        cases.scheduling_case(arg)
    else:
        raise SystemExit(f"unknown case {name}")


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", ["ttt", "c4-k1", "c4-k4", "gmk"])
def test_limits_per_move_equal_the_model(name):
    STEPS.run(__file__, "hash:" + name, 300 if name == "gmk" else 120)


@pytest.mark.parametrize("name", ["ttt", "c4"])
def test_continuous_selfplay_two_trees_equal_the_model(name):
    STEPS.run(__file__, "selfplay:" + name, 120)


def test_anchors_p1_and_fast_equal_full():
    STEPS.run(__file__, "anchors", 120)


def test_gumbel_comparator_holds_without_the_cap():
    STEPS.run(__file__, "gumbel:plain", 120)


def test_gumbel_with_the_cap_equals_host_set_limits():
    STEPS.run(__file__, "gumbel:cap", 120)


def test_gumbel_batch_4_with_the_cap_equals_gumbel_batch_1():
    STEPS.run(__file__, "gumbel:batch", 120)


@pytest.mark.parametrize("name", ["ttt", "c4", "gmk", "c4-groups", "gmk-long", "rows"])
def test_samples_device_path_equals_host_path_and_the_kept_rows(name):
    STEPS.run(__file__, "samples:" + name, 180)


@pytest.mark.parametrize("search", ["puct", "gumbel"])
def test_run_self_play_reads_the_train_config_keys(search):
    STEPS.run(__file__, "run_self_play:" + search, 120)


def test_refusals_and_lowered_run_iterations():
    STEPS.run(__file__, "refusals", 120)


@pytest.mark.parametrize("which", ["fused", "groups", "cache"])
def test_records_do_not_depend_on_scheduling(which):
    STEPS.run(__file__, "scheduling:" + which, 180)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

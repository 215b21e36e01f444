"""-m gpu: policy surprise weighting of the training rows (gaz_engine_set_sample_weighting, gaz_engine_drain_samples2) on the HIP build —
the cases of tests/surprise_cases.py against tests/surprise_model.py at the sizes where the launch shapes matter: 64 games at once per game
type, ragged counts (1, 3 and 67 Connect4 games, 1 and 9 Gomoku games), Gomoku records longer than 128 plies (the scan of k_build_samples_w
crosses wavefronts) and the 1-block network with the fused launch, two game groups and the evaluation cache.  Exact equality everywhere.

A game has at most about T <= 225 rows, so the fill of the row table never takes a second pass of 256 lanes on this
build; the long case has T > 128 with more than 128 rows, so that the scan over plies and the fill by output row cross the wavefronts at 64
and 128, and prints (plies, rows) of every game.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py; a step takes a few seconds, its limit is a kill guard."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the cases (run in the child)
def _long_gomoku_case(O):
    import surprise_cases as cases
    from playout_cap_cases import no_five_prefix
    recs, got = cases.weighted_case(O, "gmk-long", None, games_per_slot=1, witness=False, prefix=no_five_prefix(110))
    sizes = sorted((r["T"], got[k][1].shape[1]) for k, r in recs.items())
    print(f"gmk-long: (plies, rows) {sizes}", flush=True)
    assert any(T > 128 and rows > 128 for T, rows in sizes), sizes
    # and the weighting acted behind the prefix: a searched ply beyond the second wavefront with no row or with two
    assert any(r["T"] > 128 and len(set(np_counts(got[k][4], r["T"])[128:].tolist()) - {1}) > 0 for k, r in recs.items())


def np_counts(plies, T):
    import numpy as np
    return np.bincount(plies, minlength=T)


def _run_case(name):
    import tempfile
    import surprise_cases as cases
    from oracle import gaz_oracle as O
    O.build()
    kind, _, arg = name.partition(":")
    if kind == "weighted":
        cases.weighted_case(O, arg, None, G=64)
    elif kind == "ragged":
        case, _, g = arg.partition("@")
        cases.weighted_case(O, case, None, G=int(g), witness=False)
    elif kind == "long":
        _long_gomoku_case(O)
    elif kind == "full":
        recs, got = cases.weighted_case(O, "gmk-full", None, games_per_slot=1, witness=False)
        fast_rows = sum(int((r["move_kind"][got[k][4]] == 2).sum()) for k, r in recs.items())
        fast = sum(int((r["move_kind"] == 2).sum()) for r in recs.values())
        fast_written = sum(len(set(got[k][4][r["move_kind"][got[k][4]] == 2].tolist())) for k, r in recs.items())
        print(f"gmk-full: plies {sorted(r['T'] for r in recs.values())}, {fast_written} of {fast} fast plies got {fast_rows} rows", flush=True)
        assert 0 < fast_written < fast
    elif kind == "network":
        cases.network_case()
    elif kind == "anchors":
        for case, feature in (("c4-on", "plain"), ("c4-off", "plain"), ("ttt-on", "solver"), ("ttt-on", "forced"), ("ttt-on", "symmetry"), ("ttt-on", "resign")):
            print(case, feature, cases.lambda_zero_case(case, feature, None), flush=True)
        cases.switch_case(O, "ttt-on", None)
        cases.conservation_case(O, None)
    elif kind == "capacity":
        cases.capacity_case(O, None)
        cases.groups_case(O, None, G=64)
        cases.short_games_case(O, None)
    elif kind == "run":
        print(cases.refusal_case(None), flush=True)
        with tempfile.TemporaryDirectory() as tmp:
            cases.run_self_play_case(O, tmp, None, games=150, G=64)
    else:
        raise SystemExit(f"unknown case {name}")


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", ["ttt-on", "c4-on", "gmk-on", "c4-off"])
def test_64_games_at_once_equal_the_model(name):
    STEPS.run(__file__, "weighted:" + name, 40)


@pytest.mark.parametrize("arg", ["c4-on@1", "c4-on@3", "c4-on@67", "gmk-on@1", "gmk-on@9"])
def test_ragged_game_counts_equal_the_model(arg):
    STEPS.run(__file__, "ragged:" + arg, 40)


def test_gomoku_records_longer_than_128_plies():
    STEPS.run(__file__, "long", 60)


def test_gomoku_games_of_natural_length_at_the_default_fast_factor():
    """A = 225: fast plies that beat 1.5 x the mean surprise of the full ones earn rows, the others none — both must occur"""
    STEPS.run(__file__, "full", 60)


def test_network_fused_launch_two_groups_and_cache():
    STEPS.run(__file__, "network", 60)


def test_anchors_lambda_zero_switching_and_conservation():
    STEPS.run(__file__, "anchors", 60)


def test_capacity_groups_and_short_games():
    STEPS.run(__file__, "capacity", 60)


def test_refusals_and_run_self_play():
    STEPS.run(__file__, "run", 60)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

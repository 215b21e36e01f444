"""-m gpu: resignation in self-play (gaz_engine_set_resignation) on the HIP build — the cases of tests/resign_cases.py at the sizes where
the launch shapes matter (64 games: four games per wavefront, of which some resign while their neighbours play on; Gomoku's PUCT search
with compacted trees; two game groups), and the scheduling equalities with the network.  Exact equality everywhere: no tolerance.

Every GPU step is a child process of its own under a time limit (this file run as a script with the case's name); after a child that
was killed or ran out of time nothing more is started."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dead = []


def _step(case, seconds):
    if _dead:
        pytest.fail(f"not started: the GPU step {_dead[0]} was killed or ran out of time")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), case], cwd=ROOT, timeout=seconds, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _dead.append(case)
        pytest.fail(f"{case}: no result within {seconds} s")
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _dead.append(case)
    print(r.stdout[-4000:])
    assert r.returncode == 0, f"{case}: exit status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"


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
    _step("prefix:" + name, 180 if name == "gmk-puct" else 120)


def test_a_game_resigns_after_a_fast_ply():
    _step("fast", 120)


def test_anchors_late_min_ply_all_playout_and_threshold_0():
    _step("anchors", 120)


@pytest.mark.parametrize("name", ["c4", "c4-cap-forced", "ttt", "c4-gumbel"])
def test_drain_samples_equals_record_to_samples(name):
    _step("samples:" + name, 120)


@pytest.mark.parametrize("which", ["plain", "prefix"])
def test_sync_engine_halts_after_the_resigning_ply(which):
    _step("sync:" + which, 120)


def test_run_self_play_reads_the_four_keys():
    _step("run_self_play", 120)


def test_resign_curve_equals_the_restated_rule():
    _step("curve", 120)


def test_refusals():
    _step("refusals", 120)


@pytest.mark.parametrize("which", ["fused", "groups", "cache"])
def test_records_do_not_depend_on_scheduling(which):
    _step("scheduling:" + which, 180)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

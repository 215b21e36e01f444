"""CPU suite: the held-out loss (SelfPlayEngine.score_outputs / score_replay, replay.score_network, Run(replay=dict(score=...)); the "HELD-OUT
LOSS" section of include/gaz_engine.h; csrc/score.hpp) on the one-lane emulation build — the cases of tests/score_cases.py against
tests/score_model.py — the ctypes mirror of gaz_score_totals against the header, and the stand-alone sanitizer driver
(tests/emu/score_main.cpp).  Raw bits everywhere: no tolerance."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import score_cases as cases
from conftest import ROOT
from selfplay_support import emu_lib  # noqa: F401

GAMES3 = cases.GAMES3


# ------------------------------------------------------------------------------------------------ 0. the model alone
@pytest.mark.parametrize("game", GAMES3)
def test_the_model_alone_produces_the_witnesses(game):
    cases.model_witness_case(game)


# ------------------------------------------------------------------------------------------------ 1. score_outputs
@pytest.mark.parametrize("game", GAMES3)
def test_score_outputs_equals_the_model_in_every_bit(emu_lib, game):
    """all four modes, n = 1 .. 257, the hand-built rows, a batch that is all bad, n = 0"""
    assert cases.outputs_case(game, emu_lib) == 4 * len(cases.SIZES)


def test_score_outputs_on_an_engine_of_two_game_groups(emu_lib):
    assert cases.outputs_case("TicTacToe", emu_lib, grouped=True) == 4 * len(cases.SIZES)


def test_the_default_mode_is_the_engines_head(emu_lib):
    cases.own_mode_case(emu_lib)


# ------------------------------------------------------------------------------------------------ 2. score_replay
@pytest.mark.parametrize("game,sizes", [("TicTacToe", cases.REPLAY_SIZES), ("Connect4", cases.REPLAY_SIZES), ("Gomoku", (0, 2, 129))])
def test_score_replay_with_the_hash_evaluator(emu_lib, game, sizes):
    """per-row arrays, totals and means, augment off and on, the same bits for batch_rows 1, 3, 7, 64 and M, and twice the same"""
    seen = cases.replay_case(game, emu_lib, sizes=sizes)
    assert seen["plans"] == 2 * len(sizes)


def test_the_test_split_and_the_train_split(emu_lib):
    cases.split_case("Connect4", emu_lib)


def test_scoring_leaves_a_running_engines_games_untouched(emu_lib):
    assert cases.untouched_case(emu_lib) == 8


# ------------------------------------------------------------------------------------------------ 3. the engine's own rows; Run
def test_drained_rows_scored_by_score_network(emu_lib, tmp_path):
    rows = cases.drained_case(tmp_path, emu_lib)
    assert rows["test"] > 0 and rows["train"] > rows["test"]


def test_run_writes_score_json_equal_to_the_model(emu_lib, tmp_path):
    cases.run_case(tmp_path, emu_lib)


def test_every_refusal_by_its_text(emu_lib):
    msgs = cases.refusal_case(emu_lib)
    assert len(set(msgs.values())) >= 11 and "other-device" in msgs


# ------------------------------------------------------------------------------------------------ 4. ABI
def test_ctypes_mirror_of_the_totals_matches_the_header(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_stub
    from grok_alpha_zero_amd.engine import ScoreTotals
    hdr = abi_stub.parse_structs()["gaz_score_totals"]
    want = [(f, getattr(C, abi_stub.CTYPES[t])) for f, t, n in hdr]
    assert all(n == 0 for _, _, n in hdr) and list(ScoreTotals._fields_) == want
    fields = [f for f, _ in ScoreTotals._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gaz_engine.h"\nint main(void){printf("%zu\\n", sizeof(gaz_score_totals));'
                   + "".join(f'printf("%zu\\n", offsetof(gaz_score_totals, {f}));' for f in fields) + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).decode().split()]
    assert out[0] == C.sizeof(ScoreTotals) and out[1:] == [getattr(ScoreTotals, f).offset for f in fields]
    exec(abi_stub.stub_text(), ns := {"C": C})
    assert C.sizeof(ns["ScoreTotals"]) == C.sizeof(ScoreTotals)


def test_libraries_export_the_score_symbols(emu_lib):
    from grok_alpha_zero_amd import engine as E
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaz_engine.h")).read(), flags=re.S)
    want = set(re.findall(r"\b(gaz_(?:engine_)?score_\w+)\s*\(", hdr))
    assert want == {"gaz_score_totals_size", "gaz_engine_score_outputs", "gaz_engine_score_replay", "gaz_engine_score_rows_timed"}
    for lib in [emu_lib] + ([E.DEFAULT_LIB] if os.path.exists(E.DEFAULT_LIB) else []):
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
        got = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert want <= got, (lib, sorted(want - got))


# ------------------------------------------------------------------------------------------------ 5. the sanitizer driver
@pytest.fixture(scope="module")
def driver():
    return cases.build_driver()


@pytest.mark.parametrize("game", [0, 1, 2])
def test_scoring_at_the_buffer_limits_under_the_sanitizers(driver, game):
    """the scorer's host code and the one-lane build of its kernels, linked into a program of their own with -fsanitize=address,undefined
    -fno-sanitize-recover=all, driven through the C ABI with caller buffers of exactly the documented sizes"""
    rc, out = cases.run_driver(driver, game)
    assert rc == 0, f"game {game}: exit status {rc}\n{out[-3000:]}"

"""CPU suite: the replay window (grok_alpha_zero_amd/replay.py, the gaz_replay_* section of include/gaz_engine.h; csrc/replay.hpp) on the
one-lane emulation build — the cases of tests/replay_cases.py against tests/replay_model.py — the ctypes mirror of gaz_replay_config against
the header, and the stand-alone sanitizer driver (tests/emu/replay_main.cpp).  Exact equality everywhere: no tolerance."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import replay_cases as cases
import replay_model as M
from conftest import ROOT
from selfplay_support import emu_lib  # noqa: F401

GAMES3 = ("TicTacToe", "Connect4", "Gomoku")


# ------------------------------------------------------------------------------------------------ 0. the model's own pieces
def test_the_models_vectorised_philox_is_det_philox():
    from grok_alpha_zero_amd.det import philox
    rng = np.random.default_rng(0)
    c = rng.integers(0, 2 ** 32, (4, 64), dtype=np.uint64)
    x, y = M.philox_np(c[0], c[1], c[2], c[3], 0x12345678, 0x9ABCDEF0)
    for i in range(64):
        assert philox(int(c[0, i]), int(c[1, i]), int(c[2, i]), int(c[3, i]), 0x12345678, 0x9ABCDEF0)[:2] == (int(x[i]), int(y[i]))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 16, 17, 255, 256, 257, 1000])
def test_the_models_order_is_a_permutation(n):
    for epoch in (0, 1, 7):
        assert sorted(M.perm(9, q, n, epoch, 0) for q in range(n)) == list(range(n))


# ------------------------------------------------------------------------------------------------ 1. the store
@pytest.mark.parametrize("game", GAMES3)
def test_store_round_trip_ring_eviction_and_info(emu_lib, game):
    cases.store_case(game, emu_lib)


# ------------------------------------------------------------------------------------------------ 2. the plan
@pytest.mark.parametrize("rows", [1, 2, 3, 5, 255, 256, 257])
def test_plan_equals_the_model(emu_lib, rows):
    """train and test, test_fraction 0 and 0.3, target_ratio NaN / 0.5 / 0.0 / 1.0, newest_generation below the newest stored, a decay that
    empties the oldest generation"""
    seen = cases.plan_case(rows, emu_lib)
    assert seen["plans"] == 24
    if rows >= 255:
        assert seen["skipped"] > 0 and seen["empty_old_generation"] > 0 and seen["rows"] > 0, seen


def test_plan_of_65537_rows_crosses_the_scans_second_pass(emu_lib):
    seen = cases.plan_case(65537, emu_lib, windows=((0.3, 0.5),), epochs=((5, 1.0, 0.25),))
    assert seen["plans"] == 2 and seen["skipped"] > 0 and seen["rows"] > 256 * 256 // 2, seen


# ------------------------------------------------------------------------------------------------ 3. order and gather
@pytest.mark.parametrize("n_plan", [1, 2, 3, 5, 17, 257])
def test_epoch_order_symmetries_and_bytes_equal_the_model(emu_lib, n_plan):
    cases.gather_case("Connect4", n_plan, emu_lib)


@pytest.mark.parametrize("game,n_plan", [("TicTacToe", 257), ("TicTacToe", 5), ("Gomoku", 17), ("Gomoku", 257)])
def test_gather_of_the_other_games(emu_lib, game, n_plan):
    cases.gather_case(game, n_plan, emu_lib)


# ------------------------------------------------------------------------------------------------ 4. against the engine
@pytest.mark.parametrize("game", GAMES3)
@pytest.mark.parametrize("mode", ["plain", "cap"])
def test_sampled_rows_are_planes_of_the_drained_batch(emu_lib, game, mode):
    rows, plies = cases.engine_case(game, mode, emu_lib)
    assert rows > 0 and (rows == plies) == (mode == "plain")


# ------------------------------------------------------------------------------------------------ 5. run level
def test_live_and_refilled_windows_are_the_same_and_the_file_is_unchanged(emu_lib, tmp_path):
    cases.refill_case(tmp_path, emu_lib)


def test_run_with_a_replay_window_resumed_once(emu_lib, tmp_path):
    cases.run_case(tmp_path, emu_lib)


def test_every_refusal_by_its_text(emu_lib):
    msgs = cases.refusal_case(emu_lib)
    assert len(set(msgs.values())) >= 12


def test_batch_torch_refuses_a_process_that_loaded_the_library_before_torch(emu_lib, monkeypatch):
    from grok_alpha_zero_amd.engine import EngineError
    w = cases.window("TicTacToe", 10, emu_lib)
    w.append_arrays(0, *cases.random_rows(np.random.default_rng(0), "TicTacToe", [3]))
    assert w.begin_epoch() == 3
    monkeypatch.setattr(w.L, "_gaz_torch_first", False, raising=False)
    with pytest.raises(EngineError, match="import torch before"):
        w.batch_torch(0, 3)
    w.close()


# ------------------------------------------------------------------------------------------------ 6. ABI
def test_ctypes_mirror_of_the_config_matches_the_header(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_stub
    from grok_alpha_zero_amd.replay import ReplayConfig
    hdr = abi_stub.parse_structs()["gaz_replay_config"]
    want = [(f, getattr(C, abi_stub.CTYPES[t])) for f, t, n in hdr]
    assert all(n == 0 for _, _, n in hdr) and list(ReplayConfig._fields_) == want
    fields = [f for f, _ in ReplayConfig._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gaz_engine.h"\nint main(void){printf("%zu\\n", sizeof(gaz_replay_config));'
                   + "".join(f'printf("%zu\\n", offsetof(gaz_replay_config, {f}));' for f in fields) + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).decode().split()]
    assert out[0] == C.sizeof(ReplayConfig) and out[1:] == [getattr(ReplayConfig, f).offset for f in fields]


def test_libraries_export_the_replay_symbols(emu_lib):
    from grok_alpha_zero_amd import engine as E
    hdr = open(os.path.join(ROOT, "include", "gaz_engine.h")).read()
    import re
    want = set(re.findall(r"\b(gaz_replay_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert len(want) >= 14
    for lib in [emu_lib] + ([E.DEFAULT_LIB] if os.path.exists(E.DEFAULT_LIB) else []):
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
        got = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert want <= got, (lib, sorted(want - got))


# ------------------------------------------------------------------------------------------------ 7. the sanitizer driver
@pytest.fixture(scope="module")
def driver():
    return cases.build_driver()


@pytest.mark.parametrize("name", sorted(cases.DRIVER_CASES))
def test_window_at_the_buffer_limits_under_the_sanitizers(driver, name):
    """the window's host code and the one-lane build of its kernels, linked into a program of their own with -fsanitize=address,undefined
    -fno-sanitize-recover=all, driven through the C ABI with caller buffers of exactly the documented sizes"""
    rc, out = cases.run_driver(driver, name)
    assert rc == 0, f"{name}: exit status {rc}\n{out[-3000:]}"

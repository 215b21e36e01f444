"""-m gpu: the replay window (grok_alpha_zero_amd/replay.py, the gaz_replay_* section of include/gaz_engine.h; csrc/replay.hpp) on the HIP
build — the cases of tests/replay_cases.py against tests/replay_model.py, where the launch shapes matter: the ballots and the scan of the
plan builder at 1 .. 257 and 65537 live rows (one lane, a ragged wavefront, two blocks, the scan's second pass), k_replay_sample for all three
games at every batch size from 1 to 257 rows (ragged last workgroups, batches that start anywhere in the epoch, a ring that wraps; Gomoku at
257 rows exercises the wide rows), and batch_torch against batch.  Exact equality everywhere.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py; a step takes a few seconds, its limit is a kill guard."""
import os
import sys

import pytest

from gpu_step import STEPS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_case():
    """batch_torch == batch: zero-copy views of the window's device buffers handed to torch, for every game, with and without the index arrays"""
    import numpy as np
    import torch
    import replay_cases as cases
    rng = np.random.default_rng(4)
    for game in ("TicTacToe", "Connect4", "Gomoku"):
        w = cases.window(game, 300, None, seed=8)
        w.append_arrays(0, *cases.random_rows(rng, game, [7, 0, 93, 157]))
        assert w.begin_epoch() == 257
        for first, n in ((0, 257), (3, 65), (256, 1), (257, 0)):
            want = w.batch(first, n, with_index=True)
            got = w.batch_torch(first, n, with_index=True)
            assert all(t.is_cuda for t in got) and [tuple(t.shape) for t in got] == [a.shape for a in want]
            for t, a in zip(got, want):
                assert t.cpu().numpy().tobytes() == a.tobytes(), (game, first, n)
            assert len(w.batch_torch(first, n)) == 3
        x = torch.ones(4, device="cuda") * 2                               # torch goes on working next to the window
        assert float(x.sum()) == 8.0
        w.close()


def _run_case(name):
    import tempfile
    import replay_cases as cases
    kind, _, arg = name.partition(":")
    if kind == "store":
        for game in ("TicTacToe", "Connect4", "Gomoku"):
            cases.store_case(game, None)
    elif kind == "plan":
        if arg == "small":
            for rows in (1, 2, 3, 5, 255, 256, 257):
                seen = cases.plan_case(rows, None)
                print(rows, seen, flush=True)
                assert seen["plans"] == 24 and (rows < 255 or (seen["skipped"] > 0 and seen["empty_old_generation"] > 0))
        else:
            seen = cases.plan_case(65537, None, windows=((0.3, 0.5),), epochs=((5, 1.0, 0.25),))
            print(seen, flush=True)
            assert seen["plans"] == 2 and seen["skipped"] > 0 and seen["rows"] > 256 * 256 // 2
    elif kind == "gather":
        for n_plan in (1, 2, 3, 5, 17, 257):
            print(arg, n_plan, cases.gather_case(arg, n_plan, None), flush=True)
    elif kind == "engine":
        for mode in ("plain", "cap"):
            rows, plies = cases.engine_case(arg, mode, None)
            print(arg, mode, rows, plies, flush=True)
            assert rows > 0 and (rows == plies) == (mode == "plain")
    elif kind == "run":
        print(cases.refusal_case(None), flush=True)
        with tempfile.TemporaryDirectory() as tmp:
            cases.refill_case(tmp, None)
            cases.run_case(tmp, None)
    elif kind == "torch":
        _torch_case()
    else:
        raise SystemExit(f"unknown case {name}")


def test_store_round_trip_ring_eviction_and_info():
    STEPS.run(__file__, "store", 40)


def test_plans_of_1_to_257_rows_equal_the_model():
    STEPS.run(__file__, "plan:small", 60)


def test_plan_of_65537_rows_crosses_the_scans_second_pass():
    STEPS.run(__file__, "plan:65537", 40)


@pytest.mark.parametrize("game", ["TicTacToe", "Connect4", "Gomoku"])
def test_epoch_order_symmetries_and_bytes_equal_the_model(game):
    STEPS.run(__file__, "gather:" + game, 40)


@pytest.mark.parametrize("game", ["TicTacToe", "Connect4", "Gomoku"])
def test_sampled_rows_are_planes_of_the_drained_batch(game):
    STEPS.run(__file__, "engine:" + game, 60)


def test_refusals_refill_and_run():
    STEPS.run(__file__, "run", 60)


def test_batch_torch_equals_batch():
    STEPS.run(__file__, "torch", 60)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run_case(sys.argv[1])
    print("ok", flush=True)

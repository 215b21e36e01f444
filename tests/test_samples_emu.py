"""CPU suite: finished games leave the engine as training samples (gaz_engine_drain_samples, csrc/samples.hpp), on the one-lane
emulation build.  Everything is compared for EXACT equality: integer planes, copied floats, and one fp32 add and multiply that both
sides do in the same order.

  1  against the arrays the reference's Self_Play.play() wrote (the aug_* / values arrays of the golden fixtures)
  2  against the host path (drain_finished + record_to_samples) over many games, every engine shape that drains records
  3  drain_finished and drain_samples mixed on one engine; refusals
  4  run_self_play: the replay file at both settings of device_samples; foreign plugins; a failing writer"""
import os
import threading

import numpy as np
import pytest

from conftest import GOLDEN
from samples_util import (assert_matches_reference_fixture, assert_same_file, assert_same_game, device_games, file_contents,
                          host_games)
from selfplay_support import emu_lib  # noqa: F401


def _search_kw(search):
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL, SEARCH_PUCT
    return dict(search=SEARCH_GUMBEL, gumbel_m=4, c_visit=50.0, c_scale=1.0) if search == "gumbel" else dict(search=SEARCH_PUCT)


# ---- 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ttt_puct_a", "c4_puct_a", "c4_puct_c", "gmk_puct_a"])
def test_drain_samples_reproduces_reference_replay_arrays(emu_lib, name):
    """The fixture's game played by the engine (seed, slot, salt and settings from the fixture, as test_engine_emu.play_fixture does)
    and taken with drain_samples == every augmentation plane the reference wrote, dtype and shape included."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    eng = SelfPlayEngine(str(fx["game"]), 1, int(fx["run_iterations"]), int(fx["max_actions"]), int(fx["explore_first"]),
                         int(fx["explore_second"]), float(fx["c_puct_init"]), float(fx["dirichlet_alpha"]), int(fx["seed"]),
                         slot_offset=int(fx["slot"]), hash_salt=int(fx["salt"]), ring_capacity=8, lib_path=emu_lib)
    got = []
    for _ in range(20000):
        eng.run_waves(64)
        got += device_games(eng)
        if any(g[0][1] == int(fx["game_seq"]) for g in got):
            break
    eng.close()
    game = [g for g in got if g[0] == (int(fx["slot"]), int(fx["game_seq"]))][0]
    assert_matches_reference_fixture(game, fx)


# ---- 2 -------------------------------------------------------------------------------------------------------------------------
def _pair(emu_lib, game, search, G, iters, max_actions, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    kw = dict(dict(_search_kw(search), ring_capacity=8 * G), **kw)
    mk = lambda: SelfPlayEngine(game, G, iters, max_actions, 3, 2, 2.5, 0.5, seed=23, hash_salt=6, slot_offset=10, lib_path=emu_lib, **kw)   # noqa: E731
    return mk(), mk()


def _run_pair(host_eng, dev_eng, game, want, waves=16, max_calls=4000, between=None, **drain_kw):
    """both engines get the same calls; -> (host games, device games), each in the order handed out"""
    from grok_alpha_zero_amd.games import GAMES
    host, dev = [], []
    for call in range(max_calls):
        host_eng.run_waves(waves); dev_eng.run_waves(waves)
        host += host_games(host_eng, GAMES[game])
        dev += device_games(dev_eng, **drain_kw)
        if between:
            between(call, host_eng, dev_eng, len(host))
        if len(host) >= want and len(dev) >= want:
            break
    return host, dev


CASES = [("TicTacToe", "puct", 8, 12, 9, 50), ("TicTacToe", "gumbel", 8, 12, 9, 50), ("Connect4", "puct", 16, 12, 42, 50),
         ("Connect4", "gumbel", 16, 12, 42, 50), ("Gomoku", "puct", 4, 10, 10, 6), ("Gomoku", "gumbel", 4, 10, 10, 6)]


@pytest.mark.parametrize("game,search,G,iters,max_actions,want", CASES)
def test_drain_samples_equals_the_host_path(emu_lib, game, search, G, iters, max_actions, want):
    """Two engines with the same seed, one drained through drain_finished + record_to_samples and one through drain_samples: the same
    games in the same order, all arrays equal."""
    a, b = _pair(emu_lib, game, search, G, iters, max_actions)
    host, dev = _run_pair(a, b, game, want)
    a.close(); b.close()
    assert len(host) >= want and len(host) == len(dev)
    for d, h in zip(dev, host):
        assert_same_game(d, h, f"{game} {search}")


def test_drain_samples_with_two_game_groups(emu_lib):
    a, b = _pair(emu_lib, "Connect4", "puct", 12, 12, 42, game_groups=2)
    assert b.stats()["game_groups"] == 2
    host, dev = _run_pair(a, b, "Connect4", 40)
    a.close(); b.close()
    assert len(host) >= 40 and len(host) == len(dev)
    for d, h in zip(dev, host):
        assert_same_game(d, h, "two game groups")


@pytest.mark.parametrize("groups", [1, 2])
def test_drain_samples_after_repack(emu_lib, groups):
    """a generation with a budget: once slots have halted both engines repack; every admitted game still comes out, equal"""
    G, budget = 12, 40
    a, b = _pair(emu_lib, "Connect4", "puct", G, 12, 42, games_budget=budget, game_groups=groups)
    packed = []

    def between(call, ha, hb, n_host):
        if not packed and n_host >= budget - G // 2:
            ra, rb = ha.repack(), hb.repack()
            assert ra == rb
            packed.append(ra)
    host, dev = _run_pair(a, b, "Connect4", budget, between=between)
    a.close(); b.close()
    assert packed and packed[0][1] < G, packed                        # the launches did shrink
    assert len(host) == budget == len(dev)
    assert sorted(h[0] for h in host) == sorted((10 + g, k) for k in range(4) for g in range(G) if k * G + g < budget)
    for d, h in zip(dev, host):
        assert_same_game(d, h, "after repack")


def test_drain_samples_of_games_placed_by_set_position(emu_lib):
    """records of games placed by gaz_engine_set_position have a prefix without search: its rows come out as the host path gives them
    (input planes of the prefix positions, policy rows of zeros, values from q = 0)"""
    from test_engine_emu import _legal_prefix
    rng = np.random.default_rng(5)
    prefixes = [_legal_prefix("Connect4", n, rng) for n in (3, 6, 0, 9)]
    a, b = _pair(emu_lib, "Connect4", "puct", 4, 12, 42, games_budget=4)
    for eng in (a, b):
        for g, h in enumerate(prefixes):
            if h:
                eng.set_position(g, h)
    host, dev = _run_pair(a, b, "Connect4", 4)
    a.close(); b.close()
    assert len(host) == 4 == len(dev)
    for d, h in zip(dev, host):
        assert_same_game(d, h, "set_position prefix")
        n = len(prefixes[d[0][0] - 10])
        assert d[4] > n and not d[2][:, :n].any() and (n == 0 or d[1][0, n - 1].any())     # zero policies, real boards in the prefix
        assert d[2][0, n:].any()


def test_drain_samples_leaves_what_does_not_fit(emu_lib):
    """max_rows so small that games stay behind for the next call: every game still comes out exactly once, whole and in order; the
    same with a small max_games"""
    a, b = _pair(emu_lib, "TicTacToe", "puct", 8, 12, 9, ring_capacity=64)
    host, dev, left_behind = [], [], 0
    from grok_alpha_zero_amd.games import GAMES
    for call in range(400):
        a.run_waves(16); b.run_waves(16)
        host += host_games(a, GAMES["TicTacToe"])
        got = device_games(b, max_rows=20) if call % 2 == 0 else device_games(b, max_games=2)
        assert sum(g[4] for g in got) <= 20 or call % 2 == 1
        assert len(got) <= 2 or call % 2 == 0
        dev += got
        left_behind += len(host) > len(dev)
        if len(dev) >= 50:
            break
    for _ in range(200):                                              # what stayed in the ring
        got = device_games(b, max_rows=20)
        dev += got
        if not got:
            break
    a.close(); b.close()
    assert left_behind > 0 and len(dev) >= 50 and len(dev) <= len(host)
    assert len({g[0] for g in dev}) == len(dev)
    for d, h in zip(dev, host):                                       # the ring is first in, first out whatever a call takes
        assert_same_game(d, h, "small max_rows")


# ---- 3 -------------------------------------------------------------------------------------------------------------------------
def test_drain_finished_and_drain_samples_mixed(emu_lib):
    """alternated on ONE engine the two calls hand out each game once; together they give the games a reference engine gives"""
    from grok_alpha_zero_amd.games import GAMES
    ref, eng = _pair(emu_lib, "Connect4", "puct", 8, 12, 42)
    want, got = [], []
    for call in range(2000):
        ref.run_waves(16); eng.run_waves(16)
        want += host_games(ref, GAMES["Connect4"])
        got += device_games(eng, max_games=1) if call % 2 else host_games(eng, GAMES["Connect4"])[:]
        got += device_games(eng) if call % 3 == 0 else []
        if len(want) >= 30:
            break
    got += device_games(eng)
    ref.close(); eng.close()
    assert len(got) == len(want) and len({g[0] for g in got}) == len(got)
    for d, h in zip(got, want):
        assert_same_game(d, h, "mixed calls")


def test_drain_samples_refusals(emu_lib):
    from grok_alpha_zero_amd.engine import EngineError, SelfPlayEngine
    eng = SelfPlayEngine("Connect4", 2, 12, 42, 3, 2, 2.5, 0.5, seed=1, ring_capacity=8, lib_path=emu_lib)
    for _ in range(2000):
        eng.run_waves(16)
        if eng.stats()["game_stats"][2] >= 1:
            break
    with pytest.raises(EngineError, match="max_rows"):                # a Connect4 game has at least 7 plies
        eng.drain_samples(max_rows=3)
    got = device_games(eng)                                           # nothing was lost by the refusal
    assert len(got) >= 1
    eng.close()
    none = SelfPlayEngine("Connect4", 2, 12, 42, 3, 2, 2.5, 0.5, seed=1, ring_capacity=0, lib_path=emu_lib)
    none.run_waves(400)
    batch = none.drain_samples()
    assert batch.n == 0 and batch.rows == 0
    none.close()


# ---- 4 -------------------------------------------------------------------------------------------------------------------------
def _generation(tmp_path, emu_lib, tag, game_class, train, **kw):
    from grok_alpha_zero_amd.self_play import ReplayStore, run_self_play
    folder = str(tmp_path / tag / "0")
    store = ReplayStore(folder); store.create()
    n = run_self_play(game_class, ({}, train), folder, seed=7, hash_salt=3, lib_path=emu_lib, **kw)
    assert n == train["games_per_generation"]
    return file_contents(store)


TRAIN = {"TicTacToe": dict(games_per_generation=23, MCTS_iteration_limit=10, max_actions=9, num_explore_actions_first=2, num_explore_actions_second=1,
                           c_puct_init=2.5, dirichlet_alpha=0.5),
         "Connect4": dict(games_per_generation=17, MCTS_iteration_limit=8, max_actions=42, num_explore_actions_first=4, num_explore_actions_second=3,
                          c_puct_init=2.5, dirichlet_alpha=0.5)}


@pytest.mark.parametrize("game", ["TicTacToe", "Connect4"])
def test_run_self_play_writes_the_same_file_either_way(tmp_path, emu_lib, game):
    """every dataset name, dtype, shape and content and game_stats, device_samples False vs True (and None = True for a built-in plugin)"""
    from grok_alpha_zero_amd.games import GAMES
    stats = {}
    host = _generation(tmp_path, emu_lib, "host", GAMES[game], TRAIN[game], n_games=6, device_samples=False)
    dev = _generation(tmp_path, emu_lib, "dev", GAMES[game], TRAIN[game], n_games=6, device_samples=True, engine_stats=stats)
    auto = _generation(tmp_path, emu_lib, "auto", GAMES[game], TRAIN[game], n_games=6)
    n_aug = 8 if game == "TicTacToe" else 2
    assert len(host) == 1 + 3 * n_aug * TRAIN[game]["games_per_generation"] and host["game_stats"][2] == TRAIN[game]["games_per_generation"]
    assert_same_file(dev, host)
    assert_same_file(auto, host)
    assert {"gpu_wait_seconds", "sample_seconds", "queue_wait_seconds", "writer_seconds"} <= set(stats)


def test_run_self_play_foreign_plugin_takes_the_host_path(tmp_path, emu_lib, monkeypatch):
    from grok_alpha_zero_amd import engine as E
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import ReplayStore, run_self_play

    class MyTicTacToe(GAMES["TicTacToe"]):                            # a user's plugin: its own augment_sample has to run
        calls = 0

        def augment_sample(self, input_states, policies):
            MyTicTacToe.calls += 1
            return super().augment_sample(input_states, policies)

    builtin = _generation(tmp_path, emu_lib, "builtin", GAMES["TicTacToe"], TRAIN["TicTacToe"], n_games=6)

    def refuse(self, *a, **k):
        raise AssertionError("drain_samples called for a foreign plugin")
    monkeypatch.setattr(E.SelfPlayEngine, "drain_samples", refuse)
    mine = _generation(tmp_path, emu_lib, "mine", MyTicTacToe, TRAIN["TicTacToe"], n_games=6)
    assert MyTicTacToe.calls == TRAIN["TicTacToe"]["games_per_generation"]
    assert_same_file(mine, builtin)
    folder = str(tmp_path / "refused" / "0")
    ReplayStore(folder).create()
    with pytest.raises(ValueError, match="device_samples"):
        run_self_play(MyTicTacToe, ({}, TRAIN["TicTacToe"]), folder, n_games=6, seed=7, lib_path=emu_lib, device_samples=True)


@pytest.mark.parametrize("device_samples", [False, True])
def test_run_self_play_surfaces_a_failing_writer(tmp_path, emu_lib, monkeypatch, device_samples):
    """a store whose append_game raises: that exception reaches the caller of run_self_play, and no thread is left behind"""
    from grok_alpha_zero_amd import self_play as SP
    from grok_alpha_zero_amd.games import GAMES

    class DiskFull(Exception):
        pass
    real, seen = SP.ReplayStore.append_game, []

    def failing(self, *a, **k):
        seen.append(1)
        if len(seen) > 3:
            raise DiskFull("no space left")
        return real(self, *a, **k)
    monkeypatch.setattr(SP.ReplayStore, "append_game", failing)
    before = set(threading.enumerate())
    folder = str(tmp_path / "0")
    SP.ReplayStore(folder).create()
    with pytest.raises(DiskFull):
        SP.run_self_play(GAMES["TicTacToe"], ({}, dict(TRAIN["TicTacToe"], games_per_generation=60)), folder, n_games=6, seed=7, lib_path=emu_lib,
                         device_samples=device_samples)
    assert not [t for t in threading.enumerate() if t not in before and t.is_alive()]


def test_replay_writer_queue_is_bounded_in_bytes(tmp_path):
    """put() blocks while more than max_pending_bytes wait for the file, and goes on once the writer has caught up"""
    import time
    from grok_alpha_zero_amd.self_play import ReplayStore, _ReplayWriter
    gate, order = threading.Event(), []

    class SlowStore(ReplayStore):
        def append_game(self, *a):
            gate.wait(10)
            order.append(a[3])
    store = SlowStore(str(tmp_path)); store.create()
    w = _ReplayWriter(store, max_pending_bytes=100)
    game = lambda i: (np.zeros((1, 1, 1), np.int8), np.zeros((1, 1, 1), np.float32), np.zeros((1, 1, 1), np.float32), i, 1, 0)   # noqa: E731
    w.put(game(0), 60)
    done = []
    t = threading.Thread(target=lambda: (w.put(game(1), 60), done.append(1)))
    t.start(); time.sleep(0.3)
    assert not done                                                   # 120 bytes would be pending: blocked
    gate.set(); t.join(10)
    assert done
    w.close()
    assert order == [0, 1] and w.wait_seconds > 0.2

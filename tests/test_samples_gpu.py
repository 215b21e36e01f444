"""GPU suite: finished games leave the engine as training samples (gaz_engine_drain_samples, csrc/samples.hpp: k_build_samples), on
the HIP library.  Exact equality everywhere (see tests/test_samples_emu.py, whose items 1, 2 and 4 these are).

Two engines with the same seed play the same games, but on the GPU the ORDER in which games that finish in the same launch enter
the ring is decided by an atomic: where two engines are compared, games are matched by (slot, game_seq), each handed out once, and
the order is checked within one engine only (rows contiguous, in the order of `games`)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from samples_util import assert_matches_reference_fixture, assert_same_game, device_games, file_contents, host_games

pytestmark = pytest.mark.gpu


def _gpu():
    import torch
    assert torch.cuda.is_available(), "GPU test needs a GPU"


def _search_kw(search):
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL, SEARCH_PUCT
    return dict(search=SEARCH_GUMBEL, gumbel_m=4, c_visit=50.0, c_scale=1.0) if search == "gumbel" else dict(search=SEARCH_PUCT)


@pytest.mark.parametrize("name", ["ttt_puct_a", "c4_puct_a", "c4_puct_c", "gmk_puct_a"])
def test_drain_samples_on_hip_reproduces_reference_replay_arrays(name):
    """the fixture's game played by the HIP engine and taken with drain_samples == every augmentation plane the reference wrote"""
    _gpu()
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    fx = np.load(os.path.join(GOLDEN, name + ".npz"))
    eng = SelfPlayEngine(str(fx["game"]), 1, int(fx["run_iterations"]), int(fx["max_actions"]), int(fx["explore_first"]),
                         int(fx["explore_second"]), float(fx["c_puct_init"]), float(fx["dirichlet_alpha"]), int(fx["seed"]),
                         slot_offset=int(fx["slot"]), hash_salt=int(fx["salt"]), ring_capacity=8)
    got = []
    for _ in range(20000):
        eng.run_waves(64)
        got += device_games(eng)
        if any(g[0][1] == int(fx["game_seq"]) for g in got):
            break
    eng.close()
    game = [g for g in got if g[0] == (int(fx["slot"]), int(fx["game_seq"]))][0]
    assert_matches_reference_fixture(game, fx)


def _compare_pair(host_eng, dev_eng, game, want, waves, max_calls=4000, between=None):
    """the same calls on both engines; games are matched by (slot, game_seq) as they appear on both sides (with the evaluation cache
    a game may need a different number of waves on the two engines) and compared -> (games matched, games seen on one side only)"""
    from grok_alpha_zero_amd.games import GAMES
    n, host, dev, seen = 0, {}, {}, set()
    for call in range(max_calls):
        host_eng.run_waves(waves); dev_eng.run_waves(waves)
        for side, games in ((host, host_games(host_eng, GAMES[game])), (dev, device_games(dev_eng))):
            for g in games:
                assert g[0] not in side and g[0] not in seen, f"game {g[0]} handed out twice"
                side[g[0]] = g
        for key in sorted(set(host) & set(dev)):
            assert_same_game(dev.pop(key), host.pop(key), game)
            seen.add(key); n += 1
        if between:
            between(host_eng, dev_eng, n)
        if n >= want:
            break
    return n, len(host) + len(dev)


@pytest.mark.parametrize("game,search,G,iters,max_actions,want", [
    ("TicTacToe", "puct", 256, 24, 9, 1000), ("TicTacToe", "gumbel", 256, 16, 9, 1000), ("Connect4", "puct", 512, 40, 42, 1000),
    ("Connect4", "gumbel", 512, 32, 42, 1000), ("Gomoku", "puct", 64, 48, 40, 100), ("Gomoku", "gumbel", 32, 48, 24, 60)])
def test_drain_samples_on_hip_equals_the_host_path(game, search, G, iters, max_actions, want):
    _gpu()
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    mk = lambda: SelfPlayEngine(game, G, iters, max_actions, 3, 2, 2.5, 0.5, seed=23, hash_salt=6, slot_offset=10, ring_capacity=4 * G,   # noqa: E731
                                **_search_kw(search))
    a, b = mk(), mk()
    n, _ = _compare_pair(a, b, game, want, waves=32)
    a.close(); b.close()
    assert n >= want


def test_drain_samples_on_hip_headline_shape_with_the_network():
    """Connect4, 4096 slots, the 6-block network, two game groups, evaluation cache on, a budget whose tail is repacked: at least 200
    finished games, the device's samples equal to the host path's"""
    _gpu()
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
    from grok_alpha_zero_amd.net import Connect4Net
    w = Connect4Net(6, seed=4).eval().export_engine_weights()
    G, budget = 4096, 4500
    mk = lambda: SelfPlayEngine("Connect4", G, 16, 14, 4, 3, 2.5, 0.5, seed=31, evaluator=EVAL_RESNET, net_blocks=6, ring_capacity=2 * G,   # noqa: E731
                                eval_cache_log2=18, games_budget=budget, game_groups=2)
    a, b = mk(), mk()
    a.load_weights(w); b.load_weights(w)
    assert b.stats()["game_groups"] == 2
    packed = []

    def between(ha, hb, n):
        if not packed and n >= G:
            packed.append(ha.repack()); hb.repack()
    n, unmatched = _compare_pair(a, b, "Connect4", budget, waves=32, between=between)
    a.close(); b.close()
    assert n == budget >= 200 and unmatched == 0 and packed and packed[0][1] < G


def test_drain_samples_on_hip_gomoku_natural_ends():
    """Gomoku with BASELINE configs[3] parameters, 64 slots played to natural ends (tests/test_engine_gpu.py): whole-board games, rows of
    225 policies and 450-byte states, all 8 symmetries"""
    _gpu()
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    G, iters = 64, 400
    mk = lambda: SelfPlayEngine("Gomoku", G, iters, 225, 6, 4, 4.5, 0.05, seed=77, hash_salt=9, slot_offset=300, ring_capacity=4 * G, games_budget=G)   # noqa: E731
    a, b = mk(), mk()
    n, unmatched = _compare_pair(a, b, "Gomoku", G, waves=256, max_calls=20000)
    a.close(); b.close()
    assert n == G and unmatched == 0


@pytest.mark.parametrize("gumbel", [False, True], ids=["puct", "gumbel"])
def test_run_self_play_on_hip_writes_the_same_file_either_way(tmp_path, gumbel):
    """the generation of test_frows_gpu.py::test_run_self_play_on_hip_writes_the_oracles_games at both settings of device_samples:
    the files are equal dataset by dataset once the games are matched (the order of games that finish in one launch is the ring's)"""
    _gpu()
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import ReplayStore, run_self_play
    G, games = 64, 150
    train = dict(games_per_generation=games, MCTS_iteration_limit=32 if gumbel else 40, max_actions=42, num_explore_actions_first=8,
                 num_explore_actions_second=7, c_puct_init=2.5, dirichlet_alpha=0.5, use_gumbel=gumbel, m=7, c_visit=50.0, c_scale=1.0)
    out = {}
    for ds in (False, True):
        folder = str(tmp_path / f"ds{ds}" / "0")
        store = ReplayStore(folder); store.create()
        assert run_self_play(GAMES["Connect4"], ({}, train), folder, n_games=G, seed=7, hash_salt=3, device_samples=ds) == games
        out[ds] = file_contents(store)
    assert list(out[False]) == list(out[True]) and len(out[True]) == 1 + 3 * 2 * games
    np.testing.assert_array_equal(out[False]["game_stats"], out[True]["game_stats"])
    assert [(k, a.dtype, a.shape[1:]) for k, a in out[False].items()] == [(k, a.dtype, a.shape[1:]) for k, a in out[True].items()]

    def by_game(f):                                  # a game = its two augmentation triples, six consecutive datasets
        gs = []
        for k in range(games):
            arrs = [f[f"{kind}_{2 * k + j}"] for j in range(2) for kind in ("boards", "policies", "values")]
            gs.append(tuple((a.dtype.str, a.shape, a.tobytes()) for a in arrs))
        return sorted(gs)
    assert by_game(out[False]) == by_game(out[True])

"""What the case modules of the self-play features (tests/<feature>_cases.py) and their test modules share: the games' sizes, the
emulation library fixture, the loops that play a free-running engine until its games are there, record comparison, the 1-block Connect4
network engine and the skeleton of the scheduling equalities.  Every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU = os.path.join(EMU_DIR, "libgaz_emu.so")

MAXT = {"TicTacToe": 9, "Connect4": 42, "Gomoku": 225}
A_OF = {"TicTacToe": 9, "Connect4": 7, "Gomoku": 225}
N_AUG = {"TicTacToe": 8, "Connect4": 2, "Gomoku": 8}
SLOTS64 = (0, 1, 15, 16, 31, 32, 62, 63)          # first / last game of a wavefront's four teams, both ends of a 64-game batch
RECORD_KEYS = ("actions", "root_N", "root_W", "root_P", "root_visits", "policies", "values", "q", "z", "evals")
SEARCH_KEYS = ("actions", "policies", "q", "root_N", "root_W", "root_P", "root_visits", "evals")


@pytest.fixture(scope="session")
def emu_lib():
    """the one-lane emulation build of the device code.  A test module imports it by name: `from selfplay_support import emu_lib  # noqa: F401`"""
    subprocess.check_call(["make", "-s", "-C", EMU_DIR])
    return EMU


def slots_for(G, slots=SLOTS64):
    """the slots a case compares: `slots` of a 64-game batch, every slot of a smaller one"""
    return tuple(slots) if G >= 64 else tuple(range(G))


# ------------------------------------------------------------------------------------------------ playing a free-running engine
def play(eng, n, waves=32, rounds=40000, raw=False):
    """a free-running engine until n games are there -> {(slot, game_seq): record}; raw: the record's bytes (uint8 array) instead of a dict"""
    out = {}
    for _ in range(rounds):
        eng.run_waves(waves)
        if raw:
            lay = eng.layout
            buf = np.zeros((max(eng.cfg.ring_capacity, 1), lay.record_bytes), np.uint8)
            got = C.c_int32()
            eng._ck(eng.L.gaz_engine_drain_finished(eng.h, buf.ctypes.data, buf.shape[0], C.byref(got)))
            for i in range(got.value):
                hdr = buf[i, lay.off_hdr:lay.off_hdr + 16].view(np.int32)
                out[(int(hdr[2]), int(hdr[3]))] = buf[i].copy()
        else:
            for r in eng.drain_finished():
                out[(r["slot"], r["game_seq"])] = r
        if len(out) >= n:
            assert len(out) == n, (len(out), n)
            return out
    raise AssertionError(f"only {len(out)} of {n} games finished")


def first_games(eng, n_slots, waves=32, rounds=40000, samples=False, advance=None):
    """a free-running engine until every slot's first game (game_seq = first_game_seq) is there -> {slot: record}, or with `samples`
    {slot: (games row, boards, policies, values)} through drain_samples.  advance: what a round does in place of eng.run_waves(waves)"""
    first, seq0 = {}, int(eng.cfg.first_game_seq)
    for _ in range(rounds):
        advance() if advance else eng.run_waves(waves)
        if samples:
            b = eng.drain_samples()
            check_batch(b)
            for i in range(b.n):
                if int(b.games[i, 3]) == seq0:
                    bb, pp, vv, length, n_pos, w = b.game(i)
                    assert length == n_pos == int(b.games[i, 0]) and w == int(b.games[i, 1])
                    first[int(b.games[i, 2])] = (b.games[i].copy(), bb.copy(), pp.copy(), vv.copy())
        else:
            for r in eng.drain_finished():
                if r["game_seq"] == seq0:
                    first[r["slot"]] = r
        if len(first) == n_slots:
            return first
    raise AssertionError(f"only {len(first)} of {n_slots} games finished")


def check_batch(batch):
    """row accounting of one SampleBatch: rows contiguous in the order of `games`, every game T - games[:, 5] of them"""
    kept = batch.games[:, 0] - batch.games[:, 5]
    assert (batch.games[:, 5] >= 0).all() and (kept >= 1).all() if batch.n else True
    assert batch.boards.shape[1] == batch.policies.shape[1] == batch.values.shape[0] == int(kept.sum())
    row = int(batch.games[0, 4]) if batch.n else 0
    for i in range(batch.n):
        assert int(batch.games[i, 4]) == row
        row += int(kept[i])


def assert_records_equal(a, b, what, keys=RECORD_KEYS):
    assert (a["T"], a["winner"], a["slot"], a["game_seq"]) == (b["T"], b["winner"], b["slot"], b["game_seq"]), what
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what} {k}")


# ------------------------------------------------------------------------------------------------ refusals, run_self_play
def refusal_message(call, what):
    """call() must be refused with an EngineError -> its message"""
    from grok_alpha_zero_amd.engine import EngineError
    try:
        call()
    except EngineError as e:
        return str(e)
    raise AssertionError(what)


def self_play_file(tmp, key, game, train, games, **kw):
    """one generation of run_self_play with the train_config `train` into tmp/key/0 -> the replay file's datasets"""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import ReplayStore, run_self_play
    from samples_util import file_contents
    folder = os.path.join(str(tmp), key, "0")
    store = ReplayStore(folder); store.create()
    assert run_self_play(GAMES[game], ({}, train), folder, **kw) == games
    return file_contents(store)


def games_of_file(f, games, n_aug):
    """the games of a replay file as a sorted list (the order in which games reach the file is scheduling): a game = its augmentation
    triples, 3 n_aug consecutive datasets"""
    return sorted(tuple((a.dtype.str, a.shape, a.tobytes()) for a in [f[f"{kind}_{n_aug * k + j}"] for j in range(n_aug) for kind in ("boards", "policies", "values")])
                  for k in range(games))


# ------------------------------------------------------------------------------------------------ the 1-block Connect4 network (HIP build)
def c4_one_block_weights():
    from grok_alpha_zero_amd.net import Connect4Net
    return Connect4Net(1, seed=0).eval().export_engine_weights()


def net_engine(G, weights, fused=True, **kw):
    """G Connect4 games, one game each, 40 iterations a move, evaluated by the network `weights`; kw: the seed and the feature's keywords"""
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
    eng = SelfPlayEngine("Connect4", G, 40, 42, 4, 4, 2.5, 0.5, evaluator=EVAL_RESNET, net_blocks=1, ring_capacity=4 * G, games_budget=G, **kw)
    eng.load_weights(weights)
    if not fused:
        eng.set_fused_wave(False)
    return eng


def scheduling_equalities(which, G, engine_kw, collect, witness, keys=None):
    """The records of G Connect4 games with the 1-block network and a feature on (engine_kw) do not depend on the fused launch
    (which = "fused"), the game groups ("groups") or the evaluation cache ("cache"): a pair of engines that differ in that alone, and the
    pair really differed in it.  collect(eng) -> (records, the statistics of the feature that must be equal too, or None).  keys = None:
    the records are play(raw=True)'s and equal byte for byte; else first_games' and equal in `keys`.  At the end witness(records,
    statistics) of the first engine asserts that the feature really acted."""
    w = c4_one_block_weights()

    def run(fused=True, **kw):
        eng = net_engine(G, w, fused, **engine_kw, **kw)
        recs, feature = collect(eng)
        st = eng.stats()
        eng.close()
        return recs, feature, st
    if which == "fused":
        (a, fa, sa), (b, fb, sb) = run(game_groups=1), run(fused=False, game_groups=1)
        assert sa["fused_wave"] == 1 and sb["fused_wave"] == 0, (sa, sb)
    elif which == "groups":
        (a, fa, sa), (b, fb, sb) = run(game_groups=2), run(game_groups=1)
        assert sa["game_groups"] == 2 and sb["game_groups"] == 1
    else:
        (a, fa, sa), (b, fb, sb) = run(game_groups=1, eval_cache_log2=14), run(game_groups=1)
        assert sa["cache_hits"] > 0 and sb["cache_hits"] == 0
    assert sorted(a) == sorted(b) == ([(s, 0) for s in range(G)] if keys is None else list(range(G)))
    for k in a:
        if keys is None:
            assert np.array_equal(a[k], b[k]), (which, k)
        else:
            assert_records_equal(a[k], b[k], f"{which} slot {k}", keys=keys)
    assert fa == fb, (fa, fb)
    witness(a, fa)
    print(f"scheduling {which}: {G} games identical, {fa}", flush=True)

"""The cases of the held-out loss (SelfPlayEngine.score_outputs / score_replay, replay.score_network, Run(replay=dict(score=...)); the "HELD-OUT
LOSS" section of include/gaz_engine.h) that the CPU suite runs on the emulation build (tests/test_score_emu.py) and the
-m gpu suite on the HIP build (tests/test_score_gpu.py): `lib_path` = the emulation library, or None for the product library.

What the engine must return is computed by tests/score_model.py from the rows the case itself made.  Every comparison is on raw bits with 0
mismatches, and every case asserts its witnesses: that the rows it scored really held the edge it is about."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

import replay_cases as RC
import score_model as M
from oracle import gaz_oracle as O
from selfplay_support import A_OF, EMU_DIR, MAXT, ROOT, play

GAMES3 = ("TicTacToe", "Connect4", "Gomoku")
SIZES = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)      # partial teams, partial waves, partial blocks of 128, a second block
REPLAY_SIZES = (0, 1, 2, 127, 128, 129, 300)
SALT = 6
KEYS = ("policy_mode", "rows", "bad_rows", "good", "top1_rows", "value_rows", "value_sign_rows", "ce_sum", "entropy_sum", "se_sum", "policy_loss", "policy_entropy",
        "policy_kl", "value_loss", "top1", "value_sign", "val_loss")
HAND = dict(clip=0, zero=1, one_hot=2, tied=3, tied_late=4, z0=5, opposite=6, p_nan=7, p_inf=8, v_nan=9, v_inf=10, span=11, agree=12)


def engine(game, n_games, lib_path, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(game, n_games, 8, MAXT[game], 0, 0, 2.5, 0.5, **dict(dict(seed=1, hash_salt=SALT, ring_capacity=0, lib_path=lib_path), **kw))


def targets(rng, n, A):
    """valid policy rows (zeros among them, sum 1 up to rounding) and values in {-1, 0, 1}"""
    y = rng.random((n, A), dtype=np.float32)
    y[rng.random((n, A)) < 0.4] = 0
    y[np.arange(n), rng.integers(0, A, n)] += np.float32(0.5)
    y = (y / y.sum(1, keepdims=True)).astype(np.float32)
    return y, rng.integers(-1, 2, n).astype(np.float32)


# ------------------------------------------------------------------------------------------------ rows with an edge each
def hand_rows(A, mode):
    """the rows of HAND for a head of A actions under `mode` -> P f32 [13, A], v, y, z"""
    logits = mode in (1, 3)
    n = len(HAND)
    P = np.full((n, A), 0.25 if not logits else 0.5, np.float32)
    y = np.zeros((n, A), np.float32); y[:, 0] = 0.5; y[:, 1] = 0.25; y[:, 2] = 0.25
    v = np.full(n, 0.5, np.float32); z = np.ones(n, np.float32)
    # clip: q_1 < 1e-7 under y_1 > 0 (a probability of 1e-9; a softmax logit 160 below the largest; a Stablemax logit of -1e9)
    P[HAND["clip"], :3] = [0.5, 1e-9, 0.25] if not logits else ([80.0, -80.0, 0.0] if mode == 1 else [80.0, -1e9, 0.0])
    P[HAND["zero"], 1] = 0.0                                            # P_a == 0 under y_a > 0
    y[HAND["one_hot"]] = 0; y[HAND["one_hot"], A - 1] = 1.0
    y[HAND["tied"]] = np.float32(1.0 / A)                               # uniform y, tied P: both argmaxes are action 0
    y[HAND["tied_late"]] = np.float32(1.0 / A); P[HAND["tied_late"], [2, 5]] += np.float32(1.0)      # P's first largest is action 2, y's is 0
    z[HAND["z0"]] = 0.0
    v[HAND["opposite"]] = -0.25
    P[HAND["p_nan"], A - 1] = np.nan; P[HAND["p_inf"], 0] = -np.inf
    v[HAND["v_nan"]] = np.nan; v[HAND["v_inf"]] = np.inf
    P[HAND["span"], :3] = [80.0, -80.0, 3.0]; y[HAND["span"]] = 0; y[HAND["span"], :3] = [0.25, 0.5, 0.25]
    P[HAND["agree"], 0] += np.float32(0.125)                            # argmax 0 on both sides
    return P, v, y, z


def assert_witnesses(P, v, y, z, mode, ce, ent, se, fl):
    """the edges of hand_rows, read off per-row results (the model's, or the engine's)"""
    H = HAND
    q = M.probabilities(P[H["clip"]], mode)
    assert q[1] < M.EPS and y[H["clip"], 1] > 0, "clip"
    floor = -float(y[H["clip"], 1]) * O.det_log(M.EPS)
    assert ce[H["clip"]] > floor > 3.9, ("clip: the clipped entry alone", ce[H["clip"]], floor)
    assert P[H["zero"], 1] == 0 and y[H["zero"], 1] > 0 and np.isfinite(ce[H["zero"]])
    assert (y[H["one_hot"]] > 0).sum() == 1 and M.bits(ent[H["one_hot"]])[0] == M.bits(-0.0)[0], "one-hot: the entropy is -(+0 + 1 * log 1)"
    assert fl[H["tied"]] & M.TOP1 and not fl[H["tied_late"]] & M.TOP1 and fl[H["agree"]] & M.TOP1, "lowest-index argmax"
    assert fl[H["z0"]] & (M.VSIGN | M.VROW) == 0 and se[H["z0"]] == 0.25
    assert fl[H["opposite"]] & (M.VSIGN | M.VROW) == M.VROW and fl[H["agree"]] & (M.VSIGN | M.VROW) == (M.VSIGN | M.VROW)
    for k in ("p_nan", "p_inf", "v_nan", "v_inf"):
        assert fl[H[k]] == M.BAD and M.bits([ce[H[k]], ent[H[k]], se[H[k]]]).tolist() == [0, 0, 0], k
    assert all(fl[H[k]] & M.BAD == 0 for k in H if k not in ("p_nan", "p_inf", "v_nan", "v_inf"))
    if mode == 1:
        e = O.det_exp(-160.0) / 1.0
        assert 0 < e < 1e-60 and M.probabilities(P[H["span"]], 1)[1] < M.EPS, "logits spanning +-80: dexp underflows to the clip"


_BASE = {}


def base_rows(game, mode):
    """257 rows of `game` under `mode` — hand_rows, then random ones — and the model's per-row results, computed once"""
    if (game, mode) not in _BASE:
        A = A_OF[game]
        rng = np.random.default_rng(100 + 10 * GAMES3.index(game) + mode)
        n = SIZES[-1] - len(HAND)
        y, z = targets(rng, n, A)
        P = rng.random((n, A), dtype=np.float32)
        if mode in (1, 3):
            P = ((P - np.float32(0.5)) * np.float32(24.0)).astype(np.float32)
        v = (rng.random(n, dtype=np.float32) * 2 - 1).astype(np.float32)
        v[::17] = 0.0
        hP, hv, hy, hz = hand_rows(A, mode)
        P, v, y, z = np.concatenate([hP, P]), np.concatenate([hv, v]), np.concatenate([hy, y]), np.concatenate([hz, z])
        res = M.score_rows(P, v, y, z, mode)
        for a in (P, v, y, z) + res:
            a.setflags(write=False)
        _BASE[(game, mode)] = (P, v, y, z, res)
    return _BASE[(game, mode)]


def model_witness_case(game):
    """CPU only: the model alone produces the witnesses from the inputs"""
    for mode in range(4):
        P, v, y, z, (ce, ent, se, fl) = base_rows(game, mode)
        assert_witnesses(P, v, y, z, mode, ce, ent, se, fl)
        n = len(HAND)
        t = M.totals(ce[:n], ent[:n], se[:n], fl[:n], mode)
        assert t["bad_rows"] == 4 and t["good"] == n - 4 and t["value_rows"] == n - 5 and t["value_sign_rows"] == n - 6
    x = np.random.default_rng(0).random(225)
    assert O.np_sum_f64(x) == float(np.sum(x)) and O.np_sum_f64(x[:7]) == float(np.sum(x[:7]))      # the oracle's sum is numpy's, past one block of 128 too


def want_of(res, n, mode):
    ce, ent, se, fl = (a[:n] for a in res)
    return dict(M.totals(ce, ent, se, fl, mode), row_ce=ce, row_entropy=ent, row_se=se, row_flags=fl)


def outputs_case(game, lib_path, grouped=False):
    """score_outputs of the first n of base_rows for every n of SIZES under all four modes, the engine's own mode, a batch that is all bad"""
    eng = engine(game, 4, lib_path, **(dict(game_groups=2) if grouped else {}))
    seen = 0
    for mode in range(4):
        P, v, y, z, res = base_rows(game, mode)
        for n in SIZES:
            got = eng.score_outputs(P[:n], v[:n], y[:n], z[:n], policy_mode=mode, per_row=True)
            bad = M.mismatches(got, want_of(res, n, mode))
            assert bad == 0, (game, mode, n, bad)
            assert M.mismatches(eng.score_outputs(P[:n], v[:n], y[:n], z[:n], policy_mode=mode), {k: got[k] for k in KEYS}) == 0      # per-row outputs may be NULL
            seen += 1
        got = eng.score_outputs(P, v, y, z, policy_mode=mode, per_row=True)
        assert_witnesses(P, v, y, z, mode, got["row_ce"], got["row_entropy"], got["row_se"], got["row_flags"])
        assert got["rows"] == 257 and got["bad_rows"] == 4 and 0 < got["top1_rows"] < 253 and 0 < got["value_sign_rows"] < got["value_rows"] < 253
        ab = np.array([HAND["p_nan"], HAND["v_inf"], HAND["p_inf"], HAND["v_nan"], HAND["p_nan"]])
        got = eng.score_outputs(P[ab], v[ab], y[ab], z[ab], policy_mode=mode, per_row=True)
        want = M.totals(*(a[ab] for a in res), mode)
        assert M.mismatches(got, want) == 0 and got["bad_rows"] == 5 and got["good"] == 0 and np.isnan(got["val_loss"]) and (got["row_flags"] == M.BAD).all()
        zero = eng.score_outputs(P[:0], v[:0], y[:0], z[:0], policy_mode=mode, per_row=True)
        assert zero["rows"] == 0 and M.bits([zero["ce_sum"], zero["entropy_sum"], zero["se_sum"]]).tolist() == [0, 0, 0]
    P, v, y, z, res = base_rows(game, 0)
    assert M.mismatches(eng.score_outputs(P, v, y, z), M.totals(*res, 0)) == 0           # the engine's own head: probabilities
    eng.close()
    return seen


def own_mode_case(lib_path, game="Connect4"):
    """policy_mode None follows the engine's head: softmax probabilities, logits + softmax, logits + Stablemax, Stablemax probabilities"""
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL
    for kw, mode in ((dict(), 0), (dict(policy_is_logits=1, search=SEARCH_GUMBEL, gumbel_m=4), 1),
                     (dict(policy_is_logits=1, search=SEARCH_GUMBEL, gumbel_m=4, gumbel_stablemax=True), 3), (dict(policy_is_logits=2), 2)):
        eng = engine(game, 4, lib_path, **kw)
        P, v, y, z, res = base_rows(game, mode)
        got = eng.score_outputs(P[:65], v[:65], y[:65], z[:65])
        assert got["policy_mode"] == mode and M.mismatches(got, M.totals(*(a[:65] for a in res), mode)) == 0, (kw, got["policy_mode"])
        eng.close()


# ------------------------------------------------------------------------------------------------ score_replay
def fill(w, rng, game, M_rows, stones=False):
    """M_rows random rows as generation 0; stones: boards of -1 / 0 / 1 (what a network is fed) instead of any int8"""
    if M_rows:
        g, b, p, v = RC.random_rows(rng, game, RC.lengths_summing_to(rng, M_rows))
        y, z = targets(rng, M_rows, A_OF[game])
        w.append_arrays(0, g, rng.integers(-1, 2, b.shape).astype(np.int8) if stones else b, y, z)


def hash_predictions(boards, A, salt):
    """oracle.hash_eval_np of every board; Gomoku's 226 hashes of 450 bytes go through the oracle's C twin, checked against it on the first rows"""
    n = boards.shape[0]
    P, v = np.zeros((n, A), np.float32), np.zeros(n, np.float32)
    for i in range(n):
        P[i], v[i] = O.hash_eval(boards[i], A, salt) if (A > 9 and i >= 2) else O.hash_eval_np(boards[i], A, salt)
        if A > 9 and i < 2:
            p2, v2 = O.hash_eval(boards[i], A, salt)
            assert p2.tobytes() == P[i].tobytes() and np.float32(v2) == v[i]
    return P, v


def model_of_plan(w, M_rows, augment, mode, predict):
    """the model's result for the window's current plan: predict(boards) of window.batch(..., with_index=True)"""
    b, y, z, r, s = w.batch(0, M_rows, augment, with_index=True)
    P, v = predict(b)
    res = M.score_rows(P, v, y, z, mode)
    return want_of(res, M_rows, mode), (b, r, s)


def replay_case(game, lib_path, sizes=REPLAY_SIZES, batches=(1, 3, 7, 64, None)):
    """score_replay with the hash evaluator on plans of M rows: per-row arrays, totals and means against the model, augment off and on, the
    totals the same bits for every batch_rows, and twice the same"""
    rng = np.random.default_rng(40 + GAMES3.index(game))
    A = A_OF[game]
    eng = engine(game, max(max(sizes), 64), lib_path, nodes_per_tree=64)           # (it never plays: a small arena)
    seen = dict(plans=0, symmetries=0)
    for M_rows in sizes:
        w = RC.window(game, M_rows + 5, lib_path, seed=12)
        fill(w, rng, game, M_rows)
        assert w.begin_epoch("train", epoch=1, percent=1.0, decay=0.0) == M_rows
        for augment in (False, True):
            want, (_, _, sym) = model_of_plan(w, M_rows, augment, 0, lambda b: hash_predictions(b, A, SALT))
            seen["symmetries"] += int((sym != 0).sum())
            assert augment or not sym.any()
            first = None
            for br in batches:
                br = M_rows if br is None else br
                if br < 1:
                    continue
                got = eng.score_replay(w, batch_rows=br, augment=augment, per_row=True)
                assert M.mismatches(got, want) == 0, (game, M_rows, augment, br, M.mismatches(got, want))
                first = first or got
                assert M.mismatches(got, {k: first[k] for k in KEYS}) == 0
            if M_rows == 0:
                got = eng.score_replay(w, batch_rows=3, augment=augment, per_row=True)
                assert M.mismatches(got, want) == 0 and got["rows"] == 0 and np.isnan(got["val_loss"])
            again = eng.score_replay(w, batch_rows=7, augment=augment, per_row=True)
            assert M.mismatches(again, want) == 0
            seen["plans"] += 1
        if M_rows:
            assert w.begin_epoch("train", epoch=1, percent=0.0) == 0                      # an empty plan of a window that has rows
            assert eng.score_replay(w, batch_rows=4)["rows"] == 0
        w.close()
    eng.close()
    assert seen["symmetries"] > 0
    return seen


def split_case(game, lib_path):
    """the test split and the train split of one window"""
    rng = np.random.default_rng(7)
    A = A_OF[game]
    w = RC.window(game, 400, lib_path, seed=3, test_fraction=0.3)
    fill(w, rng, game, 300)
    eng = engine(game, 64, lib_path, nodes_per_tree=64)
    rows = {}
    for split in ("train", "test"):
        rows[split] = w.begin_epoch(split, epoch=2, percent=1.0, decay=0.0)
        want, _ = model_of_plan(w, rows[split], True, 0, lambda b: hash_predictions(b, A, SALT))
        got = eng.score_replay(w, batch_rows=64, augment=True, per_row=True)
        assert M.mismatches(got, want) == 0 and got["rows"] == rows[split], (split, M.mismatches(got, want))
    assert rows["train"] + rows["test"] == 300 and 40 < rows["test"] < 150, rows
    eng.close(); w.close()
    return rows


def untouched_case(lib_path, game="TicTacToe", G=8):
    """scoring on a running self-play engine leaves its games alone: the records equal those of an engine that never scored"""
    rng = np.random.default_rng(9)
    w = RC.window(game, 64, lib_path, seed=2)
    fill(w, rng, game, 40)
    assert w.begin_epoch() == 40
    recs = {}
    for scored in (True, False):
        eng = engine(game, G, lib_path, ring_capacity=4 * G, games_budget=G, seed=33)
        eng.run_waves(5)
        if scored:
            a = eng.score_replay(w, batch_rows=G)
            eng.run_waves(3)
            b = eng.score_replay(w, batch_rows=3, augment=True)
            assert a["rows"] == b["rows"] == 40 and a["ce_sum"] != b["ce_sum"]
        recs[scored] = play(eng, G, raw=True)
        eng.close()
    w.close()
    assert sorted(recs[True]) == sorted(recs[False]) and all(np.array_equal(recs[True][k], recs[False][k]) for k in recs[True])
    return len(recs[True])


# ------------------------------------------------------------------------------------------------ the engine's own rows; Run
def drained_case(tmp, lib_path):
    """the rows run_self_play(replay=window) drained, scored by replay.score_network with the hash evaluator"""
    from grok_alpha_zero_amd import replay as R
    from grok_alpha_zero_amd.self_play import ReplayStore, run_self_play
    cls = RC.game_class("TicTacToe")
    w = RC.window("TicTacToe", 4096, lib_path, seed=3, test_fraction=0.25, target_ratio=0.5)
    folder = os.path.join(str(tmp), "drained", "0")
    ReplayStore(folder).create()
    assert run_self_play(cls, ({}, RC.TRAIN), folder, n_games=8, seed=9, hash_salt=4, lib_path=lib_path, replay=w) == 12
    out = {}
    for split in ("test", "train"):
        got = R.score_network(w, cls, ({}, RC.TRAIN), None, split=split, batch_rows=16, lib_path=lib_path, hash_salt=4)
        Mr = w.begin_epoch(split, 0, percent=1.0, decay=0.0)
        want, _ = model_of_plan(w, Mr, False, 0, lambda b: hash_predictions(b, 9, 4))
        assert got["rows"] == Mr > 0 and M.mismatches(got, {k: want[k] for k in KEYS}) == 0, (split, got)
        assert 0 < got["value_rows"] <= Mr and got["bad_rows"] == 0 and np.isfinite(got["val_loss"]), got
        out[split] = Mr
    w.close()
    return out


def run_case(tmp, lib_path):
    """Run(replay=dict(score=...)) writes Score.json equal to the model's result and the generation's statistics; without `score` none"""
    from grok_alpha_zero_amd.orchestrator import Run
    cls = RC.game_class("TicTacToe")
    spec = dict(capacity_rows=4096, generations=2, test_fraction=0.2, target_ratio=None, seed=5)
    lines = []
    kw = dict(train_fn=lambda *a, **k: None, n_games=8, seed=20, lib_path=lib_path, out=lambda *a: lines.append(" ".join(str(x) for x in a)),
              self_play_kwargs=dict(hash_salt=4, allow_synthetic=True))
    root = os.path.join(str(tmp), "scored")
    stats = Run(cls, ({}, RC.TRAIN), root=root, replay=dict(spec, score=dict(batch_rows=32)), **kw)
    assert len([ln for ln in lines if ln.startswith("Score: generation")]) == 2
    for g in (0, 1):
        with open(os.path.join(root, str(g + 1), "Score.json")) as f:
            js = json.load(f)
        fresh = RC.window("TicTacToe", 4096, lib_path, seed=5, test_fraction=0.2)
        for k in range(g + 1):
            fresh.append_file(os.path.join(root, str(k)), k)
        Mr = fresh.begin_epoch("test", 0, percent=1.0, decay=0.0)
        want, _ = model_of_plan(fresh, Mr, False, 0, lambda b: hash_predictions(b, 9, 4))
        fresh.close()
        for which in ("new", "current"):
            assert M.mismatches(js[which], {k: want[k] for k in KEYS}) == 0 and js[which]["rows"] == Mr > 0, (g, which, js[which])
            assert M.mismatches(stats[g]["score"][which], {k: want[k] for k in KEYS}) == 0
        assert js["new_folder"] == os.path.join(root, str(g + 1)) and js["current_folder"] == os.path.join(root, str(g)) and js["split"] == "test"
    plain = os.path.join(str(tmp), "plain")
    stats = Run(cls, ({}, RC.TRAIN), root=plain, replay=spec, **kw)
    assert not any(os.path.exists(os.path.join(plain, str(g), "Score.json")) for g in range(4)) and not any("score" in s for s in stats)


# ------------------------------------------------------------------------------------------------ refusals
def refusal_case(lib_path):
    """every refusal by its text; after them the engine scores and the window serves what they did before"""
    from grok_alpha_zero_amd.engine import EVAL_EXTERNAL, EngineError, ScoreTotals
    msgs = {}

    def refused(name, text, call):
        try:
            call()
        except EngineError as e:
            msgs[name] = str(e)
            assert text in str(e), (name, str(e))
            return
        raise AssertionError(f"{name}: accepted")
    rng = np.random.default_rng(1)
    w = RC.window("TicTacToe", 64, lib_path, seed=2)
    fill(w, rng, "TicTacToe", 20)
    eng = engine("TicTacToe", 8, lib_path)
    L = eng.L

    def raw(e, win, batch, t=None):
        t = t or ScoreTotals(struct_size=C.sizeof(ScoreTotals))
        e._ck(L.gaz_engine_score_replay(e.h, win.h if win else None, batch, 0, C.byref(t), None, None, None, None, None))
        return t
    refused("no-plan", "no plan", lambda: raw(eng, w, 4))
    refused("no-plan-python", "no plan", lambda: eng.score_replay(w))
    assert w.begin_epoch() == 20
    before = eng.score_replay(w, batch_rows=8, per_row=True)
    plan = w.plan().tobytes()
    refused("struct-size", "gaz_score_totals.struct_size is 8", lambda: raw(eng, w, 4, ScoreTotals(struct_size=8)))
    t8 = ScoreTotals(struct_size=8)
    refused("struct-size-outputs", "gaz_score_totals.struct_size is 8", lambda: eng._ck(L.gaz_engine_score_outputs(eng.h, None, None, None, None, 0, 0, C.byref(t8), None, None, None, None)))
    refused("batch-rows-0", "batch_rows must be in [1, 8]", lambda: eng.score_replay(w, batch_rows=0))
    refused("batch-rows-9", "batch_rows must be in [1, 8]", lambda: eng.score_replay(w, batch_rows=9))
    refused("null-window", "null window", lambda: raw(eng, None, 4))
    w4 = RC.window("Connect4", 8, lib_path)
    assert w4.begin_epoch() == 0
    refused("other-game", "the window holds rows of game 1, this engine plays game 0", lambda: eng.score_replay(w4, batch_rows=4))
    w4.close()
    eng._ck(L.gaz_engine_wave_begin(eng.h))
    refused("in-a-wave", "between wave_begin and wave_end", lambda: eng.score_replay(w, batch_rows=4))
    eng._ck(L.gaz_engine_wave_end(eng.h))
    refused("mode", "policy_mode must be -1", lambda: eng.score_outputs(np.zeros((1, 9)), [0], np.zeros((1, 9)), [0], policy_mode=4))
    ext = engine("TicTacToe", 8, lib_path, evaluator=EVAL_EXTERNAL)
    refused("external", "no built-in evaluator", lambda: ext.score_replay(w, batch_rows=4))
    assert ext.score_outputs(np.full((2, 9), 0.1), [0, 0], np.full((2, 9), 0.1), [1, 0])["rows"] == 2          # needs no evaluator
    ext.close()
    grp = engine("TicTacToe", 8, lib_path, game_groups=2)
    refused("game-groups", "needs game_groups = 1", lambda: grp.score_replay(w, batch_rows=4))
    grp.close()
    if lib_path is not None:                                               # (the emulation build has every device; the HIP build would need a second card)
        wd = type(w)("TicTacToe", 8, 1, device=1, lib_path=lib_path)
        assert wd.begin_epoch() == 0
        refused("other-device", "the window is on device 1, this engine on device 0", lambda: eng.score_replay(wd, batch_rows=4))
        wd.close()
    after = eng.score_replay(w, batch_rows=8, per_row=True)
    assert M.mismatches(after, {k: v for k, v in before.items() if k != "ms"}) == 0 and w.plan().tobytes() == plan and w.info()["plan_rows"] == 20
    eng.close(); w.close()
    return msgs


# ------------------------------------------------------------------------------------------------ the network (HIP build)
def net_case(mode_kw=None, want_mode=0, sizes=(1, 3, 129, 257), batches=(1, 3, 64, 65)):
    """score_replay with the 1-block Connect4 network: the model is fed engine.evaluate() of the same boards, so the comparison is exact; the
    totals are the same bits for every batch_rows; weights not loaded is refused.  mode_kw: a logits head (policy_is_logits = 1), softmax or Stablemax"""
    from grok_alpha_zero_amd.engine import EVAL_RESNET, EngineError, SelfPlayEngine
    from selfplay_support import c4_one_block_weights
    rng = np.random.default_rng(21)
    eng = SelfPlayEngine("Connect4", 65, 40, 42, 4, 4, 2.5, 0.5, seed=1, evaluator=EVAL_RESNET, net_blocks=1, ring_capacity=0, game_groups=1, nodes_per_tree=64, **(mode_kw or {}))
    w = RC.window("Connect4", 8, None, seed=5)
    fill(w, rng, "Connect4", 3, stones=True)
    w.begin_epoch()
    try:
        eng.score_replay(w, batch_rows=8)
        raise AssertionError("an engine without weights scored")
    except EngineError as e:
        assert "weights not loaded" in str(e), str(e)
    w.close()
    eng.load_weights(c4_one_block_weights())

    def predict(boards):
        P, v = np.zeros((boards.shape[0], 7), np.float32), np.zeros(boards.shape[0], np.float32)
        for i in range(0, boards.shape[0], 65):
            P[i:i + 65], v[i:i + 65], _ = eng.evaluate(boards[i:i + 65])
        return P, v
    out = {}
    for M_rows in sizes:
        w = RC.window("Connect4", M_rows + 5, None, seed=5)
        fill(w, rng, "Connect4", M_rows, stones=True)
        assert w.begin_epoch("train", epoch=3) == M_rows
        want, _ = model_of_plan(w, M_rows, True, want_mode, predict)
        first = None
        for br in batches:
            got = eng.score_replay(w, batch_rows=br, augment=True, per_row=True)
            assert got["policy_mode"] == want_mode and M.mismatches(got, want) == 0, (M_rows, br, M.mismatches(got, want))
            first = first or got
            assert M.mismatches(got, {k: first[k] for k in KEYS}) == 0
        assert first["bad_rows"] == 0 and np.isfinite(first["val_loss"])
        out[M_rows] = (first["val_loss"], first["top1"], first["ms"])
        w.close()
    eng.close()
    return out


# ------------------------------------------------------------------------------------------------ the sanitizer driver
def build_driver():
    """tests/emu/score_main.cpp with the engine's host code and the one-lane build of its device code as ONE program under the address and
    undefined-behaviour sanitizers, the runtimes linked statically: run directly, on the CPU, never loaded into Python"""
    csrc, out = os.path.join(ROOT, "grok_alpha_zero_amd", "csrc"), os.path.join(EMU_DIR, "score_asan")
    srcs = [os.path.join(csrc, "engine.hip"), os.path.join(EMU_DIR, "emu_stubs.cpp"), os.path.join(EMU_DIR, "score_main.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")] + [os.path.join(ROOT, "include", "gaz_engine.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DGAZ_HOST_EMU", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-x", "c++"] + srcs + ["-o", out])
    return out


def run_driver(driver, game):
    r = subprocess.run([driver, f"game={game}"], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout + r.stderr

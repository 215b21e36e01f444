"""The cases of the search's random evaluation symmetry (gaz_engine_set_eval_symmetry) that the CPU suite runs on
the emulation build (tests/test_eval_symmetry_emu.py) and the -m gpu suite on the HIP build (tests/test_eval_symmetry_gpu.py): `lib_path`
= the emulation library, or None for the product library.

What the tests rest on: with symmetry on, the engine evaluates base(T_k(state)) and uses T_k^-1 of the policy, k a function of (seed,
slot, game_seq, board).  That is an evaluator of its own, eval_symmetry_model.sym_eval, so the oracle and the Python models of the searches
play the engine's games when they are given it.  k, T_k and T_k^-1 are restated in eval_symmetry_model and never read back from the engine
under test, except to compare.  Every comparison is exact.

read_batch_symmetry on rows that are not pending: a row keeps the k of the last request encoded in it (0 if there was none); the tests
look at pending rows only."""
import ctypes as C

import numpy as np

import eval_symmetry_model as M
from selfplay_support import (A_OF, MAXT, c4_one_block_weights, games_of_file, net_engine, play, refusal_message, scheduling_equalities,
                              self_play_file)

SEED, SALT = 11, 5
RECORD_KEYS = ("actions", "policies", "q", "root_N", "root_W", "root_P", "root_visits", "evals")
PH_WAIT_HOST, PH_HALT, PH_IDLE = 5, 8, 9


def hash_base(oracle, game, salt=SALT):
    return lambda s: oracle.hash_eval(s, A_OF[game], salt)


def _gumbel(m):
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL
    return dict(search=SEARCH_GUMBEL, gumbel_m=m, c_visit=50.0, c_scale=1.0, policy_is_logits=True)


# name -> (game, (run_iterations, max_actions, explore_first, explore_second, c_puct_init, dirichlet_alpha), engine keywords, gumbel m or None)
SELFPLAY = {
    "ttt": ("TicTacToe", (24, 9, 3, 3, 1.25, 1.0), {}, None),
    "c4": ("Connect4", (40, 42, 4, 4, 2.5, 0.5), {}, None),
    "gmk": ("Gomoku", (48, 6, 2, 2, 2.5, 0.05), {}, None),            # (48 < the legal moves: every move runs 3 x its legal moves)
    "c4-gumbel": ("Connect4", (32, 42, 0, 0, 0.0, 0.0), None, 7),
    "gmk-gumbel": ("Gomoku", (48, 8, 0, 0, 0.0, 0.0), None, 16),
}


def make_engine(name, G, lib_path, games, on=True, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    game, args, ekw, m = SELFPLAY[name]
    a = dict(seed=SEED, hash_salt=SALT, ring_capacity=2 * games + 8, games_budget=games, lib_path=lib_path, eval_symmetry=on)
    a.update(_gumbel(m) if m else ekw); a.update(kw)
    return SelfPlayEngine(game, G, *args, **a)


def oracle_game(oracle, name, slot, seq, evaluator):
    game, (iters, max_actions, e1, e2, c_init, alpha), _, m = SELFPLAY[name]
    if m:
        return oracle.selfplay_game_gumbel(game, iters, max_actions, m, 50.0, 1.0, SEED, slot, seq, evaluator=evaluator)
    return oracle.selfplay_game(game, iters, max_actions, e1, e2, c_init, alpha, SEED, slot, seq, evaluator=evaluator)


def assert_record(r, o, what):
    assert (r["T"], r["winner"]) == (o["T"], o["winner"]), (what, r["T"], o["T"], r["winner"], o["winner"])
    for k in RECORD_KEYS:
        np.testing.assert_array_equal(np.asarray(r[k]).reshape(np.asarray(o[k]).shape), o[k], err_msg=f"{what} {k}")


# ------------------------------------------------------------------------------------------------ 1. self-play against the oracle
def selfplay_case(oracle, name, G, lib_path, per_slot=2, **kw):
    """the hash evaluator, symmetry on, continuous self-play, `per_slot` games per slot: every game is the oracle's with
    sym_eval(hash_eval); the witnesses of the rule occurred; the symmetry-off engine plays other games"""
    game = SELFPLAY[name][0]
    n = per_slot * G
    on, off = make_engine(name, G, lib_path, n, **kw), make_engine(name, G, lib_path, n, on=False, **kw)
    assert on.eval_symmetry is True and off.eval_symmetry is False
    recs, plain = play(on, n), play(off, n)
    on.close(); off.close()
    assert sorted(recs) == sorted(plain) == sorted((s, q) for s in range(G) for q in range(per_slot))
    log, differ = [], 0
    for (slot, seq), r in sorted(recs.items()):
        o = oracle_game(oracle, name, slot, seq, M.sym_eval(oracle, hash_base(oracle, game), game, SEED, slot, seq, log))
        assert_record(r, o, f"{name} game {(slot, seq)}")
        p = plain[(slot, seq)]
        differ += r["T"] != p["T"] or not np.array_equal(r["root_P"], p["root_P"])
    M.assert_witnesses(game, log, name)
    assert differ > 0, "symmetry on and off play the same games"
    print(f"{name} G={G}: {n} games, {len(log)} requests, k counts {np.bincount([k for k, _ in log], minlength=M.NSYM[game]).tolist()}, {differ} games differ from off", flush=True)
    return recs


# ------------------------------------------------------------------------------------------------ 2. the models, 5b. switching, 6b. read_trees
class Switchable:
    """the model's evaluator with the mode of the engine it mirrors"""

    def __init__(self, oracle, game, seed, log):
        self.on, self.base = True, hash_base(oracle, game)
        self.sym = M.sym_eval(oracle, self.base, game, seed, 0, 0, log)

    def __call__(self, state):
        return self.sym(state) if self.on else self.base(state)


def _drive_move(eng, oracle, game):
    """one MCTS.run of a sync + single-tree engine with the external evaluator, answered with the hash of the row AS THE ENGINE WROTE IT
    (the network's frame) -> per launch the list of (row, batch row, k)"""
    A = A_OF[game]
    eng.start_search()
    launches = []
    for _ in range(100000):
        eng.wave_begin()
        x, pend = eng.read_batch()
        ks = eng.read_batch_symmetry()
        rows = np.flatnonzero(pend)
        launches.append([(int(r), x[r].copy(), int(ks[r])) for r in rows])
        if rows.size == 0 and eng.root_stats()["phase"][0] in (PH_WAIT_HOST, PH_HALT):
            return launches
        pol = np.full((eng.batch_rows, A), np.nan, np.float32); val = np.full(eng.batch_rows, np.nan, np.float32)
        for r in rows:
            pol[r], val[r] = oracle.hash_eval(x[r], A, SALT)
        eng.write_outputs(pol, val)
    raise AssertionError("search did not finish")


MODEL_CASES = {"TicTacToe": (30, [4, 0, 8, 2], 1.25, 1.0), "Connect4": (120, [3, 3, 2, 4, 3], 2.5, 0.5), "Gomoku": (3 * 225 + 40, [112, 113], 2.5, 0.05)}


def model_case(oracle, game, lib_path, K=1, forced_k=0.0, switch_off_at=None, seed=7):
    """a sync single-tree engine (leaf_batch = K, forced playouts k) against forced_playouts_model.ForcedTree with the wrapped evaluator:
    per move the launches (as many, the same rows, every row == T_k(the model's state) with k == the row's byte == the restated draw), root
    N / W / P / visits, and read_trees' root priors by original action.  switch_off_at = i: set_eval_symmetry(0) before move i"""
    from forced_playouts_model import ForcedTree
    from grok_alpha_zero_amd.engine import EVAL_EXTERNAL, SelfPlayEngine
    iters, moves, c_init, alpha = MODEL_CASES[game]
    eng = SelfPlayEngine(game, 1, iters, MAXT[game], 0, 0, c_init, alpha, seed=seed, sync_moves=True, single_tree=True, evaluator=EVAL_EXTERNAL,
                         nodes_per_tree=(len(moves) + 1) * (max(iters, 3 * A_OF[game]) + 4) + 64, compact_trees=-1, max_tree_sims_per_wave=4, tau=0.0,
                         leaf_batch=K, forced_playouts_k=forced_k, eval_symmetry=True, lib_path=lib_path)
    eng.set_position(0, [])
    log = []
    ev = Switchable(oracle, game, seed, log)
    model = ForcedTree(oracle, game, K, seed, c_puct_init=c_init, dirichlet_alpha=alpha, evaluator=ev, max_tree_sims=4, forced_k=forced_k)
    widest = 0
    for i, m in enumerate(list(moves) + [None]):
        if switch_off_at == i:
            eng.set_eval_symmetry(False); ev.on = False
            assert eng.eval_symmetry is False
        got, want = _drive_move(eng, oracle, game), model.run(iters)
        assert len(got) == len(want["launches"]), (game, K, i, len(got), len(want["launches"]))
        for n, (g_l, w_l) in enumerate(zip(got, want["launches"])):
            assert [r for r, _, _ in g_l] == list(range(len(w_l))), (game, K, i, n)
            for (_, row, k), state in zip(g_l, w_l):
                assert k == (M.draw(oracle, game, seed, 0, 0, state[..., -1]) if ev.on else 0), (game, K, i, n, k)
                np.testing.assert_array_equal(row, M.transform(game, state, k), err_msg=f"{game} K {K} move {i} launch {n}")
            widest = max(widest, len(w_l))
        st = eng.root_stats()
        for key in ("N", "W", "P"):
            np.testing.assert_array_equal(st[key][0], want[key], err_msg=f"{game} K {K} move {i} {key}")
        assert int(st["root_visits"][0]) == want["root_visits"]
        tree = eng.read_trees([0])[0]                                  # priors by ORIGINAL action
        e = tree.edges_of(0)
        P = np.zeros(A_OF[game], np.float32); P[e["action"]] = e["P"]
        np.testing.assert_array_equal(P, want["P"], err_msg=f"{game} read_trees move {i}")
        if m is None:
            break
        eng.apply_moves([m]); model.play(m)
    eng.close()
    if switch_off_at is None:
        M.assert_witnesses(game, log, f"model {game} K {K}")
    else:
        assert log, "no request was evaluated under a symmetry before the switch"
    return widest


# ------------------------------------------------------------------------------------------------ 3. gumbel_batch 4 == 1
def gumbel_batch_case(name, G, lib_path):
    """symmetry on: the same records byte for byte, evaluator calls, simulations and plies (the RNG events show in the records: every
    Gumbel draw and every symmetry draw decides them)"""
    a, b = make_engine(name, G, lib_path, 2 * G, gumbel_batch=1), make_engine(name, G, lib_path, 2 * G, gumbel_batch=4)
    assert b.batch_rows == 4 * G
    ra, rb = play(a, 2 * G, raw=True), play(b, 2 * G, raw=True)
    sa, sb = a.stats(), b.stats()
    a.close(); b.close()
    assert sorted(ra) == sorted(rb)
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), (name, k)
    assert (sa["evals"], sa["sims"], sa["plies"]) == (sb["evals"], sb["sims"], sb["plies"]) and sb["waves"] < sa["waves"], (sa, sb)


# ------------------------------------------------------------------------------------------------ 4. lock-step through the external evaluator
def lockstep_case(oracle, game, G, lib_path, iters, max_actions, c_init, alpha, gumbel_m=None, seed=SEED):
    """two sync engines with GAZ_EVAL_EXTERNAL and the same seed, A off and B on.  Per wave and pending row: rowB == T_k(rowA), k (B's
    byte) == the restated draw on rowA's board.  B is answered with the hash of ITS row (not equivariant), A with that policy mapped back
    and the same value: the root statistics of every move are identical to the end of the games"""
    from grok_alpha_zero_amd.engine import EVAL_EXTERNAL, SelfPlayEngine
    A = A_OF[game]
    kw = dict(seed=seed, sync_moves=True, evaluator=EVAL_EXTERNAL, ring_capacity=2 * G, lib_path=lib_path)
    if gumbel_m:
        kw.update(_gumbel(gumbel_m))
    ea = SelfPlayEngine(game, G, iters, max_actions, 2, 2, c_init, alpha, **kw)
    eb = SelfPlayEngine(game, G, iters, max_actions, 2, 2, c_init, alpha, eval_symmetry=True, **kw)
    H, W = ea.H, ea.W
    log, moves = [], 0
    for _ in range(1000000):
        (xa, pa), (xb, pb) = ea.read_batch(), eb.read_batch()
        np.testing.assert_array_equal(pa, pb)
        assert not ea.read_batch_symmetry()[pa != 0].any()
        kb = eb.read_batch_symmetry()
        rows = np.flatnonzero(pa)
        if rows.size:
            pol_a = np.full((G, A), np.nan, np.float32); pol_b = pol_a.copy(); val = np.full(G, np.nan, np.float32)
            for r in rows:
                k = int(kb[r])
                assert k == M.draw(oracle, game, seed, int(r), 0, xa[r][..., -1]), (game, r, k)
                np.testing.assert_array_equal(xb[r], M.transform(game, xa[r], k), err_msg=f"{game} row {r} k {k}")
                log.append((k, xa[r][..., -1].copy()))
                pol_b[r], val[r] = oracle.hash_eval(xb[r], A, SALT)
                pol_a[r] = M.untransform_policy(game, pol_b[r], k, H, W)
            ea.write_outputs(pol_a, val); eb.write_outputs(pol_b, val)
        else:
            sa, sb = ea.root_stats(), eb.root_stats()
            np.testing.assert_array_equal(sa["phase"], sb["phase"])
            if all(p in (PH_WAIT_HOST, PH_HALT) for p in sa["phase"]):
                for key in ("N", "W", "P", "policy", "root_visits", "q", "chosen"):
                    np.testing.assert_array_equal(sa[key], sb[key], err_msg=f"{game} move {moves} {key}")
                if all(p == PH_HALT for p in sa["phase"]):
                    break
                moves += 1
                ea.apply_moves(); eb.apply_moves()                     # (launches the wave that applies the moves: its requests are read next)
                continue
        ea.wave_begin(); eb.wave_begin()
    ra = {r["slot"]: r for r in ea.drain_finished()}
    rb = {r["slot"]: r for r in eb.drain_finished()}
    ea.close(); eb.close()
    assert sorted(ra) == sorted(rb) == list(range(G))
    for s in ra:
        assert_record(rb[s], ra[s], f"lock-step {game} slot {s}")
    M.assert_witnesses(game, log, f"lock-step {game}")
    return moves


# ------------------------------------------------------------------------------------------------ 5a. an equivariant evaluator
def equivariant_case(game, G, lib_path, iters, max_actions, c_init, alpha):
    """the uniform evaluator of tests/degenerate_eval.py (policy 1 / A, value 0: the same under every symmetry): the records with
    symmetry on are those with it off, byte for byte — while rows WERE permuted"""
    import degenerate_eval as D
    from grok_alpha_zero_amd.engine import EVAL_EXTERNAL, SelfPlayEngine
    A = A_OF[game]
    out, permuted = [], 0
    for on in (False, True):
        eng = SelfPlayEngine(game, G, iters, max_actions, 2, 2, c_init, alpha, seed=SEED, evaluator=EVAL_EXTERNAL, ring_capacity=2 * G, games_budget=G,
                             eval_symmetry=on, lib_path=lib_path)
        recs = {}
        lay = eng.layout
        for _ in range(1000000):
            eng.wave_begin()
            x, pend = eng.read_batch()
            if on:
                permuted += int(np.count_nonzero(eng.read_batch_symmetry()[pend != 0]))
            pol, val, _ = D.evaluate_many("uniform", x, A)
            eng.write_outputs(pol, val)
            buf = np.zeros((2 * G, lay.record_bytes), np.uint8); got = C.c_int32()
            eng._ck(eng.L.gaz_engine_drain_finished(eng.h, buf.ctypes.data, buf.shape[0], C.byref(got)))
            for i in range(got.value):
                recs[int(buf[i, lay.off_hdr:lay.off_hdr + 16].view(np.int32)[2])] = buf[i].tobytes()
            if len(recs) == G:
                break
        eng.close()
        out.append(recs)
    assert sorted(out[0]) == sorted(out[1]) == list(range(G)) and permuted > 0
    for s in out[0]:
        assert out[0][s] == out[1][s], (game, s)


# ------------------------------------------------------------------------------------------------ 6. unaffected surfaces
def samples_case(name, G, lib_path):
    """drain_samples on a symmetry engine == record_to_samples of its twin's records: the samples stay in the board's own frame"""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import record_to_samples
    game = SELFPLAY[name][0]
    host, dev = make_engine(name, G, lib_path, 2 * G), make_engine(name, G, lib_path, 2 * G)
    recs = play(host, 2 * G)
    host.close()
    got = {}
    for _ in range(40000):
        dev.run_waves(32)
        b = dev.drain_samples()
        for i in range(b.n):
            bb, pp, vv, _, _, _ = b.game(i)
            got[(int(b.games[i, 2]), int(b.games[i, 3]))] = (bb.copy(), pp.copy(), vv.copy())
        if len(got) == 2 * G:
            break
    dev.close()
    assert sorted(got) == sorted(recs)
    for key, r in recs.items():
        hb, hp, hv, _ = record_to_samples(GAMES[game], r)
        for what, d, h in zip(("boards", "policies", "values"), got[key], (hb, hp, hv)):
            assert d.dtype == h.dtype and d.shape == h.shape, (key, what)
            np.testing.assert_array_equal(d, h, err_msg=f"{name} game {key} {what}")


def run_self_play_case(oracle, tmp, lib_path, games=24, G=12, game="TicTacToe"):
    """run_self_play with train_config["eval_symmetry"]: the file holds the games of a directly created engine with symmetry on — which
    are the oracle's (selfplay_case) — at both settings of device_samples; without the key, other games"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import record_to_samples
    n_aug = M.NSYM[game]
    train = dict(games_per_generation=games, MCTS_iteration_limit=16, max_actions=MAXT[game], num_explore_actions_first=2, num_explore_actions_second=1,
                 c_puct_init=1.25, dirichlet_alpha=1.0, use_gumbel=False)
    files = {}
    for key, extra, ds in (("on-host", dict(eval_symmetry=True), False), ("on-device", dict(eval_symmetry=True), True), ("off", {}, True)):
        f = self_play_file(tmp, key, game, dict(train, **extra), games, n_games=G, seed=SEED, hash_salt=SALT, lib_path=lib_path, device_samples=ds)
        files[key] = games_of_file(f, games, n_aug)
    eng = SelfPlayEngine(game, G, 24, MAXT[game], 2, 1, 1.25, 1.0, seed=SEED, hash_salt=SALT, ring_capacity=4 * games, games_budget=games, eval_symmetry=True,
                         lib_path=lib_path)
    recs = play(eng, games, waves=16)
    eng.close()
    want = []
    for (slot, seq), r in recs.items():
        o = oracle.selfplay_game(game, 24, MAXT[game], 2, 1, 1.25, 1.0, SEED, slot, seq,
                                 evaluator=M.sym_eval(oracle, hash_base(oracle, game), game, SEED, slot, seq))
        assert_record(r, o, f"run_self_play twin {(slot, seq)}")
        b, p, v, _ = record_to_samples(GAMES[game], r)
        want.append(tuple((a.dtype.str, a[j].shape, np.ascontiguousarray(a[j]).tobytes()) for j in range(n_aug) for a in (b, p, v)))
    assert files["on-host"] == files["on-device"] == sorted(want)
    assert files["off"] != files["on-host"]


def mcts_class_case(oracle, game, lib_path, iters, seed=5, salt=SALT):
    """mcts.MCTS(eval_symmetry=True).run == the model's search with the wrapped evaluator (slot 0, game_seq 0)"""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.mcts import MCTS
    from leaf_batch_model import Tree
    g = GAMES[game]()
    m = MCTS(g, None, c_puct_init=2.5, dirichlet_alpha=0.5, tau=0.0, seed=seed, hash_salt=salt, eval_symmetry=True, lib_path=lib_path)
    log = []
    model = Tree(oracle, game, 1, seed, c_puct_init=2.5, dirichlet_alpha=0.5, evaluator=M.sym_eval(oracle, hash_base(oracle, game, salt), game, seed, 0, 0, log))
    for _ in range(3):
        move, rows = m.run(iters)
        want = model.run(iters)
        st = m._eng.root_stats()
        for key in ("N", "W", "P"):
            np.testing.assert_array_equal(st[key][0], want[key], err_msg=f"MCTS {game} {key}")
        assert sum(int(r[4]) for r in rows) == int(want["N"].sum())
        g.do_action(move); m.prune_tree(move); model.play(g.action_to_index(move))
    m.close()
    assert {k for k, _ in log} - {0}, "every request drew the identity"


def mcts_gumbel_class_case(oracle, lib_path):
    """mcts.MCTS_Gumbel(eval_symmetry=True) through a session: the session is shown permuted rows, and the result is that of the plain class
    given a session that permutes, asks and maps back itself (games.symmetry_transform / symmetry_untransform_policy)"""
    from grok_alpha_zero_amd.games import Connect4
    from grok_alpha_zero_amd.mcts import MCTS_Gumbel
    seed = 9

    class Session:
        def __init__(self, wrap):
            self.wrap, self.ks = wrap, []

        def run(self, output_names, input_feed, **kw):
            x = np.asarray(input_feed["inputs"]).astype(np.int8)
            pol, val = [], []
            for s in x:
                k = M.draw(oracle, "Connect4", seed, 0, 0, s[..., -1]) if self.wrap else 0
                self.ks.append(k)
                p, v = oracle.hash_eval(Connect4.symmetry_transform(s, k), 7, SALT)
                pol.append(Connect4.symmetry_untransform_policy(p, k)); val.append(v)
            return np.stack(pol), np.asarray(val, np.float32)
    out = []
    for on in (True, False):
        sess = Session(wrap=not on)
        g = Connect4()
        m = MCTS_Gumbel(g, sess, use_gumbel_noise=True, m=7, c_scale=1.0, seed=seed, eval_symmetry=on, lib_path=lib_path)
        move, rows = m.run(32)
        out.append((int(move), [(int(r[0]), float(r[1]), float(r[3]), int(r[4]), float(r[5])) for r in rows]))
        m.close()
        assert on or any(sess.ks)
    assert out[0] == out[1], out


# ------------------------------------------------------------------------------------------------ 7. refusals
def refusal_case(lib_path):
    """-> the messages, each its own.  A refused call leaves the mode as it was"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine("Connect4", 4, 40, 42, 4, 4, 2.5, 0.5, seed=1, lib_path=lib_path)
    msgs = {}
    try:
        eng.set_eval_symmetry(True)
        for mode in (-1, 2):
            assert eng.L.gaz_engine_set_eval_symmetry(eng.h, mode) != 0
            msgs[mode] = eng.L.gaz_engine_last_error(eng.h).decode()
            assert "mode must be 0" in msgs[mode] and str(mode) in msgs[mode] and eng.eval_symmetry is True
        eng.set_eval_symmetry(False)
        assert eng.eval_symmetry is False
        assert eng.L.gaz_engine_get_eval_symmetry(eng.h, None) != 0
        msgs["get-null"] = eng.L.gaz_engine_last_error(eng.h).decode()
        assert eng.L.gaz_engine_read_batch_symmetry(eng.h, None) != 0
        msgs["read-null"] = eng.L.gaz_engine_last_error(eng.h).decode()
        assert not eng.read_batch_symmetry().any()
    finally:
        eng.close()
    grp = SelfPlayEngine("Connect4", 8, 40, 42, 4, 4, 2.5, 0.5, seed=1, game_groups=2, lib_path=lib_path)
    try:
        assert grp.stats()["game_groups"] == 2
        grp.set_eval_symmetry(True)
        assert grp.eval_symmetry is True
        for fn in (grp.read_batch, grp.read_batch_symmetry):           # refused where read_batch is
            msgs[fn.__name__] = refusal_message(fn, f"{fn.__name__} on a grouped engine was not refused")
            assert "game_groups = 1" in msgs[fn.__name__]
    finally:
        grp.close()
    assert "read_batch_symmetry" in msgs["read_batch_symmetry"]
    assert len(set(msgs.values())) == len(msgs), msgs
    return msgs


def abi_case(lib_path):
    from grok_alpha_zero_amd import engine as E
    L = E.load_library(lib_path)
    assert L.gaz_engine_abi_version() == E.ABI_VERSION == 10 and E.EngineConfig._fields_[-1][0] == "forced_playouts_k"
    assert all(hasattr(L, "gaz_engine_" + f) for f in ("set_eval_symmetry", "get_eval_symmetry", "read_batch_symmetry"))


# ------------------------------------------------------------------------------------------------ 8. scheduling with a 1-block ResNet (HIP build)
def scheduling_case(which, G=64):
    """64 Connect4 games, 1-block network, symmetry on: the records do not depend on the fused launch, the game groups or the evaluation cache"""
    def symmetry_is_on(recs, on):
        assert on is True
    scheduling_equalities(which, G, dict(seed=SEED, eval_symmetry=True), lambda eng: (play(eng, G, raw=True), eng.eval_symmetry), symmetry_is_on)


# ------------------------------------------------------------------------------------------------ 9. the real network (HIP build)
def network_case(oracle, G=64):
    """64 Connect4 games, symmetry on, 1-block network, against the oracle whose evaluator is sym_eval around a second engine's evaluate()
    on single rows (rows of a batch are independent bit for bit, tests/test_evaluator_gpu.py)"""
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
    w = c4_one_block_weights()
    eng = net_engine(G, w, seed=SEED, eval_symmetry=True)
    recs = play(eng, G)
    assert eng.stats()["fused_wave"] == 1
    eng.close()
    probe = SelfPlayEngine("Connect4", 64, 1, 42, 4, 4, 2.5, 0.5, seed=0, evaluator=EVAL_RESNET, net_blocks=1, ring_capacity=0)
    probe.load_weights(w)

    memo = {}                                        # (the games share their openings, and both trees of a game ask about the same positions)

    def base(state):
        key = state.tobytes()
        if key not in memo:
            p, v, _ = probe.evaluate(state[None])
            memo[key] = (p[0].copy(), v[0])
        return memo[key]
    log = []
    for (slot, seq), r in sorted(recs.items()):
        o = oracle.selfplay_game("Connect4", 40, 42, 4, 4, 2.5, 0.5, SEED, slot, seq, evaluator=M.sym_eval(oracle, base, "Connect4", SEED, slot, seq, log))
        assert_record(r, o, f"network game {(slot, seq)}")
    probe.close()
    M.assert_witnesses("Connect4", log, "network")
    print(f"network: {G} games, {len(log)} requests", flush=True)

"""The cases of playout cap randomisation (gaz_engine_config.fast_iterations / full_search_prob; DESIGN.md "Playout cap randomisation")
that the CPU suite runs on the emulation build (tests/test_playout_cap_emu.py) and the -m gpu suite on the HIP build
(tests/test_playout_cap_gpu.py): `lib_path` = the emulation library, or None for the product library.

What a move's limit must be is computed HERE, from oracle.uniform and the first-move rule (kinds_of / base_limits), never read back from
the engine under test; the searches themselves are checked against tests/leaf_batch_model.py (PUCT; anchored to the oracle by
tests/test_leaf_batch_emu.py) and against engines created without the cap (Gumbel, anchors).  Every comparison is exact."""
import numpy as np

from selfplay_support import (A_OF, MAXT, N_AUG, RECORD_KEYS, SEARCH_KEYS, assert_records_equal, check_batch, first_games, games_of_file,
                              refusal_message, scheduling_equalities, self_play_file, slots_for)

P_PLAYOUT_CAP = 5                                  # det::P_PLAYOUT_CAP
SEED = 31                                          # checked on the CPU (test_playout_cap_emu.py): both kinds occur after move 0 in every case below


# ------------------------------------------------------------------------------------------------ what the draws must be
def kinds_of(oracle, seed, slot, seq, T, p, start=0):
    """move_kind of plies [start, T) of the game (slot, seq) searched from ply `start`: 1 full, 2 fast.  The first searched move is
    full; after it a move is full iff u < p, u = the game-level stream's uniform variate keyed by the ply."""
    out = []
    for t in range(start, T):
        full = t == start or oracle.uniform(seed, slot, seq, 2, t, P_PLAYOUT_CAP) < p
        out.append(1 if full else 2)
    return np.array(out, np.uint8)


def base_limits(kinds, R, F):
    return [R if k == 1 else min(F, R) for k in kinds]


# ------------------------------------------------------------------------------------------------ 1. limits per move against the model
# name -> game, R, F, leaf_batch, the fixed moves, c_puct_init, dirichlet_alpha
HASH_CASES = {
    "ttt": ("TicTacToe", 24, 6, 1, [4, 0, 8], 1.25, 1.0),            # F below the legal moves of plies 1 and 2: the 3 x rule on fast moves
    "c4-k1": ("Connect4", 40, 8, 1, [3, 3, 2, 4], 2.5, 0.5), "c4-k4": ("Connect4", 40, 8, 4, [3, 3, 2, 4], 2.5, 0.5),
    "gmk": ("Gomoku", 720, 240, 1, [112], 2.5, 0.05),                # two moves
}
P_HASH = 0.5


def hash_case_kinds(oracle, name, G):
    """{slot: kinds} of the compared (slot, move) pairs of a hash case"""
    _, _, _, _, moves, _, _ = HASH_CASES[name]
    return {s: kinds_of(oracle, SEED, s, 0, len(moves) + 1, P_HASH) for s in slots_for(G)}


def hash_case(oracle, name, G, lib_path):
    """G games at once (sync + single tree, hash evaluator); every game plays the same fixed moves, the RNG streams differ by slot, so the
    games of one launch — of one wavefront — run different limits.  After every move: root N / W / P / root visits of the sampled
    slots == leaf_batch_model.Tree.run(limit of that (slot, ply))."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    from leaf_batch_model import Tree
    game, R, F, K, moves, c_init, alpha = HASH_CASES[name]
    salt = 8
    eng = SelfPlayEngine(game, G, R, MAXT[game], 0, 0, c_init, alpha, seed=SEED, hash_salt=salt, sync_moves=True, single_tree=True,
                         nodes_per_tree=(len(moves) + 1) * (max(R, 3 * A_OF[game]) + 4) + 64, compact_trees=-1, max_tree_sims_per_wave=4, tau=0.0,
                         leaf_batch=K, fast_iterations=F, full_search_prob=P_HASH, lib_path=lib_path)
    kinds = hash_case_kinds(oracle, name, G)
    seen = {int(k[t]) for k in kinds.values() for t in range(1, len(moves) + 1)}
    assert seen == {1, 2}, f"{name}: the compared moves after move 0 are all of one kind {seen}: pick another seed"
    models = {s: Tree(oracle, game, K, SEED, slot=s, c_puct_init=c_init, dirichlet_alpha=alpha, hash_salt=salt, max_tree_sims=4) for s in kinds}
    for t, m in enumerate(list(moves) + [None]):
        eng.start_search(); eng.run_move()
        st = eng.root_stats()
        for s, model in models.items():
            lim = base_limits(kinds[s], R, F)[t]
            w = model.run(lim)
            what = f"{name} slot {s} ply {t} kind {kinds[s][t]} limit {lim}"
            np.testing.assert_array_equal(st["N"][s], w["N"], err_msg=what); np.testing.assert_array_equal(st["W"][s], w["W"], err_msg=what)
            np.testing.assert_array_equal(st["P"][s], w["P"], err_msg=what)
            assert int(st["root_visits"][s]) == w["root_visits"], what
        print(f"{name}: ply {t} ok, limits of the sampled slots {[base_limits(kinds[s], R, F)[t] for s in kinds]}", flush=True)
        if m is None:
            break
        eng.apply_moves([m] * G)
        for model in models.values():
            model.play(m)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2. continuous self-play, two trees
SELFPLAY_CASES = {"ttt": ("TicTacToe", 24, 6, 1.25, 1.0), "c4": ("Connect4", 40, 8, 2.5, 0.5)}


def selfplay_case(oracle, name, G, lib_path, p=0.5):
    """G slots, games_budget = G, continuous self-play with both trees: for the sampled slots move_kind == the draws, and two model
    trees per game, fed the record's actions and the per-ply limits, reproduce root N / W / P, root visits and evaluator calls"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    from leaf_batch_model import Tree
    game, R, F, c_init, alpha = SELFPLAY_CASES[name]
    salt = 6
    eng = SelfPlayEngine(game, G, R, MAXT[game], 3, 3, c_init, alpha, seed=SEED, hash_salt=salt, ring_capacity=4 * G, games_budget=G,
                         fast_iterations=F, full_search_prob=p, lib_path=lib_path)
    first = first_games(eng, G)
    eng.close()
    seen = set()
    for s in slots_for(G):
        r = first[s]
        kinds = kinds_of(oracle, SEED, s, 0, r["T"], p)
        np.testing.assert_array_equal(r["move_kind"], kinds, err_msg=f"{name} slot {s}")
        seen |= {int(k) for k in kinds[1:]}
        lims = base_limits(kinds, R, F)
        trees = [Tree(oracle, game, 1, SEED, slot=s, tree=k, c_puct_init=c_init, dirichlet_alpha=alpha, hash_salt=salt) for k in range(2)]
        for ply, a in enumerate(r["actions"]):
            w = trees[ply % 2].run(lims[ply])
            what = f"{name} slot {s} ply {ply} limit {lims[ply]}"
            np.testing.assert_array_equal(r["root_N"][ply], w["N"], err_msg=what); np.testing.assert_array_equal(r["root_W"][ply], w["W"], err_msg=what)
            np.testing.assert_array_equal(r["root_P"][ply], w["P"], err_msg=what)
            assert r["root_visits"][ply] == w["root_visits"] and r["evals"][ply] == w["evals"], what
            if ply + 1 < r["T"]:
                for t in trees:
                    t.play(a)
    assert seen == {1, 2}, seen
    return first


# ------------------------------------------------------------------------------------------------ 3. anchors
def _c4(G, lib_path, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    return SelfPlayEngine("Connect4", G, 40, 42, 4, 4, 2.5, 0.5, seed=SEED, hash_salt=6, ring_capacity=4 * G, games_budget=G, lib_path=lib_path, **kw)


def anchor_case(G, lib_path):
    """(i) p = 1: the records of an engine created without the cap, move_kind all 1.  (ii) F = R, p = 0.3: the same records except
    move_kind, and the samples lack exactly the rows of kind 2."""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import record_to_samples
    engines = dict(plain=_c4(G, lib_path), p1=_c4(G, lib_path, fast_iterations=8, full_search_prob=1.0),
                   fr=_c4(G, lib_path, fast_iterations=40, full_search_prob=0.3))
    recs = {k: first_games(e, G) for k, e in engines.items()}
    for e in engines.values():
        e.close()
    twin = _c4(G, lib_path, fast_iterations=40, full_search_prob=0.3)
    samples = first_games(twin, G, samples=True)
    twin.close()
    dropped = 0
    for s in range(G):
        a = recs["plain"][s]
        assert_records_equal(recs["p1"][s], a, f"p = 1, slot {s}")
        assert (a["move_kind"] == 1).all() and (recs["p1"][s]["move_kind"] == 1).all()
        b = recs["fr"][s]
        assert_records_equal(b, a, f"F = R, slot {s}")
        assert b["move_kind"][0] == 1 and set(b["move_kind"].tolist()) <= {1, 2}
        keep = b["move_kind"] != 2
        dropped += int((~keep).sum())
        full_b, full_p, full_v, T = record_to_samples(GAMES["Connect4"], a)           # the plain engine's record: every row
        row, sb, sp, sv = samples[s]
        assert int(row[0]) == T == a["T"] and int(row[5]) == int((~keep).sum())
        np.testing.assert_array_equal(sb, full_b[:, keep]); np.testing.assert_array_equal(sp, full_p[:, keep]); np.testing.assert_array_equal(sv, full_v[:, keep])
    assert dropped > 0
    return dropped


# ------------------------------------------------------------------------------------------------ 4. Gumbel
GUMBEL = dict(game="Connect4", R=32, F=8, m=7, p=0.5)


def _gumbel_engine(G, lib_path, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine, SEARCH_GUMBEL
    return SelfPlayEngine(GUMBEL["game"], G, GUMBEL["R"], 42, 0, 0, 0.0, 0.0, seed=SEED, hash_salt=6, ring_capacity=4 * G, search=SEARCH_GUMBEL,
                          gumbel_m=GUMBEL["m"], c_visit=50.0, c_scale=1.0, lib_path=lib_path, **kw)


def gumbel_sync_game(slot, limits, lib_path):
    """one game on a sync Gumbel engine WITHOUT the cap (slot_offset = slot, same seed), the host setting every move's limit:
    set_search_params before the move begins (a move can begin inside the launch that applies the one before it), apply_moves() after"""
    from grok_alpha_zero_amd.engine import PH_HALT
    eng = _gumbel_engine(1, lib_path, slot_offset=slot, sync_moves=True)
    for ply in range(MAXT["Connect4"] + 1):
        eng.run_move()
        if eng.root_stats()["phase"][0] == PH_HALT:
            break
        assert ply < len(limits), f"slot {slot}: the sync game is longer than the continuous one"
        eng.set_search_params(limits[ply + 1] if ply + 1 < len(limits) else GUMBEL["R"])
        eng.apply_moves()
    recs = eng.drain_finished()
    eng.close()
    assert len(recs) == 1
    return recs[0]


def gumbel_case(oracle, G, lib_path, cap=True, slots=None):
    """the continuous engine (with the cap, or without it: the comparator alone) against a one-game sync engine per slot"""
    R, F, p = GUMBEL["R"], GUMBEL["F"], GUMBEL["p"]
    eng = _gumbel_engine(G, lib_path, games_budget=G, **(dict(fast_iterations=F, full_search_prob=p) if cap else {}))
    first = first_games(eng, G)
    eng.close()
    seen = set()
    for s in (slots_for(G) if slots is None else slots):
        r = first[s]
        kinds = kinds_of(oracle, SEED, s, 0, r["T"], p) if cap else np.ones(r["T"], np.uint8)
        np.testing.assert_array_equal(r["move_kind"], kinds, err_msg=f"slot {s}")
        seen |= {int(k) for k in kinds[1:]}
        o = gumbel_sync_game(s, base_limits(kinds, R, F), lib_path)
        assert (r["T"], r["winner"]) == (o["T"], o["winner"]), (s, r["T"], o["T"])
        for k in SEARCH_KEYS:
            np.testing.assert_array_equal(r[k], o[k], err_msg=f"Gumbel cap {cap} slot {s} {k}")
    assert seen == ({1, 2} if cap else {1}), seen
    return first


def gumbel_batch_case(G, lib_path, K=4):
    """gumbel_batch = K with the cap == gumbel_batch = 1 with the cap, every array of every record"""
    recs = {}
    for k in (1, K):
        eng = _gumbel_engine(G, lib_path, games_budget=G, gumbel_batch=k, fast_iterations=GUMBEL["F"], full_search_prob=GUMBEL["p"])
        recs[k] = first_games(eng, G)
        eng.close()
    n_fast = 0
    for s in range(G):
        assert_records_equal(recs[K][s], recs[1][s], f"gumbel_batch {K} slot {s}", keys=RECORD_KEYS + ("move_kind",))
        n_fast += int((recs[1][s]["move_kind"] == 2).sum())
    assert n_fast > 0


# ------------------------------------------------------------------------------------------------ 5. samples
# name -> game, G, R, F, max_actions, search, extra engine arguments
SAMPLE_CASES = {
    "ttt": ("TicTacToe", 64, 24, 6, 9, "puct", {}), "c4": ("Connect4", 64, 40, 8, 42, "puct", {}),
    "gmk": ("Gomoku", 8, 48, 16, 6, "puct", {}),
    "c4-groups": ("Connect4", 128, 40, 8, 42, "puct", dict(game_groups=2)),
    "gmk-long": ("Gomoku", 8, 16, 4, 225, "gumbel", {}),             # GPU: T > 128 from a 110-ply start, the compaction crosses wavefronts
}


def no_five_prefix(n):
    """n legal plies that leave Gomoku running: the stones follow the colouring ((x + 2 y) % 4) // 2 of the board, which has no run
    longer than two in any direction (rows XXOO..., shifted by two from row to row), in raster order, the players alternating"""
    cells = [[y * 15 + x for y in range(15) for x in range(15) if ((x + 2 * y) % 4) // 2 == c] for c in range(2)]
    return [cells[i % 2][i // 2] for i in range(n)]


SAMPLE_PREFIX = {"gmk-long": no_five_prefix(110)}   # hash-evaluator games from the empty board end after 20 to 80 plies


def _sample_engine(name, lib_path, G=None, **kw):
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL, SEARCH_PUCT, SelfPlayEngine
    game, G0, R, F, max_actions, search, extra = SAMPLE_CASES[name]
    G = G or G0
    skw = dict(search=SEARCH_GUMBEL, gumbel_m=4, c_visit=50.0, c_scale=1.0) if search == "gumbel" else dict(search=SEARCH_PUCT)
    args = dict(seed=SEED, hash_salt=6, slot_offset=10, ring_capacity=4 * G, games_budget=G, fast_iterations=F, full_search_prob=0.4, lib_path=lib_path)
    args.update(skw); args.update(extra); args.update(kw)
    return SelfPlayEngine(game, G, R, max_actions, 3, 2, 2.5, 0.5, **args), game, G


def samples_case(name, lib_path, G=None):
    """device path against host path on paired engines; and the kept rows == the rows with move_kind != 2 of record_to_samples on the
    same record with its move_kind forced to 1; games[:, 5] == the count of kind 2"""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import record_to_samples
    host, game, G = _sample_engine(name, lib_path, G)
    dev, _, _ = _sample_engine(name, lib_path, G)
    for g in range(G if name in SAMPLE_PREFIX else 0):
        host.set_position(g, SAMPLE_PREFIX[name]); dev.set_position(g, SAMPLE_PREFIX[name])
    if "game_groups" in SAMPLE_CASES[name][6]:
        assert dev.stats()["game_groups"] == 2
    recs = first_games(host, G)
    got = first_games(dev, G, samples=True)
    host.close(); dev.close()
    assert sorted(recs) == sorted(got) == list(range(10, 10 + G))
    n_fast = 0
    for s, r in recs.items():
        row, db, dp, dv = got[s]
        kind = r["move_kind"]
        keep = kind != 2
        assert (int(row[0]), int(row[1]), int(row[2]), int(row[3]), int(row[5])) == (r["T"], r["winner"], s, r["game_seq"], int((~keep).sum())), (name, s)
        hb, hp, hv, length = record_to_samples(GAMES[game], r)                        # the host definition drops the same rows
        assert length == r["T"]
        forced = dict(r); forced["move_kind"] = np.ones_like(kind)
        fb, fp, fv, _ = record_to_samples(GAMES[game], forced)                        # every row, then filtered here
        assert fb.shape[1] == r["T"] and fb.shape[0] == N_AUG[game]
        for what, d, h, f in (("boards", db, hb, fb), ("policies", dp, hp, fp), ("values", dv, hv, fv)):
            assert d.dtype == h.dtype and d.shape == h.shape, (name, s, what, d.shape, h.shape)
            np.testing.assert_array_equal(d, h, err_msg=f"{name} slot {s} {what} (device vs host)")
            np.testing.assert_array_equal(d, f[:, keep], err_msg=f"{name} slot {s} {what} (kept rows)")
        n_fast += int((~keep).sum())
    assert n_fast > 0
    return recs


def row_accounting_case(lib_path, name="c4"):
    """max_rows counts kept rows: a drain with max_rows strictly between a game's kept rows and its T succeeds, one below its kept rows is the
    'oldest game has more rows than max_rows' error, and nothing is lost by the refused call"""
    from grok_alpha_zero_amd.engine import EngineError
    a, game, _ = _sample_engine(name, lib_path, 1)
    b, _, _ = _sample_engine(name, lib_path, 1)
    r = first_games(a, 1)[10]
    a.close()
    kept = int((r["move_kind"] != 2).sum())
    assert 1 <= kept < r["T"] - 1, "the game has fewer than two fast moves: pick another seed"
    between = kept + 1                                                                # strictly between the kept rows and T
    for _ in range(40000):
        b.run_waves(32); b.synchronize()
        if b.stats()["game_stats"][2] >= 1:
            break
    try:
        b.drain_samples(max_rows=kept - 1)
        raise AssertionError("a drain below the kept rows was not refused")
    except EngineError as e:
        assert f"has {kept} rows" in str(e) and f"max_rows is {kept - 1}" in str(e), str(e)
    batch = b.drain_samples(max_rows=between)
    assert batch.n == 1 and batch.rows == kept and int(batch.games[0, 0]) == r["T"] and int(batch.games[0, 5]) == r["T"] - kept
    check_batch(batch)
    b.close()


# ------------------------------------------------------------------------------------------------ 6. run_self_play
def run_self_play_case(tmp, lib_path, gumbel=False, games=40, G=24):
    """run_self_play with MCTS_fast_iteration_limit / full_search_prob: the same file at both settings of device_samples once the games
    are matched, total rows == the kept rows of an engine created with the scaled limits directly, game_stats count every ply"""
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL, SelfPlayEngine
    train = dict(games_per_generation=games, MCTS_iteration_limit=16, MCTS_fast_iteration_limit=4, full_search_prob=0.4, max_actions=9,
                 num_explore_actions_first=2, num_explore_actions_second=1, c_puct_init=1.25, dirichlet_alpha=1.0, use_gumbel=gumbel, m=4, c_visit=50.0, c_scale=1.0)
    out = {ds: self_play_file(tmp, f"ds{ds}", "TicTacToe", train, games, n_games=G, seed=11, hash_salt=4, lib_path=lib_path, device_samples=ds)
           for ds in (False, True)}
    R, F = (16, 4) if gumbel else (24, 6)                                             # PUCT: int(1.5 x) of both limits
    eng = SelfPlayEngine("TicTacToe", G, R, 9, 2, 1, 1.25, 1.0, seed=11, hash_salt=4, ring_capacity=4 * G, games_budget=games, fast_iterations=F,
                         full_search_prob=0.4, lib_path=lib_path, **(dict(search=SEARCH_GUMBEL, gumbel_m=4) if gumbel else {}))
    recs = []
    for _ in range(40000):
        eng.run_waves(16); recs += eng.drain_finished()
        if len(recs) == games:
            break
    eng.close()
    assert len(recs) == games
    kept = sum(int((r["move_kind"] != 2).sum()) for r in recs)
    plies = sum(r["T"] for r in recs)
    assert kept < plies
    for ds in (False, True):
        f = out[ds]
        assert len(f) == 1 + 3 * 8 * games                                           # three datasets per augmentation and game: every game has a row
        gs = f["game_stats"]
        winners = [r["winner"] for r in recs]
        assert gs[2] == games and gs[1] == plies and gs[0] == max(r["T"] for r in recs), (gs, plies)
        assert [gs[3], gs[4], gs[5]] == [winners.count(-1), winners.count(0), winners.count(1)]
        assert sum(f[f"values_{8 * k}"].shape[0] for k in range(games)) == kept
    np.testing.assert_array_equal(out[False]["game_stats"], out[True]["game_stats"])
    assert games_of_file(out[False], games, 8) == games_of_file(out[True], games, 8)


# ------------------------------------------------------------------------------------------------ 7. refusals
REFUSALS = {   # name -> engine arguments, what the message must say
    "negative": (dict(fast_iterations=-1, full_search_prob=0.5), "fast_iterations must be >= 0"),
    "above-run-iterations": (dict(fast_iterations=41, full_search_prob=0.5), "must not exceed run_iterations"),
    "prob-zero": (dict(fast_iterations=8, full_search_prob=0.0), "full_search_prob must be in (0, 1]"),
    "prob-above-one": (dict(fast_iterations=8, full_search_prob=1.5), "full_search_prob must be in (0, 1]"),
    "prob-negative": (dict(fast_iterations=8, full_search_prob=-0.25), "full_search_prob must be in (0, 1]"),
    "prob-nan": (dict(fast_iterations=8, full_search_prob=float("nan")), "full_search_prob must be in (0, 1]"),
    "prob-without-cap": (dict(fast_iterations=0, full_search_prob=0.5), "full_search_prob must be 0 with fast_iterations = 0"),
    "time-limit": (dict(fast_iterations=8, full_search_prob=0.5, move_time_limit=0.5), "move_time_limit"),
}


def refusal_case(name, lib_path):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    kw, text = REFUSALS[name]
    msg = refusal_message(lambda: SelfPlayEngine("Connect4", 8, 40, 42, 4, 4, 2.5, 0.5, seed=1, lib_path=lib_path, **kw).close(),
                          f"{name}: gaz_engine_create accepted {kw}")
    assert text in msg, (name, msg)
    return msg


def lower_run_iterations_case(oracle, lib_path):
    """lowering run_iterations below fast_iterations later is legal: a fast move then runs min(F, R)"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    from leaf_batch_model import Tree
    G, R, F, lower = 8, 40, 30, 12
    eng = SelfPlayEngine("Connect4", G, R, 42, 0, 0, 2.5, 0.5, seed=SEED, hash_salt=8, sync_moves=True, single_tree=True, tau=0.0,
                         fast_iterations=F, full_search_prob=0.5, lib_path=lib_path)
    models = {s: Tree(oracle, "Connect4", 1, SEED, slot=s, c_puct_init=2.5, dirichlet_alpha=0.5, hash_salt=8) for s in range(G)}
    kinds = {s: kinds_of(oracle, SEED, s, 0, 2, 0.5) for s in range(G)}
    assert {int(k[1]) for k in kinds.values()} == {1, 2}
    for t in range(2):
        if t == 1:
            eng.set_search_params(lower, 0)
        eng.start_search(); eng.run_move()
        st = eng.root_stats()
        for s, model in models.items():
            w = model.run(base_limits(kinds[s], R if t == 0 else lower, F)[t])
            np.testing.assert_array_equal(st["N"][s], w["N"], err_msg=f"slot {s} ply {t}"); np.testing.assert_array_equal(st["W"][s], w["W"])
        eng.apply_moves([3] * G)
        for model in models.values():
            model.play(3)
    eng.close()


# ------------------------------------------------------------------------------------------------ 8. scheduling equalities (HIP build, network)
def scheduling_case(which, G=64):
    """64 Connect4 games with a 1-block network and the cap on: the records do not depend on the fused launch, the game groups or the
    evaluation cache"""
    def some_move_is_fast(recs, _):
        n_fast = sum(int((r["move_kind"] == 2).sum()) for r in recs.values())
        assert n_fast > 0
    scheduling_equalities(which, G, dict(seed=SEED, fast_iterations=8, full_search_prob=0.5), lambda eng: (first_games(eng, G), None), some_move_is_fast,
                          keys=RECORD_KEYS + ("move_kind",))

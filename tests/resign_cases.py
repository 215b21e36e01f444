"""The cases of resignation in self-play (gaz_engine_set_resignation) that the CPU suite runs on the emulation build
(tests/test_resign_emu.py) and the -m gpu suite on the HIP build (tests/test_resign_gpu.py): `lib_path` = the emulation library, or
None for the product library.

What the tests rest on: resignation consumes one RNG event of a purpose of its own and touches no search, so the record of game
(slot, game_seq) with resignation on is a PREFIX of the record from an engine created identically with it off.  What a game must look
like — where it ends, who wins, which plies are marked — is computed HERE (trigger / expectation) from the off engine's q and move_kind
and oracle.uniform(..., tree 2, event 0, purpose 6); it is never read back from the engine under test.  Every comparison is exact."""
import ctypes as C

import numpy as np

from selfplay_support import MAXT, N_AUG, check_batch, games_of_file, play, refusal_message, scheduling_equalities, self_play_file

P_RESIGN = 6                                       # det::P_RESIGN
SEED, SALT, NO_RESIGN_PROB = 31, 6, 0.5
ROW_KEYS = ("actions", "policies", "q", "root_N", "root_W", "root_P", "root_visits", "evals", "move_kind")


# ------------------------------------------------------------------------------------------------ the rule, restated
def trigger(q, kind, p, threshold, consecutive=1, min_ply=0):
    """does the rule trigger after ply p (the caller knows that the game went on)?  q: the record's float32 values; kind: move_kind"""
    if p < min_ply or p < 2 * (consecutive - 1):
        return False
    for i in range(consecutive):
        j = p - 2 * i
        if (int(kind[j]) & 3) == 0 or not (float(q[j]) < -threshold):
            return False
    return True


def is_playout_game(oracle, seed, slot, seq, prob):
    return oracle.uniform(seed, slot, seq, 2, 0, P_RESIGN) < prob


def mover(p):
    return -1 if p % 2 == 0 else 1


def expectation(oracle, off, rule, seed=SEED):
    """what the game of the off record `off` must be with resignation on: dict(T, winner, resign_ply, would, playout, false_positive)"""
    thr, c, m, prob = rule
    trig = [p for p in range(off["T"] - 1) if trigger(off["q"], off["move_kind"], p, thr, c, m)]      # the last ply ended the game itself
    playout = is_playout_game(oracle, seed, off["slot"], off["game_seq"], prob)
    if trig and not playout:
        p = trig[0]
        return dict(T=p + 1, winner=-mover(p), resign_ply=p, would=[], playout=False, false_positive=None)
    return dict(T=off["T"], winner=off["winner"], resign_ply=-1, would=trig if playout else [], playout=playout,
                false_positive=(off["winner"] != -mover(trig[0])) if (playout and trig) else None)


def witnesses(exp):
    """the kinds of game among the expectations -> counts"""
    w = dict(resigned=0, resigned_by_minus1=0, resigned_by_plus1=0, natural=0, quiet_playout=0, would=0, false_positive=0, true_positive=0)
    for e in exp.values():
        if e["resign_ply"] >= 0:
            w["resigned"] += 1
            w["resigned_by_minus1" if mover(e["resign_ply"]) == -1 else "resigned_by_plus1"] += 1
        elif not e["playout"]:
            w["natural"] += 1
        elif not e["would"]:
            w["quiet_playout"] += 1
        else:
            w["would"] += 1
            w["false_positive" if e["false_positive"] else "true_positive"] += 1
    return w


MINIMUM = ("resigned_by_minus1", "resigned_by_plus1", "natural", "quiet_playout", "would")


def expected_stats(exp):
    """gaz_engine_get_resign_stats from the expectations"""
    w = witnesses(exp)
    return dict(resigned=w["resigned_by_minus1"] + w["resigned_by_plus1"], resigned_by_minus1=w["resigned_by_minus1"], resigned_by_plus1=w["resigned_by_plus1"],
                playout_games=sum(e["playout"] for e in exp.values()), would_resign=w["would"], false_positives=w["false_positive"],
                resigned_plies=sum(e["T"] for e in exp.values() if e["resign_ply"] >= 0))


# ------------------------------------------------------------------------------------------------ engines
def _gumbel(m=4):
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL
    return dict(search=SEARCH_GUMBEL, gumbel_m=m, c_visit=50.0, c_scale=1.0, policy_is_logits=True)


def case_table():
    """name -> (game, positional engine arguments after n_games, keyword arguments, (threshold, consecutive, min_ply, no_resign_prob))"""
    c4 = ("Connect4", (40, 42, 4, 4, 2.5, 0.5))
    ttt = ("TicTacToe", (24, 9, 3, 3, 1.25, 1.0))
    rule = (0.3, 2, 0, NO_RESIGN_PROB)
    return {
        "c4": c4 + ({}, rule), "ttt": ttt + ({}, rule), "ttt-min4": ttt + ({}, (0.5, 1, 4, NO_RESIGN_PROB)),
        "c4-gumbel": ("Connect4", (32, 42, 0, 0, 0.0, 0.0), _gumbel(), rule),
        "gmk-gumbel": ("Gomoku", (16, 225, 2, 2, 0.0, 0.05), _gumbel(), (0.1, 1, 2, NO_RESIGN_PROB)),
        "gmk-puct": ("Gomoku", (48, 12, 2, 2, 2.5, 0.05), {}, (0.05, 1, 2, NO_RESIGN_PROB)),
        "c4-leaf4": c4 + (dict(leaf_batch=4), rule), "c4-single": c4 + (dict(single_tree=True, nodes_per_tree=42 * 42 + 64), rule),       # one tree gains the records of both players' moves
        "c4-cap-forced": c4 + (dict(fast_iterations=8, full_search_prob=0.5, forced_playouts_k=2.0), rule),
    }


def make_engine(name, G, lib_path, rule=None, games=None, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    game, args, ekw, _ = case_table()[name]
    games = 2 * G if games is None else games
    a = dict(seed=SEED, hash_salt=SALT, ring_capacity=2 * games + 8, games_budget=games, lib_path=lib_path)
    a.update(ekw); a.update(kw)
    if rule is not None:
        a.update(resign_threshold=rule[0], resign_consecutive=rule[1], resign_min_ply=rule[2], no_resign_prob=rule[3])
    return SelfPlayEngine(game, G, *args, **a)


def assert_prefix(on, off, e, what):
    """the on record against its expectation and against the rows of the off record it must repeat"""
    got = (on["T"], on["winner"], on["resign_ply"], on["resigned"], on["would_resign_plies"].tolist())
    assert got == (e["T"], e["winner"], e["resign_ply"], e["resign_ply"] >= 0, e["would"]), (what, got, e)
    T = e["T"]
    for k in ROW_KEYS:
        assert len(on[k]) == T, (what, k)
        np.testing.assert_array_equal(on[k], off[k][:T], err_msg=f"{what} {k}")
    z = np.array([mover(p) * e["winner"] for p in range(T)], np.float32)
    np.testing.assert_array_equal(on["z"], z, err_msg=what)
    np.testing.assert_array_equal(on["values"], (np.float32(0.5) * (z + off["q"][:T])).astype(np.float32), err_msg=what)


def game_stats_of(recs):
    w = [r["winner"] for r in recs]
    return [max(r["T"] for r in recs), sum(r["T"] for r in recs), len(recs), w.count(-1), w.count(0), w.count(1)]


# ------------------------------------------------------------------------------------------------ 2. + 4. prefix cases and the counters
def prefix_case(oracle, name, G, lib_path, need=MINIMUM, rule=None, on_kw=None, per_slot=2):
    """paired engines, continuous self-play, two games per slot, so that game_seq 1 — the play-out draw keyed by it, the record and the
    (compacted) trees reused after a resigned game — is covered too.  per_slot = 1 is for the Gomoku cases on the one-lane EMULATION only,
    where a 48-iteration Gomoku search takes seconds per game; the HIP build plays two games per slot in every case: every game of the on engine against its expectation and the off engine's
    rows; resign_stats() and game_stats against the expectations; the witnesses in `need` must occur.  -> (off, on, expectations)"""
    rule = rule or case_table()[name][3]
    n = per_slot * G
    a, b = make_engine(name, G, lib_path, games=n), make_engine(name, G, lib_path, rule, games=n, **(on_kw or {}))
    off, on = play(a, n), play(b, n)
    stats, rs = b.stats(), b.resign_stats()
    zero = a.resign_stats()
    a.close(); b.close()
    assert sorted(off) == sorted(on) == sorted((s, q) for s in range(G) for q in range(per_slot))
    assert not any(zero.values()), zero
    exp = {k: expectation(oracle, off[k], rule) for k in off}
    for k in sorted(off):
        assert not off[k]["resigned"] and off[k]["resign_ply"] == -1 and off[k]["would_resign_plies"].size == 0
        assert_prefix(on[k], off[k], exp[k], f"{name} game {k}")
    w = witnesses(exp)
    print(f"{name} G={G} rule {rule}: {w}", flush=True)
    assert all(w[k] > 0 for k in need), (name, G, w)
    assert rs == expected_stats(exp), (rs, expected_stats(exp))
    assert [int(x) for x in stats["game_stats"]] == game_stats_of(list(on.values())), stats
    return off, on, exp


def fast_resign_case(oracle, G, lib_path):
    """the playout cap and forced playouts on: a game must resign after a FAST ply — kind 2 under the 0x10 mark — which then gives no
    sample row"""
    off, on, exp = prefix_case(oracle, "c4-cap-forced", G, lib_path, need=("resigned_by_minus1", "resigned_by_plus1", "natural"))
    fast = [k for k, e in exp.items() if e["resign_ply"] >= 0 and on[k]["move_kind"][e["resign_ply"]] == 2]
    assert fast, "no game resigns after a fast ply: pick another seed"
    return fast


# ------------------------------------------------------------------------------------------------ 3. anchors
def _mask_marks(eng, raw, bits):
    out = raw.copy()
    lay = eng.layout
    out[lay.off_move_kind:lay.off_move_kind + lay.t_pad] &= np.uint8(0xff ^ bits)
    return out


def anchor_case(G, lib_path, name="c4"):
    """(i) min_ply = max_T: the records of the off engine byte for byte, raw move_kind included.  (ii) no_resign_prob = 1: the same except
    for the 0x20 bits, and every game is counted as a play-out game.  (iii) set_resignation(0) on a fresh engine == never calling it."""
    game = case_table()[name][0]
    engines = dict(off=make_engine(name, G, lib_path), late=make_engine(name, G, lib_path, (0.3, 1, MAXT[game], 0.0)),
                   playout=make_engine(name, G, lib_path, (0.3, 1, 0, 1.0)), zero=make_engine(name, G, lib_path))
    engines["zero"].set_resignation(0.0, consecutive=99, min_ply=-5, no_resign_prob=7.0)      # off: the other arguments are not looked at
    raw = {k: play(e, 2 * G, raw=True) for k, e in engines.items()}
    rs = {k: e.resign_stats() for k, e in engines.items()}
    marked = 0
    lay = engines["off"].layout
    for key, r in raw["off"].items():
        assert r.tobytes() == raw["late"][key].tobytes() == raw["zero"][key].tobytes(), key
        p = raw["playout"][key]
        assert _mask_marks(engines["off"], p, 0x20).tobytes() == r.tobytes(), key
        mk = p[lay.off_move_kind:lay.off_move_kind + lay.t_pad]
        assert not (mk & 0x10).any() and not (mk & 0xcc).any()
        marked += int((mk & 0x20).any())
    for e in engines.values():
        e.close()
    assert marked > 0
    assert not any(rs["off"].values()) and not any(rs["late"].values()) and not any(rs["zero"].values()), rs
    assert rs["playout"]["playout_games"] == 2 * G and rs["playout"]["would_resign"] == marked and rs["playout"]["resigned"] == 0, rs
    return marked


# ------------------------------------------------------------------------------------------------ 5. samples
def samples_case(oracle, name, G, lib_path, on_kw=None):
    """drain_samples on a resign engine == record_to_samples of its twin's records (which are themselves checked against the off engine);
    a resigned game — won by the player who did NOT move last — has the values 0.5 (mover * winner + q)"""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import record_to_samples
    game, rule = case_table()[name][0], case_table()[name][3]
    host, dev = make_engine(name, G, lib_path, rule, **(on_kw or {})), make_engine(name, G, lib_path, rule, **(on_kw or {}))
    recs = play(host, 2 * G)
    host.close()
    got = {}
    for _ in range(40000):
        dev.run_waves(32)
        b = dev.drain_samples()
        check_batch(b)
        for i in range(b.n):
            bb, pp, vv, length, n_pos, w = b.game(i)
            assert length == n_pos == int(b.games[i, 0]) and w == int(b.games[i, 1])
            got[(int(b.games[i, 2]), int(b.games[i, 3]))] = (b.games[i].copy(), bb.copy(), pp.copy(), vv.copy())
        if len(got) == 2 * G:
            break
    dev.close()
    assert sorted(got) == sorted(recs)
    n_resigned = n_fast_resign = 0
    for key, r in recs.items():
        row, db, dp, dv = got[key]
        keep = r["move_kind"] != 2
        assert (int(row[0]), int(row[1]), int(row[5])) == (r["T"], r["winner"], int((~keep).sum())), key
        hb, hp, hv, length = record_to_samples(GAMES[game], r)
        assert length == r["T"]
        for what, d, h in (("boards", db, hb), ("policies", dp, hp), ("values", dv, hv)):
            assert d.dtype == h.dtype and d.shape == h.shape, (key, what, d.shape, h.shape)
            np.testing.assert_array_equal(d, h, err_msg=f"{name} game {key} {what}")
        if r["resigned"]:
            n_resigned += 1
            p = r["resign_ply"]
            assert p == r["T"] - 1 and r["winner"] == -mover(p) != 0                              # the last mover lost
            z = np.array([mover(t) * r["winner"] for t in range(r["T"])], np.float32)
            want = (np.float32(0.5) * (z + r["q"]))[keep]
            np.testing.assert_array_equal(dv[0, :, 0], want, err_msg=str(key))
            n_fast_resign += int(r["move_kind"][p] == 2)
    assert n_resigned > 0
    return n_resigned, n_fast_resign


# ------------------------------------------------------------------------------------------------ 6. sync mode
def sync_case(oracle, G, lib_path, name="c4", prefix=None):
    """a two-tree sync_moves engine driven by run_move / apply_moves(None): a slot halts after its resigning ply, and its drained record
    equals the continuous engine's first game.  With `prefix` every slot starts from that set_position prefix, in both engines, and the
    expectation comes from a continuous off engine with the same prefix: the run of `consecutive` plies starts after the prefix."""
    from grok_alpha_zero_amd.engine import PH_HALT
    rule = case_table()[name][3]
    engines = dict(off=make_engine(name, G, lib_path, games=G), cont=make_engine(name, G, lib_path, rule, games=G),
                   sync=make_engine(name, G, lib_path, rule, games=0, sync_moves=True, ring_capacity=2 * G))
    for e in engines.values():
        for g in range(G if prefix else 0):
            e.set_position(g, prefix)
    off, cont = play(engines["off"], G), play(engines["cont"], G)
    s = engines["sync"]
    halted_at = {}
    for ply in range(MAXT[case_table()[name][0]] + 1):
        s.run_move()
        ph = s.root_stats()["phase"]
        for g in range(G):
            if ph[g] == PH_HALT and g not in halted_at:
                halted_at[g] = ply
        if len(halted_at) == G:
            break
        s.apply_moves()
    recs = {(r["slot"], r["game_seq"]): r for r in s.drain_finished()}
    rs = s.resign_stats()
    for e in engines.values():
        e.close()
    assert sorted(recs) == sorted(cont) == [(g, 0) for g in range(G)]
    exp = {k: expectation(oracle, off[k], rule) for k in off}
    n0 = len(prefix or [])
    for k in sorted(recs):
        assert_prefix(cont[k], off[k], exp[k], f"continuous {k}")
        assert_prefix(recs[k], off[k], exp[k], f"sync {k}")
        assert halted_at[k[0]] == exp[k]["T"] - n0, (k, halted_at[k[0]], exp[k])            # searched plies until the slot halts
        if prefix:
            assert (off[k]["move_kind"][:n0] == 0).all()
            assert exp[k]["resign_ply"] == -1 or exp[k]["resign_ply"] >= n0 + 2 * (rule[1] - 1)
            assert all(p >= n0 + 2 * (rule[1] - 1) for p in exp[k]["would"])
    w = witnesses(exp)
    print(f"sync {name} G={G} prefix {prefix}: {w}", flush=True)
    assert w["resigned_by_minus1"] + w["resigned_by_plus1"] > 0 and w["natural"] + w["quiet_playout"] + w["would"] > 0, w
    assert rs == expected_stats(exp), (rs, expected_stats(exp))
    return exp


# ------------------------------------------------------------------------------------------------ 7. run_self_play
RSP_RULE = (0.3, 2, 0, 0.5)


def run_self_play_case(tmp, lib_path, games=40, G=24, game="TicTacToe"):
    """run_self_play with the four keys: total rows == the sum of T of a directly created engine's records, the same file at both settings of
    device_samples, engine_stats["resign"] filled, the tail's repack taken.  (Whether run_self_play meets a half-empty launch depends on how
    many games end between two of its drains: on the HIP build 64 waves finish a whole TicTacToe game, so the GPU suite plays Connect4,
    whose last games end over several hundred waves.)"""
    from grok_alpha_zero_amd import engine as E
    n_aug = N_AUG[game]
    train = dict(games_per_generation=games, MCTS_iteration_limit=16, max_actions=MAXT[game], num_explore_actions_first=2, num_explore_actions_second=1,
                 c_puct_init=1.25, dirichlet_alpha=1.0, use_gumbel=False, resign_threshold=RSP_RULE[0], resign_consecutive=RSP_RULE[1],
                 resign_min_ply=RSP_RULE[2], no_resign_prob=RSP_RULE[3])
    out, est, repacks = {}, {}, []
    real = E.SelfPlayEngine.repack

    def counting(self):
        repacks.append(1)
        return real(self)
    E.SelfPlayEngine.repack = counting
    try:
        for ds in (False, True):
            est[ds] = {}
            out[ds] = self_play_file(tmp, f"ds{ds}", game, train, games, n_games=G, seed=11, hash_salt=4, lib_path=lib_path, device_samples=ds,
                                     engine_stats=est[ds])
            assert repacks, "the tail of the generation was not repacked"
            del repacks[:]
    finally:
        E.SelfPlayEngine.repack = real
    eng = E.SelfPlayEngine(game, G, 24, MAXT[game], 2, 1, 1.25, 1.0, seed=11, hash_salt=4, ring_capacity=4 * games, games_budget=games, lib_path=lib_path,
                           resign_threshold=RSP_RULE[0], resign_consecutive=RSP_RULE[1], resign_min_ply=RSP_RULE[2], no_resign_prob=RSP_RULE[3])
    recs = list(play(eng, games, waves=16).values())
    direct = eng.resign_stats()
    eng.close()
    plies = sum(r["T"] for r in recs)
    assert direct["resigned"] > 0 and direct["playout_games"] > 0 and direct["resigned"] == sum(r["resigned"] for r in recs), direct
    for ds in (False, True):
        f = out[ds]
        assert est[ds]["resign"] == direct, (est[ds]["resign"], direct)
        assert [int(x) for x in f["game_stats"]] == game_stats_of(recs), f["game_stats"]
        assert len(f) == 1 + 3 * n_aug * games and sum(f[f"values_{n_aug * k}"].shape[0] for k in range(games)) == plies
    assert games_of_file(out[False], games, n_aug) == games_of_file(out[True], games, n_aug)
    return direct


# ------------------------------------------------------------------------------------------------ 8. resign_curve
def curve_case(G, lib_path, name="c4"):
    """self_play.resign_curve on played-out records against the restated rule"""
    from grok_alpha_zero_amd.self_play import resign_curve
    eng = make_engine(name, G, lib_path)
    recs = list(play(eng, 2 * G).values())
    eng.close()
    thresholds = [0.05, 0.3, 0.6, 0.9, 0.999]
    for c, m in ((1, 0), (2, 0), (1, 6), (3, 4)):
        rows = resign_curve(recs, thresholds, consecutive=c, min_ply=m)
        assert [r["threshold"] for r in rows] == thresholds
        for row in rows:
            would = fp = saved = 0
            for r in recs:
                trig = [p for p in range(r["T"] - 1) if trigger(r["q"], r["move_kind"], p, row["threshold"], c, m)]
                if trig:
                    would += 1; saved += r["T"] - (trig[0] + 1); fp += r["winner"] != -mover(trig[0])
            assert (row["games"], row["would_resign"], row["false_positives"], row["plies_saved"], row["plies"]) == \
                (len(recs), would, fp, saved, sum(r["T"] for r in recs)), (c, m, row)
        assert [r["would_resign"] for r in rows] == sorted((r["would_resign"] for r in rows), reverse=True)      # a higher threshold triggers less
    first = resign_curve(recs, [0.05])[0]
    assert 0 < first["would_resign"] and 0 < first["plies_saved"] < first["plies"]


# ------------------------------------------------------------------------------------------------ 9. refusals
REFUSALS = {   # name -> set_resignation arguments (threshold, consecutive, min_ply, no_resign_prob), what the message must say
    "threshold-nan": ((float("nan"), 1, 0, 0.0), "threshold must be a number"),
    "threshold-inf": ((float("inf"), 1, 0, 0.0), "threshold must be finite"),
    "threshold-negative": ((-0.25, 1, 0, 0.0), "threshold must be >= 0"),
    "threshold-one": ((1.0, 1, 0, 0.0), "threshold must be below 1"),
    "consecutive-zero": ((0.5, 0, 0, 0.0), "consecutive must be in [1, 8]"),
    "consecutive-nine": ((0.5, 9, 0, 0.0), "consecutive must be in [1, 8]"),
    "min-ply-negative": ((0.5, 1, -1, 0.0), "min_ply must be >= 0"),
    "prob-nan": ((0.5, 1, 0, float("nan")), "no_resign_prob must be in [0, 1]"),
    "prob-negative": ((0.5, 1, 0, -0.5), "no_resign_prob must be in [0, 1]"),
    "prob-above-one": ((0.5, 1, 0, 1.5), "no_resign_prob must be in [0, 1]"),
}


def refusal_case(name, lib_path):
    """-> the message.  A refused call leaves the engine as it was: off"""
    from grok_alpha_zero_amd.engine import ResignParams, SelfPlayEngine
    eng = SelfPlayEngine("Connect4", 4, 40, 42, 4, 4, 2.5, 0.5, seed=1, lib_path=lib_path)
    try:
        if name == "struct-size":
            p = ResignParams(struct_size=C.sizeof(ResignParams) - 8, consecutive=1, min_ply=0, threshold=0.5, no_resign_prob=0.0)
            assert eng.L.gaz_engine_set_resignation(eng.h, C.byref(p)) != 0
            msg = eng.L.gaz_engine_last_error(eng.h).decode()
            assert "struct_size" in msg, msg
        else:
            args, text = REFUSALS[name]
            msg = refusal_message(lambda: eng.set_resignation(*args), f"{name}: gaz_engine_set_resignation accepted {args}")
            assert text in msg, (name, msg)
            kw = dict(resign_threshold=args[0], resign_consecutive=args[1], resign_min_ply=args[2], no_resign_prob=args[3])
            assert text in refusal_message(lambda: SelfPlayEngine("Connect4", 4, 40, 42, 4, 4, 2.5, 0.5, seed=1, lib_path=lib_path, **kw).close(),
                                           f"{name}: the constructor accepted {args}")      # the constructor keywords go through the same call
        return msg
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ 10. scheduling equalities (HIP build, network)
def scheduling_case(which, G=64):
    """64 Connect4 games with a 1-block network and resignation on: the records do not depend on the fused launch, the game groups or the
    evaluation cache"""
    rule = (0.3, 2, 0, 0.5)

    def some_game_resigned(recs, rs):
        assert rs["resigned"] > 0 and rs["playout_games"] > 0, rs
    scheduling_equalities(which, G, dict(seed=SEED, resign_threshold=rule[0], resign_consecutive=rule[1], resign_min_ply=rule[2], no_resign_prob=rule[3]),
                          lambda eng: (play(eng, G, raw=True), eng.resign_stats()), some_game_resigned)

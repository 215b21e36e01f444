"""The cases of the opening book (gaz_engine_set_opening_book) that the CPU suite runs on the emulation build
(tests/test_opening_book_emu.py) and the -m gpu suite on the HIP build (tests/test_opening_book_gpu.py): `lib_path` = the emulation
library, or None for the product library.

What a game must be is never read from the engine under test: the entry a game starts from is the draw restated with
grok_alpha_zero_amd/det.py (self_play.book_entry, checked here against oracle.uniform), and the game behind the prefix is the oracle's
game from start_history = that entry.  Every comparison is exact."""
import ctypes as C

import numpy as np

from selfplay_support import MAXT, assert_records_equal, play, refusal_message

P_OPENING, BOOK_TREE, MK_BOOK = 4, 3, 3
SEARCHED = ("actions", "policies", "q", "root_N", "root_W", "root_P", "root_visits", "evals")
PER_MOVE = ("policies", "q", "root_N", "root_W", "root_P", "root_visits", "evals")


def game_class(game):
    from grok_alpha_zero_amd.games import GAMES
    return GAMES[game]


def _gumbel(m):
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL
    return dict(search=SEARCH_GUMBEL, gumbel_m=m, c_visit=50.0, c_scale=1.0)


def no_five_prefix(n):
    from playout_cap_cases import no_five_prefix as f
    return f(n)


# ------------------------------------------------------------------------------------------------ books
C4_COLUMN = [0, 0, 0, 0, 0, 0]                     # fills one column: six landing rows from one action
C4_LONG = [0, 1, 0, 1, 2, 3, 2, 3, 4, 5, 4, 5, 6, 0, 6, 1, 2, 3]      # 18 plies, more than a 16-lane team; no four in a row anywhere
TTT_ALMOST_FULL = [0, 1, 2, 4, 3, 5, 7, 6]         # eight plies without a line: one move from a full board
# name -> (game, gumbel m or None, G, run_iterations, max_actions, explore_first, explore_second, c_puct_init, alpha, seed, entries, mode)
# The seeds were chosen on the emulation build so that every witness of oracle_case holds (four games per slot).
CASES = {
    "c4-puct": ("Connect4", None, 4, 20, 42, 3, 2, 2.5, 0.5, 17, [[], [3], C4_COLUMN, C4_LONG, [3, 3, 2, 4, 2]], "game"),
    "c4-gumbel": ("Connect4", 4, 4, 16, 42, 0, 0, 0.0, 0.0, 5, [[], C4_LONG, [2, 4, 4]], "pair"),
    "c4-cap": ("Connect4", None, 4, 20, 8, 2, 1, 2.5, 0.5, 3, [[], [6], [0, 1, 2, 3, 4, 5, 6]], "game"),      # lengths 0, 1 and max_actions - 1
    "ttt-puct": ("TicTacToe", None, 4, 24, 9, 3, 2, 1.25, 1.0, 11, [[], [4], TTT_ALMOST_FULL], "game"),
    "ttt-gumbel": ("TicTacToe", 4, 4, 16, 9, 0, 0, 0.0, 0.0, 2, [[], [8], TTT_ALMOST_FULL, [0, 4], [4, 0, 8]], "game"),
    # entries of 66, 68 and 70 plies, longer than a wavefront; 160 iterations cover the 159 legal moves left (below them a move runs 3 x its legal moves)
    "gmk-puct": ("Gomoku", None, 2, 160, 72, 2, 2, 2.5, 0.05, 7, "gmk", "game"),
    "gmk-gumbel": ("Gomoku", 4, 2, 12, 72, 0, 0, 0.0, 0.0, 9, "gmk", "pair"),
}
SLOT_OFFSET, SALT = 40, 6


def entries_of(name):
    e = CASES[name][10]
    return [no_five_prefix(n) for n in (66, 68, 70)] if e == "gmk" else [list(x) for x in e]


def make_engine(name, lib_path, G=None, games_per_slot=4, book=True, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    game, m, G0, iters, max_actions, ef, es, c_init, alpha, seed, _, mode = CASES[name]
    G = G or G0
    a = dict(seed=seed, hash_salt=SALT, slot_offset=SLOT_OFFSET, ring_capacity=2 * games_per_slot * G + 8, games_budget=games_per_slot * G, lib_path=lib_path)
    if m:
        a.update(_gumbel(m))
    a.update(kw)
    eng = SelfPlayEngine(game, G, iters, max_actions, ef, es, c_init, alpha, **a)
    if book:
        eng.set_opening_book(entries_of(name), mode)
        assert eng.opening_book() == (len(entries_of(name)), mode)
    return eng


def oracle_game(oracle, name, slot, seq, prefix):
    game, m, _, iters, max_actions, ef, es, c_init, alpha, seed, _, _ = CASES[name]
    if m:
        return oracle.selfplay_game_gumbel(game, iters, max_actions, m, 50.0, 1.0, seed, slot, seq, hash_salt=SALT, start_history=prefix)
    return oracle.selfplay_game(game, iters, max_actions, ef, es, c_init, alpha, seed, slot, seq, hash_salt=SALT, start_history=prefix)


def assert_book_game(rec, o, prefix, what):
    """a record of a game started from `prefix` against the oracle's game from start_history = prefix: the prefix rows are zero with kind 3,
    the rest is the oracle's bit for bit"""
    n = len(prefix)
    assert o["n_start"] == n and rec["T"] == n + o["T"] and rec["winner"] == o["winner"], (what, rec["T"], n, o["T"], rec["winner"], o["winner"])
    np.testing.assert_array_equal(rec["actions"][:n], np.asarray(prefix, np.int32), err_msg=f"{what}: prefix actions")
    assert (rec["move_kind"][:n] == MK_BOOK).all() and not (rec["move_kind"][n:] == MK_BOOK).any() and (rec["move_kind"][n:] != 0).all(), (what, rec["move_kind"])
    for k in PER_MOVE:
        assert not np.asarray(rec[k][:n]).any(), f"{what}: {k} of the prefix rows is not 0"
    for k in SEARCHED:
        np.testing.assert_array_equal(np.asarray(rec[k][n:]).reshape(np.asarray(o[k]).shape), o[k], err_msg=f"{what}: {k}")


def oracle_case(oracle, name, lib_path, G=None, games_per_slot=4, slots=None, **kw):
    """continuous mode, hash evaluator, every slot plays `games_per_slot` games: game (slot, seq) is the oracle's game from the entry the
    restated draw names.  Witnesses: at least two entries drawn; an empty and a non-empty one where the book has an empty entry;
    book_counts equal to the restated draws"""
    from grok_alpha_zero_amd.self_play import book_entry
    seed, mode, book = CASES[name][9], CASES[name][11], entries_of(name)
    G = G or CASES[name][2]
    eng = make_engine(name, lib_path, G, games_per_slot, **kw)
    recs = play(eng, games_per_slot * G)
    bc = eng.book_counts()
    eng.close()
    assert sorted(recs) == [(SLOT_OFFSET + g, q) for g in range(G) for q in range(games_per_slot)]
    want = np.zeros(len(book), np.uint64)
    drawn = {}
    for (slot, seq) in recs:
        idx = book_entry(seed, slot, seq, len(book), mode)
        u = oracle.uniform(seed, slot, seq & ~1 if mode == "pair" else seq, BOOK_TREE, 0, P_OPENING)
        assert idx == min(int(u * len(book)), len(book) - 1), (slot, seq)
        drawn[(slot, seq)] = idx; want[idx] += 1
    for (slot, seq), r in sorted(recs.items()):
        if slots is None or slot - SLOT_OFFSET in slots:
            prefix = book[drawn[(slot, seq)]]
            assert_book_game(r, oracle_game(oracle, name, slot, seq, prefix), prefix, f"{name} game {(slot, seq)} entry {drawn[(slot, seq)]}")
        else:
            prefix = book[drawn[(slot, seq)]]
            assert list(r["actions"][:len(prefix)]) == prefix and int((r["move_kind"] == MK_BOOK).sum()) == len(prefix), (name, slot, seq)
    np.testing.assert_array_equal(bc["counts"], want, err_msg=f"{name}: book_counts")
    assert bc["started"] == len(recs) and bc["prefix_plies"] == sum(len(book[i]) for i in drawn.values()), bc
    assert len(set(drawn.values())) >= 2, f"{name}: one entry only was drawn {drawn}: pick another seed"
    if any(len(e) == 0 for e in book):
        lens = {len(book[i]) == 0 for i in drawn.values()}
        assert lens == {True, False}, f"{name}: empty and non-empty entries were not both drawn: pick another seed"
    print(f"{name} G={G}: {len(recs)} games, entries drawn {want.tolist()}", flush=True)
    return recs, drawn


# ------------------------------------------------------------------------------------------------ pairs
def pairs_case(lib_path, name="c4-puct", G=4, games_per_slot=4):
    """mode 2: the games (s, 2k) and (s, 2k + 1) share their prefix for every slot and k, and are different games behind it; mode 1: at
    least one such pair differs"""
    book = entries_of(name)
    out = {}
    for mode in ("pair", "game"):
        eng = make_engine(name, lib_path, G, games_per_slot, book=False)
        eng.set_opening_book(book, mode)
        recs = play(eng, games_per_slot * G)
        eng.close()
        same = []
        for g in range(G):
            for k in range(games_per_slot // 2):
                a, b = recs[(SLOT_OFFSET + g, 2 * k)], recs[(SLOT_OFFSET + g, 2 * k + 1)]
                na, nb = int((a["move_kind"] == MK_BOOK).sum()), int((b["move_kind"] == MK_BOOK).sum())
                same.append(na == nb and list(a["actions"][:na]) == list(b["actions"][:nb]))
        out[mode] = same
    assert all(out["pair"]), out
    assert not all(out["game"]), "mode 1 drew the same entry for both games of every pair: pick another seed"
    return out


def match_owner_case(lib_path, G=4):
    """match play with the external evaluator, Gumbel search (the owner of a request is the player to move), book in mode 2: in the two
    games of a pair the same mover is answered by opposite networks, and both start from the same prefix"""
    from grok_alpha_zero_amd.engine import EVAL_EXTERNAL, SelfPlayEngine
    book = [[3], [2, 4, 4], [3, 3, 2, 4, 2]]
    eng = SelfPlayEngine("Connect4", G, 8, 42, 0, 0, 0.0, 0.0, seed=5, evaluator=EVAL_EXTERNAL, ring_capacity=4 * G, games_budget=2 * G, game_groups=1,
                         lib_path=lib_path, **_gumbel(4))
    eng.set_match(True)
    eng.set_opening_book(book, "pair")
    rng = np.random.default_rng(0)
    seq, owners, recs = [0] * G, {}, {}
    for _ in range(200000):
        eng.wave_begin()
        x, pend = eng.read_batch()
        net = eng.read_batch_network()
        hist = eng.read_positions()
        for r in np.flatnonzero(pend):
            mover = len(hist[r]) % 2
            owners.setdefault((int(r), seq[r], mover), set()).add(int(net[r]))
        pol = rng.random((G, 7)).astype(np.float32); val = (rng.random(G).astype(np.float32) - 0.5)
        eng.write_outputs(pol, val)
        for rec in eng.drain_finished():
            recs[(rec["slot"], rec["game_seq"])] = rec; seq[rec["slot"]] += 1
        if len(recs) == 2 * G:
            break
    eng.close()
    assert len(recs) == 2 * G
    for g in range(G):
        a, b = recs[(g, 0)], recs[(g, 1)]
        n = int((a["move_kind"] == MK_BOOK).sum())
        assert n > 0 and n == int((b["move_kind"] == MK_BOOK).sum()) and list(a["actions"][:n]) == list(b["actions"][:n])
        for mover in (0, 1):
            x, y = owners[(g, 0, mover)], owners[(g, 1, mover)]
            assert len(x) == len(y) == 1 and x != y, (g, mover, x, y)
            assert x == {mover ^ (g & 1)}, (g, mover, x)
    return owners


def closed_form_pairs(headers):
    """the paired tally of match_result restated from headers (T, winner, slot, game_seq)"""
    pts = {}
    for _, winner, slot, seq in headers:
        a_first = (slot + seq) % 2 == 0
        pts.setdefault((slot, seq >> 1), {})[seq & 1] = 0.5 if winner == 0 else float((winner == -1) == a_first)
    whole = [p[0] + p[1] for p in pts.values() if len(p) == 2]
    return {s: whole.count(s) for s in (0.0, 0.5, 1.0, 1.5, 2.0)}, len(pts) - len(whole), whole


def match_result_case():
    """match_result(paired=True) against the closed form; the default output is unchanged"""
    import math
    from grok_alpha_zero_amd.self_play import match_result
    rng = np.random.default_rng(3)
    hdrs = [(9, int(rng.integers(-1, 2)), s, q) for s in range(6) for q in range(4)] + [(9, 1, 7, 0), (9, -1, 8, 3)]
    plain, paired = match_result(hdrs), match_result(hdrs, paired=True)
    assert all(paired[k] == plain[k] for k in plain) and set(paired) - set(plain) == {"pairs", "incomplete", "elo_ci95_paired"}
    pairs, incomplete, whole = closed_form_pairs(hdrs)
    assert paired["pairs"] == pairs and paired["incomplete"] == incomplete == 2 and sum(pairs.values()) == 12
    means = [w / 2 for w in whole]
    m = sum(means) / len(means)
    half = 1.96 * math.sqrt(sum((x - m) ** 2 for x in means) / len(means) / len(means))
    elo = lambda s: -400.0 * math.log10(1.0 / min(max(s, 1e-9), 1 - 1e-9) - 1.0)      # noqa: E731
    assert paired["elo_ci95_paired"] == (elo(m - half), elo(m + half))
    assert match_result([(9, 1, 0, 0)], paired=True)["elo_ci95_paired"] is None
    return paired


def play_match_case(lib_path, games=16, n_slots=4):
    """play_match(book=...) end to end with two hash salts: paired by default, every pair from one entry, the paired block in the result"""
    from grok_alpha_zero_amd.self_play import book_entry, match_result, play_match
    train = dict(MCTS_iteration_limit=12, max_actions=42, num_explore_actions_first=0, num_explore_actions_second=0, c_puct_init=2.5, dirichlet_alpha=0.5, use_gumbel=False)
    book = [[3], [2, 4, 4], [3, 3], [0, 6]]
    res = play_match(game_class("Connect4"), ({}, train), None, None, games, n_slots=n_slots, seed=21, book=book, hash_salt=5, hash_salt_b=9, lib_path=lib_path, tau=0.0,
                     use_dirichlet=False)
    hdrs = res.pop("headers")
    assert sorted((s, q) for _, _, s, q in hdrs) == [(s, q) for s in range(n_slots) for q in range(games // n_slots)]
    want = match_result(hdrs, paired=True)
    assert all(res[k] == want[k] for k in want) and res["incomplete"] == 0 and sum(res["pairs"].values()) == games // 2
    assert res["pairs"] == closed_form_pairs(hdrs)[0]
    counts = [0] * len(book)
    for _, _, s, q in hdrs:
        counts[book_entry(21, s, q, len(book), "pair")] += 1
    assert res["book"]["counts"] == counts and res["book"]["mode"] == "pair" and all(c % 2 == 0 for c in counts)
    unpaired = play_match(game_class("Connect4"), ({}, train), None, None, games, n_slots=n_slots, seed=21, book=book, paired=False, hash_salt=5, hash_salt_b=9,
                          lib_path=lib_path)
    assert "pairs" not in unpaired and unpaired["book"]["mode"] == "game"
    return res


# ------------------------------------------------------------------------------------------------ anchors
FEATURES = {   # what else is on while a book of empty entries must change nothing
    "plain": {}, "solver": dict(solver=True), "symmetry": dict(eval_symmetry=True), "forced": dict(forced_playouts_k=2.0),
    "cap": dict(fast_iterations=6, full_search_prob=0.5), "resign": dict(resign_threshold=0.5, resign_consecutive=1, resign_min_ply=2, no_resign_prob=0.25),
    "match": dict(game_groups=1, match=True), "opening": dict(opening_actions=[(1, 0.5), (5, 0.25)]),
}


def empty_book_case(lib_path, name, feature, games_per_slot=2):
    """a book of empty entries only == no book, byte for byte (opening_actions included), and the book really ran: its counters say so"""
    kw = dict(FEATURES[feature])
    match = kw.pop("match", False)
    G = CASES[name][2]
    out = []
    for book in (None, [[], [], []]):
        eng = make_engine(name, lib_path, G, games_per_slot, book=False, **kw)
        if match:
            eng.set_match(True, hash_salt_b=9)
        if book:
            eng.set_opening_book(book, "game")
        out.append(play(eng, games_per_slot * G, raw=True))
        bc = eng.book_counts()
        eng.close()
        assert (bc["started"], bc["prefix_plies"]) == ((games_per_slot * G, 0) if book else (0, 0)), bc
    a, b = out
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), (name, feature, k)
    return len(a)


def removal_case(lib_path, name="c4-puct"):
    """sync mode: the book in force when a game STARTS decides; removing it between two games restores empty starts"""
    from grok_alpha_zero_amd.engine import PH_HALT
    G = CASES[name][2]
    eng = make_engine(name, lib_path, G, book=False, sync_moves=True, games_budget=0, ring_capacity=4 * G)
    eng.set_opening_book([[3, 3, 2]], "game")

    def one_round():
        for _ in range(MAXT["Connect4"] + 1):
            eng.run_move()
            if (eng.root_stats()["phase"] == PH_HALT).all():
                break
            eng.apply_moves()
        return {r["slot"]: r for r in eng.drain_finished()}
    first = one_round()
    eng.set_opening_book(None, None)
    assert eng.opening_book() == (0, None)
    eng.reset_games()
    second = one_round()
    eng.set_opening_book([[2, 4]], "pair")
    eng.reset_games()
    third = one_round()
    eng.close()
    assert len(first) == len(second) == len(third) == G
    for r in first.values():
        assert list(r["actions"][:3]) == [3, 3, 2] and (r["move_kind"][:3] == MK_BOOK).all() and r["game_seq"] == 0
    for r in second.values():
        assert not (r["move_kind"] == MK_BOOK).any() and (r["move_kind"] == 1).all() and r["game_seq"] == 1
    for r in third.values():
        assert list(r["actions"][:2]) == [2, 4] and (r["move_kind"][:2] == MK_BOOK).all() and r["game_seq"] == 2
    return True


def set_position_anchor_case(lib_path, name, prefix):
    """sync mode: a one-entry book == set_position of that prefix on the searched plies; the records differ in move_kind only (3 vs 0)"""
    from grok_alpha_zero_amd.engine import PH_HALT
    G = CASES[name][2]
    recs = []
    for how in ("book", "set_position"):
        eng = make_engine(name, lib_path, G, book=False, sync_moves=True, games_budget=0, ring_capacity=4 * G)
        if how == "book":
            eng.set_opening_book([prefix], "game")
            assert eng.opening_book() == (1, "game")
        else:
            for g in range(G):
                eng.set_position(g, prefix)
        for _ in range(MAXT[CASES[name][0]] + 1):
            eng.run_move()
            if (eng.root_stats()["phase"] == PH_HALT).all():
                break
            eng.apply_moves()
        recs.append({r["slot"]: r for r in eng.drain_finished()})
        eng.close()
    a, b = recs
    n = len(prefix)
    assert sorted(a) == sorted(b) == [SLOT_OFFSET + g for g in range(G)]
    for k in a:
        assert_records_equal(a[k], b[k], f"{name} slot {k}")
        assert (a[k]["move_kind"][:n] == MK_BOOK).all() and (b[k]["move_kind"][:n] == 0).all()
        np.testing.assert_array_equal(a[k]["move_kind"][n:], b[k]["move_kind"][n:])
    return len(a)


# ------------------------------------------------------------------------------------------------ composition
def leaf_batch_case(oracle, lib_path, K=4, G=3):
    """leaf_batch = 4 against tests/leaf_batch_model.py started from the prefix the draw names"""
    from leaf_batch_model import Tree
    from grok_alpha_zero_amd.self_play import book_entry
    name = "c4-puct"
    game, _, _, iters, max_actions, ef, es, c_init, alpha, seed, _, mode = CASES[name]
    book = entries_of(name)
    eng = make_engine(name, lib_path, G, 2, leaf_batch=K)
    recs = play(eng, 2 * G)
    eng.close()
    for (slot, seq), r in sorted(recs.items()):
        prefix = book[book_entry(seed, slot, seq, len(book), mode)]
        n = len(prefix)
        assert list(r["actions"][:n]) == prefix and (r["move_kind"][:n] == MK_BOOK).all()
        trees = [Tree(oracle, game, K, seed, slot=slot, game_seq=seq, tree=k, c_puct_init=c_init, dirichlet_alpha=alpha, hash_salt=SALT, max_tree_sims=4, history=prefix)
                 for k in range(2)]
        for ply in range(n, r["T"]):
            m = trees[ply % 2].run(iters)
            for k, rk in (("N", "root_N"), ("W", "root_W"), ("P", "root_P")):
                np.testing.assert_array_equal(r[rk][ply], m[k], err_msg=f"leaf_batch {(slot, seq)} ply {ply} {k}")
            assert r["root_visits"][ply] == m["root_visits"] and r["evals"][ply] == m["evals"], (slot, seq, ply)
            if ply + 1 < r["T"]:
                for t in trees:
                    t.play(r["actions"][ply])
    return len(recs)


def same_records_case(lib_path, name, kw_a, kw_b, G=None, games_per_slot=2, repack=False):
    """two engine shapes that must play the same games from the book: records equal byte for byte"""
    G = G or CASES[name][2]
    out = []
    for kw in (kw_a, kw_b):
        eng = make_engine(name, lib_path, G, games_per_slot, **kw)
        if repack and kw is kw_a:
            recs = {}
            for _ in range(40000):
                eng.run_waves(8)
                for i, raw in play_raw_once(eng).items():
                    recs[i] = raw
                if len(recs) >= games_per_slot * G:
                    break
                left = games_per_slot * G - len(recs)
                if left <= G // 2 or left == 1:
                    eng.repack()
            assert len(recs) == games_per_slot * G
            out.append(recs)
        else:
            out.append(play(eng, games_per_slot * G, raw=True))
        eng.close()
    a, b = out
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), (name, kw_a, kw_b, k)
    assert any((a[k][_mk_off(lib_path, name):][:1] & 3) == MK_BOOK for k in a), "no game started from the book"
    return len(a)


_MK_OFF = {}


def _mk_off(lib_path, name):
    if name not in _MK_OFF:
        eng = make_engine(name, lib_path, 1, 1, book=False)
        _MK_OFF[name] = int(eng.layout.off_move_kind)
        eng.close()
    return _MK_OFF[name]


def play_raw_once(eng):
    lay = eng.layout
    buf = np.zeros((max(eng.cfg.ring_capacity, 1), lay.record_bytes), np.uint8)
    got = C.c_int32()
    eng._ck(eng.L.gaz_engine_drain_finished(eng.h, buf.ctypes.data, buf.shape[0], C.byref(got)))
    out = {}
    for i in range(got.value):
        hdr = buf[i, lay.off_hdr:lay.off_hdr + 16].view(np.int32)
        out[(int(hdr[2]), int(hdr[3]))] = buf[i].copy()
    return out


def single_tree_case(oracle, lib_path, G=3):
    """single_tree: one tree plays both sides from the book position — against leaf_batch_model's one-tree search"""
    from leaf_batch_model import Tree
    from grok_alpha_zero_amd.self_play import book_entry
    name = "c4-puct"
    game, _, _, iters, max_actions, ef, es, c_init, alpha, seed, _, mode = CASES[name]
    book = entries_of(name)
    eng = make_engine(name, lib_path, G, 2, single_tree=True)
    recs = play(eng, 2 * G)
    eng.close()
    for (slot, seq), r in sorted(recs.items()):
        prefix = book[book_entry(seed, slot, seq, len(book), mode)]
        n = len(prefix)
        assert list(r["actions"][:n]) == prefix and (r["move_kind"][:n] == MK_BOOK).all() and not np.asarray(r["root_N"][:n]).any()
        t = Tree(oracle, game, 1, seed, slot=slot, game_seq=seq, tree=0, c_puct_init=c_init, dirichlet_alpha=alpha, hash_salt=SALT, history=prefix)
        for ply in range(n, r["T"]):
            m = t.run(iters)
            np.testing.assert_array_equal(r["root_N"][ply], m["N"], err_msg=f"single_tree {(slot, seq)} ply {ply}")
            np.testing.assert_array_equal(r["root_W"][ply], m["W"]); np.testing.assert_array_equal(r["root_P"][ply], m["P"])
            if ply + 1 < r["T"]:
                t.play(r["actions"][ply])
    return len(recs)


# ------------------------------------------------------------------------------------------------ samples
def samples_case(lib_path, name="c4-puct", G=4, games_per_slot=3, **kw):
    """drain_samples == record_to_samples of a twin's records; a game has T minus its fast plies minus its book plies rows; a kept row's
    state shows the prefix"""
    from grok_alpha_zero_amd.self_play import record_to_samples
    from surprise_cases import all_records, all_samples
    host, dev = make_engine(name, lib_path, G, games_per_slot, **kw), make_engine(name, lib_path, G, games_per_slot, **kw)
    recs, got = all_records(host, games_per_slot * G), all_samples(dev, games_per_slot * G)
    host.close(); dev.close()
    book_plies = fast_plies = 0
    for key, r in recs.items():
        row, b, p, v, plies = got[key]
        hb, hp, hv, T = record_to_samples(game_class(CASES[name][0]), r)
        assert T == r["T"] == int(row[0]) and b.tobytes() == hb.tobytes() and p.tobytes() == hp.tobytes() and v.tobytes() == hv.tobytes(), key
        nb, nf = int((r["move_kind"] == MK_BOOK).sum()), int((r["move_kind"] == 2).sum())
        assert b.shape[1] == r["T"] - nf - nb and int(row[5]) == nf + nb, (key, b.shape, r["T"], nf, nb)
        np.testing.assert_array_equal(plies, np.flatnonzero(r["move_kind"] < 2).astype(np.uint8))
        if nb:
            assert np.asarray(b[0, 0]).any(), "the first kept row shows an empty board behind a book prefix"
        book_plies += nb; fast_plies += nf
    assert book_plies > 0 and (fast_plies > 0) == bool(kw.get("fast_iterations"))
    return book_plies, fast_plies


def surprise_expected(oracle, game, rec, lam, fast_factor, seed):
    """tests/surprise_model.py extended by the book rule — a ply of kind 3 gives no row and takes no part: the model's counts of the record
    with its book plies marked kind 0 (such a ply takes no part in the means or the sums either), the book plies' one row each taken away"""
    import surprise_model as M
    n = int((rec["move_kind"] == MK_BOOK).sum())
    assert (rec["move_kind"][:n] == MK_BOOK).all()
    as_zero = dict(rec); as_zero["move_kind"] = np.where(rec["move_kind"] == MK_BOOK, 0, rec["move_kind"]).astype(np.uint8)
    c, m = M.row_counts(oracle, as_zero, lam, fast_factor, seed)
    c = np.asarray(c, np.int64).copy()
    assert (c[:n] == 1).all()
    c[:n] = 0
    b, p, v = M.every_row(game_class(game), rec)
    rows = np.repeat(np.arange(rec["T"]), c)
    return dict(c=c, m=m, row_ply=rows.astype(np.uint8), boards=b[:, rows], policies=p[:, rows], values=v[:, rows], no_row=int((c == 0).sum()))


def surprise_case(oracle, lib_path, name="c4-puct", G=4, games_per_slot=3, lam=0.5, fast_factor=1.5):
    """surprise weighting with a book and the cap on: the weighted drain's bytes, plies and games columns, self_play.sample_row_counts and
    record_to_samples(weighting=...) all equal the extended model: book plies have no rows and take no part in the means"""
    from grok_alpha_zero_amd.self_play import record_to_samples, sample_row_counts
    from surprise_cases import all_records, all_samples
    game, seed = CASES[name][0], CASES[name][9]
    kw = dict(fast_iterations=6, full_search_prob=0.5)
    host, dev = make_engine(name, lib_path, G, games_per_slot, **kw), make_engine(name, lib_path, G, games_per_slot, **kw)
    dev.set_sample_weighting(lam, fast_factor)
    recs, got = all_records(host, games_per_slot * G), all_samples(dev, games_per_slot * G)
    host.close(); dev.close()
    book_plies = moved = 0
    for key, r in recs.items():
        row, b, p, v, plies = got[key]
        want = surprise_expected(oracle, game, r, lam, fast_factor, seed)
        n = int((r["move_kind"] == MK_BOOK).sum())
        np.testing.assert_array_equal(sample_row_counts(r, lam, fast_factor, seed), want["c"], err_msg=f"{key}: sample_row_counts")
        np.testing.assert_array_equal(plies, want["row_ply"], err_msg=f"{key}: row_ply")
        assert int(row[5]) == want["no_row"] and int(row[0]) == r["T"], key
        for k, d in (("boards", b), ("policies", p), ("values", v)):
            assert d.shape == want[k].shape and d.tobytes() == want[k].tobytes(), (key, k)
        hb, hp, hv, T = record_to_samples(game_class(game), r, weighting=(lam, fast_factor, seed))
        assert hb.tobytes() == want["boards"].tobytes() and hp.tobytes() == want["policies"].tobytes() and hv.tobytes() == want["values"].tobytes(), key
        book_plies += n; moved += int((want["c"][n:] != (r["move_kind"][n:] == 1)).sum())
    assert book_plies > 0 and moved > 0
    return book_plies, moved


def resign_case(lib_path, G=8, games_per_slot=2, threshold=0.05, consecutive=2):
    """resignation (consecutive = 2, no play-out games) behind a five-ply prefix: every game ends where the rule restated in
    self_play.resign_trigger_plies says — a book ply (kind 3) breaks a run as kind 0 does — so a game whose first searched plies are below
    the threshold resigns no earlier than after `consecutive` searched plies of the resigning player, at ply >= n + 2 (consecutive - 1).
    Witness: a game whose first searched ply is below the threshold; had the prefix counted as searched plies below the threshold, it
    would have been resigned right there"""
    from grok_alpha_zero_amd.self_play import resign_trigger_plies
    prefix = [3, 3, 2, 4, 2]
    n = len(prefix)
    eng = make_engine("c4-puct", lib_path, G, games_per_slot, book=False, resign_threshold=threshold, resign_consecutive=consecutive, resign_min_ply=0, no_resign_prob=0.0)
    eng.set_opening_book([prefix], "game")
    recs = play(eng, games_per_slot * G)
    eng.close()
    resigned = witness = 0
    for key, r in sorted(recs.items()):
        q, kind, T = r["q"], r["move_kind"], r["T"]
        assert (kind[:n] == MK_BOOK).all() and not q[:n].any(), key
        assert resign_trigger_plies(q, kind, threshold, consecutive, 0) == [], key      # no trigger at a ply the game went on after
        if r["resigned"]:
            p = r["resign_ply"]
            assert p == T - 1 and p >= n + 2 * (consecutive - 1), (key, p)
            assert all(int(kind[p - 2 * i]) in (1, 2) and float(q[p - 2 * i]) < -threshold for i in range(consecutive)), (key, p)
            resigned += 1
        fake_q = q.copy(); fake_q[:n] = -1.0
        fake_kind = np.where(kind == MK_BOOK, 1, kind)
        fake = resign_trigger_plies(fake_q, fake_kind, threshold, consecutive, 0)
        witness += bool(fake) and fake[0] < n + 2 * (consecutive - 1)
    assert resigned > 0 and witness > 0, (resigned, witness)
    return resigned, witness


# ------------------------------------------------------------------------------------------------ refusals
def refusal_case(lib_path):
    """one refusal per text; after a refused call the previous book is still in force"""
    from grok_alpha_zero_amd.engine import BookParams, SelfPlayEngine
    eng = SelfPlayEngine("Connect4", 4, 20, 10, 3, 2, 2.5, 0.5, seed=1, lib_path=lib_path)
    ttt = SelfPlayEngine("TicTacToe", 4, 20, 9, 3, 2, 1.25, 1.0, seed=1, lib_path=lib_path)
    eng.set_opening_book([[3], [2, 4]], "pair")
    msgs = {}

    def raw(e, what, n, stride, mode, acts, lens, size=None, text=None):
        p = BookParams(struct_size=C.sizeof(BookParams) if size is None else size, n_entries=n, stride=stride, mode=mode)
        a = None if acts is None else np.ascontiguousarray(acts, np.uint8)
        ln = None if lens is None else np.ascontiguousarray(lens, np.int32)
        rc = e.L.gaz_engine_set_opening_book(e.h, C.byref(p), None if a is None else a.ctypes.data, None if ln is None else ln.ctypes.data)
        assert rc != 0, f"{what}: accepted"
        msgs[what] = e.L.gaz_engine_last_error(e.h).decode()
        assert msgs[what].startswith("set_opening_book:") and text in msgs[what], (what, msgs[what])
        assert e.opening_book() == ((2, "pair") if e is eng else (0, None)), what
    one = (np.array([[3, 0]], np.uint8), [1])
    raw(eng, "struct_size", 1, 2, 1, *one, size=8, text="struct_size")
    raw(eng, "mode", 1, 2, 3, *one, text="mode must be 0")
    raw(eng, "mode-negative", 1, 2, -1, *one, text="mode must be 0")
    raw(eng, "n-negative", -1, 2, 1, *one, text="n_entries must be in")
    raw(eng, "n-large", (1 << 20) + 1, 2, 1, *one, text="n_entries must be in")
    raw(eng, "stride-zero", 1, 0, 1, *one, text="stride must be in [1, 42]")
    raw(eng, "stride-large", 1, 43, 1, *one, text="stride must be in [1, 42]")
    raw(eng, "length-negative", 1, 2, 1, one[0], [-1], text="a length of -1 is outside [0, stride = 2]")
    raw(eng, "length-above-stride", 1, 2, 1, one[0], [3], text="a length of 3 is outside [0, stride = 2]")
    raw(eng, "null-actions", 1, 2, 1, None, [1], text="must not be null")
    raw(eng, "null-lengths", 1, 2, 1, one[0], None, text="must not be null")
    assert eng.L.gaz_engine_set_opening_book(eng.h, None, None, None) != 0
    msgs["null-params"] = eng.L.gaz_engine_last_error(eng.h).decode()
    assert "null argument" in msgs["null-params"]

    def refused(e, what, entries, text):
        msgs[what] = refusal_message(lambda: e.set_opening_book(entries, "game"), f"{what}: accepted")
        assert text in msgs[what], (what, msgs[what])
        assert e.opening_book() == ((2, "pair") if e is eng else (0, None)), what
    refused(eng, "illegal-column-full", [[3], [0] * 7], "entry 1: illegal move 0 at ply 6")
    refused(eng, "illegal-out-of-range", [[3, 9]], "entry 0: illegal move 9 at ply 1")
    refused(eng, "win-in-the-middle", [[0, 1, 0, 1, 0, 1, 0, 1]], "entry 0: the game is over after ply 6")
    refused(eng, "win-at-the-end", [[], [0, 1, 0, 1, 0, 1, 0]], "entry 1: the game is over after ply 6")
    refused(eng, "length-max-actions", [[0, 1, 2, 3, 4, 5, 6, 0, 1, 2]], "entry 0: a length of 10 plies leaves no move below max_actions = 10")
    refused(ttt, "full-board", [[0, 1, 2, 4, 3, 5, 7, 6, 8]], "entry 0: a length of 9 plies leaves no move below max_actions = 9")
    refused(ttt, "occupied-cell", [[4, 4]], "entry 0: illegal move 4 at ply 1")
    for bad in ("both", 3):
        try:
            eng.set_opening_book([[3]], bad)
            raise AssertionError("a bad mode was accepted")
        except ValueError as e:
            assert "mode must be" in str(e)
    # the previous book is still in force: the next games start from it
    eng.close(); ttt.close()
    e2 = SelfPlayEngine("Connect4", 2, 12, 10, 3, 2, 2.5, 0.5, seed=1, ring_capacity=8, games_budget=2, lib_path=lib_path)
    e2.set_opening_book([[3, 3]], "game")
    refusal_message(lambda: e2.set_opening_book([[0] * 7], "game"), "accepted")
    recs = play(e2, 2)
    e2.close()
    assert all(list(r["actions"][:2]) == [3, 3] and (r["move_kind"][:2] == MK_BOOK).all() for r in recs.values())
    assert len(set(msgs.values())) >= len(msgs) - 4, msgs                    # (the pairs that share a text on purpose: mode, n_entries, stride, null pointers)
    return msgs


# ------------------------------------------------------------------------------------------------ the Python helpers, run_self_play
def helpers_case():
    from grok_alpha_zero_amd.self_play import book_from_records, enumerate_openings, load_book, save_book
    import os
    import tempfile
    ttt2 = enumerate_openings(game_class("TicTacToe"), 2)
    assert len(ttt2) == 72 and [0, 1] in ttt2 and all(len(set(e)) == 2 for e in ttt2)
    assert len(enumerate_openings(game_class("Connect4"), 2)) == 49 and enumerate_openings(game_class("Connect4"), 0) == [[]]
    ttt5 = enumerate_openings(game_class("TicTacToe"), 5)
    assert [0, 3, 1, 4, 2] not in ttt5 and len(ttt5) == 9 * 8 * 7 * 6 * 5 - sum(1 for e in _perms5() if _x_wins(e))      # the first player's lines end a sequence
    recs = [dict(actions=np.array(a)) for a in ([3, 3, 2, 1], [3, 3, 2, 5], [3, 3, 4, 0], [1, 2], [3, 3, 2])]
    assert book_from_records(recs, 3) == [[3, 3, 2], [3, 3, 4]] and book_from_records(recs, 3, min_count=2) == [[3, 3, 2]]
    assert book_from_records([[1, 2, 3]], 2) == [[1, 2]]
    with tempfile.TemporaryDirectory() as tmp:
        for ext in ("json", "npy"):
            path = os.path.join(tmp, "book." + ext)
            save_book(path, [[], [3], [3, 3, 2]])
            assert load_book(path) == [[], [3], [3, 3, 2]]
    assert load_book([(1, 2), []]) == [[1, 2], []]
    return True


def _perms5():
    from itertools import permutations
    return list(permutations(range(9), 5))


def _x_wins(e):
    lines = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6)]
    xs = {e[0], e[2], e[4]}
    return any(set(ln) <= xs for ln in lines)


def run_self_play_case(oracle, tmp, lib_path, games=12, G=4):
    """run_self_play reads train_config["opening_book"] (a list and a file) and ["opening_book_mode"]: the file's datasets, at both settings
    of device_samples, are record_to_samples of the records of an engine with the same book; game_stats count every ply, the prefix too"""
    import os
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    from grok_alpha_zero_amd.self_play import record_to_samples, save_book
    from selfplay_support import games_of_file, self_play_file
    book, seed = [[], [4], TTT_ALMOST_FULL, [0, 4]], 11
    path = os.path.join(str(tmp), "book.json")
    save_book(path, book)
    train = dict(games_per_generation=games, MCTS_iteration_limit=16, max_actions=9, num_explore_actions_first=2, num_explore_actions_second=1, c_puct_init=1.25,
                 dirichlet_alpha=1.0, opening_book_mode="pair")
    out = {ds: self_play_file(tmp, f"ds{ds}", "TicTacToe", dict(train, opening_book=path if ds else book), games, n_games=G, seed=seed, hash_salt=4, lib_path=lib_path,
                              device_samples=ds) for ds in (False, True)}
    eng = SelfPlayEngine("TicTacToe", G, 24, 9, 2, 1, 1.25, 1.0, seed=seed, hash_salt=4, ring_capacity=4 * G, games_budget=games, lib_path=lib_path)
    eng.set_opening_book(book, "pair")
    recs = play(eng, games)
    eng.close()
    want, plies, prefix = [], 0, 0
    for r in recs.values():
        b, p, v, T = record_to_samples(game_class("TicTacToe"), r)
        want.append(tuple((a.dtype.str, a.shape, a.tobytes()) for j in range(8) for a in (b[j], p[j], v[j])))
        plies += r["T"]; prefix += int((r["move_kind"] == MK_BOOK).sum())
        assert b.shape[1] == r["T"] - int((r["move_kind"] == MK_BOOK).sum())
    assert prefix > 0
    for ds in (False, True):
        f = out[ds]
        assert f["game_stats"][2] == games and f["game_stats"][1] == plies, (ds, f["game_stats"], plies)
        assert games_of_file(f, games, 8) == sorted(want), f"device_samples={ds}"
    return plies, prefix


# ------------------------------------------------------------------------------------------------ the sanitizer driver
def build_driver():
    """tests/emu/book_main.cpp with the engine's host code and the one-lane build of its device code as ONE program under the address and
    undefined-behaviour sanitizers, the runtimes linked statically: run directly, on the CPU, never loaded into Python"""
    import os
    import subprocess
    from selfplay_support import EMU_DIR, ROOT
    csrc, out = os.path.join(ROOT, "grok_alpha_zero_amd", "csrc"), os.path.join(EMU_DIR, "book_asan")
    srcs = [os.path.join(csrc, "engine.hip"), os.path.join(EMU_DIR, "emu_stubs.cpp"), os.path.join(EMU_DIR, "book_main.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")] + [os.path.join(ROOT, "include", "gaz_engine.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DGAZ_HOST_EMU", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-x", "c++"] + srcs + ["-o", out])
    return out


DRIVER_CASES = {   # name -> the program's arguments
    "c4": dict(game="Connect4", n_games=6, run_iterations=16, max_actions=42, seed=3, mode=1), "c4-gumbel-pair": dict(game="Connect4", n_games=4, gumbel=1, mode=2, seed=4),
    "ttt": dict(game="TicTacToe", n_games=8, run_iterations=16, max_actions=9, seed=5, mode=2), "gmk": dict(game="Gomoku", n_games=2, run_iterations=8, max_actions=72, seed=6, mode=1),
    "c4-groups": dict(game="Connect4", n_games=6, game_groups=2, seed=7, mode=1),
}


def run_driver(driver, name):
    import subprocess
    r = subprocess.run([driver] + [f"{k}={v}" for k, v in DRIVER_CASES[name].items()], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------ the network in the loop (HIP build)
def scheduling_case(which, G=64):
    """1-block Connect4 network, a book of five entries: the fused launch, two game groups and the evaluation cache give the records of
    separate launches, one group, no cache; fused_wave is non-zero where it is without a book"""
    from selfplay_support import scheduling_equalities
    book = [[], [3], C4_COLUMN, C4_LONG, [3, 3, 2, 4, 2]]
    lay = {}

    def collect(eng):
        eng.set_opening_book(book, "game")
        recs = play(eng, G, raw=True)
        lay["mk"], lay["act"] = int(eng.layout.off_move_kind), int(eng.layout.off_actions)
        bc = eng.book_counts()
        return recs, (bc["counts"].tolist(), bc["started"], bc["prefix_plies"])

    def witness(recs, feature):
        counts, started, plies = feature
        assert started == G and sum(counts) == G and sum(c > 0 for c in counts) >= 3 and plies > 0, feature
        n_book = sum(int(((r[lay["mk"]:lay["mk"] + 42] & 3) == MK_BOOK).sum()) for r in recs.values())
        assert n_book == plies
    scheduling_equalities(which, G, dict(seed=31), collect, witness)

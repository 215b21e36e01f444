"""The cases of policy surprise weighting (gaz_engine_set_sample_weighting; DESIGN.md "Policy surprise weighting") that the CPU suite runs
on the emulation build (tests/test_surprise_emu.py) and the -m gpu suite on the HIP build (tests/test_surprise_gpu.py): `lib_path` = the
emulation library, or None for the product library.

What a record must give is computed by tests/surprise_model.py — the rule restated with the oracle's dlog and uniform variate — from the
records of a TWIN engine (same arguments, drained with drain_finished), never read back from the engine under test.  Every comparison is
exact: bytes, row counts, plies."""
import numpy as np

import surprise_model as M
from selfplay_support import A_OF, MAXT, refusal_message

FAST_FACTOR = 1.5


def game_class(game):
    from grok_alpha_zero_amd.games import GAMES
    return GAMES[game]


# ------------------------------------------------------------------------------------------------ engines and the two ways out of them
# name -> game, G, run_iterations, fast_iterations (0 = cap off), max_actions, full_search_prob, lambda, seed.  Two games per slot.
# The seeds of the cap-on cases were chosen on the emulation build so that the MODEL shows every witness of WITNESSES below.
CASES = {
    "ttt-off": ("TicTacToe", 8, 24, 0, 9, 0.0, 0.5, 31), "ttt-on": ("TicTacToe", 16, 24, 6, 9, 0.25, 1.0, 66),
    "c4-off": ("Connect4", 8, 40, 0, 42, 0.0, 1.0, 31), "c4-on": ("Connect4", 16, 40, 8, 8, 0.25, 0.5, 215),
    "gmk-off": ("Gomoku", 4, 16, 0, 10, 0.0, 0.5, 31), "gmk-on": ("Gomoku", 8, 12, 4, 3, 0.3, 1.0, 47),
}
# HIP build only.  gmk-long: from a 110-ply prefix, records longer than 128 plies.  gmk-full: games of natural length at the default
# fast_factor, where a Gomoku fast ply (A = 225) has to beat 1.5 x the mean surprise of the full ones to earn rows
LONG_CASES = {"gmk-long": ("Gomoku", 8, 16, 4, 225, 0.4, 0.5, 31), "gmk-full": ("Gomoku", 16, 48, 12, 225, 0.25, 0.5, 7)}
FAST_FACTORS = {"gmk-on": 1.0}                     # (Gomoku's fast plies seldom exceed 1.5 x the mean surprise of the full ones)
WITNESSES = ("fast_with_rows", "full_without_rows", "ply_with_two", "ineligible_fast", "rows_exceed_plies")


def make_engine(name, lib_path, G=None, games_per_slot=2, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    game, G0, R, F, max_actions, p, _, seed = {**CASES, **LONG_CASES}[name]
    G = G or G0
    args = dict(seed=seed, hash_salt=6, slot_offset=10, ring_capacity=4 * G, games_budget=games_per_slot * G, fast_iterations=F,
                full_search_prob=p if F else 0.0, lib_path=lib_path)
    args.update(kw)
    return SelfPlayEngine(game, G, R, max_actions, 3, 2, 2.5, 0.5, **args)


def all_records(eng, n, advance=None, waves=32, rounds=40000):
    """every one of the engine's n games as records -> {(slot, game_seq): record}"""
    out = {}
    for _ in range(rounds):
        advance() if advance else eng.run_waves(waves)
        for r in eng.drain_finished():
            out[(r["slot"], r["game_seq"])] = r
        if len(out) >= n:
            assert len(out) == n
            return out
    raise AssertionError(f"only {len(out)} of {n} games finished")


def split_batch(batch, out):
    """the games of one SampleBatch (with plies) -> out[(slot, game_seq)] = (games row, boards, policies, values, plies); checks the row
    accounting of the mode: rows contiguous from games[0, 4], the batch's rows closing the last game"""
    row = int(batch.games[0, 4]) if batch.n else 0
    assert batch.boards.shape[1] == batch.policies.shape[1] == batch.values.shape[0] == batch.rows
    assert batch.plies is None or batch.plies.shape == (batch.rows,)
    for i in range(batch.n):
        assert int(batch.games[i, 4]) == row
        b, p, v, length, n_pos, w = batch.game(i)
        n = batch.rows_of(i)
        assert b.shape[1] == p.shape[1] == v.shape[1] == n and length == n_pos == int(batch.games[i, 0]) and w == int(batch.games[i, 1])
        r0 = row - int(batch.games[0, 4])
        out[(int(batch.games[i, 2]), int(batch.games[i, 3]))] = (batch.games[i].copy(), b.copy(), p.copy(), v.copy(),
                                                                  None if batch.plies is None else batch.plies[r0:r0 + n].copy())
        row += n
    assert row - (int(batch.games[0, 4]) if batch.n else 0) == batch.rows


def all_samples(eng, n, advance=None, waves=32, rounds=40000, with_plies=True, **drain_kw):
    out = {}
    for _ in range(rounds):
        advance() if advance else eng.run_waves(waves)
        split_batch(eng.drain_samples(with_plies=with_plies, **drain_kw), out)
        if len(out) >= n:
            assert len(out) == n
            return out
    raise AssertionError(f"only {len(out)} of {n} games finished")


def assert_game_equals_model(oracle, game, rec, got, lam, seed, what, fast_factor=FAST_FACTOR):
    """one game of a weighted drain against the model, and record_to_samples(weighting=...) against the model -> the model's dict"""
    from grok_alpha_zero_amd.self_play import record_to_samples, sample_row_counts
    want = M.expected(oracle, game_class(game), rec, lam, fast_factor, seed)
    row, b, p, v, plies = got
    assert (int(row[0]), int(row[1]), int(row[2]), int(row[3])) == (rec["T"], rec["winner"], rec["slot"], rec["game_seq"]), what
    assert int(row[5]) == want["no_row"], (what, int(row[5]), want["no_row"])
    if plies is not None:
        np.testing.assert_array_equal(plies, want["row_ply"], err_msg=f"{what} row_ply")
    for k, d in (("boards", b), ("policies", p), ("values", v)):
        assert d.dtype == want[k].dtype and d.shape == want[k].shape, (what, k, d.shape, want[k].shape)
        assert d.tobytes() == want[k].tobytes(), f"{what} {k}"
    np.testing.assert_array_equal(sample_row_counts(rec, lam, fast_factor, seed), want["c"], err_msg=f"{what} sample_row_counts")
    hb, hp, hv, T = record_to_samples(game_class(game), rec, weighting=(lam, fast_factor, seed))
    assert T == rec["T"] and hb.tobytes() == want["boards"].tobytes() and hp.tobytes() == want["policies"].tobytes() and hv.tobytes() == want["values"].tobytes(), what
    return want


def weighted_case(oracle, name, lib_path, G=None, games_per_slot=2, witness=True, prefix=None, setup=None, **kw):
    """twin engines: one gives records, the other — with the mode on — samples with plies.  Every game == the model: bytes, row_ply, the
    games columns, the rows.  A cap-on case asserts every witness of WITNESSES, by the model's own counts and weights."""
    game, G0, R, F, max_actions, p, lam, seed = {**CASES, **LONG_CASES}[name]
    G = G or G0
    host, dev = make_engine(name, lib_path, G, games_per_slot, **kw), make_engine(name, lib_path, G, games_per_slot, **kw)
    ff = FAST_FACTORS.get(name, FAST_FACTOR)
    dev.set_sample_weighting(lam, ff)
    assert dev.sample_weighting == (lam, ff) and host.sample_weighting == (0.0, 1.5)
    for e in (host, dev) if setup else ():           # (what both engines get before they play: match play)
        setup(e)
    for g in range(G if prefix else 0):              # (the first game of every slot starts behind the prefix)
        host.set_position(g, prefix); dev.set_position(g, prefix)
    recs, got = all_records(host, games_per_slot * G), all_samples(dev, games_per_slot * G)
    host.close(); dev.close()
    assert sorted(recs) == sorted(got)
    seen = dict.fromkeys(WITNESSES, 0)
    rows = n_full = 0
    for key, rec in sorted(recs.items()):
        want = assert_game_equals_model(oracle, game, rec, got[key], lam, seed, f"{name} game {key}", fast_factor=ff)
        c, m = want["c"], want["m"]
        searched = int(c[m["kind"] != 0].sum())                                        # (a set_position prefix keeps its rows and takes no part)
        assert abs(searched - m["n_full"]) <= int(m["E"].sum()) and int(c.sum()) <= 2 * rec["T"], (name, key)
        for k, v in M.witnesses(c, m).items():
            seen[k] += v
        rows += int(c.sum()); n_full += m["n_full"]
    print(f"{name}: {len(recs)} games, {rows} rows for {n_full} full plies, witnesses {seen}", flush=True)
    if witness and F:
        assert all(seen.values()), f"{name}: a witness is missing {seen}: pick another seed"
    elif witness:
        assert seen["ply_with_two"] or seen["full_without_rows"], (name, seen)        # (cap off: the weighting acted at all)
    return recs, got


# the mode with the engine shapes that change how records come about: leaves in flight, one tree per game, two networks
SHAPES = {"leaf-batch": dict(leaf_batch=4), "single-tree": dict(single_tree=True),
          "match": dict(game_groups=1, setup=lambda e: e.set_match(True, hash_salt_b=9))}


def shape_case(oracle, shape, lib_path, name="ttt-on"):
    recs, got = weighted_case(oracle, name, lib_path, witness=False, **SHAPES[shape])
    assert any((r["move_kind"] == 2).any() for r in recs.values())
    return recs


# ------------------------------------------------------------------------------------------------ anchors
FEATURES = {   # what else is switched on while lambda = 0 must change nothing
    "plain": {}, "solver": dict(solver=True), "forced": dict(forced_playouts_k=2.0), "symmetry": dict(eval_symmetry=True),
    "resign": dict(resign_threshold=0.6, resign_consecutive=1, resign_min_ply=2, no_resign_prob=0.25),
}


def lambda_zero_case(name, feature, lib_path):
    """lambda = 0 == the mode off, byte for byte: (i) an engine that never heard of the mode, (ii) one set to lambda 0, (iii) one set to 0.5
    and back to 0 before its first drain, (iv) lambda 0 drained with plies — the counting kernels at lambda 0 — all give the same arrays and
    games columns; and the plies of (iv) are the plies that are not fast"""
    kw = FEATURES[feature]
    game, G = CASES[name][0], CASES[name][1]
    engines = [make_engine(name, lib_path, **kw) for _ in range(5)]
    engines[1].set_sample_weighting(0.0, 3.0)
    engines[2].set_sample_weighting(0.5); engines[2].set_sample_weighting(0.0)
    engines[3].set_sample_weighting(0.0)
    plain, zero, back, plies = (all_samples(e, 2 * G, with_plies=i == 3) for i, e in enumerate(engines[:4]))
    recs = all_records(engines[4], 2 * G)
    for e in engines:
        e.close()
    n_fast = 0
    for key, a in plain.items():
        for other in (zero, back, plies):
            b = other[key]
            assert all(x.tobytes() == y.tobytes() and x.shape == y.shape for x, y in zip(a[1:4], b[1:4])), (name, feature, key)
            assert np.array_equal(a[0][[0, 1, 2, 3, 5]], b[0][[0, 1, 2, 3, 5]]), (name, feature, key)      # (the first row depends on the batch)
        keep = np.flatnonzero(recs[key]["move_kind"] != 2)
        np.testing.assert_array_equal(plies[key][4], keep.astype(np.uint8)); assert a[4] is None
        n_fast += recs[key]["T"] - len(keep)
    assert (n_fast > 0) == bool(CASES[name][3])
    return n_fast


def switch_case(oracle, name, lib_path):
    """the mode switched between two drains of ONE engine: the games of the first drain are the model's at lambda 0.5, those handed out after
    the switch the plain rows, and after switching back the model's at lambda 1"""
    game, G, _, _, _, _, _, seed = CASES[name]
    host, dev = make_engine(name, lib_path, games_per_slot=3), make_engine(name, lib_path, games_per_slot=3)
    recs = all_records(host, 3 * G)
    host.close()
    for _ in range(40000):
        dev.run_waves(32); dev.synchronize()
        if dev.stats()["game_stats"][2] >= 3 * G:
            break
    phases = []
    for lam, take in ((0.5, G), (0.0, G), (1.0, 3 * G)):
        dev.set_sample_weighting(lam)
        out = {}
        split_batch(dev.drain_samples(max_games=take, with_plies=True), out)
        phases.append((lam, out))
    dev.close()
    assert [len(o) for _, o in phases] == [G, G, G] and len({k for _, o in phases for k in o}) == 3 * G
    for lam, out in phases:
        for key, got in out.items():
            if lam:
                assert_game_equals_model(oracle, game, recs[key], got, lam, seed, f"switch {lam} {key}")
            else:
                b, p, v = M.every_row(game_class(game), recs[key])
                keep = recs[key]["move_kind"] != 2
                assert got[1].tobytes() == b[:, keep].tobytes() and got[2].tobytes() == p[:, keep].tobytes() and got[3].tobytes() == v[:, keep].tobytes()
                assert int(got[0][5]) == int((~keep).sum())


def conservation_case(oracle, lib_path, games=256, G=64):
    """256 TicTacToe games with the cap on, lambda 0.5: per game |rows - n_full| <= |E|, and the total is the model's total"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    mk = lambda: SelfPlayEngine("TicTacToe", G, 24, 9, 3, 2, 1.25, 1.0, seed=5, hash_salt=4, ring_capacity=4 * G, games_budget=games, fast_iterations=6,   # noqa: E731
                                full_search_prob=0.25, lib_path=lib_path)
    host, dev = mk(), mk()
    dev.set_sample_weighting(0.5, FAST_FACTOR)
    recs, got = all_records(host, games), all_samples(dev, games)
    host.close(); dev.close()
    total = want_total = n_full = 0
    for key, rec in recs.items():
        c, m = M.row_counts(oracle, rec, 0.5, FAST_FACTOR, 5)
        rows = got[key][1].shape[1]
        assert rows == int(c.sum()) and abs(rows - m["n_full"]) <= int(m["E"].sum()), key
        np.testing.assert_array_equal(got[key][4], np.repeat(np.arange(len(c)), c))
        total += rows; want_total += int(c.sum()); n_full += m["n_full"]
    assert total == want_total
    print(f"conservation: {games} games, {total} rows for {n_full} full plies", flush=True)
    return total, n_full


# ------------------------------------------------------------------------------------------------ degenerate records
class FirstLegal:
    """policy = 1.0 on the first legal action, value 0.  With no root noise P is one-hot, so the only term of a ply's surprise is
    pi[a] (log pi[a] - log 1) <= 0 (the search still visits every child once): every s_p is 0"""

    def __init__(self, A):
        self.A = A

    def many(self, states):
        from degenerate_eval import legal_masks
        legal = legal_masks(states, self.A)
        pol = np.zeros(legal.shape, np.float32)
        pol[np.arange(legal.shape[0]), legal.argmax(1)] = 1.0
        return pol, np.zeros(legal.shape[0], np.float32)


def degenerate_case(oracle, kind, lib_path, game="TicTacToe", G=8):
    """external evaluators, no root noise, cap on.  "first-legal" (games of three plies, every P one-hot): S == 0 in every game, so w = w0 and
    the rows are the plain ones.
    "zeros" (tests/degenerate_eval.py): plies with pi[a] > 0 where P[a] == 0 — the term is left out, the sum stays finite"""
    from degenerate_cases import serve_wave
    from degenerate_eval import Evaluator
    from grok_alpha_zero_amd.engine import EVAL_EXTERNAL, SelfPlayEngine
    seed, lam = 13, 0.5
    mk = lambda: SelfPlayEngine(game, G, 24, 3 if kind == "first-legal" else MAXT[game], 0, 0, 1.25, 1.0, seed=seed, use_dirichlet=False, evaluator=EVAL_EXTERNAL, ring_capacity=4 * G,   # noqa: E731
                                games_budget=G, fast_iterations=6, full_search_prob=0.5, lib_path=lib_path)
    host, dev = mk(), mk()
    dev.set_sample_weighting(lam, FAST_FACTOR)
    evs = [FirstLegal(A_OF[game]) if kind == "first-legal" else Evaluator(kind, A_OF[game]) for _ in range(2)]

    def serve(eng, ev):
        def advance():
            for _ in range(8):
                serve_wave(eng, ev)
        return advance
    recs, got = all_records(host, G, advance=serve(host, evs[0])), all_samples(dev, G, advance=serve(dev, evs[1]))
    host.close(); dev.close()
    zero_prior_terms = plain_games = 0
    for key, rec in recs.items():
        want = assert_game_equals_model(oracle, game, rec, got[key], lam, seed, f"{kind} {key}")
        m = want["m"]
        zero_prior_terms += int(((rec["policies"] > 0) & (rec["root_P"] == 0)).sum())
        if m["S"] == 0.0:
            plain_games += 1
            np.testing.assert_array_equal(want["c"], (rec["move_kind"] == 1).astype(np.int64))
        assert np.isfinite(m["s"]).all()
    if kind == "first-legal":
        assert plain_games == G and any((r["move_kind"] == 2).any() for r in recs.values()), plain_games
    else:
        assert zero_prior_terms > 0
    return plain_games, zero_prior_terms


def short_games_case(oracle, lib_path):
    """a game of ONE ply (max_actions = 1); games whose plies after the first are all fast (full_search_prob tiny: the first move of a game
    is always full); and a set_position prefix, whose plies (kind 0) keep one row each and take no part"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    seed, lam, G = 9, 0.5, 8
    out = {}
    for what, max_actions, p, prefix in (("one-ply", 1, 0.5, None), ("fast-tail", 42, 1e-9, None), ("prefix", 42, 0.25, [3, 3, 2, 4, 2])):
        mk = lambda: SelfPlayEngine("Connect4", G, 40, max_actions, 3, 2, 2.5, 0.5, seed=seed, hash_salt=6, ring_capacity=4 * G, games_budget=G,   # noqa: E731
                                    fast_iterations=8, full_search_prob=p, lib_path=lib_path)
        host, dev = mk(), mk()
        dev.set_sample_weighting(lam, FAST_FACTOR)
        for g in range(G if prefix else 0):
            host.set_position(g, prefix); dev.set_position(g, prefix)
        recs, got = all_records(host, G), all_samples(dev, G)
        host.close(); dev.close()
        for key, rec in recs.items():
            want = assert_game_equals_model(oracle, "Connect4", rec, got[key], lam, seed, f"{what} {key}")
            if what == "one-ply":
                assert rec["T"] == 1
            if what == "fast-tail":
                assert rec["move_kind"][0] == 1 and (rec["move_kind"][1:] == 2).all() and rec["T"] > 1 and want["m"]["n_full"] == 1
            if what == "prefix":
                assert (rec["move_kind"][:5] == 0).all() and (want["c"][:5] == 1).all() and (rec["move_kind"][5:] != 0).all()
        out[what] = len(recs)
    return out


# ------------------------------------------------------------------------------------------------ capacity
def capacity_case(oracle, lib_path, name="c4-on"):
    """max_rows exactly a game's weighted rows, one below it (the error, and nothing is lost), 2 * max_T (always progress), max_games cuts,
    and drain_finished mixed in: every game is handed out once and equals the model"""
    from grok_alpha_zero_amd.engine import EngineError
    game, G, _, _, _, _, lam, seed = CASES[name]
    host, dev = make_engine(name, lib_path), make_engine(name, lib_path)
    dev.set_sample_weighting(lam, FAST_FACTOR)
    recs = all_records(host, 2 * G)
    host.close()
    for _ in range(40000):
        dev.run_waves(32); dev.synchronize()
        if dev.stats()["game_stats"][2] >= 2 * G:
            break
    counts = {k: int(M.row_counts(oracle, r, lam, FAST_FACTOR, seed)[0].sum()) for k, r in recs.items()}
    seen, out = {}, {}
    # max_rows = 0 takes the oldest game only if all its counts are 0 (short games, few full plies); else the refusal names its rows
    need = None
    while need is None:
        try:
            b = dev.drain_samples(max_rows=0, max_games=1, with_plies=True)
            assert b.n == 1 and b.rows == 0 and counts[(int(b.games[0, 2]), int(b.games[0, 3]))] == 0 and int(b.games[0, 5]) == int(b.games[0, 0])
            split_batch(b, out)
        except EngineError as e:
            need = int(str(e).split(" has ")[1].split(" rows")[0])
            assert need >= 1 and need in counts.values() and "max_rows is 0" in str(e), str(e)
    try:
        dev.drain_samples(max_rows=need - 1)
        raise AssertionError("a drain one row short was not refused")
    except EngineError as e:
        assert f"has {need} rows" in str(e) and f"max_rows is {need - 1}" in str(e) and "2 * max_T" in str(e), str(e)
    b = dev.drain_samples(max_rows=need, max_games=1, with_plies=True)
    assert b.n == 1 and b.rows == need == counts[(int(b.games[0, 2]), int(b.games[0, 3]))]
    split_batch(b, out)
    b = dev.drain_samples(max_rows=2 * MAXT[game], max_games=2, with_plies=True)      # always progress
    assert b.n == 2 and b.rows <= 2 * MAXT[game]
    split_batch(b, out)
    b = dev.drain_samples(max_games=3, with_plies=True)
    assert b.n == 3
    split_batch(b, out)
    mixed = dev.drain_finished(max_records=2)                                         # two games leave as records
    assert len(mixed) == 2
    for r in mixed:
        seen[(r["slot"], r["game_seq"])] = r
    split_batch(dev.drain_samples(with_plies=True), out)
    dev.close()
    assert not set(seen) & set(out) and len(seen) + len(out) == 2 * G
    for key, got in out.items():
        assert got[1].shape[1] == counts[key]
        assert_game_equals_model(oracle, game, recs[key], got, lam, seed, f"capacity {key}")
    for key, r in seen.items():
        np.testing.assert_array_equal(r["policies"], recs[key]["policies"])
    return len(out)


def groups_case(oracle, lib_path, name="c4-on", G=32):
    """two game groups: the rings are visited in turn, rows and plies land at the running offsets"""
    game, _, _, _, _, _, lam, seed = CASES[name]
    host, dev = make_engine(name, lib_path, G, game_groups=1), make_engine(name, lib_path, G, game_groups=2)
    assert dev.stats()["game_groups"] == 2
    dev.set_sample_weighting(lam, FAST_FACTOR)
    assert dev.sample_weighting == (lam, FAST_FACTOR)
    recs, got = all_records(host, 2 * G), all_samples(dev, 2 * G, max_games=5)
    host.close(); dev.close()
    for key, rec in recs.items():
        assert_game_equals_model(oracle, game, rec, got[key], lam, seed, f"groups {key}")


# ------------------------------------------------------------------------------------------------ refusals, run_self_play
REFUSALS = {   # name -> (lambda, fast_factor), what the message must say
    "lambda-negative": ((-0.1, 1.5), "lambda must be in [0, 1]"), "lambda-above-one": ((1.5, 1.5), "lambda must be in [0, 1]"),
    "lambda-nan": ((float("nan"), 1.5), "lambda must be in [0, 1]"), "factor-zero": ((0.5, 0.0), "fast_factor must be a finite number above 0"),
    "factor-negative": ((0.5, -1.0), "fast_factor must be a finite number above 0"), "factor-nan": ((0.5, float("nan")), "fast_factor must be a finite number above 0"),
    "factor-inf": ((0.5, float("inf")), "fast_factor must be a finite number above 0"),
}


def refusal_case(lib_path):
    """every refusal by its text: from the library (the C entry point, called directly) and from the Python method (ValueError); the
    Gumbel engine; and a refused call leaves the mode as it was"""
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL, SelfPlayEngine
    eng = SelfPlayEngine("Connect4", 4, 40, 42, 3, 2, 2.5, 0.5, seed=1, lib_path=lib_path)
    eng.set_sample_weighting(0.25, 2.0)
    msgs = {}
    for name, ((lam, ff), text) in REFUSALS.items():
        assert eng.L.gaz_engine_set_sample_weighting(eng.h, lam, ff) != 0, name
        msgs[name] = eng.L.gaz_engine_last_error(eng.h).decode()
        assert text in msgs[name] and msgs[name].startswith("set_sample_weighting:"), (name, msgs[name])
        try:
            eng.set_sample_weighting(lam, ff)
            raise AssertionError(f"{name}: accepted")
        except ValueError as e:
            assert text in str(e), (name, str(e))
        assert eng.sample_weighting == (0.25, 2.0)
    eng.close()
    g = SelfPlayEngine("Connect4", 4, 32, 42, 0, 0, 0.0, 0.0, seed=1, search=SEARCH_GUMBEL, gumbel_m=4, lib_path=lib_path)
    msgs["gumbel"] = refusal_message(lambda: g.set_sample_weighting(0.5), "a Gumbel engine accepted the mode")
    assert "not with the Gumbel search" in msgs["gumbel"] and g.sample_weighting == (0.0, 1.5)
    g.close()
    msgs["gumbel-create"] = refusal_message(lambda: SelfPlayEngine("Connect4", 4, 32, 42, 0, 0, 0.0, 0.0, seed=1, search=SEARCH_GUMBEL, gumbel_m=4, sample_weighting=(0.5, 1.5),
                                                                   lib_path=lib_path).close(), "a Gumbel engine was created with the mode")
    assert "not with the Gumbel search" in msgs["gumbel-create"]
    return msgs


def run_self_play_case(oracle, tmp, lib_path, games=24, G=8):
    """run_self_play with policy_surprise_weight / policy_surprise_fast_factor: the replay file's datasets, at both settings of
    device_samples, are the model's rows of the records of an engine created with the same settings; game_stats count every ply"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    from selfplay_support import games_of_file, self_play_file
    lam, ff, seed = 0.5, 1.25, 11
    train = dict(games_per_generation=games, MCTS_iteration_limit=16, MCTS_fast_iteration_limit=4, full_search_prob=0.3, max_actions=9,
                 num_explore_actions_first=2, num_explore_actions_second=1, c_puct_init=1.25, dirichlet_alpha=1.0, policy_surprise_weight=lam,
                 policy_surprise_fast_factor=ff)
    out = {ds: self_play_file(tmp, f"ds{ds}", "TicTacToe", train, games, n_games=G, seed=seed, hash_salt=4, lib_path=lib_path, device_samples=ds)
           for ds in (False, True)}
    eng = SelfPlayEngine("TicTacToe", G, 24, 9, 2, 1, 1.25, 1.0, seed=seed, hash_salt=4, ring_capacity=4 * G, games_budget=games, fast_iterations=6,
                         full_search_prob=0.3, lib_path=lib_path)
    recs = all_records(eng, games)
    eng.close()
    want = []
    for rec in recs.values():
        w = M.expected(oracle, game_class("TicTacToe"), rec, lam, ff, seed)
        want.append(tuple((a.dtype.str, a.shape, a.tobytes()) for j in range(8) for a in (w["boards"][j], w["policies"][j], w["values"][j])))
    plies = sum(r["T"] for r in recs.values())
    for ds in (False, True):
        f = out[ds]
        gs = f["game_stats"]
        assert len(f) == 1 + 3 * 8 * games and gs[2] == games and gs[1] == plies, (ds, gs, plies)
        assert games_of_file(f, games, 8) == sorted(want), f"device_samples={ds}"
    return plies


# ------------------------------------------------------------------------------------------------ the sanitizer driver
def build_driver():
    """tests/emu/surprise_main.cpp with the engine's host code and the one-lane build of its device code as ONE program under the address and
    undefined-behaviour sanitizers, the runtimes linked statically (the flags of tests/emu/Makefile's capacity_asan): run directly, on the
    CPU, never loaded into Python"""
    import os
    import subprocess
    from selfplay_support import EMU_DIR, ROOT
    csrc, out = os.path.join(ROOT, "grok_alpha_zero_amd", "csrc"), os.path.join(EMU_DIR, "surprise_asan")
    srcs = [os.path.join(csrc, "engine.hip"), os.path.join(EMU_DIR, "emu_stubs.cpp"), os.path.join(EMU_DIR, "surprise_main.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")] + [os.path.join(ROOT, "include", "gaz_engine.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DGAZ_HOST_EMU", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-x", "c++"] + srcs + ["-o", out])
    return out


DRIVER_CASES = {   # name -> the program's arguments
    "c4": dict(game="Connect4", n_games=8, games=16, run_iterations=30, fast_iterations=6, max_actions=42, seed=3), "c4-lambda1": dict(game="Connect4", games=12, seed=4) | {"lambda": 1},
    "ttt-cap-off": dict(game="TicTacToe", n_games=8, games=24, run_iterations=20, fast_iterations=0, max_actions=9, seed=5),
    "gmk": dict(game="Gomoku", n_games=4, games=8, run_iterations=24, fast_iterations=8, max_actions=14, seed=6),
}


def run_driver(driver, name):
    import subprocess
    r = subprocess.run([driver] + [f"{k}={v}" for k, v in DRIVER_CASES[name].items()], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------ the network in the loop (HIP build)
def network_case(G=64, lam=0.5, seed=31):
    """Connect4 with the 1-block network: fused launch, two game groups, evaluation cache on, the cap on.  The weighted drain's bytes ==
    record_to_samples(weighting=...) on the drain_finished records of a twin engine"""
    from grok_alpha_zero_amd.self_play import record_to_samples
    from selfplay_support import c4_one_block_weights, net_engine
    w = c4_one_block_weights()
    kw = dict(seed=seed, fast_iterations=8, full_search_prob=0.25, game_groups=2, eval_cache_log2=14)
    host, dev = net_engine(G, w, **kw), net_engine(G, w, **kw)
    dev.set_sample_weighting(lam, FAST_FACTOR)
    recs, got = all_records(host, G), all_samples(dev, G)
    st = dev.stats()
    host.close(); dev.close()
    assert st["fused_wave"] == 1 and st["game_groups"] == 2 and st["cache_hits"] > 0, st
    rows = fast_rows = 0
    for key, rec in recs.items():
        hb, hp, hv, T = record_to_samples(game_class("Connect4"), rec, weighting=(lam, FAST_FACTOR, seed))
        row, b, p, v, plies = got[key]
        assert b.tobytes() == hb.tobytes() and p.tobytes() == hp.tobytes() and v.tobytes() == hv.tobytes() and int(row[0]) == T, key
        rows += len(plies); fast_rows += int((rec["move_kind"][plies] == 2).sum())
    assert fast_rows > 0
    print(f"network: {G} games, {rows} rows, {fast_rows} of fast plies, {st['cache_hits']} cache hits", flush=True)

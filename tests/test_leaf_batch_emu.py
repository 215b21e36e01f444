"""CPU suite: the leaf-batched PUCT search (gaz_engine_config.leaf_batch = K) on the emulation build of the device code against the
test model of tests/leaf_batch_model.py, which is itself anchored to the oracle at K = 1.  Bit-equal everywhere: no tolerance."""
import numpy as np
import pytest

from leaf_batch_model import WIN as WIN_CHILD, Tree, selfplay_moves
from selfplay_support import A_OF, MAXT, emu_lib  # noqa: F401 (emu_lib: a fixture)


# ------------------------------------------------------------------------------------------------ 1. the model is sound
def _model_equals_oracle(oracle, game, iters, seed, salt, c_init, alpha, plies=None, explore=(3, 3)):
    o = oracle.selfplay_game(game, iters, MAXT[game], explore[0], explore[1], c_init, alpha, seed, 0, 0, hash_salt=salt)
    T = o["T"] if plies is None else min(plies, o["T"])
    m = selfplay_moves(oracle, game, 1, seed, iters, o["actions"][:T], c_puct_init=c_init, dirichlet_alpha=alpha, hash_salt=salt)
    assert len(m) == T
    for ply in range(T):
        for k, ok in (("N", "root_N"), ("W", "root_W"), ("P", "root_P")):
            np.testing.assert_array_equal(m[ply][k], o[ok][ply], err_msg=f"{game} seed {seed} ply {ply} {k}")
        assert m[ply]["root_visits"] == o["root_visits"][ply] and m[ply]["evals"] == o["evals"][ply], (game, seed, ply)
    return o, m


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("game,iters,c_init,alpha", [("TicTacToe", 40, 1.25, 1.0), ("Connect4", 60, 2.5, 0.5)])
def test_model_k1_equals_oracle_whole_games(oracle, game, iters, c_init, alpha, seed):
    """K = 1 of the model = oracle.selfplay_game on every ply of whole games (fed the oracle's moves).  The games reach terminal
    parents: asserted on evals < simulations somewhere (a simulation that ends at a terminal leaf or creates a terminal parent needs
    no evaluator call)."""
    o, m = _model_equals_oracle(oracle, game, iters, seed, 11 + seed, c_init, alpha)
    assert any(int(o["evals"][p]) < iters for p in range(o["T"])), "no terminal parent in this game"


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_k1_equals_oracle_gomoku(oracle, seed):
    _model_equals_oracle(oracle, "Gomoku", 3 * 225, seed, 5, 2.5, 0.05, plies=6)


# ------------------------------------------------------------------------------------------------ 2. leaf_batch = 1 is the default
def test_leaf_batch_1_is_the_default_path(emu_lib):
    from grok_alpha_zero_amd.engine import SelfPlayEngine

    def play(**kw):
        eng = SelfPlayEngine("Connect4", 8, 40, 42, 4, 4, 2.5, 0.5, seed=9, hash_salt=3, ring_capacity=16, games_budget=8, lib_path=emu_lib, **kw)
        raw = []
        for _ in range(4000):
            eng.run_waves(32)
            lay = eng.layout
            buf = np.zeros((16, lay.record_bytes), np.uint8)
            import ctypes as C
            n = C.c_int32()
            eng._ck(eng.L.gaz_engine_drain_finished(eng.h, buf.ctypes.data, 16, C.byref(n)))
            raw += [buf[i].tobytes() for i in range(n.value)]
            if len(raw) == 8:
                break
        waves = eng.stats()["waves"]
        eng.close()
        assert len(raw) == 8
        return sorted(raw), waves
    a, wa = play()
    b, wb = play(leaf_batch=1)
    c, wc = play(leaf_batch=0)
    assert a == b == c and wa == wb == wc


# ------------------------------------------------------------------------------------------------ 3. + 4. engine versus model
def _drive_move(eng, oracle, game, salt):
    """One MCTS.run of a sync + single-tree engine with the external evaluator: -> per launch the list of (row, state) requested."""
    from grok_alpha_zero_amd.engine import PH_WAIT_HOST, PH_HALT
    A = A_OF[game]
    eng.start_search()
    launches = []
    for _ in range(100000):
        eng.wave_begin()
        x, pend = eng.read_batch()
        rows = np.flatnonzero(pend)
        launches.append([(int(r), x[r].copy()) for r in rows])
        # the engine's own reserved counts (NodeHdr::pad[0] summed over every node, stats()["reserved_children"]): one per requested leaf
        # (a root request, pending = 1, reserves nothing) — so 0 in the launch that ends the move
        assert eng.stats()["reserved_children"] == int(np.count_nonzero(pend == 2)), len(launches)
        if rows.size == 0 and eng.root_stats()["phase"][0] in (PH_WAIT_HOST, PH_HALT):
            return launches
        pol = np.zeros((eng.batch_rows, A), np.float32); val = np.zeros(eng.batch_rows, np.float32)
        for r in rows:
            pol[r], val[r] = oracle.hash_eval(x[r], A, salt)
        eng.write_outputs(pol, val)
    raise AssertionError("search did not finish")


def _engine_vs_model(emu_lib, oracle, game, K, iters, moves, *, use_dirichlet, seed=7, salt=4, history=(), max_tree_sims=4, c_init=2.5, alpha=0.5,
                     compact_trees=-1):
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_EXTERNAL
    # (compact_trees = 0: the engine's defaults — Gomoku re-roots with compaction into an arena of the default size)
    eng = SelfPlayEngine(game, 1, iters, MAXT[game], 0, 0, c_init, alpha, seed=seed, use_dirichlet=use_dirichlet, sync_moves=True, single_tree=True,
                         evaluator=EVAL_EXTERNAL, nodes_per_tree=(len(moves) + 1) * (max(iters, 3 * A_OF[game]) + 4) + 64 if compact_trees else 0,
                         compact_trees=compact_trees,
                         max_tree_sims_per_wave=max_tree_sims, tau=0.0, leaf_batch=K, lib_path=emu_lib)
    assert eng.batch_rows == K and eng.stats()["fused_wave"] == 0 and eng.stats()["game_groups"] == 1
    eng.set_position(0, list(history))
    model = Tree(oracle, game, K, seed, c_puct_init=c_init, dirichlet_alpha=alpha, use_dirichlet=use_dirichlet, hash_salt=salt,
                 max_tree_sims=max_tree_sims, history=history)
    widest = 0
    for m in list(moves) + [None]:
        got = _drive_move(eng, oracle, game, salt)
        want = model.run(iters)
        # the launches of the move: as many as the model's, and in each the same rows (j = 0 .. n-1 of game 0) with the same states
        assert len(got) == len(want["launches"]), (game, K, len(got), len(want["launches"]))
        for k, (g_l, w_l) in enumerate(zip(got, want["launches"])):
            assert [r for r, _ in g_l] == list(range(len(w_l))), (game, K, k)
            for (_, gs), ws in zip(g_l, w_l):
                np.testing.assert_array_equal(gs, ws, err_msg=f"{game} K {K} launch {k}")
            widest = max(widest, len(w_l))
        st = eng.root_stats()
        np.testing.assert_array_equal(st["N"][0], want["N"]); np.testing.assert_array_equal(st["W"][0], want["W"])
        np.testing.assert_array_equal(st["P"][0], want["P"])
        assert int(st["root_visits"][0]) == want["root_visits"]
        # 4.: nothing is left in flight, in the engine's node records (every launch was checked in _drive_move; once more after the move) and in the model
        assert eng.stats()["reserved_children"] == 0 and model.inflight_nodes() == 0
        if m is None:
            break
        eng.apply_moves([m]); model.play(m)
    eng.close()
    return widest


GAME_CASES = [("TicTacToe", 30, [4, 0, 8, 2], 1.25, 1.0), ("Connect4", 120, [3, 3, 2, 4, 3], 2.5, 0.5), ("Gomoku", 3 * 225 + 40, [112, 113, 97, 127], 2.5, 0.05)]


@pytest.mark.parametrize("use_dirichlet", [True, False])
@pytest.mark.parametrize("K", [2, 4, 8, 16])
@pytest.mark.parametrize("game,iters,moves,c_init,alpha", GAME_CASES, ids=[c[0] for c in GAME_CASES])
def test_engine_equals_model(emu_lib, oracle, game, iters, moves, c_init, alpha, K, use_dirichlet):
    widest = _engine_vs_model(emu_lib, oracle, game, K, iters, moves, use_dirichlet=use_dirichlet, c_init=c_init, alpha=alpha)
    assert widest > 1, "no launch carried more than one leaf"


WIN_IN_ONE = {   # history, the moves the host plays afterwards (none of them ends the game, and the three in a column stay open)
    "first-player-wins-in-one": ([3, 0, 3, 0, 3, 1], [2, 4, 5, 1]),          # the first player, to move, holds three in column 3
    "second-player-wins-in-one": ([0, 3, 1, 3, 2, 3, 6], [4, 5, 1, 0]),      # the second player, to move, holds three in column 3
}


@pytest.mark.parametrize("K", [2, 4, 8, 16])
@pytest.mark.parametrize("case", sorted(WIN_IN_ONE))
def test_engine_equals_model_win_in_one(emu_lib, oracle, K, case):
    """Connect4, the side to move has a win in one: the first search runs on a terminal root (64-at-once path); the host then plays
    something else, so the other side searches under that threat (terminal parents below the root), and so on in turn."""
    history, moves = WIN_IN_ONE[case]
    model = Tree(oracle, "Connect4", K, 7, history=history)
    assert model.root.terminal and model.next_player == (-1 if len(history) % 2 == 0 else 1) and WIN_CHILD in model.root.child
    _engine_vs_model(emu_lib, oracle, "Connect4", K, 90, moves, use_dirichlet=True, history=history)


def test_engine_equals_model_gomoku_compacting_trees(emu_lib, oracle):
    """Gomoku with the engine's defaults: the tree arena is double-buffered and every re-root compacts the kept subtree into the other
    half (the step then works on its state in global memory), after leaf-batched moves."""
    widest = _engine_vs_model(emu_lib, oracle, "Gomoku", 8, 3 * 225 + 40, [112, 113, 97, 127], use_dirichlet=True, c_init=2.5, alpha=0.05, compact_trees=0)
    assert widest > 1


def test_engine_equals_model_more_tree_sims(emu_lib, oracle):
    _engine_vs_model(emu_lib, oracle, "Connect4", 8, 150, [2, 4, 5, 1], use_dirichlet=True, history=[3, 0, 3, 0], max_tree_sims=32)


def test_no_inflight_counts_and_root_visits_after_every_move(emu_lib, oracle):
    """After every move, at K = 8 exactly as at K = 1 (same position, same iteration count): every virtual loss is gone (|W| <= N on
    every root child) and no node record of any game holds a reserved count; root_visits >= the visits the re-root carried over + one per simulation of the move (terminal parents add more
    than one); and sum(N of the root's children) lies between the simulations of the move and root_visits."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    for K in (1, 8):
        eng = SelfPlayEngine("Connect4", 4, 80, 42, 0, 0, 2.5, 0.5, seed=21, hash_salt=2, sync_moves=True, single_tree=True, leaf_batch=K, lib_path=emu_lib)
        carried = np.zeros(4, np.int64)
        for mv in (3, 2, 3, 4, 1):
            eng.start_search(); eng.run_move()
            st = eng.root_stats()
            N, W, rv = st["N"].astype(np.int64), st["W"], st["root_visits"].astype(np.int64)
            assert (np.abs(W) <= N).all() and eng.stats()["reserved_children"] == 0
            assert (N.sum(1) >= 80).all() and (rv >= carried + 80).all() and (N.sum(1) <= rv).all(), (K, N.sum(1), rv, carried)
            carried = N[:, mv]
            eng.apply_moves([mv] * 4)
        eng.close()


# ------------------------------------------------------------------------------------------------ 5. continuous self-play
def test_selfplay_first_games_equal_model(emu_lib, oracle):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    G, K, iters = 64, 4, 30
    eng = SelfPlayEngine("Connect4", G, iters, 42, 4, 4, 2.5, 0.5, seed=13, hash_salt=6, ring_capacity=4 * G, max_tree_sims_per_wave=4,
                         leaf_batch=K, lib_path=emu_lib)
    first = {}
    for _ in range(4000):
        eng.run_waves(32)
        for r in eng.drain_finished():
            if r["game_seq"] == 0:
                first[r["slot"]] = r
        if len(first) == G:
            break
    assert len(first) == G and eng.stats()["fused_wave"] == 0
    eng.close()
    for slot, r in sorted(first.items()):
        m = selfplay_moves(oracle, "Connect4", K, 13, iters, r["actions"], slot=slot, c_puct_init=2.5, dirichlet_alpha=0.5, hash_salt=6, max_tree_sims=4)
        assert len(m) == r["T"]
        for ply in range(r["T"]):
            np.testing.assert_array_equal(r["root_N"][ply], m[ply]["N"], err_msg=f"slot {slot} ply {ply}")
            np.testing.assert_array_equal(r["root_W"][ply], m[ply]["W"]); np.testing.assert_array_equal(r["root_P"][ply], m[ply]["P"])
            assert r["root_visits"][ply] == m[ply]["root_visits"] and r["evals"][ply] == m[ply]["evals"], (slot, ply)


# ------------------------------------------------------------------------------------------------ 6. refusals
@pytest.mark.parametrize("kw,field", [(dict(search=1, gumbel_m=4), "search"), (dict(eval_cache_log2=10), "eval_cache_log2"),
                                       (dict(game_groups=2), "game_groups"), (dict(leaf_batch=65), "leaf_batch")])
def test_refusals_name_the_field(emu_lib, kw, field):
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EngineError
    args = dict(leaf_batch=4, lib_path=emu_lib); args.update(kw)
    with pytest.raises(EngineError) as e:
        SelfPlayEngine("Connect4", 8, 30, 42, 4, 4, 2.5, 0.5, seed=1, **args)
    assert field in str(e.value) and "leaf_batch" in str(e.value)


def test_repack_refused_and_groups_resolve_to_one(emu_lib):
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EngineError
    eng = SelfPlayEngine("Connect4", 8, 30, 42, 4, 4, 2.5, 0.5, seed=1, games_budget=8, leaf_batch=4, lib_path=emu_lib)
    assert eng.stats()["game_groups"] == 1 and eng.stats()["fused_wave"] == 0 and eng.batch_rows == 32
    with pytest.raises(EngineError, match="leaf_batch"):
        eng.repack()
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. the MCTS class
class _CountingSession:
    def __init__(self, oracle, A, salt):
        self.oracle, self.A, self.salt = oracle, A, salt
        self.batches, self.rows = [], []

    def run(self, output_names, input_feed):
        x = input_feed["inputs"]
        assert x.ndim == 4 and x.dtype == np.float32 and output_names == ["policy", "value"]
        self.batches.append(x.shape[0])
        out = [self.oracle.hash_eval(r.astype(np.int8), self.A, self.salt) for r in x]
        self.rows += [r.astype(np.int8) for r in x]
        return np.stack([p for p, _ in out]), np.array([[v] for _, v in out], np.float32)


@pytest.mark.parametrize("game,iters,moves", [("TicTacToe", 30, [4, 0]), ("Connect4", 100, [3, 2, 3])])
def test_mcts_class_batches_its_session_calls(emu_lib, oracle, game, iters, moves):
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.mcts import MCTS
    K, A, salt, seed = 8, A_OF[game], 17, 5
    g = GAMES[game]()
    sess = _CountingSession(oracle, A, salt)
    mcts = MCTS(g, sess, c_puct_init=2.5, dirichlet_alpha=0.5, tau=0.0, seed=seed, leaf_batch=K, lib_path=emu_lib)
    model = Tree(oracle, game, K, seed, c_puct_init=2.5, dirichlet_alpha=0.5, hash_salt=salt, max_tree_sims=4)
    for m in list(moves) + [None]:
        n0 = len(sess.rows)
        move, rows = mcts.run(iteration_limit=iters, use_bar=False)
        w = model.run(iters)
        # the returned rows [action, N / sum N, W / N, W, N, P, root.visits, is_terminal], sorted by visits: the model's root, by action
        assert [r[4] for r in rows] == sorted((r[4] for r in rows), reverse=True) and len(rows) == int(np.count_nonzero(w["P"]))
        for r in rows:
            a = GAMES[game].action_to_index(r[0])
            assert (r[4], r[3], r[5], r[6]) == (w["N"][a], w["W"][a], w["P"][a], w["root_visits"]), (game, a)
            assert r[1] == w["N"][a] / float(w["N"].sum()) and r[2] == float(w["W"][a]) / float(w["N"][a])
        assert w["N"][GAMES[game].action_to_index(move)] == w["N"].max()          # tau = 0: a most visited move
        want = [s for l in w["launches"] for s in l]
        got = sess.rows[n0:]
        assert len(got) == len(want)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
        st = mcts._eng.root_stats()
        np.testing.assert_array_equal(st["N"][0], w["N"]); np.testing.assert_array_equal(st["W"][0], w["W"])
        np.testing.assert_array_equal(st["P"][0], w["P"])
        assert int(st["root_visits"][0]) == w["root_visits"]
        if m is None:
            break
        act = GAMES[game].index_to_action(m)
        g.do_action(act); mcts.prune_tree(act); model.play(m)
    assert max(sess.batches) > 1 and sum(sess.batches) == len(sess.rows) == mcts._eng.stats()["evals"] == model.n_evals
    mcts.close()
    with pytest.raises(TypeError):
        from grok_alpha_zero_amd.mcts import MCTS_Gumbel
        MCTS_Gumbel(GAMES[game](), None, leaf_batch=4, lib_path=emu_lib)


# ------------------------------------------------------------------------------------------------ run_self_play passes it through
def test_run_self_play_passes_leaf_batch_through(emu_lib, oracle, tmp_path):
    """run_self_play(leaf_batch=4) with its default eval_cache_log2 (forced off: the engine would refuse the pair) and 20 slots for 26
    games, so that the generation's tail reaches the point where run_self_play repacks (refused with leaf batching: it must not try).
    The file's counters equal those of an engine created with leaf_batch = 4 directly, and the games are the model's search (one replayed)."""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import ReplayStore, run_self_play
    folder = str(tmp_path / "Grok_Zero_Train" / "0")
    store = ReplayStore(folder); store.create()
    train = dict(games_per_generation=26, MCTS_iteration_limit=20, max_actions=9, num_explore_actions_first=2, num_explore_actions_second=1,
                 c_puct_init=1.25, dirichlet_alpha=1.0, use_gumbel=False)
    es = {}
    assert run_self_play(GAMES["TicTacToe"], ({}, train), folder, n_games=20, seed=11, hash_salt=4, lib_path=emu_lib, engine_stats=es, leaf_batch=4) == 26
    assert es["cache_hits"] == 0 and es["fused_wave"] == 0 and es["reserved_children"] == 0
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine("TicTacToe", 20, 30, 9, 2, 1, 1.25, 1.0, seed=11, hash_salt=4, ring_capacity=80, games_budget=26, leaf_batch=4, lib_path=emu_lib)
    recs = []
    for _ in range(2000):
        eng.run_waves(16); recs += eng.drain_finished()
        if len(recs) == 26:
            break
    st = eng.stats(); eng.close()
    assert len(recs) == 26 and (es["evals"], es["sims"], es["plies"]) == (st["evals"], st["sims"], st["plies"])
    gs = store.game_stats()
    winners = [r["winner"] for r in recs]
    assert gs[2] == 26 and gs[1] == sum(r["T"] for r in recs) and [gs[3], gs[4], gs[5]] == [winners.count(-1), winners.count(0), winners.count(1)]
    r = min(recs, key=lambda r: (r["slot"], r["game_seq"]))                      # and those games are the model's: slot 0, first game
    m = selfplay_moves(oracle, "TicTacToe", 4, 11, 30, r["actions"], slot=r["slot"], c_puct_init=1.25, dirichlet_alpha=1.0, hash_salt=4)
    for ply in range(r["T"]):
        np.testing.assert_array_equal(r["root_N"][ply], m[ply]["N"]); np.testing.assert_array_equal(r["root_W"][ply], m[ply]["W"])

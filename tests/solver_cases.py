"""The cases of the solver (gaz_engine_set_solver) that the CPU suite runs on the emulation build
(tests/test_solver_emu.py) and the -m gpu suite on the HIP build (tests/test_solver_gpu.py): `lib_path` = the emulation library, or None
for the product library.

What a search must give is computed HERE by tests/solver_model.py (SolverTree), never read back from the engine under test, and every
status the engine exports is held against solver_model.minimax, which shares nothing with the model.  Every comparison is exact.  A case
returns a Witness: what it reached, so that a test can assert that it did not pass vacuously."""
import numpy as np

from selfplay_support import (A_OF, MAXT, RECORD_KEYS, assert_records_equal, c4_one_block_weights, first_games, games_of_file, net_engine, play,
                              refusal_message, scheduling_equalities, self_play_file)

SEED, SALT = 31, 8
PH_WAIT_HOST, PH_HALT = 5, 8
MINIMAX_EMPTY = {"TicTacToe": 9, "Connect4": 14, "Gomoku": 0}     # positions with at most this many empty cells are solved by brute force


class Witness:
    KEYS = ("moves", "proven_nodes", "proven_hits", "masked_levels", "zero_sim_moves", "short_moves", "root_win", "root_draw", "root_loss",
            "restricted_rows", "proven_early", "minimax_checked", "statuses_checked", "deep_proofs")

    def __init__(self, name):
        self.name = name
        for k in self.KEYS:
            setattr(self, k, 0)

    def move(self, w, raw_row):
        self.moves += 1
        self.zero_sim_moves += w["sims"] == 0
        self.short_moves += 0 < w["sims"] < w["limit"]
        self.root_win += w["status"] == 1; self.root_draw += w["status"] == 2; self.root_loss += w["status"] == 3
        self.restricted_rows += not np.array_equal(w["policy"], raw_row)
        self.proven_early += bool(w["proven_early"])

    def trees(self, models):
        self.proven_nodes = sum(m.stats[0] for m in models); self.proven_hits = sum(m.stats[1] for m in models)
        self.masked_levels = sum(m.stats[7] for m in models)

    def __repr__(self):
        return f"{self.name}: " + ", ".join(f"{k} {getattr(self, k)}" for k in self.KEYS)


def raw_row(N):
    N = np.asarray(N, np.uint32)
    return (N.astype(np.float64) / float(N.astype(np.uint64).sum())).astype(np.float32)


def c4_prefix(n, seed):
    """n legal Connect4 moves from the empty board after which nobody has won and the mover has no winning move (drawn at random, retried)"""
    from grok_alpha_zero_amd.games import GAMES
    G = GAMES["Connect4"]
    rng = np.random.RandomState(seed)
    for _ in range(10000):
        board, hist, player, ok = np.zeros((6, 7), np.int8), [], -1, True
        for _ in range(n):
            legal = [int(a) for a in G.get_legal_actions_MCTS(board, 0, None)]
            a = int(legal[rng.randint(len(legal))])
            G.do_action_MCTS(board, np.int8(a), player); hist.append(a)
            if int(G.check_win_MCTS(board, player, np.array(hist, np.int8))) != -2:
                ok = False
                break
            player = -player
        if not ok:
            continue
        wins = False
        for a in G.get_legal_actions_MCTS(board, 0, None):
            b = board.copy(); G.do_action_MCTS(b, a, player)
            wins |= int(G.check_win_MCTS(b, player, np.array(hist + [int(a)], np.int8))) != -2
        if not wins:
            return hist
    raise AssertionError("no prefix found")


def replay(game, hist):
    """-> (board, mover) after the action indices `hist`"""
    from grok_alpha_zero_amd.games import GAMES
    G = GAMES[game]
    board, player = np.zeros((G.H, G.W), np.int8), -1
    for a in hist:
        G.do_action_MCTS(board, G.index_to_action(int(a)), player); player = -player
    return board, player


def check_tree(game, tree, model, hist, memo, wit, what):
    """the statuses of an exported tree == the model's, node for node; and every one of them == minimax of the node's position (positions
    with few enough empty cells), the position rebuilt from the export's own actions"""
    from solver_model import minimax
    got = tree.proven
    want = np.asarray(model.statuses(), np.int32)
    np.testing.assert_array_equal(got, want, err_msg=what + " statuses")
    wit.statuses_checked += int(np.count_nonzero(got))
    for i in np.flatnonzero(got):
        if not (int(tree.nodes["flags"][i]) & 1):
            wit.deep_proofs += 1                                        # a propagated proof: at least two plies from the end of the game
        board, mover = replay(game, list(hist) + tree.path_actions(int(i)))
        if int(np.count_nonzero(board == 0)) > MINIMAX_EMPTY[game]:
            continue
        assert int(got[i]) == minimax(game, board, list(hist) + tree.path_actions(int(i)), mover, memo), f"{what} node {i}: status {got[i]} is not the game's value"
        wit.minimax_checked += 1


def compare_move(st, s, w, what):
    for k in ("N", "W", "P", "policy"):
        np.testing.assert_array_equal(st[k][s], w[k], err_msg=f"{what} {k}")
    assert int(st["root_visits"][s]) == w["root_visits"], what
    assert np.float32(st["q"][s]) == w["q"], (what, st["q"][s], w["q"])
    assert int(st["chosen"][s]) == w["chosen"], (what, int(st["chosen"][s]), w["chosen"])


# ------------------------------------------------------------------------------------------------ sync mode against the model
# name -> game, R, prefix (action indices), explore_first / second, c_puct_init, dirichlet_alpha, use_dirichlet, create_new_root, compact, single_tree,
#         plies played at most (None = to the end of the game)
SYNC_CASES = {
    "ttt": ("TicTacToe", 600, [], 0, 0, 1.25, 1.0, True, False, -1, True, None),
    "ttt-two-trees-tau": ("TicTacToe", 600, [], 2, 1, 1.25, 1.0, True, False, -1, False, None),
    "ttt-no-noise-compact": ("TicTacToe", 600, [], 0, 0, 1.25, 1.0, False, False, 1, True, None),
    "ttt-new-root": ("TicTacToe", 600, [], 0, 0, 1.25, 1.0, True, True, -1, True, None),
    "c4-16": ("Connect4", 300, c4_prefix(16, 1), 0, 0, 2.5, 0.5, True, False, -1, True, None),
    "c4-20-two-trees": ("Connect4", 300, c4_prefix(20, 2), 0, 0, 2.5, 0.5, True, False, -1, False, None),
    "c4-24-compact-no-noise": ("Connect4", 300, c4_prefix(24, 3), 0, 0, 2.5, 0.5, False, False, 1, True, None),
    "c4-whole": ("Connect4", 300, [], 2, 2, 2.5, 0.5, True, False, -1, True, None),
    # an open four for the first player (-1) on row 7: O cannot stop both ends, and X to move wins at once
    "gmk-open-four": ("Gomoku", 24, [7 * 15 + 5, 0, 7 * 15 + 6, 1, 7 * 15 + 7, 2, 7 * 15 + 8, 16], 0, 0, 2.5, 0.05, True, False, 1, True, 1),
    # a four with one end blocked: every move of the defender but the block at the other end loses at once, so those slots are left out
    "gmk-four-one-end": ("Gomoku", 24, [7 * 15 + 5, 7 * 15 + 4, 7 * 15 + 6, 0, 7 * 15 + 7, 1, 7 * 15 + 8], 0, 0, 2.5, 0.05, True, False, 1, True, 1),
    "gmk-open-four-defender": ("Gomoku", 24, [7 * 15 + 5, 0, 7 * 15 + 6, 1, 7 * 15 + 7, 2, 7 * 15 + 8], 0, 0, 2.5, 0.05, True, False, 1, True, 2),
}


def tau_on(ply, tree, ef, es):
    """Self_Play's schedule (PH_MOVE_BEGIN)"""
    return (ply % 2 == 0 and ply // 2 < ef) if tree == 0 else ((ply + 1) % 2 == 0 and (ply + 1) // 2 < es)


def sync_case(oracle, name, G, lib_path, slots=None, switch=None, forced_k=0.0, fast=None, eval_symmetry=False, **engine_kw):
    """G games at once in sync mode with the hash evaluator, every game playing the moves its own search chose.  After every move, for the
    compared slots: root N / W / P, policy row, q, chosen move and root visits == SolverTree.run; the statuses of the whole tree
    (read_trees) == the model's and == minimax.  At the end: the records' evals and proven marks, and solver_stats == the model's counts
    (when every slot is compared).  switch = {ply: on}: the solver is switched before those plies (engine and model alike): after the search of the ply before, before its move is applied."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    from solver_model import SolverTree
    game, R, prefix, ef, es, c_init, alpha, noise, new_root, compact, single, max_plies = SYNC_CASES[name]
    slots = tuple(range(G)) if slots is None else tuple(slots)
    switch = dict(switch or {})
    on0 = switch.pop(len(prefix), True) if switch else True
    eng = SelfPlayEngine(game, G, R, MAXT[game], ef, es, c_init, alpha, seed=SEED, hash_salt=SALT, sync_moves=True, single_tree=single,
                         use_dirichlet=noise, create_new_root=new_root, compact_trees=compact, max_tree_sims_per_wave=4, forced_playouts_k=forced_k,
                         nodes_per_tree=0 if game == "Gomoku" else (MAXT[game] + 1) * (max(R, 3 * A_OF[game]) + 4) + 64,      # (one tree may search every ply)
                         solver=on0, eval_symmetry=eval_symmetry, lib_path=lib_path, **engine_kw)
    assert eng.solver == on0
    for g in range(G):
        eng.set_position(g, prefix)
    evaluator = None
    if eval_symmetry:
        from eval_symmetry_model import sym_eval
        A = A_OF[game]
        evaluator = lambda s_: sym_eval(oracle, lambda x: oracle.hash_eval(x, A, SALT), game, SEED, s_, 0)       # noqa: E731
    n_trees = 1 if single else 2
    models = {}
    for s in slots:
        kw = dict(slot=s, c_puct_init=c_init, dirichlet_alpha=alpha, use_dirichlet=noise, hash_salt=SALT, history=prefix, forced_k=forced_k, solver=on0)
        if evaluator:
            kw["evaluator"] = evaluator(s)
        models[s] = [SolverTree(oracle, game, 1, SEED, tree=t, **kw) for t in range(n_trees)]
    wit, memo = Witness(name), {}
    hist = {s: list(prefix) for s in slots}
    rows = {s: [] for s in slots}
    live = set(slots)
    ply = len(prefix)
    while live and (max_plies is None or ply < len(prefix) + max_plies):
        eng.start_search(); eng.run_move()
        st = eng.root_stats()
        t_run = 0 if single else ply % 2
        trees = dict(zip(sorted(live), eng.read_trees(sorted(live))))
        for s in sorted(live):
            m = models[s][t_run]
            w = m.run(R, tau_on=tau_on(ply, t_run, ef, es))
            what = f"{name} slot {s} ply {ply}"
            assert int(st["phase"][s]) == PH_WAIT_HOST, what
            compare_move(st, s, w, what)
            wit.move(w, raw_row(w["N"]))
            rows[s].append(w)
            check_tree(game, trees[s], m, hist[s], memo, wit, what)
        if ply + 1 in switch:
            # set_solver takes effect at the next launch, and on an engine with two trees per game the launch that applies a move goes straight on
            # into the next move's first simulations: the boundary between two moves is BEFORE the move is applied
            eng.set_solver(switch[ply + 1])
            for s in slots:
                for m in models[s]:
                    m.solver_on = bool(switch[ply + 1])
        eng.apply_moves(None)
        st2 = eng.root_stats()
        for s in sorted(live):
            a = rows[s][-1]["chosen"]
            hist[s].append(a)
            if int(st2["phase"][s]) == PH_HALT:
                live.discard(s)
                continue
            for m in models[s]:
                if new_root:
                    m._do(m.board, a, m.next_player); m.hist.append(a); m.next_player = -m.next_player; m._create_root()
                else:
                    m.play(a)
        ply += 1
    recs = {r["slot"]: r for r in eng.drain_finished()}
    for s in slots:
        if s in live:
            continue
        r = recs[s]
        assert r["T"] == len(hist[s]) and list(r["actions"]) == hist[s], (name, s)
        n0 = len(prefix)
        np.testing.assert_array_equal(r["evals"][n0:], [w["evals"] for w in rows[s]], err_msg=f"{name} slot {s} evals")
        np.testing.assert_array_equal(r["proven"][n0:], [w["status"] != 0 for w in rows[s]], err_msg=f"{name} slot {s} proven")
        np.testing.assert_array_equal(r["policies"][n0:], [w["policy"] for w in rows[s]], err_msg=f"{name} slot {s} policies")
        np.testing.assert_array_equal(r["q"][n0:], [w["q"] for w in rows[s]], err_msg=f"{name} slot {s} q")
        assert not r["proven"][:n0].any()
    all_models = [m for s in slots for m in models[s]]
    wit.trees(all_models)
    stats = eng.solver_stats()
    if len(slots) == G:
        want = [sum(m.stats[i] for m in all_models) for i in range(8)]
        assert list(stats.values()) == want, (name, stats, want)
        assert eng.stats()["sims"] == sum(w["sims"] for s in slots for w in rows[s]), name
    eng.close()
    print(wit, flush=True)
    return wit, rows, stats


# ------------------------------------------------------------------------------------------------ continuous self-play, two trees
SELFPLAY_CASES = {"ttt": ("TicTacToe", 600, 2, 1, 1.25, 1.0), "c4": ("Connect4", 300, 4, 4, 2.5, 0.5)}


def _selfplay_engine(name, G, lib_path, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    game, R, ef, es, c_init, alpha = SELFPLAY_CASES[name]
    return SelfPlayEngine(game, G, R, MAXT[game], ef, es, c_init, alpha, seed=SEED, hash_salt=SALT, ring_capacity=4 * G, games_budget=G, lib_path=lib_path, **kw)


def model_game(oracle, name, r, s, forced_k=0.0, kinds=None, F=0, evaluator=None, wit=None):
    """one record replayed by two SolverTrees driven by the record's actions: every ply's rows, policy, q, root visits, evaluator calls,
    proven mark and the move itself -> the two trees"""
    from solver_model import SolverTree
    game, R, ef, es, c_init, alpha = SELFPLAY_CASES[name]
    kw = dict(slot=s, c_puct_init=c_init, dirichlet_alpha=alpha, hash_salt=SALT, forced_k=forced_k)
    if evaluator:
        kw["evaluator"] = evaluator
    trees = [SolverTree(oracle, game, 1, SEED, tree=t, **kw) for t in range(2)]
    for ply, a in enumerate(r["actions"]):
        fast = kinds is not None and kinds[ply] == 2
        w = trees[ply % 2].run(min(F, R) if fast else R, forced=not fast, tau_on=tau_on(ply, ply % 2, ef, es))
        what = f"{name} slot {s} ply {ply}"
        np.testing.assert_array_equal(r["root_N"][ply], w["N"], err_msg=what); np.testing.assert_array_equal(r["root_W"][ply], w["W"], err_msg=what)
        np.testing.assert_array_equal(r["root_P"][ply], w["P"], err_msg=what)
        np.testing.assert_array_equal(r["policies"][ply], w["policy"], err_msg=what + " policy")
        assert r["root_visits"][ply] == w["root_visits"] and r["evals"][ply] == w["evals"], what
        assert r["q"][ply] == w["q"] and bool(r["proven"][ply]) == (w["status"] != 0), what
        assert int(a) == w["chosen"], (what, int(a), w["chosen"])
        if wit is not None:
            wit.move(w, raw_row(w["N"]))
            if fast:
                wit.fast_proven = getattr(wit, "fast_proven", 0) + (w["status"] != 0 and w["sims"] < w["limit"])
        if ply + 1 < r["T"]:
            for t in trees:
                t.play(int(a))
    return trees


def selfplay_case(oracle, name, G, lib_path, slots=None, forced_k=0.0, cap=None, evaluator_of=None, **kw):
    """G slots, games_budget = G, continuous self-play with both trees and the solver on; the compared slots' records == the model, and (all
    slots compared) solver_stats == the model's counts.  forced_k: with forced playouts; cap = (F, p): with the playout cap; evaluator_of(slot):
    the model's evaluator (eval_symmetry engines).  -> (witness, records)"""
    from playout_cap_cases import kinds_of
    if forced_k:
        kw["forced_playouts_k"] = forced_k
    if cap:
        kw.update(fast_iterations=cap[0], full_search_prob=cap[1])
    eng = _selfplay_engine(name, G, lib_path, solver=True, **kw)
    first = first_games(eng, G)
    stats = eng.solver_stats()
    eng.close()
    slots = tuple(range(G)) if slots is None else tuple(slots)
    wit, models = Witness("selfplay " + name), []
    for s in slots:
        kinds = None
        if cap:
            kinds = kinds_of(oracle, SEED, s, 0, first[s]["T"], cap[1])
            np.testing.assert_array_equal(first[s]["move_kind"], kinds, err_msg=f"slot {s}")
        models += model_game(oracle, name, first[s], s, forced_k=forced_k, kinds=kinds, F=cap[0] if cap else 0,
                             evaluator=evaluator_of(s) if evaluator_of else None, wit=wit)
    wit.trees(models)
    if len(slots) == G:
        want = [sum(m.stats[i] for m in models) for i in range(8)]
        assert list(stats.values()) == want, (stats, want)
    print(wit, flush=True)
    return wit, first


def off_records(name, G, lib_path, **kw):
    eng = _selfplay_engine(name, G, lib_path, **kw)
    first = first_games(eng, G)
    eng.close()
    return first


# ------------------------------------------------------------------------------------------------ refusals
REFUSALS = {   # name -> engine arguments, what the message must say
    "gumbel": (dict(search=1, gumbel_m=4), "Gumbel search"),
    "leaf_batch": (dict(leaf_batch=4), "leaf_batch"),
    "gumbel_batch": (dict(search=1, gumbel_m=4, gumbel_batch=4), "gumbel_batch"),
}


def refusal_case(which, lib_path):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    kw, text = REFUSALS[which]
    eng = SelfPlayEngine("Connect4", 4, 16, 42, 0, 0, 2.5, 0.5, seed=1, hash_salt=1, lib_path=lib_path, **kw)
    try:
        msg = refusal_message(lambda: eng.set_solver(True), f"{which}: set_solver was not refused")
        assert text in msg, (which, msg)
        assert not eng.solver and list(eng.solver_stats().values()) == [0] * 8
        return msg
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ anchors
def quiet_anchor_case(G, lib_path):
    """solver on, but no terminal parent is ever reached (four plies of Connect4 at 12 iterations): the solver-off records, field for field,
    and every counter 0"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    recs = {}
    for on in (False, True):
        eng = SelfPlayEngine("Connect4", G, 12, 4, 2, 2, 2.5, 0.5, seed=SEED, hash_salt=SALT, ring_capacity=4 * G, games_budget=G, solver=on, lib_path=lib_path)
        recs[on] = first_games(eng, G)
        if on:
            assert list(eng.solver_stats().values()) == [0] * 8, eng.solver_stats()
        eng.close()
    for s in range(G):
        assert_records_equal(recs[True][s], recs[False][s], f"quiet slot {s}", keys=RECORD_KEYS + ("move_kind", "proven"))


def differs_from_off_case(name, G, lib_path):
    """the solver is a different search: some record differs from the solver-off engine's"""
    on, off = off_records(name, G, lib_path, solver=True), off_records(name, G, lib_path)
    assert any(on[s]["T"] != off[s]["T"] or not np.array_equal(on[s]["root_N"], off[s]["root_N"]) or not np.array_equal(on[s]["q"], off[s]["q"]) for s in range(G))
    assert not any(off[s]["proven"].any() for s in range(G)) and any(on[s]["proven"].any() for s in range(G))


# ------------------------------------------------------------------------------------------------ compositions
def resign_case(oracle, name, G, lib_path, threshold=0.95):
    """resignation reads the exact q: with the rule (threshold, 1 ply, no play-out games) a game of the solver engine ends where the restated
    rule triggers on the records of the same engine without resignation — and some game is resigned on a ply proven lost (q = -1)"""
    from resign_cases import expectation
    off = off_records(name, G, lib_path, solver=True)
    on = off_records(name, G, lib_path, solver=True, resign_threshold=threshold, resign_consecutive=1, resign_min_ply=0, no_resign_prob=0.0)
    n_proven = 0
    for s in range(G):
        e = expectation(oracle, off[s], (threshold, 1, 0, 0.0), seed=SEED)
        r = on[s]
        assert (r["T"], r["winner"], r["resign_ply"]) == (e["T"], e["winner"], e["resign_ply"]), (s, e)
        for k in ("actions", "q", "root_N", "policies", "proven"):
            np.testing.assert_array_equal(r[k], off[s][k][:r["T"]], err_msg=f"slot {s} {k}")
        if e["resign_ply"] >= 0:
            n_proven += bool(r["proven"][e["resign_ply"]]) and r["q"][e["resign_ply"]] == np.float32(-1.0)
    assert n_proven >= 1, "no game was resigned on a ply proven lost"
    return n_proven


def samples_case(name, G, lib_path):
    """drain_samples == record_to_samples on the records of a solver engine"""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import record_to_samples
    game = SELFPLAY_CASES[name][0]
    recs = off_records(name, G, lib_path, solver=True)
    dev = _selfplay_engine(name, G, lib_path, solver=True)
    got = first_games(dev, G, samples=True)
    dev.close()
    assert any(recs[s]["proven"].any() for s in range(G))
    for s in range(G):
        hb, hp, hv, _ = record_to_samples(GAMES[game], recs[s])
        _, b, p, v = got[s]
        for what, d, h in zip(("boards", "policies", "values"), (b, p, v), (hb, hp, hv)):
            assert d.dtype == h.dtype and d.shape == h.shape, (s, what)
            np.testing.assert_array_equal(d, h, err_msg=f"{name} slot {s} {what}")


def run_self_play_case(tmp, lib_path, games=12, G=8):
    """train_config["solver"]: absent and False give the same file, True another one"""
    train = dict(games_per_generation=games, MCTS_iteration_limit=200, max_actions=9, num_explore_actions_first=2, num_explore_actions_second=1,
                 c_puct_init=1.25, dirichlet_alpha=1.0, use_gumbel=False)
    out = []
    for extra in ({}, dict(solver=False), dict(solver=True)):
        f = self_play_file(tmp, str(len(out)), "TicTacToe", dict(train, **extra), games, n_games=G, seed=11, hash_salt=4, lib_path=lib_path)
        out.append(games_of_file(f, games, 8))
    assert out[0] == out[1] and out[0] != out[2]


def mcts_class_case(oracle, lib_path, iters=600, seed=5):
    """mcts.MCTS(solver=True): run()'s rows == the model's search, MCTS.root's nodes carry .proven == the model's statuses == minimax, and
    MCTS_Gumbel does not take the keyword"""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.mcts import MCTS, MCTS_Gumbel
    from solver_model import SolverTree, minimax
    g = GAMES["TicTacToe"]()
    m = MCTS(g, None, c_puct_init=1.25, dirichlet_alpha=1.0, tau=0.0, seed=seed, hash_salt=SALT, solver=True, lib_path=lib_path)
    model = SolverTree(oracle, "TicTacToe", 1, seed, c_puct_init=1.25, dirichlet_alpha=1.0, hash_salt=SALT)
    n_proven, memo = 0, {}
    for _ in range(4):
        move, rows = m.run(iters)
        w = model.run(iters)
        st = m._eng.root_stats()
        for key in ("N", "W", "P", "policy"):
            np.testing.assert_array_equal(st[key][0], w[key], err_msg=f"MCTS {key}")
        assert g.action_to_index(move) == w["chosen"]
        root = m.root
        assert root.proven == w["status"]
        queue, want = [root], model.statuses()
        for node in queue:
            queue += [c for c in node.children if c.is_terminal is None]
        assert [n.proven for n in queue] == want
        for n in queue:
            if n.proven:
                hist = [g.action_to_index(a) for a in n.action_history]
                board, mover = replay("TicTacToe", hist)
                assert n.proven == minimax("TicTacToe", board, hist, mover, memo)
                n_proven += 1
        g.do_action(move); m.prune_tree(move); model.play(g.action_to_index(move))
    m.close()
    assert n_proven > 0
    try:
        MCTS_Gumbel(GAMES["Connect4"](), None, solver=True, lib_path=lib_path)
    except TypeError:
        return n_proven
    raise AssertionError("MCTS_Gumbel took the solver keyword")


def abi_case(lib_path):
    """GAZ_ENGINE_ABI_VERSION is still 10 and the feature is detected by its symbols; bad arguments are refused with a text"""
    from grok_alpha_zero_amd import engine as E
    L = E.load_library(lib_path)
    assert L.gaz_engine_abi_version() == E.ABI_VERSION == 10 and E.EngineConfig._fields_[-1][0] == "forced_playouts_k"
    assert all(hasattr(L, "gaz_engine_" + f) for f in ("set_solver", "get_solver", "get_solver_stats"))
    eng = E.SelfPlayEngine("Connect4", 4, 16, 42, 0, 0, 2.5, 0.5, seed=1, lib_path=lib_path)
    msgs = {}
    try:
        assert eng.solver is False and list(eng.solver_stats().values()) == [0] * 8
        for mode in (-1, 2):
            assert L.gaz_engine_set_solver(eng.h, mode) != 0
            msgs[mode] = L.gaz_engine_last_error(eng.h).decode()
            assert "mode must be 0" in msgs[mode] and str(mode) in msgs[mode] and eng.solver is False
        assert L.gaz_engine_get_solver(eng.h, None) != 0
        msgs["get"] = L.gaz_engine_last_error(eng.h).decode()
        assert L.gaz_engine_get_solver_stats(eng.h, None) != 0
        msgs["stats"] = L.gaz_engine_last_error(eng.h).decode()
        eng.set_solver(True); assert eng.solver is True
        eng.set_solver(False); assert eng.solver is False
    finally:
        eng.close()
    assert len(set(msgs.values())) == len(msgs), msgs
    return msgs


# ------------------------------------------------------------------------------------------------ the HIP build: wavefronts, a real network
def gpu_slots(G=64):
    """the four games of the first wavefront plus one game of every other wavefront (four 16-lane teams per wavefront)"""
    return (0, 1, 2, 3) + tuple(range(4, G, 4))


def scheduling_case(which, G=64):
    """64 Connect4 games, 1-block network, solver on: the records do not depend on the fused launch, the game groups or the evaluation cache"""
    def some_move_is_proven(recs, sv):
        assert sv["proven_moves"] > 0 and sv["masked_levels"] > 0, sv
    scheduling_equalities(which, G, dict(seed=SEED, solver=True), lambda eng: (play(eng, G, raw=True), eng.solver_stats()), some_move_is_proven)


def network_case(oracle, G=64, slots=(0, 1, 2, 3, 32, 63)):
    """64 Connect4 games with the 1-block network in the fused launch, solver on; the compared slots replayed by the model whose evaluator is
    a second engine's evaluate() on single rows"""
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
    w = c4_one_block_weights()
    eng = net_engine(G, w, seed=SEED, solver=True)
    first = first_games(eng, G)
    assert eng.stats()["fused_wave"] == 1
    eng.close()
    probe = SelfPlayEngine("Connect4", 64, 1, 42, 4, 4, 2.5, 0.5, seed=0, evaluator=EVAL_RESNET, net_blocks=1, ring_capacity=0)
    probe.load_weights(w)
    memo = {}

    def base(state):
        key = state.tobytes()
        if key not in memo:
            p, v, _ = probe.evaluate(state[None])
            memo[key] = (p[0].copy(), v[0])
        return memo[key]
    wit = Witness("network")
    global SELFPLAY_CASES
    SELFPLAY_CASES = dict(SELFPLAY_CASES, net=("Connect4", 40, 4, 4, 2.5, 0.5))
    models = []
    for s in slots:
        models += model_game(oracle, "net", first[s], s, evaluator=base, wit=wit)
    probe.close()
    wit.trees(models)
    print(wit, flush=True)
    assert wit.root_win + wit.root_loss > 0 and wit.masked_levels > 0
    return wit

"""The cases of forced playouts and policy target pruning (gaz_engine_config.forced_playouts_k; DESIGN.md "Forced playouts and policy
target pruning") that the CPU suite runs on the emulation build (tests/test_forced_playouts_emu.py) and the -m gpu suite on the HIP
build (tests/test_forced_playouts_gpu.py): `lib_path` = the emulation library, or None for the product library.

What a search must give is computed HERE by tests/forced_playouts_model.py (ForcedTree: forced selection on leaf_batch_model.Tree;
prune_target: the policy row from the RAW root rows), never read back from the engine under test; the playout cap's kinds come from
playout_cap_cases.kinds_of (oracle.uniform).  Every comparison is exact."""
import numpy as np

from playout_cap_cases import base_limits, kinds_of
from selfplay_support import (A_OF, MAXT, N_AUG, RECORD_KEYS, SLOTS64, assert_records_equal, first_games, games_of_file, refusal_message,
                              scheduling_equalities, self_play_file, slots_for)

SEED, SALT = 31, 8
K = 2.0                                            # KataGo's k


def terminal_root(game, history):
    """the position after `history` lets the mover end the game at once: its root is a terminal parent (no forcing, no pruning there)"""
    from grok_alpha_zero_amd.games import GAMES
    from leaf_batch_model import Tree
    t = Tree.__new__(Tree)
    t.name, t.G = game, GAMES[game]
    board, player = np.zeros((t.G.H, t.G.W), np.int8), -1
    for a in history:
        t._do(board, a, player); player = -player
    acts, _ = t._terminal_actions(board, [int(a) for a in history], player)
    return bool(acts)


def expected_policy(row_N, row_W, row_P, root_visits, k, c_init, forced, terminal):
    """the policy row of a ply from its RAW rows: pruned on a forced (full, k > 0) move whose root is no terminal parent, else N / sum(N)"""
    from forced_playouts_model import prune_target, raw_target
    if forced and k > 0 and not terminal:
        return prune_target(row_N, row_W, row_P, int(root_visits), k, c_init)
    return raw_target(row_N)


class Exercise:
    """(b): what a case's compared moves must show, counted on the model"""

    def __init__(self, name):
        self.name, self.differ, self.free, self.pruned, self.removed = name, 0, 0, 0, []

    def search(self, w):
        self.differ += w["n_differ"]; self.free += w["n_free"]

    def row(self, N, pol, forced):
        from forced_playouts_model import raw_target
        if forced and not np.array_equal(pol, raw_target(N)):
            self.pruned += 1
            self.removed.append((int(np.asarray(N, np.uint64).sum()), pol))

    def check(self):
        print(f"{self.name}: forced picks that differ from PUCT's {self.differ}, root selections with nothing owed {self.free}, pruned rows {self.pruned}",
              flush=True)
        assert self.differ >= 1, f"{self.name}: no forced selection differs from best_puct_index's choice: pick another seed / k"
        assert self.free >= 1, f"{self.name}: no root selection with nothing owed: pick another seed / k"
        assert self.pruned >= 1, f"{self.name}: no pruned row: pick another seed / k"


# ------------------------------------------------------------------------------------------------ (a) sync mode against the model
# name -> game, R, leaf_batch, the fixed moves, k, c_puct_init, dirichlet_alpha, the slots compared of 64 games
HASH_CASES = {
    "ttt": ("TicTacToe", 24, 1, [4, 0, 8], K, 1.25, 1.0, SLOTS64),
    "c4-k1": ("Connect4", 40, 1, [3, 3, 2, 4], K, 2.5, 0.5, SLOTS64), "c4-k4": ("Connect4", 40, 4, [3, 3, 2, 4], K, 2.5, 0.5, SLOTS64),
    # at k = 2 a near-uniform 225-way prior owes every child visits for the whole search: the free path would never run
    "gmk": ("Gomoku", 480, 1, [112], 0.5, 2.5, 0.05, (0, 63)),
    # (e) X 0, O 3, X 1, O 4: X wins at 2 — the last root is a terminal parent and keeps N / sum(N)
    "ttt-terminal": ("TicTacToe", 24, 1, [0, 3, 1, 4], K, 1.25, 1.0, SLOTS64),
}


def hash_case(oracle, name, G, lib_path, exercise=True):
    """G games at once (sync + single tree, hash evaluator), every game playing the same fixed moves on its own RNG streams.  After every
    move, for the compared slots: root N / W / P / root visits == ForcedTree.run, policy == prune_target of the model's raw rows."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    from forced_playouts_model import ForcedTree
    game, R, LB, moves, k, c_init, alpha, slots = HASH_CASES[name]
    eng = SelfPlayEngine(game, G, R, MAXT[game], 0, 0, c_init, alpha, seed=SEED, hash_salt=SALT, sync_moves=True, single_tree=True,
                         nodes_per_tree=(len(moves) + 1) * (max(R, 3 * A_OF[game]) + 4) + 64, compact_trees=-1, max_tree_sims_per_wave=4, tau=0.0,
                         leaf_batch=LB, forced_playouts_k=k, lib_path=lib_path)
    models = {s: ForcedTree(oracle, game, LB, SEED, slot=s, c_puct_init=c_init, dirichlet_alpha=alpha, hash_salt=SALT, max_tree_sims=4, forced_k=k)
              for s in slots_for(G, slots)}
    ex, n_terminal = Exercise(name), 0
    for t, m in enumerate(list(moves) + [None]):
        eng.start_search(); eng.run_move()
        st = eng.root_stats()
        for s, model in models.items():
            terminal = model.root.terminal
            n_terminal += terminal
            w = model.run(R)
            what = f"{name} slot {s} ply {t}"
            np.testing.assert_array_equal(st["N"][s], w["N"], err_msg=what); np.testing.assert_array_equal(st["W"][s], w["W"], err_msg=what)
            np.testing.assert_array_equal(st["P"][s], w["P"], err_msg=what)
            assert int(st["root_visits"][s]) == w["root_visits"], what
            pol = expected_policy(w["N"], w["W"], w["P"], w["root_visits"], k, c_init, True, terminal)
            np.testing.assert_array_equal(st["policy"][s], pol, err_msg=what + " policy")
            ex.search(w); ex.row(w["N"], pol, not terminal)
        print(f"{name}: ply {t} ok", flush=True)
        if m is None:
            break
        eng.apply_moves([m] * G)
        for model in models.values():
            model.play(m)
    eng.close()
    if exercise:
        ex.check()
    return ex, n_terminal


def terminal_root_case(oracle, G, lib_path):
    """(e) a root that is a terminal parent keeps N / sum(N): the last ply of "ttt-terminal" (hash_case compared it against raw_target)"""
    game, _, _, moves = HASH_CASES["ttt-terminal"][:4]
    assert terminal_root(game, moves) and not any(terminal_root(game, moves[:i]) for i in range(len(moves)))
    ex, n_terminal = hash_case(oracle, "ttt-terminal", G, lib_path, exercise=False)
    assert n_terminal == len(slots_for(G)), n_terminal                  # one terminal root per compared slot, the last ply
    assert ex.pruned >= 1                                                # and the plies before it were pruned


# ------------------------------------------------------------------------------------------------ (c), (d) continuous self-play, two trees
C4 = dict(game="Connect4", R=40, c_init=2.5, alpha=0.5, salt=6)
CAP = dict(F=8, p=0.5)


def _c4(G, lib_path, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    return SelfPlayEngine("Connect4", G, C4["R"], 42, 4, 4, C4["c_init"], C4["alpha"], seed=SEED, hash_salt=C4["salt"], ring_capacity=4 * G, games_budget=G,
                          lib_path=lib_path, **kw)


def selfplay_case(oracle, G, lib_path, cap=False, k=K):
    """G slots, games_budget = G, continuous self-play with both trees.  For the compared slots two model trees per game, fed the record's
    actions, reproduce every ply's raw rows, root visits and evaluator calls, and `policies` == prune_target of the record's OWN root_N /
    root_W / root_P / root_visits.  With the cap (F = 8, p = 0.5) the kind-2 plies are plain: the unforced search at the fast limit,
    policy N / sum(N)."""
    from forced_playouts_model import ForcedTree
    game, R = C4["game"], C4["R"]
    eng = _c4(G, lib_path, forced_playouts_k=k, **(dict(fast_iterations=CAP["F"], full_search_prob=CAP["p"]) if cap else {}))
    first = first_games(eng, G)
    eng.close()
    ex, seen = Exercise("selfplay" + (" with the cap" if cap else "")), set()
    for s in slots_for(G):
        r = first[s]
        kinds = kinds_of(oracle, SEED, s, 0, r["T"], CAP["p"]) if cap else np.ones(r["T"], np.uint8)
        np.testing.assert_array_equal(r["move_kind"], kinds, err_msg=f"slot {s}")
        seen |= {int(x) for x in kinds}
        lims = base_limits(kinds, R, CAP["F"])
        trees = [ForcedTree(oracle, game, 1, SEED, slot=s, tree=t, c_puct_init=C4["c_init"], dirichlet_alpha=C4["alpha"], hash_salt=C4["salt"], forced_k=k)
                 for t in range(2)]
        for ply, a in enumerate(r["actions"]):
            tree, full = trees[ply % 2], kinds[ply] == 1
            terminal = tree.root.terminal
            w = tree.run(lims[ply], forced=full)
            what = f"slot {s} ply {ply} kind {kinds[ply]} limit {lims[ply]}"
            np.testing.assert_array_equal(r["root_N"][ply], w["N"], err_msg=what); np.testing.assert_array_equal(r["root_W"][ply], w["W"], err_msg=what)
            np.testing.assert_array_equal(r["root_P"][ply], w["P"], err_msg=what)
            assert r["root_visits"][ply] == w["root_visits"] and r["evals"][ply] == w["evals"], what
            pol = expected_policy(r["root_N"][ply], r["root_W"][ply], r["root_P"][ply], r["root_visits"][ply], k, C4["c_init"], full, terminal)
            np.testing.assert_array_equal(r["policies"][ply], pol, err_msg=what + " policy")
            if full:
                ex.search(w); ex.row(r["root_N"][ply], pol, not terminal)
            else:
                assert w["n_differ"] == 0 and w["n_free"] == 0
            if ply + 1 < r["T"]:
                for t in trees:
                    t.play(a)
    assert seen == ({1, 2} if cap else {1}), seen
    ex.check()
    return first


# ------------------------------------------------------------------------------------------------ (e) anchor: k = 0
def k0_anchor_case(G, lib_path):
    """k = 0 gives the records of an engine created without the field's effect — every array, move_kind included; and k = 2 does not
    (the field is read)"""
    recs = {}
    for name, kw in (("plain", {}), ("k0", dict(forced_playouts_k=0.0)), ("k2", dict(forced_playouts_k=K))):
        eng = _c4(G, lib_path, **kw)
        recs[name] = first_games(eng, G)
        eng.close()
    for s in range(G):
        assert_records_equal(recs["k0"][s], recs["plain"][s], f"k = 0, slot {s}", keys=RECORD_KEYS + ("move_kind",))
    assert any(not np.array_equal(recs["k2"][s]["root_N"], recs["plain"][s]["root_N"]) for s in range(G))


# ------------------------------------------------------------------------------------------------ (f) samples
# name -> game, G, R, k, max_actions
SAMPLE_CASES = {"c4": ("Connect4", 64, 40, K, 42), "gmk": ("Gomoku", 8, 48, 0.5, 6)}


def _sample_engine(name, lib_path, G=None):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    game, G0, R, k, max_actions = SAMPLE_CASES[name]
    G = G or G0
    return SelfPlayEngine(game, G, R, max_actions, 3, 2, 2.5, 0.5, seed=SEED, hash_salt=6, slot_offset=10, ring_capacity=4 * G, games_budget=G,
                          forced_playouts_k=k, lib_path=lib_path), game, G, k


def samples_case(name, lib_path, G=None):
    """paired engines: drain_samples (the kernel) == record_to_samples of the other engine's records (the host definition), and both ==
    prune_target of the record's raw rows pushed through the augmentations"""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import record_to_samples
    from forced_playouts_model import raw_target
    host, game, G, k = _sample_engine(name, lib_path, G)
    dev = _sample_engine(name, lib_path, G)[0]
    recs = first_games(host, G)
    got = first_games(dev, G, samples=True)
    host.close(); dev.close()
    assert sorted(recs) == sorted(got) == list(range(10, 10 + G))
    pruned = 0
    for s, r in recs.items():
        row, db, dp, dv = got[s]
        assert (int(row[0]), int(row[1]), int(row[2]), int(row[3]), int(row[5])) == (r["T"], r["winner"], s, r["game_seq"], 0), (name, s)
        hb, hp, hv, length = record_to_samples(GAMES[game], r)
        assert length == r["T"] and hb.shape[0] == N_AUG[game]
        model = dict(r)
        model["policies"] = np.stack([expected_policy(r["root_N"][t], r["root_W"][t], r["root_P"][t], r["root_visits"][t], k, 2.5, True,
                                                      terminal_root(game, r["actions"][:t])) for t in range(r["T"])])
        pruned += sum(not np.array_equal(model["policies"][t], raw_target(r["root_N"][t])) for t in range(r["T"]))
        mb, mp, mv, _ = record_to_samples(GAMES[game], model)
        for what, d, h, m in (("boards", db, hb, mb), ("policies", dp, hp, mp), ("values", dv, hv, mv)):
            assert d.dtype == h.dtype == m.dtype and d.shape == h.shape == m.shape, (name, s, what, d.shape, h.shape, m.shape)
            np.testing.assert_array_equal(d, h, err_msg=f"{name} slot {s} {what} (device vs host)")
            np.testing.assert_array_equal(d, m, err_msg=f"{name} slot {s} {what} (device vs prune_target)")
    assert pruned > 0, f"{name}: no pruned row in {G} games"
    return pruned


# ------------------------------------------------------------------------------------------------ (g) run_self_play
def run_self_play_case(tmp, lib_path, games=40, G=24):
    """run_self_play with train_config["forced_playouts_k"]: the same file at both settings of device_samples, and its games are those of
    an engine created with forced_playouts_k directly (pruned rows among them)"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import record_to_samples
    from forced_playouts_model import raw_target
    train = dict(games_per_generation=games, MCTS_iteration_limit=16, forced_playouts_k=K, max_actions=9, num_explore_actions_first=2,
                 num_explore_actions_second=1, c_puct_init=1.25, dirichlet_alpha=1.0, use_gumbel=False)
    out = {ds: self_play_file(tmp, f"ds{ds}", "TicTacToe", train, games, n_games=G, seed=11, hash_salt=4, lib_path=lib_path, device_samples=ds)
           for ds in (False, True)}
    eng = SelfPlayEngine("TicTacToe", G, 24, 9, 2, 1, 1.25, 1.0, seed=11, hash_salt=4, ring_capacity=4 * G, games_budget=games, forced_playouts_k=K,
                         lib_path=lib_path)
    recs = []
    for _ in range(40000):
        eng.run_waves(16); recs += eng.drain_finished()
        if len(recs) == games:
            break
    eng.close()
    assert len(recs) == games
    assert any(not np.array_equal(r["policies"][t], raw_target(r["root_N"][t])) for r in recs for t in range(r["T"])), "no pruned row"
    np.testing.assert_array_equal(out[False]["game_stats"], out[True]["game_stats"])

    want = []
    for r in recs:
        b, p, v, _ = record_to_samples(GAMES["TicTacToe"], r)
        want.append(tuple((a.dtype.str, a.shape, a.tobytes()) for a in [np.asarray(x[j]) for j in range(8) for x in (b, p, v)]))
    for ds in (False, True):
        assert len(out[ds]) == 1 + 3 * 8 * games
    assert games_of_file(out[False], games, 8) == games_of_file(out[True], games, 8) == sorted(want)


# ------------------------------------------------------------------------------------------------ (h) refusals
REFUSALS = {   # name -> engine arguments, what the message must say
    "negative": (dict(forced_playouts_k=-0.5), "forced_playouts_k must be >= 0"),
    "nan": (dict(forced_playouts_k=float("nan")), "not NaN"),
    "infinite": (dict(forced_playouts_k=float("inf")), "forced_playouts_k must be finite"),
    "gumbel": (dict(forced_playouts_k=K, search=1, gumbel_m=4), "GAZ_SEARCH_GUMBEL"),
}


def refusal_case(name, lib_path):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    kw, text = REFUSALS[name]
    msg = refusal_message(lambda: SelfPlayEngine("Connect4", 8, 40, 42, 4, 4, 2.5, 0.5, seed=1, lib_path=lib_path, **kw).close(),
                          f"{name}: gaz_engine_create accepted {kw}")
    assert text in msg and "forced_playouts_k" in msg, (name, msg)
    return msg


# ------------------------------------------------------------------------------------------------ (i) scheduling equalities (HIP build, network)
def scheduling_case(which, G=64):
    """64 Connect4 games with a 1-block network and forced playouts on: the records do not depend on the fused launch, the game groups or
    the evaluation cache"""
    from forced_playouts_model import raw_target

    def some_row_is_pruned(recs, _):
        pruned = sum(not np.array_equal(r["policies"][t], raw_target(r["root_N"][t])) for r in recs.values() for t in range(r["T"]))
        assert pruned > 0
    scheduling_equalities(which, G, dict(seed=SEED, forced_playouts_k=K), lambda eng: (first_games(eng, G), None), some_row_is_pruned,
                          keys=RECORD_KEYS + ("move_kind",))

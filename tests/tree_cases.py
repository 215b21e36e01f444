"""Reading search trees back (gaz_engine_read_trees / gaz_engine_read_pv, SelfPlayEngine.read_trees / principal_variations, MCTS.root):
the helpers and case bodies that the CPU suite runs on the emulation build (tests/test_tree_readout_emu.py) and the -m gpu suite on the
HIP build (tests/test_tree_readout_gpu.py): `lib_path` = the emulation library, or None for the product library.

The yardstick for the PUCT trees is tests/leaf_batch_model.py (a whole tree in Python, pinned to the oracle at K = 1 by
tests/test_leaf_batch_emu.py): model_export() walks Tree.root into the canonical node / edge arrays of include/gaz_engine.h.  Every
comparison is assert_array_equal; nothing has a tolerance."""
import os

import numpy as np

from leaf_batch_model import DRAW, WIN, Tree, _Node
from selfplay_support import A_OF, MAXT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PH_SIMS = 3
FILTERED = -4
TTT_DRAWN_GAME = [4, 0, 8, 2, 6, 3, 5, 7]        # + the forced 1: a draw; wins in one are left standing on the way (terminal roots and parents)


def _dtypes():
    from grok_alpha_zero_amd.engine import TREE_EDGE_DTYPE, TREE_NODE_DTYPE
    return TREE_NODE_DTYPE, TREE_EDGE_DTYPE


# ------------------------------------------------------------------------------------------------ canonical arrays
def model_export(tree):
    """leaf_batch_model.Tree -> (nodes, edges) in the canonical order: breadth-first from Tree.root, children in slot order"""
    nd, ed = _dtypes()
    order, meta = [tree.root], [(-1, 0, 0)]
    nodes, edges = [], []
    k = 0
    while k < len(order):
        n, (parent, slot, depth) = order[k], meta[k]
        nodes.append((parent, slot, depth, len(edges), len(n.act), n.n_children, 1 if n.terminal else 0, n.n_reserved, n.player,
                      n.hist[-1] if n.hist else 0, len(n.hist), 0))
        for s, a in enumerate(n.act):
            c = n.child[s]
            if isinstance(c, _Node):
                order.append(c); meta.append((k, s, depth + 1)); code = len(order) - 1
            else:
                code = -1 if c is None else int(c)
                assert code in (-1, DRAW, WIN)
            edges.append((a, n.N[s], n.W[s], n.P[s], 0.0, code))
        k += 1
    return np.array(nodes, nd), np.array(edges, ed).reshape(-1)


def assert_trees_equal(got_nodes, got_edges, want_nodes, want_edges, what=""):
    assert got_nodes.shape == want_nodes.shape and got_edges.shape == want_edges.shape, (what, got_nodes.shape, want_nodes.shape, got_edges.shape, want_edges.shape)
    for f in want_nodes.dtype.names:
        np.testing.assert_array_equal(got_nodes[f], want_nodes[f], err_msg=f"{what} nodes.{f}")
    for f in want_edges.dtype.names:
        np.testing.assert_array_equal(got_edges[f], want_edges[f], err_msg=f"{what} edges.{f}")


def filter_export(nodes, edges, max_depth, min_visits):
    """the full export filtered and re-indexed on the host by the rules of gaz_engine_read_trees"""
    if len(nodes) == 0:
        return nodes.copy(), edges.copy()
    keep = np.zeros(len(nodes), bool); keep[0] = True
    for i in range(1, len(nodes)):
        p = int(nodes["parent"][i])
        n_edge = edges["N"][int(nodes["edge0"][p]) + int(nodes["slot"][i])]
        keep[i] = keep[p] and (max_depth is None or nodes["depth"][i] <= max_depth) and n_edge >= min_visits
    new = np.cumsum(keep) - 1
    on, oe = [], []
    for i in np.flatnonzero(keep):
        n = nodes[i].copy()
        e = edges[int(n["edge0"]):int(n["edge0"]) + int(n["n_actions"])].copy()
        for j in range(len(e)):
            if e["child"][j] >= 0:
                e["child"][j] = new[e["child"][j]] if keep[e["child"][j]] else FILTERED
        n["parent"] = -1 if i == 0 else new[n["parent"]]
        n["edge0"] = sum(len(x) for x in oe)
        on.append(n); oe.append(e)
    return np.array(on, nodes.dtype), np.concatenate(oe) if oe else edges[:0].copy()


def host_pv(nodes, edges, max_len, first_action=-1):
    """the principal variation by the rule of include/gaz_engine.h, from a full export -> [(action, N, W)]"""
    out, i = [], 0 if len(nodes) else -1
    while i >= 0 and len(out) < max_len:
        e = edges[int(nodes["edge0"][i]):int(nodes["edge0"][i]) + int(nodes["n_actions"][i])]
        if len(e) == 0:
            break
        if not out and first_action >= 0:
            hit = np.flatnonzero(e["action"] == first_action)
            if hit.size == 0:
                break
            s = int(hit[0])
        else:
            s = int(np.argmax(e["N"]))                                 # the first maximum: the lowest slot
        out.append((int(e["action"][s]), int(e["N"][s]), e["W"][s]))
        if e["child"][s] < 0 or e["N"][s] == 0:
            break
        i = int(e["child"][s])
    return out


def assert_pv_equals(pv, g, line, what=""):
    assert int(pv["len"][g]) == len(line), (what, int(pv["len"][g]), len(line))
    n = len(line)
    np.testing.assert_array_equal(pv["actions"][g, :n], np.array([a for a, _, _ in line], np.uint8), err_msg=what)
    np.testing.assert_array_equal(pv["N"][g, :n], np.array([v for _, v, _ in line], np.uint32), err_msg=what)
    np.testing.assert_array_equal(pv["W"][g, :n], np.array([w for _, _, w in line], np.float32), err_msg=what)
    assert not pv["actions"][g, n:].any() and not pv["N"][g, n:].any() and not pv["W"][g, n:].any(), what


def assert_consistent(t, what=""):
    """structure of one exported tree: parents precede children, parent / slot point back at the edge that names the node, depth, n_hist and
    action follow the parent's, edge0 is the running sum of n_actions"""
    n, e = t.nodes, t.edges
    if len(n) == 0:
        assert len(e) == 0, what
        return
    assert n["parent"][0] == -1 and n["depth"][0] == 0 and n["slot"][0] == 0, what
    np.testing.assert_array_equal(n["edge0"], np.concatenate([[0], np.cumsum(n["n_actions"])[:-1]]), err_msg=what)
    assert len(e) == int(n["n_actions"].sum()), what
    i = np.arange(1, len(n)); p = n["parent"][1:]
    assert (p >= 0).all() and (p < i).all(), what
    back = n["edge0"][p] + n["slot"][1:]
    assert (n["slot"][1:] < n["n_actions"][p]).all(), what
    np.testing.assert_array_equal(e["child"][back], i, err_msg=what)
    np.testing.assert_array_equal(n["depth"][1:], n["depth"][p] + 1, err_msg=what)
    np.testing.assert_array_equal(n["n_hist"][1:], n["n_hist"][p] + 1, err_msg=what)
    np.testing.assert_array_equal(n["action"][1:], e["action"][back], err_msg=what)
    np.testing.assert_array_equal(n["player"][1:], -n["player"][p], err_msg=what)
    named = e["child"][e["child"] >= 0]
    np.testing.assert_array_equal(np.sort(named), i, err_msg=what)      # every node but the root is named by exactly one edge
    assert (np.diff(n["depth"]) >= 0).all(), what                       # breadth first


# ------------------------------------------------------------------------------------------------ whole-tree parity, PUCT
def puct_case(oracle, lib_path, game, K, iters, moves, G, slots, *, compact=(-1,), c_init=2.5, alpha=0.5, seed=31, salt=8, max_tree_sims=4,
              filters=False, pv_len=6):
    """G games at once (sync + single tree, hash evaluator), every game plays the same fixed `moves`; RNG streams differ by slot.  After EVERY
    move the export of `slots` equals the model's tree, node for node and edge for edge (one engine per entry of `compact`: they must all
    agree), and the principal variations equal the line computed on the host from the export and from the model."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    engines = [SelfPlayEngine(game, G, iters, MAXT[game], 0, 0, c_init, alpha, seed=seed, hash_salt=salt, sync_moves=True, single_tree=True,
                              nodes_per_tree=(len(moves) + 1) * (max(iters, 3 * A_OF[game]) + 4) + 64, compact_trees=c,
                              max_tree_sims_per_wave=max_tree_sims, tau=0.0, leaf_batch=K, lib_path=lib_path) for c in compact]
    models = {s: Tree(oracle, game, K, seed, slot=s, c_puct_init=c_init, dirichlet_alpha=alpha, hash_salt=salt, max_tree_sims=max_tree_sims) for s in slots}
    sizes, longest = [], 0
    for ply, m in enumerate(list(moves) + [None]):
        want = {}
        for s, model in models.items():
            model.run(iters)
            want[s] = model_export(model)
        for eng, c in zip(engines, compact):
            eng.start_search(); eng.run_move()
            trees = eng.read_trees(list(slots))
            st = eng.root_stats()
            pv = eng.principal_variations(pv_len, first_action=st["chosen"])
            pv_free = eng.principal_variations(pv_len)
            pv_short = eng.principal_variations(2, first_action=st["chosen"])
            # a first step that is NOT the most visited move: the action of every sampled root's last slot (elsewhere: most visited); and one no root has
            other = np.full(G, -1, np.int32)
            for t, s in zip(trees, slots):
                other[s] = t.edges_of(0)["action"][-1]
            pv_other = eng.principal_variations(pv_len, first_action=other)
            for absent in (A_OF[game] + 1, 256 + int(trees[0].edges_of(0)["action"][0]), 1 << 20):      # (never matched through its low 8 bits)
                pv_none = eng.principal_variations(pv_len, first_action=np.full(G, absent, np.int32))
                assert not pv_none["len"].any() and not pv_none["N"].any(), absent
            for t, s in zip(trees, slots):
                what = f"{game} K {K} compact {c} ply {ply} slot {s}"
                assert t.slot == s
                assert_trees_equal(t.nodes, t.edges, *want[s], what=what)
                assert_consistent(t, what)
                for src in ((t.nodes, t.edges), want[s]):
                    assert_pv_equals(pv, s, host_pv(*src, pv_len, int(st["chosen"][s])), what + " pv")
                    assert_pv_equals(pv_free, s, host_pv(*src, pv_len), what + " pv most visited")
                    assert_pv_equals(pv_short, s, host_pv(*src, 2, int(st["chosen"][s])), what + " pv max_len 2")
                    assert_pv_equals(pv_other, s, host_pv(*src, pv_len, int(other[s])), what + " pv from the last slot")
                assert pv_other["actions"][s, 0] == other[s], what
                longest = max(longest, int(pv["len"][s]))
                assert pv["actions"][s, 0] == st["chosen"][s] and pv["len"][s] >= 1, what
                if filters:
                    filter_checks(eng, t, what)
            sizes.append([len(t) for t in trees])
        if m is None:
            break
        for eng in engines:
            eng.apply_moves([m] * G)
        for model in models.values():
            model.play(m)
    for eng in engines:
        eng.close()
    assert longest > 2, "no line was longer than the max_len = 2 of the short call"
    return sizes


def filter_checks(eng, full, what=""):
    for kw in [dict(max_depth=d) for d in (0, 1, 3)] + [dict(min_visits=v) for v in (1, 2, 5)] + [dict(max_depth=3, min_visits=2)]:
        got = eng.read_trees([full.slot], **kw)[0]
        wn, we = filter_export(full.nodes, full.edges, kw.get("max_depth"), kw.get("min_visits", 0))
        assert_trees_equal(got.nodes, got.edges, wn, we, what=f"{what} {kw}")


# ------------------------------------------------------------------------------------------------ leaves in flight
def inflight_case(lib_path, G=4, K=4, launches=3):
    """Connect4 at leaf_batch = K, after the first launches of the first move: the n_reserved of the exported trees of all slots sum to
    stats()["reserved_children"], and every unexpanded edge inside a node's reserved range carries its virtual loss"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine("Connect4", G, 200, 42, 0, 0, 2.5, 0.5, seed=3, hash_salt=2, sync_moves=True, single_tree=True, tau=0.0, leaf_batch=K, lib_path=lib_path)
    eng.start_search()
    seen = 0
    for _ in range(launches):
        eng.run_waves(1)
        trees = eng.read_trees(list(range(G)))
        total = 0
        for t in trees:
            assert_consistent(t)
            total += int(t.nodes["n_reserved"].sum())
            for i in np.flatnonzero(t.nodes["n_reserved"]):
                e = t.edges_of(i)
                lo = int(t.nodes["n_children"][i]); hi = lo + int(t.nodes["n_reserved"][i])
                assert hi <= len(e) and (e["child"][lo:hi] == -1).all() and (e["N"][lo:hi] >= 1).all(), (i, e)
        assert total == eng.stats()["reserved_children"]
        seen = max(seen, total)
    assert seen > G, "no launch left more than one leaf per game in flight"
    eng.close()


# ------------------------------------------------------------------------------------------------ Gumbel
def gumbel_case(lib_path, game, iters, m, K, G, n_moves, seed=23, salt=6):
    """gumbel_batch = 1 and = K: the exports of every slot are equal after every move (arena indices differ, the trees do not), and the root's
    edges scattered by action are root_stats() N / W / P"""
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL, SelfPlayEngine
    A = A_OF[game]
    engs = [SelfPlayEngine(game, G, iters, MAXT[game], 0, 0, 0.0, 0.0, seed=seed, hash_salt=salt, sync_moves=True, single_tree=True, search=SEARCH_GUMBEL,
                           gumbel_m=m, c_visit=50.0, c_scale=1.0, gumbel_batch=k, lib_path=lib_path) for k in (1, K)]
    expanded = 0
    for ply in range(n_moves):
        out = []
        for eng in engs:
            eng.start_search(); eng.run_move()
            out.append((eng.read_trees(list(range(G))), eng.root_stats()))
        (ta, sa), (tb, sb) = out
        np.testing.assert_array_equal(sa["chosen"], sb["chosen"])
        for g in range(G):
            what = f"{game} gumbel_batch {K} ply {ply} slot {g}"
            assert_trees_equal(tb[g].nodes, tb[g].edges, ta[g].nodes, ta[g].edges, what=what)
            assert_consistent(tb[g], what)
            e = tb[g].edges_of(0)
            for f in ("N", "W", "P"):
                dense = np.zeros(A, e[f].dtype); dense[e["action"]] = e[f]
                np.testing.assert_array_equal(dense, sb[f][g], err_msg=f"{what} root {f}")
            expanded += len(tb[g]) - 1
        pv = [eng.principal_variations(5, first_action=s["chosen"]) for eng, (_, s) in zip(engs, out)]
        for k in pv[0]:
            np.testing.assert_array_equal(pv[0][k], pv[1][k])
        for g in range(G):
            assert_pv_equals(pv[1], g, host_pv(tb[g].nodes, tb[g].edges, 5, int(sb["chosen"][g])), f"{game} pv slot {g}")
        for eng in engs:
            eng.apply_moves(None)
    for eng in engs:
        with np.testing.assert_raises(Exception):
            eng.read_trees([0], tree=1)
        eng.close()
    assert expanded > 0


# ------------------------------------------------------------------------------------------------ structure, with game groups
def grouped_case(lib_path, G, n_single, waves=10, seed=5):
    """continuous Connect4 self-play in two game groups: one read_trees call over all slots in shuffled order equals single-slot calls (the first
    n_single of the shuffled order), every tree is consistent, roots of slots in PH_SIMS stand at read_positions()'s ply, and the PVs of all games
    equal the host's line"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine("Connect4", G, 40, 42, 4, 4, 2.5, 0.5, seed=seed, hash_salt=3, ring_capacity=G, game_groups=2, lib_path=lib_path)
    assert eng.stats()["game_groups"] == 2
    eng.run_waves(waves)
    order = np.random.default_rng(1).permutation(G)
    trees = eng.read_trees(order)
    phase = eng.root_stats()["phase"]
    pos = eng.read_positions()
    pv = eng.principal_variations(8)
    n_sims = 0
    for t, g in zip(trees, order):
        assert t.slot == g
        assert_consistent(t, f"slot {g}")
        if phase[g] == PH_SIMS:
            assert len(t) >= 1 and int(t.nodes["n_hist"][0]) == len(pos[g]), g
            n_sims += 1
        assert_pv_equals(pv, g, host_pv(t.nodes, t.edges, 8), f"pv slot {g}")
    assert n_sims > G // 2
    for t, g in list(zip(trees, order))[:n_single]:
        one = eng.read_trees([int(g)])[0]
        assert_trees_equal(one.nodes, one.edges, t.nodes, t.edges, what=f"slot {g} alone")
    # too little capacity on a grouped engine: refused with the totals of all groups, nothing written
    from grok_alpha_zero_amd.engine import TREE_EDGE_DTYPE, TREE_NODE_DTYPE
    tn, te = sum(len(t) for t in trees), sum(len(t.edges) for t in trees)
    nodes = np.zeros(tn, TREE_NODE_DTYPE); edges = np.zeros(te, TREE_EDGE_DTYPE); nf = np.zeros(G + 1, np.int64); ef = np.zeros(G + 1, np.int64)
    o32 = np.ascontiguousarray(order, np.int32)
    rc = eng.L.gaz_engine_read_trees(eng.h, o32.ctypes.data, G, -1, -1, 0, tn - 1, te, nodes.ctypes.data, edges.ctypes.data, nf.ctypes.data, ef.ctypes.data)
    assert rc != 0 and f"{tn} nodes" in eng.L.gaz_engine_last_error(eng.h).decode() and not nodes.view(np.uint8).any() and not edges.view(np.uint8).any()
    assert int(nf[G]) == tn and int(ef[G]) == te
    both = eng.read_trees([int(order[0]), int(order[0])])                 # a slot may be asked for twice
    assert_trees_equal(both[1].nodes, both[1].edges, both[0].nodes, both[0].edges)
    other = eng.read_trees(order[:8], tree=0), eng.read_trees(order[:8], tree=1)
    for a, b, t in zip(other[0], other[1], trees):                        # the runner's tree is one of the game's two
        assert_consistent(a); assert_consistent(b)
        assert any(len(x) == len(t) and np.array_equal(x.nodes, t.nodes) and np.array_equal(x.edges, t.edges) for x in (a, b))
    eng.close()
    return sum(len(t) for t in trees)


def mixed_runner_case(lib_path, G=64, groups=1, waves=40, seed=7):
    """two trees per game, and neighbouring slots at different plies (set_position at staggered histories), so that ONE read_trees(tree=-1) call
    covers games whose running trees differ — inside one wavefront of any per-slot kernel.  Every tree equals the single-slot call and, for a
    slot in the middle of a search, the explicit read of tree = ply parity; nothing is cut (no -4 code without a filter)"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine("Connect4", G, 60, 42, 4, 4, 2.5, 0.5, seed=seed, hash_salt=3, ring_capacity=G, game_groups=groups, lib_path=lib_path)
    assert eng.stats()["game_groups"] == groups
    prefixes = [[], [3], [3, 2], [3, 2, 4]]
    for g in range(G):
        eng.set_position(g, prefixes[(g + g // 16) % 4])
    eng.run_waves(waves)
    slots = np.arange(G)
    trees = eng.read_trees(slots)
    phase, pos = eng.root_stats()["phase"], eng.read_positions()
    by_tree = [eng.read_trees(slots, tree=0), eng.read_trees(slots, tree=1)]
    pv = eng.principal_variations(8)
    seen = [0, 0]
    for g, t in enumerate(trees):
        what = f"slot {g}"
        assert_consistent(t, what)
        assert not (t.edges["child"] == FILTERED).any(), what
        one = eng.read_trees([g])[0]
        assert_trees_equal(t.nodes, t.edges, one.nodes, one.edges, what=what + " alone")
        assert_pv_equals(pv, g, host_pv(t.nodes, t.edges, 8), what + " pv")
        if phase[g] == PH_SIMS:
            r = len(pos[g]) % 2                                         # the first player's tree runs the even plies
            assert len(t) > 1 and int(t.nodes["n_hist"][0]) == len(pos[g]), what
            assert_trees_equal(t.nodes, t.edges, by_tree[r][g].nodes, by_tree[r][g].edges, what=f"{what} tree {r}")
            assert len(by_tree[1 - r][g]) != len(t) or not np.array_equal(by_tree[1 - r][g].edges, t.edges), what     # (the other tree is another tree)
            if g < 64:
                seen[r] += 1
    assert min(seen) >= 8, f"the first 64 slots do not mix runners: {seen}"
    eng.close()
    return seen


# ------------------------------------------------------------------------------------------------ the MCTS classes
def _same_node(a, b, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    assert a.is_terminal == b.is_terminal and a.current_player == b.current_player and len(a.children) == len(b.children), what
    for f in ("child_visits", "child_values", "child_prob_priors"):
        np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg=f"{what} {f}")
    for i, (x, y) in enumerate(zip(a.children, b.children)):
        _same_node(x, y, f"{what}/{i}")


def mcts_class_case(oracle, lib_path, game="Connect4", iters=100, moves=(3, 2, 3), K=8, seed=5, salt=17):
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.mcts import MCTS
    g = GAMES[game]()
    mcts = MCTS(g, None, c_puct_init=2.5, dirichlet_alpha=0.5, tau=0.0, seed=seed, hash_salt=salt, leaf_batch=K, lib_path=lib_path)
    assert mcts.root is None
    with np.testing.assert_raises(RuntimeError):
        mcts.pv(4)
    model = Tree(oracle, game, K, seed, c_puct_init=2.5, dirichlet_alpha=0.5, hash_salt=salt, max_tree_sims=4)
    for m in list(moves) + [None]:
        move, rows = mcts.run(iteration_limit=iters, use_bar=False)
        model.run(iters)
        root = mcts.root
        by_action = {GAMES[game].action_to_index(r[0]): r for r in rows}
        assert root.parent is None and root.is_terminal is None and root.current_player == -g.next_player and len(root.action_history) == len(g.action_history)
        assert root.child_visits.dtype == np.uint32 and root.child_values.dtype == np.float32
        acts = [GAMES[game].action_to_index(a) for a in root.child_actions]
        np.testing.assert_array_equal(root.child_visits, np.array([by_action[a][4] for a in acts], np.uint32))
        np.testing.assert_array_equal(root.child_values, np.array([by_action[a][3] for a in acts], np.float32))
        np.testing.assert_array_equal(root.child_prob_priors, np.array([by_action[a][5] for a in acts], np.float32))
        assert all(root.visits == by_action[a][6] for a in acts) and root.visits == model.root_visits
        assert [c.is_terminal for c in root.children] == [by_action[a][7] for a in acts[:len(root.children)]]
        np.testing.assert_array_equal(root.board, g.board)
        for i, c in enumerate(root.children):                          # the children's arrays are the model's
            mc = model.root.child[i]
            assert c.parent is root and c.child_id == i
            if isinstance(mc, _Node):
                np.testing.assert_array_equal(c.child_visits, mc.N); np.testing.assert_array_equal(c.child_values, mc.W)
                np.testing.assert_array_equal(c.child_prob_priors, mc.P); np.testing.assert_array_equal(c.board, mc.board)
                assert c.current_player == mc.player and len(c.children) == mc.n_children and c.is_terminal is None
                assert [GAMES[game].action_to_index(a) for a in c.action_history] == mc.hist
            else:
                assert c.is_terminal == (g.next_player if mc == WIN else 0) and c.children == []
        pv = mcts.pv(6)
        tree = mcts._eng.read_trees([0])[0]
        line = host_pv(tree.nodes, tree.edges, 6, GAMES[game].action_to_index(move))
        assert [(GAMES[game].action_to_index(a), n, np.float32(w)) for a, n, w in pv] == line and len(pv) >= 1
        assert GAMES[game].action_to_index(pv[0][0]) == GAMES[game].action_to_index(move)
        assert len(mcts.pv(1)) == 1
        if m is None:
            break
        act = GAMES[game].index_to_action(m)
        g.do_action(act); mcts.prune_tree(act); model.play(m)
        with np.testing.assert_raises(RuntimeError):                    # the line belongs to a finished run() of the current root
            mcts.pv(4)
        if isinstance(model.root, _Node) and model.root_visits:
            assert mcts.root.visits == model.root_visits                # carried over by the re-root (MCTS.py:654)
    mcts.close()


def gumbel_class_case(lib_path, game="Connect4", iters=32, m=7, K=4, moves=(3, 2), seed=9, salt=4):
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.mcts import MCTS_Gumbel
    games = [GAMES[game](), GAMES[game]()]
    searches = [MCTS_Gumbel(g, None, use_gumbel_noise=True, m=m, c_visit=50.0, c_scale=1.0, seed=seed, hash_salt=salt, gumbel_batch=k, lib_path=lib_path)
                for g, k in zip(games, (1, K))]
    for mv in list(moves) + [None]:
        res = [s.run(iteration_limit=iters, use_bar=False) for s in searches]
        roots = [s.root for s in searches]
        _same_node(roots[0], roots[1], "root")
        move, rows = res[1]
        root = roots[1]
        by_action = {GAMES[game].action_to_index(r[0]): r for r in rows}
        acts = [GAMES[game].action_to_index(a) for a in root.child_actions]
        assert len(root.children) == len(acts) == len(rows)
        np.testing.assert_array_equal(root.child_visits, np.array([by_action[a][4] for a in acts], np.uint32))
        np.testing.assert_array_equal(root.child_values, np.array([by_action[a][3] for a in acts], np.float32))
        np.testing.assert_array_equal(root.child_prob_priors, np.array([by_action[a][5] for a in acts], np.float32))
        np.testing.assert_array_equal(root.child_logit_priors, root.child_prob_priors)
        assert root.visits == rows[0][6]
        assert [None if c is None else c.is_terminal for c in root.children] == [by_action[a][7] for a in acts]
        assert any(c is not None for c in root.children)
        pv = [s.pv(5) for s in searches]
        assert pv[0] == pv[1] and GAMES[game].action_to_index(pv[1][0][0]) == GAMES[game].action_to_index(move)
        if mv is None:
            break
        for g, s in zip(games, searches):
            act = GAMES[game].index_to_action(mv)
            g.do_action(act); s.prune_tree(act)
    for s in searches:
        s.close()

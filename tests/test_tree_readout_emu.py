"""CPU suite: reading search trees back (gaz_engine_read_trees / gaz_engine_read_pv, SelfPlayEngine.read_trees / principal_variations,
MCTS.root / MCTS.pv) on the emulation build of the device code.  The PUCT trees are held against the whole-tree model of
tests/leaf_batch_model.py, node for node and edge for edge; the case bodies are tests/tree_cases.py, shared with the -m gpu suite.
Bit-equal everywhere: no tolerance."""
import ctypes as C

import numpy as np
import pytest

import tree_cases as TC
from selfplay_support import emu_lib  # noqa: F401


# ------------------------------------------------------------------------------------------------ whole-tree parity, PUCT
def test_tictactoe_whole_game_equals_model(emu_lib, oracle):
    """27 iterations a move over a whole drawn game with wins in one left standing: terminal roots, terminal parents, draws; filters too"""
    sizes = TC.puct_case(oracle, emu_lib, "TicTacToe", 1, 27, TC.TTT_DRAWN_GAME, 3, (0, 2), c_init=1.25, alpha=1.0, filters=True)
    assert len(sizes) == 9 and max(max(s) for s in sizes) > 20


@pytest.mark.parametrize("K", [1, 8])
def test_connect4_equals_model(emu_lib, oracle, K):
    sizes = TC.puct_case(oracle, emu_lib, "Connect4", K, 200, [3, 3, 2], 2, (0, 1), filters=True)
    assert min(min(s) for s in sizes) > 100


@pytest.mark.parametrize("K", [1, 16])
def test_gomoku_equals_model_with_and_without_compaction(emu_lib, oracle, K):
    """compact_trees = -1 and 1 re-root differently (the root keeps its arena index and a stale header / the subtree is copied): the export is the same"""
    TC.puct_case(oracle, emu_lib, "Gomoku", K, 695, [112, 113], 2, (1,), compact=(-1, 1), alpha=0.05, max_tree_sims=4)


def test_leaves_in_flight(emu_lib):
    TC.inflight_case(emu_lib)


# ------------------------------------------------------------------------------------------------ Gumbel
@pytest.mark.parametrize("game,iters,m,K,moves", [("Connect4", 32, 7, 7, 4), ("Gomoku", 48, 16, 5, 3)])
def test_gumbel_batch_exports_equal(emu_lib, game, iters, m, K, moves):
    TC.gumbel_case(emu_lib, game, iters, m, K, 3, moves)


# ------------------------------------------------------------------------------------------------ structure, with game groups
def test_grouped_structure_and_order(emu_lib):
    assert TC.grouped_case(emu_lib, 64, 64) > 64


@pytest.mark.parametrize("groups", [1, 2])
def test_one_call_over_games_with_different_running_trees(emu_lib, groups):
    TC.mixed_runner_case(emu_lib, 64, groups)


# ------------------------------------------------------------------------------------------------ errors
def _engine(emu_lib, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    args = dict(seed=1, hash_salt=2, sync_moves=True, single_tree=True, tau=0.0, lib_path=emu_lib); args.update(kw)
    return SelfPlayEngine("Connect4", 4, 60, 42, 0, 0, 2.5, 0.5, **args)


def test_refusals_name_the_argument(emu_lib):
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL, EngineError
    eng = _engine(emu_lib)
    for bad in ([4], [-1], [0, 1, 99]):
        with pytest.raises(EngineError, match="slots"):
            eng.read_trees(bad)
    with pytest.raises(EngineError, match="tree = 1.*single_tree"):
        eng.read_trees([0], tree=1)
    with pytest.raises(EngineError, match="tree = 1.*single_tree"):
        eng.principal_variations(4, tree=1)
    with pytest.raises(EngineError, match="tree must be"):
        eng.read_trees([0], tree=2)
    for n in (0, -3):
        with pytest.raises(EngineError, match="max_len"):
            eng.principal_variations(n)
    nf = np.zeros(2, np.int64); ef = np.zeros(2, np.int64); s = np.zeros(1, np.int32)
    assert eng.L.gaz_engine_read_trees(eng.h, s.ctypes.data, -1, -1, -1, 0, 0, 0, None, None, nf.ctypes.data, ef.ctypes.data) != 0
    assert b"n_slots" in eng.L.gaz_engine_last_error(eng.h)
    assert eng.read_trees([]) == []
    eng.close()
    g = _engine(emu_lib, search=SEARCH_GUMBEL, gumbel_m=4)
    with pytest.raises(EngineError, match="tree = 1.*Gumbel"):
        g.read_trees([0], tree=1)
    g.close()


def test_counting_call_before_any_search_returns_zeros(emu_lib):
    eng = _engine(emu_lib)
    s = np.arange(4, dtype=np.int32); nf = np.full(5, -7, np.int64); ef = np.full(5, -7, np.int64)
    assert eng.L.gaz_engine_read_trees(eng.h, s.ctypes.data, 4, -1, -1, 0, 0, 0, None, None, nf.ctypes.data, ef.ctypes.data) == 0
    assert not nf.any() and not ef.any()
    assert [len(t) for t in eng.read_trees(s)] == [0, 0, 0, 0]
    pv = eng.principal_variations(3)
    assert not pv["len"].any() and not pv["N"].any()
    eng.close()


def test_short_capacity_writes_nothing(emu_lib):
    from grok_alpha_zero_amd.engine import TREE_EDGE_DTYPE, TREE_NODE_DTYPE
    eng = _engine(emu_lib)
    eng.start_search(); eng.run_move()
    s = np.array([2, 0], np.int32); nf = np.zeros(3, np.int64); ef = np.zeros(3, np.int64)
    assert eng.L.gaz_engine_read_trees(eng.h, s.ctypes.data, 2, -1, -1, 0, 0, 0, None, None, nf.ctypes.data, ef.ctypes.data) == 0
    n_nodes, n_edges = int(nf[2]), int(ef[2])
    assert n_nodes > 60 and n_edges > n_nodes
    for short_nodes, short_edges in ((1, 0), (0, 1), (n_nodes, n_edges)):
        nodes = np.zeros(n_nodes + 1, TREE_NODE_DTYPE); edges = np.zeros(n_edges + 1, TREE_EDGE_DTYPE)      # + a guard record behind each array
        nodes.view(np.uint8)[:] = 0xAB; edges.view(np.uint8)[:] = 0xCD
        nf[:] = 0; ef[:] = 0
        rc = eng.L.gaz_engine_read_trees(eng.h, s.ctypes.data, 2, -1, -1, 0, n_nodes - short_nodes, n_edges - short_edges, nodes.ctypes.data, edges.ctypes.data,
                                         nf.ctypes.data, ef.ctypes.data)
        assert rc != 0 and (nodes.view(np.uint8) == 0xAB).all() and (edges.view(np.uint8) == 0xCD).all()
        msg = eng.L.gaz_engine_last_error(eng.h).decode()
        assert f"{n_nodes} nodes" in msg and f"{n_edges} edges" in msg and "max_nodes" in msg and "max_edges" in msg
        assert int(nf[2]) == n_nodes and int(ef[2]) == n_edges
    nodes = np.zeros(n_nodes + 1, TREE_NODE_DTYPE); edges = np.zeros(n_edges + 1, TREE_EDGE_DTYPE)
    nodes.view(np.uint8)[:] = 0xAB; edges.view(np.uint8)[:] = 0xCD
    assert eng.L.gaz_engine_read_trees(eng.h, s.ctypes.data, 2, -1, -1, 0, n_nodes, n_edges, nodes.ctypes.data, edges.ctypes.data, nf.ctypes.data, ef.ctypes.data) == 0
    assert (nodes[n_nodes:].view(np.uint8) == 0xAB).all() and (edges[n_edges:].view(np.uint8) == 0xCD).all()      # the exact capacity: guards untouched
    t = eng.read_trees(s)
    np.testing.assert_array_equal(nodes[:n_nodes], np.concatenate([t[0].nodes, t[1].nodes]))
    np.testing.assert_array_equal(edges[:n_edges], np.concatenate([t[0].edges, t[1].edges]))
    assert (nodes["reserved_"][:n_nodes] == 0).all()
    with pytest.raises(Exception, match="both"):
        eng._ck(eng.L.gaz_engine_read_trees(eng.h, s.ctypes.data, 2, -1, -1, 0, n_nodes, n_edges, nodes.ctypes.data, None, nf.ctypes.data, ef.ctypes.data))
    eng.close()


def test_searchtree_accessors(emu_lib):
    eng = _engine(emu_lib)
    eng.start_search(); eng.run_move()
    t = eng.read_trees([1])[0]
    kids = t.children(0)
    assert kids == list(range(1, 1 + len(kids))) and len(t.edges_of(0)) == t.nodes["n_actions"][0]
    deep = int(np.argmax(t.nodes["depth"]))
    path = t.path_actions(deep)
    assert len(path) == t.nodes["depth"][deep] and path[-1] == t.nodes["action"][deep] and t.path_actions(0) == []
    assert eng.probe_rules([path])["winner"][0] == -2                # a legal line from the empty board
    eng.close()


# ------------------------------------------------------------------------------------------------ the MCTS classes
def test_mcts_root_and_pv(emu_lib, oracle):
    TC.mcts_class_case(oracle, emu_lib)


def test_mcts_gumbel_root_and_pv(emu_lib):
    TC.gumbel_class_case(emu_lib)

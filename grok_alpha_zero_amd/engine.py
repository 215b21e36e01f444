"""ctypes binding of libgaz_engine.so (C ABI: include/gaz_engine.h) — the MI355X batched self-play engine.

The library is the hipcc build in this package directory; if it is missing the import of this module's
`load_library()` raises — there is no CPU fallback on the product path.  (tests/ may hand an explicit
`lib_path` to exercise the host logic against the one-lane CPU emulation build under tests/emu.)
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_PKG, "libgaz_engine.so")

GAME_IDS = {"TicTacToe": 0, "Connect4": 1, "Gomoku": 2}
GAME_DIMS = {0: (3, 3, 2, 9), 1: (6, 7, 4, 7), 2: (15, 15, 2, 225)}  # H, W, C, A
SEARCH_PUCT, SEARCH_GUMBEL = 0, 1
EVAL_HASH, EVAL_RESNET, EVAL_EXTERNAL = 0, 1, 2
PH_WAIT_HOST, PH_HALT, PH_IDLE = 5, 8, 9
PH_FAULT = 10                 # the game raised the engine's device error (gaz_engine.h "Capacity limits and the device error"): it stays where it is


ABI_VERSION = 10              # GAZ_ENGINE_ABI_VERSION of include/gaz_engine.h this binding was written against


class EngineConfig(C.Structure):       # gaz_engine_config — tests/test_abi.py checks names, order and sizeof against the header
    _fields_ = [("struct_size", C.c_uint32), ("game", C.c_int32), ("search", C.c_int32), ("n_games", C.c_int32), ("run_iterations", C.c_int32),
                ("max_actions", C.c_int32), ("num_explore_actions_first", C.c_int32), ("num_explore_actions_second", C.c_int32),
                ("c_puct_init", C.c_double), ("c_puct_base", C.c_double), ("dirichlet_alpha", C.c_double),
                ("dirichlet_epsilon", C.c_double), ("use_dirichlet", C.c_int32), ("create_new_root", C.c_int32),
                ("sync_moves", C.c_int32), ("nodes_per_tree", C.c_int32), ("ring_capacity", C.c_int32),
                ("seed", C.c_uint64), ("slot_offset", C.c_uint32), ("evaluator", C.c_int32), ("hash_salt", C.c_uint32),
                ("device", C.c_int32), ("net_blocks", C.c_int32), ("net_filters", C.c_int32), ("policy_is_logits", C.c_int32),
                ("gumbel_m", C.c_int32), ("c_visit", C.c_double), ("c_scale", C.c_double), ("compact_trees", C.c_int32),
                ("single_tree", C.c_int32), ("n_opening", C.c_int32), ("opening_actions", C.c_int32 * 8),
                ("opening_weights", C.c_double * 8), ("max_tree_sims_per_wave", C.c_int32), ("eval_cache_log2", C.c_int32), ("gumbel_stablemax", C.c_int32), ("fast_find_win", C.c_int32),
                ("no_gumbel_noise", C.c_int32), ("first_game_seq", C.c_uint32), ("games_budget", C.c_int64), ("tau", C.c_double), ("move_time_limit", C.c_double), ("game_groups", C.c_int32),
                ("leaf_batch", C.c_int32), ("gumbel_batch", C.c_int32), ("fast_iterations", C.c_int32), ("full_search_prob", C.c_double),
                ("forced_playouts_k", C.c_double)]


class SearchHyperparams(C.Structure):  # gaz_search_hyperparams
    _fields_ = [("struct_size", C.c_uint32), ("use_dirichlet", C.c_int32), ("c_puct_init", C.c_double), ("c_puct_base", C.c_double),
                ("dirichlet_alpha", C.c_double), ("dirichlet_epsilon", C.c_double), ("tau", C.c_double), ("gumbel_m", C.c_int32),
                ("run_iterations", C.c_int32), ("c_visit", C.c_double), ("c_scale", C.c_double)]


class Tensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.POINTER(C.c_float)), ("numel", C.c_int64)]


class RecordLayout(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("record_bytes", "max_T", "A", "t_pad", "off_hdr", "off_actions", "off_q",
                                         "off_root_visits", "off_evals", "off_policy", "off_N", "off_W", "off_P", "off_move_kind")]


class ResignParams(C.Structure):        # gaz_resign_params
    _fields_ = [("struct_size", C.c_uint32), ("consecutive", C.c_int32), ("min_ply", C.c_int32), ("reserved_", C.c_int32),
                ("threshold", C.c_double), ("no_resign_prob", C.c_double)]


class MatchParams(C.Structure):         # gaz_match_params
    _fields_ = [("struct_size", C.c_uint32), ("mode", C.c_int32), ("hash_salt_b", C.c_uint32), ("reserved_", C.c_int32)]


class BookParams(C.Structure):          # gaz_book_params
    _fields_ = [("struct_size", C.c_uint32), ("n_entries", C.c_int32), ("stride", C.c_int32), ("mode", C.c_int32)]


BOOK_MODES = {None: 0, "game": 1, "pair": 2}    # gaz_book_params.mode: an entry per game, or per pair (slot, 2k), (slot, 2k + 1)
MK_BOOK = 3                                     # move_kind of a ply of an opening-book prefix

NET_A, NET_B, NET_NONE = 0, 1, 255      # gaz_engine_read_batch_network: the network that answers a row of the evaluator batch

MK_KIND_MASK, MK_RESIGNED, MK_WOULD_RESIGN = 3, 0x10, 0x20      # the bits of a record's raw move_kind byte (gaz_record_layout.off_move_kind)
MK_PROVEN = 0x40                                                 # solver (set_solver): the ply ended with a proven root
PROVEN_UNKNOWN, PROVEN_WIN, PROVEN_DRAW, PROVEN_LOSS = 0, 1, 2, 3   # a node's status for the player to move there (SearchTree.proven)


class SampleLayout(C.Structure):        # gaz_sample_layout
    _fields_ = [(n, C.c_int32) for n in ("n_aug", "state_bytes", "A", "max_T")]


# gaz_tree_node / gaz_tree_edge (include/gaz_engine.h): the records of SelfPlayEngine.read_trees
TREE_NODE_DTYPE = np.dtype([(n, np.int32) for n in ("parent", "slot", "depth", "edge0", "n_actions", "n_children", "flags", "n_reserved", "player",
                                                   "action", "n_hist", "reserved_")])
TREE_EDGE_DTYPE = np.dtype([("action", np.int32), ("N", np.uint32), ("W", np.float32), ("P", np.float32), ("raw", np.float32), ("child", np.int32)])
CHILD_NONE, CHILD_DRAW, CHILD_WIN, CHILD_FILTERED = -1, -2, -3, -4
NF_TERMINAL_PARENT = 1

class ScoreTotals(C.Structure):         # gaz_score_totals — tests/test_score_emu.py checks names, order and sizeof against the header
    _fields_ = [("struct_size", C.c_uint32), ("policy_mode", C.c_int32), ("rows", C.c_int64), ("bad_rows", C.c_int64), ("top1", C.c_int64),
                ("value_rows", C.c_int64), ("value_sign", C.c_int64), ("ce_sum", C.c_double), ("entropy_sum", C.c_double), ("se_sum", C.c_double)]


def score_dict(t):
    """gaz_score_totals -> the raw sums and counts and the means derived from them with plain `/` (include/gaz_engine.h "HELD-OUT LOSS"); a
    mean over no rows is NaN.  val_loss is what Train.py monitors: policy cross entropy + value loss for a probability head (modes 0, 2),
    policy KL divergence + value loss for a logits head (modes 1, 3; Train.py:33-48)."""
    nan = float("nan")
    good = int(t.rows) - int(t.bad_rows)
    d = dict(policy_mode=int(t.policy_mode), rows=int(t.rows), bad_rows=int(t.bad_rows), good=good, top1_rows=int(t.top1), value_rows=int(t.value_rows),
             value_sign_rows=int(t.value_sign), ce_sum=float(t.ce_sum), entropy_sum=float(t.entropy_sum), se_sum=float(t.se_sum))
    d["policy_loss"] = d["ce_sum"] / good if good else nan
    d["policy_entropy"] = d["entropy_sum"] / good if good else nan
    d["policy_kl"] = (d["ce_sum"] - d["entropy_sum"]) / good if good else nan
    d["value_loss"] = d["se_sum"] / good if good else nan
    d["top1"] = d["top1_rows"] / good if good else nan
    d["value_sign"] = d["value_sign_rows"] / d["value_rows"] if d["value_rows"] else nan
    d["val_loss"] = (d["policy_kl"] if d["policy_mode"] in (1, 3) else d["policy_loss"]) + d["value_loss"]
    return d


_LIBS = {}


def load_library(lib_path=None):
    path = lib_path or os.environ.get("GAZ_ENGINE_LIB") or DEFAULT_LIB
    if path in _LIBS:
        return _LIBS[path]
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: build the HIP engine first (python -c 'import __graft_entry__ as g; g.build()'); "
                           "there is no CPU fallback")
    import sys
    torch_first = "torch" in sys.modules             # (replay.ReplayWindow.batch_torch: which HIP runtime this process ends up with)
    L = C.CDLL(path)
    L._gaz_torch_first = torch_first
    H = C.c_void_p
    L.gaz_engine_abi_version.restype = C.c_int; L.gaz_engine_config_size.restype = C.c_int
    if L.gaz_engine_abi_version() != ABI_VERSION or L.gaz_engine_config_size() != C.sizeof(EngineConfig):
        raise RuntimeError(f"{path}: ABI version {L.gaz_engine_abi_version()} / config size {L.gaz_engine_config_size()} does not match "
                           f"this binding ({ABI_VERSION} / {C.sizeof(EngineConfig)}): rebuild the library")
    L.gaz_engine_create.argtypes = [C.POINTER(EngineConfig), C.POINTER(H)]
    L.gaz_engine_destroy.argtypes = [H]; L.gaz_engine_destroy.restype = None
    L.gaz_engine_last_error.argtypes = [H]; L.gaz_engine_last_error.restype = C.c_char_p
    L.gaz_engine_load_weights.argtypes = [H, C.POINTER(Tensor), C.c_int32]
    L.gaz_engine_reset_games.argtypes = [H, C.POINTER(C.c_int32), C.c_int32]
    L.gaz_engine_run_move.argtypes = [H, C.POINTER(C.c_int32)]
    L.gaz_engine_get_root_stats.argtypes = [H] + [C.c_void_p] * 8
    L.gaz_engine_apply_moves.argtypes = [H, C.POINTER(C.c_int32)]
    L.gaz_engine_run_waves.argtypes = [H, C.c_int32]
    L.gaz_engine_wave_begin.argtypes = [H]
    L.gaz_engine_wave_end.argtypes = [H]
    L.gaz_engine_batch_ptrs.argtypes = [H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.gaz_engine_read_batch.argtypes = [H, C.c_void_p, C.c_void_p]
    L.gaz_engine_write_outputs.argtypes = [H, C.c_void_p, C.c_void_p]
    L.gaz_engine_batch_rows.argtypes = [H, C.POINTER(C.c_int32)]
    L.gaz_engine_evaluate.argtypes = [H, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_double)]
    L.gaz_engine_record_layout.argtypes = [H, C.POINTER(RecordLayout)]
    L.gaz_engine_drain_finished.argtypes = [H, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    L.gaz_engine_sample_layout.argtypes = [H, C.POINTER(SampleLayout)]
    L.gaz_engine_drain_samples.argtypes = [H, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    if hasattr(L, "gaz_engine_set_sample_weighting"):   # policy surprise weighting, detected by its symbols: a library built before it has none
        L.gaz_engine_set_sample_weighting.argtypes = [H, C.c_double, C.c_double]
        L.gaz_engine_get_sample_weighting.argtypes = [H, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.gaz_engine_drain_samples2.argtypes = [H, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        for f in ("set_sample_weighting", "get_sample_weighting", "drain_samples2"):
            getattr(L, "gaz_engine_" + f).restype = C.c_int
    if hasattr(L, "gaz_engine_set_opening_book"):       # opening book, detected by its symbols: a library built before it has none
        L.gaz_engine_set_opening_book.argtypes = [H, C.POINTER(BookParams), C.c_void_p, C.c_void_p]
        L.gaz_engine_get_opening_book.argtypes = [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.gaz_engine_read_book_counts.argtypes = [H, C.c_void_p, C.POINTER(C.c_uint64)]
        for f in ("set_opening_book", "get_opening_book", "read_book_counts"):
            getattr(L, "gaz_engine_" + f).restype = C.c_int
    L.gaz_engine_get_stats.argtypes = [H, C.POINTER(C.c_uint64)]
    L.gaz_engine_synchronize.argtypes = [H]
    L.gaz_engine_timing_reset.argtypes = [H, C.c_int32]
    L.gaz_engine_set_position.argtypes = [H, C.c_int32, C.POINTER(C.c_int32), C.c_int32]
    L.gaz_engine_set_search_params.argtypes = [H, C.c_int32, C.c_int32]
    L.gaz_engine_stop_search.argtypes = [H, C.c_int32]
    L.gaz_engine_start_search.argtypes = [H]
    L.gaz_engine_set_hyperparams.argtypes = [H, C.POINTER(SearchHyperparams)]
    L.gaz_engine_set_resignation.argtypes = [H, C.POINTER(ResignParams)]
    L.gaz_engine_get_resign_stats.argtypes = [H, C.POINTER(C.c_uint64)]
    L.gaz_engine_set_eval_symmetry.argtypes = [H, C.c_int32]
    L.gaz_engine_get_eval_symmetry.argtypes = [H, C.POINTER(C.c_int32)]
    L.gaz_engine_read_batch_symmetry.argtypes = [H, C.c_void_p]
    L.gaz_engine_set_solver.argtypes = [H, C.c_int32]
    L.gaz_engine_get_solver.argtypes = [H, C.POINTER(C.c_int32)]
    L.gaz_engine_get_solver_stats.argtypes = [H, C.POINTER(C.c_uint64)]
    L.gaz_engine_set_match.argtypes = [H, C.POINTER(MatchParams)]
    L.gaz_engine_get_match.argtypes = [H, C.POINTER(C.c_int32)]
    L.gaz_engine_load_weights_b.argtypes = [H, C.POINTER(Tensor), C.c_int32]
    L.gaz_engine_read_batch_network.argtypes = [H, C.c_void_p]
    L.gaz_engine_get_match_stats.argtypes = [H, C.POINTER(C.c_uint64)]
    L.gaz_engine_get_match_timing.argtypes = [H, C.POINTER(C.c_double)]
    L.gaz_engine_probe_rules.argtypes = [H, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 7
    if hasattr(L, "gaz_engine_probe_det"):              # detected by its symbol: a library built before it has none
        L.gaz_engine_probe_det.argtypes = [H, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.gaz_engine_probe_det.restype = C.c_int
    if hasattr(L, "gaz_engine_score_outputs"):          # held-out loss, detected by its symbols: a library built before it has none
        L.gaz_score_totals_size.argtypes = []; L.gaz_score_totals_size.restype = C.c_int
        L.gaz_engine_score_outputs.argtypes = [H] + [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.POINTER(ScoreTotals)] + [C.c_void_p] * 4
        L.gaz_engine_score_replay.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(ScoreTotals)] + [C.c_void_p] * 4 + [C.POINTER(C.c_double)]
        L.gaz_engine_score_rows_timed.argtypes = [H, C.c_int32, C.POINTER(C.c_double)]
        for f in ("score_outputs", "score_replay", "score_rows_timed"):
            getattr(L, "gaz_engine_" + f).restype = C.c_int
        if L.gaz_score_totals_size() != C.sizeof(ScoreTotals):
            raise RuntimeError(f"{path}: gaz_score_totals has {L.gaz_score_totals_size()} bytes in the library, {C.sizeof(ScoreTotals)} in this binding: rebuild the library")
    L.gaz_engine_set_fused_wave.argtypes = [H, C.c_int32]
    L.gaz_engine_debug_fused_fault.argtypes = [H, C.c_int32]
    L.gaz_engine_read_positions.argtypes = [H, C.c_void_p, C.c_void_p, C.c_int32]
    L.gaz_engine_repack.argtypes = [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.gaz_engine_read_trees.argtypes = [H, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_int64, C.c_int64] + [C.c_void_p] * 4
    L.gaz_engine_read_pv.argtypes = [H, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 4
    L.gaz_engine_read_head_features.argtypes = [H, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.gaz_engine_dominant_kernel.argtypes = [H, C.c_char_p, C.c_int32, C.POINTER(C.c_double)]
    L.gaz_engine_timing_get.argtypes = [H, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    for f in ("create", "load_weights", "reset_games", "run_move", "get_root_stats", "apply_moves", "run_waves", "wave_begin",
              "wave_end", "batch_ptrs", "read_batch", "write_outputs", "batch_rows", "evaluate", "record_layout", "drain_finished", "sample_layout", "drain_samples", "get_stats",
              "synchronize", "timing_reset", "timing_get", "dominant_kernel", "set_position", "set_search_params", "start_search", "stop_search",
              "set_hyperparams", "set_resignation", "get_resign_stats", "set_eval_symmetry", "get_eval_symmetry", "read_batch_symmetry", "set_solver", "get_solver", "get_solver_stats", "set_match", "get_match", "load_weights_b", "read_batch_network", "get_match_stats", "get_match_timing", "probe_rules", "read_head_features", "set_fused_wave", "debug_fused_fault", "read_positions", "repack", "read_trees", "read_pv"):
        getattr(L, "gaz_engine_" + f).restype = C.c_int
    _LIBS[path] = L
    return L


class EngineError(RuntimeError):
    pass


# the ops of SelfPlayEngine.probe_det (csrc/det_probe.hpp lists the words each reads and writes)
(DP_PHILOX, DP_DRAW, DP_UNIT, DP_DLOG, DP_DEXP, DP_DPOW, DP_DSQRT, DP_DDIV, DP_PUCT_C, DP_PUCT_FACTORS, DP_SAMPLE) = range(11)
(DP_SUM_F32, DP_SUM_F64, DP_PUCT_SCORES, DP_SOFTMAX, DP_PI) = range(16, 21)
DP_WHOLE_WAVE = 0x100        # a team op of a small board on a whole wavefront instead of a 16-lane team


class SampleBatch:
    """The finished games of one SelfPlayEngine.drain_samples() call as training samples (include/gaz_engine.h, gaz_engine_drain_samples):
    `games` int32 [n, 6] (T, winner, slot, game_seq, first row, plies left out), `boards` int8 [n_aug, R, H, W, C], `policies` f32 [n_aug, R, A],
    `values` f32 [R, 1]; rows = the games in the order handed out, plies in order.  With playout cap randomisation (fast_iterations) the
    plies of fast searches give no row: game i has T - games[i, 5] rows.  With policy surprise weighting (set_sample_weighting) a ply gives
    0, 1 or more adjacent rows: games[i, 5] counts the plies that gave none, game i has rows_of(i) rows, and `plies` (uint8 [R], with
    drain_samples(with_plies=True), else None) is the ply of every row."""

    def __init__(self, games, boards, policies, values, plies=None):
        self.games, self.boards, self.policies, self.values, self.plies = games, boards, policies, values, plies

    def rows_of(self, i):
        """the rows of game i: the difference of successive first rows, the batch's rows closing the last one"""
        end = int(self.games[i + 1, 4]) if i + 1 < self.n else int(self.games[0, 4]) + self.rows
        return end - int(self.games[i, 4])

    @property
    def n(self):
        return self.games.shape[0]

    def __len__(self):
        return self.games.shape[0]

    @property
    def rows(self):
        return self.values.shape[0]

    @property
    def nbytes(self):
        return self.games.nbytes + self.boards.nbytes + self.policies.nbytes + self.values.nbytes

    def copy(self):
        """an owning, compact copy (what another thread may keep)"""
        return SampleBatch(self.games.copy(), self.boards.copy(), self.policies.copy(), self.values.copy(), None if self.plies is None else self.plies.copy())

    def game(self, i):
        """game i as ReplayStore.append_game takes it: (boards [n_aug, n, H, W, C], policies [n_aug, n, A], values [n_aug, n, 1],
        game_length, n_positions, winner) — views, no copy.  n = the game's rows (T minus the plies of fast searches; rows_of(i) with
        policy surprise weighting); game_length and n_positions stay T, the plies played"""
        T, winner, r0 = int(self.games[i, 0]), int(self.games[i, 1]), int(self.games[i, 4]) - int(self.games[0, 4])
        n = self.rows_of(i)
        v = np.broadcast_to(self.values[None, r0:r0 + n], (self.policies.shape[0], n, 1))
        return self.boards[:, r0:r0 + n], self.policies[:, r0:r0 + n], v, T, T, winner


class SearchTree:
    """One search tree as SelfPlayEngine.read_trees returns it (include/gaz_engine.h, gaz_engine_read_trees): `nodes` (TREE_NODE_DTYPE) in
    breadth-first order from the root — index 0, parent -1 — and `edges` (TREE_EDGE_DTYPE), one per child slot of every node: node i owns
    edges[edge0 : edge0 + n_actions].  An edge's `child` is the index of the child node, or CHILD_NONE / CHILD_DRAW / CHILD_WIN /
    CHILD_FILTERED.  `slot` = the engine slot it was read from.  A slot without a tree gives empty arrays."""

    def __init__(self, slot, nodes, edges):
        self.slot, self.nodes, self.edges = int(slot), nodes, edges

    def __len__(self):
        return self.nodes.shape[0]

    def edges_of(self, i):
        """the edge records of node i, in slot order (a view)"""
        n = self.nodes[i]
        return self.edges[int(n["edge0"]):int(n["edge0"]) + int(n["n_actions"])]

    def children(self, i):
        """indices of node i's child nodes that are part of this export, in slot order"""
        c = self.edges_of(i)["child"]
        return [int(x) for x in c[c >= 0]]

    @property
    def proven(self):
        """int32 [len(self)]: what the solver (SelfPlayEngine.set_solver) proved for the player to move at every node — PROVEN_UNKNOWN (0),
        PROVEN_WIN (1), PROVEN_DRAW (2), PROVEN_LOSS (3): bits 1-2 of the node's flags, and for a terminal parent (whose status is not
        stored) a win if one of its moves wins, else a draw"""
        out = ((self.nodes["flags"] >> 1) & 3).astype(np.int32)
        for i in np.flatnonzero(self.nodes["flags"] & NF_TERMINAL_PARENT):
            out[i] = PROVEN_WIN if np.any(self.edges_of(i)["child"] == CHILD_WIN) else PROVEN_DRAW
        return out

    def path_actions(self, i):
        """action indices that lead from the root to node i"""
        out = []
        while self.nodes[i]["parent"] >= 0:
            out.append(int(self.nodes[i]["action"])); i = int(self.nodes[i]["parent"])
        return out[::-1]


class SelfPlayEngine:
    """G concurrent self-play games on one GPU.  Mirrors, per game, what Self_Play(...).play() does in the
    reference (Self_Play.py:16-208) with MCTS.run / prune_tree underneath (MCTS.py:528-671)."""

    def __init__(self, game, n_games, run_iterations, max_actions, num_explore_actions_first, num_explore_actions_second,
                 c_puct_init, dirichlet_alpha, seed, *, c_puct_base=19652.0, dirichlet_epsilon=0.25, use_dirichlet=True,
                 create_new_root=False, sync_moves=False, nodes_per_tree=0, ring_capacity=None, slot_offset=0,
                 evaluator=EVAL_HASH, hash_salt=0, device=0, net_blocks=0, net_filters=128, search=SEARCH_PUCT,
                 policy_is_logits=False, max_tree_sims_per_wave=0, gumbel_m=0, c_visit=50.0, c_scale=1.0,
                 compact_trees=0, single_tree=False, opening_actions=None, eval_cache_log2=0, gumbel_stablemax=False, fast_find_win=False,
                 use_gumbel_noise=True, first_game_seq=0, games_budget=0, tau=-1.0, move_time_limit=0.0, game_groups=0, leaf_batch=1, gumbel_batch=1,
                 fast_iterations=0, full_search_prob=0.0, forced_playouts_k=0.0,
                 resign_threshold=0.0, resign_consecutive=1, resign_min_ply=0, no_resign_prob=0.0, eval_symmetry=False, solver=False,
                 sample_weighting=None, lib_path=None):
        self.L = load_library(lib_path)
        self.game_id = GAME_IDS[game] if isinstance(game, str) else int(game)
        self.H, self.W, self.Cc, self.A = GAME_DIMS[self.game_id]
        self.n_games = n_games
        if ring_capacity is None:
            ring_capacity = 2 * n_games
        self.cfg = EngineConfig(struct_size=C.sizeof(EngineConfig), game=self.game_id, search=search, n_games=n_games,
                                run_iterations=run_iterations, max_actions=max_actions, num_explore_actions_first=num_explore_actions_first,
                                num_explore_actions_second=num_explore_actions_second, c_puct_init=c_puct_init, c_puct_base=c_puct_base,
                                dirichlet_alpha=dirichlet_alpha, dirichlet_epsilon=dirichlet_epsilon, use_dirichlet=int(use_dirichlet),
                                create_new_root=int(create_new_root), sync_moves=int(sync_moves), nodes_per_tree=nodes_per_tree,
                                ring_capacity=ring_capacity, seed=seed, slot_offset=slot_offset, evaluator=evaluator, hash_salt=hash_salt,
                                device=device, net_blocks=net_blocks, net_filters=net_filters, policy_is_logits=int(policy_is_logits),
                                gumbel_m=gumbel_m, c_visit=c_visit, c_scale=c_scale, compact_trees=compact_trees, single_tree=int(single_tree),
                                max_tree_sims_per_wave=max_tree_sims_per_wave, eval_cache_log2=int(eval_cache_log2),
                                gumbel_stablemax=int(gumbel_stablemax), fast_find_win=int(fast_find_win),
                                no_gumbel_noise=int(not use_gumbel_noise), first_game_seq=int(first_game_seq), games_budget=int(games_budget),
                                tau=float(tau), move_time_limit=float(move_time_limit or 0.0), game_groups=int(game_groups),
                                leaf_batch=int(leaf_batch), gumbel_batch=int(gumbel_batch),
                                # playout cap randomisation: a move runs run_iterations with probability full_search_prob, else fast_iterations
                                fast_iterations=int(fast_iterations), full_search_prob=float(full_search_prob),
                                # forced playouts + policy target pruning on full PUCT moves (KataGo: k = 2); 0 = off
                                forced_playouts_k=float(forced_playouts_k or 0.0))
        for i, (a, w) in enumerate(opening_actions or []):       # [(action index, weight)] — train_config["opening_actions"]
            self.cfg.opening_actions[i] = int(a); self.cfg.opening_weights[i] = float(w); self.cfg.n_opening = i + 1
        self.h = C.c_void_p()
        if self.L.gaz_engine_create(C.byref(self.cfg), C.byref(self.h)):
            raise EngineError(self.L.gaz_engine_last_error(None).decode())
        self.layout = RecordLayout()
        self._ck(self.L.gaz_engine_record_layout(self.h, C.byref(self.layout)))
        # rows of the evaluator batch: n_games * K with leaf_batch = K > 1 (row g * K + j = leaf j of game g) or gumbel_batch = K > 1 (row g * K + j =
        # candidate j of game g's current chunk of sequential halving)
        self.batch_rows = n_games
        if self.cfg.game_groups <= 1 and (self.cfg.leaf_batch > 1 or self.cfg.gumbel_batch > 1):
            r = C.c_int32()
            self._ck(self.L.gaz_engine_batch_rows(self.h, C.byref(r)))
            self.batch_rows = int(r.value)
        if resign_threshold:                         # (0 = off, the state of a new engine)
            try:
                self.set_resignation(resign_threshold, resign_consecutive, resign_min_ply, no_resign_prob)
            except EngineError:
                self.close()
                raise
        if eval_symmetry:                            # (off = the state of a new engine)
            self.set_eval_symmetry(True)
        if solver:                                   # (likewise)
            try:
                self.set_solver(True)
            except EngineError:
                self.close()
                raise
        if sample_weighting and sample_weighting[0]:     # (lambda, fast_factor); lambda 0 = off, the state of a new engine
            try:
                self.set_sample_weighting(*sample_weighting)
            except (EngineError, ValueError):
                self.close()
                raise

    def _ck(self, rc):
        if rc:
            raise EngineError(self.L.gaz_engine_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self.L.gaz_engine_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights ------------------------------------------------------------------------------------
    def _load(self, fn, named_arrays):
        keep = []
        arr = (Tensor * len(named_arrays))()
        for i, (name, a) in enumerate(named_arrays.items()):
            a = np.ascontiguousarray(a, np.float32)
            keep.append(a)
            arr[i] = Tensor(name.encode(), a.ctypes.data_as(C.POINTER(C.c_float)), a.size)
        self._ck(fn(self.h, arr, len(named_arrays)))

    def load_weights(self, named_arrays):
        self._load(self.L.gaz_engine_load_weights, named_arrays)

    def load_weights_b(self, named_arrays):
        """the weights of network B of a match (set_match): the names and shapes of load_weights"""
        self._load(self.L.gaz_engine_load_weights_b, named_arrays)

    def evaluate(self, states_i8, repeats=0):
        """Evaluator probe (Compute_Speed.py:40-63): states int8 [n,H,W,C] -> (policy [n,A], value [n], ms per batch)."""
        x = np.ascontiguousarray(states_i8, np.int8)
        n = x.shape[0]
        pol = np.zeros((n, self.A), np.float32); val = np.zeros(n, np.float32); ms = C.c_double()
        self._ck(self.L.gaz_engine_evaluate(self.h, x.ctypes.data, n, pol.ctypes.data, val.ctypes.data, repeats, C.byref(ms)))
        return pol, val, ms.value

    # ---- held-out loss (include/gaz_engine.h "HELD-OUT LOSS") ---------------------------------
    def _score_call(self, fn, n, per_row):
        if not hasattr(self.L, "gaz_engine_score_outputs"):
            raise EngineError("this library has no gaz_engine_score_outputs: rebuild it")
        t = ScoreTotals(struct_size=C.sizeof(ScoreTotals))
        rows = (np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.uint8)) if per_row else None
        self._ck(fn(t, *([a.ctypes.data for a in rows] if per_row else [None] * 4)))
        d = score_dict(t)
        if per_row:
            d.update(row_ce=rows[0], row_entropy=rows[1], row_se=rows[2], row_flags=rows[3])
        return d

    def score_outputs(self, policy_pred, value_pred, policy_target, value_target, policy_mode=None, per_row=False):
        """Scores given predictions (f32 [n, A], [n]) against targets on the device -> dict of the raw sums (ce_sum, entropy_sum, se_sum), the
        counts (rows, bad_rows, good, top1_rows, value_rows, value_sign_rows) and the means (policy_loss, policy_entropy, policy_kl, value_loss,
        top1, value_sign, val_loss); per_row: also row_ce, row_entropy, row_se (f64 [n]) and row_flags (u8 [n]: 1 top1, 2 value sign, 4 z != 0,
        8 bad).  policy_mode None = the engine's own head; 0 probabilities, 1 logits + softmax, 2 Stablemax probabilities, 3 logits + Stablemax.
        Needs no evaluator and touches no game."""
        pp, tp = np.ascontiguousarray(policy_pred, np.float32), np.ascontiguousarray(policy_target, np.float32)
        pv, tv = np.ascontiguousarray(value_pred, np.float32).reshape(-1), np.ascontiguousarray(value_target, np.float32).reshape(-1)
        n = pv.shape[0]
        if pp.size != n * self.A or tp.size != n * self.A or tv.shape[0] != n:
            raise ValueError(f"score_outputs: {n} values with policies {pp.shape}, targets {tp.shape} and {tv.shape}")
        mode = -1 if policy_mode is None else int(policy_mode)
        return self._score_call(lambda t, *r: self.L.gaz_engine_score_outputs(self.h, pp.ctypes.data, pv.ctypes.data, tp.ctypes.data, tv.ctypes.data, n, mode, C.byref(t), *r), n, per_row)

    def score_replay(self, window, batch_rows=None, augment=False, per_row=False):
        """Scores this engine's built-in evaluator on the current plan of a replay.ReplayWindow (begin_epoch), positions 0 .. M - 1 of its order,
        batch_rows at a time (default: the whole evaluator batch) -> the dict of score_outputs plus ms (device time of the pass).  The games
        of the engine are not touched; the window's batch buffers are overwritten."""
        if window._plan is None:
            raise EngineError("score_replay: no plan: call begin_epoch")
        ms = C.c_double()
        b = self.batch_rows if batch_rows is None else int(batch_rows)
        d = self._score_call(lambda t, *r: self.L.gaz_engine_score_replay(self.h, window.h, b, 1 if augment else 0, C.byref(t), *r, C.byref(ms)), window._plan[2], per_row)
        d["ms"] = ms.value
        return d

    def head_features(self, n):
        """Flat head features of the last evaluate() call (numerics tests): (p_feat [n, F], v_feat [n, F]) float32."""
        pr, vr = C.c_int32(), C.c_int32()
        self._ck(self.L.gaz_engine_read_head_features(self.h, 0, None, None, C.byref(pr), C.byref(vr)))
        p = np.zeros((n, pr.value), np.float32); v = np.zeros((n, vr.value), np.float32)
        self._ck(self.L.gaz_engine_read_head_features(self.h, n, p.ctypes.data, v.ctypes.data, None, None))
        return p, v

    # ---- synchronous per-move API ---------------------------------------------------------------------
    def run_move(self):
        n = C.c_int32()
        self._ck(self.L.gaz_engine_run_move(self.h, C.byref(n)))
        return n.value

    def root_stats(self):
        """gaz_engine_get_root_stats: the last search's root arrays per game.  `policy` is the record's policy row — with forced_playouts_k > 0
        the pruned target of a full move — while N / W / P are the raw root statistics."""
        G, A = self.n_games, self.A
        out = dict(N=np.zeros((G, A), np.uint32), W=np.zeros((G, A), np.float32), P=np.zeros((G, A), np.float32),
                   policy=np.zeros((G, A), np.float32), root_visits=np.zeros(G, np.uint32), q=np.zeros(G, np.float32),
                   chosen=np.zeros(G, np.int32), phase=np.zeros(G, np.int32))
        self._ck(self.L.gaz_engine_get_root_stats(self.h, *[out[k].ctypes.data for k in
                                                           ("N", "W", "P", "policy", "root_visits", "q", "chosen", "phase")]))
        return out

    def apply_moves(self, moves=None):
        if moves is None:
            self._ck(self.L.gaz_engine_apply_moves(self.h, None))
        else:
            m = np.ascontiguousarray(moves, np.int32)
            self._ck(self.L.gaz_engine_apply_moves(self.h, m.ctypes.data_as(C.POINTER(C.c_int32))))

    def set_position(self, slot, action_indices):
        a = np.ascontiguousarray(action_indices, np.int32)
        self._ck(self.L.gaz_engine_set_position(self.h, int(slot), a.ctypes.data_as(C.POINTER(C.c_int32)), a.size))

    def read_positions(self):
        """-> list of action-index histories, one per slot: the game in progress (game.action_history; [] for a halted slot)"""
        T = int(self.layout.t_pad)
        n = np.zeros(self.cfg.n_games, np.int32); h = np.zeros((self.cfg.n_games, T), np.uint8)
        self._ck(self.L.gaz_engine_read_positions(self.h, n.ctypes.data, h.ctypes.data, T))
        return [h[g, :n[g]].astype(np.int32).tolist() for g in range(self.cfg.n_games)]

    def read_trees(self, slots, tree=-1, max_depth=None, min_visits=0):
        """The search trees of `slots` -> list of SearchTree, in that order.  tree = 0 / 1, or -1 = the tree running the slot's current move;
        max_depth None = everything, else nodes deeper than that are left out; a child node is exported only if its edge has
        N >= min_visits.  Legal at any time, also in the middle of a move (nodes["n_reserved"] then shows the leaves in flight)."""
        s = np.ascontiguousarray(slots, np.int32).reshape(-1)
        n = int(s.size)
        nf = np.zeros(n + 1, np.int64); ef = np.zeros(n + 1, np.int64)
        depth = -1 if max_depth is None else int(max_depth)
        if depth < 0 and max_depth is not None:
            raise ValueError("max_depth must be None or >= 0")
        self._ck(self.L.gaz_engine_read_trees(self.h, s.ctypes.data, n, int(tree), depth, int(min_visits), 0, 0, None, None, nf.ctypes.data, ef.ctypes.data))
        nodes = np.zeros(max(int(nf[n]), 1), TREE_NODE_DTYPE); edges = np.zeros(max(int(ef[n]), 1), TREE_EDGE_DTYPE)
        self._ck(self.L.gaz_engine_read_trees(self.h, s.ctypes.data, n, int(tree), depth, int(min_visits), int(nf[n]), int(ef[n]), nodes.ctypes.data,
                                              edges.ctypes.data, nf.ctypes.data, ef.ctypes.data))
        return [SearchTree(s[i], nodes[nf[i]:nf[i + 1]], edges[ef[i]:ef[i + 1]]) for i in range(n)]

    def principal_variations(self, max_len, tree=-1, first_action=None):
        """The most visited line below every slot's root (ties: the lowest slot) -> dict(actions uint8 [G, max_len], N uint32, W float32, len
        int32 [G]); entries past len are 0.  first_action [G] (< 0 = most visited) names the first step: the move a finished search chose."""
        G, m = self.n_games, int(max_len)
        out = dict(actions=np.zeros((G, max(m, 0)), np.uint8), N=np.zeros((G, max(m, 0)), np.uint32), W=np.zeros((G, max(m, 0)), np.float32), len=np.zeros(G, np.int32))
        fa = None
        if first_action is not None:
            fa = np.ascontiguousarray(first_action, np.int32).reshape(-1)
            if fa.size != G:
                raise ValueError("first_action needs one entry per game")
        self._ck(self.L.gaz_engine_read_pv(self.h, int(tree), None if fa is None else fa.ctypes.data, m, out["actions"].ctypes.data, out["N"].ctypes.data,
                                           out["W"].ctypes.data, out["len"].ctypes.data))
        return out

    def start_search(self):
        self._ck(self.L.gaz_engine_start_search(self.h))

    def stop_search(self, stop=True):
        self._ck(self.L.gaz_engine_stop_search(self.h, int(bool(stop))))

    def set_search_params(self, run_iterations=0, tau_mode=-1):
        self._ck(self.L.gaz_engine_set_search_params(self.h, int(run_iterations), int(tau_mode)))

    def set_hyperparams(self, *, c_puct_init=None, c_puct_base=None, dirichlet_alpha=None, dirichlet_epsilon=None, use_dirichlet=None,
                        tau=None, m=None, c_visit=None, c_scale=None, run_iterations=None):
        """MCTS.update_hyperparams / MCTS_Gumbel.update_hyperparams (MCTS.py:134-168, MCTS_Gumbel.py:186-210); None = unchanged."""
        nan = float("nan")
        d = lambda v: nan if v is None else float(v)
        hp = SearchHyperparams(struct_size=C.sizeof(SearchHyperparams), use_dirichlet=-1 if use_dirichlet is None else int(bool(use_dirichlet)),
                               c_puct_init=d(c_puct_init), c_puct_base=d(c_puct_base), dirichlet_alpha=d(dirichlet_alpha),
                               dirichlet_epsilon=d(dirichlet_epsilon), tau=d(tau), gumbel_m=-1 if m is None else int(m),
                               run_iterations=0 if run_iterations is None else int(run_iterations), c_visit=d(c_visit), c_scale=d(c_scale))
        self._ck(self.L.gaz_engine_set_hyperparams(self.h, C.byref(hp)))

    def probe_rules(self, histories, policy=None):
        """The device's game rules on a list of positions (each a list of action indices from the empty board): dict of board
        [n,H,W], legal [n,A] bool, winner [n], input [n,H,W,C], terminal [n,A] (-1 / 0 draw / 1 win) and, with `policy` [n,A],
        legal_policy [n,A] (get_legal_actions_policy_MCTS, normalize=True).  Guide.py:135-283, Game_Tester.py:297-405."""
        n = len(histories)
        stride = max(1, max((len(h) for h in histories), default=1))
        acts = np.zeros((n, stride), np.int32); na = np.zeros(n, np.int32)
        for i, h in enumerate(histories):
            na[i] = len(h); acts[i, :len(h)] = np.asarray(h, np.int32).reshape(-1)
        out = dict(board=np.zeros((n, self.H, self.W), np.int8), legal=np.zeros((n, self.A), np.uint8), winner=np.zeros(n, np.int32),
                   input=np.zeros((n, self.H, self.W, self.Cc), np.int8), terminal=np.zeros((n, self.A), np.int32))
        pin = pout = None
        if policy is not None:
            pin = np.ascontiguousarray(policy, np.float32); assert pin.shape == (n, self.A)
            pout = np.zeros((n, self.A), np.float32); out["legal_policy"] = pout
        self._ck(self.L.gaz_engine_probe_rules(self.h, acts.ctypes.data, na.ctypes.data, n, stride, out["board"].ctypes.data,
                                               out["legal"].ctypes.data, out["winner"].ctypes.data, out["input"].ctypes.data,
                                               out["terminal"].ctypes.data, None if pin is None else pin.ctypes.data,
                                               None if pout is None else pout.ctypes.data))
        out["legal"] = out["legal"].astype(bool)
        return out

    def probe_det(self, op, words, out_words):
        """The device's bit-exact math on the caller's inputs (include/gaz_engine.h, gaz_engine_probe_det; the ops DP_* and their words are
        listed in csrc/det_probe.hpp): `words` uint64 [n, in_words], one row per item -> uint64 [n, out_words], raw bits.  A float64 is
        passed and returned as its bit pattern (`.view(np.uint64)`), a float32 / uint32 in the low half of its word."""
        fn = getattr(self.L, "gaz_engine_probe_det", None)
        if fn is None:
            raise EngineError("this library has no gaz_engine_probe_det")
        w = np.ascontiguousarray(words, np.uint64)
        assert w.ndim == 2 and w.shape[0] > 0
        out = np.zeros((w.shape[0], int(out_words)), np.uint64)
        self._ck(fn(self.h, int(op), w.shape[0], w.ctypes.data, w.shape[1], out.ctypes.data, int(out_words)))
        return out

    def reset_games(self, slots=None):
        if slots is None:
            self._ck(self.L.gaz_engine_reset_games(self.h, None, 0))
        else:
            s = np.ascontiguousarray(slots, np.int32)
            self._ck(self.L.gaz_engine_reset_games(self.h, s.ctypes.data_as(C.POINTER(C.c_int32)), s.size))

    # ---- continuous self-play -------------------------------------------------------------------------
    def run_waves(self, n):
        self._ck(self.L.gaz_engine_run_waves(self.h, int(n)))

    def synchronize(self):
        self._ck(self.L.gaz_engine_synchronize(self.h))

    # ---- external evaluator ---------------------------------------------------------------------------
    def wave_begin(self):
        self._ck(self.L.gaz_engine_wave_begin(self.h))

    def read_batch(self):
        x = np.zeros((self.batch_rows, self.H, self.W, self.Cc), np.int8)
        pend = np.zeros(self.batch_rows, np.int32)
        self._ck(self.L.gaz_engine_read_batch(self.h, x.ctypes.data, pend.ctypes.data))
        return x, pend

    def write_outputs(self, policy, value):
        p = np.ascontiguousarray(policy, np.float32); v = np.ascontiguousarray(value, np.float32)
        assert p.shape == (self.batch_rows, self.A) and v.size == self.batch_rows
        self._ck(self.L.gaz_engine_write_outputs(self.h, p.ctypes.data, v.ctypes.data))

    def set_eval_symmetry(self, on=True):
        """Evaluate every search position under a random board symmetry (gaz_engine_set_eval_symmetry), for the rows encoded from the next
        launch on: the network sees T_k(state) — the 8 transforms of a square board in the order of games.augment_sample, Connect4's column
        mirror — with k drawn per (seed, slot, game_seq, position), and the search uses the policy mapped back.  Records, samples, root
        statistics and trees stay in the board's own frame; an external evaluator sees the permuted rows and answers in their frame."""
        self._ck(self.L.gaz_engine_set_eval_symmetry(self.h, int(on)))

    @property
    def eval_symmetry(self):
        m = C.c_int32()
        self._ck(self.L.gaz_engine_get_eval_symmetry(self.h, C.byref(m)))
        return bool(m.value)

    def set_solver(self, on=True):
        """Prove wins, draws and losses in the PUCT search (gaz_engine_set_solver; MCTS-Solver), from the next launch on: moves that are
        proven lost are no longer searched, a move ends as soon as its root is proven, the policy row and the move are restricted to the
        moves that keep the proven result, and the recorded q of such a ply is the exact +1 / 0 / -1 (its `proven` flag is set).  Refused
        with the Gumbel search, leaf_batch > 1 and gumbel_batch > 1."""
        self._ck(self.L.gaz_engine_set_solver(self.h, int(bool(on))))

    @property
    def solver(self):
        m = C.c_int32()
        self._ck(self.L.gaz_engine_get_solver(self.h, C.byref(m)))
        return bool(m.value)

    def solver_stats(self):
        """gaz_engine_get_solver_stats as a dict, over the engine's life: `proven_nodes` (by propagation; terminal parents not counted),
        `proven_hits` (simulations that ended at a proven edge), `proven_moves` (moves that ended with a proven root: `root_win` +
        `root_draw` + `root_loss`), `saved_sims` (simulations those moves did not run) and `masked_levels` (descent levels at which a
        proven-lost move was left out).  A synchronisation point like stats()."""
        out = (C.c_uint64 * 8)()
        self._ck(self.L.gaz_engine_get_solver_stats(self.h, out))
        s = [int(x) for x in out]
        return dict(proven_nodes=s[0], proven_hits=s[1], proven_moves=s[2], saved_sims=s[3], root_win=s[4], root_draw=s[5], root_loss=s[6],
                    masked_levels=s[7])

    # ---- match play ---------------------------------------------------------------------------------
    def set_match(self, on=True, hash_salt_b=0):
        """Play the engine's games between two networks (gaz_engine_set_match), from the next evaluator pass on: network A = load_weights (the
        hash evaluator: hash_salt), network B = load_weights_b (hash_salt_b).  In game (slot, game_seq) A plays the first player iff slot +
        game_seq is even; a record's header therefore says who was A (self_play.match_result tallies records).  Refused with single_tree,
        leaf_batch > 1, gumbel_batch > 1, the evaluation cache and game groups."""
        p = MatchParams(struct_size=C.sizeof(MatchParams), mode=int(bool(on)), hash_salt_b=int(hash_salt_b), reserved_=0)
        self._ck(self.L.gaz_engine_set_match(self.h, C.byref(p)))

    @property
    def match(self):
        m = C.c_int32()
        self._ck(self.L.gaz_engine_get_match(self.h, C.byref(m)))
        return bool(m.value)

    def read_batch_network(self):
        """uint8 [n_games]: the network that answers every row of the evaluator batch — NET_A (0), NET_B (1), NET_NONE (255) where
        read_batch's pending is 0.  An external evaluator answers each row with the network the byte names."""
        net = np.zeros(self.n_games, np.uint8)
        self._ck(self.L.gaz_engine_read_batch_network(self.h, net.ctypes.data))
        return net

    def match_stats(self):
        """gaz_engine_get_match_stats as a dict, over the engine's life: `rows_a` / `rows_b` evaluated by each network, `waves_without_a` /
        `waves_without_b` (evaluator passes in which that network got no row) and `passes` (evaluator passes with the mode on)"""
        out = (C.c_uint64 * 8)()
        self._ck(self.L.gaz_engine_get_match_stats(self.h, out))
        s = [int(x) for x in out]
        return dict(rows_a=s[0], rows_b=s[1], waves_without_a=s[2], waves_without_b=s[3], passes=s[4])

    def match_timing(self):
        """gaz_engine_get_match_timing as a dict, per bracketed wave (timing_reset(True) brackets every 8th): `ms_route_copy` (route +
        partition + copy), `ms_sync_gap` (the stream idle from the end of the copy to the first launch after the host's wait), `ms_scatter`,
        `ms_host_wait` (the host's time inside the wait) and `waves`, the waves bracketed"""
        out = (C.c_double * 8)()
        self._ck(self.L.gaz_engine_get_match_timing(self.h, out))
        n = max(out[4], 1.0)
        return dict(ms_route_copy=out[0] / n, ms_sync_gap=out[1] / n, ms_scatter=out[2] / n, ms_host_wait=out[3] / n, waves=int(out[4]))

    def read_batch_symmetry(self):
        """uint8 [batch_rows]: the symmetry k every row of the evaluator batch was encoded under (meaningful where read_batch's
        pending is set; 0 while eval_symmetry is off)"""
        k = np.zeros(self.batch_rows, np.uint8)
        self._ck(self.L.gaz_engine_read_batch_symmetry(self.h, k.ctypes.data))
        return k

    def batch_ptrs(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._ck(self.L.gaz_engine_batch_ptrs(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    # ---- results --------------------------------------------------------------------------------------
    def stats(self):
        out = (C.c_uint64 * 16)()
        self._ck(self.L.gaz_engine_get_stats(self.h, out))
        s = [int(x) for x in out]
        return dict(game_stats=np.array(s[:6], np.uint64), evals=s[6], sims=s[7], plies=s[8], waves=s[9], cache_hits=s[10], pipeline_groups=s[11], fused_wave=s[12], fused_faults=s[13], game_groups=max(int(s[14]), 1), reserved_children=s[15])

    def set_resignation(self, threshold, consecutive=1, min_ply=0, no_resign_prob=0.0):
        """Resignation in self-play (gaz_engine_set_resignation), from the next launch on: a game ends after a ply — lost for its mover —
        when the recorded q of the mover's last `consecutive` searched plies were all below -threshold and the ply is at least `min_ply`;
        a game is instead played out with probability `no_resign_prob`, its would-be resign plies marked, so that resign_stats() can tell
        the false positives.  threshold = 0 switches it off (the other arguments are then ignored)."""
        p = ResignParams(struct_size=C.sizeof(ResignParams), consecutive=int(consecutive), min_ply=int(min_ply), reserved_=0,
                         threshold=float(threshold), no_resign_prob=float(no_resign_prob))
        self._ck(self.L.gaz_engine_set_resignation(self.h, C.byref(p)))

    def resign_stats(self):
        """gaz_engine_get_resign_stats as a dict: games `resigned` (`resigned_by_minus1` / `resigned_by_plus1`: the player who gave up),
        `playout_games` finished, of them `would_resign`, of those `false_positives` (the would-be resigner drew or won), and
        `resigned_plies`, the plies the resigned games were played for.  A synchronisation point like stats()."""
        out = (C.c_uint64 * 8)()
        self._ck(self.L.gaz_engine_get_resign_stats(self.h, out))
        s = [int(x) for x in out]
        return dict(resigned=s[0], resigned_by_minus1=s[1], resigned_by_plus1=s[2], playout_games=s[3], would_resign=s[4], false_positives=s[5],
                    resigned_plies=s[6])

    # ---- opening book --------------------------------------------------------------------------------
    def set_opening_book(self, entries, mode="game"):
        """Start games from book positions (gaz_engine_set_opening_book): `entries` is a list of action-index sequences — an empty one means
        "the empty board" — and every game that starts after the call draws one of them, a function of (seed, slot, game_seq) alone
        (self_play.book_entry restates it).  mode "game": an entry per game; "pair": the games (slot, 2k) and (slot, 2k + 1) share their
        entry — with set_match the two colour assignments of one pairing.  mode None, or no entries, removes the book.  The prefix plies of a
        record have move_kind 3 and give no training rows.  A refused call (EngineError) leaves the book in force as it was."""
        if mode not in BOOK_MODES:
            raise ValueError(f"set_opening_book: mode must be 'game', 'pair' or None, not {mode!r}")
        if not hasattr(self.L, "gaz_engine_set_opening_book"):
            raise EngineError("this library has no gaz_engine_set_opening_book")
        entries = [np.asarray(e, np.int64).reshape(-1) for e in (entries if entries is not None else [])]
        for i, e in enumerate(entries):
            if e.size and (e.min() < 0 or e.max() > 255):
                raise ValueError(f"set_opening_book: entry {i} holds an action index outside [0, 255]")
        n = len(entries) if BOOK_MODES[mode] else 0
        stride = max([1] + [int(e.size) for e in entries[:n]])
        acts = np.zeros((max(n, 1), stride), np.uint8); lens = np.zeros(max(n, 1), np.int32)
        for i, e in enumerate(entries[:n]):
            acts[i, :e.size] = e; lens[i] = e.size
        prm = BookParams(struct_size=C.sizeof(BookParams), n_entries=n, stride=stride, mode=BOOK_MODES[mode] if n else 0)
        self._ck(self.L.gaz_engine_set_opening_book(self.h, C.byref(prm), acts.ctypes.data, lens.ctypes.data))

    def opening_book(self):
        """(n_entries, mode) of the book in force — mode "game" or "pair" —, (0, None) without one"""
        if not hasattr(self.L, "gaz_engine_get_opening_book"):
            return 0, None
        n, m = C.c_int32(), C.c_int32()
        self._ck(self.L.gaz_engine_get_opening_book(self.h, C.byref(n), C.byref(m)))
        return int(n.value), {0: None, 1: "game", 2: "pair"}[int(m.value)]

    def book_counts(self):
        """gaz_engine_read_book_counts as a dict: `counts` uint64 [n_entries] — the games started from every entry of the book in force since
        it was set —, and over the engine's life `started` (games started with a book set) and `prefix_plies`.  A synchronisation point."""
        n = self.opening_book()[0]
        counts = np.zeros(max(n, 1), np.uint64); out = (C.c_uint64 * 8)()
        self._ck(self.L.gaz_engine_read_book_counts(self.h, counts.ctypes.data, out))
        return dict(counts=counts[:n], started=int(out[0]), prefix_plies=int(out[1]))

    def drain_finished(self, max_records=None):
        """Finished games as dicts: actions, policies [T,A], q, z, values (=0.5(z+q), Self_Play.py:165-172),
        root_N/W/P [T,A], root_visits, evals, move_kind (uint8 [T]: 0 no search, 1 full, 2 fast, 3 opening-book prefix), proven (bool [T]: the ply ended with a root
        the solver had proven, set_solver; its q is exact), winner, slot, game_seq, and of
        resignation (set_resignation) resigned (bool), resign_ply (the last ply of a resigned game, else -1) and would_resign_plies (the
        plies at which a game that was played out would have been resigned).
        With forced_playouts_k > 0 `policies` holds the pruned targets of the full moves; root_N / root_W / root_P stay raw."""
        lay = self.layout
        cap = max_records or max(self.cfg.ring_capacity, 1)
        buf = np.zeros((cap, lay.record_bytes), np.uint8)
        n = C.c_int32()
        self._ck(self.L.gaz_engine_drain_finished(self.h, buf.ctypes.data, cap, C.byref(n)))
        return [self.decode_record(buf[i]) for i in range(n.value)]

    sample_buffer_bytes = 256 << 20     # host buffers of drain_samples (at least one game of max_T plies)

    def set_sample_weighting(self, lam, fast_factor=1.5):
        """Policy surprise weighting of the training rows (gaz_engine_set_sample_weighting; KataGo), from the next drain_samples on: a
        game's row weight — one per fully searched ply — moves towards the plies whose search policy differs most from the priors their root
        searched with, a fast ply whose surprise exceeds `fast_factor` times the mean of the full plies earns rows too, and every weight
        becomes a whole number of rows by stochastic rounding keyed by (seed, slot, game_seq, ply).  lam in [0, 1]: 0 = off (KataGo: 0.5).
        PUCT engines only.  self_play.sample_row_counts is the host definition."""
        lam, fast_factor = float(lam), float(fast_factor)
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"set_sample_weighting: lambda must be in [0, 1] (0 = off), not {lam}")
        if not (fast_factor > 0.0 and fast_factor != float("inf")):
            raise ValueError(f"set_sample_weighting: fast_factor must be a finite number above 0, not {fast_factor}")
        if not hasattr(self.L, "gaz_engine_set_sample_weighting"):
            raise EngineError("this library has no gaz_engine_set_sample_weighting")
        self._ck(self.L.gaz_engine_set_sample_weighting(self.h, lam, fast_factor))

    @property
    def sample_weighting(self):
        """(lambda, fast_factor) of set_sample_weighting; (0.0, 1.5) on a new engine"""
        if not hasattr(self.L, "gaz_engine_get_sample_weighting"):
            return 0.0, 1.5
        a, b = C.c_double(), C.c_double()
        self._ck(self.L.gaz_engine_get_sample_weighting(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def drain_samples(self, max_games=None, max_rows=None, with_plies=False):
        """Finished games as training samples, built on the device (gaz_engine_drain_samples): a SampleBatch of the games that have
        finished, oldest first; what the buffers (or `max_games` / `max_rows`) do not hold stays in the engine for the next call; a
        `max_rows` below the oldest game's rows is an EngineError.  With forced_playouts_k > 0 the policies are the pruned targets (the
        kernel reads the record's policy rows).  May be mixed with drain_finished():
        a game is handed out once.  The host buffers are allocated once per engine and REUSED: the batch's arrays are views into them,
        valid until the next drain_samples() of this engine — a batch that goes to another thread, or is kept, is copied first
        (SampleBatch.copy(); run_self_play does that before it hands a batch to its writer thread).
        With set_sample_weighting a game has up to 2 T rows (SampleBatch.rows_of); with_plies: the batch's `plies` is the ply of every row."""
        most = 2 if self.sample_weighting[0] else 1                  # rows a ply may average: the buffers hold a game of most * max_T rows
        if getattr(self, "_sbuf", None) is None or self._sbuf[0] != most:
            sl = SampleLayout()
            self._ck(self.L.gaz_engine_sample_layout(self.h, C.byref(sl)))
            cap_games = max(int(self.cfg.ring_capacity), 1)
            row_bytes = sl.n_aug * (sl.state_bytes + 4 * sl.A) + 4
            cap_rows = max(min(cap_games * most * sl.max_T, self.sample_buffer_bytes // row_bytes), most * sl.max_T)
            self._sbuf = (most, sl, cap_games, cap_rows, np.empty((cap_games, 6), np.int32), np.empty((sl.n_aug, cap_rows, self.H, self.W, self.Cc), np.int8),
                          np.empty((sl.n_aug, cap_rows, sl.A), np.float32), np.empty((cap_rows, 1), np.float32), np.empty(cap_rows, np.uint8))
        _, sl, cap_games, cap_rows, games, boards, policies, values, plies = self._sbuf
        n, r = C.c_int32(), C.c_int64()
        take_rows, b, p = cap_rows, boards, policies
        if max_rows is not None and int(max_rows) < cap_rows:        # the augmentation planes are max_rows apart: arrays of that shape
            take_rows = int(max_rows)
            b = np.empty((sl.n_aug, max(take_rows, 1), self.H, self.W, self.Cc), np.int8)
            p = np.empty((sl.n_aug, max(take_rows, 1), sl.A), np.float32)
        take_games = min(int(max_games), cap_games) if max_games else cap_games
        if with_plies:
            if not hasattr(self.L, "gaz_engine_drain_samples2"):
                raise EngineError("this library has no gaz_engine_drain_samples2")
            self._ck(self.L.gaz_engine_drain_samples2(self.h, take_games, take_rows, games.ctypes.data, b.ctypes.data, p.ctypes.data, values.ctypes.data,
                                                      plies.ctypes.data, C.byref(n), C.byref(r)))
            return SampleBatch(games[:n.value], b[:, :r.value], p[:, :r.value], values[:r.value], plies[:r.value])
        self._ck(self.L.gaz_engine_drain_samples(self.h, take_games, take_rows, games.ctypes.data,
                                                 b.ctypes.data, p.ctypes.data, values.ctypes.data, C.byref(n), C.byref(r)))
        return SampleBatch(games[:n.value], b[:, :r.value], p[:, :r.value], values[:r.value])

    def decode_record(self, raw):
        lay, A = self.layout, self.A
        hdr = raw[lay.off_hdr:lay.off_hdr + 16].view(np.int32)
        T, winner, slot, seq = (int(x) for x in hdr)

        def arr(off, dt, shape):
            n = int(np.prod(shape)) * np.dtype(dt).itemsize
            return raw[off:off + n].view(dt).reshape(shape).copy()
        actions = arr(lay.off_actions, np.uint8, (lay.t_pad,))[:T].astype(np.int32)
        q = arr(lay.off_q, np.float32, (lay.max_T,))[:T]
        # z[p] = mover(p) * winner, the mover of ply p being -1 on even plies (target_z.append(next_player), Self_Play.py:127).  Without
        # resignation the winner is 0 or the last mover, and this is the reference's rule (the mover signs, all turned when -1 won and moved
        # last, zeros for a draw: Self_Play.py:165-172) value for value; a resigned game is won by the player who did NOT move last
        mover = np.where(np.arange(T) % 2 == 0, -1, 1)
        z = (mover * winner).astype(np.float32)
        raw_kind = arr(lay.off_move_kind, np.uint8, (lay.t_pad,))[:T]
        resigned_at = np.flatnonzero(raw_kind & MK_RESIGNED)
        return dict(T=T, winner=winner, slot=slot, game_seq=seq, actions=actions, q=q, z=z,
                    values=(np.float32(0.5) * (z + q)).astype(np.float32),
                    policies=arr(lay.off_policy, np.float32, (lay.max_T, A))[:T],
                    root_N=arr(lay.off_N, np.uint32, (lay.max_T, A))[:T], root_W=arr(lay.off_W, np.float32, (lay.max_T, A))[:T],
                    root_P=arr(lay.off_P, np.float32, (lay.max_T, A))[:T],
                    root_visits=arr(lay.off_root_visits, np.uint32, (lay.max_T,))[:T],
                    evals=arr(lay.off_evals, np.uint32, (lay.max_T,))[:T],
                    move_kind=raw_kind & np.uint8(MK_KIND_MASK), proven=(raw_kind & np.uint8(MK_PROVEN)) != 0, resigned=bool(resigned_at.size),
                    resign_ply=int(resigned_at[0]) if resigned_at.size else -1,
                    would_resign_plies=np.flatnonzero(raw_kind & MK_WOULD_RESIGN).astype(np.int32))

    # ---- measurement ----------------------------------------------------------------------------------
    def repack(self):
        """Move the games still running to the lowest slots and shrink the launches to them (generation tails); -> (active, launch size)."""
        a, b = C.c_int32(), C.c_int32()
        self._ck(self.L.gaz_engine_repack(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_fused_wave(self, on=True):
        """tree step + trunk kernel as one launch (default where available) or as separate launches; results do not change"""
        self._ck(self.L.gaz_engine_set_fused_wave(self.h, int(bool(on))))

    def debug_fused_fault(self, mod):
        """TEST HOOK: trunk workgroups with index % mod == 1 of the following fused launches give up their wait at once (0 = off)"""
        self._ck(self.L.gaz_engine_debug_fused_fault(self.h, int(mod)))

    def timing_reset(self, enable=True):
        self._ck(self.L.gaz_engine_timing_reset(self.h, int(enable)))

    def dominant_kernel(self):
        buf = C.create_string_buffer(1024); fl = C.c_double()
        self._ck(self.L.gaz_engine_dominant_kernel(self.h, buf, 1024, C.byref(fl)))
        return buf.value.decode(), fl.value

    def timing(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        d, e = C.c_int64(), C.c_int64()
        self._ck(self.L.gaz_engine_timing_get(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e)))
        return dict(ms_tree=a.value, ms_eval=b.value, ms_dominant=c.value, n_dominant=d.value, n_waves=e.value)

"""Test model of the solver (gaz_engine_set_solver; DESIGN.md section 19, include/gaz_engine.h: MCTS-Solver — proven wins, draws and
losses in the PUCT search).  There is no reference implementation: the model is written from the rules in the header.

SolverTree is forced_playouts_model.ForcedTree at K = 1 with rules 1 - 5: a status per node OBJECT (0 unknown, 1 win, 2 draw, 3 loss for
the player to move there; a terminal parent's is derived from its children), propagation along the simulation's own path after a
terminal parent was created, the masked argmax and the proven hit in the descent, the early end of a move, and move_end_row.  The masked
argmax uses that module's score / mean_value / puct_factors; at EVERY selection the unmasked restated argmax is held against
oracle.best_puct_index, which pins the restated score to the oracle's.

minimax() is a brute-force game solver with memoisation, independent of all of the above: it is what every exported status is held
against."""
import numpy as np

from forced_playouts_model import ForcedTree, mean_value, owed_slots, prune_slots, puct_factors, score
from leaf_batch_model import DRAW as LEAF_DRAW, WIN as LEAF_WIN, _Leaf, _Node, f32

U, WIN, DRAW, LOSS = 0, 1, 2, 3
P_MOVE = 2                                           # det::P_MOVE
VALUE = {WIN: 1.0, DRAW: 0.0, LOSS: -1.0}


class _SNode(_Node):
    __slots__ = ("status",)

    def __init__(self, board, hist, player):
        super().__init__(board, hist, player)
        self.status = U


def node_status(node):
    """rule 1 for a terminal parent, else what propagation wrote on the node"""
    if node.terminal:
        return WIN if any(c == LEAF_WIN for c in node.child[:node.n_children]) else DRAW
    return node.status


def edge_status(node, s):
    """the edge value of child slot s for node's mover, as WIN (+1) / DRAW (0) / LOSS (-1) / U"""
    c = node.child[s]
    if isinstance(c, _Node):
        return {U: U, WIN: LOSS, DRAW: DRAW, LOSS: WIN}[node_status(c)]
    if c == LEAF_WIN:
        return WIN
    if c == LEAF_DRAW:
        return DRAW
    return U


def candidates(root_status, es, N):
    """rule 5: the candidate slots"""
    n = len(es)
    if root_status == WIN:
        return [i for i in range(n) if es[i] == WIN]
    if root_status == DRAW:
        return [i for i in range(n) if es[i] == DRAW]
    if root_status == LOSS:
        return list(range(n))
    c = [i for i in range(n) if es[i] != LOSS and int(N[i]) > 0]
    return c or list(range(n))


def move_end_row(counts, N, es, root_status):
    """rule 5 in SLOT order: counts = what the row would be made of without the solver (N, or the pruned counts), N the raw visits, es the
    edge values -> (the row f32 [n] or None when it is left as it was, the candidate slots, the move of a root proven WIN / DRAW or None)"""
    C = candidates(root_status, es, N)
    total = sum(int(counts[i]) for i in C)
    row = None
    if total:
        row = np.zeros(len(es), f32)
        for i in C:
            row[i] = f32(float(int(counts[i])) / float(total))
    move = None
    if root_status in (WIN, DRAW):
        move = max(C, key=lambda i: (int(N[i]), -i))
    return row, C, move


class SolverTree(ForcedTree):
    """One PUCT tree with the solver.  `solver_on` may be switched between moves.  stats[0..7] are gaz_engine_get_solver_stats' counters of
    this tree.  run() -> Tree.run's dict plus sims, limit, policy [A], q, status (the root's at move end), chosen (the action, for the given
    tau_on), cand (candidate ACTIONS)."""

    def __init__(self, *a, solver=True, **kw):
        self.solver_on = bool(solver)
        self.stats = [0] * 8
        kw.setdefault("forced_k", 0.0)
        super().__init__(*a, **kw)
        assert self.K == 1

    # ---- nodes carry their status ------------------------------------------------------------------------
    def _create_root(self):
        self.root = _SNode(self.board.copy(), list(self.hist), -self.next_player)
        self.root_visits = 0
        acts, wins = self._terminal_actions(self.board, self.hist, self.next_player)
        if acts:
            self._terminal_parent(self.root, acts, wins, True)
            self.root_visits = len(acts)
            return
        state = self._state(self.board, -self.next_player, self.hist)
        policy, _ = self.evaluator(state); self.n_evals += 1
        self.root.set_children(*self._priors(policy, self._legal(self.board)))
        self.root_request = state

    def _reserve(self, node, path):
        slot = node.n_children
        a, mover = node.act[slot], -node.player
        board = node.board.copy(); self._do(board, a, mover)
        hist = node.hist + [a]
        acts, wins = self._terminal_actions(board, hist, -mover)
        child = _SNode(board, hist, mover)
        path = path + [(node, slot)]
        if acts:
            self._terminal_parent(child, acts, wins, False)
            node.child[slot] = child; node.n_children = slot + 1
            self._backup(path, -f32(len(acts)) if any(wins) else f32(0.0), len(acts))
            if self.solver_on:
                self._propagate(path)
            return 1, None
        leaf = _Leaf(); leaf.parent, leaf.slot, leaf.node, leaf.path = node, slot, child, path
        leaf.state = self._state(board, mover, hist)
        node.n_reserved += 1
        return 0, leaf

    # ---- rule 2 ------------------------------------------------------------------------------------------
    def _propagate(self, path):
        for node, _ in reversed(path):
            if node.terminal or node.status != U:
                break
            es = [edge_status(node, i) for i in range(len(node.act))]
            if WIN in es:
                st = WIN
            elif node.n_children == len(node.act) and U not in es:
                st = DRAW if DRAW in es else LOSS
            else:
                break
            node.status = st
            self.stats[0] += 1

    # ---- rule 3 ------------------------------------------------------------------------------------------
    def _select(self):
        node, path, pv = self.root, [], self.root_visits
        while True:
            if node.terminal:
                wins = [i for i in range(node.n_children) if node.child[i] == LEAF_WIN]
                cand = wins if np.any(node.W[:node.n_children] > 0) else list(range(node.n_children))
                k = self.O.pick(self.seed, self.slot, self.seq, self.tree, self.event, len(cand)); self.event += 1
                path.append((node, cand[k]))
                return 1, node, path, node.child[cand[k]] == LEAF_WIN
            n = len(node.act)
            s, c = puct_factors(pv, self.c_init, self.c_base)
            scores = [score(node.P[i], mean_value(node.W[i], node.N[i]), int(node.N[i]), s, c) for i in range(n)]
            best = max(range(n), key=lambda i: (scores[i], -i))
            assert best == self.O.best_puct_index(node.P, node.W, node.N, pv, self.c_init, self.c_base), "restated argmax != the oracle's"
            self.n_selections += 1
            es = [edge_status(node, i) for i in range(n)] if self.solver_on else [U] * n
            if LOSS in es:
                self.stats[7] += 1
                keep = [i for i in range(n) if es[i] != LOSS]
                best = max(keep, key=lambda i: (scores[i], -i)) if keep else 0
            if node is self.root:
                self.n_root += 1
                if self.forced_on:
                    owed = [i for i in owed_slots(node.N, node.P, node.n_children, pv, self.forced_k) if es[i] != LOSS]
                    if owed:
                        self.n_differ += owed[0] != best
                        best = owed[0]
                    else:
                        self.n_free += 1
            if self.solver_on and best < node.n_children and es[best] != U:
                path.append((node, best))
                return 3, node, path, es[best]
            if best == node.n_children:
                return 0, node, path, False
            assert best < node.n_children, "PUCT picked an un-poppable child"
            path.append((node, best))
            pv = int(node.N[best]); node = node.child[best]

    # ---- rules 4 and 5 -----------------------------------------------------------------------------------
    def run(self, iterations, forced=True, tau_on=False):
        self.forced_on = bool(forced) and self.forced_k > 0.0
        self.n_root = self.n_differ = self.n_free = 0
        self.n_selections = getattr(self, "n_selections", 0)
        self.root_request = None
        n_legal = len(self._legal(self.board))
        limit = 1 if n_legal == 1 else (3 * n_legal if iterations < n_legal else iterations)
        root, evals0 = self.root, self.n_evals
        done, fully, early = 0, False, False
        while done < limit:
            if not fully and not np.any(root.N == 0):
                fully = True
            if self.solver_on and node_status(root) != U:
                if fully:
                    break
                early = True                                           # proven before every root child had a visit: root expansions go on
            if fully and root.terminal:
                _, _, path, win = self._select()
                self._backup(path, 1.0 if win else 0.0, 1); done += 1
                continue
            kind, node, path, win = self._select() if fully else (0, root, [], False)
            if kind == 3:
                self._backup(path, VALUE[win], 1); done += 1; self.stats[1] += 1
            elif kind == 1:
                self._backup(path, 1.0 if win else 0.0, 1); done += 1
            else:
                r, leaf = self._reserve(node, path)
                if r == 0:
                    self._apply(leaf)
                done += 1
        assert root.n_children == len(root.act), "root not fully expanded at move end"
        n = len(root.act)
        status = node_status(root) if self.solver_on else U
        es = [edge_status(root, i) for i in range(n)] if self.solver_on else [U] * n
        pruned = self.forced_on and not root.terminal
        counts = prune_slots(root.N, root.W, root.P, self.root_visits, self.forced_k, self.c_init, self.c_base) if pruned else [int(v) for v in root.N]
        total = sum(counts)
        row = np.asarray([f32(float(v) / float(total)) for v in counts], f32)
        cand = list(range(n))
        move = None
        if self.solver_on:
            r2, cand, move = move_end_row(counts, root.N, es, status)
            if r2 is not None:
                row = r2
        u = self.O.uniform(self.seed, self.slot, self.seq, self.tree, self.event, P_MOVE); self.event += 1
        w = [int(root.N[i]) if i in cand else 0 for i in range(n)]
        if move is None:
            if not tau_on:
                move = max(range(n), key=lambda i: (w[i], -i))
            else:                                                      # move_end: N / visits, their float64 numpy sum, the cdf against u
                den = float(self.root_visits)
                g = np.asarray([float(v) / den for v in w], np.float64)
                ssum = float(self.O.np_sum_f64(g))
                acc = 0.0
                for i in range(n):
                    acc = acc + g[i] / ssum
                last, acc, move = acc, 0.0, n - 1
                for i in range(n):
                    acc = acc + g[i] / ssum
                    if acc / last > u:
                        move = i
                        break
        q = f32(VALUE[status]) if status != U else f32(float(root.W[move]) / float(int(root.N[move])))
        if status != U:
            self.stats[2] += 1; self.stats[3] += limit - done; self.stats[3 + status] += 1
        N = np.zeros(self.A, np.uint32); W = np.zeros(self.A, f32); P = np.zeros(self.A, f32); pol = np.zeros(self.A, f32)
        for i, a in enumerate(root.act):
            N[a], W[a], P[a], pol[a] = root.N[i], root.W[i], root.P[i], row[i]
        return dict(N=N, W=W, P=P, root_visits=self.root_visits, evals=self.n_evals - evals0, sims=done, limit=limit, policy=pol, q=q, status=status,
                    chosen=int(root.act[move]), cand=sorted(int(root.act[i]) for i in cand), n_root=self.n_root, n_differ=self.n_differ, n_free=self.n_free,
                    proven_early=early)

    def statuses(self):
        """the status of every node below the root, breadth-first, the expanded children of a node in slot order (the order of read_trees)"""
        out, queue = [], [self.root]
        for node in queue:
            out.append(node_status(node))
            queue += [c for c in node.child[:node.n_children] if isinstance(c, _Node)]
        return out

    def nodes_bfs(self):
        queue = [self.root]
        for node in queue:
            queue += [c for c in node.child[:node.n_children] if isinstance(c, _Node)]
        return queue


# ---------------------------------------------------------------------------------------------------- brute force
def _winner_after(G, board, a_index, mover, hist):
    """the game's own rule code: -2 running, 0 draw, else the winner"""
    act = G.index_to_action(int(a_index))
    G.do_action_MCTS(board, act, mover)
    return int(G.check_win_MCTS(board, mover, np.array([G.index_to_action(int(x)) for x in hist + [a_index]])))


def minimax(game, board, hist, mover, memo=None):
    """WIN / DRAW / LOSS for `mover`, to move on `board` (not terminal), by exhaustive search over grok_alpha_zero_amd.games' rules.  Memoised
    on (board bytes, mover) in `memo` (pass one dict per game to share it); for TicTacToe, and Connect4 positions with few empty cells."""
    from grok_alpha_zero_amd.games import GAMES
    G = GAMES[game]
    memo = {} if memo is None else memo

    def solve(b, h, p):
        key = (b.tobytes(), p)
        if key in memo:
            return memo[key]
        best, after = LOSS, []
        for a in sorted(G.action_to_index(x) for x in G.get_legal_actions_MCTS(b, 0, None)):      # the moves that end the game first
            nb = b.copy()
            after.append((a, nb, _winner_after(G, nb, a, p, h)))
        if any(r == p for _, _, r in after):
            memo[key] = WIN
            return WIN
        for a, nb, r in after:
            if r == 0:
                v = DRAW
            else:
                v = {WIN: LOSS, DRAW: DRAW, LOSS: WIN}[solve(nb, h + [a], -p)]
            if v == WIN:
                best = WIN
                break
            if v == DRAW:
                best = DRAW
        memo[key] = best
        return best
    return solve(np.asarray(board, np.int8).copy(), [int(x) for x in hist], int(mover))

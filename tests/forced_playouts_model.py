"""Test model of forced playouts and policy target pruning (gaz_engine_config.forced_playouts_k = k; DESIGN.md "Forced playouts and
policy target pruning"; KataGo, Wu 2019, section 3.2).  There is no reference implementation: the model is written from the rules.

Forced selection (ForcedTree): at a fully visited root that is no terminal parent, on a full move, child slot i is OWED a visit iff
N_i > 0 and float(N_i) < sqrt((k * P_i) * root_visits); the lowest owed slot replaces the choice of oracle.best_puct_index, the descent
below it is the ordinary one, statistics are taken as they stand (virtual losses included) and reserved slots are never owed.

Target pruning (prune_target): with (s, c) the two factors of the PUCT score that depend on the parent's visits and
score(P, q, n) = q + (P * (s / (n + 1))) * c, the most visited child c* (lowest slot on ties) keeps its visits, every other visited child
gives back up to min(N_i, floor(sqrt((k * P_i) * root_visits))) visits one at a time while score(P_i, q_i, n - 1) < score of c*, and a
child left with one visit after giving some back gets none.  The target is n / sum(n).

Priors are leaf_batch_model.Tree._priors' (the zero-mass rule included: a node whose legal entries sum to no positive finite number gets
1 / n_legal); this module builds none of its own.

Arithmetic: Python floats (float64) and np.float32 in the stated order, the logarithm from the oracle library (gaz_api_log), the root
from math.sqrt (correctly rounded).  restated_best() is the score's argmax; tests hold it against oracle.best_puct_index, which pins
the restated score to the oracle's without touching the oracle."""
import math

import numpy as np

from leaf_batch_model import WIN, Tree, f32


def puct_factors(root_visits, c_init, c_base):
    """(s, c) of puct_factors: sqrt(pv), c_init + ln((pv + c_base + 1) / c_base)"""
    from oracle import gaz_oracle
    pv = float(root_visits)
    return math.sqrt(pv), float(c_init) + float(gaz_oracle.lib().gaz_api_log((pv + float(c_base) + 1.0) / float(c_base)))


def score(P, q, n, s, c):
    """best_puct_slot's expression for a child with prior P (f32), mean value q (f32) and n visits"""
    return float(q) + (float(P) * (s / float(n + 1))) * c


def mean_value(W, N):
    """Q of a child: W as it is for an unvisited one, else f32(W / N) in float64"""
    return f32(W) if int(N) == 0 else f32(float(W) / float(int(N)))


def restated_best(P, W, N, parent_visits, c_init, c_base):
    """argmax of the restated score over the children, first maximum (what oracle.best_puct_index must return)"""
    s, c = puct_factors(parent_visits, c_init, c_base)
    best, best_score = 0, 0.0
    for i in range(len(P)):
        sc = score(P[i], mean_value(W[i], N[i]), int(N[i]), s, c)
        if i == 0 or sc > best_score:
            best, best_score = i, sc
    return best


def owed_slots(N, P, n_children, root_visits, k):
    """the owed slots among the first n_children, ascending"""
    rv = float(root_visits)
    return [i for i in range(n_children) if int(N[i]) > 0 and float(int(N[i])) < math.sqrt((k * float(P[i])) * rv)]


def forced_floor(N_i, P_i, root_visits, k):
    """min(N_i, floor(sqrt((k * P_i) * root_visits)))"""
    t = math.sqrt((k * float(P_i)) * float(root_visits))
    return int(N_i) if t >= float(int(N_i)) else int(math.floor(t))


def prune_slots(N, W, P, root_visits, k, c_init, c_base):
    """rule 3 on the root's arrays in SLOT order -> the pruned visit counts (list of int)"""
    s, c = puct_factors(root_visits, c_init, c_base)
    N = [int(v) for v in N]
    star = int(np.argmax(np.asarray(N, np.uint64)))                    # first maximum = lowest slot
    if N[star] == 0:
        return N
    s_star = score(P[star], mean_value(W[star], N[star]), N[star], s, c)
    out = list(N)
    for i in range(len(N)):
        if i == star or N[i] == 0:
            continue
        q = mean_value(W[i], N[i])
        n = N[i]
        for _ in range(forced_floor(N[i], P[i], root_visits, k)):
            if score(P[i], q, n - 1, s, c) < s_star:
                n -= 1
            else:
                break
        if n == 1 and n < N[i]:
            n = 0
        out[i] = n
    return out


def prune_target(N, W, P, root_visits, k, c_init=2.5, c_base=19652.0):
    """rule 3 on a root's raw rows BY ACTION (a record's root_N / root_W / root_P row, Tree.run's N / W / P) -> the policy row, f32 [A].
    Slot order is the children's: priors descending, ties higher action first (make_priors); only visited actions matter — an
    unvisited one neither is c* nor gives anything back."""
    N = np.asarray(N, np.uint32); W = np.asarray(W, f32); P = np.asarray(P, f32)
    acts = sorted((a for a in range(N.size) if N[a] > 0), key=lambda a: (-float(P[a]), -a))
    pol = np.zeros(N.size, f32)
    if not acts:
        return pol
    left = prune_slots([N[a] for a in acts], [W[a] for a in acts], [P[a] for a in acts], int(root_visits), float(k), c_init, c_base)
    total = float(sum(left))
    for a, n in zip(acts, left):
        pol[a] = f32(float(n) / total)
    return pol


def raw_target(N):
    """the policy row without pruning: f32(N / sum(N)) in float64"""
    N = np.asarray(N, np.uint32)
    return (N.astype(np.float64) / float(N.astype(np.uint64).sum())).astype(f32)


class ForcedTree(Tree):
    """leaf_batch_model.Tree with rule 2 at the root.  run(iterations, forced=...) switches it per move (a fast move of the playout cap
    runs plain).  After a run: n_root (root selections of that run), n_differ (forced picks that differ from best_puct_index's choice),
    n_free (root selections with nothing owed); with keep_rows, `rows` = (P, W, N, parent visits, oracle's best) of every root selection."""

    def __init__(self, *a, forced_k=0.0, keep_rows=False, **kw):
        self.forced_k, self.forced_on, self.keep_rows = float(forced_k), False, keep_rows
        self.n_root = self.n_differ = self.n_free = 0
        self.rows = []
        super().__init__(*a, **kw)

    def run(self, iterations, forced=True):
        self.forced_on = bool(forced) and self.forced_k > 0.0
        self.n_root = self.n_differ = self.n_free = 0
        self.rows = []
        out = super().run(iterations)
        out.update(n_root=self.n_root, n_differ=self.n_differ, n_free=self.n_free)
        return out

    def _select(self):
        node, path, pv = self.root, [], self.root_visits
        while True:
            if node.terminal:
                wins = [i for i in range(node.n_children) if node.child[i] == WIN]
                cand = wins if np.any(node.W[:node.n_children] > 0) else list(range(node.n_children))
                k = self.O.pick(self.seed, self.slot, self.seq, self.tree, self.event, len(cand)); self.event += 1
                path.append((node, cand[k]))
                return 1, node, path, node.child[cand[k]] == WIN
            best = self.O.best_puct_index(node.P, node.W, node.N, pv, self.c_init, self.c_base)
            if node is self.root:
                self.n_root += 1
                if self.keep_rows:
                    self.rows.append((node.P.copy(), node.W.copy(), node.N.copy(), int(pv), best))
                if self.forced_on:
                    owed = owed_slots(node.N, node.P, node.n_children, pv, self.forced_k)
                    if owed:
                        self.n_differ += owed[0] != best
                        best = owed[0]
                    else:
                        self.n_free += 1
            if best == node.n_children + node.n_reserved:
                return 0, node, path, False
            assert best < node.n_children + node.n_reserved, "PUCT picked an un-poppable child"
            if best >= node.n_children:
                return 2, node, path, False
            path.append((node, best))
            pv = int(node.N[best]); node = node.child[best]

"""Evaluators whose outputs are tied, exactly zero or saturated — what a fresh network (near-uniform heads), a sharp float32 softmax
(exact 0.0 on many cells at once) and tanh (exactly +-1) give, and what the hash evaluator and randomly initialised networks never do.

Every kind is a pure function state int8 [H, W, C] -> (policy float32 [A], value float32) seeded by the CRC-32 of the state bytes, so the
oracle, the Python models and the engine (through GAZ_EVAL_EXTERNAL) may ask in any order and get the same answer.  Legality comes from
the board plane of the state (the last channel): Connect4 = the top row, the other games = the empty cells.

  uniform    policy 1 / A, value 0
  dups       priors drawn from {1, 2, 3} / sum — all positive —, value from {-1, -.5, 0, .5, 1}
  zeros      priors drawn from {0, 1, 2} / sum with at least one positive legal entry, value as dups
  saturated  priors as dups, value exactly -1, 0 or +1
  zeromass   as dups, but on one state in four every legal entry is 0.0 and the mass sits on the occupied cells (all of it is 0.0 where
             nothing is occupied): the node's legal mass is 0 — the zero-mass rule of DESIGN.md

A row of kind uniform / dups / saturated with two or more legal actions has at least two EQUAL legal priors by construction (the second
legal entry repeats the first one's draw); Evaluator asserts it on every row it makes."""
import zlib

import numpy as np

f32 = np.float32
KINDS = ("uniform", "dups", "zeros", "saturated", "zeromass")
VALUES5 = np.array([-1.0, -0.5, 0.0, 0.5, 1.0], f32)
VALUES3 = np.array([-1.0, 0.0, 1.0], f32)
ZEROMASS_SHARE = 4                                  # one state in four
_M32 = np.uint64(0xFFFFFFFF)


def legal_masks(states, A):
    """legal actions of n positions from the board plane: bool [n, A]"""
    board = np.asarray(states)[..., -1]                                  # [n, H, W]
    if A == board.shape[2] and A != board.shape[1] * board.shape[2]:      # Connect4: a column is open while its top cell is empty
        return board[:, 0, :] == 0
    return board.reshape(board.shape[0], -1) == 0


def legal_mask(state, A):
    return legal_masks(np.asarray(state)[None], A)[0]


_WEYL = {}


def _draws(seeds, n):
    """n pseudo-random uint32 per 32-bit seed (murmur3 finaliser over a Weyl sequence; uint32 arrays wrap around): [len(seeds), n]"""
    w = _WEYL.get(n)
    if w is None:
        w = _WEYL[n] = np.arange(1, n + 1, dtype=np.uint32) * np.uint32(0x9E3779B1)
    x = w[None, :] + seeds[:, None]
    x ^= x >> np.uint32(16); x *= np.uint32(0x85EBCA6B)
    x ^= x >> np.uint32(13); x *= np.uint32(0xC2B2AE35)
    x ^= x >> np.uint32(16)
    return x


def evaluate_many(kind, states, A):
    """the pure function, row by row of states int8 [n, H, W, C]: -> (policy f32 [n, A], value f32 [n], legal bool [n, A]).  Every sum is
    one of small integers, exact in float32 in any order, so a row does not depend on the rows it is batched with."""
    s = np.ascontiguousarray(states, np.int8)
    n = s.shape[0]
    legal = legal_masks(s, A)
    if kind == "uniform":
        return np.full((n, A), f32(1.0) / f32(A), f32), np.zeros(n, f32), legal
    flat = s.reshape(n, -1)
    seeds = np.fromiter((zlib.crc32(flat[i].tobytes()) for i in range(n)), np.uint32, n)
    d = _draws(seeds, A + 1)
    raw = (d[:, :A] % np.uint32(3)).astype(f32)                   # {0, 1, 2}
    rows, first = np.arange(n), legal.argmax(1)                   # (first legal action; 0 where there is none)
    if kind == "zeros":
        fix = legal.any(1) & ~((raw > 0) & legal).any(1)
        raw[rows[fix], first[fix]] = 1.0
    else:
        raw += f32(1.0)                                           # {1, 2, 3}
        rest = legal.copy(); rest[rows, first] = False
        two, second = rest.any(1), rest.argmax(1)
        raw[rows[two], second[two]] = raw[rows[two], first[two]]  # two equal legal priors, whatever was drawn
    if kind == "zeromass":
        raw[((seeds >> np.uint32(8)) % np.uint32(ZEROMASS_SHARE) == 0)[:, None] & legal] = 0.0
    total = raw.sum(1, dtype=f32)
    policy, some = raw.copy(), total > 0
    policy[some] = raw[some] / total[some, None]
    values = VALUES3 if kind == "saturated" else VALUES5
    return policy, values[d[:, A] % np.uint32(values.size)], legal


def evaluate(kind, state, A):
    """one state [H, W, C] -> (policy f32 [A], value f32, legal bool [A])"""
    p, v, m = evaluate_many(kind, np.asarray(state)[None], A)
    return p[0], v[0], m[0]


_ROWS = {}                                           # (kind, A) -> {state bytes: (policy, value, tied, zero, zeromass)}: the functions are pure


class Evaluator:
    """evaluate(kind, ., A) behind a table keyed by the state bytes (shared by all instances: the functions are pure), with the witness
    counts of the DISTINCT rows THIS instance was asked for: rows, rows with two equal legal priors, rows with an exactly zero legal prior,
    rows whose legal mass is zero"""

    def __init__(self, kind, A):
        assert kind in KINDS, kind
        self.kind, self.A, self.table, self.seen = kind, int(A), _ROWS.setdefault((kind, int(A)), {}), set()
        self.n_tied = self.n_zero = self.n_zeromass = 0

    @property
    def n_rows(self):
        return len(self.seen)

    def _make(self, keys, states):
        policy, value, legal = evaluate_many(self.kind, states, self.A)
        n_legal = legal.sum(1)
        q = np.sort(np.where(legal, policy, -(np.arange(self.A, dtype=f32) + f32(1.0))), axis=1)     # illegal entries: distinct, negative
        tied = (q[:, 1:] == q[:, :-1]).any(1)
        positive = (policy > 0) & legal
        zero, zeromass = ((policy == 0) & legal).any(1), (n_legal > 0) & ~positive.any(1)
        if self.kind in ("uniform", "dups", "saturated"):
            assert (tied | (n_legal < 2)).all() and (positive == legal).all(), self.kind
            assert np.isin(value, [0.0] if self.kind == "uniform" else VALUES3 if self.kind == "saturated" else VALUES5).all()
        if self.kind == "zeros":
            assert not zeromass.any()
        for i, k in enumerate(keys):
            self.table[k] = (policy[i], value[i], bool(tied[i]), bool(zero[i]), bool(zeromass[i]))

    def many(self, states):
        """states int8 [n, H, W, C] -> (policy f32 [n, A], value f32 [n])"""
        s = np.ascontiguousarray(states, np.int8)
        keys = [s[i].tobytes() for i in range(s.shape[0])]
        new = {k: i for i, k in enumerate(keys) if k not in self.table}
        if new:
            self._make(list(new), s[list(new.values())])
        pol, val = np.empty((len(keys), self.A), f32), np.empty(len(keys), f32)
        for i, k in enumerate(keys):
            hit = self.table[k]
            if k not in self.seen:
                self.seen.add(k)
                self.n_tied += hit[2]; self.n_zero += hit[3]; self.n_zeromass += hit[4]
            pol[i], val[i] = hit[0], hit[1]
        return pol, val

    def __call__(self, state):
        pol, val = self.many(np.asarray(state)[None])
        return pol[0], val[0]

    def witness(self):
        return dict(rows=self.n_rows, tied=self.n_tied, zero=self.n_zero, zeromass=self.n_zeromass)


class Constant:
    """one (policy, value) pair for every state: what a network whose heads ignore the trunk gives"""

    def __init__(self, policy, value):
        self.policy, self.value = np.asarray(policy, f32).copy(), f32(value)

    def __call__(self, state):
        return self.policy, self.value

    def many(self, states):
        n = np.asarray(states).shape[0]
        return np.broadcast_to(self.policy, (n, self.policy.size)), np.full(n, self.value, f32)

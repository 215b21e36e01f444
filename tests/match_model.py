"""Test model of match play (gaz_engine_set_match): the games of one engine played by two networks.

The rule, restated here and never read back from the engine under test: in game (slot, game_seq) network A plays the first player (-1)
iff slot + game_seq is even; a request of PUCT tree k (tree 0 searches for player -1) or, with the Gumbel search, of the player to move
(-1 -> 0, 1 -> 1) is answered by network  owner ^ ((slot + game_seq) & 1)  (0 = A, 1 = B).

PUCT: two leaf_batch_model.Tree(K = 1), each with the evaluator of the network that owns it, driven with the moves the engine played.
Gumbel: oracle.selfplay_game_gumbel with an evaluator that routes every call by the ply it belongs to.  The oracle evaluates in the
order root(ply 0), the evals[0] expansions of ply 0, root(ply 1), ... — a root is evaluated unless its position has a terminal move —
so the ply of call i follows from the record's `evals` and from whether the call's state is the root position of the next ply, which the
game's rules give from the record's actions.  The oracle's own `evals` must then equal the record's: a schedule that passes is the true
one, since the first ply at which it was wrong would change that ply's own count."""
import numpy as np

from grok_alpha_zero_amd.games import GAMES
from leaf_batch_model import Tree

A_OF = {"TicTacToe": 9, "Connect4": 7, "Gomoku": 225}


def colour(slot, seq):
    """0: network A plays the first player (-1) of game (slot, game_seq); 1: network B does"""
    return (int(slot) + int(seq)) & 1


def hash_pair(oracle, game, salt_a, salt_b):
    """[network A, network B] as evaluators: the hash evaluator under two salts"""
    A = A_OF[game]
    return [lambda s, salt=salt: oracle.hash_eval(s, A, salt) for salt in (salt_a, salt_b)]


def puct_plies(oracle, game, seed, iterations, slot, seq, actions, nets, mode_at=None, **kw):
    """-> per ply the runner's Tree.run dict.  nets = [A, B]; mode_at(ply) -> whether match play is on while the requests that follow the
    search of `ply` (the re-rooting after its move, then the search of ply + 1) are answered; None = always.  Off = everything is A's"""
    c = colour(slot, seq)
    state = {"on": True if mode_at is None else bool(mode_at(-1))}
    evs = [(lambda s, k=k: nets[(k ^ c) if state["on"] else 0](s)) for k in range(2)]
    trees = [Tree(oracle, game, 1, seed, slot=slot, game_seq=seq, tree=k, evaluator=evs[k], **kw) for k in range(2)]
    out = []
    for ply, a in enumerate(actions):
        out.append(trees[ply % 2].run(iterations))
        if ply + 1 == len(actions):
            break
        if mode_at is not None:
            state["on"] = bool(mode_at(ply))
        for t in trees:
            t.play(a)
    return out


def assert_puct_record(oracle, game, seed, iterations, max_actions, rec, nets, what, **kw):
    """the record of one finished game against the model, exactly: root N / W / P, root visits and evaluator calls of every ply, and the
    result of the game by the rules"""
    plies = puct_plies(oracle, game, seed, iterations, rec["slot"], rec["game_seq"], rec["actions"], nets, **kw)
    assert len(plies) == rec["T"], what
    for ply, m in enumerate(plies):
        for k, rk in (("N", "root_N"), ("W", "root_W"), ("P", "root_P")):
            np.testing.assert_array_equal(rec[rk][ply], m[k], err_msg=f"{what} ply {ply} {k}")
        assert int(rec["root_visits"][ply]) == m["root_visits"] and int(rec["evals"][ply]) == m["evals"], (what, ply)
    assert rec["winner"] == winner_of(game, rec["actions"], max_actions), what


def winner_of(game, actions, max_actions):
    """the result of the game these moves make, by the rules; a game that reaches max_actions plies is a draw whatever its last move did
    (Self_Play.py:142-157)"""
    G = GAMES[game]
    board, player, hist, r = np.zeros((G.H, G.W), np.int8), -1, [], -2
    for a in actions:
        assert r == -2, "moves after the end of the game"
        G.do_action_MCTS(board, G.index_to_action(int(a)), player); hist.append(G.index_to_action(int(a)))
        r = G.check_win_MCTS(board, player, np.array(hist))
        player = -player
    return 0 if r == -2 or len(actions) >= max_actions else int(r)


class GumbelRouter:
    """the evaluator of oracle.selfplay_game_gumbel for one game of a match (see the module docstring)"""

    def __init__(self, game, slot, seq, rec, nets):
        G = GAMES[game]
        self.nets, self.c, self.evals = nets, colour(slot, seq), [int(e) for e in rec["evals"]]
        self.roots, self.ply, self.left, self.calls = [], -1, 0, [0, 0]
        board, player, hist = np.zeros((G.H, G.W), np.int8), -1, []
        for a in rec["actions"]:
            self.roots.append(np.ascontiguousarray(G.get_input_state_MCTS(board, -player, np.array(hist)), np.int8))
            G.do_action_MCTS(board, G.index_to_action(int(a)), player); hist.append(G.index_to_action(int(a))); player = -player

    def __call__(self, s):
        root = False
        while self.left == 0 and not root:
            self.ply += 1
            assert self.ply < len(self.evals), "more evaluator calls than the record's plies account for"
            self.left = self.evals[self.ply]
            root = np.array_equal(s, self.roots[self.ply])
        if not root:
            self.left -= 1
        net = (self.ply & 1) ^ self.c                                 # the player to move at ply p is -1 iff p is even
        self.calls[net] += 1
        return self.nets[net](s)

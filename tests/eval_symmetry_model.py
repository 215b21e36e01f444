"""Test model of the search's random evaluation symmetry (gaz_engine_set_eval_symmetry).

The rule is restated here in numpy and through the oracle's variates, never read from the product code: the position key is a hash of the
int8 board (the state's last channel, cells in canonical order c = y * W + x), the draw is oracle.uniform(seed, slot, game_seq, tree 2,
event = key, purpose 7), the transforms are written out as index arithmetic on (y, x).  sym_eval wraps any evaluator state -> (policy, value):
being a function of the state alone (for a fixed game) it plugs into oracle.selfplay_game, oracle.selfplay_game_gumbel,
leaf_batch_model.Tree and forced_playouts_model.ForcedTree unchanged."""
import numpy as np

P_EVAL_SYMMETRY = 7                                 # det::P_EVAL_SYMMETRY
NSYM = {"TicTacToe": 8, "Connect4": 2, "Gomoku": 8}
INVERSE = (0, 1, 2, 7, 4, 5, 6, 3)
_M64 = (1 << 64) - 1


def mix64(x):
    x &= _M64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & _M64
    x ^= x >> 31
    return x


def _mix64_u64(x):
    """mix64 on a uint64 array (the arithmetic wraps)"""
    x = x ^ (x >> np.uint64(30)); x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27)); x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def position_event(board):
    """board int8 [H, W] -> the 32-bit event of the draw: h = sum over cells c of mix64((c + 1) << 32 | uint8(board[c])) mod 2^64,
    event = mix64(h) >> 32"""
    cells = np.ascontiguousarray(board, np.int8).reshape(-1).view(np.uint8).astype(np.uint64)
    with np.errstate(over="ignore"):
        keys = (np.arange(1, cells.size + 1, dtype=np.uint64) << np.uint64(32)) | cells
        h = int(_mix64_u64(keys).sum(dtype=np.uint64))
    return mix64(h) >> 32


def draw(oracle, game, seed, slot, game_seq, board):
    """the symmetry k of a request for `board` in game (seed, slot, game_seq)"""
    n = NSYM[game]
    u = oracle.uniform(seed, slot, game_seq, 2, position_event(board), P_EVAL_SYMMETRY)
    return min(n - 1, int(u * n))


def src_cell(game, k, y, x, n):
    """cell (y, x) of T_k(m) shows m[src]: the list of games._GridGame.augment_sample written out (np.rot90 turns counter-clockwise:
    rot90(m)[y][x] = m[x][n - y]); Connect4: the column mirror.  n = side - 1 (Connect4: W - 1)"""
    if game == "Connect4":
        return (y, n - x) if k else (y, x)
    return ((y, x), (n - y, x), (y, n - x), (x, n - y), (x, y), (n - x, n - y), (n - y, n - x), (n - x, y))[k]


_SRC = {}


def src_table(game, k, H, W):
    """flat source cell of every flat cell of T_k, from src_cell"""
    t = _SRC.get((game, k, H, W))
    if t is None:
        t = _SRC[(game, k, H, W)] = np.array([src_cell(game, k, y, x, W - 1)[0] * W + src_cell(game, k, y, x, W - 1)[1] for y in range(H) for x in range(W)])
    return t


def transform(game, state, k):
    """T_k of an [H, W, ...] array over axes (0, 1): out[c] = state[src_k(c)]"""
    s = np.asarray(state)
    H, W = s.shape[:2]
    flat = s.reshape((H * W,) + s.shape[2:])
    return np.ascontiguousarray(flat[src_table(game, k, H, W)].reshape(s.shape))


def untransform_policy(game, policy, k, H, W):
    """T_k^-1 of the network's policy: entry of the original action at cell c = net_policy[dst_k(c)], dst_k the inverse of src_k"""
    p = np.asarray(policy, np.float32).reshape(-1)
    out = np.empty_like(p)
    if game == "Connect4":
        out[src_table(game, k, 1, W)] = p            # network column x shows the position's column src_k(x)
    else:
        out[src_table(game, k, H, W)] = p            # network cell c shows the position's cell src_k(c)
    return out


def invariant(game, board, k):
    return np.array_equal(transform(game, board, k), np.asarray(board))


class sym_eval:
    """base(T_k(state)) with the policy mapped back; keeps a log of (k, board) per request for the witnesses"""

    def __init__(self, oracle, base, game, seed, slot, game_seq, log=None):
        self.O, self.base, self.game, self.seed, self.slot, self.seq, self.log = oracle, base, game, seed, slot, game_seq, log

    def __call__(self, state):
        s = np.asarray(state, np.int8)
        board = s[..., -1]
        k = draw(self.O, self.game, self.seed, self.slot, self.seq, board)
        if self.log is not None:
            self.log.append((k, board.copy()))
        policy, value = self.base(np.ascontiguousarray(transform(self.game, s, k)))
        return untransform_policy(self.game, policy, k, s.shape[0], s.shape[1]), value


def assert_witnesses(game, log, what=""):
    """every k occurred; square boards: k = 3 and k = 7 each on a board that is not invariant under it (a src / dst mix-up passes otherwise)"""
    ks = {k for k, _ in log}
    assert ks == set(range(NSYM[game])), (what, sorted(ks))
    for k in ((3, 7) if game != "Connect4" else (1,)):
        assert any(kk == k and not invariant(game, b, k) for kk, b in log), (what, k)

"""The rules of the replay window (include/gaz_engine.h, the gaz_replay_* section, rules 1-5) restated in numpy from det.philox, with
games.augment_sample for the transforms.  Never derived from the library under test: the tests feed both the same rows and compare bytes.

A window's contents are described by `games`: a list of (generation, index within the generation, rows) in store order; row s of the store
order is then (g, i, j) by counting."""
import numpy as np

from grok_alpha_zero_amd.det import philox

KEY = 0x5245504C41590000
N_AUG = {"TicTacToe": 8, "Connect4": 2, "Gomoku": 8}


def key(seed):
    k = (seed ^ KEY) & 0xFFFFFFFFFFFFFFFF
    return k & 0xFFFFFFFF, k >> 32


def ph(seed, c0, c1, c2, c3):
    return philox(c0 & 0xFFFFFFFF, c1 & 0xFFFFFFFF, c2 & 0xFFFFFFFF, c3 & 0xFFFFFFFF, *key(seed))


def u52(words):
    x, y = words[0], words[1]
    return float(((x >> 6) << 26) | (y >> 6)) * (1.0 / 4503599627370496.0)


def row_ids(games):
    """[(g, i, j)] of every stored row, in store order"""
    return [(g, i, j) for g, i, n in games for j in range(n)]


def held_out(seed, gij, test_fraction):
    g, i, j = gij
    return u52(ph(seed, g, i, j, 0x80000000)) < test_fraction


def admitted(games, newest, target_ratio):
    """rule 2 -> one bool per game of `games` (store order).  target_ratio None = NaN = no balancing"""
    out = [False] * len(games)
    f = s = 0
    gens = sorted({g for g, _, _ in games if g <= newest}, reverse=True)
    for gen in gens:
        for k, (g, _, n) in enumerate(games):
            if g != gen:
                continue
            if target_ratio is None:
                out[k] = True
                continue
            ratio = 0.0 if f + s == 0 else f / (f + s)
            if n % 2 == 1:
                if ratio - 0.02 > target_ratio:
                    continue
                f += 1
            else:
                if ratio + 0.02 < target_ratio:
                    continue
                s += 1
            out[k] = True
    return out


def philox_np(c0, c1, c2, c3, k0, k1):
    """det.philox on uint64 arrays of counters (the same ten rounds; tests/test_replay_emu.py compares the two) -> the first two words"""
    M32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & M32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1


def u52_np(x, y):
    return (((x >> np.uint64(6)) << np.uint64(26)) | (y >> np.uint64(6))).astype(np.float64) * (1.0 / 4503599627370496.0)


def plan(seed, games, split, epoch, newest, percent, decay, test_fraction, target_ratio):
    """rules 1-3 -> the included rows (store order), ascending"""
    adm = admitted(games, newest, target_ratio)
    n = np.array([r for _, _, r in games], np.int64)
    g = np.repeat(np.array([x for x, _, _ in games], np.int64), n)
    i = np.repeat(np.array([x for _, x, _ in games], np.int64), n)
    j = np.concatenate([np.arange(r) for r in n]) if len(n) else np.zeros(0, np.int64)
    ok = np.repeat(np.array(adm, bool), n) & (g <= newest)
    p = np.maximum(percent - (newest - g).astype(np.float64) * decay, 0.0)
    k0, k1 = key(seed)
    gu, iu, ju = g.astype(np.uint64) & np.uint64(0xFFFFFFFF), i.astype(np.uint64), j.astype(np.uint64)
    held = u52_np(*philox_np(gu, iu, ju, np.full(len(g), 0x80000000, np.uint64), k0, k1)) < test_fraction
    draw = u52_np(*philox_np(gu, iu, ju, np.full(len(g), 0x40000000 | epoch, np.uint64), k0, k1))
    return np.flatnonzero(ok & (held == bool(split)) & (draw < p)).astype(np.uint32)


def perm(seed, q, M, epoch, split):
    h = 1
    while 4 ** h < M:
        h += 1
    mask = (1 << h) - 1
    x = q
    while True:
        L, R = x >> h, x & mask
        for r in range(4):
            L, R = R, L ^ (ph(seed, R, r, epoch, 0xC0000010 | split)[0] & mask)
        x = (L << h) | R
        if x < M:
            return x


def symmetry(seed, q, epoch, split, n_aug, augment=True):
    return (ph(seed, epoch, q, split, 0xC0000000)[0] * n_aug) >> 32 if augment else 0


def augmented(game_class, board, policy):
    """the n_aug planes of ONE row through the plugin's augment_sample -> boards [n_aug, H, W, C], policies [n_aug, A]"""
    if game_class.__name__ == "Connect4":
        b, p = game_class.augment_sample(board[None], policy[None])
    else:
        b, p = game_class().augment_sample(board[None], policy[None])
    return np.asarray(b)[:, 0].astype(np.int8), np.asarray(p, np.float32)[:, 0]


def epoch_rows(seed, plan_rows, epoch, split, n_aug, first, n, augment=True):
    """positions first .. first + n - 1 -> (source rows uint32 [n], symmetries uint8 [n])"""
    M = len(plan_rows)
    rows = np.array([plan_rows[perm(seed, q, M, epoch, split)] for q in range(first, first + n)], np.uint32)
    sym = np.array([symmetry(seed, q, epoch, split, n_aug, augment) for q in range(first, first + n)], np.uint8)
    return rows, sym

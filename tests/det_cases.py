"""The cases of the math probe (SelfPlayEngine.probe_det, csrc/det_probe.hpp), shared by tests/test_det_probe_emu.py (emulation build)
and tests/test_det_probe_gpu.py (HIP build): the inputs, the oracle's answers and the comparison.

Every comparison is on bits: the device's uint64 words against the words made from the oracle's results, 0 mismatches allowed, no
tolerance, nothing skipped or filtered afterwards.  Inputs outside a function's domain are not generated.  Every case prints and asserts
its WITNESSES — facts computed from the inputs and the oracle alone, never from the device — that the inputs reach the branch the case
names.  Element ops run at 1, 63, 64, 65 items and at their full size (a launch that fills no wavefront, one, and one lane more).

The reference of the plain float64 division is the host's IEEE-754 division (numpy float64, correctly rounded): the oracle's own
divisions are that instruction.
"""
from contextlib import closing
from fractions import Fraction

import numpy as np

from grok_alpha_zero_amd import engine as E

MAXT = {"TicTacToe": 9, "Connect4": 42, "Gomoku": 225}
A_OF = {"TicTacToe": 9, "Connect4": 7, "Gomoku": 225}
# team shapes: what owns one item of a team op.  On the emulation build a team is one lane whatever the shape, and the shapes differ by
# the game's array sizes only
SHAPES = {"gomoku": ("Gomoku", 0), "ttt-teams": ("TicTacToe", 0), "c4-teams": ("Connect4", 0), "c4-wave": ("Connect4", E.DP_WHOLE_WAVE)}
ALPHAS = (0.03, 0.05, 0.3, 0.5, 1.0, 1.25, 10.0)
RAGGED = (1, 63, 64, 65)
C_INIT, C_BASE = 2.5, 19652.0
SPLIT = 0x6A09E667F3BCD                      # dlog's mantissa split: sqrt(2)
MIN_NORMAL = 2.2250738585072014e-308
POISON = 1e30


def make_engine(game, lib_path):
    return closing(E.SelfPlayEngine(game, 2, 8, MAXT[game], 0, 0, C_INIT, 0.5, seed=1, c_puct_base=C_BASE, lib_path=lib_path))


def b64(x):
    return np.ascontiguousarray(x, np.float64).reshape(-1).view(np.uint64)


def b32(x):
    return np.ascontiguousarray(x, np.float32).reshape(-1).view(np.uint32).astype(np.uint64)


def from_bits(u):
    return np.ascontiguousarray(u, np.uint64).view(np.float64)


def witness(name, text, ok):
    print(f"{name}: witness: {text}: {'yes' if ok else 'NO'}", flush=True)
    assert ok, f"{name}: witness failed: {text}"


def check(name, eng, op, words, want, counts=RAGGED, labels=None):
    """the op at every count of `counts` below the full size, and at the full size: all output words of all items equal `want`.
    Mismatches are counted per output word and, with `labels` (one per item), per label: a failure names what differs"""
    words = np.ascontiguousarray(words, np.uint64); want = np.ascontiguousarray(want, np.uint64)
    n = words.shape[0]
    assert want.shape[0] == n
    total = 0
    for cnt in sorted({c for c in counts if c < n} | {n}):
        got = eng.probe_det(op, words[:cnt], want.shape[1])
        bad = np.flatnonzero((got != want[:cnt]).any(axis=1))
        print(f"{name}: {cnt} items: {bad.size} mismatches", flush=True)
        if bad.size:
            per_word = (got != want[:cnt]).sum(axis=0)
            print(f"  items differing per output word: { {int(c): int(per_word[c]) for c in np.flatnonzero(per_word)[:12]} }", flush=True)
            if labels is not None:
                print(f"  items differing per label: { {str(k): int(sum(1 for i in bad if labels[i] == k)) for k in sorted(set(labels[i] for i in bad))} }", flush=True)
        for i in bad[:6]:
            cols = np.flatnonzero(got[i] != want[i])
            print(f"  item {i}: in {[hex(int(w)) for w in words[i][:12]]} word {int(cols[0])}: device {int(got[i][cols[0]]):#018x} oracle {int(want[i][cols[0]]):#018x}"
                  f" ({cols.size} words differ)", flush=True)
        total += bad.size
    assert total == 0, f"{name}: {total} items differ from the oracle"


def rand_pos_bits(rng, n):
    """random positive finite float64 bit patterns (the biased exponent uniform over 0..2046, 0 = subnormal)"""
    return rng.integers(1, 0x7FF0000000000000, n, dtype=np.uint64)


def rand_subnormal_bits(rng, n):
    return rng.integers(1, 1 << 52, n, dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ scalars
def case_dlog(O, lib_path):
    rng = np.random.default_rng(101)
    one = np.float64(1.0)
    xs = [b64([5e-324]), b64(np.ldexp(1.0, np.arange(-1074, 1024))), b64([np.nextafter(one, 0.0), np.nextafter(one, 2.0), np.finfo(np.float64).max]),
          np.array([(e << 52) | m for e in (1, 1023, 2046) for m in (SPLIT - 1, SPLIT, SPLIT + 1)], np.uint64),
          b64((np.arange(16384, dtype=np.float64) + C_BASE + 1.0) / C_BASE), rand_pos_bits(rng, 4096), rand_subnormal_bits(rng, 64),
          b64([O.u_open(int(a), int(b)) for a, b in rng.integers(0, 1 << 32, (4096, 2), dtype=np.uint64)])]
    x = np.concatenate(xs)
    witness("dlog", "at least 50 subnormal inputs", int(((x >> np.uint64(52)) == 0).sum()) >= 50)
    m = x & np.uint64((1 << 52) - 1)
    witness("dlog", "mantissas on both sides of the sqrt(2) split", bool((m >= SPLIT).any() and (m < SPLIT).any()))
    want = b64([O.det_log(v) for v in from_bits(x)])
    with make_engine("Connect4", lib_path) as eng:
        check("dlog", eng, E.DP_DLOG, x[:, None], want[:, None])


def _exp_k(x):
    """dexp's k for input x (the statements of gaz_exp, in Python's IEEE doubles)"""
    x = min(x, 709.0)
    fk = x * 1.44269504088896338700e+00
    return int(fk + (-0.5 if fk < 0.0 else 0.5))


def case_dexp(O, lib_path):
    rng = np.random.default_rng(102)
    ln2 = 0.6931471805599453
    mid = np.array([(n + 0.5) * ln2 for n in range(-20, 21)])
    xs = np.concatenate([[0.0, -0.0, 709.0, 709.5, 800.0, -745.0, -745.2, -800.0], np.linspace(-745.0, -708.0, 512), mid, np.nextafter(mid, -np.inf),
                         np.nextafter(mid, np.inf), rng.uniform(-746.0, 710.0, 4096), rng.uniform(-1.0, 1.0, 4096)])
    ys = np.array([O.det_exp(v) for v in xs])
    witness("dexp", "the clamp x > 709 is hit", bool((xs > 709.0).any()))
    witness("dexp", "the early zero x < -745 is hit", bool((xs < -745.0).any()))
    witness("dexp", "the k < -1021 path is hit", any(v >= -745.0 and _exp_k(v) < -1021 for v in xs))
    witness("dexp", "some oracle outputs are subnormal", bool(((ys > 0.0) & (ys < MIN_NORMAL)).any()))
    with make_engine("Connect4", lib_path) as eng:
        check("dexp", eng, E.DP_DEXP, b64(xs)[:, None], b64(ys)[:, None])


def case_dpow(O, lib_path):
    pairs = [(0.0, 2.0), (0.0, 0.0), (0.0, 0.5), (1.0, 3.5), (1.0, 0.0), (7.0, 0.0), (2.0, 0.0)]
    pairs += [(float(n), 1.0 / tau) for tau in (0.25, 0.5, 0.8, 1.25, 2.0) for n in range(1, 2001)]
    p = np.array(pairs, np.float64)
    witness("dpow", "x = 0, x = 1 and y = 0 are present", bool((p[:, 0] == 0).any() and (p[:, 0] == 1).any() and (p[:, 1] == 0).any()))
    want = b64([O.det_pow(x, y) for x, y in p])
    with make_engine("Connect4", lib_path) as eng:
        check("dpow", eng, E.DP_DPOW, b64(p).reshape(-1, 2), want[:, None])


def case_dsqrt(O, lib_path):
    rng = np.random.default_rng(104)
    roots = np.concatenate([rng.integers(1, 1 << 26, 511), [1 << 26]]).astype(np.float64)
    x = np.concatenate([b64(np.arange(20001, dtype=np.float64)), np.array([1, (1 << 52) - 1], np.uint64), rand_subnormal_bits(rng, 64), b64(roots * roots),
                        rand_pos_bits(rng, 4096)])
    witness("dsqrt", "subnormal inputs present", int(((x >> np.uint64(52)) == 0).sum()) >= 60)
    witness("dsqrt", "perfect squares up to 2^52 present", bool((roots * roots).max() == 2.0 ** 52))
    want = b64([O.det_sqrt(v) for v in from_bits(x)])
    with make_engine("Connect4", lib_path) as eng:
        check("dsqrt", eng, E.DP_DSQRT, x[:, None], want[:, None])


def case_ddiv(O, lib_path):
    rng = np.random.default_rng(105)
    sign = np.uint64(1) << np.uint64(63)
    a = rand_pos_bits(rng, 6144) | (rng.integers(0, 2, 6144, dtype=np.uint64) * sign)
    b = rand_pos_bits(rng, 6144) | (rng.integers(0, 2, 6144, dtype=np.uint64) * sign)
    # subnormal quotients: a ~ 2^-1000, b ~ 2^30..2^70
    a1 = np.ldexp(rng.uniform(1.0, 2.0, 1024), -1000); b1 = np.ldexp(rng.uniform(1.0, 2.0, 1024), rng.integers(30, 71, 1024))
    # quotients that ROUND to a power of two: possible only where the result is subnormal (its spacing is absolute).  b = m * 2^60,
    # a = m * 2^(60 - 1023 - j) plus k units in the last place: the true quotient is 2^(-1023 - j) * (1 + ~k * 2^-52), and k < 2^(j - 1)
    j = rng.integers(12, 41, 1024); k = rng.integers(1, 1000, 1024).astype(np.uint64)
    b2 = np.ldexp(rng.uniform(1.0, 2.0, 1024), 60)
    a2 = from_bits(b64(np.ldexp(b2, -(1023 + j))) + k)
    av = np.concatenate([from_bits(a), a1, a2]); bv = np.concatenate([from_bits(b), b1, b2])
    with np.errstate(all="ignore"):
        q = av / bv
    sub = (np.abs(q) > 0) & (np.abs(q) < MIN_NORMAL)
    witness("ddiv", "at least 1024 subnormal quotients", int(sub.sum()) >= 1024)
    q2 = q[-1024:]
    pow2 = (b64(q2) & (b64(q2) - np.uint64(1))) == 0                 # a subnormal power of two: one mantissa bit, no exponent bits
    inexact = np.array([Fraction(float(x)) / Fraction(float(y)) != Fraction(float(z)) for x, y, z in zip(a2, b2, q2)])
    witness("ddiv", "at least 512 inexact quotients that round to a power of two", int((pow2 & inexact & (np.abs(q2) < MIN_NORMAL)).sum()) >= 512)
    with make_engine("Connect4", lib_path) as eng:
        check("ddiv", eng, E.DP_DDIV, np.stack([b64(av), b64(bv)], 1), b64(q)[:, None])


def case_philox(O, lib_path):
    rng = np.random.default_rng(106)
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    words = np.concatenate([np.array([c + k for c, k, _ in kat], np.uint64), rng.integers(0, 1 << 32, (1024, 6), dtype=np.uint64)])
    want = np.array([O.philox(w[:4], w[4:]) for w in words], np.uint64)
    witness("philox", "the oracle gives the three Random123 known answers", all(list(want[i]) == kat[i][2] for i in range(3)))
    with make_engine("Connect4", lib_path) as eng:
        check("philox", eng, E.DP_PHILOX, words, want)


def case_draw(O, lib_path):
    rng = np.random.default_rng(107)
    rows, want = [], []
    for lane in (0, 1, 224, 1023, 1024):
        for attempt in (0, 1, 0x1FFFF, 0x20000):
            for purpose in range(8):
                for tree in range(3):
                    key0, key1, slot, seq, event = (int(v) for v in rng.integers(0, 1 << 32, 5, dtype=np.uint64))
                    ev = (key0 | (key1 << 32), slot, seq, tree, event, purpose)
                    r = O.draw(ev, lane, attempt)
                    c3 = (tree << 30) | (purpose << 27) | ((lane & 1023) << 17) | (attempt & 0x1FFFF)
                    assert list(r) == list(O.philox([slot, seq, event, c3], [key0, key1])), "the oracle's own packing of counter word 3"
                    if lane == 1024:
                        assert list(r) == list(O.draw(ev, 0, attempt))
                    if attempt == 0x20000:
                        assert list(r) == list(O.draw(ev, lane, 0))
                    rows.append([key0, key1, slot, seq, event, tree, purpose, lane, attempt]); want.append(r)
    witness("draw", "480 draws, the oracle packs c3 = tree<<30 | purpose<<27 | (lane & 1023)<<17 | (attempt & 0x1FFFF); lane 1024 and attempt 0x20000 wrap",
            len(rows) == 480)
    with make_engine("Connect4", lib_path) as eng:
        check("draw", eng, E.DP_DRAW, np.array(rows, np.uint64), np.array(want, np.uint64))


def case_unit(O, lib_path):
    rng = np.random.default_rng(108)
    words = np.concatenate([np.array([[0, 0], [0xFFFFFFFF, 0xFFFFFFFF], [63, 63], [64, 0], [0, 64]], np.uint64), rng.integers(0, 1 << 32, (4096, 2), dtype=np.uint64)])
    want = np.zeros((words.shape[0], 3), np.uint64)
    for i, (a, b) in enumerate(words):
        want[i, 0] = O.k52(int(a), int(b))
        want[i, 1:] = b64([O.u_open(int(a), int(b)), O.u_half(int(a), int(b))])
    witness("unit", "k52 = 0 (u_half = 0, u_open = 2^-53) and k52 = 2^52 - 1 are present", bool(want[0, 0] == 0 and want[1, 0] == (1 << 52) - 1 and want[2, 0] == 0))
    with make_engine("Connect4", lib_path) as eng:
        check("unit", eng, E.DP_UNIT, words, want)


BIG_PV = (16383, 16384, 10 ** 6, 2 ** 32 + 5)


def case_puct_c(O, lib_path):
    rows = [(float(pv), C_INIT, C_BASE) for pv in range(16384)] + [(float(pv), ci, cb) for pv in BIG_PV for ci, cb in ((C_INIT, C_BASE), (1.25, 1.0), (4.0, 100.0))]
    want = b64([O.puct_factors(int(pv), ci, cb)[1] for pv, ci, cb in rows])
    witness("puct_c", "every table index and parent visits beyond 2^32 are present", len(rows) == 16384 + 12)
    with make_engine("Connect4", lib_path) as eng:
        check("puct_c", eng, E.DP_PUCT_C, b64(np.array(rows, np.float64)).reshape(-1, 3), want[:, None])


def case_puct_table(O, lib_path):
    """the engine's own E.puct_table, filled on the device at create time: all 16384 x 2 entries; and puct_factors' computed path, with
    table = nullptr at every index and with the table past its end"""
    pvs = list(range(16384))
    rows = [(pv, 1) for pv in pvs] + [(pv, 0) for pv in pvs] + [(pv, t) for pv in BIG_PV for t in (0, 1)]
    want = np.zeros((len(rows), 3), np.uint64)
    memo = {}
    for i, (pv, t) in enumerate(rows):
        if pv not in memo:
            memo[pv] = b64(O.puct_factors(pv, C_INIT, C_BASE))
        want[i, :2] = memo[pv]; want[i, 2] = 1 if (t and pv < 16384) else 0
    witness("puct_table", "16384 + 1 items must come from the table (every index, the last one twice), 16384 + 7 from the computed path",
            int(want[:, 2].sum()) == 16385 and len(rows) == 2 * 16384 + 8)
    with make_engine("Connect4", lib_path) as eng:
        check("puct_table", eng, E.DP_PUCT_FACTORS, np.array(rows, np.uint64), want)


# ------------------------------------------------------------------------------------------------ samplers
def case_samplers(O, lib_path, alpha):
    """lanes 0..224 of 64 events: uniform, pick, gumbel, normal (+ draws), gamma (+ draws, accepting test).  The items are in lane order, so a
    wavefront holds 64 consecutive lanes, which leave the rejection loops at different attempts"""
    name = f"samplers[alpha={alpha}]"
    seed = 0x9E3779B97F4A7C15 ^ int(alpha * 1000)
    rows, want = [], []
    for e in range(64):
        slot, seq, tree, event, purpose = 3 + 7 * e, e % 5, e % 3, 1000 + e, e % 8
        ev = (seed, slot, seq, tree, event, purpose)
        pick_n = (1, 2, 7, 9, 225)[e % 5]
        u = int(b64([O.uniform(*ev)])[0]); pk = O.pick_p(ev, pick_n)
        for lane in range(225):
            nv, nd = O.normal(ev, lane)
            gv, gd, gt = O.gamma(ev, lane, alpha)
            rows.append([seed & 0xFFFFFFFF, seed >> 32, slot, seq, event, tree, purpose, lane, int(b64([alpha])[0]), pick_n])
            want.append([u, pk, int(b64([O.gumbel_p(ev, lane)])[0]), int(b64([nv])[0]), nd, int(b64([gv])[0]), gd, gt])
    want = np.array(want, np.uint64)
    gd, gt = want[:, 6].astype(np.int64), want[:, 7]
    lo = 3 if alpha < 1.0 else 2                      # the boost's draw, one polar pair, one acceptance uniform
    waves = [gd[i:i + 64] for i in range(0, gd.size - 63, 64)]
    mixed = sum(1 for w in waves if (w == lo).any() and (w >= lo + 3).any())
    print(f"{name}: gamma draws min {gd.min()} max {gd.max()}, waves with both ends {mixed} of {len(waves)}, log-test acceptances {int((gt == 2).sum())}, "
          f"zero variates {int((from_bits(want[:, 5]) == 0.0).sum())}", flush=True)
    witness(name, f"the minimum is {lo} draws", int(gd.min()) == lo)
    witness(name, "a 64-lane wave holds lanes with the minimum of draws and lanes with >= 3 more", mixed >= 1)
    witness(name, "at least one variate accepted by the log test", bool((gt == 2).any()) and bool((gt == 1).any()))
    witness(name, "every pick n of 1, 2, 7, 9, 225 is drawn", set(np.array(rows)[:, 9]) == {1, 2, 7, 9, 225})
    with make_engine("Connect4", lib_path) as eng:
        check(name, eng, E.DP_SAMPLE, np.array(rows, np.uint64), want)


# ------------------------------------------------------------------------------------------------ team reductions
def _sum_lengths():
    """(1, 7, 8, 42) first, then every n = 1..256 dealt so that the four teams of a wavefront hold four different n, small next to large"""
    return [1, 7, 8, 42] + [q * 64 + r + 1 for r in range(64) for q in range(4)]


def case_sums(O, lib_path, shape):
    game, flag = SHAPES[shape]
    rng = np.random.default_rng(110)
    with make_engine(game, lib_path) as eng:
        for dtype, op, bits, osum in ((np.float32, E.DP_SUM_F32, b32, O.np_sum_f32), (np.float64, E.DP_SUM_F64, b64, O.np_sum_f64)):
            name = f"sums[{shape},{np.dtype(dtype).name}]"
            ns = _sum_lengths()
            words = np.zeros((len(ns), 1 + 256), np.uint64); want = np.zeros((len(ns), 1), np.uint64)
            differ = set()
            for i, n in enumerate(ns):
                a = (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(-20.0, 20.0, n)).astype(dtype)
                row = np.full(256, POISON, dtype); row[:n] = a              # behind n: the poison the n < 8 branch must not pick up
                words[i, 0] = n; words[i, 1:] = bits(row)
                ref = osum(a)
                want[i, 0] = bits([ref])[0]
                seq = dtype(0)
                for v in a:
                    seq = dtype(seq + v)
                if seq != dtype(ref):
                    differ.add(n)
            witness(name, f"every n = 1..256 is present, and a left-to-right sum differs from the oracle's at >= 100 lengths ({len(differ)})",
                    set(ns) == set(range(1, 257)) and len(differ) >= 100)
            witness(name, "arrays shorter than 8 carry the poison behind n", bool((words[0, 2:9] == bits([POISON])[0]).all()) and ns[0] == 1)
            check(name, eng, op | flag, words, want, counts=(1, 3))


def case_puct_scores(O, lib_path, shape):
    game, flag = SHAPES[shape]
    A = A_OF[game]; cap = max(A, 8)
    name = f"puct_scores[{shape}]"
    rng = np.random.default_rng(111)
    must = [n for n in (1, 7, 8, 9, 225) if n <= A]
    ns = [must[i % len(must)] if i % 2 == 0 else int(rng.integers(1, A + 1)) for i in range(256)]
    words = np.zeros((256, 3 + 3 * cap), np.uint64); want = np.zeros((256, 1 + A), np.uint64)
    unvisited = negative = 0
    for i, n in enumerate(ns):
        N = rng.integers(1, 60, n).astype(np.uint32)
        N[rng.random(n) < (1.0 if i % 16 == 3 else 0.35)] = 0
        W = (rng.uniform(-1.0, 1.0, n) * np.maximum(N, i % 2)).astype(np.float32)      # odd nodes: an unvisited slot may carry a value (a virtual loss does)
        P = rng.dirichlet(np.full(n, 0.5)).astype(np.float32)
        s, c = O.puct_factors(int(N.sum()) + 1 + (2 ** 33 if i % 64 == 5 else 0), C_INIT, C_BASE)
        unvisited += int((N == 0).sum()); negative += int((W < 0).sum())
        rec = np.zeros((cap, 3), np.uint64); rec[:, 0] = 7; rec[:, 1] = b32([POISON])[0]; rec[:, 2] = b32([POISON])[0]
        rec[:n, 0] = N; rec[:n, 1] = b32(W); rec[:n, 2] = b32(P)
        words[i, 0] = n; words[i, 1:3] = b64([s, c]); words[i, 3:] = rec.reshape(-1)
        best, sc = O.puct_scores(P, W, N, s, c)
        want[i, 0] = best; want[i, 1:1 + n] = b64(sc)
    witness(name, f"n of {must} present, unvisited slots ({unvisited}) and negative W ({negative}) present", set(must) <= set(ns) and unvisited > 0 and negative > 0)
    with make_engine(game, lib_path) as eng:
        check(name, eng, E.DP_PUCT_SCORES | flag, words, want, counts=(1, 3))


# ------------------------------------------------------------------------------------------------ Gumbel
def _gumbel_ns(shape):
    A = A_OF[SHAPES[shape][0]]
    return [n for n in list(range(1, 10)) + [64, 65, 225] if n <= A]


def case_softmax(O, lib_path, shape):
    game, flag = SHAPES[shape]
    A = A_OF[game]; cap = max(A, 8)
    name = f"softmax[{shape}]"
    rng = np.random.default_rng(112)
    ns = [n for n in _gumbel_ns(shape) for _ in range(6)]
    order = rng.permutation(len(ns))
    words = np.zeros((len(ns), 1 + cap), np.uint64); want = np.zeros((len(ns), A), np.uint64)
    tiny = 0
    for i, k in enumerate(order):
        n = ns[k]
        x = rng.uniform(-30.0, 30.0, n) * (25.0 if k % 3 == 2 else 1.0)          # a third of them spread over +-750: exp underflows to 0 and to subnormals
        row = np.full(cap, POISON); row[:n] = x
        words[i, 0] = n; words[i, 1:] = b64(row)
        p = O.softmax(x)
        tiny += int((p < MIN_NORMAL).sum())
        want[i, :n] = b64(p)
    witness(name, f"n < 8 present, n >= 8 present where the game has such nodes, zero / subnormal probabilities present ({tiny})",
            min(ns) < 8 and (max(ns) >= 8 or A < 8) and tiny > 0)
    with make_engine(game, lib_path) as eng:
        check(name, eng, E.DP_SOFTMAX | flag, words, want, counts=(1, 3))


KINDS = ("none", "all", "one", "equal", "equal_raw")


def case_pi(O, lib_path, shape):
    """compute_pi (both modes), N_b, the sum of visits and g_det_select's slot for synthetic nodes; the items are shuffled, so the four teams of a
    wavefront hold nodes of different n, N_b and mode"""
    game, flag = SHAPES[shape]
    A = A_OF[game]; cap = max(A, 8)
    name = f"compute_pi[{shape}]"
    rng = np.random.default_rng(113)
    items = [(n, kind, rep, stable) for n in _gumbel_ns(shape) for kind in KINDS for rep in range(3) for stable in (0, 1)]
    order = rng.permutation(len(items))
    words = np.zeros((len(items), 4 + 4 * cap), np.uint64); want = np.zeros((len(items), 3 + A), np.uint64)
    eps_nodes = 0
    for i, k in enumerate(order):
        n, kind, rep, stable = items[k]
        c_visit, c_scale = ((50.0, 1.0), (0.5, 0.1), (50.0, 0.03))[rep]
        L = rng.uniform(-30.0, 30.0, n).astype(np.float32)
        RAW = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        N = np.zeros(n, np.uint32)
        if kind == "all":
            N = rng.integers(1, 40, n).astype(np.uint32)
        elif kind == "one":
            N[rng.integers(0, n)] = rng.integers(1, 40)
        elif kind == "equal":
            N[:] = rng.integers(1, 40)
        W = (rng.uniform(-1.0, 1.0, n) * N).astype(np.float32)
        if kind == "equal":
            W[:] = W[0]
        if kind == "equal_raw":
            RAW[:] = RAW[0]
        rec = np.zeros((cap, 4), np.uint64); rec[:, 0] = 1000000; rec[:, 1:] = b32([POISON])[0]
        rec[:n, 0] = N; rec[:n, 1] = b32(W); rec[:n, 2] = b32(L); rec[:n, 3] = b32(RAW)
        words[i, 0] = n; words[i, 1] = stable; words[i, 2:4] = b64([c_visit, c_scale]); words[i, 4:] = rec.reshape(-1)
        pi = O.compute_pi(N, W, RAW, L, c_visit, c_scale, stable=bool(stable))
        want[i, 0] = int(N.max()); want[i, 1] = int(N.sum()); want[i, 2] = O.det_select(N, W, RAW, L, c_visit, c_scale, stable=bool(stable))
        want[i, 3:3 + n] = b64(pi) if stable else b32(pi)
        if kind in ("equal", "equal_raw") and not stable:
            # equal completed Q: max - min = 0, den = F32_EPS, every rescaled q is 0 and the logits pass unchanged — the oracle's pi is then softmax(logits)
            assert np.array_equal(pi, O.softmax(L.astype(np.float64)).astype(np.float32)), "the oracle did not take the F32_EPS branch"
            eps_nodes += 1
    ns = {it[0] for it in items}
    witness(name, f"the F32_EPS branch of the rescaling is hit ({eps_nodes} nodes), n < 8 present, n >= 8 present where the game has such nodes",
            eps_nodes > 0 and min(ns) < 8 and (max(ns) >= 8 or A < 8))
    witness(name, "all slots unvisited, all visited and one visited are present, both modes", {it[1] for it in items} == set(KINDS) and {it[3] for it in items} == {0, 1})
    with make_engine(game, lib_path) as eng:
        check(name, eng, E.DP_PI | flag, words, want, counts=(1, 3), labels=["stablemax" if items[k][3] else "softmax" for k in order])


CASES = {"dlog": case_dlog, "dexp": case_dexp, "dpow": case_dpow, "dsqrt": case_dsqrt, "ddiv": case_ddiv, "philox": case_philox, "draw": case_draw,
         "unit": case_unit, "puct_c": case_puct_c, "puct_table": case_puct_table}
for _a in ALPHAS:
    CASES[f"samplers:{_a}"] = (lambda O, lib_path, _a=_a: case_samplers(O, lib_path, _a))
for _s in SHAPES:
    for _k, _f in (("sums", case_sums), ("puct_scores", case_puct_scores), ("softmax", case_softmax), ("compute_pi", case_pi)):
        CASES[f"{_k}:{_s}"] = (lambda O, lib_path, _f=_f, _s=_s: _f(O, lib_path, _s))


def run_case(name, O, lib_path=None):
    CASES[name](O, lib_path)

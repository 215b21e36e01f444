"""The engine's counter-based noise and its bit-reproducible logarithm (csrc/det.hpp) in pure Python: Philox4x32-10 keyed by
(seed, slot, game_seq, tree, event, purpose), the uniform variate of an event, and dlog.  Python floats are IEEE-754 float64 and + - * /
are correctly rounded without contraction, so every value equals the device's bit for bit.  Host definitions only (self_play.py): nothing on
the hot path calls this."""
import struct

M32 = 0xFFFFFFFF
P_OPENING = 4                                      # det::P_OPENING (tree 2: the opening_actions draw; tree 3: the opening book's)
P_PLAYOUT_CAP = 5                                  # det::P_PLAYOUT_CAP


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10: counter (c0..c3), key (k0, k1) -> four uint32"""
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c3 ^ k1) & M32, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def draw(seed, slot, game_seq, tree, event, purpose, lane=0, attempt=0):
    """det::draw: all 32 bits of the event are counter word 2; tree, purpose, lane and attempt share word 3"""
    c3 = ((tree << 30) | (purpose << 27) | ((lane & 1023) << 17) | (attempt & 0x1FFFF)) & M32
    return philox(slot & M32, game_seq & M32, event & M32, c3, seed & M32, (seed >> 32) & M32)


def uniform(seed, slot, game_seq, tree, event, purpose):
    """det::uniform: u_half of the first two words, k52 / 2^52 in [0, 1)"""
    x, y, _, _ = draw(seed, slot, game_seq, tree, event, purpose)
    return float(((x >> 6) << 26) | (y >> 6)) * (1.0 / 4503599627370496.0)


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _double(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def dlog(x):
    """det::dlog: natural log of a finite x > 0, fdlibm's form in a fixed operation order"""
    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    Lg1, Lg2, Lg3, Lg4 = 6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01
    Lg5, Lg6, Lg7 = 1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01
    x = float(x)
    k = 0
    ix = _bits(x)
    if (ix >> 52) == 0:
        x = x * 18014398509481984.0
        ix = _bits(x)
        k -= 54
    e = (ix >> 52) - 1023
    m = ix & 0x000FFFFFFFFFFFFF
    if m >= 0x6A09E667F3BCD:
        e += 1
        ix = m | 0x3FE0000000000000
    else:
        ix = m | 0x3FF0000000000000
    k += e
    f = _double(ix) - 1.0
    dk = float(k)
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (Lg2 + w * (Lg4 + w * Lg6))
    t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)))
    R = t2 + t1
    hfsq = 0.5 * f * f
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f)

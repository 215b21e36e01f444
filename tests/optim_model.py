"""The optimizer step of include/gaz_engine.h ("OPTIMIZER") restated in numpy: every elementwise operation f32 and on a
line of its own, the four dot products as float64 sums in the documented order, the bias corrections from the oracle's dpow.  The model, never
the library, says what a step must give."""
import numpy as np

from oracle import gaz_oracle as O

CHUNK, SLOTS = 2048, 256
F = np.float32
TINY = F(1e-30)


def chunk_sum(prod):
    """float64 sum of one chunk's products (len <= 2048) in the documented order"""
    n = prod.shape[0]
    G = n // 4
    x = np.zeros(SLOTS, np.float64)
    s = np.arange(SLOTS)
    for i in range(CHUNK // 4 // SLOTS):                       # slot s: group s, then group s + 256, the four elements in ascending order
        j = s + i * SLOTS
        on = j < G
        for c in range(4):
            x[on] = x[on] + prod[j[on] * 4 + c]
    for k in range(G * 4, n):                                  # slot 0: the elements behind the last whole group
        x[0] = x[0] + prod[k]
    for d in (32, 16, 8, 4, 2, 1):
        x = x + x[s ^ d]
    return ((x[0] + x[64]) + x[128]) + x[192]


def dot(a, b):
    """sum of a[i] * b[i] (f32 values, exact f64 products): the chunks' sums in ascending order, from +0.0"""
    prod = a.astype(np.float64) * b.astype(np.float64)
    tot = np.float64(0.0)
    for c0 in range(0, prod.shape[0], CHUNK):
        tot = tot + chunk_sum(prod[c0:c0 + CHUNK])
    return tot


def corrections(beta_1, beta_2, t):
    return F(1.0 - O.det_pow(beta_1, float(t))), F(1.0 - O.det_pow(beta_2, float(t)))


def step_tensor(w, g, m, v, e, lr, t, kind=1, beta_1=0.9, beta_2=0.999, epsilon=1e-7, weight_decay=0.0, orthograd=False, grokfast=False, alpha=0.99, lamb=5.0):
    """one tensor through one step -> (w, m, v, e, norms f64 [4], aux); e may be None without grokfast.  Inputs are f32 arrays, untouched.
    aux: what the witnesses and the independent check of the sums look at — w1 (w after the decay), go, gg (g2 * g2), den (sqrt(v / c2), before eps)"""
    lr, wd, b1, b2, eps, al, lm = F(lr), F(weight_decay), F(beta_1), F(beta_2), F(epsilon), F(alpha), F(lamb)
    omb1 = F(1.0) - b1
    omb2 = F(1.0) - b2
    oma = F(1.0) - al
    c1, c2 = corrections(beta_1, beta_2, t)
    norms = np.zeros(4, np.float64)
    go = None
    with np.errstate(all="ignore"):
        if wd != 0:
            a = w * wd
            b = a * lr
            w = w - b
        w1 = w
        g1 = g
        if orthograd:
            norms[0], norms[1], norms[2] = dot(w, g), dot(w, w), dot(g, g)
            den = F(norms[1]) + TINY
            proj = F(norms[0]) / den
            p = proj * w
            go = g - p
            norms[3] = dot(go, go)
            sn = np.sqrt(F(norms[2]))
            sd = np.sqrt(F(norms[3]))
            sd = sd + TINY
            s = sn / sd
            g1 = go * s
        g2 = g1
        if grokfast:
            ea = e * al
            gb = g1 * oma
            e = ea + gb
            el = e * lm
            g2 = g1 + el
        m1 = b1 * m
        m2 = omb1 * g2
        m = m1 + m2
        v1 = b2 * v
        gg = g2 * g2
        v2 = omb2 * gg
        v = v1 + v2
        mh = m / c1
        vh = v / c2
        num = mh
        if kind == 1:
            n1 = mh * b1
            n2 = m2 / c1
            num = n1 + n2
        root = np.sqrt(vh)
        den = root + eps
        u = num / den
        ul = u * lr
        w = w - ul
    for x in (w, m, v):
        assert x.dtype == np.float32
    return w, m, v, e, norms, dict(w1=w1, go=go, gg=gg, root=root)


def layout(sizes):
    """offsets (elements) and the arena's total: every tensor on a 16-byte boundary"""
    offs, at = [], 0
    for n in sizes:
        offs.append(at)
        at += (n + 3) // 4 * 4
    return offs, at

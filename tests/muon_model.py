"""The Muon step of include/gaz_engine.h ("MUON"; the reference's Net/Optimizers/muon.py) restated in numpy: every elementwise
operation f32 and on a line of its own, bf16 rounding on the bit pattern, every matrix product one f32 chain over k ascending, the float64 sums in
the order of tests/optim_model.py.  The model, never the library, says what a step must give.  ns_exact is NOT the rule: it is muon.py's
iteration in float64 with no rounding anywhere, what the rule's result is held against."""
import numpy as np

import optim_model as M

F = np.float32
NS_EPS = F(1e-7)
DEFAULTS = dict(muon_beta=0.95, nesterov=True, muon_a=3.4445, muon_b=-4.7750, muon_c=2.0315, ns_steps=5, adam_lr_ratio=1.0)
THIN = 4


def bf16(x):
    """f32 -> the nearest bf16 value (ties to even) as f32, on the bit pattern; NaN stays NaN"""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u | 0x00400000) & 0xFFFF0000, r)
    return r.astype(np.uint32).view(np.float32).reshape(x.shape)


def chain(a, b):
    """a [M, K] times b [K, N]: every element one f32 chain acc = acc + a[i, k] * b[k, j] over k ascending from +0 (the products are exact)"""
    acc = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in range(a.shape[1]):
        p = np.outer(a[:, k], b[k, :])
        acc = acc + p
    assert acc.dtype == np.float32
    return acc


def scale_of(shape):
    """0.2 * sqrt(max(1, shape[-2] / shape[-1])) in f32"""
    return F(0.2) * np.sqrt(np.maximum(F(1.0), F(shape[-2]) / F(shape[-1])))


def gram(X):
    """bf16(X X^T) of X [P, Q] -> (A, the float64 sums of the thin path or None)"""
    P = X.shape[0]
    if P > THIN:
        return bf16(chain(X, np.ascontiguousarray(X.T))), None
    sums = np.zeros((P, P), np.float64)
    for i in range(P):
        for j in range(i, P):
            sums[i, j] = sums[j, i] = M.dot(np.ascontiguousarray(X[i]), np.ascontiguousarray(X[j]))     # the chunk order over the column index
    return bf16(sums.astype(np.float32)), sums


def newton_schulz(u, rows, cols, muon_a, muon_b, muon_c, ns_steps):
    """u f32 [rows * cols] -> (X f32 [rows * cols] in the tensor's own layout, aux: X0, n, norm64, A, B, gram64, transposed, Xprev = the X [P, Q]
    that entered the last iteration)"""
    a, b, c = bf16(F(muon_a)), bf16(F(muon_b)), bf16(F(muon_c))
    x0 = bf16(u)
    norm64 = M.dot(x0, x0)
    n = np.sqrt(F(norm64))
    d = n + NS_EPS
    q = x0 / d
    X = bf16(q).reshape(rows, cols)
    transposed = rows > cols
    if transposed:
        X = np.ascontiguousarray(X.T)
    P = X.shape[0]
    A, B, g64, prev = np.zeros((P, P), np.float32), np.zeros((P, P), np.float32), None, None
    for _ in range(ns_steps):
        prev = X
        A, g64 = gram(X)
        aa = bf16(chain(A, A))
        t1 = bf16(b * A)
        t2 = bf16(c * aa)
        B = bf16(t1 + t2)
        bx = bf16(chain(B, X))
        ax = bf16(a * X)
        X = bf16(ax + bx)
    if transposed:
        X = np.ascontiguousarray(X.T)
    return X.reshape(-1), dict(X0=x0.reshape(rows, cols), n=n, norm64=norm64, A=A, B=B, gram64=g64, transposed=transposed, Xprev=prev)


def ns_exact(u, rows, cols, muon_a, muon_b, muon_c, ns_steps):
    """muon.py's zeropower_via_newtonschulz5 in float64, nothing rounded -> [rows, cols]"""
    X = np.asarray(u, np.float64).reshape(rows, cols)
    tr = rows > cols
    if tr:
        X = X.T
    X = X / (np.sqrt((X * X).sum()) + 1e-7)
    for _ in range(ns_steps):
        A = X @ X.T
        B = muon_b * A + muon_c * (A @ A)
        X = muon_a * X + B @ X
    return X.T if tr else X


def grad_stages(w, g, e, orthograd, grokfast, alpha, lamb):
    """stages 1 and 2 of Muon mode: Orthograd on the undecayed w, Grokfast -> (g2, e, norms f64 [4], go)"""
    al, lm = F(alpha), F(lamb)
    oma = F(1.0) - al
    norms, go = np.zeros(4, np.float64), None
    g1 = g
    if orthograd:
        norms[0], norms[1], norms[2] = M.dot(w, g), M.dot(w, w), M.dot(g, g)
        den = F(norms[1]) + M.TINY
        proj = F(norms[0]) / den
        p = proj * w
        go = g - p
        norms[3] = M.dot(go, go)
        sn = np.sqrt(F(norms[2]))
        sd = np.sqrt(F(norms[3]))
        sd = sd + M.TINY
        s = sn / sd
        g1 = go * s
    g2 = g1
    if grokfast:
        ea = e * al
        gb = g1 * oma
        e = ea + gb
        el = e * lm
        g2 = g1 + el
    return g2, e, norms, go


def decayed(w, lr, wd):
    if wd == 0:
        return w
    a = lr * wd
    b = a * w
    return w - b


def step_tensor(w, g, m, v, e, lr, t, shape, is_muon, kind=1, beta_1=0.9, beta_2=0.995, epsilon=1e-8, weight_decay=0.0, orthograd=False, grokfast=False,
                alpha=0.99, lamb=5.0, muon_beta=0.95, nesterov=True, muon_a=3.4445, muon_b=-4.7750, muon_c=2.0315, ns_steps=5, adam_lr_ratio=1.0):
    """one tensor through one step in Muon mode -> (w, m, v, e, norms, aux).  For a Muon tensor v is u, and aux is newton_schulz's."""
    lr, wd = F(lr), F(weight_decay)
    with np.errstate(all="ignore"):
        g2, e, norms, go = grad_stages(w, g, e, orthograd, grokfast, alpha, lamb)
        if not is_muon:
            lr_a = F(adam_lr_ratio) * lr
            # stage 4 of section 28 at lr_a with no decay in front (g2 passed as the gradient of a plain Adam step), then the decay
            w2, m, v, _, _, _ = M.step_tensor(w, g2, m, v, None, lr_a, t, kind=kind, beta_1=beta_1, beta_2=beta_2, epsilon=epsilon)
            return decayed(w2, lr_a, wd), m, v, e, norms, dict(go=go)
        beta = F(muon_beta)
        omb = F(1.0) - beta
        m1 = beta * m
        m2 = g2 * omb
        m = m1 + m2
        u = m
        if nesterov:
            mb = m * beta
            u = g2 + mb
        rows, cols = int(shape[0]), int(np.prod(shape[1:]))
        X, aux = newton_schulz(u, rows, cols, muon_a, muon_b, muon_c, ns_steps)
        xs = X * scale_of(shape)
        ul = xs * lr
        w2 = w - ul
        w = decayed(w2, lr, wd)
    aux.update(go=go, X=X.reshape(rows, cols), u=u)
    for x in (w, m, u):
        assert x.dtype == np.float32
    return w, m, u, e, norms, aux

"""The held-out loss rule (include/gaz_engine.h "HELD-OUT LOSS") restated in numpy, one row at a time, out of the oracle's
pinned operations: oracle.det_log (det::dlog), oracle.softmax (gumbel_core.hpp softmax_inplace: det::dexp of x - max, numpy's pairwise sum, a
divide) and oracle.np_sum_f64 (numpy's pairwise add-reduce).  Everything is float64; the cases compare raw bits.

    score_rows(P, v, y, z, mode) -> per-row ce, entropy, se (f64) and flags (u8)
    totals(ce, ent, se, flags, mode) -> the dict SelfPlayEngine.score_outputs returns: np.sum of blocks of 128 rows, the blocks added left to right
"""
import numpy as np

from oracle import gaz_oracle as O

TOP1, VSIGN, VROW, BAD = 1, 2, 4, 8
EPS = 1e-7                                          # Keras' epsilon
BLOCK = 128


def probabilities(P_row, mode):
    """the prediction of one row as probabilities q (float64 [A]); modes 0 / 2: as given, not renormalised"""
    x = np.asarray(P_row, np.float32).astype(np.float64)
    if mode in (0, 2):
        return x
    if mode == 1:
        return O.softmax(x)
    s = np.array([xa + 1.0 if xa >= 0.0 else 1.0 / (1.0 - xa) for xa in x], np.float64)
    return s / O.np_sum_f64(s)


def score_row(P_row, v, y_row, z, mode):
    P_row, y_row = np.asarray(P_row, np.float32), np.asarray(y_row, np.float32)
    v, z = np.float32(v), np.float32(z)
    if not (np.isfinite(P_row).all() and np.isfinite(v)):
        return 0.0, 0.0, 0.0, BAD
    q = probabilities(P_row, mode)
    t = np.zeros(len(y_row), np.float64)
    e = np.zeros(len(y_row), np.float64)
    for a, ya in enumerate(y_row):
        if ya > 0:
            yd = float(ya)
            t[a] = yd * O.det_log(max(float(q[a]), EPS))
            e[a] = yd * O.det_log(yd)
    ce, ent = -O.np_sum_f64(t), -O.np_sum_f64(e)
    d = float(v) - float(z)
    flags = (TOP1 if int(np.argmax(P_row)) == int(np.argmax(y_row)) else 0) | (VSIGN if z != 0 and float(v) * float(z) > 0.0 else 0) | (VROW if z != 0 else 0)
    return ce, ent, d * d, flags


def score_rows(P, v, y, z, mode):
    """P, y f32 [n, A]; v, z f32 [n] -> (ce, entropy, se) float64 [n], flags uint8 [n]"""
    P, y = np.asarray(P, np.float32), np.asarray(y, np.float32)
    v, z = np.asarray(v, np.float32).reshape(-1), np.asarray(z, np.float32).reshape(-1)
    n = v.shape[0]
    ce, ent, se, fl = np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.uint8)
    for r in range(n):
        ce[r], ent[r], se[r], fl[r] = score_row(P[r], v[r], y[r], z[r], mode)
    return ce, ent, se, fl


def block_sum(x):
    """np.sum of each block of 128 rows, the blocks added left to right"""
    tot = 0.0
    for b in range(0, len(x), BLOCK):
        tot = tot + O.np_sum_f64(x[b:b + BLOCK])
    return float(tot)


def totals(ce, ent, se, flags, mode):
    """the dict of engine.score_dict, from the per-row arrays"""
    nan = float("nan")
    rows, bad = len(flags), int(((flags & BAD) != 0).sum())
    good = rows - bad
    d = dict(policy_mode=mode, rows=rows, bad_rows=bad, good=good, top1_rows=int(((flags & TOP1) != 0).sum()), value_rows=int(((flags & VROW) != 0).sum()),
             value_sign_rows=int(((flags & VSIGN) != 0).sum()), ce_sum=block_sum(ce), entropy_sum=block_sum(ent), se_sum=block_sum(se))
    d["policy_loss"] = d["ce_sum"] / good if good else nan
    d["policy_entropy"] = d["entropy_sum"] / good if good else nan
    d["policy_kl"] = (d["ce_sum"] - d["entropy_sum"]) / good if good else nan
    d["value_loss"] = d["se_sum"] / good if good else nan
    d["top1"] = d["top1_rows"] / good if good else nan
    d["value_sign"] = d["value_sign_rows"] / d["value_rows"] if d["value_rows"] else nan
    d["val_loss"] = (d["policy_kl"] if mode in (1, 3) else d["policy_loss"]) + d["value_loss"]
    return d


def bits(x):
    """the raw bits of a float64 (array or scalar): what the cases compare"""
    return np.asarray(x, np.float64).reshape(-1).view(np.uint64)


def mismatches(got, want):
    """number of fields / rows that differ in their bits between a result dict of the engine and the model's (per-row arrays included when both have them)"""
    bad = 0
    for k, w in want.items():
        g = got[k]
        if isinstance(w, float):
            bad += int(bits(g)[0] != bits(w)[0])
        elif isinstance(w, np.ndarray):
            bad += int((bits(g) != bits(w)).sum()) if w.dtype == np.float64 else int((np.asarray(g) != w).sum())
        else:
            bad += int(g != w)
    return bad

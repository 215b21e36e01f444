"""Policy surprise weighting of the training rows (include/gaz_engine.h, gaz_engine_set_sample_weighting), restated for the tests: what a
finished record must give, written from the rule alone and with the ORACLE's dlog and uniform variate (oracle.det_log, oracle.uniform, as
tests/det_cases.py calls them) — not with grok_alpha_zero_amd.det or self_play.sample_row_counts, which are among the things under test.
The rows themselves come from the existing record_to_samples with the cap ignored (every ply's row), repeated c_p times."""
import math

import numpy as np

P_PLAYOUT_CAP = 5                                  # det::P_PLAYOUT_CAP
EVENT0 = 0x40000000                                # ply p rounds with the variate of event EVENT0 + p


def surprise(oracle, pi, P):
    """step 1: max(0, sum over a ascending of pi[a] (log pi[a] - log P[a])) over pi[a] > 0 and P[a] > 0, float64, sequential"""
    s = 0.0
    for a in range(len(pi)):
        x, y = float(pi[a]), float(P[a])
        if x > 0.0 and y > 0.0:
            s += x * (oracle.det_log(x) - oracle.det_log(y))
    if math.isnan(s) or math.isinf(s):
        return 0.0
    return max(0.0, s)


def weights(oracle, rec, lam, fast_factor):
    """steps 1-4 -> dict: s [T], w [T] (NaN for a ply of kind 0: it keeps its one row and takes no part), E (bool [T]), n_full, mean, S"""
    kind = np.asarray(rec["move_kind"]).astype(int) & 3
    T = len(kind)
    s = np.array([0.0 if kind[p] == 0 else surprise(oracle, rec["policies"][p], rec["root_P"][p]) for p in range(T)])
    full = np.flatnonzero(kind == 1)
    n_full = len(full)
    acc = 0.0
    for p in full:
        acc += s[p]
    mean = acc / n_full if n_full else 0.0
    E = (kind == 1) | ((kind == 2) & (s > fast_factor * mean))
    S = 0.0
    for p in range(T):
        if E[p]:
            S += s[p]
    w0 = (kind == 1).astype(np.float64)
    if n_full == 0 or S == 0.0 or not math.isfinite(S):
        w = w0.copy()
    else:
        w = np.zeros(T)
        for p in range(T):
            if E[p]:
                w[p] = (1.0 - lam) * w0[p] + lam * n_full * s[p] / S
    w[kind == 0] = np.nan
    return dict(s=s, w=w, E=E, n_full=n_full, mean=mean, S=S, kind=kind)


def row_counts(oracle, rec, lam, fast_factor, seed):
    """step 5 -> (c [T] int64, the dict of weights())"""
    m = weights(oracle, rec, lam, fast_factor)
    c = np.zeros(len(m["w"]), np.int64)
    for p, w in enumerate(m["w"]):
        if m["kind"][p] == 0:
            c[p] = 1
            continue
        fl = math.floor(w)
        u = oracle.uniform(seed, int(rec["slot"]), int(rec["game_seq"]), 2, EVENT0 + p, P_PLAYOUT_CAP)
        c[p] = int(fl) + int(u < w - fl)
    return c, m


def every_row(game_class, rec):
    """the row of every ply as it is with the cap off: the existing record_to_samples on the record with its move_kind forced to 1"""
    from grok_alpha_zero_amd.self_play import record_to_samples
    forced = dict(rec)
    forced["move_kind"] = np.ones_like(np.asarray(rec["move_kind"]))
    b, p, v, T = record_to_samples(game_class, forced)
    assert b.shape[1] == p.shape[1] == v.shape[1] == T == len(rec["actions"])
    return b, p, v


def expected(oracle, game_class, rec, lam, fast_factor, seed):
    """-> dict: c, row_ply (uint8 [rows]), boards / policies [n_aug, rows, ...], values [n_aug, rows, 1], no_row (plies with c == 0) and the
    weights() dict as `m`"""
    c, m = row_counts(oracle, rec, lam, fast_factor, seed)
    plies = np.repeat(np.arange(len(c)), c)
    b, p, v = every_row(game_class, rec)
    return dict(c=c, row_ply=plies.astype(np.uint8), boards=b[:, plies], policies=p[:, plies], values=v[:, plies], no_row=int((c == 0).sum()), m=m)


def witnesses(c, m):
    """what a cap-on case must show, from the model alone"""
    kind, E = m["kind"], m["E"]
    return dict(fast_with_rows=bool(((kind == 2) & (c > 0)).any()), full_without_rows=bool(((kind == 1) & (c == 0)).any()),
                ply_with_two=bool((c >= 2).any()), ineligible_fast=bool(((kind == 2) & ~E).any()), rows_exceed_plies=bool(c.sum() > len(c)))

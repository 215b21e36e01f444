"""The cases of Muon in the fused optimizer step (optim.FusedOptimizer(muon=...); the "MUON" part of include/gaz_engine.h; csrc/muon.hpp; DESIGN.md
section 29) that the CPU suite runs on the emulation build (tests/test_muon_emu.py) and the -m gpu suite on the HIP build (tests/test_muon_gpu.py):
`lib_path` = the emulation library, or None for the product library.

What a step must give is computed by tests/muon_model.py from the arrays the case itself made.  Every comparison is on raw bits with 0 mismatches,
and every case asserts its witnesses from the model's values."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import muon_model as MM
import optim_model as M
from optim_cases import bits, same_bits
from selfplay_support import EMU_DIR, ROOT, refusal_message

CHUNK = M.CHUNK
# (shape, takes Adam although it has two dimensions).  One optimizer holds Adam and Muon tensors interleaved; odd-sized tensors come first, so the
# later ones start behind pads.  General path (smaller dimension >= 5): partial MFMA tiles in both dimensions, K no multiple of the MFMA's k or of
# the LDS stage, both orientations, more than one tile.  Thin path (smaller dimension <= 4): the conv kernels and the N x 1 Dense.
TENSORS = (
    ((7,), False),            # a bias
    ((5, 7), False),          # general: one partial tile, K = 7 odd
    ((1, 1, 2, 9), False),    # thin 1 x 18: a 1 x 1 conv
    ((3,), False),
    ((3, 3, 2, 3), False),    # thin 3 x 18: a 3 x 3 conv 2 -> 3
    ((17, 33), False),        # general: partial tiles, K = 33 one over the stage
    ((65, 33), False),        # general, transposed (33 x 65): two tiles along Q
    ((6, 5), True),           # two dimensions, excluded: Adam
    ((16, 48), False),
    ((64, 64), False),        # rows == cols: exactly one full tile, not transposed
    ((33, 130), False),       # three tiles along Q
    ((70, 257), False),       # K = 257 in the Gram product, K = 70 in the other two: 2 x 2 and 2 x 5 tiles, all edges partial
    ((3, 6147), False),       # thin: three chunks of columns with a tail
    ((130, 1), False),        # thin, transposed (1 x 130): the N x 1 Dense
    ((4, 9), False),          # thin at its limit
    ((33,), False),
)
SHAPES = [t[0] for t in TENSORS]
SIZES = [int(np.prod(s)) for s in SHAPES]
ADAM_2D = [k for k, t in enumerate(TENSORS) if t[1]]
IS_MUON = [len(s) >= 2 and not ex for s, ex in TENSORS]
STEPS_T = (1, 2, 3, 1000)
LR = 2e-3
# every switch in both positions, ns_steps 0, 1 and 5; the first is the reference's Gomoku configuration
COMBOS = [
    dict(kind=1, orthograd=True, grokfast=True, weight_decay=0.004, nesterov=True, ns_steps=5, adam_lr_ratio=1.0),
    dict(kind=0, orthograd=False, grokfast=False, weight_decay=0.0, nesterov=False, ns_steps=5, adam_lr_ratio=0.5),
    dict(kind=1, orthograd=False, grokfast=True, weight_decay=0.004, nesterov=True, ns_steps=1, adam_lr_ratio=0.5),
    dict(kind=0, orthograd=True, grokfast=False, weight_decay=0.0, nesterov=False, ns_steps=1, adam_lr_ratio=1.0),
    dict(kind=1, orthograd=True, grokfast=False, weight_decay=0.004, nesterov=False, ns_steps=0, adam_lr_ratio=0.5),
    dict(kind=0, orthograd=False, grokfast=True, weight_decay=0.0, nesterov=True, ns_steps=0, adam_lr_ratio=1.0),
]
MUON_KEYS = ("muon_beta", "nesterov", "muon_a", "muon_b", "muon_c", "ns_steps", "adam_lr_ratio")
BASE = dict(kind=1, beta_1=0.9, beta_2=0.995, epsilon=1e-8, weight_decay=0.0, orthograd=False, grokfast=False, alpha=0.99, lamb=2.0)


def split(kw):
    """a combination -> (FusedOptimizer's own keywords, the muon dict's)"""
    return dict(BASE, **{k: v for k, v in kw.items() if k not in MUON_KEYS}), {k: v for k, v in kw.items() if k in MUON_KEYS}


def make(shapes, lib_path, adam_2d=(), **kw):
    from grok_alpha_zero_amd.optim import FusedOptimizer
    okw, mkw = split(kw)
    return FusedOptimizer([int(np.prod(s)) for s in shapes], lib_path=lib_path, muon=dict(mkw, adam_tensors=list(adam_2d)), shapes=list(shapes), **okw)


def expected_launches(shapes, is_muon, kw):
    """the launches entry of gaz_optim_layout in Muon mode"""
    p = [min(s[0], int(np.prod(s[1:]))) for s, mu in zip(shapes, is_muon) if mu]
    base = 3 if kw.get("orthograd") else 1
    if not p:
        return base
    return base + 2 + kw.get("ns_steps", 5) * (2 + (1 if any(x > MM.THIN for x in p) else 0))


class ModelState:
    """the model's copy of an optimizer in Muon mode"""

    def __init__(self, shapes, is_muon, kw):
        okw, mkw = split(kw)
        self.shapes, self.is_muon, self.kw = list(shapes), list(is_muon), dict(okw, **dict(MM.DEFAULTS, **mkw))
        self.sizes = [int(np.prod(s)) for s in shapes]
        z = lambda: [np.zeros(n, np.float32) for n in self.sizes]      # noqa: E731
        self.w, self.m, self.v, self.e = z(), z(), z(), z()
        self.norms = np.zeros((len(shapes), 4))
        self.aux = [None] * len(shapes)

    def step(self, grads, lr, t):
        for k in range(len(self.sizes)):
            self.w[k], self.m[k], self.v[k], e, self.norms[k], self.aux[k] = MM.step_tensor(self.w[k], grads[k], self.m[k], self.v[k], self.e[k], lr, t, self.shapes[k],
                                                                                           self.is_muon[k], **self.kw)
            if self.kw["grokfast"]:
                self.e[k] = e


def compare(opt, model, what, grads_want=None):
    """every arena against the model (the velocity range of a Muon tensor holds u), the pads against zero, the norms, and through muon_debug X0, n,
    A, B and X of every Muon tensor"""
    offs, total = M.layout(model.sizes)
    assert list(opt.offsets) == offs and opt.total == total
    pad = np.ones(total, bool)
    for o, n in zip(offs, model.sizes):
        pad[o:o + n] = False
    arenas = [("params", model.w), ("momentum", model.m), ("velocity", model.v)] + ([("ema", model.e)] if model.kw["grokfast"] else [])
    if grads_want is not None:
        arenas.append(("grads", grads_want))
    for name, want in arenas:
        flat = opt.read(name)
        assert not bits(flat[pad]).any(), f"{what}: {name}: a pad element is not zero"
        for k, (o, n) in enumerate(zip(offs, model.sizes)):
            same_bits(flat[o:o + n], want[k], f"{what}: {name}[{k}] {model.shapes[k]}")
    same_bits(opt.norms(), model.norms if model.kw["orthograd"] else np.zeros_like(model.norms), f"{what}: norms")
    for k, mu in enumerate(model.is_muon):
        if not mu:
            continue
        d, a = opt.muon_debug(k), model.aux[k]
        for name in ("X0", "A", "B", "X"):
            same_bits(d[name], a[name], f"{what}: {name} of tensor {k} {model.shapes[k]}")
        same_bits(np.float32(d["n"]).reshape(1), np.float32(a["n"]).reshape(1), f"{what}: n of tensor {k}")


def check_sums_independently(model, what):
    """the float64 sums of the rule against math.fsum of the exact products, within the any-order bound (n - 1) 2^-53 sum |terms| of recursive
    summation (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2): the norm sum of every Muon tensor and every thin-path Gram sum of
    the last iteration -> the number of sums checked"""
    done = 0
    for k, mu in enumerate(model.is_muon):
        if not mu:
            continue
        a = model.aux[k]
        x0 = a["X0"].astype(np.float64).reshape(-1)
        todo = [(a["norm64"], x0 * x0)]
        if a["gram64"] is not None:
            X = a["Xprev"].astype(np.float64)
            todo += [(a["gram64"][i, j], X[i] * X[j]) for i in range(X.shape[0]) for j in range(i, X.shape[0])]
        for got, terms in todo:
            exact, bound = math.fsum(terms.tolist()), (terms.size - 1) * 2.0 ** -53 * math.fsum(np.abs(terms).tolist())
            assert abs(float(got) - exact) <= bound, f"{what}: tensor {k}: {got!r} against {exact!r}, bound {bound!r}"
            done += 1
    return done


# ------------------------------------------------------------------------------------------------ 1. bit equality over the tensor list
def bits_case(lib_path, combos=None, seed=21):
    """one optimizer over TENSORS per combination; four steps at t = 1, 2, 3, 1000 with fresh random grads -> the number of (combination, step) pairs"""
    done = 0
    for kw in COMBOS if combos is None else combos:
        rng = np.random.default_rng(seed + COMBOS.index(kw))
        opt, model = make(SHAPES, lib_path, adam_2d=ADAM_2D, **kw), ModelState(SHAPES, IS_MUON, kw)
        assert opt.muon_tensors == [k for k, mu in enumerate(IS_MUON) if mu]
        assert opt.launches_per_step == expected_launches(SHAPES, IS_MUON, kw), (opt.launches_per_step, kw)
        for k, n in enumerate(SIZES):
            model.w[k] = (rng.standard_normal(n) * 0.1).astype(np.float32)
            opt.set("params", k, model.w[k])
        for t in STEPS_T:
            grads = [(rng.standard_normal(n) * 10.0 ** rng.integers(-4, 1)).astype(np.float32) for n in SIZES]
            for k in range(len(SIZES)):
                opt.set("grads", k, grads[k])
            opt.step(LR, t)
            model.step(grads, LR, t)
            what = f"{kw} t {t}"
            compare(opt, model, what, grads_want=[np.zeros(n, np.float32) for n in SIZES])
            for k, mu in enumerate(IS_MUON):                                 # the matrices really iterated: X is no multiple of X0
                if mu and kw["ns_steps"]:
                    assert model.aux[k]["A"].any() and model.aux[k]["transposed"] == (SHAPES[k][0] > SIZES[k] // SHAPES[k][0])
            assert check_sums_independently(model, what) >= sum(IS_MUON)
            done += 1
        opt.close()
    return done


# ------------------------------------------------------------------------------------------------ 2. the witnesses
WITNESSES = ("zero", "rank_1", "tie", "square")


def witness_case(lib_path, seed=4):
    """a matrix per edge under momentum 0 without Nesterov, so that u is the gradient itself -> the witnesses seen"""
    shapes = [(6, 9), (8, 12), (5, 6), (8, 8), (3, 7)]                      # zero, rank 1, ties, rows == cols, and a thin zero matrix
    kw = dict(kind=1, muon_beta=0.0, nesterov=False, ns_steps=5)
    rng = np.random.default_rng(seed)
    opt, model = make(shapes, lib_path, **kw), ModelState(shapes, [True] * len(shapes), kw)
    g = [rng.standard_normal(int(np.prod(s))).astype(np.float32) for s in shapes]
    g[0][:] = 0
    g[4][:] = 0
    g[1] = np.outer([1, -1, 1, 1, 0, 0, 0, 0], [1, 1, -1, 0, 0, 1, 0, 0, 0, 0, 0, 0]).astype(np.float32).reshape(-1)      # sixteen +-1: exact in bf16, n = 4
    g[2][0], g[2][1], g[2][2] = np.float32(1.0 + 2.0 ** -8), np.float32(1.0 + 3 * 2.0 ** -8), np.float32(-(1.0 + 2.0 ** -8))      # exact ties between two bf16 values
    for k in range(len(shapes)):
        model.w[k] = (rng.standard_normal(model.sizes[k]) * 0.1).astype(np.float32)
        opt.set("params", k, model.w[k]); opt.set("grads", k, g[k])
    w0 = [w.copy() for w in model.w]
    opt.step(LR, 1, zero_grads=False)
    model.step(g, LR, 1)
    compare(opt, model, "witnesses", grads_want=g)
    a, seen = model.aux, set()
    for k in range(len(shapes)):
        same_bits(a[k]["u"], g[k], "momentum 0 without Nesterov: u is the gradient")
    for k in (0, 4):
        assert a[k]["n"] == 0 and not a[k]["X"].any() and not a[k]["A"].any()
        same_bits(model.w[k], w0[k], "a zero gradient leaves w")
    seen.add("zero")
    sv0, sv = np.linalg.svd(a[1]["X0"].astype(np.float64), compute_uv=False), np.linalg.svd(a[1]["X"].astype(np.float64), compute_uv=False)
    assert a[1]["n"] == 4 and sv0[1] < 1e-12 * sv0[0]                          # exactly rank 1, and X = X0 / 4 is exact too
    assert 0.5 < sv[0] < 1.5 and sv[1] < 1e-12                                 # it stays rank 1: one singular value near 1
    seen.add("rank_1")
    low = g[2][:3].view(np.uint32) & 0xFFFF
    assert (low == 0x8000).all()                                              # the three are exact ties
    assert a[2]["X0"].reshape(-1)[:3].tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0]   # to even: down, up, down
    seen.add("tie")
    assert a[3]["X"].shape == (8, 8) and not a[3]["transposed"] and a[3]["A"].shape == (8, 8)
    seen.add("square")
    opt.close()
    assert seen == set(WITNESSES)
    return sorted(seen)


# ------------------------------------------------------------------------------------------------ 3. state() / load_state()
def round_trip_case(lib_path, seed=8):
    shapes = [(3,), (9, 5), (3, 3, 2, 2), (2, 7)]
    kw = dict(kind=1, orthograd=True, grokfast=True, weight_decay=0.004, ns_steps=5)
    rng = np.random.default_rng(seed)
    a, model = make(shapes, lib_path, adam_2d=[3], **kw), ModelState(shapes, [False, True, True, False], kw)
    for k, n in enumerate(model.sizes):
        model.w[k] = (rng.standard_normal(n) * 0.1).astype(np.float32)
        a.set("params", k, model.w[k])
    grads = [[rng.standard_normal(n).astype(np.float32) for n in model.sizes] for _ in range(3)]
    for s in range(2):
        for k in range(len(shapes)):
            a.set("grads", k, grads[s][k])
        a.step(LR); model.step(grads[s], LR, s + 1)
    b = make(shapes, lib_path, adam_2d=[3], **kw)
    b.load_state(a.state())
    assert b.steps == 2
    for o in (a, b):
        for k in range(len(shapes)):
            o.set("grads", k, grads[2][k])
        o.step(LR)
    model.step(grads[2], LR, 3)
    compare(a, model, "the first optimizer, step 3"); compare(b, model, "the one loaded from state(), step 3")
    a.close(); b.close()
    return 3


# ------------------------------------------------------------------------------------------------ 4. refusals
def refusal_case(lib_path):
    """every refusal by its text -> {what: message}"""
    from grok_alpha_zero_amd import optim as P
    from grok_alpha_zero_amd.engine import EngineError
    shapes = [(3,), (4, 5)]
    out = {}

    def raw(opt, **over):
        """gaz_muon_set with a hand-made config -> the refusal's text"""
        rows, cols, scale = np.array([0, 4], np.int32), np.array([0, 5], np.int32), np.array([0, 0.2], np.float32)
        kw = dict(struct_size=C.sizeof(P.MuonConfig), n_tensors=2, rows=rows.ctypes.data, cols=cols.ctypes.data, scale=scale.ctypes.data, muon_beta=0.95, nesterov=1,
                  ns_steps=5, muon_a=3.4445, muon_b=-4.775, muon_c=2.0315, adam_lr_ratio=1.0)
        if "rows_cols" in over:
            rows[1], cols[1] = over.pop("rows_cols")
        cfg = P.MuonConfig(**dict(kw, **over))
        P.bind_muon(opt.L)
        assert opt.L.gaz_muon_set(opt.h, C.byref(cfg)) != 0, f"{over} was accepted"
        return opt.L.gaz_optim_last_error(opt.h).decode()

    plain = P.FusedOptimizer([3, 20], lib_path=lib_path)
    out["rows_cols"] = raw(plain, rows_cols=(4, 6))
    assert "tensor 1: rows * cols = 4 * 6 is not its size 20" in out["rows_cols"]
    for ns in (-1, 17):
        out[f"ns_steps={ns}"] = raw(plain, ns_steps=ns)
        assert f"ns_steps must be in 0 .. 16, not {ns}" in out[f"ns_steps={ns}"]
    for name in ("muon_a", "muon_b", "muon_c"):
        out[name] = raw(plain, **{name: float("nan") if name != "muon_b" else float("inf")})
        assert "muon_a, muon_b and muon_c must be finite" in out[name]
    for beta in (1.0, -0.5, float("nan")):
        out[f"muon_beta={beta}"] = raw(plain, muon_beta=beta)
        assert "muon_beta must be in [0, 1)" in out[f"muon_beta={beta}"]
    out["struct_size"] = raw(plain, struct_size=C.sizeof(P.MuonConfig) - 8)
    assert "struct_size" in out["struct_size"] and str(C.sizeof(P.MuonConfig)) in out["struct_size"]
    out["n_tensors"] = raw(plain, n_tensors=3)
    assert "n_tensors is 3, the optimizer has 2 tensors" in out["n_tensors"]
    out["not_muon"] = refusal_message(lambda: plain.muon_debug(1), "muon_debug of a plain optimizer")
    assert "not in Muon mode" in out["not_muon"]
    assert plain.launches_per_step == 1
    plain.step(LR)
    out["after_step"] = raw(plain)
    assert "before the first step" in out["after_step"]
    plain.close()
    opt = make(shapes, lib_path)
    out["second"] = raw(opt)
    assert "in Muon mode already" in out["second"]
    out["adam_tensor"] = refusal_message(lambda: opt.muon_debug(0), "muon_debug of an Adam tensor")
    assert "tensor 0 is an Adam tensor" in out["adam_tensor"]
    buf = np.zeros(20, np.float32)
    assert opt.L.gaz_muon_read(opt.h, 1, 5, buf.ctypes.data) != 0
    out["what"] = opt.L.gaz_optim_last_error(opt.h).decode()
    assert "what must be 0 (X0), 1 (n), 2 (X), 3 (A) or 4 (B), not 5" in out["what"]
    assert opt.L.gaz_muon_read(opt.h, 2, 0, buf.ctypes.data) != 0 and "tensor 2 of 2" in opt.L.gaz_optim_last_error(opt.h).decode()
    opt.close()
    for key, call, text in (("shapes", lambda: P.FusedOptimizer([20], lib_path=lib_path, muon={}, shapes=[(4, 6)]), "shapes must give the shape of every tensor"),
                            ("keys", lambda: P.FusedOptimizer([20], lib_path=lib_path, muon=dict(caution=True), shapes=[(4, 5)]), "unknown keys ['caution']")):
        try:
            call()
        except ValueError as e:
            out[key] = str(e)
        assert text in out[key]
    return out


# ------------------------------------------------------------------------------------------------ 5. the sanitizer driver
def build_driver():
    """tests/emu/muon_main.cpp with the engine's host code and the one-lane build of its device code as ONE program under the address and
    undefined-behaviour sanitizers, the runtimes linked statically: run directly, on the CPU, never loaded into Python"""
    csrc, out = os.path.join(ROOT, "grok_alpha_zero_amd", "csrc"), os.path.join(EMU_DIR, "muon_asan")
    srcs = [os.path.join(csrc, "engine.hip"), os.path.join(EMU_DIR, "emu_stubs.cpp"), os.path.join(EMU_DIR, "muon_main.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")] + [os.path.join(ROOT, "include", "gaz_engine.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DGAZ_HOST_EMU", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-x", "c++"] + srcs + ["-o", out])
    return out


def run_driver(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout + r.stderr

"""The cases of the optimizer step (optim.FusedOptimizer; the "OPTIMIZER" section of include/gaz_engine.h) that the CPU suite
runs on the emulation build (tests/test_optim_emu.py) and the -m gpu suite on the HIP build (tests/test_optim_gpu.py): `lib_path` = the emulation
library, or None for the product library.

What a step must give is computed by tests/optim_model.py from the arrays the case itself made.  Every comparison is on raw bits with 0 mismatches
(NaN equals NaN), and every case asserts its witnesses from the model's values: that the tensors it stepped really held the edge it is about."""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np

import optim_model as M
from selfplay_support import EMU_DIR, ROOT, refusal_message

CHUNK = M.CHUNK
# odd sizes in front of vector-aligned ones: a tensor behind an odd one starts after pad elements.  Tails of 1 .. 3, partial wavefronts, one
# chunk - 1 / exactly / + 1, three chunks + 5 (the cross-chunk stage with a tail)
SIZES = (1, 3, 5, 7, 63, 65, 255, 257, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 5, 4, 64, 256, CHUNK)
STEPS_T = (1, 2, 3, 1000)
LR = 2e-3
COMBOS = [dict(kind=k, orthograd=o, grokfast=g, weight_decay=wd) for k, o, g, wd in itertools.product((0, 1), (False, True), (False, True), (0.0, 0.004))]


def make(sizes, lib_path, **kw):
    from grok_alpha_zero_amd.optim import FusedOptimizer
    return FusedOptimizer(sizes, lib_path=lib_path, **dict(dict(lamb=2.0), **kw))


def model_kw(kw):
    return dict(dict(kind=1, beta_1=0.9, beta_2=0.999, epsilon=1e-7, weight_decay=0.0, orthograd=False, grokfast=False, alpha=0.99, lamb=2.0), **kw)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(got, want, what):
    """raw bits, NaN equal to NaN"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = (bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} differ, first at {int(np.argmax(bad))}: {got.reshape(-1)[np.argmax(bad)]!r} != {want.reshape(-1)[np.argmax(bad)]!r}"


class ModelState:
    """the model's copy of an optimizer: per-tensor arrays, stepped by optim_model.step_tensor"""

    def __init__(self, sizes, kw):
        self.sizes, self.kw = list(sizes), model_kw(kw)
        z = lambda: [np.zeros(n, np.float32) for n in sizes]      # noqa: E731
        self.w, self.m, self.v, self.e = z(), z(), z(), z()
        self.norms = np.zeros((len(sizes), 4))
        self.aux = [None] * len(sizes)

    def step(self, grads, lr, t):
        for k in range(len(self.sizes)):
            self.w[k], self.m[k], self.v[k], e, self.norms[k], self.aux[k] = M.step_tensor(self.w[k], grads[k], self.m[k], self.v[k], self.e[k], lr, t, **self.kw)
            if self.kw["grokfast"]:
                self.e[k] = e


def compare(opt, model, what, grads_want=None):
    """every arena of the optimizer against the model, the pads against zero, the norms"""
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
            same_bits(flat[o:o + n], want[k], f"{what}: {name}[{k}] ({n} elements)")
    same_bits(opt.norms(), model.norms if model.kw["orthograd"] else np.zeros_like(model.norms), f"{what}: norms")


def check_sums_independently(model, grads, what):
    """every dot product of the model's last step against math.fsum of the exact products: the any-order bound (n - 1) 2^-53 sum |terms| of
    recursive summation in float64 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2) — derived, not measured"""
    for k, n in enumerate(model.sizes):
        aux = model.aux[k]
        w1, go, g = aux["w1"].astype(np.float64), aux["go"].astype(np.float64), grads[k].astype(np.float64)
        for j, terms in enumerate((w1 * g, w1 * w1, g * g, go * go)):
            exact, bound = math.fsum(terms.tolist()), (n - 1) * 2.0 ** -53 * math.fsum(np.abs(terms).tolist())
            assert abs(float(model.norms[k, j]) - exact) <= bound, f"{what}: tensor {k} sum {j}: {model.norms[k, j]!r} against {exact!r}, bound {bound!r}"


# ------------------------------------------------------------------------------------------------ 1. bit equality over the size list
def bits_case(lib_path, combos=None, seed=11):
    """one optimizer over SIZES per combination; four steps at t = 1, 2, 3, 1000 with fresh random grads -> the number of (combination, step) pairs"""
    done = 0
    for ci, kw in enumerate(COMBOS if combos is None else combos):
        rng = np.random.default_rng(seed + ci)
        opt, model = make(SIZES, lib_path, **kw), ModelState(SIZES, kw)
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
            if kw["orthograd"]:
                check_sums_independently(model, grads, what)
                assert (model.norms[:, 1:3] > 0).all(), what
            done += 1
        assert opt.steps == 1000 and opt.launches_per_step == (3 if kw["orthograd"] else 1)
        nc = sum((n + CHUNK - 1) // CHUNK for n in SIZES)
        assert (opt.n_chunks, opt.chunk) == (nc, CHUNK)
        opt.close()
    return done


# ------------------------------------------------------------------------------------------------ 2. the witnesses
WITNESSES = ("w_zero", "g_zero", "g_parallel", "g2_subnormal", "g2_zero", "small_velocity")


def witness_case(lib_path, seed=5):
    """a tensor per edge, each asserted from the model's values, under the full chain and under plain Adam -> the witnesses seen"""
    n = 37
    sizes = [n] * len(WITNESSES)
    seen = set()
    for kw in (dict(kind=1, orthograd=True, grokfast=True, weight_decay=0.004), dict(kind=0)):
        rng = np.random.default_rng(seed)
        opt, model = make(sizes, lib_path, **kw), ModelState(sizes, kw)
        w = [(rng.standard_normal(n) * 0.1).astype(np.float32) for _ in sizes]
        g = [rng.standard_normal(n).astype(np.float32) for _ in sizes]
        ix = {name: i for i, name in enumerate(WITNESSES)}
        w[ix["w_zero"]][:] = 0                                         # the zero-initialised last Dense layers
        g[ix["g_zero"]][:] = 0
        g[ix["g_parallel"]] = w[ix["g_parallel"]] * np.float32(0.5)    # go is rounding residue only
        g[ix["g2_subnormal"]][:] = 1e-20                               # g * g = 1e-40: an f32 subnormal
        g[ix["g2_zero"]][:] = 1e-25                                    # g * g = 0
        g[ix["small_velocity"]][:] = 1e-12
        for k in range(len(sizes)):
            model.w[k] = w[k]
            opt.set("params", k, w[k]); opt.set("grads", k, g[k])
        model.v[ix["small_velocity"]][:] = 1e-20                       # sqrt(v / c2) = 1e-10 is below eps = 1e-7
        opt.set("velocity", ix["small_velocity"], model.v[ix["small_velocity"]])
        for t in (1, 2):
            opt.step(LR, t, zero_grads=False)
            model.step(g, LR, t)
            compare(opt, model, f"witnesses {kw} t {t}", grads_want=g)
            ortho = bool(kw.get("orthograd"))
            if t == 1:
                a = model.aux
                if ortho:
                    assert model.norms[ix["w_zero"], 0] == 0 and model.norms[ix["w_zero"], 1] == 0 and np.isfinite(model.w[ix["w_zero"]]).all()
                    same_bits(a[ix["w_zero"]]["go"], g[ix["w_zero"]], "w = 0: go is g")
                    assert model.norms[ix["g_zero"], 2] == 0 and model.norms[ix["g_zero"], 3] == 0
                    assert 0 <= model.norms[ix["g_parallel"], 3] < 1e-10 * model.norms[ix["g_parallel"], 2]
                    seen.update(("w_zero", "g_parallel"))
                if not kw.get("grokfast") and not kw.get("weight_decay"):
                    same_bits(model.w[ix["g_zero"]], w[ix["g_zero"]], "g = 0 and no decay: w stays")
                assert not model.m[ix["g_zero"]].any() and not model.v[ix["g_zero"]].any()
                seen.add("g_zero")
                if not ortho and not kw.get("grokfast"):
                    gg = a[ix["g2_subnormal"]]["gg"]
                    assert (gg > 0).all() and (gg < np.float32(1.1754944e-38)).all()
                    assert not a[ix["g2_zero"]]["gg"].any() and not model.v[ix["g2_zero"]].any() and model.m[ix["g2_zero"]].all()
                    assert (a[ix["small_velocity"]]["root"] < np.float32(1e-7)).all() and (a[ix["small_velocity"]]["root"] > 0).all()
                    seen.update(("g2_subnormal", "g2_zero", "small_velocity"))
        opt.close()
    assert seen == set(WITNESSES), sorted(set(WITNESSES) - seen)
    return sorted(seen)


# ------------------------------------------------------------------------------------------------ 3. accumulation, zero_grads, the views
def accumulation_case(lib_path, seed=3):
    """two backward-style adds into the grads views and one step == one step on the summed grads; zero_grads=False leaves them in place"""
    sizes = (5, 64, CHUNK + 1)
    kw = dict(kind=1, orthograd=True, grokfast=True, weight_decay=0.004)
    rng = np.random.default_rng(seed)
    w = [(rng.standard_normal(n) * 0.1).astype(np.float32) for n in sizes]
    g1 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    g2 = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    a, b = make(sizes, lib_path, **kw), make(sizes, lib_path, **kw)
    for k in range(len(sizes)):
        a.set("params", k, w[k]); b.set("params", k, w[k])
        a.set("grads", k, g1[k] + g2[k])
    views = b.grads
    for k in range(len(sizes)):
        if b.host_memory:
            views[k] += g1[k]; views[k] += g2[k]
        else:
            import torch
            views[k] += torch.from_numpy(g1[k]).to(views[k].device); views[k] += torch.from_numpy(g2[k]).to(views[k].device)
            torch.cuda.synchronize()
    a.step(LR); b.step(LR, zero_grads=False)
    for name in ("params", "momentum", "velocity", "ema"):
        same_bits(b.read(name), a.read(name), f"accumulation: {name}")
    assert not bits(a.read("grads")).any()
    for k in range(len(sizes)):
        same_bits(b.get("grads", k), g1[k] + g2[k], "zero_grads=False leaves the grads")
    pv = b.params
    for k in range(len(sizes)):                                           # the params views show the stepped values
        got = np.array(pv[k]) if b.host_memory else pv[k].cpu().numpy()
        same_bits(got, b.get("params", k), "the params view")
    assert (a.steps, b.steps) == (1, 1)
    del views, pv
    a.close(); b.close()
    return len(sizes)


# ------------------------------------------------------------------------------------------------ 4. state() / load_state()
def round_trip_case(lib_path, seed=9):
    sizes = (3, 257, CHUNK + 1)
    kw = dict(kind=0, orthograd=True, grokfast=True, weight_decay=0.004)
    rng = np.random.default_rng(seed)
    a, model = make(sizes, lib_path, **kw), ModelState(sizes, kw)
    for k, n in enumerate(sizes):
        model.w[k] = (rng.standard_normal(n) * 0.1).astype(np.float32)
        a.set("params", k, model.w[k])
    grads = [[rng.standard_normal(n).astype(np.float32) for n in sizes] for _ in range(3)]
    for s in range(2):
        for k in range(len(sizes)):
            a.set("grads", k, grads[s][k])
        a.step(LR); model.step(grads[s], LR, s + 1)
    st = a.state()
    b = make(sizes, lib_path, **kw)
    b.load_state(st)
    assert b.steps == 2
    for o in (a, b):
        for k in range(len(sizes)):
            o.set("grads", k, grads[2][k])
        o.step(LR)
    model.step(grads[2], LR, 3)
    compare(a, model, "the first optimizer, step 3"); compare(b, model, "the one loaded from state(), step 3")
    a.close(); b.close()
    return 3


# ------------------------------------------------------------------------------------------------ 5. refusals
def refusal_case(lib_path):
    """every refusal by its text -> {what: message}"""
    from grok_alpha_zero_amd import optim as P
    from grok_alpha_zero_amd.engine import load_library
    out = {}
    out["n_tensors"] = refusal_message(lambda: make([], lib_path), "n_tensors 0 was accepted")
    assert "n_tensors must be at least 1" in out["n_tensors"]
    out["size"] = refusal_message(lambda: make([4, 0, 3], lib_path), "a size of 0 was accepted")
    assert "sizes[1] must be at least 1, not 0" in out["size"]
    assert "sizes[0] must be at least 1, not -2" in refusal_message(lambda: make([-2], lib_path), "a negative size was accepted")
    out["kind"] = refusal_message(lambda: make([4], lib_path, kind=2), "kind 2 was accepted")
    assert "kind must be 0 (Adam) or 1 (Nadam), not 2" in out["kind"]
    for name, val in (("beta_1", 1.0), ("beta_2", -0.1), ("beta_1", float("nan"))):
        out[f"{name}={val}"] = refusal_message(lambda: make([4], lib_path, **{name: val}), f"{name} = {val} was accepted")
        assert f"{name} must be in [0, 1)" in out[f"{name}={val}"]
    L = P.bind(load_library(lib_path))
    sizes = np.array([4], np.int64)
    cfg = P.OptimConfig(struct_size=C.sizeof(P.OptimConfig) - 8, n_tensors=1, kind=1, sizes=sizes.ctypes.data, beta_1=0.9, beta_2=0.999, epsilon=1e-7)
    h = C.c_void_p()
    assert L.gaz_optim_create(C.byref(cfg), C.byref(h)) != 0 and not h.value
    out["struct_size"] = L.gaz_optim_last_error(None).decode()
    assert "struct_size" in out["struct_size"] and str(C.sizeof(P.OptimConfig)) in out["struct_size"]
    opt = make([5, 3], lib_path)
    assert opt.total == 12
    out["t"] = refusal_message(lambda: opt.step(LR, 0), "t = 0 was accepted")
    assert "t must be at least 1, not 0" in out["t"]
    for lr in (float("inf"), float("nan")):
        out[f"lr={lr}"] = refusal_message(lambda: opt.step(lr, 1), f"lr = {lr} was accepted")
        assert "lr must be finite" in out[f"lr={lr}"]
    out["read"] = refusal_message(lambda: opt.read("params", 8, 5), "a read past the arena was accepted")
    assert "elements 8 .. 13 of an arena of 12" in out["read"]
    out["write"] = refusal_message(lambda: opt.write("grads", np.zeros(13, np.float32)), "a write past the arena was accepted")
    out["ema"] = refusal_message(lambda: opt.read("ema"), "the ema arena of an optimizer without grokfast was read")
    assert "no ema arena" in out["ema"]
    out["arena"] = refusal_message(lambda: opt.read(5), "arena 5 was read")
    assert opt.steps == 0 and not bits(opt.read("params")).any()
    opt.write("params", np.ones(12, np.float32))                             # a write over pads leaves them zero
    assert opt.read("params").tolist() == [1] * 5 + [0] * 3 + [1] * 3 + [0]
    opt.close()
    return out


# ------------------------------------------------------------------------------------------------ 6. the sanitizer driver
def build_driver():
    """tests/emu/optim_main.cpp with the engine's host code and the one-lane build of its device code as ONE program under the address and
    undefined-behaviour sanitizers, the runtimes linked statically: run directly, on the CPU, never loaded into Python"""
    csrc, out = os.path.join(ROOT, "grok_alpha_zero_amd", "csrc"), os.path.join(EMU_DIR, "optim_asan")
    srcs = [os.path.join(csrc, "engine.hip"), os.path.join(EMU_DIR, "emu_stubs.cpp"), os.path.join(EMU_DIR, "optim_main.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")] + [os.path.join(ROOT, "include", "gaz_engine.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DGAZ_HOST_EMU", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-x", "c++"] + srcs + ["-o", out])
    return out


def run_driver(driver):
    r = subprocess.run([driver], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout + r.stderr

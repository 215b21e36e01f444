"""CPU suite: the fused optimizer step (optim.FusedOptimizer; the "OPTIMIZER" section of include/gaz_engine.h; csrc/optim.hpp) on the one-lane
emulation build — the cases of tests/optim_cases.py against tests/optim_model.py — the ctypes mirror of gaz_optim_config against the header, and
the stand-alone sanitizer driver (tests/emu/optim_main.cpp).  Raw bits everywhere: no tolerance."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import optim_cases as cases
import optim_model as M
from conftest import ROOT
from selfplay_support import emu_lib  # noqa: F401


# ------------------------------------------------------------------------------------------------ 0. the model alone
def test_the_models_sum_order_against_fsum():
    """the documented order is a summation like any other: within the any-order bound of the exact sum, and exact where every partial sum is"""
    rng = np.random.default_rng(1)
    for n in (1, 3, 4, 5, 1023, 1024, 1025, cases.CHUNK - 1, cases.CHUNK, cases.CHUNK + 1, 3 * cases.CHUNK + 5):
        a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
        terms = a.astype(np.float64) * b.astype(np.float64)
        assert abs(M.dot(a, b) - math.fsum(terms.tolist())) <= (n - 1) * 2.0 ** -53 * math.fsum(np.abs(terms).tolist())
        ones = np.ones(n, np.float32)
        assert M.dot(ones, ones) == n
    assert M.layout((1, 3, 4, 5)) == ([0, 4, 8, 12], 20)


# ------------------------------------------------------------------------------------------------ 1. the step
@pytest.mark.parametrize("kind", [0, 1])
def test_every_arena_equals_the_model_in_every_bit(emu_lib, kind):
    """Adam / Nadam x Orthograd x Grokfast x decay over the size list, four steps at t = 1, 2, 3, 1000: params, momentum, velocity, ema, the zeroed
    grads, the pads and read_norms; the sums also against math.fsum"""
    combos = [c for c in cases.COMBOS if c["kind"] == kind]
    assert cases.bits_case(emu_lib, combos) == 8 * len(cases.STEPS_T)


def test_the_witnesses(emu_lib):
    assert cases.witness_case(emu_lib) == sorted(cases.WITNESSES)


def test_accumulation_and_zero_grads(emu_lib):
    assert cases.accumulation_case(emu_lib) == 3


def test_state_round_trip(emu_lib):
    assert cases.round_trip_case(emu_lib) == 3


def test_every_refusal_by_its_text(emu_lib):
    msgs = cases.refusal_case(emu_lib)
    assert len(set(msgs.values())) >= 10


def test_a_library_without_the_feature():
    from grok_alpha_zero_amd import optim as P
    from grok_alpha_zero_amd.engine import EngineError
    with pytest.raises(EngineError, match="no gaz_optim_create: rebuild it"):
        P.bind(types.SimpleNamespace())


def test_attach_points_a_torch_module_at_the_arenas(emu_lib):
    """.data and .grad of every parameter are views of the arenas: backward accumulates into the grads arena, a step moves the module"""
    import torch
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(), torch.nn.Linear(7, 3))
    before = [p.detach().clone().numpy().reshape(-1) for p in net.parameters()]
    sizes = [p.numel() for p in net.parameters()]
    opt = cases.make(sizes, emu_lib, kind=1, orthograd=True, grokfast=True, weight_decay=0.004)
    opt.attach(net)
    model = cases.ModelState(sizes, dict(kind=1, orthograd=True, grokfast=True, weight_decay=0.004))
    for k in range(len(sizes)):
        cases.same_bits(opt.get("params", k), before[k], "attach keeps the values")
        model.w[k] = before[k]
    x = torch.randn(4, 5)
    for t in (1, 2, 3):
        for _ in range(2):                                      # two backward passes accumulate
            net(x).square().sum().backward()
        grads = [opt.get("grads", k) for k in range(len(sizes))]
        for p, g in zip(net.parameters(), grads):
            cases.same_bits(p.grad.detach().numpy().reshape(-1), g, "p.grad is the arena")
            assert g.any()
        opt.step(cases.LR)
        model.step(grads, cases.LR, t)
        cases.compare(opt, model, f"attached module, step {t}", grads_want=[np.zeros(n, np.float32) for n in sizes])
        for k, p in enumerate(net.parameters()):
            cases.same_bits(p.detach().numpy().reshape(-1), model.w[k], "the module sees the step")
            assert not p.grad.numpy().any()
    with pytest.raises(ValueError, match="attach"):
        opt.attach(torch.nn.Linear(2, 2))


# ------------------------------------------------------------------------------------------------ 2. ABI
def test_ctypes_mirror_of_the_config_matches_the_header(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_stub
    from grok_alpha_zero_amd.optim import OptimConfig
    hdr = abi_stub.parse_structs()["gaz_optim_config"]
    want = [(f, getattr(C, abi_stub.CTYPES[t]) if t in abi_stub.CTYPES else C.c_void_p) for f, t, n in hdr]
    assert all(n == 0 for _, _, n in hdr) and list(OptimConfig._fields_) == want
    fields = [f for f, _ in OptimConfig._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gaz_engine.h"\nint main(void){printf("%zu\\n", sizeof(gaz_optim_config));'
                   + "".join(f'printf("%zu\\n", offsetof(gaz_optim_config, {f}));' for f in fields) + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).decode().split()]
    assert out[0] == C.sizeof(OptimConfig) and out[1:] == [getattr(OptimConfig, f).offset for f in fields]
    exec(abi_stub.stub_text(), ns := {"C": C})
    assert C.sizeof(ns["OptimCfg"]) == C.sizeof(OptimConfig)
    m = re.search(r"#define\s+GAZ_ENGINE_ABI_VERSION\s+(\d+)", open(os.path.join(ROOT, "include", "gaz_engine.h")).read())
    assert int(m.group(1)) == 10


def test_libraries_export_the_optim_symbols(emu_lib):
    from grok_alpha_zero_amd import engine as E
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaz_engine.h")).read(), flags=re.S)
    want = set(re.findall(r"\b(gaz_optim_\w+)\s*\(", hdr))
    assert want == {"gaz_optim_" + f for f in ("config_size", "create", "destroy", "last_error", "layout", "ptrs", "read", "write", "step", "step_timed", "read_norms",
                                               "synchronize")}
    for lib in [emu_lib] + ([E.DEFAULT_LIB] if os.path.exists(E.DEFAULT_LIB) else []):
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
        got = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert want <= got, (lib, sorted(want - got))


# ------------------------------------------------------------------------------------------------ 3. the sanitizer driver
def test_the_step_at_the_buffer_limits_under_the_sanitizers():
    """the optimizer's host code and the one-lane build of its kernels, linked into a program of their own with -fsanitize=address,undefined
    -fno-sanitize-recover=all, driven through the C ABI with caller buffers of exactly the documented sizes"""
    rc, out = cases.run_driver(cases.build_driver())
    assert rc == 0, f"exit status {rc}\n{out[-3000:]}"

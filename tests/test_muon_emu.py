"""CPU suite: Muon in the fused optimizer step (optim.FusedOptimizer(muon=...); the "MUON" part of include/gaz_engine.h; csrc/muon.hpp) on the one-lane
emulation build — the cases of tests/muon_cases.py against tests/muon_model.py — the model itself against muon.py's iteration in float64, the
ctypes mirror of gaz_muon_config against the header, and the stand-alone sanitizer driver (tests/emu/muon_main.cpp).  Raw bits everywhere the
library is compared: no tolerance."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import muon_cases as cases
import muon_model as MM
from conftest import ROOT
from selfplay_support import emu_lib  # noqa: F401

COEFFS = (3.4445, -4.7750, 2.0315)
# The relative Frobenius gap between the rule's X (bf16 operands, bf16 coefficients) and muon.py's polynomial iteration in float64 with nothing
# rounded, five iterations, standard normal u, seeds 100 .. 104, largest of the five per shape of muon_cases.TENSORS — measured on the model:
#   5x7 0.068   1x18 0.040   3x18 0.188   17x33 0.066   65x33 0.064   16x48 0.054   64x64 0.057   33x130 0.077   70x257 0.062   3x6147 0.259
#   130x1 0.041   4x9 0.081
# The gap is bf16's own rounding (2^-9 relative per operand and per coefficient) carried through a polynomial that does not contract near its
# fixed region; it is largest where the singular values are nearly equal (the thin matrices).  The bound is twice the largest measured value; a
# transposed or mis-scaled product misses by order 1.
GAP_BOUND = 2 * 0.2592


# ------------------------------------------------------------------------------------------------ 0. the model alone
def test_the_model_against_the_iteration_in_float64():
    worst = {}
    for shape, is_muon in zip(cases.SHAPES, cases.IS_MUON):
        if not is_muon:
            continue
        rows, cols = shape[0], int(np.prod(shape[1:]))
        for seed in range(100, 105):
            u = np.random.default_rng(seed).standard_normal(rows * cols).astype(np.float32)
            X, _ = MM.newton_schulz(u, rows, cols, *COEFFS, 5)
            E = MM.ns_exact(u, rows, cols, *COEFFS, 5)
            gap = float(np.linalg.norm(X.reshape(rows, cols) - E) / np.linalg.norm(E))
            worst[(rows, cols)] = max(worst.get((rows, cols), 0.0), gap)
    print({k: round(v, 4) for k, v in worst.items()})
    assert len(worst) == 12 and max(worst.values()) <= GAP_BOUND, worst
    # what the bound is there to catch: the product taken on the wrong side misses by order 1
    rows, cols = 17, 33
    u = np.random.default_rng(100).standard_normal(rows * cols).astype(np.float32)
    E = MM.ns_exact(u, rows, cols, *COEFFS, 5)
    wrong = MM.ns_exact(u, rows, cols, *COEFFS, 5) * 0.5
    assert np.linalg.norm(wrong - E) / np.linalg.norm(E) >= 0.5


def test_bf16_rounds_to_nearest_even_on_the_bit_pattern():
    f = np.float32
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -1.0 - 2.0 ** -8, 3.4445, 0.0, -0.0, np.inf, 3.4e38, 1e-40], f)
    got = MM.bf16(x)
    assert got[:5].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0] and got[5] == f(3.4375) and got[8] == np.inf and got[9] == np.inf
    assert np.signbit(got[7]) and not np.signbit(got[6]) and not (got.view(np.uint32) & 0xFFFF).any()
    assert np.isnan(MM.bf16(np.array([np.nan], f))[0])
    import torch
    r = np.random.default_rng(0).standard_normal(4096).astype(f) * f(10.0) ** np.random.default_rng(1).integers(-20, 20, 4096).astype(f)
    cases.same_bits(MM.bf16(r), torch.from_numpy(r).to(torch.bfloat16).to(torch.float32).numpy(), "bf16 against torch's conversion")


def test_the_chain_is_a_matrix_product_and_the_thin_gram_a_sum():
    rng = np.random.default_rng(2)
    a, b = MM.bf16(rng.standard_normal((5, 9)).astype(np.float32)), MM.bf16(rng.standard_normal((9, 4)).astype(np.float32))
    want = a.astype(np.float64) @ b.astype(np.float64)
    assert np.abs(MM.chain(a, b) - want).max() <= 9 * 2.0 ** -24 * np.abs(want).max() * 4
    A, sums = MM.gram(MM.bf16(rng.standard_normal((3, 50)).astype(np.float32)))
    assert sums.shape == (3, 3) and (sums == sums.T).all() and (A == A.T).all()
    assert float(MM.scale_of((3, 3, 64, 64))) == float(np.float32(0.2)) and float(MM.scale_of((1800, 512))) == float(np.float32(0.2) * np.sqrt(np.float32(1800) / np.float32(512)))


# ------------------------------------------------------------------------------------------------ 1. the step
@pytest.mark.parametrize("ns_steps", [0, 1, 5])
def test_every_arena_and_every_matrix_equals_the_model_in_every_bit(emu_lib, ns_steps):
    """Adam and Muon tensors interleaved, general and thin matrices in both orientations, four steps at t = 1, 2, 3, 1000: params, momentum, u, ema,
    the zeroed grads, the pads, read_norms, and X0, n, A, B, X through muon_debug; the float64 sums also against math.fsum"""
    combos = [c for c in cases.COMBOS if c["ns_steps"] == ns_steps]
    assert cases.bits_case(emu_lib, combos) == 2 * len(cases.STEPS_T)


def test_the_witnesses(emu_lib):
    assert cases.witness_case(emu_lib) == sorted(cases.WITNESSES)


def test_state_round_trip(emu_lib):
    assert cases.round_trip_case(emu_lib) == 3


def test_every_refusal_by_its_text(emu_lib):
    msgs = cases.refusal_case(emu_lib)
    assert len(set(msgs.values())) >= 12


def test_a_step_without_muon_is_the_parents_step(emu_lib):
    """an optimizer that never saw gaz_muon_set launches what it launched before, and the symbols are what tells the feature"""
    from grok_alpha_zero_amd import optim as P
    from grok_alpha_zero_amd.engine import EngineError
    opt = P.FusedOptimizer([5, 20], orthograd=True, lib_path=emu_lib)
    assert opt.launches_per_step == 3 and opt.muon is None
    opt.close()
    with pytest.raises(EngineError, match="no gaz_muon_set: rebuild it"):
        P.bind_muon(types.SimpleNamespace())


# ------------------------------------------------------------------------------------------------ 2. ABI
def test_ctypes_mirror_of_the_config_matches_the_header(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import abi_stub
    from grok_alpha_zero_amd.optim import MuonConfig
    hdr = abi_stub.parse_structs()["gaz_muon_config"]
    want = [(f, getattr(C, abi_stub.CTYPES[t]) if t in abi_stub.CTYPES else C.c_void_p) for f, t, n in hdr]
    assert all(n == 0 for _, _, n in hdr) and list(MuonConfig._fields_) == want
    fields = [f for f, _ in MuonConfig._fields_]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gaz_engine.h"\nint main(void){printf("%zu\\n", sizeof(gaz_muon_config));'
                   + "".join(f'printf("%zu\\n", offsetof(gaz_muon_config, {f}));' for f in fields) + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "probe")])
    out = [int(x) for x in subprocess.check_output([str(tmp_path / "probe")]).decode().split()]
    assert out[0] == C.sizeof(MuonConfig) and out[1:] == [getattr(MuonConfig, f).offset for f in fields]


def test_libraries_export_the_muon_symbols(emu_lib):
    from grok_alpha_zero_amd import engine as E
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gaz_engine.h")).read(), flags=re.S)
    want = set(re.findall(r"\b(gaz_muon_\w+)\s*\(", hdr))
    assert want == {"gaz_muon_config_size", "gaz_muon_set", "gaz_muon_read"}
    for lib in [emu_lib] + ([E.DEFAULT_LIB] if os.path.exists(E.DEFAULT_LIB) else []):
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
        got = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
        assert want <= got, (lib, sorted(want - got))


# ------------------------------------------------------------------------------------------------ 3. the sanitizer driver
def test_the_step_at_the_buffer_limits_under_the_sanitizers():
    """the optimizer's host code and the one-lane build of the Muon kernels, linked into a program of their own with -fsanitize=address,undefined
    -fno-sanitize-recover=all, driven through the C ABI with caller buffers of exactly the documented sizes"""
    rc, out = cases.run_driver(cases.build_driver())
    assert rc == 0, f"exit status {rc}\n{out[-3000:]}"

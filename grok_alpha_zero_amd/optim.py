"""FusedOptimizer — the reference's optimizer chain Orthograd(Grokfast_EMA(Adam | Nadam)) (Train.py:25-31) as one multi-tensor HIP step over
flat arenas (the gaz_optim_* section of include/gaz_engine.h; csrc/optim.hpp).  The parameters and gradients of every
tensor live in two flat device arenas that PyTorch sees as views, so autograd accumulates straight into the grads arena and a step is one
kernel launch (three with Orthograd) whatever the number of tensors.

    opt = FusedOptimizer([p.numel() for p in net.parameters()], kind="nadam", orthograd=True, grokfast=True, lamb=2.0)
    opt.attach(net)                                # .data and .grad of every parameter become views of the arenas
    loss(net(x), y).backward()
    opt.step(lr)                                   # t counts from 1; the grads arena is zero afterwards

Muon (the reference's Net/Optimizers/muon.py; csrc/muon.hpp): with muon=dict(...) and the tensors' shapes, every tensor of two
and more dimensions that is not listed in muon["adam_tensors"] takes momentum and five Newton-Schulz iterations on f32 MFMA, every other one
muon.py's Adam / Nadam; the launch count of a step still does not depend on the number of tensors.

    opt = FusedOptimizer(sizes, kind="nadam", beta_2=0.995, epsilon=1e-8, weight_decay=0.004, orthograd=True, grokfast=True,
                         muon=dict(adam_tensors=[k for k, name in enumerate(names) if "bias" in name]), shapes=[tuple(p.shape) for p in params])
"""
import ctypes as C

import numpy as np

from .engine import EngineError, load_library
from .replay import _DevView

KINDS = {"adam": 0, "nadam": 1}
ARENAS = {"params": 0, "grads": 1, "momentum": 2, "velocity": 3, "ema": 4}


class OptimConfig(C.Structure):         # gaz_optim_config — tests/test_optim_emu.py checks names, order and sizeof against the header
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("n_tensors", C.c_int32), ("kind", C.c_int32), ("sizes", C.c_void_p),
                ("beta_1", C.c_double), ("beta_2", C.c_double), ("epsilon", C.c_double), ("weight_decay", C.c_double), ("orthograd", C.c_int32),
                ("grokfast", C.c_int32), ("alpha", C.c_double), ("lamb", C.c_double)]


class MuonConfig(C.Structure):          # gaz_muon_config — tests/test_muon_emu.py checks names, order and sizeof against the header
    _fields_ = [("struct_size", C.c_uint32), ("n_tensors", C.c_int32), ("rows", C.c_void_p), ("cols", C.c_void_p), ("scale", C.c_void_p),
                ("muon_beta", C.c_double), ("nesterov", C.c_int32), ("ns_steps", C.c_int32), ("muon_a", C.c_double), ("muon_b", C.c_double),
                ("muon_c", C.c_double), ("adam_lr_ratio", C.c_double)]


MUON_DEFAULTS = dict(muon_beta=0.95, nesterov=True, muon_a=3.4445, muon_b=-4.7750, muon_c=2.0315, ns_steps=5, adam_lr_ratio=1.0, adam_tensors=())
MUON_WHAT = {"X0": 0, "n": 1, "X": 2, "A": 3, "B": 4}


def muon_scale(shape):
    """muon.py's scaling_factor of a tensor of this shape, in f32 as TensorFlow computes it: 0.2 * sqrt(max(1, shape[-2] / shape[-1]))"""
    f = np.float32
    return f(0.2) * np.sqrt(np.maximum(f(1.0), f(shape[-2]) / f(shape[-1])))


def muon_table(shapes, adam_tensors=()):
    """(rows i32, cols i32, scale f32) of gaz_muon_config: a tensor of two and more dimensions outside adam_tensors is a Muon tensor, read as
    shape[0] x the rest; rows = cols = 0 names an Adam tensor"""
    n, adam = len(shapes), {int(k) for k in adam_tensors}
    if adam - set(range(n)):
        raise ValueError(f"muon: adam_tensors names the tensors {sorted(adam - set(range(n)))} of {n}")
    rows, cols, scale = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    for k, sh in enumerate(shapes):
        sh = tuple(int(d) for d in sh)
        if len(sh) >= 2 and k not in adam:
            rows[k], cols[k], scale[k] = sh[0], int(np.prod(sh[1:], dtype=np.int64)), muon_scale(sh)
    return rows, cols, scale


def bind(L):
    """argument types of the gaz_optim_* entry points on a loaded library; a library built before the feature has none of them"""
    if getattr(L, "_gaz_optim_bound", False):
        return L
    if not hasattr(L, "gaz_optim_create"):
        raise EngineError("this library has no gaz_optim_create: rebuild it")
    H, P, I32, I64, D = C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.gaz_optim_config_size.argtypes = []
    L.gaz_optim_create.argtypes = [C.POINTER(OptimConfig), C.POINTER(H)]
    L.gaz_optim_destroy.argtypes = [H]; L.gaz_optim_destroy.restype = None
    L.gaz_optim_last_error.argtypes = [H]; L.gaz_optim_last_error.restype = C.c_char_p
    L.gaz_optim_layout.argtypes = [H, P, P]
    L.gaz_optim_ptrs.argtypes = [H] + [C.POINTER(C.c_void_p)] * 5
    L.gaz_optim_read.argtypes = [H, I32, I64, I64, P]
    L.gaz_optim_write.argtypes = [H, I32, I64, I64, P]
    L.gaz_optim_step.argtypes = [H, D, I64, I32]
    L.gaz_optim_step_timed.argtypes = [H, D, I64, I32, I32, C.POINTER(D)]
    L.gaz_optim_read_norms.argtypes = [H, P]
    L.gaz_optim_synchronize.argtypes = [H]
    for f in ("config_size", "create", "layout", "ptrs", "read", "write", "step", "step_timed", "read_norms", "synchronize"):
        getattr(L, "gaz_optim_" + f).restype = C.c_int
    if L.gaz_optim_config_size() != C.sizeof(OptimConfig):
        raise RuntimeError(f"gaz_optim_config has {L.gaz_optim_config_size()} bytes in the library, {C.sizeof(OptimConfig)} in this binding: rebuild the library")
    L._gaz_optim_bound = True
    return L


def bind_muon(L):
    """the gaz_muon_* entry points; a library built before Muon has none of them"""
    if getattr(L, "_gaz_muon_bound", False):
        return L
    if not hasattr(L, "gaz_muon_set"):
        raise EngineError("this library has no gaz_muon_set: rebuild it")
    L.gaz_muon_config_size.argtypes = []
    L.gaz_muon_set.argtypes = [C.c_void_p, C.POINTER(MuonConfig)]
    L.gaz_muon_read.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    for f in ("config_size", "set", "read"):
        getattr(L, "gaz_muon_" + f).restype = C.c_int
    if L.gaz_muon_config_size() != C.sizeof(MuonConfig):
        raise RuntimeError(f"gaz_muon_config has {L.gaz_muon_config_size()} bytes in the library, {C.sizeof(MuonConfig)} in this binding: rebuild the library")
    L._gaz_muon_bound = True
    return L


class FusedOptimizer:
    """One optimizer over the tensors of `sizes` (elements each) on one device.  kind "adam" / "nadam" (or 0 / 1); weight_decay is Keras'
    decoupled decay; orthograd / grokfast switch the two gradient stages on, alpha and lamb are Grokfast's.  muon = a dict over MUON_DEFAULTS
    (muon.py's keywords, and adam_tensors: the indices of the tensors of two and more dimensions that take Adam all the same) with shapes = the
    shape of every tensor: Muon mode, in which kind, beta_1, beta_2 and epsilon are those of muon.py's own Adam."""

    def __init__(self, sizes, kind="nadam", beta_1=0.9, beta_2=0.999, epsilon=1e-7, weight_decay=0.0, orthograd=False, grokfast=False, alpha=0.99,
                 lamb=5.0, device=0, lib_path=None, muon=None, shapes=None):
        self.L = bind(load_library(lib_path))
        if isinstance(kind, str):
            if kind.lower() not in KINDS:
                raise ValueError(f"kind must be 'adam' or 'nadam', not {kind!r}")
            kind = KINDS[kind.lower()]
        self.sizes = [int(s) for s in sizes]
        self._sizes = np.asarray(self.sizes, np.int64).reshape(-1)
        self.cfg = OptimConfig(struct_size=C.sizeof(OptimConfig), device=int(device), n_tensors=len(self.sizes), kind=int(kind), sizes=self._sizes.ctypes.data,
                               beta_1=float(beta_1), beta_2=float(beta_2), epsilon=float(epsilon), weight_decay=float(weight_decay), orthograd=int(bool(orthograd)),
                               grokfast=int(bool(grokfast)), alpha=float(alpha), lamb=float(lamb))
        self.h = C.c_void_p()
        if self.L.gaz_optim_create(C.byref(self.cfg), C.byref(self.h)) != 0:
            self.h = None
            raise EngineError(self.L.gaz_optim_last_error(None).decode())
        n = len(self.sizes)
        self.offsets, info = np.zeros(n, np.int64), (C.c_int64 * 5)()
        self._ck(self.L.gaz_optim_layout(self.h, self.offsets.ctypes.data, info))
        self.total, self.n_chunks, self.chunk, self.launches_per_step, self.host_memory = int(info[0]), int(info[1]), int(info[2]), int(info[3]), bool(info[4])
        p = [C.c_void_p() for _ in range(5)]
        self._ck(self.L.gaz_optim_ptrs(self.h, *[C.byref(x) for x in p]))
        self.ptrs = tuple(x.value or 0 for x in p)
        self.steps = 0
        self._views = {}
        self.muon = None
        if muon is not None:
            try:
                self._set_muon(dict(muon), shapes)
            except Exception:
                self.close()
                raise

    def _set_muon(self, muon, shapes):
        unknown = set(muon) - set(MUON_DEFAULTS)
        if unknown:
            raise ValueError(f"muon: unknown keys {sorted(unknown)}")
        if shapes is None or len(shapes) != len(self.sizes) or any(int(np.prod(sh, dtype=np.int64)) != n for sh, n in zip(shapes, self.sizes)):
            raise ValueError("muon: shapes must give the shape of every tensor of sizes")
        bind_muon(self.L)
        m = dict(MUON_DEFAULTS, **muon)
        self.shapes = [tuple(int(d) for d in sh) for sh in shapes]
        self._muon_rows, self._muon_cols, self._muon_scale = muon_table(self.shapes, m["adam_tensors"])
        mc = MuonConfig(struct_size=C.sizeof(MuonConfig), n_tensors=len(self.sizes), rows=self._muon_rows.ctypes.data, cols=self._muon_cols.ctypes.data,
                        scale=self._muon_scale.ctypes.data, muon_beta=float(m["muon_beta"]), nesterov=int(bool(m["nesterov"])), ns_steps=int(m["ns_steps"]),
                        muon_a=float(m["muon_a"]), muon_b=float(m["muon_b"]), muon_c=float(m["muon_c"]), adam_lr_ratio=float(m["adam_lr_ratio"]))
        self._ck(self.L.gaz_muon_set(self.h, C.byref(mc)))
        info = (C.c_int64 * 5)()
        self._ck(self.L.gaz_optim_layout(self.h, None, info))
        self.launches_per_step = int(info[3])
        self.muon = dict(m, adam_tensors=sorted(int(k) for k in m["adam_tensors"]))
        self.muon_tensors = [k for k in range(len(self.sizes)) if self._muon_rows[k] > 0]

    def muon_debug(self, k):
        """of Muon tensor k after the last step: X0 and the final X [rows, cols], n, and A, B [P, P] of the last iteration, P = min(rows, cols)"""
        if self.muon is None:
            raise EngineError("this optimizer is not in Muon mode")
        r, c = int(self._muon_rows[k]), int(self._muon_cols[k])
        p, out = max(min(r, c), 1), {}
        for name, shape in (("X0", (r, c)), ("n", ()), ("X", (r, c)), ("A", (p, p)), ("B", (p, p))):
            buf = np.zeros(max(int(np.prod(shape, dtype=np.int64)), 1), np.float32)
            self._ck(self.L.gaz_muon_read(self.h, int(k), MUON_WHAT[name], buf.ctypes.data))
            out[name] = buf[:int(np.prod(shape, dtype=np.int64))].reshape(shape) if shape else buf[0]
        return out

    def _ck(self, rc):
        if rc != 0:
            raise EngineError(self.L.gaz_optim_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.gaz_optim_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            if not self._views:                  # a view handed out keeps the arenas: they go with the process
                self.close()
        except Exception:      # noqa: BLE001 — interpreter shutdown
            pass

    # ------------------------------------------------------------------------------------------------ the arenas
    def _arena(self, arena):
        return ARENAS[arena] if isinstance(arena, str) else int(arena)

    def read(self, arena, first=0, n=None):
        """elements first .. first + n - 1 of an arena ("params", "grads", "momentum", "velocity", "ema" or 0 .. 4), pads included -> f32 [n]"""
        n = self.total - first if n is None else n
        out = np.zeros(max(int(n), 0), np.float32)
        self._ck(self.L.gaz_optim_read(self.h, self._arena(arena), int(first), int(n), out.ctypes.data))
        return out

    def write(self, arena, data, first=0):
        data = np.ascontiguousarray(data, np.float32).reshape(-1)
        self._ck(self.L.gaz_optim_write(self.h, self._arena(arena), int(first), data.shape[0], data.ctypes.data))

    def get(self, arena, k):
        """tensor k of an arena -> f32 [sizes[k]]"""
        return self.read(arena, int(self.offsets[k]), self.sizes[k])

    def set(self, arena, k, data):
        data = np.ascontiguousarray(data, np.float32).reshape(-1)
        if data.shape[0] != self.sizes[k]:
            raise ValueError(f"tensor {k} has {self.sizes[k]} elements, not {data.shape[0]}")
        self.write(arena, data, int(self.offsets[k]))

    def _flat(self, arena):
        """the whole arena as the build's zero-copy view: a numpy array on the one-lane build, a torch tensor on the device otherwise"""
        a = self._arena(arena)
        if a not in self._views:
            if not self.ptrs[a]:
                raise EngineError("this optimizer has no ema arena (grokfast is off)")
            if self.host_memory:
                self._views[a] = np.ctypeslib.as_array((C.c_float * self.total).from_address(self.ptrs[a]))
            else:
                if not getattr(self.L, "_gaz_torch_first", False):
                    raise EngineError("FusedOptimizer views: import torch before the first engine, replay window or optimizer of the process is created, so that "
                                      "the engine library and torch share one HIP runtime")
                import torch
                self._views[a] = torch.as_tensor(_DevView(self.ptrs[a], (self.total,), "<f4"), device=torch.device("cuda", int(self.cfg.device)))
        return self._views[a]

    def _tensors(self, arena):
        flat = self._flat(arena)
        return [flat[int(o):int(o) + s] for o, s in zip(self.offsets, self.sizes)]

    @property
    def params(self):
        """the tensors of the params arena as zero-copy views (flat, sizes[k] elements each)"""
        return self._tensors(0)

    @property
    def grads(self):
        return self._tensors(1)

    def attach(self, module):
        """re-points every nn.Parameter of a torch module, in module.parameters() order: .data becomes a view of the params arena (holding the
        parameter's present values), .grad a view of the grads arena, so that autograd accumulates straight into it.  Keep the gradients where
        they are: zero them through step(zero_grads=True), not through zero_grad(set_to_none=True)."""
        import torch
        ps = list(module.parameters())
        if [p.numel() for p in ps] != self.sizes:
            raise ValueError(f"attach: the module's parameters have the sizes {[p.numel() for p in ps]}, this optimizer was made for {self.sizes}")
        wrap = torch.from_numpy if self.host_memory else (lambda x: x)
        for p, w, g in zip(ps, self.params, self.grads):
            if p.dtype != torch.float32:
                raise ValueError("attach: every parameter must be float32")
            w, g = wrap(w).view(p.shape), wrap(g).view(p.shape)
            with torch.no_grad():
                w.copy_(p.data)
            p.data = w
            p.grad = g
        return module

    # ------------------------------------------------------------------------------------------------ stepping
    def step(self, lr, t=None, zero_grads=True):
        """one step at learning rate lr; t = the step number of the bias corrections (default: one more than the last step's)"""
        t = self.steps + 1 if t is None else int(t)
        self._ck(self.L.gaz_optim_step(self.h, float(lr), t, 1 if zero_grads else 0))
        self.steps = t

    def step_timed(self, lr, t=1, zero_grads=True, repeats=100):
        """measurement hook: ms per step, HIP events around `repeats` steps (after one warm-up); the state moves"""
        ms = C.c_double()
        self._ck(self.L.gaz_optim_step_timed(self.h, float(lr), int(t), 1 if zero_grads else 0, int(repeats), C.byref(ms)))
        return ms.value

    def synchronize(self):
        self._ck(self.L.gaz_optim_synchronize(self.h))

    def norms(self):
        """f64 [n_tensors, 4]: the sums w.g, w.w, g.g, go.go of the last step before their rounding to f32 (zeros without orthograd)"""
        out = np.zeros((len(self.sizes), 4), np.float64)
        self._ck(self.L.gaz_optim_read_norms(self.h, out.ctypes.data))
        return out

    def state(self):
        """what a later optimizer of the same sizes and settings needs to continue bit for bit: the step counter and the arenas"""
        st = dict(steps=self.steps, sizes=list(self.sizes), params=self.read(0), momentum=self.read(2), velocity=self.read(3))
        if self.cfg.grokfast:
            st["ema"] = self.read(4)
        return st

    def load_state(self, st):
        if list(st["sizes"]) != self.sizes:
            raise ValueError(f"load_state: a state of the sizes {list(st['sizes'])} for an optimizer of {self.sizes}")
        if bool(self.cfg.grokfast) != ("ema" in st):
            raise ValueError("load_state: the state and the optimizer differ in grokfast")
        for name in ("params", "momentum", "velocity") + (("ema",) if self.cfg.grokfast else ()):
            if np.asarray(st[name]).size != self.total:
                raise ValueError(f"load_state: {name} has {np.asarray(st[name]).size} elements, the arenas have {self.total}")
            self.write(name, st[name])
        self.steps = int(st["steps"])


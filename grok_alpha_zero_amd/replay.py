"""ReplayWindow — the training rows of the last generations on the device, served as shuffled, augmented minibatches (the gaz_replay_* section
of include/gaz_engine.h).  It replaces the reference's Dataloader.py: the rows stay un-augmented in device memory, the
plan of an epoch (generation decay, held-out test rows, the reference's win-ratio balancing) is built by kernels, and a minibatch is one
gather kernel that applies the board symmetry as it reads.  Every draw is a stateless function of (seed, generation, game, row, epoch), so a
window refilled from the replay files serves exactly what the live one served.

    w = ReplayWindow("Connect4", capacity_rows=4_000_000, seed=1)
    run_self_play(..., replay=w)                   # or w.append(generation, engine.drain_samples()) / w.append_file(folder, generation)
    M = w.begin_epoch("train", epoch=0)
    for boards, policies, values in w.batches(256): ...
"""
import ctypes as C
import math

import numpy as np

from .engine import GAME_DIMS, GAME_IDS, EngineError, load_library

N_AUG = {0: 8, 1: 2, 2: 8}
SPLITS = {"train": 0, "test": 1, 0: 0, 1: 1}


class ReplayConfig(C.Structure):        # gaz_replay_config — tests/test_replay_emu.py checks names, order and sizeof against the header
    _fields_ = [("struct_size", C.c_uint32), ("game", C.c_int32), ("device", C.c_int32), ("reserved_", C.c_int32), ("capacity_rows", C.c_int64),
                ("seed", C.c_uint64), ("test_fraction", C.c_double), ("target_ratio", C.c_double)]


def bind(L):
    """argument types of the gaz_replay_* entry points on a loaded library; a library built before the feature has none of them"""
    if getattr(L, "_gaz_replay_bound", False):
        return L
    if not hasattr(L, "gaz_replay_create"):
        raise EngineError("this library has no gaz_replay_create: rebuild it")
    H, P, I32, I64 = C.c_void_p, C.c_void_p, C.c_int32, C.c_int64
    L.gaz_replay_config_size.argtypes = []
    L.gaz_replay_create.argtypes = [C.POINTER(ReplayConfig), C.POINTER(H)]
    L.gaz_replay_destroy.argtypes = [H]; L.gaz_replay_destroy.restype = None
    L.gaz_replay_last_error.argtypes = [H]; L.gaz_replay_last_error.restype = C.c_char_p
    L.gaz_replay_append.argtypes = [H, I32, I32, P, P, P, P, I64]
    L.gaz_replay_evict.argtypes = [H, I32]
    L.gaz_replay_info.argtypes = [H, P, I32, P, C.POINTER(I32)]
    L.gaz_replay_read_rows.argtypes = [H, I64, I64, P, P, P, P]
    L.gaz_replay_begin_epoch.argtypes = [H, I32, C.c_uint32, I32, C.c_double, C.c_double, C.POINTER(I64)]
    L.gaz_replay_read_plan.argtypes = [H, I64, I64, P]
    L.gaz_replay_sample.argtypes = [H, I64, I32, I32]
    L.gaz_replay_sample_timed.argtypes = [H, I64, I32, I32, I32, C.POINTER(C.c_double)]; L.gaz_replay_sample_timed.restype = C.c_int
    L.gaz_replay_batch_ptrs.argtypes = [H] + [C.POINTER(C.c_void_p)] * 5
    L.gaz_replay_read_batch.argtypes = [H, P, P, P, P, P]
    L.gaz_replay_synchronize.argtypes = [H]
    for f in ("config_size", "create", "append", "evict", "info", "read_rows", "begin_epoch", "read_plan", "sample", "batch_ptrs", "read_batch", "synchronize"):
        getattr(L, "gaz_replay_" + f).restype = C.c_int
    if L.gaz_replay_config_size() != C.sizeof(ReplayConfig):
        raise RuntimeError(f"gaz_replay_config has {L.gaz_replay_config_size()} bytes in the library, {C.sizeof(ReplayConfig)} in this binding: rebuild the library")
    L._gaz_replay_bound = True
    return L


class _DevView:
    """a device buffer as torch.as_tensor takes it (__cuda_array_interface__, version 2)"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = dict(shape=tuple(shape), typestr=typestr, data=(int(ptr), False), version=2, strides=None)


class ReplayWindow:
    """One window of training rows on one device.  `capacity_rows` un-augmented rows; `test_fraction` of the rows are held out for the test
    split for good; `target_ratio` (None = no balancing) is the reference's first-player win ratio that begin_epoch balances the admitted games
    towards, by its parity rule (a game counts as a first-player win iff it has an odd number of rows)."""

    def __init__(self, game, capacity_rows, seed, test_fraction=0.1, target_ratio=0.5, device=0, lib_path=None):
        self.L = bind(load_library(lib_path))
        self.game = game
        self.game_id = GAME_IDS[game] if game in GAME_IDS else -1
        self.H, self.W, self.Cc, self.A = GAME_DIMS.get(self.game_id, (0, 0, 0, 0))
        self.SB, self.n_aug = self.H * self.W * self.Cc, N_AUG.get(self.game_id, 0)
        self.capacity_rows, self.seed = int(capacity_rows), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.cfg = ReplayConfig(struct_size=C.sizeof(ReplayConfig), game=self.game_id, device=device, capacity_rows=self.capacity_rows, seed=self.seed,
                                test_fraction=float(test_fraction), target_ratio=float("nan") if target_ratio is None else float(target_ratio))
        self.h = C.c_void_p()
        if self.L.gaz_replay_create(C.byref(self.cfg), C.byref(self.h)) != 0:
            self.h = None
            raise EngineError(self.L.gaz_replay_last_error(None).decode())
        self._plan = None                            # (split, epoch, M) of the current plan
        self._last_n = 0

    def _ck(self, rc):
        if rc != 0:
            raise EngineError(self.L.gaz_replay_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.gaz_replay_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001 — interpreter shutdown
            pass

    # ------------------------------------------------------------------------------------------------ filling
    def append_arrays(self, generation, games, boards, policies, values):
        """games int32 [n, 6] as drain_samples gives them (column 4 = the game's first row), boards int8 [R, H, W, C], policies f32 [R, A],
        values f32 [R] or [R, 1]: augmentation plane 0 of a drain"""
        games = np.ascontiguousarray(games, np.int32).reshape(-1, 6)
        boards = np.ascontiguousarray(boards, np.int8); policies = np.ascontiguousarray(policies, np.float32)
        values = np.ascontiguousarray(values, np.float32).reshape(-1)
        R = values.shape[0]
        if boards.size != R * self.SB or policies.size != R * self.A:
            raise ValueError(f"append: {R} values with boards {boards.shape} and policies {policies.shape}")
        self._plan = None
        self._ck(self.L.gaz_replay_append(self.h, int(generation), games.shape[0], games.ctypes.data, boards.ctypes.data, policies.ctypes.data, values.ctypes.data, R))

    def append(self, generation, batch):
        """a SampleBatch of SelfPlayEngine.drain_samples: its games, in order, join `generation`"""
        self.append_arrays(generation, batch.games, batch.boards[0], batch.policies[0], batch.values)

    def append_file(self, folder, generation):
        """the games of a replay file that run_self_play wrote, in file order — the order in which a live window got them.  A game is n_aug
        consecutive dataset triples, plane 0 first; only that one is read.  Returns the number of games."""
        from .self_play import ReplayStore
        store = ReplayStore(folder)
        n = store.n_datasets() // 3 // self.n_aug
        games, b, p, v, row = np.zeros((n, 6), np.int32), [], [], [], 0
        for k in range(n):
            bk = store.read(f"boards_{self.n_aug * k}")
            games[k, 0], games[k, 4] = bk.shape[0], row
            b.append(np.asarray(bk, np.int8).reshape(-1, self.SB)); p.append(np.asarray(store.read(f"policies_{self.n_aug * k}"), np.float32).reshape(-1, self.A))
            v.append(np.asarray(store.read(f"values_{self.n_aug * k}"), np.float32).reshape(-1))
            row += bk.shape[0]
        cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dt)      # noqa: E731
        self.append_arrays(generation, games, cat(b, (0, self.SB), np.int8), cat(p, (0, self.A), np.float32), cat(v, (0,), np.float32))
        return n

    def evict(self, before_generation):
        self._plan = None
        self._ck(self.L.gaz_replay_evict(self.h, int(before_generation)))

    def info(self):
        """dict: rows, games, oldest, newest (None when empty), held_out, capacity, plan_rows (None without a plan) and generations =
        [(generation, games, rows)], oldest first"""
        out, n = (C.c_int64 * 8)(), C.c_int32()
        self._ck(self.L.gaz_replay_info(self.h, out, 0, None, C.byref(n)))
        g = np.zeros((max(n.value, 1), 3), np.int64)
        self._ck(self.L.gaz_replay_info(self.h, out, g.shape[0], g.ctypes.data, C.byref(n)))
        return dict(rows=int(out[0]), games=int(out[1]), oldest=None if out[2] < 0 else int(out[2]), newest=None if out[3] < 0 else int(out[3]), held_out=int(out[4]),
                    capacity=int(out[5]), plan_rows=None if out[7] < 0 else int(out[7]), generations=[tuple(int(x) for x in r) for r in g[:n.value]])

    def rows(self, first=0, n=None):
        """stored rows by store order -> (boards int8 [n, H, W, C], policies f32 [n, A], values f32 [n], meta int32 [n, 3] = generation, game
        within it, row within the game)"""
        if n is None:
            n = self.info()["rows"] - first
        b, p = np.zeros((n, self.H, self.W, self.Cc), np.int8), np.zeros((n, self.A), np.float32)
        v, m = np.zeros(n, np.float32), np.zeros((n, 3), np.int32)
        self._ck(self.L.gaz_replay_read_rows(self.h, int(first), int(n), b.ctypes.data, p.ctypes.data, v.ctypes.data, m.ctypes.data))
        return b, p, v, m

    # ------------------------------------------------------------------------------------------------ an epoch
    def begin_epoch(self, split="train", epoch=0, newest_generation=None, percent=1.0, decay=0.75):
        """builds the epoch's plan on the device -> M, the number of rows the epoch serves.  A row takes part iff its game is admitted by the
        balancing, it belongs to `split`, and its draw for this epoch falls below max(percent - age * decay, 0), age counted in generations
        back from `newest_generation` (default: the newest stored)."""
        if split not in SPLITS:
            raise ValueError(f"begin_epoch: split must be 'train' or 'test', not {split!r}")
        if newest_generation is None:
            newest_generation = self.info()["newest"]
            newest_generation = 0 if newest_generation is None else newest_generation
        M = C.c_int64()
        self._plan = None
        self._ck(self.L.gaz_replay_begin_epoch(self.h, SPLITS[split], int(epoch), int(newest_generation), float(percent), float(decay), C.byref(M)))
        self._plan = (SPLITS[split], int(epoch), int(M.value))
        return int(M.value)

    def plan(self):
        """the current plan: the included rows (store order), ascending, uint32 [M]"""
        if self._plan is None:
            raise EngineError("no plan: call begin_epoch")
        out = np.zeros(self._plan[2], np.uint32)
        self._ck(self.L.gaz_replay_read_plan(self.h, 0, out.shape[0], out.ctypes.data))
        return out

    def sample(self, first, n, augment=True):
        """queues the gather of positions first .. first + n - 1 of the epoch on the window's stream; batch_ptrs() are its outputs"""
        self._ck(self.L.gaz_replay_sample(self.h, int(first), int(n), 1 if augment else 0))
        self._last_n = int(n)

    def sample_timed(self, first, n, augment=True, repeats=100):
        """measurement hook: ms per gather of this batch, HIP events around `repeats` launches on the window's stream (after one warm-up)"""
        ms = C.c_double()
        self._ck(self.L.gaz_replay_sample_timed(self.h, int(first), int(n), 1 if augment else 0, int(repeats), C.byref(ms)))
        self._last_n = int(n)
        return ms.value

    def batch_ptrs(self):
        p = [C.c_void_p() for _ in range(5)]
        self._ck(self.L.gaz_replay_batch_ptrs(self.h, *[C.byref(x) for x in p]))
        return tuple(x.value or 0 for x in p)

    def synchronize(self):
        self._ck(self.L.gaz_replay_synchronize(self.h))

    def batch(self, first, n, augment=True, with_index=False):
        """positions first .. first + n - 1 of the epoch -> numpy (boards int8 [n, H, W, C], policies f32 [n, A], values f32 [n]); with_index:
        also the source rows (store order, uint32 [n]) and the symmetries (uint8 [n])"""
        self.sample(first, n, augment)
        b, p, v = np.zeros((n, self.H, self.W, self.Cc), np.int8), np.zeros((n, self.A), np.float32), np.zeros(n, np.float32)
        r, s = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        self._ck(self.L.gaz_replay_read_batch(self.h, b.ctypes.data, p.ctypes.data, v.ctypes.data, r.ctypes.data if with_index else None, s.ctypes.data if with_index else None))
        return (b, p, v, r, s) if with_index else (b, p, v)

    def batch_torch(self, first, n, augment=True, with_index=False):
        """batch() as torch tensors on the window's device: zero-copy views of batch_ptrs() through __cuda_array_interface__ after
        synchronize(), cloned — the clones are the caller's, the window's buffers are reused by the next sample.
        torch has to be imported BEFORE the first engine or window of the process is created: the torch wheel carries a HIP runtime of its own
        under the same soname as the system's, and the dynamic linker makes the two one instance only when torch's is loaded first (the engine
        library then resolves to it).  The other way round the process holds two runtimes, torch finds no GPU and a pointer of one means nothing
        to the other; that order is refused here."""
        if not getattr(self.L, "_gaz_torch_first", False):
            raise EngineError("batch_torch: import torch before the first engine or replay window of the process is created, so that the engine library "
                              "and torch share one HIP runtime")
        import torch
        self.sample(first, n, augment)
        self.synchronize()
        dev = torch.device("cuda", int(self.cfg.device))
        if n == 0:
            out = (torch.zeros((0, self.H, self.W, self.Cc), dtype=torch.int8, device=dev), torch.zeros((0, self.A), dtype=torch.float32, device=dev),
                   torch.zeros(0, dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.uint8, device=dev))
            return out if with_index else out[:3]
        pb, pp, pv, pr, ps = self.batch_ptrs()
        views = [(pb, (n, self.H, self.W, self.Cc), "|i1"), (pp, (n, self.A), "<f4"), (pv, (n,), "<f4")]
        if with_index:
            views += [(pr, (n,), "<i4"), (ps, (n,), "|u1")]       # (torch has no uint32 everywhere: the rows are below 2^31)
        return tuple(torch.as_tensor(_DevView(ptr, shape, ts), device=dev).clone() for ptr, shape, ts in views)

    def batch_sizes(self, batch_size):
        """the batches of the current epoch as (first, n): the reference's last short batch (Dataloader.py:168-174)"""
        if self._plan is None:
            raise EngineError("no plan: call begin_epoch")
        M, bs = self._plan[2], int(batch_size)
        if bs < 1:
            raise ValueError("batch_size must be at least 1")
        if M == 0:
            return []
        if M < bs:
            return [(0, M)]
        return [(k * bs, min(bs, M - k * bs)) for k in range(math.ceil(M / bs))]

    def batches(self, batch_size, augment=True, torch=False):
        """yields the current epoch, batch by batch"""
        for first, n in self.batch_sizes(batch_size):
            yield (self.batch_torch if torch else self.batch)(first, n, augment)


def score_network(window, game_class, configs, weights, split="test", epoch=0, batch_rows=1024, device=0, lib_path=None, hash_salt=0):
    """The held-out loss of a network on the window's rows (SelfPlayEngine.score_replay; include/gaz_engine.h "HELD-OUT LOSS"): what the
    reference reads off its test dataloader as val_loss (Train.py:46-64), for the network as self-play runs it — the engine's evaluator with
    these weights, under the head mode of engine_search_settings.  A small scoring engine is made as orchestrator.compute_speed makes its
    own (n_games = batch_rows, no record ring, one game group) and closed again; weights = None scores the synthetic hash evaluator under
    `hash_salt`.  The window gets the plan begin_epoch(split, epoch, percent=1.0, decay=0.0): every row of the split.  -> the dict of score_replay."""
    from .engine import EVAL_HASH, EVAL_RESNET, SelfPlayEngine
    from .self_play import engine_search_settings
    build_config = configs[0]
    args, kw = engine_search_settings(game_class, configs)
    head = {k: kw[k] for k in ("search", "gumbel_m", "c_visit", "c_scale", "policy_is_logits", "gumbel_stablemax")}
    name = getattr(game_class, "ENGINE_NAME", game_class.__name__)
    use_net = weights is not None
    eng = SelfPlayEngine(name, int(batch_rows), *args, 0, evaluator=EVAL_RESNET if use_net else EVAL_HASH, hash_salt=hash_salt,
                         net_blocks=build_config.get("num_resnet_layers", 0) if use_net else 0, net_filters=build_config.get("num_filters", 128),
                         ring_capacity=0, game_groups=1, device=device, lib_path=lib_path, **head)
    try:
        if use_net:
            eng.load_weights(weights)
        window.begin_epoch(split, epoch, percent=1.0, decay=0.0)
        return eng.score_replay(window, batch_rows=int(batch_rows))
    finally:
        eng.close()

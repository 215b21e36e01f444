"""The cases of the replay window (grok_alpha_zero_amd/replay.py, the gaz_replay_* section of include/gaz_engine.h) that
the CPU suite runs on the emulation build (tests/test_replay_emu.py) and the -m gpu suite on the HIP build (tests/test_replay_gpu.py):
`lib_path` = the emulation library, or None for the product library.

What the window must store, plan and serve is computed by tests/replay_model.py from the rows the case itself made.  Every comparison is
exact: bytes, rows, symmetries.  The stored rows are RANDOM int8 states and f32 policies: real boards are sparse and would hide a wrong cell map."""
import os
import subprocess

import numpy as np

import replay_model as M
from selfplay_support import A_OF, EMU_DIR, N_AUG, ROOT, first_games

DIMS = {"TicTacToe": (3, 3, 2), "Connect4": (6, 7, 4), "Gomoku": (15, 15, 2)}
BATCH_SIZES = (1, 2, 63, 64, 65, 257)


def game_class(game):
    from grok_alpha_zero_amd.games import GAMES
    return GAMES[game]


def window(game, capacity, lib_path, seed=7, test_fraction=0.0, target_ratio=None):
    from grok_alpha_zero_amd.replay import ReplayWindow
    return ReplayWindow(game, capacity, seed, test_fraction=test_fraction, target_ratio=target_ratio, lib_path=lib_path)


def random_rows(rng, game, lengths):
    """games of the given row counts as a drain hands them over -> (games int32 [n, 6], boards, policies, values)"""
    H, W, Cc = DIMS[game]
    R = int(sum(lengths))
    games = np.zeros((len(lengths), 6), np.int32)
    games[:, 0] = lengths
    games[:, 4] = np.cumsum([0] + list(lengths[:-1])) if len(lengths) else 0
    return (games, rng.integers(-128, 128, (R, H, W, Cc)).astype(np.int8), rng.random((R, A_OF[game]), dtype=np.float32),
            (rng.random(R, dtype=np.float32) * 2 - 1).astype(np.float32))


def lengths_summing_to(rng, total, most=9):
    """ragged game lengths, zeros included, that sum to `total`"""
    out = []
    while sum(out) < total:
        out.append(int(min(rng.integers(0, most + 1), total - sum(out))))
    return out


def assert_rows(w, want_b, want_p, want_v, want_meta, what):
    b, p, v, m = w.rows()
    assert b.shape == want_b.shape and b.tobytes() == want_b.tobytes(), f"{what}: boards"
    assert p.tobytes() == want_p.tobytes() and v.tobytes() == want_v.tobytes(), f"{what}: policies / values"
    np.testing.assert_array_equal(m, np.array(want_meta, np.int32).reshape(-1, 3), err_msg=f"{what}: meta")


def meta_of(games):
    return M.row_ids(games)


# ------------------------------------------------------------------------------------------------ the store
def store_case(game, lib_path):
    """append / rows round trip with ragged games (a 0-row game among them), a ring of 100 rows wrapping, eviction of whole generations, the
    over-capacity error leaving the window unchanged, out-of-order generations refused, info"""
    from grok_alpha_zero_amd.engine import EngineError
    rng = np.random.default_rng(11)
    w = window(game, 100, lib_path, test_fraction=0.3)
    assert w.info() == dict(rows=0, games=0, oldest=None, newest=None, held_out=0, capacity=100, plan_rows=None, generations=[])
    parts, games = [], []                                                   # what is live: (generation, (games, b, p, v)), and (g, i, rows)

    def add(gen, lengths):
        d = random_rows(rng, game, lengths)
        d[0][:, 4] += 5                                                     # (a batch's first row need not be 0: rows are differences)
        w.append_arrays(gen, *d)
        i0 = sum(1 for g, _, _ in games if g == gen)
        parts.append((gen, d))
        games.extend((gen, i0 + k, n) for k, n in enumerate(lengths))

    def check(what):
        live = [d for _, d in parts]
        cat = lambda k: np.concatenate([d[k] for d in live])                 # noqa: E731
        assert_rows(w, cat(1), cat(2), cat(3), meta_of(games), what)
        info = w.info()
        gens = sorted({g for g, _, _ in games})
        assert info["rows"] == sum(n for _, _, n in games) and info["games"] == len(games) and info["oldest"] == gens[0] and info["newest"] == gens[-1]
        assert info["generations"] == [(g, sum(1 for x in games if x[0] == g), sum(x[2] for x in games if x[0] == g)) for g in gens], (what, info)
        assert info["held_out"] == sum(M.held_out(7, r, 0.3) for r in M.row_ids(games)), what
        return info

    add(3, [4, 0, 9, 1, 7]); add(3, [6]); check("one generation, two appends")
    add(4, [9, 9, 0, 8, 5]); add(5, [3, 2, 30])
    info = check("three generations")
    assert info["rows"] == 93
    # 12 more rows do not fit: generation 3 (27 rows) leaves as a whole, the ring wraps
    add(6, [5, 7])
    del parts[:2]; del games[:6]
    info = check("wrapped")
    assert info["rows"] == 78 and info["oldest"] == 4
    sub = w.rows(70, 8)                                                    # a read across the physical end of the ring
    full = w.rows()
    assert all(a.tobytes() == b[70:78].tobytes() for a, b in zip(sub, full))
    # a generation that alone exceeds the capacity: refused, and the window is what it was
    before = [x.tobytes() for x in w.rows()]
    try:
        w.append_arrays(6, *random_rows(rng, game, [50, 40]))
        raise AssertionError("102 rows of one generation were accepted")
    except EngineError as e:
        assert "generation 6 alone has 102 rows" in str(e) and "capacity_rows is 100" in str(e), str(e)
    try:
        w.append_arrays(5, *random_rows(rng, game, [1]))
        raise AssertionError("generation 5 after generation 6 was accepted")
    except EngineError as e:
        assert "non-decreasing order" in str(e), str(e)
    assert [x.tobytes() for x in w.rows()] == before and check("after the refusals") == info
    add(6, [40, 30])                                                        # fits only without generations 4 and 5
    del parts[:2]; del games[:8]
    assert check("evicted to the generation being appended to")["generations"] == [(6, 4, 82)]
    add(9, [10]); w.evict(7); del parts[:2]; del games[:4]
    assert check("evict(7)")["generations"] == [(9, 1, 10)]
    w.evict(100)
    assert w.info()["rows"] == 0 and w.info()["games"] == 0 and w.rows()[0].shape[0] == 0
    w.close()


# ------------------------------------------------------------------------------------------------ the plan
PLAN_WINDOWS = ((0.0, None), (0.3, 0.5), (0.3, 0.0), (0.3, 1.0))          # (test_fraction, target_ratio)
PLAN_EPOCHS = ((5, 1.0, 0.75), (4, 0.9, 0.25), (5, 0.5, 0.0))             # (newest_generation, percent, decay): p reaches 0 for generation 3 in the first


def plan_case(live_rows, lib_path, windows=PLAN_WINDOWS, epochs=PLAN_EPOCHS, seed=21):
    """begin_epoch against the model, train and test, over TicTacToe rows in three generations -> the witnesses"""
    rng = np.random.default_rng(live_rows)
    per_gen = [live_rows // 3, live_rows // 3, live_rows - 2 * (live_rows // 3)]
    data, games = [], []
    for gen, rows in zip((3, 4, 5), per_gen):
        lengths = lengths_summing_to(rng, rows)
        if lengths:
            data.append((gen, random_rows(rng, "TicTacToe", lengths)))
            games.extend((gen, k, n) for k, n in enumerate(lengths))
    seen = dict(skipped=0, empty_old_generation=0, plans=0, rows=0)
    for tf, tr in windows:
        w = window("TicTacToe", live_rows + 3, lib_path, seed=seed, test_fraction=tf, target_ratio=tr)
        for gen, d in data:
            w.append_arrays(gen, *d)
        for newest, percent, decay in epochs:
            adm = M.admitted(games, newest, tr)
            walked = [a for a, (g, _, _) in zip(adm, games) if g <= newest]
            if tr is None:
                assert all(walked)                                        # NaN: no game is skipped
            else:
                seen["skipped"] += walked.count(False)
            for split in (0, 1):
                want = M.plan(seed, games, split, 3, newest, percent, decay, tf, tr)
                got_M = w.begin_epoch("test" if split else "train", epoch=3, newest_generation=newest, percent=percent, decay=decay)
                assert got_M == len(want) == w.info()["plan_rows"], (live_rows, tf, tr, newest, split, got_M, len(want))
                np.testing.assert_array_equal(w.plan(), want)
                if tf == 0.0 and split == 1:
                    assert got_M == 0
                seen["plans"] += 1; seen["rows"] += got_M
            if percent - (newest - 3) * decay <= 0 and per_gen[0]:
                seen["empty_old_generation"] += 1
        w.close()
    return seen


# ------------------------------------------------------------------------------------------------ order and gather
def gather_case(game, n_plan, lib_path, seed=5):
    """the whole epoch through batch() at every batch size, `first` no multiple of anything: rows, symmetries and bytes against the model"""
    rng = np.random.default_rng(n_plan)
    n_aug, cls = N_AUG[game], game_class(game)
    w = window(game, n_plan + 2, lib_path, seed=seed)
    w.append_arrays(1, *random_rows(rng, game, [n_plan + 1]))              # rows that leave again: the live rows start at the ring's last row and wrap
    w.evict(2)
    lengths = lengths_summing_to(rng, n_plan)
    games, sb, sp, sv = random_rows(rng, game, lengths)
    w.append_arrays(2, games, sb, sp, sv)
    assert w.info()["generations"] == [(2, len(lengths), n_plan)]
    planes = [M.augmented(cls, sb[s], sp[s]) for s in range(n_plan)]
    seen = dict(sym=set(), differs=set())
    orders = []
    for epoch, sizes in ((0, BATCH_SIZES), (1, BATCH_SIZES[::-1])):
        assert w.begin_epoch("train", epoch=epoch) == n_plan
        plan = w.plan()
        np.testing.assert_array_equal(plan, np.arange(n_plan, dtype=np.uint32))
        first, k, rows_seen, blobs = 0, 0, [], []
        while first < n_plan:
            n = min(sizes[k % len(sizes)], n_plan - first); k += 1
            b, p, v, r, s = w.batch(first, n, with_index=True)
            want_r, want_s = M.epoch_rows(seed, plan, epoch, 0, n_aug, first, n)
            np.testing.assert_array_equal(r, want_r); np.testing.assert_array_equal(s, want_s)
            for q in range(n):
                wb, wp = planes[r[q]]
                assert b[q].tobytes() == wb[s[q]].tobytes(), (game, n_plan, epoch, first + q, int(r[q]), int(s[q]))
                assert p[q].tobytes() == wp[s[q]].tobytes() and v[q].tobytes() == sv[r[q]].tobytes(), (game, n_plan, epoch, first + q)
                seen["sym"].add(int(s[q]))
                if s[q] and (b[q].tobytes() != sb[r[q]].tobytes() or p[q].tobytes() != sp[r[q]].tobytes()):
                    seen["differs"].add(int(s[q]))
            rows_seen += r.tolist(); blobs.append(b.tobytes() + p.tobytes() + v.tobytes())
            first += n
        assert sorted(rows_seen) == plan.tolist()                           # a permutation of the plan
        orders.append(rows_seen)
        again = w.batch(0, min(n_plan, 65), with_index=True)               # the same epoch twice: the same bytes
        first_again = w.batch(0, min(n_plan, 65), with_index=True)
        assert all(a.tobytes() == c.tobytes() for a, c in zip(again, first_again))
    # without augmentation: the stored rows themselves, and their multiset is the plan
    b, p, v, r, s = w.batch(0, n_plan, augment=False, with_index=True)
    assert not s.any() and sorted(r.tolist()) == list(range(n_plan))
    assert b.tobytes() == sb[r].tobytes() and p.tobytes() == sp[r].tobytes() and v.tobytes() == sv[r].tobytes()
    assert w.batch(n_plan, 0)[0].shape[0] == 0                              # n = 0 is legal, also at the end
    sizes = w.batch_sizes(64)
    assert sum(n for _, n in sizes) == n_plan and all(n == 64 for _, n in sizes[:-1]) and [f for f, _ in sizes] == list(range(0, n_plan, 64))
    w.close()
    if n_plan >= 17:
        assert orders[0] != orders[1]                                       # two epochs: two orders
    if n_plan >= 257:
        assert seen["sym"] == set(range(n_aug)) and seen["differs"] == set(range(1, n_aug)), seen
    return seen


# ------------------------------------------------------------------------------------------------ against the engine
ENGINE_CASES = {   # game -> iterations, fast iterations, max_actions
    "TicTacToe": (24, 6, 9), "Connect4": (40, 8, 42), "Gomoku": (12, 4, 4),
}


def engine_case(game, mode, lib_path, G=8, seed=66):
    """8 hash-evaluator games: a sampled row with symmetry k equals plane k of the drained batch.  mode "plain", or "cap" = the playout cap
    and the surprise weighting on (a game's rows are not its plies)"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    R, F, max_actions = ENGINE_CASES[game]
    cap = mode == "cap"
    eng = SelfPlayEngine(game, G, R, max_actions, 3, 2, 2.5, 0.5, seed=seed, hash_salt=6, ring_capacity=4 * G, games_budget=G, fast_iterations=F if cap else 0,
                         full_search_prob=0.3 if cap else 0.0, lib_path=lib_path)
    if cap:
        eng.set_sample_weighting(0.5, 1.0)
    if cap:                                             # (first_games' row accounting is the unweighted one: a weighted game's rows are differences)
        from surprise_cases import all_samples
        first = {slot: got[:4] for (slot, _), got in all_samples(eng, G, with_plies=False).items()}
    else:
        first = first_games(eng, G, samples=True)
    eng.close()
    rows = [first[s][1].shape[1] for s in sorted(first)]
    games = np.stack([first[s][0] for s in sorted(first)]).astype(np.int32)
    games[:, 4] = np.cumsum([0] + rows[:-1])
    planes_b = np.concatenate([first[s][1] for s in sorted(first)], axis=1)    # [n_aug, R, H, W, C]
    planes_p = np.concatenate([first[s][2] for s in sorted(first)], axis=1)
    values = np.concatenate([first[s][3][0] for s in sorted(first)]).reshape(-1)
    total = sum(rows)
    if cap:
        assert total != int(games[:, 0].sum()), "rows == plies: the cap and the weighting did not act"
    w = window(game, total + 1, lib_path, seed=seed)
    w.append_arrays(0, games, planes_b[0], planes_p[0], values)
    assert w.begin_epoch("train", epoch=2) == total
    b, p, v, r, s = w.batch(0, total, with_index=True)
    w.close()
    assert sorted(r.tolist()) == list(range(total)) and len(set(s.tolist())) > 1
    for q in range(total):
        assert b[q].tobytes() == planes_b[s[q], r[q]].tobytes() and p[q].tobytes() == planes_p[s[q], r[q]].tobytes() and v[q] == values[r[q]], (game, mode, q)
    return total, int(games[:, 0].sum())


# ------------------------------------------------------------------------------------------------ run_self_play and Run
TRAIN = dict(games_per_generation=12, MCTS_iteration_limit=16, max_actions=9, num_explore_actions_first=2, num_explore_actions_second=1, c_puct_init=1.25,
             dirichlet_alpha=1.0, total_generations=2)


def same_windows(a, b, what):
    """two windows: the same rows, plans and batches"""
    ia, ib = a.info(), b.info()
    assert {k: v for k, v in ia.items() if k != "plan_rows"} == {k: v for k, v in ib.items() if k != "plan_rows"}, (what, ia, ib)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.rows(), b.rows())), what
    for split in ("train", "test"):
        Ma, Mb = a.begin_epoch(split, epoch=1), b.begin_epoch(split, epoch=1)
        assert Ma == Mb and a.plan().tobytes() == b.plan().tobytes(), what
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a.batch(0, Ma, with_index=True), b.batch(0, Mb, with_index=True))), what
    return ia


def refill_case(tmp, lib_path):
    """a window fed live by run_self_play(replay=) and a fresh one refilled from the file it wrote are the same window, and the file is the
    file written without replay="""
    from grok_alpha_zero_amd.self_play import ReplayStore, run_self_play
    from samples_util import assert_same_file, file_contents
    cls, files = game_class("TicTacToe"), {}
    live = window("TicTacToe", 4096, lib_path, seed=3, test_fraction=0.25, target_ratio=0.5)
    for key, rp in (("with", live), ("without", None)):
        folder = os.path.join(str(tmp), key, "0")
        ReplayStore(folder).create()
        assert run_self_play(cls, ({}, TRAIN), folder, n_games=8, seed=9, hash_salt=4, lib_path=lib_path, replay=rp) == 12
        files[key] = file_contents(ReplayStore(folder))
    assert_same_file(files["with"], files["without"])
    for name in files["with"]:
        assert files["with"][name].tobytes() == files["without"][name].tobytes(), name
    fresh = window("TicTacToe", 4096, lib_path, seed=3, test_fraction=0.25, target_ratio=0.5)
    assert fresh.append_file(os.path.join(str(tmp), "with", "0"), 0) == 12
    info = same_windows(live, fresh, "live and refilled")
    assert info["games"] == 12 and info["rows"] == int(files["with"]["game_stats"][1]) and 0 < info["held_out"] < info["rows"]
    try:
        run_self_play(cls, ({}, TRAIN), os.path.join(str(tmp), "with", "0"), n_games=8, seed=9, lib_path=lib_path, device_samples=False, replay=live)
        raise AssertionError("replay= with device_samples=False was accepted")
    except ValueError as e:
        assert "device_samples=True" in str(e)
    live.close(); fresh.close()


def run_case(tmp, lib_path):
    """Run(replay=...) over two synthetic generations, then resumed for a third: what train_fn is given, and the resumed window is the one
    a refill from the files makes"""
    from grok_alpha_zero_amd.orchestrator import Run
    cls, calls = game_class("TicTacToe"), []
    spec = dict(capacity_rows=4096, generations=2, test_fraction=0.2, target_ratio=None, seed=5)
    root = os.path.join(str(tmp), "run")

    def train_fn(generation, folder, save_folder, replay=None):
        info = replay.info()
        M_train = replay.begin_epoch("train", epoch=generation)
        calls.append((generation, os.path.basename(folder), os.path.basename(save_folder), info, M_train, replay.batch(0, M_train, with_index=True)))
    quiet = lambda *a: None                                                 # noqa: E731
    kw = dict(train_fn=train_fn, root=root, n_games=8, seed=20, lib_path=lib_path, out=quiet, self_play_kwargs=dict(hash_salt=4, allow_synthetic=True), replay=spec)
    Run(cls, ({}, TRAIN), **kw)
    assert [(c[0], c[1], c[2]) for c in calls] == [(0, "0", "1"), (1, "1", "2")]
    assert [g for g, _, _ in calls[0][3]["generations"]] == [0] and [(g, n) for g, n, _ in calls[1][3]["generations"]] == [(0, 12), (1, 12)]
    Run(cls, ({}, dict(TRAIN, total_generations=3)), **kw)                   # resumed: generation 2 is played, the window refilled from folders 1 and 2
    assert [(c[0], c[1], c[2]) for c in calls[2:]] == [(2, "2", "3")]
    assert [(g, n) for g, n, _ in calls[2][3]["generations"]] == [(1, 12), (2, 12)]
    fresh = window("TicTacToe", 4096, lib_path, seed=5, test_fraction=0.2)
    fresh.append_file(os.path.join(root, "1"), 1); fresh.append_file(os.path.join(root, "2"), 2)
    assert fresh.begin_epoch("train", epoch=2) == calls[2][4]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(fresh.batch(0, calls[2][4], with_index=True), calls[2][5]))
    fresh.close()
    plain = []
    Run(cls, ({}, TRAIN), train_fn=lambda *a, **k: plain.append((a, k)), root=os.path.join(str(tmp), "plain"), n_games=8, seed=20, lib_path=lib_path, out=quiet,
        self_play_kwargs=dict(hash_salt=4, allow_synthetic=True))
    assert [len(a) for a, k in plain] == [3, 3] and not any(k for _, k in plain)      # without replay=: the call train_fn always got


# ------------------------------------------------------------------------------------------------ refusals
def refusal_case(lib_path):
    """every refusal by its text"""
    import ctypes as C
    from grok_alpha_zero_amd import replay as R
    from grok_alpha_zero_amd.engine import EngineError, load_library
    msgs = {}

    def refused(name, text, call):
        try:
            call()
        except EngineError as e:
            msgs[name] = str(e)
            assert text in str(e), (name, str(e))
            return
        raise AssertionError(f"{name}: accepted")
    mk = lambda **kw: R.ReplayWindow(**dict(dict(game="TicTacToe", capacity_rows=10, seed=1, lib_path=lib_path), **kw)).close()      # noqa: E731
    refused("game", "unknown game", lambda: mk(game="Chess"))
    refused("capacity", "capacity_rows must be in [1, 2^31 - 1]", lambda: mk(capacity_rows=0))
    refused("test-fraction", "test_fraction must be in [0, 1)", lambda: mk(test_fraction=1.0))
    refused("test-fraction-nan", "test_fraction must be in [0, 1)", lambda: mk(test_fraction=float("nan")))
    refused("target-ratio", "target_ratio must be NaN (no balancing) or in [0, 1]", lambda: mk(target_ratio=1.5))
    refused("allocation", "allocation failure", lambda: mk(game="Gomoku", capacity_rows=2 ** 31 - 1))
    L = R.bind(load_library(lib_path))
    cfg = R.ReplayConfig(struct_size=C.sizeof(R.ReplayConfig) - 8, game=0, capacity_rows=10)
    h = C.c_void_p()
    assert L.gaz_replay_create(C.byref(cfg), C.byref(h)) != 0 and not h.value
    msgs["struct"] = L.gaz_replay_last_error(None).decode()
    assert "struct_size" in msgs["struct"] and str(C.sizeof(R.ReplayConfig)) in msgs["struct"]
    w = window("TicTacToe", 10, lib_path)
    rng = np.random.default_rng(0)
    refused("no-plan", "no plan", lambda: w.batch(0, 1))
    w.append_arrays(2, *random_rows(rng, "TicTacToe", [3, 4]))
    refused("no-plan-after-append", "no plan", lambda: w.sample(0, 1))
    refused("rows-not-ascending", "not ascending", lambda: w.append_arrays(2, np.array([[3, 0, 0, 0, 2, 0], [1, 0, 0, 0, 0, 0]], np.int32), *random_rows(rng, "TicTacToe", [3])[1:]))
    assert w.begin_epoch() == 7
    refused("beyond-the-plan", "of an epoch of 7 rows", lambda: w.batch(5, 3))
    refused("read-rows", "of 7 live rows", lambda: w.rows(5, 3))
    refused("split", "split must be 0 (train) or 1 (test)", lambda: w._ck(w.L.gaz_replay_begin_epoch(w.h, 2, 0, 2, 1.0, 0.0, None)))
    refused("epoch", "epoch must be below 2^30", lambda: w.begin_epoch(epoch=2 ** 30))
    refused("percent-nan", "must not be NaN", lambda: w.begin_epoch(percent=float("nan")))
    w.evict(3)
    refused("no-plan-after-evict", "no plan", lambda: w.plan() if w._plan else w.sample(0, 0))
    w.close()
    return msgs


# ------------------------------------------------------------------------------------------------ the sanitizer driver
def build_driver():
    """tests/emu/replay_main.cpp with the engine's host code and the one-lane build of its device code as ONE program under the address and
    undefined-behaviour sanitizers, the runtimes linked statically: run directly, on the CPU, never loaded into Python"""
    csrc, out = os.path.join(ROOT, "grok_alpha_zero_amd", "csrc"), os.path.join(EMU_DIR, "replay_asan")
    srcs = [os.path.join(csrc, "engine.hip"), os.path.join(EMU_DIR, "emu_stubs.cpp"), os.path.join(EMU_DIR, "replay_main.cpp")]
    deps = srcs + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")] + [os.path.join(ROOT, "include", "gaz_engine.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DGAZ_HOST_EMU", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-x", "c++"] + srcs + ["-o", out])
    return out


DRIVER_CASES = {"ttt": dict(game=0, capacity=100, seed=3), "c4": dict(game=1, capacity=61, seed=4), "gmk": dict(game=2, capacity=37, seed=5)}


def run_driver(driver, name):
    r = subprocess.run([driver] + [f"{k}={v}" for k, v in DRIVER_CASES[name].items()], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout + r.stderr

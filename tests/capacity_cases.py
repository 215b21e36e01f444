"""The engine at its capacity limits: the tree arena at exact fit and one node below it, the default arena sizing, set_hyperparams' check of
it, and the record ring under pressure.  The bodies take a lib_path: tests/test_capacity_emu.py runs them on the emulation build,
tests/test_capacity_gpu.py on the HIP build.  Every comparison is exact: a run is deterministic and independent of the capacities, so the
records of a tight engine are those of a roomy one, byte for byte, or there are none.

The "device error" of this module is the engine's own error word (include/gaz_engine.h "Capacity limits and the device error"): a defined,
recoverable return value.  Nothing here makes the device fault."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from selfplay_support import EMU_DIR, RECORD_KEYS, assert_records_equal, refusal_message

ARENA_FULL = "tree arena full (raise nodes_per_tree)"
ROOMY = 4096                                      # nodes per tree no case below comes near
DRIVER = os.path.join(EMU_DIR, "capacity_asan")

# name -> (game, slots, run_iterations, max_actions, games, search, the feature's keywords).  Sixteen slots are four wavefronts of four
# 16-lane teams: a game that fails shares its wavefront with three that go on.  Gomoku: one game per wavefront, the default compaction,
# run_iterations >= 226 so that the 3 x legal-moves floor of a move's limit does not apply
ARENA_CASES = {
    "c4-puct": ("Connect4", 16, 30, 42, 32, "puct", {}),
    "c4-compact": ("Connect4", 16, 30, 42, 32, "puct", dict(compact_trees=1)),
    "c4-leaf8": ("Connect4", 16, 30, 42, 32, "puct", dict(leaf_batch=8)),
    "c4-gumbel": ("Connect4", 16, 32, 42, 32, "gumbel", dict(gumbel_m=7)),
    "c4-gumbel-batch7": ("Connect4", 16, 32, 42, 32, "gumbel", dict(gumbel_m=7, gumbel_batch=7)),
    "c4-solver": ("Connect4", 16, 30, 42, 32, "puct", dict(solver=True)),
    "c4-symmetry": ("Connect4", 16, 30, 42, 32, "puct", dict(eval_symmetry=True)),
    "ttt-single": ("TicTacToe", 16, 50, 9, 32, "puct", dict(single_tree=True)),
    "gmk-compact": ("Gomoku", 3, 226, 6, 3, "puct", {}),
}
SEED, SALT = 3, 2
# Where the fullest tree of a run is that of a game's FIRST move, c* - 1 fails before any game has finished, whatever the seed: Gumbel builds a
# fresh tree per move and an opening move ends none of its simulations at a terminal position (c* = 1 root + 7 root children + 31 leaves);
# Gomoku with compaction keeps a subtree of one or two nodes, so every move needs its 226 expansions and the first one, from the empty board,
# wastes none (c* = 227).  There the witness "a game finished before the error" cannot hold; "a game was under way" stands in for it.
FIRST_MOVE_IS_FULLEST = ("c4-gumbel", "c4-gumbel-batch7", "gmk-compact")


def make(name, nodes_per_tree, lib_path, **more):
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL, SEARCH_PUCT, SelfPlayEngine
    game, G, R, max_actions, games, search, kw = ARENA_CASES[name]
    return SelfPlayEngine(game, G, R, max_actions, 2, 2, 2.5, 0.5, seed=SEED, hash_salt=SALT, ring_capacity=4 * G, games_budget=games,
                          search=SEARCH_GUMBEL if search == "gumbel" else SEARCH_PUCT, nodes_per_tree=nodes_per_tree, lib_path=lib_path,
                          **dict(kw, **more))


def raw_drain(eng, max_records=None):
    """gaz_engine_drain_finished without the binding's check -> (return code, the records it handed out): what a caller that ignored the
    return value would hold"""
    lay = eng.layout
    cap = max_records or max(eng.cfg.ring_capacity, 1)
    buf = np.zeros((cap, lay.record_bytes), np.uint8)
    n = C.c_int32()
    rc = eng.L.gaz_engine_drain_finished(eng.h, buf.ctypes.data, cap, C.byref(n))
    return rc, [eng.decode_record(buf[i]) for i in range(n.value)]


def play_all(eng, games, waves=32, rounds=40000):
    """a free-running engine until `games` records are there -> ({(slot, game_seq): record}, None), or until a call returns the engine's
    error -> (the records handed out by the calls that succeeded, the message)"""
    from grok_alpha_zero_amd.engine import EngineError
    out = {}
    try:
        for _ in range(rounds):
            eng.run_waves(waves)
            for r in eng.drain_finished():
                assert (r["slot"], r["game_seq"]) not in out, "a game arrived twice"
                out[(r["slot"], r["game_seq"])] = r
            if len(out) >= games:
                eng.synchronize()
                assert len(out) == games
                return out, None
    except EngineError as e:
        return out, str(e)
    raise AssertionError(f"only {len(out)} of {games} games finished")


_ROOMY, _CSTAR = {}, {}


def roomy_records(name, lib_path):
    """the reference of a case: its games in an arena of ROOMY nodes per tree (played once per library)"""
    if (name, lib_path) not in _ROOMY:
        eng = make(name, ROOMY, lib_path)
        recs, err = play_all(eng, ARENA_CASES[name][4])
        eng.close()
        assert err is None, err
        _ROOMY[(name, lib_path)] = recs
    return _ROOMY[(name, lib_path)]


def fits(name, nodes_per_tree, lib_path):
    eng = make(name, nodes_per_tree, lib_path)
    recs, err = play_all(eng, ARENA_CASES[name][4])
    eng.close()
    assert err is None or ARENA_FULL in err, err
    return err is None


def smallest_fit(name, emu_path):
    """c*: the smallest nodes_per_tree at which the case plays through, by bisection on the emulation build (fits() is monotone: the run
    does not depend on the capacity)"""
    if name not in _CSTAR:
        lo, hi = 1, ROOMY                              # lo fails, hi fits
        assert not fits(name, lo, emu_path)
        roomy_records(name, emu_path)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if fits(name, mid, emu_path):
                hi = mid
            else:
                lo = mid
        _CSTAR[name] = hi
    return _CSTAR[name]


def default_capacity(eng):
    """the nodes per tree an engine created with nodes_per_tree = 0 sized its arena for: set_hyperparams names it when it refuses"""
    msg = refusal_message(lambda: eng.set_hyperparams(run_iterations=1 << 20), "a million iterations were accepted")
    cap, need = (int(x) for x in re.search(r"\((\d+) nodes per tree, (\d+) needed\)", msg).groups())
    assert need > cap
    return cap


# ------------------------------------------------------------------------------------------------ 1. exact fit, and one node below it
def exact_fit_case(name, c_star, lib_path):
    """at c* every record equals the roomy run's in RECORD_KEYS, and c* lies below the engine's own default"""
    want = roomy_records(name, lib_path)
    eng = make(name, c_star, lib_path)
    got, err = play_all(eng, ARENA_CASES[name][4])
    eng.close()
    assert err is None, err
    assert sorted(got) == sorted(want)
    for k in want:
        assert_records_equal(got[k], want[k], f"{name} at c* = {c_star}, game {k}")
    dflt = make(name, 0, lib_path)
    cap = default_capacity(dflt)
    dflt.close()
    print(f"{name}: smallest fit c* = {c_star} nodes per tree, the engine's default {cap}", flush=True)
    assert c_star < cap, (c_star, cap)


def one_below_case(name, c_star, lib_path, extra_launches=64):
    """at c* - 1: the arena-full error, as too_small_case states it; where the fullest tree is not a first move's, a game had finished before it"""
    too_small_case(name, c_star - 1, lib_path, "c* - 1", name not in FIRST_MOVE_IS_FULLEST, extra_launches)


# Gumbel arenas that hold the root and only some of its m = 7 children: the game stops where it expands a root child, before any simulation
# (gumbel_core.hpp: stage 0 of PH_SIMS, and with gumbel_batch the chunk step's reservation).  At c* - 1 = 38 it stops in a descent instead.
# One node: the first child has no room.  Five: four children are in, and with gumbel_batch = 7 four rows are in flight when the fifth fails.
# (g_root_pre's own failure cannot be reached: it resets the tree to no nodes before it takes one, and an arena has at least one.)
ROOT_CHILD_CASES = {"c4-gumbel-1": ("c4-gumbel", 1), "c4-gumbel-5": ("c4-gumbel", 5),
                    "c4-gumbel-batch7-1": ("c4-gumbel-batch7", 1), "c4-gumbel-batch7-5": ("c4-gumbel-batch7", 5)}


def root_child_case(case, lib_path):
    name, nodes = ROOT_CHILD_CASES[case]
    failed, plies = too_small_case(name, nodes, lib_path, "root children only", False)
    assert len(failed) == ARENA_CASES[name][1] and set(plies) == {0}, (failed, plies)      # every game, at its first move


def too_small_case(name, nodes_per_tree, lib_path, what, finished_before, extra_launches=64):
    """an arena the case does not fit: the error comes back from the first synchronising call after the failing launch and from every later
    one, the games that raised it stay where they are, nothing that differs from the roomy run is ever handed out, and the process goes on
    with a fresh engine -> (the slots that stopped, the plies they stopped at)"""
    from grok_alpha_zero_amd.engine import PH_FAULT
    want = roomy_records(name, lib_path)
    games = ARENA_CASES[name][4]
    eng = make(name, nodes_per_tree, lib_path)
    G = eng.n_games
    got, launches, first = {}, 0, None

    def take(records, when):
        for r in records:
            k = (r["slot"], r["game_seq"])
            assert k in want and k not in got, (when, k)
            assert_records_equal(r, want[k], f"{name} at {what} = {nodes_per_tree}, {when}, game {k}")
            got[k] = r
    while first is None:
        assert launches < 200000 and len(got) < games, f"{what} = {nodes_per_tree} played through: the fit is not tight"
        eng.run_waves(1)
        launches += 1
        rc, records = raw_drain(eng)
        take(records, "before the error" if rc == 0 else "with the error")
        if rc:
            first = eng.L.gaz_engine_last_error(eng.h).decode()
    assert ARENA_FULL in first, first
    before = len(got)
    assert before < games, before                  # some game did not finish ...
    if finished_before:
        assert before >= 1, before                 # ... and some game had finished before the error

    def state():
        rs = eng.root_stats()
        return eng.read_positions(), rs
    pos0, rs0 = state()
    failed = [g for g in range(G) if rs0["phase"][g] == PH_FAULT]
    assert failed, rs0["phase"]
    eng.run_waves(extra_launches)
    for call in (eng.synchronize, eng.stats, eng.drain_finished, eng.synchronize):
        assert ARENA_FULL in refusal_message(call, f"{call.__name__} after the error succeeded")
    for _ in range(8):                             # what the ring still holds: games of slots that had not failed
        rc, records = raw_drain(eng)
        assert rc != 0
        take(records, "after the error")
        if not records:
            break
    pos1, rs1 = state()
    for g in failed:
        assert pos1[g] == pos0[g] and rs1["phase"][g] == PH_FAULT, (g, pos0[g], pos1[g], rs1["phase"][g])
        for k in ("N", "W", "P", "policy", "root_visits", "q", "chosen"):
            np.testing.assert_array_equal(rs1[k][g], rs0[k][g], err_msg=f"slot {g} {k}")
    running = {g: len(pos0[g]) for g in failed}
    assert len(got) < games
    eng.close()
    print(f"{name}: at {what} = {nodes_per_tree} the error came after {launches} launches, {before} of {games} games before it, {len(got)} in all; "
          f"slots {failed} stopped at plies {[running[g] for g in failed]} and stayed there for {extra_launches} launches", flush=True)
    fresh = make(name, ROOMY, lib_path)
    again, err = play_all(fresh, games)
    fresh.close()
    assert err is None and sorted(again) == sorted(want), err
    for k in want:
        assert_records_equal(again[k], want[k], f"{name}, a fresh engine after the error, game {k}")
    return failed, [running[g] for g in failed]


# ------------------------------------------------------------------------------------------------ 2. the sanitizer driver (CPU only)
def build_driver():
    subprocess.check_call(["make", "-s", "-C", EMU_DIR, "capacity_asan"])
    return DRIVER


def driver_args(name, nodes_per_tree, extra_launches=64):
    game, G, R, max_actions, games, search, kw = ARENA_CASES[name]
    a = dict(game=game, search=search, n_games=G, run_iterations=R, max_actions=max_actions, games_budget=games, seed=SEED, hash_salt=SALT,
             nodes_per_tree=nodes_per_tree, extra_launches=extra_launches)
    a.update({k: int(v) for k, v in kw.items()})
    return [f"{k}={v}" for k, v in a.items()]


def run_driver(name, nodes_per_tree, extra_launches=64):
    """the stand-alone program on one configuration -> (exit status, output).  The sanitizer runtimes are linked into the program statically
    (tests/emu/Makefile): it is started in the caller's environment as it is, and nothing is preloaded for it"""
    r = subprocess.run([DRIVER] + driver_args(name, nodes_per_tree, extra_launches), capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------ 4. the default sizing is enough
# name -> (game, slots, run_iterations, max_actions, games, search, keywords): nodes_per_tree = 0, games >= 3 x slots
DEFAULT_CASES = {
    "c4": ("Connect4", 8, 30, 42, 24, "puct", {}),
    "c4-iterations3": ("Connect4", 8, 3, 42, 24, "puct", {}),
    "c4-leaf16": ("Connect4", 8, 30, 42, 24, "puct", dict(leaf_batch=16)),
    "c4-leaf16-200": ("Connect4", 4, 200, 42, 12, "puct", dict(leaf_batch=16)),
    "c4-solver": ("Connect4", 8, 30, 42, 24, "puct", dict(solver=True)),
    "c4-forced": ("Connect4", 8, 30, 42, 24, "puct", dict(forced_playouts_k=2.0)),
    "c4-playout-cap": ("Connect4", 8, 30, 42, 24, "puct", dict(fast_iterations=6, full_search_prob=0.25)),
    "c4-new-root": ("Connect4", 8, 30, 42, 24, "puct", dict(create_new_root=True)),
    "c4-compact": ("Connect4", 8, 30, 42, 24, "puct", dict(compact_trees=1)),
    "c4-compact-leaf16": ("Connect4", 8, 30, 42, 24, "puct", dict(compact_trees=1, leaf_batch=16)),
    "c4-single": ("Connect4", 8, 30, 42, 48, "puct", dict(single_tree=True)),      # (its first game of 42 plies is the 45th)
    "ttt-single": ("TicTacToe", 8, 50, 9, 24, "puct", dict(single_tree=True)),
    "c4-gumbel": ("Connect4", 8, 32, 42, 24, "gumbel", dict(gumbel_m=7)),
    "c4-gumbel-batch7": ("Connect4", 8, 32, 42, 24, "gumbel", dict(gumbel_m=7, gumbel_batch=7)),
    "gmk": ("Gomoku", 4, 226, 5, 12, "puct", {}),
    "gmk-whole-game": ("Gomoku", 4, 226, 5, 12, "puct", dict(compact_trees=-1)),
    "gmk-leaf8": ("Gomoku", 4, 226, 5, 12, "puct", dict(leaf_batch=8)),
}


def make_default(name, lib_path, **more):
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL, SEARCH_PUCT, SelfPlayEngine
    game, G, R, max_actions, games, search, kw = DEFAULT_CASES[name]
    return SelfPlayEngine(game, G, R, max_actions, 2, 2, 2.5, 0.5, seed=SEED, hash_salt=SALT, ring_capacity=4 * G, games_budget=games,
                          search=SEARCH_GUMBEL if search == "gumbel" else SEARCH_PUCT, lib_path=lib_path, **dict(kw, **more))


def default_sizing_case(name, lib_path):
    """the arena the engine sizes itself holds every game, those of the full length included"""
    games, max_actions = DEFAULT_CASES[name][4], DEFAULT_CASES[name][3]
    eng = make_default(name, lib_path)
    recs, err = play_all(eng, games)
    eng.close()
    assert err is None, f"{name} at the default arena, after {len(recs)} of {games} games: {err}"
    longest = max(r["T"] for r in recs.values())
    assert longest == max_actions, (name, longest, max_actions)      # a game of the full length was among them


def hyperparams_boundary_case(lib_path):
    """set_hyperparams holds run_iterations and gumbel_m against the arena that was sized at create time: the largest value the arena was
    sized for is accepted and plays full-length games, one more is refused with both numbers; with an explicit nodes_per_tree every value is
    accepted, and running past the arena is the arena-full error"""
    # PUCT, created at 3 iterations: a move runs at least 3 x 7 simulations, so the arena holds 21 a move and no more
    eng = make_default("c4-iterations3", lib_path)
    cap = default_capacity(eng)
    eng.set_hyperparams(run_iterations=21)
    msg = refusal_message(lambda: eng.set_hyperparams(run_iterations=22), "22 iterations were accepted")
    assert f"({cap} nodes per tree, " in msg and int(re.search(r", (\d+) needed", msg).group(1)) > cap, msg
    recs, err = play_all(eng, DEFAULT_CASES["c4-iterations3"][4])
    eng.close()
    assert err is None and max(r["T"] for r in recs.values()) == 42, err
    assert all((r["root_visits"][r["evals"] > 1] >= 21).any() for r in recs.values())           # the games really ran at 21
    # Gumbel: its own m and iterations are accepted, one more of either is refused
    eng = make_default("c4-gumbel", lib_path)
    cap = default_capacity(eng)
    eng.set_hyperparams(m=7, run_iterations=32)
    for kw in (dict(m=8), dict(run_iterations=33)):
        msg = refusal_message(lambda: eng.set_hyperparams(**kw), f"{kw} was accepted")
        assert f"({cap} nodes per tree, " in msg and int(re.search(r", (\d+) needed", msg).group(1)) > cap, msg
    recs, err = play_all(eng, DEFAULT_CASES["c4-gumbel"][4])
    eng.close()
    assert err is None and max(r["T"] for r in recs.values()) == 42, err
    # an explicit nodes_per_tree: accepted as documented; the arena of 600 nodes holds games at 30 iterations, not at 200
    def at_200(npt):
        e = make("c4-puct", npt, lib_path)
        e.set_hyperparams(run_iterations=200)
        out = play_all(e, ARENA_CASES["c4-puct"][4])
        e.close()
        return out
    want, err = at_200(16384)
    assert err is None, err
    got, err = at_200(600)
    assert err is not None and ARENA_FULL in err, err
    for k in got:
        assert_records_equal(got[k], want[k], f"600 nodes at 200 iterations, game {k}")


# ------------------------------------------------------------------------------------------------ 5. the record ring under pressure
RING_CASES = {"ring1-drain1": (1, 1, {}), "ring2-drain1": (2, 1, {}), "ring3-drain2": (3, 2, {}), "ring5-drain5": (5, 5, {}),
              "ring3-groups2": (3, 2, dict(game_groups=2))}
RING_G, RING_GAMES, RING_LAUNCHES = 64, 256, 8


def ring_engine(lib_path, ring_capacity, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    return SelfPlayEngine("TicTacToe", RING_G, 12, 9, 2, 2, 2.5, 0.5, seed=SEED, hash_salt=SALT, ring_capacity=ring_capacity, games_budget=RING_GAMES,
                          lib_path=lib_path, **kw)


def drain_rounds(eng, games, take, launches=RING_LAUNCHES, rounds=200000):
    """`launches` launches, then one drain of at most `take` records, until `games` records are there -> ({key: record}, drain rounds)"""
    out = {}
    for n in range(1, rounds + 1):
        eng.run_waves(launches)
        for r in eng.drain_finished(max_records=take):
            assert (r["slot"], r["game_seq"]) not in out, "a game arrived twice"
            out[(r["slot"], r["game_seq"])] = r
        if len(out) >= games:
            return out, n
    raise AssertionError(f"only {len(out)} of {games} games arrived")


_RING_ROOMY = {}


def ring_roomy(lib_path, **kw):
    key = (lib_path, tuple(sorted(kw.items())))
    if key not in _RING_ROOMY:
        eng = ring_engine(lib_path, RING_GAMES, **kw)
        recs, rounds = drain_rounds(eng, RING_GAMES, RING_GAMES)
        st = eng.stats()
        eng.close()
        _RING_ROOMY[key] = (recs, rounds, st)
    return _RING_ROOMY[key]


def assert_tight_equals_roomy(got, rounds, st, want, rounds_roomy, st_roomy, what):
    assert sorted(got) == sorted(want), what                        # every (slot, game_seq), once
    for k in want:
        assert_records_equal(got[k], want[k], f"{what}, game {k}")
    np.testing.assert_array_equal(st["game_stats"], st_roomy["game_stats"], err_msg=what)      # counted once, not once per retry
    for k in ("evals", "sims", "plies"):
        assert st[k] == st_roomy[k], (what, k, st[k], st_roomy[k])
    print(f"{what}: {len(got)} games equal the roomy ring's, {rounds} drain rounds against {rounds_roomy}", flush=True)
    assert rounds > rounds_roomy, (what, rounds, rounds_roomy)       # games really waited for room


def ring_case(name, lib_path):
    cap, take, kw = RING_CASES[name]
    want, rounds_roomy, st_roomy = ring_roomy(lib_path, **kw)
    eng = ring_engine(lib_path, cap, **kw)
    if kw.get("game_groups"):
        assert eng.stats()["game_groups"] == kw["game_groups"]
    got, rounds = drain_rounds(eng, RING_GAMES, take)
    st = eng.stats()
    eng.close()
    assert_tight_equals_roomy(got, rounds, st, want, rounds_roomy, st_roomy, f"{name} (ring_capacity {cap}, {take} a drain)")


def ring_samples_case(lib_path, G=64, launches=32):
    """Connect4, a ring of 2 from which one game is taken every 32 launches: gaz_engine_drain_samples hands out the samples of the roomy run's
    games, each game once"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    from grok_alpha_zero_amd.games import GAMES
    from samples_util import assert_same_game, device_games, host_games

    def engine(ring):
        return SelfPlayEngine("Connect4", G, 12, 42, 2, 2, 2.5, 0.5, seed=SEED, hash_salt=SALT, ring_capacity=ring, games_budget=G, lib_path=lib_path)
    roomy = engine(4 * G)
    host, rounds_roomy = {}, 0
    while len(host) < G:
        roomy.run_waves(launches); rounds_roomy += 1
        host.update({g[0]: g for g in host_games(roomy, GAMES["Connect4"])})
        assert rounds_roomy < 100000
    st_roomy = roomy.stats()
    roomy.close()
    tight = engine(2)
    dev, rounds = {}, 0
    while len(dev) < G:
        tight.run_waves(launches); rounds += 1
        for g in device_games(tight, max_games=1):
            assert g[0] not in dev, "a game arrived twice"
            dev[g[0]] = g
        assert rounds < 100000
    st = tight.stats()
    tight.close()
    assert sorted(dev) == sorted(host)
    for k in host:
        assert_same_game(dev[k], host[k], "ring of 2")
    np.testing.assert_array_equal(st["game_stats"], st_roomy["game_stats"])
    print(f"drain_samples from a ring of 2: {G} games equal the roomy ring's, {rounds} drain rounds against {rounds_roomy}", flush=True)
    assert rounds > rounds_roomy


# ------------------------------------------------------------------------------------------------ the 1-block network (HIP build only)
NET_G = 64


def net_arena_case(fused):
    """64 Connect4 games with the 1-block network in an arena of three moves' worth of nodes: every game raises the error a few moves in.
    The call returns it — in the one-launch wave the trunk workgroups are not left waiting for a game that has stopped"""
    from grok_alpha_zero_amd.engine import PH_FAULT
    from selfplay_support import c4_one_block_weights, net_engine
    eng = net_engine(NET_G, c4_one_block_weights(), fused, seed=SEED, nodes_per_tree=3 * 42, game_groups=1)
    recs, err = play_all(eng, NET_G, waves=8)
    assert err is not None and ARENA_FULL in err, (len(recs), err)
    out = (C.c_uint64 * 16)()
    assert eng.L.gaz_engine_get_stats(eng.h, out) != 0          # the outputs are filled before the error is returned
    print(f"fused_wave {int(out[12])} fused_faults {int(out[13])}, {len(recs)} games before the error", flush=True)
    assert int(out[12]) == (1 if fused else 0) and int(out[13]) == 0, (int(out[12]), int(out[13]))
    pos0, ph0 = eng.read_positions(), eng.root_stats()["phase"]
    failed = [g for g in range(NET_G) if ph0[g] == PH_FAULT]
    assert failed
    eng.run_waves(64)
    assert ARENA_FULL in refusal_message(eng.synchronize, "synchronize after the error succeeded")
    pos1, ph1 = eng.read_positions(), eng.root_stats()["phase"]
    for g in failed:
        assert pos1[g] == pos0[g] and ph1[g] == PH_FAULT, g
    assert eng.L.gaz_engine_get_stats(eng.h, out) != 0 and int(out[13]) == 0, int(out[13])
    eng.close()
    print(f"{len(failed)} games stopped and stayed stopped for 64 launches", flush=True)


def net_ring_case():
    """the 1-block network in the one-launch wave with a ring of 3, two records taken every 64 launches (the 64 games last some 1300
    launches, so the roomy ring is empty after about 20 rounds and the tight one after no fewer than 32): many teams finish in one launch
    and race for ring_head"""
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
    from selfplay_support import c4_one_block_weights
    w = c4_one_block_weights()

    def run(ring, take):
        eng = SelfPlayEngine("Connect4", NET_G, 40, 42, 4, 4, 2.5, 0.5, evaluator=EVAL_RESNET, net_blocks=1, ring_capacity=ring, games_budget=NET_G,
                             seed=SEED, game_groups=1)
        eng.load_weights(w)
        recs, rounds = drain_rounds(eng, NET_G, take, launches=64)
        st = eng.stats()
        eng.close()
        assert st["fused_wave"] == 1 and st["fused_faults"] == 0, st
        return recs, rounds, st
    want, rounds_roomy, st_roomy = run(4 * NET_G, 4 * NET_G)
    got, rounds, st = run(3, 2)
    assert_tight_equals_roomy(got, rounds, st, want, rounds_roomy, st_roomy, "1-block network, one-launch wave, ring_capacity 3")

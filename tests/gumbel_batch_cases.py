"""The cases of the batched sequential halving (gaz_engine_config.gumbel_batch = K) that the CPU suite runs on the emulation build
(tests/test_gumbel_batch_emu.py) and the -m gpu suite on the HIP build (tests/test_gumbel_batch_gpu.py): `lib_path` = the emulation
library, or None for the product library.  The yardsticks are the reference's own fixtures and the oracle, unchanged; every comparison is
assert_array_equal."""
import glob
import json
import os

import numpy as np

from selfplay_support import MAXT, first_games

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
GUMBEL_FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*_gumbel_*.npz")))
CLASS_FIXTURES = ["c4_gsingle_nonoise", "ttt_gsingle_nonoise", "c4_gsingle_update"]
RECORD_KEYS = ("actions", "root_N", "root_W", "root_P", "root_visits", "policies", "values", "q", "evals")
PH_WAIT_HOST = 5


def fixture(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def assert_matches_fixture(r, fx):
    """the checks of tests/test_engine_emu.py assert_matches_fixture"""
    assert r["T"] == len(fx["actions"])
    for k in ("actions", "root_N", "root_visits", "root_W", "root_P", "policies"):
        np.testing.assert_array_equal(r[k], fx[k], err_msg=k)
    np.testing.assert_array_equal(np.asarray(r["values"]).reshape(-1), fx["values"].reshape(-1))
    gs = fx["game_stats"]
    assert gs[r["winner"] + 4] == 1 and gs[1] == r["T"]


def assert_record_equals_oracle(r, o, what=""):
    assert (r["T"], r["winner"]) == (o["T"], o["winner"]), (what, r["T"], o["T"], r["winner"], o["winner"])
    for k in RECORD_KEYS:
        np.testing.assert_array_equal(np.asarray(r[k]).reshape(np.asarray(o[k]).shape), o[k], err_msg=f"{what} {k}")


# ------------------------------------------------------------------------------------------------ 1. the reference's fixtures
def play_gumbel_fixture(fx, K, lib_path):
    from grok_alpha_zero_amd.engine import SelfPlayEngine, SEARCH_GUMBEL
    eng = SelfPlayEngine(str(fx["game"]), 1, int(fx["run_iterations"]), int(fx["max_actions"]), 0, 0, 0.0, 0.0, int(fx["seed"]),
                         slot_offset=int(fx["slot"]), hash_salt=int(fx["salt"]), ring_capacity=8, search=SEARCH_GUMBEL,
                         gumbel_m=int(fx["m"]), c_visit=float(fx["c_visit"]), c_scale=float(fx["c_scale"]),
                         gumbel_stablemax=bool(int(fx["stablemax"])) if "stablemax" in fx else False, first_game_seq=int(fx["game_seq"]),
                         gumbel_batch=K, lib_path=lib_path)
    assert eng.batch_rows == max(K, 1)
    r = first_games(eng, 1, waves=64, rounds=20000)[int(fx["slot"])]
    eng.close()
    return r


def fixture_case(name, K, lib_path):
    fx = fixture(name)
    assert_matches_fixture(play_gumbel_fixture(fx, int(fx["m"]) if K == "m" else K, lib_path), fx)


def net_fixture_case(lib_path, K=7):
    """c4_netg_a (the reference's Self_Play.play() with a real network behind session.run) through GAZ_EVAL_EXTERNAL, as
    tests/test_net_fixtures.py drives it — with K rows per game, of which slot 0's are answered from the fixture's table"""
    from grok_alpha_zero_amd.engine import EVAL_EXTERNAL, SEARCH_GUMBEL, SelfPlayEngine
    fx = fixture("c4_netg_a")
    G = 3
    eng = SelfPlayEngine(str(fx["game"]), G, int(fx["run_iterations"]), int(fx["max_actions"]), int(fx["explore_first"]), int(fx["explore_second"]),
                         float(fx["c_puct_init"]), float(fx["dirichlet_alpha"]), int(fx["seed"]), slot_offset=int(fx["slot"]),
                         evaluator=EVAL_EXTERNAL, ring_capacity=16, search=SEARCH_GUMBEL, gumbel_m=int(fx["m"]), c_visit=float(fx["c_visit"]),
                         c_scale=float(fx["c_scale"]), first_game_seq=int(fx["game_seq"]), games_budget=G, gumbel_batch=K, lib_path=lib_path)
    assert eng.batch_rows == G * K
    tab = {s.tobytes(): (p, v) for s, p, v in zip(fx["eval_states"], fx["eval_policy"], fx["eval_value"])}
    A = fx["eval_policy"].shape[1]
    uniform = np.full(A, 1.0 / A, np.float32)
    n_lookups, rec, widest = 0, None, 0
    for _ in range(200000):
        eng.wave_begin()
        x, pend = eng.read_batch()
        pol = np.full((G * K, A), np.nan, np.float32); val = np.full(G * K, np.nan, np.float32)     # a row nobody asked for is never read
        for row in np.flatnonzero(pend):
            if row < K and rec is None:
                pol[row], val[row] = tab[x[row].tobytes()]; n_lookups += 1
            else:
                pol[row] = uniform; val[row] = 0.0
        widest = max(widest, int(np.count_nonzero(pend[:K])))
        eng.write_outputs(pol, val)
        for r in eng.drain_finished():
            if r["slot"] == int(fx["slot"]) and r["game_seq"] == int(fx["game_seq"]) and rec is None:
                rec = r
        if rec is not None:
            break
    eng.close()
    assert rec is not None and n_lookups == int(fx["evaluator_calls"]) and widest > 1
    assert rec["T"] == len(fx["actions"])
    for k in ("actions", "root_N", "root_visits", "root_W", "root_P", "policies"):
        np.testing.assert_array_equal(rec[k], fx[k], err_msg=k)
    np.testing.assert_array_equal(np.asarray(rec["values"]).reshape(-1), fx["values"].reshape(-1))


# ------------------------------------------------------------------------------------------------ 3. concurrent games against the oracle
# name -> game, run_iterations, max_actions, m, K, stablemax, gumbel noise
CONCURRENT = {
    "c4-k7": ("Connect4", 32, 42, 7, 7, False, True), "c4-k2": ("Connect4", 32, 42, 7, 2, False, True),
    "ttt-k4": ("TicTacToe", 16, 9, 4, 4, False, True),
    "gmk-k16": ("Gomoku", 48, 8, 16, 16, False, True), "gmk-k5": ("Gomoku", 48, 8, 16, 5, False, True),
    "c4-k7-stablemax": ("Connect4", 32, 42, 7, 7, True, True), "ttt-k4-nonoise": ("TicTacToe", 16, 9, 4, 4, False, False),
}


def concurrent_case(oracle, name, G, lib_path, seed=23, salt=6, **kw):
    """G games at once, free-running, hash evaluator: the first game of EVERY slot is the oracle's selfplay_game_gumbel"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, SEARCH_GUMBEL
    game, iters, max_actions, m, K, stablemax, noise = CONCURRENT[name]
    eng = SelfPlayEngine(game, G, iters, max_actions, 0, 0, 0.0, 0.0, seed=seed, hash_salt=salt, ring_capacity=4 * G, search=SEARCH_GUMBEL, gumbel_m=m,
                         c_visit=50.0, c_scale=1.0, gumbel_stablemax=stablemax, use_gumbel_noise=noise, gumbel_batch=K, lib_path=lib_path, **kw)
    assert eng.batch_rows == G * K and eng.stats()["fused_wave"] == 0 and eng.stats()["game_groups"] == 1
    first = first_games(eng, G, waves=32, rounds=20000)
    eng.close()
    for slot in range(G):
        o = oracle.selfplay_game_gumbel(game, iters, max_actions, m, 50.0, 1.0, seed, slot, 0, hash_salt=salt, stablemax=stablemax, gumbel_noise=noise)
        assert_record_equals_oracle(first[slot], o, f"{name} slot {slot}")
    return first


# ------------------------------------------------------------------------------------------------ 5. launch counts
def vpc_schedule(n, m):
    """(candidates, visits per candidate) of every sequential-halving phase from a position with at least m legal moves, when every
    visit is an iteration (MCTS_Gumbel.py:212-224, 603-623)"""
    out, it, phase, take = [], 0, 0, m
    while take > 1:
        halved = max(m / 2 ** phase, 1.0)
        vpc = max(int(n / (np.log2(m) * halved)), 1)
        if take in (2, 3):
            vpc = max((n - it) // take, 1)
        out.append((take, vpc)); it += take * vpc
        phase += 1
        take = min(int(max(m / 2 ** phase, 1.0)), take)
    return out


def launches_of_first_move(game, iters, m, K, lib_path):
    """sync mode, one game from the empty board: launches from start_search until the game waits for the host, and its evaluator calls"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, SEARCH_GUMBEL
    eng = SelfPlayEngine(game, 1, iters, MAXT[game], 0, 0, 0.0, 0.0, seed=3, hash_salt=5, sync_moves=True, single_tree=True, search=SEARCH_GUMBEL,
                         gumbel_m=m, c_visit=50.0, c_scale=1.0, max_tree_sims_per_wave=64, gumbel_batch=K, lib_path=lib_path)
    eng.set_position(0, [])
    eng.start_search()
    for n in range(1, 2000):
        eng.run_waves(1)
        if eng.root_stats()["phase"][0] == PH_WAIT_HOST:
            break
    st, evals = eng.root_stats(), eng.stats()["evals"]
    eng.close()
    return n, evals, st


def launch_bound_case(game, iters, m, K, bound, lib_path):
    sched = vpc_schedule(iters, m)
    assert 2 + sum(1 + v for _, v in sched) == bound, sched
    n1, e1, s1 = launches_of_first_move(game, iters, m, 1, lib_path)
    nk, ek, sk = launches_of_first_move(game, iters, m, K, lib_path)
    print(f"{game} n {iters} m {m}: {n1} launches at gumbel_batch 1, {nk} at {K} (bound {bound}); {e1} evaluator calls", flush=True)
    assert nk <= bound < n1 and ek == e1
    for k in ("N", "W", "P", "policy", "root_visits", "q", "chosen"):
        np.testing.assert_array_equal(sk[k], s1[k], err_msg=k)


# ------------------------------------------------------------------------------------------------ 7. the MCTS_Gumbel class
class CountingSession:
    def __init__(self, oracle, A, salt):
        self.oracle, self.A, self.salt, self.batches = oracle, A, salt, []

    def run(self, output_names, input_feed, **kw):
        x = input_feed["inputs"]
        assert x.ndim == 4 and x.dtype == np.float32 and output_names == ["policy", "value"]
        self.batches.append(x.shape[0])
        out = [self.oracle.hash_eval(r.astype(np.int8), self.A, self.salt) for r in x]
        return np.stack([p for p, _ in out]), np.array([[v] for _, v in out], np.float32)


def class_case(oracle, name, lib_path, K=4):
    """the driver of tests/test_mcts_classes.py (_drive_gumbel_fixture) with MCTS_Gumbel(gumbel_batch=K) and a session that takes batches"""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.mcts import MCTS_Gumbel
    fx = fixture(name)
    game = GAMES[str(fx["game"])]()
    A = game.policy_shape[0]
    sess = CountingSession(oracle, A, int(fx["salt"]))
    mcts = MCTS_Gumbel(game, sess, use_gumbel_noise=bool(int(fx["use_gumbel_noise"])), m=int(fx["m"]), c_visit=float(fx["c_visit"]),
                       c_scale=float(fx["c_scale"]), seed=int(fx["seed"]), gumbel_batch=K, lib_path=lib_path)
    assert mcts._eng.batch_rows == K
    updates = {int(k): v for k, v in json.loads(str(fx["update_json"])).items()}
    for ply in range(len(fx["actions"])):
        if ply in updates:
            mcts.update_hyperparams(**updates[ply])
        move, rows = mcts.run(iteration_limit=int(fx["iteration_limit"]), use_bar=False)
        pol = np.zeros(A, np.float32); N = np.zeros(A, np.uint32); Wv = np.zeros(A, np.float32); P = np.zeros(A, np.float32)
        for r in rows:
            a = type(game).action_to_index(r[0]); pol[a] = r[1]; N[a] = r[4]; Wv[a] = r[3]; P[a] = r[5]
        for k, v in (("root_N", N), ("root_W", Wv), ("root_P", P), ("policies", pol)):
            np.testing.assert_array_equal(v, fx[k][ply], err_msg=f"{k} ply {ply}")
        assert type(game).action_to_index(move) == fx["actions"][ply]
        game.do_action(move)
        if game.check_win() != -2:
            break
        mcts.prune_tree(move)
    assert ply == len(fx["actions"]) - 1
    assert max(sess.batches) > 1 and sum(sess.batches) == int(fx["evaluator_calls"]) == mcts._eng.stats()["evals"]
    mcts.close()


# ------------------------------------------------------------------------------------------------ the ResNet evaluator (HIP build)
RESNET = {   # name -> game, blocks, G, run_iterations, m, K, max_actions
    "resnet-c4": ("Connect4", 6, 16, 32, 7, 7, 6),
    "resnet-gmk": ("Gomoku", 10, 2, 48, 16, 16, 4),
}


def resnet_case(name, lib_path=None):
    """the network behind the search: every slot's first game with gumbel_batch = K against an engine with gumbel_batch = 1, the same
    weights and the same seed — the code path as it was before gumbel_batch existed.  Every field of the records."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET, SEARCH_GUMBEL
    from grok_alpha_zero_amd.net import NETS
    game, blocks, G, iters, m, K, max_actions = RESNET[name]
    w = NETS[game](blocks, seed=0).eval().export_engine_weights()
    recs = {}
    for k in (1, K):
        eng = SelfPlayEngine(game, G, iters, max_actions, 0, 0, 0.0, 0.0, seed=5, evaluator=EVAL_RESNET, net_blocks=blocks, net_filters=128, policy_is_logits=1,
                             ring_capacity=4 * G, games_budget=G, search=SEARCH_GUMBEL, gumbel_m=m, c_visit=50.0, c_scale=1.0, gumbel_batch=k, lib_path=lib_path)
        eng.load_weights(w)
        assert eng.batch_rows == G * k
        recs[k] = first_games(eng, G, waves=16, rounds=20000)
        print(f"{name}: gumbel_batch {k}: {eng.stats()['waves']} waves, {eng.stats()['evals']} evaluator calls", flush=True)
        eng.close()
    for slot in range(G):
        a, b = recs[1][slot], recs[K][slot]
        assert set(a) == set(b)
        for key, v in a.items():
            np.testing.assert_array_equal(b[key], v, err_msg=f"{name} slot {slot} {key}")

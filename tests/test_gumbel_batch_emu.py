"""CPU suite: batched sequential halving (gaz_engine_config.gumbel_batch = K — the candidates of one halving phase of the Gumbel search
in one evaluator batch) on the emulation build of the device code.  The search does not change, so the yardsticks are the reference's own
fixtures and the oracle, unchanged, and every comparison is bit for bit (tests/gumbel_batch_cases.py)."""
import numpy as np
import pytest

import gumbel_batch_cases as GB
from selfplay_support import emu_lib  # noqa: F401


# ------------------------------------------------------------------------------------------------ 1. the reference's fixtures
@pytest.mark.parametrize("K", ["m", 3])
@pytest.mark.parametrize("name", GB.GUMBEL_FIXTURES)
def test_reference_fixture(emu_lib, name, K):
    """K = the fixture's m: one chunk per phase; K = 3: a last chunk shorter than K for m = 4, 7, 16"""
    GB.fixture_case(name, K, emu_lib)


def test_reference_fixture_with_a_real_network_external_evaluator(emu_lib):
    GB.net_fixture_case(emu_lib, K=7)


# ------------------------------------------------------------------------------------------------ 2. gumbel_batch 0 / 1 = the default path
def test_gumbel_batch_0_and_1_are_the_default_path(emu_lib):
    import ctypes as C
    from grok_alpha_zero_amd.engine import SelfPlayEngine, SEARCH_GUMBEL

    def play(**kw):
        eng = SelfPlayEngine("Connect4", 8, 32, 42, 0, 0, 0.0, 0.0, seed=9, hash_salt=3, ring_capacity=16, games_budget=8, search=SEARCH_GUMBEL, gumbel_m=7,
                             c_visit=50.0, c_scale=1.0, lib_path=emu_lib, **kw)
        assert eng.batch_rows == 8
        raw = []
        for _ in range(4000):
            eng.run_waves(32)
            buf = np.zeros((16, eng.layout.record_bytes), np.uint8)
            n = C.c_int32()
            eng._ck(eng.L.gaz_engine_drain_finished(eng.h, buf.ctypes.data, 16, C.byref(n)))
            raw += [buf[i].tobytes() for i in range(n.value)]
            if len(raw) == 8:
                break
        waves = eng.stats()["waves"]
        eng.close()
        assert len(raw) == 8
        return sorted(raw), waves
    a, wa = play()
    b, wb = play(gumbel_batch=1)
    c, wc = play(gumbel_batch=0)
    assert a == b == c and wa == wb == wc


# ------------------------------------------------------------------------------------------------ 3. concurrent games, every slot
@pytest.mark.parametrize("name", sorted(GB.CONCURRENT))
def test_concurrent_games_equal_oracle(emu_lib, oracle, name):
    GB.concurrent_case(oracle, name, 3 if name.startswith("gmk") else 20, emu_lib)


# ------------------------------------------------------------------------------------------------ 4. max_tree_sims_per_wave: scheduling only
def test_max_tree_sims_per_wave_is_scheduling_only(emu_lib, oracle):
    recs = [GB.concurrent_case(oracle, "c4-k7", 6, emu_lib, max_tree_sims_per_wave=cap) for cap in (1, 4, 64)]
    for other in recs[1:]:
        for slot in range(6):
            assert set(recs[0][slot]) == set(other[slot])
            for k, v in recs[0][slot].items():
                np.testing.assert_array_equal(v, other[slot][k], err_msg=k)


# ------------------------------------------------------------------------------------------------ 5. launch counts
@pytest.mark.parametrize("game,iters,m,K,bound", [("Connect4", 32, 7, 7, 13), ("Gomoku", 64, 16, 16, 21)])
def test_first_move_launch_count(emu_lib, game, iters, m, K, bound):
    """at most 2 + sum over phases of (1 + vpc) launches: the root's evaluation and the move's last launch, and per phase one launch that
    expands the candidates' root children plus one per visit — with the evaluator calls of gumbel_batch = 1"""
    GB.launch_bound_case(game, iters, m, K, bound, emu_lib)


# ------------------------------------------------------------------------------------------------ 6. sparse pending rows
def _drive_external(eng, oracle, A, salt):
    """one move of a sync + single-tree engine with the external evaluator; rows nobody asked for get NaN outputs.
    -> per launch (rows flagged, their states)"""
    from grok_alpha_zero_amd.engine import PH_HALT
    eng.start_search()
    launches = []
    for _ in range(10000):
        eng.wave_begin()
        x, pend = eng.read_batch()
        rows = np.flatnonzero(pend)
        if rows.size == 0 and eng.root_stats()["phase"][0] in (GB.PH_WAIT_HOST, PH_HALT):
            return launches
        launches.append((rows.tolist(), [x[r].copy() for r in rows]))
        pol = np.full((eng.batch_rows, A), np.nan, np.float32); val = np.full(eng.batch_rows, np.nan, np.float32)
        for r in rows:
            pol[r], val[r] = oracle.hash_eval(x[r], A, salt)
        eng.write_outputs(pol, val)
    raise AssertionError("search did not finish")


def test_read_batch_flags_exactly_the_rows_with_a_request(emu_lib, oracle):
    """Connect4 after 3 0 3 0 3: the side to move must answer three in column 3.  Every root child but the block is a position with a win
    in one — a terminal parent, expanded and visited without the network — so in every launch of the first phase only the block's row
    carries a request, and it is not row 0.  A row flagged without a request would be an extra evaluator call, a request not flagged would
    consume NaN: the requested states are those of gumbel_batch = 1, the result the oracle's."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_EXTERNAL, SEARCH_GUMBEL
    history, iters, m, seed, salt = [3, 0, 3, 0, 3], 32, 7, 2, 9
    got = {}
    for K in (1, 7):
        eng = SelfPlayEngine("Connect4", 1, iters, 42, 0, 0, 0.0, 0.0, seed=seed, sync_moves=True, single_tree=True, evaluator=EVAL_EXTERNAL,
                             search=SEARCH_GUMBEL, gumbel_m=m, c_visit=50.0, c_scale=1.0, gumbel_batch=K, lib_path=emu_lib)
        eng.set_position(0, history)
        got[K] = (_drive_external(eng, oracle, 7, salt), eng.root_stats(), eng.stats()["evals"])
        eng.close()
    (l1, s1, e1), (l7, s7, e7) = got[1], got[7]
    assert all(rows in ([0], []) for rows, _ in l1)          # (a launch may end on its allowance of evaluation-free visits: no request)
    assert any(rows and min(rows) > 0 for rows, _ in l7), "no launch with an idle row below a waiting one"
    assert all(len(set(rows)) == len(rows) and all(0 <= r < 7 for r in rows) for rows, _ in l7)
    states1 = sorted(s.tobytes() for _, ss in l1 for s in ss)
    states7 = sorted(s.tobytes() for _, ss in l7 for s in ss)
    assert states1 == states7 and e1 == e7 == len(states7) and len(l7) < len(l1)
    o = oracle.selfplay_game_gumbel("Connect4", iters, 42, m, 50.0, 1.0, seed, 0, 0, hash_salt=salt, start_history=history)
    for st in (s1, s7):
        np.testing.assert_array_equal(st["N"][0], o["root_N"][0]); np.testing.assert_array_equal(st["W"][0], o["root_W"][0])
        np.testing.assert_array_equal(st["P"][0], o["root_P"][0]); np.testing.assert_array_equal(st["policy"][0], o["policies"][0])
        assert int(st["root_visits"][0]) == int(o["root_visits"][0]) and int(st["chosen"][0]) == int(o["actions"][0]) and st["q"][0] == o["q"][0]
    assert e7 == 1 + int(o["evals"][0])                      # the root's own evaluation + the move's


# ------------------------------------------------------------------------------------------------ 7. the MCTS_Gumbel class
@pytest.mark.parametrize("name", GB.CLASS_FIXTURES)
def test_mcts_gumbel_class_batches_its_session_calls(emu_lib, oracle, name):
    GB.class_case(oracle, name, emu_lib, K=4)


def test_gumbel_batch_is_keyword_only(emu_lib):
    import inspect
    from grok_alpha_zero_amd.mcts import MCTS_Gumbel
    p = inspect.signature(MCTS_Gumbel.__init__).parameters["gumbel_batch"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default == 1


# ------------------------------------------------------------------------------------------------ 8. refusals
@pytest.mark.parametrize("kw,field", [(dict(search=0), "search"), (dict(eval_cache_log2=10), "eval_cache_log2"), (dict(game_groups=2), "game_groups"),
                                       (dict(leaf_batch=4), "leaf_batch"), (dict(search=0, leaf_batch=4), "leaf_batch"), (dict(gumbel_batch=65), "gumbel_batch"),
                                       (dict(gumbel_batch=-1), "gumbel_batch")])
def test_refusals_name_both_fields(emu_lib, kw, field):
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EngineError
    args = dict(search=1, gumbel_m=4, gumbel_batch=4, lib_path=emu_lib); args.update(kw)
    with pytest.raises(EngineError) as e:
        SelfPlayEngine("Connect4", 8, 30, 42, 0, 0, 0.0, 0.0, seed=1, **args)
    assert field in str(e.value) and "gumbel_batch" in str(e.value)


def test_repack_refused_groups_resolve_to_one_no_fused_wave(emu_lib):
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EngineError
    eng = SelfPlayEngine("Connect4", 8, 30, 42, 0, 0, 0.0, 0.0, seed=1, games_budget=8, search=1, gumbel_m=4, gumbel_batch=4, lib_path=emu_lib)
    assert eng.stats()["game_groups"] == 1 and eng.stats()["fused_wave"] == 0 and eng.batch_rows == 32
    with pytest.raises(EngineError, match="gumbel_batch"):
        eng.repack()
    with pytest.raises(EngineError, match="gumbel_batch"):
        eng.debug_fused_fault(2)
    eng.run_waves(8)
    assert eng.stats()["fused_wave"] == 0
    eng.close()


def test_raising_m_above_k_at_run_time_gives_more_chunks(emu_lib, oracle):
    """set_hyperparams(m = 7) on an engine created with m = 4, gumbel_batch = 4: two chunks per first phase, the oracle's m = 7 move"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine("Connect4", 2, 32, 42, 0, 0, 0.0, 0.0, seed=4, hash_salt=2, sync_moves=True, search=1, gumbel_m=4, c_visit=50.0, c_scale=1.0,
                         nodes_per_tree=256, gumbel_batch=4, lib_path=emu_lib)
    eng.set_hyperparams(m=7)
    eng.run_move()
    st = eng.root_stats()
    for g in range(2):
        o = oracle.selfplay_game_gumbel("Connect4", 32, 42, 7, 50.0, 1.0, 4, g, 0, hash_salt=2)
        np.testing.assert_array_equal(st["N"][g], o["root_N"][0]); np.testing.assert_array_equal(st["W"][g], o["root_W"][0])
        np.testing.assert_array_equal(st["policy"][g], o["policies"][0])
        assert int(st["root_visits"][g]) == int(o["root_visits"][0]) and int(st["chosen"][g]) == int(o["actions"][0])
    eng.close()


# ------------------------------------------------------------------------------------------------ 9. run_self_play passes it through
def test_run_self_play_passes_gumbel_batch_through(emu_lib, oracle, tmp_path):
    """run_self_play(use_gumbel, gumbel_batch=4) with its default eval_cache_log2 (forced off: the engine would refuse the pair) and 20
    slots for 26 games, so that the generation's tail reaches the point where run_self_play would repack (refused: it must not try).  The
    file's counters and every sample in it are those of the oracle's 26 games, and so are the engine's evaluator calls."""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import ReplayStore, run_self_play
    folder = str(tmp_path / "Grok_Zero_Train" / "0")
    store = ReplayStore(folder); store.create()
    train = dict(games_per_generation=26, MCTS_iteration_limit=16, max_actions=9, use_gumbel=True, m=4, c_visit=50.0, c_scale=1.0)
    es = {}
    assert run_self_play(GAMES["TicTacToe"], ({}, train), folder, n_games=20, seed=11, hash_salt=4, lib_path=emu_lib, engine_stats=es, gumbel_batch=4) == 26
    assert es["cache_hits"] == 0 and es["fused_wave"] == 0
    games = [oracle.selfplay_game_gumbel("TicTacToe", 16, 9, 4, 50.0, 1.0, 11, k % 20, k // 20, hash_salt=4) for k in range(26)]
    winners = [o["winner"] for o in games]
    gs = store.game_stats()
    assert gs[2] == 26 and gs[1] == sum(o["T"] for o in games) and gs[0] == max(o["T"] for o in games)
    assert [gs[3], gs[4], gs[5]] == [winners.count(-1), winners.count(0), winners.count(1)]
    assert es["plies"] == sum(o["T"] for o in games) and es["evals"] == sum(o["total_evals"] for o in games)
    # every sample the file holds, read back: per game and augmentation one (boards, policies, values) triple, those of the oracle's games
    from grok_alpha_zero_amd.self_play import record_to_samples
    want = []
    for o in games:
        ab, ap, av, _ = record_to_samples(GAMES["TicTacToe"], o)
        want += [(np.asarray(ab[i]).tobytes(), np.asarray(ap[i], np.float32).tobytes(), np.asarray(av[i], np.float32).tobytes()) for i in range(ap.shape[0])]
    n = store.n_datasets() // 3                          # three datasets per triple
    got = [(store.read(f"boards_{k}").tobytes(), store.read(f"policies_{k}").tobytes(), store.read(f"values_{k}").tobytes()) for k in range(n)]
    assert n == len(want) and sorted(got) == sorted(want)


# ------------------------------------------------------------------------------------------------ resets with requests in flight
@pytest.mark.parametrize("waves", [2, 3, 5])
@pytest.mark.parametrize("history", [[0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 2], []], ids=["six-legal", "five-legal", "empty"])
def test_reposition_with_requests_in_flight(emu_lib, history, waves):
    """set_position in the middle of a move, with up to 7 requests in flight, into a position with fewer candidates than K: the per-row
    state lives outside GameState, and none of it may reach the new game.  The move is that of a fresh engine, and of gumbel_batch = 1."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, SEARCH_GUMBEL

    def move(K, interrupted):
        eng = SelfPlayEngine("Connect4", 1, 32, 42, 0, 0, 0.0, 0.0, seed=6, hash_salt=3, sync_moves=True, single_tree=True, search=SEARCH_GUMBEL, gumbel_m=7,
                             c_visit=50.0, c_scale=1.0, gumbel_batch=K, lib_path=emu_lib)
        if interrupted:
            eng.set_position(0, []); eng.start_search(); eng.run_waves(waves)
        eng.set_position(0, history); eng.start_search(); eng.run_move()
        st = eng.root_stats()
        eng.close()
        return st
    want = move(1, False)
    for K, interrupted in ((7, False), (7, True), (1, True)):
        got = move(K, interrupted)
        for k in ("N", "W", "P", "policy", "root_visits", "q", "chosen"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"gumbel_batch {K} interrupted {interrupted} {k}")


def test_reset_games_with_requests_in_flight(emu_lib, oracle):
    """reset_games(all) after a few launches of free-running games, m lowered to 3 (chunks of 3 rows where 7 were in flight): every slot's
    next game is the oracle's"""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, SEARCH_GUMBEL
    G = 5
    eng = SelfPlayEngine("Connect4", G, 32, 42, 0, 0, 0.0, 0.0, seed=8, hash_salt=2, ring_capacity=4 * G, search=SEARCH_GUMBEL, gumbel_m=7, c_visit=50.0,
                         c_scale=1.0, gumbel_batch=7, lib_path=emu_lib)
    eng.run_waves(3)
    eng.reset_games()
    eng.set_hyperparams(m=3)
    recs = {}
    for _ in range(4000):
        eng.run_waves(32)
        for r in eng.drain_finished():
            recs.setdefault(r["slot"], r)
        if len(recs) == G:
            break
    eng.close()
    assert len(recs) == G
    for slot, r in recs.items():
        GB.assert_record_equals_oracle(r, oracle.selfplay_game_gumbel("Connect4", 32, 42, 3, 50.0, 1.0, 8, slot, r["game_seq"], hash_salt=2), f"slot {slot}")

"""The cases of match play (gaz_engine_set_match) that the CPU suite runs on the emulation build
(tests/test_match_emu.py) and the -m gpu suite on the HIP build (tests/test_match_gpu.py): `lib_path` = the emulation library, or None for
the product library.

Two hash salts are two networks, so every game of a match engine is compared exactly with tests/match_model.py: PUCT games with two
leaf_batch_model.Tree, Gumbel games with the oracle under a routing evaluator.  Nothing expected is read from the engine under test."""
import ctypes as C

import numpy as np

import match_model as M
from selfplay_support import A_OF, MAXT, play, refusal_message, slots_for

SEED, SALT_A, SALT_B = 17, 5, 9
PH_WAIT_HOST, PH_HALT = 5, 8


def _gumbel(m):
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL
    return dict(search=SEARCH_GUMBEL, gumbel_m=m, c_visit=50.0, c_scale=1.0, policy_is_logits=True)


# name -> (game, (run_iterations, max_actions, explore_first, explore_second, c_puct_init, dirichlet_alpha), gumbel m or None)
SELFPLAY = {
    "ttt": ("TicTacToe", (24, 9, 3, 3, 1.25, 1.0), None),
    "c4": ("Connect4", (40, 42, 4, 4, 2.5, 0.5), None),
    "gmk": ("Gomoku", (48, 3, 2, 2, 2.5, 0.05), None),               # (48 < the legal moves: every move runs 3 x its legal moves)
    "ttt-gumbel": ("TicTacToe", (16, 9, 0, 0, 0.0, 0.0), 4),
    "c4-gumbel": ("Connect4", (32, 42, 0, 0, 0.0, 0.0), 7),
}


def make_engine(name, G, lib_path, games, match=True, salt_b=SALT_B, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    game, args, m = SELFPLAY[name]
    a = dict(seed=SEED, hash_salt=SALT_A, ring_capacity=2 * games + 8, games_budget=games, lib_path=lib_path)
    if m:
        a.update(_gumbel(m))
    a.update(kw)
    eng = SelfPlayEngine(game, G, *args, **a)
    if match:
        eng.set_match(True, hash_salt_b=salt_b)
        assert eng.match is True
    return eng


def assert_game(oracle, name, rec, nets, what):
    """one finished game of a match against the model (PUCT: the two trees; Gumbel: the oracle under the routing evaluator)"""
    game, (iters, max_actions, e1, e2, c_init, alpha), m = SELFPLAY[name]
    if not m:
        M.assert_puct_record(oracle, game, SEED, iters, max_actions, rec, nets, what, c_puct_init=c_init, dirichlet_alpha=alpha)
        return
    router = M.GumbelRouter(game, rec["slot"], rec["game_seq"], rec, nets)
    o = oracle.selfplay_game_gumbel(game, iters, max_actions, m, 50.0, 1.0, SEED, rec["slot"], rec["game_seq"], evaluator=router)
    assert (rec["T"], rec["winner"]) == (o["T"], o["winner"]), (what, rec["T"], o["T"])
    np.testing.assert_array_equal(o["evals"], rec["evals"], err_msg=f"{what}: the routing schedule")
    for k in ("actions", "policies", "q", "root_N", "root_W", "root_P", "root_visits"):
        np.testing.assert_array_equal(np.asarray(rec[k]).reshape(np.asarray(o[k]).shape), o[k], err_msg=f"{what} {k}")
    assert router.calls[0] > 0 and router.calls[1] > 0, (what, router.calls)


# ------------------------------------------------------------------------------------------------ 1. / 2. self-play of a match against the model
def selfplay_case(oracle, name, G, lib_path, per_slot=2, slots=None, **kw):
    """two hash salts, continuous mode, `per_slot` games per slot: the compared games are the model's; both colours occurred and both
    networks evaluated rows; a match-off engine plays other games"""
    game = SELFPLAY[name][0]
    n = per_slot * G
    eng = make_engine(name, G, lib_path, n, **kw)
    recs = play(eng, n)
    ms, st = eng.match_stats(), eng.stats()
    eng.close()
    assert sorted(recs) == sorted((s, q) for s in range(G) for q in range(per_slot))
    assert st["fused_wave"] == 0
    nets = M.hash_pair(oracle, game, SALT_A, SALT_B)
    look = slots_for(G) if slots is None else slots
    colours = set()
    for (slot, seq), r in sorted(recs.items()):
        if slot in look:
            assert_game(oracle, name, r, nets, f"{name} game {(slot, seq)}")
            colours.add(M.colour(slot, seq))
    assert colours == {0, 1} or G * per_slot == 1, colours
    assert ms["rows_a"] > 0 and ms["rows_b"] > 0 and ms["passes"] > 0, ms
    assert ms["rows_a"] + ms["rows_b"] == st["evals"], (ms, st)
    off = make_engine(name, G, lib_path, n, match=False, **kw)
    plain = play(off, n)
    off.close()
    assert any(recs[k]["T"] != plain[k]["T"] or not np.array_equal(recs[k]["root_W"], plain[k]["root_W"]) for k in recs), "match on and off play the same games"
    print(f"{name} G={G}: {n} games, match stats {ms}", flush=True)
    return recs, ms


# ------------------------------------------------------------------------------------------------ 3. the external evaluator
def external_case(oracle, name, G, lib_path, uniform_b=False):
    """GAZ_EVAL_EXTERNAL, continuous mode, one game per slot: every pending row is answered by the network read_batch_network names (two
    hash salts, or with uniform_b network B = the uniform evaluator of tests/degenerate_eval.py); net == 255 exactly where pending == 0;
    the records are the model's"""
    import degenerate_eval as D
    from grok_alpha_zero_amd.engine import EVAL_EXTERNAL
    game = SELFPLAY[name][0]
    A = A_OF[game]
    nets = M.hash_pair(oracle, game, SALT_A, SALT_B)
    if uniform_b:
        def uniform(s):
            p, v, _ = D.evaluate_many("uniform", np.asarray(s)[None], A)
            return p[0], v[0]
        nets[1] = uniform
    eng = make_engine(name, G, lib_path, G, evaluator=EVAL_EXTERNAL)
    recs, asked = {}, [0, 0]
    for _ in range(1000000):
        eng.wave_begin()
        x, pend = eng.read_batch()
        net = eng.read_batch_network()
        np.testing.assert_array_equal(net == 255, pend == 0)
        pol = np.full((G, A), np.nan, np.float32); val = np.full(G, np.nan, np.float32)
        for r in np.flatnonzero(pend):
            assert net[r] in (0, 1)
            pol[r], val[r] = nets[int(net[r])](x[r]); asked[int(net[r])] += 1
        eng.write_outputs(pol, val)
        for r in eng.drain_finished():
            recs[(r["slot"], r["game_seq"])] = r
        if len(recs) == G:
            break
    ms = eng.match_stats()
    eng.close()
    assert ms["passes"] == 0 and asked[0] > 0 and asked[1] > 0, (ms, asked)
    for key, r in sorted(recs.items()):
        assert_game(oracle, name, r, nets, f"external {name} game {key}")
    return asked


# ------------------------------------------------------------------------------------------------ 4. the anchor: B == A is match off
def anchor_case(name, G, lib_path, games=None, **kw):
    """hash_salt_b == hash_salt: byte-identical records to the same engine with match off, while the routing ran"""
    n = games or 2 * G
    on, off = make_engine(name, G, lib_path, n, salt_b=SALT_A, **kw), make_engine(name, G, lib_path, n, match=False, **kw)
    assert off.match is False
    ra, rb = play(on, n, raw=True), play(off, n, raw=True)
    ms, ms_off, sa, sb = on.match_stats(), off.match_stats(), on.stats(), off.stats()
    on.close(); off.close()
    assert sorted(ra) == sorted(rb) and len(ra) == n
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), (name, k)
    assert (sa["evals"], sa["sims"], sa["plies"]) == (sb["evals"], sb["sims"], sb["plies"])
    assert ms["rows_a"] > 0 and ms["rows_b"] > 0 and ms["rows_a"] + ms["rows_b"] == sa["evals"], (ms, sa)
    assert not any(ms_off.values()), ms_off
    return ms


ANCHOR_ALL = dict(solver=True, eval_symmetry=True, forced_playouts_k=2.0, fast_iterations=12, full_search_prob=0.5)


# ------------------------------------------------------------------------------------------------ 5. sync mode, and switching
def sync_case(oracle, name, G, lib_path, switch=()):
    """run_move / get_root_stats / apply_moves over whole games against the model.  switch = plies after whose search the mode is toggled
    (before apply_moves: the launch that applies the move makes the next requests).  Then a wave with no request at all"""
    game, (iters, max_actions, e1, e2, c_init, alpha), m = SELFPLAY[name]
    assert not m
    from leaf_batch_model import Tree
    eng = make_engine(name, G, lib_path, 0, sync_moves=True, games_budget=0, ring_capacity=2 * G)
    nets = M.hash_pair(oracle, game, SALT_A, SALT_B)
    mode = {"on": True}
    trees = {}
    for g in range(G):
        c = M.colour(g, 0)
        trees[g] = [Tree(oracle, game, 1, SEED, slot=g, game_seq=0, tree=k, c_puct_init=c_init, dirichlet_alpha=alpha,
                         evaluator=(lambda s, k=k, c=c: nets[(k ^ c) if mode["on"] else 0](s))) for k in range(2)]
    plies = 0
    for ply in range(max_actions + 1):
        eng.run_move()
        st = eng.root_stats()
        live = [g for g in range(G) if st["phase"][g] != PH_HALT]
        if not live:
            break
        for g in live:
            want = trees[g][ply % 2].run(iters)
            for k in ("N", "W", "P"):
                np.testing.assert_array_equal(st[k][g], want[k], err_msg=f"sync {name} slot {g} ply {ply} {k}")
            assert int(st["root_visits"][g]) == want["root_visits"], (g, ply)
        if ply == 1:                                                     # a wave with no request at all: every game waits for the host
            before = eng.match_stats()
            assert (eng.read_batch_network() == 255).all()
            eng.run_waves(1)
            after, st2 = eng.match_stats(), eng.root_stats()
            assert after["passes"] == before["passes"] + 1 and after["waves_without_a"] == before["waves_without_a"] + 1
            assert after["waves_without_b"] == before["waves_without_b"] + 1 and (after["rows_a"], after["rows_b"]) == (before["rows_a"], before["rows_b"])
            for k in ("N", "W", "P", "chosen", "phase"):
                np.testing.assert_array_equal(st[k], st2[k])
        if ply in switch:
            mode["on"] = not mode["on"]
            eng.set_match(mode["on"], hash_salt_b=SALT_B)
            assert eng.match is mode["on"]
        eng.apply_moves()
        for g in live:
            if len(trees[g][0].hist) + 1 < max_actions and not _ended(game, trees[g][0], int(st["chosen"][g])):
                for t in trees[g]:
                    t.play(int(st["chosen"][g]))
        plies += 1
    recs = {r["slot"]: r for r in eng.drain_finished()}
    ms = eng.match_stats()
    eng.close()
    assert sorted(recs) == list(range(G)) and ms["rows_a"] > 0 and ms["rows_b"] > 0
    for g, r in recs.items():
        assert r["winner"] == M.winner_of(game, r["actions"], max_actions)
    return plies, ms


def eng_hist(tree):
    return [int(a) for a in tree.hist]


def _ended(game, tree, action):
    """does `action` end the game the tree stands in (a win or a full board)?"""
    from grok_alpha_zero_amd.games import GAMES
    G = GAMES[game]
    b = tree.board.copy()
    G.do_action_MCTS(b, G.index_to_action(action), tree.next_player)
    hist = np.array([G.index_to_action(a) for a in eng_hist(tree) + [action]])
    return G.check_win_MCTS(b, tree.next_player, hist) != -2


# ------------------------------------------------------------------------------------------------ 6. edge cases: 1 and 2 games
def one_game_case(oracle, name, lib_path):
    """1 game: every wave has all its rows on one side or none"""
    recs, ms = selfplay_case(oracle, name, 1, lib_path, per_slot=2)
    assert ms["waves_without_a"] + ms["waves_without_b"] >= ms["passes"] > 0, ms
    return ms


# ------------------------------------------------------------------------------------------------ 7. refusals
def refusal_case(lib_path):
    """-> the messages, each its own and naming its field"""
    from grok_alpha_zero_amd.engine import MatchParams, SelfPlayEngine
    msgs = {}

    def engine(**kw):
        a = dict(seed=1, lib_path=lib_path); a.update(kw)
        return SelfPlayEngine("Connect4", 8, 40, 42, 4, 4, 2.5, 0.5, **a)
    for field, kw in (("single_tree", dict(single_tree=True, sync_moves=True)), ("leaf_batch", dict(leaf_batch=4)),
                      ("gumbel_batch", dict(gumbel_batch=4, **_gumbel(7))), ("eval_cache_log2", dict(eval_cache_log2=10)),
                      ("game_groups = 1", dict(game_groups=2))):
        eng = engine(**kw)
        try:
            msgs[field] = refusal_message(lambda: eng.set_match(True), f"set_match with {field} was not refused")
            assert field in msgs[field] and eng.match is False, msgs[field]
            eng.set_match(False)                                         # switching off is always legal
            m2 = refusal_message(eng.read_batch_network, f"read_batch_network with {field} was not refused")
            assert field in m2 and "read_batch_network" in m2
        finally:
            eng.close()
    eng = engine(games_budget=8)
    try:
        for what, p in (("struct_size", MatchParams(struct_size=8, mode=1)), ("mode", MatchParams(struct_size=C.sizeof(MatchParams), mode=2)),
                        ("mode-neg", MatchParams(struct_size=C.sizeof(MatchParams), mode=-1))):
            assert eng.L.gaz_engine_set_match(eng.h, C.byref(p)) != 0
            msgs[what] = eng.L.gaz_engine_last_error(eng.h).decode()
            assert what.split("-")[0] in msgs[what] and eng.match is False
        for fn, arg in (("set_match", None), ("get_match", None), ("read_batch_network", None), ("get_match_stats", None)):
            assert getattr(eng.L, "gaz_engine_" + fn)(eng.h, arg) != 0
            msgs[fn + "-null"] = eng.L.gaz_engine_last_error(eng.h).decode()
            assert "null" in msgs[fn + "-null"]
        eng.set_match(True, hash_salt_b=3)
        msgs["repack"] = refusal_message(eng.repack, "repack with match on was not refused")
        assert "match" in msgs["repack"]
        msgs["debug_fused_fault"] = refusal_message(lambda: eng.debug_fused_fault(3), "debug_fused_fault with match on was not refused")
        eng.run_waves(4)
        assert eng.stats()["fused_wave"] == 0
        eng.set_match(False)
        eng.repack()
    finally:
        eng.close()
    assert len(set(msgs.values())) == len(msgs), msgs
    return msgs


def weights_b_refusal_case():
    """HIP build: with match on and the ResNet evaluator, run_waves / run_move before load_weights_b are refused"""
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
    from selfplay_support import c4_one_block_weights
    out = []
    for sync in (False, True):
        eng = SelfPlayEngine("Connect4", 4, 40, 42, 4, 4, 2.5, 0.5, seed=1, evaluator=EVAL_RESNET, net_blocks=1, sync_moves=sync, game_groups=1)
        try:
            eng.load_weights(c4_one_block_weights())
            eng.set_match(True)
            m = refusal_message(eng.run_move if sync else (lambda: eng.run_waves(1)), "no refusal before load_weights_b")
            assert "weights of network B not loaded" in m
            out.append(m)
            eng.load_weights_b(c4_one_block_weights())
            eng.run_move() if sync else eng.run_waves(1)
        finally:
            eng.close()
    return out


# ------------------------------------------------------------------------------------------------ 8. two real networks (HIP build)
def _flipped(weights, key):
    """the same tensors with one layer's sign flipped: another network of the same shapes"""
    w = {k: np.array(v, np.float32, copy=True) for k, v in weights.items()}
    w[key] = -w[key]
    return w


def _probe_net(game, weights, rows=64):
    """the network `weights` as an evaluator: evaluate() of an ordinary engine on single rows (rows of a batch are independent bit for bit,
    tests/test_evaluator_gpu.py).  -> (evaluator, close)"""
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
    probe = SelfPlayEngine(game, rows, 1, MAXT[game], 0, 0, 2.5, 0.5, seed=0, evaluator=EVAL_RESNET, net_blocks=1, ring_capacity=0, game_groups=1)
    probe.load_weights(weights)
    memo = {}

    def ev(state):
        key = np.ascontiguousarray(state, np.int8).tobytes()
        if key not in memo:
            p, v, _ = probe.evaluate(np.ascontiguousarray(state, np.int8)[None])
            memo[key] = (p[0].copy(), v[0])
        return memo[key]
    return ev, probe.close


NETWORK = {   # game -> (net class name, run_iterations, max_actions, explore, c_puct_init, alpha, the layer whose sign makes network B)
    "Connect4": ("Connect4Net", 12, 42, 4, 2.5, 0.5, "block0.conv2.w"),
    "Gomoku": ("GomokuNet", 228, 8, 2, 2.5, 0.05, "block0.conv2.w"),     # (228 >= the 225 legal moves: a move runs 228 simulations, not 3 x 225)
}


def network_weights(game):
    from grok_alpha_zero_amd import net
    cls, *_, flip = NETWORK[game]
    a = getattr(net, cls)(1, seed=0).eval().export_engine_weights()
    return a, _flipped(a, flip)


def network_engine(game, G, games, weights_a, weights_b=None, **kw):
    """G games of `game` with the 1-block network, one group; weights_b: match on against them"""
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
    _, iters, max_actions, explore, c_init, alpha, _ = NETWORK[game]
    eng = SelfPlayEngine(game, G, iters, max_actions, explore, explore, c_init, alpha, seed=SEED, evaluator=EVAL_RESNET, net_blocks=1, ring_capacity=2 * games + 8,
                         games_budget=games, game_groups=1, **kw)
    eng.load_weights(weights_a)
    if weights_b is not None:
        eng.load_weights_b(weights_b)
        eng.set_match(True)
    return eng


def network_case(oracle, game, G, slots=None):
    """G games, one per slot, network A against network B: the compared slots are the model's with the evaluators of two ordinary
    engines; then the anchor B = A: byte-identical to match off (separate launches, one group)"""
    _, iters, max_actions, explore, c_init, alpha, _ = NETWORK[game]
    wa, wb = network_weights(game)
    eng = network_engine(game, G, G, wa, wb)
    recs = play(eng, G)
    ms, st = eng.match_stats(), eng.stats()
    eng.close()
    assert st["fused_wave"] == 0 and ms["rows_a"] > 0 and ms["rows_b"] > 0 and ms["rows_a"] + ms["rows_b"] == st["evals"], (ms, st)
    (ea, close_a), (eb, close_b) = _probe_net(game, wa), _probe_net(game, wb)
    try:
        s0 = np.random.default_rng(0).integers(-1, 2, size=(eng.H, eng.W, eng.Cc)).astype(np.int8)      # (on the empty board's all-zero planes every network says the same)
        assert not np.array_equal(ea(s0)[0], eb(s0)[0]), "the two networks do not differ: the case would show nothing"
        look = slots_for(G) if slots is None else slots
        for (slot, seq), r in sorted(recs.items()):
            if slot in look:
                M.assert_puct_record(oracle, game, SEED, iters, max_actions, r, [ea, eb], f"network {game} game {(slot, seq)}", c_puct_init=c_init, dirichlet_alpha=alpha)
    finally:
        close_a(); close_b()
    on, off = network_engine(game, G, G, wa, wa), network_engine(game, G, G, wa)
    off.set_fused_wave(False)
    ra, rb = play(on, G, raw=True), play(off, G, raw=True)
    sa, sb = on.stats(), off.stats()
    on.close(); off.close()
    assert sa["fused_wave"] == 0 and sb["fused_wave"] == 0 and sorted(ra) == sorted(rb) == [(s, 0) for s in range(G)]
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), (game, k)
    print(f"network {game} G={G}: match stats {ms}", flush=True)


def play_match_case():
    """play_match end to end on the 1-block Connect4 network: 128 games on 64 slots"""
    from grok_alpha_zero_amd.games import Connect4
    from grok_alpha_zero_amd.self_play import match_result, play_match
    wa, wb = network_weights("Connect4")
    train = dict(MCTS_iteration_limit=8, max_actions=42, num_explore_actions_first=4, num_explore_actions_second=4, c_puct_init=2.5, dirichlet_alpha=0.5, use_gumbel=False)
    res = play_match(Connect4, (dict(num_resnet_layers=1, num_filters=128), train), wa, wb, 128, n_slots=64, seed=SEED)
    hdrs = res.pop("headers")
    assert sorted((s, q) for _, _, s, q in hdrs) == [(s, q) for s in range(64) for q in range(2)]
    assert res["n"] == res["a_wins"] + res["draws"] + res["b_wins"] == 128 and res["a_first"]["n"] == res["a_second"]["n"] == 64
    want = match_result(hdrs)
    assert all(res[k] == want[k] for k in want) and res["positions"] == sum(h[0] for h in hdrs)
    assert res["match_stats"]["rows_a"] > 0 and res["match_stats"]["rows_b"] > 0
    print({k: v for k, v in res.items() if k != "match_stats"}, flush=True)

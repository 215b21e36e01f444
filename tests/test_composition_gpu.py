"""-m gpu: every BASELINE configuration at its REAL composition against the oracle.

The other GPU tests check the pieces — the full-size search with the hash evaluator, the network per layer, the fused launch against
separate launches.  Here the thing that is benchmarked is the thing that is checked: the full batch, the full network, the default
launch shape (Connect4: tree step + trunk as ONE launch with the edge tiles; Gomoku: the 10-block launch with block 0 inside; Gumbel:
logits head), the configuration's own search parameters — and sampled slots are replayed by the CPU oracle (oracle/gaz_puct.c,
gaz_gumbel.c: MCTS.py / MCTS_Gumbel.py / Self_Play.py restated) whose session.run is served by the SAME HIP network on single rows
(rows of a batch are independent bit for bit, tests/test_evaluator_gpu.py).  Bar: actions, visit counts N, W, P, policies and values
bit-exact (north_star: integer visit counts bit-exact, Q / V within 1e-5 — here equal)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _first_games(eng, n_games, max_rounds, waves):
    recs = []
    for _ in range(max_rounds):
        eng.run_waves(waves)
        recs += eng.drain_finished(n_games)
        if len(recs) >= n_games:
            break
    return {r["slot"]: r for r in recs if r["game_seq"] == 0}


def _check(r, o, what):
    assert r["T"] == o["T"], what
    for k in ("actions", "root_N", "root_visits", "root_W", "root_P", "policies", "values"):
        np.testing.assert_array_equal(np.asarray(r[k]), np.asarray(o[k]), err_msg=f"{what}: {k}")


# The headline engine runs as two game groups of 2048 slots (choose_game_groups), each with its own trunk launch over its own rows.  A group's
# rows are tiled by the grouped plan (resnet.hip make_trunk_plan, shared_chip): 2048 // 3 = 682 three-board tiles (group rows 0 .. 2045), then
# one two-board tile (rows 2046, 2047).  Slots: both ends of both groups (0, 2047 | 2048, 4095), first tile's last board / second tile's first
# (2, 3 | 2050), the last three-board tile's last board (2045 | 4093), the two-board tile (2046, 2047 | 4094, 4095), the second board of
# group 1 (2049) — and the tile edges of ONE batch of 4096 (1535, 1536, 3071, 3072, 3073, 4000), kept from before the groups.
HEADLINE_SLOTS = (0, 2, 3, 1535, 1536, 2045, 2046, 2047, 2048, 2049, 2050, 3071, 3072, 3073, 4000, 4093, 4094, 4095)


def test_headline_composition_connect4_4096_games_6_blocks_fused_launch(oracle):
    """BASELINE configs[1] exactly as bench.py runs it: 4096 concurrent Connect4 games, 200 simulations per move, the 6-block network in
    bf16, tree step + trunk in ONE launch (k_wave_trunk<mix, edge tiles>), two game groups, tau schedule 8 / 7, Dirichlet 0.5 — every slot
    plays its first game to the end (Self_Play.py:71-157); the slots of HEADLINE_SLOTS (group and tile edges) are replayed by the oracle with
    the HIP network as its evaluator."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import Connect4Net
    G, sims = 4096, 200
    net = Connect4Net(6, seed=0).eval()
    w = net.export_engine_weights()
    eng = SelfPlayEngine("Connect4", G, sims, 42, 8, 7, 2.5, 0.5, seed=1234, evaluator=EVAL_RESNET, net_blocks=6, ring_capacity=G, games_budget=G)
    eng.load_weights(w)
    first = _first_games(eng, G, 200, 400)
    st = eng.stats()
    assert len(first) == G and st["fused_wave"] == 1 and st["fused_faults"] == 0 and st["game_groups"] == 2, (len(first), st)
    assert st["game_stats"][0] == max(r["T"] for r in first.values()) and st["game_stats"][2] == G, st
    eng.close()
    probe = SelfPlayEngine("Connect4", 64, 1, 42, 8, 7, 2.5, 0.5, seed=0, evaluator=EVAL_RESNET, net_blocks=6, ring_capacity=0)
    probe.load_weights(w)

    def ev(state):
        p, v, _ = probe.evaluate(state[None])
        return p[0], v[0]
    for slot in HEADLINE_SLOTS:
        o = oracle.selfplay_game("Connect4", sims, 42, 8, 7, 2.5, 0.5, 1234, slot, 0, evaluator=ev)
        _check(first[slot], o, f"Connect4 headline composition, slot {slot}")
    probe.close()
    lengths = np.array([r["T"] for r in first.values()])
    assert 7 <= lengths.min() and lengths.max() <= 42


def test_gomoku_composition_2048_games_10_blocks(oracle):
    """BASELINE configs[3]: 2048 concurrent Gomoku games, 400 simulations per move (on an empty 15 x 15 board MCTS.run raises that to 3 x the
    legal moves, MCTS.py:545-546), the 10-block network (256-channel stem, block 0 with its projection inside the 8-wave trunk launch, heads on
    two streams), alpha 0.05, c_puct 4.5 — max_actions = 3 keeps the oracle's side to seconds (a game is then a draw after 3 plies,
    Self_Play.py:155-157); 4 sampled slots replayed by the oracle with the HIP network as its evaluator."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import NETS
    G, sims, plies = 2048, 400, 3
    net = NETS["Gomoku"](10, seed=0).eval()
    w = net.export_engine_weights()
    eng = SelfPlayEngine("Gomoku", G, sims, plies, 6, 4, 4.5, 0.05, seed=77, evaluator=EVAL_RESNET, net_blocks=10, net_filters=128, ring_capacity=G, games_budget=G)
    eng.load_weights(w)
    first = _first_games(eng, G, 60, 100)
    assert len(first) == G, len(first)
    eng.close()
    probe = SelfPlayEngine("Gomoku", 8, 1, plies, 6, 4, 4.5, 0.05, seed=0, evaluator=EVAL_RESNET, net_blocks=10, net_filters=128, ring_capacity=0)
    probe.load_weights(w)

    def ev(state):
        p, v, _ = probe.evaluate(state[None])
        return p[0], v[0]
    for slot in (0, 1, 1023, 2047):
        o = oracle.selfplay_game("Gomoku", sims, plies, 6, 4, 4.5, 0.05, 77, slot, 0, evaluator=ev)
        _check(first[slot], o, f"Gomoku composition, slot {slot}")
    probe.close()


def test_gumbel_composition_8192_games_logits_head(oracle):
    """BASELINE configs[4]: 8192 concurrent Connect4 games under the Gumbel search (n = 32, m = 7, c_visit 50, c_scale 1, Gumbel noise on;
    MCTS_Gumbel.py:562-679) with the 6-block network's LOGITS head behind it (Connect4/Build_Model.py:54-60) — whole games; 8 sampled slots
    replayed by the oracle with the HIP network as its evaluator."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET, SEARCH_GUMBEL
    from grok_alpha_zero_amd.net import Connect4Net
    G, n, m = 8192, 32, 7
    net = Connect4Net(6, seed=0, policy_head="linear").eval()
    w = net.export_engine_weights()
    eng = SelfPlayEngine("Connect4", G, n, 42, 8, 7, 2.5, 0.5, seed=4321, evaluator=EVAL_RESNET, net_blocks=6, ring_capacity=G, games_budget=G,
                         search=SEARCH_GUMBEL, gumbel_m=m, c_visit=50.0, c_scale=1.0, policy_is_logits=True)
    eng.load_weights(w)
    first = _first_games(eng, G, 100, 200)
    st = eng.stats()
    assert len(first) == G and st["game_groups"] == 2 and st["fused_wave"] == 1 and st["fused_faults"] == 0, (len(first), st)
    assert st["game_stats"][0] == max(r["T"] for r in first.values()) and st["game_stats"][2] == G, st
    eng.close()
    probe = SelfPlayEngine("Connect4", 64, 1, 42, 8, 7, 2.5, 0.5, seed=0, evaluator=EVAL_RESNET, net_blocks=6, ring_capacity=0, policy_is_logits=True)
    probe.load_weights(w)

    def ev(state):
        p, v, _ = probe.evaluate(state[None])
        return p[0], v[0]
    for slot in (0, 1, 1536, 4095, 4096, 6000, 8190, 8191):
        o = oracle.selfplay_game_gumbel("Connect4", n, 42, m, 50.0, 1.0, 4321, slot, 0, evaluator=ev)
        _check(first[slot], o, f"Gumbel composition, slot {slot}")
    probe.close()


def _gomoku_position(rng, mine, theirs, keep_empty, n=60):
    """An n-ply Gomoku history (engine action indices, cell = row * 15 + col) whose first mover (-1, to move after an even n) holds the
    cells `mine` and the second mover `theirs`, the rest of the stones scattered at random where they extend no line of their colour
    beyond two; `keep_empty` stays free.  Checked with the game rules: no ply of it ends the game."""
    from grok_alpha_zero_amd.games import GAMES
    stones = {}
    for c in mine:
        stones[c] = -1
    for c in theirs:
        stones[c] = 1

    def run(cell, p):
        best = 1
        for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
            k = 1
            for s in (1, -1):
                y, x = cell[0] + s * dy, cell[1] + s * dx
                while 0 <= y < 15 and 0 <= x < 15 and stones.get((y, x)) == p:
                    k += 1; y += s * dy; x += s * dx
            best = max(best, k)
        return best
    lists = {-1: list(mine), 1: list(theirs)}
    for p in (-1, 1):
        while len(lists[p]) < n // 2:
            cell = (int(rng.integers(0, 15)), int(rng.integers(0, 15)))
            if cell in stones or cell in keep_empty or run(cell, p) > 2:
                continue
            stones[cell] = p; lists[p].append(cell)
    h = []
    for i in range(n // 2):
        h += [lists[-1][i][0] * 15 + lists[-1][i][1], lists[1][i][0] * 15 + lists[1][i][1]]
    g = GAMES["Gomoku"]()
    for a in h:
        g.do_action(GAMES["Gomoku"].index_to_action(a))
        assert g.check_win() == -2
    return h


def test_gomoku_composition_bench_positions_2048_games_10_blocks(oracle):
    """BASELINE configs[3] in the state bench.py times it in: 2048 Gomoku games, 400 simulations per move, the 10-block network, the automatic
    two game groups of fused k_wave_trunk_gmk launches, every slot placed at bench.random_histories("Gomoku", 2048, default_rng(977), 60) by
    gaz_engine_set_position — mid-game positions: fewer legal moves, terminal actions in the tree.  max_actions = 64 ends the sampled games
    within a few plies.  Six slots (both ends of both groups, 0 / 1023 | 1024 / 2047, and two inside) are overwritten with 60-ply positions:
    the mover has an open four (its win is a terminal action of the root), or must block the opponent's four, or neither; two slots keep a long
    random history.  Those games are replayed by the oracle from the same history with the HIP network as its evaluator, bit for bit from
    the first searched ply."""
    import sys
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import NETS
    from conftest import ROOT
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from bench import random_histories
    G, sims, M = 2048, 400, 64
    hs = random_histories("Gomoku", G, np.random.default_rng(977), 60)
    rng = np.random.default_rng(5)
    open_four = lambda y, x: dict(mine=[(y, x + i) for i in range(4)], theirs=[], keep_empty=[(y, x - 1), (y, x + 4)])
    must_block = lambda y, x: dict(mine=[(y, x - 1)], theirs=[(y, x + i) for i in range(4)], keep_empty=[(y, x + 4)])
    placed = {0: open_four(7, 5), 1023: must_block(3, 2), 1024: must_block(11, 9), 2047: open_four(2, 8), 700: dict(mine=[], theirs=[], keep_empty=[]),
              1500: must_block(12, 3)}
    for slot, spec in placed.items():
        hs[slot] = _gomoku_position(rng, **spec)
    interior = [g for g in range(1, G - 1) if g not in placed and len(hs[g]) >= 58][:2]
    sampled = sorted(placed) + interior
    net = NETS["Gomoku"](10, seed=0).eval()
    w = net.export_engine_weights()
    eng = SelfPlayEngine("Gomoku", G, sims, M, 6, 4, 4.5, 0.05, seed=1234, evaluator=EVAL_RESNET, net_blocks=10, net_filters=128, ring_capacity=G,
                         games_budget=G)
    eng.load_weights(w)
    for slot, h in enumerate(hs):
        if h:
            eng.set_position(slot, h)
    eng.synchronize()
    recs = {}
    for _ in range(200):
        eng.run_waves(100)
        recs.update({r["slot"]: r for r in eng.drain_finished(G) if r["game_seq"] == 0})
        if all(s in recs for s in sampled):
            break
    st = eng.stats()
    assert all(s in recs for s in sampled), sorted(set(sampled) - set(recs))
    assert st["game_groups"] == 2 and st["fused_wave"] == 1 and st["fused_faults"] == 0, st
    eng.close()
    probe = SelfPlayEngine("Gomoku", 8, 1, M, 6, 4, 4.5, 0.05, seed=0, evaluator=EVAL_RESNET, net_blocks=10, net_filters=128, ring_capacity=0)
    probe.load_weights(w)

    def ev(state):
        p, v, _ = probe.evaluate(state[None])
        return p[0], v[0]
    fives = 0
    for slot in sampled:
        r, h, n = recs[slot], hs[slot], len(hs[slot])
        o = oracle.selfplay_game("Gomoku", sims, M, 6, 4, 4.5, 0.05, 1234, slot, 0, evaluator=ev, start_history=h)
        what = f"Gomoku at the bench's positions, slot {slot} ({n} plies)"
        assert r["T"] == n + o["T"] and r["winner"] == o["winner"], (what, r["T"], n, o["T"], r["winner"], o["winner"])
        np.testing.assert_array_equal(r["actions"][:n], h, err_msg=what)
        for k in ("actions", "root_N", "root_visits", "root_W", "root_P", "policies", "values"):
            np.testing.assert_array_equal(np.asarray(r[k][n:]), np.asarray(o[k]), err_msg=f"{what}: {k}")
        fives += r["winner"] != 0 and r["T"] < M
    probe.close()
    assert fives >= 1 and recs[0]["winner"] == -1 and recs[0]["T"] == 61 and recs[2047]["winner"] == -1, fives

"""Every launch shape at game counts that fill no wave, block or tile: the case bodies that the CPU suite runs
on the emulation build (tests/test_ragged_emu.py) and the -m gpu suite on the HIP build (tests/test_ragged_gpu.py): `lib_path` = the
emulation library, or None for the product library.

The units a game count n can fail to fill: the four 16-lane teams of a Connect4 / TicTacToe wavefront ((n + 3) / 4 wavefronts); the tree
blocks of the one-launch wave (queue_gpb games each, stepped in rounds of NT; the completion queue is rank-major over n / gpb full blocks
and one partial block of n % gpb games); the 2- and 3-board trunk tiles of Connect4; the 16 positions of a heads block; the game groups
(n / k (+ 1) slots each, the budget split by a formula of its own).  The sizes:

    n = 1      one team of four; one board in a 2-board tile; no full tree block (queue_nfull = 0)
    n = 2      one whole 2-board tile, half a wavefront
    n = 3, 5   a partial wavefront; a last tile with one board; odd
    n = 17     one full PUCT tree block + 1 game; a partial Gumbel block that spans two rounds
    n = 67     one Gumbel / Gomoku block (64) + 3; 4 PUCT blocks + 3; 22 three-board tiles + 1 board
    n = 9      one Gomoku round (8) + 1

Every engine gets games_budget = 2 n: every slot plays game_seq 0 and 1 and halts, whatever n is.  Everything is bit-exact."""
import numpy as np

N_C4 = (1, 2, 3, 5, 17, 67)                        # also TicTacToe
N_GMK = (1, 3, 9, 67)
ORACLE_KEYS = ("actions", "root_N", "root_visits", "root_W", "root_P", "policies", "values", "q")       # (test_hip_engine_matches_oracle_many_games)
SEED, SALT, OFFSET = 2024, 17, 1000

# game -> run_iterations, max_actions, explore first / second, c_puct_init, dirichlet_alpha.  Gomoku runs 3 x legal simulations a move
# when run_iterations is below the number of legal moves, so it asks for 225 (the fewest it can run), and its games are cut short
# (max_actions 2: one move of either tree; 67 slots of it take the one-lane emulation 12 s).
PUCT = {"Connect4": (20, 42, 4, 3, 2.5, 0.5), "TicTacToe": (16, 9, 2, 1, 1.25, 1.0), "Gomoku": (225, 2, 1, 1, 4.5, 0.05)}
GUMBEL = {"Connect4": (16, 42, 4), "TicTacToe": (16, 9, 4)}                  # game -> n, max_actions, m
GROUPS = ((2, 2), (5, 2), (7, 3), (5, 5))          # (n, k): two groups of one game; 3 | 2; 3 | 2 | 2; five groups of one game


def sizes_of(game):
    return N_GMK if game == "Gomoku" else N_C4


def play_budget(eng, budget, waves=32, rounds=40000, after=4):
    """a free-running engine with a games_budget until `budget` games are there, then `after` launches more: every slot has halted, so
    nothing may follow -> the records"""
    recs = []
    for _ in range(rounds):
        eng.run_waves(waves)
        recs += eng.drain_finished()
        if len(recs) >= budget:
            break
    eng.run_waves(after)
    recs += eng.drain_finished()
    assert len(recs) == budget, f"{len(recs)} games finished, budget {budget}"
    return recs


def oracle_game(oracle, game, search, slot, seq, seed=SEED, **kw):
    if search == "gumbel":
        n, max_actions, m = GUMBEL[game]
        return oracle.selfplay_game_gumbel(game, n, max_actions, m, 50.0, 1.0, seed, slot, seq, **kw)
    R, max_actions, ef, es, c, alpha = PUCT[game]
    return oracle.selfplay_game(game, R, max_actions, ef, es, c, alpha, seed, slot, seq, **kw)


def assert_equals_oracle(r, o, what, keys=ORACLE_KEYS):
    assert (r["T"], r["winner"]) == (o["T"], o["winner"]), (what, r["T"], o["T"], r["winner"], o["winner"])
    for k in keys:
        np.testing.assert_array_equal(np.asarray(r[k]).reshape(np.asarray(o[k]).shape), o[k], err_msg=f"{what} {k}")


def search_kw(game, search):
    from grok_alpha_zero_amd.engine import SEARCH_GUMBEL, SEARCH_PUCT
    if search == "gumbel":
        return dict(search=SEARCH_GUMBEL, gumbel_m=GUMBEL[game][2], c_visit=50.0, c_scale=1.0)
    return dict(search=SEARCH_PUCT)


def hash_engine(game, search, n, budget, lib_path, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    if search == "gumbel":
        R, max_actions, _ = GUMBEL[game]
        ef, es, c, alpha = 0, 0, 0.0, 0.0
    else:
        R, max_actions, ef, es, c, alpha = PUCT[game]
    return SelfPlayEngine(game, n, R, max_actions, ef, es, c, alpha, seed=SEED, hash_salt=SALT, slot_offset=OFFSET, ring_capacity=4 * n, games_budget=budget,
                          lib_path=lib_path, **dict(search_kw(game, search), **kw))


# ------------------------------------------------------------------------------------------------ A.1 self-play against the oracle
def selfplay_case(oracle, game, search, n, lib_path, **kw):
    """n games at once, hash evaluator, budget 2 n: both games of EVERY slot == the oracle's"""
    from conftest import oracle_many
    eng = hash_engine(game, search, n, 2 * n, lib_path, **kw)
    recs = play_budget(eng, 2 * n)
    st = eng.stats()
    eng.close()
    assert {(r["slot"], r["game_seq"]) for r in recs} == {(OFFSET + g, q) for q in (0, 1) for g in range(n)}, sorted((r["slot"], r["game_seq"]) for r in recs)
    assert st["game_stats"][2] == 2 * n and st["plies"] == sum(r["T"] for r in recs) and st["game_groups"] == 1, st
    ora = oracle_many(lambda s, q: oracle_game(oracle, game, search, s, q, hash_salt=SALT), [((r["slot"], r["game_seq"]), {}) for r in recs])
    for r, o in zip(recs, ora):
        assert_equals_oracle(r, o, f"{game} {search} {kw} n = {n} slot {r['slot']} game {r['game_seq']}")
    print(f"self-play {game} {search} {kw}: n = {n}: {len(recs)} games equal the oracle's, {st['waves']} launches", flush=True)
    return recs


# ------------------------------------------------------------------------------------------------ A.3 game groups
def groups_case(oracle, search, n, k, lib_path):
    """Connect4, k game groups of n / k (+ 1) slots, budget 2 n + 1 (no multiple of n: one slot plays a third game, through the `extra`
    term of the groups' own budgets): exactly the games {q n + g < budget}, every one == the oracle's"""
    budget = 2 * n + 1
    eng = hash_engine("Connect4", search, n, budget, lib_path, game_groups=k)
    recs = play_budget(eng, budget, waves=8, after=600)      # (longer than a whole game: a game admitted beyond the budget would finish and show)
    st = eng.stats()
    eng.close()
    assert st["game_groups"] == k, st
    keys = sorted((r["slot"], r["game_seq"]) for r in recs)
    assert keys == sorted((OFFSET + g, q) for q in range(4) for g in range(n) if q * n + g < budget), keys
    assert st["game_stats"][2] == budget and st["plies"] == sum(r["T"] for r in recs), st
    for r in recs:
        o = oracle_game(oracle, "Connect4", search, r["slot"], r["game_seq"], hash_salt=SALT)
        assert_equals_oracle(r, o, f"groups {search} n = {n} k = {k} slot {r['slot']} game {r['game_seq']}")
    print(f"game groups {search}: n = {n} in {k} groups, budget {budget}: {len(recs)} games equal the oracle's", flush=True)


# ------------------------------------------------------------------------------------------------ A.4 repack down to one slot
# name -> game, G and budget on the emulation build, run_iterations, max_actions, search; the explore plies, c_puct_init, alpha, seed, salt and
# slot_offset are test_engine_emu._repack_run's own (4, 3, 2.5, 0.5, 13, 6, 200)
REPACK = {"gumbel-c4": ("Connect4", 12, 30, 16, 42, "gumbel"), "puct-ttt": ("TicTacToe", 12, 30, 16, 9, "puct"), "puct-gmk": ("Gomoku", 9, 27, 225, 6, "puct")}


def stagger(eng, n, waves):
    """Gomoku games cut short by max_actions all take the same number of launches (3 x legal simulations a move, no game ends before its
    cap), so the slots of a fresh engine finish together and a launch never has a half that idles.  This restarts slot g's first game
    from the empty board `waves` launches after slot g - 1's (gaz_engine_set_position with no history: the game keeps its game_seq and
    is the same game), which spreads the finishing times for the rest of the run."""
    for g in range(1, n):
        eng.run_waves(waves)
        eng.set_position(g, [])


def repack_case(oracle, name, lib_path, G=None, budget=None):
    """test_engine_emu._repack_run (it repacks whenever half of the launch idles, down to a launch of one or two slots); the oracle's games
    are played beforehand, several at a time.  Gomoku: with staggered starts (stagger), or no repack would ever happen"""
    from conftest import oracle_many
    from test_engine_emu import _repack_run
    game, G0, budget0, iters, max_actions, search = REPACK[name]
    G, budget = G or G0, budget or budget0
    if search == "gumbel":
        kw = dict(search_kw(game, search), gumbel_m=4)
        fn = lambda s, q: oracle.selfplay_game_gumbel(game, iters, max_actions, 4, 50.0, 1.0, 13, s, q, hash_salt=6)
    else:
        kw = {}
        fn = lambda s, q: oracle.selfplay_game(game, iters, max_actions, 4, 3, 2.5, 0.5, 13, s, q, hash_salt=6)
    keys = [(200 + g, q) for q in range(8) for g in range(G) if q * G + g < budget]
    ora = dict(zip(keys, oracle_many(fn, [(key, {}) for key in keys], threads=12)))
    _repack_run(lib_path, oracle, game, G, budget, iters, max_actions, kw, lambda s, q: ora[(s, q)],
                prepare=(lambda eng: stagger(eng, G, max(200 // G, 3))) if game == "Gomoku" else None)     # (_repack_run looks every 16 launches)
    print(f"repack {name}: G = {G}, budget {budget}: every game equals the oracle's", flush=True)


# ------------------------------------------------------------------------------------------------ B. the one-launch wave with a real network (HIP)
# 24 simulations a move; Connect4: the 2-block network, max_actions 14; Gomoku: max_actions 3 (675 simulations a move whatever is asked for).
NET_FIELDS = ("actions", "root_N", "root_W", "root_P", "policies", "q", "evals", "root_visits", "winner", "T")
NET_ORACLE_KEYS = ("actions", "root_N", "root_visits", "root_W", "root_P", "policies", "values")          # (test_net_widths_gpu._check)
NET_SEED, NET_OFFSET, NET_SIMS, REF_SLOTS = 41, 300, 24, 128
NET_GROUPS = ((3, 3), (5, 2), (7, 3), (67, 2))
# kind -> game, blocks, max_actions, explore first / second, c_puct_init, alpha, Gumbel.
# gomoku: the 1-block network the sizes were asked at.  The Gomoku evaluator joins the tree step's launch only from two residual blocks
# on (resnet.hip fusable(): blocks > 1 — block 0 runs inside the one trunk launch, and a 1-block network has no trunk launch to join), so
# that case asserts fused_wave == 0; gomoku2 is the same with the 2-block network, where the launch is the one under test.
NET = {"puct": ("Connect4", 2, 14, 4, 3, 2.5, 0.5, False), "gumbel": ("Connect4", 2, 14, 0, 0, 0.0, 0.0, True),
       "gomoku": ("Gomoku", 1, 3, 1, 1, 4.5, 0.05, False), "gomoku2": ("Gomoku", 2, 3, 1, 1, 4.5, 0.05, False)}
NET_FUSES = {"puct": 1, "gumbel": 1, "gomoku": 0, "gomoku2": 1}
GUMBEL_M = 7


def net_weights(kind):
    from grok_alpha_zero_amd.net import NETS
    game, blocks, _, _, _, _, _, gumbel = NET[kind]
    return NETS[game](blocks, seed=3, policy_head="linear" if gumbel else "softmax").eval().export_engine_weights()


def net_engine(kind, n, w, budget=None, **kw):
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SEARCH_GUMBEL, SelfPlayEngine
    game, blocks, max_actions, ef, es, c, alpha, gumbel = NET[kind]
    if gumbel:
        kw = dict(dict(search=SEARCH_GUMBEL, gumbel_m=GUMBEL_M, c_visit=50.0, c_scale=1.0, policy_is_logits=True), **kw)
    eng = SelfPlayEngine(game, n, NET_SIMS, max_actions, ef, es, c, alpha, seed=NET_SEED, slot_offset=NET_OFFSET, evaluator=EVAL_RESNET, net_blocks=blocks,
                         ring_capacity=4 * n, games_budget=budget or 2 * n, **dict(dict(game_groups=1), **kw))
    eng.load_weights(w)
    return eng


def by_key(recs):
    out = {(r["slot"], r["game_seq"]): r for r in recs}
    assert len(out) == len(recs), "a game was handed out twice"
    return out


def net_reference(kind, w):
    """the first reference: a regular engine of 128 slots, one batch, separate launches, the same seed, slot_offset and weights, budget 256.
    A game is a function of (seed, slot, game_seq) alone and rows are batch-independent -> {(slot, game_seq): record}"""
    eng = net_engine(kind, REF_SLOTS, w)
    eng.set_fused_wave(False)
    recs = play_budget(eng, 2 * REF_SLOTS)
    st = eng.stats()
    eng.close()
    assert st["fused_wave"] == 0 and st["game_groups"] == 1 and st["fused_faults"] == 0, st
    return by_key(recs)


def assert_equals_reference(got, ref, what):
    for key, r in got.items():
        for f in NET_FIELDS:
            np.testing.assert_array_equal(np.asarray(r[f]), np.asarray(ref[key][f]), err_msg=f"{what} {key} {f}")


class NetOracle:
    """the second reference: the oracle's game of one slot, its evaluator a probe engine's evaluate() on one state at a time"""

    def __init__(self, oracle, kind, w):
        from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
        game, blocks, _, _, _, _, _, gumbel = NET[kind]
        self.oracle, self.kind, self.memo = oracle, kind, {}
        self.probe = SelfPlayEngine(game, 64 if game == "Connect4" else 8, 1, 3, 1, 1, 2.5, 0.5, seed=0, evaluator=EVAL_RESNET, net_blocks=blocks, ring_capacity=0,
                                    policy_is_logits=gumbel)
        self.probe.load_weights(w)

    def ev(self, state):
        p, v, _ = self.probe.evaluate(state[None])
        return p[0], v[0]

    def game(self, slot, seq):
        if (slot, seq) not in self.memo:
            game, _, max_actions, ef, es, c, alpha, gumbel = NET[self.kind]
            if gumbel:
                self.memo[(slot, seq)] = self.oracle.selfplay_game_gumbel(game, NET_SIMS, max_actions, GUMBEL_M, 50.0, 1.0, NET_SEED, slot, seq, evaluator=self.ev)
            else:
                self.memo[(slot, seq)] = self.oracle.selfplay_game(game, NET_SIMS, max_actions, ef, es, c, alpha, NET_SEED, slot, seq, evaluator=self.ev)
        return self.memo[(slot, seq)]

    def close(self):
        self.probe.close()


def net_case(kind, n, w, ref, k=1, net_oracle=None, **kw):
    """n games in k groups with the network in the loop, budget 2 n -> (records, stats).  Witnesses, printed and asserted: fused_wave as
    NET_FUSES says (1: the one-launch wave), no fused_faults, game_groups == k, 2 n records of exactly the slots' two games; every record ==
    the regular engine's; at n = 1 and 67 the first and the last slot == the oracle's."""
    eng = net_engine(kind, n, w, game_groups=k, **kw)
    recs = play_budget(eng, 2 * n, waves=16)
    st = eng.stats()
    eng.close()
    print(f"network {kind} {kw}: n = {n}, groups {st['game_groups']}: fused_wave {st['fused_wave']}, fused_faults {st['fused_faults']}, records {len(recs)}, "
          f"launches {st['waves']}, cache hits {st['cache_hits']}", flush=True)
    assert st["fused_wave"] == NET_FUSES[kind], st
    assert st["fused_faults"] == 0 and st["game_groups"] == k and len(recs) == 2 * n, st
    got = by_key(recs)
    assert set(got) == {(NET_OFFSET + g, q) for q in (0, 1) for g in range(n)}, sorted(got)
    assert_equals_reference(got, ref, f"network {kind} {kw} n = {n} k = {k}")
    if net_oracle is not None and n in (1, 67):
        for slot in sorted({NET_OFFSET, NET_OFFSET + n - 1}):
            for q in (0, 1):
                assert_equals_oracle(got[(slot, q)], net_oracle.game(slot, q), f"network {kind} {kw} n = {n} slot {slot} game {q} (oracle)", NET_ORACLE_KEYS)
        print(f"network {kind} {kw}: n = {n}: slots {sorted({0, n - 1})} equal the oracle's games", flush=True)
    return got, st


def net_sizes_case(oracle, kind, **kw):
    """net_case over every size of the game, one reference and one probe for all of them"""
    w = net_weights(kind)
    ref = net_reference(kind, w)
    no = NetOracle(oracle, kind, w)
    for n in sizes_of(NET[kind][0]):
        net_case(kind, n, w, ref, net_oracle=no, **kw)
    no.close()


def net_groups_case(kind):
    w = net_weights(kind)
    ref = net_reference(kind, w)
    for n, k in NET_GROUPS:
        net_case(kind, n, w, ref, k=k)


def net_repack_case(kind, gpb, G=67, budget=201):
    """the one-launch wave + repack to one slot: repack whenever remaining * 2 <= launch and launch > 1; the records == those of a
    regular engine (separate launches, never repacked).  Witnesses: fused_wave == 1 at the end; the launch sizes visited include an odd
    one, one below queue_gpb (`gpb`: a launch of nothing but a partial tree block) and 1."""
    w = net_weights(kind)
    gomoku = NET[kind][0] == "Gomoku"                # (its games finish together unless their starts are staggered: stagger)
    reg = net_engine(kind, G, w, budget=budget)
    reg.set_fused_wave(False)
    if gomoku:
        stagger(reg, G, 16)
    ref = by_key(play_budget(reg, budget))
    assert reg.stats()["fused_wave"] == 0
    reg.close()
    eng = net_engine(kind, G, w, budget=budget)
    if gomoku:
        stagger(eng, G, 16)
    recs, launch, sizes = [], G, []
    for _ in range(100000):
        eng.run_waves(8)
        recs += eng.drain_finished()
        remaining = budget - len(recs)
        if remaining == 0:
            break
        if remaining * 2 <= launch and launch > 1:
            active, launch = eng.repack()
            assert active <= remaining and launch == max(active, 1)
            sizes.append(launch)
    st = eng.stats()
    eng.close()
    print(f"network {kind} repack: G = {G}, budget {budget}: launch sizes {[G] + sizes}, fused_wave {st['fused_wave']}, fused_faults {st['fused_faults']}, "
          f"records {len(recs)}", flush=True)
    assert st["fused_wave"] == 1 and st["fused_faults"] == 0 and len(recs) == budget, st
    visited = [G] + sizes
    assert any(s % 2 == 1 for s in visited) and any(s < gpb for s in visited) and visited[-1] == 1, visited
    got = by_key(recs)
    assert set(got) == set(ref) == {(NET_OFFSET + g, q) for q in range(3) for g in range(G)}
    assert_equals_reference(got, ref, f"network {kind} repack")


def net_giveup_case(n):
    """the bounded wait's give-up path on a partial tile (PUCT Connect4: n = 5 is 2 + 2 + 1 boards, n = 17 eight tiles + 1 board):
    gaz_engine_debug_fused_fault(2) after a few waves makes every second trunk workgroup of the real launches stop waiting, as
    test_fused_launch_bounded_wait_recovers_without_changing_games does at 1600 games.  The games == an undisturbed engine's (and the
    regular engine's), fused_faults > 0, and the engine falls back to separate launches."""
    w = net_weights("puct")
    ref = net_reference("puct", w)
    got = []
    for fault in (True, False):
        eng = net_engine("puct", n, w)
        eng.run_waves(10); eng.synchronize()
        assert eng.stats()["fused_wave"] == 1
        if fault:
            eng.debug_fused_fault(2)
            eng.run_waves(48)                          # no host synchronisation in between
            st = eng.stats()
            assert st["fused_faults"] > 0 and st["fused_wave"] == 0, st
        recs = play_budget(eng, 2 * n, waves=16)
        st = eng.stats()
        assert st["fused_wave"] == (0 if fault else 1), st
        print(f"network puct give-up: n = {n}, disturbed {fault}: fused_wave {st['fused_wave']}, fused_faults {st['fused_faults']}, records {len(recs)}", flush=True)
        got.append(by_key(recs))
        eng.close()
    a, b = got
    assert set(a) == set(b) == {(NET_OFFSET + g, q) for q in (0, 1) for g in range(n)}
    assert_equals_reference(a, b, f"give-up n = {n} against the undisturbed engine")
    assert_equals_reference(a, ref, f"give-up n = {n} against the regular engine")

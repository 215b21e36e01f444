"""The searches on tied, zero and saturated evaluator outputs (tests/degenerate_eval.py): the case bodies that the CPU suite runs on the
emulation build (tests/test_degenerate_emu.py) and the -m gpu suite on the HIP build (tests/test_degenerate_gpu.py): `lib_path` = the
emulation library, or None for the product library.

The cross-lane tie rules (team_argmax / wave_argmax and their _u32 forms: lowest index; the rank sort of make_priors: higher original
index first; the Gumbel top-m and halving argsorts: stable ascending) are serial loops on the one-lane emulation and butterflies on the
HIP build.  The evaluators reach the engine through GAZ_EVAL_EXTERNAL (one host round trip per launch) and the oracle / the Python models
as their `evaluator`; every comparison is exact.  A case that never sees a tie proves nothing, so every case counts its ties on the
ORACLE's or the MODEL's side and asserts them.  The Dirichlet noise of every node breaks nearly all ties among the priors themselves:
the self-play cases carry tied visit counts into the kernels, the leaf_batch cases without noise carry tied priors.

The zero-mass rule (DESIGN.md "Oracle"): a node whose legal policy entries sum to no positive finite number gets the prior 1 / n_legal
for every legal action.  The `zeromass` cases also replay every record with grok_alpha_zero_amd.games (every action legal when played) and
want finite root_P / policies."""
import numpy as np

import selfplay_support
from degenerate_eval import Constant, Evaluator
from selfplay_support import A_OF, MAXT, SLOTS64, slots_for

PUCT_KEYS = ("actions", "root_N", "root_W", "root_P", "policies", "q", "root_visits", "evals")
PH_WAIT_HOST, PH_HALT = 5, 8                       # grok_alpha_zero_amd.engine
TIE_KINDS = ("uniform", "dups", "zeros", "saturated")
MIN_TIED_PLIES, MIN_ZEROMASS_ROWS = 10, 20


# ------------------------------------------------------------------------------------------------ the external evaluator loop
def serve_wave(eng, ev):
    """one launch of a GAZ_EVAL_EXTERNAL engine: the requested rows answered by `ev`, the others NaN (nobody reads them) -> pending"""
    eng.wave_begin()
    x, pend = eng.read_batch()
    pol = np.full((eng.batch_rows, eng.A), np.nan, np.float32); val = np.full(eng.batch_rows, np.nan, np.float32)
    rows = np.flatnonzero(pend)
    if rows.size:
        pol[rows], val[rows] = ev.many(x[rows])
    eng.write_outputs(pol, val)
    return pend


def first_games(eng, ev, n_slots, launches=400000, every=8):
    """a free-running external-evaluator engine until every slot's first game is there -> {slot: record}; drained after every `every` launches"""
    def advance():
        for _ in range(every):
            serve_wave(eng, ev)
    return selfplay_support.first_games(eng, n_slots, rounds=launches // every, advance=advance)


def drive_move(eng, ev, launches=200000):
    """one search of every game of a sync-mode external-evaluator engine -> the launches each game's move took (int [G])"""
    eng.start_search()
    ended = np.zeros(eng.n_games, np.int64)
    for k in range(1, launches):
        eng.wave_begin()
        x, pend = eng.read_batch()
        ph = eng.root_stats()["phase"]
        ended[(ph == PH_WAIT_HOST) & (ended == 0)] = k
        rows = np.flatnonzero(pend)
        if rows.size == 0 and np.isin(ph, (PH_WAIT_HOST, PH_HALT)).all():
            return ended
        pol = np.full((eng.batch_rows, eng.A), np.nan, np.float32); val = np.full(eng.batch_rows, np.nan, np.float32)
        pol[rows], val[rows] = ev.many(x[rows])
        eng.write_outputs(pol, val)
    raise AssertionError("the search did not finish")


# ------------------------------------------------------------------------------------------------ witnesses
def explores(ply, first, second):
    """tau = 1 at this ply (Self_Play.py:86-95): the mover still samples its move"""
    return (ply // 2 < first) if ply % 2 == 0 else ((ply + 1) // 2 < second)


def tied_plies(rec, first, second):
    """plies past the exploration plies whose root_N has a tied maximum: the move there is the tie rule's"""
    n = 0
    for ply in range(rec["T"]):
        row = rec["root_N"][ply]
        n += (not explores(ply, first, second)) and int(np.count_nonzero(row == row.max())) >= 2
    return n


def assert_actions_legal(game, actions, what=""):
    """replay with grok_alpha_zero_amd.games: every action legal when it was played, and nothing played after the game ended"""
    from grok_alpha_zero_amd.games import GAMES
    G = GAMES[game]
    board, player, hist = np.zeros((G.H, G.W), np.int8), -1, []
    for ply, a in enumerate(actions):
        legal = {G.action_to_index(x) for x in G.get_legal_actions_MCTS(board, 0, None)}
        assert int(a) in legal, f"{what}: ply {ply} plays {int(a)}, legal {sorted(legal)}"
        G.do_action_MCTS(board, G.index_to_action(int(a)), player); hist.append(int(a))
        over = G.check_win_MCTS(board, player, np.array([G.index_to_action(h) for h in hist])) != -2
        assert not over or ply == len(actions) - 1, f"{what}: ply {ply} ended the game, {len(actions)} plies recorded"
        player = -player


def assert_finite(rec, what=""):
    for k in ("root_P", "policies", "q", "root_W"):
        assert np.isfinite(np.asarray(rec[k])).all(), f"{what}: {k} is not finite"


def check_witness(name, kind, ev, tied=None, collisions=None):
    w = ev.witness()
    print(f"{name}: evaluator rows {w['rows']} (two equal legal priors {w['tied']}, an exactly zero legal prior {w['zero']}, zero legal mass "
          f"{w['zeromass']})" + (f", tied plies {tied}" if tied is not None else "") + (f", launches ended by a collision {collisions}" if collisions is not None else ""),
          flush=True)
    if kind in ("uniform", "dups", "saturated"):
        assert w["tied"] > 0, (name, w)                                   # (every row with two or more legal actions: asserted per row in Evaluator)
    if kind == "zeros":
        assert w["zero"] > 0, (name, w)
    if kind == "zeromass":
        assert w["zeromass"] >= MIN_ZEROMASS_ROWS, f"{name}: {w['zeromass']} zero-mass rows: pick another seed / more iterations"
    else:
        assert w["zeromass"] == 0, (name, w)
    if collisions is not None:
        assert collisions >= 1, f"{name}: no launch ended on a collision"


def assert_record_equals_oracle(r, o, keys, what):
    assert (r["T"], r["winner"]) == (o["T"], o["winner"]), (what, r["T"], o["T"], r["winner"], o["winner"])
    for k in keys:
        np.testing.assert_array_equal(np.asarray(r[k]).reshape(np.asarray(o[k]).shape), o[k], err_msg=f"{what} {k}")


# ------------------------------------------------------------------------------------------------ a. PUCT self-play, two trees
# game -> run_iterations, max_actions, explore first / second, c_puct_init, dirichlet_alpha, seed.  Chosen on the CPU so that the oracle
# alone meets the witness condition below at the emulation suite's sizes and at the HIP suite's (Gomoku runs 3 x legal = 675 - 3 ply
# simulations a move whatever run_iterations says; its flat Dirichlet noise, alpha = 10, keeps the 225 visit counts close together).
PUCT = {"TicTacToe": (16, 9, 1, 1, 1.25, 1.0, 3), "Connect4": (24, 42, 2, 2, 2.5, 0.5, 11), "Gomoku": (8, 6, 1, 1, 2.5, 10.0, 1)}
# Gomoku runs the kind `uniform` only: with unequal priors or non-zero values the maximum of 225 visit counts after 675 simulations is
# practically never shared (measured on the oracle, alpha 1 to 1000, with and without exploration plies: 0 to 3 tied plies in 24), so the
# kinds dups / zeros / saturated could not meet the witness below and would prove nothing about a tie.
PUCT_KINDS = {"TicTacToe": TIE_KINDS, "Connect4": TIE_KINDS, "Gomoku": ("uniform",)}
EMU_GAMES = {"TicTacToe": 32, "Connect4": 12, "Gomoku": 4}
HIP_SLOTS = {"TicTacToe": tuple(range(64)), "Connect4": tuple(range(64)), "Gomoku": SLOTS64}     # of 64 games at once; all contain SLOTS64


def puct_ties_case(oracle, game, G, lib_path, slots=None):
    """puct_selfplay_case for the tie kinds of one game (PUCT_KINDS).  The witness, counted on the ORACLE's records of the compared slots:
    plies past the exploration plies whose root_N has a tied maximum — there the played move, the policy target's argmax and q are the
    tie rule's (np.argmax over the visits in slot order, the slot order itself from the rank sort) — at least MIN_TIED_PLIES of them
    for EVERY kind.  (The Dirichlet noise of every node breaks nearly all ties among the priors themselves before the rank sort; what
    this case carries into the kernels is tied visit counts.  Tied priors reach them in leaf_batch_case without noise.)"""
    tied = {kind: puct_selfplay_case(oracle, game, kind, G, lib_path, slots)[1] for kind in PUCT_KINDS[game]}
    print(f"PUCT {game}: plies with a tied maximum of root_N past the exploration plies {tied}", flush=True)
    assert min(tied.values()) >= MIN_TIED_PLIES, f"PUCT {game}: {tied}: pick another seed / more games"
    return tied


def puct_selfplay_case(oracle, game, kind, G, lib_path, slots=None):
    """continuous self-play, both trees, Dirichlet noise on: the first game of the compared slots == oracle.selfplay_game(evaluator=ev)"""
    from grok_alpha_zero_amd.engine import EVAL_EXTERNAL, SelfPlayEngine
    R, max_actions, ef, es, c_init, alpha, seed = PUCT[game]
    ev = Evaluator(kind, A_OF[game])
    eng = SelfPlayEngine(game, G, R, max_actions, ef, es, c_init, alpha, seed=seed, evaluator=EVAL_EXTERNAL, ring_capacity=4 * G, games_budget=G,
                         lib_path=lib_path)
    first = first_games(eng, ev, G)
    eng.close()
    ora = Evaluator(kind, A_OF[game])                                     # the witnesses are the oracle's own
    tied = 0
    for s in slots or slots_for(G):
        o = oracle.selfplay_game(game, R, max_actions, ef, es, c_init, alpha, seed, s, 0, evaluator=ora)
        what = f"PUCT {game} {kind} slot {s}"
        tied += tied_plies(o, ef, es)
        if kind == "zeromass":
            assert_actions_legal(game, first[s]["actions"], what); assert_finite(first[s], what); assert_finite(o, what + " (oracle)")
        assert_record_equals_oracle(first[s], o, PUCT_KEYS, what)
    check_witness(f"PUCT {game} {kind}", kind, ora, tied=tied)
    return first, tied


# ------------------------------------------------------------------------------------------------ b. Gumbel self-play
# game -> run_iterations, max_actions, m, seed
GUMBEL = {"TicTacToe": (32, 9, 4, 23), "Connect4": (32, 42, 7, 23), "Gomoku": (48, 8, 16, 23)}
GUMBEL_EMU_GAMES = {"TicTacToe": 8, "Connect4": 4, "Gomoku": 4}
# kind, gumbel noise, stablemax.  Without noise and with equal logits every top-m and every halving step is a tie.
GUMBEL_CONFIGS = (("uniform", False, False), ("uniform", True, False), ("uniform", False, True), ("dups", False, False), ("dups", True, True),
                  ("zeros", False, True), ("saturated", False, False), ("zeromass", False, False), ("zeromass", True, True))
GUMBEL_KEYS = ("actions", "root_N", "root_W", "root_P", "policies", "q", "root_visits", "evals")


def gumbel_selfplay_case(oracle, game, config, G, lib_path, slots=None):
    """the first game of the compared slots == oracle.selfplay_game_gumbel(evaluator=ev) at gumbel_batch = 1 and = m (the same games).
    zeromass: the Gumbel search reads the legal entries as logits WITHOUT normalising them, so a zero-mass row is a row of equal logits
    (0.0) — softmax gives 1 / n_legal, nothing is NaN; the case pins that (finite records, legal actions, equal to the oracle)."""
    from grok_alpha_zero_amd.engine import EVAL_EXTERNAL, SEARCH_GUMBEL, SelfPlayEngine
    kind, noise, stablemax = config
    R, max_actions, m, seed = GUMBEL[game]
    name = f"Gumbel {game} {kind} noise {int(noise)} stablemax {int(stablemax)}"
    got = {}
    for K in (1, m):
        ev = Evaluator(kind, A_OF[game])
        eng = SelfPlayEngine(game, G, R, max_actions, 0, 0, 0.0, 0.0, seed=seed, evaluator=EVAL_EXTERNAL, ring_capacity=4 * G, games_budget=G,
                             search=SEARCH_GUMBEL, gumbel_m=m, c_visit=50.0, c_scale=1.0, gumbel_stablemax=stablemax, use_gumbel_noise=noise,
                             gumbel_batch=K, lib_path=lib_path)
        assert eng.batch_rows == G * K
        got[K] = first_games(eng, ev, G)
        eng.close()
    ora = Evaluator(kind, A_OF[game])
    for s in slots or slots_for(G):
        o = oracle.selfplay_game_gumbel(game, R, max_actions, m, 50.0, 1.0, seed, s, 0, evaluator=ora, stablemax=stablemax, gumbel_noise=noise)
        for K in (1, m):
            what = f"{name} gumbel_batch {K} slot {s}"
            if kind == "zeromass":
                assert_actions_legal(game, got[K][s]["actions"], what); assert_finite(got[K][s], what); assert_finite(o, what + " (oracle)")
            assert_record_equals_oracle(got[K][s], o, GUMBEL_KEYS, what)
    check_witness(name, kind, ora)
    return got


# ------------------------------------------------------------------------------------------------ c. leaf-batched PUCT, d. tree readout
# game -> run_iterations, the fixed moves, c_puct_init, dirichlet_alpha, seed.  Chosen on the CPU so that the MODEL alone collides in every
# case of both suites: a collision needs a reserved child that still beats its siblings after the virtual loss — spiky noise (Connect4), a
# small c_puct (TicTacToe); Gomoku's 225-wide nodes collide only at K = 16 with a very large c_puct and spiky noise (nothing at K = 4).
LEAF = {"TicTacToe": (96, [4, 0, 8], 0.5, 0.5, 2), "Connect4": (48, [3, 3, 2, 4], 2.5, 0.03, 31), "Gomoku": (3 * 225 + 20, [112], 30.0, 0.03, 31)}
LEAF_TREE_SIMS = 32                                # (at 4 terminal completions a launch, launches of K = 4 end on that limit before they collide)


def duplicate_prior_nodes(tree):
    """(nodes of a model tree whose children hold two or more EQUAL priors, nodes with two or more children) — terminal parents left out"""
    from leaf_batch_model import _Node
    dup = total = 0
    stack = [tree.root]
    while stack:
        n = stack.pop()
        stack += [c for c in n.child if isinstance(c, _Node)]
        if not n.terminal and len(n.act) >= 2:
            total += 1; dup += np.unique(n.P).size < n.P.size
    return dup, total


def leaf_batch_case(oracle, game, kind, K, G, lib_path, forced_k=0.0, readout=False, slots=None, dirichlet=True):
    """G games at once, sync + single tree, leaf_batch = K, every game playing the same fixed moves on its own RNG streams.  After every
    move, for the compared slots: root N / W / P / root visits and the launches the move took == leaf_batch_model.Tree(evaluator=ev) —
    with forced_k > 0 forced_playouts_model.ForcedTree, and the policy row == the pruned target of the model's raw rows.  readout (d.):
    read_trees and principal_variations == the model's tree, and the principal variation walks through a tied visit maximum.
    dirichlet = False: no noise, so the evaluator's equal priors reach the rank sort and best_puct_slot as they are — asserted on the
    MODEL's trees: every node with two or more children holds equal priors (with noise the count is printed, nothing is claimed)."""
    from grok_alpha_zero_amd.engine import EVAL_EXTERNAL, SelfPlayEngine
    from forced_playouts_cases import expected_policy
    from forced_playouts_model import ForcedTree
    import tree_cases
    R, moves, c_init, alpha, seed = LEAF[game]
    name = f"leaf_batch {K} {game} {kind}" + (f" forced_playouts_k {forced_k}" if forced_k else "") + (" readout" if readout else "") + \
        ("" if dirichlet else " no Dirichlet noise")
    ev = Evaluator(kind, A_OF[game])
    eng = SelfPlayEngine(game, G, R, MAXT[game], 0, 0, c_init, alpha, seed=seed, use_dirichlet=dirichlet, evaluator=EVAL_EXTERNAL, sync_moves=True, single_tree=True,
                         nodes_per_tree=(len(moves) + 1) * (max(R, 3 * A_OF[game]) + 4) + 64, compact_trees=-1, max_tree_sims_per_wave=LEAF_TREE_SIMS, tau=0.0,
                         leaf_batch=K, forced_playouts_k=forced_k, lib_path=lib_path)
    assert eng.batch_rows == G * K
    mev = Evaluator(kind, A_OF[game])                                     # the witnesses are the model's own
    slots = tuple(slots or slots_for(G))
    models = {s: ForcedTree(oracle, game, K, seed, slot=s, c_puct_init=c_init, dirichlet_alpha=alpha, use_dirichlet=dirichlet, evaluator=mev, max_tree_sims=LEAF_TREE_SIMS,
                            forced_k=forced_k)
              for s in slots}
    collisions = pv_ties = 0
    for ply, m in enumerate(list(moves) + [None]):
        ended = drive_move(eng, ev)
        st = eng.root_stats()
        if readout:
            trees = eng.read_trees(list(slots))
            pv = eng.principal_variations(6, first_action=st["chosen"]); pv_free = eng.principal_variations(6)
        for i, (s, model) in enumerate(models.items()):
            terminal = model.root.terminal
            w = model.run(R)
            what = f"{name} slot {s} ply {ply}"
            np.testing.assert_array_equal(st["N"][s], w["N"], err_msg=what); np.testing.assert_array_equal(st["W"][s], w["W"], err_msg=what)
            np.testing.assert_array_equal(st["P"][s], w["P"], err_msg=what)
            assert int(st["root_visits"][s]) == w["root_visits"], what
            assert int(ended[s]) == len(w["launches"]), (what, int(ended[s]), len(w["launches"]))
            assert model.inflight_nodes() == 0
            assert np.isfinite(st["P"][s]).all() and np.isfinite(st["policy"][s]).all(), what
            collisions += w["collisions"]
            if forced_k:
                pol = expected_policy(w["N"], w["W"], w["P"], w["root_visits"], forced_k, c_init, True, terminal)
                np.testing.assert_array_equal(st["policy"][s], pol, err_msg=what + " policy")
            if readout:
                want = tree_cases.model_export(model)
                tree_cases.assert_trees_equal(trees[i].nodes, trees[i].edges, *want, what=what)
                tree_cases.assert_consistent(trees[i], what)
                tree_cases.assert_pv_equals(pv, s, tree_cases.host_pv(*want, 6, int(st["chosen"][s])), what + " pv")
                tree_cases.assert_pv_equals(pv_free, s, tree_cases.host_pv(*want, 6), what + " pv most visited")
                pv_ties += pv_tie_steps(*want, 6)
        assert eng.stats()["reserved_children"] == 0
        if m is None:
            break
        eng.apply_moves([m] * G)
        for model in models.values():
            model.play(m)
    eng.close()
    check_witness(name, kind, mev, collisions=collisions if K > 1 else None)
    dup, total = (sum(x) for x in zip(*(duplicate_prior_nodes(m) for m in models.values())))
    print(f"{name}: nodes of the model's trees with two equal priors {dup} of {total}", flush=True)
    if not dirichlet:
        assert kind in ("uniform", "dups", "saturated") and dup == total > 0, f"{name}: {dup} of {total} nodes hold equal priors"
    if readout:
        print(f"{name}: steps of the principal variations taken at a tied visit maximum {pv_ties}", flush=True)
        assert pv_ties >= 1, f"{name}: no principal variation walks through a tie"
    return collisions


def pv_tie_steps(nodes, edges, max_len):
    """steps of the most visited line (tree_cases.host_pv's walk) at which the maximum of N is shared by two or more edges"""
    n, i, steps = 0, 0 if len(nodes) else -1, 0
    while i >= 0 and steps < max_len:
        e = edges[int(nodes["edge0"][i]):int(nodes["edge0"][i]) + int(nodes["n_actions"][i])]
        if len(e) == 0:
            break
        s = int(np.argmax(e["N"]))
        n += int(np.count_nonzero(e["N"] == e["N"][s])) >= 2 and e["N"][s] > 0
        steps += 1
        if e["child"][s] < 0 or e["N"][s] == 0:
            break
        i = int(e["child"][s])
    return n


# ------------------------------------------------------------------------------------------------ e. the production launch shape (HIP build)
def constant_network(game, gumbel):
    """a one-block network whose heads ignore the trunk: the last dense layer's weights of both heads are zero, the policy bias has repeated
    entries, the value bias is free -> the same (policy, value) for every state, with exact duplicates.  -> engine weights"""
    from grok_alpha_zero_amd.net import NETS
    w = NETS[game](1, seed=0, policy_head="linear" if gumbel else "softmax").eval().export_engine_weights()
    last_p = "p.d3" if game == "Connect4" else "p.d2"
    A = A_OF[game]
    w[last_p + ".w"] = np.zeros_like(w[last_p + ".w"]); w["v.d3.w"] = np.zeros_like(w["v.d3.w"])
    w[last_p + ".bias"] = (np.array([0.5, -0.25, 0.5, 0.0, -0.25, 0.5, 0.0], np.float32)[np.arange(A) % 7]).astype(np.float32)
    w["v.d3.bias"] = np.full_like(w["v.d3.bias"], 0.375)
    return w


def constant_pair(game, weights, gumbel):
    """the one (policy, value) pair of constant_network, read back through a probe engine's evaluate() on a few different states"""
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SelfPlayEngine
    probe = SelfPlayEngine(game, 8, 1, MAXT[game], 0, 0, 2.5, 0.5, seed=0, evaluator=EVAL_RESNET, net_blocks=1, ring_capacity=0, policy_is_logits=gumbel)
    probe.load_weights(weights)
    x = np.random.default_rng(5).integers(-1, 2, size=(5, probe.H, probe.W, probe.Cc)).astype(np.int8)
    p, v, _ = probe.evaluate(x)
    probe.close()
    assert np.isfinite(p).all() and np.isfinite(v).all()
    assert (p == p[0]).all() and (v == v[0]).all(), "the heads do not ignore the trunk"
    assert np.unique(p[0]).size <= 3 < p[0].size, "the policy has no exact duplicates"
    return Constant(p[0], v[0])


def network_case(oracle, game, gumbel=False, G=256, **kw):
    """self-play with the constant network in the loop (EVAL_RESNET: for Connect4 the fused tree-and-trunk launch): the records of the
    slots SLOTS64 of every game group == the oracle's with the constant evaluator"""
    from grok_alpha_zero_amd.engine import EVAL_RESNET, SEARCH_GUMBEL, SelfPlayEngine
    w = constant_network(game, gumbel)
    ev = constant_pair(game, w, gumbel)
    R, max_actions, ef, es, c_init, alpha, seed = PUCT[game]
    m = GUMBEL[game][2]
    if game == "Gomoku":
        R, max_actions = 3 * 225, 6
    if gumbel:
        R = GUMBEL[game][0]
        ef = es = 0
        kw = dict(kw, search=SEARCH_GUMBEL, gumbel_m=m, c_visit=50.0, c_scale=1.0, policy_is_logits=True)
    eng = SelfPlayEngine(game, G, R, max_actions, ef, es, 0.0 if gumbel else c_init, 0.0 if gumbel else alpha, seed=seed, evaluator=EVAL_RESNET, net_blocks=1,
                         ring_capacity=4 * G, games_budget=G, **kw)
    eng.load_weights(w)
    first, seq0 = {}, int(eng.cfg.first_game_seq)
    for _ in range(40000):
        eng.run_waves(32)
        for r in eng.drain_finished():
            if r["game_seq"] == seq0:
                first[r["slot"]] = r
        if len(first) == G:
            break
    st = eng.stats()
    eng.close()
    assert len(first) == G, f"only {len(first)} of {G} games finished"
    assert st["fused_faults"] == 0, st
    groups = st["game_groups"]
    per = G // groups
    slots = sorted({g * per + s for g in range(groups) for s in SLOTS64 if s < per})
    tied = 0
    for s in slots:
        what = f"network {game} {'Gumbel' if gumbel else 'PUCT'} {kw} slot {s}"
        if gumbel:
            o = oracle.selfplay_game_gumbel(game, R, max_actions, m, 50.0, 1.0, seed, s, 0, evaluator=ev)
        else:
            o = oracle.selfplay_game(game, R, max_actions, ef, es, c_init, alpha, seed, s, 0, evaluator=ev)
            tied += tied_plies(o, ef, es)
        assert_record_equals_oracle(first[s], o, PUCT_KEYS, what)
    print(f"network {game} {'Gumbel' if gumbel else 'PUCT'} {kw}: {len(slots)} slots of {G} games equal the oracle, stats {st}, tied plies {tied}", flush=True)
    return st, tied

"""-m gpu: the leaf-batched PUCT search (gaz_engine_config.leaf_batch = K) of the HIP build against the test model of
tests/leaf_batch_model.py (anchored to the oracle at K = 1 by tests/test_leaf_batch_emu.py).  Bit-equal: no tolerance.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py."""
import os
import sys

import numpy as np
import pytest

from gpu_step import STEPS
from selfplay_support import MAXT, SLOTS64 as SLOTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the cases (run in the child)
def _hash_case(game, K, iters, moves, c_init, alpha, max_tree_sims):
    """64 games at once (sync + single tree, hash evaluator); every game plays the same fixed moves, the RNG streams differ by slot.  The
    slots of SLOTS against the model: root N / W / P / root_visits after every move, and the launches every move took."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, PH_WAIT_HOST
    from oracle import gaz_oracle as O
    from leaf_batch_model import Tree
    O.build()
    G, seed, salt = 64, 31, 8
    eng = SelfPlayEngine(game, G, iters, MAXT[game], 0, 0, c_init, alpha, seed=seed, hash_salt=salt, sync_moves=True, single_tree=True,
                         nodes_per_tree=(len(moves) + 1) * (max(iters, 3 * MAXT[game]) + 4) + 64, compact_trees=-1,
                         max_tree_sims_per_wave=max_tree_sims, tau=0.0, leaf_batch=K)
    assert eng.batch_rows == G * K and eng.stats()["fused_wave"] == 0
    models = {s: Tree(O, game, K, seed, slot=s, c_puct_init=c_init, dirichlet_alpha=alpha, hash_salt=salt, max_tree_sims=max_tree_sims) for s in SLOTS}
    for m in list(moves) + [None]:
        eng.start_search()
        ended = np.zeros(G, np.int64)
        for wave in range(1, 100000):
            eng.run_waves(1)
            ph = eng.root_stats()["phase"]
            ended[(ph == PH_WAIT_HOST) & (ended == 0)] = wave
            if (ended > 0).all():
                break
        st = eng.root_stats()
        for s, model in models.items():
            w = model.run(iters)
            what = f"{game} K {K} slot {s}"
            np.testing.assert_array_equal(st["N"][s], w["N"], err_msg=what); np.testing.assert_array_equal(st["W"][s], w["W"], err_msg=what)
            np.testing.assert_array_equal(st["P"][s], w["P"], err_msg=what)
            assert int(st["root_visits"][s]) == w["root_visits"], what
            assert int(ended[s]) == len(w["launches"]), (what, int(ended[s]), len(w["launches"]))
            assert model.inflight_nodes() == 0
        assert eng.stats()["reserved_children"] == 0          # NodeHdr::pad[0] summed over every node record of the 64 games
        print(f"{game} K {K} max_tree_sims {max_tree_sims}: move ok, launches of the sampled slots {[int(ended[s]) for s in SLOTS]}", flush=True)
        if m is None:
            break
        eng.apply_moves([m] * G)
        for model in models.values():
            model.play(m)
    eng.close()


def _resnet_case():
    """Gomoku, one game, the 10-block network, K = 16, 400 iterations, 3 moves: the model's evaluator is a probe engine's evaluate() on
    single rows (rows of a batch are independent bit for bit), as tests/test_composition_gpu.py serves the oracle."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import NETS
    from oracle import gaz_oracle as O
    from leaf_batch_model import Tree
    O.build()
    K, iters, seed, moves = 16, 400, 5, [112, 113]
    w = NETS["Gomoku"](10, seed=0).eval().export_engine_weights()
    eng = SelfPlayEngine("Gomoku", 1, iters, 225, 0, 0, 4.5, 0.05, seed=seed, evaluator=EVAL_RESNET, net_blocks=10, net_filters=128, sync_moves=True,
                         single_tree=True, ring_capacity=0, tau=0.0, max_tree_sims_per_wave=32, leaf_batch=K)
    eng.load_weights(w)
    probe = SelfPlayEngine("Gomoku", 8, 1, 225, 0, 0, 4.5, 0.05, seed=0, evaluator=EVAL_RESNET, net_blocks=10, net_filters=128, ring_capacity=0)
    probe.load_weights(w)

    def ev(state):
        p, v, _ = probe.evaluate(state[None])
        return p[0], v[0]
    model = Tree(O, "Gomoku", K, seed, c_puct_init=4.5, dirichlet_alpha=0.05, evaluator=ev, max_tree_sims=32)
    for m in moves + [None]:
        eng.start_search(); eng.run_move()
        st, want = eng.root_stats(), model.run(iters)
        np.testing.assert_array_equal(st["N"][0], want["N"]); np.testing.assert_array_equal(st["W"][0], want["W"])
        np.testing.assert_array_equal(st["P"][0], want["P"])
        assert int(st["root_visits"][0]) == want["root_visits"] and eng.stats()["reserved_children"] == 0
        print(f"Gomoku 10 blocks K {K}: move ok, {len(want['launches'])} launches for {iters} simulations", flush=True)
        if m is None:
            break
        eng.apply_moves([m]); model.play(m)
    eng.close(); probe.close()


HASH_CASES = {
    "c4-k4": ("Connect4", 4, 120, [3, 3, 2, 4], 2.5, 0.5, 4), "c4-k32": ("Connect4", 32, 200, [3, 3, 2, 4], 2.5, 0.5, 4),
    "c4-k32-mts32": ("Connect4", 32, 200, [3, 0, 3, 0, 2], 2.5, 0.5, 32),
    "ttt-k4": ("TicTacToe", 4, 40, [4, 0, 8], 1.25, 1.0, 4), "ttt-k32": ("TicTacToe", 32, 60, [4, 0, 8], 1.25, 1.0, 4),
    "gmk-k4": ("Gomoku", 4, 3 * 225 + 20, [112, 113], 2.5, 0.05, 4), "gmk-k32": ("Gomoku", 32, 3 * 225 + 20, [112, 113], 2.5, 0.05, 32),
}


@pytest.mark.parametrize("case", sorted(HASH_CASES))
def test_engine_equals_model_hash_evaluator(case):
    STEPS.run(__file__, case, 600 if case.startswith("gmk") else 240)


def test_gomoku_10_blocks_k16_equals_model():
    STEPS.run(__file__, "resnet-gmk-k16", 600)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    name = sys.argv[1]
    if name == "resnet-gmk-k16":
        _resnet_case()
    else:
        _hash_case(*HASH_CASES[name])
    print("ok", flush=True)

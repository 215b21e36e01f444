"""-m gpu: reading search trees back (gaz_engine_read_trees / gaz_engine_read_pv) on the HIP build: the case bodies of tests/tree_cases.py
that tests/test_tree_readout_emu.py runs on the emulation build, with 64 games at once and the sampled slots at the first and last team
of a wavefront and both ends of the batch.  The PUCT trees are held against the whole-tree model of tests/leaf_batch_model.py, node for
node and edge for edge.  Bit-equal: no tolerance.

Every GPU case runs as a child step of the shared runner, tests/gpu_step.py."""
import os
import sys

import pytest

from gpu_step import STEPS
from selfplay_support import SLOTS64 as SLOTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the cases (run in the child)
def _oracle():
    from oracle import gaz_oracle as O
    O.build()
    return O


def _resnet_case():
    """Gomoku, one game, the 10-block network, leaf_batch = 16, 400 iterations, the first move and the re-rooted second: the export against the
    model, whose evaluator is a probe engine's evaluate() on single rows (rows of a batch are independent bit for bit), as
    tests/test_leaf_batch_gpu.py serves it."""
    import tree_cases as TC
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import NETS
    from leaf_batch_model import Tree
    O = _oracle()
    K, iters, seed = 16, 400, 5
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
    for m in [112, None]:
        eng.start_search(); eng.run_move()
        model.run(iters)
        t = eng.read_trees([0])[0]
        TC.assert_trees_equal(t.nodes, t.edges, *TC.model_export(model), what="Gomoku 10 blocks")
        TC.assert_consistent(t)
        st = eng.root_stats()
        TC.assert_pv_equals(eng.principal_variations(8, first_action=st["chosen"]), 0, TC.host_pv(t.nodes, t.edges, 8, int(st["chosen"][0])))
        print(f"Gomoku 10 blocks K {K}: export of {len(t)} nodes / {len(t.edges)} edges equals the model", flush=True)
        if m is None:
            break
        eng.apply_moves([m]); model.play(m)
    eng.close(); probe.close()


def _run(name):
    import tree_cases as TC
    if name == "resnet-gmk-k16":
        return _resnet_case()
    if name in ("c4-k1", "c4-k8"):
        s = TC.puct_case(_oracle(), None, "Connect4", int(name[4:]), 200, [3, 3, 2], 64, SLOTS, filters=name == "c4-k8")
    elif name == "gmk-k16":
        s = TC.puct_case(_oracle(), None, "Gomoku", 16, 695, [112], 64, (0, 63), compact=(-1, 1), alpha=0.05)   # (a game per wavefront: the batch's ends)
    elif name == "ttt":
        s = TC.puct_case(_oracle(), None, "TicTacToe", 1, 27, TC.TTT_DRAWN_GAME, 64, SLOTS, c_init=1.25, alpha=1.0, filters=True)
    elif name == "inflight":
        s = TC.inflight_case(None, G=64, K=4)
    elif name == "gumbel-c4":
        s = TC.gumbel_case(None, "Connect4", 32, 7, 7, 64, 4)
    elif name == "gumbel-gmk":
        s = TC.gumbel_case(None, "Gomoku", 48, 16, 5, 64, 3)
    elif name == "grouped-4096":
        s = TC.grouped_case(None, 4096, 64)
    elif name in ("mixed-runners", "mixed-runners-groups"):
        s = [TC.mixed_runner_case(None, G, 2 if name.endswith("groups") else 1) for G in (64, 200)]
    elif name == "classes":
        TC.mcts_class_case(_oracle(), None); s = TC.gumbel_class_case(None)
    else:
        raise SystemExit(f"unknown case {name}")
    print(name, "sizes", s, flush=True)


CASES = ["c4-k1", "c4-k8", "gmk-k16", "ttt", "inflight", "gumbel-c4", "gumbel-gmk", "grouped-4096", "mixed-runners", "mixed-runners-groups", "classes"]


@pytest.mark.parametrize("case", CASES)
def test_export_cases(case):
    STEPS.run(__file__, case, 240)


def test_gomoku_10_blocks_k16_export_equals_model():
    STEPS.run(__file__, "resnet-gmk-k16", 300)


if __name__ == "__main__":
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    _run(sys.argv[1])
    print("ok", flush=True)

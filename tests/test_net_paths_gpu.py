"""-m gpu: the evaluator's kernel choice by game, width and block count, checked exactly.

The evaluator (csrc/resnet.hip) picks its launches from the game, num_filters and net_blocks: at one block, block 0 is also the last block
(it feeds the heads), at three or more there are middle blocks, and Gomoku at 128 filters runs other kernels at each of these counts.
tests/test_net_paths.py shows on the host that appending a residual block with zero convolution weights and conv2 bias (random batch
norm) leaves every output of the restated network unchanged, bit for bit.  The HIP evaluator must have the same property: evaluate() of
the k-block network and of the (k + 1)-block network with that block appended give identical policy, value and head features, ragged
batches and single rows alike.  A launch that wires the last block, a middle block or the heads differently from the others, or that
rounds at other points at one block count, breaks the equality.

Gomoku at 128 filters, 1 -> 2: the default 2-block launch runs block 0 inside k_trunk on v_mfma_f32_16x16x32_bf16 (another accumulation
order than k_block0), so that pair is compared with k_block0 ahead of the trunk launch: GAZ_TRUNK_M16=0 (k_trunk RESG on 32x32x16) and
GAZ_BLOCK0_IN_TRUNK=0 (the 8-wave k_trunk for block 1)."""
import numpy as np
import pytest

from test_net_paths import append_zeroed_block, make_net, states

pytestmark = pytest.mark.gpu

N = {"Connect4": 77, "Gomoku": 9, "TicTacToe": 150}       # ragged: 3234 / 2025 / 1350 rows, partial last tiles everywhere

PATHS = ([("Connect4", F, k, {}) for F in (64, 128, 192, 256) for k in (1, 2)] +
         [("Gomoku", F, k, {}) for F in (64, 192, 256) for k in (1, 2)] +
         [("Gomoku", 128, 1, {"GAZ_TRUNK_M16": "0"}), ("Gomoku", 128, 1, {"GAZ_BLOCK0_IN_TRUNK": "0"}),
          ("Gomoku", 128, 2, {}), ("Gomoku", 128, 2, {"GAZ_TRUNK_M16": "0"})] +
         [("TicTacToe", 64, k, {}) for k in (1, 2)])


def _id(p):
    game, F, k, env = p
    return f"{game}-F{F}-{k}to{k + 1}" + "".join(f"-{key[4:]}={v}" for key, v in env.items())


def engine(game, n, blocks, F, logits=0):
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    if game == "Connect4":
        args = (max(n, 64), 200, 42, 8, 7, 2.5, 0.5)
    elif game == "Gomoku":
        args = (max(n, 8), 50, 150, 2, 1, 1.25, 1.0)
    else:
        args = (max(n, 64), 50, 9, 2, 2, 2.5, 1.0)
    return SelfPlayEngine(game, *args, seed=1, evaluator=EVAL_RESNET, net_blocks=blocks, net_filters=F, ring_capacity=0,
                          policy_is_logits=logits)


def _run(net, game, F, logits, batches):
    """(policy, value, p_feat, v_feat) of every batch, one engine"""
    eng = engine(game, batches[0].shape[0], len(net.blocks), F, logits)
    eng.load_weights(net.export_engine_weights())
    out = []
    for x in batches:
        p, v, _ = eng.evaluate(x)
        pf, vf = eng.head_features(x.shape[0])
        out.append((p, v, pf, vf))
    eng.close()
    return out


@pytest.mark.parametrize("logits", [0, 1])
@pytest.mark.parametrize("path", PATHS, ids=_id)
def test_a_zeroed_block_leaves_the_outputs_unchanged(path, logits, monkeypatch):
    game, F, k, env = path
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    net = make_net(game, k, F, "linear" if logits else "softmax")
    net2 = append_zeroed_block(net)
    n = N[game]
    x = states(game, n, F + k)
    batches = [x, x[n // 2:n // 2 + 1]]
    got, want = _run(net2, game, F, logits, batches), _run(net, game, F, logits, batches)
    for b, (o2, o1) in enumerate(zip(got, want)):
        assert np.isfinite(o1[0]).all() and np.isfinite(o1[1]).all()
        for name, a2, a1 in zip(("policy", "value", "p_feat", "v_feat"), o2, o1):
            np.testing.assert_array_equal(a2, a1, err_msg=f"{name}, {'single row' if b else f'{n} rows'}: {k + 1} blocks (last one zeroed) vs {k}")
    assert np.abs(want[0][0] - want[0][0][:1]).max() > 0 and np.abs(want[0][2] - want[0][2][:1]).max() > 0    # rows differ: not vacuous


@pytest.mark.parametrize("game,F", [("Connect4", 64), ("Connect4", 128), ("Connect4", 192), ("Connect4", 256),
                                    ("Gomoku", 64), ("Gomoku", 128), ("Gomoku", 192), ("Gomoku", 256), ("TicTacToe", 64)])
def test_one_block_rows_are_batch_independent(game, F):
    """One-block networks (block 0 feeds the heads): permuted and truncated batches and single rows give the same bits, as the
    multi-block tests in tests/test_evaluator_gpu.py and tests/test_net_widths_gpu.py check at 2 and 3 blocks."""
    n = {"Connect4": 131, "Gomoku": 21, "TicTacToe": 150}[game]
    rng = np.random.default_rng(n + F)
    net = make_net(game, 1, F, "softmax", seed=5)
    eng = engine(game, n, 1, F)
    eng.load_weights(net.export_engine_weights())
    x = states(game, n, F)
    p1, v1, _ = eng.evaluate(x)
    perm = rng.permutation(n)
    p2, v2, _ = eng.evaluate(x[perm])
    assert np.isfinite(p1).all() and np.array_equal(p1[perm], p2) and np.array_equal(v1[perm], v2)
    p3, v3, _ = eng.evaluate(x[:11])
    assert np.array_equal(p1[:11], p3) and np.array_equal(v1[:11], v3)
    for i in (0, n // 2, n - 1):
        p4, v4, _ = eng.evaluate(x[i:i + 1])
        assert np.array_equal(p1[i], p4[0]) and v1[i] == v4[0]
    eng.close()

"""The premise of tests/test_net_paths_gpu.py, on the host: a residual block whose convolution weights and conv2 bias are zero passes the
residual stream through bit for bit (x' = bf16((0 + 0) + x) = x), so appending one to a network leaves every output of
forward_engine_numerics unchanged — head features, logits, pre-tanh value, policy and value — for every game, width and policy head,
whatever the zeroed block's (random) batch-norm parameters make of its pre-activation.  The HIP evaluator picks its kernels by game,
width and block count; it must have the same property."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

from grok_alpha_zero_amd.net import NETS, ResNetBlock

CASES = [("Connect4", 64), ("Connect4", 128), ("Connect4", 192), ("Connect4", 256),
         ("Gomoku", 64), ("Gomoku", 128), ("Gomoku", 192), ("Gomoku", 256), ("TicTacToe", 64)]


def make_net(game, blocks, F, head, seed=11):
    """A network with random batch-norm statistics (so that every pre-activation is non-trivial)."""
    kw = {} if game == "TicTacToe" else dict(num_filters=F)
    return NETS[game](blocks, policy_head=head, seed=seed, **kw).eval().randomize_bn(seed + 1)


def append_zeroed_block(net, seed=99):
    """A copy of `net` with one more residual block at the end: conv1 / conv2 weights and conv2 bias zero, batch norm random."""
    out = copy.deepcopy(net)
    F = out.blocks[-1].conv2.weight.shape[3]
    b = ResNetBlock(F, F)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        b.bn1.randomize(g); b.bn2.randomize(g)
        b.conv1.bias.copy_(0.1 * torch.randn(F, generator=g))     # bn2's input is then a non-zero constant
        b.conv1.weight.zero_(); b.conv2.weight.zero_(); b.conv2.bias.zero_()
    out.blocks = nn.ModuleList(list(out.blocks) + [b.eval()])
    return out


def states(game, n, seed):
    net = NETS[game]
    rng = np.random.default_rng(seed)
    x = rng.integers(-1, 2, size=(n, net.H, net.W, net.C)).astype(np.int8)
    x[..., 0] = rng.choice([-1, 1], size=(n, 1, 1))
    return x


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("head", ["linear", "softmax"])
@pytest.mark.parametrize("game,F", CASES)
def test_a_zeroed_block_leaves_the_restated_network_unchanged(game, F, head, k):
    net = make_net(game, k, F, head)
    net2 = append_zeroed_block(net)
    assert len(net2.blocks) == k + 1 and len(net.blocks) == k
    x = torch.from_numpy(states(game, 6 if game == "Gomoku" else 40, F + k))
    a, b = net.forward_engine_numerics(x), net2.forward_engine_numerics(x)
    assert set(a) == set(b)
    for name in a:
        assert np.isfinite(a[name]).all()
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    # the export carries the appended block with its non-trivial pre-activation: the HIP evaluator runs it
    w = net2.export_engine_weights()
    assert f"block{k}.conv1.w" in w and not np.any(w[f"block{k}.conv2.w"]) and np.any(w[f"block{k}.conv1.shift"])

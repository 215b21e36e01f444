"""Networks at num_filters other than 128 (build_config["num_filters"] in {64, 192, 256}), host side: the engine export with the
block-0 projection, the bf16-faithful restatement of the k_conv_wide path (csrc/conv_wide.hpp) against the fp32 network, the Keras
weight round trip, and run_self_play's width / weights check, which refuses before any engine exists."""
import os

import numpy as np
import pytest
import torch

from grok_alpha_zero_amd.net import Connect4Net, GomokuNet, flops_per_position

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("F", [64, 192, 256])
def test_connect4_export_holds_the_block0_projection(F):
    w = Connect4Net(2, num_filters=F).export_engine_weights()
    assert w["block0.proj.w"].shape == (1, F, 128) and w["block0.proj.bias"].shape == (F,)
    assert w["block0.conv1.w"].shape == (9, F, 128) and w["block0.bn1.scale"].shape == (128,)
    assert w["block1.conv1.w"].shape == (9, F, F) and "block1.proj.w" not in w
    assert w["heads.conv.w"].shape == (9, 32, F)
    assert not np.any(w["heads.conv.w"][:, 16:])


def test_connect4_width_128_export_is_unchanged():
    w = Connect4Net(2).export_engine_weights()
    assert not any(k.endswith(".proj.w") for k in w) and w["heads.conv.w"].shape == (9, 32, 128)


@pytest.mark.parametrize("F", [64, 128, 192, 256])
def test_flops_per_position_counts_the_projection(F):
    hw = 42
    f = flops_per_position(3, F)
    want = 2 * hw * 9 * (128 * F + F * F) + (2 * hw * 128 * F if F != 128 else 0) + 2 * 2 * 2 * hw * 9 * F * F
    assert f["trunk"] == want


def _states(net, n, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-1, 2, size=(n, net.H, net.W, net.C)).astype(np.int8)
    x[..., 0] = rng.choice([-1, 1], size=(n, 1, 1))
    return torch.from_numpy(x)


@pytest.mark.parametrize("game,F", [("Connect4", 64), ("Connect4", 192), ("Connect4", 256), ("Gomoku", 64), ("Gomoku", 192), ("Gomoku", 256)])
@pytest.mark.parametrize("head", ["linear", "softmax"])
def test_engine_numerics_agree_with_the_fp32_network(game, F, head):
    """The loose bound _faithful_metrics (tests/test_evaluator_gpu.py) asserts between forward_engine_numerics and forward."""
    cls = Connect4Net if game == "Connect4" else GomokuNet
    net = cls(2, num_filters=F, policy_head=head, seed=3).eval().randomize_bn(7)
    x = _states(net, 6 if game == "Gomoku" else 40, F)
    ref = net.forward_engine_numerics(x)
    with torch.no_grad():
        p32, v32 = net(x)
    assert np.abs(ref["policy"] - p32.numpy()).max() <= (1.0 if head == "linear" else 6e-2)
    assert np.abs(ref["value"] - v32.numpy().reshape(-1)).max() <= 0.15


def test_gomoku_256_has_no_projection():
    w = GomokuNet(2, num_filters=256).export_engine_weights()
    assert not any(k.endswith(".proj.w") for k in w) and w["block0.conv1.w"].shape == (9, 256, 256)
    w = GomokuNet(2, num_filters=64).export_engine_weights()
    assert w["block0.proj.w"].shape == (1, 64, 256) and w["p.c1.w"].shape == (9, 32, 64)


@pytest.mark.parametrize("game,F", [("Connect4", 64), ("Connect4", 256), ("Gomoku", 64)])
def test_keras_round_trip_at_other_widths(tmp_path, game, F):
    from grok_alpha_zero_amd.keras_weights import load_keras_weights, save_keras_style
    cls = Connect4Net if game == "Connect4" else GomokuNet
    src = cls(2, num_filters=F, seed=1).eval().randomize_bn(3)
    path = str(tmp_path / "w.weights.h5")
    save_keras_style(src, path)
    dst = load_keras_weights(path, cls(2, num_filters=F, seed=2).eval())
    a, b = src.export_engine_weights(), dst.export_engine_weights()
    assert set(a) == set(b) and any(k.endswith(".proj.w") for k in a)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def _emu():
    import subprocess
    emu_dir = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-s", "-C", emu_dir])
    return os.path.join(emu_dir, "libgaz_emu.so")


def test_run_self_play_refuses_unsupported_widths_and_mismatched_weights(tmp_path, monkeypatch):
    from grok_alpha_zero_amd import engine as E
    from grok_alpha_zero_amd.engine import EngineError
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import ReplayStore, run_self_play
    emu = _emu()
    created = []
    real = E.SelfPlayEngine.__init__

    def spy(self, *a, **k):
        created.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(E.SelfPlayEngine, "__init__", spy)
    folder = str(tmp_path / "Grok_Zero_Train" / "1")
    ReplayStore(folder).create()
    train = dict(games_per_generation=2, MCTS_iteration_limit=8, max_actions=42, num_explore_actions_first=2, num_explore_actions_second=1,
                 c_puct_init=2.5, dirichlet_alpha=0.5, use_gumbel=False)
    w64 = Connect4Net(2, num_filters=64).export_engine_weights()
    with pytest.raises(EngineError, match=r"num_filters = 96 .*64, 128, 192, 256"):
        run_self_play(GAMES["Connect4"], (dict(num_resnet_layers=2, num_filters=96), train), folder, n_games=2, seed=1, lib_path=emu, weights=w64)
    with pytest.raises(EngineError, match=r"num_filters = 192.*'block0\.bn1\.scale'|num_filters = 192.*'block0\.conv1\.w'"):
        run_self_play(GAMES["Connect4"], (dict(num_resnet_layers=2, num_filters=192), train), folder, n_games=2, seed=1, lib_path=emu, weights=w64)
    with pytest.raises(EngineError, match=r"num_filters = 128.*'block0\.conv1\.w'"):
        run_self_play(GAMES["Connect4"], (dict(num_resnet_layers=2, num_filters=128), train), folder, n_games=2, seed=1, lib_path=emu, weights=w64)
    with pytest.raises(EngineError, match=r"num_filters = 64.*'block2\.bn1\.scale' is missing"):
        run_self_play(GAMES["Connect4"], (dict(num_resnet_layers=3, num_filters=64), train), folder, n_games=2, seed=1, lib_path=emu, weights=w64)
    with pytest.raises(EngineError, match="num_filters = 512"):
        run_self_play(GAMES["Gomoku"], (dict(num_resnet_layers=2, num_filters=512), dict(train, max_actions=225)), folder, n_games=2, seed=1,
                      lib_path=emu, weights=w64)
    assert not created


@pytest.mark.parametrize("slots", [8, 16, 24, 32])
def test_conv_wide_swizzle_is_conflict_free_for_ds_read_b128(slots):
    """conv_wide.hpp cw_swz: an A-fragment read puts lane l (l < 32) on image row r0 + l at logical slot s (lanes 32-63: slot s + 1);
    ds_read_b128 serves the wave in four 16-lane groups (MI355X_MICROARCH.md §LDS), bank of byte address a = (a / 4) mod 64.  Every group
    must cover 16 distinct 16-byte slots of the 256-byte bank row, for every starting row and logical slot."""
    groups = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
    groups += [[l + 32 for l in g] for g in groups]
    swz = (lambda r: r & 15) if slots % 16 == 0 else (lambda r: (r >> 1) & 7)
    for r0 in range(32):
        for s in range(0, slots, 2):
            for g in groups:
                pos = set()
                for lane in g:
                    row, ls = r0 + (lane & 31), s + (lane >> 5)
                    phys = ls ^ swz(row)
                    assert phys // (16 if slots % 16 == 0 else 8) == ls // (16 if slots % 16 == 0 else 8)   # stays in its aligned group
                    pos.add((row * slots + phys) % 16)
                assert len(pos) == 16, (slots, r0, s, g)

"""GPU suite: the HIP ResNet evaluator (csrc/resnet.hip, bf16 MFMA trunk, fp32 heads) against the fp32 PyTorch
restatement of the reference network (grok_alpha_zero_amd/net.py).  Floating-point kernel => tolerance test:
bf16 operands with fp32 accumulation through 13 convolutions; tolerance |dp| <= 6e-2 abs (mean <= 3e-3) on probabilities and
|dv| <= 5e-2 on tanh values, with mean error an order of magnitude below (written asserts below).
NN numerics vs Keras/ONNX Runtime are "parity unpinned" (no TensorFlow, no shipped weights)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _mk(n_games, blocks, randomize_bn, seed=0, game_groups=1):
    """an engine as a carrier of the evaluator: ONE batch (game_groups = 1), so that evaluate(n rows) is one launch over n rows"""
    import torch
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import Connect4Net
    net = Connect4Net(blocks, seed=seed).eval()
    if randomize_bn:
        net.randomize_bn()
    eng = SelfPlayEngine("Connect4", n_games, 200, 42, 8, 7, 2.5, 0.5, seed=1, evaluator=EVAL_RESNET, net_blocks=blocks,
                         ring_capacity=2 * n_games, game_groups=game_groups)
    eng.load_weights(net.export_engine_weights())
    return net, eng


def _random_states(n, rng):
    """plausible Connect4 input planes: random playouts encoded by the oracle's get_input_state."""
    from oracle import gaz_oracle as O
    import ctypes as C
    L = O.lib()
    out = np.zeros((n, 6, 7, 4), np.int8)
    for i in range(n):
        board = np.zeros(42, np.int8); hist = []; player = -1
        for _ in range(rng.integers(0, 30)):
            legal = (C.c_int * 7)(); k = L.gaz_api_legal_actions(1, board.ctypes.data_as(C.POINTER(C.c_int8)), legal)
            if k == 0:
                break
            a = int(legal[rng.integers(0, k)])
            L.gaz_api_do_action(1, board.ctypes.data_as(C.POINTER(C.c_int8)), a, player)
            hist.append(a); player = -player
        h = np.array(hist if hist else [0], np.int32)
        L.gaz_api_input_state(1, board.ctypes.data_as(C.POINTER(C.c_int8)), -player, h.ctypes.data_as(C.POINTER(C.c_int)),
                              len(hist), out[i].ctypes.data_as(C.POINTER(C.c_int8)))
    return out


@pytest.mark.parametrize("blocks,randomize_bn,n", [(1, True, 70), (6, False, 512), (6, True, 333)])
def test_resnet_evaluator_matches_torch_fp32(blocks, randomize_bn, n):
    import torch
    rng = np.random.default_rng(blocks * 7 + n)
    net, eng = _mk(max(n, 64), blocks, randomize_bn)
    x = _random_states(n, rng)
    pol, val, _ = eng.evaluate(x)
    with torch.no_grad():
        p_ref, v_ref = net(torch.from_numpy(x))
    p_ref = p_ref.numpy(); v_ref = v_ref.numpy().reshape(-1)
    dp = np.abs(pol - p_ref); dv = np.abs(val - v_ref)
    assert np.isfinite(pol).all() and np.isfinite(val).all()
    assert np.allclose(pol.sum(1), 1.0, atol=1e-5)
    assert dp.max() <= 6e-2 and dp.mean() <= 3e-3, (dp.max(), dp.mean())
    # randomised BN statistics give a high-gain net whose tanh input is O(10): allow 0.15 there
    assert dv.max() <= (0.15 if randomize_bn and blocks > 1 else 5e-2) and dv.mean() <= 1e-2, (dv.max(), dv.mean())
    # argmax agreement on clear-cut rows
    clear = (np.sort(p_ref, 1)[:, -1] - np.sort(p_ref, 1)[:, -2]) > 0.1
    assert (pol.argmax(1)[clear] == p_ref.argmax(1)[clear]).all()
    eng.close()


def test_rows_are_batch_independent():
    """A row's outputs must not depend on its position in the batch or on the other rows (bit-exact)."""
    rng = np.random.default_rng(5)
    net, eng = _mk(300, 2, True)
    x = _random_states(300, rng)
    p1, v1, _ = eng.evaluate(x)
    perm = rng.permutation(300)
    p2, v2, _ = eng.evaluate(x[perm])
    assert np.array_equal(p1[perm], p2) and np.array_equal(v1[perm], v2)
    p3, v3, _ = eng.evaluate(x[:77])
    assert np.array_equal(p1[:77], p3) and np.array_equal(v1[:77], v3)
    eng.close()


@pytest.mark.parametrize("game,blocks,filters,n", [("Gomoku", 3, 128, 37), ("TicTacToe", 2, 64, 150)])
def test_rows_are_batch_independent_generic_networks(game, blocks, filters, n):
    """The same for the Gomoku network (block 0 inside the 8-wave trunk launch, one board per workgroup; 32-row dense tiles) and the
    TicTacToe network: permuted and truncated batches and single rows give the same bits."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import NETS
    rng = np.random.default_rng(n)
    net = NETS[game](blocks).eval()
    net.randomize_bn()
    eng = SelfPlayEngine(game, n, 50, 9 if game == "TicTacToe" else 150, 2, 1, 1.25, 1.0, seed=1, evaluator=EVAL_RESNET, net_blocks=blocks,
                         net_filters=filters, ring_capacity=0)
    eng.load_weights(net.export_engine_weights())
    x = rng.integers(-1, 2, size=(n, net.H, net.W, net.C)).astype(np.int8)
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


@pytest.mark.parametrize("blocks,n", [(1, 1), (2, 2), (2, 7), (6, 100), (3, 1537), (6, 4096)])
def test_edge_tile_permutation_is_bit_identical(blocks, n, monkeypatch):
    """trunk.hpp / TrunkArgs::perm: the cells of each board edge gathered into whole 16-row MFMA tiles that sit out the taps on which
    they read nothing but zero padding (30 of 36 tile-taps per wave left on a 3-board tile, 45 of 54 on a 2-board tile).  The skipped
    products are exact zeros, so policy, value and head features equal the natural row order (GAZ_TILE_PERM=0) bit for bit — ragged
    batches (last tile with 1 or 2 boards, 2-board tiles of the mixed launch) included."""
    rng = np.random.default_rng(blocks * 1000 + n)
    x = _random_states(n, rng)
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("GAZ_TILE_PERM", flag)
        net, eng = _mk(max(n, 8), blocks, True, seed=3)
        p, v, _ = eng.evaluate(x)
        pf, vf = eng.head_features(n)
        outs.append((p, v, pf.copy(), vf.copy()))
        eng.close()
    for a, b in zip(*outs):
        assert np.isfinite(a).all() and np.array_equal(a, b)


@pytest.mark.parametrize("blocks,n", [(1, 5), (6, 334), (3, 4096)])
def test_whole_trunk_kernel_equals_per_block_kernels(blocks, n, monkeypatch):
    """k_trunk / k_trunk_mix (csrc/trunk.hpp: stem, every residual block and the heads' first convolution in one launch, activations
    resident in LDS).  On v_mfma_f32_32x32x16_bf16 (GAZ_TRUNK_M16=0) it is the arithmetic of the per-block kernels in the same order:
    mixed tile shapes | one tile shape | blocks only (behind k_stem_mfma, in front of k_conv_heads) | one k_resblock3 launch per block
    are bit-exact against each other, ragged last tiles included (n not a multiple of the 3 or 2 boards a workgroup owns).  The default
    build of the blocks (v_mfma_f32_16x16x32_bf16: another accumulation order inside the MFMA) is bit-exact between its own two launch
    configurations — a board's outputs must not depend on the tile shape it lands in — and within bf16 tolerance of the 32x32x16 one."""
    rng = np.random.default_rng(blocks + n)
    x = _random_states(n, rng) if n < 1000 else rng.integers(-1, 2, size=(n, 6, 7, 4)).astype(np.int8)

    def run(trunk, whole, mix, m16):
        for k, v in (("GAZ_TRUNK", trunk), ("GAZ_TRUNK_WHOLE", whole), ("GAZ_TRUNK_MIX", mix), ("GAZ_TRUNK_M16", m16)):
            monkeypatch.setenv(k, v)
        net, eng = _mk(max(n, 64), blocks, True, seed=3)
        out = eng.evaluate(x)[:2]
        eng.close()
        return out
    ref32 = run("1", "1", "1", "0")
    assert np.isfinite(ref32[0]).all()
    for cfg in (("1", "1", "0", "0"), ("1", "0", "0", "0"), ("0", "0", "0", "0")):
        o = run(*cfg)
        assert np.array_equal(ref32[0], o[0]) and np.array_equal(ref32[1], o[1]), cfg
    d16 = run("1", "1", "1", "1")
    o = run("1", "1", "0", "1")
    assert np.array_equal(d16[0], o[0]) and np.array_equal(d16[1], o[1])
    dp = np.abs(d16[0] - ref32[0]); dv = np.abs(d16[1] - ref32[1])
    assert dp.max() <= 6e-2 and dp.mean() <= 3e-3 and dv.max() <= 0.15 and dv.mean() <= 1e-2, (dp.max(), dp.mean(), dv.max(), dv.mean())


@pytest.mark.parametrize("blocks,n", [(2, 3), (4, 37), (10, 300)])
def test_gomoku_trunk_kernel_equals_per_block_kernels(blocks, n, monkeypatch):
    """Gomoku: k_block0 + ONE k_trunk launch for blocks 1.. against k_block0 + one k_resblock3 launch per block (GAZ_TRUNK=0).  The
    32x32x16 build of the trunk launch (GAZ_TRUNK_M16=0: one board per 4-wave workgroup, residual stream through L2, trunk.hpp RESG) is
    the per-block arithmetic bit for bit; the 16x16x32 builds (8-wave workgroup, both images in LDS) within bf16 tolerance: the default
    with block 0 inside the launch (trunk.hpp B0) and GAZ_BLOCK0_IN_TRUNK=0 with k_block0 ahead of it."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import NETS
    rng = np.random.default_rng(blocks + n)
    net = NETS["Gomoku"](blocks).eval()
    net.randomize_bn()
    x = rng.integers(-1, 2, size=(n, 15, 15, 2)).astype(np.int8)
    outs = []
    for trunk, m16, b0 in (("1", "0", "1"), ("0", "0", "1"), ("1", "1", "1"), ("1", "1", "0")):
        monkeypatch.setenv("GAZ_TRUNK", trunk)
        monkeypatch.setenv("GAZ_TRUNK_M16", m16)
        monkeypatch.setenv("GAZ_BLOCK0_IN_TRUNK", b0)
        eng = SelfPlayEngine("Gomoku", max(n, 8), 50, 150, 2, 1, 1.25, 1.0, seed=1, evaluator=EVAL_RESNET, net_blocks=blocks, net_filters=128,
                             ring_capacity=0)
        eng.load_weights(net.export_engine_weights())
        outs.append(eng.evaluate(x)[:2])
        eng.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    for o in outs[2:]:
        assert np.isfinite(outs[0][0]).all() and np.isfinite(o[0]).all()
        dp = np.abs(o[0] - outs[0][0]); dv = np.abs(o[1] - outs[0][1])
        assert dp.max() <= 6e-2 and dp.mean() <= 3e-3 and dv.max() <= 0.15 and dv.mean() <= 1e-2, (dp.max(), dp.mean(), dv.max(), dv.mean())


def test_search_with_resnet_matches_oracle_with_same_outputs(oracle):
    """End-to-end: HIP search + HIP network vs the CPU oracle whose session.run is served by the SAME HIP network
    (evaluate() on one row) — visit counts bit-exact, so tree kernels and evaluator compose correctly."""
    G, iters = 6, 48
    net, eng = _mk(G, 2, True)
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    probe = SelfPlayEngine("Connect4", 64, 1, 42, 8, 7, 2.5, 0.5, seed=0, evaluator=EVAL_RESNET, net_blocks=2)
    probe.load_weights(net.export_engine_weights())
    recs = []
    for _ in range(600):
        eng.run_waves(32); recs += eng.drain_finished()
        if len({r["slot"] for r in recs if r["game_seq"] == 0}) == G:
            break
    first = {r["slot"]: r for r in recs if r["game_seq"] == 0}
    assert len(first) == G

    def ev(state):
        p, v, _ = probe.evaluate(state[None])
        return p[0], v[0]
    for slot in (0, 3):
        o = oracle.selfplay_game("Connect4", iters_fix(iters), 42, 8, 7, 2.5, 0.5, 1, slot, 0, evaluator=ev)
        r = first[slot]
        np.testing.assert_array_equal(r["actions"], o["actions"])
        np.testing.assert_array_equal(r["root_N"], o["root_N"])
        np.testing.assert_array_equal(r["root_W"], o["root_W"])
    eng.close(); probe.close()


def test_gomoku_search_with_resnet_matches_oracle_with_same_outputs(oracle):
    """The same composition check for Gomoku: the one-game-per-wavefront tree kernel + the Gomoku network (stem, block 0 inside the
    trunk launch, heads on two streams) against the oracle served by evaluate() on single rows."""
    _gomoku_search_vs_oracle(oracle, 2)


def test_one_block_gomoku_search_matches_oracle_with_same_outputs(oracle):
    """The same with a one-block Gomoku network (num_resnet_layers = 1: stem, k_block0, k_conv_head32, no trunk launch)."""
    _gomoku_search_vs_oracle(oracle, 1)


def _gomoku_search_vs_oracle(oracle, blocks):
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import NETS
    G, iters, plies = 5, 36, 3         # a Gomoku move runs >= 3 x (legal moves) simulations when the limit is below that count (MCTS.py:545-546): ~670 per ply
    net = NETS["Gomoku"](blocks).eval()
    net.randomize_bn()
    w = net.export_engine_weights()
    eng = SelfPlayEngine("Gomoku", G, iters, plies, 3, 2, 4.5, 0.05, seed=3, evaluator=EVAL_RESNET, net_blocks=blocks, net_filters=128, ring_capacity=4 * G)
    probe = SelfPlayEngine("Gomoku", 8, 1, plies, 3, 2, 4.5, 0.05, seed=0, evaluator=EVAL_RESNET, net_blocks=blocks, net_filters=128, ring_capacity=0)
    eng.load_weights(w); probe.load_weights(w)
    recs = []
    for _ in range(100):
        eng.run_waves(64); recs += eng.drain_finished()
        if len({r["slot"] for r in recs if r["game_seq"] == 0}) == G:
            break
    first = {r["slot"]: r for r in recs if r["game_seq"] == 0}
    assert len(first) == G

    def ev(state):
        p, v, _ = probe.evaluate(state[None])
        return p[0], v[0]
    for slot in (0, 4):
        o = oracle.selfplay_game("Gomoku", iters, plies, 3, 2, 4.5, 0.05, 3, slot, 0, evaluator=ev)
        r = first[slot]
        np.testing.assert_array_equal(r["actions"], o["actions"])
        np.testing.assert_array_equal(r["root_N"], o["root_N"])
        np.testing.assert_array_equal(r["root_W"], o["root_W"])
        np.testing.assert_array_equal(r["policies"], o["policies"])
    eng.close(); probe.close()


def iters_fix(i):
    return 200   # _mk builds the engine with run_iterations = 200


@pytest.mark.parametrize("game,blocks,n", [("Gomoku", 2, 9), ("Gomoku", 10, 40), ("TicTacToe", 2, 300)])
def test_gomoku_tictactoe_evaluators_match_torch_fp32(game, blocks, n):
    """Gomoku (stem 256, projected first block, 32/8/4-channel head convs, Dense512/225) and TicTacToe (5x5 stem, 64-filter
    blocks with projection, 1x1 heads) networks: HIP vs the fp32 PyTorch restatement.  bf16 trunk => tolerance test."""
    import torch
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import NETS
    rng = np.random.default_rng(blocks + n)
    net = NETS[game](blocks).eval()
    if blocks <= 2:
        net.randomize_bn()        # deep stacks with random BN gains saturate the softmax (one-hot policies): not a numerics test
    H, W, C, A = net.H, net.W, net.C, net.A
    eng = SelfPlayEngine(game, max(n, 8), 50, 9 if game == "TicTacToe" else 150, 2, 1, 1.25, 1.0, seed=1, evaluator=EVAL_RESNET,
                         net_blocks=blocks, net_filters=128 if game == "Gomoku" else 64, ring_capacity=0)
    eng.load_weights(net.export_engine_weights())
    x = rng.integers(-1, 2, size=(n, H, W, C)).astype(np.int8)
    x[..., 0] = rng.choice([-1, 1], size=(n, 1, 1))
    pol, val, _ = eng.evaluate(x)
    with torch.no_grad():
        p_ref, v_ref = net(torch.from_numpy(x))
    dp = np.abs(pol - p_ref.numpy()); dv = np.abs(val - v_ref.numpy().reshape(-1))
    assert np.isfinite(pol).all() and np.allclose(pol.sum(1), 1.0, atol=1e-5)
    # 10 random-init blocks + he_normal Dense225 give very peaked 225-way softmaxes: allow 0.15 on the single largest entry there
    assert dp.max() <= (6e-2 if blocks <= 2 else 0.15) and dp.mean() <= 3e-3, (dp.max(), dp.mean())
    assert dv.max() <= 0.15 and dv.mean() <= 2e-2, (dv.max(), dv.mean())
    assert (pol.argmax(1) == p_ref.numpy().argmax(1)).mean() >= 0.9
    eng.close()


_PIPE_SCRIPT = r"""
import sys, hashlib, numpy as np
sys.path.insert(0, sys.argv[1])
from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
from grok_alpha_zero_amd.net import Connect4Net
net = Connect4Net(2, seed=3).eval()
eng = SelfPlayEngine("Connect4", 2048, 24, 12, 4, 3, 2.5, 0.5, seed=11, evaluator=EVAL_RESNET, net_blocks=2, ring_capacity=8192)
eng.load_weights(net.export_engine_weights())
eng.run_waves(300)
eng.run_waves(150)
eng.synchronize()
groups = eng.stats()["pipeline_groups"]
recs = eng.drain_finished(8192)
h = hashlib.sha256()
for r in sorted(recs, key=lambda r: (r["slot"], r["game_seq"])):
    for k in ("slot", "game_seq", "winner", "T"):
        h.update(np.int64(r[k]).tobytes())
    for k in ("actions", "root_N", "root_W", "policies", "q"):
        h.update(np.ascontiguousarray(r[k]).tobytes())
print(groups, len(recs), h.hexdigest())
"""


def test_group_pipeline_gives_identical_games(tmp_path):
    """GAZ_PIPELINE (engine.hip run_waves_pipelined: the games in groups, the trunk kernel of one group on the main stream while the
    heads kernels and the next tree step of the other groups run behind it on two side streams) must not change a single game:
    same finished records, bit for bit, for the default grouping (one full trunk round + remainder) and an explicit three-group
    split.  The switch is read once per process, hence the subprocesses."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "pipe.py"; script.write_text(_PIPE_SCRIPT)
    outs = {}
    for flag in ("0", "1", "512,512,1024"):
        env = dict(os.environ, GAZ_PIPELINE=flag)
        r = subprocess.run([sys.executable, str(script), root], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[flag] = r.stdout.strip().splitlines()[-1].split()
    assert [outs[f][0] for f in ("0", "1", "512,512,1024")] == ["0", "2", "3"]          # the pipeline really was engaged
    assert int(outs["0"][1]) > 400                         # games did finish
    assert outs["0"][1:] == outs["1"][1:] == outs["512,512,1024"][1:]


@pytest.mark.parametrize("game,blocks,n", [("Connect4", 3, 200), ("TicTacToe", 2, 64), ("Gomoku", 2, 64)])
def test_stablemax_policy_head_matches_torch(game, blocks, n):
    """policy_is_logits = 2: the Stablemax layer (Net/Stablemax.py:8-12, build_config["use_stablemax"]) as the policy epilogue."""
    import torch
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import NETS
    net = NETS[game](blocks, seed=4, policy_head="stablemax").eval()
    H, W, Cc = net.H, net.W, net.C
    eng = SelfPlayEngine(game, max(n, 64), 10, H * W, 0, 0, 1.0, 0.5, seed=1, evaluator=EVAL_RESNET, net_blocks=blocks,
                         net_filters=64 if game == "TicTacToe" else 128, ring_capacity=0, policy_is_logits=2)
    eng.load_weights(net.export_engine_weights())
    rng = np.random.default_rng(5)
    x = rng.integers(-1, 2, size=(n, H, W, Cc)).astype(np.int8)
    pol, val, _ = eng.evaluate(x)
    with torch.no_grad():
        p_ref, v_ref = net(torch.from_numpy(x))
    dp = np.abs(pol - p_ref.numpy())
    assert np.allclose(pol.sum(1), 1.0, atol=1e-5) and (pol > 0).all()
    assert dp.max() <= 3e-2 and dp.mean() <= 3e-3, (dp.max(), dp.mean())
    eng.close()


def _faithful_metrics(net_factory, blocks, x, mix, monkeypatch):
    """HIP evaluator vs net.forward_engine_numerics for both policy-head modes -> dict of max / mean differences."""
    import torch
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    monkeypatch.setenv("GAZ_TRUNK_MIX", mix)
    n = x.shape[0]
    m = {}
    for head, logits_mode in (("linear", 1), ("softmax", 0)):
        net = net_factory(head)
        eng = SelfPlayEngine("Connect4", max(n, 64), 200, 42, 8, 7, 2.5, 0.5, seed=1, evaluator=EVAL_RESNET, net_blocks=blocks,
                             ring_capacity=0, policy_is_logits=logits_mode)
        eng.load_weights(net.export_engine_weights())
        pol, val, _ = eng.evaluate(x)
        pf, vf = eng.head_features(n)
        eng.close()
        ref = net.forward_engine_numerics(torch.from_numpy(x))
        assert np.isfinite(pol).all() and np.isfinite(val).all()
        for name, got, want in (("p_feat", pf, ref["p_feat"]), ("v_feat", vf, ref["v_feat"])):
            d = np.abs(got - want)
            m[name + "_rel_max"] = float((d / np.maximum(np.abs(want), 1.0)).max()); m[name + "_mean"] = float(d.mean())
        m["value_max"] = float(np.abs(val - ref["value"]).max())
        ok = np.abs(ref["v_pre"]) < 2.5                                  # atanh is well conditioned there
        m["vpre_max"] = float(np.abs(np.arctanh(np.clip(val[ok].astype(np.float64), -0.999999, 0.999999)) - ref["v_pre"][ok]).max()) if ok.any() else 0.0
        if logits_mode:
            m["logits_max"] = float(np.abs(pol - ref["logits"]).max())
        else:
            m["prob_max"] = float(np.abs(pol - ref["policy"]).max())
            assert np.allclose(pol.sum(1), 1.0, atol=1e-5)
        with torch.no_grad():                                            # the faithful reference is the same network as the fp32 one
            p32, v32 = net(torch.from_numpy(x))
        assert np.abs(ref["policy"] - p32.numpy()).max() <= (1.0 if logits_mode else 6e-2) and np.abs(ref["value"] - v32.numpy().reshape(-1)).max() <= 0.15
    return m


@pytest.mark.parametrize("blocks,active,n,mix", [(1, 0, 77, "1"), (1, 0, 77, "0"), (1, 0, 5, "1")] +
                         [(6, k, 200, "1") for k in range(6)] + [(6, 2, 200, "0"), (6, 5, 1600, "1")])
def test_resnet_evaluator_matches_bf16_faithful_reference_per_layer(blocks, active, n, mix, monkeypatch):
    """TIGHT per-layer numerics check (the fp32 comparison, at 6e-2 / 0.15, cannot see a wrong tap at one board edge or a
    swapped channel group in one layer).  Reference = net.forward_engine_numerics: the same network with a bf16 rounding at exactly
    the points the kernels round (stem output, pre-activations, h, the residual stream between blocks), fp32 everywhere else.
    One residual block is ACTIVE at a time: the convolution weights and conv2 bias of every other block are zero, so those blocks
    pass the residual stream through bit for bit (x' = bf16((0 + 0) + x) = x) while still running their slice of the fused
    kernel's weight stream and parameter sets — block k of the 6-block k_trunk_mix launch is then compared at ONE-layer tightness:
      head features (stem + blocks + heads' first conv), per element      <= 1e-2 of max(|f|, 1) (one bf16 ulp of a flipped rounding), mean <= 1e-4
      policy logits, pre-tanh value                                        <= 2e-3
      softmax probabilities, tanh value                                    <= 1e-3
    over ragged batches and both tile shapes of k_trunk_mix (GAZ_TRUNK_MIX; 1600 boards = 1024 three-board + 32 two-board tiles).
    What is left between the two sides: the MFMA's accumulation order (~1e-6 relative), the fast-erfc GELU (|err| < 1e-7) and the
    rare bf16 roundings those flip.  NN numerics vs Keras / ONNX Runtime stay parity unpinned (no TensorFlow, no shipped weights)."""
    import torch
    from grok_alpha_zero_amd.net import Connect4Net
    rng = np.random.default_rng(blocks * 1000 + n + active)
    x = _random_states(n, rng)

    def factory(head):
        net = Connect4Net(blocks, seed=11, policy_head=head).eval().randomize_bn(7)
        with torch.no_grad():
            for i, b in enumerate(net.blocks):
                if i != active:
                    b.conv1.weight.zero_(); b.conv2.weight.zero_(); b.conv2.bias.zero_()
        return net
    m = _faithful_metrics(factory, blocks, x, mix, monkeypatch)
    assert m["p_feat_rel_max"] <= 1e-2 and m["v_feat_rel_max"] <= 1e-2 and m["p_feat_mean"] <= 1e-4 and m["v_feat_mean"] <= 1e-4, m
    assert m["logits_max"] <= 2e-3 and m["vpre_max"] <= 2e-3 and m["prob_max"] <= 1e-3 and m["value_max"] <= 1e-3, m


@pytest.mark.parametrize("blocks,n", [(6, 333), (3, 64)])
def test_resnet_evaluator_matches_bf16_faithful_reference_end_to_end(blocks, n, monkeypatch):
    """All blocks active, end to end.  Two bf16 pipelines that differ only in accumulation order do NOT stay within one-layer
    tightness over 12 stacked convolutions: every flipped rounding perturbs the next layer, which flips more — measured on the
    MI355X with this high-gain random-BN network: mean feature difference 2e-5 after one block, 1e-2 after six (features of magnitude
    ~10), logits up to 0.11, probabilities up to 3.1e-2, tanh value up to 4.8e-2.  That is the bf16 noise floor of the stack itself
    (the same order as bf16 vs fp32), so end to end only a sanity bound is asserted; the tight check is the per-layer test above."""
    import torch
    from grok_alpha_zero_amd.net import Connect4Net
    x = _random_states(n, np.random.default_rng(blocks * 77 + n))
    m = _faithful_metrics(lambda head: Connect4Net(blocks, seed=11, policy_head=head).eval().randomize_bn(7), blocks, x, "1", monkeypatch)
    print("end-to-end faithful metrics", blocks, m)
    assert m["prob_max"] <= 6e-2 and m["value_max"] <= 0.1 and m["p_feat_mean"] <= 3e-2 and m["v_feat_mean"] <= 3e-2, m


@pytest.mark.parametrize("search", ["puct", "gumbel", "gumbel_one_game_per_wave"])
def test_fused_tree_and_trunk_launch_gives_identical_games(search, monkeypatch):
    """k_wave_trunk / k_wave_trunk_gumbel (resnet.hip): the tree step of every Connect4 game and the trunk kernel of their leaf rows in ONE launch —
    tree blocks first, each trunk workgroup waiting only for the done flags of its own three boards, the leaf rows handed over through
    system-scope stores / loads while both roles are running.  Scheduling only: the finished games must equal, bit for bit, those of
    separate launches (gaz_engine_set_fused_wave(0)) — every record, including the evaluator-call counts per move.  Round 3: the Gumbel search
    (MCTS_Gumbel.py:562-679) in the same launch shape, four games per wavefront or one."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET, SEARCH_GUMBEL, SEARCH_PUCT
    from grok_alpha_zero_amd.net import Connect4Net
    gumbel = search != "puct"
    if search == "gumbel_one_game_per_wave":
        monkeypatch.setenv("GAZ_FUSE_GUMBEL_TEAMS", "0")
    w = Connect4Net(2, seed=5, policy_head="linear" if gumbel else "softmax").eval().export_engine_weights()
    kw = dict(search=SEARCH_GUMBEL, gumbel_m=5, c_visit=50.0, c_scale=1.0, policy_is_logits=True) if gumbel else dict(search=SEARCH_PUCT)
    got = []
    for fused in (True, False):
        eng = SelfPlayEngine("Connect4", 1600, 24, 14, 4, 3, 2.5, 0.5, seed=19, evaluator=EVAL_RESNET, net_blocks=2, ring_capacity=8192, **kw)
        eng.load_weights(w)
        eng.set_fused_wave(fused)
        eng.run_waves(260); eng.run_waves(140); eng.synchronize()
        st = eng.stats()
        assert st["fused_wave"] == int(fused) and st["fused_faults"] == 0, st
        got.append({(r["slot"], r["game_seq"]): r for r in eng.drain_finished(8192)})
        eng.close()
    a, b = got
    assert len(a) > (800 if gumbel else 1600) and set(a) == set(b)
    for k in a:
        for f in ("actions", "root_N", "root_W", "root_P", "policies", "q", "evals", "root_visits", "winner", "T"):
            np.testing.assert_array_equal(np.asarray(a[k][f]), np.asarray(b[k][f]), err_msg=f"{k} {f}")


def test_fused_launch_fallback_also_happens_for_a_caller_that_only_drains():
    """gaz_engine_drain_finished is a host synchronisation point like synchronize / get_stats: a self-play loop that only ever runs waves and drains
    (self_play.run_self_play) must get the fallback to separate launches after trunk workgroups gave up — otherwise every later fused launch
    finds the fault counter set, gives up at once, and no game ever moves again."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import Connect4Net
    w = Connect4Net(2, seed=5).eval().export_engine_weights()
    eng = SelfPlayEngine("Connect4", 1600, 24, 14, 4, 3, 2.5, 0.5, seed=23, evaluator=EVAL_RESNET, net_blocks=2, ring_capacity=8192, games_budget=1600, game_groups=2)
    eng.load_weights(w)
    eng.run_waves(40); eng.synchronize()
    eng.debug_fused_fault(5)
    recs = []
    for _ in range(200):
        eng.run_waves(50)
        recs += eng.drain_finished(8192)            # the only synchronisation in the loop
        if len(recs) >= 1600:
            break
    st = eng.stats()
    eng.close()
    assert len(recs) == 1600 and st["fused_faults"] > 0 and st["fused_wave"] == 0, (len(recs), st)


def test_fused_launch_is_tried_again_after_a_transient_fault():
    """After trunk workgroups gave up, the engine runs separate launches — but not for good on the first occasion: a give-up can be a transient
    (two game groups' launches holding each other's slots), and separate launches cost a grouped engine a fifth of its rate.  20000 waves later the
    one-launch form is back (at most twice); the games do not notice either switch."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import Connect4Net
    w = Connect4Net(2, seed=5).eval().export_engine_weights()
    got = []
    for fault in (True, False):
        eng = SelfPlayEngine("Connect4", 512, 24, 14, 4, 3, 2.5, 0.5, seed=31, evaluator=EVAL_RESNET, net_blocks=2, ring_capacity=4096, games_budget=3000)
        eng.load_weights(w)
        eng.run_waves(40); eng.synchronize()
        if fault:
            eng.debug_fused_fault(5); eng.run_waves(8)
            st = eng.stats()
            assert st["fused_faults"] > 0 and st["fused_wave"] == 0, st
            seen = st["fused_faults"]
        recs = []
        for _ in range(22):
            eng.run_waves(1000)
            recs += eng.drain_finished(4096)
        st = eng.stats()
        assert st["fused_wave"] == 1 and (not fault or st["fused_faults"] == seen), st
        got.append({(r["slot"], r["game_seq"]): r for r in recs})
        eng.close()
    a, b = got
    assert len(a) == 3000 and set(a) == set(b)
    for key in a:
        for f in ("actions", "root_N", "root_W", "policies", "q", "evals"):
            np.testing.assert_array_equal(np.asarray(a[key][f]), np.asarray(b[key][f]), err_msg=f"{key} {f}")


def test_game_groups_evaluate_and_head_features_cover_all_rows():
    """gaz_engine_evaluate / gaz_engine_read_head_features on a grouped engine: rows [first[c], first[c + 1]) go through group c — the outputs must be
    those of one batch, row for row (rows are independent of the batch they are evaluated in)."""
    rng = np.random.default_rng(5)
    x = _random_states(1000, rng)
    outs = []
    for k in (1, 3):
        net, eng = _mk(1000, 2, True, seed=3, game_groups=k)
        p, v, _ = eng.evaluate(x)
        q, u, _ = eng.evaluate(x[:700])                    # a prefix that ends inside the last group
        pf, vf = eng.head_features(700)
        outs.append((p, v, q, u, pf.copy(), vf.copy()))
        assert eng.stats()["game_groups"] == k
        eng.close()
    for a, b in zip(*outs):
        assert np.isfinite(a).all() and np.array_equal(a, b)
    assert np.array_equal(outs[0][0][:700], outs[0][2])


@pytest.mark.parametrize("groups,fault,cache", [(2, False, 0), (3, False, 0), (2, True, 0), (2, False, 16)])
def test_game_groups_with_fused_launches_in_flight_together_give_identical_games(groups, fault, cache):
    """gaz_engine_config::game_groups (engine.hip GroupEngine, round 3): the games as K groups, each with its own stream, batch and fused tree + trunk
    launch per wave — K launches in flight on the chip at once, each one's trunk workgroups polling only their own group's completion queue.
    Scheduling only: with a games_budget the grouped engine must finish exactly the games of one batch, bit for bit — also while workgroups of the
    concurrent launches give up waiting (gaz_engine_debug_fused_fault) and the groups fall back to separate launches, and with the evaluation
    cache (a table per group) against one batch without it."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import Connect4Net
    w = Connect4Net(2, seed=5).eval().export_engine_weights()
    G, budget = 1600, 2000
    got = []
    for k in (groups, 1):
        eng = SelfPlayEngine("Connect4", G, 24, 14, 4, 3, 2.5, 0.5, seed=29, evaluator=EVAL_RESNET, net_blocks=2, ring_capacity=8192, games_budget=budget, game_groups=k,
                             eval_cache_log2=cache if k > 1 else 0)
        eng.load_weights(w)
        eng.run_waves(30); eng.synchronize()
        st = eng.stats()
        assert st["game_groups"] == k and st["fused_wave"] == 1, st
        if fault and k > 1:
            eng.debug_fused_fault(5)
            eng.run_waves(24)
            st = eng.stats()
            assert st["fused_faults"] >= 24 * k and st["fused_wave"] == 0, st
        for _ in range(60):
            eng.run_waves(100)
            if eng.stats()["game_stats"][2] >= budget:
                break
        got.append({(r["slot"], r["game_seq"]): r for r in eng.drain_finished(8192)})
        eng.close()
    a, b = got
    assert len(a) == budget and set(a) == set(b)
    for key in a:
        for f in ("actions", "root_N", "root_W", "root_P", "policies", "q", "evals", "root_visits", "winner", "T"):
            np.testing.assert_array_equal(np.asarray(a[key][f]), np.asarray(b[key][f]), err_msg=f"{key} {f}")


@pytest.mark.parametrize("cache", [0, 16])
def test_fused_launch_bounded_wait_recovers_without_changing_games(cache):
    """The fused launch's hand-over is bounded (trunk.hpp TrunkArgs::spin_ticks; ADVICE r2 / VERDICT r2 item 5): a trunk workgroup whose games'
    tree block does not show up gives up, leaves its boards unevaluated and marks them; the games keep their requests pending, the next wave
    evaluates them, and the host falls back to separate launches at its next synchronisation point.  gaz_engine_debug_fused_fault makes every
    5th trunk workgroup of the REAL k_wave_trunk launches take that path (one wave in four of its games' evaluations is lost, for 48 launches in a
    row): the finished games must equal those of an undisturbed engine bit for bit, and the engine must report the faults and the fallback."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import Connect4Net
    w = Connect4Net(2, seed=5).eval().export_engine_weights()
    got = []
    for fault in (True, False):
        eng = SelfPlayEngine("Connect4", 1600, 24, 14, 4, 3, 2.5, 0.5, seed=23, evaluator=EVAL_RESNET, net_blocks=2, ring_capacity=8192, games_budget=1600,
                             eval_cache_log2=cache)
        eng.load_weights(w)
        eng.run_waves(40); eng.synchronize()
        assert eng.stats()["fused_wave"] == 1
        if fault:
            eng.debug_fused_fault(5)
            eng.run_waves(48)                          # no host synchronisation in between: 48 fused launches with workgroups giving up
            st = eng.stats()
            assert st["fused_faults"] >= 48 and st["fused_wave"] == 0, st
        for _ in range(40):
            eng.run_waves(100)
            got_now = eng.stats()
            if got_now["game_stats"][2] >= 1600:
                break
        assert eng.stats()["fused_wave"] == (0 if fault else 1)
        got.append({(r["slot"], r["game_seq"]): r for r in eng.drain_finished(8192)})
        eng.close()
    a, b = got
    assert len(a) == 1600 and set(a) == set(b)
    for k in a:
        for f in ("actions", "root_N", "root_W", "root_P", "policies", "q", "evals", "root_visits", "winner", "T"):
            np.testing.assert_array_equal(np.asarray(a[k][f]), np.asarray(b[k][f]), err_msg=f"{k} {f}")


@pytest.mark.parametrize("blocks,active,n,b0", [(2, 1, 23, "1"), (2, -1, 9, "1"), (2, -1, 9, "0"), (10, 1, 12, "1"), (10, 5, 12, "1"), (10, 9, 33, "1"), (10, 9, 33, "0"),
                                                (1, -1, 9, "1")])
def test_gomoku_evaluator_matches_bf16_faithful_reference_per_layer(blocks, active, n, b0, monkeypatch):
    """The Gomoku network's kernels (k_stem_mfma; block 0 with its in-LDS pre-activation and the projection accumulated into conv2 —
    inside the 8-wave k_trunk launch (b0 = "1", the default) or as k_block0 ahead of it (GAZ_BLOCK0_IN_TRUNK=0); the 8-wave k_trunk for
    blocks 1.., k_conv_head32, k_conv_small, the fp32 dense chain) against GomokuNet.forward_engine_numerics —
    the same network with a bf16 rounding at exactly the points these kernels round.  Block 0 (it carries the 256 -> 128 projection)
    is always live; of blocks 1.. ONE is active at a time (the others have zero convolution weights and conv2 bias and pass the
    residual stream through bit for bit), so every slice of the 10-block weight stream is checked with only a few rounding stages
    between input and output (block 0's two, the active block's two, the heads' bf16 conv output).  Measured on the MI355X: block 0
    alone — feature mean 7e-5, logits 3.8e-3, probabilities 1e-4; block 0 + one more — feature mean 6 - 12e-4 (isolated elements up to
    3.8e-2 of max(|f|, 1): flipped bf16 roundings two stages up), logits 2.2e-2, probabilities 2.3e-3.  Asserted with ~2x margin; a wrong
    tap at a board edge or a swapped channel group shows as O(1) feature errors, 20x above these bounds (the fp32 comparison above
    allows 0.15 on probabilities).  active = -1: block 0 alone is live (both convolutions of block 1 zeroed), or the one-block network
    (k_block0 straight into k_conv_head32: block 0 is also the last block; measured: feature mean 9.9e-5, logits 5.6e-3, probabilities 2.4e-4)."""
    import torch
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import GomokuNet
    monkeypatch.setenv("GAZ_BLOCK0_IN_TRUNK", b0)
    rng = np.random.default_rng(blocks * 100 + n)
    x = rng.integers(-1, 2, size=(n, 15, 15, 2)).astype(np.int8)
    x[..., 0] = rng.choice([-1, 1], size=(n, 1, 1))
    m = {}
    for head, logits_mode in (("linear", 1), ("softmax", 0)):
        net = GomokuNet(blocks, seed=21, policy_head=head).eval().randomize_bn(5)
        with torch.no_grad():
            for i, b in enumerate(net.blocks):
                if i >= 1 and i != active:
                    b.conv1.weight.zero_(); b.conv2.weight.zero_(); b.conv2.bias.zero_()
        eng = SelfPlayEngine("Gomoku", max(n, 8), 50, 150, 2, 1, 1.25, 1.0, seed=1, evaluator=EVAL_RESNET, net_blocks=blocks, net_filters=128,
                             ring_capacity=0, policy_is_logits=logits_mode)
        eng.load_weights(net.export_engine_weights())
        pol, val, _ = eng.evaluate(x)
        pf, vf = eng.head_features(n)
        eng.close()
        ref = net.forward_engine_numerics(torch.from_numpy(x))
        assert np.isfinite(pol).all() and np.isfinite(val).all()
        for name, got, want in (("p_feat", pf, ref["p_feat"]), ("v_feat", vf, ref["v_feat"])):
            d = np.abs(got - want)
            m[name + "_rel_max"] = float((d / np.maximum(np.abs(want), 1.0)).max()); m[name + "_mean"] = float(d.mean())
        m["value_max"] = float(np.abs(val - ref["value"]).max())
        ok = np.abs(ref["v_pre"]) < 2.5
        m["vpre_max"] = float(np.abs(np.arctanh(np.clip(val[ok].astype(np.float64), -0.999999, 0.999999)) - ref["v_pre"][ok]).max()) if ok.any() else 0.0
        if logits_mode:
            m["logits_max"] = float(np.abs(pol - ref["logits"]).max())
        else:
            m["prob_max"] = float(np.abs(pol - ref["policy"]).max())
    print("gomoku faithful metrics", blocks, active, m)
    if active < 0:
        assert m["p_feat_rel_max"] <= 4e-2 and m["v_feat_rel_max"] <= 4e-2 and m["p_feat_mean"] <= 2e-4 and m["v_feat_mean"] <= 2e-4, m
        assert m["logits_max"] <= 8e-3 and m["vpre_max"] <= 8e-3 and m["prob_max"] <= 5e-4 and m["value_max"] <= 2e-3, m
    else:
        assert m["p_feat_rel_max"] <= 8e-2 and m["v_feat_rel_max"] <= 8e-2 and m["p_feat_mean"] <= 2.5e-3 and m["v_feat_mean"] <= 2.5e-3, m
        assert m["logits_max"] <= 4e-2 and m["vpre_max"] <= 3e-2 and m["prob_max"] <= 5e-3 and m["value_max"] <= 1e-2, m


@pytest.mark.parametrize("blocks,active,n", [(2, 0, 300), (2, 1, 300), (3, 2, 77), (3, -1, 9)])
def test_tictactoe_evaluator_matches_bf16_faithful_reference_per_layer(blocks, active, n):
    """the TicTacToe network (5x5 stem 2 -> 128, block 0 projecting 128 -> 64; netops.hpp k_stem_generic / k_conv_direct /
    k_dense) had only the 6e-2 fp32 comparison.  Same scheme as the Connect4 and Gomoku launches: TicTacToeNet.forward_engine_numerics rounds to
    bf16 exactly where the kernels do, and ONE residual block is active at a time (block 0's projection is always live — it is the skip path —
    the other blocks have zero convolution weights and conv2 bias and pass the stream through bit for bit); active = -1: only the projection."""
    import torch
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import TicTacToeNet
    rng = np.random.default_rng(blocks * 100 + n + active)
    x = np.zeros((n, 3, 3, 2), np.int8)
    who = rng.integers(0, 3, size=(n, 3, 3))
    x[..., 0] = who == 1; x[..., 1] = who == 2
    for head, logits_mode in (("linear", 1), ("softmax", 0)):
        net = TicTacToeNet(blocks, seed=4, policy_head=head).eval().randomize_bn(9)
        with torch.no_grad():
            for i, b in enumerate(net.blocks):
                if i != active:
                    b.conv1.weight.zero_(); b.conv2.weight.zero_(); b.conv2.bias.zero_()
        eng = SelfPlayEngine("TicTacToe", max(n, 64), 50, 9, 2, 2, 2.5, 1.0, seed=1, evaluator=EVAL_RESNET, net_blocks=blocks, net_filters=64,
                             ring_capacity=0, policy_is_logits=logits_mode)
        eng.load_weights(net.export_engine_weights())
        pol, val, _ = eng.evaluate(x)
        pf, vf = eng.head_features(n)
        eng.close()
        ref = net.forward_engine_numerics(torch.from_numpy(x))
        m = {}
        for name, got, want in (("p_feat", pf, ref["p_feat"]), ("v_feat", vf, ref["v_feat"])):
            d = np.abs(got - want)
            m[name + "_rel_max"] = float((d / np.maximum(np.abs(want), 1.0)).max()); m[name + "_mean"] = float(d.mean())
        m["value_max"] = float(np.abs(val - ref["value"]).max())
        m["pol_max"] = float(np.abs(pol - ref["policy"]).max())
        print("tictactoe faithful metrics", blocks, active, head, m)
        assert m["p_feat_rel_max"] <= 1e-2 and m["v_feat_rel_max"] <= 1e-2 and m["p_feat_mean"] <= 2e-4 and m["v_feat_mean"] <= 2e-4, m
        # measured on the MI355X (block 0 active, 300 positions): features 4.5e-3 rel (one flipped bf16 rounding), logits 2.8e-3, value 1.6e-3 — ~2x margin
        assert m["pol_max"] <= (6e-3 if logits_mode else 2e-3) and m["value_max"] <= 4e-3, m


@pytest.mark.parametrize("blocks,n", [(2, 5), (10, 300), (10, 2048)])
def test_gomoku_stem_inside_the_trunk_launch_is_bit_identical(blocks, n, monkeypatch):
    """Round 3 (trunk.hpp S0): the Gomoku network's 256-channel stem (Gomoku/Build_Model.py:21-24) computed inside the one trunk launch, half
    by half, straight into block 0's operand image (opt-in, GAZ_STEM_IN_TRUNK=1: measured slower on its own, see resnet.hip) — against the
    stem kernel + the launch that reads its output back (the default):
    same arithmetic in the same order (k_stem_mfma's hi + lo split on v_mfma_f32_32x32x16_bf16, ReLU, bf16, block 0's pre-activation from the
    rounded value), so policy, value and head features must be bit-identical, ragged batches included."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import NETS
    net = NETS["Gomoku"](blocks, seed=3).eval().randomize_bn(5)
    w = net.export_engine_weights()
    rng = np.random.default_rng(blocks + n)
    who = rng.integers(0, 3, size=(n, 15, 15))
    x = np.zeros((n, 15, 15, 2), np.int8); x[..., 0] = who == 1; x[..., 1] = who == 2
    out = []
    for flag in ("1", "0"):
        monkeypatch.setenv("GAZ_STEM_IN_TRUNK", flag)
        eng = SelfPlayEngine("Gomoku", max(n, 8), 8, 10, 2, 2, 4.5, 0.05, seed=1, evaluator=EVAL_RESNET, net_blocks=blocks, net_filters=128, ring_capacity=0)
        eng.load_weights(w)
        pol, val, _ = eng.evaluate(x)
        pf, vf = eng.head_features(n)
        eng.close()
        out.append((pol, val, pf, vf))
    for a, b, name in zip(out[0], out[1], ("policy", "value", "p_feat", "v_feat")):
        np.testing.assert_array_equal(a, b, err_msg=name)
    assert np.isfinite(out[0][0]).all() and np.abs(out[0][0].sum(1) - 1).max() < 1e-4


@pytest.mark.parametrize("fault", [0, 5])
def test_gomoku_fused_tree_and_trunk_launch_gives_identical_games(fault):
    """Round 3: Gomoku's PUCT tree step (one game per wavefront, 64 games per tree block in eight rounds) and the 8-wave trunk launch with block 0
    and the stem inside as ONE launch (resnet.hip k_wave_trunk_gmk): completion queue, leaf rows handed over with release / acquire (450-byte rows are
    not dword-aligned).  Scheduling only: finished games equal those of separate launches bit for bit; fault = 5: every fifth trunk workgroup
    gives up its wait (gaz_engine_debug_fused_fault) for 24 launches — the games must still come out identical and the engine must fall back."""
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    from grok_alpha_zero_amd.net import NETS
    w = NETS["Gomoku"](2, seed=8).eval().export_engine_weights()
    got = []
    for fused in (True, False):
        eng = SelfPlayEngine("Gomoku", 300, 24, 4, 2, 2, 4.5, 0.05, seed=31, evaluator=EVAL_RESNET, net_blocks=2, net_filters=128, ring_capacity=1024, games_budget=300)
        eng.load_weights(w)
        eng.set_fused_wave(fused)
        eng.run_waves(30); eng.synchronize()
        assert eng.stats()["fused_wave"] == int(fused)
        if fused and fault:
            eng.debug_fused_fault(fault)
            eng.run_waves(24)
            st = eng.stats()
            assert st["fused_faults"] >= 24 and st["fused_wave"] == 0, st
        for _ in range(60):
            eng.run_waves(100)
            if eng.stats()["game_stats"][2] >= 300:
                break
        st = eng.stats()
        assert st["fused_wave"] == int(fused and not fault) and (fault or st["fused_faults"] == 0), st
        got.append({(r["slot"], r["game_seq"]): r for r in eng.drain_finished(1024)})
        eng.close()
    a, b = got
    assert len(a) == 300 and set(a) == set(b)
    for k in a:
        for f in ("actions", "root_N", "root_W", "root_P", "policies", "q", "evals", "root_visits", "winner", "T"):
            np.testing.assert_array_equal(np.asarray(a[k][f]), np.asarray(b[k][f]), err_msg=f"{k} {f}")

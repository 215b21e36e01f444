"""GPU suite: k_heads_c4 (csrc/resnet.hip), the Connect4 network's dense heads as ONE launch — Dense(336 -> 128) + BN + ReLU ->
Dense(128 -> 64) -> Dense(64 -> 7 | 1) -> softmax | logits | Stablemax | tanh for 32 positions of one head per item — against
the two launches it replaces (k_dense1_mfma + k_tail, GAZ_HEADS_ONE=0).  The switch is read when an evaluator is constructed, so one
process holds an engine of each kind.  Same summation orders => every comparison here is for equal bytes, no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POS = 32                                 # positions per item of k_heads_c4 (HC4_POS)
BATCHES = (1, POS - 1, POS, POS + 1, 2 * POS + 1)       # under a block, a block, a block plus one, two blocks plus one
_states = {}


def _random_states(n):
    """Connect4 input planes (int8 -1 | 0 | 1), the same for every test of the module"""
    if n not in _states:
        _states[n] = np.random.default_rng(1000 + n).integers(-1, 2, size=(n, 6, 7, 4)).astype(np.int8)
    return _states[n]


def _engine(monkeypatch, heads_one, weights, **kw):
    from grok_alpha_zero_amd.engine import SelfPlayEngine, EVAL_RESNET
    if heads_one:
        monkeypatch.delenv("GAZ_HEADS_ONE", raising=False)
    else:
        monkeypatch.setenv("GAZ_HEADS_ONE", "0")
    args = dict(run_iterations=200, max_actions=42, first=8, second=7, seed=1)
    args.update(kw.pop("args", {}))
    eng = SelfPlayEngine("Connect4", kw.pop("n_games", 64), args["run_iterations"], args["max_actions"], args["first"], args["second"], 2.5, 0.5,
                         seed=args["seed"], evaluator=EVAL_RESNET, net_blocks=1, **kw)
    eng.load_weights(weights)
    return eng


@pytest.fixture(scope="module")
def weights():
    from grok_alpha_zero_amd.net import Connect4Net
    net = Connect4Net(1, seed=11).eval()
    net.randomize_bn()
    return net.export_engine_weights()


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["softmax", "logits", "stablemax"])
def test_one_heads_kernel_equals_the_two_it_replaces(mode, weights, monkeypatch):
    """two engines in one process, the same seeded one-block network: policy and value byte-equal for every batch size around the
    kernel's 32 positions per item, in each policy mode (policy_is_logits = 0 | 1 | 2)"""
    two = _engine(monkeypatch, False, weights, n_games=128, game_groups=1, policy_is_logits=mode)
    one = _engine(monkeypatch, True, weights, n_games=128, game_groups=1, policy_is_logits=mode)
    try:
        for n in BATCHES:
            x = _random_states(n)
            p2, v2, _ = two.evaluate(x)
            p1, v1, _ = one.evaluate(x)
            assert p1.shape == (n, 7) and v1.shape == (n,)
            assert np.isfinite(p1).all() and np.isfinite(v1).all()
            if mode != 1:
                assert np.allclose(p1.sum(1), 1.0, atol=1e-5)
            assert p1.tobytes() == p2.tobytes(), (mode, n, np.abs(p1 - p2).max())
            assert v1.tobytes() == v2.tobytes(), (mode, n, np.abs(v1 - v2).max())
        assert len({p1[i].tobytes() for i in range(len(p1))}) > 1        # (the rows differ: the comparison is not of constants)
    finally:
        two.close(); one.close()


def test_64_games_in_two_groups_play_the_same_games(weights, monkeypatch):
    """64 Connect4 games as two game groups (a fused tree + trunk launch and a heads launch per group and wave), PUCT, 40 waves: the
    finished records and the positions of the games in progress are equal with either heads path.  Seven simulations per move (the floor: one per
    root child) and games cut at 3 plies (max_actions), so that 40 waves finish games and start their successors."""
    got = []
    for heads_one in (False, True):
        eng = _engine(monkeypatch, heads_one, weights, game_groups=2, ring_capacity=256, args=dict(run_iterations=7, max_actions=3, first=4, second=3, seed=29))
        try:
            eng.run_waves(40); eng.synchronize()
            assert eng.stats()["game_groups"] == 2
            got.append(({(r["slot"], r["game_seq"]): r for r in eng.drain_finished(256)}, eng.read_positions()))
        finally:
            eng.close()
    (a, pa), (b, pb) = got
    print(f"finished {len(a)} | {len(b)} games; plies of the games in progress {sorted(len(h) for h in pa)[::8]}")
    assert len(a) > 0 and set(a) == set(b)
    for key in a:
        assert set(a[key]) == set(b[key])
        for f in a[key]:
            np.testing.assert_array_equal(np.asarray(a[key][f]), np.asarray(b[key][f]), err_msg=f"{key} {f}")
    assert pa == pb and any(len(h) for h in pa)


@pytest.mark.parametrize("wgs", [1, 3])
def test_workgroups_that_walk_through_several_items(wgs, weights, monkeypatch):
    """an evaluator of a game group launches at most GAZ_HEADS_WGS workgroups (default 128), each of which takes every wgs-th item: 200
    rows over two groups = 100 rows = 8 items (4 blocks x 2 heads, the last block ragged) per launch on 1 | 3 workgroups"""
    monkeypatch.setenv("GAZ_HEADS_WGS", str(wgs))
    two = _engine(monkeypatch, False, weights, n_games=200, game_groups=2)
    one = _engine(monkeypatch, True, weights, n_games=200, game_groups=2)
    try:
        x = _random_states(200)
        p2, v2, _ = two.evaluate(x)
        p1, v1, _ = one.evaluate(x)
        assert np.isfinite(p1).all() and np.allclose(p1.sum(1), 1.0, atol=1e-5)
        assert p1.tobytes() == p2.tobytes() and v1.tobytes() == v2.tobytes()
    finally:
        two.close(); one.close()

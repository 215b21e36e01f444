"""Shared by tests/test_samples_emu.py and tests/test_samples_gpu.py: finished games as training samples, once through the host path
(drain_finished + record_to_samples: the definition) and once through gaz_engine_drain_samples (the kernel)."""
import numpy as np


def host_games(eng, game_class):
    """one drain through the host path -> [((slot, game_seq), boards, policies, values, T, winner)]"""
    from grok_alpha_zero_amd.self_play import record_to_samples
    out = []
    for r in eng.drain_finished():
        b, p, v, length = record_to_samples(game_class, r)
        assert length == r["T"]
        out.append(((r["slot"], r["game_seq"]), b, p, v, r["T"], r["winner"]))
    return out


def device_games(eng, **kw):
    """one drain through drain_samples -> the same tuples (copies: the engine reuses its buffers)"""
    batch = eng.drain_samples(**kw)
    assert batch.games.dtype == np.int32 and batch.games.shape == (batch.n, 6)
    assert batch.boards.dtype == np.int8 and batch.policies.dtype == np.float32 and batch.values.dtype == np.float32
    assert batch.boards.shape[1] == batch.policies.shape[1] == batch.values.shape[0] == int(batch.games[:, 0].sum())
    assert batch.values.shape[1:] == (1,)
    out, row = [], int(batch.games[0, 4]) if batch.n else 0
    for i in range(batch.n):
        T, winner, slot, seq, r0, zero = (int(x) for x in batch.games[i])
        assert r0 == row and zero == 0
        row += T
        b, p, v, length, n_pos, w = batch.game(i)
        assert length == T == n_pos and w == winner
        out.append(((slot, seq), b.copy(), p.copy(), v.copy(), T, winner))
    return out


def assert_same_game(dev, host, what=""):
    (kd, bd, pd, vd, Td, wd), (kh, bh, ph, vh, Th, wh) = dev, host
    assert kd == kh and Td == Th and wd == wh, (what, kd, kh, Td, Th, wd, wh)
    for name, a, b in (("boards", bd, bh), ("policies", pd, ph), ("values", vd, vh)):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, kd, a.dtype, b.dtype, a.shape, b.shape)
        np.testing.assert_array_equal(a, b, err_msg=f"{what} {name} of game {kd}")


def assert_matches_reference_fixture(game, fx):
    """one game from device_games() vs the arrays the reference's Self_Play.play() wrote for that game (aug_boards_k / aug_policies_k / values)"""
    _, b, p, v, T, _ = game
    n_aug = int(fx["n_aug"])
    assert T == len(fx["actions"]) and b.shape[0] == n_aug == p.shape[0] == v.shape[0]
    for k in range(n_aug):
        want_b, want_p = fx[f"aug_boards_{k}"], fx[f"aug_policies_{k}"]
        assert b[k].dtype == want_b.dtype == np.int8 and p[k].dtype == want_p.dtype == np.float32
        assert b[k].shape == want_b.shape and p[k].shape == want_p.shape
        np.testing.assert_array_equal(b[k], want_b, err_msg=f"boards, augmentation {k}")
        np.testing.assert_array_equal(p[k], want_p, err_msg=f"policies, augmentation {k}")
        assert v[k].dtype == fx["values"].dtype and v[k].shape == fx["values"].shape
        np.testing.assert_array_equal(v[k], fx["values"], err_msg=f"values, augmentation {k}")


def file_contents(store):
    """every dataset of a replay file: {name: array}"""
    n = store.n_datasets()
    assert n % 3 == 0
    out = {"game_stats": store.game_stats()}
    for k in range(n // 3):
        for kind in ("boards", "policies", "values"):
            out[f"{kind}_{k}"] = store.read(f"{kind}_{k}")
    return out


def assert_same_file(a, b):
    assert list(a) == list(b)
    for name in a:
        assert a[name].dtype == b[name].dtype and a[name].shape == b[name].shape, name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)

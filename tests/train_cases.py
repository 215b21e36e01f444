"""The cases of training on the device (grok_alpha_zero_amd/train.py, orchestrator.Run(train=...)) that the CPU suite runs
on the emulation build with torch on the CPU (tests/test_train_emu.py) and the -m gpu suite on the HIP build with torch on the device
(tests/test_train_gpu.py): `lib_path` = the emulation library, or None for the product library.

The network is the smallest the evaluator runs, the 1-block TicTacToe network; the window holds at most 256 random rows made by the generators of
tests/replay_cases.py.  What the optimizer must do to the network is computed by tests/optim_model.py from the grads the case reads back after each
backward pass — bit for bit, with no tolerance on torch's convolutions; the losses are held to tests/score_model.py and to a numpy restatement of
Keras' clips."""
import json
import math
import os

import numpy as np

import optim_cases as OC
import replay_cases as RC
import score_cases as SC
import score_model as SM

GAME = "TicTacToe"
BUILD = dict(num_resnet_layers=1, use_grok_fast=True, use_orthograd=True, grok_fast_lambda=2.0)
TRAIN = dict(RC.TRAIN, learning_rate=1e-3, lr_decay=0.5, decay_lr_after=1, beta_1=0.9, beta_2=0.995, optimizer="Nadam", train_epochs=3, train_batch_size=64,
             test_batch_size=None, train_percent=1.0, train_decay=0.25, test_percent=1.0, test_decay=0.25)
OPT_KW = dict(kind=1, beta_1=0.9, beta_2=0.995, orthograd=True, grokfast=True, lamb=2.0, weight_decay=0.0)
U = 2.0 ** -24                                     # the unit roundoff of float32


def filled_window(lib_path, rows=256, generations=(0,), seed=4, test_fraction=0.2):
    """a window of `rows` random rows per generation, in games of up to 9 rows"""
    rng = np.random.default_rng(seed)
    w = RC.window(GAME, 4096, lib_path, seed=seed, test_fraction=test_fraction)
    for g in generations:
        lengths = [n for n in RC.lengths_summing_to(rng, rows) if n > 0]
        games, b, p, v = RC.random_rows(rng, GAME, lengths)
        b = rng.integers(-1, 2, b.shape).astype(np.int8)                  # boards of -1 / 0 / 1, as the games'
        p = (p / p.sum(1, keepdims=True)).astype(np.float32)
        w.append_arrays(g, games, b, p, v)
    return w


def torch_batch(w, first, n, on_host):
    import torch
    if on_host:
        return tuple(torch.from_numpy(a) for a in w.batch(first, n))
    return w.batch_torch(first, n)


# ------------------------------------------------------------------------------------------------ 1. three optimizer steps on the network
def steps_case(lib_path, gumbel=False):
    """forward, backward and three steps: after each backward the grads arena is read back and fed to the model; the library's params, state and
    the module's own tensors must equal the model's in every bit -> the number of tensors"""
    import torch
    from grok_alpha_zero_amd import train as T
    from grok_alpha_zero_amd.optim import FusedOptimizer
    configs = (BUILD, dict(TRAIN, use_gumbel=gumbel))
    mode = T.head_mode(configs)
    assert mode == (1 if gumbel else 0)
    net = T.training_network(RC.game_class(GAME), configs, seed=2)
    assert any(isinstance(m, T.TrainBN) for m in net.modules()) and not net.p_d3.weight.any()      # the reference's zero last Dense layers
    sizes = [p.numel() for p in net.parameters()]
    before = [p.detach().numpy().reshape(-1).copy() for p in net.parameters()]
    opt = FusedOptimizer(sizes, lib_path=lib_path, **OPT_KW)
    on_host = opt.host_memory
    net.to(torch.device("cpu") if on_host else torch.device("cuda", 0))
    opt.attach(net)
    model = OC.ModelState(sizes, OPT_KW)
    for k in range(len(sizes)):
        model.w[k] = before[k]
        OC.same_bits(opt.get("params", k), before[k], "attach keeps the values")
    w = filled_window(lib_path)
    M = w.begin_epoch("train", 0)
    assert 3 * 64 <= M <= 256
    net.train()
    for t in (1, 2, 3):
        b, y, z = torch_batch(w, 64 * (t - 1), 64, on_host)
        p, v = net(b)
        pl, vl = T.losses(p.double(), v.double(), y, z, mode) if gumbel else T.losses(p, v, y, z, mode)
        (pl + vl).float().backward()
        if not on_host:
            torch.cuda.synchronize()
        grads = [opt.get("grads", k) for k in range(len(sizes))]
        # (step 1: both heads end in the reference's zero Dense layers, so only those four tensors have a gradient; they move, and the rest follows)
        assert all(np.isfinite(g).all() for g in grads) and sum(bool(g.any()) for g in grads) >= (4 if t == 1 else len(sizes) // 2), "the backward pass reached the arena"
        opt.step(1e-3)
        model.step(grads, 1e-3, t)
        OC.compare(opt, model, f"network step {t}", grads_want=[np.zeros(n, np.float32) for n in sizes])
        for k, prm in enumerate(net.parameters()):
            OC.same_bits(prm.detach().cpu().numpy().reshape(-1), model.w[k], f"the module's tensor {k} after step {t}")
    moved = sum(bool((model.w[k] != before[k]).any()) for k in range(len(sizes)))
    last = [n for n, _ in net.named_parameters()].index("p_d3.weight")
    assert moved >= len(sizes) // 2 and not before[last].any() and model.w[last].any(), "Orthograd moves a zero tensor along its gradient"
    w.close()
    del net, prm
    opt.close()
    return len(sizes)


# ------------------------------------------------------------------------------------------------ 2. the training batch-norm
def batch_norm_case():
    """TrainBN on a [5, 7] input against numpy in float64.  Tolerance: the f32 path takes at most 17 roundings to an output (5 for the mean, a
    subtraction, a square, 5 for the variance, + eps, sqrt, /, * gamma, + beta), each a relative error of at most u = 2^-24 of a quantity bounded by
    A = max|gamma| max|x - mean| / sqrt(min var + eps) + max|beta| + 1 -> 20 u A; the moving statistics take three more on top of the mean's or the
    variance's, of quantities bounded by max(1, max x^2) -> 20 u max(1, max x^2)"""
    import torch
    from grok_alpha_zero_amd import train as T
    rng = np.random.default_rng(8)
    x = rng.standard_normal((5, 7)).astype(np.float32) * np.float32(1.5) + np.float32(0.3)
    bn = T.TrainBN(7)
    bn.randomize(torch.Generator().manual_seed(1))
    gamma, beta = bn.weight.detach().numpy().astype(np.float64), bn.bias.detach().numpy().astype(np.float64)
    rm0, rv0 = bn.running_mean.numpy().astype(np.float64), bn.running_var.numpy().astype(np.float64)
    xd = x.astype(np.float64)
    mean, var = xd.mean(0), xd.var(0)                                    # the biased variance
    want = (xd - mean) / np.sqrt(var + 1e-3) * gamma + beta
    bn.train()
    got = bn(torch.from_numpy(x)).detach().numpy()
    A = np.abs(gamma).max() * np.abs(xd - mean).max() / math.sqrt(var.min() + 1e-3) + np.abs(beta).max() + 1
    assert np.abs(got - want).max() <= 20 * U * A, (np.abs(got - want).max(), 20 * U * A)
    tol = 20 * U * max(1.0, float((xd * xd).max()))
    assert np.abs(bn.running_mean.numpy() - (rm0 * 0.99 + mean * 0.01)).max() <= tol
    assert np.abs(bn.running_var.numpy() - (rv0 * 0.99 + var * 0.01)).max() <= tol
    assert np.abs(bn.running_var.numpy() - (rv0 * 0.99 + xd.var(0, ddof=1) * 0.01)).max() > tol, "the moving variance takes the biased variance"
    bn.eval()                                                            # eval mode is net._BN: the moving statistics
    rm, rv = bn.running_mean.numpy().astype(np.float64), bn.running_var.numpy().astype(np.float64)
    got = bn(torch.from_numpy(x)).detach().numpy()
    want = (xd - rm) / np.sqrt(rv + 1e-3) * gamma + beta
    assert np.abs(got - want).max() <= 20 * U * (np.abs(gamma).max() * np.abs(xd - rm).max() / math.sqrt(rv.min() + 1e-3) + np.abs(beta).max() + 1)
    return float(np.abs(got - want).max())


# ------------------------------------------------------------------------------------------------ 3. the losses
def keras_cce(P, y):
    q = P / P.sum()
    q = np.clip(q, 1e-7, 1 - 1e-7)
    return float(-(y * np.log(q)).sum())


def keras_kld(q, y):
    yc, qc = np.clip(y, 1e-7, 1.0), np.clip(q, 1e-7, 1.0)
    return float((yc * np.log(yc / qc)).sum())


def loss_case(A=9):
    """train.losses in float64, a row at a time, on the hand-built edge rows of tests/score_cases.py.
    Against tests/score_model.py: the value loss is its se; the policy loss differs from its ce (modes 0, 2) or ce - entropy (modes 1, 3) by what
    Keras adds and the score model leaves out — the renormalisation by sum(P) and the clip to [1e-7, 1 - 1e-7] under modes 0 / 2, the terms
    1e-7 log(1e-7 / q) of the entries with y = 0 under modes 1 / 3 — so the comparison is made on the rows where no clip acts, with that
    difference added; every row is also held to a numpy restatement of Keras' formula, and the clip is tested on its own -> rows compared"""
    import torch
    from grok_alpha_zero_amd import train as T
    rel = lambda a, b: abs(a - b) <= 1e-10 * max(1.0, abs(b))             # noqa: E731 — float64 throughout: rounding only
    seen = dict(model=0, keras=0, clip=0)
    for mode in (0, 1, 2, 3):
        P, v, y, z = SC.hand_rows(A, mode)
        for r in range(P.shape[0]):
            ce, ent, se, flags = SM.score_row(P[r], v[r], y[r], z[r], mode)
            if flags & SM.BAD:
                continue
            Pd, yd = P[r].astype(np.float64), y[r].astype(np.float64)
            pl, vl = T.losses(torch.from_numpy(Pd)[None], torch.tensor([[float(v[r])]], dtype=torch.float64), torch.from_numpy(y[r])[None], torch.tensor([float(z[r])]), mode)
            pl, vl = float(pl), float(vl)
            assert vl == se, (mode, r, vl, se)
            q = SM.probabilities(P[r], mode)
            if mode in (0, 2):
                assert rel(pl, keras_cce(Pd, yd)), (mode, r, pl)
                qn = Pd / Pd.sum()
                unclipped = (qn[yd > 0] > 1e-7).all() and (qn[yd > 0] < 1 - 1e-7).all() and (Pd[yd > 0] > 1e-7).all()
                if unclipped:                                             # Keras' ce = the model's + sum(y) log(sum P)
                    assert rel(pl, ce + yd.sum() * math.log(Pd.sum())), (mode, r, pl, ce)
                    seen["model"] += 1
            else:
                assert rel(pl, keras_kld(q, yd)), (mode, r, pl)
                if (q[yd > 0] > 1e-7).all() and (yd[yd > 0] >= 1e-7).all():   # Keras' KL = the model's + the y = 0 entries at y = 1e-7
                    extra = sum(1e-7 * math.log(1e-7 / max(qa, 1e-7)) for qa, ya in zip(q, yd) if ya == 0)
                    assert rel(pl, (ce - ent) + extra), (mode, r, pl, ce - ent, extra)
                    seen["model"] += 1
            seen["keras"] += 1
    # the clip on its own: a probability below 1e-7 under y > 0 costs -y log(1e-7), one above 1 - 1e-7 costs -y log(1 - 1e-7), never 0 or inf
    y = torch.tensor([[0.5, 0.5, 0.0]], dtype=torch.float64)
    pl, _ = T.losses(torch.tensor([[1.0 - 1e-12, 1e-12, 0.0]], dtype=torch.float64), torch.zeros(1, 1, dtype=torch.float64), y, torch.zeros(1), 0)
    assert rel(float(pl), -0.5 * math.log(1e-7) - 0.5 * math.log(1 - 1e-7)); seen["clip"] += 1
    pl, _ = T.losses(torch.tensor([[200.0, -200.0, 0.0]], dtype=torch.float64), torch.zeros(1, 1, dtype=torch.float64), y, torch.zeros(1), 1)
    assert rel(float(pl), keras_kld(np.array([1.0, 0.0, math.exp(-200.0)]), np.array([0.5, 0.5, 0.0]))) and math.isfinite(float(pl)); seen["clip"] += 1
    pl, vl = T.losses(torch.tensor([[0.2, 0.3, 0.5], [0.5, 0.25, 0.25]]), torch.tensor([[0.5], [-1.0]]), torch.tensor([[1.0, 0, 0], [0, 1.0, 0]]), torch.tensor([1.0, 1.0]), 0)
    assert abs(float(pl) - (-math.log(0.2) - math.log(0.25)) / 2) < 1e-6 and abs(float(vl) - (0.25 + 4.0) / 2) < 1e-6      # the mean over the batch
    assert seen["model"] >= 12 and seen["keras"] >= 30, seen
    return seen


# ------------------------------------------------------------------------------------------------ 4. train_generation
def generation_case(tmp, lib_path):
    """generation 0 from a fresh network, generation 1 from generation 0's train_state.pt, and a generation of no epochs that must hand the
    loaded state on unchanged -> the three summaries"""
    import torch
    from grok_alpha_zero_amd import train as T
    from grok_alpha_zero_amd.net import check_engine_weights
    cls, configs = RC.game_class(GAME), (BUILD, TRAIN)
    w = filled_window(lib_path, rows=160, generations=(0, 1))
    dirs = [os.path.join(str(tmp), str(g)) for g in range(4)]
    os.makedirs(dirs[0], exist_ok=True)
    lines, out = [], []
    for g in (0, 1):
        out.append(T.train_generation(w, cls, configs, g, dirs[g], dirs[g + 1], lib_path=lib_path, out=lines.append))
        s = out[-1]
        with open(os.path.join(dirs[g + 1], "Train.json")) as f:
            assert json.load(f) == json.loads(json.dumps(s))
        assert s["resumed"] == (g == 1) and len(s["epochs"]) == TRAIN["train_epochs"] and s["launches_per_step"] == 3
        assert s["lr"] == 1e-3 * 0.5 ** g and s["optimizer"]["kind"] == "nadam" and s["optimizer"]["beta_2"] == 0.995 and s["optimizer"]["lamb"] == 2.0
        val = [e["val_loss"] for e in s["epochs"]]
        assert all(math.isfinite(e["train_loss"]) and math.isfinite(e["val_loss"]) and e["train_rows"] > 0 and e["val_rows"] > 0 for e in s["epochs"])
        assert s["best_epoch"] == val.index(min(val)), "the epoch of the lowest val loss is kept"
        steps = [sum(1 for _ in range(0, e["train_rows"], 64)) if e["train_rows"] >= 64 else 1 for e in s["epochs"]]
        assert [e["steps"] for e in s["epochs"]] == list(np.cumsum(steps)), "a step per batch, the short last batch included"
        weights = T.weights_from_folder(dirs[g + 1])
        check_engine_weights(GAME, 1, 128, weights)
        assert all(np.isfinite(a).all() for a in weights.values())
    assert out[1]["epochs"][0]["train_rows"] > out[0]["epochs"][0]["train_rows"], "generation 1 trains on both generations' rows"
    assert T.weights_from_folder(dirs[0]) is None
    a, b = T.weights_from_folder(dirs[1]), T.weights_from_folder(dirs[2])
    assert any(a[k].tobytes() != b[k].tobytes() for k in a), "generation 1 moved the network"
    # the loaded state equals the saved one: no epochs -> train_state.pt and weights.npz of folder 2 arrive in folder 3 bit for bit, through
    # load, the arenas and export
    s = T.train_generation(w, cls, (BUILD, dict(TRAIN, train_epochs=0)), 2, dirs[2], dirs[3], lib_path=lib_path, out=lines.append)
    assert s["resumed"] and s["epochs"] == [] and s["best_epoch"] is None
    s2, s3 = (torch.load(os.path.join(d, "train_state.pt"), weights_only=True)["model"] for d in dirs[2:4])
    assert list(s2) == list(s3) and all(s2[k].numpy().tobytes() == s3[k].numpy().tobytes() for k in s2)
    c = T.weights_from_folder(dirs[3])
    assert all(b[k].tobytes() == c[k].tobytes() for k in b)
    assert any(ln.startswith("Started training for generation: 1 using lr = 0.0005") for ln in lines)
    w.close()
    return out + [s]


# ------------------------------------------------------------------------------------------------ 5. Run(train=...)
def run_case(tmp, lib_path):
    """Run(replay=..., train=dict()) over two generations at a handful of games.  On the emulation build the network cannot be played (the ResNet
    evaluator needs the HIP build): weights_fn says None and self-play stays synthetic.  On the HIP build weights_fn is the default: generation 1's
    self-play must load the weights.npz training wrote, and Score.json's `new` must differ from `current`."""
    from grok_alpha_zero_amd import engine as E
    from grok_alpha_zero_amd import train as T
    from grok_alpha_zero_amd.orchestrator import Run
    from grok_alpha_zero_amd.optim import FusedOptimizer
    cls = RC.game_class(GAME)
    probe = FusedOptimizer([4], lib_path=lib_path)
    on_host = probe.host_memory
    probe.close()
    root = os.path.join(str(tmp), "run")
    train_cfg = dict(TRAIN, train_epochs=2, train_batch_size=32)
    spec = dict(capacity_rows=4096, generations=2, test_fraction=0.2, target_ratio=None, seed=5)
    kw = dict(root=root, n_games=8, seed=20, lib_path=lib_path, out=lambda *a: None, train=dict(seed=3))
    loaded = []
    real = E.SelfPlayEngine.load_weights

    def spy(self, weights, *a, **k):
        loaded.append((int(self.cfg.evaluator), np.asarray(weights["stem.w"]).tobytes()))
        return real(self, weights, *a, **k)
    E.SelfPlayEngine.load_weights = spy
    try:
        if on_host:
            stats = Run(cls, (BUILD, train_cfg), weights_fn=lambda folder: None, replay=spec, self_play_kwargs=dict(hash_salt=4, allow_synthetic=True), **kw)
        else:
            stats = Run(cls, (BUILD, train_cfg), replay=dict(spec, score=dict(batch_rows=32)), self_play_kwargs=dict(hash_salt=4), **kw)
    finally:
        E.SelfPlayEngine.load_weights = real
    assert len(stats) == 2 and all(len(st["train"]["epochs"]) == 2 for st in stats) and stats[1]["train"]["resumed"] and not stats[0]["train"]["resumed"]
    for g in (1, 2):
        folder = os.path.join(root, str(g))
        assert all(os.path.exists(os.path.join(folder, f)) for f in ("train_state.pt", "weights.npz", "Train.json"))
    w1, w2 = T.weights_from_folder(os.path.join(root, "1")), T.weights_from_folder(os.path.join(root, "2"))
    assert w1["stem.w"].tobytes() != w2["stem.w"].tobytes()
    if not on_host:
        assert (E.EVAL_RESNET, w1["stem.w"].tobytes()) in loaded, "generation 1's self-play loaded the weights.npz that generation 0's training wrote"
        for g in (1, 2):
            with open(os.path.join(root, str(g), "Score.json")) as f:
                sc = json.load(f)
            assert sc["new"]["val_loss"] != sc["current"]["val_loss"] and sc["new"]["rows"] > 0 and math.isfinite(sc["new"]["val_loss"]), sc
    return stats


def refusal_case(tmp, lib_path):
    """train with train_fn, train without replay, "muon", mixed_precision — each by its text, before anything is played"""
    from grok_alpha_zero_amd.engine import EngineError
    from grok_alpha_zero_amd.orchestrator import Run
    cls, root = RC.game_class(GAME), os.path.join(str(tmp), "refused")
    spec = dict(capacity_rows=64, generations=1)
    msgs = {}
    for what, exc, call in (
            ("train_fn", ValueError, lambda: Run(cls, (BUILD, TRAIN), train_fn=lambda *a, **k: None, replay=spec, train=dict(), root=root, lib_path=lib_path)),
            ("replay", ValueError, lambda: Run(cls, (BUILD, TRAIN), train=dict(), root=root, lib_path=lib_path)),
            ("muon", EngineError, lambda: Run(cls, (BUILD, dict(TRAIN, optimizer="muon")), replay=spec, train=dict(), root=root, lib_path=lib_path)),
            ("muon in optimizer_config", EngineError, lambda: Run(cls, (BUILD, TRAIN, dict(optimizer="Muon")), replay=spec, train=dict(), root=root, lib_path=lib_path)),
            ("mixed_precision", EngineError, lambda: Run(cls, (BUILD, dict(TRAIN, mixed_precision="mixed_float16")), replay=spec, train=dict(), root=root, lib_path=lib_path))):
        try:
            call()
        except exc as e:
            msgs[what] = str(e)
        else:
            raise AssertionError(f"{what}: accepted")
    assert "exclude each other" in msgs["train_fn"] and "needs replay=" in msgs["replay"] and "'muon' is not supported" in msgs["muon"]
    assert "'muon' is not supported" in msgs["muon in optimizer_config"] and "mixed_precision = 'mixed_float16' is not supported" in msgs["mixed_precision"]
    assert not os.path.exists(root), "a refused Run leaves nothing behind"
    return msgs

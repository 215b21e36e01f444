"""Training on the device — the step that Train_NN + train (<Game>/main.py:100-135, Train.py:14-66) take between two generations of self-play:
the net.py networks in training form, the reference's losses, and train_generation, which produces generation g + 1's weights from the replay
window (replay.ReplayWindow) with optim.FusedOptimizer.  The forward and backward passes are PyTorch autograd; the optimizer chain
Orthograd(Grokfast_EMA(Adam | Nadam | Muon)) is the HIP step of csrc/optim.hpp and csrc/muon.hpp (DESIGN.md sections 28 and 29).  With
optimizer = "muon" (Gomoku.py's optimizer_config) the parameters are classified as muon.py's _should_use_adamw does — muon_classification — and
the weight matrices take momentum and Newton-Schulz on f32 MFMA.

    Run(game_class, configs, replay=dict(capacity_rows=..., generations=3), train=dict())      # plays, trains, scores and plays again

Not here: a training-mode forward or backward in HIP, fp16 / bf16 training (mixed_precision is refused), Muon's caution=True and Muon named without
an optimizer_config kwargs dict (both refused), multi-GPU training."""
import json
import math
import os
import re
import time

import numpy as np
import torch
import torch.nn as nn

from . import net as N
from .engine import EngineError

KERAS_EPS = 1e-7                                    # keras.backend.epsilon(): the clip of CategoricalCrossentropy and KLDivergence
BN_MOMENTUM = 0.99                                  # keras.layers.BatchNormalization's default
# muon.py's keywords with its defaults; learning_rate is read by configured_lr, caution is accepted only as False
MUON_KWARGS = dict(learning_rate=None, adam_lr_ratio=1.0, use_nadam=True, weight_decay=0.004, exclude_layers=(), exclude_embeddings=True, nesterov=True, adam_beta_1=0.9,
                   adam_beta_2=0.995, muon_beta=0.95, muon_a=3.4445, muon_b=-4.7750, muon_c=2.0315, ns_steps=5, epsilon=1e-8, caution=False)
# the Keras layer names <Game>/Build_Model.py gives explicitly, by net.py module: what exclude_layers patterns are written against.  The other
# layers carry Keras' automatic names (dense_3, conv2d_7), which depend on what the process built before and are not reproduced.
KERAS_LAYER_NAMES = {"TicTacToe": {}, "Connect4": {}, "Gomoku": {"p_d1": "policy_1", "p_d2": "policy_2", "v_d1": "value_1", "v_d2": "value_2", "v_d3": "value_3"}}


class TrainBN(N._BN):
    """net._BN with Keras' training behaviour: in train() mode the batch statistics over every axis but the last normalise the input — the
    BIASED variance, which is also what moves the moving variance — and moving = moving * 0.99 + batch * 0.01; eps = 1e-3.  In eval() mode it
    is net._BN: the moving statistics, and affine() is what export_engine_weights folds."""

    def forward(self, x):
        if not self.training:
            return super().forward(x)
        axes = tuple(range(x.dim() - 1))
        mean = x.mean(axes)
        var = (x - mean).square().mean(axes)
        with torch.no_grad():
            self.running_mean.mul_(BN_MOMENTUM).add_(mean.detach() * (1.0 - BN_MOMENTUM))
            self.running_var.mul_(BN_MOMENTUM).add_(var.detach() * (1.0 - BN_MOMENTUM))
        return (x - mean) / torch.sqrt(var + N.BN_EPS) * self.weight + self.bias


def head_mode(configs):
    """the policy_mode of the held-out loss (include/gaz_engine.h "HELD-OUT LOSS") that the configs' head has: 0 softmax probabilities, 2 Stablemax
    probabilities, 1 / 3 logits of a softmax / Stablemax head (use_gumbel)"""
    stable = bool(configs[0].get("use_stablemax"))
    return (3 if stable else 1) if configs[1].get("use_gumbel") else (2 if stable else 0)


def training_network(game_class, configs, seed=0):
    """the game's net.py network for these configs with every batch-norm a TrainBN; a fresh one has the reference's zero last Dense layers"""
    name = getattr(game_class, "ENGINE_NAME", game_class.__name__)
    if name not in N.NETS:
        raise EngineError(f"train: no network for the game {name}")
    build_config = configs[0]
    head = {0: "softmax", 2: "stablemax", 1: "linear", 3: "linear"}[head_mode(configs)]
    kw = dict(policy_head=head, seed=seed)
    if name != "TicTacToe":
        kw["num_filters"] = int(build_config.get("num_filters", 128))
    if name != "Gomoku":
        kw["final_std"] = 0.0
    net = N.NETS[name](int(build_config["num_resnet_layers"]), **kw)
    for m in net.modules():
        if type(m) is N._BN:
            m.__class__ = TrainBN                       # same parameters and buffers, the training forward
    return net


def losses(p, v, y, z, mode):
    """(policy loss, value loss), each the mean over the batch, of network outputs p [B, A] (probabilities under modes 0 / 2, logits under 1 / 3)
    and v [B, 1] or [B] against targets y [B, A] and z [B]; computed in p's dtype.
    Modes 0 / 2, Net/Alpha_Loss.py: Keras' CategoricalCrossentropy on probabilities — p / sum(p), clipped to [1e-7, 1 - 1e-7], -sum(y log p) — and
    MeanSquaredError.  Modes 1 / 3, Net/Gumbel_Loss.py: the activation (softmax, or Stablemax for 3) on the logits, then Keras' KLDivergence —
    y and q clipped to [1e-7, 1], sum(y log(y / q)) — and MeanSquaredError; the reference runs these in float64, pass doubles for that."""
    y, z = y.to(p.dtype), z.to(p.dtype).reshape(-1)
    if mode in (0, 2):
        q = p / p.sum(-1, keepdim=True)
        q = q.clamp(KERAS_EPS, 1.0 - KERAS_EPS)
        pl = -(y * q.log()).sum(-1)
    else:
        q = torch.softmax(p, -1) if mode == 1 else N.stablemax(p)
        yc, qc = y.clamp(KERAS_EPS, 1.0), q.clamp(KERAS_EPS, 1.0)
        pl = (yc * (yc / qc).log()).sum(-1)
    vl = (v.reshape(-1) - z).square()
    return pl.mean(), vl.mean()


def optimizer_settings(configs):
    """what the configs say about the optimizer -> the keywords of optim.FusedOptimizer plus train_epochs and accumulation.  A key comes from
    configs[2] (Train.py's optimizer_config) where present, else from the names Connect4.py uses in train_config / build_config."""
    build_config, train_config = configs[0], configs[1]
    oc = configs[2] if len(configs) > 2 and configs[2] else {}

    def pick(pairs, default=None):
        for d, k in pairs:
            if k in d and d[k] is not None:
                return d[k]
        return default
    if train_config.get("mixed_precision") is not None:
        raise EngineError(f"train: mixed_precision = {train_config['mixed_precision']!r} is not supported: training is float32")
    name = str(pick([(oc, "optimizer"), (train_config, "optimizer")], "Nadam")).lower()
    if name not in ("adam", "adamw", "nadam", "muon"):
        raise EngineError(f"train: unknown optimizer {name!r}: use 'Adam', 'AdamW', 'Nadam' or 'Muon'")
    kwargs = dict(oc.get("kwargs") or {})
    common = dict(orthograd=bool(pick([(oc, "use_orthograd"), (build_config, "use_orthograd")], False)),
                  grokfast=bool(pick([(oc, "use_grokfast"), (oc, "use_grok_fast"), (build_config, "use_grok_fast")], False)),
                  lamb=float(pick([(oc, "grokfast_lambda"), (oc, "grok_fast_lambda"), (build_config, "grok_fast_lambda")], 5.0)),
                  train_epochs=int(pick([(oc, "train_epochs"), (train_config, "train_epochs")], 1)),
                  accumulation=max(int(pick([(oc, "gradient_accumulation_steps"), (train_config, "gradient_accumulation_steps")], 1)), 1))
    if name == "muon":                              # Net/Optimizers/muon.py: its own Adam constants, its own keywords
        # Train.py reaches Muon only as Muon(**optimizer_config["kwargs"]): there is no Muon under the train_config names Connect4.py uses, and an
        # optimizer_config without its kwargs dict fails there too
        if not isinstance(oc.get("kwargs"), dict) or str(oc.get("optimizer", "")).lower() != "muon":
            raise EngineError("train: the optimizer 'muon' is not supported without its keywords: name it in optimizer_config (configs[2]) with a kwargs dict, as "
                              "Gomoku.py does (an empty one takes muon.py's defaults)")
        unknown = sorted(set(kwargs) - set(MUON_KWARGS))
        if unknown:
            raise EngineError(f"train: the optimizer 'muon' has no keywords {unknown}: it takes {sorted(MUON_KWARGS)}")
        k = dict(MUON_KWARGS, **{a: b for a, b in kwargs.items() if b is not None})
        if k["caution"]:
            raise EngineError("train: the optimizer 'muon' with caution=True is not supported: pass caution=False")
        return dict(common, kind="nadam" if k["use_nadam"] else "adam", beta_1=float(k["adam_beta_1"]), beta_2=float(k["adam_beta_2"]), epsilon=float(k["epsilon"]),
                    weight_decay=float(k["weight_decay"]), exclude_layers=[str(p) for p in k["exclude_layers"]], exclude_embeddings=bool(k["exclude_embeddings"]),
                    muon=dict(muon_beta=float(k["muon_beta"]), nesterov=bool(k["nesterov"]), muon_a=float(k["muon_a"]), muon_b=float(k["muon_b"]), muon_c=float(k["muon_c"]),
                              ns_steps=int(k["ns_steps"]), adam_lr_ratio=float(k["adam_lr_ratio"])))
    return dict(kind="nadam" if name == "nadam" else "adam",
                beta_1=float(pick([(kwargs, "beta_1"), (train_config, "beta_1")], 0.9)), beta_2=float(pick([(kwargs, "beta_2"), (train_config, "beta_2")], 0.999)),
                epsilon=float(pick([(kwargs, "epsilon"), (train_config, "epsilon")], 1e-7)),
                weight_decay=float(pick([(kwargs, "weight_decay"), (train_config, "weight_decay")], 0.004 if name == "adamw" else 0.0)),     # 0.004: Keras' AdamW default
                **common)


def learning_rate(train_config, generation, accumulation=1):
    """learning_rate * lr_decay ** (generation // decay_lr_after) (<Game>/main.py:122-123), divided by the accumulation steps (Train.py:17-19)"""
    lr = float(train_config["learning_rate"]) * math.pow(float(train_config.get("lr_decay", 1.0)), generation // max(int(train_config.get("decay_lr_after", 1)), 1))
    return lr / accumulation if accumulation >= 2 else lr


def configured_lr(configs, generation, accumulation=1):
    """the learning rate of a generation: optimizer_config["kwargs"]["learning_rate"] where present — a number, or a function of the generation as in
    Gomoku.py (<Game>/main.py:122-125) — else learning_rate(train_config, ...); divided by the accumulation steps either way"""
    oc = configs[2] if len(configs) > 2 and configs[2] else {}
    lr = (oc.get("kwargs") or {}).get("learning_rate")
    if lr is None:
        return learning_rate(configs[1], generation, accumulation)
    lr = float(lr(generation) if callable(lr) else lr)
    return lr / accumulation if accumulation >= 2 else lr


def muon_classification(game_name, net, exclude_layers=(), exclude_embeddings=True):
    """every parameter of a net.py network as muon.py's _should_use_adamw sees it -> a list, in net.parameters() order, of dict(name, keras_name, shape,
    path "adam" | "muon", and for a Muon tensor rows, cols, scale).  Adam: fewer than two dimensions, "bias" in the name, "embedding" in the name
    (exclude_embeddings), or a pattern of exclude_layers found by re.search in the Keras variable path (KERAS_LAYER_NAMES) or in the net.py name."""
    from .optim import muon_scale
    table, out = KERAS_LAYER_NAMES.get(game_name, {}), []
    for name, p in net.named_parameters():
        module, _, leaf = name.rpartition(".")
        keras = f"{table[module]}/{'kernel' if leaf == 'weight' else leaf}" if module in table else None
        shape = tuple(int(d) for d in p.shape)
        seen = [x for x in (name, keras) if x]
        adam = (len(shape) < 2 or any("bias" in x.lower() for x in seen) or (exclude_embeddings and any("embedding" in x.lower() for x in seen))
                or any(re.search(pat, x) for pat in exclude_layers for x in seen))
        row = dict(name=name, keras_name=keras, shape=list(shape), path="adam" if adam else "muon")
        if not adam:
            row.update(rows=shape[0], cols=int(np.prod(shape[1:])), scale=float(muon_scale(shape)))
        out.append(row)
    return out


def weights_from_folder(folder):
    """the weights_fn of orchestrator.Run for what train_generation writes: the tensors of folder/weights.npz, or None when there is none"""
    path = os.path.join(folder, "weights.npz")
    if not os.path.exists(path):
        return None
    with np.load(path) as f:
        return {k: f[k] for k in f.files}


def _cpu_state(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def train_generation(window, game_class, configs, generation, folder, save_folder, device=0, lib_path=None, out=print, seed=0):
    """Train_NN + train: the network of folder/train_state.pt (a fresh one when there is none) is trained for train_epochs on the window's train
    split — begin_epoch("train", epoch) with train_percent / train_decay, batches of train_batch_size with the reference's short last batch — by a
    NEW FusedOptimizer (the reference makes one per generation) at learning_rate(...); after every epoch the mean loss on the test split in
    eval mode (test_percent, test_decay, test_batch_size); the state of the epoch with the lowest val loss is kept (ModelCheckpoint,
    save_best_only; without test rows: the last epoch's).  Writes save_folder/train_state.pt, weights.npz (export_engine_weights()) and
    Train.json, and returns Train.json's dict."""
    from .optim import FusedOptimizer
    build_config, train_config = configs[0], configs[1]
    name = getattr(game_class, "ENGINE_NAME", game_class.__name__)
    st = optimizer_settings(configs)
    epochs, accum = st.pop("train_epochs"), st.pop("accumulation")
    mode = head_mode(configs)
    lr = configured_lr(configs, generation, accum)
    net = training_network(game_class, configs, seed=seed)
    classification = None
    if "muon" in st:
        classification = muon_classification(name, net, st.pop("exclude_layers"), st.pop("exclude_embeddings"))
        st["muon"] = dict(st["muon"], adam_tensors=[k for k, row in enumerate(classification) if row["path"] == "adam" and len(row["shape"]) >= 2])
        st["shapes"] = [tuple(row["shape"]) for row in classification]
    state_path = os.path.join(folder, "train_state.pt")
    resumed = os.path.exists(state_path)
    if resumed:
        net.load_state_dict(torch.load(state_path, weights_only=True)["model"])
    opt = FusedOptimizer([p.numel() for p in net.parameters()], device=device, lib_path=lib_path, **st)
    on_host = opt.host_memory                       # the one-lane test build: torch on the CPU, the arenas shared through numpy
    dev = torch.device("cpu") if on_host else torch.device("cuda", int(device))
    net.to(dev)
    opt.attach(net)
    bs = int(train_config["train_batch_size"])
    test_bs = int(train_config.get("test_batch_size") or bs)

    def batch(first, n):
        if on_host:
            return tuple(torch.from_numpy(a) for a in window.batch(first, n))
        return window.batch_torch(first, n)

    def forward_loss(first, n):
        b, y, z = batch(first, n)
        p, v = net(b)
        if mode in (1, 3):
            p, v = p.double(), v.double()           # Gumbel_Loss.py runs in float64
        pl, vl = losses(p, v, y, z, mode)
        return (pl + vl).float()
    out(f"Started training for generation: {generation} using lr = {lr}!")
    log, best, best_state, steps, pending = [], None, None, 0, 0
    for epoch in range(epochs):
        t0 = time.time()
        rows = window.begin_epoch("train", epoch, newest_generation=generation, percent=float(train_config.get("train_percent", 1.0)),
                                  decay=float(train_config.get("train_decay", 0.0)))
        net.train()
        total = torch.zeros((), dtype=torch.float64, device=dev)
        for first, n in window.batch_sizes(bs):
            loss = forward_loss(first, n)
            loss.backward()
            pending += 1
            if pending == accum:                    # gradient accumulation: a step every accum-th batch, the grads arena adds up in between
                opt.step(lr)
                steps, pending = steps + 1, 0
            total += loss.detach().double() * n
        train_loss = float(total) / rows if rows else None
        val_rows = window.begin_epoch("test", epoch, newest_generation=generation, percent=float(train_config.get("test_percent", 1.0)),
                                      decay=float(train_config.get("test_decay", 0.0)))
        net.eval()
        total = torch.zeros((), dtype=torch.float64, device=dev)
        with torch.no_grad():
            for first, n in window.batch_sizes(test_bs):
                total += forward_loss(first, n).double() * n
        val_loss = float(total) / val_rows if val_rows else None
        opt.synchronize()
        if val_loss is None or best is None or val_loss < best:
            best = val_loss if val_loss is not None else best
            best_state, best_epoch = _cpu_state(net), epoch
        log.append(dict(epoch=epoch, train_loss=train_loss, val_loss=val_loss, train_rows=rows, val_rows=val_rows, lr=lr, steps=steps, seconds=time.time() - t0))
        out(f"epoch {epoch + 1}/{epochs}: loss {train_loss} val_loss {val_loss} ({rows} / {val_rows} rows, {steps} steps)")
    if best_state is None:
        best_state, best_epoch = _cpu_state(net), None
    opt.close()
    final = training_network(game_class, configs, seed=seed)
    final.load_state_dict(best_state)
    weights = final.eval().export_engine_weights()
    N.check_engine_weights(name, int(build_config["num_resnet_layers"]), int(build_config.get("num_filters", 128)), weights)
    os.makedirs(save_folder, exist_ok=True)
    torch.save(dict(model=best_state, generation=int(generation)), os.path.join(save_folder, "train_state.pt"))
    np.savez(os.path.join(save_folder, "weights.npz"), **weights)
    summary = dict(generation=int(generation), resumed=bool(resumed), lr=lr, policy_mode=mode, optimizer=dict({k: v for k, v in st.items() if k != "shapes"}, accumulation=accum),
                   epochs=log, best_epoch=best_epoch, steps=steps, launches_per_step=opt.launches_per_step)
    if classification is not None:
        summary["muon_classification"] = classification
    with open(os.path.join(save_folder, "Train.json"), "w") as f:
        json.dump(summary, f, indent=1)
    return summary

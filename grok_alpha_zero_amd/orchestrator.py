"""Generation loop around the engine — the self-play half of the reference's `Run()` (<Game>/main.py:232-352).

    Run(game_class, configs, train_fn, weights_fn)

keeps the reference's on-disk contract (`Grok_Zero_Train/<generation>/Self_Play_Data.h5`, resume from the highest generation
folder and from `game_stats[2]` inside it, `Print_Stats`, `compute_speed`) and replaces `run_self_play`'s worker processes +
inference server by one engine per GPU.  ONNX export and TensorRT caching are NOT part of this path (out of scope).  Training: either
Run(..., replay=dict(...), train=dict()) — the loop trains by itself with train.train_generation and plays with what it trained — or the caller
supplies

    train_fn(generation, folder_path, save_folder_path)   # Train_NN of <Game>/main.py:99-136; must leave the next
                                                          # generation's weights where weights_fn finds them
    weights_fn(folder_path) -> dict | None                # tensors for SelfPlayEngine.load_weights (net.export_engine_weights()
                                                          # or keras_weights.load_keras_weights); None = synthetic evaluator

Generation 0 plays with the synthetic evaluator, like the reference's session=None dummy (Self_Play.py:40).
"""
import json
import os
import time
from glob import glob
from pathlib import Path

import numpy as np

from .self_play import ReplayStore, play_match, run_self_play


def make_generation_folder(root, generation):
    os.makedirs(os.path.join(root, str(generation)), exist_ok=True)                     # <Game>/main.py:77-80


def make_dataset_file(folder_path):
    """`Self_Play_Data.h5` with a zeroed `game_stats` u32[6] (<Game>/main.py:82-86)."""
    ReplayStore(folder_path).create()


def current_generation(root):
    """Highest numbered folder under `root`, 0 when there is none (<Game>/main.py:251-254)."""
    gens = [int(Path(p).name) for p in glob(os.path.join(root, "*")) if Path(p).name.isdigit()]
    return max(gens) if gens else 0


def print_stats(folder_path, out=print):
    """<Game>/main.py:88-96."""
    max_actions, total_actions, n_games, p1, draws, p2 = (int(x) for x in ReplayStore(folder_path).game_stats())
    n = max(n_games, 1)
    out("---------Game Statistics---------")
    out(f"Longest game is: {max_actions} actions long!")
    out(f"Average moves: {round(total_actions / n, 4)}")
    out(f"Player -1 winrate: {round(p1 / n, 4)}")
    out(f"Draw rate: {round(draws / n, 4)}")
    out(f"Player 1 winrate: {round(p2 / n, 4)}\n")
    return dict(max_actions=max_actions, total_actions=total_actions, games=n_games, wins_m1=p1, draws=draws, wins_p1=p2)


def compute_speed(game_class, configs, weights, batch=None, iterations=200, device=0, lib_path=None, out=print):
    """Evaluator probe (Compute_Speed.py:9-63): forward passes per second at `batch` positions (default `num_workers`, the
    reference's batch; the engine's own batch is the number of concurrent games).  Returns it/s."""
    from .engine import EVAL_RESNET, SelfPlayEngine
    build_config, train_config = configs[0], configs[1]
    name = getattr(game_class, "ENGINE_NAME", game_class.__name__)
    batch = int(batch or train_config.get("num_workers", 1))
    eng = SelfPlayEngine(name, batch, 1, train_config["max_actions"], 0, 0, 0.0, 0.0, 0, evaluator=EVAL_RESNET,
                         net_blocks=build_config["num_resnet_layers"], net_filters=build_config.get("num_filters", 128),
                         ring_capacity=0, device=device, lib_path=lib_path)
    try:
        eng.load_weights(weights)
        shape = game_class().get_input_state().shape
        x = np.random.default_rng(0).integers(-1, 2, size=(batch, *shape)).astype(np.int8)
        _, _, ms = eng.evaluate(x, repeats=iterations)
    finally:
        eng.close()
    out(f"Took {ms / 1e3} seconds per iteration at {1e3 / ms:0.2f} it/s!")
    return 1e3 / ms


def Run(game_class, configs, train_fn=None, weights_fn=None, root="Grok_Zero_Train", n_games=1024, seed=None, device=0,
        lib_path=None, out=print, self_play_kwargs=None, match=None, replay=None, train=None):
    """The loop of <Game>/main.py:312-352: for every generation self-play (resumable), statistics, `train_fn`, next dataset file.
    Returns the list of per-generation statistics.
    `match` = None: nothing else.  match = dict(games=..., n_slots=None, threshold=None[, hash_salt_b=...]): after `train_fn` of a generation
    g >= 1 the new network, weights_fn(folder g + 1), plays self_play.play_match as network A against the network that self-play currently
    uses (the last accepted folder's; weights_fn returning None on both sides = the synthetic evaluator under two salts).  The result goes into
    folder g + 1 as Match.json — `result`, `new_folder`, `old_folder`, `accepted`, `accepted_folder` — and into that generation's statistics
    (`match`).  With a `threshold`, a new network whose score is below it is not accepted: the following generations' self-play keeps the
    last accepted folder's weights.  A resumed Run reads the last accepted folder from the newest Match.json.
    match["book"] (an opening book: a list of action-index sequences or a file, as train_config["opening_book"]) and match["paired"] go
    to play_match: with a book the games are played in colour-swapped pairs from shared openings, and `result` in Match.json carries the
    paired block — `pairs`, `incomplete`, `elo_ci95_paired` — and `book` (the entries' counts).
    `replay` = None: nothing else.  replay = dict(capacity_rows=..., generations=N[, test_fraction=..., target_ratio=..., seed=...]): one
    replay.ReplayWindow lives through the run and holds the rows of the last N generations on the device.  A resumed Run refills it from the
    replay files of the last N generation folders (ReplayWindow.append_file), every generation's run_self_play feeds it (replay=window), and
    `train_fn` is called as train_fn(generation, folder, save_folder, replay=window).
    replay["score"] = dict(batch_rows=...) (absent: nothing else): after `train_fn` of generation g the new network, weights_fn(folder g + 1), and the
    network self-play is using are both scored on the window's test split (replay.score_network: the held-out loss of the engine's own
    evaluator).  Both dicts go into folder g + 1 as Score.json — `new`, `current`, `new_folder`, `current_folder` — and into that generation's
    statistics (`score`).  Nothing is decided from them: acceptance stays with `match`.
    `train` = None: nothing else.  train = dict() (its keys are keywords of train.train_generation, e.g. seed=...): the loop trains by itself —
    where it would call `train_fn` it calls train.train_generation(window, game_class, configs, generation, folder, save_folder), which continues
    from folder/train_state.pt and leaves train_state.pt, weights.npz and Train.json in the next generation's folder (its dict goes into the
    generation's statistics as `train`), and `weights_fn` defaults to train.weights_from_folder.  It needs `replay` and excludes `train_fn`.  A
    resumed Run continues from the last train_state.pt."""
    if train is not None:
        if train_fn is not None:
            raise ValueError("Run: train= and train_fn= exclude each other: train= makes the loop call train.train_generation itself")
        if replay is None:
            raise ValueError("Run: train= needs replay=dict(capacity_rows=..., generations=...): train_generation reads its rows from the replay window")
        if not isinstance(train, dict):
            raise ValueError(f"Run: train must be a dict of train_generation's keywords (an empty one will do), not {type(train).__name__}")
        from . import train as T                                                        # (imports torch before the first library handle of the run)
        T.optimizer_settings(configs)                                                   # refusals (an unknown optimizer, mixed_precision) before anything is played
        if weights_fn is None:
            weights_fn = T.weights_from_folder

        def train_fn(generation, folder, save_folder, replay=None):
            stats[-1]["train"] = T.train_generation(replay, game_class, configs, generation, folder, save_folder, device=device, lib_path=lib_path, out=out, **train)
    train_config = configs[1]
    total = int(train_config["total_generations"])
    gen = current_generation(root)
    if gen == 0 and not ReplayStore(os.path.join(root, "0")).exists():                  # Initialize (<Game>/main.py:255-269)
        make_generation_folder(root, 0)
        make_dataset_file(os.path.join(root, "0"))
    out("\n*************Starting*************\n")
    out(f"Generation: {gen} / {total - 1}")
    if not ReplayStore(os.path.join(root, str(gen))).exists():                          # training of gen-1 finished, file missing
        make_dataset_file(os.path.join(root, str(gen)))
    stats = []
    accepted = None                                                                     # folder whose weights self-play uses; None = the generation's own
    if match is not None:
        for g in range(gen, 0, -1):                                                     # resume: the newest Match.json says which folder was accepted last
            mj = os.path.join(root, str(g), "Match.json")
            if os.path.exists(mj):
                with open(mj) as f:
                    accepted = json.load(f)["accepted_folder"]
                break
    window, keep = None, 0
    if replay is not None:
        from .replay import ReplayWindow
        name = getattr(game_class, "ENGINE_NAME", game_class.__name__)
        keep = max(int(replay.get("generations", 1)), 1)
        window = ReplayWindow(name, replay["capacity_rows"], replay.get("seed", 0 if seed is None else seed), test_fraction=replay.get("test_fraction", 0.1),
                              target_ratio=replay.get("target_ratio", 0.5), device=device, lib_path=lib_path)
        for g in range(max(gen - keep + 1, 0), gen + 1):                                # resume: what the files of the last N generations hold
            if ReplayStore(os.path.join(root, str(g))).exists():
                window.append_file(os.path.join(root, str(g)), g)
    for generation in range(gen, total):
        folder = os.path.join(root, str(generation))
        sp_kw = dict(self_play_kwargs or {})
        if window is not None:
            window.evict(generation - keep + 1)
            sp_kw["replay"] = window
        played_folder = folder if accepted is None else accepted
        weights = weights_fn(played_folder) if (weights_fn and generation > 0) else None
        t0 = time.time()
        played = run_self_play(game_class, configs, folder, n_games=n_games, seed=None if seed is None else seed + generation,
                               weights=weights, device=device, lib_path=lib_path, **sp_kw)
        st = print_stats(folder, out)
        st.update(generation=generation, played_now=played, seconds=time.time() - t0)
        stats.append(st)
        if train_fn is not None:
            make_generation_folder(root, generation + 1)
            if window is not None:
                train_fn(generation, folder, os.path.join(root, str(generation + 1)), replay=window)
            else:
                train_fn(generation, folder, os.path.join(root, str(generation + 1)))
            if window is not None and replay.get("score") is not None:
                from .replay import score_network
                new_folder = os.path.join(root, str(generation + 1))
                skw = dict(batch_rows=int(replay["score"].get("batch_rows", 1024)), device=device, lib_path=lib_path, hash_salt=(self_play_kwargs or {}).get("hash_salt", 0))
                new = score_network(window, game_class, configs, weights_fn(new_folder) if weights_fn else None, **skw)
                cur = score_network(window, game_class, configs, weights, **skw)
                with open(os.path.join(new_folder, "Score.json"), "w") as f:
                    json.dump(dict(new=new, current=cur, new_folder=new_folder, current_folder=played_folder, split="test"), f, indent=1)
                st["score"] = dict(new=new, current=cur)
                out(f"Score: generation {generation + 1} val_loss {new['val_loss']:.4f} (current {cur['val_loss']:.4f}) on {new['rows']} held-out rows")
            if match is not None and generation >= 1:
                new_folder = os.path.join(root, str(generation + 1))
                kw = {k: v for k, v in match.items() if k not in ("games", "n_slots", "threshold")}
                res = play_match(game_class, configs, weights_fn(new_folder) if weights_fn else None, weights, match["games"],
                                 n_slots=match.get("n_slots"), seed=0 if seed is None else seed + generation, device=device, lib_path=lib_path, **kw)
                res.pop("headers", None)
                threshold = match.get("threshold")
                ok = threshold is None or res["score"] >= threshold
                accepted = new_folder if ok else played_folder
                with open(os.path.join(new_folder, "Match.json"), "w") as f:
                    json.dump(dict(result=res, new_folder=new_folder, old_folder=played_folder, accepted=bool(ok), accepted_folder=accepted), f, indent=1)
                st["match"] = dict(res, accepted=bool(ok))
                out(f"Match: generation {generation + 1} scored {res['score']:.3f} against {played_folder} over {res['n']} games: {'accepted' if ok else 'rejected'}")
        if generation < total - 1:
            make_generation_folder(root, generation + 1)
            make_dataset_file(os.path.join(root, str(generation + 1)))
            out(f"Generation: {generation + 1} / {total - 1}")
    out("-----------Training Done!-----------")
    if window is not None:
        window.close()
    return stats

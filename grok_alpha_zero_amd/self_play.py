"""run_self_play — the reference's self-play driver surface on top of the MI355X engine.

Mirrors `run_self_play(game_class, configs, folder_path, per_process_wait_time)` (Self_Play.py:259-413) and what
`Self_Play.play()` appends to the replay file (Self_Play.py:159-208): per finished game and per augmentation k,
datasets `boards_k` (board dtype), `policies_k` (f32), `values_k` (f32) with `values = 0.5 * (z + q)`, and the
`game_stats` u32[6] counters [max_len, total_actions, n_games, wins(-1), draws, wins(+1)].

Instead of N worker processes + a shared-memory inference server (Self_Play.py:334-400, Client_Server.py) all games run
concurrently on the GPU; `num_workers` therefore only bounds nothing here — the concurrency is `n_games`.

Storage: the reference writes HDF5 through h5py.  h5py is not installed in this image, so `ReplayStore` uses h5py when it is
importable and otherwise the system libhdf5 through h5io.py (ctypes) — a real `Self_Play_Data.h5` with the same dataset
names / dtypes / shapes / libver either way.
"""
import logging
import math
import os
import queue
import threading
import time

import numpy as np

from .engine import EVAL_HASH, EVAL_RESNET, SEARCH_GUMBEL, SEARCH_PUCT, SelfPlayEngine


class ReplayStore:
    """`Self_Play_Data.h5`: game_stats + boards_k / policies_k / values_k (Self_Play.py:178-208).  Backend: h5py when installed,
    else libhdf5 through h5io.py (a real HDF5 file either way), else — no HDF5 library at all — an .npy directory."""

    def __init__(self, folder_path):
        self.folder = folder_path
        try:
            import h5py  # noqa: F401
            self.backend = "h5py"
        except ImportError:
            from . import h5io
            self.backend = "libhdf5" if h5io.available() else "npy"
        self.path = os.path.join(folder_path, "Self_Play_Data.h5" if self.backend != "npy" else "Self_Play_Data.npzdir")
        self._buf, self._buf_bytes, self._in_session = [], 0, False

    def _open(self, mode):
        if self.backend == "h5py":
            import h5py
            return _H5pyAdapter(h5py.File(self.path, mode, libver="latest"))
        from .h5io import H5File
        return H5File(self.path, mode)

    def exists(self):
        return os.path.exists(self.path)

    def create(self):
        os.makedirs(self.folder, exist_ok=True)
        if self.backend == "npy":
            os.makedirs(self.path, exist_ok=True)
            np.save(os.path.join(self.path, "game_stats.npy"), np.zeros(6, np.uint32))
            return
        with self._open("w") as f:                                    # <Game>/main.py:83-86
            f.create_dataset("game_stats", np.zeros(6, np.uint32), maxshape=(6,), dtype=np.uint32)

    def game_stats(self):
        return self.read("game_stats")

    def n_datasets(self):
        if self.backend == "npy":
            return len([n for n in os.listdir(self.path) if n != "game_stats.npy"])
        with self._open_read() as f:
            return f.n_links() - 1

    # A generation appends thousands of games.  Opening the file and counting its datasets per game made the writer, not the GPU,
    # the limit (0.3 s per game, growing with the file); holding one handle open for the whole generation (round 1) left the
    # superblock's write flag set when the process was killed, and the file could not be reopened.  So `writing()` BUFFERS games and
    # writes them in batches — open, append `flush_every` games, close: the file is open for write only for the milliseconds of a
    # batch (the reference's exposure is one game's write, Self_Play.py:178-208), and a killed run keeps every batch it completed.
    def recover(self):
        """Repair a file that a KILLED writer left "open for write" (libhdf5 then refuses every open): clear the superblock's status flags, what
        `h5clear -s` does.  Only for the generation's single writer (run_self_play calls it before it reads the counters); a reader never
        repairs — the flag is also what a LIVE writer's open file looks like.  Returns True if a repair was made; any other reason for the
        file not opening is raised as it is."""
        if self.backend != "libhdf5" or not os.path.exists(self.path):
            return False
        try:
            self._open("r").close()
            return False
        except OSError as first:
            from .h5io import H5File, superblock_status_flags
            flags = superblock_status_flags(self.path)
            if not flags:                                             # not the interrupted-writer case: permissions, truncation, not HDF5 ...
                raise
            f = H5File(self.path, "r+", clear_status_flags=True)
            try:
                ok = f.n_links() >= 1 and f.read("game_stats").shape == (6,)      # must still be readable, else beyond this repair
            finally:
                f.close()
            if not ok:
                raise OSError(f"{self.path}: left inconsistent by an interrupted writer") from first
            logging.getLogger("grok_alpha_zero_amd").warning("%s was left open (status flags %#x) by an interrupted writer; flags cleared", self.path, flags)
            return True

    def _open_read(self):
        try:
            return self._open("r")
        except OSError as e:
            if self.backend == "libhdf5":
                from .h5io import superblock_status_flags
                if superblock_status_flags(self.path):
                    raise OSError(f"{self.path} is marked open for write: a writer is running, or one was killed — in that case the generation's "
                                  "writer repairs it (ReplayStore.recover(), which run_self_play calls); readers do not") from e
            raise

    def _open_rw(self):
        """the single writer's open: repairs after a killed predecessor"""
        try:
            return self._open("r+")
        except OSError:
            if not self.recover():
                raise
            return self._open("r+")

    def writing(self, flush_every=64, flush_bytes=64 << 20):
        store = self

        class _Session:
            def __enter__(self_inner):
                store._buf, store._buf_bytes = [], 0
                store._flush_every, store._flush_bytes, store._in_session = flush_every, flush_bytes, True
                return store

            def __exit__(self_inner, *a):
                try:
                    store._flush()
                finally:
                    store._in_session = False
                return False
        return _Session()

    def _flush(self):
        """append the buffered games / dataset triples / stats in ONE open-write-close"""
        buf, self._buf, self._buf_bytes = self._buf, [], 0
        if not buf:
            return
        if self.backend == "npy":
            for item in buf:
                self._write_npy(item)
            return
        f = self._open_rw()
        try:
            stats = f.read("game_stats").astype(np.uint32)
            k = (f.n_links() - 1) // 3                                # dataset_name = (len(keys) - 1) // 3 (Self_Play.py:190)
            if (f.n_links() - 1) % 3:                                 # a writer died inside a triple: drop its incomplete tail
                for nm in (f"boards_{k}", f"policies_{k}", f"values_{k}"):
                    if f.exists(nm):
                        f.delete(nm)
            for kind, payload in buf:
                if kind == "stats":
                    stats = payload.copy()
                    f.write("game_stats", stats)
                    continue
                if kind == "game":
                    boards_aug, policies_aug, values_aug, game_length, n_positions, winner = payload
                    stats[0] = max(int(stats[0]), game_length); stats[1] += n_positions; stats[2] += 1; stats[winner + 4] += 1
                    # the counters BEFORE the game's datasets, as the reference does (Self_Play.py:181-188 precede :190-208): a writer killed
                    # inside a batch then never leaves games in the file that game_stats[2] does not count — run_self_play resumes from that
                    # count (games_left, first_game_seq), and an under-count would replay the (slot, game_seq) streams of the uncounted games
                    f.write("game_stats", stats)
                    triples = [(boards_aug[i], policies_aug[i], values_aug[i]) for i in range(policies_aug.shape[0])]
                else:
                    triples = [payload]
                for b, p, v in triples:
                    f.create_dataset(f"boards_{k}", b, maxshape=(None, *b.shape[1:]), dtype=b.dtype)
                    f.create_dataset(f"policies_{k}", p, maxshape=(None, *p.shape[1:]), dtype=np.float32)
                    f.create_dataset(f"values_{k}", v, maxshape=(None, *v.shape[1:]), dtype=np.float32)
                    k += 1
        finally:
            f.close()

    def _write_npy(self, item):
        kind, payload = item
        if kind == "stats":
            np.save(os.path.join(self.path, "game_stats.npy"), payload)
            return
        k = self.n_datasets() // 3
        if kind == "game":
            boards_aug, policies_aug, values_aug, game_length, n_positions, winner = payload
            stats = self.game_stats().astype(np.uint32)
            stats[0] = max(int(stats[0]), game_length); stats[1] += n_positions; stats[2] += 1; stats[winner + 4] += 1
            np.save(os.path.join(self.path, "game_stats.npy"), stats)
            triples = [(boards_aug[i], policies_aug[i], values_aug[i]) for i in range(policies_aug.shape[0])]
        else:
            triples = [payload]
        for b, p, v in triples:
            np.save(os.path.join(self.path, f"boards_{k}.npy"), b)
            np.save(os.path.join(self.path, f"policies_{k}.npy"), np.asarray(p, np.float32))
            np.save(os.path.join(self.path, f"values_{k}.npy"), np.asarray(v, np.float32))
            k += 1

    def _put(self, item, nbytes):
        if not getattr(self, "_in_session", False):
            with self.writing():
                return self._put(item, nbytes)
        self._buf.append(item); self._buf_bytes += nbytes
        n_games = sum(1 for kind, _ in self._buf if kind != "stats")
        if n_games >= self._flush_every or self._buf_bytes >= self._flush_bytes:
            self._flush()

    def append_game(self, boards_aug, policies_aug, values_aug, game_length, n_positions, winner):
        """One finished game: arrays [n_aug, T, ...] (Self_Play.py:174-208)."""
        boards_aug = np.ascontiguousarray(boards_aug); policies_aug = np.ascontiguousarray(policies_aug, np.float32)
        values_aug = np.ascontiguousarray(values_aug, np.float32)
        self._put(("game", (boards_aug, policies_aug, values_aug, int(game_length), int(n_positions), int(winner))),
                  boards_aug.nbytes + policies_aug.nbytes + values_aug.nbytes)

    def append_datasets(self, boards, policies, values):
        """one (boards_k, policies_k, values_k) triple as the next k, without touching game_stats (shard merge, parallel.py)"""
        boards = np.ascontiguousarray(boards); policies = np.ascontiguousarray(policies, np.float32); values = np.ascontiguousarray(values, np.float32)
        self._put(("triple", (boards, policies, values)), boards.nbytes + policies.nbytes + values.nbytes)

    def set_game_stats(self, stats):
        self._put(("stats", np.asarray(stats).astype(np.uint32)), 24)

    def read(self, name):
        if self.backend == "npy":
            return np.load(os.path.join(self.path, name + ".npy"))
        with self._open_read() as f:
            return f.read(name)


class _H5pyAdapter:
    """h5py.File behind the four calls ReplayStore uses."""

    def __init__(self, f):
        self.f = f

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.f.close()
        return False

    def keys(self):
        return list(self.f.keys())

    def n_links(self):
        return len(self.f)

    def flush(self):
        self.f.flush()

    def exists(self, name):
        return name in self.f

    def delete(self, name):
        del self.f[name]

    def close(self):
        self.f.close()

    def create_dataset(self, name, data, maxshape=None, dtype=None):
        self.f.create_dataset(name, maxshape=maxshape, dtype=dtype, data=data, chunks=None)

    def write(self, name, data):
        self.f[name][...] = data

    def read(self, name):
        return np.array(self.f[name])


def _fast_states(name, actions):
    """Input states of every ply of one game for the built-in plugins (games.py), without a Python call per ply: [T, H, W, C]
    int8, equal to stacking game.get_input_state() before each move (checked against the plugin path in the tests)."""
    T = len(actions)
    if name == "Connect4":
        boards = np.zeros((T + 1, 6, 7), np.int8)                     # boards[t] = position before move t
        heights = [0] * 7
        player = -1
        for t, a in enumerate(actions):
            a = int(a)
            boards[t + 1] = boards[t]
            boards[t + 1, 5 - heights[a], a] = player
            heights[a] += 1; player = -player
        st = np.zeros((T, 6, 7, 4), np.int8)
        st[..., 3] = boards[:T]
        if T > 2: st[2:, :, :, 2] = boards[1:T - 1]                   # one move back, once two moves were played
        if T > 3: st[3:, :, :, 1] = boards[1:T - 2]
        cur = np.where(np.arange(T) % 2 == 0, 1, -1).astype(np.int8)  # -next_player: the first mover is -1
        st[..., 0] = cur[:, None, None]
        if T > 4: st[4:, :, :, 0] = boards[1:T - 3]                   # >= 4 moves: the board three moves back (Connect4.py:340-345)
        return st
    W = 3 if name == "TicTacToe" else 15
    boards = np.zeros((T + 1, W, W), np.int8)
    player = -1
    for t, a in enumerate(actions):
        a = int(a)
        boards[t + 1] = boards[t]
        boards[t + 1, a // W, a % W] = player
        player = -player
    st = np.empty((T, W, W, 2), np.int8)
    st[..., 1] = boards[:T]
    st[..., 0] = np.where(np.arange(T) % 2 == 0, -1, 1).astype(np.int8)[:, None, None]   # -current_player = next_player... see games.py:118
    return st


SURPRISE_EVENT = 0x40000000                        # the event of ply p's rounding variate is SURPRISE_EVENT + p (csrc/samples.hpp)


def sample_row_counts(rec, lam, fast_factor, seed):
    """Policy surprise weighting (SelfPlayEngine.set_sample_weighting; include/gaz_engine.h states the rule, steps 1-5): the rows every ply
    of one finished PUCT record gives -> int array [T].  The prior of a ply is rec["root_P"], the priors its root searched with (Dirichlet
    noise included).  Every sum is a sequential float64 sum, in action / ply order, as the kernel's."""
    from . import det
    lam, fast_factor = float(lam), float(fast_factor)
    kind = [int(k) & 3 for k in rec["move_kind"]]
    T = len(kind)
    s = [0.0] * T
    for p in range(T):
        if kind[p] in (0, 3):                        # no search ran there: a set_position prefix, an opening-book prefix
            continue
        acc = 0.0
        for x, y in zip(rec["policies"][p], rec["root_P"][p]):
            if x > 0 and y > 0:
                acc = acc + float(x) * (det.dlog(float(x)) - det.dlog(float(y)))
        s[p] = acc if math.isfinite(acc) and acc > 0.0 else 0.0
    full = [p for p in range(T) if kind[p] == 1]
    n_full = len(full)
    total = 0.0
    for p in full:
        total = total + s[p]
    cut = fast_factor * (total / n_full) if n_full else 0.0
    in_E = [kind[p] == 1 or (kind[p] == 2 and s[p] > cut) for p in range(T)]
    S = 0.0
    for p in range(T):
        if in_E[p]:
            S = S + s[p]
    plain = n_full == 0 or not S > 0.0 or not math.isfinite(S) or lam == 0.0
    counts = np.zeros(T, np.int64)
    for p in range(T):
        if kind[p] == 0:
            counts[p] = 1
            continue
        if kind[p] == 3:                             # a book ply gives no row and takes no part
            continue
        w0 = 1.0 if kind[p] == 1 else 0.0
        w = w0 if plain else ((1.0 - lam) * w0 + lam * n_full * s[p] / S if in_E[p] else 0.0)
        fl = math.floor(w)
        u = det.uniform(int(seed), int(rec["slot"]), int(rec["game_seq"]), 2, SURPRISE_EVENT + p, det.P_PLAYOUT_CAP)
        counts[p] = int(fl) + (1 if u < w - fl else 0)
    return counts


def record_to_samples(game_class, rec, weighting=None):
    """Rebuild what Self_Play.play() collected for one finished game (Self_Play.py:80,114-127,159-175): input states by
    replaying the moves through the Game plugin, improved policies, values = 0.5 (z + q), then augment_sample.  Plies whose search was
    a fast one (rec["move_kind"] == 2, playout cap randomisation) give no row, nor do the plies of an opening-book prefix (move_kind 3,
    SelfPlayEngine.set_opening_book); the length returned stays the plies played.  With forced
    playouts (forced_playouts_k > 0) rec["policies"] already holds the pruned targets: nothing is recomputed here.
    weighting = (lambda, fast_factor, seed) — seed the engine's — applies policy surprise weighting: ply p gives sample_row_counts()[p]
    adjacent copies of the row it has with the cap off; lambda = 0 or None is the plain rule above."""
    game = game_class()
    from . import games as _builtin
    if game_class in (_builtin.Connect4, _builtin.Gomoku, _builtin.TicTacToe):
        board_states = _fast_states(game_class.ENGINE_NAME, rec["actions"])
        n_plies = len(rec["actions"])
    else:
        states = []
        for idx in rec["actions"]:
            states.append(np.array(game.get_input_state()).copy())
            game.do_action(game_class.index_to_action(int(idx)) if hasattr(game_class, "index_to_action") else idx)
        board_states = np.array(states, dtype=game.board.dtype)
        n_plies = len(game.action_history)
    policies = np.asarray(rec["policies"], np.float32)
    values = np.asarray(rec["values"], np.float32).reshape(-1, 1)
    kind = rec.get("move_kind")
    if weighting is not None and float(weighting[0]) != 0.0:
        rows = np.repeat(np.arange(len(values)), sample_row_counts(rec, *weighting))
        if rows.size == 0 and len(values):           # every count rounded to 0: arrays of no rows, shaped by the augmentations of one row
            aug_b, aug_p = (np.asarray(a) for a in game.augment_sample(board_states[:1], policies[:1]))
            return aug_b[:, :0], aug_p[:, :0], np.zeros((aug_p.shape[0], 0, 1), np.float32), n_plies
        board_states, policies, values = board_states[rows], policies[rows], values[rows]
    elif kind is not None and np.any(np.asarray(kind) >= 2):     # fast plies (2) and the plies of an opening-book prefix (3)
        keep = np.asarray(kind) < 2
        board_states, policies, values = board_states[keep], policies[keep], values[keep]
    aug_b, aug_p = game.augment_sample(board_states, policies)
    aug_b, aug_p = np.asarray(aug_b), np.asarray(aug_p)
    aug_v = np.repeat(values[None], aug_p.shape[0], axis=0)
    return aug_b, aug_p, aug_v, n_plies


def resign_trigger_plies(q, move_kind, threshold, consecutive=1, min_ply=0):
    """The plies of one game at which the resign rule of SelfPlayEngine.set_resignation triggers, from the record's q and move_kind:
    ply p < T - 1 (the game went on after it) with p >= min_ply, p >= 2 (consecutive - 1) and, for i in 0 .. consecutive-1, ply p - 2i
    searched (move_kind 1 or 2) and q[p - 2i] < -threshold (the float32 widened to double, strict).  A ply of an opening-book prefix
    (move_kind 3) breaks a run as move_kind 0 does: no search ran there, and its recorded q is 0."""
    T = len(q)
    out = []
    for p in range(max(int(min_ply), 2 * (int(consecutive) - 1)), T - 1):
        if all((int(move_kind[p - 2 * i]) & 3) in (1, 2) and float(q[p - 2 * i]) < -float(threshold) for i in range(int(consecutive))):
            out.append(p)
    return out


def resign_curve(records, thresholds, consecutive=1, min_ply=0):
    """What resignation would have done to games that were played out (records of SelfPlayEngine.drain_finished(), e.g. a generation
    with no_resign_prob = 1), per threshold: a list of dicts with `threshold`, `games`, `would_resign` (games in which the rule
    triggers), `false_positives` (of those, games the player who would have resigned first went on to draw or win), `plies_saved`
    (plies after the first trigger, summed) and `plies` (all plies played).  The threshold to use is the lowest one whose
    false_positives / would_resign is acceptable (AlphaGo Zero: under 5 %)."""
    rows = []
    for thr in thresholds:
        would = false_pos = saved = plies = 0
        for r in records:
            plies += int(r["T"])
            hit = resign_trigger_plies(r["q"], r["move_kind"], thr, consecutive, min_ply)
            if not hit:
                continue
            f = hit[0]
            would += 1
            saved += int(r["T"]) - (f + 1)
            resigner = 1 if f % 2 else -1            # the mover of ply f: -1 moves first
            false_pos += int(r["winner"]) != -resigner
        rows.append(dict(threshold=float(thr), games=len(records), would_resign=would, false_positives=false_pos, plies_saved=saved, plies=plies))
    return rows


# ------------------------------------------------------------------------------------------------ opening book
BOOK_TREE = 3                                      # the stream of the book's draw (csrc/det.hpp: trees 0 / 1 / 2 are the searches')


def book_entry(seed, slot, game_seq, n_entries, mode="game"):
    """The entry of an n_entries book that game (slot, game_seq) starts from (SelfPlayEngine.set_opening_book; include/gaz_engine.h states
    the rule): idx = min(int(u * n_entries), n_entries - 1), u the uniform variate of (seed, slot, key_seq, tree 3, event 0, P_OPENING),
    key_seq = game_seq in mode "game" and game_seq & ~1 in mode "pair".  slot is the GLOBAL slot, as in the record header."""
    from . import det
    if mode not in ("game", "pair"):
        raise ValueError(f"book_entry: mode must be 'game' or 'pair', not {mode!r}")
    if n_entries <= 0:
        raise ValueError("book_entry: the book has no entries")
    seq = int(game_seq) & 0xFFFFFFFF
    u = det.uniform(int(seed), int(slot), seq & ~1 if mode == "pair" else seq, BOOK_TREE, 0, det.P_OPENING)
    return min(int(u * n_entries), n_entries - 1)


def book_from_records(records, plies, min_count=1):
    """The distinct `plies`-long prefixes of finished games (drain_finished's dicts, or action sequences) that occur at least `min_count`
    times, most frequent first (ties: in action order) -> list of lists of action indices.  Games of `plies` plies or fewer are left out:
    their prefix is a finished game, which no book may hold."""
    seen = {}
    for r in records:
        a = [int(x) for x in (r["actions"] if isinstance(r, dict) else r)]
        if len(a) > plies:
            key = tuple(a[:plies])
            seen[key] = seen.get(key, 0) + 1
    return [list(k) for k, c in sorted(seen.items(), key=lambda kc: (-kc[1], kc[0])) if c >= min_count]


def enumerate_openings(game_class, plies):
    """Every legal unfinished position `plies` moves from the empty board, through the Game API (get_legal_actions, do_action, check_win),
    as action-index sequences in depth-first order of the legal actions.  Different sequences that reach the same position are all listed
    (a position's history is part of the network's input)."""
    to_index = game_class.action_to_index if hasattr(game_class, "action_to_index") else int
    to_action = game_class.index_to_action if hasattr(game_class, "index_to_action") else (lambda i: i)
    out = []

    def walk(seq):
        game = game_class()
        for i in seq:
            game.do_action(to_action(i))
        if seq and game.check_win() != -2:
            return
        if len(seq) == plies:
            out.append(list(seq))
            return
        for a in game.get_legal_actions():
            walk(seq + [int(to_index(a))])
    walk([])
    return out


def save_book(path, entries):
    """a book as the file run_self_play's train_config["opening_book"] names: .json (a list of lists) or .npy (int16 [n, stride], rows
    padded with -1)"""
    entries = [[int(a) for a in e] for e in entries]
    if str(path).endswith(".json"):
        import json
        with open(path, "w") as f:
            json.dump(entries, f)
        return
    if not str(path).endswith(".npy"):
        raise ValueError("save_book: the path must end in .json or .npy")
    arr = np.full((len(entries), max([1] + [len(e) for e in entries])), -1, np.int16)
    for i, e in enumerate(entries):
        arr[i, :len(e)] = e
    np.save(path, arr)


def load_book(book):
    """train_config["opening_book"] -> list of lists of action indices: a list as it is, or the .json / .npy file save_book writes"""
    if isinstance(book, (str, os.PathLike)):
        if str(book).endswith(".json"):
            import json
            with open(book) as f:
                book = json.load(f)
        elif str(book).endswith(".npy"):
            book = [[int(a) for a in row if a >= 0] for row in np.load(book)]
        else:
            raise ValueError(f"opening_book: {book} is neither a .json nor a .npy file")
    return [[int(a) for a in e] for e in book]


def _book_mode(mode):
    if mode in (None, "game", "pair"):
        return mode
    raise ValueError(f"opening_book_mode must be 'game' or 'pair', not {mode!r}")


class _ReplayWriter:
    """The generation's writer thread: the only user of the ReplayStore while it lives, inside one `writing()` session.  The loop that
    queues the waves hands it work with put(); work is a SampleBatch (every game of it is appended, in order) or one game's
    append_game arguments.  The queue is bounded in BYTES: put() blocks while more than `max_pending_bytes` wait, which is the
    back-pressure that keeps host memory finite when the file is slower than the GPU (one item is always admitted).  An exception
    of the writer is re-raised by the next put() or by close(); close() lets the writer finish what is queued and joins it."""

    def __init__(self, store, max_pending_bytes):
        self.store, self.max_bytes = store, max(int(max_pending_bytes), 1)
        self.q, self.cv, self.pending, self.error = queue.Queue(), threading.Condition(), 0, None
        self.write_seconds = self.wait_seconds = 0.0
        self.thread = threading.Thread(target=self._run, name="gaz-replay-writer", daemon=True)
        self.thread.start()

    def _run(self):
        try:
            with self.store.writing():
                while True:
                    item = self.q.get()
                    if item is None:
                        break
                    work, nbytes = item
                    t0 = time.perf_counter()
                    try:
                        if self.error is None:              # after a failure: only release the queue
                            if isinstance(work, tuple):
                                self.store.append_game(*work)
                            else:
                                for i in range(work.n):
                                    self.store.append_game(*work.game(i))
                    except BaseException as e:              # noqa: BLE001 — handed to the caller
                        self.error = e
                    finally:
                        self.write_seconds += time.perf_counter() - t0
                        with self.cv:
                            self.pending -= nbytes
                            self.cv.notify_all()
                t0 = time.perf_counter()                    # (the session's last flush happens on leaving the with block)
            self.write_seconds += time.perf_counter() - t0
        except BaseException as e:                          # noqa: BLE001
            if self.error is None:
                self.error = e
            with self.cv:
                self.pending = 0
                self.cv.notify_all()

    def put(self, work, nbytes):
        t0 = time.perf_counter()
        with self.cv:
            while self.pending > 0 and self.pending + nbytes > self.max_bytes and self.error is None and self.thread.is_alive():
                self.cv.wait(0.5)
            self.pending += nbytes
        self.wait_seconds += time.perf_counter() - t0
        if self.error is not None:
            raise self.error
        self.q.put((work, nbytes))

    def close(self, reraise=True):
        self.q.put(None)
        self.thread.join()
        if reraise and self.error is not None:
            raise self.error


def engine_search_settings(game_class, configs):
    """What train_config / build_config say about the search, as SelfPlayEngine takes it -> ((run_iterations, max_actions,
    num_explore_actions_first, num_explore_actions_second, c_puct_init, dirichlet_alpha), keywords): the settings run_self_play and
    play_match share."""
    build_config, train_config = configs[0], configs[1]
    gumbel = bool(train_config.get("use_gumbel"))
    # PUCT runs int(1.5 * limit) iterations per move (Self_Play.py:99), Gumbel runs `limit` (Self_Play.py:110-112)
    iters = int(train_config["MCTS_iteration_limit"]) if gumbel else int(train_config["MCTS_iteration_limit"] * 1.5)
    fast = int(train_config.get("MCTS_fast_iteration_limit") or 0)
    fast = fast if gumbel else int(fast * 1.5)
    args = (iters, train_config["max_actions"], train_config.get("num_explore_actions_first", 0), train_config.get("num_explore_actions_second", 0),
            train_config.get("c_puct_init", 0.0), train_config.get("dirichlet_alpha", 0.0))
    kw = dict(search=SEARCH_GUMBEL if gumbel else SEARCH_PUCT, gumbel_m=train_config.get("m", 0),
              c_visit=train_config.get("c_visit", 50.0), c_scale=train_config.get("c_scale", 1.0),
              # policy head: raw logits for Gumbel, else Stablemax or softmax (Build_Model.py:54-60)
              policy_is_logits=1 if gumbel else (2 if build_config.get("use_stablemax") else 0),
              gumbel_stablemax=bool(gumbel and build_config.get("use_stablemax")),
              opening_actions=[(game_class.action_to_index(a) if hasattr(game_class, "action_to_index") else int(a), w)
                               for a, w in train_config.get("opening_actions", []) or []],
              create_new_root=train_config.get("create_new_root", False),
              # Self_Play.py:35,100-112: every MCTS.run gets time_limit = MCTS_time_limit next to its iteration limit; the engine keeps a
              # wall clock per game and move (PUCT) / runs 3 x legal moves iterations per move (Gumbel, MCTS_Gumbel.py:576-578)
              move_time_limit=float(train_config.get("MCTS_time_limit") or 0.0),
              fast_iterations=fast, full_search_prob=float(train_config.get("full_search_prob") or 0.0) if fast else 0.0,
              forced_playouts_k=float(train_config.get("forced_playouts_k") or 0.0),
              resign_threshold=float(train_config.get("resign_threshold") or 0.0), resign_consecutive=int(train_config.get("resign_consecutive") or 1),
              resign_min_ply=int(train_config.get("resign_min_ply") or 0), no_resign_prob=float(train_config.get("no_resign_prob") or 0.0),
              # policy surprise weighting of the training rows (SelfPlayEngine.set_sample_weighting; absent or 0 = off, and then no call is made)
              sample_weighting=(float(train_config.get("policy_surprise_weight") or 0.0), float(train_config.get("policy_surprise_fast_factor") or 1.5)))
    return args, kw


def run_self_play(game_class, configs, folder_path, per_process_wait_time=1e-3, *, n_games=1024, seed=None, weights=None,
                  device=0, slot_offset=0, hash_salt=0, lib_path=None, progress=None, eval_cache_log2=22, generation=None,
                  first_game_seq=None, allow_synthetic=False, engine_stats=None, game_groups=0, device_samples=None,
                  max_pending_bytes=1 << 30, leaf_batch=1, gumbel_batch=1, replay=None):
    """Generate `games_per_generation - game_stats[2]` self-play games into `folder_path` (Self_Play.py:259-272).
    (`engine_stats`: a dict that receives the engine's counters — evaluator calls, simulations, waves — when the generation is done,
    and the host's timers: `gpu_wait_seconds` / `sample_seconds` / `queue_wait_seconds` of the thread that queues the waves (waiting for
    the launches; obtaining the samples of finished games; blocked by the writer's full queue) and `writer_seconds` of the writer thread.
    `device_samples`: finished games leave the device as training samples (SelfPlayEngine.drain_samples: the states, augmentations and
    values are built by a kernel, one call per drain) instead of as records that record_to_samples converts game by game.  None = on
    for the three built-in plugins of games.py, off for any other plugin class — its own get_input_state / augment_sample have to run;
    False = the host path; True with a foreign plugin is a ValueError.  The file is the same byte for byte.  Either way the file is
    written by a thread of its own, fed through a queue of at most `max_pending_bytes` of samples.
    `game_groups`: gaz_engine_config.game_groups, scheduling only: 0 = the library's choice, 1 = one batch.
    `leaf_batch`: gaz_engine_config.leaf_batch; above 1 (PUCT only) every game keeps up to that many leaves in flight per wave — a
    different search, for generations of few games; the evaluation cache and the repack of generation tails are off then.
    `gumbel_batch`: gaz_engine_config.gumbel_batch; above 1 (use_gumbel only) every game keeps up to that many candidates of a halving
    phase in flight per wave — the same games byte for byte in fewer launches, for generations of few games; the evaluation cache
    and the repack of generation tails are off then.)
    Playout cap randomisation: train_config["MCTS_fast_iteration_limit"] (absent or 0 = off) and train_config["full_search_prob"] — a
    move is searched at the full limit with that probability (the first move of a game always), else at the fast limit, scaled like
    the full one (int(1.5 x) for PUCT); only fully searched plies are written as samples, game_stats count every ply played.
    Forced playouts and policy target pruning: train_config["forced_playouts_k"] (absent or 0 = off; KataGo uses 2; PUCT only) — every
    visited root child of a full move gets at least sqrt(k * prior * root visits) visits, and the policy written is the pruned target.
    Resignation: train_config["resign_threshold"] (absent or 0 = off), ["resign_consecutive"] (default 1), ["resign_min_ply"] (default 0)
    and ["no_resign_prob"] (default 0) — SelfPlayEngine.set_resignation: a game is resigned after a ply when the recorded q of its
    mover's last `resign_consecutive` searched plies were all below -resign_threshold; with probability no_resign_prob a game is played
    out instead and its would-be resign plies are marked.  The file format does not change: a resigned game has fewer rows, its winner
    is the player who did not resign, and game_stats count it like any other game.  `engine_stats["resign"]` receives
    SelfPlayEngine.resign_stats() (the false positives among the games played out); resign_curve() picks a threshold from the records
    of a generation played with no_resign_prob = 1.
    Policy surprise weighting: train_config["policy_surprise_weight"] (lambda in [0, 1]; absent or 0 = off; KataGo uses 0.5; PUCT only) and
    ["policy_surprise_fast_factor"] (default 1.5) — SelfPlayEngine.set_sample_weighting: a game's rows are redistributed towards the plies whose
    search policy differs most from the prior, and fast plies that surprise enough earn rows too.  The replay file just gets the rows;
    game_stats are unchanged.
    Solver: train_config["solver"] (absent or False = off, and then no call is made) — SelfPlayEngine.set_solver: the PUCT search proves
    wins, draws and losses; proven plies end early, and their value targets use the exact q.  PUCT with leaf_batch 1 only (else an EngineError).
    Random evaluation symmetry: train_config["eval_symmetry"] (absent or False = off, and then no call is made) —
    SelfPlayEngine.set_eval_symmetry: the network sees every search position under a board symmetry drawn per game and position, and the
    search uses the policy mapped back.  Records and samples stay in the board's own frame; the file format does not change.
    Opening book: train_config["opening_book"] (absent = none) — a list of action-index sequences, or the path of a .json / .npy file that
    save_book writes from book_from_records / enumerate_openings — and ["opening_book_mode"] ("game", the default, or "pair") —
    SelfPlayEngine.set_opening_book: every game starts from the entry that book_entry(seed, slot, game_seq, ...) names; an empty entry is the
    empty board.  The prefix plies give no rows; game_stats count every ply of a game, the prefix included.
    `replay`: a replay.ReplayWindow that receives every drained batch as well (ReplayWindow.append(generation, batch)), in the order the
    writer gets them — the window then holds what the file holds, un-augmented, on the device.  `device_samples` path only (a ValueError
    otherwise); the file is byte for byte what it is without the argument.
    `configs` = (build_config, train_config[, optimizer_config]).  `weights` = dict from net.export_engine_weights()
    (generation > 0); generation 0 (folder name "0") plays with the synthetic evaluator like the reference's
    session=None dummy (Self_Play.py:40, MCTS.py:237-241).

    Which games: the reference starts exactly the missing games and runs every one of them to its end (Self_Play.py:346-408).
    The engine restarts slots on device, so the admitted set is fixed up front the same way: slot g plays its k-th game iff
    k * G + g < games_left (`games_budget`), then halts; every admitted game is written, whatever order they finish in.  (Keeping
    the first games to FINISH instead would favour short games.)  RNG streams are keyed by (seed, slot, game_seq) and game_seq
    starts at `first_game_seq` (default: the games already in the file), so a resumed generation never replays a game even
    with the same seed."""
    build_config, train_config = configs[0], configs[1]
    from . import games as _builtin
    builtin = game_class in (_builtin.Connect4, _builtin.Gomoku, _builtin.TicTacToe)     # (the test record_to_samples makes)
    if device_samples and not builtin:
        raise ValueError(f"device_samples=True: {game_class.__name__} is not one of the built-in plugins; its own augment_sample has to run on the host")
    device_samples = builtin if device_samples is None else bool(device_samples)
    if replay is not None and not device_samples:
        raise ValueError("replay=: the window is fed from the device-built samples; it needs device_samples=True (a built-in plugin)")
    store = ReplayStore(folder_path)
    if not store.exists():
        raise ValueError("Dataset file hasn't been created. Self play depends on that file!")     # Self_Play.py:264-265
    store.recover()                                 # this process is the generation's single writer: repair what a killed predecessor left
    games_done = int(store.game_stats()[2])
    games_left = int(train_config["games_per_generation"] - games_done)
    if games_left <= 0:
        return 0
    if generation is None:
        generation = int(str(folder_path).rstrip("/").split("/")[-1])                 # Self_Play.py:274
    name = getattr(game_class, "ENGINE_NAME", game_class.__name__)
    if generation > 0 and weights is None and not allow_synthetic:
        # the reference would fail loading model.onnx here; silently writing hash-evaluator games as training data is worse
        raise ValueError(f"generation {generation} needs network weights (weights=net.export_engine_weights()); "
                         "pass allow_synthetic=True to play with the synthetic evaluator on purpose")
    use_net = generation > 0 and weights is not None
    if use_net:                                     # width and weights against build_config, before any engine exists
        from .net import check_engine_weights
        check_engine_weights(name, build_config.get("num_resnet_layers", 0), build_config.get("num_filters", 128), weights)
    G = min(n_games, games_left)
    if seed is None:
        seed = int.from_bytes(os.urandom(8), "little")                 # np.random.seed() from OS entropy (Self_Play.py:221)
    if first_game_seq is None:
        first_game_seq = games_done
    gumbel = bool(train_config.get("use_gumbel"))
    args, search_kw = engine_search_settings(game_class, configs)
    eng = SelfPlayEngine(name, G, *args, seed, slot_offset=slot_offset, device=device,
                         evaluator=EVAL_RESNET if use_net else EVAL_HASH, hash_salt=hash_salt,
                         net_blocks=build_config.get("num_resnet_layers", 0) if use_net else 0,
                         net_filters=build_config.get("num_filters", 128), ring_capacity=max(4 * G, 64), lib_path=lib_path,
                         eval_cache_log2=0 if leaf_batch > 1 or gumbel_batch > 1 else eval_cache_log2,    # on-device Session_Cache (Self_Play.py:234-236): same games, fewer waves
                         games_budget=games_left, first_game_seq=first_game_seq, game_groups=game_groups,
                         leaf_batch=leaf_batch, gumbel_batch=gumbel_batch, **search_kw)
    if train_config.get("MCTS_time_limit") and gumbel:
        logging.getLogger("grok_alpha_zero_amd").warning("Time limit isn't allowed for gumbel MCTS defaulting to use 3 * len_legal_actions")   # MCTS_Gumbel.py:578
    logging.getLogger("grok_alpha_zero_amd").info("run_self_play: generation %d, %d games on %d slots, evaluator = %s, game_seq from %d",
                                                  generation, games_left, G, "ResNet (HIP)" if use_net else "synthetic hash evaluator", first_game_seq)
    if use_net:
        eng.load_weights(weights)
    if train_config.get("eval_symmetry"):
        eng.set_eval_symmetry(True)
    if train_config.get("solver"):
        eng.set_solver(True)
    if train_config.get("opening_book") is not None:
        try:
            eng.set_opening_book(load_book(train_config["opening_book"]), _book_mode(train_config.get("opening_book_mode") or "game"))
        except BaseException:
            eng.close()
            raise
    weighting = (*eng.sample_weighting, seed) if eng.sample_weighting[0] else None      # (the host path's: record_to_samples)
    written = 0
    launch = G                                          # slots the launches cover (shrinks in the generation's tail, see repack)
    clock = time.perf_counter
    t_wait = t_samples = 0.0
    writer = None
    try:
        writer = _ReplayWriter(store, max_pending_bytes)
        eng.run_waves(64)
        idle = 0
        while written < games_left:
            t0 = clock()
            eng.synchronize()                       # waits for the launches queued so far
            t1 = clock()
            if device_samples:
                batch = eng.drain_samples()
                got = batch.n
                batch = batch.copy() if got else None               # the engine reuses its buffers: the writer gets a copy
            else:
                recs = eng.drain_finished()
                got = len(recs)
            t_wait += t1 - t0; t_samples += clock() - t1
            # tail of the generation: every game has been started and the slots halt one by one, but a wave still evaluates all
            # of them — once half of the covered slots are idle, move the live games together and shrink the launches
            remaining = games_left - written - got                  # games not finished yet >= games still running
            if 0 < remaining and remaining * 2 <= launch and launch > 16 and leaf_batch <= 1 and gumbel_batch <= 1:
                _, launch = eng.repack()
            eng.run_waves(64)                       # queue the next ones right away: the GPU works while the host converts and writes
            if device_samples:                      # every game is one of the admitted games (games_budget)
                if got:
                    if replay is not None:
                        replay.append(generation, batch)
                    writer.put(batch, batch.nbytes)
            else:
                for rec in recs:
                    t0 = clock()
                    aug_b, aug_p, aug_v, length = record_to_samples(game_class, rec, weighting)
                    t_samples += clock() - t0
                    writer.put((aug_b, aug_p, aug_v, length, rec["T"], rec["winner"]), aug_b.nbytes + aug_p.nbytes + aug_v.nbytes)
            if progress:
                for i in range(got):
                    progress(written + i + 1, games_left)
            written += got
            idle = 0 if got else idle + 1
            if idle > 100000:
                raise RuntimeError("self-play made no progress")
        w, writer = writer, None
        w.close()                                   # everything queued is in the file; a failure of the writer surfaces here
        if engine_stats is not None:
            engine_stats.update({k: v for k, v in eng.stats().items() if k != "game_stats"})
            engine_stats["resign"] = eng.resign_stats()
            engine_stats.update(gpu_wait_seconds=t_wait, sample_seconds=t_samples, queue_wait_seconds=w.wait_seconds, writer_seconds=w.write_seconds)
    finally:
        if writer is not None:                      # an error above: what was queued is still written, the thread is joined, the error stays the caller's
            writer.close(reraise=False)
        eng.close()
    return written


# ------------------------------------------------------------------------------------------------ match play
def _elo(score):
    return None if score <= 0.0 or score >= 1.0 else -400.0 * math.log10(1.0 / score - 1.0)


def match_result(records, paired=False):
    """The result of a match (SelfPlayEngine.set_match) from its finished games: records (drain_finished's dicts) or headers (T, winner,
    slot, game_seq).  Network A plays the first player (-1) of game (slot, game_seq) iff slot + game_seq is even, so a header says who
    was A.  -> dict: n, a_wins, draws, b_wins; `a_first` / `a_second`, the same counts over the games in which A was the first / the
    second player; score = (a_wins + 0.5 draws) / n; elo = -400 log10(1 / score - 1), None at score 0 or 1; elo_ci95 = that formula on
    score -+ 1.96 sqrt(var / n), var the (population) variance of the per-game scores 1 / 0.5 / 0 and both ends clipped into
    [1e-9, 1 - 1e-9].
    paired=True (a match from an opening book in mode "pair": the games (slot, 2k) and (slot, 2k + 1) share their opening and swap colours,
    so the PAIR is the statistical unit) adds three keys: `pairs`, the counts of the pair scores {0, 0.5, 1, 1.5, 2} (A's points over the
    two games) over the complete pairs (slot, game_seq >> 1); `incomplete`, the pairs of which only one game is there; and
    `elo_ci95_paired`, the elo formula on m -+ 1.96 sqrt(var / n_pairs) with m and var the mean and (population) variance of the pair
    means (pair score / 2) over the complete pairs, clipped as above; None without a complete pair.  The other keys do not change."""
    split = {True: dict(n=0, a_wins=0, draws=0, b_wins=0), False: dict(n=0, a_wins=0, draws=0, b_wins=0)}
    scores, by_pair = [], {}
    for r in records:
        _, winner, slot, seq = (int(r[k]) for k in ("T", "winner", "slot", "game_seq")) if isinstance(r, dict) else (int(x) for x in r)
        a_first = (slot + seq) % 2 == 0
        key = "draws" if winner == 0 else ("a_wins" if (winner == -1) == a_first else "b_wins")
        split[a_first]["n"] += 1; split[a_first][key] += 1
        scores.append(0.5 if winner == 0 else (1.0 if key == "a_wins" else 0.0))
        by_pair.setdefault((slot, (seq & 0xFFFFFFFF) >> 1), {})[seq & 1] = scores[-1]
    n = len(scores)
    if n == 0:
        raise ValueError("match_result: no games")
    out = {k: split[True][k] + split[False][k] for k in ("n", "a_wins", "draws", "b_wins")}
    score = (out["a_wins"] + 0.5 * out["draws"]) / n
    var = sum((x - score) ** 2 for x in scores) / n
    half = 1.96 * math.sqrt(var / n)
    clip = lambda x: min(max(x, 1e-9), 1.0 - 1e-9)
    out.update(a_first=split[True], a_second=split[False], score=score, elo=_elo(score), elo_ci95=(_elo(clip(score - half)), _elo(clip(score + half))))
    if paired:
        whole = [g[0] + g[1] for g in by_pair.values() if len(g) == 2]
        out["pairs"] = {s: sum(1 for x in whole if x == s) for s in (0.0, 0.5, 1.0, 1.5, 2.0)}
        out["incomplete"] = len(by_pair) - len(whole)
        out["elo_ci95_paired"] = None
        if whole:
            means = [x / 2.0 for x in whole]
            m = sum(means) / len(means)
            half_p = 1.96 * math.sqrt(sum((x - m) ** 2 for x in means) / len(means) / len(means))
            out["elo_ci95_paired"] = (_elo(clip(m - half_p)), _elo(clip(m + half_p)))
    return out


def play_match(game_class, configs, weights_a, weights_b, games, n_slots=None, seed=0, book=None, paired=None, **engine_kw):
    """`games` games between network A (`weights_a`) and network B (`weights_b`) in one engine -> match_result of them, plus `positions`
    (plies played), `seconds` and `match_stats`.  Weights are dicts from net.export_engine_weights(); None for both plays the synthetic
    hash evaluator under engine_kw's hash_salt (A) and hash_salt_b (B).  `games` must be a positive multiple of 2 * n_slots (default
    n_slots = games / 2): every slot then plays as many games with A first as with B first.  The search settings come from train_config
    as in run_self_play; the engine has one game group and no evaluation cache (SelfPlayEngine.set_match).
    book: an opening book (a list of action-index sequences, or a file as train_config["opening_book"]); paired (default: True with a book)
    sets its mode to "pair" — the two games (slot, 2k), (slot, 2k + 1), which swap colours, start from the same entry — and the result
    carries match_result(paired=True)'s keys; paired=False draws an entry per game.  A match at playing strength (tau 0, no root noise)
    needs a book: without one every slot plays the same two games."""
    build_config = configs[0]
    if paired is None:
        paired = book is not None
    if paired and engine_kw.get("first_game_seq", 0) % 2:
        raise ValueError("play_match: paired games need an even first_game_seq (a pair is (slot, 2k), (slot, 2k + 1))")
    if n_slots is None:
        n_slots = max(int(games) // 2, 1)
    if games <= 0 or n_slots <= 0 or games % (2 * n_slots):
        raise ValueError(f"play_match: games ({games}) must be a positive multiple of 2 * n_slots ({2 * n_slots}), so that the colours balance")
    if (weights_a is None) != (weights_b is None):
        raise ValueError("play_match: give the weights of both networks, or of neither (the synthetic evaluator under two salts)")
    use_net = weights_a is not None
    name = getattr(game_class, "ENGINE_NAME", game_class.__name__)
    if use_net:
        from .net import check_engine_weights
        for w in (weights_a, weights_b):
            check_engine_weights(name, build_config.get("num_resnet_layers", 0), build_config.get("num_filters", 128), w)
    args, kw = engine_search_settings(game_class, configs)
    salt_b = engine_kw.pop("hash_salt_b", 0)
    kw.update(evaluator=EVAL_RESNET if use_net else EVAL_HASH, net_blocks=build_config.get("num_resnet_layers", 0) if use_net else 0,
              net_filters=build_config.get("num_filters", 128), ring_capacity=max(4 * n_slots, 64), games_budget=int(games), game_groups=1)
    kw.update(engine_kw)
    eng = SelfPlayEngine(name, n_slots, *args, seed, **kw)
    try:
        if use_net:
            eng.load_weights(weights_a); eng.load_weights_b(weights_b)
        eng.set_match(True, hash_salt_b=salt_b)
        if book is not None:
            eng.set_opening_book(load_book(book), "pair" if paired else "game")
        train_config = configs[1]
        if train_config.get("eval_symmetry"):
            eng.set_eval_symmetry(True)
        if train_config.get("solver"):
            eng.set_solver(True)
        t0 = time.perf_counter()
        records, idle = [], 0
        while len(records) < games:
            eng.run_waves(64)
            got = eng.drain_finished()
            records += got
            idle = 0 if got else idle + 1
            if idle > 100000:
                raise RuntimeError("the match made no progress")
        seconds = time.perf_counter() - t0
        out = match_result(records, paired=bool(paired))
        if book is not None:
            bc = eng.book_counts()
            out["book"] = dict(entries=len(bc["counts"]), mode="pair" if paired else "game", counts=[int(c) for c in bc["counts"]], prefix_plies=bc["prefix_plies"])
        out.update(positions=sum(int(r["T"]) for r in records), seconds=seconds, match_stats=eng.match_stats())
        out["headers"] = [(int(r["T"]), int(r["winner"]), int(r["slot"]), int(r["game_seq"])) for r in records]
    finally:
        eng.close()
    return out

/*
 * gaz_engine.h — C ABI of the MI355X batched self-play engine (libgaz_engine.so).
 *
 * The reference (subtotechnoblade/Grok_Alpha_Zero, pure Python) has no FFI; its boundaries are the
 * duck-typed Python surfaces listed below.  The Python package grok_alpha_zero_amd/ re-presents those
 * surfaces (same names / arguments) on top of this ABI; INTEGRATION.md shows the ctypes stub a reference
 * maintainer would add.  Every entry point returns 0 on success, non-zero on failure
 * (gaz_engine_last_error gives the text); no exceptions, no torch types, caller-owned buffers,
 * one host thread per engine (= per GPU), HIP streams internal.
 *
 * Reference interface replaced by each entry point (file:line under /root/reference):
 *   gaz_engine_create          Self_Play.__init__ building MCTS x2 per game   Self_Play.py:16-69, MCTS.py:78-132
 *                              + run_self_play's worker / server start-up      Self_Play.py:259-363
 *   gaz_engine_load_weights    rt.InferenceSession(onnx_path) in the server    Client_Server.py:119-120
 *   gaz_engine_reset_games     self_play_task -> game_class()                  Self_Play.py:237-245
 *   gaz_engine_run_move        MCTS.run(iteration_limit) for every live game   MCTS.py:528-618 (Self_Play.py:97-106)
 *   gaz_engine_get_root_stats  the move_probs rows MCTS.run returns            MCTS.py:591-600
 *   gaz_engine_apply_moves     game.do_action + mcts1/2.prune_tree             Self_Play.py:142-157, MCTS.py:657-671
 *   gaz_engine_run_waves       the whole Self_Play.play loop, device resident  Self_Play.py:71-157
 *   gaz_engine_wave_begin/end  session.run(["policy","value"], {"inputs": x})  MCTS.py:224-235, Client_Server.py:28-55,162-217
 *   gaz_engine_drain_finished  the per-game arrays play() hands to HDF5        Self_Play.py:159-175
 *   gaz_engine_get_stats       file["game_stats"] u32[6]                       Self_Play.py:181-188
 *   gaz_engine_set_position    MCTS.__init__ attaching to a live game object   MCTS.py:100,132,296-313
 *   gaz_engine_read_positions  game.action_history of every game in progress      Guide.py:111-133 (the attribute MCTS reads at MCTS.py:297-313)
 *   gaz_engine_set_search_params  run(iteration_limit) / update_hyperparams(tau) MCTS.py:134-168,528
 *   gaz_engine_set_hyperparams    MCTS.update_hyperparams(c_puct_*, dirichlet_*, tau) MCTS.py:134-168;
 *                                 MCTS_Gumbel.update_hyperparams(m, c_visit, c_scale)  MCTS_Gumbel.py:186-210
 *   gaz_engine_probe_rules     the Game plugin's static *_MCTS functions          Guide.py:135-283, Game_Tester.py:297-405
 *   gaz_engine_probe_det       (test probe; no reference counterpart: the device's float64 / Philox arithmetic as raw bits)
 *   gaz_engine_stop_search        run(time_limit)                             MCTS.py:560-563
 *   gaz_engine_repack             finished workers no longer load the inference server  Self_Play.py:380-400
 *   gaz_engine_set_fused_wave     (scheduling switch; no reference counterpart: Client_Server.py's server loop is what it replaces)
 *   gaz_engine_debug_fused_fault  (test hook for that launch's bounded hand-over; what it replaces is the client's unbounded
 *                                  spin on the server's flag, Client_Server.py:42-55)
 *   gaz_engine_evaluate        sess.run on a stacked batch (evaluator probe)   Compute_Speed.py:40-63, Client_Server.py:199-206
 *   gaz_engine_read_head_features  intermediate tensors of that probe (numerics tests)  Connect4/Build_Model.py:41-47,62-66
 *   gaz_engine_config.leaf_batch / gaz_engine_batch_rows  (no reference counterpart: several leaves of one tree per evaluator batch, kept
 *                                  apart by a virtual loss — the first open item of the reference's roadmap, README.md:59)
 *   gaz_engine_config.gumbel_batch  (scheduling of MCTS_Gumbel.run's loop over the surviving root children, MCTS_Gumbel.py:625-645: the
 *                                  candidates of one halving phase in one evaluator batch, same results)
 *   gaz_engine_read_trees      MCTS.root and everything below it: Node.children / child_visits / child_values /
 *                              child_prob_priors / is_terminal of every node                                MCTS.py:20-72,403-426
 *   gaz_engine_read_pv         (no reference counterpart: the most visited line below every root)
 *   gaz_engine_set_resignation / gaz_engine_get_resign_stats  (no reference counterpart: Self_Play.play() plays every game to its end;
 *                              resignation with a share of games played out to measure its false positives is AlphaGo Zero's, Silver 2017)
 *   the 0x10 / 0x20 bits of a record's move_kind  (no reference counterpart: the marks that rule leaves in the record)
 *   gaz_engine_set_solver / gaz_engine_get_solver / gaz_engine_get_solver_stats  (no reference counterpart: proven wins, draws and losses in
 *     the PUCT tree), bits 1-2 of gaz_tree_node.flags and the 0x40 bit of a record's move_kind
 *   gaz_engine_set_eval_symmetry / gaz_engine_get_eval_symmetry / gaz_engine_read_batch_symmetry  (no reference counterpart: the reference
 *                              augments its training samples with the board symmetries, Guide.py:255-283, but always shows the search's
 *                              network one orientation; a random symmetry per evaluation is AlphaGo Zero's and KataGo's)
 *   gaz_engine_set_match / gaz_engine_get_match / gaz_engine_load_weights_b / gaz_engine_read_batch_network / gaz_engine_get_match_stats /
 *   gaz_engine_get_match_timing
 *                              (no reference counterpart: the reference's Run has no evaluation step, every generation's network is played on
 *                              unconditionally, <game>/main.py; a match between the new and the current network is AlphaGo Zero's evaluator)
 *   gaz_engine_set_opening_book / gaz_engine_get_opening_book / gaz_engine_read_book_counts and the kind 3 of a record's move_kind
 *                              (no reference counterpart: Self_Play.play() starts every game on the empty board and opening_actions,
 *                              Self_Play.py:130-140, overrides move 0 only; an opening book played in colour-swapped pairs is the usual
 *                              remedy of engine testing, starting a share of the self-play games from book positions is KataGo's)
 */
#ifndef GAZ_ENGINE_H
#define GAZ_ENGINE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct gaz_engine gaz_engine;

enum { GAZ_GAME_TICTACTOE = 0, GAZ_GAME_CONNECT4 = 1, GAZ_GAME_GOMOKU = 2 };
enum { GAZ_SEARCH_PUCT = 0, GAZ_SEARCH_GUMBEL = 1 };
enum { GAZ_EVAL_HASH = 0,      /* synthetic bit-reproducible evaluator (parity tests) */
       GAZ_EVAL_RESNET = 1,    /* the ResNet policy/value network, HIP MFMA kernels */
       GAZ_EVAL_EXTERNAL = 2   /* caller evaluates the batch between wave_begin / wave_end */ };

#define GAZ_ENGINE_ABI_VERSION 10  /* bumped whenever something EXISTING changes: a field of gaz_engine_config / gaz_search_hyperparams / a layout
                                      struct, or the signature or meaning of an entry point.  A new entry point or a new struct next to
                                      unchanged ones does not bump it: a caller detects such a feature by its symbol (dlsym), as with
                                      gaz_engine_set_resignation */

typedef struct {
    uint32_t struct_size;         /* = sizeof(gaz_engine_config) of the header the caller was built against; gaz_engine_create
                                     rejects any other value (a stale binding would otherwise be read past its end) */
    int32_t game;                 /* GAZ_GAME_* */
    int32_t search;               /* GAZ_SEARCH_* */
    int32_t n_games;              /* concurrent games on this GPU */
    int32_t run_iterations;       /* iteration_limit passed to MCTS.run (Self_Play passes int(1.5*MCTS_iteration_limit)) */
    int32_t max_actions;          /* train_config["max_actions"] */
    int32_t num_explore_actions_first, num_explore_actions_second;
    double c_puct_init, c_puct_base;
    double dirichlet_alpha, dirichlet_epsilon;
    int32_t use_dirichlet;
    int32_t create_new_root;      /* train_config.get("create_new_root", False) */
    int32_t sync_moves;           /* 1: stop after each move for get_root_stats/apply_moves; 0: continuous self-play */
    int32_t nodes_per_tree;       /* arena capacity per (game, tree); 0 = default for the game */
    int32_t ring_capacity;        /* finished-game records kept for drain_finished; 0 = keep none */
    uint64_t seed;
    uint32_t slot_offset;         /* global slot of local game 0 (rank * n_games) */
    int32_t evaluator;            /* GAZ_EVAL_* */
    uint32_t hash_salt;
    int32_t device;               /* HIP device ordinal */
    /* ResNet (evaluator == GAZ_EVAL_RESNET): trunk of `net_blocks` pre-activation blocks x `net_filters`
       (build_config["num_filters"]).  Connect4 and Gomoku: 64, 128, 192 or 256 — 128 runs the fused trunk kernels, the other
       widths one k_conv_wide launch per convolution (separate launches, one game group by default); any other value fails
       gaz_engine_create.  TicTacToe: 64 (0 and 128 are accepted and mean 64). */
    int32_t net_blocks, net_filters;
    int32_t policy_is_logits;     /* policy head: 0 = softmax (float64, Build_Model.py:60), 1 = raw logits (Gumbel),
                                     2 = stablemax (Net/Stablemax.py:8-12, build_config["use_stablemax"]) */
    int32_t gumbel_m;             /* train_config["m"]: actions sampled in the first stage of sequential halving */
    double c_visit, c_scale;      /* train_config["c_visit"], ["c_scale"] (MCTS_Gumbel.py:160-161) */
    int32_t compact_trees;        /* re-root compaction of the tree arena: 0 = auto (on for Gomoku), 1 = on, -1 = off */
    int32_t single_tree;          /* 1: one tree plays both sides (MCTS used on its own: Connect4/play.py, Game_Tester.py:480-513) */
    int32_t n_opening;            /* train_config["opening_actions"] (Self_Play.py:130-140): up to 8 [action, weight] pairs */
    int32_t opening_actions[8];
    double opening_weights[8];
    int32_t max_tree_sims_per_wave; /* evaluation-free simulations a game may run per launch before it yields (0 = the configuration's measured default: 4 .. 32);
                                       scheduling only — results do not depend on it.  With leaf_batch > 1 it is part of the search (which leaves share a launch
                                       decides the result): only simulations that complete without an evaluation count, reserved leaves do not, and the count
                                       starts again with every move */
    int32_t eval_cache_log2;      /* on-device evaluation cache with 2^n entries, keyed by the encoded leaf state (replaces
                                     Session_Cache.Cache_Wrapper, Session_Cache.py:4-26 / Self_Play.py:234-236); 0 = off.
                                     A hit returns the bits the evaluator produced for the same input: results do not change */
    int32_t gumbel_stablemax;     /* 1: MCTS_Gumbel(activation_fn="stablemax") — build_config["use_stablemax"] (Self_Play.py:69):
                                     stablemax instead of softmax inside deterministic_selection (MCTS_Gumbel.py:144-148) */
    int32_t fast_find_win;        /* MCTS(fast_find_win=True) (MCTS.py:88,282-283; MCTS_Gumbel.py:313): a position with a winning
                                     move keeps only the first one (in legal-action order); Self_Play always passes False */
    int32_t no_gumbel_noise;      /* 1: MCTS_Gumbel(use_gumbel_noise=False), the class default (MCTS_Gumbel.py:157,592-596): no Gumbel
                                     variates are added to the root logits and no RNG event is consumed.  Self_Play passes True (:64) */
    uint32_t first_game_seq;      /* game sequence number of the first game of every slot (RNG streams are keyed by (seed, slot,
                                     game_seq)): a resumed generation passes the games already in the replay file so that no game
                                     is replayed (Self_Play.py:267-272 resumes by count; its workers reseed from OS entropy, :221) */
    int64_t games_budget;         /* continuous self-play only: > 0 = play exactly this many games — slot g plays its k-th game
                                     (k = game_seq - first_game_seq) iff k * n_games + g < games_budget, then halts — so a generation
                                     is the FIRST games_budget games STARTED, all run to completion (Self_Play.py:346-408), not the
                                     first ones to finish; 0 = slots restart forever */
    double tau;                   /* MCTS(tau=...) (MCTS.py:116-120,602-610): < 0 = Self_Play's schedule (tau 1 for the first
                                     num_explore_actions plies of each player, then 0); 0 = most visited move; > 0 = sample with
                                     weights N^(1/tau).  gaz_engine_set_hyperparams changes it between runs */
    double move_time_limit;       /* train_config["MCTS_time_limit"] in seconds (Self_Play.py:35,100-112), 0 = none.  PUCT: every game's move ends when its
                                     own wall clock since the move began passes the limit or run_iterations are used up, whichever comes first — at
                                     least one simulation (MCTS.py:559-560); results then depend on timing, as in the reference.  Gumbel: any
                                     limit makes every move run 3 x its legal moves iterations ("Time limit isn't allowed for gumbel",
                                     MCTS_Gumbel.py:576-578).  Continuous self-play only */
    int32_t game_groups;          /* scheduling only — no game depends on it.  K >= 2: the games run as K groups of consecutive slots, each with its own
                                     stream, evaluator batch and launch per wave, stepped alternately: the trunk tiles of one group fill the chip while
                                     another group's tree step starts or its heads run (continuous self-play with a built-in evaluator only; the
                                     wave_begin / batch API is refused).  1 = one batch.  0 = automatic: 2 where measured to pay (Connect4 PUCT +
                                     ResNet from 3072 games: +9.7 % evaluations/s; Gomoku PUCT + ResNet from 2048 games: +8.6 %; Connect4 Gumbel + ResNet from 6144 games: +6 %), else 1.  With the evaluation cache every group keeps a table of its own */
    int32_t leaf_batch;           /* PUCT search only.  0 / 1: one leaf per game and wave (the search of the reference, bit for bit).  K in 2..64: a game may
                                     hold up to K leaves in flight per wave; a leaf on its way carries a virtual loss (N + 1, W - 1 on every edge of its
                                     path) and the next wave applies the K results in the order they were reserved — a different, deterministic search
                                     (DESIGN.md "Leaf-batched PUCT search") that fills the evaluator batch from few games.  The batch then has n_games * K
                                     rows (gaz_engine_batch_rows), row g * K + j = leaf j of game g; game_groups = 0 resolves to 1 and the tree step and the
                                     evaluator run as separate launches.  Refused by gaz_engine_create with search = GAZ_SEARCH_GUMBEL, eval_cache_log2 > 0,
                                     game_groups > 1, or a value above 64; gaz_engine_repack is refused on such an engine */
    int32_t gumbel_batch;         /* Gumbel search only.  0 / 1: one candidate of sequential halving per game and wave.  K in 2..64: a game keeps up to K
                                     candidates of the current halving phase in flight per wave, each with a leaf of its own.  The phase's candidate list is
                                     served in consecutive chunks of K (the last one may be shorter); a chunk is finished when every one of its candidates
                                     has its root child expanded and has used its visits, then the next chunk starts, and after the last one the phase ends
                                     as with 1.  A launch first applies every row the previous evaluator pass answered, in row order, then every candidate
                                     of the chunk advances until it needs the network again, has used its visits, or has started max_tree_sims_per_wave
                                     visits in this launch (scheduling only here); within one candidate the visits stay strictly sequential, and a move
                                     ends only with nothing in flight.  Everything a visit touches belongs to its root child, so the SAME search comes out,
                                     bit for bit: records, evaluator calls, simulations, root visits and RNG events per move are those of gumbel_batch = 1
                                     (node indices inside the arena may differ) — in fewer launches (DESIGN.md "Batched sequential halving").
                                     The batch then has n_games * K rows (gaz_engine_batch_rows), row g * K + j = candidate chunk * K + j of game g;
                                     game_groups = 0 resolves to 1 and the tree step and the evaluator run as separate launches.  Raising gumbel_m above K
                                     with gaz_engine_set_hyperparams is legal (more chunks).  Refused by gaz_engine_create with search = GAZ_SEARCH_PUCT,
                                     eval_cache_log2 > 0, game_groups > 1, leaf_batch > 1, or a value above 64; gaz_engine_repack and
                                     gaz_engine_debug_fused_fault are refused on such an engine */
    int32_t fast_iterations;      /* playout cap randomisation (KataGo, Wu 2019; DESIGN.md "Playout cap randomisation"; no reference counterpart).  0 = off: every
                                     move runs run_iterations.  F > 0: a move is a FULL search (run_iterations) with probability full_search_prob, else a
                                     FAST one of min(F, run_iterations) iterations that only advances the game — its ply is left out of the training samples
                                     (gaz_engine_drain_samples) and marked 2 in the record's move_kind.  Per move one uniform variate of the game-level stream
                                     (tree 2, event = the ply, purpose 5) decides; the first searched move of every game is always full.  The PUCT rules
                                     "one legal move: 1 iteration" and "limit below the legal moves: 3 x legal moves" apply to the chosen limit as before.
                                     Refused by gaz_engine_create when negative, above run_iterations, or combined with move_time_limit > 0 */
    double full_search_prob;      /* p in (0, 1] with fast_iterations > 0; must be 0 with fast_iterations = 0 */
    double forced_playouts_k;     /* forced playouts and policy target pruning (KataGo, Wu 2019, section 3.2; DESIGN.md "Forced playouts and policy target
                                     pruning"; no reference counterpart).  PUCT search only.  0 = off: every game is what it is without the field.  k > 0
                                     (KataGo: 2), on every FULL move (with the playout cap off: every move) whose root is no terminal parent: at the fully
                                     visited root a child with N > 0 and N < sqrt(k * P * root visits) is owed a visit, and the lowest owed slot is
                                     selected instead of PUCT's choice (no RNG event is consumed); at the end of the move the record's POLICY row is written
                                     without the forced visits that PUCT would not have chosen — the root's N / W / P rows, the move sample and q stay raw.
                                     Composes with leaf_batch, single_tree, sync and continuous mode, the evaluation cache, game groups, fused launches,
                                     gaz_engine_repack, move_time_limit and the playout cap.  Refused by gaz_engine_create when negative, NaN or infinite,
                                     or when > 0 with search = GAZ_SEARCH_GUMBEL */
} gaz_engine_config;

/* MCTS.update_hyperparams(**kwargs) (MCTS.py:134-168) / MCTS_Gumbel.update_hyperparams (MCTS_Gumbel.py:186-210): values take
 * effect at the next launch.  A NaN double / negative int32 field means "unchanged" (kwargs.get(...) is None). */
typedef struct {
    uint32_t struct_size;         /* = sizeof(gaz_search_hyperparams) */
    int32_t use_dirichlet;        /* < 0 unchanged */
    double c_puct_init, c_puct_base, dirichlet_alpha, dirichlet_epsilon;
    double tau;                   /* as gaz_engine_config.tau; NaN unchanged */
    int32_t gumbel_m;             /* < 0 unchanged */
    int32_t run_iterations;       /* <= 0 unchanged */
    double c_visit, c_scale;
} gaz_search_hyperparams;

typedef struct {
    const char* name;             /* e.g. "stem.conv.weight" — see grok_alpha_zero_amd/net.py */
    const float* data;            /* host pointer, float32, C-contiguous */
    int64_t numel;
} gaz_tensor;

/* layout of one finished-game record in the byte blob returned by drain_finished */
typedef struct {
    int32_t record_bytes, max_T, A, t_pad;
    int32_t off_hdr, off_actions, off_q, off_root_visits, off_evals, off_policy, off_N, off_W, off_P;
    int32_t off_move_kind;        /* u8 [t_pad] per ply: 0 = no search ran there (a gaz_engine_set_position prefix), 1 = full search, 2 = fast search
                                     (gaz_engine_config.fast_iterations), 3 = a ply of an opening-book prefix (gaz_engine_set_opening_book: no search
                                     ran there either, and unlike kind 0 it gives no training row); always 1 for a searched ply with the cap off.
                                     That kind is the byte's low two bits (& 3).  With resignation on (gaz_engine_set_resignation) two more bits may be set: 0x10 on the last
                                     ply of a game that was resigned after it, 0x20 on every ply of a game played out with resignation
                                     disabled at which it would have been resigned.  With the solver on (gaz_engine_set_solver) 0x40 marks a ply
                                     that ended with a proven root (its q is the exact +1 / 0 / -1); all other bits are 0 */
} gaz_record_layout;

int gaz_engine_abi_version(void);                   /* GAZ_ENGINE_ABI_VERSION of the library */
int gaz_engine_config_size(void);                   /* sizeof(gaz_engine_config) of the library */
int gaz_engine_create(const gaz_engine_config* cfg, gaz_engine** out);
void gaz_engine_destroy(gaz_engine* h);
const char* gaz_engine_last_error(gaz_engine* h);   /* h may be NULL: last create() error */

/* Capacity limits and the device error.  The kernels report what they cannot carry on with through one error word on the
 * device, first code wins: 1 "tree arena full (raise nodes_per_tree)", 2 "root not fully expanded at move end", 3 "selection path longer than the
 * game can last", 4 "state-machine loop guard", 5 "PUCT picked an un-poppable child".  A call that synchronises with the device — gaz_engine_run_move,
 * gaz_engine_apply_moves, gaz_engine_drain_finished, gaz_engine_drain_samples, gaz_engine_get_stats, gaz_engine_get_resign_stats,
 * gaz_engine_read_batch, gaz_engine_read_batch_symmetry, gaz_engine_synchronize — reads the word and fails with last_error "device error: <text>".
 * gaz_engine_run_waves only queues launches and does not look.  It is a return value, not a GPU fault: the process and the device go on.
 *   - The game that raised error 1, 2, 3 or 5 does not advance again, in that launch or in any later one: no further node is written, no move applied,
 *     no record pushed, no evaluator request made on its behalf (its phase is 10, "fault", in gaz_engine_get_root_stats' out_phase).  In a launch that
 *     runs the tree step and the network together it still reports itself done, so nothing waits for it.  Error 4 belongs to no game: it says that a
 *     wavefront used up its steps for one launch; its games keep their phases, consistent, and go on in the next launch.
 *   - The other games are unaffected until the host reads the error: what they push into the ring is what they would have played in a larger arena.
 *   - The error is sticky on the handle: the word is never cleared, every later synchronising call fails with the same text, and the only way on is
 *     gaz_engine_destroy and a new engine (with a larger nodes_per_tree).  A caller that wants no doubtful data drops what a failing call handed out.
 *   - Reading state after the error: gaz_engine_read_positions and gaz_engine_get_root_stats do not look at the word and succeed;
 *     gaz_engine_get_stats and gaz_engine_drain_finished fill their outputs and then return the error.
 * The tree arena.  nodes_per_tree = 0 sizes every tree for the longest game the configuration can play: (plies the tree searches + 1) x
 * (max(run_iterations, 3 x actions) + 2) + 64 nodes, where a tree searches every other ply of its game, or every ply with single_tree = 1; with
 * re-root compaction 4 x max(run_iterations, 3 x actions) + 3 x actions + 64 per half; Gumbel 2 x (run_iterations + gumbel_m) + 3 x actions + 64; plus
 * leaf_batch nodes for the leaves in flight.  gaz_engine_set_hyperparams holds later run_iterations / gumbel_m against the same formula and refuses what
 * the arena was not sized for; with an explicit nodes_per_tree it accepts every value, and a game that outgrows the arena raises error 1.
 * The record ring.  A game that finishes while ring_capacity records wait to be drained keeps its record and retries the push in every launch; it
 * is counted in game_stats once, when it finishes.  Nothing is lost or duplicated however small the ring (>= 1) and however little a drain takes. */

int gaz_engine_load_weights(gaz_engine* h, const gaz_tensor* tensors, int32_t n);
int gaz_engine_reset_games(gaz_engine* h, const int32_t* slots, int32_t n);   /* slots NULL = all */

/* synchronous per-move API (cfg.sync_moves = 1) */
int gaz_engine_run_move(gaz_engine* h, int32_t* n_waiting);                    /* runs waves until every live game finished its MCTS.run */
int gaz_engine_get_root_stats(gaz_engine* h, uint32_t* out_N, float* out_W, float* out_P, float* out_policy,
                              uint32_t* out_root_visits, float* out_q, int32_t* out_chosen, int32_t* out_phase);
                              /* [n_games][A] x4, [n_games] x4; any pointer may be NULL.  out_policy is the record's policy row of the move: with
                                 forced_playouts_k > 0 the PRUNED target of a full move, while out_N / out_W / out_P stay the raw root arrays */
int gaz_engine_apply_moves(gaz_engine* h, const int32_t* moves);               /* moves NULL / entry < 0 = play the sampled move */

/* continuous device-resident self-play (cfg.sync_moves = 0) */
int gaz_engine_run_waves(gaz_engine* h, int32_t n_waves);

/* external evaluator: wave_begin leaves the batch in HBM, wave_end consumes policy/value written by the caller */
int gaz_engine_wave_begin(gaz_engine* h);
int gaz_engine_wave_end(gaz_engine* h);
int gaz_engine_batch_ptrs(gaz_engine* h, void** d_inputs_i8, void** d_policy_f32, void** d_value_f32);   /* device pointers */
int gaz_engine_read_batch(gaz_engine* h, int8_t* inputs, int32_t* pending);    /* host copies: [rows][H*W*C], [rows] */
int gaz_engine_write_outputs(gaz_engine* h, const float* policy, const float* value);   /* host -> device rows: [rows][A], [rows] */
/* rows of the evaluator batch: n_games, or n_games * leaf_batch with leaf_batch > 1 — then read_batch, write_outputs and batch_ptrs address
 * that many rows, pending[g * leaf_batch + j] says whether row g * leaf_batch + j (leaf j of game g) carries a request, and
 * gaz_engine_evaluate takes up to that many rows.  Rows nobody requested are evaluated and ignored.  The same with gumbel_batch = K > 1:
 * n_games * K rows, and pending[] is per row — the rows of a game that carry a request need not be its first ones. */
int gaz_engine_batch_rows(gaz_engine* h, int32_t* rows);

/* Random board symmetry per evaluator request.  mode 0 = off (the state of a new engine), 1 = on; any other value is refused.  Legal on any
 * engine at any time; it takes effect for the rows encoded from the next launch on, and a request already in flight is answered under the
 * symmetry it was encoded with.  No struct changes and GAZ_ENGINE_ABI_VERSION stays 10: the feature is detected by its symbols.
 * With the mode on, every request the searches encode (root creations and leaf expansions; PUCT, leaf_batch, Gumbel, gumbel_batch) shows the
 * network T_k(state), and the search uses T_k^-1 of the policy row it gets back; the value is used as it is.  k is drawn per POSITION of a game:
 *   h = sum over the cells c = y * W + x of mix64(((uint64)(c + 1) << 32) | (uint8)board[c])  (mod 2^64; board = the int8 board, -1 -> 0xff),
 *   mix64(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31,
 *   u = the uniform variate of (seed, slot, game_seq, tree 2, event = (uint32)(mix64(h) >> 32), purpose 7),  k = min(NSYM - 1, (int)(u * NSYM)).
 * No tree's event counter moves and no other variate changes; both trees of a game, every launch shape and the evaluation cache see the same k
 * for the same position of the same game.  Square boards (NSYM = 8): the transforms of the training samples in their order — identity, flipud,
 * fliplr, rot90, flipud(rot90), fliplr(rot90), rot180, rot270 (counter-clockwise) — applied to the [H][W][C] state over its first two axes; the
 * inverses are k' = [0, 1, 2, 7, 4, 5, 6, 3].  Connect4 (NSYM = 2): k = 1 mirrors the COLUMNS (x -> 6 - x) of all four planes, and the policy
 * likewise (this is not the row reversal its sample augmentation applies to states).
 * Everything else stays in the board's own frame: records, gaz_engine_drain_samples, gaz_engine_get_root_stats, gaz_engine_read_trees / read_pv,
 * gaz_engine_probe_rules, gaz_engine_evaluate.  A GAZ_EVAL_EXTERNAL caller sees the PERMUTED rows in gaz_engine_read_batch / batch_ptrs and
 * answers in that frame — a network needs nothing else; gaz_engine_read_batch_symmetry tells which k a row was written under. */
int gaz_engine_set_eval_symmetry(gaz_engine* h, int32_t mode);
int gaz_engine_get_eval_symmetry(gaz_engine* h, int32_t* mode);
/* sym[rows] (gaz_engine_batch_rows): the k of every row of the evaluator batch — meaningful where gaz_engine_read_batch's pending is set; a row
 * without a request keeps the k of the last request written there (0 if none, and 0 everywhere while the mode has never been on).  Available and
 * refused where gaz_engine_read_batch is (game groups: refused). */
int gaz_engine_read_batch_symmetry(gaz_engine* h, uint8_t* sym);

/* Match play: the games of one engine played by TWO networks, to tell whether one is stronger (no reference counterpart).
 * Network A is the weight set of gaz_engine_load_weights (GAZ_EVAL_HASH: the salt gaz_engine_config.hash_salt), network B that of
 * gaz_engine_load_weights_b (hash_salt_b).  mode 0 = off (the state of a new engine), 1 = on.  No struct changes and GAZ_ENGINE_ABI_VERSION stays
 * 10: the feature is detected by its symbols.
 * RULE.  In game (slot, game_seq) — slot = the global slot, slot_offset + the slot the game started in, as in the record header — network A
 * plays the first player (-1) iff (slot + game_seq) is even: colours alternate over the slots and over the successive games of a slot.  The
 * OWNER of a pending request is, PUCT with two trees: the tree that asks (tree 0 searches for player -1, tree 1 for player 1; a root creation
 * after a move belongs to the tree it builds); Gumbel: the player to move in the game, -1 -> 0, 1 -> 1.  The request is answered by network
 *   owner XOR ((slot + game_seq) & 1)                                                     (0 = A, 1 = B).
 * The rule is a function of the game state alone: switching the mode takes effect at the next evaluator pass and needs no migration, and a
 * record's header (T, winner, slot, game_seq) says who was A, so results are tallied from records (records are unchanged).
 * Allowed: PUCT with two trees and Gumbel; GAZ_EVAL_HASH, GAZ_EVAL_RESNET (every num_filters) and GAZ_EVAL_EXTERNAL; sync and continuous mode;
 * games_budget, the playout cap, forced playouts, resignation, the solver and the evaluation symmetry (none of them is touched).
 * Refused, each with its own last_error text: single_tree = 1, leaf_batch > 1, gumbel_batch > 1, eval_cache_log2 > 0, an engine that resolved to
 * game groups (create it with game_groups = 1), a struct_size other than sizeof(gaz_match_params), a mode other than 0 or 1; and with the mode on
 * and GAZ_EVAL_RESNET, gaz_engine_run_move / gaz_engine_run_waves before gaz_engine_load_weights_b ("weights of network B not loaded").
 * While the mode is on the tree step and the evaluator pass are separate launches (gaz_engine_get_stats [12] is 0), the host waits once per
 * wave for the two row counts, rows without a request are neither evaluated nor written, and gaz_engine_repack and
 * gaz_engine_debug_fused_fault are refused; gaz_engine_evaluate stays network A.  Switching off restores everything.
 * Out of scope: leaf_batch / gumbel_batch, the evaluation cache, game groups, the fused launch and repack with the mode on; more than two
 * networks; matches over several GPUs. */
typedef struct {
    uint32_t struct_size;         /* = sizeof(gaz_match_params) */
    int32_t mode;                 /* 0 off, 1 on */
    uint32_t hash_salt_b;         /* GAZ_EVAL_HASH: the salt of network B (ignored by the other evaluators) */
    int32_t reserved_;
} gaz_match_params;
int gaz_engine_set_match(gaz_engine* h, const gaz_match_params* p);
int gaz_engine_get_match(gaz_engine* h, int32_t* mode);
/* the weights of network B: the names and shapes of gaz_engine_load_weights.  Legal before the mode is switched on */
int gaz_engine_load_weights_b(gaz_engine* h, const gaz_tensor* tensors, int32_t n);
/* net[rows] (rows = n_games): the network that answers every row of the evaluator batch as the games stand — 0 = A, 1 = B, 255 = the row
 * carries no request (exactly where gaz_engine_read_batch's pending is 0).  A GAZ_EVAL_EXTERNAL caller answers each row with the network the
 * byte names.  Legal with the mode off too (the rule is stateless); refused where gaz_engine_set_match(1) is. */
int gaz_engine_read_batch_network(gaz_engine* h, uint8_t* net);
/* host counters over the engine's life: [0] rows evaluated by A, [1] by B, [2] waves in which A got no row, [3] in which B got none,
 * [4] evaluator passes with the mode on, [5..7] 0.  (GAZ_EVAL_EXTERNAL: the engine runs no evaluator pass, all 0.) */
int gaz_engine_get_match_stats(gaz_engine* h, uint64_t out[8]);
/* what the routing stage costs (tools/match_bench.py), summed over the waves that gaz_engine_timing_reset(1) brackets (every 8th), in ms, HIP
 * events on the engine's stream: [0] route + partition + copy, [1] the stream's idle gap from the end of the copy to the first launch after
 * the host's wait for the row counts, [2] the scatter; [3] the host's time inside that wait (host clock), [4] the waves bracketed, [5..7] 0.
 * A host synchronisation point. */
int gaz_engine_get_match_timing(gaz_engine* h, double out[8]);

/* Solver (MCTS-Solver): proven wins, draws and losses in the PUCT search.  mode 0 = off (the state of a new engine), 1 = on; any other value
 * is refused.  It takes effect at the next launch; statuses are written and used only while it is on.  Refused — each with its own last_error
 * text — on engines with the Gumbel search, with leaf_batch > 1 and with gumbel_batch > 1.  No struct changes and GAZ_ENGINE_ABI_VERSION stays
 * 10: the feature is detected by its symbols.  With the mode on the search is a different, deterministic one; while it has never been on, every
 * launched kernel is the one of an engine without the feature.
 * A node may carry a STATUS for the player to move there: WIN (+1), DRAW (0), LOSS (-1), or none.  The EDGE VALUE e(Y, s) of child slot s of
 * node Y, for Y's mover: +1 for a winning terminal move (edge code -3), 0 for a drawing one (-2), -status(X) for an expanded child X with a
 * status, unknown otherwise.
 *   1. Sources.  A terminal parent (root or not) is a WIN if one of its children is a winning move, else a DRAW — in these games a drawing move
 *      exists only when it is the only legal move, so nothing legal was dropped.  That status is derived from the record, never stored: it holds
 *      for terminal parents made while the solver was off.
 *   2. Propagation starts only when an expansion has just created a terminal parent below (Y, s), after that creation's ordinary backup: along
 *      the simulation's own path from its deepest node up to the root, a node Y without a status becomes a WIN if some edge is +1; else, if all
 *      its n_actions children are expanded and every edge value is known, a DRAW if some edge is 0, else a LOSS; otherwise the walk stops.  A newly
 *      proven Y is written and the walk goes on to its parent.
 *   3. Selection leaves slots whose edge value is -1 out of the PUCT argmax (the score is unchanged, the first un-popped slot still wins among
 *      the un-popped ones).  If the chosen slot has a known edge value the simulation ends there as a PROVEN HIT: the path includes that edge, the
 *      edge value is backed up with one visit in the sign convention of a terminal-leaf hit, no random variate is drawn, and it counts as an
 *      evaluation-free simulation.  A non-root terminal parent is thus never entered.  With forced playouts a -1 slot is never owed.  (Only edge
 *      value 0 can be met this way in a tree searched with the solver on throughout.  Under terminal parents made while it was off a known +1 or -1
 *      edge can be chosen as well — it is backed up the same way —, and a node all of whose slots are left out takes slot 0.)
 *   4. A move also ends as soon as the root has a status and every root child has a visit; that may hold when the move begins (a re-rooted
 *      proven subtree, a terminal-parent root): the move then runs 0 simulations.
 *   5. Move and policy row.  Candidate slots C: root WIN — the slots with e = +1; DRAW — those with e = 0; LOSS — all; no status — those with
 *      e != -1 and N > 0 (all slots if there are none).  The policy row is the counts it would be without the solver (N, or the pruned counts of
 *      a forced-playouts move) restricted to C: f32(n_i / sum over C) on C, 0 elsewhere; left as it was if that sum is 0.  Root WIN or DRAW: the
 *      move is the slot of C with the most visits, lowest slot on ties, whatever tau says; otherwise the tau-0 argmax / tau sampling runs with the
 *      weights of slots outside C set to 0.  The move variate is drawn and the event counter advances as without the solver.  q is the exact
 *      +1 / 0 / -1 as f32 when the root has a status, else W / N of the chosen child.  Root N / W / P rows, root_visits and evals stay raw
 *      (gaz_engine_get_root_stats' out_policy and out_q follow this rule).  Such a ply's move_kind has 0x40 set.
 *   6. Proofs are about the game's rules; max_actions is no part of them.  Statuses live in the tree: they survive re-rooting and compaction and
 *      die with create_new_root; the two trees of a game prove independently.
 * Follow-up, refused today: the Gumbel search, leaf_batch > 1, gumbel_batch > 1. */
int gaz_engine_set_solver(gaz_engine* h, int32_t mode);
int gaz_engine_get_solver(gaz_engine* h, int32_t* mode);
/* a host synchronisation point; summed over game groups, over the engine's life: [0] nodes proven by propagation (terminal parents not counted),
 * [1] proven hits, [2] moves that ended with a proven root, [3] simulations those moves did not run (iteration limit - simulations done),
 * [4] / [5] / [6] of [2]: root WIN / DRAW / LOSS, [7] descent levels at which at least one slot was left out.  All 0 while never switched on. */
int gaz_engine_get_solver_stats(gaz_engine* h, uint64_t out[8]);

/* place one slot at the position reached by `n` actions from the empty board (new roots are built there).  The game keeps its
 * game_seq, the next player follows from the parity of n, both trees start fresh (event counter 0), and the tau schedule, the
 * last-moves input planes and the max_actions cap count the prefix: the game ends by the cap at ply max_actions, so n must be
 * below max_actions (refused otherwise).  No opening override for n > 0.  The drained record of that game spans all plies from
 * the empty board: T counts the prefix, actions[0, n) are the prefix and every per-move field of rows [0, n) (policy, q, root
 * N / W / P, root visits, evaluator calls) is 0 — no search ran there.  Their move_kind is 0, and they keep their training rows — which tells them
 * from the prefix of an opening book (gaz_engine_set_opening_book, kind 3). */
int gaz_engine_set_position(gaz_engine* h, int32_t slot, const int32_t* actions, int32_t n);
/* iteration_limit of the following MCTS.run calls (<= 0: unchanged); tau_mode -1 = Self_Play schedule, 0 / 1 = fixed tau */
int gaz_engine_set_search_params(gaz_engine* h, int32_t run_iterations, int32_t tau_mode);
/* MCTS.update_hyperparams / MCTS_Gumbel.update_hyperparams for every tree of the engine (see gaz_search_hyperparams) */
int gaz_engine_set_hyperparams(gaz_engine* h, const gaz_search_hyperparams* hp);
/* Resignation in self-play, with games played out to calibrate it (no reference counterpart).  Legal on any engine
 * and at any time; takes effect at the next launch, like gaz_engine_set_hyperparams.  threshold = 0 = off, the state of a new engine (the
 * other fields are then ignored).  With threshold in (0, 1): after ply p (0-based) of a game that goes on — natural ends and the
 * max_actions cap take precedence — the rule triggers iff p >= min_ply, p >= 2 (consecutive - 1) and for i in 0 .. consecutive-1 ply
 * p - 2i was searched ((move_kind & 3) != 0) and its recorded q, the float widened to double, is < -threshold: the mover's last
 * `consecutive` searched plies all saw the game as lost.  A ply without a search (a gaz_engine_set_position prefix, a host move on an idle
 * slot) breaks a run; fast plies of the playout cap count like full ones.  A game is a PLAY-OUT game iff the uniform variate (tree 2,
 * event 0, purpose 6) of its (seed, slot, game_seq) is < no_resign_prob; no other variate is drawn and no search changes, so a game's
 * record with resignation on is a prefix of its record with it off.
 *   trigger, not a play-out game: the game ends after ply p, the move played and recorded: hdr = [p + 1, -mover, slot, game_seq],
 *                                 move_kind[p] |= 0x10, game_stats count it like any other game
 *   trigger, play-out game:       move_kind[p] |= 0x20 and the game goes on
 * The value target of a record is z[p] = mover(p) * winner (the winner of a resigned game is not its last mover).
 * Refused (last_error): a struct_size other than sizeof(gaz_resign_params); threshold NaN, infinite, negative or >= 1; consecutive outside
 * [1, 8]; min_ply < 0; no_resign_prob NaN or outside [0, 1]. */
typedef struct {
    uint32_t struct_size;         /* = sizeof(gaz_resign_params) */
    int32_t consecutive;          /* 1 .. 8 */
    int32_t min_ply;              /* >= 0 */
    int32_t reserved_;
    double threshold;             /* 0 = off, else in (0, 1) */
    double no_resign_prob;        /* in [0, 1]: the share of games played out (AlphaGo Zero: 0.1, false positives kept under 5 %) */
} gaz_resign_params;
int gaz_engine_set_resignation(gaz_engine* h, const gaz_resign_params* p);
/* counters over the engine's life, summed over the game groups; a host synchronisation point like gaz_engine_get_stats:
 * [0] games ended by resignation, [1] of them resigned by player -1, [2] by player 1, [3] play-out games finished, [4] of those with a
 * would-have-resigned ply, [5] of those false positives (the would-be resigner of the FIRST such ply drew or won), [6] plies of the
 * resigned games (sum of T), [7] 0 */
int gaz_engine_get_resign_stats(gaz_engine* h, uint64_t out[8]);

/* OPENING BOOK: games that start from book positions, paired for matches (no reference counterpart).  No struct changes and
 * GAZ_ENGINE_ABI_VERSION stays 10: the feature is detected by its symbols.
 * The book is a table of n_entries action sequences, actions[i * stride + k] = ply k of entry i as an action index (the encoding of
 * gaz_engine_set_position / gaz_engine_read_positions), entry i having lengths[i] plies, 0 <= lengths[i] <= stride.  A length of 0 is "start
 * on the empty board": a book that is half empty entries starts half the games from the book, so there is no probability parameter.  The engine
 * keeps a copy in device memory (every game group one of its own); mode = 0 or n_entries = 0 removes the book.
 * RULE, stateless, a function of the game's identity.  Game (slot, game_seq) — slot = the global slot, as in the record header — draws
 *   u   = the uniform variate of (seed, slot, key_seq, tree 3, event 0, purpose 4)     key_seq = game_seq in mode 1, game_seq & ~1 in mode 2
 *   idx = min((int)(u * n_entries), n_entries - 1)                                       (float64)
 * Tree 3 is the book's stream alone: no other variate changes and no tree's event counter moves.  In mode 2 the games (slot, 2k) and
 * (slot, 2k + 1) — with match play the two colour assignments of one pairing — start from the same entry; everything else about them differs as
 * before (their streams are keyed by game_seq).  The rule survives gaz_engine_repack, game groups, slot_offset and first_game_seq.
 * It applies to every game that STARTS after the call — the first game of a slot when set before the first run, the next game of a slot in
 * continuous mode, a game after gaz_engine_reset_games — in sync and continuous mode, PUCT and Gumbel, on every engine configuration.
 * gaz_engine_set_position does not start a game and stays as it is.  A game that starts while a book is set is started by a kernel of its own
 * in front of the next tree step (one wave later than without a book; results do not depend on it).
 * A game started from entry e of length n is what gaz_engine_set_position(e, n) makes of a slot: the prefix on the board, the next player from
 * the parity of n, both trees fresh (event counter 0), and the tau schedule, the last-moves planes and the max_actions cap count the prefix.  No
 * opening override for n > 0; for n = 0 the game is byte for byte the game without a book, opening_actions included.  Its record carries the
 * prefix in actions[0, n), zeros in every per-move field of rows [0, n), and move_kind[0, n) = 3.  A ply of kind 3 gives NO training row
 * (gaz_engine_drain_samples / drain_samples2: kinds 2 and 3 are left out alike; a kept row's state still shows every prefix move), takes no part
 * in the surprise weighting (neither the means nor the rows), and breaks a resignation run as kind 0 does.
 * Refused, each with its own last_error text, the book in force staying as it was: a struct_size other than sizeof(gaz_book_params); a mode
 * outside 0 .. 2; n_entries < 0 or above 2^20; stride < 1 or above the game's max_T; null pointers with n_entries > 0; a length outside
 * [0, stride]; and — found by a kernel that replays every entry with the search's own rules, the first bad entry named with its ply — an illegal
 * move, an entry after one of whose plies (the last included) the game is won or drawn, a length that is not below max_actions. */
typedef struct { uint32_t struct_size; int32_t n_entries, stride, mode; } gaz_book_params;   /* mode 0 off, 1 per game, 2 per pair */
int gaz_engine_set_opening_book(gaz_engine* h, const gaz_book_params* p, const uint8_t* actions /* [n_entries][stride] */, const int32_t* lengths /* [n_entries] */);
int gaz_engine_get_opening_book(gaz_engine* h, int32_t* n_entries, int32_t* mode);      /* the book in force: 0, 0 = none */
/* a host synchronisation point.  counts[i] (n_entries of the book in force; may be NULL without one) = the games started from entry i since
 * that book was set — a device atomic per entry, summed over game groups; a new book starts its counters at 0.  Over the engine's life:
 * out[0] = games started with a book set, out[1] = prefix plies placed; out[2..7] = 0. */
int gaz_engine_read_book_counts(gaz_engine* h, uint64_t* counts, uint64_t out[8]);
/* MCTS.run(time_limit=...) (MCTS.py:528-563): stop != 0 makes every running search finish its move at the next launch, as the
 * reference's `time.time() - start_time < time_limit` test does between iterations; stop = 0 re-arms.  The host owns the clock. */
int gaz_engine_stop_search(gaz_engine* h, int32_t stop);

/* sync + single_tree engines idle after set_position / apply_moves; this starts MCTS.run for the idle slots */
int gaz_engine_start_search(gaz_engine* h);

/* Game-rules probe: n_positions positions, each given as n_actions[p] action indices (row p of actions[n_positions][stride]) played
 * from the empty board, first mover = -1.  The DEVICE rule code the search uses answers, per position: board int8 [H*W]; legal
 * uint8 [A] mask (get_legal_actions_MCTS); winner = check_win_MCTS after the last action (-2 running, -1 / 1 winner, 0 draw; -99 =
 * the history was not legal); input int8 [H*W*C] (get_input_state_MCTS); terminal int32 [A]: -1 not terminal, 1 the move wins, 0 it
 * draws (get_terminal_actions_fn, MCTS.py:247-294; all -1 for a finished position); and, when policy_in f32 [n][A] is given,
 * policy_out f32 [n][A] = get_legal_actions_policy_MCTS(..., normalize=True): policy at the legal actions / their sum, 0 elsewhere.
 * Output pointers may be NULL.  Reference: the static *_MCTS methods of the Game plugin (Guide.py:135-283), Game_Tester.py:297-405. */
int gaz_engine_probe_rules(gaz_engine* h, const int32_t* actions, const int32_t* n_actions, int32_t n_positions, int32_t stride,
                           int8_t* board, uint8_t* legal, int32_t* winner, int8_t* input, int32_t* terminal,
                           const float* policy_in, float* policy_out);

/* Math probe: the device's bit-exact arithmetic (csrc/det.hpp, the PUCT factors and scores, numpy's pairwise sum, the Gumbel softmax /
 * compute_pi / deterministic selection), one function per op on n_items inputs of the caller, answered by the functions the search kernels
 * call.  Everything is 64-bit words: item i reads in[i * in_words ...] and writes out[i * out_words ...]; a float64 is its bit pattern,
 * a float32 / uint32 the low half of its word; nothing is formatted or rounded.  The ops, their words and the team shapes are listed at
 * the top of csrc/det_probe.hpp (DP_*); counts an item carries are checked on the host.  The engine's games are not touched.  A library
 * without this symbol predates it (GAZ_ENGINE_ABI_VERSION is unchanged: no struct changed). */
int gaz_engine_probe_det(gaz_engine* h, int32_t op, int32_t n_items, const uint64_t* in, int32_t in_words, uint64_t* out, int32_t out_words);

/* run the built-in evaluator on a host batch: inputs int8 [n][H*W*C] -> policy f32 [n][A], value f32 [n]; n <= n_games */
int gaz_engine_evaluate(gaz_engine* h, const int8_t* inputs, int32_t n, float* policy, float* value, int32_t repeats, double* ms_per_batch);

/* diagnostics for the numerics tests: the flat head features the last gaz_engine_evaluate left in HBM — for the Connect4 network
 * relu(bn0(conv3x3(x) + b)) of the policy and the value head, f32 [n][H*W*8] each (Connect4/Build_Model.py:41-47,62-66), i.e. the
 * output of stem + every residual block + the heads' first convolution.  *_row_floats receive the row length; p / v may be NULL. */
int gaz_engine_read_head_features(gaz_engine* h, int32_t n, float* p_feat, float* v_feat, int32_t* p_row_floats, int32_t* v_row_floats);

int gaz_engine_record_layout(gaz_engine* h, gaz_record_layout* out);
/* finished games as records (gaz_record_layout).  With forced_playouts_k > 0 the policy rows (off_policy) of full moves are the pruned
 * targets; the root N / W / P rows (off_N / off_W / off_P), q and root_visits are the raw search statistics, forced visits included */
int gaz_engine_drain_finished(gaz_engine* h, void* out, int32_t max_records, int32_t* n_out);

/* Finished games as TRAINING SAMPLES, built on the device from the same ring gaz_engine_drain_finished empties: the arrays
 * Self_Play.play() collects and augments for the replay file (Self_Play.py:159-175; augment_sample, Guide.py:255-283 —
 * Connect4.py:442-443 [identity, np.fliplr], Gomoku.py:265-303 / Tictactoe.py:321-358 the 8 symmetries in the reference's order).
 * A ply whose search was a fast one (move_kind 2, gaz_engine_config.fast_iterations) gives no row, nor does a ply of an opening-book prefix
 * (move_kind 3, gaz_engine_set_opening_book); with the cap off and no book every ply does.  For the
 * R = sum of the KEPT rows of the games taken, row = games in the order handed out, kept plies in order (a kept row is what it would be
 * without the cap: its state shows every move played before it, fast ones included):
 *   boards   int8 [n_aug][R][state_bytes]   get_input_state() before the move ([H][W][C]), augmented
 *   policies f32  [n_aug][R][A]             the improved policy of the ply, same augmentation
 *   values   f32  [R]                       0.5 * (z + q)  (the replay file repeats it per augmentation)
 *   games    int32 [n][6]                   T (every ply played), winner, slot, game_seq, first row of the game, plies left out (the game has
 *                                           T - that many rows)
 * The augmentation planes of the caller's arrays are max_rows rows apart (plane k of boards starts at boards + k * max_rows *
 * state_bytes), so they are allocated once: boards n_aug * max_rows * state_bytes bytes, policies n_aug * max_rows * A floats, values
 * max_rows floats, games 6 * max_games ints.  Games leave the ring oldest first, as many WHOLE games as fit in max_games and max_rows;
 * the rest stays for the next call (max_rows, *n_rows and the rule below count kept rows).  The call may be mixed with gaz_engine_drain_finished: a game is
 * handed out once, by either.  An oldest game with more rows than max_rows is an error (last_error says so); max_rows >= max_T always makes progress.  ring_capacity = 0:
 * nothing to drain.  Rows of a gaz_engine_set_position prefix carry the zeros of their record (policy, q).  With game groups the groups'
 * rings are visited in turn, as drain_finished does.  A host synchronisation point like gaz_engine_drain_finished.
 * With forced_playouts_k > 0 `policies` carries the pruned targets: the kernel reads the record's policy rows as move_end wrote them. */
typedef struct { int32_t n_aug, state_bytes, A, max_T; } gaz_sample_layout;
int gaz_engine_sample_layout(gaz_engine* h, gaz_sample_layout* out);
int gaz_engine_drain_samples(gaz_engine* h, int32_t max_games, int64_t max_rows,
                             int32_t* games, int8_t* boards, float* policies, float* values,
                             int32_t* n_games, int64_t* n_rows);

/* POLICY SURPRISE WEIGHTING of the training rows (KataGo, Wu 2019, section 3.3; DESIGN.md "Policy surprise weighting"; no reference
 * counterpart).  A game's row weight — one row per fully searched ply — is redistributed towards the plies whose search policy differs most
 * from the prior; fast plies (playout cap randomisation) that surprise enough earn rows too; a weight becomes an integer number of rows by
 * stochastic rounding.  PUCT records only.  No struct changes and GAZ_ENGINE_ABI_VERSION stays 10: the feature is detected by its symbols
 * (gaz_engine_set_sample_weighting, gaz_engine_get_sample_weighting, gaz_engine_drain_samples2).
 * The rule is stateless — a function of one finished record, (lambda, fast_factor) and gaz_engine_config.seed.  For ply p of a record with T
 * plies, kind = move_kind[p] & 3, pi_p = the record's policy row (the pruned target with forced playouts), P_p = the record's P row: the
 * priors the root searched with, Dirichlet noise included when it is on — the only prior a record keeps:
 *   1  surprise  s_p = max(0, sum over a ascending of (double)pi_p[a] * (dlog((double)pi_p[a]) - dlog((double)P_p[a]))), only terms with
 *      pi_p[a] > 0 and P_p[a] > 0, a sequential float64 sum in that order with the engine's dlog (csrc/det.hpp); NaN or infinite counts as 0
 *   2  base weight  w0_p = 1 for kind 1 (full), 0 for kind 2 (fast).  A ply of kind 0 (a gaz_engine_set_position prefix) keeps exactly one
 *      row, as without the mode, and takes no part in anything below
 *   3  n_full = the number of full plies, mean = (sum of s_p over the full plies, in ply order) / n_full; a fast ply is eligible iff
 *      s_p > fast_factor * mean; E = the full plies and the eligible fast plies; S = the sum of s_p over E, in ply order
 *   4  w_p = (1 - lambda) * w0_p + lambda * n_full * s_p / S on E (evaluated left to right), 0 elsewhere; w_p = w0_p if n_full == 0 or S is
 *      0 or not finite.  The game's weight is conserved: sum w_p == n_full up to rounding
 *   5  rows  c_p = floor(w_p) + (u_p < w_p - floor(w_p)), u_p = the uniform variate of (seed, the record's slot, its game_seq, tree 2,
 *      event 0x40000000 + p, purpose 5 = the playout cap's): all 32 bits of the event enter the Philox counter, so it collides with no other
 *      draw (the cap's own uses event p), and no tree's event counter moves
 *   6  a game's rows stay one contiguous range, in ply order, the c_p copies of a ply adjacent.  A row is byte for byte what that ply's row is
 *      without the mode — for a fast ply what it would be with the cap off: the board shows every earlier move, the value is 0.5 * (z + q[p]).
 *      A game has at most n_full + |E| <= 2 * T rows
 * lambda in [0, 1]: 0 = off, the state of a new engine (KataGo uses 0.5); with lambda == 0 every output is what it is without the mode, byte
 * for byte.  fast_factor > 0, finite (default 1.5).  Legal at any time; it takes effect at the next drain.  Refused, with its own text, on an
 * engine with the Gumbel search, for lambda outside [0, 1] or NaN, and for fast_factor <= 0, NaN or infinite.
 * With the mode on, for gaz_engine_drain_samples and gaz_engine_drain_samples2: games[i][5] is the number of plies that gave no row; a game's
 * rows are the difference of successive games[i][4], *n_rows closing the last one; max_rows >= 2 * max_T always makes progress, and an oldest
 * game with more rows than max_rows is the same error as before.
 * gaz_engine_drain_samples2 = gaz_engine_drain_samples plus row_ply (u8 [max_rows], may be NULL): the ply of every row, mode on or off. */
int gaz_engine_set_sample_weighting(gaz_engine* h, double lambda, double fast_factor);
int gaz_engine_get_sample_weighting(gaz_engine* h, double* lambda, double* fast_factor);
int gaz_engine_drain_samples2(gaz_engine* h, int32_t max_games, int64_t max_rows,
                              int32_t* games, int8_t* boards, float* policies, float* values, uint8_t* row_ply,
                              int32_t* n_games, int64_t* n_rows);

int gaz_engine_get_stats(gaz_engine* h, uint64_t out[16]);  /* [0..5] game_stats, [6] evaluator calls, [7] simulations,
                                                               [8] plies played (= positions, incl. games in progress), [9] waves launched,
                                                               [10] evaluations answered by the evaluation cache, [11] groups of the group pipeline (0 = off),
                                                               [12] 1 = tree step and trunk kernel run as ONE fused launch,
                                                               [13] trunk workgroups of fused launches that gave up waiting for their games (see
                                                                    gaz_engine_debug_fused_fault); non-zero = the engine has fallen back to separate launches ([12] says whether it still is: the
                                                                    one-launch form is tried again after 20000 waves, at most twice),
                                                               [14] game groups (gaz_engine_config::game_groups as resolved; 0 = one batch): with groups, [0] (the longest
                                                                    game) is the maximum over the groups, [1..8], [10], [13] are sums over the groups and [12] says that every
                                                                    group runs the one-launch form,
                                                               [15] leaf_batch > 1: reserved children (leaves in flight) summed over every node of every tree — 0 whenever
                                                                    every game waits for the host or has ended: a move never ends with a leaf in flight */
int gaz_engine_synchronize(gaz_engine* h);

/* Connect4 PUCT with the ResNet evaluator runs the tree step and the trunk kernel of a wave as ONE launch (k_wave_trunk: the trunk
 * starts on the boards whose games are done while the slow games still search); on = 0 launches them separately (same results bit
 * for bit; bench.py uses it to time the trunk kernel on its own).  Scheduling only. */
int gaz_engine_set_fused_wave(gaz_engine* h, int32_t on);

/* The fused launch hands leaf rows from tree blocks to trunk workgroups INSIDE one running kernel, which assumes that the tree blocks (lowest
 * block indices) become resident before the trunk workgroups that wait for them — HIP promises no dispatch order.  The wait is therefore
 * bounded (20 ms): a trunk workgroup that runs out of time leaves its boards unevaluated and marks them, the games keep their requests
 * pending and are evaluated by the next wave (no result changes), and at its next synchronisation point (synchronize, get_stats,
 * drain_finished) the engine switches to separate launches (get_stats [13] counts the workgroups that gave up) — for 20000 waves, then the one-launch
 * form is tried again; after the third give-up for good.  This hook makes every trunk workgroup with index % mod == 1 behave
 * as if its wait had timed out (mod = 0: off), so that the recovery path can be tested where the assumption holds. */
int gaz_engine_debug_fused_fault(gaz_engine* h, int32_t mod);

/* Continuous self-play with a games_budget: towards the end of a generation more and more slots have played their last game, but a
 * wave still steps and evaluates every slot.  repack moves the games that still run into the lowest slots (tree arena slice, records,
 * pending evaluator rows; a game keeps its identity) and shrinks all later launches to them.  *n_active = games still running,
 * *n_launch = slots the launches cover from now on.  Results do not change.  (The reference's counterpart is simply that finished
 * worker processes stop asking the inference server, Self_Play.py:380-400.)
 * After a repack a PHYSICAL slot index no longer identifies a game (records carry the game's own slot id): gaz_engine_set_position and
 * gaz_engine_reset_games with a slot list are refused from then on; gaz_engine_reset_games(h, NULL, 0) restarts every slot and makes the
 * launches cover all of them again.  The batch-level calls (read_batch / write_outputs / get_root_stats) keep addressing physical rows. */
int gaz_engine_repack(gaz_engine* h, int32_t* n_active, int32_t* n_launch);

/* The action history of every slot's game in progress — game.action_history of the reference's Game objects, as action indices; what
 * gaz_engine_set_position takes.  n_hist int32 [n_games] (0 for a halted slot), hist uint8 [n_games][stride] with stride >= the game's
 * max_T (gaz_record_layout.max_T): row g starts at hist + g * stride, and its bytes past the history are 0.  Synchronises the engine's stream.  bench.py draws its staggered start from it. */
int gaz_engine_read_positions(gaz_engine* h, int32_t* n_hist, uint8_t* hist, int32_t stride);

/* ---- reading search trees back (DESIGN.md "Reading search trees back") ----------------------------------------------------------------
 * A CANONICAL export of the tree below a slot's current root: it depends on the tree alone, never on where the engine keeps its node
 * records.  Nodes come in breadth-first order from the root — parents in export order, the children of a node in slot order — and every
 * exported node contributes one edge record per child slot [0, n_actions), in slot order, nodes in export order.  Export index 0 is the
 * root (parent = -1, slot = 0, depth = 0), whatever the engine's record says after a re-root.  Only what is reachable from the current
 * root is exported.  Read-only: no search state changes. */
typedef struct {                  /* 48 bytes */
    int32_t parent;               /* export index of the parent, -1 for the root */
    int32_t slot;                 /* child slot in the parent (child_id, MCTS.py:32); 0 for the root */
    int32_t depth;                /* 0 for the root */
    int32_t edge0;                /* index of the node's first edge within this tree's edge range; its edges are [edge0, edge0 + n_actions) */
    int32_t n_actions;            /* len(child_visits) */
    int32_t n_children;           /* PUCT: len(children), the expanded prefix of the slots.  Gumbel search: the count of a terminal parent, else 0
                                     (children are expanded in any order there; an edge's `child` says whether it is) */
    int32_t flags;                /* bit 0: terminal parent — every child ends the game (edge codes -2 / -3); bits 1-2: the status the solver proved
                                     for the player to move here (gaz_engine_set_solver): 0 unknown, 1 win, 2 draw, 3 loss.  A terminal parent's
                                     status is not stored: it is a win if one of its edges is -3, else a draw */
    int32_t n_reserved;           /* leaf_batch > 1: children reserved and not yet applied (leaves in flight), slots [n_children, n_children + n_reserved) */
    int32_t player;               /* current_player: who moved into this position (-1 / 1) */
    int32_t action;               /* action_history[-1] as an action index (0 at the empty board) */
    int32_t n_hist;               /* len(action_history) */
    int32_t reserved_;            /* 0 */
} gaz_tree_node;
typedef struct {                  /* 24 bytes */
    int32_t action;               /* the slot's action index */
    uint32_t N;                   /* child_visits (with leaf_batch > 1: virtual losses of leaves in flight included) */
    float W;                      /* child_values */
    float P;                      /* child_prob_priors; Gumbel search: the raw logit */
    float raw;                    /* Gumbel search: child_raw_values (the evaluator's value of the expanded child); PUCT: 0 */
    int32_t child;                /* >= 0: export index of the child node; -1 not expanded; -2 the move draws, -3 it wins (terminal children have no
                                     node); -4: the child has a node that max_depth / min_visits left out of this export */
} gaz_tree_edge;
enum { GAZ_TREE_CHILD_NONE = -1, GAZ_TREE_CHILD_DRAW = -2, GAZ_TREE_CHILD_WIN = -3, GAZ_TREE_CHILD_FILTERED = -4 };

/* The trees of `n_slots` slots (any order, repeats allowed) into the caller's arrays, tree after tree in the order of `slots`: tree i has the
 * nodes [node_first[i], node_first[i + 1]) and the edges [edge_first[i], edge_first[i + 1]).  tree = 0 / 1: that tree of the game; -1: the
 * tree running the game's current move (a single_tree or Gumbel engine has tree 0 only: tree = 1 is refused).  A tree without a root exports
 * nothing.  max_depth < 0: no limit, else nodes deeper than max_depth are left out; a child node is exported only if its edge has
 * N >= min_visits; the root always is.
 * nodes == NULL and edges == NULL: only node_first / edge_first are filled (the counts) — the first call of the usual two.  Otherwise both
 * arrays are required, and max_nodes / max_edges below the totals is an error: last_error names the needed counts, node_first / edge_first
 * are filled and nothing is written to nodes / edges.
 * A host synchronisation point like gaz_engine_get_root_stats, legal at any time: between the waves of continuous self-play, and in the
 * middle of a leaf_batch / gumbel_batch move (n_reserved then shows the leaves in flight).  With game groups the slots are forwarded to their
 * groups and the results come back in the caller's order; after gaz_engine_repack slots are physical. */
int gaz_engine_read_trees(gaz_engine* h, const int32_t* slots, int32_t n_slots, int32_t tree, int32_t max_depth, uint32_t min_visits,
                          int64_t max_nodes, int64_t max_edges, gaz_tree_node* nodes, gaz_tree_edge* edges,
                          int64_t* node_first /* [n_slots + 1] */, int64_t* edge_first /* [n_slots + 1] */);
/* The principal variation of every slot: from the root, follow the edge with the most visits (ties: the lowest slot).  first_action
 * (NULL, or per game; < 0 = most visited) names the first step instead — the move a finished search chose: sequential halving ends with
 * two equally visited candidates, so "most visited" is not always the move played.  Step k of game g: actions / N / W [g * max_len + k] =
 * the edge's action, visits and value sum; entries from len[g] on are 0.  The line ends after an edge whose child is terminal, is not
 * expanded or has N = 0, at max_len, and before a node without children; a first_action the root does not have gives len 0.
 * Synchronisation and slot rules as for gaz_engine_read_trees. */
int gaz_engine_read_pv(gaz_engine* h, int32_t tree, const int32_t* first_action /* [n_games] or NULL */, int32_t max_len,
                       uint8_t* actions, uint32_t* N, float* W /* [n_games][max_len] each */, int32_t* len /* [n_games] */);

/* measurement hooks (bench.py): HIP-event timing of the kernels launched on the engine's stream */
int gaz_engine_timing_reset(gaz_engine* h, int32_t enable);
/* the kernel priced against the roofline: its name (copied into `name`) and the algorithmic FLOPs of one launch */
int gaz_engine_dominant_kernel(gaz_engine* h, char* name, int32_t cap, double* flops_per_launch);
/* sums over the TIMED waves (run_waves brackets every 8th wave: an event record costs a barrier packet): tree-kernel ms, evaluator
 * ms, ms and launch count of the dominant kernel, number of timed waves.  With game groups (gaz_engine_config::game_groups) the ms are sums
 * over the groups' launches — which overlap in time, so they are kernel time, not wall clock — and gaz_engine_dominant_kernel prices ONE group's
 * launch; a per-kernel roofline is measured on an engine with game_groups = 1 (bench.py does) */
int gaz_engine_timing_get(gaz_engine* h, double* ms_tree, double* ms_eval, double* ms_dominant, int64_t* n_dominant, int64_t* n_waves);

/* ---- REPLAY WINDOW: the training rows of the last generations on the device, served as shuffled, augmented minibatches.
 * Replaces the reference's Dataloader.py (split(): :68-145, the per-row batch copy: :178-189).  A handle of its own, because a window outlives
 * the engines of several generations.  No existing entry point or struct changes and GAZ_ENGINE_ABI_VERSION stays 10: the feature is detected by
 * its symbols (gaz_replay_create).  One host thread per window; every call returns 0 or non-zero with gaz_replay_last_error's text.
 * STORE.  A circular store of capacity_rows rows: state int8 [state_bytes], policy f32 [A], value f32 — un-augmented, the sizes of
 * gaz_sample_layout — plus the row's game and its row within the game.  The STORE ORDER numbers the live rows from 0 = the oldest.  The host
 * keeps the game table: generation, index of the game within its generation in append order, first row, rows.
 * RULES, stateless functions of the window's contents and its seed.  ph(c0, c1, c2, c3) = Philox4x32-10 (csrc/det.hpp) with the key (low, high 32
 * bits of seed ^ 0x5245504C41590000); u52(x, y) = the mapping of gaz::det::uniform, ((x >> 6) << 26 | (y >> 6)) / 2^52, of the first two output
 * words.  A row is (g, i, j) = (generation, game within g in append order, row within the game): no rule depends on where a row sits in the
 * ring, so a window refilled from the replay files draws what the live one drew.
 *   1  held-out   the row is held out iff u52(ph(g, i, j, 0x80000000)) < test_fraction; membership never changes
 *   2  admission  the reference's parity rule (Dataloader.py:90-105), on the host at begin_epoch: generations newest to oldest starting at
 *      newest_generation, games in append order, counters f = s = 0; a game is "first" iff its row count is odd; ratio = f + s == 0 ? 0.0 :
 *      f / (f + s); a first game is skipped iff ratio - 0.02 > target_ratio, else f += 1; any other game is skipped iff ratio + 0.02 <
 *      target_ratio, else s += 1.  target_ratio NaN: every game is admitted.  Known blind spots of the parity: a draw on a board with an odd
 *      number of cells counts as a first-player win, a resigned game has the parity of the resigner's last ply, and a game thinned by the
 *      playout cap, the surprise weighting or a book prefix has whatever parity its rows are left with
 *   3  inclusion  a = newest_generation - g (rows with g > newest_generation are out), p = max(percent - (double)a * decay, 0.0) — linear, as
 *      Dataloader.py:134-138 is despite the name.  A row is in the PLAN iff its game is admitted, its held-out bit equals split and
 *      u52(ph(g, i, j, 0x40000000 | epoch)) < p.  The plan lists the included rows in store order; M is their count
 *   4  order      position q of the epoch is plan entry perm(q): h = the smallest value >= 1 with 4^h >= M, mask = 2^h - 1; x = q, then repeat
 *      until x < M: (L, R) = (x >> h, x & mask); for r = 0 .. 3: (L, R) = (R, L ^ (ph(R, r, epoch, 0xC0000010 | split)[0] & mask));
 *      x = (L << h) | R.  An exact permutation of [0, M)
 *   5  symmetry   position q uses k = augment ? (ph(epoch, q, split, 0xC0000000)[0] * n_aug) >> 32 : 0; the sampled board and policy are plane
 *      k of gaz_engine_drain_samples for that row, byte for byte; the value is unchanged
 * Per-row independent draws replace the reference's exact-count np.random.choice; the expectations are the same, and a held-out row never
 * reaches a training plan. */
typedef struct gaz_replay gaz_replay;
typedef struct {
    uint32_t struct_size;         /* = sizeof(gaz_replay_config); gaz_replay_create rejects any other value */
    int32_t game;                 /* GAZ_GAME_* */
    int32_t device;               /* HIP device ordinal */
    int32_t reserved_;
    int64_t capacity_rows;        /* 1 .. 2^31 - 1 */
    uint64_t seed;
    double test_fraction;         /* in [0, 1) */
    double target_ratio;          /* NaN = no balancing, else in [0, 1] */
} gaz_replay_config;
int gaz_replay_config_size(void);
/* refused, each with its own text: a stale struct_size, an unknown game, capacity_rows outside its range, test_fraction outside [0, 1) or NaN,
 * target_ratio outside [0, 1] (NaN allowed), allocation failure */
int gaz_replay_create(const gaz_replay_config* cfg, gaz_replay** out);
void gaz_replay_destroy(gaz_replay* h);
const char* gaz_replay_last_error(gaz_replay* h);   /* h may be NULL: last create() error */
/* games int32 [n_games][6], boards, policies, values, n_rows: host arrays exactly as gaz_engine_drain_samples2 returns them; only augmentation
 * plane 0 is read (n_rows rows from the pointers on).  Game i has the rows games[i][4] - games[0][4] .. games[i + 1][4] - games[0][4], n_rows
 * closing the last one (0 rows is legal).  Generations must arrive in non-decreasing order.  If the rows do not fit, whole oldest generations
 * are evicted, never the one being appended to; a generation that alone exceeds capacity_rows is an error and leaves the window unchanged.
 * A host synchronisation point; drops the epoch's plan */
int gaz_replay_append(gaz_replay* h, int32_t generation, int32_t n_games, const int32_t* games, const int8_t* boards, const float* policies,
                      const float* values, int64_t n_rows);
int gaz_replay_evict(gaz_replay* h, int32_t before_generation);      /* every generation below it leaves; drops the plan */
/* out: [0] live rows, [1] live games, [2] oldest, [3] newest generation (-1: empty), [4] held-out rows among the live ones (counted on the
 * device), [5] capacity_rows, [6] generations, [7] rows of the current plan (-1: none).  generations (may be NULL) int64 [max_generations][3]:
 * generation, games, rows, oldest first; *n_generations (may be NULL) = their number */
int gaz_replay_info(gaz_replay* h, int64_t out[8], int32_t max_generations, int64_t* generations, int32_t* n_generations);
/* rows first .. first + n - 1 of the store order as stored; meta int32 [n][3] = generation, game within it, row within the game; any output may be NULL */
int gaz_replay_read_rows(gaz_replay* h, int64_t first, int64_t n, int8_t* boards, float* policies, float* values, int32_t* meta);
/* builds the plan of (split 0 train / 1 test, epoch < 2^30) on the device: a flag per row with per-block counts, a scan of the counts, a
 * compaction.  The host's part is the admission pass over the game table.  *n_rows = M.  A host synchronisation point */
int gaz_replay_begin_epoch(gaz_replay* h, int32_t split, uint32_t epoch, int32_t newest_generation, double percent, double decay, int64_t* n_rows);
int gaz_replay_read_plan(gaz_replay* h, int64_t first, int64_t n, uint32_t* rows);      /* plan entries (store-order rows), ascending */
/* positions first .. first + n - 1 of the current plan's order into the window's own output buffers (grown on demand), queued on the window's
 * stream.  first + n beyond the plan is an error; n = 0 is legal */
int gaz_replay_sample(gaz_replay* h, int64_t first, int32_t n, int32_t augment);
/* measurement hook (tools/replay_bench.py): the same batch `repeats` times between two HIP events on the window's stream, after one warm-up */
int gaz_replay_sample_timed(gaz_replay* h, int64_t first, int32_t n, int32_t augment, int32_t repeats, double* ms_per_batch);
/* device pointers of those buffers, valid until a later gaz_replay_sample has to grow them: boards int8 [n][H][W][C], policies f32 [n][A],
 * values f32 [n], source row (store order) u32 [n], symmetry u8 [n]; any pointer may be NULL */
int gaz_replay_batch_ptrs(gaz_replay* h, void** boards, void** policies, void** values, void** rows, void** sym);
/* the synchronising host copy of the last sampled batch; any pointer may be NULL */
int gaz_replay_read_batch(gaz_replay* h, int8_t* boards, float* policies, float* values, uint32_t* rows, uint8_t* sym);
int gaz_replay_synchronize(gaz_replay* h);

/* ---- HELD-OUT LOSS: what a network's predictions score on training rows, computed on the device (csrc/score.hpp).
 * Replaces the reference's validation pass — Train.py:46-57, model.fit(validation_data=...) with the losses of Net/Alpha_Loss.py or
 * Net/Gumbel_Loss.py and KL divergence as the metric — for the network self-play really runs: the engine's own evaluator with its imported
 * weights.  No existing entry point or struct changes and GAZ_ENGINE_ABI_VERSION stays 10: the feature is detected by its symbols
 * (gaz_engine_score_outputs).
 * THE RULE.  Everything is float64, out of operations the project pins bit for bit: no tolerance anywhere.  A row has a prediction P[A] (f32)
 * and v (f32), a target y[A] (f32) and z (f32), and is scored under a policy_mode: 0 = P are probabilities, 1 = P are logits of a softmax head,
 * 2 = P are Stablemax probabilities, 3 = P are logits of a Stablemax head; -1 = the engine's own (policy_is_logits 0 -> 0, 2 -> 2, 1 -> 1 or,
 * with gumbel_stablemax, 3).
 *   q          modes 0 and 2: q_a = (double)P_a as given, NOT renormalised.  Mode 1: x = (double)P, q = softmax(x) exactly as gumbel_core.hpp
 *              softmax_inplace: e_a = dexp(x_a + (-max x)), q_a = e_a / np.sum(e).  Mode 3: s_a = x_a >= 0 ? x_a + 1 : 1 / (1 - x_a),
 *              q_a = s_a / np.sum(s)
 *   ce         -np.sum_a(t_a), t_a = y_a > 0 ? (double)y_a * dlog(max(q_a, 1e-7)) : +0.0 — all A entries in action order, numpy's pairwise
 *              order (det::np_pairwise_sum<double>), dlog = det::dlog; 1e-7 is Keras' epsilon.  Each product is stored before it is summed
 *   entropy    -np.sum_a(y_a > 0 ? (double)y_a * dlog((double)y_a) : +0.0)
 *   se         d * d, d = (double)v - (double)z
 *   flags      bit 0 top1: argmax of the raw P == argmax of y, the lowest index among equals (the activations are monotone: the raw outputs
 *              decide); bit 1: z != 0 and v z > 0 (the exact product); bit 2: z != 0; bit 3 bad: some P_a or v is not finite
 *   bad rows   ce = entropy = se = 0 and only bit 3: they count in bad_rows and in nothing else.  Targets are taken to be finite
 * TOTALS over the M rows 0 .. M - 1 (epoch positions of a window, caller order of arrays): for block b, S_b = np.sum(x[128 b : 128 b + 128])
 * (det::np_sum_block) of ce, entropy and se; the total is the left-to-right float64 sum of S_0, S_1, .. on the host; the counts are integers.
 * The blocks follow the row index, never the evaluator batch, and the evaluator's rows are independent: the totals are the same bits for every
 * batch_rows.  The caller derives policy_loss = ce_sum / good, policy_kl = (ce_sum - entropy_sum) / good, value_loss = se_sum / good with
 * good = rows - bad_rows, top1 / good, value_sign / value_rows, and val_loss = policy_loss + value_loss (modes 0, 2) or policy_kl + value_loss
 * (modes 1, 3), as Train.py:33-48 pairs the losses.
 * DIFFERENCES FROM KERAS: float64 where Keras computes in float32; the prediction is not renormalised (Keras' categorical cross entropy divides
 * by its sum); y is not clipped (KLDivergence clips y to [1e-7, 1]). */
typedef struct {
    uint32_t struct_size;         /* = sizeof(gaz_score_totals), set by the caller; any other value is refused */
    int32_t policy_mode;          /* out: the mode the rows were scored under (0 .. 3) */
    int64_t rows, bad_rows, top1, value_rows, value_sign;
    double ce_sum, entropy_sum, se_sum;
} gaz_score_totals;
int gaz_score_totals_size(void);
/* replaces Net/Alpha_Loss.py / Net/Gumbel_Loss.py applied to given outputs: scores caller-supplied predictions (host arrays policy_pred f32
 * [n][A], value_pred f32 [n]) against targets (policy_target f32 [n][A], value_target f32 [n]).  Needs no evaluator, works on every engine
 * (game groups included) and touches no game.  policy_mode -1 .. 3 as above.  The per-row outputs (f64 [n] each, flags u8 [n]) may be NULL.
 * n = 0 gives zero totals.  A host synchronisation point on a stream of its own */
int gaz_engine_score_outputs(gaz_engine* h, const float* policy_pred, const float* value_pred, const float* policy_target, const float* value_target,
                             int64_t n, int32_t policy_mode, gaz_score_totals* totals, double* row_ce, double* row_entropy, double* row_se,
                             uint8_t* row_flags);
/* replaces the validation pass of Train.py:46-57: scores the engine's built-in evaluator (network A, also in match mode; the evaluation cache
 * is not consulted) on the window's CURRENT plan, positions 0 .. M - 1 of its order, batch_rows at a time, under the engine's own policy_mode.
 * Per batch: gaz_replay_sample on the window's stream, an event the engine's stream waits on, the forward pass straight from the window's
 * board buffer into buffers of the scorer's own (the games' pending outputs are not touched), k_score_rows against the window's policy and
 * value buffers, an event the window's stream waits on before its next gather.  Then k_score_blocks, ONE read-back and the host's sum: one
 * host synchronisation at the end, none per batch.  *ms_total (may be NULL): HIP-event time on the engine's stream from the first batch to the
 * block sums.  Refused, each by its text, leaving the engine and the window as they were: a wrong struct_size, game_groups > 1, a call
 * between gaz_engine_wave_begin and gaz_engine_wave_end, no built-in evaluator, weights not loaded, a window of another game or device, no
 * plan, batch_rows outside [1, gaz_engine_batch_rows].  M = 0 gives zero totals */
int gaz_engine_score_replay(gaz_engine* h, gaz_replay* window, int32_t batch_rows, int32_t augment, gaz_score_totals* totals, double* row_ce,
                            double* row_entropy, double* row_se, uint8_t* row_flags, double* ms_total);
/* measurement hook (tools/score_bench.py): the k_score_rows launch of the last gaz_engine_score_outputs call, `repeats` times between two HIP events */
int gaz_engine_score_rows_timed(gaz_engine* h, int32_t repeats, double* ms_per_launch);

/* ---- OPTIMIZER: the reference's chain Orthograd(Grokfast_EMA(Adam | Nadam)) (Train.py:25-31, Net/Optimizers/{ortho_grad,grok_fast,adam,nadam}.py)
 * as ONE multi-tensor step over flat arenas (csrc/optim.hpp).  A handle of its own, independent of any engine.  No existing
 * entry point or struct changes and GAZ_ENGINE_ABI_VERSION stays 10: the feature is detected by its symbols (gaz_optim_create).  One host thread
 * per object; every call returns 0 or non-zero with gaz_optim_last_error's text.  The kernels run on the device's default stream, in order with
 * whatever else the process queues there (PyTorch's default stream is that stream).
 * ARENAS.  Five flat f32 arenas of one layout: 0 params, 1 grads, 2 momentum, 3 velocity, 4 ema (only with grokfast).  Tensor k starts at
 * offsets[k] elements, offsets[0] = 0, offsets[k + 1] = offsets[k] + sizes[k] rounded up to a multiple of 4 (16 bytes); total = the end of
 * the last tensor, rounded likewise.  The pad elements are zero and stay zero.  Everything starts at zero.
 * ONE STEP, per tensor with params w, grads g and state m, v, e.  Every elementwise operation is f32 and rounded on its own (no fused
 * multiply-add), division and square root are the correctly rounded ones, denormals are kept.  The scalars are rounded to f32 once: lr, wd,
 * b1, b2, eps, alpha, lamb, 1 - b1, 1 - b2, 1 - alpha (each difference an f32 subtraction from 1.0f), c1 = (float)(1.0 - dpow(beta_1, t)), c2 =
 * (float)(1.0 - dpow(beta_2, t)) with dpow = det::dpow on doubles.
 *   1  decay      wd != 0:  w = w - (w * wd) * lr                                  (Keras' decoupled decay, before the update)
 *   2  orthograd  proj = f32(w.g) / (f32(w.w) + 1e-30f);  go = g - proj * w;  s = sqrt(f32(g.g)) / (sqrt(f32(go.go)) + 1e-30f);  g1 = go * s
 *   3  grokfast   e = e * alpha + g1 * (1 - alpha);  g2 = g1 + e * lamb
 *   4  adam       m = b1 * m + (1 - b1) * g2;  v = b2 * v + (1 - b2) * (g2 * g2);  u = (m / c1) / (sqrt(v / c2) + eps);  w = w - u * lr
 *      nadam      the same with the numerator (m / c1) * b1 + ((1 - b1) * g2) / c1
 *   5  zero_grads g = 0
 * (a stage that is off passes its input on: g1 = g, g2 = g1.)  THE DOT PRODUCTS w.g, w.w, g.g, go.go are float64 sums of the exact products of
 * f32 values, in a fixed order that depends on nothing but the tensor's size: the tensor is cut into CHUNKS of 2048 elements; in a chunk of
 * len elements with G = len / 4 whole groups of four, slot s (0 .. 255) adds, starting from +0.0, the elements of group s and then of group
 * s + 256 (those below G) in ascending order, and slot 0 then adds the len % 4 elements behind the last whole group; the 256 slot sums are
 * combined by six butterfly rounds x[s] = x[s] + x[s ^ d], d = 32, 16, 8, 4, 2, 1, and the chunk's sum is ((x[0] + x[64]) + x[128]) + x[192];
 * the tensor's sum is the chunks' sums added in ascending order starting from +0.0, rounded to f32 once by f32().
 * REFERENCE QUIRK, not reproduced: a wrapped Keras optimizer's update_step is called directly, so its iterations never advance (the bias
 * correction stays at t = 1) and its weight decay is never applied.  Here t is the caller's step number and the decay is applied. */
typedef struct gaz_optim gaz_optim;
typedef struct {
    uint32_t struct_size;         /* = sizeof(gaz_optim_config); gaz_optim_create rejects any other value */
    int32_t device;               /* HIP device ordinal */
    int32_t n_tensors;            /* >= 1 */
    int32_t kind;                 /* 0 Adam, 1 Nadam */
    const int64_t* sizes;         /* [n_tensors], each >= 1; read by create only */
    double beta_1, beta_2;        /* in [0, 1) */
    double epsilon, weight_decay; /* finite, >= 0 */
    int32_t orthograd, grokfast;  /* 0 / 1 */
    double alpha, lamb;           /* Grokfast's EMA factor and gain; finite */
} gaz_optim_config;
int gaz_optim_config_size(void);
/* refused, each with its own text: a stale struct_size, n_tensors < 1, a size < 1 (or a total of 2^40 elements and more), an unknown kind, a
 * beta outside [0, 1), epsilon / weight_decay / alpha / lamb not finite or a negative epsilon / weight_decay, allocation failure */
int gaz_optim_create(const gaz_optim_config* cfg, gaz_optim** out);
void gaz_optim_destroy(gaz_optim* h);
const char* gaz_optim_last_error(gaz_optim* h);     /* h may be NULL: last create() error */
/* offsets (may be NULL) int64 [n_tensors]; info: [0] total elements of an arena, [1] chunks, [2] elements per chunk, [3] kernel launches per step,
 * [4] 1 when the arenas are host memory (the one-lane test build), else 0 */
int gaz_optim_layout(gaz_optim* h, int64_t* offsets, int64_t info[5]);
/* the five device pointers (ema NULL without grokfast), valid for the object's life; any argument may be NULL */
int gaz_optim_ptrs(gaz_optim* h, void** params, void** grads, void** momentum, void** velocity, void** ema);
/* elements first .. first + n - 1 of arena 0 .. 4 (pads included) to / from n host floats.  A range past the arena, or arena 4 without grokfast,
 * is refused.  write leaves the pad elements inside the range zero whatever the caller passes.  Host synchronisation points */
int gaz_optim_read(gaz_optim* h, int32_t arena, int64_t first, int64_t n, float* out);
int gaz_optim_write(gaz_optim* h, int32_t arena, int64_t first, int64_t n, const float* in);
/* one step at learning rate lr (finite) and step number t >= 1: queued, not waited for.  Without orthograd one launch (k_optim_apply); with
 * it three: k_optim_dots, k_optim_gogo (which first finishes the three sums of its tensor), k_optim_apply (which finishes go.go) */
int gaz_optim_step(gaz_optim* h, double lr, int64_t t, int32_t zero_grads);
/* measurement hook (tools/optim_bench.py): `repeats` steps at t, t + 1, .. between two HIP events, after one warm-up step; the state moves */
int gaz_optim_step_timed(gaz_optim* h, double lr, int64_t t, int32_t zero_grads, int32_t repeats, double* ms_per_step);
/* f64 [n_tensors][4]: the sums w.g, w.w, g.g, go.go of the last step before their rounding to f32 (zeros before the first step and without
 * orthograd).  A host synchronisation point */
int gaz_optim_read_norms(gaz_optim* h, double* out);
int gaz_optim_synchronize(gaz_optim* h);

/* -- MUON (Net/Optimizers/muon.py; csrc/muon.hpp): gaz_muon_set turns an optimizer into the reference's Muon, wrapped like
 * the chain above: Orthograd(Grokfast_EMA(Muon)).  The feature is detected by its symbols (gaz_muon_set); gaz_optim_config does not change.
 * A tensor with rows = cols = 0 is an ADAM TENSOR, every other one a MUON TENSOR whose flat memory is read as a rows x cols matrix (muon.py's
 * reshape(update, (shape[0], -1)); rows * cols = its size).  The binding decides which is which (_should_use_adamw) and computes
 * scale = 0.2 * sqrt(max(1, shape[-2] / shape[-1])) from the tensor's real shape.
 * ONE STEP IN MUON MODE, with the rounding rules of the OPTIMIZER section (f32 operations rounded one by one, scalars rounded to f32 once):
 *   1  orthograd  as stage 2 above, on the UNDECAYED w
 *   2  grokfast   as stage 3 above -> g2
 *   3a Adam tensor   stage 4 above (kind, beta_1, beta_2, epsilon of the optimizer's config) with lr_a = f32(adam_lr_ratio) * lr in place of lr
 *   3b Muon tensor   m = beta * m + g2 * (1 - beta);  u = g2 + m * beta with nesterov, else u = m;  X = NS(u);  w = w - (X * scale) * lr
 *   4  decay      wd != 0:  w = w - ((l * wd) * w), l = lr_a for an Adam tensor, lr for a Muon tensor       (muon.py: after the update)
 *   5  zero_grads g = 0
 * m lives in the momentum arena; the velocity arena's range of a Muon tensor holds u.
 * NS(u), the Newton-Schulz iteration on bf16 VALUES HELD IN F32; bf16() rounds an f32 to nearest even on its bit pattern.  P = min(rows, cols),
 * Q = max(rows, cols); X is P x Q: the matrix itself, or its transpose when rows > cols (read transposed, never copied).
 *   X0 = bf16(u);  n = sqrtf(f32(sum X0^2)), the sum a float64 sum over the tensor's flat memory in the OPTIMIZER section's chunk order;
 *   X = bf16(X0 / (n + 1e-7f));  a, b, c = bf16(f32(muon_a)), bf16(f32(muon_b)), bf16(f32(muon_c));  then ns_steps times
 *   A = bf16(X X^T);  B = bf16(bf16(b * A) + bf16(c * bf16(A A)));  X = bf16(bf16(a * X) + bf16(B X))
 * EVERY MATRIX PRODUCT element is one f32 chain acc = fmaf(x, y, acc) over k ascending from 0 with acc = +0 at the start and no split of K (a
 * product of two bf16 values is exact in f32, so multiply-then-add gives the same bits).  THIN MATRICES (P <= 4): only X X^T differs; its
 * P (P + 1) / 2 entries are float64 sums of the exact products over the column index q = 0 .. Q - 1 in the chunk order of the OPTIMIZER section
 * applied to q (chunks of 2048 columns, slots, butterfly, the chunks' sums ascending from +0.0), each rounded to f32 and then to bf16.
 * REFERENCE QUIRK, not reproduced, as above: t is the caller's step number and the decay is applied although the optimizer is wrapped. */
typedef struct {
    uint32_t struct_size;         /* = sizeof(gaz_muon_config) */
    int32_t n_tensors;            /* the optimizer's */
    const int32_t* rows;          /* [n_tensors]; rows = cols = 0: an Adam tensor */
    const int32_t* cols;          /* [n_tensors] */
    const float* scale;           /* [n_tensors]; read for Muon tensors */
    double muon_beta;             /* in [0, 1) */
    int32_t nesterov;             /* 0 / 1 */
    int32_t ns_steps;             /* 0 .. 16 */
    double muon_a, muon_b, muon_c;/* finite */
    double adam_lr_ratio;         /* finite, >= 0 */
} gaz_muon_config;
int gaz_muon_config_size(void);
/* after gaz_optim_create and before the first step, once.  Allocates two X buffers of an arena's size and A, B (P x P) of every Muon tensor.
 * Refused, each by its text: a stale struct_size, another n_tensors, rows * cols different from a tensor's size, ns_steps outside 0 .. 16,
 * non-finite coefficients or scale, muon_beta outside [0, 1), a bad adam_lr_ratio or nesterov, a call after the first step, a second call.
 * From then on gaz_optim_layout's launches entry is: the 1 or 3 above, and with at least one Muon tensor + 2 (k_muon_norm, k_muon_finish)
 * + ns_steps * (k_muon_gram, k_muon_poly when a Muon tensor has P >= 5, k_muon_update) — whatever the number of tensors */
int gaz_muon_set(gaz_optim* h, const gaz_muon_config* cfg);
/* for tests: of Muon tensor `tensor` after the last step, what = 0 X0 [size, the tensor's flat layout], 1 n [1], 2 the final X [size, flat
 * layout], 3 / 4 A / B of the last iteration [P * P, row-major] (zeros with ns_steps = 0).  A host synchronisation point */
int gaz_muon_read(gaz_optim* h, int32_t tensor, int32_t what, float* out);

#ifdef __cplusplus
}
#endif
#endif

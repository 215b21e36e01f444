"""CPU suite: resignation in self-play and the games played out to calibrate it (gaz_engine_set_resignation) on the emulation build of
the device code — the cases of tests/resign_cases.py at sizes the one-lane emulation plays in seconds.  Exact equality everywhere."""
import numpy as np
import pytest

import resign_cases as cases
from selfplay_support import emu_lib  # noqa: F401

BOTH = cases.MINIMUM + ("false_positive", "true_positive")


# ------------------------------------------------------------------------------------------------ 1. draws and rule (no engine)
def _product_rule(q, kind, p, threshold, consecutive=1, min_ply=0):
    """the shipped Python statement of the rule, self_play.resign_trigger_plies, asked about ply p of a game that went on after it (the
    function leaves out the last ply of what it is given, so it gets the plies up to p and one more)"""
    from grok_alpha_zero_amd.self_play import resign_trigger_plies
    return p in resign_trigger_plies(list(q[:p + 1]) + [0.0], list(kind[:p + 1]) + [1], threshold, consecutive, min_ply)


@pytest.mark.parametrize("t", [cases.trigger, _product_rule], ids=["restated", "self_play.resign_trigger_plies"])
def test_the_rule_on_hand_made_records(t):
    one = np.ones(8, np.uint8)
    q = np.array([0.0, -0.5, -0.2, -0.5, -0.31, -0.5, -0.5, -0.9], np.float32)
    assert t(q, one, 1, 0.3) and not t(q, one, 2, 0.3) and not t(q, one, 0, 0.3)
    half = np.array([-0.5], np.float32)
    assert not t(half, one, 0, 0.5) and t(half, one, 0, 0.4999)                       # strict <
    # the float32 record value is widened to double: float32(-0.3) lies below the double -0.3
    assert float(np.float32(-0.3)) < -0.3 and t(np.array([-0.3], np.float32), one, 0, 0.3)
    # consecutive = 2 looks at p and p - 2, the mover's own plies: ply 3 (-0.5) and ply 1 (-0.5) yes; ply 4 (-0.31) and ply 2 (-0.2) no
    assert t(q, one, 3, 0.3, 2) and not t(q, one, 4, 0.3, 2) and t(q, one, 5, 0.3, 3) and not t(q, one, 6, 0.3, 3)
    assert not t(q, one, 1, 0.3, 2)                                                   # p < 2 (consecutive - 1): no run yet
    assert not t(q, one, 3, 0.3, 1, min_ply=4) and t(q, one, 4, 0.3, 1, min_ply=4)
    kind = one.copy(); kind[3] = 0                                                    # a ply without a search breaks the run
    assert not t(q, kind, 5, 0.3, 2) and not t(q, kind, 3, 0.3) and t(q, kind, 7, 0.3, 2)
    assert t(q, np.full(8, 0x22, np.uint8), 3, 0.3, 2)                                # fast plies count, marks above the kind do not matter


def test_the_last_ply_never_resigns_and_the_playout_draw_decides(oracle):
    from grok_alpha_zero_amd.self_play import resign_curve, resign_trigger_plies
    q = np.full(6, -0.9, np.float32)
    assert resign_trigger_plies(q, np.ones(6, np.uint8), 0.3, 2, 0) == [2, 3, 4]                   # never ply 5, the last
    row = resign_curve([dict(T=6, winner=-1, q=q, move_kind=np.ones(6, np.uint8))], [0.3, 0.95], consecutive=2)
    assert (row[0]["would_resign"], row[0]["false_positives"], row[0]["plies_saved"], row[1]["would_resign"]) == (1, 1, 3, 0)
    off = dict(T=6, winner=1, slot=3, game_seq=2, q=q, move_kind=np.ones(6, np.uint8))
    slot_p = next(s for s in range(64) if cases.is_playout_game(oracle, cases.SEED, s, 2, 0.5))
    slot_r = next(s for s in range(64) if not cases.is_playout_game(oracle, cases.SEED, s, 2, 0.5))
    e = cases.expectation(oracle, dict(off, slot=slot_r), (0.3, 2, 0, 0.5))
    assert (e["T"], e["winner"], e["resign_ply"], e["would"]) == (3, 1, 2, [])        # ply 2: -1 moved, so 1 wins
    e = cases.expectation(oracle, dict(off, slot=slot_p), (0.3, 2, 0, 0.5))
    assert (e["T"], e["winner"], e["resign_ply"], e["would"], e["false_positive"]) == (6, 1, -1, [2, 3, 4], False)      # never ply 5, the last
    e = cases.expectation(oracle, dict(off, slot=slot_p, winner=-1), (0.3, 2, 0, 0.5))
    assert e["false_positive"] is True                                                # -1 would have resigned at ply 2 and won


def test_the_playout_draw_is_a_variate_of_its_own(oracle):
    prob, n = 0.1, 4000
    u = np.array([oracle.uniform(7, s, 3, 2, 0, cases.P_RESIGN) for s in range(n)])
    assert (u >= 0).all() and (u < 1).all()
    assert abs(float((u < prob).mean()) - prob) < 4 * np.sqrt(prob * (1 - prob) / n)  # four standard deviations of a binomial rate
    assert oracle.uniform(7, 3, 2, 2, 0, 6) != oracle.uniform(7, 3, 2, 2, 0, 4) and oracle.uniform(7, 3, 2, 2, 0, 6) != oracle.uniform(7, 3, 2, 2, 0, 5)
    assert [cases.is_playout_game(oracle, 7, s, 3, prob) for s in range(n)] == (u < prob).tolist()


# ------------------------------------------------------------------------------------------------ 2. + 4. prefix cases, counters
@pytest.mark.parametrize("name,G,need", [
    ("c4", 16, cases.MINIMUM + ("false_positive",)), ("c4", 64, BOTH), ("ttt", 64, BOTH), ("ttt-min4", 16, cases.MINIMUM + ("true_positive",)),
    ("c4-gumbel", 64, cases.MINIMUM), ("c4-gumbel", 16, cases.MINIMUM), ("c4-leaf4", 16, cases.MINIMUM), ("c4-single", 16, cases.MINIMUM)])
def test_records_are_prefixes_and_the_counters_follow(emu_lib, oracle, name, G, need):
    cases.prefix_case(oracle, name, G, emu_lib, need=need)


def test_gomoku_gumbel_whole_games(emu_lib, oracle):
    """(one game per slot on the one-lane emulation; the -m gpu suite plays two)"""
    off, _, _ = cases.prefix_case(oracle, "gmk-gumbel", 8, emu_lib, need=("resigned", "would", "false_positive"), per_slot=1)
    assert all(36 <= r["T"] <= 64 for r in off.values()), sorted(r["T"] for r in off.values())


def test_gomoku_puct_with_compacted_trees(emu_lib, oracle):
    """(one game per slot, two slots: a 48-iteration Gomoku search is slow on one lane.  The -m gpu suite plays 64 slots, two games each,
    and asserts the witnesses there)"""
    cases.prefix_case(oracle, "gmk-puct", 2, emu_lib, need=("natural",), per_slot=1)


def test_a_game_resigns_after_a_fast_ply(emu_lib, oracle):
    cases.fast_resign_case(oracle, 16, emu_lib)


# ------------------------------------------------------------------------------------------------ 3.
def test_anchors_late_min_ply_all_playout_and_threshold_0(emu_lib):
    cases.anchor_case(16, emu_lib)


def test_switching_off_between_launches(emu_lib, oracle):
    """takes effect at the next launch, like set_hyperparams: on from the start, off once three games have resigned — the games that
    finish afterwards are played to their end, the counters keep what they counted, every record is its off record or a prefix of it"""
    rule = cases.case_table()["c4"][3]
    a, b = cases.make_engine("c4", 16, emu_lib), cases.make_engine("c4", 16, emu_lib, rule)
    off = cases.play(a, 32)
    a.close()
    for _ in range(4000):
        b.run_waves(8)
        if b.resign_stats()["resigned"] >= 3:
            break
    b.set_resignation(0.0)
    before = b.resign_stats()
    on = cases.play(b, 32)
    after = b.resign_stats()
    b.close()
    assert before["resigned"] >= 3 and after == before
    exp = {k: cases.expectation(oracle, off[k], rule) for k in off}
    assert sum(r["resigned"] for r in on.values()) == before["resigned"] < sum(e["resign_ply"] >= 0 for e in exp.values())
    for k, r in on.items():
        if r["resigned"]:
            cases.assert_prefix(r, off[k], exp[k], f"game {k}")
        else:                                        # (a game played out may carry marks from before the switch)
            assert r["T"] == off[k]["T"] and r["winner"] == off[k]["winner"] and np.array_equal(r["actions"], off[k]["actions"]), k


# ------------------------------------------------------------------------------------------------ 5.
@pytest.mark.parametrize("name", ["c4", "c4-cap-forced", "ttt", "c4-gumbel"])
def test_drain_samples_equals_record_to_samples(emu_lib, oracle, name):
    n_resigned, n_fast = cases.samples_case(oracle, name, 16, emu_lib)
    assert name != "c4-cap-forced" or n_fast > 0                                      # a resigned fast ply (0x12) gives no row


# ------------------------------------------------------------------------------------------------ 6.
def test_sync_engine_halts_after_the_resigning_ply(emu_lib, oracle):
    cases.sync_case(oracle, 16, emu_lib)


def test_a_set_position_prefix_breaks_the_run(emu_lib, oracle):
    cases.sync_case(oracle, 16, emu_lib, prefix=[3, 3, 2])


# ------------------------------------------------------------------------------------------------ 7.
@pytest.mark.parametrize("game", ["TicTacToe", "Connect4"])
def test_run_self_play_reads_the_four_keys(emu_lib, tmp_path, game):
    cases.run_self_play_case(tmp_path, emu_lib, game=game)


def test_run_self_play_without_the_keys_is_unchanged(emu_lib, tmp_path):
    """absent keys, and resign_threshold = 0 next to the others, mean off: the same file"""
    from grok_alpha_zero_amd.games import GAMES
    from grok_alpha_zero_amd.self_play import ReplayStore, run_self_play
    from samples_util import assert_same_file, file_contents
    train = dict(games_per_generation=12, MCTS_iteration_limit=16, max_actions=9, num_explore_actions_first=2, num_explore_actions_second=1,
                 c_puct_init=1.25, dirichlet_alpha=1.0, use_gumbel=False)
    out, est = [], {}
    for extra in ({}, dict(resign_threshold=0, resign_consecutive=2, resign_min_ply=3, no_resign_prob=0.5)):
        folder = str(tmp_path / str(len(out)) / "0")
        store = ReplayStore(folder); store.create()
        assert run_self_play(GAMES["TicTacToe"], ({}, dict(train, **extra)), folder, n_games=8, seed=11, hash_salt=4, lib_path=emu_lib, engine_stats=est) == 12
        out.append(file_contents(store))
    assert_same_file(out[0], out[1])
    assert est["resign"] and not any(est["resign"].values())


# ------------------------------------------------------------------------------------------------ 8.
def test_resign_curve_equals_the_restated_rule(emu_lib):
    cases.curve_case(16, emu_lib)


# ------------------------------------------------------------------------------------------------ 9.
@pytest.mark.parametrize("name", sorted(cases.REFUSALS) + ["struct-size"])
def test_refusals(emu_lib, name):
    cases.refusal_case(name, emu_lib)


def test_refusal_messages_are_distinct(emu_lib):
    names = ("struct-size", "threshold-nan", "threshold-inf", "threshold-negative", "threshold-one", "consecutive-zero", "min-ply-negative", "prob-nan")
    msgs = {n: cases.refusal_case(n, emu_lib) for n in names}
    assert len(set(msgs.values())) == len(names), msgs


def test_the_abi_number_and_the_structs_did_not_move(emu_lib):
    """the feature is detected by its symbols: nothing that existed changed"""
    from grok_alpha_zero_amd import engine as E
    L = E.load_library(emu_lib)
    assert L.gaz_engine_abi_version() == E.ABI_VERSION == 10 and E.EngineConfig._fields_[-1][0] == "forced_playouts_k"
    assert hasattr(L, "gaz_engine_set_resignation") and hasattr(L, "gaz_engine_get_resign_stats")
    assert E.RecordLayout._fields_[-1][0] == "off_move_kind"

"""CPU suite: match play (gaz_engine_set_match) on the emulation build — the cases of tests/match_cases.py, every game
against tests/match_model.py, exactly; then the Python layer (self_play.match_result / play_match, orchestrator.Run(match=...))."""
import json
import math
import os

import numpy as np
import pytest

import match_cases as cases
import match_model as M
from selfplay_support import emu_lib  # noqa: F401 (a fixture)


# ------------------------------------------------------------------------------------------------ 1. / 2. self-play against the model
@pytest.mark.parametrize("name,G", [("ttt", 5), ("c4", 8), ("gmk", 2), ("ttt-gumbel", 5), ("c4-gumbel", 8)])
def test_match_games_are_the_models(oracle, emu_lib, name, G):
    cases.selfplay_case(oracle, name, G, emu_lib)


# ------------------------------------------------------------------------------------------------ 3. the external evaluator
@pytest.mark.parametrize("name,uniform_b", [("c4", False), ("ttt", True), ("ttt-gumbel", False)])
def test_external_evaluator_answers_by_read_batch_network(oracle, emu_lib, name, uniform_b):
    cases.external_case(oracle, name, 4, emu_lib, uniform_b=uniform_b)


# ------------------------------------------------------------------------------------------------ 4. the anchor
@pytest.mark.parametrize("name,kw", [("c4", cases.ANCHOR_ALL), ("c4-gumbel", {}), ("gmk", {})])
def test_same_network_twice_is_match_off(emu_lib, name, kw):
    cases.anchor_case(name, 5 if name != "gmk" else 2, emu_lib, **kw)


# ------------------------------------------------------------------------------------------------ 5. sync mode, switching, a wave without requests
def test_sync_mode_whole_games(oracle, emu_lib):
    plies, _ = cases.sync_case(oracle, "c4", 3, emu_lib)
    assert plies >= 7


def test_switching_off_and_on_between_moves(oracle, emu_lib):
    plies, _ = cases.sync_case(oracle, "ttt", 4, emu_lib, switch=(1, 3))
    assert plies >= 5


# ------------------------------------------------------------------------------------------------ 6. edge cases
def test_one_game_has_all_rows_on_one_side(oracle, emu_lib):
    cases.one_game_case(oracle, "c4", emu_lib)


def test_two_games(oracle, emu_lib):
    cases.selfplay_case(oracle, "c4-gumbel", 2, emu_lib)
    cases.selfplay_case(oracle, "ttt", 2, emu_lib)


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals_name_their_field(emu_lib):
    msgs = cases.refusal_case(emu_lib)
    assert len(msgs) >= 13


def test_match_timing_brackets_every_eighth_wave(emu_lib):
    """timing_reset(True) brackets the routing stage on the waves it brackets the tree step on; off: nothing is bracketed"""
    for on in (True, False):
        eng = cases.make_engine("c4", 4, emu_lib, 8, match=on)
        eng.timing_reset(True)
        eng.run_waves(32)
        t, waves = eng.match_timing(), eng.timing()["n_waves"]
        eng.close()
        assert waves == 4 and t["waves"] == (4 if on else 0) and t["ms_host_wait"] >= 0.0, (on, t, waves)


# ------------------------------------------------------------------------------------------------ 8. Python
def test_match_result_closed_form():
    from grok_alpha_zero_amd.self_play import match_result
    # (T, winner, slot, game_seq): A is the first player (-1) iff slot + game_seq is even
    hdrs = [(5, -1, 0, 0), (5, 1, 0, 0), (5, 0, 2, 0), (5, 1, 1, 0), (5, -1, 1, 0), (5, 0, 0, 1), (5, -1, 1, 1), (5, -1, 3, 1)]
    r = match_result(hdrs)
    # A first in games 0, 1, 2, 6, 7: wins 0, 6, 7, loss 1, draw 2; A second in 3, 4, 5: win 3, loss 4, draw 5
    assert (r["n"], r["a_wins"], r["draws"], r["b_wins"]) == (8, 4, 2, 2)
    assert r["a_first"] == dict(n=5, a_wins=3, draws=1, b_wins=1) and r["a_second"] == dict(n=3, a_wins=1, draws=1, b_wins=1)
    assert r["score"] == 5 / 8 and r["elo"] == -400 * math.log10(8 / 5 - 1)
    var = (4 * (3 / 8) ** 2 + 2 * (1 / 8) ** 2 + 2 * (5 / 8) ** 2) / 8
    half = 1.96 * math.sqrt(var / 8)
    lo, hi = (-400 * math.log10(1 / (5 / 8 + s * half) - 1) for s in (-1, 1))
    assert r["elo_ci95"] == pytest.approx((lo, hi), rel=1e-12) and lo < r["elo"] < hi
    # records work as headers do; a clean sweep has no Elo, and its interval is clipped
    sweep = match_result([dict(T=3, winner=-1, slot=0, game_seq=0), dict(T=3, winner=1, slot=1, game_seq=0)])
    assert sweep["score"] == 1.0 and sweep["elo"] is None and sweep["a_wins"] == 2
    assert sweep["elo_ci95"][1] == pytest.approx(-400 * math.log10(1 / (1 - 1e-9) - 1))
    assert match_result([(3, 1, 0, 0)])["elo"] is None and match_result([(3, 1, 0, 0)])["score"] == 0.0
    with pytest.raises(ValueError):
        match_result([])


TRAIN = dict(games_per_generation=8, MCTS_iteration_limit=16, max_actions=9, num_explore_actions_first=3, num_explore_actions_second=3,
             c_puct_init=1.25, dirichlet_alpha=1.0, use_gumbel=False, total_generations=4)


def test_play_match_against_the_model(oracle, emu_lib):
    """play_match with two salts: every game is the model's (so the winners are), and the result is match_result of them"""
    from grok_alpha_zero_amd.games import TicTacToe
    from grok_alpha_zero_amd.self_play import match_result, play_match
    res = play_match(TicTacToe, ({}, TRAIN), None, None, 16, n_slots=4, seed=cases.SEED, hash_salt=cases.SALT_A, hash_salt_b=cases.SALT_B, lib_path=emu_lib)
    hdrs = res.pop("headers")
    assert sorted((s, q) for _, _, s, q in hdrs) == [(s, q) for s in range(4) for q in range(4)]
    # the same games from an engine of its own, each against the model
    from grok_alpha_zero_amd.engine import SelfPlayEngine
    eng = SelfPlayEngine("TicTacToe", 4, 24, 9, 3, 3, 1.25, 1.0, seed=cases.SEED, hash_salt=cases.SALT_A, games_budget=16, ring_capacity=64, lib_path=emu_lib)
    eng.set_match(True, hash_salt_b=cases.SALT_B)
    from selfplay_support import play
    recs = play(eng, 16)
    eng.close()
    nets = M.hash_pair(oracle, "TicTacToe", cases.SALT_A, cases.SALT_B)
    for key, r in sorted(recs.items()):
        M.assert_puct_record(oracle, "TicTacToe", cases.SEED, 24, 9, r, nets, f"play_match game {key}", c_puct_init=1.25, dirichlet_alpha=1.0)
    want = match_result([(r["T"], M.winner_of("TicTacToe", r["actions"], 9), r["slot"], r["game_seq"]) for r in recs.values()])
    for k in want:
        assert res[k] == want[k], k
    assert res["a_first"]["n"] == res["a_second"]["n"] == 8 and res["positions"] == sum(r["T"] for r in recs.values())
    assert res["match_stats"]["rows_a"] > 0 and res["match_stats"]["rows_b"] > 0 and res["seconds"] > 0


@pytest.mark.parametrize("games,n_slots", [(0, 1), (6, 2), (8, 8), (-4, 1)])
def test_play_match_refuses_unbalanced_games(emu_lib, games, n_slots):
    from grok_alpha_zero_amd.games import TicTacToe
    from grok_alpha_zero_amd.self_play import play_match
    with pytest.raises(ValueError, match="multiple of 2 \\* n_slots"):
        play_match(TicTacToe, ({}, TRAIN), None, None, games, n_slots=n_slots, lib_path=emu_lib)


def test_run_with_a_match_after_every_generation(emu_lib, tmp_path):
    """Run(match=...) on the hash evaluator: Match.json of every generation from 2 on, a rejected generation keeps the accepted folder's
    weights for self-play, and a resumed Run reads the accepted folder back"""
    from grok_alpha_zero_amd.games import TicTacToe
    from grok_alpha_zero_amd.orchestrator import Run
    root = str(tmp_path / "train")
    asked = []

    def weights_fn(folder):
        asked.append(os.path.basename(folder))
        return None

    def run(total, threshold):
        cfg = ({}, dict(TRAIN, total_generations=total))
        return Run(TicTacToe, cfg, train_fn=lambda g, folder, nxt: None, weights_fn=weights_fn, root=root, n_games=4, seed=3, lib_path=emu_lib,
                   out=lambda *a: None, self_play_kwargs=dict(allow_synthetic=True, eval_cache_log2=0),
                   match=dict(games=8, n_slots=4, threshold=threshold, hash_salt=cases.SALT_A, hash_salt_b=cases.SALT_B))
    stats = run(3, 2.0)                                                  # no score reaches 2: every new generation is rejected
    assert "match" not in stats[0] and stats[1]["match"]["accepted"] is False and stats[2]["match"]["accepted"] is False
    for g in (2, 3):
        mj = json.load(open(os.path.join(root, str(g), "Match.json")))
        assert mj["accepted"] is False and os.path.basename(mj["accepted_folder"]) == "1" and os.path.basename(mj["new_folder"]) == str(g)
        assert os.path.basename(mj["old_folder"]) == "1" and mj["result"]["n"] == 8 and mj["result"]["a_first"]["n"] == 4
        assert mj["result"] == json.loads(json.dumps({k: v for k, v in stats[g - 1]["match"].items() if k != "accepted"}))
    assert not os.path.exists(os.path.join(root, "1", "Match.json"))
    # self-play of generation 1 asked for folder 1, the match after it for folder 2; generation 2 kept folder 1
    assert asked == ["1", "2", "1", "3"], asked
    del asked[:]
    stats = run(5, None)                                                 # resumed at generation 3: folder 1 is still the accepted one; no threshold now
    assert asked[:2] == ["1", "4"] and stats[0]["generation"] == 3 and stats[0]["match"]["accepted"] is True, asked
    assert asked[2:] == ["4", "5"], asked                                # generation 4 plays the accepted folder 4
    mj = json.load(open(os.path.join(root, "4", "Match.json")))
    assert mj["accepted"] is True and os.path.basename(mj["accepted_folder"]) == "4" and os.path.basename(mj["old_folder"]) == "1"

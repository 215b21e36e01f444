"""CPU suite: training with Muon (grok_alpha_zero_amd/train.py with optimizer = "muon") on the one-lane emulation build, torch
on the CPU — the cases of tests/muon_train_cases.py.  The optimizer's part is exact: tests/muon_model.py fed with the grads autograd left in the
arena."""
import pytest

import muon_train_cases as cases
from selfplay_support import emu_lib  # noqa: F401


def test_the_three_networks_are_classified_as_should_use_adamw_does():
    assert cases.classification_case() == {"Gomoku": 13, "Connect4": 14, "TicTacToe": 14}      # (a projection only where a block changes the width)


def test_three_muon_steps_on_the_network_equal_the_model_in_every_bit(emu_lib):
    assert cases.steps_case(emu_lib) >= 10


def test_train_generation_with_muon_records_the_classification(emu_lib, tmp_path):
    assert cases.generation_case(tmp_path, emu_lib)["steps"] >= 2


def test_run_trains_with_muon(emu_lib, tmp_path):
    assert len(cases.run_case(tmp_path, emu_lib)) == 2


def test_muon_settings_and_what_stays_refused():
    from grok_alpha_zero_amd import train as T
    from grok_alpha_zero_amd.engine import EngineError
    st = T.optimizer_settings((dict(), dict(), dict(optimizer="muon", kwargs={})))    # muon.py's defaults
    assert (st["kind"], st["beta_2"], st["epsilon"], st["weight_decay"], st["exclude_layers"], st["exclude_embeddings"]) == ("nadam", 0.995, 1e-8, 0.004, [], True)
    st = T.optimizer_settings((dict(), dict(), dict(optimizer="Muon", kwargs=dict(use_nadam=False, nesterov=False, ns_steps=3, adam_lr_ratio=0.5, caution=False))))
    assert st["kind"] == "adam" and st["muon"]["nesterov"] is False and st["muon"]["ns_steps"] == 3 and st["muon"]["adam_lr_ratio"] == 0.5
    with pytest.raises(EngineError, match="caution=True is not supported"):
        T.optimizer_settings((dict(), dict(), dict(optimizer="muon", kwargs=dict(caution=True))))
    with pytest.raises(EngineError, match="mixed_precision"):
        T.optimizer_settings((dict(), dict(mixed_precision="mixed_bfloat16"), dict(optimizer="muon")))
    for configs in ((dict(), dict(optimizer="muon")), (dict(), dict(), dict(optimizer="Muon")), (dict(), dict(optimizer="muon"), dict(kwargs={}))):
        with pytest.raises(EngineError, match="'muon' is not supported without its keywords"):       # as Train.py: Muon(**optimizer_config["kwargs"])
            T.optimizer_settings(configs)
    with pytest.raises(EngineError, match=r"has no keywords \['beta_1'\]"):
        T.optimizer_settings((dict(), dict(), dict(optimizer="muon", kwargs=dict(beta_1=0.8))))

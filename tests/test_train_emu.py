"""CPU suite: training on the device (grok_alpha_zero_amd/train.py, orchestrator.Run(train=...)) on the one-lane emulation
build, torch on the CPU and the arenas shared through numpy — the cases of tests/train_cases.py.  The optimizer's part is exact (tests/optim_model.py
fed with the grads autograd left in the arena); the batch-norm and the losses are held to numpy restatements."""
import pytest

import train_cases as cases
from selfplay_support import emu_lib  # noqa: F401


def test_training_batch_norm_against_numpy():
    assert cases.batch_norm_case() >= 0.0


def test_losses_against_the_score_model_and_keras_clips():
    seen = cases.loss_case()
    assert seen["clip"] == 2


@pytest.mark.parametrize("gumbel", [False, True])
def test_three_steps_on_the_network_equal_the_model_in_every_bit(emu_lib, gumbel):
    assert cases.steps_case(emu_lib, gumbel=gumbel) > 20


def test_train_generation_twice_and_a_generation_of_no_epochs(emu_lib, tmp_path):
    assert len(cases.generation_case(tmp_path, emu_lib)) == 3


def test_run_trains_by_itself(emu_lib, tmp_path):
    assert len(cases.run_case(tmp_path, emu_lib)) == 2


def test_every_refusal_by_its_text(emu_lib, tmp_path):
    assert len(cases.refusal_case(tmp_path, emu_lib)) == 5


def test_optimizer_settings_prefer_the_optimizer_config():
    from grok_alpha_zero_amd import train as T
    st = T.optimizer_settings((cases.BUILD, cases.TRAIN))
    assert (st["kind"], st["beta_2"], st["orthograd"], st["grokfast"], st["lamb"], st["train_epochs"], st["weight_decay"]) == ("nadam", 0.995, True, True, 2.0, 3, 0.0)
    oc = dict(optimizer="AdamW", use_orthograd=False, use_grokfast=False, grokfast_lambda=7.0, train_epochs=5, gradient_accumulation_steps=4, kwargs=dict(beta_2=0.99))
    st = T.optimizer_settings((cases.BUILD, cases.TRAIN, oc))
    assert (st["kind"], st["beta_2"], st["orthograd"], st["grokfast"], st["lamb"], st["train_epochs"], st["weight_decay"], st["accumulation"]) == \
        ("adam", 0.99, False, False, 7.0, 5, 0.004, 4)
    assert T.learning_rate(cases.TRAIN, 3, 4) == 1e-3 * 0.5 ** 3 / 4 and T.learning_rate(cases.TRAIN, 0) == 1e-3

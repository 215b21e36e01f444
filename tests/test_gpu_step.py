"""tests/gpu_step.py ChildSteps on children that open no GPU: tiny scripts that import nothing of the project and nothing of torch.  Every
test has a runner of its own, never gpu_step.STEPS."""
import os

import pytest

from gpu_step import ROOT, ChildSteps

MARK = "import sys\nopen(sys.argv[1], 'w').close()\n"          # the child after a dead one: started, it would leave the file named by its case


def _script(tmp_path, name, body):
    p = tmp_path / (name + ".py")
    p.write_text(body)
    return str(p)


def _fails(steps, script, case, seconds=30, **kw):
    with pytest.raises(pytest.fail.Exception) as e:         # (AssertionError is not a subclass: only pytest.fail is caught here)
        steps.run(script, case, seconds, **kw)
    return str(e.value)


def test_exit_0_passes(tmp_path, capsys):
    steps = ChildSteps()
    steps.run(_script(tmp_path, "fine", "import sys\nprint('case', sys.argv[1])\n"), "a", 30)
    assert "case a" in capsys.readouterr().out and steps.dead is None


def test_an_ordinary_failure_fails_its_step_and_the_next_one_still_starts(tmp_path):
    steps, marker = ChildSteps(), tmp_path / "started"
    with pytest.raises(AssertionError) as e:
        steps.run(_script(tmp_path, "three", "import sys\nprint('said on stdout')\nprint('said on stderr', file=sys.stderr)\nsys.exit(3)\n"), "a", 30)
    assert "a: exit status 3" in str(e.value) and "said on stdout" in str(e.value) and "said on stderr" in str(e.value)
    assert steps.dead is None
    steps.run(_script(tmp_path, "mark", MARK), str(marker), 30)
    assert marker.exists()


DEAD = {
    "abort-status": ("import sys\nsys.exit(134)\n", 30),
    "segfault-status": ("import sys\nsys.exit(139)\n", 30),
    "signal": ("import os, signal\nos.kill(os.getpid(), signal.SIGTERM)\n", 30),
    "gpu-fault-text": ("import sys\nprint('HIP error: an illegal memory access was encountered', file=sys.stderr)\nsys.exit(1)\n", 30),
    "time-limit": ("import time\ntime.sleep(5)\n", 1),
}


@pytest.mark.parametrize("kind", sorted(DEAD))
def test_after_a_dead_step_nothing_more_is_started(tmp_path, kind):
    body, seconds = DEAD[kind]
    steps, marker = ChildSteps(), tmp_path / "started"
    with pytest.raises((AssertionError, pytest.fail.Exception)):
        steps.run(_script(tmp_path, "test_feature_gpu", body), "case:" + kind, seconds)
    assert steps.dead == "test_feature_gpu:case:" + kind
    msg = _fails(steps, _script(tmp_path, "mark", MARK), str(marker))
    assert msg == f"not started: the GPU step test_feature_gpu:case:{kind} was killed or ran out of time"
    assert not marker.exists()
    _fails(steps, _script(tmp_path, "mark", MARK), str(marker))          # and stays dead
    assert not marker.exists()


def test_the_time_limit_is_reported(tmp_path):
    assert _fails(ChildSteps(), _script(tmp_path, "slow", "import time\ntime.sleep(5)\n"), "a", seconds=1) == "a: no result within 1 s"


def test_env_reaches_the_child_over_the_inherited_environment(tmp_path, monkeypatch):
    monkeypatch.setenv("GPU_STEP_INHERITED", "kept")
    body = "import os, sys\nsys.exit(0 if (os.environ['GPU_STEP_INHERITED'], os.environ['GPU_STEP_GIVEN']) == ('kept', sys.argv[1]) else 3)\n"
    steps = ChildSteps()
    steps.run(_script(tmp_path, "env", body), "given", 30, env={"GPU_STEP_GIVEN": "given"})
    with pytest.raises(AssertionError):
        steps.run(_script(tmp_path, "env", body), "given", 30)


def test_tail_bounds_the_printed_output(tmp_path, capsys):
    ChildSteps().run(_script(tmp_path, "long", "print('x' * 100 + 'END')\n"), "a", 30, tail=10)
    assert capsys.readouterr().out.strip() == "xxxxxxEND"


def test_children_run_from_the_repository_root(tmp_path):
    body = "import os, sys\nsys.exit(0 if os.getcwd() == sys.argv[1] else 3)\n"
    ChildSteps().run(_script(tmp_path, "cwd", body), os.path.realpath(ROOT), 30)

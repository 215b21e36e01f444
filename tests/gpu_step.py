"""The one runner of the -m gpu modules whose cases run as child processes: a case is the test module itself run as a script with the
case's name, under a time limit (a kill guard, not a measurement).  A child that was killed, aborted, faulted the GPU or ran out of time
makes the runner dead, and a dead runner starts nothing more: the card such a child leaves behind is not to be used by the next one.
STEPS is the instance of the whole pytest process, so the rule holds for the run, not for one file."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAD_CODES = (124, 134, 137, 139)                  # timeout(1), SIGABRT, SIGKILL, SIGSEGV as a shell reports them; a negative code is the signal itself
GPU_FAULT = "illegal memory access"                # HIP's error text: the child may have gone on and ended with an ordinary status


class ChildSteps:
    def __init__(self):
        self.dead = None                           # "<module>:<case>" of the first dead step

    def run(self, script, case, seconds, env=None, tail=4000):
        """[python, script, case] from the repository root with `env` over os.environ; fails the calling test unless the child ends with 0"""
        if self.dead:
            pytest.fail(f"not started: the GPU step {self.dead} was killed or ran out of time")
        name = f"{os.path.splitext(os.path.basename(script))[0]}:{case}"
        try:
            r = subprocess.run([sys.executable, os.path.abspath(script), case], cwd=ROOT, timeout=seconds, capture_output=True, text=True,
                               env=dict(os.environ, **(env or {})))
        except subprocess.TimeoutExpired:
            self.dead = name
            pytest.fail(f"{case}: no result within {seconds} s")
        if r.returncode < 0 or r.returncode in DEAD_CODES or GPU_FAULT in r.stderr:
            self.dead = name
        print(r.stdout[-tail:])
        assert r.returncode == 0, f"{case}: exit status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"


STEPS = ChildSteps()

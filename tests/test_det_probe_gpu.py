"""-m gpu: the device's bit-exact math on the HIP build, function by function against the oracle through SelfPlayEngine.probe_det — the
cases of tests/det_cases.py (tests/test_det_probe_emu.py runs them on the emulation build).  Bits, no tolerance; every case prints and
asserts its witnesses.

What only this module reaches: the compiler's expansion of the float64 division and of __dsqrt_rn, the divergent rejection loops of
det::gamma / det::normal (lanes of one wavefront leave at different attempts), compute_pi_small and its tlane_val / seq_sum_lanes /
max_lanes shuffles (readlane on a whole-wave team, DPP row broadcasts on 16-lane teams, where the four teams of a wavefront hold
different nodes), and the puct_table the engine fills on the device.

Every case is a child step of the shared runner, tests/gpu_step.py; the limit is a kill guard, the kernels take milliseconds."""
import os
import sys

import pytest

from gpu_step import STEPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                      # run as a script (a child step): nothing has put the repository on the path yet
    sys.path.insert(0, ROOT)

import det_cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(det_cases.CASES))
def test_det_probe_equals_the_oracle(name):
    STEPS.run(__file__, name, 120, tail=6000)


if __name__ == "__main__":
    from oracle import gaz_oracle as O
    O.build()
    det_cases.run_case(sys.argv[1], O, None)
    print("ok", flush=True)

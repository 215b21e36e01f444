"""CPU suite: the device's bit-exact math (csrc/det.hpp, the PUCT factors and scores, numpy's pairwise sum, the Gumbel softmax /
compute_pi / deterministic selection) on the emulation build, function by function against the oracle through SelfPlayEngine.probe_det —
the cases of tests/det_cases.py, which tests/test_det_probe_gpu.py runs on the HIP build.  Bits, no tolerance.

On the emulation build a team is one lane: the shuffles of the HIP build do not exist there, compute_pi_small is not compiled and the
general path of compute_pi serves every n (on the HIP build n < 8 runs compute_pi_small), and the lanes of a "wave" cannot leave a
rejection loop at different attempts.  What this module pins is the arithmetic of the shared source under the emulation library's flags."""
import pytest

import det_cases
from selfplay_support import emu_lib  # noqa: F401


@pytest.mark.parametrize("name", list(det_cases.CASES))
def test_det_probe_equals_the_oracle(name, emu_lib, oracle):  # noqa: F811
    det_cases.run_case(name, oracle, emu_lib)


def test_probe_det_rejects_what_would_index_past_an_array(emu_lib):  # noqa: F811
    import numpy as np
    from grok_alpha_zero_amd import engine as E
    with det_cases.make_engine("Connect4", emu_lib) as eng:
        one = np.zeros((1, 1 + 256), np.uint64)
        for n in (0, 257):                                           # np_pairwise_sum serves 1..256
            one[0, 0] = n
            with pytest.raises(E.EngineError):
                eng.probe_det(E.DP_SUM_F64, one, 1)
        node = np.zeros((1, 4 + 4 * 8), np.uint64); node[0, 0] = 8   # a Connect4 node has at most 7 children
        with pytest.raises(E.EngineError):
            eng.probe_det(E.DP_PI, node, 3 + 8)
        node[0, 0] = 7
        with pytest.raises(E.EngineError):
            eng.probe_det(E.DP_PI, node, 3 + 6)                      # no room for the seventh output
        with pytest.raises(E.EngineError):
            eng.probe_det(E.DP_DLOG, np.ones((4, 2), np.uint64), 1)  # an element op's words are exact
        with pytest.raises(E.EngineError):
            eng.probe_det(99, np.ones((4, 1), np.uint64), 1)

"""CPU suite: how the whole-trunk launch of a batch is cut into 128-row and 96-row tiles (grok_alpha_zero_amd/csrc/tile_perm.hpp trunk_split,
through the test hook of the emulation build).  The evaluator's launch plan (make_trunk_plan), its separate launch (forward_trunk) and the
figure bench.py prices (dominant_kernel) all take the split from this one function; the expected values below were produced from the
expressions the evaluator held before the function existed, not from the function."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")


@pytest.fixture(scope="module")
def split():
    subprocess.run(["make", "-s", "-C", EMU_DIR], check=True)
    L = C.CDLL(os.path.join(EMU_DIR, "libgaz_emu.so"))
    L.gaz_test_trunk_split.restype = None

    def f(n, HW, n_cus, mix_allowed, fill_big):
        out = [C.c_int(-1) for _ in range(4)]
        L.gaz_test_trunk_split(n, HW, n_cus, int(mix_allowed), int(fill_big), *[C.byref(o) for o in out])
        n_big, n_small, nwg, mix = (o.value for o in out)
        return n_big, n_small, nwg, bool(mix)
    return f


def test_connect4_tiles_cover_every_batch_exactly(split):
    HW, n_cus = 42, 256                                                   # 3 boards per 128-row tile, 2 per 96-row tile
    for n in range(1, 8193):
        for fill_big in (False, True):
            n_big, n_small, nwg, mix = split(n, HW, n_cus, True, fill_big)
            assert n_big >= 0 and n_small >= 0 and n_big * 3 <= n, (n, fill_big, n_big, n_small)
            assert n_big * 3 + n_small * 2 >= n, (n, fill_big, n_big, n_small)                 # every board has a tile ...
            assert n_big * 3 + (n_small - 1) * 2 < n if n_small else n_big * 3 == n, (n, fill_big, n_big, n_small)     # ... and no tile is spare
            if fill_big:
                assert n_big == n // 3 and mix, (n, n_big, mix)           # a launch that shares the chip: every board that fits in a 3-board tile
            else:
                assert n_big % (2 * n_cus) == 0, (n, n_big)               # a launch of its own: whole rounds of 3-board tiles only
            assert nwg == (n_big + n_small if mix else (n + 2) // 3), (n, fill_big, nwg, mix)


# (n, n_cus, fill_big) -> (n_big, n_small, mix): ResNetEvaluator::make_trunk_plan's expressions of the commit before trunk_split, run on the CPU
PARENT = {
    (1, 256, False): (0, 1, True),
    (7, 256, False): (0, 4, True),
    (100, 256, False): (0, 50, True),
    (334, 256, False): (0, 167, True),
    (1536, 256, False): (512, 0, False),
    (1537, 256, False): (512, 1, True),
    (2048, 256, False): (512, 256, True),
    (4096, 256, False): (1024, 512, True),
    (8192, 256, False): (2560, 256, True),
    (1, 256, True): (0, 1, True),
    (7, 256, True): (2, 1, True),
    (100, 256, True): (33, 1, True),
    (334, 256, True): (111, 1, True),
    (1536, 256, True): (512, 0, True),
    (1537, 256, True): (512, 1, True),
    (2048, 256, True): (682, 1, True),
    (4096, 256, True): (1365, 1, True),
    (8192, 256, True): (2730, 1, True),
    (1, 304, False): (0, 1, True),
    (7, 304, False): (0, 4, True),
    (100, 304, False): (0, 50, True),
    (334, 304, False): (0, 167, True),
    (1536, 304, False): (0, 768, False),
    (1537, 304, False): (0, 769, False),
    (2048, 304, False): (608, 112, True),
    (4096, 304, False): (1216, 224, True),
    (8192, 304, False): (2432, 448, True),
    (1, 304, True): (0, 1, True),
    (7, 304, True): (2, 1, True),
    (100, 304, True): (33, 1, True),
    (334, 304, True): (111, 1, True),
    (1536, 304, True): (512, 0, True),
    (1537, 304, True): (512, 1, True),
    (2048, 304, True): (682, 1, True),
    (4096, 304, True): (1365, 1, True),
    (8192, 304, True): (2730, 1, True),
}


def test_trunk_split_makes_the_choices_the_evaluator_made_before(split):
    assert {n for n, _, _ in PARENT} == {1, 7, 100, 334, 1536, 1537, 2048, 4096, 8192} and {c for _, c, _ in PARENT} == {256, 304}
    for (n, n_cus, fill_big), want in PARENT.items():
        n_big, n_small, nwg, mix = split(n, 42, n_cus, True, fill_big)
        assert (n_big, n_small, mix) == want, (n, n_cus, fill_big)
        assert nwg == (n_big + n_small if mix else (n + 2) // 3)


def test_gomoku_and_tictactoe_never_mix(split):
    """96 / 225 = 0: no Gomoku board fits a 96-row tile; TicTacToe (14 boards per 128-row tile) has no whole-trunk launch at all."""
    for HW in (225, 9):
        for n in (1, 2, 3, 100, 511, 512, 513, 2048, 8192):
            for n_cus in (256, 304):
                for mix_allowed in (False, True):
                    for fill_big in (False, True):
                        assert split(n, HW, n_cus, mix_allowed, fill_big)[3] is False, (HW, n, n_cus, mix_allowed, fill_big)


def test_a_switched_off_mix_is_one_tile_shape(split):
    for n in (1, 7, 1537, 4096):
        n_big, n_small, nwg, mix = split(n, 42, 256, False, False)
        assert not mix and nwg == (n + 2) // 3

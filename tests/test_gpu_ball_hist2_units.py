"""Anisotropic pair counts (nbkd_query_ball_hist2) on coordinates away from the
unit box: the frames of tests/units.py (kpc/h and Mpc/h boxes, scales 2^-20 and
2^40, a large offset, a set centred on 0), edges as fractions of the frame's
scale, compared with the brute force of tests/aniso_ref.py in that frame.
s-45 is left out on purpose: the product M * s2 goes subnormal there, which
include/nbkd.h lists as untested."""
import numpy as np
import pytest

from tests import aniso_ref as ar
from tests import units

pytestmark = pytest.mark.gpu

N, M = 3000, 600
FRAMES = ("L205000", "L67.77", "s+40", "s-20", "off1000", "centred17")
CASES = [c for c in units.CASES if c[0] in FRAMES]
E1_FRACTIONS = (0.0, 0.01, 0.03, 0.07, 0.07, 0.15)
PI_FRACTIONS = (0.004, 0.05, 0.05, 0.35)
MU = np.array([0.0, 0.3, 0.6, 0.6, 1.0], np.float32)


def test_the_cases_are_the_intended_ones():
    assert sorted({c[0] for c in CASES}) == sorted(FRAMES)
    assert len(CASES) == 8  # the two dyadic scales run plain and periodic


@pytest.mark.parametrize("mode", [ar.RPPI, ar.SMU], ids=["rppi", "smu"])
@pytest.mark.parametrize("case", CASES, ids=units.case_id)
def test_parity_in_the_frame(gpu, case, mode):
    name, box = case
    pts, q = units.inputs(name, N, M)
    e1 = np.array([units.length(name, f) for f in E1_FRACTIONS], np.float32)
    e2 = MU if mode == ar.SMU else np.array([units.length(name, f) for f in PI_FRACTIONS],
                                            np.float32)
    t = gpu.Tree(pts, leafsize=32, boxsize=box)
    for los in (0, 1, 2):
        ref = ar.hist2_ref(pts, q, e1, e2, mode, los, box)
        assert ref.sum() > 2000 and ref[0, 0] >= M // 3  # the self rows sit in bin (0, 0)
        got = t.ball_hist2(q, e1, e2, mode, los)
        assert np.array_equal(got, ref), f"los {los}"

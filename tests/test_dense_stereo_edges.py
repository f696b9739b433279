"""The edge cases of dense stereo (tests/dense_stereo_edge_cases.py) are what they claim — conditions on the numpy restatement
(tests/dense_stereo_restatement.py), so that a later edit of the generators cannot hollow out the tests that run the kernels on
them — and two properties of the restatement that follow from the definition (include/vo_hip.h, "Dense stereo") alone: a pair
turned upside down gives the result turned upside down, and a monotone remap of the grey values changes nothing. No GPU."""
import numpy as np
import pytest

from dense_stereo_edge_cases import EDGE_CASES, FLIP_CASES, SATURATED, TINY, TINY_SHAPES, flipped, restated
from dense_stereo_restatement import DEFAULTS, dense_stereo
from test_dense_stereo_emu import same_planes


def test_saturation_cases_reach_the_upper_half_of_the_u16_volume():
    a, b = restated("sat_n64"), restated("sat_n128")
    print("sat_n64", a["s_max"], a["above_32767"], a["n_accepted"], "sat_n128", b["s_max"], b["above_32767"], b["n_accepted"])
    assert a["s_max"] <= 65528 and a["above_32767"] > 0.10
    assert 40000 < b["s_max"] <= 65528 and b["above_32767"] > 0.03
    for r, name in ((a, "sat_n64"), (b, "sat_n128")):  # the large values sit next to accepted parabolas
        assert r["n_accepted"] > r["status"].size // 2, name
    # ... in sat_n64 inside them and inside the uniqueness test: S2 and S(d_best - 1) above 32767 at accepted pixels
    print("sat_n64 accepted pixels with S2 > 32767:", a["s2_large_accepted"], "with S(d_best - 1) > 32767:", a["sm_large_accepted"])
    assert a["s2_large_accepted"] >= 1000 and a["sm_large_accepted"] >= 1000
    for name in SATURATED + ("paths4_p2_8129",):
        assert restated(name)["s_max"] <= 65528 and EDGE_CASES[name][3]["p2"] == 8129, name


def test_ties_show_in_the_disparity_only_without_the_uniqueness_test():
    u0, df = restated("ties_uniq0"), restated("ties")
    far = u0["far_ties"]
    assert np.array_equal(far, df["far_ties"])  # (the volume does not depend on uniqueness)
    print("far ties", int(far.sum()), "accepted among them with uniqueness 0", int((u0["status"][far] == 1).sum()))
    assert far.sum() >= 100 and (u0["status"][far] == 1).sum() >= 20
    assert np.isin(df["status"][far], (2, 4)).all()
    # the accepted ones lie at the first of the equal minima: one period (8) further the disparity would differ by 8
    d_min = EDGE_CASES["ties_uniq0"][3]["d_min"]
    acc = far & (u0["status"] == 1)
    S = dense_stereo(*EDGE_CASES["ties_uniq0"][:3], **EDGE_CASES["ties_uniq0"][3])["S"]
    first = S.argmin(axis=2)
    assert (np.abs(u0["disparity"][acc] - (d_min + first[acc])) <= 0.5).all()
    assert ((S == S.min(axis=2, keepdims=True)).sum(axis=2)[acc] >= 2).all()
    assert not far.all() and (u0["status"][~far] == 1).sum() > 1000  # ties in places only


def test_every_status_occurs_and_the_checks_bite():
    seen = set()
    for name in EDGE_CASES:
        seen |= set(np.unique(restated(name)["status"]).tolist())
    assert seen == {0, 1, 2, 3, 4}
    assert restated("uniq_99")["n_accepted"] < restated("uniq_0")["n_accepted"]
    assert (restated("uniq_0")["status"] != 2).all() and (restated("uniq_99")["status"] == 2).sum() > (restated("lr_0")["status"] == 2).sum()
    # lr_max >= n_disp: no difference of two disparities is larger, so status 3 is left for x_r < 0 alone
    left, right, mask, prm, _ = EDGE_CASES["lr_64"]
    S = dense_stereo(left, right, mask, **prm)["S"]
    xr = np.arange(left.shape[1])[None, :] - DEFAULTS["d_min"] - S.argmin(axis=2)
    assert (xr[restated("lr_64")["status"] == 3] < 0).all()
    assert restated("lr_64")["n_accepted"] > restated("lr_0")["n_accepted"]  # (the same pair and uniqueness: lr_max alone differs)
    assert (restated("lr_64")["status"] == 3).sum() < (restated("lr_0")["status"] == 3).sum()
    for name in ("d_min_39", "d_min_40"):  # no right pixel inside the image (d_min_39: at one column and d = 0 alone)
        assert (restated(name)["status"] == 4).all() and (restated(name)["disparity"] == 0).all(), name
    assert restated("p1_0_p2_1")["s_max"] <= 8 * (62 + 1)


def test_tiny_shapes_are_the_ones_named():
    shapes = {EDGE_CASES[name][0].shape[::-1] for name in TINY}
    assert shapes == set(TINY_SHAPES) and len(TINY) == len(TINY_SHAPES) + 2
    assert any(EDGE_CASES[name][2] is not None for name in TINY) and any(EDGE_CASES[name][4] > 0 for name in TINY)
    assert any(s[0] * s[1] % 8 for s in TINY_SHAPES)  # a pixel count that is no multiple of the decision's 8 pixels a wavefront
    for name in TINY:
        r = restated(name)
        assert r["status"].shape == EDGE_CASES[name][0].shape and r["n_accepted"] == int((r["status"] == 1).sum())


# ---- two properties that need nothing but the definition ---------------------------------------------------------------------------
@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("name", FLIP_CASES)
def test_vertical_flip(name, paths):
    """both direction sets are closed under the flip, and the flip only permutes the census bits of both images alike, which
    leaves the Hamming distances alone: all four planes and S, bit for bit"""
    left, right = EDGE_CASES[name][:2]
    a = dense_stereo(left, right, paths=paths)
    b = dense_stereo(left[::-1], right[::-1], paths=paths)
    assert np.array_equal(b["S"], a["S"][::-1])
    ok, where = same_planes(b, flipped(a))
    assert ok, where
    assert b["n_accepted"] == a["n_accepted"]
    assert not np.array_equal(a["S"], a["S"][::-1])  # (the case is not its own mirror image)


def test_monotone_grey_remap():
    """v -> 2 v + 1 on a pair of values 0..127 keeps every comparison of the census, so every plane stays"""
    left, right, mask, prm, _ = EDGE_CASES["grey_0_127"]
    assert left.max() <= 127 and right.max() <= 127
    a = dense_stereo(left, right, mask, **prm)
    b = dense_stereo(2 * left + 1, 2 * right + 1, mask, **prm)
    assert (2 * left + 1).dtype == np.uint8 and np.array_equal(a["S"], b["S"])
    ok, where = same_planes(b, a)
    assert ok, where
    ok, _ = same_planes(a, restated("grey_0_127"))
    assert ok

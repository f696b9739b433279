"""Dense stereo on the device (include/vo_hip.h, "Dense stereo") on the edge cases of
tests/dense_stereo_edge_cases.py, everything bit for bit: every case against the numpy restatement — the summed volume above 32767
with one and with two disparities a lane, ties, the penalties and the two checks at the ends of their ranges, d_min at and beyond
the width, shapes below the census window and below a wavefront's pixels —, host planes everywhere and device planes for five of
them; the vertical flip and the monotone grey remap, which need no restatement; and one fresh context taken through 128, 256 and 64
disparities, 8 and 4 paths and shapes from 288 x 288 down to 1 x 1, where every result is right whatever the volume held before and
the allocation count moves only when vo_dense_stereo_workspace grows."""
import numpy as np
import pytest

from dense_stereo_edge_cases import EDGE_CASES, FLIP_CASES, flipped, restated
from dense_stereo_restatement import dense_stereo
from test_dense_stereo_emu import same_planes
from test_dense_stereo_gpu import PLANES, _download, _load
from util import DeviceBuffer

pytestmark = pytest.mark.gpu

ON_DEVICE_TOO = ("sat_n128", "ties_uniq0", "tiny_1x1", "tiny_2x64", "tiny_13x7_mask")


@pytest.fixture(scope="module")
def ds_ctx(vo):
    c = vo.Context(device=0, max_width=288, max_height=288, max_points=256, n_slots=2, max_level=0)
    yield c
    c.close()


def _into_device_planes(ctx, shape, prm):
    """the operator into device planes that held something else -> what it left there"""
    bufs = {k: DeviceBuffer(np.full(shape, 0x5A, np.uint8).astype(dt)) for k, dt in PLANES}
    try:
        assert ctx.denseStereo(0, 1, out={k: b.data_ptr() for k, b in bufs.items()}, **prm) is None
        return {k: _download(bufs[k], dt, shape) for k, dt in PLANES}
    finally:
        for b in bufs.values():
            b.free()


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_operator_equals_restatement(ds_ctx, name):
    ctx = ds_ctx
    left, right, mask, prm, _ = EDGE_CASES[name]
    want = restated(name)
    _load(ctx, left, right, mask)
    got = ctx.denseStereo(0, 1, **prm)
    ok, where = same_planes(got._asdict(), want)
    assert ok, where
    assert got.n_accepted == want["n_accepted"]
    if name in ON_DEVICE_TOO:
        ok, where = same_planes(_into_device_planes(ctx, left.shape, prm), want)
        assert ok, where


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("name", FLIP_CASES)
def test_vertical_flip(ds_ctx, name, paths):
    """the pair turned upside down gives the result turned upside down: no restatement enters"""
    ctx = ds_ctx
    left, right = EDGE_CASES[name][:2]
    prm = dict(n_disp=64, paths=paths)
    _load(ctx, left, right, None)
    a = ctx.denseStereo(0, 1, **prm)
    _load(ctx, np.ascontiguousarray(left[::-1]), np.ascontiguousarray(right[::-1]), None)
    b = ctx.denseStereo(0, 1, **prm)
    ok, where = same_planes(b._asdict(), flipped(a._asdict()))
    assert ok, where
    assert a.n_accepted == b.n_accepted


def test_monotone_grey_remap(ds_ctx):
    """v -> 2 v + 1 keeps every comparison of the census: every plane stays"""
    ctx = ds_ctx
    left, right, mask, prm, _ = EDGE_CASES["grey_0_127"]
    _load(ctx, left, right, mask)
    a = ctx.denseStereo(0, 1, **prm)
    _load(ctx, 2 * left + 1, 2 * right + 1, mask)
    b = ctx.denseStereo(0, 1, **prm)
    ok, where = same_planes(b._asdict(), a._asdict())
    assert ok, where
    assert a.n_accepted == b.n_accepted > 1000


def test_workspace_reused_across_n_disp_paths_and_shapes(vo):
    """one fresh context; the volume's layout changes with n_disp and with the shape, and the first direction must store where the
    others add: every result is its restatement, whatever the volume held before. Device planes, so that the workspace is the only
    thing a call can allocate: the count moves exactly where the bytes vo_dense_stereo_workspace reports pass what is held."""
    wide = EDGE_CASES["uniq_0"][:2]  # the 97 x 21 pair
    n256 = dict(n_disp=256)
    want256 = dense_stereo(*wide, **n256)
    steps = [(EDGE_CASES["sat_n128"], restated("sat_n128")), ((*wide, None, n256, 0), want256), (EDGE_CASES["sat_n64"], restated("sat_n64")),
             (EDGE_CASES["tiny_1x1"], restated("tiny_1x1")), (EDGE_CASES["paths4_p2_8129"], restated("paths4_p2_8129")),
             (EDGE_CASES["sat_n64"], restated("sat_n64"))]
    assert [s[0][3]["n_disp"] for s in steps] == [128, 256, 64, 64, 64, 64] and steps[4][0][3]["paths"] == 4
    c = vo.Context(device=0, max_width=288, max_height=288, max_points=256, n_slots=2, max_level=0)
    try:
        held, moved, expected = 0, [], []
        for k, ((left, right, mask, prm, _), want) in enumerate(steps):
            _load(c, left, right, mask)
            need = c.denseStereoWorkspace(left.shape[1], left.shape[0], **prm)
            assert need == left.size * (16 + 2 * prm["n_disp"])
            expected.append(int(need > held))
            held = max(held, need)
            n0 = c.allocation_count()
            got = _into_device_planes(c, left.shape, prm)
            moved.append(c.allocation_count() - n0)
            ok, where = same_planes(got, want)
            assert ok, (k, where)
        assert moved == expected and expected[0] == 1, (moved, expected)
        for k in (1, 0):  # and through host planes: the context's own copies of the planes are made by the first such call alone
            (left, right, mask, prm, _), want = steps[k]
            _load(c, left, right, mask)
            n1 = c.allocation_count()
            got = c.denseStereo(0, 1, **prm)
            ok, where = same_planes(got._asdict(), want)
            assert ok, (k, where)
            assert k == 1 or c.allocation_count() == n1
    finally:
        c.close()

"""The speckle filter's kernels (csrc/dense_speckle_device.hpp) on CPU threads (tests/emu/emu_dense_speckle.cpp, with the product's launch
geometry: 64 x 16 tiles, a lane per edge pixel, a workgroup per tile, a lane per pixel) against the restatement
(tests/dense_speckle_restatement.py): label, size, status, disparity and sigma equal to the bit, the two counters exact. Generated
planes that are hard for a tiled union-find — a serpentine corridor through every tile, a spiral, U shapes whose arms meet in another
tile, a comb, one component over the frame, a checkerboard of singletons —, the edges of the definition (steps of exactly max_diff
and one float above it, max_size and max_size + 1 pixels, max_size = 0, NaN and Inf, other statuses), odd shapes, and two dense
results. Workgroups in reverse order and on 1, 3 and 8 CPUs give the same bits; once under the address and undefined-behaviour
sanitizers. No GPU."""
import os
import subprocess

import numpy as np
import pytest

from dense_speckle_restatement import DEFAULTS, speckle_filter
from test_semidense_emu import synthetic_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 150, 70  # 3 x 5 tiles of 64 x 16, neither a multiple of the tile


def _planes(valid, disparity=5.0, sigma=0.25):
    valid = np.asarray(valid, bool)
    d = np.where(valid, np.float32(disparity), np.float32(0)).astype(np.float32)
    return d, np.where(valid, np.float32(sigma), np.float32(0)).astype(np.float32), valid.astype(np.uint8)


def _serpentine():
    v = np.zeros((H, W), bool)
    v[0::2, :] = True
    for y in range(1, H, 2):
        v[y, W - 1 if (y // 2) % 2 == 0 else 0] = True
    return _planes(v) + ({},)


def _spiral():
    v = np.zeros((H, W), bool)
    l, t, r, b = 0, 0, W - 1, H - 1
    x = y = 0
    while True:
        if x > r:
            break
        v[y, x:r + 1] = True
        x, t = r, t + 2
        if y > b or t > b:
            break
        v[y:b + 1, x] = True
        y, r = b, r - 2
        if l > r:
            break
        v[y, l:x + 1] = True
        x, b = l, b - 2
        if t > b:
            break
        v[t:y + 1, x] = True
        y, l = t, l + 2
    return _planes(v) + ({},)


def _u_shapes():
    v = np.zeros((H, W), bool)
    v[0:21, 10] = v[0:21, 20] = v[20, 10:21] = True  # arms in tile row 0, joined in tile row 1
    v[3, 30:81] = v[9, 30:81] = v[3:10, 80] = True  # arms in tile column 0, joined in tile column 1
    v[40, 70:141] = v[44, 70:141] = v[40:45, 70] = True  # joined left of the tile the arms end in
    v[48:67, 100] = v[48:67, 104] = v[48, 100:105] = True  # joined above: the smallest index is in the first tile met
    v[50:70, 30] = v[50:70, 34] = v[69, 30:35] = True  # joined in the last, partial tile row
    return _planes(v) + ({},)


def _comb():
    v = np.zeros((H, W), bool)
    v[0, :] = True
    v[:, 0::2] = True
    return _planes(v) + ({},)


def _full():
    return _planes(np.ones((H, W), bool)) + ({},)


def _checkerboard():
    yy, xx = np.mgrid[0:H, 0:W]
    return _planes((xx + yy) % 2 == 0) + ({},)


def _nothing():
    d, s, st = _planes(np.zeros((H, W), bool))
    st[::3, ::2] = 2
    return d, s, st, {}


def _ramp(split):
    """steps of exactly max_diff from column to column: one component though the ends differ by far more; split: one step, on a
    tile's edge, of the next float above max_diff"""
    x = np.arange(W, dtype=np.float32)
    row = np.where(x <= 63, 63 - x, x - 63).astype(np.float32)  # 63 .. 0 | 1 .. : every step is exactly 1
    if split:
        row[64] = np.nextafter(np.float32(1), np.float32(np.inf))  # 63 -> 64: 1 + 2^-23 > 1; 64 -> 65: 1 - 2^-23
    d, s, st = _planes(np.ones((H, W), bool))
    d[:] = row[None, :]
    return d, s, st, dict(max_diff=1.0)


def _sizes(max_size):
    v = np.zeros((H, W), bool)
    v[11:21, 59:69] = True  # 100 pixels over a corner of four tiles
    v[40:50, 100:110] = True  # 101 pixels
    v[40, 110] = True
    v[60:62, 5:55] = True  # 100 pixels in a strip
    v[66, 61:128] = True  # 101 pixels in an L over two tiles' edges
    v[33:67, 128] = True
    return _planes(v) + (dict(max_size=max_size),)


def _nan_inf():
    d, s, st = _planes(np.ones((H, W), bool))
    d[5, 5] = np.nan
    d[20, 70] = d[20, 71] = np.inf  # (Inf - Inf is a NaN: two singletons)
    d[47, 63] = -np.inf
    d[15, 64] = np.float32(np.nan)
    return d, s, st, {}


def _random(w, h, seed, **prm):
    """valid with probability 0.7 among statuses 0, 2..5 whose planes hold arbitrary bits that have to survive; disparities 0..3 with
    a little noise: many components of many sizes"""
    rng = np.random.default_rng(seed)
    st = np.where(rng.random((h, w)) < 0.7, 1, rng.choice([0, 2, 3, 4, 5], (h, w))).astype(np.uint8)
    d = (rng.integers(0, 4, (h, w)) + rng.random((h, w)) * 0.5).astype(np.float32)
    s = rng.random((h, w)).astype(np.float32)
    junk = rng.integers(0, 2 ** 32, (h, w), dtype=np.uint64).astype(np.uint32)
    d.view(np.uint32)[st != 1] = junk[st != 1]  # (NaN payloads and denormals among them)
    return d, s, st, prm


def _dense(name):
    from test_dense_stereo_emu import restated
    pair = synthetic_pair()
    r = restated(pair, name)
    return r["disparity"], r["sigma_invd"], r["status"], dict(max_size=20)


CASES = {
    "serpentine": _serpentine, "spiral": _spiral, "u_shapes": _u_shapes, "comb": _comb, "full": _full, "checkerboard": _checkerboard,
    "nothing_valid": _nothing, "ramp": lambda: _ramp(False), "ramp_split": lambda: _ramp(True),
    "sizes_100": lambda: _sizes(100), "sizes_max_size_0": lambda: _sizes(0), "nan_inf": _nan_inf,
    "statuses_mixed": lambda: _random(W, H, 1, max_size=6), "statuses_mixed_diff_2": lambda: _random(W, H, 2, max_size=40, max_diff=2.0),
    "1x97": lambda: _random(1, 97, 3, max_size=2), "97x1": lambda: _random(97, 1, 4, max_size=2),
    "65x17": lambda: _random(65, 17, 5, max_size=5), "203x37": lambda: _random(203, 37, 6, max_size=5, max_diff=0.75),
    "no_sigma": lambda: (lambda d, s, st, p: (d, None, st, p))(*_random(W, H, 7, max_size=6)),
    "dense_203x37_n128": lambda: _dense("203x37_n128"), "dense_97x21": lambda: _dense("97x21"),
}

_MADE = {}


def case(name):
    """(disparity, sigma_invd or None, status, parameters, the restatement's result) of a case: made once, shared
    (tests/test_dense_speckle_gpu.py too), never changed"""
    if name not in _MADE:
        d, s, st, prm = CASES[name]()
        d, st = np.ascontiguousarray(d, np.float32), np.ascontiguousarray(st, np.uint8)
        s = None if s is None else np.ascontiguousarray(s, np.float32)
        want = speckle_filter(d, s, st, **prm)
        for v in (d, s, st) + tuple(want.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _MADE[name] = (d, s, st, prm, want)
    return _MADE[name]


def same_result(got, want):
    """None where label, size, status, disparity and sigma_invd are the same bits and the counters equal, else where they differ"""
    for k in ("label", "size", "status", "disparity", "sigma_invd"):
        if want[k] is None or (k in ("label", "size") and got.get(k) is None):
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            return (k, len(ys), int(ys[0]), int(xs[0]), got[k][ys[0], xs[0]], want[k][ys[0], xs[0]])
    for k in ("n_removed", "n_components"):
        if got.get(k) is not None and got[k] != want[k]:
            return (k, got[k], want[k])
    return None


def test_the_cases_are_what_they_claim():
    one = lambda name: case(name)[4]
    for name in ("serpentine", "spiral", "comb", "full", "ramp"):
        w = one(name)
        assert w["n_components"] == 1 and w["n_removed"] == 0 and w["label"].max() == 0, name
        tiles = {(y // 16, x // 64) for y, x in zip(*np.nonzero(w["label"] == 0))}
        assert len(tiles) == 15, name  # every tile is visited
    assert one("serpentine")["size"].max() == 35 * W + 35
    assert one("u_shapes")["n_components"] == 5
    cb = one("checkerboard")
    assert cb["n_components"] == cb["n_removed"] == (H * W + 1) // 2 and cb["size"].max() == 1
    assert one("nothing_valid")["n_components"] == 0 and (one("nothing_valid")["label"] == -1).all()
    assert one("ramp_split")["n_components"] == 2
    s100, s0 = one("sizes_100"), one("sizes_max_size_0")
    assert sorted(np.unique(s100["size"]).tolist()) == [0, 100, 101] and s100["n_components"] == 4 and s100["n_removed"] == 200
    assert s0["n_removed"] == 0 and np.array_equal(s0["label"], s100["label"])
    ni = one("nan_inf")
    assert ni["n_components"] == 6 and ni["n_removed"] == 5
    d, s, st, _, mixed = case("statuses_mixed")
    assert set(np.unique(st).tolist()) == {0, 1, 2, 3, 4, 5} and 0 < mixed["n_removed"] < (st == 1).sum()
    keep = mixed["status"] != 6
    assert np.array_equal(mixed["disparity"].view(np.uint32)[keep], d.view(np.uint32)[keep]) and np.array_equal(mixed["status"][keep], st[keep])
    for name in ("dense_203x37_n128", "dense_97x21"):
        assert 0 < one(name)["n_removed"] < (case(name)[2] == 1).sum(), name


def build_emu(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", *flags,
                           os.path.join(ROOT, "tests", "emu", "emu_dense_speckle.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu") / "emu_dense_speckle")


@pytest.fixture(scope="module")
def emu_san(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu_san") / "emu_dense_speckle_san", "-g", "-fsanitize=address,undefined",
                     "-fno-sanitize-recover=all")


def run_emu(exe, tmp_path, d, s, st, prm, reverse=0, cpus=0):
    p = dict(DEFAULTS, **prm)
    h, w = st.shape
    n = w * h
    fi, fo = tmp_path / "in.raw", tmp_path / "out.raw"
    fi.write_bytes(d.tobytes() + (b"" if s is None else s.tobytes()) + st.tobytes())
    subprocess.check_call([exe, str(reverse), str(cpus), str(w), str(h), str(p["max_size"]),
                           "%08x" % int(np.float32(p["max_diff"]).view(np.uint32)), "0" if s is None else "1", str(fi), str(fo)])
    raw = fo.read_bytes()
    ns = 0 if s is None else 4 * n
    assert len(raw) == 4 * n + ns + n + 8 * n + 8
    o = 4 * n + ns
    cnt = np.frombuffer(raw[o + 9 * n:], np.int32)
    return dict(disparity=np.frombuffer(raw[:4 * n], np.float32).reshape(h, w),
                sigma_invd=None if s is None else np.frombuffer(raw[4 * n:o], np.float32).reshape(h, w),
                status=np.frombuffer(raw[o:o + n], np.uint8).reshape(h, w), label=np.frombuffer(raw[o + n:o + 5 * n], np.int32).reshape(h, w),
                size=np.frombuffer(raw[o + 5 * n:o + 9 * n], np.int32).reshape(h, w), n_removed=int(cnt[0]), n_components=int(cnt[1]))


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_text_equals_restatement(emu, tmp_path, name):
    d, s, st, prm, want = case(name)
    assert same_result(run_emu(emu, tmp_path, d, s, st, prm), want) is None


@pytest.mark.parametrize("name,reverse,cpus", [("serpentine", 1, 0), ("u_shapes", 1, 0), ("spiral", 0, 1), ("statuses_mixed", 0, 3),
                                               ("u_shapes", 1, 8), ("dense_203x37_n128", 1, 3)])
def test_workgroup_order_and_cpu_count_do_not_enter(emu, tmp_path, name, reverse, cpus):
    d, s, st, prm, want = case(name)
    assert same_result(run_emu(emu, tmp_path, d, s, st, prm, reverse=reverse, cpus=cpus), want) is None


@pytest.mark.parametrize("name", ["203x37", "u_shapes", "1x97"])
def test_kernel_text_under_the_sanitizers(emu_san, tmp_path, name):
    """exactly sized buffers: an access outside one, or undefined behaviour, ends the program with an error"""
    d, s, st, prm, want = case(name)
    assert same_result(run_emu(emu_san, tmp_path, d, s, st, prm), want) is None

"""The dense stereo kernels (csrc/dense_stereo_device.hpp) on CPU threads (tests/emu/emu_dense_stereo.cpp, with the product's launch
geometry: a launch per direction with one wavefront per path and lanes as disparities, then the decision) against the numpy
restatement (tests/dense_stereo_restatement.py): all four planes equal to the bit. Crops of the synthetic pair (left and right
cropped at the same rows and columns, which keeps disparities): two disparities per lane on a width that is a multiple of nothing,
a small one, one narrower than the range, one taller than wide (the diagonals' start enumeration), d_min > 0, four paths, three and
four disparities per lane, a stride above the width, a mask, a constant right image, the checks switched off. Workgroups in reverse
order and on 1, 3 and 8 CPUs give the same bits; once under the address and undefined-behaviour sanitizers. No GPU."""
import os
import subprocess

import numpy as np
import pytest

from dense_stereo_restatement import DEFAULTS, dense_stereo
from test_semidense_emu import synthetic_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (crop x0, y0, w, h), parameters, stride - w, mask, constant right image
CASES = {
    "203x37_n128": ((300, 150, 203, 37), dict(n_disp=128), 0, False, False),
    "97x21": ((120, 60, 97, 21), dict(n_disp=64), 0, False, False),
    "40x21_narrower_than_the_range": ((120, 60, 40, 21), dict(n_disp=64), 0, False, False),
    "37x120_tall": ((300, 60, 37, 120), dict(n_disp=64), 0, False, False),
    "d_min_3": ((330, 170, 97, 21), dict(d_min=3, n_disp=64), 0, False, False),
    "paths_4": ((120, 60, 97, 21), dict(n_disp=64, paths=4), 0, False, False),
    "stride": ((120, 60, 97, 21), dict(n_disp=64), 13, False, False),
    "mask": ((120, 60, 97, 21), dict(n_disp=64), 0, True, False),
    "constant_right": ((120, 60, 97, 21), dict(n_disp=64), 0, False, True),
    "no_checks": ((120, 60, 97, 21), dict(n_disp=64, uniqueness=0, lr_max=-1), 0, False, False),
    "n192": ((120, 60, 97, 21), dict(n_disp=192), 0, False, False),
    "203x37_n256": ((300, 150, 203, 37), dict(n_disp=256), 0, False, False),
}


def case_inputs(pair, name):
    """left, right, mask (or None), parameters and row padding (stride - width) of a case"""
    L, R, _, bf = pair
    (x0, y0, w, h), prm, pad, masked, const = CASES[name]
    left, right = np.ascontiguousarray(L[y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(R[y0:y0 + h, x0:x0 + w])
    if const:
        right = np.full_like(right, 93)
    mask = None
    if masked:
        mask = np.ones((h, w), np.uint8)
        mask[:, 30:55] = 0
        mask[5:9, :] = 0
        mask[20, 80] = 0
    return left, right, mask, dict(prm, bf=float(bf)), pad


@pytest.fixture(scope="module")
def pair():
    return synthetic_pair()


_WANT = {}


def restated(pair, name):
    """the restatement of a case: computed once, shared (tests/test_dense_stereo_gpu.py too), never changed"""
    if name not in _WANT:
        left, right, mask, prm, _ = case_inputs(pair, name)
        r = dense_stereo(left, right, mask, **prm)
        r.pop("S")
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WANT[name] = r
    return _WANT[name]


def build_emu(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", *flags,
                           os.path.join(ROOT, "tests", "emu", "emu_dense_stereo.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu") / "emu_dense_stereo")


@pytest.fixture(scope="module")
def emu_san(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu_san") / "emu_dense_stereo_san", "-g", "-fsanitize=address,undefined",
                     "-fno-sanitize-recover=all")


def run_emu(exe, tmp_path, left, right, mask, pad, prm, reverse=0, cpus=0):
    p = dict(DEFAULTS, **prm)
    h, w = left.shape
    files = []
    for k, img in enumerate((left, right)):
        buf = np.full((h, w + pad), 0xEE, np.uint8)
        buf[:, :w] = img
        files.append(tmp_path / f"img{k}.raw")
        files[-1].write_bytes(buf.tobytes()[:(w + pad) * (h - 1) + w])
    fm = "-"
    if mask is not None:
        fm = tmp_path / "mask.raw"
        fm.write_bytes(mask.tobytes())
    fo = tmp_path / "out.raw"
    f32 = lambda v: repr(float(np.float32(v)))
    subprocess.check_call([exe, str(reverse), str(cpus), str(w), str(h), str(w + pad), str(p["d_min"]), str(p["n_disp"]), str(p["paths"]),
                           str(p["p1"]), str(p["p2"]), str(p["uniqueness"]), str(p["lr_max"]), f32(p["eps_d"]), f32(p["bf"]),
                           str(files[0]), str(files[1]), str(fm), str(fo)])
    raw = fo.read_bytes()
    n = w * h
    assert len(raw) == 11 * n
    return dict(disparity=np.frombuffer(raw[:4 * n], np.float32).reshape(h, w), cost=np.frombuffer(raw[4 * n:6 * n], np.uint16).reshape(h, w),
                sigma_invd=np.frombuffer(raw[6 * n:10 * n], np.float32).reshape(h, w), status=np.frombuffer(raw[10 * n:], np.uint8).reshape(h, w))


def same_planes(got, want):
    for k in ("status", "cost", "disparity", "sigma_invd"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if a.shape != b.shape or not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            return False, (k, len(ys), int(ys[0]), int(xs[0]), got[k][ys[0], xs[0]], want[k][ys[0], xs[0]])
    return True, None


def test_the_cases_exercise_every_status(pair):
    seen = set()
    for name in CASES:
        want = restated(pair, name)
        seen |= set(np.unique(want["status"]).tolist())
        if name in ("203x37_n128", "97x21"):
            assert want["n_accepted"] >= 1000, (name, want["n_accepted"])
    assert seen == {0, 1, 2, 3, 4}
    const = restated(pair, "constant_right")  # all costs tie: d_best = 0 everywhere, nothing is accepted
    assert (const["status"] == 4).all() and (const["disparity"] == 0).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_text_equals_restatement(emu, pair, tmp_path, name):
    left, right, mask, prm, pad = case_inputs(pair, name)
    got = run_emu(emu, tmp_path, left, right, mask, pad, prm)
    ok, where = same_planes(got, restated(pair, name))
    assert ok, where


@pytest.mark.parametrize("reverse,cpus", [(1, 0), (0, 1), (0, 3), (1, 8)])
def test_workgroup_order_and_cpu_count_do_not_enter(emu, pair, tmp_path, reverse, cpus):
    name = "paths_4" if cpus == 1 else "97x21"
    left, right, mask, prm, pad = case_inputs(pair, name)
    got = run_emu(emu, tmp_path, left, right, mask, pad, prm, reverse=reverse, cpus=cpus)
    ok, where = same_planes(got, restated(pair, name))
    assert ok, where


@pytest.mark.parametrize("name", ["40x21_narrower_than_the_range", "stride"])
def test_kernel_text_under_the_sanitizers(emu_san, pair, tmp_path, name):
    """exactly sized buffers: an access outside one, or undefined behaviour, ends the program with an error"""
    left, right, mask, prm, pad = case_inputs(pair, name)
    got = run_emu(emu_san, tmp_path, left, right, mask, pad, prm)
    ok, where = same_planes(got, restated(pair, name))
    assert ok, where

"""The dense stereo kernels' text on CPU threads (tests/emu/emu_dense_stereo.cpp, built and run through the helpers of
tests/test_dense_stereo_emu.py) on the edge cases of tests/dense_stereo_edge_cases.py against the numpy restatement, all four planes
to the bit: the summed volume above 32767, ties, the penalties and checks at the ends of their ranges, shapes below the census
window and the wavefront. The vertical flip and the grey remap hold on the kernel text without the restatement; the largest
two-disparities-a-lane case and the tie case also with the workgroups reversed on 3 CPUs; the tiny shapes under the address and
undefined-behaviour sanitizers with exactly sized buffers (a stand-alone program). No GPU."""
import numpy as np
import pytest

from dense_stereo_edge_cases import EDGE_CASES, FLIP_CASES, TINY, flipped, restated
from test_dense_stereo_emu import build_emu, run_emu, same_planes


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu") / "emu_dense_stereo")


@pytest.fixture(scope="module")
def emu_san(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu_san") / "emu_dense_stereo_san", "-g", "-fsanitize=address,undefined",
                     "-fno-sanitize-recover=all")


def _run(exe, tmp_path, name, **how):
    left, right, mask, prm, pad = EDGE_CASES[name]
    return run_emu(exe, tmp_path, left, right, mask, pad, prm, **how)


@pytest.mark.parametrize("name", sorted(EDGE_CASES))
def test_kernel_text_equals_restatement(emu, tmp_path, name):
    ok, where = same_planes(_run(emu, tmp_path, name), restated(name))
    assert ok, where


@pytest.mark.parametrize("name", ["sat_n128", "ties_uniq0"])
def test_workgroup_order_and_cpu_count_do_not_enter(emu, tmp_path, name):
    ok, where = same_planes(_run(emu, tmp_path, name, reverse=1, cpus=3), restated(name))
    assert ok, where


@pytest.mark.parametrize("paths", [4, 8])
@pytest.mark.parametrize("name", FLIP_CASES)
def test_vertical_flip_on_the_kernel_text(emu, tmp_path, name, paths):
    left, right = EDGE_CASES[name][:2]
    prm = dict(n_disp=64, paths=paths)
    a = run_emu(emu, tmp_path, left, right, None, 0, prm)
    b = run_emu(emu, tmp_path, np.ascontiguousarray(left[::-1]), np.ascontiguousarray(right[::-1]), None, 0, prm)
    ok, where = same_planes(b, flipped(a))
    assert ok, where


def test_monotone_grey_remap_on_the_kernel_text(emu, tmp_path):
    left, right, mask, prm, pad = EDGE_CASES["grey_0_127"]
    a = run_emu(emu, tmp_path, left, right, mask, pad, prm)
    b = run_emu(emu, tmp_path, 2 * left + 1, 2 * right + 1, mask, pad, prm)
    ok, where = same_planes(b, a)
    assert ok, where


@pytest.mark.parametrize("name", TINY)
def test_tiny_shapes_under_the_sanitizers(emu_san, tmp_path, name):
    """exactly sized buffers: an access outside one, or undefined behaviour, ends the program with an error"""
    ok, where = same_planes(_run(emu_san, tmp_path, name), restated(name))
    assert ok, where

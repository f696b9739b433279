"""CPU suite of MonoVO's debug image (vo_mvo_set_debug_image): the text of csrc/mono_debug_device.hpp — membership in the pose-only
BA's set, inverseSE3_f of the frame's pose, projectToPixel, the draw / keep word — compiled by g++ without contraction, driven as
mvo_debug_gather_kernel drives it and compared bit for bit with the numpy float32 restatement (tests/mono_debug_restatement.py);
the same program once under the address and undefined-behaviour sanitizers; the new entry points in the header and the symbol
list; the compiler's resource report of the gather kernel. The GPU inherits the restatement through tests/
test_mono_debug_image_gpu.py."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import mono_debug_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "emu_mono_debug.cpp")
K = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
SIZES = (0, 1, 11, 300)  # none; one lane; a partial block; more than one block of 256 lanes
FILL = 0xA5


def _compile(tmp, name, extra):
    out = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off"] + extra + [SRC, "-o", out])
    return out


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("emu_mono_debug"), "emu_mono_debug", [])


@pytest.fixture(scope="module")
def emu_sanitized(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("emu_mono_debug_san"), "emu_mono_debug_san",
                    ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _pose(n):
    """A pose with a large rotation (2.2 rad = 126 degrees about a skew axis) and a translation of mixed signs."""
    ax = np.array([0.3, -0.8, 0.52], np.float64)
    ax /= np.linalg.norm(ax)
    a = 2.2
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)
    T[:3, 3] = [0.4, -1.7, 0.9]
    return T.astype(np.float32)


def _case(n):
    """stage 0..4 and ba_ok 0/1 in every combination; points whose depth under the pose is 0, negative and tiny; a NaN pixel."""
    rng = np.random.default_rng(100 + n)
    dT01 = _pose(n)
    stage = (np.arange(n) % 5).astype(np.uint8)
    ba_ok = (np.arange(n) % 3 != 0).astype(np.uint8)
    Xc = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(0.5, 30, n)], axis=1)
    if n >= 11:  # members (stage >= 2 and ba_ok) whose camera-frame depth is chosen
        mem = np.nonzero(R.members(stage, ba_ok))[0]
        Xc[mem[0], 2] = 0.0
        Xc[mem[1], 2] = -4.0
    if n == 1:
        stage[0], ba_ok[0] = 3, 1
    # Xp = T01 Xc in double, rounded once: the depth the float arithmetic finds is close to the chosen one
    T01 = dT01.astype(np.float64)
    Xp = (Xc @ T01[:3, :3].T + T01[:3, 3]).astype(np.float32)
    if n >= 11:
        # depth exactly 0: Xp = (0, 0, x) gives Xc_2 = fl(fl(c x) + t) with c = R10[2][2], |c| < 1, so consecutive x step the
        # product by less than its own spacing and some x near -t / c makes it -t exactly
        T10 = R.inverse_se3(dT01)
        c, t = T10[2, 2], T10[2, 3]
        x = np.float32(-t / c)
        for _ in range(64):
            p = np.float32(c * x)
            if p == -t:
                break
            x = np.nextafter(x, np.float32(np.inf) if (p < -t) == (c > 0) else np.float32(-np.inf))
        Xp[mem[0]] = (0.0, 0.0, x)
        Xp[mem[2]] = (0.0, 0.0, np.nextafter(x, np.float32(np.inf)))  # the tiny depth: one step of the product away from 0
    pts1 = np.stack([rng.uniform(0, 752, n), rng.uniform(0, 480, n)], axis=1).astype(np.float32)
    if n >= 11:
        pts1[mem[3], 0] = np.nan
    return dict(n=n, dT01=dT01, stage=stage, ba_ok=ba_ok, pts1=pts1, Xp=Xp)


def _run(exe, tmp, c, need):
    n = c["n"]
    fin, fout = str(tmp / f"in_{n}_{need}.bin"), str(tmp / f"out_{n}_{need}.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("ii", n, need))
        f.write(K.tobytes() + c["dT01"].tobytes() + c["stage"].tobytes() + c["ba_ok"].tobytes() + c["pts1"].tobytes() + c["Xp"].tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    raw = open(fout, "rb").read()
    assert len(raw) == 16 + 8 * n + 8 * n + n
    ctl = np.frombuffer(raw[:16], np.int32)
    pba = np.frombuffer(raw[16:16 + 8 * n], np.uint32).reshape(n, 2)
    proj = np.frombuffer(raw[16 + 8 * n:16 + 16 * n], np.uint32).reshape(n, 2)
    valid = np.frombuffer(raw[16 + 16 * n:], np.uint8)
    return ctl, pba, proj, valid


def _check(exe, tmp, n, need):
    c = _case(n)
    ctl, pba, proj, valid = _run(exe, tmp, c, need)
    untouched32 = np.uint32(0xA5A5A5A5)
    if need or n == 0:  # keep: the word says so and nothing else is written
        assert ctl[0] == 0
        assert (ctl[1:].view(np.uint32) == untouched32).all()
        assert (pba == untouched32).all() and (proj == untouched32).all() and (valid == FILL).all()
        return c, None
    assert ctl[0] == 1 and ctl[1] == n and (ctl[2:].view(np.uint32) == untouched32).all()
    m = R.members(c["stage"], c["ba_ok"])
    assert np.array_equal(valid, m.astype(np.uint8))
    want_ba, want_proj = R.ba_sets(c["stage"], c["ba_ok"], c["pts1"], c["Xp"], c["dT01"], K)
    assert np.array_equal(pba[m], R.bits(want_ba))
    assert np.array_equal(proj[m], R.bits(want_proj))
    # a non-member's entries are NaN: the drawing rules skip them, so the un-compacted sets draw the compacted sets' picture
    assert np.isnan(pba[~m].view(np.float32)).all() and np.isnan(proj[~m].view(np.float32)).all()
    return c, want_proj


@pytest.mark.parametrize("need", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_gather_text_equals_the_restatement(emu, tmp_path, n, need):
    _check(emu, tmp_path, n, need)


def test_the_cases_hold_what_they_claim():
    """The 11- and 300-feature cases do contain every stage with both ba_ok values, a member at depth exactly 0, one behind the
    camera, one at a tiny depth, and a member with a NaN pixel — and their projections are what float arithmetic makes of them."""
    for n in (11, 300):
        c = _case(n)
        m = R.members(c["stage"], c["ba_ok"])
        mem = np.nonzero(m)[0]
        assert len(mem) >= 4 and (~m).any()
        if n == 300:
            assert {(int(s), int(b)) for s, b in zip(c["stage"], c["ba_ok"])} == {(s, b) for s in range(5) for b in (0, 1)}
        z = R.transform(R.inverse_se3(c["dT01"]), c["Xp"])[:, 2]
        assert z[mem[0]] == 0 and z[mem[1]] < 0 and 0 < abs(z[mem[2]]) < 1e-3, z[mem[:3]]
        proj = R.project(c["dT01"], K, c["Xp"])
        assert not np.isfinite(proj[mem[0]]).all()
        assert np.isnan(c["pts1"][mem[3], 0])
    R0 = _pose(0)[:3, :3].astype(np.float64)
    assert np.degrees(np.arccos((np.trace(R0) - 1) / 2)) > 120


def test_gather_text_under_the_sanitizers(emu_sanitized, tmp_path):
    """The same stand-alone program under -fsanitize=address,undefined: the output arrays hold exactly n entries, so a lane past n
    that read or wrote would be reported."""
    for n in SIZES:
        for need in (0, 1):
            _check(emu_sanitized, tmp_path, n, need)


def test_header_and_symbol_list_name_the_new_entry_points():
    from visual_odometry_ros_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    for name in ("vo_mvo_set_debug_image", "vo_mvo_get_debug_image", "vo_mvo_get_debug_points"):
        assert re.search(r"^int " + name + r"\(vo_mvo \*mvo,", hdr, re.M), name
        assert name in _capi.SYMBOLS
    assert "MonoVO has no such option yet" not in hdr
    assert "#define VO_HIP_ABI_VERSION 3\n" in hdr  # additions only


def test_gather_kernel_uses_no_scratch_memory():
    from visual_odometry_ros_amd import build as B
    if not os.path.exists(B.HIPCC):
        pytest.skip("no hipcc")
    flags = [f for f in B.FLAGS if f not in ("-Wall", "-Wno-unused-function")]
    cmd = [B.HIPCC] + flags + ["-I" + os.path.join(ROOT, "include"), "-I" + B.CSRC, "--offload-device-only",
                               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, "mono_vo.hip"), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    block = r.stderr.split("Function Name: _Z23mvo_debug_gather_kernel")[1].split("Function Name:")[0]
    val = {k: int(re.search(re.escape(k) + r": (\d+)", block).group(1)) for k in ("ScratchSize [bytes/lane]", "VGPRs Spill", "VGPRs")}
    # (one 256-lane workgroup next to a resident replay pool must fit into the 236 registers that pool leaves on a SIMD)
    assert val["ScratchSize [bytes/lane]"] == 0 and val["VGPRs Spill"] == 0 and val["VGPRs"] <= 64, val

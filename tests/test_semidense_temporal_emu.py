"""The temporal semi-dense kernel (csrc/semidense_temporal_device.hpp) on CPU threads (tests/emu/emu_semidense_temporal.cpp, with
the product's launch geometry: 64-column segments x rows, 256 threads, batches of at most 16 candidates) against the numpy
restatement (tests/semidense_temporal_restatement.py): all five planes equal to the bit. Crops of the synthetic stream (the
principal point moves with the crop): forward motion with the epipole inside the crop and a padded stride; sideways motion (the
right image as the current one: C2 = 0); no prior anywhere with max_search 48; the largest and a one-row window; a mask; a
constant current image; a depth range whose near end lies behind the current camera. The first case once more through the same
program built with the address and undefined-behaviour sanitizers: every buffer there has exactly the bytes it holds. No GPU."""
import os
import subprocess

import numpy as np
import pytest

import semidense_restatement as SR
import semidense_temporal_restatement as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = (370.72, 370.72, 319.5, 119.5)

# name -> (crop x0, y0, w, h), motion, parameters, stride - w, prior, mask, constant current image
CASES = {
    "203x61_forward_epipole": ((220, 90, 203, 61), "forward", dict(), 13, True, False, False),
    "97x45_sideways": ((120, 60, 97, 45), "sideways", dict(), 0, True, False, False),
    "no_prior_max48": ((300, 120, 203, 61), "forward", dict(max_search=48), 0, False, False, False),
    "hw15_hh3": ((200, 150, 203, 61), "forward", dict(hw=15, hh=3), 3, True, False, False),
    "hw3_hh0": ((120, 60, 97, 45), "sideways", dict(hw=3, hh=0), 0, True, False, False),
    "mask": ((300, 120, 203, 61), "forward", dict(), 0, True, True, False),
    "constant_current": ((120, 60, 97, 45), "forward", dict(), 0, True, False, True),
    "near_end_behind": ((400, 100, 97, 45), "forward", dict(z_min=0.5), 5, True, False, False),
}


def synthetic_frames():
    """key pair (pose 2), the next left image (pose 3) and T_ck of both motions"""
    from visual_odometry_ros_amd.synthetic import StereoStream
    st = StereoStream(width=640, height=240, K=K, seed=2)
    poses = st.poses(4)
    Lk, Rk, depth = st.render_pair(poses[2])
    Lc, _, _ = st.render_pair(poses[3])
    T_fwd = (np.linalg.inv(poses[3]) @ poses[2]).astype(np.float32)
    T_side = np.eye(4, dtype=np.float32)
    T_side[0, 3] = -np.float32(st.baseline)
    return dict(Lk=Lk, Rk=Rk, Lc=Lc, depth=depth, bf=np.float32(K[0] * st.baseline), forward=T_fwd, sideways=T_side)


def case_inputs(fr, name):
    """key, cur, K, T_ck, map, mask (or None), parameters, row padding of a case"""
    (x0, y0, w, h), motion, prm, pad, prior, masked, const = CASES[name]
    crop = lambda a: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])
    key, right = crop(fr["Lk"]), crop(fr["Rk"])
    cur = crop(fr["Lc"]) if motion == "forward" else right
    if const:
        cur = np.full_like(cur, 93)
    Kc = (K[0], K[1], K[2] - x0, K[3] - y0)
    if prior:
        s = SR.semidense(key, right, d_min=0, d_max=60, bf=float(fr["bf"]))
        m = TR.seed(s["disparity"], s["sigma_invd"], s["status"], fr["bf"])
    else:
        m = TR.empty_map(key.shape)
    mask = None
    if masked:
        mask = np.ones((h, w), np.uint8)
        mask[:, 60:130] = 0
        mask[5:9, :] = 0
        mask[20, 150] = 0
    return key, cur, Kc, fr[motion], m, mask, prm, pad


@pytest.fixture(scope="module")
def frames():
    return synthetic_frames()


def build_emu(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", *flags,
                           os.path.join(ROOT, "tests", "emu", "emu_semidense_temporal.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu") / "emu_semidense_temporal")


def run_emu(exe, tmp_path, key, cur, Kc, T_ck, m, mask, pad, prm, env=None):
    p = dict(TR.DEFAULTS, **prm)
    h, w = key.shape
    files = []
    for k, img in enumerate((key, cur)):
        buf = np.full((h, w + pad), 0xEE, np.uint8)
        buf[:, :w] = img
        files.append(tmp_path / f"img{k}.raw")
        files[-1].write_bytes(buf.tobytes()[:(w + pad) * (h - 1) + w])
    fm = "-"
    if mask is not None:
        fm = tmp_path / "mask.raw"
        fm.write_bytes(mask.tobytes())
    fmap, fo = tmp_path / "map.raw", tmp_path / "out.raw"
    fmap.write_bytes(m["invd"].tobytes() + m["sigma"].tobytes() + m["n_obs"].tobytes() + m["tstatus"].tobytes())
    f32 = lambda v: repr(float(np.float32(v)))
    subprocess.check_call([exe, str(w), str(h), str(w + pad), str(p["hw"]), str(p["hh"]), str(p["g_min"]), f32(p["thres_best"]),
                           f32(p["thres_peak"]), str(p["peak_px"]), str(p["edge_px"]), f32(p["eps_edge"]), f32(p["eps_epi"]), f32(p["z_min"]),
                           f32(p["z_max"]), str(p["max_search"]), f32(p["j_min"]), f32(p["eps_scale"])] + [f32(v) for v in Kc] +
                          [f32(v) for v in np.asarray(T_ck, np.float32).reshape(-1)] + [str(files[0]), str(files[1]), str(fm), str(fmap), str(fo)],
                          env=env)
    raw = fo.read_bytes()
    n = w * h
    f = np.frombuffer(raw[:8 * n], np.float32).reshape(2, h, w)
    b = np.frombuffer(raw[8 * n:10 * n], np.uint8).reshape(2, h, w)
    return dict(invd=f[0], sigma=f[1], n_obs=b[0], tstatus=b[1], score=np.frombuffer(raw[10 * n:14 * n], np.float32).reshape(h, w))


def same_planes(got, want):
    for k in ("tstatus", "n_obs", "invd", "sigma", "score"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            return False, (k, len(ys), int(ys[0]), int(xs[0]), got[k][ys[0], xs[0]], want[k][ys[0], xs[0]])
    return True, None


def test_the_cases_exercise_every_status_and_an_uneven_batch(frames):
    seen = set()
    for name in CASES:
        key, cur, Kc, T, m, mask, prm, _ = case_inputs(frames, name)
        want = TR.temporal(key, cur, Kc, T, m, mask, **prm)
        seen |= set(np.unique(want["tstatus"]).tolist())
        searched = np.isin(want["tstatus"], (1, 2, 3, 4, 5)) | ((want["tstatus"] == 8) & (want["score"] != 0))
        if name in ("203x61_forward_epipole", "97x45_sideways"):
            assert (want["tstatus"] == 1).sum() >= 100, name
            # (the searched candidates of a 64-column segment are no multiple of the batch of 16 somewhere)
            per_seg = [int(searched[y, x:x + 64].sum()) for y in range(key.shape[0]) for x in range(0, key.shape[1], 64)]
            assert any(c % 16 for c in per_seg) and max(per_seg) > 16, name
        if name == "no_prior_max48":
            assert (want["tstatus"] == 6).sum() >= 100 and (want["tstatus"] == 1).sum() >= 20
        if name == "203x61_forward_epipole":  # (the epipole lies inside: no parallax around it)
            assert (want["tstatus"] == 7).sum() >= 20
    assert seen == set(range(9)), seen


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_text_equals_restatement(emu, frames, tmp_path, name):
    key, cur, Kc, T, m, mask, prm, pad = case_inputs(frames, name)
    want = TR.temporal(key, cur, Kc, T, m, mask, **prm)
    got = run_emu(emu, tmp_path, key, cur, Kc, T, m, mask, pad, prm)
    ok, where = same_planes(got, want)
    assert ok, where
    keep = want["tstatus"] != 1  # (what is not accepted keeps its map entry)
    for k in ("invd", "sigma", "n_obs"):
        assert np.array_equal(got[k][keep], m[k][keep]), k
    if name == "constant_current":
        assert not (want["tstatus"] == 1).any() and (want["score"][want["tstatus"] == 2] == -1).all() and (want["tstatus"] == 2).any()
    if name == "mask":
        assert (want["tstatus"][mask == 0] == 0).all()


def test_sanitized_emulation_of_the_first_case(frames, tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined: no tap, key or current, leaves its exactly sized image."""
    exe = build_emu(tmp_path / "emu_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    name = "203x61_forward_epipole"
    key, cur, Kc, T, m, mask, prm, pad = case_inputs(frames, name)
    got = run_emu(exe, tmp_path, key, cur, Kc, T, m, mask, pad, prm)
    ok, where = same_planes(got, TR.temporal(key, cur, Kc, T, m, mask, **prm))
    assert ok, where

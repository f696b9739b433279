"""The propagation kernels (csrc/semidense_propagate_device.hpp) on CPU threads (tests/emu/emu_semidense_propagate.cpp, with the
product's launch geometry: ceil(W H / 256) workgroups of 256 threads, the scatter and then the resolve; hip_emu.h's atomicMax serves
the 64-bit keys) against the numpy restatement (tests/semidense_propagate_restatement.py): all six planes equal to the bit, and the
plane of keys all 0 again. Crops of the synthetic stream (the principal point moves with the crop): the map of pose 2, fused with
poses 3, 4, 5, carried forward to pose 6 (holes, origin 1..3; a padded stride) and backward to pose 0 (many collisions); hand-made
maps: two layers under sideways motion (the near one must win), a fronto-parallel layer under backward translation (exact ties: the
smallest source index wins), a map that disagrees with static (origin 4); a mask; max_diff 0; a pose that puts part of the map
behind the camera; min_obs 2. The first case once more through the same program built with the address and undefined-behaviour
sanitizers: every buffer there has exactly the bytes it holds. No GPU."""
import functools
import os
import subprocess

import numpy as np
import pytest

import semidense_propagate_restatement as PR
import semidense_restatement as SR
import semidense_temporal_restatement as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = (370.72, 370.72, 319.5, 119.5)
F = np.float32
PLANES = ("origin", "src", "n_obs", "tstatus", "invd", "sigma")

# name -> (crop x0, y0, w, h), stride - w, parameters
CASES = {
    "203x61_forward": ((220, 90, 203, 61), 13, dict()),
    "203x61_backward": ((220, 90, 203, 61), 0, dict()),
    "97x45_two_layers": ((0, 0, 97, 45), 0, dict(max_diff=255)),
    "97x45_ties": ((0, 0, 97, 45), 3, dict(max_diff=255)),
    "97x45_inconsistent": ((120, 60, 97, 45), 0, dict(max_diff=255, chi=2.0)),
    "mask": ((300, 120, 203, 61), 0, dict()),
    "max_diff_0": ((300, 120, 203, 61), 0, dict(max_diff=0)),
    "behind_camera": ((270, 98, 97, 45), 5, dict(max_diff=255)),
    "min_obs_2": ((220, 90, 203, 61), 0, dict(min_obs=2, sigma_add=0.0)),
}


@functools.lru_cache(maxsize=None)
def synthetic_setup():
    """the 640 x 240 stream: the left images of poses 0, 2, 6, 7, the map of pose 2 fused with poses 3, 4, 5, the static result of
    pose 6 and its depth — computed once for every test module that asks"""
    from visual_odometry_ros_amd.synthetic import StereoStream
    st = StereoStream(width=640, height=240, K=K, seed=2)
    poses = st.poses(8)
    bf = F(K[0] * st.baseline)
    pairs = {i: st.render_pair(poses[i]) for i in (0, 2, 3, 4, 5, 6, 7)}
    L2, R2, _ = pairs[2]
    s2 = SR.semidense(L2, R2, d_min=0, d_max=67, bf=float(bf))
    m = TR.seed(s2["disparity"], s2["sigma_invd"], s2["status"], bf)
    for i in (3, 4, 5):
        out = TR.temporal(L2, pairs[i][0], K, (np.linalg.inv(poses[i]) @ poses[2]).astype(F), m)
        m = {k: out[k] for k in ("invd", "sigma", "n_obs", "tstatus")}
    L6, R6, z6 = pairs[6]
    s6 = SR.semidense(L6, R6, d_min=0, d_max=67, bf=float(bf))
    T = lambda b, a: (np.linalg.inv(poses[b]) @ poses[a]).astype(F)
    return dict(L0=pairs[0][0], R0=pairs[0][1], L2=L2, L6=L6, L7=pairs[7][0], depth6=z6, map2=m, s6=s6, bf=bf, T_62=T(6, 2), T_02=T(0, 2),
                T_76=T(7, 6))


def empty_static(shape):
    return dict(disparity=np.zeros(shape, F), sigma_invd=np.zeros(shape, F), status=np.zeros(shape, np.uint8))


def case_inputs(fr, name):
    """dict(old, La, Lb, stat, bf, K, T, mask, prm, pad) of a case"""
    (x0, y0, w, h), pad, prm = CASES[name]
    crop = lambda a: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])
    cropd = lambda d, keys: {k: crop(d[k]) for k in keys}
    Kc = (K[0], K[1], K[2] - x0, K[3] - y0)
    c = dict(bf=fr["bf"], K=Kc, mask=None, prm=prm, pad=pad)
    old2 = cropd(fr["map2"], ("invd", "sigma", "n_obs"))
    s6 = cropd(fr["s6"], ("disparity", "sigma_invd", "status"))
    flat = np.full((h, w), 93, np.uint8)
    if name in ("203x61_forward", "mask", "max_diff_0", "min_obs_2"):
        c.update(old=old2, La=crop(fr["L2"]), Lb=crop(fr["L6"]), stat=s6, T=fr["T_62"])
        if name == "mask":
            c["mask"] = np.ones((h, w), np.uint8)
            c["mask"][:, 60:130] = 0
            c["mask"][5:9, :] = 0
            c["mask"][20, 150] = 0
    elif name == "203x61_backward":
        s0 = SR.semidense(crop(fr["L0"]), crop(fr["R0"]), d_min=0, d_max=60, bf=float(fr["bf"]))
        c.update(old=old2, La=crop(fr["L2"]), Lb=crop(fr["L0"]), stat={k: s0[k] for k in ("disparity", "sigma_invd", "status")}, T=fr["T_02"])
    elif name == "97x45_two_layers":  # a far layer everywhere, a near rectangle in front of it; the camera moves sideways
        invd = np.full((h, w), 0.05, F)
        invd[10:30, 40:60] = 0.2
        T = np.eye(4, dtype=F)
        T[0, 3] = -0.2
        c.update(old=dict(invd=invd, sigma=np.full((h, w), 0.01, F), n_obs=np.full((h, w), 3, np.uint8)), La=flat, Lb=flat,
                 stat=empty_static((h, w)), T=T, K=(K[0], K[1], 48.0, 22.0))
    elif name == "97x45_ties":  # one fronto-parallel layer; the camera moves backward: the image shrinks, invd_b is one value
        T = np.eye(4, dtype=F)
        T[2, 3] = 5.0
        c.update(old=dict(invd=np.full((h, w), 0.1, F), sigma=np.full((h, w), 0.01, F), n_obs=np.full((h, w), 2, np.uint8)), La=flat, Lb=flat,
                 stat=empty_static((h, w)), T=T, K=(K[0], K[1], 48.0, 22.0))
    elif name == "97x45_inconsistent":  # the map says half the depth static measures, and is sure of it
        seed = TR.seed(s6["disparity"], s6["sigma_invd"], s6["status"], fr["bf"])
        old = dict(invd=(seed["invd"] * F(2)).astype(F), sigma=(seed["sigma"] * F(0.5)).astype(F), n_obs=(seed["n_obs"] * 4).astype(np.uint8))
        c.update(old=old, La=crop(fr["L6"]), Lb=crop(fr["L6"]), stat=s6, T=np.eye(4, dtype=F))
    elif name == "behind_camera":  # 40 m forward: what is nearer than 44.4 m has D <= 0.1 (the principal point lies inside the crop)
        T = np.eye(4, dtype=F)
        T[2, 3] = -40.0
        c.update(old=old2, La=crop(fr["L2"]), Lb=crop(fr["L6"]), stat=s6, T=T)
    return c


def restate(c):
    return PR.propagate(c["old"], c["La"], c["Lb"], c["stat"], c["bf"], c["K"], c["T"], c["mask"], **c["prm"])


@pytest.fixture(scope="module")
def frames():
    return synthetic_setup()


def build_emu(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", *flags,
                           os.path.join(ROOT, "tests", "emu", "emu_semidense_propagate.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu") / "emu_semidense_propagate")


def run_emu(exe, tmp_path, c):
    p = dict(PR.DEFAULTS, **c["prm"])
    h, w = c["La"].shape
    pad = c["pad"]
    files = []
    for k, img in enumerate((c["La"], c["Lb"])):
        buf = np.full((h, w + pad), 0xEE, np.uint8)
        buf[:, :w] = img
        files.append(tmp_path / f"img{k}.raw")
        files[-1].write_bytes(buf.tobytes()[:(w + pad) * (h - 1) + w])
    fm = "-"
    if c["mask"] is not None:
        fm = tmp_path / "mask.raw"
        fm.write_bytes(c["mask"].tobytes())
    fold, fstat, fo = tmp_path / "old.raw", tmp_path / "static.raw", tmp_path / "out.raw"
    fold.write_bytes(b"".join(np.ascontiguousarray(c["old"][k]).tobytes() for k in ("invd", "sigma", "n_obs")))
    fstat.write_bytes(b"".join(np.ascontiguousarray(c["stat"][k]).tobytes() for k in ("disparity", "sigma_invd", "status")))
    f32 = lambda v: repr(float(F(v)))
    subprocess.check_call([exe, str(w), str(h), str(w + pad), str(p["min_obs"]), str(p["max_diff"]), f32(p["chi"]), f32(p["sigma_add"]), f32(c["bf"])] +
                          [f32(v) for v in c["K"]] + [f32(v) for v in np.asarray(c["T"], F).reshape(-1)] +
                          [str(fold), str(files[0]), str(files[1]), str(fm), str(fstat), str(fo)])
    raw = fo.read_bytes()
    n = w * h
    assert len(raw) == 15 * n + 1
    f = np.frombuffer(raw[:8 * n], F).reshape(2, h, w)
    b = np.frombuffer(raw[12 * n:15 * n], np.uint8).reshape(3, h, w)
    return dict(invd=f[0], sigma=f[1], src=np.frombuffer(raw[8 * n:12 * n], np.int32).reshape(h, w), n_obs=b[0], tstatus=b[1], origin=b[2],
                keys_clean=raw[-1] == 1)


def same_planes(got, want):
    for k in PLANES:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if a.shape != b.shape or not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            return False, (k, len(ys), int(ys[0]), int(xs[0]), got[k][ys[0], xs[0]], want[k][ys[0], xs[0]])
    return True, None


def winners_by_loop(c):
    """target raster index -> (winner's source index, sources kept for it, of which with the winner's invd_b): a direct loop over
    the sources, independent of the restatement's sort"""
    h, w = c["La"].shape
    p = dict(PR.DEFAULTS, **c["prm"])
    old = {k: np.ascontiguousarray(c["old"][k]).reshape(-1) for k in ("invd", "sigma", "n_obs")}
    idx = np.nonzero((old["n_obs"] >= p["min_obs"]) & (old["sigma"] > 0) & (old["invd"] > 0))[0]
    ok, invd_b, _, px, py = PR._warp(idx, old["invd"], old["sigma"], w, c["K"], c["T"], p["sigma_add"])
    X, Y = PR._pix(px), PR._pix(py)
    best = {}
    for i, o, r, x, y in zip(idx, ok, invd_b, X, Y):
        if not o or not (1 <= x <= w - 2 and 1 <= y <= h - 2):
            continue
        if c["mask"] is not None and c["mask"][y, x] == 0:
            continue
        if abs(int(c["La"].reshape(-1)[i]) - int(c["Lb"][y, x])) > p["max_diff"]:
            continue
        b = best.get(y * w + x)
        if b is None or r > b[1]:
            best[y * w + x] = [int(i), r, (b[2] if b else 0) + 1, 1]
        else:
            b[2] += 1
            b[3] += int(r == b[1])  # (sources come in ascending index: the first of equal values stays)
    return {t: (b[0], b[2], b[3]) for t, b in best.items()}


def test_the_cases_meet_their_conditions(frames):
    """every origin value; at least 50 collisions in the backward crop; at least 20 exact ties in the tie case — by the restatement
    alone; and the restatement's winners equal a direct loop's where sources collide"""
    seen = set()
    for name in CASES:
        c = case_inputs(frames, name)
        want = restate(c)
        seen |= set(np.unique(want["origin"]).tolist())
        cnt = want["counts"]
        if name == "203x61_forward":
            assert {1, 2, 3} <= set(np.unique(want["origin"]).tolist()) and (want["origin"] == 0).sum() > 1000
            assert min((want["origin"] == k).sum() for k in (1, 2, 3)) >= 100, cnt
        if name == "203x61_backward":
            assert cnt["collisions"] >= 50, cnt
        if name == "97x45_ties":
            assert cnt["ties"] >= 20, cnt
        if name == "97x45_inconsistent":
            assert (want["origin"] == 4).sum() >= 100 and (want["n_obs"][want["origin"] == 4] == 1).all()
        if name == "behind_camera":
            old = c["old"]
            ys, xs = np.nonzero((old["n_obs"] >= 1) & (old["sigma"] > 0))
            a2 = F(1)  # (no rotation)
            D = a2 + old["invd"][ys, xs] * F(c["T"][2, 3])
            assert (D <= F(0.1)).sum() >= 50 and (D > F(0.1)).sum() >= 50 and (want["origin"] >= 2).any()
        if name == "mask":
            assert (want["origin"][c["mask"] == 0] <= 1).all() and (want["src"][c["mask"] == 0] == -1).all()
        if name == "max_diff_0":
            ys, xs = np.nonzero(want["src"] >= 0)
            assert len(ys) >= 20 and (c["La"].reshape(-1)[want["src"][ys, xs]] == c["Lb"][ys, xs]).all()
        if name == "min_obs_2":
            ys, xs = np.nonzero(want["src"] >= 0)
            assert len(ys) >= 100 and (c["old"]["n_obs"].reshape(-1)[want["src"][ys, xs]] >= 2).all()
        if name in ("203x61_backward", "97x45_two_layers", "97x45_ties"):
            loop = winners_by_loop(c)
            src = want["src"].reshape(-1)
            assert set(np.nonzero(src >= 0)[0].tolist()) == set(loop)
            assert all(src[t] == s for t, (s, _, _) in loop.items())
            assert sum(k - 1 for _, k, _ in loop.values()) == cnt["collisions"] and sum(e - 1 for _, _, e in loop.values()) == cnt["ties"]
    assert seen == {0, 1, 2, 3, 4}, seen


def test_two_layers_the_near_one_wins_every_shared_target(frames):
    c = case_inputs(frames, "97x45_two_layers")
    want = restate(c)
    h, w = c["La"].shape
    loop = winners_by_loop(c)
    near = (c["old"]["invd"] == F(0.2)).reshape(-1)
    ok, _, _, px, py = PR._warp(np.arange(h * w), c["old"]["invd"].reshape(-1), c["old"]["sigma"].reshape(-1), w, c["K"], c["T"], 0.0)
    tgt = PR._pix(py) * w + PR._pix(px)
    shared = set(tgt[near].tolist()) & set(tgt[~near].tolist()) & set(loop)
    assert len(shared) >= 100
    src = want["src"].reshape(-1)
    assert all(near[src[t]] for t in shared)
    assert (want["n_obs"].reshape(-1)[list(shared)] == 3).all() and (want["origin"].reshape(-1)[list(shared)] == 2).all()


def test_ties_the_smallest_source_index_wins(frames):
    c = case_inputs(frames, "97x45_ties")
    want = restate(c)
    h, w = c["La"].shape
    ok, invd_b, _, px, py = PR._warp(np.arange(h * w), c["old"]["invd"].reshape(-1), c["old"]["sigma"].reshape(-1), w, c["K"], c["T"], 0.0)
    assert len(np.unique(invd_b.view(np.uint32))) == 1  # one value: every collision is a tie
    X, Y = PR._pix(px), PR._pix(py)
    inside = (X >= 1) & (X <= w - 2) & (Y >= 1) & (Y <= h - 2)
    tgt = Y * w + X
    src = want["src"].reshape(-1)
    n_tied = 0
    for t in np.unique(tgt[inside]):
        members = np.nonzero(inside & (tgt == t))[0]
        assert src[t] == members.min()
        n_tied += len(members) - 1
    assert n_tied == want["counts"]["ties"] >= 20


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_text_equals_restatement(emu, frames, tmp_path, name):
    c = case_inputs(frames, name)
    want = restate(c)
    got = run_emu(emu, tmp_path, c)
    ok, where = same_planes(got, want)
    assert ok, where
    assert got["keys_clean"]


def test_sanitized_emulation_of_the_first_case(frames, tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined: no access, of an image, the mask, a map or the keys, leaves its
    exactly sized buffer."""
    exe = build_emu(tmp_path / "emu_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    c = case_inputs(frames, "203x61_forward")
    got = run_emu(exe, tmp_path, c)
    ok, where = same_planes(got, restate(c))
    assert ok, where
    assert got["keys_clean"]

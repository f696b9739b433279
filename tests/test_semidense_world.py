"""The world-frame voxel map by its numpy restatement alone (tests/semidense_world_restatement.py; include/vo_hip.h, "Semi-dense world
map"): the cases every other test of the block runs meet their conditions, a plain Python loop over the points equals the
vectorised form, and the guards DESIGN.md §24 quotes hold on the full 640 x 240 maps. The cases are crops of the synthetic stream
(the principal point moves with the crop): the map of pose 2, fused with poses 3, 4, 5, integrated at pose 2, then the seeded static
map of pose 6 at pose 6, with the stream's own poses. No GPU.

capacity_log2 = 12 and the 203 x 61 crop: the definition refuses an integration where occupied + W H exceeds half the table, and
203 x 61 = 12 383 > 2 048, so the crop as ONE integration into 4 096 slots is a refusal by the definition itself (case g asserts
exactly that). The long probe chains are therefore exercised by the same crop cut into strips 5 columns wide (305 pixels each), the two
maps' strips in turn, integrated one after the other into 4 096 slots until the table refuses (case b)."""
import functools

import numpy as np
import pytest

import semidense_temporal_restatement as TR
import semidense_world_restatement as WR
from test_semidense_propagate_emu import K, synthetic_setup

F = np.float32
CROP = (400, 90, 203, 61)
BASE = dict(voxel=0.1, capacity_log2=16, min_obs=1, z_max=30.0)
CASES = {
    "a_203x61": dict(BASE),
    "b_cap12_strips": dict(BASE, capacity_log2=12),
    "c_97x45_plane": dict(BASE, capacity_log2=15),
    "d_rotated_negative": dict(BASE, voxel=0.125),
    "e_out_of_range": dict(BASE),
    "f_min_obs_z_max": dict(BASE, min_obs=2, z_max=20.0),
    "g_refusal": dict(BASE, capacity_log2=12),
    "h_saturation": dict(BASE, capacity_log2=15),
    "i_no_key_plane": dict(BASE),
}


@functools.lru_cache(maxsize=None)
def stream_poses():
    from visual_odometry_ros_amd.synthetic import StereoStream
    return [np.asarray(p, np.float64) for p in StereoStream(width=640, height=240, K=K, seed=2).poses(8)]


@functools.lru_cache(maxsize=None)
def full_maps():
    """(map of pose 2, L2, T_w2), (seeded static map of pose 6, L6, T_w6) at 640 x 240"""
    fr = synthetic_setup()
    s6 = fr["s6"]
    m6 = TR.seed(s6["disparity"], s6["sigma_invd"], s6["status"], fr["bf"])
    P = stream_poses()
    m2 = {k: fr["map2"][k] for k in ("invd", "sigma", "n_obs")}
    return (m2, fr["L2"], P[2].astype(F)), ({k: m6[k] for k in ("invd", "sigma", "n_obs")}, fr["L6"], P[6].astype(F))


def _crop(m, L, x0, y0, w, h):
    c = lambda a: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])
    return {k: c(v) for k, v in m.items()}, c(L), (K[0], K[1], K[2] - x0, K[3] - y0)


def _plane(z, sigma, n_obs=3, w=97, h=45, seed=3):
    m = dict(invd=np.full((h, w), F(1) / F(z), F), sigma=np.full((h, w), sigma, F), n_obs=np.full((h, w), n_obs, np.uint8))
    return m, np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


def _shift(x, y, z):
    T = np.eye(4, dtype=F)
    T[:3, 3] = (x, y, z)
    return T


def case_steps(name):
    """the integrations of a case, in order: dicts map, Lk (or None), pad (the key plane's stride - width), K, T"""
    (m2, L2, T2), (m6, L6, T6) = full_maps()
    x0, y0, w, h = CROP
    step = lambda m, L, Kc, T, pad=0: dict(map=m, Lk=L, pad=pad, K=tuple(float(v) for v in Kc), T=np.asarray(T, F))
    two = [step(*_crop(m2, L2, *CROP), T2, 13), step(*_crop(m6, L6, *CROP), T6)]
    if name in ("a_203x61", "f_min_obs_z_max"):
        return two
    if name == "i_no_key_plane":
        return [dict(s, Lk=None) for s in two]
    if name == "b_cap12_strips":
        return [step(*_crop(m, L, x0 + dx, y0, min(5, w - dx), h), T, dx % 3) for dx in range(0, w, 5) for m, L, T in ((m2, L2, T2), (m6, L6, T6))]
    if name == "c_97x45_plane":  # z = 4 m: a pixel is 4 / 370.72 = 0.0108 m wide, 9 x 9 of them share a voxel of 0.1 m
        m, L = _plane(4.0, 0.01)
        return [step(m, L, (K[0], K[1], 48.0, 22.0), np.eye(4), 3)]
    if name == "d_rotated_negative":
        a, b = 0.7, -0.3
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Ry @ Rx, (-5.0, -3.0, -20.0)
        # z = 8 m and fx = fy = 64: X = (x - 48) / 8, Y = (y - 22) / 8, exact multiples of the voxel 0.125: every point on a face, on all axes
        m, L = _plane(8.0, 0.01)
        Kp = (64.0, 64.0, 48.0, 22.0)
        # the column x = 48 has X = 0: with t_x = -1e-9 its u is a negative number that rounds u - floorf(u) to 1.0f (the clamp to 1023)
        return [step(*_crop(m2, L2, *CROP), T, 5), step(m, L, Kp, _shift(-8.0, -4.0, -16.0)), step(m, L, Kp, _shift(-1e-9, 0.0, 0.0))]
    if name == "e_out_of_range":  # 2^20 voxels of 0.1 m end at 104 857.6 m
        mc, Lc, Kc = _crop(m2, L2, *CROP)
        return [step(mc, Lc, Kc, _shift(104857.0, 0.0, 0.0)), step(mc, Lc, Kc, _shift(0.0, -104858.5, 0.0))]
    if name == "g_refusal":
        return [step(*_crop(m2, L2, x0 + 60, y0 + 10, 40, 30), T2, 1), step(*_crop(m2, L2, *CROP), T2), step(*_crop(m6, L6, x0 + 70, y0 + 10, 20, 30), T6)]
    if name == "h_saturation":
        (ma, L), (mb, _) = _plane(4.0, 1e-9), _plane(4.0, 10.0)
        return [step(ma, L, (K[0], K[1], 48.0, 22.0), np.eye(4)), step(mb, L, (K[0], K[1], 48.0, 22.0), _shift(0.03, 0.0, 0.0))]
    raise KeyError(name)


def run_world(name, loop=False, upto=None):
    w = WR.World(**CASES[name])
    accepted = []
    for s in case_steps(name)[:upto]:
        accepted.append((w.integrate_loop if loop else w.integrate)(s["map"], s["K"], s["T"], s["Lk"]))
    return w, accepted


@functools.lru_cache(maxsize=None)
def restated(name):
    """(the restated table, its sorted records, which steps were accepted) — computed once for every test of any module; not to be modified"""
    w, accepted = run_world(name)
    return w, w.records(), accepted


def same_records(got, want, fields=("key", "index", "sums", "count", "keyframes", "weight", "grey", "xyz")):
    for k in fields:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(a, b):
            bad = np.nonzero((a != b).reshape(len(a), -1).any(1))[0] if a.shape == b.shape else []
            return False, (k, a.shape, b.shape, len(bad), (got[k][bad[0]], want[k][bad[0]]) if len(bad) else None)
    return True, None


def test_the_cases_meet_their_conditions():
    for name in CASES:
        w, rec, accepted = restated(name)
        st, steps = w.stats, case_steps(name)
        n_kf = [int((rec["keyframes"] == k).sum()) for k in (1, 2)]
        print(name, st, "kf 1/2:", n_kf, "max cnt", int(rec["count"].max()))
        assert st["occupied"] == len(rec["key"]) and st["inserted"] == int(rec["count"].sum())
        assert (rec["sums"][:, 0] >= rec["count"]).all() and (np.diff(rec["key"].astype(np.uint64)) > 0).all()
        if name in ("a_203x61", "i_no_key_plane"):
            assert n_kf[0] >= 100 and n_kf[1] >= 100 and rec["count"].max() >= 8 and all(accepted)
            assert (rec["sums"][:, 4] == 0).all() == (name == "i_no_key_plane")
        if name == "b_cap12_strips":
            assert st["refused"] >= 1 and st["integrations"] >= 20 and st["occupied"] > 0.35 * st["capacity"]
        if name == "c_97x45_plane":
            assert st["inserted"] == 97 * 45 and st["inserted"] >= 16 * st["occupied"]
        if name == "d_rotated_negative":
            assert (rec["index"] < 0).any(0).all()
            P1, _, _ = WR.points(steps[1]["map"], steps[1]["K"], steps[1]["T"], steps[1]["Lk"], **CASES[name])
            assert len(P1["key"]) == 97 * 45 and (P1["q"] == 0).all() and (WR.key_index(P1["key"]) < 0).all()  # exactly on faces, negative
            P2, _, _ = WR.points(steps[2]["map"], steps[2]["K"], steps[2]["T"], steps[2]["Lk"], **CASES[name])
            col = P2["x"] == 48
            assert col.sum() == 45 and (WR.key_index(P2["key"])[col, 0] == -1).all() and (P2["q"][col, 0] == 1023).all()
        if name == "e_out_of_range":
            assert st["out_of_range"] >= 50 and st["inserted"] >= 50
        if name == "f_min_obs_z_max":
            by_obs = by_z = 0  # dropped by one gate alone
            for s in steps:
                m = s["map"]
                ent = WR.entries(m)
                with np.errstate(all="ignore"):
                    far = ent & (F(1) / m["invd"] > F(20.0))
                by_obs += int((ent & (m["n_obs"] < 2) & ~far).sum())
                by_z += int((far & (m["n_obs"] >= 2)).sum())
            print(name, "dropped by min_obs alone", by_obs, "by z_max alone", by_z)
            assert by_obs >= 50 and by_z >= 50 and st["skipped"] >= 100 and st["inserted"] >= 100
        if name == "g_refusal":
            assert accepted == [True, False, True] and st["refused"] == 1 and st["integrations"] == 2
            before, _ = run_world(name, upto=1)
            after, _ = run_world(name, upto=2)
            assert same_records(after.records(), before.records())[0] and {**after.stats, "refused": 0} == before.stats
            assert len(rec["key"]) > len(before.key) and w.seq == 3  # (the refused call took a sequence number)
        if name == "h_saturation":
            P0, _, _ = WR.points(steps[0]["map"], steps[0]["K"], steps[0]["T"], steps[0]["Lk"], **CASES[name])
            P1, _, _ = WR.points(steps[1]["map"], steps[1]["K"], steps[1]["T"], steps[1]["Lk"], **CASES[name])
            assert (P0["wq"] == 65536).all() and (P1["wq"] == 1).all() and rec["keyframes"].max() == 2


@pytest.mark.parametrize("name", ["a_203x61", "b_cap12_strips", "d_rotated_negative", "e_out_of_range"])
def test_a_loop_over_the_points_equals_the_vectorised_form(name):
    w, rec, accepted = restated(name)
    wl, acc_l = run_world(name, loop=True)
    assert acc_l == accepted and wl.stats == w.stats
    ok, where = same_records(wl.records(), rec)
    assert ok, where
    print(name, "insertions whose home slot was taken:", wl.home_taken)
    if name == "b_cap12_strips":
        assert wl.home_taken >= 50


# ---- guards: what a user has today (the concatenated per-keyframe clouds) against the voxel map ---------------------------------------
def surface_distance(xyz):
    """CorridorScene is an axis-aligned box: the distance to the nearest of its floor, ceiling and walls"""
    x, y = xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)
    return np.minimum(np.minimum(np.abs(y - 1.65), np.abs(y + 5.0)), np.minimum(np.abs(x + 7.0), np.abs(x - 7.5)))


@functools.lru_cache(maxsize=None)
def guard_figures(voxel):
    """the figures DESIGN.md §24 quotes at this voxel, on the full 640 x 240 maps with min_obs 1 and z_max 30"""
    prm = dict(BASE, voxel=voxel, capacity_log2=20)
    w = WR.World(**prm)
    cloud = []
    for m, L, T in full_maps():
        assert w.integrate(m, K, T, L)
        P, _, _ = WR.points(m, K, T, L, **prm)
        z = 1.0 / m["invd"][P["y"], P["x"]].astype(np.float64)
        X = np.stack([(P["x"] - K[2]) / K[0] * z, (P["y"] - K[3]) / K[1] * z, z, np.ones_like(z)], -1)
        cloud.append((X @ T.astype(np.float64).T)[:, :3])
    cloud = np.concatenate(cloud)
    r1, r2 = w.records(), w.records(min_keyframes=2)
    share = lambda xyz: float((surface_distance(xyz) <= voxel).mean())
    return dict(points=len(cloud), voxels=len(r1["key"]), voxels_kf2=len(r2["key"]), max_count=int(r1["count"].max()),
                share_cloud=share(cloud), share_voxels=share(r1["xyz"]), share_kf2=share(r2["xyz"]))


@pytest.mark.parametrize("voxel", [0.05, 0.1, 0.2])
def test_guards_on_the_full_maps(voxel):
    g = guard_figures(voxel)
    print(voxel, g)
    assert g["voxels"] < g["points"]
    assert g["share_kf2"] > g["share_cloud"]

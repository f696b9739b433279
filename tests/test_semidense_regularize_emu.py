"""The regularisation kernel (csrc/semidense_regularize_device.hpp) on CPU threads (tests/emu/emu_semidense_regularize.cpp, with the
product's launch geometry: ceil(W / 64) x ceil(H / 8) workgroups of 256 threads, one launch) against the numpy restatement
(tests/semidense_regularize_restatement.py): all four planes equal to the bit. The cases: a crop of the synthetic stream's fused
map (a padded key stride; every radius), a hand-made step between two layers with holes on the step, inside a layer, on a flat key
plane and under the mask, single entries and one outlier inside a layer, images smaller than a neighbourhood, sizes one more and one
less than a multiple of the tile's, NaN / inf / negative / zero values sprinkled into the map, and no filling. The first case once
more through the same program built with the address and undefined-behaviour sanitizers: every buffer there has exactly the bytes it
holds. The quality guards run the restatement alone on the full 640 x 240 map against the renderer's depth. No GPU."""
import functools
import os
import subprocess

import numpy as np
import pytest

import semidense_regularize_restatement as RR
from test_semidense_propagate_emu import synthetic_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PLANES = ("rstatus", "n_obs", "invd", "sigma")
CROP = (220, 90, 203, 61)
TILE = (64, 8)
FAR, NEAR = F(0.05), F(0.2)

# name -> parameters (the inputs: case_inputs)
CASES = {
    "a_203x61": dict(),
    "b_radius_1": dict(radius=1, min_support=2, fill_min=3),
    "b_radius_3": dict(radius=3, fill_min=12),
    "c_97x45_step": dict(),
    "d_singles": dict(),
    "d_singles_min_support_0": dict(min_support=0),
    "e_3x3": dict(radius=3, fill_min=3),
    "e_5x5": dict(radius=3, fill_min=3),
    "e_9x7": dict(radius=3, fill_min=3),
    "f_129x17": dict(),
    "f_127x15": dict(),
    "g_nonfinite": dict(),
    "h_no_fill": dict(fill_min=0),
}

# (c): the near rectangle, and the holes by kind (y, x)
RECT = (10, 30, 40, 60)  # rows 10..29, columns 40..59
STEP_HOLES = ([(9, x) for x in range(40, 60, 2)] + [(30, x) for x in range(41, 60, 2)] + [(y, 39) for y in range(11, 29, 2)] +
              [(y, 60) for y in range(10, 29, 2)] + [(10, x) for x in range(43, 58, 3)])
INNER_HOLES = ([(4, x) for x in range(5, 80, 5)] + [(33, x) for x in range(5, 80, 5)] + [(15, 47), (20, 45), (20, 50), (20, 55), (25, 52)])
FLAT_HOLES = [(40, x) for x in range(5, 80, 5)]
MASKED_HOLES = [(y, 88) for y in range(5, 35, 5)]
# (d): single entries, and the outlier inside the layer of rows 12..26, columns 20..34
SINGLES = [(3, 3), (3, 12), (8, 36), (25, 5), (0, 39), (29, 0)]
OUTLIER = (19, 27)


def _random_map(h, w, seed):
    rng = np.random.default_rng(seed)
    ent = rng.random((h, w)) < 0.6
    invd = np.where(ent, F(0.1) + rng.normal(0, 0.004, (h, w)).astype(F), F(0)).astype(F)
    sigma = np.where(ent, rng.uniform(0.005, 0.02, (h, w)).astype(F), F(0)).astype(F)
    return dict(invd=invd, sigma=sigma, n_obs=np.where(ent, rng.integers(1, 6, (h, w)), 0).astype(np.uint8)), rng.integers(0, 256, (h, w)).astype(np.uint8)


def case_inputs(fr, name):
    """dict(map, Lk, mask, prm, pad) of a case"""
    prm = CASES[name]
    c = dict(mask=None, prm=prm, pad=0)

    def crop_of(x0, y0, w, h):
        crop = lambda a: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])
        return {k: crop(fr["map2"][k]) for k in ("invd", "sigma", "n_obs")}, crop(fr["L2"])

    if name[0] in "abgh":
        c["map"], c["Lk"] = crop_of(*CROP)
        c["pad"] = 13
        if name == "g_nonfinite":
            m = {k: v.copy() for k, v in c["map"].items()}
            h, w = c["Lk"].shape
            rng = np.random.default_rng(5)
            ys, xs = rng.integers(0, h, 90), rng.integers(0, w, 90)
            bad = [("invd", np.nan), ("invd", np.inf), ("invd", -0.1), ("invd", 0.0), ("sigma", np.nan), ("sigma", np.inf), ("sigma", -0.01),
                   ("sigma", 0.0), ("n_obs", 0)]
            for i, (y, x) in enumerate(zip(ys, xs)):
                k, v = bad[i % len(bad)]
                m["invd"][y, x], m["sigma"][y, x], m["n_obs"][y, x] = F(0.08), F(0.01), 2  # (non-zero values under n_obs = 0 too)
                m[k][y, x] = v
            c["map"], c["bad"] = m, (ys, xs)
    elif name == "c_97x45_step":
        h, w = 45, 97
        invd = np.full((h, w), FAR, F)
        invd[RECT[0]:RECT[1], RECT[2]:RECT[3]] = NEAR
        m = dict(invd=invd, sigma=np.full((h, w), 0.01, F), n_obs=np.full((h, w), 3, np.uint8))
        for y, x in STEP_HOLES + INNER_HOLES + FLAT_HOLES + MASKED_HOLES:
            m["invd"][y, x], m["sigma"][y, x], m["n_obs"][y, x] = 0, 0, 0
        Lk = np.empty((h, w), np.uint8)
        Lk[:] = 60 + 100 * ((np.arange(w) // 2) % 2)  # stripes two pixels wide: |gx| = 100 everywhere
        Lk[37:] = 93                                  # flat: no gradient from row 38 on
        c["mask"] = np.ones((h, w), np.uint8)
        c["mask"][:, 80:] = 0
        c.update(map=m, Lk=Lk, pad=3)
    elif name.startswith("d_singles"):
        h, w = 30, 40
        m = dict(invd=np.zeros((h, w), F), sigma=np.zeros((h, w), F), n_obs=np.zeros((h, w), np.uint8))
        m["invd"][12:27, 20:35], m["sigma"][12:27, 20:35], m["n_obs"][12:27, 20:35] = FAR, 0.005, 2
        m["invd"][OUTLIER] = FAR / F(2)  # twice the depth
        for y, x in SINGLES:
            m["invd"][y, x], m["sigma"][y, x], m["n_obs"][y, x] = F(0.07), F(0.01), 4
        c.update(map=m, Lk=np.full((h, w), 93, np.uint8))
    elif name[0] == "e":
        w, h = (int(v) for v in name[2:].split("x"))
        c["map"], c["Lk"] = _random_map(h, w, 7 + w)
        for k in c["map"]:
            c["map"][k][h // 2, w // 2] = 0  # a hole in the middle (of 3 x 3 the only pixel that may be filled)
        c["Lk"][h // 2, w // 2 - 1], c["Lk"][h // 2, w // 2 + 1] = 10, 200
        c["pad"] = 1
    elif name[0] == "f":
        w, h = (int(v) for v in name[2:].split("x"))
        c["map"], c["Lk"] = crop_of(CROP[0], CROP[1], w, h)
    return c


def restate(c):
    return RR.regularize(c["map"], c["Lk"], c["mask"], **c["prm"])


@pytest.fixture(scope="module")
def frames():
    return synthetic_setup()


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement of a case, computed once for every test (of any module) that asks; not to be modified"""
    c = case_inputs(synthetic_setup(), name)
    return c, restate(c)


def build_emu(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", *flags,
                           os.path.join(ROOT, "tests", "emu", "emu_semidense_regularize.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu") / "emu_semidense_regularize")


def run_emu(exe, tmp_path, c):
    p = dict(RR.DEFAULTS, **c["prm"])
    h, w = c["Lk"].shape
    pad = c["pad"]
    buf = np.full((h, w + pad), 0xEE, np.uint8)
    buf[:, :w] = c["Lk"]
    fk = tmp_path / "key.raw"
    fk.write_bytes(buf.tobytes()[:(w + pad) * (h - 1) + w])
    fm = "-"
    if c["mask"] is not None:
        fm = tmp_path / "mask.raw"
        fm.write_bytes(c["mask"].tobytes())
    fmap, fo = tmp_path / "map.raw", tmp_path / "out.raw"
    fmap.write_bytes(b"".join(np.ascontiguousarray(c["map"][k]).tobytes() for k in ("invd", "sigma", "n_obs")))
    f32 = lambda v: repr(float(F(v)))
    subprocess.check_call([exe, str(w), str(h), str(w + pad), str(p["radius"]), f32(p["chi"]), f32(p["dist_sigma"]), str(p["min_support"]),
                           str(p["fill_min"]), str(p["g_min"]), str(fmap), str(fk), str(fm), str(fo)])
    raw = fo.read_bytes()
    n = w * h
    assert len(raw) == 10 * n
    f = np.frombuffer(raw[:8 * n], F).reshape(2, h, w)
    b = np.frombuffer(raw[8 * n:], np.uint8).reshape(2, h, w)
    return dict(invd=f[0], sigma=f[1], n_obs=b[0], rstatus=b[1])


def same_planes(got, want):
    for k in PLANES:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if a.shape != b.shape or not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            return False, (k, len(ys), int(ys[0]), int(xs[0]), got[k][ys[0], xs[0]], want[k][ys[0], xs[0]])
    return True, None


def at(plane, pts):
    return np.array([plane[y, x] for y, x in pts])


def test_the_cases_meet_their_conditions():
    """by the restatement alone: the crop has every kind of pixel in numbers; every rstatus value occurs; the step refuses its edge
    holes and fills the inner ones; the singles and the outlier go the way the rules say; no NaN leaves a map that holds some"""
    seen = set()
    for name in CASES:
        c, want = restated(name)
        rs = want["rstatus"]
        seen |= set(np.unique(rs).tolist())
        n = [int((rs == k).sum()) for k in range(4)]
        ent = RR.entries(c["map"])
        assert ((rs == 1) | (rs == 2))[ent].all() and not ((rs == 1) | (rs == 2))[~ent].any()
        assert (want["invd"][(rs == 0) | (rs == 2)] == 0).all() and (want["n_obs"][(rs == 0) | (rs == 2)] == 0).all()
        assert (want["n_obs"][rs == 1] == c["map"]["n_obs"][rs == 1]).all() and (want["n_obs"][rs == 3] == 1).all()
        assert not np.isnan(want["invd"]).any() and not np.isnan(want["sigma"]).any(), name
        if name == "a_203x61":
            print(name, n)
            assert n[1] >= 100 and n[3] >= 100 and n[2] >= 10, n
        if name.startswith("b_"):
            assert n[1] >= 100 and n[3] >= 20 and n[2] >= 1, (name, n)
        if name == "c_97x45_step":
            layer = np.full(rs.shape, FAR, F)
            layer[RECT[0]:RECT[1], RECT[2]:RECT[3]] = NEAR
            kept = (rs == 1) | (rs == 3)
            assert (np.abs(want["invd"] - layer)[kept] <= F(1e-5) * layer[kept]).all()
            assert len(STEP_HOLES) >= 20 and (at(rs, STEP_HOLES) == 0).all() and not at(want["filled"], STEP_HOLES).any()
            assert len(INNER_HOLES) >= 20 and (at(rs, INNER_HOLES) == 3).all()
            assert (at(rs, FLAT_HOLES) == 0).all() and (at(rs, MASKED_HOLES) == 0).all()
            assert n[3] == len(INNER_HOLES)
        if name == "d_singles":
            assert (at(rs, SINGLES) == 2).all() and rs[OUTLIER] == 2 and n[3] == 0
            assert n[2] == len(SINGLES) + 1  # nothing else goes: the layer's corners have 8 consistent neighbours
        if name == "d_singles_min_support_0":
            assert (at(rs, SINGLES) == 1).all()
            assert rs[OUTLIER] == 2 and want["support"][OUTLIER] == 0 and want["conflict"][OUTLIER] == 24  # the conflict rule alone
        if name[0] == "e":
            assert n[1] >= 3 and n[3] >= 1, (name, n)
        if name[0] == "f":
            h, w = rs.shape
            assert (w % TILE[0] in (1, TILE[0] - 1)) and (h % TILE[1] in (1, TILE[1] - 1)) and rs[:, TILE[0]:].any() and rs[TILE[1]:].any()
        if name == "g_nonfinite":
            ys, xs = c["bad"]
            assert not ent[ys, xs].any() and np.isin(rs[ys, xs], (0, 3)).all()
            assert np.isnan(c["map"]["invd"]).any() and np.isinf(c["map"]["sigma"]).any()
        if name == "h_no_fill":
            assert n[3] == 0 and n[1] >= 100
    assert seen == {0, 1, 2, 3}, seen


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_text_equals_restatement(emu, tmp_path, name):
    c, want = restated(name)
    got = run_emu(emu, tmp_path, c)
    ok, where = same_planes(got, want)
    assert ok, where


def test_sanitized_emulation_of_the_first_case(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined: no access, of the key plane, the mask or a map plane, leaves its
    exactly sized buffer."""
    exe = build_emu(tmp_path / "emu_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    c, want = restated("a_203x61")
    ok, where = same_planes(run_emu(exe, tmp_path, c), want)
    assert ok, where


# ---- quality guards: the restatement on the full 640 x 240 map of pose 2 against the renderer's depth ---------------------------------
@functools.lru_cache(maxsize=None)
def quality():
    """the figures DESIGN.md §23 quotes; errors are |1 / invd - z| / z"""
    from visual_odometry_ros_amd.synthetic import StereoStream
    from test_semidense_propagate_emu import K
    fr = synthetic_setup()
    st = StereoStream(width=640, height=240, K=K, seed=2)
    z = st.render_pair(st.poses(8)[2])[2]
    m = fr["map2"]
    out = RR.regularize(m, fr["L2"])
    ent, rs = RR.entries(m), out["rstatus"]
    err = lambda invd, sel: np.abs(1.0 / invd[sel].astype(np.float64) - z[sel]) / z[sel]
    stats = lambda e: dict(n=int(len(e)), median=float(np.median(e)), within5=float((e <= 0.05).mean()), above20=float((e > 0.2).mean()),
                           n_above20=int((e > 0.2).sum()))
    kept = rs == 1
    return dict(raw=stats(err(m["invd"], ent)), kept_raw=stats(err(m["invd"], kept)), kept=stats(err(out["invd"], kept)),
                removed=stats(err(m["invd"], rs == 2)), filled=stats(err(out["invd"], rs == 3)),
                conflict_only=stats(err(m["invd"], (rs == 2) & (out["support"] >= 1))))


def test_quality_guards_on_the_full_map():
    """Robustness and coverage, not precision: against the raw values on the same pixels the kept pixels have strictly fewer errors
    above 20 %, a strictly larger share within 5 % and a median at most 1.05 x the raw one; the filled pixels' share within 5 % is
    at least the raw map's minus 0.01; the removed set's share of errors above 20 % exceeds the raw map's."""
    q = quality()
    for k, v in q.items():
        print(k, v)
    assert q["kept"]["n_above20"] < q["kept_raw"]["n_above20"]
    assert q["kept"]["within5"] > q["kept_raw"]["within5"]
    assert q["kept"]["median"] <= 1.05 * q["kept_raw"]["median"]
    assert q["filled"]["within5"] >= q["raw"]["within5"] - 0.01
    assert q["removed"]["above20"] > q["raw"]["above20"]

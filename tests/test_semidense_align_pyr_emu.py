"""The kernels of the coarse-to-fine alignment (csrc/semidense_map_pyramid_device.hpp, csrc/semidense_align_device.hpp) on CPU threads
(tests/emu/emu_semidense_align_pyr.cpp, with the product's launches: one map pyramid launch per level, then per level from the top
down its iterations' launches, the first of a level taking the pose over) against the numpy restatement
(tests/semidense_align_pyr_restatement.py): every field, final and per level, and every plane of the map pyramid equal to the bit.
Crops of the synthetic stream's fused map where a coarse level can go wrong: 203 x 61 with 3 levels (odd sizes at every level,
102 x 31 and 51 x 16, and a padded stride); 97 x 45 with 3 levels (49 x 23 and 25 x 12: the top level is smaller than one block); a
31 x 29 map with 2 levels; a top level that ends with status 2 (min_pixels above its count) and hands its pose down; unequal
iteration counts per level. The first case once more through the same stand-alone program built with the address and
undefined-behaviour sanitizers: every buffer there has exactly the bytes it holds. No GPU."""
import os
import subprocess

import numpy as np
import pytest

import semidense_align_pyr_restatement as PR
import semidense_align_restatement as AR
from test_semidense_align_emu import K, XI_START, perturbed, same_result, synthetic_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

# name -> (crop x0, y0, w, h), parameters, stride - w, the start's perturbation in units of XI_START
CASES = {
    "203x61_3_levels": ((220, 90, 203, 61), dict(levels=3, max_iters=6, min_pixels=50), 13, 1.0),
    "97x45_3_levels_top_below_a_block": ((120, 60, 97, 45), dict(levels=3, min_pixels=20), 0, 0.6),
    "31x29_2_levels": ((330, 150, 31, 29), dict(levels=2, min_pixels=20), 3, 0.3),
    "top_level_status_2": ((220, 90, 203, 61), dict(levels=3, max_iters=5, min_pixels=1000), 5, 0.6),
    "iterations_per_level": ((300, 120, 203, 61), dict(levels=3, max_iters=4, max_iters_level=(3, 0, 7), min_pixels=50, huber=6.0), 0, 1.0),
}


def case_inputs(fr, pyr_down, name):
    """key levels, current levels, K, T_start, level-0 map, parameters, row padding of a case"""
    (x0, y0, w, h), prm, pad, scale = CASES[name]
    crop = lambda a: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])
    L = prm["levels"]
    key, cur = PR.image_pyramid(crop(fr["L"][2]), L, pyr_down), PR.image_pyramid(crop(fr["L"][3]), L, pyr_down)
    T = perturbed(fr["T"][3], scale * np.asarray(XI_START))
    Kc = (K[0], K[1], K[2] - x0, K[3] - y0)
    m = {k: crop(fr["map2"][k]) for k in ("invd", "sigma", "n_obs")}
    return key, cur, Kc, T, m, prm, pad


@pytest.fixture(scope="module")
def frames():
    return synthetic_setup()


@pytest.fixture(scope="module")
def pyr_down(oracle):
    return oracle.pyr_down


def build_emu(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", *flags,
                           os.path.join(ROOT, "tests", "emu", "emu_semidense_align_pyr.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu") / "emu_semidense_align_pyr")


def run_emu(exe, tmp_path, key, cur, Kc, T, m, pad, prm):
    """the stand-alone program's result: the final fields as align returns them, levels=[per level dict], maps=[per level dict]"""
    p = dict(PR.DEFAULTS, **prm)
    L, iters = p["levels"], PR.level_iters(p)
    files = []
    for k, levels in enumerate((key, cur)):
        raw = b""
        for img in levels:
            h, w = img.shape
            buf = np.full((h, w + pad), 0xEE, np.uint8)
            buf[:, :w] = img
            raw += buf.tobytes()[:(w + pad) * (h - 1) + w]
        files.append(tmp_path / f"img{k}.raw")
        files[-1].write_bytes(raw)
    fmap, fo = tmp_path / "map.raw", tmp_path / "out.raw"
    fmap.write_bytes(np.ascontiguousarray(m["invd"], F).tobytes() + np.ascontiguousarray(m["sigma"], F).tobytes() +
                     np.ascontiguousarray(m["n_obs"], np.uint8).tobytes())
    f32 = lambda v: repr(float(F(v)))
    h0, w0 = key[0].shape
    subprocess.check_call([exe, str(w0), str(h0), str(pad), str(L), str(p["min_obs"]), f32(p["huber"]), f32(p["eps"]), str(p["min_pixels"])] +
                          [str(v) for v in (iters + [1] * 6)[:6]] + [f32(v) for v in Kc] + [f32(v) for v in np.asarray(T, F).reshape(-1)] +
                          [str(files[0]), str(files[1]), str(fmap), str(fo)])
    raw = fo.read_bytes()
    ints = np.frombuffer(raw[64:80], np.int32)
    d = np.frombuffer(raw[80:80 + 8 * 29], np.float64)
    off = 80 + 8 * 29
    lv_i = np.frombuffer(raw[off:off + 96], np.int32).reshape(6, 4)
    lv_d = np.frombuffer(raw[off + 96:off + 192], np.float64).reshape(6, 2)
    off += 192

    def rms(swrr, sw):
        with np.errstate(all="ignore"):
            return float(np.sqrt(swrr / sw) / np.float64(16)) if sw > 0 else 0.0
    out = dict(T_ck=np.frombuffer(raw[:64], F).reshape(4, 4), status=int(ints[0]), iters=int(ints[1]), count=int(ints[2]), start_prev=int(ints[3]),
               rms=rms(d[0], d[1]), H=d[2:23], b=d[23:29])
    out["levels"] = [dict(status=int(lv_i[l, 0]), iters=int(lv_i[l, 1]), count=int(lv_i[l, 2]), launches=int(lv_i[l, 3]), rms=rms(*lv_d[l]))
                     for l in range(L)]
    maps = [None]
    for l in range(1, L):
        w, h = PR.level_size(w0, h0, l)
        n = w * h
        maps.append(dict(invd=np.frombuffer(raw[off:off + 4 * n], F).reshape(h, w), sigma=np.frombuffer(raw[off + 4 * n:off + 8 * n], F).reshape(h, w),
                         n_obs=np.frombuffer(raw[off + 8 * n:off + 9 * n], np.uint8).reshape(h, w)))
        off += 9 * n
    assert off == len(raw)
    out["maps"] = maps
    return out


def same_levels(got, want):
    """the per-level fields, bit for bit: (ok, the first that differs)"""
    if len(got) != len(want):
        return False, ("levels", len(got), len(want))
    for l, (g, w) in enumerate(zip(got, want)):
        for k in ("status", "iters", "count"):
            if int(g[k]) != int(w[k]):
                return False, (l, k, g[k], w[k])
        if np.float64(g["rms"]).tobytes() != np.float64(w["rms"]).tobytes():
            return False, (l, "rms", g["rms"], w["rms"])
    return True, None


def same_maps(got, want):
    """levels 1.. of a map pyramid, every plane bit for bit: (ok, the first that differs)"""
    for l in range(1, len(want)):
        for k, dt in (("invd", np.uint32), ("sigma", np.uint32), ("n_obs", np.uint8)):
            a, b = np.ascontiguousarray(got[l][k]), np.ascontiguousarray(want[l][k])
            if a.shape != b.shape or not np.array_equal(a.view(dt), b.view(dt)):
                return False, (l, k)
    return True, None


def pixels(m, min_obs=1):
    return int(((m["n_obs"] >= min_obs) & (m["sigma"] > 0) & (m["invd"] > 0)).sum())


def test_the_cases_exercise_what_they_name(frames, pyr_down):
    for name in CASES:
        key, cur, Kc, T, m, prm, pad = case_inputs(frames, pyr_down, name)
        want = PR.align_pyr(key, cur, Kc, T, m, **prm)
        L = prm["levels"]
        sizes = [k.shape[::-1] for k in key]
        maps = PR.map_pyramid(m, L)
        print(name, sizes, [pixels(x) for x in maps], want["levels"])
        assert [x["invd"].shape[::-1] for x in maps] == sizes
        if name == "203x61_3_levels":
            assert sizes == [(203, 61), (102, 31), (51, 16)] and pad > 0 and all(d["status"] in (0, 1) and d["iters"] > 1 for d in want["levels"])
        if name == "97x45_3_levels_top_below_a_block":
            assert sizes == [(97, 45), (49, 23), (25, 12)] and 25 * 12 < AR.BLOCK and want["levels"][2]["status"] in (0, 1)
        if name == "31x29_2_levels":
            assert sizes == [(31, 29), (16, 15)] and want["levels"][1]["count"] >= 20
        if name == "top_level_status_2":  # the top level has too few pixels: one evaluation, the pose handed down, the next level runs
            assert want["levels"][2]["status"] == 2 and want["levels"][2]["iters"] == 1 and 0 < want["levels"][2]["count"] < prm["min_pixels"]
            assert want["levels"][1]["status"] in (0, 1) and want["levels"][1]["count"] >= prm["min_pixels"] and want["status"] in (0, 1)
        if name == "iterations_per_level":
            assert PR.level_iters(dict(PR.DEFAULTS, **prm)) == [3, 4, 7]
            assert want["levels"][2]["iters"] > 4 and want["levels"][0]["status"] == 1 and want["levels"][0]["iters"] == 3


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_text_equals_restatement(emu, frames, pyr_down, tmp_path, name):
    key, cur, Kc, T, m, prm, pad = case_inputs(frames, pyr_down, name)
    want = PR.align_pyr(key, cur, Kc, T, m, **prm)
    got = run_emu(emu, tmp_path, key, cur, Kc, T, m, pad, prm)
    ok, where = same_maps(got["maps"], PR.map_pyramid(m, prm["levels"]))
    assert ok, where
    ok, where = same_result(got, want)
    assert ok, where
    ok, where = same_levels(got["levels"], want["levels"])
    assert ok, where
    assert [d["launches"] for d in got["levels"]] == [d["iters"] for d in want["levels"]]  # (a launch behind its level's "done" returns at once)
    assert got["start_prev"] == 0 and np.isfinite(got["T_ck"]).all()


def test_one_level_is_the_level_0_operator(emu, frames, pyr_down, tmp_path):
    key, cur, Kc, T, m, prm, pad = case_inputs(frames, pyr_down, "203x61_3_levels")
    prm = dict(prm, levels=1)
    got = run_emu(emu, tmp_path, key[:1], cur[:1], Kc, T, m, pad, prm)
    ok, where = same_result(got, AR.align(key[0], cur[0], Kc, T, m, **{k: v for k, v in prm.items() if k != "levels"}))
    assert ok, where


def test_sanitized_emulation_of_the_first_case(frames, pyr_down, tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined: no access, to an image level or to a level of the map, leaves
    its exactly sized buffer."""
    exe = build_emu(tmp_path / "emu_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    key, cur, Kc, T, m, prm, pad = case_inputs(frames, pyr_down, "203x61_3_levels")
    prm = dict(prm, max_iters=2)
    got = run_emu(exe, tmp_path, key, cur, Kc, T, m, pad, prm)
    ok, where = same_result(got, PR.align_pyr(key, cur, Kc, T, m, **prm))
    assert ok, where
    ok, where = same_maps(got["maps"], PR.map_pyramid(m, prm["levels"]))
    assert ok, where

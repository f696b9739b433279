"""The kernel of the alignment with affine brightness (csrc/semidense_align_affine_device.hpp) on CPU threads
(tests/emu/emu_semidense_align_affine.cpp, with the product's launches: the map pyramid's, then per level from the top down its
iterations' launches, the first of a level taking pose and brightness over) against the numpy restatement
(tests/semidense_align_affine_restatement.py): every result field, G and O, the state after each level, every plane of the map
pyramid and the 47 per-block sums of the first iteration equal to the bit. The crops of tests/test_semidense_align_pyr_emu.py with
the current image mapped by clip(round(0.7 I + 25)) — 203 x 61 with a padded stride and 3 levels, 97 x 45 with 3 levels (the top
level is smaller than one block), 31 x 29 with 2 levels —, the first once more unchanged (1, 0); gain0 = 8 against a black image
(status 5 at either level, the state handed down as started); a top level that ends with status 2 and hands T, G, O down (a start
gain0 = 0.8, offset0 = 20, so that what is handed down is not the default). The first case once more through the same stand-alone
program built with the address and undefined-behaviour sanitizers: every buffer there has exactly the bytes it holds. No GPU."""
import os
import subprocess

import numpy as np
import pytest

import semidense_align_affine_restatement as FR
import semidense_align_pyr_restatement as PR
import semidense_align_restatement as AR
from test_semidense_align_emu import K, XI_START, perturbed, synthetic_setup
from test_semidense_align_pyr_emu import same_maps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

# name -> (crop x0, y0, w, h), parameters, stride - w, the start's perturbation in units of XI_START, the current image's (g, o) or
# None for a black image
CASES = {
    "203x61_3_levels": ((220, 90, 203, 61), dict(levels=3, max_iters=6, min_pixels=50), 13, 1.0, (0.7, 25)),
    "97x45_3_levels_top_below_a_block": ((120, 60, 97, 45), dict(levels=3, min_pixels=20), 0, 0.6, (0.7, 25)),
    "31x29_2_levels": ((330, 150, 31, 29), dict(levels=2, min_pixels=20), 3, 0.3, (0.7, 25)),
    "203x61_unchanged": ((220, 90, 203, 61), dict(levels=3, max_iters=6, min_pixels=50), 13, 1.0, (1, 0)),
    "range_status": ((220, 90, 203, 61), dict(levels=2, max_iters=4, min_pixels=50, gain0=8.0), 5, 0.6, None),
    "top_level_status_2": ((220, 90, 203, 61), dict(levels=3, max_iters=5, min_pixels=1000, gain0=0.8, offset0=20.0), 5, 0.6, (0.7, 25)),
}


def case_inputs(fr, pyr_down, name):
    """key levels, current levels, K, T_start, level-0 map, parameters, row padding of a case"""
    (x0, y0, w, h), prm, pad, scale, go = CASES[name]
    crop = lambda a: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])
    L = prm["levels"]
    cur = np.zeros((h, w), np.uint8) if go is None else FR.map_image(crop(fr["L"][3]), *go)
    key, cur = PR.image_pyramid(crop(fr["L"][2]), L, pyr_down), PR.image_pyramid(cur, L, pyr_down)
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
                           os.path.join(ROOT, "tests", "emu", "emu_semidense_align_affine.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu") / "emu_semidense_align_affine")


def run_emu(exe, tmp_path, key, cur, Kc, T, m, pad, prm):
    """the stand-alone program's result: the final fields as align_pyr returns them, levels=[per level dict], maps=[per level dict]"""
    p = dict(FR.PYR_DEFAULTS, **prm)
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
                          [f32(p["gain0"]), f32(p["offset0"]), str(files[0]), str(files[1]), str(fmap), str(fo)])
    raw = fo.read_bytes()
    ints = np.frombuffer(raw[64:88], np.int32)
    d = np.frombuffer(raw[88:88 + 8 * 46], np.float64)
    off = 88 + 8 * 46
    lv_i = np.frombuffer(raw[off:off + 144], np.int32).reshape(6, 6)
    lv_d = np.frombuffer(raw[off + 144:off + 240], np.float64).reshape(6, 2)
    lv_T = np.frombuffer(raw[off + 240:off + 240 + 384], F).reshape(6, 4, 4)
    off += 240 + 384

    def rms(swrr, sw):
        with np.errstate(all="ignore"):
            return float(np.sqrt(swrr / sw) / np.float64(16)) if sw > 0 else 0.0
    out = dict(T_ck=np.frombuffer(raw[:64], F).reshape(4, 4), status=int(ints[0]), iters=int(ints[1]), count=int(ints[2]), start_prev=int(ints[3]),
               G=int(ints[4]), O=int(ints[5]), rms=rms(d[0], d[1]), H=d[2:38], b=d[38:46])
    out["levels"] = [dict(status=int(lv_i[l, 0]), iters=int(lv_i[l, 1]), count=int(lv_i[l, 2]), launches=int(lv_i[l, 3]), G=int(lv_i[l, 4]),
                          O=int(lv_i[l, 5]), rms=rms(*lv_d[l]), T_ck=lv_T[l]) for l in range(L)]
    wt, ht = PR.level_size(w0, h0, L - 1)
    nb = (wt * ht + AR.BLOCK - 1) // AR.BLOCK
    out["top_first_sums"] = np.frombuffer(raw[off:off + 8 * nb * FR.NSUM], np.int64).reshape(nb, FR.NSUM)
    off += 8 * nb * FR.NSUM
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


def same_result(got, want):
    """every field of an affine alignment's result, bit for bit: (ok, the first field that differs)"""
    for k in ("status", "iters", "count", "G", "O"):
        if int(got[k]) != int(want[k]):
            return False, (k, got[k], want[k])
    for k, dt, n in (("T_ck", np.uint32, 16), ("H", np.uint64, 36), ("b", np.uint64, 8)):
        a, b = np.ascontiguousarray(got[k]).reshape(-1), np.ascontiguousarray(want[k]).reshape(-1)
        if a.size != n or b.size != n or not np.array_equal(a.view(dt), b.view(dt)):
            return False, (k, a, b)
    if np.float64(got["rms"]).tobytes() != np.float64(want["rms"]).tobytes():
        return False, ("rms", got["rms"], want["rms"])
    return True, None


def same_levels(got, want, pose=True):
    """the per-level fields, bit for bit: (ok, the first that differs)"""
    if len(got) != len(want):
        return False, ("levels", len(got), len(want))
    for l, (g, w) in enumerate(zip(got, want)):
        for k in ("status", "iters", "count", "G", "O"):
            if int(g[k]) != int(w[k]):
                return False, (l, k, g[k], w[k])
        if np.float64(g["rms"]).tobytes() != np.float64(w["rms"]).tobytes():
            return False, (l, "rms", g["rms"], w["rms"])
        if pose and not np.array_equal(np.ascontiguousarray(g["T_ck"], F).view(np.uint32), np.ascontiguousarray(w["T_ck"], F).view(np.uint32)):
            return False, (l, "T_ck", g["T_ck"], w["T_ck"])
    return True, None


def test_the_cases_exercise_what_they_name(frames, pyr_down):
    for name in CASES:
        key, cur, Kc, T, m, prm, pad = case_inputs(frames, pyr_down, name)
        want = FR.align_pyr(key, cur, Kc, T, m, **prm)
        L = prm["levels"]
        sizes = [k.shape[::-1] for k in key]
        lv = want["levels"]
        print(name, sizes, [(d["status"], d["iters"], d["count"], d["G"], d["O"]) for d in lv])
        G0, O0 = FR.start_GO(prm.get("gain0", 1.0), prm.get("offset0", 0.0))
        if name == "203x61_3_levels":
            assert sizes == [(203, 61), (102, 31), (51, 16)] and pad > 0 and all(d["status"] in (0, 1) and d["iters"] > 1 for d in lv)
            assert abs(want["gain"] - 0.7) < 0.1 and abs(want["offset"] - 25) < 10 and len({(d["G"], d["O"]) for d in lv}) == 3
        if name == "97x45_3_levels_top_below_a_block":
            assert sizes == [(97, 45), (49, 23), (25, 12)] and 25 * 12 < AR.BLOCK and lv[2]["status"] in (0, 1)
        if name == "31x29_2_levels":
            assert sizes == [(31, 29), (16, 15)] and lv[1]["count"] >= 20 and want["status"] in (0, 1)
        if name == "203x61_unchanged":
            assert want["status"] in (0, 1) and abs(want["gain"] - 1) < 0.1
        if name == "range_status":  # either level: one evaluation, the state as started
            assert [(d["status"], d["iters"], d["G"], d["O"]) for d in lv] == [(FR.RANGE, 1, G0, O0)] * L and G0 == FR.G_MAX
            assert np.array_equal(want["T_ck"], T) and want["count"] >= prm["min_pixels"]
        if name == "top_level_status_2":  # the top level has too few pixels: one evaluation, T, G, O handed down, the next level runs
            assert lv[2]["status"] == 2 and lv[2]["iters"] == 1 and 0 < lv[2]["count"] < prm["min_pixels"]
            assert (lv[2]["G"], lv[2]["O"]) == (G0, O0) != FR.start_GO() and np.array_equal(lv[2]["T_ck"], T)
            assert lv[1]["status"] in (0, 1) and lv[1]["count"] >= prm["min_pixels"] and (lv[1]["G"], lv[1]["O"]) != (G0, O0)
            # ... and the levels below run from the state the top level was given: the same bits as two levels
            two = FR.align_pyr(key[:2], cur[:2], Kc, T, m, **dict(prm, levels=2))
            ok, where = same_result(want, two)
            assert ok, where


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_text_equals_restatement(emu, frames, pyr_down, tmp_path, name):
    key, cur, Kc, T, m, prm, pad = case_inputs(frames, pyr_down, name)
    want = FR.align_pyr(key, cur, Kc, T, m, **prm)
    got = run_emu(emu, tmp_path, key, cur, Kc, T, m, pad, prm)
    assert np.array_equal(got["top_first_sums"], want["top_first_sums"])  # the 47 integer sums of every block, first iteration
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
    prm = dict(prm, levels=1, gain0=0.9, offset0=-3.0)
    got = run_emu(emu, tmp_path, key[:1], cur[:1], Kc, T, m, pad, prm)
    want = FR.align(key[0], cur[0], Kc, T, m, **{k: v for k, v in prm.items() if k != "levels"})
    ok, where = same_result(got, want)
    assert ok, where
    assert np.array_equal(got["top_first_sums"], want["first_sums"]) and want["first_sums"].shape == (13, 47)


def test_sanitized_emulation_of_the_first_case(frames, pyr_down, tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined: no access, to an image level, a level of the map, a row of
    partial sums or the staged rows, leaves its exactly sized buffer."""
    exe = build_emu(tmp_path / "emu_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    key, cur, Kc, T, m, prm, pad = case_inputs(frames, pyr_down, "203x61_3_levels")
    prm = dict(prm, max_iters=2)
    got = run_emu(exe, tmp_path, key, cur, Kc, T, m, pad, prm)
    ok, where = same_result(got, FR.align_pyr(key, cur, Kc, T, m, **prm))
    assert ok, where
    ok, where = same_maps(got["maps"], PR.map_pyramid(m, prm["levels"]))
    assert ok, where

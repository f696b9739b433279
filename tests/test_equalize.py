"""CLAHE equalisation, host side (no GPU): hand-derived pins of the numpy restatement (tests/clahe_restatement.py), the new C
symbols, the C++ mirrors' setEqualize against the type-check stand-ins, the Python argument forms, the examples' --clahe options,
and what the option is for: on a low-contrast image the oracle's detect-and-bucket fills more buckets after equalisation."""
import os
import subprocess
import sys

import numpy as np
import pytest

from clahe_restatement import clahe, clip_limit_int, extension, tile_luts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "typecheck_stubs")
NEW_SYMBOLS = ("vo_set_equalize", "vo_get_equalize", "vo_equalize_image")


def test_constant_image_by_hand():
    """64 x 48 of value 77, 8 x 8 tiles, clip 40: 48-pixel tiles, limit (int)(40 * 48 / 256) = 7, 41 clipped, batch 0, residual
    41, step 6: bins 0, 6, ..., 240; 13 of them are at or below 77 (0 .. 72), plus the 7 left in bin 77: 20 * 255 / 48 = 106.25"""
    img = np.full((48, 64), 77, np.uint8)
    assert extension(64, 48, 8, 8) == (64, 48, 8, 6) and clip_limit_int(40.0, 48) == 7
    out, luts = clahe(img, 40.0, (8, 8))
    assert (out == 106).all()
    assert luts[0, 0, 76] == round(13 * 255 / 48) and luts[0, 0, 77] == 106 and luts[0, 0, 255] == 255
    # clip 0: nothing is clipped — all 48 pixels sit in bin 77, the running sum there is the tile: 255
    out0, luts0 = clahe(img, 0.0, (8, 8))
    assert (out0 == 255).all() and (luts0[:, :, :77] == 0).all() and (luts0[:, :, 77:] == 255).all()


def test_extension_rule():
    """either remainder non-zero extends BOTH dimensions: 72 divides by 8 and still grows by a full 8"""
    assert extension(72, 45, 8, 8) == (80, 48, 10, 6)
    assert extension(67, 45, 4, 3) == (68, 48, 17, 16)   # 45 divides by 3: a full 3 more rows
    assert extension(1241, 376, 8, 8) == (1248, 384, 156, 48)
    assert extension(64, 48, 8, 8) == (64, 48, 8, 6)
    assert extension(33, 17, 32, 16) == (64, 32, 2, 2)
    # the extension is REFLECT_101: a tile made of reflected columns only counts the columns it mirrors
    img = np.zeros((45, 72), np.uint8)
    img[:, 62:71] = np.arange(9, dtype=np.uint8)[None, :] + 10   # columns 62 .. 70 hold 10 .. 18, column 71 holds 0
    luts = tile_luts(img, 0.0, (8, 8))
    # tile column 7 = extended columns 70 .. 79 = columns 70, 71, 70, 69, ..., 63: values 18, 0, 18, 17, ..., 11
    want = np.bincount([18, 0, 18, 17, 16, 15, 14, 13, 12, 11], minlength=256) * 6  # th = 6 rows, all alike
    got = np.diff(np.concatenate([[0], np.rint(luts[0, 7].astype(np.float64) * 60 / 255)]))
    assert np.array_equal(got, want)


def test_clip_limit_floor_and_residual_wrap():
    assert clip_limit_int(0.5, 15) == 1          # 0.5 * 15 / 256 floors to 0, raised to 1 (40 x 24 at 8 x 8: 5 x 3 tiles)
    assert clip_limit_int(0.0, 48) is None and clip_limit_int(1e300, 48) is None
    # residual above 128: step 1, bins 0 .. residual-1 get one each
    img = np.full((32, 32), 200, np.uint8)       # one tile of 1024 pixels, clip 1 -> limit 4: 1020 clipped, batch 3, residual 252
    luts = tile_luts(img, 1.0, (1, 1))
    hist = np.full(256, 3)
    hist[200] += 4
    hist[:252] += 1
    want = np.clip(np.rint((np.cumsum(hist).astype(np.float32) * (np.float32(255) / np.float32(1024)))), 0, 255)
    assert np.array_equal(luts[0, 0], want.astype(np.uint8))


def test_new_symbols_declared_listed_and_exported(vo):
    from visual_odometry_ros_amd import _capi
    import ctypes as C
    header = open(os.path.join(ROOT, "include", "vo_hip.h")).read()
    lib = vo.load()
    for name in NEW_SYMBOLS:
        assert name in _capi.SYMBOLS and f"int {name}(" in header and hasattr(lib, name), name
    assert lib.vo_abi_version() == 3  # additions only
    assert "VO_EQ_OFF = 0, VO_EQ_CLAHE = 1" in header
    # NULL arguments: a negative status before anything is touched
    assert lib.vo_set_equalize(None, 1, C.c_double(40.0), 8, 8) < 0
    assert lib.vo_get_equalize(None, None, None, None, None) < 0
    assert lib.vo_equalize_image(None, None, 0, 0, 0, None, 0, None, 0) < 0
    assert callable(vo.Context.set_equalize) and callable(vo.Context.equalizeImage) and isinstance(vo.Context.equalize, property)


def test_setequalize_type_checks():
    src = os.path.join(ROOT, "tests", "cpp", "equalize_typecheck.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", ROOT, "-I", os.path.join(STUBS, "thirdparty"),
                        "-I", os.path.join(STUBS, "reference"), "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_from_yaml_equalize_argument():
    from visual_odometry_ros_amd.api import _equalize_arg
    assert _equalize_arg(None) is None and _equalize_arg("clahe") == {}
    assert _equalize_arg({"clip_limit": 2.0, "tiles": (4, 4)}) == {"clip_limit": 2.0, "tiles": (4, 4)}
    for bad in ("hist", {"clip": 2.0}, 3):
        with pytest.raises(ValueError):
            _equalize_arg(bad)
    import visual_odometry_ros_amd as V
    cfg = os.path.join(ROOT, "tests", "golden", "reference_config")
    with pytest.raises(ValueError):  # found before any device is touched
        V.StereoVO.from_yaml(os.path.join(cfg, "stereo", "kitti_00_stereo.yaml"), equalize="histogram")
    with pytest.raises(ValueError):
        V.MonoVO.from_yaml(os.path.join(cfg, "mono", "kitti_00.yaml"), equalize={"tile": (8, 8)})


@pytest.mark.parametrize("example,base", [("run_stereo_sequence", ["--config", "c.yaml", "--left", "l", "--right", "r"]),
                                          ("run_mono_sequence", ["--config", "c.yaml", "--images", "i"])])
def test_examples_clahe_options(example, base):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        ex = __import__(example)
    finally:
        sys.path.pop(0)
    assert ex.clahe_options(ex.parse_args(base)) == {}
    assert ex.clahe_options(ex.parse_args(base + ["--clahe"])) == {"equalize": {"clip_limit": 40.0, "tiles": (8, 8)}}
    assert ex.clahe_options(ex.parse_args(base + ["--clahe", "2.5", "--clahe-tiles", "16", "4"])) == {"equalize": {"clip_limit": 2.5, "tiles": (16, 4)}}
    for bad in (["--clahe-tiles", "8", "8"], ["--clahe", "-1"], ["--clahe", "--clahe-tiles", "0", "8"], ["--clahe", "--clahe-tiles", "8", "33"],
                ["--clahe", "nan"], ["--clahe", "inf"]):
        with pytest.raises(SystemExit):
            ex.clahe_options(ex.parse_args(base + bad))


def test_equalisation_fills_more_buckets_on_low_contrast(oracle):
    """One synthetic image compressed to low contrast around mid-grey: the oracle's detect-and-bucket (as tests/mask_ref.py drives
    it) fills strictly more buckets on the restatement-equalised image than on the compressed one."""
    from visual_odometry_ros_amd import synthetic as S
    from mask_ref import masked_table
    w, h, nbu, nbv = 320, 200, 16, 10
    st = S.StereoStream(width=w, height=h, K=(300.0, 300.0, 160.0, 100.0), n_u=10, n_v=6, n_new=10, seed=7, margin=5.0)
    img = st.render_pair(st.poses(1)[0])[0]
    low = (128 + (img.astype(np.int32) - 128) // LOW_CONTRAST_DIVISOR).astype(np.uint8)
    f = np.float32
    iu, iv = f(1.0) / f(w // nbu), f(1.0) / f(h // nbv)
    n_low = int(masked_table(low, None, iu, iv, nbu, nbv)[1].sum())
    n_eq = int(masked_table(clahe(low)[0], None, iu, iv, nbu, nbv)[1].sum())
    print(f"buckets filled: {n_low} on the compressed image, {n_eq} after equalisation, of {nbu * nbv}")
    assert n_eq > n_low


# chosen on the CPU so that the oracle shows the gap: FAST's threshold (15 grey levels) is absolute, the synthetic image's
# corners have a few tens of levels of contrast
LOW_CONTRAST_DIVISOR = 6

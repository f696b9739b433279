"""The map merge's kernel (csrc/semidense_map_merge_device.hpp) on CPU threads (tests/emu/emu_semidense_map_merge.cpp, with the product's
launch geometry: 256 lanes a workgroup, four pixels a lane, the launcher's alignment rule) against the restatement
(tests/semidense_map_merge_restatement.py): every plane to the bit, the six counts exact. The smallest shapes at which the kernel can go
wrong (1, 3, 4, 5, 1023, 1024, 1025 pixels; 97 x 21; 203 x 37), every plane one element off a 16-byte boundary on its own and all
together (the path that moves single elements), no map and a map without entries, every status 0..6 with arbitrary bits under the
statuses that are not accepted, n_obs 254 and 255, pixels exactly on the agreement boundary and one float above it, both sigmas 0,
NaN and +-Inf in each input plane in turn, keep_obs 0, 1, 2 and 256, the outputs aliased onto the map, origin and counts NULL.
Workgroups in reverse order and on 1, 3 and 8 CPUs give the same bits; once under the address and undefined-behaviour sanitizers with
exactly sized buffers. No GPU."""
import os
import subprocess

import numpy as np
import pytest

from semidense_map_merge_restatement import DEFAULTS, merge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PLANES = ("map_invd", "map_sigma", "map_n_obs", "disparity", "sigma_invd", "status", "invd", "sigma", "n_obs", "origin")


def _random(w, h, seed, with_map=True, **prm):
    """every status 0..6, accepted with probability 0.6, arbitrary bits (NaN payloads, denormals, infinities among them) in disparity
    and sigma_invd under every other status; a map with entries on 60 % of the pixels whose inverse depth lies within a few sigma of the
    result's on most of them and far off on the rest, n_obs from 1, 2, 3, 254, 255; bf = 38.6"""
    rng = np.random.default_rng(seed)
    bf = 38.6
    st = np.where(rng.random((h, w)) < 0.6, 1, rng.choice([0, 2, 3, 4, 5, 6], (h, w))).astype(np.uint8)
    d = (1.0 + 60.0 * rng.random((h, w))).astype(F)
    sg = (0.002 + 0.01 * rng.random((h, w))).astype(F)
    junk = rng.integers(0, 2 ** 32, (2, h, w), dtype=np.uint64).astype(np.uint32)
    d.view(np.uint32)[st != 1] = junk[0][st != 1]
    sg.view(np.uint32)[st != 1] = junk[1][st != 1]
    m = None
    if with_map:
        has = rng.random((h, w)) < 0.6
        truth = (1.0 + 60.0 * rng.random((h, w))) / bf
        with np.errstate(all="ignore"):
            near = np.where((st == 1) & np.isfinite(d), d.astype(np.float64) / bf, truth)
        ms = (0.001 + 0.01 * rng.random((h, w))).astype(F)
        far = rng.random((h, w)) < 0.25
        mi = (near + np.where(far, 0.5, 1.0) * rng.normal(size=(h, w)) * np.where(far, 1.0, 2.5 * ms)).astype(F)
        mn = rng.choice([1, 2, 3, 254, 255], (h, w)).astype(np.uint8)
        m = dict(invd=np.where(has, mi, F(0)).astype(F), sigma=np.where(has, ms, F(0)).astype(F), n_obs=np.where(has, mn, 0).astype(np.uint8))
    return m, d, sg, st, bf, prm


def _empty_map():
    m, d, sg, st, bf, prm = _random(97, 21, 20)
    m["n_obs"][:] = 0  # (invd and sigma keep their values: without an entry they must not be read into anything)
    return m, d, sg, st, bf, prm


def boundary_values():
    """a pixel exactly on the agreement boundary with chi = 3, in float32: sigma = 3/32, sig_d = 4/32, so s2 + m2 = 25/1024 and
    chi2 (s2 + m2) = 225/1024 = (15/32)^2; rho_d = 1 (disparity 2, bf 2), invd = 1 + 15/32. Every number is exact in float32."""
    return dict(sigma=F(3 / 32), sig_d=F(4 / 32), disparity=F(2), bf=2.0, invd=F(1 + 15 / 32))


def _boundary():
    b = boundary_values()
    w, h = 8, 1
    d, sg, st = np.full((h, w), b["disparity"], F), np.full((h, w), b["sig_d"], F), np.ones((h, w), np.uint8)
    mi, ms = np.full((h, w), b["invd"], F), np.full((h, w), b["sigma"], F)
    mn = np.array([[1, 1, 1, 1, 2, 2, 254, 255]], np.uint8)
    up, dn = np.nextafter(b["invd"], F(np.inf)), np.nextafter(F(1 - 15 / 32), F(-np.inf))
    mi[0, 1] = up  # one float above the boundary: disagree, n_obs 1 < keep_obs: dropped
    mi[0, 2] = F(1 - 15 / 32)  # the boundary from below: agree
    mi[0, 3] = dn  # one float beyond it
    mi[0, 5] = up  # disagree, n_obs 2 >= keep_obs: the map kept
    return dict(invd=mi, sigma=ms, n_obs=mn), d, sg, st, b["bf"], {}


def _sum_zero():
    """both sigmas 0 on pixels that have both entries: the test fails whatever the difference, equal values included"""
    m, d, sg, st, bf, prm = _random(5, 1, 21)
    st[:] = 1
    d[:] = F(19.3)
    sg[:] = F(0)
    m["invd"][:] = (d / F(bf)).astype(F)
    m["sigma"][:] = F(0)
    m["n_obs"][:] = np.array([[1, 2, 3, 255, 0]], np.uint8)
    return m, d, sg, st, bf, prm


def _special(plane, value):
    """`value` in one input plane on pixels that carry both entries (n_obs 1, 2, 255), one entry, or none"""
    m, d, sg, st, bf, prm = _random(12, 1, 22)
    st[0, :9], st[0, 9:] = 1, 0
    d[0, :9], sg[0, :9] = F(19.3), F(0.004)
    m["invd"][:], m["sigma"][:] = (F(19.3) / F(bf)), F(0.003)
    m["n_obs"][:] = np.array([[1, 2, 255, 1, 2, 255, 0, 0, 0, 1, 0, 0]], np.uint8)
    tgt = dict(map_invd=m["invd"], map_sigma=m["sigma"], disparity=d, sigma_invd=sg)[plane]
    tgt[0, [0, 1, 2, 6, 9, 10]] = F(value)
    return m, d, sg, st, bf, prm


CASES = {"%dx%d" % (w, h): (lambda w=w, h=h, k=k: _random(w, h, k))
         for k, (w, h) in enumerate([(1, 1), (3, 1), (4, 1), (5, 1), (1023, 1), (1024, 1), (1025, 1), (97, 21), (203, 37)])}
CASES.update({
    "no_map_97x21": lambda: _random(97, 21, 30, with_map=False), "no_map_5x1": lambda: _random(5, 1, 31, with_map=False),
    "map_without_entries": _empty_map, "boundary": _boundary, "sum_zero": _sum_zero,
    "keep_obs_0": lambda: _random(97, 21, 32, keep_obs=0), "keep_obs_1": lambda: _random(97, 21, 32, keep_obs=1),
    "keep_obs_256": lambda: _random(97, 21, 32, keep_obs=256), "chi_1": lambda: _random(203, 37, 33, chi=1.0),
})
for _p in ("map_invd", "map_sigma", "disparity", "sigma_invd"):
    for _n, _v in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
        CASES["%s_%s" % (_p, _n)] = (lambda p=_p, v=_v: _special(p, v))

_MADE = {}


def case(name):
    """(map or None, disparity, sigma_invd, status, bf, parameters, the restatement's result) of a case: made once, shared
    (tests/test_semidense_map_merge_gpu.py too), never changed"""
    if name not in _MADE:
        m, d, sg, st, bf, prm = CASES[name]()
        d, sg, st = np.ascontiguousarray(d, F), np.ascontiguousarray(sg, F), np.ascontiguousarray(st, np.uint8)
        if m is not None:
            m = dict(invd=np.ascontiguousarray(m["invd"], F), sigma=np.ascontiguousarray(m["sigma"], F), n_obs=np.ascontiguousarray(m["n_obs"], np.uint8))
        want = merge(m, d, sg, st, bf, **prm)
        for v in (d, sg, st) + tuple(want.values()) + (() if m is None else tuple(m.values())):
            v.setflags(write=False)
        _MADE[name] = (m, d, sg, st, bf, prm, want)
    return _MADE[name]


def same_result(got, want, computed_nan_any_bits=False):
    """None where invd, sigma, n_obs and origin are the same bits and the counts equal, else where they differ. Planes that `got` holds
    as None are not compared. computed_nan_any_bits: on pixels of origin 2 and 3 — whose values come out of arithmetic — two NaNs are
    equal whatever their sign and payload (which NaN an operation produces is the processor's choice, not IEEE 754's; origins 1 and 4
    copy bits and are compared as bits)."""
    for k in ("origin", "n_obs", "invd", "sigma"):
        if got.get(k) is None:
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype:
            return (k, a.shape, a.dtype, b.shape, b.dtype)
        ab, bb = (a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else (a, b)
        diff = ab != bb
        if computed_nan_any_bits and a.dtype == np.float32:
            diff &= ~(np.isnan(a) & np.isnan(b) & ((want["origin"] == 2) | (want["origin"] == 3)))
        if diff.any():
            ys, xs = np.nonzero(diff)
            return (k, len(ys), int(ys[0]), int(xs[0]), got[k][ys[0], xs[0]], want[k][ys[0], xs[0]])
    if got.get("counts") is not None and not np.array_equal(np.asarray(got["counts"], np.uint64), want["counts"]):
        return ("counts", list(got["counts"]), list(want["counts"]))
    return None


def test_the_cases_are_what_they_claim():
    b = boundary_values()
    dd = b["invd"] - b["disparity"] / F(b["bf"])
    tot = b["sigma"] * b["sigma"] + b["sig_d"] * b["sig_d"]
    assert dd * dd == F(3) * F(3) * tot and type(dd * dd) is np.float32  # an equality in float32, not a near miss
    up = np.nextafter(b["invd"], F(np.inf)) - F(1)
    assert up * up > F(9) * tot
    want = case("boundary")[6]
    assert want["origin"].tolist() == [[3, 5, 3, 5, 3, 4, 3, 3]] and want["n_obs"].tolist() == [[2, 0, 2, 0, 3, 2, 255, 255]]
    assert case("sum_zero")[6]["origin"].tolist() == [[5, 4, 4, 4, 2]]
    m, d, sg, st, bf, prm, want = case("203x37")
    assert set(np.unique(st).tolist()) == set(range(7)) and set(np.unique(want["origin"]).tolist()) == set(range(6))
    assert int(want["counts"].sum()) == st.size and (want["n_obs"][(want["origin"] == 3) & (m["n_obs"] >= 254)] == 255).all()
    assert not np.isfinite(d[st != 1]).all()  # the bits under the other statuses are arbitrary ...
    keep = (want["origin"] == 1) | (want["origin"] == 4)  # ... and never reach an output: these carry the map's bits
    assert np.array_equal(want["invd"].view(np.uint32)[keep], m["invd"].view(np.uint32)[keep]) and (want["origin"][st != 1] <= 1).all()
    assert case("no_map_97x21")[0] is None and set(np.unique(case("no_map_97x21")[6]["origin"]).tolist()) == {0, 2}
    assert set(np.unique(case("map_without_entries")[6]["origin"]).tolist()) == {0, 2}
    k0, k1, k2, k256 = (case(n)[6]["counts"] for n in ("keep_obs_0", "keep_obs_1", "97x21", "keep_obs_256"))
    assert k0[5] == 0 and k256[4] == 0 and k1[5] == 0 and k1[4] == k0[4] and k256[5] == k0[4]  # (every entry has n_obs >= 1)
    for p in ("map_invd", "map_sigma", "disparity", "sigma_invd"):
        assert (case(p + "_nan")[6]["origin"][0, :3] != 3).all(), p  # a NaN anywhere fails the test
        assert (case("97x21")[6]["origin"] == 3).any()


def build_emu(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", *flags,
                           os.path.join(ROOT, "tests", "emu", "emu_semidense_map_merge.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu") / "emu_semidense_map_merge")


@pytest.fixture(scope="module")
def emu_san(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu_san") / "emu_semidense_map_merge_san", "-g", "-fsanitize=address,undefined",
                     "-fno-sanitize-recover=all")


def _hex(x):
    return "%08x" % int(np.float32(x).view(np.uint32))


def run_emu(exe, tmp_path, m, d, sg, st, bf, prm, reverse=0, cpus=0, origin=True, counts=True, alias=False, offsets=()):
    """-> the result as the restatement returns it (origin / counts None where not asked for) and `wide`: the 16-byte path ran"""
    p = dict(DEFAULTS, **prm)
    h, w = st.shape
    n = w * h
    fi, fo = tmp_path / "in.raw", tmp_path / "out.raw"
    fi.write_bytes((b"" if m is None else m["invd"].tobytes() + m["sigma"].tobytes() + m["n_obs"].tobytes()) + d.tobytes() + sg.tobytes() + st.tobytes())
    mask = sum(1 << PLANES.index(k) for k in offsets)
    subprocess.check_call([exe, str(reverse), str(cpus), str(w), str(h), _hex(p["chi"]), str(p["keep_obs"]), _hex(bf), "0" if m is None else "1",
                           str(int(origin)), str(int(counts)), str(int(alias)), str(mask), str(fi), str(fo)])
    raw = fo.read_bytes()
    assert len(raw) == 9 * n + (n if origin else 0) + (48 if counts else 0) + 1
    o = 9 * n + (n if origin else 0)
    return dict(invd=np.frombuffer(raw[:4 * n], F).reshape(h, w), sigma=np.frombuffer(raw[4 * n:8 * n], F).reshape(h, w),
                n_obs=np.frombuffer(raw[8 * n:9 * n], np.uint8).reshape(h, w),
                origin=np.frombuffer(raw[9 * n:10 * n], np.uint8).reshape(h, w) if origin else None,
                counts=np.frombuffer(raw[o:o + 48], np.uint64) if counts else None), bool(raw[-1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_text_equals_restatement(emu, tmp_path, name):
    m, d, sg, st, bf, prm, want = case(name)
    got, wide = run_emu(emu, tmp_path, m, d, sg, st, bf, prm)
    assert wide and same_result(got, want) is None


@pytest.mark.parametrize("offsets", [(k,) for k in PLANES] + [PLANES])
def test_a_plane_off_the_16_byte_boundary_takes_the_scalar_path_with_the_same_bits(emu, tmp_path, offsets):
    for name in ("203x37", "1025x1"):
        m, d, sg, st, bf, prm, want = case(name)
        got, wide = run_emu(emu, tmp_path, m, d, sg, st, bf, prm, offsets=offsets)
        assert not wide and same_result(got, want) is None, name


@pytest.mark.parametrize("name,offsets", [("203x37", ()), ("1025x1", ()), ("5x1", ()), ("boundary", ()), ("97x21", ("map_invd", "invd"))])
def test_outputs_aliased_onto_the_map(emu, tmp_path, name, offsets):
    m, d, sg, st, bf, prm, want = case(name)
    got, wide = run_emu(emu, tmp_path, m, d, sg, st, bf, prm, alias=True, offsets=tuple(k for k in offsets if k.startswith("map_")))
    assert wide == (not offsets) and same_result(got, want) is None


@pytest.mark.parametrize("origin,counts", [(False, True), (True, False), (False, False)])
def test_origin_and_counts_may_be_null(emu, tmp_path, origin, counts):
    for name in ("203x37", "no_map_5x1"):
        m, d, sg, st, bf, prm, want = case(name)
        got, _ = run_emu(emu, tmp_path, m, d, sg, st, bf, prm, origin=origin, counts=counts)
        assert same_result(got, want) is None, name


@pytest.mark.parametrize("name,reverse,cpus", [("203x37", 1, 0), ("1025x1", 1, 0), ("203x37", 0, 1), ("97x21", 0, 3), ("203x37", 1, 8),
                                               ("no_map_97x21", 1, 3)])
def test_workgroup_order_and_cpu_count_do_not_enter(emu, tmp_path, name, reverse, cpus):
    m, d, sg, st, bf, prm, want = case(name)
    assert same_result(run_emu(emu, tmp_path, m, d, sg, st, bf, prm, reverse=reverse, cpus=cpus)[0], want) is None


@pytest.mark.parametrize("name,kw", [("203x37", {}), ("1025x1", {}), ("1023x1", dict(offsets=PLANES)), ("5x1", dict(alias=True)), ("1x1", {}),
                                     ("no_map_97x21", dict(origin=False, counts=False)), ("97x21", dict(offsets=("status",)))])
def test_kernel_text_under_the_sanitizers(emu_san, tmp_path, name, kw):
    """exactly sized buffers: an access behind one, a misaligned wide access or other undefined behaviour ends the program with an error"""
    m, d, sg, st, bf, prm, want = case(name)
    assert same_result(run_emu(emu_san, tmp_path, m, d, sg, st, bf, prm, **kw)[0], want) is None

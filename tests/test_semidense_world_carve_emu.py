"""The carve kernel of the world map (csrc/semidense_world_carve_device.hpp), in both forms, next to the integration and the removal
on CPU threads (tests/emu/emu_semidense_world_carve.cpp, with the product's launch geometry) against the numpy restatement
(tests/semidense_world_carve_restatement.py): the operations of tests/test_semidense_world_carve.py on every case of it; after the
canonical sort by key `free` of every claimed slot, vacated ones included, every counter of the carve, and every other field of every
slot and every other counter equal to the bit. The first case once more with the workgroups walked from the last to the first and with
the process confined to 1, 3 and 8 CPUs: the bytes written are the same. Once more through the same stand-alone program built with the
address and undefined-behaviour sanitizers: every buffer there has exactly the bytes it holds. No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import semidense_world_carve_restatement as CR
import semidense_world_reanchor_restatement as RR
import semidense_world_restatement as WR
from test_semidense_world import same_records
from test_semidense_world_carve import CARVE_CASES, TABLE, carve_ops, restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
STATE = ("occupied", "claimed", "ticket", "integrations", "refused", "n_extract")
RSTATE = ("r_ticket", "removals", "refused_removals", "vacant")
OPS = {"integrate": 0, "remove": 1, "carve": 3, "clear": 4}
FORMS = {"aggregated": 0, "simple": 1}


def build_emu(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", *flags,
                           os.path.join(ROOT, "tests", "emu", "emu_semidense_world_carve.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu") / "emu_semidense_world_carve")


def ops_bytes(ops):
    out = []
    for op, s, prm in ops:
        if op == "clear":
            out.append(struct.pack("<5i", OPS[op], 0, 0, 0, 0))
            continue
        h, w = s["map"]["invd"].shape
        stride = w + s["pad"]
        has_key = int(s["Lk"] is not None and op != "carve")
        c = dict(CR.CARVE_DEFAULTS, **(prm or {}))
        out.append(struct.pack("<5i", OPS[op], w, h, stride, has_key))
        out.append(np.asarray(s["K"], F).tobytes() + np.ascontiguousarray(s["T"], F).tobytes() + np.asarray([c["margin"], c["chi"], c["z_near"]], F).tobytes())
        out += [np.ascontiguousarray(s["map"][k]).tobytes() for k in ("invd", "sigma", "n_obs")]
        if has_key:
            buf = np.full((h, stride), 0xEE, np.uint8)
            buf[:, :w] = s["Lk"]
            out.append(buf.tobytes()[:stride * (h - 1) + w])
    return b"".join(out)


def run_emu(exe, tmp_path, name, ops, form=0, reverse=0, cpus=0):
    p = CARVE_CASES[name]
    fi, fo = tmp_path / "ops.raw", tmp_path / f"out_{form}_{reverse}_{cpus}.raw"
    if not fi.exists():
        fi.write_bytes(ops_bytes(ops))
    f32 = lambda v: repr(float(F(v)))
    subprocess.check_call([exe, str(reverse), str(cpus), str(form), f32(p["voxel"]), str(p["capacity_log2"]), str(p["min_obs"]), f32(p["z_max"]),
                           str(fi), str(fo)])
    return fo.read_bytes()


def parse(raw):
    st = dict(zip(STATE, struct.unpack_from("<6I", raw, 0)))
    st.update(zip(("inserted", "skipped", "out_of_range"), struct.unpack_from("<3Q", raw, 24)))
    rs = dict(zip(RSTATE, struct.unpack_from("<4I", raw, 48)))
    rs.update(zip(("removed", "missing"), struct.unpack_from("<2Q", raw, 64)))
    cs = dict(zip(CR.CCOUNTERS, struct.unpack_from("<5Q", raw, 80)))
    n, = struct.unpack_from("<Q", raw, 120)
    assert len(raw) == 128 + 64 * n
    q = np.frombuffer(raw, np.uint64, 8 * n, 128).reshape(n, 8)
    u = np.frombuffer(raw, np.uint32, 16 * n, 128).reshape(n, 16)
    return st, rs, cs, dict(key=q[:, 0].copy(), sums=q[:, 1:6].copy(), count=u[:, 12].copy(), keyframes=u[:, 13].copy(), last_seq=u[:, 14].copy(),
                            free=u[:, 15].copy())


def check(raw, w):
    st, rs, cs, got = parse(raw)
    ok, where = same_records(got, w.table(), fields=TABLE)
    assert ok, where
    assert cs == w.cstats, (cs, w.cstats)
    assert {k: st[k] for k in WR.COUNTERS if k != "capacity"} == {k: v for k, v in w.stats.items() if k != "capacity"}
    assert {k: rs[k] for k in RR.RCOUNTERS if k != "reanchors"} == {k: v for k, v in w.rstats.items() if k != "reanchors"}
    assert st["claimed"] == 0 and st["ticket"] == 0 and rs["r_ticket"] == 0 and st["n_extract"] == st["occupied"]
    assert got["last_seq"].max(initial=0) <= w.seq
    return cs, got


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", sorted(CARVE_CASES))
def test_kernel_text_equals_restatement(emu, tmp_path, name, form):
    cs, got = check(run_emu(emu, tmp_path, name, carve_ops(name), FORMS[form]), restated(name))
    print(name, form, cs, "slots with free", int((got["free"] > 0).sum()))


def test_arrival_order_changes_no_byte(emu, tmp_path):
    """the first case with the workgroups in reverse order and on 1, 3 and 8 CPUs, either form: the output's bytes are those of the
    forward run. Case (a) has no hit (a static scene), so the phantom case goes the same way: its free words are busy."""
    for name in ("a_203x61", "j_phantom"):
        d = tmp_path / name
        d.mkdir()
        ref = run_emu(emu, d, name, carve_ops(name))
        check(ref, restated(name))
        for form, reverse, cpus in ((0, 1, 0), (1, 0, 1), (0, 1, 3), (1, 0, 8), (0, 1, 1), (1, 1, 0))[:6 if name == "a_203x61" else 3]:
            assert run_emu(emu, d, name, carve_ops(name), form, reverse, cpus) == ref, (name, form, reverse, cpus)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_sanitized_emulation_of_the_first_case(tmp_path, form):
    """The same stand-alone program with -fsanitize=address,undefined: no access, of a map plane, the table, the carve's words or the
    extraction's records, leaves its exactly sized buffer."""
    exe = build_emu(tmp_path / "emu_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    check(run_emu(exe, tmp_path, "a_203x61", carve_ops("a_203x61"), FORMS[form]), restated("a_203x61"))

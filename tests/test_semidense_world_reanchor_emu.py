"""The removal kernel of the world map (csrc/semidense_world_device.hpp), the integration it undoes and the vacant count on CPU threads
(tests/emu/emu_semidense_world_reanchor.cpp, with the product's launch geometry) against the numpy restatement
(tests/semidense_world_reanchor_restatement.py): the operations of tests/test_semidense_world_reanchor.py — every step of a case
integrated, removals, re-anchors, a re-anchor with equal poses — on the cases (a) two maps, (c) many points per voxel, (d) negative
indices, voxel faces and the q clamp, (h) wq saturated and 1; after the canonical sort by key every accumulator of every claimed slot,
vacated ones included, and every counter equal to the bit. Case (a) once more with the workgroups walked from the last to the first
and with the process confined to 1, 3 and 8 CPUs: the bytes written are the same. Once more through the same program built with the
address and undefined-behaviour sanitizers: every buffer there has exactly the bytes it holds. The empty table and the refusals. No
GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import semidense_world_reanchor_restatement as RR
import semidense_world_restatement as WR
from test_semidense_world import CASES, case_steps, same_records
from test_semidense_world_reanchor import OP_CASES, apply_ops, filled_past_the_bound, moved_pose, reanchor_ops, restated_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
STATE = ("occupied", "claimed", "ticket", "integrations", "refused", "n_extract")
RSTATE = ("r_ticket", "removals", "refused_removals", "vacant")
OPS = {"integrate": 0, "remove": 1, "reanchor": 2}
TABLE = ("key", "sums", "count", "keyframes")


def build_emu(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", *flags,
                           os.path.join(ROOT, "tests", "emu", "emu_semidense_world_reanchor.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu") / "emu_semidense_world_reanchor")


def ops_bytes(ops):
    out = []
    for op, s, T, T2 in ops:
        h, w = s["map"]["invd"].shape
        stride = w + s["pad"]
        out.append(struct.pack("<5i", OPS[op], w, h, stride, int(s["Lk"] is not None)))
        out.append(np.asarray(s["K"], F).tobytes() + np.ascontiguousarray(T, F).tobytes() + np.ascontiguousarray(T if T2 is None else T2, F).tobytes())
        out += [np.ascontiguousarray(s["map"][k]).tobytes() for k in ("invd", "sigma", "n_obs")]
        if s["Lk"] is not None:
            buf = np.full((h, stride), 0xEE, np.uint8)
            buf[:, :w] = s["Lk"]
            out.append(buf.tobytes()[:stride * (h - 1) + w])
    return b"".join(out)


def run_emu(exe, tmp_path, name, ops, reverse=0, cpus=0, tag=""):
    p = CASES[name]
    fi, fo = tmp_path / f"ops{tag}.raw", tmp_path / f"out{tag}_{reverse}_{cpus}.raw"
    fi.write_bytes(ops_bytes(ops))
    f32 = lambda v: repr(float(F(v)))
    subprocess.check_call([exe, str(reverse), str(cpus), f32(p["voxel"]), str(p["capacity_log2"]), str(p["min_obs"]), f32(p["z_max"]), str(fi), str(fo)])
    return fo.read_bytes()


def parse(raw):
    st = dict(zip(STATE, struct.unpack_from("<6I", raw, 0)))
    st.update(zip(("inserted", "skipped", "out_of_range"), struct.unpack_from("<3Q", raw, 24)))
    rs = dict(zip(RSTATE, struct.unpack_from("<4I", raw, 48)))
    rs.update(zip(("removed", "missing", "reanchors"), struct.unpack_from("<3Q", raw, 64)))
    n, = struct.unpack_from("<Q", raw, 88)
    assert len(raw) == 96 + 64 * n
    q = np.frombuffer(raw, np.uint64, 8 * n, 96).reshape(n, 8)
    u = np.frombuffer(raw, np.uint32, 16 * n, 96).reshape(n, 16)
    return st, rs, dict(key=q[:, 0].copy(), sums=q[:, 1:6].copy(), count=u[:, 12].copy(), keyframes=u[:, 13].copy(), last_seq=u[:, 14].copy())


def check(raw, w):
    st, rs, got = parse(raw)
    ok, where = same_records(got, w.table(), fields=TABLE)
    assert ok, where
    assert {k: st[k] for k in WR.COUNTERS if k != "capacity"} == {k: v for k, v in w.stats.items() if k != "capacity"}
    assert {k: rs[k] for k in RR.RCOUNTERS} == w.rstats
    assert st["claimed"] == 0 and st["ticket"] == 0 and rs["r_ticket"] == 0 and st["n_extract"] == st["occupied"]
    assert got["last_seq"].max(initial=0) <= w.seq
    return st, rs, got


@pytest.mark.parametrize("name", OP_CASES)
def test_kernel_text_equals_restatement(emu, tmp_path, name):
    st, rs, got = check(run_emu(emu, tmp_path, name, reanchor_ops(name)), restated_ops(name))
    assert rs["missing"] == 0 and rs["vacant"] == int((got["count"] == 0).sum()) >= 1


def test_arrival_order_changes_no_byte(emu, tmp_path):
    """case (a) with the workgroups in reverse order and on 1, 3 and 8 CPUs: the output's bytes are those of the forward run (last_seq
    and every sum included)"""
    name = "a_203x61"
    ops = reanchor_ops(name)
    ref = run_emu(emu, tmp_path, name, ops)
    check(ref, restated_ops(name))
    for reverse, cpus in ((1, 0), (0, 1), (1, 3), (0, 8), (1, 1)):
        assert run_emu(emu, tmp_path, name, ops, reverse, cpus) == ref, (reverse, cpus)


def test_sanitized_emulation_of_the_first_case(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined: no access, of a map plane, the key plane, the table, the
    removal's words or the extraction's records, leaves its exactly sized buffer."""
    exe = build_emu(tmp_path / "emu_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    check(run_emu(exe, tmp_path, "a_203x61", reanchor_ops("a_203x61")), restated_ops("a_203x61"))


def test_removal_from_an_empty_table(emu, tmp_path):
    name = "a_203x61"
    A = case_steps(name)[0]
    ops = [("remove", A, A["T"], None)]
    w = apply_ops(RR.World(**CASES[name]), ops)
    st, rs, got = check(run_emu(emu, tmp_path, name, ops), w)
    assert rs["missing"] == w.rstats["missing"] >= 1000 and rs["removed"] == 0 and len(got["key"]) == 0 and st["occupied"] == 0


def test_refused_removal_and_reanchor_touch_nothing(emu, tmp_path):
    """2^12 slots filled past the bound: the table's bytes are those of the run without the refused call; refused_removals is 1"""
    name = "b_cap12_strips"
    ops, s = filled_past_the_bound()
    base = run_emu(emu, tmp_path, name, ops, tag="base")
    st0, rs0, _ = check(base, apply_ops(RR.World(**CASES[name]), ops))
    assert st0["refused"] >= 1
    for tag, extra in (("rem", ("remove", s, s["T"], None)), ("rea", ("reanchor", s, s["T"], moved_pose(s["T"])))):
        raw = run_emu(emu, tmp_path, name, ops + [extra], tag=tag)
        st, rs, _ = check(raw, apply_ops(RR.World(**CASES[name]), ops + [extra]))
        assert raw[96:] == base[96:]  # every slot, last_seq included
        assert rs["refused_removals"] == 1 and rs["removals"] == 0 and st["refused"] == st0["refused"] + (tag == "rea")
        assert {k: v for k, v in st.items() if k != "refused"} == {k: v for k, v in st0.items() if k != "refused"}

"""The world map's kernels (csrc/semidense_world_device.hpp) on CPU threads (tests/emu/emu_semidense_world.cpp, with the product's
launch geometry: ceil(W H / 1024) workgroups of 256 threads per integration, then the extraction kernel over every slot) against the
numpy restatement (tests/semidense_world_restatement.py) on every case of tests/test_semidense_world.py: after the canonical sort by
key every accumulator of every voxel and every counter equal to the bit, for the pre-aggregated kernel form and for the simple one.
The first case once more with the workgroups walked from the last to the first and with the process confined to 1, 3 and 8 CPUs (its
256 threads then arrive in other orders): the bytes written are the same. And once more through the same program built with the
address and undefined-behaviour sanitizers: every buffer there has exactly the bytes it holds. No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import semidense_world_restatement as WR
from test_semidense_world import CASES, case_steps, restated, same_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
STATE = ("occupied", "claimed", "ticket", "integrations", "refused", "n_extract")


def build_emu(out, *flags):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-ffp-contract=off", *flags,
                           os.path.join(ROOT, "tests", "emu", "emu_semidense_world.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("emu") / "emu_semidense_world")


def steps_bytes(steps):
    out = []
    for s in steps:
        h, w = s["map"]["invd"].shape
        stride = w + s["pad"]
        out.append(struct.pack("<4i", w, h, stride, int(s["Lk"] is not None)))
        out.append(np.asarray(s["K"], F).tobytes() + np.ascontiguousarray(s["T"], F).tobytes())
        out += [np.ascontiguousarray(s["map"][k]).tobytes() for k in ("invd", "sigma", "n_obs")]
        if s["Lk"] is not None:
            buf = np.full((h, stride), 0xEE, np.uint8)
            buf[:, :w] = s["Lk"]
            out.append(buf.tobytes()[:stride * (h - 1) + w])
    return b"".join(out)


def run_emu(exe, tmp_path, name, form=0, reverse=0, cpus=0):
    p = CASES[name]
    fi, fo = tmp_path / "steps.raw", tmp_path / f"out_{form}_{reverse}_{cpus}.raw"
    fi.write_bytes(steps_bytes(case_steps(name)))
    f32 = lambda v: repr(float(F(v)))
    subprocess.check_call([exe, str(form), str(reverse), str(cpus), f32(p["voxel"]), str(p["capacity_log2"]), str(p["min_obs"]), f32(p["z_max"]),
                           str(fi), str(fo)])
    return fo.read_bytes()


def parse(raw):
    st = dict(zip(STATE, struct.unpack_from("<6I", raw, 0)))
    st.update(zip(("inserted", "skipped", "out_of_range"), struct.unpack_from("<3Q", raw, 24)))
    n, = struct.unpack_from("<Q", raw, 48)
    assert len(raw) == 56 + 64 * n
    q = np.frombuffer(raw, np.uint64, 8 * n, 56).reshape(n, 8)
    u = np.frombuffer(raw, np.uint32, 16 * n, 56).reshape(n, 16)
    return st, dict(key=q[:, 0].copy(), sums=q[:, 1:6].copy(), count=u[:, 12].copy(), keyframes=u[:, 13].copy(), last_seq=u[:, 14].copy())


def check(raw, name):
    w, want, _ = restated(name)
    st, got = parse(raw)
    ok, where = same_records(got, want, fields=("key", "sums", "count", "keyframes"))
    assert ok, where
    assert {k: st[k] for k in WR.COUNTERS if k != "capacity"} == {k: v for k, v in w.stats.items() if k != "capacity"}
    assert st["claimed"] == 0 and st["ticket"] == 0 and st["n_extract"] == st["occupied"]
    assert got["last_seq"].max(initial=0) <= w.seq


@pytest.mark.parametrize("form", [0, 1], ids=["aggregated", "simple"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_text_equals_restatement(emu, tmp_path, name, form):
    check(run_emu(emu, tmp_path, name, form), name)


def test_arrival_order_changes_no_byte(emu, tmp_path):
    """the first case with the workgroups in reverse order and on 1, 3 and 8 CPUs, both kernel forms: the sorted table's bytes are
    those of the forward run (last_seq and every sum included)"""
    name = "a_203x61"
    ref = run_emu(emu, tmp_path, name)
    check(ref, name)
    for form, reverse, cpus in ((0, 1, 0), (1, 1, 0), (0, 0, 1), (0, 1, 3), (1, 0, 8), (1, 1, 1)):
        assert run_emu(emu, tmp_path, name, form, reverse, cpus) == ref, (form, reverse, cpus)


def test_sanitized_emulation_of_the_first_case(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined: no access, of a map plane, the key plane, the table or the
    extraction's records, leaves its exactly sized buffer."""
    exe = build_emu(tmp_path / "emu_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for form in (0, 1):
        check(run_emu(exe, tmp_path, "a_203x61", form), "a_203x61")

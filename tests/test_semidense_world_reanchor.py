"""Removal and re-anchoring on the world-frame voxel map by the numpy restatement alone
(tests/semidense_world_reanchor_restatement.py; include/vo_hip.h, "Semi-dense world map: removal and re-anchoring"):
a removal leaves every live voxel with the bits of a table that never saw the removed map, a re-anchor those of a table fed the map
with the new pose in the first place, the vacated voxels keep their keys, nothing is missing; a plain Python loop over the points
equals the vectorised form; the empty table and the refusals. `reanchor_ops` is the sequence of operations every other test of the
block (the CPU emulation of the kernels, the device) runs a case of tests/test_semidense_world.py through. No GPU."""
import functools

import numpy as np
import pytest

import semidense_world_reanchor_restatement as RR
from test_semidense_world import CASES, case_steps, same_records

F = np.float32
OP_CASES = ("a_203x61", "c_97x45_plane", "d_rotated_negative", "h_saturation")


def moved_pose(T, k=1):
    """T followed by a small motion, as a bundle adjustment would apply: a rotation of 2k mrad about y and a few centimetres"""
    a = 0.002 * k
    D = np.eye(4)
    D[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    D[:3, 3] = (0.013 * k, -0.021 * k, 0.034 * k)
    return (D @ np.asarray(T, np.float64).reshape(4, 4)).astype(F)


def reanchor_ops(name):
    """the operations of a case: tuples (op, step, T, T2) with op 'integrate' | 'remove' | 'reanchor'. Every step of the case goes in,
    the first comes out again, the last moves, the first goes in once more (into the voxels it vacated, where they were not taken
    since) and moves too; a re-anchor with equal poses in between is nothing."""
    steps = case_steps(name)
    first, last = steps[0], steps[-1]
    ops = [("integrate", s, s["T"], None) for s in steps]
    ops.append(("remove", first, first["T"], None))
    ops.append(("reanchor", last, last["T"], last["T"].copy()))
    if last is not first:
        ops.append(("reanchor", last, last["T"], moved_pose(last["T"])))
    ops.append(("integrate", first, first["T"], None))
    ops.append(("reanchor", first, first["T"], moved_pose(first["T"], 2)))
    return ops


def apply_ops(w, ops, loop=False):
    for op, s, T, T2 in ops:
        if op == "integrate":
            (w.integrate_loop if loop else w.integrate)(s["map"], s["K"], T, s["Lk"])
        elif op == "remove":
            (w.remove_loop if loop else w.remove)(s["map"], s["K"], T, s["Lk"])
        else:
            w.reanchor(s["map"], s["K"], T, T2, s["Lk"], loop=loop)
    return w


@functools.lru_cache(maxsize=None)
def restated_ops(name):
    """the restated table after reanchor_ops(name) — computed once for every test of any module; not to be modified"""
    return apply_ops(RR.World(**CASES[name]), reanchor_ops(name))


def _fed(name, seq):
    w = RR.World(**CASES[name])
    for s, T in seq:
        assert w.integrate(s["map"], s["K"], T, s["Lk"])
    return w


def test_removal_leaves_the_table_fed_the_rest():
    name = "a_203x61"
    A, B = case_steps(name)
    w = _fed(name, [(A, A["T"]), (B, B["T"])])
    assert w.remove(A["map"], A["K"], A["T"], A["Lk"])
    only_b, only_a = _fed(name, [(B, B["T"])]), _fed(name, [(A, A["T"])])
    ok, where = same_records(w.records(), only_b.records())
    assert ok, where
    n_only_a = len(np.setdiff1d(only_a.key, only_b.key))
    r = w.rstats
    print(r, "voxels of A", len(only_a.key), "of B", len(only_b.key), "only A", n_only_a)
    assert n_only_a >= 100 and r["vacant"] == n_only_a and r["missing"] == 0 and r["removed"] == only_a.stats["inserted"]
    assert r["removals"] == 1 and r["refused_removals"] == 0 and w.seq == 3
    assert w.stats["occupied"] == len(only_b.key) + n_only_a  # the vacated voxels keep their slots
    t = w.table()
    assert (t["sums"][t["count"] == 0] == 0).all() and (t["keyframes"][t["count"] == 0] == 0).all()


def test_reanchor_equals_the_table_fed_the_new_pose():
    name = "a_203x61"
    A, B = case_steps(name)
    T2 = moved_pose(A["T"])
    w = _fed(name, [(A, A["T"]), (B, B["T"])])
    assert w.reanchor(A["map"], A["K"], A["T"], T2, A["Lk"])
    want = _fed(name, [(B, B["T"]), (A, T2)])
    ok, where = same_records(w.records(), want.records())
    assert ok, where
    stale = _fed(name, [(A, A["T"]), (B, B["T"])])
    assert not same_records(w.records(), stale.records())[0]  # (the motion is large enough to change the table)
    r = w.rstats
    assert r["missing"] == 0 and r["reanchors"] == 1 and r["removals"] == 1 and w.stats["integrations"] == 3 and w.seq == 4
    before = (w.table(), dict(w.stats), w.rstats, w.seq)
    assert not w.reanchor(A["map"], A["K"], T2, T2.copy(), A["Lk"])  # equal bits: nothing, no seq
    assert same_records(w.table(), before[0], fields=("key", "sums", "count", "keyframes"))[0] and (dict(w.stats), w.rstats, w.seq) == before[1:]


@pytest.mark.parametrize("name", OP_CASES)
def test_the_operations_of_a_case_and_the_loop_form(name):
    w = restated_ops(name)
    wl = apply_ops(RR.World(**CASES[name]), reanchor_ops(name), loop=True)
    ok, where = same_records(wl.table(), w.table(), fields=("key", "sums", "count", "keyframes"))
    assert ok, where
    assert wl.stats == w.stats and wl.rstats == w.rstats and wl.seq == w.seq
    # the end of the operations is a table fed every step but the first and the last at their own poses, those two at the moved ones
    steps = case_steps(name)
    seq = [(s, s["T"]) for s in steps[1:-1]]
    if len(steps) > 1:
        seq.append((steps[-1], moved_pose(steps[-1]["T"])))
    seq.append((steps[0], moved_pose(steps[0]["T"], 2)))
    ok, where = same_records(w.records(), _fed(name, seq).records())
    assert ok, where
    r = w.rstats
    print(name, w.stats, r)
    assert r["missing"] == 0 and r["refused_removals"] == 0 and r["removals"] == r["reanchors"] + 1 and r["reanchors"] == (2 if len(steps) > 1 else 1)
    assert r["vacant"] >= 1


def test_removal_from_an_empty_table():
    name = "a_203x61"
    A = case_steps(name)[0]
    w = RR.World(**CASES[name])
    assert w.remove(A["map"], A["K"], A["T"], A["Lk"])
    n = _fed(name, [(A, A["T"])]).stats["inserted"]
    assert w.rstats == dict(removals=1, refused_removals=0, removed=0, missing=n, reanchors=0, vacant=0) and len(w.key) == 0 and n >= 1000


def filled_past_the_bound():
    """case b's strips into 2^12 slots until the table refuses: the operations, and a strip that is refused from then on"""
    steps = case_steps("b_cap12_strips")
    return [("integrate", s, s["T"], None) for s in steps], steps[0]


def test_refused_removal_and_reanchor_touch_nothing():
    name = "b_cap12_strips"
    ops, s = filled_past_the_bound()
    base = apply_ops(RR.World(**CASES[name]), ops)
    assert base.stats["refused"] >= 1 and base.stats["occupied"] + s["map"]["invd"].size > base.stats["capacity"] // 2
    w = apply_ops(RR.World(**CASES[name]), ops)
    assert not w.remove(s["map"], s["K"], s["T"], s["Lk"])
    assert same_records(w.table(), base.table(), fields=("key", "sums", "count", "keyframes"))[0]
    assert w.stats == base.stats and w.rstats == dict(base.rstats, refused_removals=1) and w.seq == base.seq + 1
    w = apply_ops(RR.World(**CASES[name]), ops)
    assert w.reanchor(s["map"], s["K"], s["T"], moved_pose(s["T"]), s["Lk"])  # (the poses differ: the pair is enqueued, and refused)
    assert same_records(w.table(), base.table(), fields=("key", "sums", "count", "keyframes"))[0]
    assert w.stats == dict(base.stats, refused=base.stats["refused"] + 1) and w.seq == base.seq + 2
    assert w.rstats == dict(base.rstats, refused_removals=1, reanchors=1)

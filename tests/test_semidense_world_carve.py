"""Free-space carving on the world-frame voxel map by the numpy restatement alone (tests/semidense_world_carve_restatement.py;
include/vo_hip.h, "Semi-dense world map: free-space carving"). `carve_ops` is the sequence of operations every other
test of the block (the CPU emulation of the kernel, the device) runs a case through: the small cases of tests/test_semidense_world.py
with a carve behind each integration, and the cases of this file — a phantom plane in front of a background, a large sigma that
shortens the rays, a carve into an empty table, `free` on a vacated voxel, clear. The cases meet their conditions; a plain Python loop
over rays and k equals the vectorised form; the guards DESIGN.md §26 quotes hold on the full 640 x 240 maps. No GPU.

The guards' bounds were fixed with the definition, before any kernel ran: on the static scene at most 1 % of the two-keyframe voxels and at most 2 % of all voxels have
free >= 1; of a phantom's voxels at least 0.95 have free >= 1 and at least 0.8 have 2 free > cnt, of the others at most 2 % have
free >= 1."""
import functools

import numpy as np
import pytest

import semidense_world_carve_restatement as CR
import semidense_world_restatement as WR
from test_semidense_world import BASE, CASES, K, _plane, _shift, case_steps, full_maps, same_records

F = np.float32
REUSED = ("a_203x61", "b_cap12_strips", "d_rotated_negative", "e_out_of_range", "f_min_obs_z_max")
OWN = {
    "j_phantom": dict(BASE, capacity_log2=15),
    "k_large_sigma": dict(BASE, capacity_log2=15),
    "l_empty_table": dict(BASE),
    "m_vacated": dict(BASE, capacity_log2=15),
    "n_clear": dict(BASE, capacity_log2=15),
    "o_loaded_far": dict(BASE, capacity_log2=12),
}
CARVE_CASES = dict({k: CASES[k] for k in REUSED}, **OWN)
KP = (K[0], K[1], 48.0, 22.0)
TABLE = ("key", "sums", "count", "keyframes", "free")


def _step(m, L, Kc, T, pad=0):
    return dict(map=m, Lk=L, pad=pad, K=tuple(float(v) for v in Kc), T=np.asarray(T, F))


@functools.lru_cache(maxsize=None)
def carve_ops(name):
    """the operations of a case: tuples (op, step, carve parameters) with op 'integrate' | 'carve' | 'remove' | 'clear'"""
    both = lambda s, **prm: [("integrate", s, None), ("carve", s, prm)]
    if name in REUSED:
        return [o for s in case_steps(name) for o in both(s)]
    if name == "j_phantom":  # 97 x 45 fronto-parallel planes from one pose: 5 m, then 10 m behind it
        return both(_step(*_plane(5.0, 0.002), KP, np.eye(4), 3)) + both(_step(*_plane(10.0, 0.002, seed=4), KP, np.eye(4)))
    if name == "k_large_sigma":  # a plane at 2 m; then one at 4 m whose sigma grows with the column: chi * sz from 0.24 m (> margin * voxel) to 3.8 m
        m, L = _plane(4.0, 0.01, seed=5)
        m["sigma"] = np.broadcast_to(np.linspace(0.005, 0.08, 97).astype(F), (45, 97)).copy()
        far = _step(m, L, KP, np.eye(4))
        return both(_step(*_plane(2.0, 0.002), KP, np.eye(4))) + both(far) + [("carve", far, dict(chi=0.0)), ("carve", far, dict(margin=1.0, chi=0.5, z_near=1.25))]
    if name == "l_empty_table":
        return [("carve", case_steps("a_203x61")[0], {})]
    if name in ("m_vacated", "n_clear"):
        near, far = _step(*_plane(5.0, 0.002), KP, np.eye(4), 3), _step(*_plane(10.0, 0.002, seed=4), KP, _shift(0.02, 0.0, 0.0))
        if name == "m_vacated":  # the near plane is taken out again: its voxels keep their keys and collect free like any other;
            # the extraction skips a vacated voxel, so the plane goes in once more at the end: the count it collected shows
            return [("integrate", near, None), ("remove", near, None)] + both(far) + [("integrate", near, None)]
        return both(near) + both(far) + [("clear", None, None)] + both(near) + both(far)
    if name == "o_loaded_far":  # the strips' table of 4 096 slots, loaded past a third; then carves alone of a far surface behind all of it
        ops = list(carve_ops("b_cap12_strips"))
        for o in ops[0:160:20]:  # (every tenth strip of the pose-2 map: the same pixels' rays, to 29 m)
            s = o[1]
            m = dict(invd=np.full_like(s["map"]["invd"], F(1) / F(29)), sigma=np.full_like(s["map"]["sigma"], 0.001), n_obs=np.full_like(s["map"]["n_obs"], 3))
            ops.append(("carve", dict(s, map=m), {}))
        return ops
    raise KeyError(name)


def apply_ops(w, ops, loop=False):
    for op, s, prm in ops:
        if op == "integrate":
            (w.integrate_loop if loop else w.integrate)(s["map"], s["K"], s["T"], s["Lk"])
        elif op == "remove":
            (w.remove_loop if loop else w.remove)(s["map"], s["K"], s["T"], s["Lk"])
        elif op == "carve":
            (w.carve_loop if loop else w.carve)(s["map"], s["K"], s["T"], **prm)
        else:
            w.clear()
    return w


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restated table after carve_ops(name) — computed once for every test of any module; not to be modified"""
    return apply_ops(CR.World(**CARVE_CASES[name]), carve_ops(name))


def _keys_of(s, name):
    return np.unique(WR.points(s["map"], s["K"], s["T"], None, **CARVE_CASES[name])[0]["key"])


def test_the_cases_meet_their_conditions():
    for name in CARVE_CASES:
        w, ops = restated(name), carve_ops(name)
        c, t = w.cstats, w.table()
        print(name, c, "voxels", len(t["key"]), "with free", int((t["free"] > 0).sum()), "max free", int(t["free"].max(initial=0)))
        assert c["carves"] == sum(o[0] == "carve" for o in ops[max([i for i, o in enumerate(ops) if o[0] == "clear"], default=-1) + 1:])
        assert c["hits"] == int(t["free"].astype(np.uint64).sum()) and c["hits"] <= c["visits"] and c["short_rays"] <= c["rays"]
        # no field of the table but free differs from the run without the carves
        plain = apply_ops(CR.World(**CARVE_CASES[name]), [o for o in ops if o[0] != "carve"])
        ok, where = same_records(t, plain.table(), fields=TABLE[:4])
        assert ok and w.stats == plain.stats and w.rstats == plain.rstats and w.seq == plain.seq and not plain.free.any(), where
        if name == "a_203x61":
            assert c["visits"] >= 100000  # (the static scene: next to no voxel lies in front of another keyframe's surface)
        if name == "b_cap12_strips":  # the long probe chains: the table is loaded past a third, the refused strips are carved all the same
            assert w.stats["refused"] >= 1 and w.stats["occupied"] > 0.35 * w.stats["capacity"] and c["carves"] == len(ops) // 2
        if name == "o_loaded_far":  # hits at the end of long probe chains
            assert w.stats["occupied"] > 0.35 * w.stats["capacity"] and c["hits"] >= 1000 and (t["free"] >= 1).sum() >= 300
        if name == "e_out_of_range":  # samples with key 0: the second pose lies outside the range on y for all but the lowest rays
            s = ops[3][1]
            v, n_rays, n_short = CR.visits(s["map"], s["K"], s["T"], CARVE_CASES[name])
            v0, _, _ = CR.visits(s["map"], s["K"], np.eye(4), CARVE_CASES[name])
            print(name, "visits of the second carve", len(v), "of the same rays in range", len(v0))
            assert len(v) < 0.5 * len(v0) and n_rays > n_short and c["visits"] >= 1000
        if name == "f_min_obs_z_max":  # skipped points cast no ray
            assert c["rays"] == w.stats["inserted"] + w.stats["out_of_range"] and w.stats["skipped"] >= 100
        if name == "j_phantom":
            near, far = _keys_of(ops[0][1], name), _keys_of(ops[2][1], name)
            f = dict(zip(t["key"].tolist(), t["free"].tolist()))
            assert len(near) >= 50 and len(far) >= 50 and all(f[k] >= 1 for k in near.tolist()) and all(f[k] == 0 for k in far.tolist())
        if name == "k_large_sigma":
            far = ops[2][1]
            one = lambda **prm: apply_ops(CR.World(**CARVE_CASES[name]), ops[:3] + [("carve", far, prm)]).cstats
            c3, c0, cn = one(), one(chi=0.0), one(margin=1.0, chi=0.5, z_near=1.25)
            m = far["map"]
            z = F(1) / m["invd"]
            sz = (m["sigma"] * z) * z
            assert (F(3.0) * sz > F(2.0) * F(0.1)).all()  # chi * sz > margin * voxel on every ray: all of them are shortened
            n_short = int((z - F(3.0) * sz <= F(0.5)).sum())  # z - m <= z_near: no k has z_near <= z_k < z_end
            print(name, c3, c0, cn, n_short)
            assert c3["short_rays"] == n_short >= 45 and c0["short_rays"] == 0 and c3["visits"] < c0["visits"] and 0 < c3["hits"] < c0["hits"]
            assert cn["visits"] < c0["visits"]
        if name == "l_empty_table":
            assert c["visits"] >= 10000 and c["hits"] == 0 and len(t["key"]) == 0
        if name == "m_vacated":
            wv = apply_ops(CR.World(**CARVE_CASES[name]), ops[:-1])  # before the plane goes in again
            tv = wv.table()
            vac = tv["count"] == 0
            assert vac.sum() >= 50 and (tv["free"][vac] >= 1).all() and wv.rstats["vacant"] == int(vac.sum())
            assert len(wv.records()["key"]) == int((~vac).sum())  # the extraction skips them as before
            again = np.isin(t["key"], tv["key"][vac])
            assert w.rstats["vacant"] == 0 and np.array_equal(t["free"][again], tv["free"][vac]) and (t["count"][again] >= 1).all()
        if name == "n_clear":
            once = apply_ops(CR.World(**CARVE_CASES[name]), ops[5:])
            ok, where = same_records(t, once.table(), fields=TABLE)
            assert ok and w.cstats == once.cstats and c["carves"] == 2, where


def test_the_short_rays_of_the_large_sigma_case_start_behind_their_end():
    """what `short` means, on numbers: z_near = 0.5 is the sample k = 10 (dz = 0.05), so a ray is short exactly where z_end <= 0.5"""
    assert float(F(10) * F(F(0.1) * F(0.5))) == 0.5 > float(F(9) * F(F(0.1) * F(0.5)))


@pytest.mark.parametrize("name", ["b_cap12_strips", "k_large_sigma"])
def test_a_loop_over_the_rays_equals_the_vectorised_form(name):
    ops = carve_ops(name)
    if name == "b_cap12_strips":
        ops = ops[:16]  # (the first eight strips)
    w = apply_ops(CR.World(**CARVE_CASES[name]), ops)
    wl = apply_ops(CR.World(**CARVE_CASES[name]), ops, loop=True)
    ok, where = same_records(wl.table(), w.table(), fields=TABLE)
    assert ok and wl.cstats == w.cstats and wl.stats == w.stats and w.cstats["visits"] >= 1000, (where, wl.cstats, w.cstats)


def test_the_free_filter_of_the_extraction():
    w = restated("j_phantom")
    rec = w.records()
    assert (rec["free"] > 0).any() and (rec["free"] == 0).any()
    for mf in ((0, 1), (1, 2), (1, 1), (3, 1), (0, 0)):
        got = w.records(max_free=mf)
        want = np.array([int(f) * mf[1] <= int(c) * mf[0] or mf[1] == 0 for f, c in zip(rec["free"], rec["count"])])
        ok, where = same_records(got, {k: v[want] for k, v in rec.items()}, fields=("key", "count", "free", "xyz"))
        assert ok, (mf, where)
    assert len(w.records(max_free=(0, 1))["key"]) == int((rec["free"] == 0).sum())


def test_bad_parameters():
    for prm in (dict(margin=0.5), dict(margin=float("nan")), dict(chi=-1.0), dict(chi=float("inf")), dict(z_near=0.0), dict(z_near=float("nan"))):
        assert not CR.check_params(**prm), prm
    assert CR.check_params() and CR.check_params(margin=1.0, chi=0.0, z_near=1e-3)


# ---- guards on the full 640 x 240 maps, min_obs 1, z_max 30, the default carve parameters ---------------------------------------------
GUARD = dict(BASE, capacity_log2=20)
PHANTOM = (slice(100, 140), slice(290, 350))  # y 100 .. 139, x 290 .. 349 of the pose-2 map


def phantom_maps():
    """the pose-2 map with the phantom in it, the phantom alone (what tells its voxels), the pose-6 map; each with its pose"""
    (m2, _, T2), (m6, _, T6) = full_maps()
    mp = {k: v.copy() for k, v in m2.items()}
    mp["invd"][PHANTOM], mp["sigma"][PHANTOM], mp["n_obs"][PHANTOM] = F(1) / F(4), F(0.002), 3
    alone = {k: np.zeros_like(v) for k, v in mp.items()}
    for k in alone:
        alone[k][PHANTOM] = mp[k][PHANTOM]
    return (mp, T2), (alone, T2), (m6, T6)


def guard_shares(voxel, rec, phantom_keys=None):
    """the figures the guards bound, from an extraction with `free` (dict key or index, count, keyframes, free)"""
    key = rec["key"] if "key" in rec else WR.make_key(*np.asarray(rec["index"], np.int64).T)
    free, cnt, kf = rec["free"], rec["count"], rec["keyframes"]
    g = dict(voxel=voxel, voxels=len(key), with_free=int((free >= 1).sum()), kf2=int((kf >= 2).sum()), kf2_with_free=int(((kf >= 2) & (free >= 1)).sum()))
    if phantom_keys is not None:
        ph = np.isin(key, phantom_keys)
        g.update(phantom=int(ph.sum()), phantom_free=float((free[ph] >= 1).mean()),
                 phantom_half=float((2 * free[ph].astype(np.int64) > cnt[ph].astype(np.int64)).mean()), others_free=float((free[~ph] >= 1).mean()))
    return g


def assert_guards(g):
    if "phantom" not in g:  # the static scene
        assert g["kf2"] >= 1000 and g["kf2_with_free"] <= 0.01 * g["kf2"] and g["with_free"] <= 0.02 * g["voxels"], g
    else:
        assert g["phantom"] >= 10 and g["phantom_free"] >= 0.95 and g["phantom_half"] >= 0.8 and g["others_free"] <= 0.02, g


@functools.lru_cache(maxsize=None)
def guard_figures(voxel, phantom):
    prm = dict(GUARD, voxel=voxel)
    w = CR.World(**prm)
    (mp, T2), (alone, _), (m6, T6) = phantom_maps()
    first = mp if phantom else full_maps()[0][0]
    for m, T in ((first, T2), (m6, T6)):
        assert w.integrate(m, K, T, None)
        w.carve(m, K, T)
    keys = np.unique(WR.points(alone, K, T2, None, **prm)[0]["key"]) if phantom else None
    return guard_shares(voxel, w.records(), keys), w.cstats


@pytest.mark.parametrize("phantom", [False, True])
@pytest.mark.parametrize("voxel", [0.1, 0.2])
def test_guards_on_the_full_maps(voxel, phantom):
    g, c = guard_figures(voxel, phantom)
    print(g, c)
    assert_guards(g)

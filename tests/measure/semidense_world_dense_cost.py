"""What feeding the dense result into the world voxel map (vo_semidense_map_merge, the sources VO_SEMIDENSE_WORLD_DENSE / _MERGED of
vo_svo_set_semidense_world) costs on one MI355X, at 1241 x 376 with bf = 386.1, z_min = 3 m, 128 disparities and 8 paths
(the settings of dense_stereo_cost.py), the speckle filter's defaults, voxel 0.1 m, min_obs 1, z_max 40 m:
  merge        the merge launch alone between two events on the stream (the context's profiler), every plane on the device: the map of
               semidense_world_cost.py (the stream's third pair fused with the next three left images) against the filtered dense result
               of the same pair; planes on 16-byte boundaries (the wide path) and one element off them (single elements). The bytes it
               moves (18 read, 10 written a pixel; 9 + 10 without a map) and, as the yardstick, a device-to-device hipMemcpyAsync of
               half as many bytes — which reads and writes as many in all — between two events of its own. The six counts.
  world        the integration and the carve of the merged map against the same calls on the raw map (the planes the merge read), each
               in a fresh table of 2^22 slots: points inserted, voxels occupied, rays, visits, and the launches' times.
  growth       the stereo loop at BASELINE configs[1] with the source `merged`: voxels occupied after every keyframe, and the number of
               keyframes the default 2^22 slots take before an integration is refused (occupied + W H > 2^21).
  loops        that loop, per frame: static per keyframe + temporal + dense per keyframe + speckle + world map with the source `raw`,
               against THE SAME RUN with the source `merged`, through
                 sync        one trackStereoImages call per frame
                 look_ahead  result k, enqueue k + 1, prefetch k + 2, call by call from Python
               The settings ALTERNATE within one run, every repeat on a fresh context; median and min..max over the repeats.
Measurement tool, not a test.
usage: python tests/measure/semidense_world_dense_cost.py [--frames 72] [--repeats 4] [--no-loops]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from dense_speckle_cost import DENSE  # noqa: E402
from pose_covariance_cost import WARM, Stereo  # noqa: E402
from semidense_regularize_cost import BF, Z_MIN, fused_map, stats  # noqa: E402
from semidense_world_cost import WPRM  # noqa: E402
from semidense_world_reanchor_cost import timed  # noqa: E402

F = np.float32
SOURCES = ("raw", "merged")


def copy_us(hip, dst, src, nbytes, n):
    """a device-to-device hipMemcpyAsync of nbytes on the null stream between two events, n times [us]"""
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    t = []
    for _ in range(n):
        assert hip.hipEventRecord(ev[0], None) == 0
        assert hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), 3, None) == 0
        assert hip.hipEventRecord(ev[1], None) == 0
        assert hip.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        t.append(1e3 * ms.value)
    for e in ev:
        hip.hipEventDestroy(e)
    return t


def merge_and_world(vo, DeviceBuffer, cfg, repeats, batch=20):
    La, Ra = cfg.imgs[2]
    h, w = La.shape
    n = h * w
    out = {"pixels": int(n)}
    T0 = np.asarray(cfg.st.poses(7)[2], F)
    with vo.Context(device=0, max_width=w, max_height=h, max_points=256, n_slots=2, max_level=0) as c:
        m, _ = fused_map(vo, c, cfg, 5)
        c.set_image(0, La)
        c.set_image(1, Ra)
        ds = c.denseStereo(0, 1, speckle=True, **DENSE)
        host = dict(map_invd=m["invd"], map_sigma=m["sigma"], map_n_obs=m["n_obs"], disparity=ds.disparity, sigma_invd=ds.sigma_invd, status=ds.status,
                    invd=np.zeros((h, w), F), sigma=np.zeros((h, w), F), n_obs=np.zeros((h, w), np.uint8), origin=np.zeros((h, w), np.uint8))
        bufs = {}
        try:
            for k, v in host.items():  # (room for one element in front: the misaligned variant starts there)
                flat = np.concatenate([np.zeros(1, v.dtype), np.ascontiguousarray(v).reshape(-1), np.zeros(16, v.dtype)])
                bufs[k] = (DeviceBuffer(flat), v.dtype.itemsize)
            c.profile_enable(4)
            for name, lead in (("aligned", 16), ("one_element_off", 1)):
                # `aligned`: 16 elements in: 64 bytes for f32, 16 for u8. The planes' contents moved with the pointer: refill.
                ptr = {}
                for k, (b, sz) in bufs.items():
                    v = np.ascontiguousarray(host[k]).reshape(-1)
                    flat = np.zeros(n + 17, v.dtype)
                    flat[lead:lead + n] = v
                    assert b.hip.hipMemcpy(b.ptr, flat.ctypes.data_as(C.c_void_p), C.c_size_t(flat.nbytes), 1) == 0
                    ptr[k] = b.data_ptr() + lead * sz
                mp = {k: ptr["map_" + k] for k in ("invd", "sigma", "n_obs")}
                dp = tuple(ptr[k] for k in ("disparity", "sigma_invd", "status"))
                op = {k: ptr[k] for k in ("invd", "sigma", "n_obs", "origin")}
                res = {}
                for what, mm in (("merged", mp), ("dense_only", None)):
                    call = lambda: c.semiDenseMapMerge(mm, dp, BF, out=op, on_device=(w, h))  # noqa: E731
                    r = call()
                    us = timed(c, lambda: None, call, repeats * batch, 1)
                    nbytes = n * (28 if mm else 19)
                    res[what] = dict(us=stats(us, 2), bytes=nbytes, tb_per_s=round(nbytes / (np.median(us) * 1e-6) / 1e12, 3),
                                     counts=[int(x) for x in r.counts])
                out[name] = res
            b0, b1 = DeviceBuffer(np.zeros(28 * n, np.uint8)), DeviceBuffer(np.zeros(28 * n, np.uint8))
            try:
                # 28 n bytes copied: the merge's byte count as a copy's size; 14 n copied: the same 28 n bytes read and written in all
                for what, nb in (("copy_28_bytes_a_pixel", 28 * n), ("copy_14_bytes_a_pixel", 14 * n)):
                    copy_us(b0.hip, b1.data_ptr(), b0.data_ptr(), nb, 3)
                    us = copy_us(b0.hip, b1.data_ptr(), b0.data_ptr(), nb, repeats * batch)
                    out[what] = dict(us=stats(us, 2), bytes_copied=nb, tb_per_s_moved=round(2 * nb / (np.median(us) * 1e-6) / 1e12, 3))
            finally:
                b0.free()
                b1.free()
            # ---- the merged map against the raw one through the world map's launches
            mg = c.semiDenseMapMerge(m, ds, BF)
            world = {}
            for what, planes in (("raw", m), ("merged", dict(invd=mg.invd, sigma=mg.sigma, n_obs=mg.n_obs))):
                db = {k: DeviceBuffer(np.ascontiguousarray(v)) for k, v in planes.items()}
                pl = {k: b.data_ptr() for k, b in db.items()}
                try:
                    with c.semiDenseWorld(**WPRM) as wm:
                        wm.integrate(pl, cfg.K, T0, on_device=(w, h))
                        st = wm.stats()
                        res = dict(entries=int((planes["n_obs"] >= WPRM["min_obs"]).sum()), inserted=st["inserted"], voxels=st["occupied"])
                        res["integrate_us"] = stats(timed(c, lambda: None, lambda: wm.integrate(pl, cfg.K, T0, on_device=(w, h)), repeats * batch, 1), 2)
                        c0 = wm.carveStats()
                        res["carve_us"] = stats(timed(c, lambda: None, lambda: wm.carve(pl, cfg.K, T0, on_device=(w, h)), repeats * batch, 1), 2)
                        c1 = wm.carveStats()
                        k = c1["carves"] - c0["carves"]
                        res["per_carve"] = {q: (c1[q] - c0[q]) // k for q in ("rays", "short_rays", "visits", "hits")}
                        world[what] = res
                finally:
                    for b in db.values():
                        b.free()
            out["world_one_map"] = world
        finally:
            for b, _ in bufs.values():
                b.free()
    return out


def make(vo, cfg, c, source):
    o, _ = cfg.make(vo, c, False)
    o.setSemiDense(dict(bf=BF, z_min=Z_MIN), every="keyframe")
    o.setSemiDenseTemporal({})
    o.setDenseStereo(dict(DENSE), every="keyframe")
    o.setDenseSpeckle(True)
    o.setSemiDenseWorld(dict(WPRM, source=source))  # (the default 2^22 slots)
    return o


def growth(vo, cfg):
    src, n = cfg.src, len(cfg.src)
    occ, refused_at = [], None
    with cfg.context(vo) as c:
        o = make(vo, cfg, c, "merged")
        for k in range(n):
            if cfg.track(o, src[k]).is_keyframe:
                st = o.getSemiDenseWorldStats()
                occ.append(st["occupied"])
                if st["refused"] and refused_at is None:
                    refused_at = st["integrations"]
        st = o.getSemiDenseWorldStats()
        o.close()
    steps = [b - a for a, b in zip(occ[:-1], occ[1:]) if b > a]
    return dict(occupied_after_each_keyframe=occ, voxels_added_per_keyframe=stats(steps, 0) if steps else None, integrations=st["integrations"],
                refused=st["refused"], integrations_before_first_refusal=refused_at, capacity=st["capacity"])


def one_run(vo, cfg, mode, source):
    src, n = cfg.src, len(cfg.src)
    n_kf = 0
    with cfg.context(vo) as c:
        o = make(vo, cfg, c, source)
        t0 = None
        if mode == "sync":
            for k in range(n):
                if k == WARM:
                    t0 = time.perf_counter()
                n_kf += int(cfg.track(o, src[k]).is_keyframe)
        else:
            cfg.enqueue(o, src[0])
            cfg.prefetch(o, src[1])
            for k in range(n):
                if k == WARM:
                    t0 = time.perf_counter()
                n_kf += int(o.result().is_keyframe)
                if k + 1 < n:
                    cfg.enqueue(o, src[k + 1])
                    if k + 2 < n:
                        cfg.prefetch(o, src[k + 2])
        o.getDenseStereo()
        o.getSemiDenseWorldStats()  # (the side stream's last launches belong to the run)
        dt = time.perf_counter() - t0
        st = o.getSemiDenseWorldStats()
        o.close()
    return 1e3 * dt / (n - WARM), n_kf, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=72)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--no-loops", action="store_true")
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    from util import DeviceBuffer
    cfg = Stereo(S, a.frames)
    out = {"launch_1241x376": merge_and_world(vo, DeviceBuffer, cfg, a.repeats)}
    print(json.dumps(out), flush=True)
    if not a.no_loops:
        cfg.upload(DeviceBuffer)
        res = {}
        try:
            res["growth_merged"] = growth(vo, cfg)
            print(json.dumps(res), flush=True)
            for mode in ("sync", "look_ahead"):
                one_run(vo, cfg, mode, "merged")  # (untimed: code objects loaded, clocks up)
                t = {s: [] for s in SOURCES}
                for _ in range(a.repeats):
                    for s in SOURCES:
                        ms, n_kf, st = one_run(vo, cfg, mode, s)
                        t[s].append(ms)
                        res.setdefault("stats_" + s, st)
                res[mode] = {s: stats(v) for s, v in t.items()}
                res[mode]["keyframes"] = n_kf
        finally:
            cfg.free()
        out["stereo_configs1"] = res
    out["unit"] = "loops: ms per frame; launches: us"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()

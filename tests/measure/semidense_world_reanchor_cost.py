"""What removal and re-anchoring on the world-frame voxel map (vo_semidense_world_remove / _reanchor,
vo_svo_set_semidense_world_reanchor) cost on one MI355X, at 1241 x 376 with bf = 386.1, voxel 0.1 m, min_obs 1, z_max
40 m, in the form of semidense_world_cost.py:
  launch       the map of that script (the stream's third pair fused with the next three left images), every plane on the device, in a
               table that holds it: the removal alone between two events on the stream (the context's profiler) — each one undoes
               an integration made in front of the timed region —, and the re-anchor's pair, removal and integration back to back,
               with the pose moved to and fro by a few centimetres.
  loops        the stereo loop at BASELINE configs[1] (the stream and settings of semidense_world_cost.py, device images), per frame:
               static per keyframe + temporal + world map, against THE SAME RUN with the re-anchoring on, min_move 0 and min_move
               0.25 voxels, through
                 sync        one trackStereoImages call per frame
                 look_ahead  result k, enqueue k + 1, prefetch k + 2, call by call from Python
               The settings ALTERNATE within one run, every repeat on a fresh context; median and min..max over the repeats.
  effect       on the 640 x 240 synthetic stream of the tests (20 frames, true poses known): per integrated keyframe the pose error
               (translation [m], rotation [rad]) of the pose its map was integrated with and of the applied pose, against the true
               pose relative to the first frame; the number of two-keyframe voxels and the share of them within one voxel edge of the
               corridor's surface, with and without the option. Recorded whichever way they come out.
Measurement tool, not a test.
usage: python tests/measure/semidense_world_reanchor_cost.py [--frames 80] [--repeats 4] [--no-loops] [--no-effect]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pose_covariance_cost import WARM, Stereo  # noqa: E402
from semidense_regularize_cost import BF, K_AUX, Z_MIN, fused_map, stats  # noqa: E402
from semidense_world_cost import WPRM  # noqa: E402

SETTINGS = (("world", None), ("reanchor_0", 0.0), ("reanchor_0.25", 0.25))
F = np.float32


def timed(c, prepare, call, n, launches):
    c.profile_set_classes(1 << K_AUX)
    t = []
    for _ in range(n):
        prepare()
        c.profile_reset()
        call()
        k, ms = c.profile_get(K_AUX)
        assert k == launches, k
        t.append(1e3 * ms)
    c.profile_set_classes(1 << 0)  # (the profiler cannot be switched off: a class these launches are not in)
    return t


def launch(vo, DeviceBuffer, cfg, repeats, batch=20):
    La = cfg.imgs[2][0]
    h, w = La.shape
    out = {"pixels": int(h * w)}
    T0 = np.asarray(cfg.st.poses(7)[2], F)
    T1 = T0.copy()
    T1[:3, 3] += F(0.03), F(-0.02), F(0.04)
    with vo.Context(device=0, max_width=w, max_height=h, max_points=256, n_slots=2, max_level=0) as c:
        m, _ = fused_map(vo, c, cfg, 5)
        bufs = {k: DeviceBuffer(np.ascontiguousarray(v)) for k, v in m.items()}
        dkey = DeviceBuffer(La)
        planes = {k: b.data_ptr() for k, b in bufs.items()}
        kw = dict(key=dkey.data_ptr(), on_device=(w, h), key_on_device=w)
        try:
            c.profile_enable(4)
            with c.semiDenseWorld(**WPRM, capacity_log2=22) as wm:
                wm.integrate(planes, cfg.K, T0, **kw)
                out["voxels"] = len(wm.points().xyz)
                out["remove_us"] = stats(timed(c, lambda: wm.integrate(planes, cfg.K, T0, **kw), lambda: wm.remove(planes, cfg.K, T0, **kw),
                                               repeats * batch, 1), 2)
                pose = [T0, T1]

                def pair():
                    assert wm.reanchor(planes, cfg.K, pose[0], pose[1], **kw)
                    pose.reverse()
                out["reanchor_pair_us"] = stats(timed(c, lambda: None, pair, repeats * batch, 2), 2)
                r = wm.reanchorStats()
                assert r["missing"] == 0 and r["refused_removals"] == 0, r
                out["reanchor_stats"] = r
        finally:
            dkey.free()
            for b in bufs.values():
                b.free()
    return out


def one_run(vo, cfg, mode, min_move):
    src, n = cfg.src, len(cfg.src)
    n_kf = 0
    with cfg.context(vo) as c:
        o, _ = cfg.make(vo, c, False)
        o.setSemiDense(dict(bf=BF, z_min=Z_MIN), every="keyframe")
        o.setSemiDenseTemporal({})
        o.setSemiDenseWorld(dict(WPRM))  # (the default 2^22 slots)
        if min_move is not None:
            o.setSemiDenseWorldReanchor(dict(min_move=min_move))
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
        o.getSemiDenseWorldStats()  # (the side stream's last launch belongs to the run)
        dt = time.perf_counter() - t0
        st = dict(o.getSemiDenseWorldStats(), **o.getSemiDenseWorldReanchorStats())
        o.close()
    return 1e3 * dt / (n - WARM), n_kf, st


def effect(vo):
    from visual_odometry_ros_amd import synthetic as S
    from test_semidense_temporal_gpu import K, SH, SW, TPRM, _driver
    from test_semidense_world import surface_distance
    n, voxel = 20, 0.1
    st = S.StereoStream(width=SW, height=SH, K=K, n_u=20, n_v=8, seed=2, speed=0.5)
    true = [np.asarray(p, np.float64) for p in st.poses(n)]
    imgs = [st.render_pair(p)[:2] for p in true]
    sd = dict(bf=float(F(K[0] * st.baseline)), d_min=0, d_max=67, every="keyframe", temporal=dict(TPRM))
    out = {}
    for name, world in (("off", dict(voxel=voxel, capacity_log2=20, min_obs=1, z_max=30.0)),
                        ("on", dict(voxel=voxel, capacity_log2=20, min_obs=1, z_max=30.0, reanchor=True))):
        c, svo = _driver(vo, st, dict(sd, world=world))
        try:
            own, pos = {}, {}
            for k in range(n):
                pos[int(svo.trackStereoImages(*imgs[k]).frame_id)] = k
                m = svo.getSemiDenseMap()
                if m is not None:
                    own[int(m.frame_id)] = m.T_wc.astype(np.float64)
            svo.flushSemiDenseWorld()
            kf2 = svo.getSemiDenseWorld(min_keyframes=2)
            res = dict(voxels=len(svo.getSemiDenseWorld().xyz), voxels_kf2=len(kf2.xyz),
                       share_kf2_near_surface=round(float((surface_distance(kf2.xyz @ true[0][:3, :3].T + true[0][:3, 3]) <= voxel).mean()), 4))
            if name == "on":
                an = svo.getSemiDenseWorldAnchors()
                res["reanchor_stats"] = svo.getSemiDenseWorldReanchorStats()
                rows = []
                for fid, T in zip(an["frame_id"], an["T_wk"]):
                    ref = np.linalg.inv(true[0]) @ true[pos[int(fid)]]

                    def err(Tx):
                        d = np.linalg.inv(ref) @ Tx
                        return [float(np.linalg.norm(d[:3, 3])), float(np.arccos(np.clip((np.trace(d[:3, :3]) - 1) / 2, -1, 1)))]
                    rows.append(dict(frame_id=int(fid), integrated=err(own[int(fid)]), applied=err(T.astype(np.float64))))
                res["pose_error_m_rad"] = rows
            out[name] = res
        finally:
            svo.close()
            c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=80)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--no-loops", action="store_true")
    ap.add_argument("--no-effect", action="store_true")
    a = ap.parse_args()
    import visual_odometry_ros_amd as vo
    from visual_odometry_ros_amd import synthetic as S
    from util import DeviceBuffer
    cfg = Stereo(S, a.frames)
    out = {"launch_1241x376": launch(vo, DeviceBuffer, cfg, a.repeats)}
    print(json.dumps(out), flush=True)
    if not a.no_effect:
        out["effect_640x240"] = effect(vo)
        print(json.dumps({"effect_640x240": out["effect_640x240"]}), flush=True)
    if not a.no_loops:
        cfg.upload(DeviceBuffer)
        res = {}
        try:
            for mode in ("sync", "look_ahead"):
                one_run(vo, cfg, mode, 0.0)  # (untimed: code objects loaded, clocks up)
                t = {s: [] for s, _ in SETTINGS}
                for _ in range(a.repeats):
                    for s, mm in SETTINGS:
                        ms, n_kf, st = one_run(vo, cfg, mode, mm)
                        t[s].append(ms)
                        res.setdefault("stats_" + s, st)
                res[mode] = {s: stats(v) for s, v in t.items()}
                res[mode]["keyframes"] = n_kf
        finally:
            cfg.free()
        out["stereo_configs1"] = res
    out["unit"] = "loops: ms per frame; launch: us"
    out["frames_timed"], out["repeats"] = a.frames - WARM, a.repeats
    print(json.dumps(out))


if __name__ == "__main__":
    main()

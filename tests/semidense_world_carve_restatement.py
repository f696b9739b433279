"""Free-space carving on the world-frame voxel map (include/vo_hip.h, "Semi-dense world map: free-space carving"),
restated on top of tests/semidense_world_reanchor_restatement.py and independent of the kernels: every float operation a float32
numpy operation of its own in the order the header states, the samples of a chunk of rays a (rays x k) array over ALL k of 1 .. 4096
up to the chunk's longest ray — the sample test, the key and the consecutive rule are evaluated for every one of them, there is no
first or last k worked out in advance — the visited voxels found with np.unique, looked up in the table's sorted key array and added to
`free`, an unsigned 32-bit array next to the table's others. `World.carve_loop` is the same definition once more as a plain Python
loop over rays and k with scalar float32 arithmetic on a dict. Every operation of the classes below (integrate, remove, re-anchor)
carries `free` along by key: it belongs to the cell, whatever happens to the sums."""
import numpy as np

import semidense_world_reanchor_restatement as RR
import semidense_world_restatement as WR

F = np.float32
CARVE_DEFAULTS = dict(margin=2.0, chi=3.0, z_near=0.5)
CCOUNTERS = ("carves", "rays", "short_rays", "visits", "hits")
MAX_K = 4096
M32 = (1 << 32) - 1


def check_params(**prm):
    p = dict(CARVE_DEFAULTS, **prm)
    m, c, zn = (float(F(p[k])) for k in ("margin", "chi", "z_near"))
    return np.isfinite([m, c, zn]).all() and m >= 1.0 and c >= 0.0 and zn > 0.0


def rays(m, world_params):
    """the pixels that cast a ray, in raster order: ys, xs, z, sigma"""
    p = dict(WR.DEFAULTS, **world_params)
    ys, xs = np.nonzero(WR.entries(m))
    with np.errstate(all="ignore"):
        invd, sigma, no = m["invd"][ys, xs].astype(F), m["sigma"][ys, xs].astype(F), m["n_obs"][ys, xs].astype(np.int64)
        z = (F(1) / invd).astype(F)
        keep = ~((no < int(p["min_obs"])) | (z > F(p["z_max"])))
    return ys[keep], xs[keep], z[keep], sigma[keep]


def sample_keys(xs, ys, zk, K, T_wk, voxel):
    """key of the sample at depth zk [n, nk] on the rays of the pixels xs, ys [n]; 0 where an axis is out of range"""
    fx, fy, cx, cy = (F(v) for v in K)
    T = np.asarray(T_wk, F).reshape(4, 4)
    with np.errstate(all="ignore"):
        X = (((xs.astype(F) - cx).astype(F) / fx).astype(F)[:, None] * zk).astype(F)
        Y = (((ys.astype(F) - cy).astype(F) / fy).astype(F)[:, None] * zk).astype(F)
        ok = np.ones(zk.shape, bool)
        idx = []
        for r in range(3):
            inner = ((T[r, 1] * Y).astype(F) + (T[r, 2] * zk).astype(F)).astype(F)
            Xw = (((T[r, 0] * X).astype(F) + inner).astype(F) + T[r, 3]).astype(F)
            fl = np.floor((Xw / voxel).astype(F)).astype(F)
            ok &= (fl >= F(-1048576.0)) & (fl < F(1048576.0))
            idx.append(np.where(ok, fl, 0).astype(np.int64))
    return np.where(ok, WR.make_key(*idx), np.uint64(0))


def visits(m, K, T_wk, world_params, chunk=2048, **prm):
    """the visited keys of one carve, one entry per visit (any order), and the numbers of rays and of short rays"""
    p, c = dict(WR.DEFAULTS, **world_params), dict(CARVE_DEFAULTS, **prm)
    voxel, margin, chi, z_near = F(p["voxel"]), F(c["margin"]), F(c["chi"]), F(c["z_near"])
    ys, xs, z, sigma = rays(m, world_params)
    with np.errstate(all="ignore"):
        sz = ((sigma * z).astype(F) * z).astype(F)
        mm = np.fmax(F(margin * voxel), (chi * sz).astype(F)).astype(F)  # fmaxf: the other operand where one is NaN
        z_end = (z - mm).astype(F)
        dz = F(voxel * F(0.5))
        zk_all = (np.arange(1, MAX_K + 1).astype(F) * dz).astype(F)
    out, n_short = [], 0
    for i0 in range(0, len(z), chunk):
        sl = slice(i0, i0 + chunk)
        ze = z_end[sl]
        nk = int((zk_all < ze.max(initial=-np.inf)).sum()) if len(ze) else 0  # (no k behind this one is a sample of any ray of the chunk)
        zk = np.broadcast_to(zk_all[:nk], (len(ze), nk))
        sample = (z_near <= zk) & (zk < ze[:, None])
        n_short += int((~sample.any(1)).sum())
        if nk == 0:
            continue
        key = sample_keys(xs[sl], ys[sl], zk, K, T_wk, voxel)
        prev_is_sample = np.concatenate([np.zeros((len(ze), 1), bool), sample[:, :-1]], 1)
        prev_key = np.concatenate([np.zeros((len(ze), 1), np.uint64), key[:, :-1]], 1)
        visit = sample & (key != 0) & (~prev_is_sample | (key != prev_key))
        out.append(key[visit])
    return (np.concatenate(out) if out else np.zeros(0, np.uint64)), len(z), n_short


class World(RR.World):
    def clear(self):
        super().clear()
        self.free = np.zeros(0, np.uint32)
        self._c = dict.fromkeys(CCOUNTERS, 0)

    @property
    def cstats(self):
        return dict(self._c)

    def _carry(self, op, *a, **k):
        """an operation of the classes below, with `free` carried along by key"""
        keys, free = self.key.copy(), self.free
        r = op(*a, **k)
        new = np.zeros(len(self.key), np.uint32)
        new[np.searchsorted(self.key, keys)] = free  # (no operation drops a key)
        self.free = new
        return r

    def integrate(self, *a, **k):
        return self._carry(super().integrate, *a, **k)

    def integrate_loop(self, *a, **k):
        return self._carry(super().integrate_loop, *a, **k)

    def remove(self, *a, **k):
        return self._carry(super().remove, *a, **k)

    def remove_loop(self, *a, **k):
        return self._carry(super().remove_loop, *a, **k)

    def _add(self, keys, counts, n_rays, n_short):
        pos = np.minimum(np.searchsorted(self.key, keys), max(len(self.key) - 1, 0))
        found = self.key[pos] == keys if len(self.key) else np.zeros(len(keys), bool)
        with np.errstate(over="ignore"):
            self.free[pos[found]] += counts[found].astype(np.uint32)  # (distinct keys; modulo 2^32)
        c = self._c
        c["carves"] += 1
        c["rays"] += n_rays
        c["short_rays"] += n_short
        c["visits"] += int(counts.sum())
        c["hits"] += int(counts[found].sum())

    def carve(self, m, K, T_wk, **prm):
        """one carve of the map m (dict invd, sigma, n_obs; not modified); never refused, no seq"""
        assert check_params(**prm)
        v, n_rays, n_short = visits(m, K, T_wk, self.p, **prm)
        uk, cnt = np.unique(v, return_counts=True)
        self._add(uk, cnt.astype(np.uint64), n_rays, n_short)

    def carve_loop(self, m, K, T_wk, **prm):
        """the same carve as a loop over the pixels in raster order and over every k of 1 .. 4096 short of the ray's end, scalar float32"""
        p, c = self.p, dict(CARVE_DEFAULTS, **prm)
        voxel, z_max = F(p["voxel"]), F(p["z_max"])
        margin, chi, z_near = F(c["margin"]), F(c["chi"]), F(c["z_near"])
        fx, fy, cx, cy = (F(v) for v in K)
        T = np.asarray(T_wk, F).reshape(4, 4)
        H, W = m["invd"].shape
        seen, n_rays, n_short = {}, 0, 0
        dz = F(voxel * F(0.5))
        with np.errstate(all="ignore"):
            for y in range(H):
                for x in range(W):
                    no, iv, sg = int(m["n_obs"][y, x]), F(m["invd"][y, x]), F(m["sigma"][y, x])
                    if not (no >= 1 and sg > 0 and sg <= WR.FMAX and iv > 0 and iv <= WR.FMAX):
                        continue
                    z = F(F(1) / iv)
                    if no < int(p["min_obs"]) or z > z_max:
                        continue
                    n_rays += 1
                    sz = F(F(sg * z) * z)
                    a, b = F(margin * voxel), F(chi * sz)
                    mm = a if (np.isnan(b) or a >= b) else b
                    z_end = F(z - mm)
                    rx, ry = F(F(F(x) - cx) / fx), F(F(F(y) - cy) / fy)
                    n_samples, prev = 0, None
                    for k in range(1, MAX_K + 1):
                        zk = F(F(k) * dz)
                        if not zk < z_end:
                            break  # (z_k does not fall with k)
                        if not z_near <= zk:
                            continue
                        n_samples += 1
                        X = (F(rx * zk), F(ry * zk), zk)
                        key = 1 << 63
                        for r in range(3):
                            Xw = F(F(F(T[r, 0] * X[0]) + F(F(T[r, 1] * X[1]) + F(T[r, 2] * X[2]))) + T[r, 3])
                            fl = F(np.floor(F(Xw / voxel)))
                            if not (fl >= F(-1048576.0) and fl < F(1048576.0)):
                                key = 0
                                break
                            key |= (int(fl) + (1 << 20)) << (42 - 21 * r)
                        if key != 0 and (prev is None or key != prev):
                            seen[key] = seen.get(key, 0) + 1
                        prev = key
                    n_short += n_samples == 0
        ks = sorted(seen)
        self._add(np.array(ks, np.uint64), np.array([seen[k] for k in ks], np.uint64), n_rays, n_short)

    def table(self):
        return dict(super().table(), free=self.free.copy())

    def records(self, min_count=1, min_keyframes=1, max_free=None):
        """the extraction with `free`; max_free=(num, den): with den >= 1 only the voxels with free * den <= cnt * num"""
        sel = (self.cnt >= min_count) & (self.kf_cnt >= min_keyframes)
        rec = dict(super().records(min_count, min_keyframes), free=self.free[sel])
        if max_free is not None and int(max_free[1]) >= 1:
            num, den = np.uint64(max_free[0]), np.uint64(max_free[1])
            keep = rec["free"].astype(np.uint64) * den <= rec["count"].astype(np.uint64) * num
            rec = {k: v[keep] for k, v in rec.items()}
        return rec

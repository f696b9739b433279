"""The world-frame voxel map (include/vo_hip.h, "Semi-dense world map"), restated in numpy from the definition and
independent of the kernels: every float operation a float32 numpy operation of its own in the order the header states, the voxels of
one integration found with np.unique and summed with np.add.at on unsigned 64-bit integers, the table a set of arrays sorted by key —
no hash, no slot, no atomics. `World.integrate_loop` is the same definition once more as a plain Python loop over the points into a
dict, with scalar float32 arithmetic; it also walks an open-addressing table in raster order to count the insertions whose home slot
was taken (a property of the case, not of the result: which slot a voxel sits in depends on arrival order)."""
import numpy as np

DEFAULTS = dict(voxel=0.10, capacity_log2=22, min_obs=2, z_max=40.0)
F = np.float32
FMAX = np.finfo(np.float32).max
HASH_MUL = 0x9E3779B97F4A7C15
SUMS = ("sw", "sx", "sy", "sz", "sg")
COUNTERS = ("occupied", "capacity", "integrations", "refused", "inserted", "skipped", "out_of_range")


def entries(m):
    with np.errstate(all="ignore"):
        return (m["n_obs"] >= 1) & (m["sigma"] > 0) & (m["sigma"] <= FMAX) & (m["invd"] > 0) & (m["invd"] <= FMAX)


def make_key(ix, iy, iz):
    o = np.uint64(1 << 20)
    return (np.uint64(1 << 63) | ((ix.astype(np.int64).astype(np.uint64) + o) << np.uint64(42)) |
            ((iy.astype(np.int64).astype(np.uint64) + o) << np.uint64(21)) | (iz.astype(np.int64).astype(np.uint64) + o))


def key_index(key):
    key = np.asarray(key, np.uint64)
    return np.stack([((key >> np.uint64(s)) & np.uint64(0x1FFFFF)).astype(np.int64) - (1 << 20) for s in (42, 21, 0)], -1).astype(np.int32)


def home_slot(key, capacity_log2):
    return ((int(key) * HASH_MUL) & ((1 << 64) - 1)) >> (64 - capacity_log2)


def points(m, K, T_wk, Lk=None, **params):
    """the points of one integration in raster order: dict(key u64, wq, q [n, 3], grey, y, x), and the numbers skipped / out of range"""
    p = dict(DEFAULTS, **params)
    voxel, z_max = F(p["voxel"]), F(p["z_max"])
    fx, fy, cx, cy = (F(v) for v in K)
    T = np.asarray(T_wk, F).reshape(4, 4)
    ys, xs = np.nonzero(entries(m))
    with np.errstate(all="ignore"):
        invd, sigma, no = m["invd"][ys, xs].astype(F), m["sigma"][ys, xs].astype(F), m["n_obs"][ys, xs].astype(np.int64)
        z = (F(1) / invd).astype(F)
        skip = (no < int(p["min_obs"])) | (z > z_max)
        keep = ~skip
        ys, xs, z, sigma = ys[keep], xs[keep], z[keep], sigma[keep]
        X = (((xs.astype(F) - cx).astype(F) / fx).astype(F) * z).astype(F)
        Y = (((ys.astype(F) - cy).astype(F) / fy).astype(F) * z).astype(F)
        idx, q, ok = [], [], np.ones(len(z), bool)
        for r in range(3):
            inner = ((T[r, 1] * Y).astype(F) + (T[r, 2] * z).astype(F)).astype(F)
            Xw = (((T[r, 0] * X).astype(F) + inner).astype(F) + T[r, 3]).astype(F)
            u = (Xw / voxel).astype(F)
            fl = np.floor(u).astype(F)
            ok &= (fl >= F(-1048576.0)) & (fl < F(1048576.0))
            idx.append(fl)
            q.append(((u - fl).astype(F) * F(1024)).astype(F))
        sel = ok
        ys, xs, z, sigma = ys[sel], xs[sel], z[sel], sigma[sel]
        idx = [v[sel].astype(np.int64) for v in idx]
        q = np.stack([np.minimum(v[sel].astype(np.int64), 1023) for v in q], -1).reshape(-1, 3)
        sz = ((sigma * z).astype(F) * z).astype(F)
        rr = (voxel / sz).astype(F)
        w = (rr * rr).astype(F)
        wq = np.where(w >= F(65535.0), 65536, np.where(w >= F(65535.0), 0, w).astype(np.int64) + 1).astype(np.uint64)
    grey = Lk[ys, xs].astype(np.uint64) if Lk is not None else np.zeros(len(ys), np.uint64)
    return dict(key=make_key(*idx), wq=wq, q=q.astype(np.uint64), grey=grey, y=ys, x=xs), int(skip.sum()), int((~ok).sum())


class World:
    def __init__(self, **params):
        self.p = dict(DEFAULTS, **params)
        self.clear()

    def clear(self):
        self.key = np.zeros(0, np.uint64)
        self.sums = np.zeros((0, 5), np.uint64)
        self.cnt = np.zeros(0, np.uint32)
        self.kf_cnt = np.zeros(0, np.uint32)
        self.seq = 0
        self.stats = dict.fromkeys(COUNTERS, 0)
        self.stats["capacity"] = 1 << int(self.p["capacity_log2"])
        self.home_taken = 0      # integrate_loop only
        self._slots = {}         # integrate_loop only: slot -> key

    def _accept(self, m):
        self.seq += 1
        H, W = m["invd"].shape
        if self.stats["occupied"] + W * H > self.stats["capacity"] // 2:
            self.stats["refused"] += 1
            return False
        return True

    def integrate(self, m, K, T_wk, Lk=None):
        """one integration of the map m (dict invd, sigma, n_obs; not modified); False: refused as a whole"""
        if not self._accept(m):
            return False
        P, n_skip, n_oor = points(m, K, T_wk, Lk, **self.p)
        uk, inv = np.unique(P["key"], return_inverse=True)
        s = np.zeros((len(uk), 5), np.uint64)
        np.add.at(s[:, 0], inv, P["wq"])
        for a in range(3):
            np.add.at(s[:, 1 + a], inv, P["wq"] * P["q"][:, a])
        np.add.at(s[:, 4], inv, P["wq"] * P["grey"])
        c = np.bincount(inv, minlength=len(uk)).astype(np.uint32)
        allk = np.union1d(self.key, uk)
        sums, cnt, kf = np.zeros((len(allk), 5), np.uint64), np.zeros(len(allk), np.uint32), np.zeros(len(allk), np.uint32)
        io, inw = np.searchsorted(allk, self.key), np.searchsorted(allk, uk)
        sums[io], cnt[io], kf[io] = self.sums, self.cnt, self.kf_cnt
        sums[inw] += s
        cnt[inw] += c
        kf[inw] += np.uint32(1)
        self.key, self.sums, self.cnt, self.kf_cnt = allk, sums, cnt, kf
        self._count(len(P["key"]), n_skip, n_oor)
        return True

    def _count(self, n_ins, n_skip, n_oor):
        st = self.stats
        st["occupied"] = len(self.key)
        st["integrations"] += 1
        st["inserted"] += n_ins
        st["skipped"] += n_skip
        st["out_of_range"] += n_oor

    def integrate_loop(self, m, K, T_wk, Lk=None):
        """the same integration as a loop over the pixels in raster order, scalar float32 arithmetic, into a dict"""
        if not self._accept(m):
            return False
        p = self.p
        voxel, z_max = F(p["voxel"]), F(p["z_max"])
        fx, fy, cx, cy = (F(v) for v in K)
        T = np.asarray(T_wk, F).reshape(4, 4)
        tab = {int(k): [int(v) for v in s] + [int(c), int(f)] for k, s, c, f in zip(self.key, self.sums, self.cnt, self.kf_cnt)}
        seen = set()
        H, W = m["invd"].shape
        n_ins = n_skip = n_oor = 0
        cap_log2 = int(p["capacity_log2"])
        mask = (1 << cap_log2) - 1
        with np.errstate(all="ignore"):
            for y in range(H):
                for x in range(W):
                    no, iv, sg = int(m["n_obs"][y, x]), F(m["invd"][y, x]), F(m["sigma"][y, x])
                    if not (no >= 1 and sg > 0 and sg <= FMAX and iv > 0 and iv <= FMAX):
                        continue
                    z = F(F(1) / iv)
                    if no < int(p["min_obs"]) or z > z_max:
                        n_skip += 1
                        continue
                    X = (F(F(F(F(x) - cx) / fx) * z), F(F(F(F(y) - cy) / fy) * z), z)
                    key, qs, ok = 1 << 63, [], True
                    for r in range(3):
                        Xw = F(F(F(T[r, 0] * X[0]) + F(F(T[r, 1] * X[1]) + F(T[r, 2] * X[2]))) + T[r, 3])
                        u = F(Xw / voxel)
                        fl = F(np.floor(u))
                        if not (fl >= F(-1048576.0) and fl < F(1048576.0)):
                            ok = False
                            break
                        qs.append(min(int(F(F(u - fl) * F(1024))), 1023))
                        key |= (int(fl) + (1 << 20)) << (42 - 21 * r)
                    if not ok:
                        n_oor += 1
                        continue
                    sz = F(F(sg * z) * z)
                    rr = F(voxel / sz)
                    w = F(rr * rr)
                    wq = 65536 if w >= F(65535.0) else int(w) + 1
                    g = int(Lk[y, x]) if Lk is not None else 0
                    n_ins += 1
                    if key not in tab:
                        tab[key] = [0, 0, 0, 0, 0, 0, 0]
                        h = home_slot(key, cap_log2)
                        self.home_taken += h in self._slots
                        while h in self._slots:
                            h = (h + 1) & mask
                        self._slots[h] = key
                    e = tab[key]
                    e[0] += wq
                    e[1] += wq * qs[0]
                    e[2] += wq * qs[1]
                    e[3] += wq * qs[2]
                    e[4] += wq * g
                    e[5] += 1
                    if key not in seen:
                        seen.add(key)
                        e[6] += 1
        ks = sorted(tab)
        self.key = np.array(ks, np.uint64)
        self.sums = np.array([tab[k][:5] for k in ks], np.uint64).reshape(-1, 5)
        self.cnt = np.array([tab[k][5] for k in ks], np.uint32)
        self.kf_cnt = np.array([tab[k][6] for k in ks], np.uint32)
        self._count(n_ins, n_skip, n_oor)
        return True

    def records(self, min_count=1, min_keyframes=1):
        """the extraction, ascending key order: dict(key, index, xyz, weight, count, keyframes, grey, sums)"""
        sel = (self.cnt >= min_count) & (self.kf_cnt >= min_keyframes)
        key, s, cnt, kf = self.key[sel], self.sums[sel], self.cnt[sel], self.kf_cnt[sel]
        index = key_index(key).reshape(-1, 3)
        sw = s[:, 0].astype(np.float64)
        xyz = np.zeros((len(key), 3), F)
        for a in range(3):
            f = s[:, 1 + a].astype(np.float64) / sw + 0.5
            xyz[:, a] = ((index[:, a].astype(np.float64) + f * (1.0 / 1024)) * np.float64(F(self.p["voxel"]))).astype(F)
        weight = np.minimum(s[:, 0], np.uint64(0xFFFFFFFF)).astype(np.uint32)
        grey = ((s[:, 4] + s[:, 0] // np.uint64(2)) // np.maximum(s[:, 0], np.uint64(1))).astype(np.uint8)
        return dict(key=key, index=index, xyz=xyz, weight=weight, count=cnt, keyframes=kf, grey=grey, sums=s)

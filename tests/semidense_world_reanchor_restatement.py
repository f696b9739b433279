"""Removal and re-anchoring on the world-frame voxel map (include/vo_hip.h, "Semi-dense world map: removal and re-anchoring"; DESIGN.md
§25), restated on top of tests/semidense_world_restatement.py and independent of the kernels: the points of the removal are those of
the integration (WR.points), the voxels of one removal found with np.unique and summed with np.add.at on unsigned 64-bit integers,
then subtracted modulo 2^64 from the table's sorted arrays. A vacated voxel (cnt 0) keeps its key: the arrays keep the row, `occupied`
keeps counting it, records() — min_count >= 1 — skips it. `World.remove_loop` is the same definition once more as a plain Python loop
over the points on a dict."""
import numpy as np

import semidense_world_restatement as WR

F = np.float32
RCOUNTERS = ("removals", "refused_removals", "removed", "missing", "reanchors", "vacant")
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1


class World(WR.World):
    def clear(self):
        super().clear()
        self._r = dict.fromkeys(RCOUNTERS[:5], 0)

    @property
    def rstats(self):
        return dict(self._r, vacant=int((self.cnt == 0).sum()))

    def _accept_removal(self, m):
        self.seq += 1
        H, W = m["invd"].shape
        if self.stats["occupied"] + W * H > self.stats["capacity"] // 2:  # the integration's own test; a removal never changes `occupied`
            self._r["refused_removals"] += 1
            return False
        return True

    def remove(self, m, K, T_wk, Lk=None):
        """the removal of integrate(m, K, T_wk, Lk); False: refused as a whole"""
        if not self._accept_removal(m):
            return False
        P, _, _ = WR.points(m, K, T_wk, Lk, **self.p)
        uk, inv = np.unique(P["key"], return_inverse=True)
        s = np.zeros((len(uk), 5), np.uint64)
        np.add.at(s[:, 0], inv, P["wq"])
        for a in range(3):
            np.add.at(s[:, 1 + a], inv, P["wq"] * P["q"][:, a])
        np.add.at(s[:, 4], inv, P["wq"] * P["grey"])
        c = np.bincount(inv, minlength=len(uk)).astype(np.uint32)
        pos = np.minimum(np.searchsorted(self.key, uk), max(len(self.key) - 1, 0))
        found = self.key[pos] == uk if len(self.key) else np.zeros(len(uk), bool)
        at = pos[found]
        with np.errstate(over="ignore"):
            self.sums[at] -= s[found]  # (modulo 2^64)
            self.cnt[at] -= c[found]
            self.kf_cnt[at] -= np.uint32(1)
        self._count_removal(int(c[found].sum()), int(c[~found].sum()))
        return True

    def _count_removal(self, n_removed, n_missing):
        self._r["removals"] += 1
        self._r["removed"] += n_removed
        self._r["missing"] += n_missing

    def remove_loop(self, m, K, T_wk, Lk=None):
        """the same removal point by point on a dict"""
        if not self._accept_removal(m):
            return False
        P, _, _ = WR.points(m, K, T_wk, Lk, **self.p)
        tab = {int(k): [int(v) for v in s] + [int(c), int(f)] for k, s, c, f in zip(self.key, self.sums, self.cnt, self.kf_cnt)}
        seen, n_removed, n_missing = set(), 0, 0
        for key, wq, q, g in zip(P["key"], P["wq"], P["q"], P["grey"]):
            key, wq, g = int(key), int(wq), int(g)
            e = tab.get(key)
            if e is None:
                n_missing += 1
                continue
            n_removed += 1
            e[0] = (e[0] - wq) & M64
            for a in range(3):
                e[1 + a] = (e[1 + a] - wq * int(q[a])) & M64
            e[4] = (e[4] - wq * g) & M64
            e[5] = (e[5] - 1) & M32
            if key not in seen:
                seen.add(key)
                e[6] = (e[6] - 1) & M32
        ks = sorted(tab)
        self.sums = np.array([tab[k][:5] for k in ks], np.uint64).reshape(-1, 5)
        self.cnt = np.array([tab[k][5] for k in ks], np.uint32)
        self.kf_cnt = np.array([tab[k][6] for k in ks], np.uint32)
        self._count_removal(n_removed, n_missing)
        return True

    def reanchor(self, m, K, T_old, T_new, Lk=None, loop=False):
        """False where the first 12 floats of the two poses have the same bits (nothing happens, no seq); else the removal with T_old
        and the integration with T_new, each refused or not on its own (they decide alike), and True"""
        a, b = np.asarray(T_old, F).reshape(-1)[:12], np.asarray(T_new, F).reshape(-1)[:12]
        if a.tobytes() == b.tobytes():
            return False
        (self.remove_loop if loop else self.remove)(m, K, T_old, Lk)
        (self.integrate_loop if loop else self.integrate)(m, K, T_new, Lk)
        self._r["reanchors"] += 1
        return True

    def table(self):
        """every claimed slot, vacated ones included, in ascending key order: dict(key, sums, count, keyframes)"""
        return dict(key=self.key.copy(), sums=self.sums.copy(), count=self.cnt.copy(), keyframes=self.kf_cnt.copy())

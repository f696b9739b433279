"""Python host-side mirror of the reference operator interface, on the C ABI.

Class and method names follow the reference
(core/visual_odometry/feature_tracker.h:44-104, motion_estimator.h:117-120,
feature_extractor.h descriptorDistance); argument meaning and error behaviour
match: a reference `throw std::runtime_error` surfaces as VoError, a reference
`return false` as False. numpy arrays stand in for PixelVec / PointVec /
MaskVec; matrices are row-major numpy arrays.

Everything here calls libvo_hip.so. Nothing falls back to numpy or the oracle.
"""
import collections
import ctypes as C
import os
import weakref

import numpy as np

from . import _capi
from ._capi import (FIVE_POINT_FN, BinParams, FivePointInfo, FivePointParams, FrameCounts, GnInfo, MonoCounts, MonoParams, MvoFrameInfo, MvoParams, OrbParams,
                    SbaProblem, StereoParams, SvoFrameInfo, SvoParams, VoConfig, VoError)

KLT_USE_INITIAL_FLOW = 4
GN_CORE, GN_STANDALONE = 0, 1


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _p(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


def mask_lookup(mask, x, y):
    """The ignore mask's lookup as the device does it (include/vo_hip.h, "Ignore mask"): mask[(int)(y + 0.5f)][(int)(x + 0.5f)]
    in float32, an index outside the plane (or a NaN coordinate) reads as 0. `x`, `y`: scalars or arrays. Returns bool:
    True = usable."""
    mask = np.asarray(mask)
    fx = np.asarray(x, np.float32) + np.float32(0.5)
    fy = np.asarray(y, np.float32) + np.float32(0.5)
    h, w = mask.shape
    with np.errstate(invalid="ignore"):
        ok = (fx > -1.0) & (fx < np.float32(w)) & (fy > -1.0) & (fy < np.float32(h))
    xi = np.where(ok, fx, 0).astype(np.int64)  # (astype truncates toward zero, as the C cast)
    yi = np.where(ok, fy, 0).astype(np.int64)
    return ok & (mask[yi, xi] != 0)


def _mask_arg(mask, width, height):
    """A mask as the C calls take it: a (height, width) u8 array, or a (device address, stride) pair; None clears.
    Returns (keep-alive, address, stride, on_device)."""
    if mask is None:
        return None, None, 0, 0
    if isinstance(mask, np.ndarray):
        if mask.dtype == bool:
            mask = mask.astype(np.uint8) * np.uint8(255)
        if mask.ndim != 2 or mask.shape != (height, width) or mask.dtype != np.uint8:
            raise VoError(-1, f"a mask is a {width} x {height} plane of uint8, got {mask.dtype} {mask.shape}")
        if mask.strides[1] != 1:
            mask = np.ascontiguousarray(mask)
        return mask, mask.ctypes.data, mask.strides[0], 0
    return mask, int(mask[0]), int(mask[1]), 1


def _equalize_arg(equalize):
    """from_yaml's `equalize`: None -> None; "clahe" -> {} (OpenCV's defaults); a dict with clip_limit and / or tiles -> itself"""
    if equalize is None:
        return None
    if equalize == "clahe":
        return {}
    if isinstance(equalize, dict) and set(equalize) <= {"clip_limit", "tiles"}:
        return dict(equalize)
    raise ValueError(f'equalize must be None, "clahe" or dict(clip_limit=, tiles=), not {equalize!r}')


class SemiDenseResult(collections.namedtuple("SemiDenseResult", "disparity score sigma_invd status frame_id T_wc n_accepted")):
    """The planes of a semi-dense stereo result (include/vo_hip.h, "Semi-dense stereo"): disparity, score, sigma_invd float32
    (height, width), status uint8; from a driver also the frame's id, its T_wc and the number of accepted pixels (status 1)."""
    __slots__ = ()

    @property
    def accepted(self):
        return self.status == 1


def semidense_disparity_range(bf, z_min, z_max=float("inf")):
    """(d_min, d_max) of a depth range [z_min, z_max] in metres with bf = focal length x baseline: floor(bf / z_max), ceil(bf / z_min)"""
    import math
    if not (bf > 0 and z_min > 0 and z_max >= z_min):
        raise ValueError("semidense_disparity_range: bf > 0 and 0 < z_min <= z_max")
    return (0 if math.isinf(z_max) else int(math.floor(bf / z_max))), int(math.ceil(bf / z_min))


def _semidense_params(lib, params):
    """keyword parameters -> vo_semidense_params: the C defaults, then the caller's fields; z_min / z_max (with bf) give d_min / d_max"""
    p = _capi.SemiDenseParams()
    lib.vo_semidense_default_params(C.byref(p))
    params = dict(params)
    z_min, z_max = params.pop("z_min", None), params.pop("z_max", None)
    known = {f[0] for f in _capi.SemiDenseParams._fields_}
    for k, v in params.items():
        if k not in known:
            raise ValueError(f"semi-dense: unknown parameter {k!r}; known: {sorted(known)} and z_min, z_max")
        setattr(p, k, v)
    if z_min is not None or z_max is not None:
        if "d_min" in params or "d_max" in params or "bf" not in params or z_min is None:
            raise ValueError("semi-dense: z_min (and z_max) need bf and replace d_min / d_max")
        p.d_min, p.d_max = semidense_disparity_range(float(params["bf"]), float(z_min), float("inf") if z_max is None else float(z_max))
    return p


class DenseStereoResult(collections.namedtuple("DenseStereoResult", "disparity cost sigma_invd status frame_id T_wc n_accepted")):
    """The planes of a dense stereo result (include/vo_hip.h, "Dense stereo"): disparity, sigma_invd float32 (height, width), cost
    uint16, status uint8 — disparity, sigma_invd and status as a SemiDenseResult's; from a driver also the frame's id, its T_wc;
    n_accepted: the number of accepted pixels (status 1)."""
    __slots__ = ()

    @property
    def accepted(self):
        return self.status == 1


DENSE_STEREO_DISPARITIES = (64, 128, 192, 256)


def _dense_stereo_params(lib, params):
    """keyword parameters -> vo_dense_stereo_params: the C defaults, then the caller's fields. z_min [m] (with bf, in place of d_min)
    gives d_max as the semi-dense option derives it; n_disp is then rounded up to the next allowed value and d_min = max(0, d_max + 1
    - n_disp)."""
    p = _capi.DenseStereoParams()
    lib.vo_dense_stereo_default_params(C.byref(p))
    params = dict(params)
    z_min = params.pop("z_min", None)
    known = {f[0] for f in _capi.DenseStereoParams._fields_}
    for k, v in params.items():
        if k not in known:
            raise ValueError(f"dense stereo: unknown parameter {k!r}; known: {sorted(known)} and z_min")
        setattr(p, k, v)
    if z_min is not None:
        if "d_min" in params or "bf" not in params:
            raise ValueError("dense stereo: z_min needs bf and replaces d_min")
        d_max = semidense_disparity_range(float(params["bf"]), float(z_min))[1]
        fits = [n for n in DENSE_STEREO_DISPARITIES if n >= int(p.n_disp)]
        if not fits:
            raise ValueError(f"dense stereo: n_disp={p.n_disp}: at most {DENSE_STEREO_DISPARITIES[-1]}")
        p.n_disp = fits[0]
        p.d_min = max(0, d_max + 1 - p.n_disp)
    return p


class SpeckleResult(collections.namedtuple("SpeckleResult", "disparity sigma_invd status label size n_removed n_components")):
    """What the speckle filter (include/vo_hip.h, "Speckle filter") returns: the filtered planes disparity, sigma_invd float32 (height,
    width) and status uint8 — removed pixels carry status 6 (VO_DISPARITY_SPECKLE) and zeros; None for planes in device memory, which
    are filtered in place —, with labels=True the int32 planes label and size of the components before the removal (-1 and 0 on
    invalid pixels; else None), the number of removed pixels and the number of components."""
    __slots__ = ()


DISPARITY_SPECKLE = 6  # VO_DISPARITY_SPECKLE


def _speckle_params(lib, params):
    """True or keyword parameters -> vo_speckle_params: the C defaults, then the caller's fields (max_size, max_diff)"""
    p = _capi.SpeckleParams()
    lib.vo_speckle_default_params(C.byref(p))
    known = {f[0] for f in _capi.SpeckleParams._fields_}
    for k, v in ({} if params is True else dict(params)).items():
        if k not in known:
            raise ValueError(f"speckle filter: unknown parameter {k!r}; known: {sorted(known)}")
        setattr(p, k, v)
    return p


class SemiDenseMap(collections.namedtuple("SemiDenseMap", "invd sigma n_obs tstatus score frame_id T_wc n_fused")):
    """A keyframe's semi-dense map (include/vo_hip.h, "Semi-dense temporal"): invd, sigma float32 (height, width) — both 0 where
    there is nothing yet —, n_obs, tstatus uint8; score float32 (the operator's diagnostic plane, None from a driver); from a driver
    also the keyframe's frame id, its T_wc and the number of frames fused so far."""
    __slots__ = ()


def _semidense_temporal_params(lib, params):
    """keyword parameters -> vo_semidense_temporal_params: the C defaults, then the caller's fields"""
    p = _capi.SemiDenseTemporalParams()
    lib.vo_semidense_temporal_default_params(C.byref(p))
    known = {f[0] for f in _capi.SemiDenseTemporalParams._fields_}
    for k, v in dict(params).items():
        if k not in known:
            raise ValueError(f"semi-dense temporal: unknown parameter {k!r}; known: {sorted(known)}")
        setattr(p, k, v)
    return p


class SemiDensePropagated(collections.namedtuple("SemiDensePropagated", "invd sigma n_obs tstatus origin src")):
    """A map carried over to a new keyframe (include/vo_hip.h, "Semi-dense propagation"): the map's four planes, origin uint8
    (0 nothing, 1 static only, 2 propagated only, 3 fused, 4 static replaced an inconsistent propagated value) and src int32 (the
    winning source's raster index in the old map, -1 where none)."""
    __slots__ = ()


def _semidense_propagate_params(lib, params):
    """keyword parameters -> vo_semidense_propagate_params: the C defaults, then the caller's fields"""
    p = _capi.SemiDensePropagateParams()
    lib.vo_semidense_propagate_default_params(C.byref(p))
    known = {f[0] for f in _capi.SemiDensePropagateParams._fields_}
    for k, v in dict(params).items():
        if k not in known:
            raise ValueError(f"semi-dense propagation: unknown parameter {k!r}; known: {sorted(known)}")
        setattr(p, k, v)
    return p


SEMIDENSE_RSTATUS = {0: "nothing", 1: "kept and smoothed", 2: "an entry removed", 3: "filled and kept"}


class SemiDenseRegularized(collections.namedtuple("SemiDenseRegularized", "invd sigma n_obs rstatus frame_id T_wc n_fused",
                                                  defaults=(None, None, None))):
    """A regularised semi-dense map (include/vo_hip.h, "Semi-dense regularisation"): invd, sigma float32 (height, width), n_obs uint8
    — a map like a SemiDenseMap: semiDenseAlign, semiDenseAlignPyramid and semiDenseMapPyramid take it as their map, semiDenseMapPoints
    its planes — and rstatus uint8 (the keys of SEMIDENSE_RSTATUS); from a driver also the keyframe's frame id, its T_wc and the
    number of frames fused so far."""
    __slots__ = ()


def _semidense_regularize_params(lib, params):
    """keyword parameters -> vo_semidense_regularize_params: the C defaults, then the caller's fields"""
    p = _capi.SemiDenseRegularizeParams()
    lib.vo_semidense_regularize_default_params(C.byref(p))
    known = {f[0] for f in _capi.SemiDenseRegularizeParams._fields_}
    for k, v in dict(params).items():
        if k not in known:
            raise ValueError(f"semi-dense regularisation: unknown parameter {k!r}; known: {sorted(known)}")
        setattr(p, k, v)
    return p


SEMIDENSE_WORLD_SOURCE = {"raw": 0, "regularized": 1, "dense": 2, "merged": 3}
SEMIDENSE_MERGE_ORIGIN = {0: "nothing", 1: "the map's", 2: "the result's", 3: "fused", 4: "inconsistent: the map kept", 5: "inconsistent: dropped"}


class SemiDenseMerged(collections.namedtuple("SemiDenseMerged", "invd sigma n_obs origin counts frame_id", defaults=(None,))):
    """A map merged with a disparity result (include/vo_hip.h, "Semi-dense map merge"): invd, sigma float32 (height, width), n_obs uint8
    — a map like a SemiDenseMap: semiDenseAlign, semiDenseMapRegularize, SemiDenseWorld.integrate and semiDenseMapPoints take it —,
    origin uint8 (the keys of SEMIDENSE_MERGE_ORIGIN) and counts uint64 [6], the number of pixels per origin; from a driver also the
    keyframe's frame id. None for planes in device memory."""
    __slots__ = ()


def _semidense_merge_params(lib, params):
    """keyword parameters -> vo_semidense_map_merge_params: the C defaults, then the caller's fields (chi, keep_obs)"""
    p = _capi.SemiDenseMapMergeParams()
    lib.vo_semidense_map_merge_default_params(C.byref(p))
    known = {f[0] for f in _capi.SemiDenseMapMergeParams._fields_}
    for k, v in ({} if params is True else dict(params)).items():
        if k not in known:
            raise ValueError(f"semi-dense map merge: unknown parameter {k!r}; known: {sorted(known)}")
        setattr(p, k, v)
    return p


class SemiDenseWorldPoints(collections.namedtuple("SemiDenseWorldPoints", "index xyz weight count keyframes grey sums", defaults=(None,))):
    """The voxels of a world map in ascending key order (include/vo_hip.h, "Semi-dense world map"): index int32 [n, 3], xyz float32
    [n, 3] (the weighted mean position [m]), weight uint32 [n], count uint32 [n] (points), keyframes uint32 [n] (integrations that
    reached the voxel), grey uint8 [n]; from the operator also sums uint64 [n, 5] = sw, sx, sy, sz, sg."""
    __slots__ = ()


class SemiDenseWorldFreePoints(collections.namedtuple("SemiDenseWorldFreePoints", "index xyz weight count keyframes grey sums free")):
    """What a getter given max_free returns: the fields of SemiDenseWorldPoints and, behind them, free uint32 [n], the number of
    carving rays that passed through the voxel (include/vo_hip.h, "Semi-dense world map: free-space carving")."""
    __slots__ = ()


def _semidense_world_params(lib, params):
    """keyword parameters -> vo_semidense_world_params: the C defaults, then the caller's fields"""
    p = _capi.SemiDenseWorldParams()
    lib.vo_semidense_world_default_params(C.byref(p))
    known = {f[0] for f in _capi.SemiDenseWorldParams._fields_}
    for k, v in dict(params).items():
        if k not in known:
            raise ValueError(f"semi-dense world map: unknown parameter {k!r}; known: {sorted(known)}")
        setattr(p, k, v)
    return p


def _semidense_world_carve_params(lib, params):
    """True or keyword parameters -> vo_semidense_world_carve_params: the C defaults, then the caller's fields"""
    p = _capi.SemiDenseWorldCarveParams()
    lib.vo_semidense_world_carve_default_params(C.byref(p))
    known = {f[0] for f in _capi.SemiDenseWorldCarveParams._fields_}
    for k, v in ({} if params is True else dict(params)).items():
        if k not in known:
            raise ValueError(f"world map carving: unknown parameter {k!r}; known: {sorted(known)}")
        setattr(p, k, v)
    return p


def _max_free(max_free):
    """max_free=(num, den): keep the voxels with free * den <= count * num; den 0: no filter"""
    num, den = (int(v) for v in max_free)
    return num, den


def _semidense_world_points(check, get, capacity, with_sums, with_free=False):
    """the two-call pattern of the getters: the count, then the records"""
    n = C.c_int()
    if capacity is None:
        rc = get(0, None, None, None, None, None, None, *((None,) if with_sums else ()), *((None,) if with_free else ()), C.byref(n))
        if rc < 0 and rc != -8:  # (VO_ERR_CAPACITY: the count is what was asked for)
            check(rc)
        capacity = n.value
    cap = int(capacity)
    m = max(cap, 1)
    idx, xyz = np.zeros((m, 3), np.int32), np.zeros((m, 3), np.float32)
    wt, cnt, kf, grey = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(m, np.uint8)
    sums, free = np.zeros((m, 5), np.uint64), np.zeros(m, np.uint32)
    rc = get(cap, idx.ctypes.data, xyz.ctypes.data, wt.ctypes.data, cnt.ctypes.data, kf.ctypes.data, grey.ctypes.data,
             *((sums.ctypes.data,) if with_sums else ()), *((free.ctypes.data,) if with_free else ()), C.byref(n))
    try:
        check(rc)
    except VoError as e:
        e.n = n.value
        raise
    k = min(n.value, cap)
    if with_free:
        return SemiDenseWorldFreePoints(idx[:k], xyz[:k], wt[:k], cnt[:k], kf[:k], grey[:k], sums[:k] if with_sums else None, free[:k])
    return SemiDenseWorldPoints(idx[:k], xyz[:k], wt[:k], cnt[:k], kf[:k], grey[:k], sums[:k] if with_sums else None)


class SemiDenseWorld:
    """A world-frame voxel map (include/vo_hip.h, "Semi-dense world map"; Context.semiDenseWorld makes one): a hash table of
    2^capacity_log2 slots on the context's device into which semi-dense maps are integrated with their keyframes' poses."""

    def __init__(self, ctx, **params):
        self.ctx, self.lib = ctx, ctx.lib
        self.params = _semidense_world_params(self.lib, params)
        self._h = C.c_void_p()
        ctx.check(self.lib.vo_semidense_world_create(ctx.handle, C.byref(self.params), C.byref(self._h)))
        ctx._children.add(self)

    def integrate(self, map, K, T_wk, key=None, on_device=None, key_on_device=None):
        """One integration: map a SemiDenseMap / SemiDenseRegularized / dict(invd=, sigma=, n_obs=) of arrays, K = fx, fy, cx, cy,
        T_wk (4, 4), key the keyframe's left u8 plane or None. With on_device=(width, height) the map's planes are DEVICE addresses;
        with key_on_device=stride so is key. Whether it was refused shows in stats()."""
        self._launch(self.lib.vo_semidense_world_integrate, map, K, (T_wk,), key, on_device, key_on_device)

    def remove(self, map, K, T_wk, key=None, on_device=None, key_on_device=None):
        """The exact removal of an earlier integrate(...) with the same arguments (include/vo_hip.h, "Semi-dense world map: removal
        and re-anchoring"): every sum of every voxel it reached goes back by what it added. Whether it was refused, and the points
        that found no voxel, show in reanchorStats()."""
        self._launch(self.lib.vo_semidense_world_remove, map, K, (T_wk,), key, on_device, key_on_device)

    def reanchor(self, map, K, T_old, T_new, key=None, on_device=None, key_on_device=None):
        """The map integrated earlier with T_old moves to T_new: the removal with T_old and the integration with T_new back to
        back. Returns False, with nothing launched, where the two poses' first 12 floats have the same bits; True otherwise."""
        moved = C.c_int()
        self._launch(self.lib.vo_semidense_world_reanchor, map, K, (T_old, T_new), key, on_device, key_on_device, C.byref(moved))
        return bool(moved.value)

    def carve(self, map, K, T_wk, on_device=None, **params):
        """One carve (include/vo_hip.h, "Semi-dense world map: free-space carving"): every voxel of the table that a ray of the map
        passes through on its way to the map's own surface gets 1 added to its `free` count. map, K, T_wk and on_device as
        integrate() takes them; params: margin=, chi=, z_near=. Never refused; no other field of any voxel changes."""
        p = _semidense_world_carve_params(self.lib, params)
        get = (lambda k: getattr(map, k)) if isinstance(map, tuple) else (lambda k: map[k])
        Ka = np.ascontiguousarray(K, np.float32).reshape(4)
        T = np.ascontiguousarray(T_wk, np.float32).reshape(4, 4)
        if on_device is not None:
            w, h = on_device
            planes = [C.c_void_p(get(k)) for k in ("invd", "sigma", "n_obs")]
        else:
            invd, sigma = np.ascontiguousarray(get("invd"), np.float32), np.ascontiguousarray(get("sigma"), np.float32)
            n_obs = np.ascontiguousarray(get("n_obs"), np.uint8)
            if invd.ndim != 2 or sigma.shape != invd.shape or n_obs.shape != invd.shape:
                raise ValueError("invd, sigma and n_obs are planes of one (height, width)")
            h, w = invd.shape
            planes = [invd.ctypes.data, sigma.ctypes.data, n_obs.ctypes.data]
        self.ctx.check(self.lib.vo_semidense_world_carve(self._h, *planes, int(w), int(h), int(on_device is not None), Ka.ctypes.data,
                                                         T.ctypes.data, C.byref(p)))

    def carveStats(self):
        """dict(carves, rays, short_rays, visits, hits)"""
        info = _capi.SemiDenseWorldCarveInfo()
        self.ctx.check(self.lib.vo_semidense_world_carve_stats(self._h, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in _capi.SemiDenseWorldCarveInfo._fields_}

    def reanchorStats(self):
        """dict(removals, refused_removals, removed, missing, reanchors, vacant); vacant is counted by a launch of its own"""
        info = _capi.SemiDenseWorldReanchorInfo()
        self.ctx.check(self.lib.vo_semidense_world_reanchor_stats(self._h, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in _capi.SemiDenseWorldReanchorInfo._fields_}

    def _launch(self, fn, map, K, poses, key, on_device, key_on_device, *tail):
        get = (lambda k: getattr(map, k)) if isinstance(map, tuple) else (lambda k: map[k])
        Ka = np.ascontiguousarray(K, np.float32).reshape(4)
        Ts = [np.ascontiguousarray(T, np.float32).reshape(4, 4) for T in poses]
        if on_device is not None:
            w, h = on_device
            planes = [C.c_void_p(get(k)) for k in ("invd", "sigma", "n_obs")]
        else:
            invd, sigma = np.ascontiguousarray(get("invd"), np.float32), np.ascontiguousarray(get("sigma"), np.float32)
            n_obs = np.ascontiguousarray(get("n_obs"), np.uint8)
            if invd.ndim != 2 or sigma.shape != invd.shape or n_obs.shape != invd.shape:
                raise ValueError("invd, sigma and n_obs are planes of one (height, width)")
            h, w = invd.shape
            planes = [invd.ctypes.data, sigma.ctypes.data, n_obs.ctypes.data]
        if key is None:
            pk, stride = None, 0
        elif key_on_device is not None:
            pk, stride = C.c_void_p(key), int(key_on_device)
        else:
            ka = _u8(key)
            if ka.shape != (h, w):
                raise ValueError("key is a plane of the map's (height, width)")
            pk, stride = ka.ctypes.data, ka.strides[0]
        self.ctx.check(fn(self._h, *planes, pk, stride, int(key_on_device is not None), int(w), int(h), int(on_device is not None),
                          Ka.ctypes.data, *(T.ctypes.data for T in Ts), *tail))

    def points(self, min_count=1, min_keyframes=1, capacity=None, max_free=None):
        """The voxels with count >= min_count and keyframes >= min_keyframes: a SemiDenseWorldPoints in ascending key order. With
        max_free=(num, den) the result is a SemiDenseWorldFreePoints, with `free`, and with den >= 1 only the voxels with
        free * den <= count * num are kept ((0, 0): all of them)."""
        if max_free is not None:
            num, den = _max_free(max_free)
            get = lambda cap, *a: self.lib.vo_semidense_world_points_free(self._h, int(min_count), int(min_keyframes), num, den, cap, *a)
            return _semidense_world_points(self.ctx.check, get, capacity, True, True)
        get = lambda *a: self.lib.vo_semidense_world_points(self._h, int(min_count), int(min_keyframes), *a)
        return _semidense_world_points(self.ctx.check, get, capacity, True)

    def stats(self):
        """dict(occupied, capacity, integrations, refused, inserted, skipped, out_of_range)"""
        info = _capi.SemiDenseWorldInfo()
        self.ctx.check(self.lib.vo_semidense_world_stats(self._h, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in _capi.SemiDenseWorldInfo._fields_}

    def clear(self):
        self.ctx.check(self.lib.vo_semidense_world_clear(self._h))

    def close(self):
        if self._h:
            self.lib.vo_semidense_world_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


SEMIDENSE_ALIGN_STATUS = {0: "converged", 1: "max_iters reached", 2: "too few pixels", 3: "singular system", 4: "no result"}


SEMIDENSE_ALIGN_START = {"odometry": 0, "previous": 1}
SemiDenseAlignedLevel = collections.namedtuple("SemiDenseAlignedLevel", "status iters count rms")
# with affine brightness (include/vo_hip.h, "Semi-dense alignment with affine brightness"): one more status, G and O per level
SEMIDENSE_ALIGN_AFFINE_STATUS = {**SEMIDENSE_ALIGN_STATUS, 5: "gain or offset left its range"}
SemiDenseAlignedAffineLevel = collections.namedtuple("SemiDenseAlignedAffineLevel", "status iters count rms G O")


class SemiDenseAligned(collections.namedtuple("SemiDenseAligned",
                                              "T_ck status iters count rms H b T_wc frame_id key_frame_id levels start gain offset G O",
                                              defaults=(None, None, None, None, None, None))):
    """An alignment against a semi-dense map (include/vo_hip.h, "Semi-dense alignment"): T_ck float32 (4, 4); status (the keys of
    SEMIDENSE_ALIGN_STATUS), iters; from the last evaluated system count, rms [grey levels], H float64 (6, 6) and b float64 (6,),
    in the order xi = (v, omega) of se3Exp_f. From a driver also T_wc float32 (4, 4) = the keyframe's T_wc times inverseSE3(T_ck),
    the frame's id and the keyframe's (-1 with status 4: a keyframe frame has no result). From the coarse-to-fine calls ("Semi-dense
    alignment on a map pyramid") and a driver also levels: a tuple of SemiDenseAlignedLevel(status, iters, count, rms), index =
    pyramid level, and from a driver start: "previous" where the previous frame's aligned pose was the start, else "odometry" (the
    pose the call was given: the odometry's, or the identity at the first frame after a keyframe). With affine brightness
    ("Semi-dense alignment with affine brightness") also gain, offset [grey levels] and the integers G, O they are formed from; H
    is then (8, 8) and b (8,), in the order (xi, dg, do), status may be 5 (SEMIDENSE_ALIGN_AFFINE_STATUS) and the levels are
    SemiDenseAlignedAffineLevel(status, iters, count, rms, G, O)."""
    __slots__ = ()


def _semidense_align_params(lib, params):
    """keyword parameters -> vo_semidense_align_params: the C defaults, then the caller's fields"""
    p = _capi.SemiDenseAlignParams()
    lib.vo_semidense_align_default_params(C.byref(p))
    known = {f[0] for f in _capi.SemiDenseAlignParams._fields_}
    for k, v in dict(params).items():
        if k not in known:
            raise ValueError(f"semi-dense alignment: unknown parameter {k!r}; known: {sorted(known)}")
        setattr(p, k, v)
    return p


def _semidense_align_pyr_params(lib, params):
    """keyword parameters -> vo_semidense_align_pyr_params: the C defaults, then the caller's fields (max_iters_level: up to 6 counts,
    index = level, 0 = max_iters)"""
    p = _capi.SemiDenseAlignPyrParams()
    lib.vo_semidense_align_pyr_default_params(C.byref(p))
    known = {f[0] for f in _capi.SemiDenseAlignPyrParams._fields_}
    for k, v in dict(params).items():
        if k not in known:
            raise ValueError(f"semi-dense alignment: unknown parameter {k!r}; known: {sorted(known)}")
        if k == "max_iters_level":
            v = [int(x) for x in v]
            if len(v) > 6:
                raise ValueError("semi-dense alignment: max_iters_level holds at most 6 counts")
            v = (C.c_int * 6)(*(v + [0] * (6 - len(v))))
        setattr(p, k, v)
    return p


def _semidense_affine_params(lib, affine):
    """True or dict(gain0=, offset0=) -> vo_semidense_affine_params: the C defaults, then the caller's fields"""
    p = _capi.SemiDenseAffineParams()
    lib.vo_semidense_affine_default_params(C.byref(p))
    known = {f[0] for f in _capi.SemiDenseAffineParams._fields_}
    for k, v in ({} if affine is True else dict(affine)).items():
        if k not in known:
            raise ValueError(f"semi-dense alignment, affine brightness: unknown parameter {k!r}; known: {sorted(known)}")
        setattr(p, k, v)
    return p


def _semidense_aligned(r, T_wc=None, frame_id=None, key_frame_id=None, with_levels=True):
    """vo_semidense_align_result / vo_semidense_align_pyr_result / vo_semidense_align_affine_result -> SemiDenseAligned (H as the
    full symmetric matrix)"""
    affine = isinstance(r, _capi.SemiDenseAlignAffineResult)
    nu = 8 if affine else 6
    H = np.zeros((nu, nu), np.float64)
    n = 0
    for i in range(nu):
        for j in range(i, nu):
            H[i, j] = H[j, i] = r.H[n]
            n += 1
    levels = start = None
    if affine:
        if with_levels:
            levels = tuple(SemiDenseAlignedAffineLevel(int(r.level_status[l]), int(r.level_iters[l]), int(r.level_count[l]),
                                                       float(r.level_rms[l]), int(r.level_G[l]), int(r.level_O[l])) for l in range(r.levels))
        start = None if frame_id is None else ("previous" if r.start_prev else "odometry")
        return SemiDenseAligned(np.array(r.T_ck, np.float32).reshape(4, 4), int(r.status), int(r.iters), int(r.count), float(r.rms), H,
                                np.array(r.b, np.float64), T_wc, frame_id, key_frame_id, levels, start, float(r.gain), float(r.offset),
                                int(r.G), int(r.O))
    if isinstance(r, _capi.SemiDenseAlignPyrResult):
        levels = tuple(SemiDenseAlignedLevel(int(r.level_status[l]), int(r.level_iters[l]), int(r.level_count[l]), float(r.level_rms[l]))
                       for l in range(r.levels))
        start = None if frame_id is None else ("previous" if r.start_prev else "odometry")
    return SemiDenseAligned(np.array(r.T_ck, np.float32).reshape(4, 4), int(r.status), int(r.iters), int(r.count), float(r.rms), H,
                            np.array(r.b, np.float64), T_wc, frame_id, key_frame_id, levels, start)


def _zncc_gate_arg(gate, stereo):
    """zncc_gate= / setZnccGate: None -> off; dict(thres=, win=15, pattern="centered", pairs=("temporal",)) -> the C call's
    (pairs, win, pattern, thres). pairs: names out of "temporal", "stereo" (StereoVO only)."""
    if gate is None:
        return 0, 15, 1, 0.0
    if not isinstance(gate, dict) or "thres" not in gate or not set(gate) <= {"thres", "win", "pattern", "pairs"}:
        raise ValueError(f"zncc_gate must be None or dict(thres=, win=, pattern=, pairs=), not {gate!r}")
    pattern = gate.get("pattern", "centered")
    if pattern not in Context.ZNCC_PATTERNS:
        raise ValueError(f"pattern must be one of {sorted(Context.ZNCC_PATTERNS)}, not {pattern!r}")
    pairs = gate.get("pairs", ("temporal",))
    if isinstance(pairs, str):
        pairs = (pairs,)
    bits = 0
    for p in pairs:
        if p not in Context.ZNCC_PAIRS or (p == "stereo" and not stereo):
            raise ValueError(f'pairs must be out of {"temporal, stereo" if stereo else "temporal"}, not {p!r}')
        bits |= Context.ZNCC_PAIRS[p]
    if not bits:
        raise ValueError("pairs is empty: pass None to switch the gate off")
    return bits, int(gate.get("win", 15)), Context.ZNCC_PATTERNS[pattern], float(gate["thres"])


class Context:
    """Owns one vo_ctx: a HIP stream, image-pyramid slots and point buffers."""

    SUM_ORDERS = {"tree": 0, "reference": 1}  # include/vo_hip.h: VO_SUM_ORDER_TREE / VO_SUM_ORDER_REFERENCE

    def __init__(self, device=0, max_width=1241, max_height=376, max_points=4096, n_slots=4,
                 max_level=6, sum_order="tree"):
        if sum_order not in self.SUM_ORDERS:
            raise ValueError(f"sum_order must be one of {sorted(self.SUM_ORDERS)}, not {sum_order!r}")
        self.lib = _capi.load()
        self._h = C.c_void_p()
        cfg = VoConfig(device, max_width, max_height, max_points, n_slots, max_level)
        rc = self.lib.vo_create(C.byref(cfg), C.byref(self._h))
        if rc != 0:
            msg = self.lib.vo_last_error(self._h if self._h else None).decode()
            if self._h:
                self.lib.vo_destroy(self._h)
                self._h = C.c_void_p()
            raise VoError(rc, msg)
        self.cfg = cfg
        self.sum_order = sum_order
        self._children = weakref.WeakSet()  # objects that hold device state of this context (StereoVO): closed before it
        # test / measurement switches (include/vo_hip.h: vo_debug_set). Neither the library nor this mirror reads them from
        # the environment in normal use: only a process started with VO_TEST_SWITCHES=1 (the test-suite's child processes,
        # tools/) has the variables below applied to the contexts it creates, and `debug_switches` says which are active
        # (bench.py reports them).
        self.debug_switches = {}
        if os.environ.get("VO_TEST_SWITCHES") == "1":
            for key, name in ((0, "VO_DEBUG_FAIL_JOIN"), (1, "VO_CONC_GRID"), (2, "VO_SBA_LDS_SOLVE"), (3, "VO_DEBUG_SKIP_DETECT"),
                              (5, "VO_MVO_HOST_ADVANCE"), (6, "VO_STAGED_DETECT"), (7, "VO_CANDS_IN_FRAME"),
                              (8, "VO_SBA_SPLIT")):
                v = os.environ.get(name)
                if v:
                    self.debug_set(key, int(v) if v.lstrip("-").isdigit() else 1)
                    self.debug_switches[name] = v

    DBG_FAIL_JOIN, DBG_CONC_GRID, DBG_SBA_LDS_SOLVE, DBG_SKIP_DETECT, OPT_POLL_YIELD, DBG_MVO_HOST_ADVANCE, DBG_STAGED_DETECT, DBG_CANDS_IN_FRAME = 0, 1, 2, 3, 4, 5, 6, 7
    DBG_SBA_SPLIT = 8
    DBG_SDP_STAGE = 9

    @property
    def sum_order(self):
        """Summation order of the IC and GN reductions on this context: "tree" (the default) or "reference" (the
        reference's sequential order; bit-exact against the oracle's SUM_SEQ, slower). Every operator, frame class,
        StereoVO and MonoVO of the context follows it; a change takes effect at the next call or enqueue."""
        order = self.lib.vo_get_sum_order(self._h)
        self.check(order)
        return {v: k for k, v in self.SUM_ORDERS.items()}[order]

    @sum_order.setter
    def sum_order(self, order):
        if order not in self.SUM_ORDERS:
            raise ValueError(f"sum_order must be one of {sorted(self.SUM_ORDERS)}, not {order!r}")
        self.check(self.lib.vo_set_sum_order(self._h, self.SUM_ORDERS[order]))

    def debug_set(self, key, value):
        self.check(self.lib.vo_debug_set(self._h, int(key), int(value)))

    def allocation_count(self):
        """Device + pinned allocations made for this context so far (a steady-state frame makes none)."""
        n = C.c_longlong(0)
        self.check(self.lib.vo_debug_allocation_count(self._h, C.byref(n)))
        return n.value

    def close(self):
        if getattr(self, "_h", None):
            for ch in list(getattr(self, "_children", ())):  # (a StereoVO left open by an exception must not outlive its context)
                ch.close()
            self.lib.vo_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def check(self, rc):
        if rc < 0:
            raise VoError(rc, self.lib.vo_last_error(self._h).decode())
        return rc

    @property
    def handle(self):
        return self._h

    @property
    def stream(self):
        return self.lib.vo_stream(self._h)

    def synchronize(self):
        self.check(self.lib.vo_synchronize(self._h))

    # ---- images ---------------------------------------------------------
    def set_image(self, slot, img):
        img = _u8(img)
        assert img.ndim == 2
        self.check(self.lib.vo_set_image(self._h, slot, _p(img, C.c_uint8), img.shape[1], img.shape[0],
                                         img.strides[0]))

    def slot_image_size(self, slot):
        """(width, height) of the image in `slot`, (0, 0) if it holds none (vo_slot_image_size: host state, no device work)"""
        w, h = C.c_int(), C.c_int()
        self.check(self.lib.vo_slot_image_size(self._h, slot, C.byref(w), C.byref(h)))
        return w.value, h.value

    def set_slot_mask(self, slot, mask):
        """The ignore mask of the image in `slot` (vo_set_slot_mask): a u8 (or bool) array of the image's shape, 0 = ignore; a
        (device address, stride) pair (a plane of the image's size; the stride is checked against its width); None clears it.
        Read by the per-bin candidate table, extractORBwithBinning_fast and the frame operators' stage-4 gate for that image;
        never by detect(). The slot must hold its image already; an image of another size put into the slot drops the mask."""
        w, h = self.slot_image_size(slot) if mask is not None else (0, 0)
        if mask is not None and w == 0:
            raise VoError(-1, f"slot {slot} holds no image: a mask has the dimensions of the slot's image")
        _, ptr, stride, dev = _mask_arg(mask, w, h)
        self.check(self.lib.vo_set_slot_mask(self._h, slot, ptr, stride, dev))

    # ---- image_processing::calcZNCC (include/vo_hip.h, "ZNCC") ---------------------------------------------------------------
    ZNCC_PATTERNS = {"reference": 0, "centered": 1}  # VO_ZNCC_PATTERN_*
    ZNCC_PAIRS = {"temporal": 1, "stereo": 2}         # VO_ZNCC_*

    def calcZNCC(self, slot0, slot1, pts0, pts1, win=15, pattern="reference"):
        """calcZNCC(img0, img1, pt0, pt1, win) for every pair of points: float32 [n], the ZNCC of the win x win patches of the
        images in slot0 / slot1 (level 0, as the tracker sees them). pattern "reference": the reference's own taps (the patch
        lies up-left of the point); "centered": the patch around the point. The sums follow the context's sum_order. A flat
        pair gives NaN."""
        if pattern not in self.ZNCC_PATTERNS:
            raise ValueError(f"pattern must be one of {sorted(self.ZNCC_PATTERNS)}, not {pattern!r}")
        p0 = np.ascontiguousarray(pts0, np.float32).reshape(-1, 2)
        p1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
        if len(p0) != len(p1):
            raise ValueError("pts0 and pts1 must hold the same number of points")
        out = np.zeros(len(p0), np.float32)
        self.check(self.lib.vo_zncc(self._h, int(slot0), int(slot1), p0.ctypes.data, p1.ctypes.data, len(p0), int(win),
                                    self.ZNCC_PATTERNS[pattern], out.ctypes.data))
        return out

    # ---- semi-dense stereo depth (include/vo_hip.h, "Semi-dense stereo") --------------------------------------------------------
    def semiDenseStereo(self, slot_l, slot_r, out=None, **params):
        """Semi-dense depth of the rectified pair in slot_l / slot_r (level 0; the left slot's ignore mask applies): a
        SemiDenseResult of (height, width) planes. params: the fields of vo_semidense_params (hw, hh, d_min, d_max, g_min,
        thres_best, thres_peak, peak_px, edge_px, eps_edge, eps_epi, bf), or z_min / z_max [m] with bf in place of d_min / d_max.
        out: dict(disparity=, score=, sigma_invd=, status=) of DEVICE addresses (any may be missing) — the planes are then written
        there, tightly packed, and None is returned."""
        p = _semidense_params(self.lib, params)
        if out is not None:
            ptr = [C.c_void_p(out.get(k)) if out.get(k) else None for k in ("disparity", "score", "sigma_invd", "status")]
            self.check(self.lib.vo_semidense_stereo(self._h, int(slot_l), int(slot_r), C.byref(p), *ptr, 1))
            return None
        w, h = self.slot_image_size(slot_l)
        if w <= 0:
            raise VoError(-1, f"slot {slot_l} holds no image")
        d, sc, sg = (np.zeros((h, w), np.float32) for _ in range(3))
        st = np.zeros((h, w), np.uint8)
        self.check(self.lib.vo_semidense_stereo(self._h, int(slot_l), int(slot_r), C.byref(p), d.ctypes.data, sc.ctypes.data, sg.ctypes.data,
                                                st.ctypes.data, 0))
        return SemiDenseResult(d, sc, sg, st, None, None, int((st == 1).sum()))

    # ---- dense stereo disparity (include/vo_hip.h, "Dense stereo") ---------------------------------------------------------------
    def denseStereo(self, slot_l, slot_r, out=None, speckle=None, **params):
        """Dense disparity (census + semi-global matching) of the rectified pair in slot_l / slot_r (level 0; the left slot's ignore
        mask applies): a DenseStereoResult of (height, width) planes. params: the fields of vo_dense_stereo_params (d_min, n_disp,
        paths, p1, p2, uniqueness, lr_max, eps_d, bf), or z_min [m] with bf in place of d_min. out: dict(disparity=, cost=,
        sigma_invd=, status=) of DEVICE addresses (any may be missing) — the planes are then written there, tightly packed, and
        None is returned. The planes go into semiDensePoints, semiDenseMapSeed and SemiDenseWorld.integrate as a SemiDenseResult's.
        speckle: True or dict(max_size=, max_diff=) — a convenience: disparitySpeckleFilter behind the decision, on the same stream
        (with `out`, in place on its disparity and status, which are then needed, and its sigma_invd where given)."""
        p = _dense_stereo_params(self.lib, params)
        sp = None if speckle is None or speckle is False else _speckle_params(self.lib, speckle)
        if out is not None:
            if sp is not None and not (out.get("disparity") and out.get("status")):
                raise ValueError("denseStereo: speckle needs the disparity and status planes in out")
            ptr = [C.c_void_p(out.get(k)) if out.get(k) else None for k in ("disparity", "cost", "sigma_invd", "status")]
            self.check(self.lib.vo_dense_stereo(self._h, int(slot_l), int(slot_r), C.byref(p), *ptr, 1))
            if sp is not None:
                w, h = self.slot_image_size(slot_l)
                self.check(self.lib.vo_disparity_speckle_filter(self._h, ptr[0], ptr[2], ptr[3], w, h, C.byref(sp), None, None, None, None, 1))
            return None
        w, h = self.slot_image_size(slot_l)
        if w <= 0:
            raise VoError(-1, f"slot {slot_l} holds no image")
        d, sg = (np.zeros((h, w), np.float32) for _ in range(2))
        co, st = np.zeros((h, w), np.uint16), np.zeros((h, w), np.uint8)
        self.check(self.lib.vo_dense_stereo(self._h, int(slot_l), int(slot_r), C.byref(p), d.ctypes.data, co.ctypes.data, sg.ctypes.data,
                                            st.ctypes.data, 0))
        if sp is not None:
            self.check(self.lib.vo_disparity_speckle_filter(self._h, d.ctypes.data, sg.ctypes.data, st.ctypes.data, w, h, C.byref(sp), None, None,
                                                            None, None, 0))
        return DenseStereoResult(d, co, sg, st, None, None, int((st == 1).sum()))

    # ---- speckle filter for disparity planes (include/vo_hip.h, "Speckle filter") ------------------------------------------------
    def disparitySpeckleFilter(self, disparity, sigma_invd, status, max_size=100, max_diff=1.0, labels=False, on_device=None):
        """The connected components (4-neighbours, |Δdisparity| <= max_diff) of the accepted pixels of disparity planes — a dense or
        semi-dense result's — labelled on the device, those of at most max_size pixels removed: a SpeckleResult. The planes are
        arrays (sigma_invd may be None), which are not changed: the result holds the filtered copies, and with labels=True the label
        and size planes. Or DEVICE addresses with on_device=(width, height) (sigma_invd may be None): filtered in place; labels is
        then False or dict(label=, size=) of DEVICE addresses (either may be missing), and the result holds the two counts only."""
        p = _speckle_params(self.lib, dict(max_size=max_size, max_diff=max_diff))
        nr, nc = C.c_int(), C.c_int()
        if on_device is not None:
            w, h = on_device
            lab = labels if isinstance(labels, dict) else {}
            self.check(self.lib.vo_disparity_speckle_filter(self._h, C.c_void_p(disparity), C.c_void_p(sigma_invd) if sigma_invd else None,
                                                            C.c_void_p(status), int(w), int(h), C.byref(p),
                                                            C.c_void_p(lab["label"]) if lab.get("label") else None,
                                                            C.c_void_p(lab["size"]) if lab.get("size") else None, C.byref(nr), C.byref(nc), 1))
            return SpeckleResult(None, None, None, None, None, nr.value, nc.value)
        d, st = np.array(disparity, np.float32, order="C"), np.array(status, np.uint8, order="C")
        sg = None if sigma_invd is None else np.array(sigma_invd, np.float32, order="C")
        if d.ndim != 2 or st.shape != d.shape or (sg is not None and sg.shape != d.shape):
            raise ValueError("disparity, sigma_invd and status are planes of one (height, width)")
        lab, sz = (np.zeros(d.shape, np.int32) for _ in range(2)) if labels else (None, None)
        self.check(self.lib.vo_disparity_speckle_filter(self._h, d.ctypes.data, None if sg is None else sg.ctypes.data, st.ctypes.data, d.shape[1],
                                                        d.shape[0], C.byref(p), None if lab is None else lab.ctypes.data,
                                                        None if sz is None else sz.ctypes.data, C.byref(nr), C.byref(nc), 0))
        return SpeckleResult(d, sg, st, lab, sz, nr.value, nc.value)

    def disparitySpeckleWorkspace(self, width, height):
        """bytes of device memory disparitySpeckleFilter's workspace takes for width x height planes (counters, labels, sizes)"""
        n = C.c_size_t()
        self.check(self.lib.vo_speckle_workspace(int(width), int(height), C.byref(n)))
        return n.value

    def denseStereoWorkspace(self, width, height, **params):
        """bytes of device memory denseStereo's workspace takes for a width x height pair (two census planes and the summed volume)"""
        p = _dense_stereo_params(self.lib, params)
        n = C.c_size_t()
        self.check(self.lib.vo_dense_stereo_workspace(int(width), int(height), C.byref(p), C.byref(n)))
        return n.value

    def semiDensePoints(self, disparity, sigma_invd, status, K, bf, T=None, capacity=None, on_device=None):
        """The accepted pixels of semi-dense planes in raster order: (xyz float32 [n, 3], sigma_invd float32 [n], pixel uint16
        [n, 2]) with z = bf / disparity, K = (fx, fy, cx, cy) and, with T (4 x 4), in T's target frame. The planes are arrays, or
        DEVICE addresses with on_device=(width, height). capacity: room for that many points (default: every pixel); more accepted
        pixels raise VoError(VO_ERR_CAPACITY) whose `n` attribute holds the true count."""
        if on_device is not None:
            w, h = on_device
            pd, ps, pt = C.c_void_p(disparity), C.c_void_p(sigma_invd), C.c_void_p(status)
        else:
            d = np.ascontiguousarray(disparity, np.float32)
            sg = np.ascontiguousarray(sigma_invd, np.float32)
            st = np.ascontiguousarray(status, np.uint8)
            if d.ndim != 2 or sg.shape != d.shape or st.shape != d.shape:
                raise ValueError("disparity, sigma_invd and status are planes of one (height, width)")
            h, w = d.shape
            pd, ps, pt = d.ctypes.data, sg.ctypes.data, st.ctypes.data
        cap = w * h if capacity is None else int(capacity)
        Ka = np.ascontiguousarray(K, np.float32).reshape(4)
        Ta = None if T is None else np.ascontiguousarray(T, np.float32).reshape(4, 4)
        xyz, so, px = np.zeros((max(cap, 1), 3), np.float32), np.zeros(max(cap, 1), np.float32), np.zeros((max(cap, 1), 2), np.uint16)
        n = C.c_int()
        rc = self.lib.vo_semidense_points(self._h, pd, ps, pt, w, h, int(on_device is not None), Ka.ctypes.data, float(bf),
                                          None if Ta is None else Ta.ctypes.data, cap, xyz.ctypes.data, so.ctypes.data, px.ctypes.data, C.byref(n))
        try:
            self.check(rc)
        except VoError as e:
            e.n = n.value
            raise
        return xyz[:n.value], so[:n.value], px[:n.value]

    # ---- semi-dense temporal search and fusion (include/vo_hip.h, "Semi-dense temporal") ---------------------------------------
    def semiDenseMapSeed(self, disparity, sigma_invd, status, bf, out=None, on_device=None):
        """The map of a static result: a SemiDenseMap (invd = disparity / bf, sigma = sigma_invd, n_obs = 1 where status == 1, else
        0). The planes are arrays, or DEVICE addresses with on_device=(width, height) and out=dict(invd=, sigma=, n_obs=, tstatus=)
        of DEVICE addresses (None is returned then)."""
        if on_device is not None:
            w, h = on_device
            self.check(self.lib.vo_semidense_map_seed(self._h, C.c_void_p(disparity), C.c_void_p(sigma_invd), C.c_void_p(status), int(w), int(h),
                                                      float(bf), *(C.c_void_p(out[k]) for k in ("invd", "sigma", "n_obs", "tstatus")), 1))
            return None
        d, sg, st = np.ascontiguousarray(disparity, np.float32), np.ascontiguousarray(sigma_invd, np.float32), np.ascontiguousarray(status, np.uint8)
        if d.ndim != 2 or sg.shape != d.shape or st.shape != d.shape:
            raise ValueError("disparity, sigma_invd and status are planes of one (height, width)")
        invd, sigma = np.zeros(d.shape, np.float32), np.zeros(d.shape, np.float32)
        n_obs, ts = np.zeros(d.shape, np.uint8), np.zeros(d.shape, np.uint8)
        self.check(self.lib.vo_semidense_map_seed(self._h, d.ctypes.data, sg.ctypes.data, st.ctypes.data, d.shape[1], d.shape[0], float(bf),
                                                  invd.ctypes.data, sigma.ctypes.data, n_obs.ctypes.data, ts.ctypes.data, 0))
        return SemiDenseMap(invd, sigma, n_obs, ts, None, None, None, None)

    def semiDenseMapMerge(self, map, dense, bf, chi=3.0, keep_obs=2, out=None, on_device=None):
        """A map merged per pixel with a disparity result of the same keyframe (include/vo_hip.h, "Semi-dense map merge"): the fusion
        where both have the pixel and agree within chi, the map where they disagree and it has keep_obs observations at least, the
        result's value where it is the only one. map: a SemiDenseMap / SemiDenseRegularized / dict(invd=, sigma=, n_obs=) of arrays, or
        None (the result seeded); dense: a DenseStereoResult / SemiDenseResult / dict(disparity=, sigma_invd=, status=) / the three
        planes as a tuple. Returns a SemiDenseMerged; the arguments stay. With on_device=(width, height) every plane is a DEVICE address
        (any alignment) and out=dict(invd=, sigma=, n_obs=[, origin=]) names the outputs — each may be the map's plane of the same kind —;
        the result then holds the counts only."""
        p = _semidense_merge_params(self.lib, dict(chi=chi, keep_obs=keep_obs))
        getm = None if map is None else ((lambda k: getattr(map, k)) if isinstance(map, tuple) and hasattr(map, "_fields") else (lambda k: map[k]))
        if hasattr(dense, "_fields"):
            dp = [getattr(dense, k) for k in ("disparity", "sigma_invd", "status")]
        elif isinstance(dense, dict):
            dp = [dense[k] for k in ("disparity", "sigma_invd", "status")]
        else:
            dp = list(dense)
            if len(dp) != 3:
                raise ValueError("semiDenseMapMerge: dense is a result or its planes disparity, sigma_invd, status")
        counts = np.zeros(6, np.uint64)
        if on_device is not None:
            w, h = on_device
            mp = [None] * 3 if map is None else [C.c_void_p(getm(k)) for k in ("invd", "sigma", "n_obs")]
            self.check(self.lib.vo_semidense_map_merge(self._h, *mp, *(C.c_void_p(x) for x in dp), int(w), int(h), float(bf), C.byref(p),
                                                       *(C.c_void_p(out[k]) for k in ("invd", "sigma", "n_obs")),
                                                       C.c_void_p(out["origin"]) if out.get("origin") else None, counts.ctypes.data, 1))
            return SemiDenseMerged(None, None, None, None, counts)
        d, sg, st = np.ascontiguousarray(dp[0], np.float32), np.ascontiguousarray(dp[1], np.float32), np.ascontiguousarray(dp[2], np.uint8)
        if d.ndim != 2 or sg.shape != d.shape or st.shape != d.shape:
            raise ValueError("disparity, sigma_invd and status are planes of one (height, width)")
        mp = [None] * 3
        if map is not None:
            keep = [np.ascontiguousarray(getm("invd"), np.float32), np.ascontiguousarray(getm("sigma"), np.float32),
                    np.ascontiguousarray(getm("n_obs"), np.uint8)]
            if any(x.shape != d.shape for x in keep):
                raise ValueError("the map's planes and the result's are of one (height, width)")
            mp = [x.ctypes.data for x in keep]
        invd, sigma = np.zeros(d.shape, np.float32), np.zeros(d.shape, np.float32)
        n_obs, origin = np.zeros(d.shape, np.uint8), np.zeros(d.shape, np.uint8)
        self.check(self.lib.vo_semidense_map_merge(self._h, *mp, d.ctypes.data, sg.ctypes.data, st.ctypes.data, d.shape[1], d.shape[0], float(bf),
                                                   C.byref(p), invd.ctypes.data, sigma.ctypes.data, n_obs.ctypes.data, origin.ctypes.data,
                                                   counts.ctypes.data, 0))
        return SemiDenseMerged(invd, sigma, n_obs, origin, counts)

    def semiDenseTemporal(self, key, slot_cur, K, T_ck, map, key_on_device=None, map_on_device=False, **params):
        """One temporal launch: the key plane's pixels searched in slot_cur's level-0 plane along the epipolar lines of T_ck (4 x 4,
        X_c = R X_k + t) with K = (fx, fy, cx, cy); the slot's ignore mask applies to the key pixels. key: a u8 array, or a DEVICE
        address with key_on_device=stride. map: a SemiDenseMap / dict(invd=, sigma=, n_obs=) of arrays — a new SemiDenseMap is
        returned, the arguments stay —, or with map_on_device dict(invd=, sigma=, n_obs=, tstatus=[, score=]) of DEVICE addresses,
        updated in place (None is returned). params: the fields of vo_semidense_temporal_params."""
        p = _semidense_temporal_params(self.lib, params)
        Ka = np.ascontiguousarray(K, np.float32).reshape(4)
        Ta = np.ascontiguousarray(T_ck, np.float32).reshape(4, 4)
        if key_on_device is not None:
            pk, stride = C.c_void_p(key), int(key_on_device)
        else:
            ka = _u8(key)
            pk, stride = ka.ctypes.data, ka.strides[0]
        if map_on_device:
            sc = map.get("score")
            self.check(self.lib.vo_semidense_temporal(self._h, pk, stride, int(key_on_device is not None), int(slot_cur), Ka.ctypes.data, Ta.ctypes.data,
                                                      C.byref(p), *(C.c_void_p(map[k]) for k in ("invd", "sigma", "n_obs", "tstatus")),
                                                      C.c_void_p(sc) if sc else None, 1))
            return None
        get = (lambda k: getattr(map, k)) if isinstance(map, SemiDenseMap) else (lambda k: map[k])
        invd, sigma = np.array(get("invd"), np.float32, order="C"), np.array(get("sigma"), np.float32, order="C")
        n_obs = np.array(get("n_obs"), np.uint8, order="C")
        w, h = self.slot_image_size(slot_cur)
        if invd.shape != (h, w) or sigma.shape != (h, w) or n_obs.shape != (h, w):
            raise ValueError(f"the map's planes must be ({h}, {w}) like slot {slot_cur}'s image")
        ts, score = np.zeros((h, w), np.uint8), np.zeros((h, w), np.float32)
        self.check(self.lib.vo_semidense_temporal(self._h, pk, stride, int(key_on_device is not None), int(slot_cur), Ka.ctypes.data, Ta.ctypes.data,
                                                  C.byref(p), invd.ctypes.data, sigma.ctypes.data, n_obs.ctypes.data, ts.ctypes.data, score.ctypes.data, 0))
        return SemiDenseMap(invd, sigma, n_obs, ts, score, None, None, None)

    def semiDenseAlign(self, key, slot_cur, K, T_ck, map, key_on_device=None, map_on_device=False, affine=None, **params):
        """slot_cur's level-0 plane aligned photometrically against the key plane's semi-dense map (include/vo_hip.h, "Semi-dense
        alignment"), from the start T_ck (4 x 4, X_c = R X_k + t) with K = (fx, fy, cx, cy): at most max_iters launches, one call.
        key: a u8 array, or a DEVICE address with key_on_device=stride. map: a SemiDenseMap / dict(invd=, sigma=, n_obs=) of
        arrays, or with map_on_device of DEVICE addresses; it is not modified. Returns a SemiDenseAligned. params: the fields of
        vo_semidense_align_params. affine=True or dict(gain0=, offset0=): a gain and an offset of the key's grey levels are estimated
        next to the pose ("Semi-dense alignment with affine brightness"); the result also has gain, offset, H (8, 8), b (8,)."""
        p = _semidense_align_params(self.lib, params)
        Ka = np.ascontiguousarray(K, np.float32).reshape(4)
        Ta = np.ascontiguousarray(T_ck, np.float32).reshape(4, 4)
        if key_on_device is not None:
            pk, stride = C.c_void_p(key), int(key_on_device)
        else:
            ka = _u8(key)
            pk, stride = ka.ctypes.data, ka.strides[0]
        get = (lambda k: getattr(map, k)) if isinstance(map, tuple) else (lambda k: map[k])
        res = _capi.SemiDenseAlignResult()
        if map_on_device:
            planes = [C.c_void_p(get(k)) for k in ("invd", "sigma", "n_obs")]
        else:
            invd, sigma = np.ascontiguousarray(get("invd"), np.float32), np.ascontiguousarray(get("sigma"), np.float32)
            n_obs = np.ascontiguousarray(get("n_obs"), np.uint8)
            w, h = self.slot_image_size(slot_cur)
            if invd.shape != (h, w) or sigma.shape != (h, w) or n_obs.shape != (h, w):
                raise ValueError(f"the map's planes must be ({h}, {w}) like slot {slot_cur}'s image")
            planes = [invd.ctypes.data, sigma.ctypes.data, n_obs.ctypes.data]
        if affine:
            ap, res = _semidense_affine_params(self.lib, affine), _capi.SemiDenseAlignAffineResult()
            self.check(self.lib.vo_semidense_align_affine(self._h, pk, stride, int(key_on_device is not None), int(slot_cur), Ka.ctypes.data,
                                                          Ta.ctypes.data, C.byref(p), C.byref(ap), *planes, int(bool(map_on_device)), C.byref(res)))
            return _semidense_aligned(res, with_levels=False)
        self.check(self.lib.vo_semidense_align(self._h, pk, stride, int(key_on_device is not None), int(slot_cur), Ka.ctypes.data, Ta.ctypes.data,
                                               C.byref(p), *planes, int(bool(map_on_device)), C.byref(res)))
        return _semidense_aligned(res)

    def semiDenseMapPyramid(self, map, levels, on_device=None, out=None):
        """Levels 1 .. levels - 1 of a semi-dense map (include/vo_hip.h, "Semi-dense alignment on a map pyramid"): a list of
        dict(invd=, sigma=, n_obs=) per level, [0] the map's own planes. map: a SemiDenseMap / dict(invd=, sigma=, n_obs=) of arrays,
        or with on_device=(width, height) of DEVICE addresses and out=dict(invd=, sigma=, n_obs=) of DEVICE buffers that take each
        plane kind's levels one behind the other (None is returned then)."""
        get = (lambda k: getattr(map, k)) if isinstance(map, tuple) else (lambda k: map[k])
        if on_device is not None:
            w, h = on_device
            self.check(self.lib.vo_semidense_map_pyramid(self._h, *(C.c_void_p(get(k)) for k in ("invd", "sigma", "n_obs")), int(w), int(h),
                                                         int(levels), *(C.c_void_p(out[k]) for k in ("invd", "sigma", "n_obs")), 1))
            return None
        invd, sigma = np.ascontiguousarray(get("invd"), np.float32), np.ascontiguousarray(get("sigma"), np.float32)
        n_obs = np.ascontiguousarray(get("n_obs"), np.uint8)
        if invd.ndim != 2 or sigma.shape != invd.shape or n_obs.shape != invd.shape:
            raise ValueError("invd, sigma and n_obs are planes of one (height, width)")
        h, w = invd.shape
        n = C.c_longlong()
        self.check(self.lib.vo_semidense_map_pyramid_size(w, h, int(levels), C.byref(n)))
        oi, os_, on = np.zeros(max(n.value, 1), np.float32), np.zeros(max(n.value, 1), np.float32), np.zeros(max(n.value, 1), np.uint8)
        self.check(self.lib.vo_semidense_map_pyramid(self._h, invd.ctypes.data, sigma.ctypes.data, n_obs.ctypes.data, w, h, int(levels),
                                                     oi.ctypes.data, os_.ctypes.data, on.ctypes.data, 0))
        out_levels, off = [dict(invd=invd, sigma=sigma, n_obs=n_obs)], 0
        for _ in range(1, int(levels)):
            w, h = (w + 1) // 2, (h + 1) // 2
            out_levels.append({k: a[off:off + w * h].reshape(h, w).copy() for k, a in (("invd", oi), ("sigma", os_), ("n_obs", on))})
            off += w * h
        return out_levels

    def semiDenseAlignPyramid(self, slot_key, slot_cur, K, T_ck, map, levels=4, map_on_device=False, affine=None, **params):
        """slot_cur's image aligned against slot_key's image and its semi-dense map, coarse to fine over `levels` levels of both
        slots' pyramids and of a map pyramid the call builds (include/vo_hip.h, "Semi-dense alignment on a map pyramid"), from the
        start T_ck (4 x 4, X_c = R X_k + t) with K = (fx, fy, cx, cy) of level 0. map: a SemiDenseMap / dict(invd=, sigma=, n_obs=)
        of level-0 arrays, or with map_on_device of DEVICE addresses; it is not modified. Returns a SemiDenseAligned with levels.
        params: the fields of vo_semidense_align_pyr_params. affine=True or dict(gain0=, offset0=): as semiDenseAlign's; gain and
        offset are handed from level to level with the pose, and every level reports the G, O it left."""
        p = _semidense_align_pyr_params(self.lib, dict(params, levels=int(levels)))
        Ka = np.ascontiguousarray(K, np.float32).reshape(4)
        Ta = np.ascontiguousarray(T_ck, np.float32).reshape(4, 4)
        get = (lambda k: getattr(map, k)) if isinstance(map, tuple) else (lambda k: map[k])
        res = _capi.SemiDenseAlignPyrResult()
        if map_on_device:
            planes = [C.c_void_p(get(k)) for k in ("invd", "sigma", "n_obs")]
        else:
            invd, sigma = np.ascontiguousarray(get("invd"), np.float32), np.ascontiguousarray(get("sigma"), np.float32)
            n_obs = np.ascontiguousarray(get("n_obs"), np.uint8)
            w, h = self.slot_image_size(slot_cur)
            if invd.shape != (h, w) or sigma.shape != (h, w) or n_obs.shape != (h, w):
                raise ValueError(f"the map's planes must be ({h}, {w}) like slot {slot_cur}'s image")
            planes = [invd.ctypes.data, sigma.ctypes.data, n_obs.ctypes.data]
        if affine:
            ap, res = _semidense_affine_params(self.lib, affine), _capi.SemiDenseAlignAffineResult()
            self.check(self.lib.vo_semidense_align_pyr_affine(self._h, int(slot_key), int(slot_cur), Ka.ctypes.data, Ta.ctypes.data, C.byref(p),
                                                              C.byref(ap), *planes, int(bool(map_on_device)), C.byref(res)))
            return _semidense_aligned(res)
        self.check(self.lib.vo_semidense_align_pyr(self._h, int(slot_key), int(slot_cur), Ka.ctypes.data, Ta.ctypes.data, C.byref(p), *planes,
                                                   int(bool(map_on_device)), C.byref(res)))
        return _semidense_aligned(res)

    def semiDenseMapPropagate(self, old_map, key, slot_new, static, bf, K, T_ba, out=None, key_on_device=None, **params):
        """The old keyframe's map carried over to the keyframe whose left image is in slot_new (include/vo_hip.h, "Semi-dense
        propagation"): old_map a SemiDenseMap / dict(invd=, sigma=, n_obs=), key the old keyframe's left u8 plane, static a
        SemiDenseResult / dict(disparity=, sigma_invd=, status=) of the new pair, T_ba 4 x 4 (X_b = R X_a + t); slot_new's ignore
        mask applies to the targets. Returns a SemiDensePropagated. With out=dict(invd=, sigma=, n_obs=, tstatus=[, origin=, src=])
        of DEVICE addresses every plane is a DEVICE address (key with key_on_device=stride) and None is returned. params: the
        fields of vo_semidense_propagate_params."""
        p = _semidense_propagate_params(self.lib, params)
        Ka = np.ascontiguousarray(K, np.float32).reshape(4)
        Ta = np.ascontiguousarray(T_ba, np.float32).reshape(4, 4)
        gm = (lambda k: getattr(old_map, k)) if isinstance(old_map, tuple) else (lambda k: old_map[k])
        gs = (lambda k: getattr(static, k)) if isinstance(static, tuple) else (lambda k: static[k])
        if out is not None:
            if key_on_device is None:
                raise ValueError("semiDenseMapPropagate: with out= every plane is a device address: key_on_device=stride")
            opt = lambda k: C.c_void_p(out[k]) if out.get(k) else None
            self.check(self.lib.vo_semidense_map_propagate(
                self._h, *(C.c_void_p(gm(k)) for k in ("invd", "sigma", "n_obs")), C.c_void_p(key), int(key_on_device), int(slot_new),
                *(C.c_void_p(gs(k)) for k in ("disparity", "sigma_invd", "status")), float(bf), Ka.ctypes.data, Ta.ctypes.data, C.byref(p),
                *(C.c_void_p(out[k]) for k in ("invd", "sigma", "n_obs", "tstatus")), opt("origin"), opt("src"), 1))
            return None
        w, h = self.slot_image_size(slot_new)
        ka = _u8(key)
        o_invd, o_sigma = np.ascontiguousarray(gm("invd"), np.float32), np.ascontiguousarray(gm("sigma"), np.float32)
        o_no = np.ascontiguousarray(gm("n_obs"), np.uint8)
        d, sg = np.ascontiguousarray(gs("disparity"), np.float32), np.ascontiguousarray(gs("sigma_invd"), np.float32)
        st = np.ascontiguousarray(gs("status"), np.uint8)
        for a in (ka, o_invd, o_sigma, o_no, d, sg, st):
            if a.shape != (h, w):
                raise ValueError(f"every plane must be ({h}, {w}) like slot {slot_new}'s image")
        invd, sigma = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
        n_obs, ts, origin, src = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8), np.zeros((h, w), np.int32)
        self.check(self.lib.vo_semidense_map_propagate(
            self._h, o_invd.ctypes.data, o_sigma.ctypes.data, o_no.ctypes.data, ka.ctypes.data, ka.strides[0], int(slot_new), d.ctypes.data,
            sg.ctypes.data, st.ctypes.data, float(bf), Ka.ctypes.data, Ta.ctypes.data, C.byref(p), invd.ctypes.data, sigma.ctypes.data,
            n_obs.ctypes.data, ts.ctypes.data, origin.ctypes.data, src.ctypes.data, 0))
        return SemiDensePropagated(invd, sigma, n_obs, ts, origin, src)

    def semiDenseMapRegularize(self, map, key, mask=None, out=None, key_on_device=None, **params):
        """A map regularised over each pixel's neighbourhood (include/vo_hip.h, "Semi-dense regularisation"): entries without
        consistent neighbours removed, high-gradient holes whose neighbours agree filled, every kept value smoothed. map: a
        SemiDenseMap / dict(invd=, sigma=, n_obs=) of arrays, key the keyframe's left u8 plane (an array, or a DEVICE address with
        key_on_device=stride), mask an optional u8 plane (0 = ignore). Returns a SemiDenseRegularized; the arguments stay. With
        out=dict(invd=, sigma=, n_obs=, rstatus=, size=(width, height)) of DEVICE addresses the map's planes and the mask are DEVICE
        addresses too and None is returned. params: the fields of vo_semidense_regularize_params."""
        p = _semidense_regularize_params(self.lib, params)
        get = (lambda k: getattr(map, k)) if isinstance(map, tuple) else (lambda k: map[k])
        if key_on_device is not None:
            pk, stride = C.c_void_p(key), int(key_on_device)
        else:
            ka = _u8(key)
            pk, stride = ka.ctypes.data, ka.strides[0]
        if out is not None:
            w, h = out["size"]
            self.check(self.lib.vo_semidense_map_regularize(
                self._h, *(C.c_void_p(get(k)) for k in ("invd", "sigma", "n_obs")), pk, stride, int(key_on_device is not None),
                C.c_void_p(mask) if mask else None, int(w), int(h), C.byref(p),
                *(C.c_void_p(out[k]) for k in ("invd", "sigma", "n_obs", "rstatus")), 1))
            return None
        invd, sigma = np.ascontiguousarray(get("invd"), np.float32), np.ascontiguousarray(get("sigma"), np.float32)
        n_obs = np.ascontiguousarray(get("n_obs"), np.uint8)
        ma = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if invd.ndim != 2 or sigma.shape != invd.shape or n_obs.shape != invd.shape or (ma is not None and ma.shape != invd.shape) or \
                (key_on_device is None and ka.shape != invd.shape):
            raise ValueError("invd, sigma, n_obs, key and mask are planes of one (height, width)")
        h, w = invd.shape
        o_invd, o_sigma = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
        o_no, o_rs = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
        self.check(self.lib.vo_semidense_map_regularize(
            self._h, invd.ctypes.data, sigma.ctypes.data, n_obs.ctypes.data, pk, stride, int(key_on_device is not None),
            None if ma is None else ma.ctypes.data, w, h, C.byref(p), o_invd.ctypes.data, o_sigma.ctypes.data, o_no.ctypes.data,
            o_rs.ctypes.data, 0))
        return SemiDenseRegularized(o_invd, o_sigma, o_no, o_rs)

    def semiDenseWorld(self, **params):
        """A world-frame voxel map on this context (include/vo_hip.h, "Semi-dense world map"): a SemiDenseWorld with integrate(map,
        K, T_wk, key=None), points(min_count=1, min_keyframes=1), stats(), clear() and close(). params: voxel=0.1 [m],
        capacity_log2=22 (64-byte slots), min_obs=2, z_max=40 [m]."""
        return SemiDenseWorld(self, **params)

    def semiDenseMapPoints(self, invd, sigma=None, n_obs=None, K=None, T=None, min_obs=1, capacity=None, on_device=None):
        """The map's pixels with n_obs >= min_obs in raster order: (xyz float32 [n, 3], sigma float32 [n], pixel uint16 [n, 2]) with
        z = 1 / invd; the rest as semiDensePoints. In place of the three planes a map tuple (SemiDenseMap, SemiDenseRegularized,
        SemiDensePropagated) may be given alone: semiDenseMapPoints(map, K=K, ...)."""
        if isinstance(invd, tuple) and sigma is None and n_obs is None:
            invd, sigma, n_obs = invd.invd, invd.sigma, invd.n_obs
        if sigma is None or n_obs is None or K is None:
            raise ValueError("semiDenseMapPoints: invd, sigma, n_obs (or a map tuple) and K")
        if on_device is not None:
            w, h = on_device
            pi, ps, pn = C.c_void_p(invd), C.c_void_p(sigma), C.c_void_p(n_obs)
        else:
            a, sg, no = np.ascontiguousarray(invd, np.float32), np.ascontiguousarray(sigma, np.float32), np.ascontiguousarray(n_obs, np.uint8)
            if a.ndim != 2 or sg.shape != a.shape or no.shape != a.shape:
                raise ValueError("invd, sigma and n_obs are planes of one (height, width)")
            h, w = a.shape
            pi, ps, pn = a.ctypes.data, sg.ctypes.data, no.ctypes.data
        cap = w * h if capacity is None else int(capacity)
        Ka = np.ascontiguousarray(K, np.float32).reshape(4)
        Ta = None if T is None else np.ascontiguousarray(T, np.float32).reshape(4, 4)
        xyz, so, px = np.zeros((max(cap, 1), 3), np.float32), np.zeros(max(cap, 1), np.float32), np.zeros((max(cap, 1), 2), np.uint16)
        n = C.c_int()
        rc = self.lib.vo_semidense_map_points(self._h, pi, ps, pn, w, h, int(on_device is not None), Ka.ctypes.data,
                                              None if Ta is None else Ta.ctypes.data, int(min_obs), cap, xyz.ctypes.data, so.ctypes.data,
                                              px.ctypes.data, C.byref(n))
        try:
            self.check(rc)
        except VoError as e:
            e.n = n.value
            raise
        m = min(n.value, cap)
        return xyz[:m], so[:m], px[:m]

    def set_image_device(self, slot, dev_ptr, width, height, stride):
        self.check(self.lib.vo_set_image_device(self._h, slot, C.c_void_p(dev_ptr), width, height, stride))

    def set_stereo_pair_device(self, slot_l, ptr_l, slot_r, ptr_r, width, height, stride):
        rc = self.lib.vo_set_stereo_pair_device(self._h, slot_l, ptr_l, slot_r, ptr_r, width, height, stride)
        if rc < 0:
            self.check(rc)

    # include/vo_hip.h: VO_PIX_*; what an array of each format looks like: (dtype, trailing channels)
    INPUT_FORMATS = {"mono8": 0, "rgb8": 1, "bgr8": 2, "mono16u": 3, "mono16s": 4, "f32": 5}
    _FORMAT_ARRAYS = {"mono8": (np.uint8, 0), "rgb8": (np.uint8, 3), "bgr8": (np.uint8, 3), "mono16u": (np.uint16, 0),
                      "mono16s": (np.int16, 0), "f32": (np.float32, 0)}
    _fmt = "mono8"

    def set_input_format(self, fmt):
        """Pixel format of the images the RECTIFYING entry points take (vo_set_input_format): "mono8" (default), "rgb8"
        (what the reference makes of any 3-channel image: channel 0 weighted as R), "bgr8", "mono16u", "mono16s", "f32".
        set_image_rectified, Camera.undistortImage, StereoCamera.rectifyStereoImages and StereoVO / MonoVO created with
        rectify=True then take (H, W, 3) uint8 or (H, W) uint16 / int16 / float32 arrays; everything else keeps
        requiring uint8 planes. Refused while a frame is in flight."""
        if fmt not in self.INPUT_FORMATS:
            raise ValueError(f"input format must be one of {sorted(self.INPUT_FORMATS)}, not {fmt!r}")
        self.check(self.lib.vo_set_input_format(self._h, self.INPUT_FORMATS[fmt]))
        self._fmt = fmt

    @property
    def input_format(self):
        f = C.c_int()
        self.check(self.lib.vo_get_input_format(self._h, C.byref(f)))
        return {v: k for k, v in self.INPUT_FORMATS.items()}[f.value]

    # ---- CLAHE equalisation in front of the ingestion (include/vo_hip.h: vo_set_equalize) ----------------------------------
    def set_equalize(self, mode="clahe", clip_limit=40.0, tiles=(8, 8)):
        """mode "clahe": every 8-bit grey image that enters a slot from now on — through any ingestion call of this context and
        the StereoVO / MonoVO drivers on it — is first equalised as cv::createCLAHE(clip_limit, tiles).apply would; everything
        downstream reads the equalised image. None: off (the default). tiles = (tiles_x, tiles_y), each 1..32; clip_limit >= 0
        (0: no clipping). Refused while the input format is not "mono8" and while a frame is in flight. The first call that turns
        it on allocates everything the option needs."""
        if mode not in (None, "clahe"):
            raise ValueError(f'equalisation mode must be "clahe" or None, not {mode!r}')
        tx, ty = tiles
        self.check(self.lib.vo_set_equalize(self._h, 1 if mode else 0, float(clip_limit), int(tx), int(ty)))

    @property
    def equalize(self):
        """None while equalisation is off, else {"mode": "clahe", "clip_limit": ..., "tiles": (tiles_x, tiles_y)}"""
        m, tx, ty, clip = C.c_int(), C.c_int(), C.c_int(), C.c_double()
        self.check(self.lib.vo_get_equalize(self._h, C.byref(m), C.byref(clip), C.byref(tx), C.byref(ty)))
        return {"mode": "clahe", "clip_limit": clip.value, "tiles": (tx.value, ty.value)} if m.value else None

    def equalizeImage(self, img):
        """The operator on its own (vo_equalize_image) with the current parameters: (out, luts), both numpy arrays. `img`: a
        (H, W) uint8 array (rows may be padded), or (device_ptr, stride, w, h): an image in device memory (read only; the result
        comes back to the host). out: (H, W) uint8; luts: uint8 [tiles_y, tiles_x, 256], the per-tile
        look-up tables."""
        eq = self.equalize
        if eq is None:
            raise VoError(-1, "equalizeImage: equalisation is off (set_equalize)")
        tx, ty = eq["tiles"]
        luts = np.zeros((ty, tx, 256), np.uint8)
        if isinstance(img, tuple):
            ptr, stride, w, h = (int(v) for v in img)
            if w <= 0 or h <= 0:
                raise VoError(-1, f"equalizeImage: a {w} x {h} image")
            out = np.empty((h, w), np.uint8)
            self.check(self.lib.vo_equalize_image(self._h, C.c_void_p(ptr), stride, w, h, C.c_void_p(out.ctypes.data), w,
                                                  C.c_void_p(luts.ctypes.data), 2))  # VO_EQ_DEVICE_TO_HOST
            return out, luts
        if not isinstance(img, np.ndarray) or img.dtype != np.uint8 or img.ndim != 2 or img.strides[1] != 1 or img.strides[0] < img.shape[1]:
            img = _u8(img)
            assert img.ndim == 2
        h, w = img.shape
        out = np.empty((h, w), np.uint8)
        self.check(self.lib.vo_equalize_image(self._h, C.c_void_p(img.ctypes.data), img.strides[0], w, h, C.c_void_p(out.ctypes.data), w,
                                              C.c_void_p(luts.ctypes.data), 0))
        return out, luts

    def _format_image(self, img):
        """`img` as the C-contiguous array the rectifying entry points read: for "mono8" what _u8 makes of it (as always),
        for the other formats an array of exactly the format's dtype and shape, VoError otherwise."""
        if self._fmt == "mono8":
            return _u8(img)
        dt, ch = self._FORMAT_ARRAYS[self._fmt]
        if not isinstance(img, np.ndarray) or img.dtype != dt or img.ndim != (3 if ch else 2) or (ch and img.shape[2] != ch):
            want = f"(H, W, {ch}) " if ch else "(H, W) "
            got = f"{getattr(img, 'shape', None)} {getattr(img, 'dtype', type(img).__name__)}"
            raise VoError(-1, f"input format {self._fmt!r} takes {want}{np.dtype(dt).name} arrays, not {got}")
        return np.ascontiguousarray(img)

    def set_image_rectified(self, slot, img, cam=0):
        img = self._format_image(img)
        if img.ndim != 2 and self._fmt == "mono8":
            raise VoError(-1, f"input format 'mono8' takes (H, W) uint8 planes, not an array of shape {img.shape}")
        self.check(self.lib.vo_set_image_rectified(self._h, slot, C.c_void_p(img.ctypes.data), img.shape[1], img.shape[0],
                                                   img.strides[0], cam))

    def set_image_rectified_device(self, slot, dev_ptr, width, height, stride, cam=0):
        self.check(self.lib.vo_set_image_rectified_device(self._h, slot, C.c_void_p(dev_ptr), width, height, stride,
                                                          cam))

    def set_stereo_pair_rectified_device(self, slot_l, ptr_l, slot_r, ptr_r, width, height, stride):
        self.check(self.lib.vo_set_stereo_pair_rectified_device(self._h, slot_l, C.c_void_p(ptr_l), slot_r,
                                                                C.c_void_p(ptr_r), width, height, stride))

    # ---- debug image (include/vo_hip.h: vo_draw_tracking, vo_draw_tracking_ba) -----------------------------------
    def _draw(self, fn, slot, sets):
        h, w = self.get_level(slot, 0).shape  # (the picture has the size of the slot's image)
        out = np.zeros((h, w, 3), np.uint8)
        sets = [_f32(pts).reshape(-1, 2) for pts in sets]
        args = [a for pts in sets for a in (pts.ctypes.data if len(pts) else None, len(pts))]
        self.check(fn(self._h, slot, *args, out.ctypes.data, out.strides[0]))
        return out

    def draw_tracking(self, slot, pts0, pts1, pts_new):
        """showTracking on level 0 of `slot`: (H, W, 3) uint8, lines pts0[i] -> pts1[i] and the three point sets' markers"""
        return self._draw(self.lib.vo_draw_tracking, slot, (pts0, pts1, pts_new))

    def draw_tracking_ba(self, slot, pts, pts_proj):
        """showTrackingBA on level 0 of `slot`: (H, W, 3) uint8, discs at pts and hollow squares at pts_proj"""
        return self._draw(self.lib.vo_draw_tracking_ba, slot, (pts, pts_proj))

    def set_pyramid_window_hint(self, win):
        self.check(self.lib.vo_set_pyramid_window_hint(self._h, win))

    def set_ingest_side_stream(self, on=True):
        """Image ingestion (copies + pyramid chains) on the side stream, concurrent with the frame in flight."""
        self.check(self.lib.vo_set_ingest_side_stream(self._h, int(bool(on))))

    def set_stereo_pair_host_async(self, slot_l, ptr_l, slot_r, ptr_r, width, height, stride):
        """Host images (addresses; pinned memory for a true asynchronous copy) without a host synchronisation."""
        rc = self.lib.vo_set_stereo_pair_host_async(self._h, slot_l, ptr_l, slot_r, ptr_r, width, height, stride)
        if rc < 0:
            self.check(rc)

    def frame_recoveries(self):
        """frames re-issued after a device-side join time-out (0 in normal operation)"""
        return self.lib.vo_stereo_frame_recoveries(self._h)

    def swap_slots(self, a, b):
        self.check(self.lib.vo_swap_slots(self._h, a, b))

    def pyramid_levels(self, w, h, win, max_level):
        return self.lib.vo_pyramid_levels(w, h, win, max_level)

    def get_level(self, slot, level):
        w, h = C.c_int(), C.c_int()
        buf = np.zeros((self.cfg.max_height, self.cfg.max_width), np.uint8).reshape(-1)
        self.check(self.lib.vo_get_level(self._h, slot, level, _p(buf, C.c_uint8), C.byref(w), C.byref(h)))
        return buf[: w.value * h.value].reshape(h.value, w.value).copy()

    # ---- profiling --------------------------------------------------------
    def profile_enable(self, max_records):
        self.check(self.lib.vo_profile_enable(self._h, max_records))

    def profile_set_classes(self, mask):
        self.check(self.lib.vo_profile_set_classes(self._h, C.c_uint(mask)))

    def profile_reset(self):
        self.check(self.lib.vo_profile_reset(self._h))

    def profile_get(self, cls):
        n, ms = C.c_int(), C.c_double()
        self.check(self.lib.vo_profile_get(self._h, cls, C.byref(n), C.byref(ms)))
        return n.value, ms.value


class ImageSlots:
    """What stands between the reference's cv::Mat arguments and the context's image slots (the C++ classes keep the same
    table, feature_tracker.h: slot_for): an image is identified by (buffer address, size, caller-supplied frame stamp);
    a slot that already holds it is reused — upload and pyramid once per image and frame instead of once per operator
    call (the reference rebuilds 8 pyramids per stereo frame) — otherwise the least recently used slot takes it.
    stamp None: no identity, always uploaded (the reference's behaviour)."""

    def __init__(self, ctx, slots):
        self.ctx, self.slots = ctx, list(slots)
        self.key = {s: None for s in self.slots}
        self.clock, self.used = 0, {s: 0 for s in self.slots}
        self.uploads = 0

    def get(self, img, stamp=None, avoid=()):
        img = _u8(img)
        k = None if stamp is None else (img.ctypes.data, img.shape, img.strides[0], stamp)
        self.clock += 1
        if k is not None:
            for s in self.slots:
                if self.key[s] == k:
                    self.used[s] = self.clock
                    return s
        s = min((q for q in self.slots if q not in avoid), key=lambda q: self.used[q])
        self.ctx.set_image(s, img)
        self.uploads += 1
        self.key[s], self.used[s] = k, self.clock
        return s


class FeatureTracker:
    """Mirror of the reference FeatureTracker. Images live in context slots
    (set with Context.set_image) instead of cv::Mat arguments; everything else
    keeps the reference argument order."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.lib = ctx.lib

    def calcOpticalFlowPyrLK(self, slot0, slot1, pts0, pts1=None, win=21, max_level=3, flags=0,
                             max_iter=30, eps=0.01, min_eig=1e-4):
        pts0 = _f32(pts0).reshape(-1, 2)
        n = pts0.shape[0]
        p1 = np.zeros((max(n, 1), 2), np.float32)
        if pts1 is not None:
            p1[:n] = _f32(pts1).reshape(-1, 2)
        status = np.zeros(max(n, 1), np.uint8)
        err = np.zeros(max(n, 1), np.float32)
        rc = self.ctx.check(self.lib.vo_klt_track(
            self.ctx.handle, slot0, slot1, _p(pts0), _p(p1), n, win, max_level, flags, max_iter,
            C.c_double(eps), C.c_float(min_eig), _p(status, C.c_uint8), _p(err)))
        return rc, p1[:n], status[:n], err[:n]

    def _run(self, fn, slot0, slot1, pts0, pts_track, mask_valid, win, max_level, extra):
        pts0 = _f32(pts0).reshape(-1, 2)
        n = pts0.shape[0]
        pt = np.zeros((max(n, 1), 2), np.float32)
        if pts_track is not None:
            pts_track = _f32(pts_track).reshape(-1, 2)
            if pts_track.shape[0] != n:
                raise VoError(-4, "pts_track.size() != pts0.size()")
            pt[:n] = pts_track
        m = np.ones(max(n, 1), np.uint8)
        if mask_valid is not None:
            m[:n] = np.asarray(mask_valid, np.uint8)
        self.ctx.check(fn(self.ctx.handle, slot0, slot1, _p(pts0), n, win, max_level, *extra, _p(pt),
                          _p(m, C.c_uint8)))
        return pt[:n], m[:n].astype(bool)

    def track(self, slot0, slot1, pts0, window_size, max_pyr_lvl, thres_err, mask_valid=None):
        return self._run(self.lib.vo_track, slot0, slot1, pts0, None, mask_valid, window_size,
                         max_pyr_lvl, (C.c_float(thres_err),))

    def trackBidirection(self, slot0, slot1, pts0, window_size, max_pyr_lvl, thres_err,
                         thres_bidirection, mask_valid=None):
        return self._run(self.lib.vo_track_bidirection, slot0, slot1, pts0, None, mask_valid,
                         window_size, max_pyr_lvl, (C.c_float(thres_err), C.c_float(thres_bidirection)))

    def trackBidirectionWithPrior(self, slot0, slot1, pts0, window_size, max_pyr_lvl, thres_err,
                                  thres_bidirection, pts_track, mask_valid=None):
        return self._run(self.lib.vo_track_bidirection_with_prior, slot0, slot1, pts0, pts_track,
                         mask_valid, window_size, max_pyr_lvl,
                         (C.c_float(thres_err), C.c_float(thres_bidirection)))

    def trackWithPrior(self, slot0, slot1, pts0, window_size, max_pyr_lvl, thres_err, pts_track,
                       mask_valid=None):
        return self._run(self.lib.vo_track_with_prior, slot0, slot1, pts0, pts_track, mask_valid,
                         window_size, max_pyr_lvl, (C.c_float(thres_err),))

    def calcPrior(self, pts0, Xw, Tw1, K):
        pts0, Xw = _f32(pts0).reshape(-1, 2), _f32(Xw).reshape(-1, 3)
        Tw1, K = _f32(Tw1).reshape(16), _f32(K).reshape(9)
        out = np.zeros_like(pts0)
        self.ctx.check(self.lib.vo_calc_prior(self.ctx.handle, _p(pts0), pts0.shape[0], _p(Xw),
                                              Xw.shape[0], _p(Tw1), _p(K), _p(out)))
        return out

    def trackWithScale(self, slot0, slot1, pts0, scale_est, pts_track, mask_valid=None,
                       strict_border=True):
        pts0 = _f32(pts0).reshape(-1, 2)
        n = pts0.shape[0]
        pt = _f32(pts_track).reshape(-1, 2).copy()
        if pt.shape[0] != n:
            raise VoError(-4, "pts_track.size() != pts0.size()")  # feature_tracker.cpp:282-283
        scale = _f32(scale_est)
        m = np.ones(max(n, 1), np.uint8)
        if mask_valid is not None:
            m[:n] = np.asarray(mask_valid, np.uint8)
        if n == 0:
            return pt, m[:0].astype(bool)
        self.ctx.check(self.lib.vo_track_with_scale(self.ctx.handle, slot0, slot1, _p(pts0), _p(scale),
                                                    n, _p(pt), _p(m, C.c_uint8), int(strict_border)))
        return pt, m[:n].astype(bool)


PoseInformation = collections.namedtuple("PoseInformation", "H Sigma s2 valid")
PoseCovariance = collections.namedtuple("PoseCovariance", "P Sigma_xi s2 valid n_points n_unknown_steps")


def _hat(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def se3_adjoint(T):
    """Ad(T) = [[R, [t]x R], [0, R]] for the order xi = [rho; phi] of se3Exp_f (float64)."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = A[3:, 3:] = R
    A[:3, 3:] = _hat(t) @ R
    return A


def propagate_pose_covariance(P, T10, Sigma=None):
    """One step of the chain the drivers keep on the device, in numpy float64:
    P_k = Ad(T10) P_k-1 Ad(T10)^T + Sigma, with T_wc,k = T_wc,k-1 T01 and T10 = T01^-1. P is the covariance of the right
    (body-frame) perturbation: T_wc_true ~ T_wc_est exp(-e), e ~ N(0, P). Sigma=None: the step is only carried."""
    A = se3_adjoint(T10)
    Pn = A @ np.asarray(P, np.float64).reshape(6, 6) @ A.T
    if Sigma is not None:
        Pn = Pn + np.asarray(Sigma, np.float64).reshape(6, 6)
    return 0.5 * (Pn + Pn.T)


def pose_covariance_ros(P, T_wc):
    """P in the form of nav_msgs::Odometry::pose.covariance: C = B P B^T, B = blkdiag(R_wc, R_wc) — position and world-axis
    rotation, order (x, y, z, rot x, rot y, rot z) — as 36 doubles, row-major."""
    R = np.asarray(T_wc, np.float64).reshape(4, 4)[:3, :3]
    B = np.zeros((6, 6))
    B[:3, :3] = B[3:, 3:] = R
    Cm = B @ np.asarray(P, np.float64).reshape(6, 6) @ B.T
    return (0.5 * (Cm + Cm.T)).reshape(36)


class MotionEstimator:
    """Mirror of the reference MotionEstimator's pose-only BA entry points."""

    def __init__(self, ctx, is_stereo_mode=False, T_left2right=None):
        self.ctx = ctx
        self.lib = ctx.lib
        self.is_stereo_mode_ = bool(is_stereo_mode)
        self.T_left2right_ = np.eye(4, dtype=np.float32) if T_left2right is None else _f32(T_left2right)
        self.thres_1p_, self.thres_5p_ = 10.0, 1.5  # motion_estimator.cpp:6-7
        self._five_point = None

    def poseOnlyBundleAdjustment(self, X, pts1, K, thres_reproj_outlier, R01, t01, variant=GN_CORE):
        X, pts1 = _f32(X).reshape(-1, 3), _f32(pts1).reshape(-1, 2)
        if X.shape[0] != pts1.shape[0]:  # motion_estimator.cpp:669-670
            raise VoError(-4, "In 'poseOnlyBundleAdjustment()': X.size() != pts1.size().")
        n = X.shape[0]
        K = _f32(K)
        R = _f32(R01).reshape(9).copy()
        t = _f32(t01).reshape(3).copy()
        mask = np.zeros(max(n, 1), np.uint8)
        info = GnInfo()
        rc = self.ctx.check(self.lib.vo_gn_pose_mono(
            self.ctx.handle, _p(X), _p(pts1), n, _p(K), int(thres_reproj_outlier), _p(R), _p(t),
            _p(mask, C.c_uint8), variant, C.byref(info)))
        return bool(rc), R.reshape(3, 3), t, mask[:n].astype(bool), info

    def poseOnlyBundleAdjustment_Stereo(self, X, pts_l1, pts_r1, Kl, Kr, T_lr, thres_reproj_outlier, T01):
        if not self.is_stereo_mode_:  # motion_estimator.cpp:866-867
            raise VoError(-1, "In 'poseOnlyBundleAdjustment_Stereo()', is_stereo_mode_ == false")
        X = _f32(X).reshape(-1, 3)
        pts_l1, pts_r1 = _f32(pts_l1).reshape(-1, 2), _f32(pts_r1).reshape(-1, 2)
        if X.shape[0] != pts_l1.shape[0] or X.shape[0] != pts_r1.shape[0]:  # :872-873
            raise VoError(-4, "In 'poseOnlyStereoBundleAdjustment()': size mismatch")
        n = X.shape[0]
        Kl, Kr, T_lr = _f32(Kl), _f32(Kr), _f32(T_lr).reshape(16)
        T = _f32(T01).reshape(16).copy()
        mask = np.zeros(max(n, 1), np.uint8)
        info = GnInfo()
        rc = self.ctx.check(self.lib.vo_gn_pose_stereo(
            self.ctx.handle, _p(X), _p(pts_l1), _p(pts_r1), n, _p(Kl), _p(Kr), _p(T_lr),
            C.c_float(thres_reproj_outlier), _p(T), _p(mask, C.c_uint8), C.byref(info)))
        return bool(rc), T.reshape(4, 4), mask[:n].astype(bool), info

    def poseInformation(self, X, pts1, K, R01, t01, sigma_px=0.0):
        """Covariance of the pose poseOnlyBundleAdjustment returned (vo_gn_pose_information_mono): the set it ran on and its
        R01, t01. Returns PoseInformation(H, Sigma, s2, valid); Sigma = s2 H^-1, or sigma_px^2 H^-1 with sigma_px > 0."""
        X, pts1 = _f32(X).reshape(-1, 3), _f32(pts1).reshape(-1, 2)
        if X.shape[0] != pts1.shape[0]:
            raise VoError(-4, "In 'poseInformation()': X.size() != pts1.size().")
        K, R, t = _f32(K), _f32(R01).reshape(9), _f32(t01).reshape(3)
        H, S, s2, valid = np.zeros((6, 6)), np.zeros((6, 6)), C.c_double(), C.c_int()
        self.ctx.check(self.lib.vo_gn_pose_information_mono(self.ctx.handle, _p(X), _p(pts1), X.shape[0], _p(K), _p(R), _p(t),
                                                            float(sigma_px), H.ctypes.data, S.ctypes.data, C.addressof(s2),
                                                            C.addressof(valid)))
        return PoseInformation(H, S, s2.value, bool(valid.value))

    def poseInformation_Stereo(self, X, pts_l1, pts_r1, Kl, Kr, T_lr, T01, sigma_px=0.0):
        """The stereo form (vo_gn_pose_information_stereo), for the pose poseOnlyBundleAdjustment_Stereo returned."""
        X = _f32(X).reshape(-1, 3)
        pts_l1, pts_r1 = _f32(pts_l1).reshape(-1, 2), _f32(pts_r1).reshape(-1, 2)
        if X.shape[0] != pts_l1.shape[0] or X.shape[0] != pts_r1.shape[0]:
            raise VoError(-4, "In 'poseInformation_Stereo()': size mismatch")
        Kl, Kr, T_lr, T = _f32(Kl), _f32(Kr), _f32(T_lr).reshape(16), _f32(T01).reshape(16)
        H, S, s2, valid = np.zeros((6, 6)), np.zeros((6, 6)), C.c_double(), C.c_int()
        self.ctx.check(self.lib.vo_gn_pose_information_stereo(self.ctx.handle, _p(X), _p(pts_l1), _p(pts_r1), X.shape[0], _p(Kl),
                                                              _p(Kr), _p(T_lr), _p(T), float(sigma_px), H.ctypes.data,
                                                              S.ctypes.data, C.addressof(s2), C.addressof(valid)))
        return PoseInformation(H, S, s2.value, bool(valid.value))

    def setThres1p(self, thres_1p):  # motion_estimator.cpp:655-658 (consumed by the host-side 1-point RANSAC)
        self.thres_1p_ = float(thres_1p)

    def setThres5p(self, thres_5p):  # :660-663
        self.thres_5p_ = float(thres_5p)

    def calcPose5PointsAlgorithm(self, pts0, pts1, K):
        """motion_estimator.cpp:21-123: the essential-matrix pose of pts0 -> pts1 with the RANSAC threshold thres_5p_ (pixels),
        on the device (FivePointRansac). Returns (ok, R10, t10 (unit length), mask); ok is False where the reference has no
        pose (fewer than 5 pairs, no model). X0_true of the reference is not returned."""
        fp = self._five_point
        if fp is None or fp.thres_px != np.float32(self.thres_5p_):
            if fp is not None:
                fp.close()
            fp = self._five_point = FivePointRansac(self.ctx, K, thres_px=self.thres_5p_)
        ok, R, t, mask, _ = fp.estimate(pts0, pts1, K)
        return ok, R, t, mask

    # ---- epipolar gates (motion_estimator.cpp:538-653) ----
    @staticmethod
    def fundamentalFromPose(K, R10, t10):
        """F10 = Kinv^T [t10]x R10 Kinv (motion_estimator.cpp:551-552) in float32, K = (fx, fy, cx, cy).
        3x3 products associate as Eigen's unrolled redux does: e0 + (e1 + e2)."""
        f = np.float32
        K, R, t = _f32(K).reshape(4), _f32(R10).reshape(3, 3), _f32(t10).reshape(3)
        fxi, fyi = f(1.0) / K[0], f(1.0) / K[1]
        Kinv = np.array([[fxi, 0, -K[2] * fxi], [0, fyi, -K[3] * fyi], [0, 0, 1]], f)
        S = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], f)

        def mul(A, B):
            Cm = np.zeros((3, 3), f)
            for i in range(3):
                for j in range(3):
                    Cm[i, j] = f(A[i, 0] * B[0, j]) + f(f(A[i, 1] * B[1, j]) + f(A[i, 2] * B[2, j]))
            return Cm
        return mul(mul(Kinv.T.copy(), mul(S, R)), Kinv)

    def _epi(self, fn, pts0, pts1, F10):
        pts0, pts1 = _f32(pts0).reshape(-1, 2), _f32(pts1).reshape(-1, 2)
        if pts0.shape[0] != pts1.shape[0]:  # motion_estimator.cpp:541-542, :575-576, :625-626
            raise VoError(-4, "pts0.size() != pts1.size()")
        n = pts0.shape[0]
        out = np.zeros(max(n, 1), np.float32)
        if n:
            self.ctx.check(fn(self.ctx.handle, _p(pts0), _p(pts1), n, _p(_f32(F10).reshape(9)), _p(out)))
        return out[:n]

    def calcSampsonDistance(self, pts0, pts1, F10=None, K=None, R10=None, t10=None):
        """calcSampsonDistance(pts0, pts1, F10) (:572-599) or, with K/R10/t10, the camera overload (:538-570)."""
        if F10 is None:
            F10 = self.fundamentalFromPose(K, R10, t10)
        return self._epi(self.lib.vo_sampson_distance, pts0, pts1, F10)

    def calcSymmetricEpipolarDistance(self, pts0, pts1, K, R10, t10):
        """motion_estimator.cpp:621-653"""
        return self._epi(self.lib.vo_symmetric_epipolar_distance, pts0, pts1, self.fundamentalFromPose(K, R10, t10))


class FeatureExtractor:
    """descriptorDistance (feature_extractor.cpp:338-357) for whole descriptor sets, and the
    reference-owned bucketing around cv::ORB::detect: WeightBin (feature_extractor.h:58-135) and the
    arg-max-per-bin selection of extractORBwithBinning_fast (feature_extractor.cpp:241-277)."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.lib = ctx.lib
        self.n_bins_u_ = self.n_bins_v_ = 0

    def initParams(self, n_cols, n_rows, n_bins_u, n_bins_v, THRES_FAST=15, radius=5):
        """feature_extractor.cpp:26-69 minus cv::ORB::create: WeightBin::init (feature_extractor.h:90-118)."""
        f = np.float32
        self.n_bins_u_, self.n_bins_v_ = int(n_bins_u), int(n_bins_v)
        self.u_step = int(np.floor(f(n_cols) / f(n_bins_u)))
        self.v_step = int(np.floor(f(n_rows) / f(n_bins_v)))
        self.inv_u_step_ = f(1.0) / f(self.u_step)
        self.inv_v_step_ = f(1.0) / f(self.v_step)
        self.weight = np.ones(self.n_bins_u_ * self.n_bins_v_, np.int32)
        # extractor_orb_ settings, feature_extractor.cpp:48-56
        self.orb = OrbParams()
        self.orb.nfeatures, self.orb.scale_factor, self.orb.n_levels = 10000, 1.2, 8
        self.orb.edge_threshold, self.orb.fast_threshold = 31, int(THRES_FAST)

    def detect(self, slot, max_kp=60000):
        """extractor_orb_->detect(img, fts) (feature_extractor.cpp:241) on the image in `slot`:
        (xy, response, octave)."""
        xy = np.zeros((max_kp, 2), np.float32)
        resp = np.zeros(max_kp, np.float32)
        octv = np.zeros(max_kp, np.int32)
        n = C.c_int()
        self.ctx.check(self.lib.vo_orb_detect(self.ctx.handle, slot, C.byref(self.orb), _p(xy), _p(resp),
                                              _p(octv, C.c_int32), max_kp, C.byref(n)))
        return xy[: n.value].copy(), resp[: n.value].copy(), octv[: n.value].copy()

    def extractAndComputeORB(self, slot, set=0, steer=True, max_kp=60000):
        """extractAndComputeORB (feature_extractor.cpp:321-332) on the image in `slot`: detection as detect() and the
        descriptors of all keypoints, which also stay on the device as descriptor set `set` (0 / 1) for matchSets:
        (xy, response, octave, angle [degrees], size [31 * scale, as cv::KeyPoint::size], desc [n, 32])."""
        xy = np.zeros((max_kp, 2), np.float32)
        resp, ang = np.zeros(max_kp, np.float32), np.zeros(max_kp, np.float32)
        octv = np.zeros(max_kp, np.int32)
        desc = np.zeros((max_kp, 32), np.uint8)
        n = C.c_int()
        self.ctx.check(self.lib.vo_orb_detect_and_compute(
            self.ctx.handle, slot, C.byref(self.orb), int(bool(steer)), int(set), xy.ctypes.data, resp.ctypes.data,
            octv.ctypes.data, ang.ctypes.data, desc.ctypes.data, max_kp, C.addressof(n)))
        n = n.value
        if not hasattr(self, "_set_size"):
            self._set_size = {}
        self._set_size[int(set)] = n
        octv = octv[:n].copy()
        size = np.float32(31.0) * np.power(float(self.orb.scale_factor), octv.astype(np.float64)).astype(np.float32)
        return xy[:n].copy(), resp[:n].copy(), octv, ang[:n].copy(), size, desc[:n].copy()

    def compute(self, slot, xy, octave, steer=True):
        """cv::ORB::compute restated (include/vo_hip.h) for the caller's keypoints on the image in `slot`:
        (angle, desc [n, 32], valid); a keypoint too close to its level's border or of an octave that does not exist is
        invalid: angle 0, zero descriptor."""
        xy, octave = _f32(xy).reshape(-1, 2), np.ascontiguousarray(octave, np.int32).reshape(-1)
        if xy.shape[0] != octave.shape[0]:
            raise VoError(-4, "keypoint positions / octaves differ in length")
        n = xy.shape[0]
        ang, desc, valid = np.zeros(max(n, 1), np.float32), np.zeros((max(n, 1), 32), np.uint8), np.zeros(max(n, 1), np.uint8)
        self.ctx.check(self.lib.vo_orb_compute(self.ctx.handle, slot, C.byref(self.orb), xy.ctypes.data, octave.ctypes.data, n,
                                               int(bool(steer)), ang.ctypes.data, desc.ctypes.data, valid.ctypes.data))
        return ang[:n], desc[:n], valid[:n].astype(bool)

    def getPattern(self):
        """The 512 x (x, y) sampling table of the descriptor (int8, each coordinate in [-15, 15])."""
        pat = np.zeros((512, 2), np.int8)
        self.ctx.check(self.lib.vo_orb_get_pattern(self.ctx.handle, pat.ctypes.data))
        return pat

    def setPattern(self, pattern):
        """Replaces the context's table (e.g. by OpenCV's bit_pattern_31_); VoError -1 for a coordinate outside [-15, 15]."""
        pat = np.asarray(pattern)
        if pat.size != 1024 or np.any(pat < -128) or np.any(pat > 127):
            raise VoError(-1, "a pattern is 512 x 2 int8")
        pat = np.ascontiguousarray(pat, np.int8).reshape(512, 2)
        self.ctx.check(self.lib.vo_orb_set_pattern(self.ctx.handle, pat.ctypes.data))

    def matchSets(self, a, b, th_low=50, ratio=0.6):
        """match() on two descriptor sets left on the device by extractAndComputeORB(set=a / b): no upload, any size."""
        na = getattr(self, "_set_size", {}).get(int(a))
        if na is None or int(b) not in self._set_size:
            raise VoError(-1, "matchSets: extractAndComputeORB has not filled both sets through this object")
        bi, bd, sd = np.zeros(max(na, 1), np.int32), np.zeros(max(na, 1), np.uint16), np.zeros(max(na, 1), np.uint16)
        self.ctx.check(self.lib.vo_orb_match_sets(self.ctx.handle, int(a), int(b), th_low, C.c_float(ratio), bi.ctypes.data,
                                                  bd.ctypes.data, sd.ctypes.data))
        return bi[:na], bd[:na], sd[:na]

    def extractORBwithBinning_fast(self, slot):
        """feature_extractor.cpp:211-318 with flag_nonmax_ (the branch initParams selects, :37): detection and the
        per-bin arg-max on the device; returns pts_extracted."""
        pts = np.zeros((self.weight.size + 1, 2), np.float32)
        m, nd = C.c_int(), C.c_int()
        self.ctx.check(self.lib.vo_extract_orb_with_binning(
            self.ctx.handle, slot, C.byref(self.orb), C.c_float(self.inv_u_step_), C.c_float(self.inv_v_step_),
            self.n_bins_u_, self.n_bins_v_, _p(self.weight, C.c_int32), _p(pts), C.byref(m), C.byref(nd)))
        self.n_detected = nd.value
        return pts[: m.value].copy()

    def enqueueExtract(self, slot):
        """extractORBwithBinning_fast, asynchronous: runs on the context's side stream (overlaps the frame
        operator of the same image pair); resultExtract() collects pts_extracted."""
        self.ctx.check(self.lib.vo_extract_orb_with_binning_enqueue(
            self.ctx.handle, slot, C.byref(self.orb), C.c_float(self.inv_u_step_), C.c_float(self.inv_v_step_),
            self.n_bins_u_, self.n_bins_v_, _p(np.ascontiguousarray(self.weight, np.int32), C.c_int32)))

    def resultExtract(self):
        if getattr(self, "_pts_buf", None) is None or self._pts_buf.shape[0] < self.weight.size + 1:
            self._pts_buf = np.zeros((self.weight.size + 1, 2), np.float32)
        m, nd = C.c_int(), C.c_int()
        self.ctx.check(self.lib.vo_extract_orb_with_binning_result(self.ctx.handle, _p(self._pts_buf), C.byref(m),
                                                                   C.byref(nd)))
        self.n_detected = nd.value
        return self._pts_buf[: m.value]

    def binParams(self):
        """The bins and detector settings as the closed step [10] takes them (vo_bin_params)."""
        b = BinParams()
        b.n_bins_u, b.n_bins_v, b.u_step, b.v_step = self.n_bins_u_, self.n_bins_v_, self.u_step, self.v_step
        b.inv_u_step, b.inv_v_step = float(self.inv_u_step_), float(self.inv_v_step_)
        b.orb = self.orb
        return b

    def enqueueCandidates(self, slot, table):
        """Detection + best keypoint of EVERY bin for the image in `slot`, on the side stream, into table 0 / 1
        (the image-only part of extractORBwithBinning_fast; StereoFramePipeline.enqueue_closed consumes it)."""
        if getattr(self, "_bin_params", None) is None:
            self._bin_params = self.binParams()
        rc = self.lib.vo_new_point_candidates_enqueue(self.ctx.handle, slot, self._bin_params, table)
        if rc < 0:
            self.ctx.check(rc)

    def getCandidates(self, table):
        """test hook: (xy[n_bins, 2], has[n_bins], n_detected) of a table"""
        nb = self.n_bins_u_ * self.n_bins_v_
        xy, has, nd = np.zeros((nb, 2), np.float32), np.zeros(nb, np.uint8), C.c_int()
        self.ctx.check(self.lib.vo_new_point_candidates_get(self.ctx.handle, table, _p(xy), _p(has, C.c_uint8), C.byref(nd)))
        return xy, has.astype(bool), nd.value

    def resetWeightBin(self):
        self.weight[:] = 1

    def suppressCenterBins(self):
        """feature_extractor.cpp:76-92 (host-side: a fixed pattern of a few dozen bins)"""
        nu, nv = self.n_bins_u_, self.n_bins_v_
        u_cent, v_cent = int(nu * 0.5), int(nv * 0.5)
        wu, wv, wv2 = int(np.float32(0.15) * nu), int(np.float32(0.30) * nv), int(np.float32(0.15) * nv)
        for w in range(-wv, wv + 1):
            v_idx = nu * (w + v_cent - wv2)
            for u in range(-wu, wu + 1):
                self.weight[v_idx + u + u_cent] = 0

    def updateWeightBin(self, fts):
        """feature_extractor.cpp:94-98: reset, then weight 0 for every bin that holds a tracked point"""
        pts = _f32(fts).reshape(-1, 2)
        w = np.zeros(self.weight.size, np.int32)
        self.ctx.check(self.ctx.lib.vo_weight_bin_update(self.ctx.handle, _p(pts), pts.shape[0], self.u_step,
                                                         self.v_step, self.n_bins_u_, self.n_bins_v_,
                                                         _p(w, C.c_int32)))
        self.weight = w
        return w

    def bucketKeypoints(self, kp_xy, kp_response):
        """The flag_nonmax_ branch of extractORBwithBinning_fast (feature_extractor.cpp:241-277) on the
        keypoints cv::ORB::detect returned (positions, responses, detector order)."""
        kp, r = _f32(kp_xy).reshape(-1, 2), _f32(kp_response).reshape(-1)
        if kp.shape[0] != r.shape[0]:
            raise VoError(-4, "keypoint positions / responses differ in length")
        tot = self.weight.size
        out, idx, m = np.zeros((max(tot, 1), 2), np.float32), np.zeros(max(tot, 1), np.int32), C.c_int()
        self.ctx.check(self.ctx.lib.vo_bucket_argmax(
            self.ctx.handle, _p(kp), _p(r), kp.shape[0], C.c_float(self.inv_u_step_), C.c_float(self.inv_v_step_),
            self.n_bins_u_, self.n_bins_v_, _p(np.ascontiguousarray(self.weight, np.int32), C.c_int32), _p(out),
            _p(idx, C.c_int32), C.byref(m)))
        return out[: m.value].copy(), idx[: m.value].copy()

    def descriptorDistance(self, a, b):
        a, b = _u8(a).reshape(-1, 32), _u8(b).reshape(-1, 32)
        out = np.zeros((a.shape[0], b.shape[0]), np.uint16)
        if a.shape[0] and b.shape[0]:
            self.ctx.check(self.lib.vo_orb_hamming(self.ctx.handle, _p(a, C.c_uint8), a.shape[0],
                                                   _p(b, C.c_uint8), b.shape[0], _p(out, C.c_uint16)))
        return out

    def match(self, a, b, th_low=50, ratio=0.6):
        a, b = _u8(a).reshape(-1, 32), _u8(b).reshape(-1, 32)
        na = a.shape[0]
        bi = np.zeros(max(na, 1), np.int32)
        bd = np.zeros(max(na, 1), np.uint16)
        sd = np.zeros(max(na, 1), np.uint16)
        self.ctx.check(self.lib.vo_orb_match(self.ctx.handle, _p(a, C.c_uint8), na, _p(b, C.c_uint8),
                                             b.shape[0], th_low, C.c_float(ratio), _p(bi, C.c_int32),
                                             _p(bd, C.c_uint16), _p(sd, C.c_uint16)))
        return bi[:na], bd[:na], sd[:na]


def compact_indices(ctx, mask, alive=None, tracked=None):
    """Stable compaction of mask && alive && tracked (landmark.cpp:291-332)."""
    mask = _u8(mask)
    n = mask.shape[0]
    idx = np.zeros(max(n, 1), np.int32)
    cnt = C.c_int()
    al = _u8(alive) if alive is not None else None
    tk = _u8(tracked) if tracked is not None else None
    ctx.check(ctx.lib.vo_compact_indices(
        ctx.handle, _p(mask, C.c_uint8), _p(al, C.c_uint8) if al is not None else None,
        _p(tk, C.c_uint8) if tk is not None else None, n, _p(idx, C.c_int32), C.byref(cnt)))
    return idx[: cnt.value].copy()


def se3Exp_f(ctx, xi):
    """geometry::se3Exp_f (geometry_library.cpp:386-440) and inverseSE3_f (:554-560) as the GN kernel evaluates
    them on the device; returns (T, inverse(T)), row-major 4x4."""
    xi = _f32(xi).reshape(6)
    T, Ti = np.zeros(16, np.float32), np.zeros(16, np.float32)
    ctx.check(ctx.lib.vo_se3_exp(ctx.handle, _p(xi), _p(T), _p(Ti)))
    return T.reshape(4, 4), Ti.reshape(4, 4)


def write_trajectory(path, frame_ids, T_wc):
    """The reference's trajectory dump (stereo_vo.cpp:55-115, mono_vo.cpp:64-125): one line per frame,
    `<frame id> r00 r01 r02 tx r10 r11 r12 ty r20 r21 r22 tz`, fixed notation, precision 4."""
    T = np.asarray(T_wc, np.float32).reshape(-1, 4, 4)
    ids = list(frame_ids)
    if len(ids) != T.shape[0]:
        raise ValueError("ids and poses differ in length")
    with open(path, "w") as f:  # (the reference throws "file_dir cannot be opened!" when it cannot)
        for j, Tj in zip(ids, T):
            f.write(str(int(j)) + "".join(" %.4f" % float(v) for v in Tj[:3].reshape(-1)) + "\n")


class TrackIds:
    """Landmark / Frame IDs of ONE image stream and the mask-compaction constructors with their side effect.
    The reference's counters are process-global statics (landmark.h:64, frame.h:53); here they belong to the
    context, so several streams in one process keep the IDs each would have alone."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.lib = ctx.lib

    def reset(self, next_landmark_id=0, next_frame_id=0):
        self.ctx.check(self.lib.vo_ids_reset(self.ctx.handle, int(next_landmark_id), int(next_frame_id)))

    def peek(self):
        a, b = C.c_int32(), C.c_int32()
        self.ctx.check(self.lib.vo_ids_peek(self.ctx.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def newFrames(self, n):
        """n Frame constructions (a StereoFrame is two: left, right — frame.cpp:176-180)."""
        ids = np.zeros(max(n, 1), np.int32)
        self.ctx.check(self.lib.vo_ids_new_frames(self.ctx.handle, int(n), _p(ids, C.c_int32)))
        return ids[:n]

    def newLandmarks(self, accept):
        """One Landmark construction per accepted candidate, in candidate order (stereo_vo.cpp:716-729);
        returns ids with -1 at the rejected candidates."""
        accept = _u8(accept).reshape(-1)
        n = accept.shape[0]
        ids = np.zeros(max(n, 1), np.int32)
        made = C.c_int()
        self.ctx.check(self.lib.vo_ids_new_landmarks(self.ctx.handle, _p(accept, C.c_uint8), n, _p(ids, C.c_int32),
                                                     C.byref(made)))
        return ids[:n]

    def compactTracks(self, mask, alive, tracked, ids):
        """StereoLandmarkTracking(src, mask) / LandmarkTracking(src, mask) (landmark.cpp:291-332, :194-231):
        returns (index_valid, tracked after the constructor's setUntracked() calls, ids of the survivors)."""
        mask, alive = _u8(mask).reshape(-1), _u8(alive).reshape(-1)
        tracked = _u8(tracked).reshape(-1).copy()
        ids = np.ascontiguousarray(ids, np.int32).reshape(-1)
        n = mask.shape[0]
        if not (alive.shape[0] == tracked.shape[0] == ids.shape[0] == n):
            raise VoError(-4, "lmtrack sizes differ from mask.size()")  # landmark.cpp:196-197, :293-295
        idx = np.zeros(max(n, 1), np.int32)
        ids_out = np.zeros(max(n, 1), np.int32)
        cnt = C.c_int()
        self.ctx.check(self.lib.vo_compact_tracks(
            self.ctx.handle, _p(mask, C.c_uint8), _p(alive, C.c_uint8), _p(tracked, C.c_uint8), _p(ids, C.c_int32), n,
            _p(idx, C.c_int32), _p(ids_out, C.c_int32), C.byref(cnt)))
        return idx[:cnt.value].copy(), tracked, ids_out[:cnt.value].copy()


def make_stereo_params(width, height, win, max_level, thres_err, thres_bidir, thres_poseba, Kl, Kr,
                       T_lr, thres_sampson=60.0):
    p = StereoParams()
    p.thres_sampson = thres_sampson  # feature_tracker.thres_sampson (60 in kitti_00_stereo.yaml)
    p.width, p.height, p.win, p.max_level = width, height, win, max_level
    p.thres_err, p.thres_bidirection, p.thres_poseba = thres_err, thres_bidir, thres_poseba
    T = _f32(T_lr).reshape(16)
    for i in range(4):
        p.Kl[i] = float(Kl[i])
        p.Kr[i] = float(Kr[i])
    for i in range(16):
        p.T_lr[i] = float(T[i])
    return p


class StereoFramePipeline:
    """The steady-state stereo frame (stereo_vo.cpp:483-711 operator sequence)
    chained on the device. Slots: 0 = previous left, 1 = current left,
    2 = current right; advance() rotates current-left into previous-left."""

    def __init__(self, ctx, params, strict_border=False):
        self.ctx = ctx
        self.lib = ctx.lib
        self.prm = params
        self.ctx.check(self.lib.vo_stereo_frame_set_strict_border(ctx.handle, int(strict_border)))

    def enqueue(self, pts_l0, pts_r0, Xp, dT_prior, pts_new, slots=(0, 1, 2), lm_flags=None):
        """lm_flags[i] bit 0 = lm->isTriangulated() (stereo_vo.cpp:490, :599); None = every landmark is."""
        pts_l0, pts_r0 = _f32(pts_l0).reshape(-1, 2), _f32(pts_r0).reshape(-1, 2)
        Xp = _f32(Xp).reshape(-1, 3)
        dT = _f32(dT_prior).reshape(16)
        pts_new = _f32(pts_new).reshape(-1, 2)
        self._n, self._nn = pts_l0.shape[0], pts_new.shape[0]
        self._closed = False
        fl = None
        if lm_flags is not None:
            fl = _u8(lm_flags).reshape(-1)
            if fl.shape[0] != self._n:
                raise ValueError("lm_flags.size() != pts_l0.size()")
        self.ctx.check(self.lib.vo_stereo_frame_enqueue(
            self.ctx.handle, C.byref(self.prm), slots[0], slots[1], slots[2], _p(pts_l0), _p(pts_r0),
            _p(Xp), fl.ctypes.data if fl is not None else None, self._n, _p(dT), _p(pts_new), self._nn, 0))

    def enqueue_device(self, d_pts_l0, d_pts_r0, d_Xp, n, dT_prior, d_pts_new, n_new, slots=(0, 1, 2), d_lm_flags=None):
        dT = dT_prior if (isinstance(dT_prior, np.ndarray) and dT_prior.dtype == np.float32 and dT_prior.flags.c_contiguous) \
            else _f32(dT_prior)
        self._n, self._nn = n, n_new
        self._closed = False
        rc = self.lib.vo_stereo_frame_enqueue(self.ctx.handle, self.prm, slots[0], slots[1], slots[2], d_pts_l0, d_pts_r0,
                                              d_Xp, d_lm_flags, n, dT.ctypes.data, d_pts_new, n_new, 1)
        if rc < 0:
            self.ctx.check(rc)

    def enqueue_closed(self, pts_l0, pts_r0, Xp, dT_prior, bins, table, slots=(0, 1, 2), lm_flags=None):
        """The frame with step [10] closed on the device: candidates = best keypoint of every bin of `table`
        (FeatureExtractor.enqueueCandidates on the image in slots[1]), emitted for the bins lmtrack_final leaves
        empty. `bins` = FeatureExtractor.binParams()."""
        pts_l0, pts_r0 = _f32(pts_l0).reshape(-1, 2), _f32(pts_r0).reshape(-1, 2)
        Xp = _f32(Xp).reshape(-1, 3)
        dT = _f32(dT_prior).reshape(16)
        self._n, self._nn = pts_l0.shape[0], bins.n_bins_u * bins.n_bins_v
        self._closed = True
        fl = None
        if lm_flags is not None:
            fl = _u8(lm_flags).reshape(-1)
            if fl.shape[0] != self._n:
                raise ValueError("lm_flags.size() != pts_l0.size()")
        self.ctx.check(self.lib.vo_stereo_frame_enqueue_closed(
            self.ctx.handle, self.prm, slots[0], slots[1], slots[2], pts_l0.ctypes.data, pts_r0.ctypes.data,
            Xp.ctypes.data, fl.ctypes.data if fl is not None else None, self._n, dT.ctypes.data, bins, table, 0))

    def enqueue_closed_device(self, d_pts_l0, d_pts_r0, d_Xp, n, dT_prior, bins, table, slots=(0, 1, 2), d_lm_flags=None):
        dT = dT_prior if (isinstance(dT_prior, np.ndarray) and dT_prior.dtype == np.float32 and dT_prior.flags.c_contiguous) \
            else _f32(dT_prior)
        self._n, self._nn = n, bins.n_bins_u * bins.n_bins_v
        self._closed = True
        rc = self.lib.vo_stereo_frame_enqueue_closed(self.ctx.handle, self.prm, slots[0], slots[1], slots[2], d_pts_l0,
                                                     d_pts_r0, d_Xp, d_lm_flags, n, dT.ctypes.data, bins, table, 1)
        if rc < 0:
            self.ctx.check(rc)

    def _buffers(self, n, nn):
        key = (n, nn)
        if getattr(self, "_buf_key", None) != key:
            self._buf_key = key
            self._b = dict(pts_l1=np.zeros((max(n, 1), 2), np.float32), pts_r1=np.zeros((max(n, 1), 2), np.float32),
                           stage=np.zeros(max(n, 1), np.uint8), dT=np.zeros(16, np.float32),
                           pnr=np.zeros((max(nn, 1), 2), np.float32), mnew=np.zeros(max(nn, 1), np.uint8),
                           pnl=np.zeros((max(nn, 1), 2), np.float32), n_new=C.c_int(), counts=FrameCounts(), gn=GnInfo())
            b = self._b
            self._args = (_p(b["pts_l1"]), _p(b["pts_r1"]), _p(b["stage"], C.c_uint8), _p(b["dT"]), _p(b["pnr"]),
                          _p(b["mnew"], C.c_uint8), C.byref(b["counts"]), C.byref(b["gn"]))
        return self._b

    def result(self, copy=True):
        """Waits for the enqueued frame. copy=False returns views of internal buffers that the
        next result() overwrites (what a frame-by-frame consumer needs; no allocations)."""
        n, nn = self._n, self._nn
        b = self._buffers(n, nn)
        rc = self.lib.vo_stereo_frame_result(self.ctx.handle, *self._args)
        if rc < 0:
            self.ctx.check(rc)
        closed = getattr(self, "_closed", False)
        if closed:  # the candidates are the device's: their number and left pixels come with the result
            self._closed = False
            rc = self.lib.vo_stereo_frame_new_points(self.ctx.handle, b["pnl"].ctypes.data, C.addressof(b["n_new"]))
            if rc < 0:
                self.ctx.check(rc)
            nn = b["n_new"].value
        out = dict(pts_l1=b["pts_l1"][:n], pts_r1=b["pts_r1"][:n], stage=b["stage"][:n], dT=b["dT"].reshape(4, 4),
                   pts_new_r=b["pnr"][:nn], mask_new=b["mnew"][:nn].view(bool), counts=b["counts"], gn=b["gn"])
        if closed:
            out["pts_new"] = b["pnl"][:nn]
        if copy:
            cnt, gn = FrameCounts(), GnInfo()
            C.memmove(C.byref(cnt), C.byref(b["counts"]), C.sizeof(cnt))
            C.memmove(C.byref(gn), C.byref(b["gn"]), C.sizeof(gn))
            out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}
            out["counts"], out["gn"] = cnt, gn
        return out


    def enqueue_closed_world(self, pts_l0, pts_r0, Xw, dT_prior, T_pw, T_cw_prior, bins, table, slots=(0, 1, 2), lm_flags=None):
        """enqueue_closed on the reference's own data flow (stereo_vo.cpp:475-522): Xw = landmarks in the WORLD frame,
        T_pw = previous pose inverse, T_cw_prior = inverseSE3_f(T_wp * dT_pc_prev)."""
        pts_l0, pts_r0 = _f32(pts_l0).reshape(-1, 2), _f32(pts_r0).reshape(-1, 2)
        Xw = _f32(Xw).reshape(-1, 3)
        dT, Tp, Tc = _f32(dT_prior).reshape(16), _f32(T_pw).reshape(16), _f32(T_cw_prior).reshape(16)
        self._n, self._nn = pts_l0.shape[0], bins.n_bins_u * bins.n_bins_v
        self._closed = True
        fl = None
        if lm_flags is not None:
            fl = _u8(lm_flags).reshape(-1)
            if fl.shape[0] != self._n:
                raise ValueError("lm_flags.size() != pts_l0.size()")
        self.ctx.check(self.lib.vo_stereo_frame_enqueue_closed_world(
            self.ctx.handle, self.prm, slots[0], slots[1], slots[2], pts_l0.ctypes.data, pts_r0.ctypes.data,
            Xw.ctypes.data, fl.ctypes.data if fl is not None else None, self._n, dT.ctypes.data, Tp.ctypes.data,
            Tc.ctypes.data, bins, table, 0))


def triangulateDLT(ctx, pts0, pts1, T_10, K0, K1):
    """mapping::triangulateDLT (core/util/triangulate_3d.cpp:91-130) for n pixel pairs: (X0, X1 = R10 X0 + t10)."""
    pts0, pts1 = _f32(pts0).reshape(-1, 2), _f32(pts1).reshape(-1, 2)
    if pts0.shape[0] != pts1.shape[0]:
        raise VoError(-4, "pts0.size() != pts1.size()")  # triangulate_3d.cpp:9-10
    n = pts0.shape[0]
    X0, X1 = np.zeros((max(n, 1), 3), np.float32), np.zeros((max(n, 1), 3), np.float32)
    T, K0, K1 = _f32(T_10).reshape(16), _f32(K0).reshape(4), _f32(K1).reshape(4)
    ctx.check(ctx.lib.vo_triangulate_dlt(ctx.handle, pts0.ctypes.data, pts1.ctypes.data, n, T.ctypes.data, K0.ctypes.data,
                                         K1.ctypes.data, X0.ctypes.data, X1.ctypes.data))
    return X0[:n], X1[:n]


class StereoVO:
    """StereoVO (core/visual_odometry/stereo_vo/stereo_vo.h:233-249): trackStereoImages with the track set carried on
    the device (include/vo_hip.h: vo_svo_*). The YAML loading of the reference's constructor is the caller's: the
    parameters arrive as numbers. The context needs >= 5 image slots."""

    def __init__(self, ctx, width, height, Kl, Kr, T_lr, n_bins_u, n_bins_v, thres_fastscore=15, window_size=21, max_level=6,
                 thres_error=80.0, thres_bidirection=0.5, thres_poseba_error=3.0, thres_alive_ratio=0.6, thres_rotation=15.0,
                 thres_trans=10.0, n_max_keyframes_in_window=9, strict_border=4, local_ba=True, rectify=False, thres_sampson=60.0,
                 debug_image=False, pose_covariance=False, sigma_px=0.0, mask=None, zncc_gate=None, semidense=None, dense=None):
        """debug_image=True: every tracked frame draws the reference's img_debug_ on the device (getDebugImage).
        semidense: dict of semi-dense stereo parameters (setSemiDense; "every": "keyframe" or "frame") — depth of the keyframes' pairs;
        its "temporal": True or dict(z_max=..., max_search=...) also switches setSemiDenseTemporal on, and with it
        "propagate": True or dict(min_obs=, max_diff=, chi=, sigma_add=) setSemiDensePropagate,
        "regularize": True or dict(radius=, chi=, dist_sigma=, min_support=, fill_min=, g_min=) setSemiDenseRegularize,
        "world": True or dict(voxel=, capacity_log2=, min_obs=, z_max=, source="raw" | "regularized") setSemiDenseWorld; with
        reanchor=True or reanchor=dict(min_move=0.0) in it, the maps follow the local BA (setSemiDenseWorldReanchor); with carve=True
        or carve=dict(margin=, chi=, z_near=) in it, every integration is followed by a free-space carve (setSemiDenseWorldCarve),
        "align": True or dict(min_obs=, huber=, max_iters=, eps=, min_pixels=) setSemiDenseAlign; with levels=, max_iters_level= or
        start="odometry" | "previous" in it, coarse to fine on a map pyramid (setSemiDenseAlignPyramid); with affine=True or
        affine=dict(gain0=, offset0=) in it, gain and offset are estimated next to the pose (setSemiDenseAlignAffine).
        dense: dict of dense stereo parameters (setDenseStereo; "every": "keyframe" or "frame"), e.g. dict(bf=, z_min=3.0,
        n_disp=128) — a disparity for every pixel of the keyframes' pairs; independent of semidense. Its "speckle": True or
        dict(max_size=, max_diff=) switches setDenseSpeckle on: the small islands of each result removed.
        mask: the ignore mask every pair carries from the first one on (setMask).
        zncc_gate: dict(thres=, win=15, pattern="centered", pairs=("temporal",)) — the appearance gate (setZnccGate).
        pose_covariance=True: every frame chains the covariance of its pose on the device (getPoseCovariance); sigma_px > 0
        scales by that pixel noise instead of the a-posteriori variance.
        rectify=True is system_flags_.flagDoUndistortion: the context's stereo rectification maps (StereoCamera.
        initStereoCameraToRectify on the same context) are applied to every incoming pair; Kl / Kr / T_lr are then the
        rectified camera and extrinsics (getRectifiedCamera / getRectifiedStereoPoseLeft2Right)."""
        self.ctx, self.lib = ctx, ctx.lib
        fe = FeatureExtractor(ctx)
        fe.initParams(width, height, n_bins_u, n_bins_v, THRES_FAST=thres_fastscore)
        p = SvoParams()
        p.frame = make_stereo_params(width, height, window_size, max_level, thres_error, thres_bidirection, thres_poseba_error,
                                     Kl, Kr, T_lr, thres_sampson)
        p.bins = fe.binParams()
        p.kf_overlap_ratio, p.kf_rotation_deg, p.kf_translation = thres_alive_ratio, thres_rotation, thres_trans
        p.kf_window, p.strict_border, p.local_ba = n_max_keyframes_in_window, int(strict_border), int(bool(local_ba))
        p.rectify = int(bool(rectify))
        self.prm, self.width, self.height = p, width, height
        self._h = C.c_void_p()
        ctx.check(self.lib.vo_svo_create(ctx.handle, C.byref(p), C.byref(self._h)))
        ctx._children.add(self)
        if debug_image:
            ctx.check(self.lib.vo_svo_set_debug_image(self._h, 1))
        if pose_covariance:
            ctx.check(self.lib.vo_svo_set_pose_covariance(self._h, 1, float(sigma_px)))
        if mask is not None:
            self.setMask(mask)
        if zncc_gate is not None:
            self.setZnccGate(zncc_gate)
        if semidense is not None:
            sd = dict(semidense)
            temporal, propagate, align = sd.pop("temporal", None), sd.pop("propagate", None), sd.pop("align", None)
            regularize, world = sd.pop("regularize", None), sd.pop("world", None)
            if world and not temporal:
                raise ValueError('semidense: "world" needs "temporal"')
            if propagate and not temporal:
                raise ValueError('semidense: "propagate" needs "temporal"')
            if regularize and not temporal:
                raise ValueError('semidense: "regularize" needs "temporal"')
            if align and not temporal:
                raise ValueError('semidense: "align" needs "temporal"')
            self.setSemiDense(sd, every=sd.pop("every", "keyframe"))
            if temporal:
                self.setSemiDenseTemporal({} if temporal is True else temporal)
            if propagate:
                self.setSemiDensePropagate({} if propagate is True else propagate)
            if align:
                self.setSemiDenseAlign({} if align is True else align)
            if regularize:
                self.setSemiDenseRegularize({} if regularize is True else regularize)
            world_late = bool(world) and world is not True and dict(world).get("source") in ("dense", "merged")
            if world_late and dense is None:
                raise ValueError('semidense: world source "dense" / "merged" needs dense=')
            if world and not world_late:
                self.setSemiDenseWorld({} if world is True else world)
        else:
            world, world_late = None, False
        if dense is not None:
            ds = dict(dense)
            speckle = ds.pop("speckle", None)
            self.setDenseStereo(ds, every=ds.pop("every", "keyframe"))
            if speckle is not None and speckle is not False:
                self.setDenseSpeckle(speckle)
        if world_late:  # (the sources that read the dense result need that option on first)
            self.setSemiDenseWorld(world)
        self._info = SvoFrameInfo()
        self.stats_frame = []  # AlgorithmStatistics::FrameStatistics::Twc per frame (stereo_vo.cpp:979-980)

    @classmethod
    def from_yaml(cls, path, device=0, max_points=None, input_format="mono8", mask=None, mask_erode=0, equalize=None, zncc_gate=None,
                  semidense=None, dense=None, **overrides):
        """StereoVO(mode = "rosbag", directory_intrinsic = path) of the reference (stereo_vo.cpp:15-57, :118-280): the
        object configured by one of its config/stereo/*.yaml files. The context is created here (sized by the file) and
        closed with the object. With flagDoUndistortion the pairs go through the rectification maps and the loop runs on
        the rectified camera (:414-427); without, on the raw cameras and T_lr of the file. `overrides`: keyword
        arguments of the constructor that the file does not know (strict_border, local_ba). `max_points`: capacity of a
        track set (default 2 * bins + 1024; the reference has no such bound — several survivors may share a bin while
        every empty bin adds a landmark — so a caller that sees VO_ERR_CAPACITY raises it). `input_format`: the pairs'
        pixel format (Context.set_input_format); anything but "mono8" needs flagDoUndistortion in the file.
        `mask`: an ignore mask (setMask), or "rectified": the left camera's validity mask (StereoCamera.validityMask(mask_erode):
        what cv::remap fills with 0 is not looked at), which needs flagDoUndistortion in the file.
        `equalize`: None, "clahe" (OpenCV's defaults) or dict(clip_limit=, tiles=): Context.set_equalize on the new context.
        `zncc_gate`: the constructor's (setZnccGate). `semidense`: the constructor's (setSemiDense); without "bf" the (rectified)
        camera's focal length x baseline is filled in. `dense`: the constructor's (setDenseStereo), bf filled in likewise."""
        from . import config as _config
        cfg = _config.load_stereo_config(path)
        eq = _equalize_arg(equalize)
        if isinstance(mask, str) and (mask != "rectified" or not cfg["flagDoUndistortion"]):
            raise ValueError('mask="rectified" is the only named mask, and it needs flagDoUndistortion in the file')
        cl, cr = cfg["camera"]["left"], cfg["camera"]["right"]
        W, H = cl["width"], cl["height"]
        fe, ft, me, ku = cfg["feature_extractor"], cfg["feature_tracker"], cfg["motion_estimator"], cfg["keyframe_update"]
        cap = int(max_points) if max_points else 2 * fe["n_bins_u"] * fe["n_bins_v"] + 1024
        ctx = Context(device=device, max_width=W, max_height=H, max_points=cap, n_slots=5,
                      max_level=ft["max_level"])
        try:
            if input_format != "mono8":
                ctx.set_input_format(input_format)
            if eq is not None:
                ctx.set_equalize("clahe", **eq)
            Kl, Kr, T_lr, rectify = cl["K"], cr["K"], cfg["T_lr"], False
            if cfg["flagDoUndistortion"]:
                cam = StereoCamera(ctx)
                cam.initParams(W, H, cl["K"], cl["D"], cr["K"], cr["D"])
                cam.setStereoPoseLeft2Right(cfg["T_lr"])
                cam.initStereoCameraToRectify()
                Kl = Kr = cam.getRectifiedCamera()
                T_lr, rectify = cam.getRectifiedStereoPoseLeft2Right(), True
                if isinstance(mask, str):
                    mask = cam.validityMask(mask_erode)
            if semidense is not None:
                semidense = dict(semidense)
                semidense.setdefault("bf", float(np.asarray(Kl, np.float64).reshape(-1)[0] * np.linalg.norm(np.asarray(T_lr, np.float64).reshape(4, 4)[:3, 3])))
                overrides = dict(overrides, semidense=semidense)
            if dense is not None:
                dense = dict(dense)
                dense.setdefault("bf", float(np.asarray(Kl, np.float64).reshape(-1)[0] * np.linalg.norm(np.asarray(T_lr, np.float64).reshape(4, 4)[:3, 3])))
                overrides = dict(overrides, dense=dense)
            obj = cls(ctx, W, H, Kl, Kr, T_lr, fe["n_bins_u"], fe["n_bins_v"], thres_fastscore=fe["thres_fastscore"],
                      window_size=ft["window_size"], max_level=ft["max_level"], thres_error=ft["thres_error"],
                      thres_sampson=ft["thres_sampson"],
                      thres_bidirection=ft["thres_bidirection"], thres_poseba_error=me["thres_poseba_error"],
                      thres_alive_ratio=ku["thres_alive_ratio"], thres_rotation=ku["thres_rotation"], thres_trans=ku["thres_trans"],
                      n_max_keyframes_in_window=ku["n_max_keyframes_in_window"], rectify=rectify, mask=mask, zncc_gate=zncc_gate, **overrides)
        except Exception:
            ctx.close()
            raise
        obj._own_ctx, obj.config = ctx, cfg
        return obj

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vo_svo_destroy(self._h)
            self._h = C.c_void_p()
        own = getattr(self, "_own_ctx", None)
        if own is not None:
            self._own_ctx = None
            own.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setMask(self, mask):
        """The ignore mask (include/vo_hip.h, "Ignore mask") of every pair handed over FROM NOW ON: a (height, width) u8 / bool
        array, 0 = ignore, or a (device address, stride) pair — a segmentation network's output stays on the device; None: no
        mask. Legal between any two of trackStereoImages / enqueue / prefetch / result; a pair already handed over (a
        prefetched one included) keeps the mask it came with. The library copies: the array is free on return."""
        _, ptr, stride, dev = _mask_arg(mask, self.width, self.height)
        self.ctx.check(self._set_mask_fn()(self._h, ptr, stride, dev))

    def _set_mask_fn(self):
        return self.lib.vo_svo_set_mask

    _zncc_pairs = 0

    def setZnccGate(self, gate):
        """The ZNCC appearance gate (include/vo_hip.h, "ZNCC") of the frames tracked FROM NOW ON: dict(thres=, win=15,
        pattern="centered", pairs=("temporal",)) — a feature is promoted to the next track set only where the ZNCC of its
        win x win patches exceeds thres: "temporal" the previous left image at its input pixel against the current left image
        at its final pixel, "stereo" the current left against the current right image. None: off (the default). Refused while
        a frame is in flight."""
        pairs, win, pattern, thres = _zncc_gate_arg(gate, True)
        self.ctx.check(self.lib.vo_svo_set_zncc_gate(self._h, pairs, win, pattern, thres))
        self._zncc_pairs = pairs

    def getZncc(self):
        """Inspection: the values the gate computed for the last steady-state frame, per INPUT feature of that frame (the
        track set before it): {"temporal": float32 [n] or None, "stereo": float32 [n] or None}. A feature that was lost on the
        way has whatever its pixels gave."""
        n = C.c_int()
        self.ctx.check(self.lib.vo_svo_get_zncc(self._h, None, None, 0, C.byref(n)))
        t, s = np.full(n.value, np.nan, np.float32), np.full(n.value, np.nan, np.float32)
        self.ctx.check(self.lib.vo_svo_get_zncc(self._h, t.ctypes.data, s.ctypes.data, n.value, C.byref(n)))
        return {"temporal": t if self._zncc_pairs & 1 else None, "stereo": s if self._zncc_pairs & 2 else None}

    SEMIDENSE_EVERY = {"keyframe": 0, "frame": 1}  # VO_SEMIDENSE_*

    def setSemiDense(self, params, every="keyframe"):
        """Semi-dense stereo depth (include/vo_hip.h, "Semi-dense stereo") of every keyframe's — every="frame": every frame's —
        own rectified pair, computed on the side stream behind the frame; the odometry's results do not change. params: dict of
        Context.semiDenseStereo's parameters (bf is needed), None: off. Refused while a frame is in flight. StereoVO only."""
        if params is None:
            self.ctx.check(self.lib.vo_svo_set_semidense(self._h, None, 0))
            return
        if every not in self.SEMIDENSE_EVERY:
            raise ValueError(f"every must be one of {sorted(self.SEMIDENSE_EVERY)}, not {every!r}")
        if "bf" not in params:
            raise ValueError("setSemiDense: bf (focal length x baseline) is needed")
        p = _semidense_params(self.lib, params)
        self.ctx.check(self.lib.vo_svo_set_semidense(self._h, C.byref(p), self.SEMIDENSE_EVERY[every]))

    def getSemiDense(self):
        """The last semi-dense result (a SemiDenseResult with frame_id, T_wc (4, 4) and n_accepted), None before any. Waits for
        that result's launch only."""
        w, h, fid, na = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        T = np.zeros((4, 4), np.float32)
        self.ctx.check(self.lib.vo_svo_get_semidense(self._h, None, None, None, None, C.byref(w), C.byref(h), C.byref(fid), None, None))
        if w.value <= 0:
            return None
        d, sc, sg = (np.zeros((h.value, w.value), np.float32) for _ in range(3))
        st = np.zeros((h.value, w.value), np.uint8)
        self.ctx.check(self.lib.vo_svo_get_semidense(self._h, d.ctypes.data, sc.ctypes.data, sg.ctypes.data, st.ctypes.data, C.byref(w), C.byref(h),
                                                     C.byref(fid), T.ctypes.data, C.byref(na)))
        return SemiDenseResult(d, sc, sg, st, fid.value, T, na.value)

    def setDenseStereo(self, params, every="keyframe"):
        """Dense stereo disparity (include/vo_hip.h, "Dense stereo") of every keyframe's — every="frame": every frame's — own
        rectified pair, computed on the side stream behind the frame; the odometry's and the semi-dense options' results do not
        change. params: dict of Context.denseStereo's parameters (bf is needed), None: off. Refused while a frame is in flight.
        StereoVO only; independent of setSemiDense."""
        if params is None:
            self.ctx.check(self.lib.vo_svo_set_dense_stereo(self._h, None, 0))
            return
        if every not in self.SEMIDENSE_EVERY:
            raise ValueError(f"every must be one of {sorted(self.SEMIDENSE_EVERY)}, not {every!r}")
        if "bf" not in params:
            raise ValueError("setDenseStereo: bf (focal length x baseline) is needed")
        p = _dense_stereo_params(self.lib, params)
        self.ctx.check(self.lib.vo_svo_set_dense_stereo(self._h, C.byref(p), self.SEMIDENSE_EVERY[every]))

    def getDenseStereo(self):
        """The last dense stereo result (a DenseStereoResult with frame_id, T_wc (4, 4) and n_accepted), None before any. Waits for
        that result's launches only."""
        w, h, fid, na = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        T = np.zeros((4, 4), np.float32)
        self.ctx.check(self.lib.vo_svo_get_dense_stereo(self._h, None, None, None, None, C.byref(w), C.byref(h), C.byref(fid), None, None))
        if w.value <= 0:
            return None
        d, sg = (np.zeros((h.value, w.value), np.float32) for _ in range(2))
        co, st = np.zeros((h.value, w.value), np.uint16), np.zeros((h.value, w.value), np.uint8)
        self.ctx.check(self.lib.vo_svo_get_dense_stereo(self._h, d.ctypes.data, co.ctypes.data, sg.ctypes.data, st.ctypes.data, C.byref(w), C.byref(h),
                                                        C.byref(fid), T.ctypes.data, C.byref(na)))
        return DenseStereoResult(d, co, sg, st, fid.value, T, na.value)

    def setDenseSpeckle(self, params=True):
        """The speckle filter (include/vo_hip.h, "Speckle filter") behind every dense result, on the side stream, in place:
        getDenseStereo and getDensePoints then leave the small components out (status 6). params: True (the defaults: max_size 100,
        max_diff 1.0) or dict(max_size=, max_diff=); None or False: off. Needs setDenseStereo. Refused while a frame is in flight."""
        if params is None or params is False:
            self.ctx.check(self.lib.vo_svo_set_dense_speckle(self._h, None))
            return
        p = _speckle_params(self.lib, params)
        self.ctx.check(self.lib.vo_svo_set_dense_speckle(self._h, C.byref(p)))

    def getDenseSpeckleStats(self):
        """(n_removed, n_components) of the last dense result's filter; (0, 0) before any. Waits for that result's launches only."""
        nr, nc = C.c_int(), C.c_int()
        self.ctx.check(self.lib.vo_svo_get_dense_speckle_stats(self._h, C.byref(nr), C.byref(nc)))
        return nr.value, nc.value

    def getDensePoints(self, world=True, capacity=None):
        """The accepted pixels of the last dense stereo result as points, raster order: getSemiDensePoints' dict; None before any."""
        return self._semidense_points(lambda *a: self.lib.vo_svo_get_dense_points(self._h, int(bool(world)), *a), capacity)

    def setSemiDenseTemporal(self, params):
        """The temporal search and fusion (include/vo_hip.h, "Semi-dense temporal"): every keyframe's static result seeds a map that
        each later frame until the next keyframe updates, on the side stream; the odometry's results do not change. params: dict
        of Context.semiDenseTemporal's parameters ({}: the defaults), None: off. Needs setSemiDense. Refused while a frame is in flight."""
        if params is None:
            self.ctx.check(self.lib.vo_svo_set_semidense_temporal(self._h, None))
            return
        p = _semidense_temporal_params(self.lib, params)
        self.ctx.check(self.lib.vo_svo_set_semidense_temporal(self._h, C.byref(p)))

    def getSemiDenseMap(self, regularized=False):
        """The last keyframe's map (a SemiDenseMap with frame_id, T_wc (4, 4) and n_fused), None before a keyframe. Waits for the side
        stream's last launch only. regularized=True (setSemiDenseRegularize): the regularised copy of that map instead, a
        SemiDenseRegularized with rstatus; None before the first frame since the option was switched on."""
        w, h, fid, nf = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        T = np.zeros((4, 4), np.float32)
        if regularized:
            get = self.lib.vo_svo_get_semidense_regularized
            self.ctx.check(get(self._h, None, None, None, None, C.byref(w), C.byref(h), C.byref(fid), None, None))
            if w.value <= 0:
                return None
            invd, sg = np.zeros((h.value, w.value), np.float32), np.zeros((h.value, w.value), np.float32)
            no, rs = np.zeros((h.value, w.value), np.uint8), np.zeros((h.value, w.value), np.uint8)
            self.ctx.check(get(self._h, invd.ctypes.data, sg.ctypes.data, no.ctypes.data, rs.ctypes.data, C.byref(w), C.byref(h), C.byref(fid),
                               T.ctypes.data, C.byref(nf)))
            return SemiDenseRegularized(invd, sg, no, rs, fid.value, T, nf.value)
        self.ctx.check(self.lib.vo_svo_get_semidense_map(self._h, None, None, None, None, C.byref(w), C.byref(h), C.byref(fid), None, None))
        if w.value <= 0:
            return None
        invd, sg = np.zeros((h.value, w.value), np.float32), np.zeros((h.value, w.value), np.float32)
        no, ts = np.zeros((h.value, w.value), np.uint8), np.zeros((h.value, w.value), np.uint8)
        self.ctx.check(self.lib.vo_svo_get_semidense_map(self._h, invd.ctypes.data, sg.ctypes.data, no.ctypes.data, ts.ctypes.data, C.byref(w),
                                                         C.byref(h), C.byref(fid), T.ctypes.data, C.byref(nf)))
        return SemiDenseMap(invd, sg, no, ts, None, fid.value, T, nf.value)

    def setSemiDensePropagate(self, params):
        """The map carried over to the next keyframe (include/vo_hip.h, "Semi-dense propagation"): at a keyframe the old map is
        warped into the new keyframe under the odometry's pose and fused with its static result instead of being thrown away, so
        getSemiDensePoints(fused=True, min_obs=2) has points on a keyframe frame too; the odometry's results do not change. params:
        dict(min_obs=, max_diff=, chi=, sigma_add=) ({}: the defaults), None: off. Needs setSemiDenseTemporal. Refused while a
        frame is in flight."""
        if params is None:
            self.ctx.check(self.lib.vo_svo_set_semidense_propagate(self._h, None))
            return
        p = _semidense_propagate_params(self.lib, params)
        self.ctx.check(self.lib.vo_svo_set_semidense_propagate(self._h, C.byref(p)))

    def setSemiDenseRegularize(self, params):
        """A regularised copy of the map (include/vo_hip.h, "Semi-dense regularisation"): behind every launch that writes the map one
        launch on the side stream removes the entries their neighbours contradict, fills high-gradient holes whose neighbours agree
        and smooths the rest, into planes of its own (getSemiDenseMap(regularized=True), getSemiDensePoints(fused=True,
        regularized=True)); the odometry's results, the semi-dense results and the map itself do not change. params:
        dict(radius=, chi=, dist_sigma=, min_support=, fill_min=, g_min=) ({}: the defaults), None: off. Needs setSemiDenseTemporal.
        Refused while a frame is in flight."""
        if params is None:
            self.ctx.check(self.lib.vo_svo_set_semidense_regularize(self._h, None))
            return
        p = _semidense_regularize_params(self.lib, params)
        self.ctx.check(self.lib.vo_svo_set_semidense_regularize(self._h, C.byref(p)))

    def setSemiDenseWorld(self, params, source=None):
        """The keyframes' maps fused into one world-frame voxel map (include/vo_hip.h, "Semi-dense world map"): when a keyframe is
        replaced, one launch on the side stream integrates its map, with its T_wc and key plane, into a hash table of voxels;
        flushSemiDenseWorld() integrates the current keyframe's at the end of a sequence, getSemiDenseWorld() reads the voxels. The
        odometry's results, the semi-dense results and the map do not change. params: dict(voxel=, capacity_log2=, min_obs=, z_max=,
        source="raw" | "regularized" | "dense" | "merged", merge=dict(chi=, keep_obs=)) ({}: the defaults), None: off. Needs
        setSemiDenseTemporal; source="regularized" also setSemiDenseRegularize; "dense" (the keyframe's dense result seeded) and "merged"
        (the keyframe's map merged with it: "Semi-dense map merge") also setDenseStereo. Refused while a frame is in flight."""
        if params is None:
            self.ctx.check(self.lib.vo_svo_set_semidense_world(self._h, None, 0))
            return
        params = dict(params)
        src = params.pop("source", "raw")
        reanchor = params.pop("reanchor", None)
        carve = params.pop("carve", None)
        merge = params.pop("merge", None)
        if source is not None:
            src = source
        if src not in SEMIDENSE_WORLD_SOURCE:
            raise ValueError(f"setSemiDenseWorld: source {src!r}; known: {sorted(SEMIDENSE_WORLD_SOURCE)}")
        p = _semidense_world_params(self.lib, params)
        self.ctx.check(self.lib.vo_svo_set_semidense_world(self._h, C.byref(p), SEMIDENSE_WORLD_SOURCE[src]))
        if reanchor is not None:
            self.setSemiDenseWorldReanchor(reanchor)
        if carve is not None:
            self.setSemiDenseWorldCarve(carve)
        if merge is not None:
            self.setSemiDenseWorldMerge(merge)

    def setSemiDenseWorldMerge(self, params=None):
        """chi and keep_obs of the merges the world map's sources "dense" and "merged" enqueue from now on: dict(chi=, keep_obs=);
        None or True: the defaults (3, 2). Refused while a frame is in flight."""
        if params is None or params is True:
            self.ctx.check(self.lib.vo_svo_set_semidense_world_merge(self._h, None))
            return
        p = _semidense_merge_params(self.lib, params)
        self.ctx.check(self.lib.vo_svo_set_semidense_world_merge(self._h, C.byref(p)))

    def getSemiDenseWorldSource(self):
        """What the world map's source "dense" or "merged" last integrated: a SemiDenseMerged with the keyframe's frame id — the planes,
        origin and counts of the last merge the driver enqueued —, or None where there is none yet. Waits for the side stream only."""
        w, h, fid = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.lib.vo_svo_get_semidense_world_source(self._h, None, None, None, None, C.byref(w), C.byref(h), C.byref(fid), None))
        if w.value == 0:
            return None
        shape = (h.value, w.value)
        invd, sigma = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        n_obs, origin, counts = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8), np.zeros(6, np.uint64)
        self.ctx.check(self.lib.vo_svo_get_semidense_world_source(self._h, invd.ctypes.data, sigma.ctypes.data, n_obs.ctypes.data, origin.ctypes.data,
                                                                  C.byref(w), C.byref(h), C.byref(fid), counts.ctypes.data))
        return SemiDenseMerged(invd, sigma, n_obs, origin, counts, fid.value)

    def setSemiDenseWorldCarve(self, params):
        """Free-space carving on the world map (include/vo_hip.h, "Semi-dense world map: free-space carving"): directly behind every
        integration of a keyframe's map, one more launch on the side stream marches that map's rays through the table and counts, per
        voxel, the rays that passed through it on their way to a surface behind (`free` of getSemiDenseWorld(max_free=...)). A voxel
        left by a moving object or a flying pixel collects free counts; a surface does not. params: True or dict(margin=, chi=,
        z_near=); None or False: off. Needs setSemiDenseWorld. The odometry's results, the semi-dense results, the keyframe poses
        and every other field of every voxel do not change. Refused while a frame is in flight."""
        if params is None or params is False:
            self.ctx.check(self.lib.vo_svo_set_semidense_world_carve(self._h, None))
            return
        p = _semidense_world_carve_params(self.lib, params)
        self.ctx.check(self.lib.vo_svo_set_semidense_world_carve(self._h, C.byref(p)))

    def getSemiDenseWorldCarveStats(self):
        """dict(carves, rays, short_rays, visits, hits) of the world map"""
        info = _capi.SemiDenseWorldCarveInfo()
        self.ctx.check(self.lib.vo_svo_get_semidense_world_carve_stats(self._h, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in _capi.SemiDenseWorldCarveInfo._fields_}

    def setSemiDenseWorldReanchor(self, params):
        """The world map follows the local BA (include/vo_hip.h, "Semi-dense world map: removal and re-anchoring"): the maps of the
        keyframes in the BA's window are retained on the device, and at every keyframe each one whose keyframe the BA has moved is
        taken out of the table and put back with the keyframe's current pose, so that getSemiDenseWorld() agrees with
        getKeyframes(). params: True or dict(min_move=0.0) — the smallest motion, in voxels, worth a re-anchor; None or False: off.
        Needs setSemiDenseWorld and local_ba. The odometry's results, the semi-dense results and the keyframe poses do not change.
        Refused while a frame is in flight."""
        if params is None or params is False:
            self.ctx.check(self.lib.vo_svo_set_semidense_world_reanchor(self._h, 0, 0.0))
            return
        prm = {} if params is True else dict(params)
        min_move = float(prm.pop("min_move", 0.0))
        if prm:
            raise ValueError(f"setSemiDenseWorldReanchor: unknown parameter {sorted(prm)[0]!r}; known: ['min_move']")
        self.ctx.check(self.lib.vo_svo_set_semidense_world_reanchor(self._h, 1, min_move))

    def getSemiDenseWorldAnchors(self):
        """Per keyframe integrated with setSemiDenseWorldReanchor on, in integration order: dict(frame_id int32 [n], index int32 [n]
        (the keyframe's place in getKeyframes()), T_wk float32 [n, 4, 4] (the pose its map is in the table with), in_window bool [n])."""
        n = C.c_int()
        rc = self.lib.vo_svo_get_semidense_world_anchors(self._h, 0, None, None, None, None, C.byref(n))
        if rc < 0 and rc != -8:
            self.ctx.check(rc)
        m = max(n.value, 1)
        fid, idx, T, inw = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros((m, 4, 4), np.float32), np.zeros(m, np.int32)
        self.ctx.check(self.lib.vo_svo_get_semidense_world_anchors(self._h, n.value, fid.ctypes.data, idx.ctypes.data, T.ctypes.data, inw.ctypes.data,
                                                                   C.byref(n)))
        k = n.value
        return dict(frame_id=fid[:k], index=idx[:k], T_wk=T[:k], in_window=inw[:k].astype(bool))

    def getSemiDenseWorldReanchorStats(self):
        """dict(removals, refused_removals, removed, missing, reanchors, vacant) of the world map"""
        info = _capi.SemiDenseWorldReanchorInfo()
        self.ctx.check(self.lib.vo_svo_get_semidense_world_reanchor_stats(self._h, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in _capi.SemiDenseWorldReanchorInfo._fields_}

    def flushSemiDenseWorld(self):
        """Integrates the current keyframe's map now (the end of a sequence); the next keyframe change does not integrate it again."""
        self.ctx.check(self.lib.vo_svo_semidense_world_flush(self._h))

    def clearSemiDenseWorld(self):
        self.ctx.check(self.lib.vo_svo_semidense_world_clear(self._h))

    def getSemiDenseWorld(self, min_count=1, min_keyframes=1, capacity=None, max_free=None):
        """The world map's voxels with count >= min_count and keyframes >= min_keyframes: a SemiDenseWorldPoints in ascending key
        order. With max_free=(num, den) the result is a SemiDenseWorldFreePoints, with `free`, and with den >= 1 only the voxels with
        free * den <= count * num are kept ((0, 0): all of them). Waits for the side stream's last launch only."""
        if max_free is not None:
            num, den = _max_free(max_free)
            get = lambda cap, *a: self.lib.vo_svo_get_semidense_world_points_free(self._h, int(min_count), int(min_keyframes), num, den, cap, *a)
            return _semidense_world_points(self.ctx.check, get, capacity, False, True)
        get = lambda *a: self.lib.vo_svo_get_semidense_world_points(self._h, int(min_count), int(min_keyframes), *a)
        return _semidense_world_points(self.ctx.check, get, capacity, False)

    def getSemiDenseWorldStats(self):
        """dict(occupied, capacity, integrations, refused, inserted, skipped, out_of_range) of the world map"""
        info = _capi.SemiDenseWorldInfo()
        self.ctx.check(self.lib.vo_svo_get_semidense_world_stats(self._h, C.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in _capi.SemiDenseWorldInfo._fields_}

    def setSemiDenseAlignAffine(self, params):
        """A modifier of whichever alignment is on (include/vo_hip.h, "Semi-dense alignment with affine brightness"): its launches
        estimate a gain and an offset of the keyframe's grey levels next to the pose, so that an exposure change between the keyframe
        and the frame does not bias the pose. params: True or dict(gain0=1, offset0=0); None: off. Needs setSemiDenseAlign or
        setSemiDenseAlignPyramid on; turning the alignment off turns it off too. getSemiDenseAlign then has gain, offset, G, O, H (8,
        8) and b (8,). The odometry's results, the semi-dense results and the map do not change. Refused while a frame is in flight."""
        if params is None or params is False:
            self.ctx.check(self.lib.vo_svo_set_semidense_align_affine(self._h, None))
            self._sda_affine = False
            return
        p = _semidense_affine_params(self.lib, params)
        self.ctx.check(self.lib.vo_svo_set_semidense_align_affine(self._h, C.byref(p)))
        self._sda_affine = True

    def setSemiDenseAlign(self, params):
        """Direct image alignment on the keyframe's map (include/vo_hip.h, "Semi-dense alignment"): every frame that is not a
        keyframe aligns its left image against the map as the previous frames left it, from the odometry's pose, on the side stream
        in front of the frame's temporal launch; the odometry's results, the semi-dense results and the map do not change. params:
        dict(min_obs=, huber=, max_iters=, eps=, min_pixels=) ({}: the defaults), None: off. Needs setSemiDenseTemporal. Refused
        while a frame is in flight. A dict that names levels, max_iters_level or start goes to setSemiDenseAlignPyramid."""
        if params is None:
            self.ctx.check(self.lib.vo_svo_set_semidense_align(self._h, None))
            self._sda_affine = False
            return
        if {"levels", "max_iters_level", "start"} & set(params):
            return self.setSemiDenseAlignPyramid(params)
        params = dict(params)
        affine = params.pop("affine", None)
        p = _semidense_align_params(self.lib, params)
        self.ctx.check(self.lib.vo_svo_set_semidense_align(self._h, C.byref(p)))
        if affine is not None:
            self.setSemiDenseAlignAffine(affine)

    def setSemiDenseAlignPyramid(self, params):
        """The alignment of setSemiDenseAlign coarse to fine (include/vo_hip.h, "Semi-dense alignment on a map pyramid"): at a
        keyframe the left image's coarser levels are kept next to its plane; at every other frame a pyramid of the map is formed and
        the alignment runs from the top level down, on the side stream in front of the frame's temporal launch. params: dict(levels=4,
        max_iters_level=(...), start="odometry" | "previous", and setSemiDenseAlign's fields); None: off. start="previous": the
        alignment follows its own pose — the identity at the first frame after a keyframe, then the previous frame's aligned pose
        where that frame converged (status 0 or 1), else the odometry's. Takes effect with the next keyframe. The odometry's results,
        the semi-dense results and the map do not change. Needs setSemiDenseTemporal. Refused while a frame is in flight."""
        if params is None:
            self.ctx.check(self.lib.vo_svo_set_semidense_align_pyr(self._h, None, 0))
            self._sda_affine = False
            return
        prm = dict(params)
        affine = prm.pop("affine", None)
        start = prm.pop("start", "odometry")
        if start not in SEMIDENSE_ALIGN_START:
            raise ValueError(f"semi-dense alignment: start={start!r}; known: {sorted(SEMIDENSE_ALIGN_START)}")
        p = _semidense_align_pyr_params(self.lib, prm)
        self.ctx.check(self.lib.vo_svo_set_semidense_align_pyr(self._h, C.byref(p), SEMIDENSE_ALIGN_START[start]))
        if affine is not None:
            self.setSemiDenseAlignAffine(affine)

    def getSemiDenseAlign(self):
        """The last frame's alignment (a SemiDenseAligned with T_wc, frame_id, key_frame_id, the per-level fields and the start that
        was used); status 4 and key_frame_id -1 at a keyframe frame, which has none. Waits for the side stream's last launch only.
        With setSemiDenseAlignAffine on: the affine run's, with gain, offset, G, O, H (8, 8) and b (8,)."""
        affine = getattr(self, "_sda_affine", False)
        res = _capi.SemiDenseAlignAffineResult() if affine else _capi.SemiDenseAlignPyrResult()
        T = np.zeros((4, 4), np.float32)
        fid, kid = C.c_int(), C.c_int()
        get = self.lib.vo_svo_get_semidense_align_affine if affine else self.lib.vo_svo_get_semidense_align_pyr
        self.ctx.check(get(self._h, C.byref(res), T.ctypes.data, C.byref(fid), C.byref(kid)))
        return _semidense_aligned(res, T, fid.value, kid.value)

    def getSemiDenseOrigin(self):
        """(origin uint8 (height, width), from_frame_id) of the last keyframe's map — 0 nothing, 1 static only, 2 propagated only,
        3 fused, 4 static replaced an inconsistent propagated value; from_frame_id: the keyframe the map was propagated from, -1
        where it was seeded without a predecessor. None before a keyframe. Waits for the side stream's last launch only."""
        w, h, fid = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.lib.vo_svo_get_semidense_origin(self._h, None, C.byref(w), C.byref(h), C.byref(fid)))
        if w.value <= 0:
            return None
        origin = np.zeros((h.value, w.value), np.uint8)
        self.ctx.check(self.lib.vo_svo_get_semidense_origin(self._h, origin.ctypes.data, C.byref(w), C.byref(h), C.byref(fid)))
        return origin, fid.value

    def getSemiDensePoints(self, world=True, capacity=None, fused=False, min_obs=2, regularized=False):
        """The accepted pixels of the last semi-dense result as points, raster order: dict(xyz float32 [n, 3] — in the world frame
        (the frame's T_wc) or, world=False, the left camera's —, sigma_invd [n], pixel uint16 [n, 2], frame_id); None before any.
        capacity: room for that many points (default: all); more raise VoError(VO_ERR_CAPACITY) whose `n` holds the true count.
        fused=True (setSemiDenseTemporal): the last keyframe's map instead — its pixels with n_obs >= min_obs, z = 1 / invd; with
        regularized=True (setSemiDenseRegularize) the regularised copy of that map (a filled pixel has n_obs 1)."""
        if regularized:
            if not fused:
                raise ValueError("getSemiDensePoints: regularized=True is of the fused map: fused=True")
            get = lambda *a: self.lib.vo_svo_get_semidense_regularized_points(self._h, int(bool(world)), int(min_obs), *a)
        elif fused:
            get = lambda *a: self.lib.vo_svo_get_semidense_map_points(self._h, int(bool(world)), int(min_obs), *a)
        else:
            get = lambda *a: self.lib.vo_svo_get_semidense_points(self._h, int(bool(world)), *a)
        return self._semidense_points(get, capacity)

    def _semidense_points(self, get, capacity):
        n, fid = C.c_int(), C.c_int()
        rc = get(0, None, None, None, C.byref(n), C.byref(fid))
        if rc < 0 and rc != -8:  # (VO_ERR_CAPACITY: the count is what was asked for)
            self.ctx.check(rc)
        if fid.value < 0:
            return None
        cap = n.value if capacity is None else int(capacity)
        xyz, sg, px = np.zeros((max(cap, 1), 3), np.float32), np.zeros(max(cap, 1), np.float32), np.zeros((max(cap, 1), 2), np.uint16)
        rc = get(cap, xyz.ctypes.data, sg.ctypes.data, px.ctypes.data, C.byref(n), C.byref(fid))
        try:
            self.ctx.check(rc)
        except VoError as e:  # (VO_ERR_CAPACITY: `n` holds the true count)
            e.n = n.value
            raise
        m = min(n.value, cap)
        return dict(xyz=xyz[:m], sigma_invd=sg[:m], pixel=px[:m], frame_id=fid.value)

    def _img(self, a):
        """a host image as the library reads it: a u8 plane, or — with rectify=True — an array of the context's input format"""
        if self.prm.rectify and self.ctx._fmt != "mono8":
            return self.ctx._format_image(a)
        return _u8(a)

    def _nd(self):
        return 3 if self.prm.rectify and self.ctx._fmt in ("rgb8", "bgr8") else 2

    def _ptrs(self, left, right):
        if isinstance(left, np.ndarray):
            left, right = self._img(left), self._img(right)
            if left.ndim != self._nd() or left.shape != right.shape:
                raise ValueError("images must be two u8 planes of one size")
            return left, right, left.ctypes.data, right.ctypes.data, left.strides[0], 0
        return left, right, int(left[0]), int(right[0]), int(left[1]), 1  # (device address, stride) pairs

    def _out(self):
        i = self._info
        T = np.array(i.T_wc, np.float32).reshape(4, 4)
        self.stats_frame.append(T)
        return SvoFrameInfo.from_buffer_copy(i)  # (the caller's own copy: a stored info must not change with the next frame)

    def trackStereoImages(self, img_left, img_right, timestamp=0.0):
        """numpy u8 images (host) or (device address, stride) pairs. Returns the frame's SvoFrameInfo."""
        a, b, pl, pr, st, dev = self._ptrs(img_left, img_right)
        self._keep = (a, b)
        rc = self.lib.vo_svo_track(self._h, pl, pr, st, dev, float(timestamp), self._info)
        if rc < 0:
            self.ctx.check(rc)
        return self._out()

    def enqueue(self, img_left, img_right, timestamp=0.0):
        a, b, pl, pr, st, dev = self._ptrs(img_left, img_right)
        self._keep = (a, b)
        rc = self.lib.vo_svo_enqueue(self._h, pl, pr, st, dev, float(timestamp))
        if rc < 0:
            self.ctx.check(rc)

    def prefetch(self, img_left, img_right):
        a, b, pl, pr, st, dev = self._ptrs(img_left, img_right)
        self._keep_next = (a, b)
        rc = self.lib.vo_svo_prefetch(self._h, pl, pr, st, dev)
        if rc < 0:
            self.ctx.check(rc)

    def result(self):
        rc = self.lib.vo_svo_result(self._h, self._info)
        if rc < 0:
            self.ctx.check(rc)
        return self._out()

    def runSequence(self, pairs, k_begin=0, k_end=None):
        """A recorded sequence of (device address, stride) pairs — [((left, stride), (right, stride)), ...] — or of (left, right)
        numpy u8 images of one size and layout (host memory: uploaded one frame ahead, under the frame in flight) through the
        loop inside the library (vo_svo_run): frames k_begin .. k_end - 1 are collected; frame k_end is left in flight for the
        next call (or result()). Returns (list of SvoFrameInfo, numpy array of CLOCK_MONOTONIC stamps)."""
        n = len(pairs)
        k_end = n if k_end is None else int(k_end)
        host = n > 0 and isinstance(pairs[0][0], np.ndarray)
        if host:  # (the arrays themselves are handed to the library: they are kept alive with the list, below)
            if getattr(self, "_seq_ref", None) is not pairs or len(getattr(self, "_seq_host", ())) != n:
                self._seq_host = [(self._img(L), self._img(R)) for L, R in pairs]
                st0 = self._seq_host[0][0].strides[0]
                if any(a.ndim != self._nd() or a.shape != b.shape or a.strides[0] != st0 or b.strides[0] != st0 for a, b in self._seq_host):
                    raise ValueError("runSequence: host images must be u8 planes of one size and row stride")
            src = [((a.ctypes.data, a.strides[0]), (b.ctypes.data, b.strides[0])) for a, b in self._seq_host]
        else:
            src = pairs
        # The address arrays are kept between calls on the SAME list object (held here, so its id cannot be reused) of the
        # same length, and the entries this call hands to the library (k_begin .. k_end + 1) are compared with them: a list
        # that was changed in place, or another list, rebuilds the arrays.
        L, R = getattr(self, "_seq_L", None), getattr(self, "_seq_R", None)
        fresh = getattr(self, "_seq_ref", None) is not pairs or L is None or len(L) != n
        if not fresh:
            for k in range(max(int(k_begin), 0), min(k_end + 2, n)):
                if L[k] != int(src[k][0][0]) or R[k] != int(src[k][1][0]):
                    fresh = True
                    break
        if fresh:
            self._seq_L = (C.c_void_p * n)(*[int(p[0][0]) for p in src])
            self._seq_R = (C.c_void_p * n)(*[int(p[1][0]) for p in src])
            self._seq_ref = pairs
        self._seq_stride = int(src[0][0][1])
        m = k_end - int(k_begin)
        infos = (SvoFrameInfo * max(m, 1))()
        stamps = np.zeros(max(m, 1), np.float64)
        rc = self.lib.vo_svo_run(self._h, self._seq_L, self._seq_R, n, self._seq_stride, 0 if host else 1, int(k_begin), k_end, infos,
                                 stamps.ctypes.data)
        if rc < 0:
            self.ctx.check(rc)
        out = [SvoFrameInfo.from_buffer_copy(infos[j]) for j in range(m)]
        for i in out:
            self.stats_frame.append(np.array(i.T_wc, np.float32).reshape(4, 4))
        return out, stamps[:m]

    def getDebugImage(self):
        """img_debug_ of the last frame that drew one (debug_image=True): an (H, W, 3) uint8 array — published as bgr8 by the
        reference's nodes, (0, 255, 0) is green — or an empty (0, 0, 3) array before the first one and with the option off."""
        w, h = C.c_int(), C.c_int()
        self.ctx.check(self.lib.vo_svo_get_debug_image(self._h, None, 0, C.addressof(w), C.addressof(h)))
        out = np.zeros((h.value, w.value, 3), np.uint8)
        if out.size:
            self.ctx.check(self.lib.vo_svo_get_debug_image(self._h, out.ctypes.data, out.strides[0], C.addressof(w), C.addressof(h)))
        return out

    def setPoseCovariance(self, on, sigma_px=0.0):
        """Switches the option (vo_svo_set_pose_covariance); switching it on starts the chain at P = 0."""
        self.ctx.check(self.lib.vo_svo_set_pose_covariance(self._h, int(bool(on)), float(sigma_px)))

    def getPoseCovariance(self):
        """PoseCovariance(P, Sigma_xi, s2, valid, n_points, n_unknown_steps) of the last frame (pose_covariance=True): waits
        for that frame's covariance launch only."""
        P, S = np.zeros((6, 6)), np.zeros((6, 6))
        s2, valid, n, unk = C.c_double(), C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.lib.vo_svo_get_pose_covariance(self._h, P.ctypes.data, S.ctypes.data, C.addressof(s2), C.addressof(valid),
                                                           C.addressof(n), C.addressof(unk)))
        return PoseCovariance(P, S, s2.value, bool(valid.value), n.value, unk.value)

    def getPoseCovarianceRos(self):
        """The 36 doubles of nav_msgs::Odometry::pose.covariance for the last frame's pose (pose_covariance_ros)."""
        return pose_covariance_ros(self.getPoseCovariance().P, np.array(self._info.T_wc, np.float32).reshape(4, 4))

    def getPoseCovarianceInputs(self):
        """Test hook: what the last frame's covariance launch read: dict(X, pts_l, pts_r, T01)."""
        n, T = C.c_int(), np.zeros(16, np.float32)
        self.ctx.check(self.lib.vo_svo_get_pose_covariance_inputs(self._h, None, None, None, 0, C.addressof(n), T.ctypes.data))
        m = max(n.value, 1)
        X, pl, pr = np.zeros((m, 3), np.float32), np.zeros((m, 2), np.float32), np.zeros((m, 2), np.float32)
        self.ctx.check(self.lib.vo_svo_get_pose_covariance_inputs(self._h, X.ctypes.data, pl.ctypes.data, pr.ctypes.data, m,
                                                                  C.addressof(n), T.ctypes.data))
        k = n.value
        return dict(X=X[:k], pts_l=pl[:k], pts_r=pr[:k], T01=T.reshape(4, 4))

    def getTracks(self):
        """The track set the next frame starts from: dict(ids, pts_l, pts_r, Xw, flags)."""
        n = C.c_int()
        self.ctx.check(self.lib.vo_svo_get_tracks(self._h, None, None, None, None, None, 0, C.addressof(n)))
        m = max(n.value, 1)
        ids, pl, pr = np.zeros(m, np.int32), np.zeros((m, 2), np.float32), np.zeros((m, 2), np.float32)
        X, fl = np.zeros((m, 3), np.float32), np.zeros(m, np.uint8)
        self.ctx.check(self.lib.vo_svo_get_tracks(self._h, ids.ctypes.data, pl.ctypes.data, pr.ctypes.data, X.ctypes.data,
                                                  fl.ctypes.data, m, C.addressof(n)))
        k = n.value
        return dict(ids=ids[:k], pts_l=pl[:k], pts_r=pr[:k], Xw=X[:k], flags=fl[:k])

    def getNewPoints(self):
        """Step [10] of the last frame: dict(pts_l, pts_r, mask_new, accept)."""
        nb = self.prm.bins.n_bins_u * self.prm.bins.n_bins_v
        pl, pr = np.zeros((nb, 2), np.float32), np.zeros((nb, 2), np.float32)
        m, a, n = np.zeros(nb, np.uint8), np.zeros(nb, np.uint8), C.c_int()
        self.ctx.check(self.lib.vo_svo_get_new_points(self._h, pl.ctypes.data, pr.ctypes.data, m.ctypes.data, a.ctypes.data,
                                                      C.addressof(n)))
        k = n.value
        return dict(pts_l=pl[:k], pts_r=pr[:k], mask_new=m[:k].astype(bool), accept=a[:k].astype(bool))

    def deviceBytes(self):
        """Device memory held for this stream's keyframes (table, ring, pool, the local BA's scratch and arena)."""
        n = C.c_size_t(0)
        self.ctx.check(self.lib.vo_svo_device_bytes(self._h, C.byref(n)))
        return n.value

    def getKeyframes(self):
        """AlgorithmStatistics::stats_keyframe as of now (stereo_vo.cpp:805-821): [(T_wc, mappoints [n][3])] for every
        keyframe so far — current poses, current 3-D points of the related landmarks."""
        n, tot = C.c_int(), C.c_size_t()
        self.ctx.check(self.lib.vo_svo_keyframe_count(self._h, C.addressof(n)))
        nk = n.value
        if nk == 0:
            return []
        T, cnt = np.zeros((nk, 16), np.float32), np.zeros(nk, np.int32)
        self.ctx.check(self.lib.vo_svo_get_keyframes(self._h, T.ctypes.data, cnt.ctypes.data, None, 0, C.addressof(tot)))
        X = np.zeros((max(tot.value, 1), 3), np.float32)
        if tot.value:
            self.ctx.check(self.lib.vo_svo_get_keyframes(self._h, None, None, X.ctypes.data, tot.value, C.addressof(tot)))
        off = np.concatenate([[0], np.cumsum(cnt)])
        return [(T[j].reshape(4, 4).copy(), X[off[j]:off[j + 1]].copy()) for j in range(nk)]

    def getKeyframe(self, j):
        """One keyframe of stats_keyframe: (T_wc, mappoints)."""
        T, m = np.zeros(16, np.float32), C.c_int()
        self.ctx.check(self.lib.vo_svo_get_keyframe(self._h, int(j), T.ctypes.data, None, 0, C.addressof(m)))
        X = np.zeros((max(m.value, 1), 3), np.float32)
        if m.value:
            self.ctx.check(self.lib.vo_svo_get_keyframe(self._h, int(j), None, X.ctypes.data, m.value, C.addressof(m)))
        return T.reshape(4, 4), X[:m.value]

    def getStatistics(self):
        return dict(stats_frame=[T.copy() for T in self.stats_frame], stats_keyframe=self.getKeyframes())


class StereoBatch:
    """S independent stereo streams on one GPU (include/vo_hip.h: vo_batch_*): a context, a StereoVO and a host thread per
    stream inside the library. `svo_params` = StereoVO(...).prm of a template object (or an SvoParams)."""

    def __init__(self, device, n_streams, width, height, max_points, max_level, svo_params):
        self.lib = _capi.load()
        self.n, self.prm = int(n_streams), svo_params
        self.cfg = VoConfig(device, width, height, max_points, 5, max_level)
        self._h = C.c_void_p()
        rc = self.lib.vo_batch_create(C.byref(self.cfg), C.byref(svo_params), self.n, C.byref(self._h))
        if rc < 0:
            raise VoError(rc, "vo_batch_create failed")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vo_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def debug_set(self, key, value):
        if self.lib.vo_batch_debug_set(self._h, int(key), int(value)) < 0:
            raise VoError(-1, "vo_batch_debug_set failed")

    def strict_border(self):
        """The replay arrangement the streams run with (3, 4, 5 become the stream-ordered 1 when S > 1, same results)."""
        return int(self.lib.vo_batch_strict_border(self._h))

    def run(self, left_ptrs, right_ptrs, stride, warmup=0, on_device=True, ids_cap=8192):
        """left_ptrs / right_ptrs: [n_streams][n_frames] addresses. Returns dict(T_wc, ids (list), seconds, wall)."""
        nf = len(left_ptrs[0])
        L = (C.c_void_p * (self.n * nf))(*[p for row in left_ptrs for p in row])
        R = (C.c_void_p * (self.n * nf))(*[p for row in right_ptrs for p in row])
        T = np.zeros((self.n, nf, 4, 4), np.float32)
        ids = np.zeros((self.n, ids_cap), np.int32)
        nid = np.zeros(self.n, np.int32)
        sec = np.zeros(self.n, np.float64)
        wall = C.c_double()
        rc = self.lib.vo_batch_run(self._h, L, R, nf, int(stride), int(bool(on_device)), int(warmup), T.ctypes.data, ids.ctypes.data,
                                   ids_cap, nid.ctypes.data, sec.ctypes.data, C.addressof(wall))
        if rc < 0:
            raise VoError(rc, self.lib.vo_batch_last_error(self._h).decode())
        return dict(T_wc=T, ids=[ids[s, :nid[s]].copy() for s in range(self.n)], seconds=sec, wall=wall.value)


def make_mono_params(width, height, win, max_level, thres_err, thres_bidir, thres_poseba, thres_sampson, K):
    p = MonoParams()
    p.width, p.height, p.win, p.max_level = width, height, win, max_level
    p.thres_err, p.thres_bidirection = thres_err, thres_bidir
    p.thres_poseba, p.thres_sampson = int(thres_poseba), thres_sampson
    for i in range(4):
        p.K[i] = float(K[i])
    return p


class MonoFramePipeline:
    """The steady-state mono frame (mono_vo.cpp:739-963 operator sequence) chained on the
    device: prior + scale, trackBidirectionWithPrior, trackWithScale, pose-only BA on the
    landmarks flagged for it, mask_motion and the Sampson gate. flags[i]: bit 0 =
    lm->isBundled(), bit 1 = member of the class used for the pose-only BA (:800-826)."""

    def __init__(self, ctx, params, strict_border=False):
        self.ctx = ctx
        self.lib = ctx.lib
        self.prm = params
        self.ctx.check(self.lib.vo_stereo_frame_set_strict_border(ctx.handle, int(strict_border)))

    def enqueue(self, pts0, Xw, flags, Tcw_prev, Tcw_prior, dT01_prior, slots=(0, 1)):
        pts0 = _f32(pts0).reshape(-1, 2)
        Xw = _f32(Xw).reshape(-1, 3)
        flags = np.ascontiguousarray(flags, np.uint8)
        self._n = pts0.shape[0]
        if Xw.shape[0] != self._n or flags.shape[0] != self._n:
            raise ValueError("pts0 / Xw / flags differ in length")
        self.ctx.check(self.lib.vo_mono_frame_enqueue(
            self.ctx.handle, C.byref(self.prm), slots[0], slots[1], _p(pts0), _p(Xw), _p(flags, C.c_uint8), self._n,
            _p(_f32(Tcw_prev).reshape(16)), _p(_f32(Tcw_prior).reshape(16)), _p(_f32(dT01_prior).reshape(16)), 0))

    def enqueue_device(self, d_pts0, d_Xw, d_flags, n, Tcw_prev, Tcw_prior, dT01_prior, slots=(0, 1)):
        self._n = n
        f = C.POINTER(C.c_float)
        self.ctx.check(self.lib.vo_mono_frame_enqueue(
            self.ctx.handle, C.byref(self.prm), slots[0], slots[1], C.cast(C.c_void_p(d_pts0), f),
            C.cast(C.c_void_p(d_Xw), f), C.cast(C.c_void_p(d_flags), C.POINTER(C.c_uint8)), n,
            _p(_f32(Tcw_prev).reshape(16)), _p(_f32(Tcw_prior).reshape(16)), _p(_f32(dT01_prior).reshape(16)), 1))

    def enqueue_closed(self, pts0, Xw, flags, Tcw_prev, Tcw_prior, dT01_prior, bins, table, slots=(0, 1)):
        """The frame with its new-point step (mono_vo.cpp:977-1001) closed on the device: candidates = best keypoint of
        every bin of `table` (FeatureExtractor.enqueueCandidates on the image in slots[1]), back-tracked inside the frame
        kernel, emitted for the bins lmtrack_final leaves empty. `bins` = FeatureExtractor.binParams()."""
        pts0 = _f32(pts0).reshape(-1, 2)
        Xw = _f32(Xw).reshape(-1, 3)
        flags = np.ascontiguousarray(flags, np.uint8)
        self._n = pts0.shape[0]
        if Xw.shape[0] != self._n or flags.shape[0] != self._n:
            raise ValueError("pts0 / Xw / flags differ in length")
        self._closed_bins = bins.n_bins_u * bins.n_bins_v
        self.ctx.check(self.lib.vo_mono_frame_enqueue_closed(
            self.ctx.handle, C.byref(self.prm), slots[0], slots[1], pts0.ctypes.data, Xw.ctypes.data, flags.ctypes.data,
            self._n, _f32(Tcw_prev).reshape(16).ctypes.data, _f32(Tcw_prior).reshape(16).ctypes.data,
            _f32(dT01_prior).reshape(16).ctypes.data, C.byref(bins), table, 0))

    def enqueue_closed_device(self, d_pts0, d_Xw, d_flags, n, Tcw_prev, Tcw_prior, dT01_prior, bins, table, slots=(0, 1)):
        self._n = n
        self._closed_bins = bins.n_bins_u * bins.n_bins_v
        self.ctx.check(self.lib.vo_mono_frame_enqueue_closed(
            self.ctx.handle, C.byref(self.prm), slots[0], slots[1], d_pts0, d_Xw, d_flags, n,
            _f32(Tcw_prev).reshape(16).ctypes.data, _f32(Tcw_prior).reshape(16).ctypes.data,
            _f32(dT01_prior).reshape(16).ctypes.data, C.byref(bins), table, 1))

    def result(self):
        n = self._n
        pts1 = np.zeros((max(n, 1), 2), np.float32)
        scale = np.zeros(max(n, 1), np.float32)
        stage = np.zeros(max(n, 1), np.uint8)
        dT = np.zeros(16, np.float32)
        cnt, gn = MonoCounts(), GnInfo()
        self.ctx.check(self.lib.vo_mono_frame_result(self.ctx.handle, _p(pts1), _p(scale), _p(stage, C.c_uint8),
                                                     _p(dT), C.byref(cnt), C.byref(gn)))
        out = dict(pts1=pts1[:n], scale=scale[:n], stage=stage[:n], dT01=dT.reshape(4, 4), counts=cnt, gn=gn)
        nb = getattr(self, "_closed_bins", 0)
        if nb:  # the new points of the closed frame: pixels in I1, back-tracked pixels in I0, masks
            self._closed_bins = 0
            p1n, p0n = np.zeros((nb, 2), np.float32), np.zeros((nb, 2), np.float32)
            mn, nn = np.zeros(nb, np.uint8), C.c_int()
            self.ctx.check(self.lib.vo_mono_frame_new_points(self.ctx.handle, p1n.ctypes.data, p0n.ctypes.data,
                                                             mn.ctypes.data, C.addressof(nn)))
            out.update(pts1_new=p1n[:nn.value], pts0_new=p0n[:nn.value], mask_new=mn[:nn.value].view(bool))
        return out


class Camera:
    """Camera (core/visual_odometry/camera.h:22-137): the distortion model, its image-undistortion map
    (generateImageUndistortMaps, camera.cpp:56-90) and undistortImage (camera.cpp:166-183). The map lives
    on the device (`cam` selects which of the context's two map sets); undistortImage delivers straight
    into an image slot's pyramid, including the driver's convertTo(CV_8UC1) (mono_vo.cpp:512)."""

    def __init__(self, ctx, cam=0):
        self.ctx, self.lib, self.cam = ctx, ctx.lib, cam
        self.initialized = False

    def initParams(self, n_cols, n_rows, K, D):
        self.n_cols, self.n_rows = int(n_cols), int(n_rows)
        self.K, self.D = _f32(K).reshape(4), _f32(D).reshape(5)  # fx fy cx cy ; k1 k2 p1 p2 k3
        self.ctx.check(self.lib.vo_rectify_init_mono(self.ctx.handle, self.cam, self.n_cols, self.n_rows, _p(self.K),
                                                     _p(self.D)))
        self.initialized = True

    def fx(self): return float(self.K[0])
    def fy(self): return float(self.K[1])
    def cx(self): return float(self.K[2])
    def cy(self): return float(self.K[3])

    def maps(self):
        return _get_maps(self.ctx, self.cam)

    def validityMask(self, erode=0):
        """Where the undistorted image shows the source (vo_rectify_validity_mask): 255 where every pixel within `erode`
        (0..31) samples inside the raw image, else 0 — an ignore mask for MonoVO.setMask."""
        return _validity_mask(self.ctx, self.cam, erode)

    def undistortImage(self, raw, slot):
        raw = self.ctx._format_image(raw)  # (an array of the context's input format: Context.set_input_format)
        if raw.size == 0 or raw.shape[:2] != (self.n_rows, self.n_cols):  # camera.cpp:168-169
            raise VoError(-4, "undistort image: provided image has not the same size as the camera model!")
        self.ctx.set_image_rectified(slot, raw, self.cam)


def _validity_mask(ctx, cam, erode):
    w, h = C.c_int(), C.c_int()
    ctx.check(ctx.lib.vo_rectify_get_maps(ctx.handle, cam, None, None, C.byref(w), C.byref(h)))
    out = np.zeros((h.value, w.value), np.uint8)
    ctx.check(ctx.lib.vo_rectify_validity_mask(ctx.handle, cam, int(erode), out.ctypes.data, out.strides[0], 0))
    return out


def _get_maps(ctx, cam):
    w, h = C.c_int(), C.c_int()
    ctx.check(ctx.lib.vo_rectify_get_maps(ctx.handle, cam, None, None, C.byref(w), C.byref(h)))
    mu = np.zeros((h.value, w.value), np.float32)
    mv = np.zeros((h.value, w.value), np.float32)
    ctx.check(ctx.lib.vo_rectify_get_maps(ctx.handle, cam, _p(mu), _p(mv), None, None))
    return mu, mv


class StereoCamera:
    """StereoCamera (core/visual_odometry/camera.h:140-195): setStereoPoseLeft2Right,
    initStereoCameraToRectify (generateStereoImagesUndistortAndRectifyMaps, camera.cpp:364-546),
    rectifyStereoImages (camera.cpp:300-336), the rectified camera and extrinsics."""

    def __init__(self, ctx):
        self.ctx, self.lib = ctx, ctx.lib
        self.is_initialized_to_stereo_rectify_ = False
        self.T_lr = np.eye(4, dtype=np.float32)

    def initParams(self, n_cols, n_rows, Kl, Dl, Kr, Dr):
        self.n_cols, self.n_rows = int(n_cols), int(n_rows)
        self.Kl, self.Dl = _f32(Kl).reshape(4), _f32(Dl).reshape(5)
        self.Kr, self.Dr = _f32(Kr).reshape(4), _f32(Dr).reshape(5)

    def setStereoPoseLeft2Right(self, T_lr):
        self.T_lr = _f32(T_lr).reshape(4, 4)

    def initStereoCameraToRectify(self):
        K_rect, T1, T2 = np.zeros(4, np.float32), np.zeros(16, np.float32), np.zeros(16, np.float32)
        self.ctx.check(self.lib.vo_rectify_init_stereo(
            self.ctx.handle, self.n_cols, self.n_rows, _p(self.Kl), _p(self.Dl), _p(self.Kr), _p(self.Dr),
            _p(_f32(self.T_lr).reshape(16)), _p(K_rect), _p(T1), _p(T2)))
        self.K_rect, self.T_lr_rect, self.T_rl_rect = K_rect, T1.reshape(4, 4), T2.reshape(4, 4)
        self.is_initialized_to_stereo_rectify_ = True

    def _need_init(self, where):
        if not self.is_initialized_to_stereo_rectify_:
            raise VoError(-1, f"In '{where}', is_initialized_to_stereo_rectify_ == false")

    def getRectifiedCamera(self):
        self._need_init("getRectifiedCamera()")
        return self.K_rect

    def getRectifiedStereoPoseLeft2Right(self):
        self._need_init("getRectifiedStereoPoseLeft2Right()")
        return self.T_lr_rect

    def getRectifiedStereoPoseRight2Left(self):
        self._need_init("getRectifiedStereoPoseRight2Left()")
        return self.T_rl_rect

    def maps(self):
        return _get_maps(self.ctx, 0), _get_maps(self.ctx, 1)

    def validityMask(self, erode=0, cam=0):
        """Where the rectified LEFT image (cam=1: the right one) shows the source (vo_rectify_validity_mask): 255 where every
        pixel within `erode` (0..31) samples inside the raw image, else 0 — an ignore mask for StereoVO.setMask."""
        self._need_init("validityMask()")
        return _validity_mask(self.ctx, cam, erode)

    def rectifyStereoImages(self, img_left, img_right, slot_l, slot_r):
        self._need_init("rectifyStereoImages()")
        for im in (img_left, img_right):  # camera.cpp:307, :324
            if np.asarray(im).shape[:2] != (self.n_rows, self.n_cols):
                raise VoError(-4, "In 'rectifyStereoImages()': provided image has not the same size as the camera model!")
        self.ctx.set_image_rectified(slot_l, img_left, 0)
        self.ctx.set_image_rectified(slot_r, img_right, 1)


class SparseBundleAdjustmentSolver:
    """SparseBundleAdjustmentSolver (core/visual_odometry/ba_solver/sparse_bundle_adjustment.h:42-158) on the
    device. The reference configures it through setCamera / setStereoCameras, setHuberThreshold and a
    SparseBAParameters object; here the same pieces of information arrive as arrays (see
    include/vo_hip.h, vo_sba_solve) — the landmark / keyframe graph that SparseBAParameters walks stays
    with the caller."""

    POSE_SCALE = 10.0  # SparseBAParameters::pose_scale_ (sparse_ba_parameters.h:255)

    def __init__(self, ctx, is_stereo=False):
        self.ctx, self.lib, self.is_stereo = ctx, ctx.lib, bool(is_stereo)
        self.Kl = self.Kr = None
        self.T_lr = np.eye(4)
        self.thres_huber = 0.0

    def setCamera(self, K):
        if self.is_stereo:
            raise VoError(-1, "In 'SparseBundleAdjustmentSolver::setCamera()': Before call this function, "
                              "'is_stereo' should be set to 'false'.")
        self.Kl = self.Kr = np.asarray(K, np.float64).reshape(4)

    def setStereoCameras(self, Kl, Kr, T_lr_scaled):
        if not self.is_stereo:
            raise VoError(-1, "In 'SparseBundleAdjustmentSolver::setStereoCameras()': Before call this function, "
                              "'is_stereo' should be set to 'true'.")
        self.Kl, self.Kr = np.asarray(Kl, np.float64).reshape(4), np.asarray(Kr, np.float64).reshape(4)
        self.T_lr = np.asarray(T_lr_scaled, np.float64).reshape(4, 4)

    def setHuberThreshold(self, thres_huber):
        self.thres_huber = float(thres_huber)

    def solveForFiniteIterations(self, MAX_ITER, T_jw, opt_index, X, obs_ptr, obs_frame, obs_right, obs_px):
        """Returns (flag_success, T_jw, X, avg_err); raises VoError where the reference throws (NaN)."""
        T = np.ascontiguousarray(T_jw, np.float64).reshape(-1, 16).copy()
        Xo = np.ascontiguousarray(X, np.float64).reshape(-1, 3).copy()
        opt_index = np.ascontiguousarray(opt_index, np.int32)
        obs_ptr, obs_frame = np.ascontiguousarray(obs_ptr, np.int32), np.ascontiguousarray(obs_frame, np.int32)
        obs_right, obs_px = np.ascontiguousarray(obs_right, np.uint8), np.ascontiguousarray(obs_px, np.float64).reshape(-1, 2)
        if obs_ptr.shape[0] != Xo.shape[0] + 1 or opt_index.shape[0] != T.shape[0]:
            raise ValueError("obs_ptr / opt_index do not match the number of landmarks / frames")
        if obs_frame.shape[0] != obs_px.shape[0] or obs_right.shape[0] != obs_px.shape[0]:
            raise ValueError("observation arrays differ in length")
        p = SbaProblem()
        p.n_frames, p.n_points, p.n_obs = T.shape[0], Xo.shape[0], obs_px.shape[0]
        p.n_opt = int(opt_index.max()) + 1 if opt_index.size else 0
        p.stereo, p.max_iter, p.thres_huber = int(self.is_stereo), int(MAX_ITER), self.thres_huber
        for k in range(4):
            p.Kl[k], p.Kr[k] = float(self.Kl[k]), float(self.Kr[k])
        for k in range(16):
            p.T_lr[k] = float(self.T_lr.reshape(16)[k])
        err = np.zeros(max(int(MAX_ITER), 1), np.float64)
        d, i32 = C.c_double, C.c_int32
        rc = self.ctx.check(self.lib.vo_sba_solve(self.ctx.handle, C.byref(p), _p(T, d), _p(opt_index, i32), _p(Xo, d),
                                                  _p(obs_ptr, i32), _p(obs_frame, i32), _p(obs_right, C.c_uint8),
                                                  _p(obs_px, d), _p(err, d)))
        return bool(rc), T.reshape(-1, 4, 4), Xo, err[: int(MAX_ITER)]


class FivePointRansac:
    """MotionEstimator::calcPose5PointsAlgorithm (motion_estimator.cpp:21-123): cv::findEssentialMat(..., RANSAC, confidence,
    thres_px) + the reference's SVD decomposition and chirality test, on the device (include/vo_hip.h: vo_five_point_*).
    `solver(pts0, pts1) -> (ok, R10, t10, mask)` is the hook shape MonoVO takes; a MonoVO given this object calls it natively.
    A child of the context: closed with it at the latest. The workspace is sized here (max_points: the context's by default,
    max_iters) and no call allocates."""

    def __init__(self, ctx, K, thres_px=2.0, confidence=0.999, max_iters=1000, seed=0, max_points=None):
        self.ctx, self.lib = ctx, ctx.lib
        self.K = _f32(K).reshape(4).copy()
        self.prm = FivePointParams(float(thres_px), float(confidence), int(max_iters), int(seed))
        self.thres_px = np.float32(thres_px)
        self.max_points = int(ctx.cfg.max_points if max_points is None else max_points)
        self._h = C.c_void_p()
        ctx.check(self.lib.vo_five_point_create(ctx.handle, C.byref(self.prm), self.max_points, C.byref(self._h)))
        ctx._children.add(self)

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vo_five_point_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def estimate(self, pts0, pts1, K=None):
        """(ok, R10 3x3, t10 (unit), mask (bool, n), info): info = vo_five_point_info (E10, n_inliers_5p, n_inliers, iterations,
        models, best_sample). ok is False where the reference has no pose; other errors raise VoError."""
        p0, p1 = _f32(pts0).reshape(-1, 2), _f32(pts1).reshape(-1, 2)
        if p0.shape[0] != p1.shape[0]:  # motion_estimator.cpp:27-28
            raise VoError(-4, "calcPose5PointsAlgorithm(): pts0.size() != pts1.size()")
        n = p0.shape[0]
        Kc = self.K if K is None else _f32(K).reshape(4)
        R, t = np.zeros(9, np.float32), np.zeros(3, np.float32)
        mask = np.zeros(max(n, 1), np.uint8)
        info = FivePointInfo()
        rc = self.lib.vo_five_point_pose(self._h, p0.ctypes.data, p1.ctypes.data, n, Kc.ctypes.data, R.ctypes.data, t.ctypes.data,
                                         mask.ctypes.data, C.byref(info))
        if rc == -9:  # VO_ERR_GN_FAILED: no pose
            return False, R.reshape(3, 3), t, np.zeros(n, bool), info
        self.ctx.check(rc)
        return True, R.reshape(3, 3), t, mask[:n].astype(bool), info

    def __call__(self, pts0, pts1):
        ok, R, t, mask, _ = self.estimate(pts0, pts1)
        return ok, R, t, mask

    def minimal(self, x0, x1):
        """The minimal solver alone (test hook): sets of five NORMALISED pairs (n_sets x 5 x 2 each) -> (E n_sets x 10 x 3 x 3,
        n_sol n_sets)."""
        x0 = np.ascontiguousarray(x0, np.float64).reshape(-1, 5, 2)
        x1 = np.ascontiguousarray(x1, np.float64).reshape(-1, 5, 2)
        m = x0.shape[0]
        E = np.zeros((max(m, 1), 10, 3, 3), np.float64)
        ns = np.zeros(max(m, 1), np.int32)
        self.ctx.check(self.lib.vo_five_point_minimal(self._h, x0.ctypes.data, x1.ctypes.data, m, E.ctypes.data, ns.ctypes.data))
        return E[:m], ns[:m]

    def samples(self):
        """Of the last call (test hook): dict(subsets (S x 5), n_models (S), best_count (S), counts (S x 10: every model's
        inlier count in solver order, -1 past the sample's models))."""
        S = C.c_int()
        self.ctx.check(self.lib.vo_five_point_samples(self._h, None, None, None, 0, C.addressof(S)))
        k = S.value
        sub, nm, bc = np.zeros((max(k, 1), 5), np.int32), np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.int32)
        cnt = np.full((max(k, 1), 10), -1, np.int32)
        if k:
            self.ctx.check(self.lib.vo_five_point_samples(self._h, sub.ctypes.data, nm.ctypes.data, bc.ctypes.data, k, C.addressof(S)))
            self.ctx.check(self.lib.vo_five_point_counts(self._h, cnt.ctypes.data, k, C.addressof(S)))
        return dict(subsets=sub[:k], n_models=nm[:k], best_count=bc[:k], counts=cnt[:k])


class MonoVO:
    """MonoVO (core/visual_odometry/mono_vo/mono_vo.h:235-243, :267): trackImage(img, timestamp) / getStatistics(), the track
    set, the keyframes and the mono local BA carried on the device (vo_mvo_*). `five_point` is MotionEstimator::
    calcPose5PointsAlgorithm, called for the second image and whenever the pose-only BA yields no pose: None (the default)
    builds the library's FivePointRansac(ctx, K, thres_px=thres_5p_error); a FivePointRansac is wired natively (no Python
    callback; this object keeps it alive); any other callable `(pts0, pts1) -> (ok, R10, t10, mask)` is called back."""

    def __init__(self, ctx, width, height, K, n_bins_u, n_bins_v, five_point=None, thres_fastscore=15, window_size=15, max_level=5,
                 thres_error=20.0, thres_bidirection=1.0, thres_poseba_error=5, thres_sampson=1.0, thres_parallax=1.0,
                 thres_overlap_ratio=0.7, thres_rotation=3.0, thres_translation=3.0, n_max_keyframes_in_window=9, strict_border=4,
                 local_ba=True, rectify=False, thres_5p_error=2.0, debug_image=False, pose_covariance=False, sigma_px=0.0,
                 mask=None, zncc_gate=None):
        """debug_image=True: every frame draws the reference's img_debug_ on the device (getDebugImage, getDebugPoints).
        zncc_gate: dict(thres=, win=15, pattern="centered") — the appearance gate of the steady-state frames (setZnccGate).
        pose_covariance=True: every frame chains the covariance of its pose on the device, in map units (getPoseCovariance);
        sigma_px > 0 scales by that pixel noise instead of the a-posteriori variance.
        mask: the ignore mask every image carries from the first one on (setMask)."""
        self.ctx, self.lib = ctx, ctx.lib
        self._own_fp = None
        if five_point is None:
            five_point = self._own_fp = FivePointRansac(ctx, K, thres_px=thres_5p_error)
        fe = FeatureExtractor(ctx)
        fe.initParams(width, height, n_bins_u, n_bins_v, THRES_FAST=thres_fastscore)
        p = MvoParams()
        p.frame = make_mono_params(width, height, window_size, max_level, thres_error, thres_bidirection, thres_poseba_error,
                                   thres_sampson, K)
        p.bins = fe.binParams()
        p.kf_overlap_ratio, p.kf_rotation_deg, p.kf_translation = thres_overlap_ratio, thres_rotation, thres_translation
        p.kf_window, p.thres_parallax_deg = n_max_keyframes_in_window, thres_parallax
        p.strict_border, p.local_ba, p.rectify = int(strict_border), int(bool(local_ba)), int(bool(rectify))
        self._user_hook = five_point

        def _hook(user, p0, p1, n, Kp, R10, t10, mask):
            a0 = np.ctypeslib.as_array(p0, shape=(max(n, 1), 2))[:n].copy()
            a1 = np.ctypeslib.as_array(p1, shape=(max(n, 1), 2))[:n].copy()
            try:
                ok, R, t, m = self._user_hook(a0, a1)
            except Exception:  # (an exception must not cross the C boundary: the call fails like the reference's throw)
                return 0
            if not ok:
                return 0
            np.ctypeslib.as_array(R10, shape=(9,))[:] = np.asarray(R, np.float32).reshape(9)
            np.ctypeslib.as_array(t10, shape=(3,))[:] = np.asarray(t, np.float32).reshape(3)
            if n:
                np.ctypeslib.as_array(mask, shape=(n,))[:] = np.asarray(m, bool).astype(np.uint8)
            return 1

        if isinstance(five_point, FivePointRansac):
            self._cb = None
            ctx.check(self.lib.vo_mvo_params_set_five_point(C.byref(p), five_point.handle))
        else:
            self._cb = FIVE_POINT_FN(_hook)  # (kept alive with the object)
            p.five_point = self._cb
            p.five_point_user = None
        self.prm, self.width, self.height = p, width, height
        self._h = C.c_void_p()
        try:
            ctx.check(self.lib.vo_mvo_create(ctx.handle, C.byref(p), C.byref(self._h)))
        except Exception:
            if self._own_fp is not None:
                self._own_fp.close()
            raise
        ctx._children.add(self)
        if debug_image:
            ctx.check(self.lib.vo_mvo_set_debug_image(self._h, 1))
        if pose_covariance:
            ctx.check(self.lib.vo_mvo_set_pose_covariance(self._h, 1, float(sigma_px)))
        if mask is not None:
            self.setMask(mask)
        if zncc_gate is not None:
            self.setZnccGate(zncc_gate)
        self._info = MvoFrameInfo()
        self.stats_frame = []

    @classmethod
    def from_yaml(cls, path, device=0, max_points=None, input_format="mono8", mask=None, mask_erode=0, equalize=None, zncc_gate=None,
                  **overrides):
        """MonoVO(mode = "rosbag", directory_intrinsic = path) of the reference (mono_vo.cpp:15-60, :137-225): the object
        configured by one of its config/mono/*.yaml files, with the library's 5-point solver at motion_estimator.
        thres_5p_error. The context is created here (sized by the file) and closed with the object. With flagDoUndistortion
        the images go through the camera's undistortion map (mono_vo.cpp:509-513). `overrides`: keyword arguments of the
        constructor (five_point, strict_border, local_ba, debug_image, ...). `max_points`: capacity of a track set (default
        2 * bins + 1024, as StereoVO.from_yaml). `input_format`: the images' pixel format (Context.set_input_format); anything but
        "mono8" needs flagDoUndistortion in the file. `mask`: an ignore mask (setMask), or "rectified": the camera's validity
        mask (Camera.validityMask(mask_erode)), which needs flagDoUndistortion in the file. `equalize`: None, "clahe" (OpenCV's
        defaults) or dict(clip_limit=, tiles=): Context.set_equalize on the new context. `zncc_gate`: the constructor's
        (setZnccGate)."""
        from . import config as _config
        cfg = _config.load_mono_config(path)
        eq = _equalize_arg(equalize)
        if isinstance(mask, str) and (mask != "rectified" or not cfg["flagDoUndistortion"]):
            raise ValueError('mask="rectified" is the only named mask, and it needs flagDoUndistortion in the file')
        cam = cfg["camera"]
        W, H = cam["width"], cam["height"]
        fe, ft, me, ku = cfg["feature_extractor"], cfg["feature_tracker"], cfg["motion_estimator"], cfg["keyframe_update"]
        cap = int(max_points) if max_points else 2 * fe["n_bins_u"] * fe["n_bins_v"] + 1024
        ctx = Context(device=device, max_width=W, max_height=H, max_points=cap, n_slots=3, max_level=max(ft["max_level"], 1))
        try:
            if input_format != "mono8":
                ctx.set_input_format(input_format)
            if eq is not None:
                ctx.set_equalize("clahe", **eq)
            if cfg["flagDoUndistortion"]:
                camera = Camera(ctx, 0)
                camera.initParams(W, H, cam["K"], cam["D"])
                if isinstance(mask, str):
                    mask = camera.validityMask(mask_erode)
            # (keys the file does not have keep the constructor's defaults: a 0 there is refused or meaningless — mono0.yaml
            # has no motion_estimator.* and no keyframe window)
            names = {"feature_extractor.thres_fastscore": ("thres_fastscore", fe["thres_fastscore"]),
                     "feature_tracker.window_size": ("window_size", ft["window_size"]),
                     "feature_tracker.max_level": ("max_level", ft["max_level"]),
                     "feature_tracker.thres_error": ("thres_error", ft["thres_error"]),
                     "feature_tracker.thres_bidirection": ("thres_bidirection", ft["thres_bidirection"]),
                     "feature_tracker.thres_sampson": ("thres_sampson", ft["thres_sampson"]),
                     "motion_estimator.thres_poseba_error": ("thres_poseba_error", int(me["thres_poseba_error"])),
                     "motion_estimator.thres_5p_error": ("thres_5p_error", me["thres_5p_error"]),
                     "map_update.thres_parallax": ("thres_parallax", cfg["map_update"]["thres_parallax"]),
                     "keyframe_update.thres_overlap_ratio": ("thres_overlap_ratio", ku["thres_overlap_ratio"]),
                     "keyframe_update.thres_rotation": ("thres_rotation", ku["thres_rotation"]),
                     "keyframe_update.thres_translation": ("thres_translation", ku["thres_translation"]),
                     "keyframe_update.n_max_keyframes_in_window": ("n_max_keyframes_in_window", ku["n_max_keyframes_in_window"])}
            kw = {arg: v for key, (arg, v) in names.items() if key not in cfg["missing"]}
            kw["rectify"] = bool(cfg["flagDoUndistortion"])
            kw["mask"] = mask
            kw["zncc_gate"] = zncc_gate
            kw.update(overrides)
            obj = cls(ctx, W, H, cam["K"], fe["n_bins_u"], fe["n_bins_v"], **kw)
        except Exception:
            ctx.close()
            raise
        obj._own_ctx, obj.config = ctx, cfg
        return obj

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vo_mvo_destroy(self._h)
            self._h = C.c_void_p()
        fp = getattr(self, "_own_fp", None)
        if fp is not None:
            self._own_fp = None
            fp.close()
        own = getattr(self, "_own_ctx", None)
        if own is not None:
            self._own_ctx = None
            own.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    _img, _nd = StereoVO._img, StereoVO._nd
    setMask = StereoVO.setMask  # (the mono image's mask; MonoVO's first two images and 5-point-fallback frames have no stage-4 gate:
                                # there it acts on the detection only)

    def _set_mask_fn(self):
        return self.lib.vo_mvo_set_mask

    def setZnccGate(self, gate):
        """StereoVO.setZnccGate for the mono stream: dict(thres=, win=15, pattern="centered"), the previous image at the
        feature's input pixel against the current image at its final pixel; None: off. pairs, if given, is ("temporal",). The
        first two images and a 5-point-fallback frame are host-driven and have no gate. Refused while a frame is in flight."""
        pairs, win, pattern, thres = _zncc_gate_arg(gate, False)
        self.ctx.check(self.lib.vo_mvo_set_zncc_gate(self._h, pairs, win, pattern, thres))

    def getZncc(self):
        """Inspection: float32 [n], the values the gate computed for the last steady-state frame, per INPUT feature."""
        n = C.c_int()
        self.ctx.check(self.lib.vo_mvo_get_zncc(self._h, None, 0, C.byref(n)))
        t = np.full(n.value, np.nan, np.float32)
        self.ctx.check(self.lib.vo_mvo_get_zncc(self._h, t.ctypes.data, n.value, C.byref(n)))
        return t

    def _ptr(self, img):
        if isinstance(img, np.ndarray):
            img = self._img(img)
            if img.ndim != self._nd():
                raise ValueError("the image must be one u8 plane")
            return img, img.ctypes.data, img.strides[0], 0
        return img, int(img[0]), int(img[1]), 1  # (device address, stride)

    def _out(self):
        self.stats_frame.append(np.array(self._info.T_wc, np.float32).reshape(4, 4))
        return MvoFrameInfo.from_buffer_copy(self._info)

    def trackImage(self, img, timestamp=0.0):
        a, p, st, dev = self._ptr(img)
        self._keep = a
        rc = self.lib.vo_mvo_track(self._h, p, st, dev, float(timestamp), self._info)
        if rc < 0:
            self.ctx.check(rc)
        return self._out()

    def enqueue(self, img, timestamp=0.0):
        a, p, st, dev = self._ptr(img)
        self._keep = a
        rc = self.lib.vo_mvo_enqueue(self._h, p, st, dev, float(timestamp))
        if rc < 0:
            self.ctx.check(rc)

    def prefetch(self, img):
        a, p, st, dev = self._ptr(img)
        self._keep_next = a
        rc = self.lib.vo_mvo_prefetch(self._h, p, st, dev)
        if rc < 0:
            self.ctx.check(rc)

    def result(self):
        rc = self.lib.vo_mvo_result(self._h, self._info)
        if rc < 0:
            self.ctx.check(rc)
        return self._out()

    def setPoseCovariance(self, on, sigma_px=0.0):
        """Switches the option (vo_mvo_set_pose_covariance); switching it on starts the chain at P = 0."""
        self.ctx.check(self.lib.vo_mvo_set_pose_covariance(self._h, int(bool(on)), float(sigma_px)))

    def getPoseCovariance(self):
        """PoseCovariance(P, Sigma_xi, s2, valid, n_points, n_unknown_steps) of the last frame (pose_covariance=True), in map
        units: waits for that frame's covariance launch only."""
        P, S = np.zeros((6, 6)), np.zeros((6, 6))
        s2, valid, n, unk = C.c_double(), C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.lib.vo_mvo_get_pose_covariance(self._h, P.ctypes.data, S.ctypes.data, C.addressof(s2), C.addressof(valid),
                                                           C.addressof(n), C.addressof(unk)))
        return PoseCovariance(P, S, s2.value, bool(valid.value), n.value, unk.value)

    def getPoseCovarianceRos(self):
        """The 36 doubles of nav_msgs::Odometry::pose.covariance for the last frame's pose (pose_covariance_ros)."""
        return pose_covariance_ros(self.getPoseCovariance().P, np.array(self._info.T_wc, np.float32).reshape(4, 4))

    def getPoseCovarianceInputs(self):
        """Test hook: what the last steady-state frame's covariance launch read: dict(X, pts, R01, t01)."""
        n, R, t = C.c_int(), np.zeros(9, np.float32), np.zeros(3, np.float32)
        self.ctx.check(self.lib.vo_mvo_get_pose_covariance_inputs(self._h, None, None, 0, C.addressof(n), R.ctypes.data, t.ctypes.data))
        m = max(n.value, 1)
        X, p = np.zeros((m, 3), np.float32), np.zeros((m, 2), np.float32)
        self.ctx.check(self.lib.vo_mvo_get_pose_covariance_inputs(self._h, X.ctypes.data, p.ctypes.data, m, C.addressof(n),
                                                                  R.ctypes.data, t.ctypes.data))
        k = n.value
        return dict(X=X[:k], pts=p[:k], R01=R.reshape(3, 3), t01=t)

    def runSequence(self, images, k_begin=0, k_end=None):
        """A recorded sequence of (device address, stride) images — or of numpy u8 images of one size and layout (host memory) —
        through the loop inside the library (vo_mvo_run): frames k_begin .. k_end - 1 are collected, frame k_end is left in
        flight. Returns (list of MvoFrameInfo, stamps)."""
        n = len(images)
        k_end = n if k_end is None else int(k_end)
        host = n > 0 and isinstance(images[0], np.ndarray)
        if host:
            if getattr(self, "_seq_ref", None) is not images or len(getattr(self, "_seq_host", ())) != n:
                self._seq_host = [self._img(I) for I in images]
                st0 = self._seq_host[0].strides[0]
                if any(a.ndim != self._nd() or a.shape != self._seq_host[0].shape or a.strides[0] != st0 for a in self._seq_host):
                    raise ValueError("runSequence: host images must be u8 planes of one size and row stride")
            src = [(a.ctypes.data, a.strides[0]) for a in self._seq_host]
        else:
            src = images
        I = getattr(self, "_seq_I", None)  # kept between calls on the same, unchanged list only (as StereoVO.runSequence)
        fresh = getattr(self, "_seq_ref", None) is not images or I is None or len(I) != n
        if not fresh:
            for k in range(max(int(k_begin), 0), min(k_end + 2, n)):
                if I[k] != int(src[k][0]):
                    fresh = True
                    break
        if fresh:
            self._seq_I = (C.c_void_p * n)(*[int(p[0]) for p in src])
            self._seq_ref = images
        self._seq_stride = int(src[0][1])
        m = k_end - int(k_begin)
        infos = (MvoFrameInfo * max(m, 1))()
        stamps = np.zeros(max(m, 1), np.float64)
        rc = self.lib.vo_mvo_run(self._h, self._seq_I, n, self._seq_stride, 0 if host else 1, int(k_begin), k_end, infos, stamps.ctypes.data)
        if rc < 0:
            self.ctx.check(rc)
        out = [MvoFrameInfo.from_buffer_copy(infos[j]) for j in range(m)]
        for i in out:
            self.stats_frame.append(np.array(i.T_wc, np.float32).reshape(4, 4))
        return out, stamps[:m]

    def getDebugImage(self):
        """img_debug_ of the last frame that drew one (debug_image=True): an (H, W, 3) uint8 array — published as bgr8 by the
        reference's node — or an empty (0, 0, 3) array before the first one and with the option off. A steady-state frame
        that took the 5-point fallback draws nothing, as in the reference: the previous picture stays."""
        w, h = C.c_int(), C.c_int()
        self.ctx.check(self.lib.vo_mvo_get_debug_image(self._h, None, 0, C.addressof(w), C.addressof(h)))
        out = np.zeros((h.value, w.value, 3), np.uint8)
        if out.size:
            self.ctx.check(self.lib.vo_mvo_get_debug_image(self._h, out.ctypes.data, out.strides[0], C.addressof(w), C.addressof(h)))
        return out

    def getDebugPoints(self):
        """What the last picture was drawn from (vo_mvo_get_debug_points): (kind, set0, set1, set2), (n, 2) float32 arrays.
        kind 0: none yet; 1: showTracking (pts0, pts1, pts_new); 2: showTrackingBA (pts1_ba, pts1_proj_ba, empty)."""
        kind, n = C.c_int(), (C.c_int * 3)()
        self.ctx.check(self.lib.vo_mvo_get_debug_points(self._h, C.addressof(kind), None, None, None, n, 0))
        cap = max(max(n), 1)
        sets = [np.zeros((cap, 2), np.float32) for _ in range(3)]
        self.ctx.check(self.lib.vo_mvo_get_debug_points(self._h, C.addressof(kind), sets[0].ctypes.data, sets[1].ctypes.data,
                                                        sets[2].ctypes.data, n, cap))
        return (kind.value,) + tuple(a[:n[k]].copy() for k, a in enumerate(sets))

    def getTracks(self):
        """frame_prev_'s related landmarks: dict(ids, pts, Xw, flags, age, cos_parallax)."""
        n = C.c_int()
        self.ctx.check(self.lib.vo_mvo_get_tracks(self._h, None, None, None, None, None, None, 0, C.addressof(n)))
        m = max(n.value, 1)
        ids, pts, X = np.zeros(m, np.int32), np.zeros((m, 2), np.float32), np.zeros((m, 3), np.float32)
        fl, age, cp = np.zeros(m, np.uint8), np.zeros(m, np.int32), np.zeros(m, np.float32)
        self.ctx.check(self.lib.vo_mvo_get_tracks(self._h, ids.ctypes.data, pts.ctypes.data, X.ctypes.data, fl.ctypes.data,
                                                  age.ctypes.data, cp.ctypes.data, m, C.addressof(n)))
        k = n.value
        return dict(ids=ids[:k], pts=pts[:k], Xw=X[:k], flags=fl[:k], age=age[:k], cos_parallax=cp[:k])

    def getKeyframes(self):
        """stats_keyframe (mono_vo.cpp:1130-1155): [(T_wc, mappoints)] of every keyframe so far, current values."""
        n, tot = C.c_int(), C.c_size_t()
        self.ctx.check(self.lib.vo_mvo_keyframe_count(self._h, C.addressof(n)))
        nk = n.value
        if nk == 0:
            return []
        T, cnt = np.zeros((nk, 16), np.float32), np.zeros(nk, np.int32)
        self.ctx.check(self.lib.vo_mvo_get_keyframes(self._h, T.ctypes.data, cnt.ctypes.data, None, 0, C.addressof(tot)))
        X = np.zeros((max(tot.value, 1), 3), np.float32)
        if tot.value:
            self.ctx.check(self.lib.vo_mvo_get_keyframes(self._h, None, None, X.ctypes.data, tot.value, C.addressof(tot)))
        off = np.concatenate([[0], np.cumsum(cnt)])
        return [(T[j].reshape(4, 4).copy(), X[off[j]:off[j + 1]].copy()) for j in range(nk)]

    def getStatistics(self):
        """AlgorithmStatistics: stats_frame (pose per frame as it was when the frame returned)."""
        return dict(stats_frame=list(self.stats_frame))

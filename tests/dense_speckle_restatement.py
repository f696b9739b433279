"""The speckle filter for disparity planes (include/vo_hip.h, "Speckle filter"), restated in numpy and plain Python from
the definition and from nothing else: the connected components of the valid pixels under 4-neighbour joins with |Δd| <= max_diff in
float32, labelled by their smallest raster index, found by a breadth-first search; the components of at most max_size pixels removed."""
import collections

import numpy as np

DEFAULTS = dict(max_size=100, max_diff=1.0)
SPECKLE = 6  # VO_DISPARITY_SPECKLE


def joins(disparity, status, max_diff):
    """(right, down): right[y, x] — (x, y) and (x + 1, y) are joined; down[y, x] — (x, y) and (x, y + 1)"""
    d = np.asarray(disparity, np.float32)
    valid = np.asarray(status) == 1
    md = np.float32(max_diff)
    right, down = np.zeros(d.shape, bool), np.zeros(d.shape, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        right[:, :-1] = valid[:, :-1] & valid[:, 1:] & (np.abs(d[:, :-1] - d[:, 1:]) <= md)  # (a NaN compares false)
        down[:-1, :] = valid[:-1, :] & valid[1:, :] & (np.abs(d[:-1, :] - d[1:, :]) <= md)
    return right, down


def speckle_filter(disparity, sigma_invd, status, **params):
    """-> dict: label, size int32 (h, w) (-1 and 0 on invalid pixels; the components before the removal), the filtered disparity,
    sigma_invd (None where None was given) and status, n_removed, n_components. The inputs are not changed."""
    p = dict(DEFAULTS, **params)
    max_size, max_diff = int(p["max_size"]), float(np.float32(p["max_diff"]))
    assert max_size >= 0 and max_diff >= 0 and np.isfinite(max_diff)
    disparity, status = np.array(disparity, np.float32), np.array(status, np.uint8)
    sigma_invd = None if sigma_invd is None else np.array(sigma_invd, np.float32)
    h, w = status.shape
    right, down = joins(disparity, status, max_diff)
    right, down = right.ravel().tolist(), down.ravel().tolist()
    valid = (status == 1).ravel().tolist()
    label, size = np.full(h * w, -1, np.int32), np.zeros(h * w, np.int32)
    seen = [False] * (h * w)
    n_components = 0
    for start in range(h * w):  # raster order: a component's first pixel met is its smallest raster index
        if not valid[start] or seen[start]:
            continue
        n_components += 1
        seen[start] = True
        members, queue = [start], collections.deque([start])
        while queue:
            i = queue.popleft()
            x = i % w
            near = []
            if x + 1 < w and right[i]:
                near.append(i + 1)
            if x > 0 and right[i - 1]:
                near.append(i - 1)
            if i + w < h * w and down[i]:
                near.append(i + w)
            if i >= w and down[i - w]:
                near.append(i - w)
            for j in near:
                if not seen[j]:
                    seen[j] = True
                    members.append(j)
                    queue.append(j)
        label[members] = start
        size[members] = len(members)
    label, size = label.reshape(h, w), size.reshape(h, w)
    gone = (label >= 0) & (size <= max_size)
    status[gone] = SPECKLE
    disparity[gone] = 0
    if sigma_invd is not None:
        sigma_invd[gone] = 0
    return dict(label=label, size=size, disparity=disparity, sigma_invd=sigma_invd, status=status, n_removed=int(gone.sum()),
                n_components=n_components)

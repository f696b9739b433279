"""The propagation kernels (csrc/semidense_propagate.hip) run on the side stream next to a frame in flight: they satisfy the
co-residency bound of the side-chain kernels (tests/test_kernel_resources_semidense.py: (lanes / 256) x allocated VGPRs <= 236),
keep everything in registers — no scratch, no spills — and use no LDS (one lane per pixel, nothing shared). hipcc cross-compiles
for gfx950 without a GPU; device code only."""
import os

import pytest

from visual_odometry_ros_amd import build as B
from test_kernel_resources_semidense_temporal import KEYS, _usage

KERNELS = (("semidense_propagate_scatter_kernel", 256), ("semidense_propagate_resolve_kernel", 256))


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_semidense_propagate_kernels_fit_next_to_the_replay_pool():
    res = _usage("semidense_propagate.hip")
    for k, lanes in KERNELS:
        hit = [v for n, v in res.items() if k in n]
        assert hit, (k, sorted(res))
        for v in hit:
            assert set(KEYS) <= set(v), (k, v)
            vgprs = (v["VGPRs"] + 7) // 8 * 8
            per_simd = (lanes // 256 if lanes >= 256 else 1) * vgprs
            print(k, v)
            assert per_simd <= 236 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, lanes, v)
            assert v["LDS Size [bytes/block]"] == 0, (k, v)

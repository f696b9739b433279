"""The dense stereo kernels (csrc/dense_stereo.hip) run on the side stream next to a frame in flight: they have to satisfy the
co-residency bound of the side-chain kernels (tests/test_kernel_resources.py: (lanes / 256) x allocated VGPRs <= 236) and keep
everything in registers — no scratch, no spills — for every number of disparities per lane. hipcc cross-compiles for gfx950 without a
GPU; device code only."""
import os

import pytest

from test_kernel_resources import _usage
from visual_odometry_ros_amd import build as B

# name, lanes per workgroup, instances (the aggregation and the decision once per 1..4 disparities a lane)
KERNELS = (("dense_census_kernel", 256, 1), ("dense_aggregate_kernel", 256, 4), ("dense_decide_kernel", 256, 4))


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_dense_stereo_kernels_fit_next_to_the_replay_pool():
    res = _usage("dense_stereo.hip")
    for k, lanes, instances in KERNELS:
        hit = [v for n, v in res.items() if k in n]
        assert len(hit) == instances, (k, sorted(res))
        for v in hit:
            per_simd = (lanes // 256 if lanes >= 256 else 1) * ((v["VGPRs"] + 7) // 8 * 8)
            assert per_simd <= 236 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, lanes, v)

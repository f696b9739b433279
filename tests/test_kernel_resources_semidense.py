"""The semi-dense stereo kernel (csrc/semidense.hip) runs on the side stream next to a frame in flight: it has to satisfy the
co-residency bound of the side-chain kernels (tests/test_kernel_resources.py: (lanes / 256) x allocated VGPRs <= 236) and keeps
everything in registers — no scratch, no spills. hipcc cross-compiles for gfx950 without a GPU; device code only."""
import os

import pytest

from test_kernel_resources import _usage
from visual_odometry_ros_amd import build as B

KERNELS = (("semidense_kernel", 256), ("semidense_points_kernel", 256), ("semidense_key_kernel", 256))


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_semidense_kernels_fit_next_to_the_replay_pool():
    res = _usage("semidense.hip")
    for k, lanes in KERNELS:
        hit = [v for n, v in res.items() if k in n]
        assert hit, (k, sorted(res))
        for v in hit:
            per_simd = (lanes // 256 if lanes >= 256 else 1) * ((v["VGPRs"] + 7) // 8 * 8)
            assert per_simd <= 236 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, lanes, v)

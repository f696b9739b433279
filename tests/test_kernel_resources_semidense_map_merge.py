"""The map merge's kernel (csrc/semidense_map_merge.hip) runs on the side stream next to a frame in flight, in front of the world map's
integration: it has to satisfy the co-residency bound of the side-chain kernels (tests/test_kernel_resources_dense_stereo.py: (lanes /
256) x allocated VGPRs <= 236) and keep everything in registers — no scratch, no spills. hipcc cross-compiles for gfx950 without a GPU;
device code only."""
import os

import pytest

from test_kernel_resources import _usage
from visual_odometry_ros_amd import build as B

KERNELS = ("semidense_map_merge_kernel",)  # 256 lanes


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_semidense_map_merge_kernel_fits_next_to_the_replay_pool():
    res = _usage("semidense_map_merge.hip")
    for k in KERNELS:
        hit = [v for n, v in res.items() if k in n]
        assert len(hit) == 1, (k, sorted(res))
        v = hit[0]
        per_simd = (v["VGPRs"] + 7) // 8 * 8
        assert per_simd <= 236 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, v)

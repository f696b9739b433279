"""The speckle filter's kernels (csrc/dense_speckle.hip) run on the side stream next to a frame in flight, behind the dense decision:
they have to satisfy the co-residency bound of the side-chain kernels (tests/test_kernel_resources_dense_stereo.py: (lanes / 256) x
allocated VGPRs <= 236) and keep everything in registers — no scratch, no spills. hipcc cross-compiles for gfx950 without a GPU;
device code only."""
import os

import pytest

from test_kernel_resources import _usage
from visual_odometry_ros_amd import build as B

KERNELS = ("speckle_local_kernel", "speckle_merge_kernel", "speckle_flatten_kernel", "speckle_apply_kernel")  # 256 lanes each


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_dense_speckle_kernels_fit_next_to_the_replay_pool():
    res = _usage("dense_speckle.hip")
    for k in KERNELS:
        hit = [v for n, v in res.items() if k in n]
        assert len(hit) == 1, (k, sorted(res))
        v = hit[0]
        per_simd = (v["VGPRs"] + 7) // 8 * 8
        assert per_simd <= 236 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, v)

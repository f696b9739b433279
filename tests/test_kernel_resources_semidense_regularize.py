"""The regularisation kernel (csrc/semidense_regularize.hip) runs on the side stream next to a frame in flight: it satisfies the
co-residency bound of the side-chain kernels (tests/test_kernel_resources_semidense.py: (lanes / 256) x allocated VGPRs <= 236),
keeps everything in registers — no scratch, no spills — and its static LDS is the figure DESIGN.md §23 states: the staged region of
(64 + 12) x (8 + 12) cells at three floats and two flag bytes each, the work list of (64 + 6) x (8 + 6) 16-bit cell indices and its two
counters, 23 248 bytes, below the 40 KB the side chain allows itself (the affine alignment kernel's 37 272 bytes is its largest). hipcc cross-compiles for gfx950 without a GPU; device code only."""
import os

import pytest

from visual_odometry_ros_amd import build as B
from test_kernel_resources_semidense_temporal import KEYS, _usage

KERNELS = (("semidense_regularize_kernel", 256),)
LDS_BYTES = (64 + 12) * (8 + 12) * (3 * 4 + 2) + (64 + 6) * (8 + 6) * 2 + 2 * 4


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_semidense_regularize_kernel_fits_next_to_the_replay_pool():
    res = _usage("semidense_regularize.hip")
    assert LDS_BYTES == 23248
    for k, lanes in KERNELS:
        hit = [v for n, v in res.items() if k in n]
        assert hit, (k, sorted(res))
        for v in hit:
            assert set(KEYS) <= set(v), (k, v)
            vgprs = (v["VGPRs"] + 7) // 8 * 8
            per_simd = (lanes // 256 if lanes >= 256 else 1) * vgprs
            print(k, v)
            assert per_simd <= 236 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, lanes, v)
            assert v["LDS Size [bytes/block]"] == LDS_BYTES <= 40 * 1024, (k, v)

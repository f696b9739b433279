"""The kernels of the coarse-to-fine alignment (csrc/semidense_align.hip) run on the side stream next to a frame in flight: the new
map pyramid kernel and the alignment kernel with its level bookkeeping (the pose source of a level's first launch, the per-level
record) satisfy the co-residency bound of the side-chain kernels (tests/test_kernel_resources_semidense.py: (lanes / 256) x allocated
VGPRs <= 236) and keep everything in registers — no scratch, no spills. The map pyramid kernel uses no LDS at all (one coarse pixel
per thread, nine children in registers); the alignment kernel's static LDS stays what DESIGN.md §20 states, at most 37 KB. The
figures are printed (DESIGN.md §21 records them). hipcc cross-compiles for gfx950 without a GPU; device code only."""
import os

import pytest

from visual_odometry_ros_amd import build as B
from test_kernel_resources_semidense_align import LDS_ARRAYS
from test_kernel_resources_semidense_temporal import CU_LDS, KEYS, _usage

KERNELS = (("semidense_map_pyramid_kernel", 256), ("semidense_align_kernel", 256))


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_semidense_align_pyr_kernels_fit_next_to_the_replay_pool():
    res = _usage("semidense_align.hip")
    for k, lanes in KERNELS:
        hit = [v for n, v in res.items() if k in n]
        assert len(hit) == 1, (k, sorted(res))
        v = hit[0]
        assert set(KEYS) <= set(v), (k, v)
        vgprs = (v["VGPRs"] + 7) // 8 * 8
        per_simd = (lanes // 256 if lanes >= 256 else 1) * vgprs
        print(k, v)
        assert per_simd <= 236 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, lanes, v)
        lds = v["LDS Size [bytes/block]"]
        if k == "semidense_map_pyramid_kernel":
            assert lds == 0 and vgprs <= 64, v  # (a streaming kernel: eight waves per SIMD)
        else:
            assert LDS_ARRAYS <= lds <= 37 * 1024 and CU_LDS // lds >= 4, v

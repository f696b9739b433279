"""The alignment kernel (csrc/semidense_align.hip) runs on the side stream next to a frame in flight: it satisfies the co-residency
bound of the side-chain kernels (tests/test_kernel_resources_semidense.py: (lanes / 256) x allocated VGPRs <= 236) and keeps
everything in registers — no scratch, no spills: the 6 x 6 solve of the last workgroup's thread 0 included, whose loops all unroll.
Its static LDS is what DESIGN.md §20 states: the records' 32 KB (which the last workgroup reuses for the staged rows), the list's
2 KB, the eight parts' 2 KB and a few words — at most 37 KB, four workgroups per compute unit (160 KB of LDS). hipcc cross-compiles
for gfx950 without a GPU; device code only."""
import os

import pytest

from visual_odometry_ros_amd import build as B
from test_kernel_resources_semidense_temporal import CU_LDS, KEYS, _usage

KERNELS = (("semidense_align_kernel", 256),)
LDS_ARRAYS = 8 * 1024 * 4 + 1024 * 2 + 8 * 32 * 8 + 4 * 4 + 4 + 32 * 8  # records, list, parts, wave counts, the "last" word, the 30 sums


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_semidense_align_kernel_fits_next_to_the_replay_pool():
    res = _usage("semidense_align.hip")
    for k, lanes in KERNELS:
        hit = [v for n, v in res.items() if k in n]
        assert hit, (k, sorted(res))
        for v in hit:
            assert set(KEYS) <= set(v), (k, v)
            vgprs = (v["VGPRs"] + 7) // 8 * 8
            per_simd = (lanes // 256 if lanes >= 256 else 1) * vgprs
            print(k, v)
            assert per_simd <= 236 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, lanes, v)
            lds = v["LDS Size [bytes/block]"]
            assert LDS_ARRAYS <= lds <= 37 * 1024, v
            assert CU_LDS // lds >= 4, lds

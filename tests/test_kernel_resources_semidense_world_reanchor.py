"""The world map's removal kernel (csrc/semidense_world.hip) runs on the side stream next to a frame in flight, like the integration it
undoes: it satisfies the co-residency bound of the side-chain kernels (tests/test_kernel_resources_semidense.py: (lanes / 256) x
allocated VGPRs <= 236) and keeps everything in registers — no scratch, no spills. LDS: the list of the block's entries, the counters
and the workgroup's hash of 512 slots of six 64-bit words and a count (SDW_LDS_BYTES_REMOVE). The vacant count, off the hot path, one
word. hipcc cross-compiles for gfx950 without a GPU; device code only."""
import os

import pytest

from visual_odometry_ros_amd import build as B
from test_kernel_resources_semidense_temporal import KEYS, _usage

SDW_BLOCK, SDW_LH = 1024, 512
# kernel (a part of its mangled name) -> lanes, LDS bytes
KERNELS = (("semidense_world_remove_kernel", 256, SDW_BLOCK * 2 + 4 * 4 + SDW_LH * (6 * 8 + 4)), ("semidense_world_vacant_kernel", 256, 4))


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_semidense_world_removal_fits_next_to_the_replay_pool():
    res = _usage("semidense_world.hip")
    for k, lanes, lds in KERNELS:
        hit = [v for n, v in res.items() if k in n]
        assert len(hit) == 1, (k, sorted(res))
        for v in hit:
            assert set(KEYS) <= set(v), (k, v)
            vgprs = (v["VGPRs"] + 7) // 8 * 8
            per_simd = (lanes // 256 if lanes >= 256 else 1) * vgprs
            print(k, v)
            assert per_simd <= 236 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, lanes, v)
            assert v["LDS Size [bytes/block]"] == lds, (k, v)

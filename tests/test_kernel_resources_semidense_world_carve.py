"""The world map's carve kernel (csrc/semidense_world_carve_device.hpp, launched from csrc/semidense_world.hip) runs on the side
stream next to a frame in flight, directly behind the integration: both forms satisfy the co-residency bound of the side-chain
kernels (tests/test_kernel_resources_semidense.py: (lanes / 256) x allocated VGPRs <= 236) and keep everything in registers — no
scratch, no spills. LDS: the list of the block's entries, three floats per ray and the counters (SDWC_LDS_BYTES_SIMPLE), plus the
workgroup's hash of 512 slots of a key and a count (SDWC_LDS_BYTES_AGG) — the constants the header declares, read from it here. The
free extraction, off the hot path, two words. hipcc cross-compiles for gfx950 without a GPU; device code only."""
import os
import re

import pytest

from visual_odometry_ros_amd import build as B
from test_kernel_resources_semidense_temporal import KEYS, _usage


def _header_constants():
    """the #defines of the two device headers, evaluated: the LDS bytes the carve header declares"""
    env = {}
    for name in ("semidense_world_device.hpp", "semidense_world_carve_device.hpp"):
        with open(os.path.join(B.CSRC, name)) as f:
            for m in re.finditer(r"^#define (SDWC?_[A-Z_]+) (\(.*?\)|\d+)\s*(?://.*)?$", f.read(), re.M):
                env[m.group(1)] = eval(m.group(2), {}, env)
    return env


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_semidense_world_carve_fits_next_to_the_replay_pool():
    c = _header_constants()
    assert c["SDWC_LDS_BYTES_SIMPLE"] == 1024 * 14 + 28 and c["SDWC_LDS_BYTES_AGG"] == c["SDWC_LDS_BYTES_SIMPLE"] + 4 + 512 * 12
    # kernel (a part of its mangled name) -> lanes, LDS bytes
    kernels = (("semidense_world_carve_kernelILb0E", 256, c["SDWC_LDS_BYTES_SIMPLE"]), ("semidense_world_carve_kernelILb1E", 256, c["SDWC_LDS_BYTES_AGG"]),
               ("semidense_world_extract_free_kernel", 256, 8))
    res = _usage("semidense_world.hip")
    for k, lanes, lds in kernels:
        hit = [v for n, v in res.items() if k in n]
        assert len(hit) == 1, (k, sorted(res))
        for v in hit:
            assert set(KEYS) <= set(v), (k, v)
            vgprs = (v["VGPRs"] + 7) // 8 * 8
            per_simd = (lanes // 256 if lanes >= 256 else 1) * vgprs
            print(k, v)
            assert per_simd <= 236 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, lanes, v)
            assert v["LDS Size [bytes/block]"] == lds, (k, v)

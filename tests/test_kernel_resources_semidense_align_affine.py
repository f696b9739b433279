"""The kernel of the alignment with affine brightness (csrc/semidense_align.hip: semidense_affine_kernel) runs where the alignment's
launches run, on the side stream next to a frame in flight: it satisfies the co-residency bound of the side-chain kernels
(tests/test_kernel_resources_semidense.py: (lanes / 256) x allocated VGPRs <= 236) and keeps everything in registers — no scratch, no
spills: the 8 x 8 solve of the last workgroup's thread 0 included, whose loops all unroll. Its static LDS: the records' 32 KB (eight
words per listed pixel still: the key's grey level rides in the weight word; the last workgroup reuses them for 85 staged rows of 48
doubles), the list's 2 KB, the four parts' 2 KB, the 48 sums and a few words — at most 37 KB, four workgroups per compute unit (160 KB
of LDS). The existing alignment kernel is still found exactly once under its name, which the new kernel's name does not contain.
The figures are printed (DESIGN.md §22 records them). hipcc cross-compiles for gfx950 without a GPU; device code only."""
import os

import pytest

from visual_odometry_ros_amd import build as B
from test_kernel_resources_semidense_temporal import CU_LDS, KEYS, _usage

KERNEL, LANES = "semidense_affine_kernel", 256
LDS_ARRAYS = 8 * 1024 * 4 + 1024 * 2 + 4 * 64 * 8 + 4 * 4 + 4 + 48 * 8  # records, list, parts, wave counts, the "last" word, the sums


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_semidense_affine_kernel_fits_next_to_the_replay_pool():
    res = _usage("semidense_align.hip")
    assert len([n for n in res if "semidense_align_kernel" in n]) == 1, sorted(res)  # the existing kernel, once
    hit = [v for n, v in res.items() if KERNEL in n]
    assert len(hit) == 1 and "semidense_align_kernel" not in KERNEL, sorted(res)
    v = hit[0]
    assert set(KEYS) <= set(v), v
    vgprs = (v["VGPRs"] + 7) // 8 * 8
    print(KERNEL, v)
    assert (LANES // 256) * vgprs <= 236 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, v
    lds = v["LDS Size [bytes/block]"]
    assert LDS_ARRAYS <= lds <= 37 * 1024 and CU_LDS // lds >= 4, v

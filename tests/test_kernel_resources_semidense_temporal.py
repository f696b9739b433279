"""The temporal semi-dense kernels (csrc/semidense_temporal.hip) run on the side stream next to a frame in flight: they satisfy
the co-residency bound of the side-chain kernels (tests/test_kernel_resources_semidense.py: (lanes / 256) x allocated VGPRs <=
236), keep everything in registers — no scratch, no spills — and the search kernel's static LDS is what DESIGN.md §18 states: the
17 556 bytes of its arrays plus the compiler's alignment padding, at most 18 KB, which admits more workgroups per compute unit (160 KB of LDS) than its registers do: LDS is not what limits
the 7 wavefronts per SIMD §18 claims. hipcc cross-compiles for gfx950 without a GPU; device code only."""
import os
import re
import subprocess

import pytest

from visual_odometry_ros_amd import build as B

KERNELS = (("semidense_temporal_kernel", 256), ("semidense_map_seed_kernel", 256), ("semidense_map_key_kernel", 256))
KEYS = ("ScratchSize [bytes/lane]", "VGPRs Spill", "VGPRs", "LDS Size [bytes/block]")
CU_LDS = 160 * 1024
SIMD_VGPRS = 512           # per lane; a wavefront's allocation is rounded up to 8
WAVES_PER_SIMD_CLAIMED = 7  # DESIGN.md §18 (the hardware's ceiling is 8)
LDS_ARRAYS = 17556          # s_geo 1536 + s_npos 256 + s_bcol 264 + s_slot_col 64 + s_slot_off 68 + three counters 12
                            # + s_key 16 x 224 x 2 = 7168 + s_sc 2048 x 4 = 8192


def _usage(src):
    """kernel -> the resources hipcc reports for it (test_kernel_resources._usage, with the LDS size as well)"""
    flags = [f for f in B.FLAGS if f not in ("-Wall", "-Wno-unused-function")]
    cmd = [B.HIPCC] + flags + ["-I" + os.path.join(os.path.dirname(B.HERE), "include"), "-I" + B.CSRC, "--offload-device-only",
                               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, src), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key in KEYS:
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                out[name].setdefault(key, int(m.group(1)))
    return out


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_semidense_temporal_kernels_fit_next_to_the_replay_pool():
    res = _usage("semidense_temporal.hip")
    for k, lanes in KERNELS:
        hit = [v for n, v in res.items() if k in n]
        assert hit, (k, sorted(res))
        for v in hit:
            assert set(KEYS) <= set(v), (k, v)
            vgprs = (v["VGPRs"] + 7) // 8 * 8
            per_simd = (lanes // 256 if lanes >= 256 else 1) * vgprs
            assert per_simd <= 236 and v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, lanes, v)
            lds = v["LDS Size [bytes/block]"]
            if k != "semidense_temporal_kernel":
                assert lds == 0, (k, v)
                continue
            assert LDS_ARRAYS <= lds <= 18 * 1024, v  # (the arrays, padded to their alignments: 18 KB is the figure §18 states)
            # a 256-thread workgroup puts one wavefront on each SIMD: workgroups per compute unit = wavefronts per SIMD
            by_registers = min(8, SIMD_VGPRS // vgprs)
            by_lds = CU_LDS // lds
            assert by_registers >= WAVES_PER_SIMD_CLAIMED, (vgprs, by_registers)
            assert by_lds >= 8 >= by_registers, (lds, by_lds)  # LDS admits the hardware's ceiling: it never limits co-residency

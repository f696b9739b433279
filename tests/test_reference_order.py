"""The reference summation order without a GPU: its C ABI is declared and exported, and the kernels of the ordered sums keep
everything in registers, like their tree-order instantiations, with the one exception listed in ALLOWED."""
import ctypes as C
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from visual_odometry_ros_amd import _capi
from visual_odometry_ros_amd import build as B

HEADER = os.path.join(os.path.dirname(B.HERE), "include", "vo_hip.h")

ORDERED = {
    # mangled-name prefixes of the instantiations with ORD = true
    "gn_pose.hip": ("gn_pose_kernelILb1ELb1E", "gn_pose_kernelILb0ELb1E"),
    "ic_refine.hip": ("ic_refine_kernelILb1E", "ic_jacobi_kernelILb1E", "ic_strict_kernelILb1E"),
    "frame_fused.hip": tuple(f"frame_{k}_kernelILi{w}ELb1E" for k in ("track", "replay", "fallback") for w in (13, 15, 21, 31)),
    "frame_mono.hip": tuple(f"mono_track_kernelILi{w}ELb1E" for w in (13, 15, 21, 31)) + ("mono_replay_kernelILb1E",
                                                                                          "mono_fallback_kernelILb1E"),
}
# The one exception: window 31's frame kernel (no configuration of the reference uses it) sits at its 256-register cap in
# both orders, and the ordered sums push two registers of its KLT part to scratch (12 bytes per lane; its tree twin: none).
ALLOWED = {"frame_track_kernelILi31ELb1E": (12, 2)}  # (scratch bytes per lane, spilled VGPRs) at most


def test_sum_order_in_the_abi():
    text = open(HEADER).read()
    assert re.search(r"VO_SUM_ORDER_TREE\s*=\s*0", text) and re.search(r"VO_SUM_ORDER_REFERENCE\s*=\s*1", text)
    assert "int vo_set_sum_order(vo_ctx *ctx, int order);" in text
    assert "int vo_get_sum_order(const vo_ctx *ctx);" in text
    assert re.search(r"#define VO_HIP_ABI_VERSION 3\b", text)  # adding functions is backward compatible
    assert {"vo_set_sum_order", "vo_get_sum_order"} <= set(_capi.SYMBOLS)


@pytest.mark.skipif(not os.path.exists(_capi.LIB_PATH), reason="library not built")
def test_sum_order_without_a_context():
    lib = C.CDLL(_capi.LIB_PATH)
    lib.vo_set_sum_order.argtypes = [C.c_void_p, C.c_int]
    lib.vo_get_sum_order.argtypes = [C.c_void_p]
    assert lib.vo_set_sum_order(None, 1) == -1 and lib.vo_get_sum_order(None) == -1


def _usage(src):
    flags = [f for f in B.FLAGS if f not in ("-Wall", "-Wno-unused-function")]
    cmd = [B.HIPCC] + flags + ["-I" + os.path.dirname(HEADER), "-I" + B.CSRC, "--offload-device-only",
                               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, src), "-o", os.devnull]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        for key in ("ScratchSize [bytes/lane]", "VGPRs Spill", "VGPRs"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                out[name].setdefault(key, int(m.group(1)))
    return out


@pytest.mark.skipif(not os.path.exists(B.HIPCC), reason="no hipcc")
def test_ordered_kernels_use_no_scratch_memory():
    with ThreadPoolExecutor(4) as ex:
        res = dict(zip(ORDERED, ex.map(_usage, ORDERED)))
    for src, kernels in ORDERED.items():
        for k in kernels:
            hit = [v for n, v in res[src].items() if k in n]
            assert hit, (src, k, sorted(res[src]))
            scratch, spill = ALLOWED.get(k, (0, 0))
            for v in hit:
                assert v["ScratchSize [bytes/lane]"] <= scratch and v["VGPRs Spill"] <= spill, (src, k, v)


def test_the_batch_has_no_sum_order():
    """vo_batch streams stay in tree order: StereoBatch has no sum_order (its handle is not a vo_ctx)."""
    from visual_odometry_ros_amd.api import StereoBatch
    assert not hasattr(StereoBatch, "sum_order")

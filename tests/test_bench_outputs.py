"""bench.py --dump-outputs on CPU: the helpers that turn what the timed path hands its caller (frame records, result dicts)
into DIR/<name>.npy files — float32 or float64 holding the values exactly, 64 MB at most."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from visual_odometry_ros_amd import _capi  # noqa: E402


def _frame_record():
    i = _capi.SvoFrameInfo()
    i.frame_id, i.is_keyframe, i.n_final = 77, 1, 1234
    i.counts.n_l0l1, i.gn.err = 1500, 0.125
    for k in range(16):
        i.T_wc[k] = np.float32(k) / 3
    return i


def test_frame_record_flattens_in_declaration_order():
    v = bench.struct_values(_frame_record())
    assert v[0] == 77 and v[2] == 1 and 1234 in v and 1500 in v and 0.125 in v
    assert len(v) == 10 + 8 + 6 + 16 + 16 + 4  # scalars, FrameCounts, GnInfo, dT, T_wc, local-BA fields


def test_loop_outputs_and_dtypes(tmp_path):
    traj = [np.eye(4, dtype=np.float32) * k for k in range(10)]
    out = bench.loop_outputs(_frame_record(), traj, 4)
    bench.dump_outputs(str(tmp_path), out)
    T = np.load(tmp_path / "T_wc.npy")
    assert T.dtype == np.float32 and T.reshape(-1).tolist() == [np.float32(k) / 3 for k in range(16)]
    tr = np.load(tmp_path / "trajectory_T_wc.npy")
    assert tr.dtype == np.float32 and tr.shape == (4, 4, 4) and tr[0, 0, 0] == 6 and tr[-1, 0, 0] == 9  # the timed frames
    fi = np.load(tmp_path / "frame_info.npy")
    assert fi.dtype == np.float64 and fi[0] == 77


def test_result_dict_arrays(tmp_path):
    r = {"pts": np.arange(6, dtype=np.float32).reshape(3, 2), "stage": np.array([4, 0, 4], np.uint8),
         "mask": np.array([True, False]), "ids": np.array([2 ** 30 + 1], np.int32), "dT": np.eye(4),
         "counts": _capi.FrameCounts(n_l0l1=5), "new": {"pts_l": np.zeros((2, 2), np.float32)}, "n": 3}
    bench.dump_outputs(str(tmp_path), bench.result_arrays(r))
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"pts", "stage", "mask", "ids", "dT", "counts", "new_pts_l"}
    assert {k: v.dtype for k, v in got.items()} == {"pts": np.float32, "stage": np.float32, "mask": np.float32, "ids": np.float64,
                                                    "dT": np.float64, "counts": np.float64, "new_pts_l": np.float32}
    assert got["ids"][0] == 2 ** 30 + 1 and got["counts"][0] == 5 and got["stage"].tolist() == [4, 0, 4]


def test_dump_refuses_more_than_64_mb(tmp_path):
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path), {"big": np.zeros((64 << 20) // 8 + 1, np.float64)})
    assert not os.listdir(tmp_path)

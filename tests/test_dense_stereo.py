"""Dense stereo disparity (include/vo_hip.h, "Dense stereo"): what the definition — as tests/dense_stereo_restatement.py
states it — is worth on the synthetic pair, whose renderer knows the true depth, next to the semi-dense operator on the same pair:
coverage, not precision. The planes' contract, the C defaults and the workspace size. No GPU."""
import ctypes as C

import numpy as np
import pytest

from dense_stereo_restatement import DEFAULTS, dense_stereo
from semidense_restatement import semidense
from test_semidense_emu import synthetic_pair


@pytest.fixture(scope="module")
def results():
    L, R, depth, bf = synthetic_pair()
    return dense_stereo(L, R, n_disp=64, bf=float(bf)), semidense(L, R, d_min=0, d_max=67, bf=float(bf)), depth, bf


def test_definition_covers_the_synthetic_pair(results):
    r, sd, depth, bf = results
    acc, sd_acc = r["status"] == 1, sd["status"] == 1
    truth = float(bf) / depth
    err = np.abs(r["disparity"].astype(np.float64) - truth)
    sd_err = np.abs(sd["disparity"].astype(np.float64) - truth)
    both = acc & sd_acc
    share, within1, ratio = acc.mean(), np.mean(err[acc] <= 1.0), acc.sum() / sd_acc.sum()
    # recorded, not asserted: on the pixels both operators accept the dense disparity is the less precise one
    print(f"accepted {int(acc.sum())} of {acc.size} ({share:.4f}); within 1 px {within1:.4f}; within 0.5 px {np.mean(err[acc] <= 0.5):.4f}; "
          f"median {np.median(err[acc]):.3f} px; {ratio:.2f} x the semi-dense operator's {int(sd_acc.sum())}; on the {int(both.sum())} pixels "
          f"both accept: median {np.median(err[both]):.3f} px dense, {np.median(sd_err[both]):.3f} px semi-dense")
    assert share >= 0.90
    assert within1 >= 0.99
    assert acc.sum() >= 4 * sd_acc.sum()
    # the planes' contract: the meaning of vo_semidense_stereo's planes
    assert (r["disparity"][~acc] == 0).all() and (r["sigma_invd"][~acc] == 0).all()
    assert (r["sigma_invd"][acc] == np.float32(DEFAULTS["eps_d"]) / np.float32(bf)).all() and (r["disparity"][acc] >= 0.5).all()
    assert set(np.unique(r["status"]).tolist()) <= {1, 2, 3, 4} and r["cost"].dtype == np.uint16


def test_parameters_defaults_and_workspace(vo):
    from visual_odometry_ros_amd import _capi
    lib = vo.load()
    p = _capi.DenseStereoParams()
    assert lib.vo_dense_stereo_default_params(C.byref(p)) == 0 and lib.vo_dense_stereo_default_params(None) < 0
    for k, v in DEFAULTS.items():
        assert getattr(p, k) == (np.float32(v) if isinstance(v, float) else v), k
    nbytes = C.c_size_t()
    assert lib.vo_dense_stereo_workspace(1241, 376, C.byref(p), C.byref(nbytes)) == 0
    # two census planes (u64) and the summed volume (u16 per pixel and disparity)
    assert nbytes.value == 1241 * 376 * (2 * 8 + 2 * 64)
    p.n_disp = 100
    assert lib.vo_dense_stereo_workspace(1241, 376, C.byref(p), C.byref(nbytes)) == -1
    p.n_disp = 64
    assert lib.vo_dense_stereo_workspace(0, 376, C.byref(p), C.byref(nbytes)) == -1
    assert lib.vo_dense_stereo(None, 0, 1, C.byref(p), None, None, None, None, 0) < 0

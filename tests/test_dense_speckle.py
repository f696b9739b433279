"""The speckle filter (include/vo_hip.h, "Speckle filter"): what the definition — as tests/dense_speckle_restatement.py
states it — is worth behind the dense operator on the synthetic pair, whose renderer knows the true depth: it takes out the islands
of wrong disparity and next to nothing else. The C defaults, the workspace size and the argument errors. No GPU."""
import ctypes as C

import numpy as np
import pytest

from dense_speckle_restatement import DEFAULTS, SPECKLE, speckle_filter
from dense_stereo_restatement import dense_stereo
from test_semidense_emu import synthetic_pair


@pytest.fixture(scope="module")
def results():
    L, R, depth, bf = synthetic_pair()
    r = dense_stereo(L, R, n_disp=64, bf=float(bf))
    return r, speckle_filter(r["disparity"], r["sigma_invd"], r["status"]), depth, bf


def test_definition_removes_the_wrong_islands_of_the_synthetic_pair(results):
    r, f, depth, bf = results
    acc, kept, gone = r["status"] == 1, f["status"] == 1, f["status"] == SPECKLE
    wrong = np.abs(r["disparity"].astype(np.float64) - float(bf) / depth) > 1.0
    n_acc, n_kept, n_gone = int(acc.sum()), int(kept.sum()), int(gone.sum())
    wrong_acc, wrong_kept, wrong_gone = int((wrong & acc).sum()), int((wrong & kept).sum()), int((wrong & gone).sum())
    print(f"accepted {n_acc}, of them more than 1 px wrong {wrong_acc}; removed {n_gone}, of them wrong {wrong_gone} "
          f"({wrong_gone / max(n_gone, 1):.3f}); kept {n_kept} ({n_kept / n_acc:.4f}), of them wrong {wrong_kept}; "
          f"{f['n_components']} components, the largest of {int(f['size'].max())} pixels")
    assert n_gone == f["n_removed"] == n_acc - n_kept and n_gone > 0
    assert wrong_gone >= 0.9 * n_gone
    assert 2 * wrong_kept <= wrong_acc
    assert n_kept >= 0.995 * n_acc
    # the planes' contract: removed pixels carry zeros, every other pixel every bit
    assert (f["disparity"][gone] == 0).all() and (f["sigma_invd"][gone] == 0).all() and not (gone & ~acc).any()
    for k in ("disparity", "sigma_invd"):
        assert np.array_equal(f[k].view(np.uint32)[~gone], r[k].view(np.uint32)[~gone]), k
    assert np.array_equal(f["status"][~gone], r["status"][~gone])
    assert (f["label"][~acc] == -1).all() and (f["size"][~acc] == 0).all() and (f["size"][acc] >= 1).all()
    assert np.array_equal(gone, acc & (f["size"] <= DEFAULTS["max_size"]))


def test_parameters_defaults_workspace_and_argument_errors(vo):
    from visual_odometry_ros_amd import _capi, api
    lib = vo.load()
    p = _capi.SpeckleParams()
    assert lib.vo_speckle_default_params(C.byref(p)) == 0 and lib.vo_speckle_default_params(None) == -1
    for k, v in DEFAULTS.items():
        assert getattr(p, k) == (np.float32(v) if isinstance(v, float) else v), k
    assert api.DISPARITY_SPECKLE == SPECKLE == 6
    nbytes = C.c_size_t()
    assert lib.vo_speckle_workspace(1241, 376, C.byref(nbytes)) == 0
    assert nbytes.value == 16 + 2 * 4 * 1241 * 376  # the counters, the label plane and the size plane
    assert lib.vo_speckle_workspace(1, 1, C.byref(nbytes)) == 0 and nbytes.value == 24
    assert lib.vo_speckle_workspace(65535, 32768, C.byref(nbytes)) == 0  # 2^31 - 32768 pixels
    for w, h in ((0, 376), (1241, 0), (-1, 5), (65536, 1), (1, 65536), (65535, 65535), (65535, 32769)):
        assert lib.vo_speckle_workspace(w, h, C.byref(nbytes)) == -1, (w, h)
    assert lib.vo_speckle_workspace(1241, 376, None) == -1
    d, st = np.zeros((4, 4), np.float32), np.ones((4, 4), np.uint8)
    args = (d.ctypes.data, None, st.ctypes.data, 4, 4, C.byref(p), None, None, None, None, 0)
    assert lib.vo_disparity_speckle_filter(None, *args) == -1  # no context
    assert lib.vo_svo_set_dense_speckle(None, C.byref(p)) == -1 and lib.vo_svo_get_dense_speckle_stats(None, None, None) == -1
    q = api._speckle_params(lib, dict(max_size=7, max_diff=0.5))
    assert (q.max_size, q.max_diff) == (7, 0.5) and api._speckle_params(lib, True).max_size == 100
    with pytest.raises(ValueError):
        api._speckle_params(lib, dict(max_sise=7))

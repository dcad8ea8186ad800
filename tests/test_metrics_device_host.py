"""CPU: the host half of the device J&F path (swem_amd.metrics "on the device", include/swem_hip_metrics.h): the scores formed
from integer counts equal the CPU metric's, the disk radius, and the entry point's argument checks (they run before any HIP
call, so they need no GPU).  The counts themselves are compared on the GPU: tests/test_gpu_metrics.py."""
import ctypes

import numpy as np
import pytest

from swem_amd import metrics as M
from tests import test_gpu_metrics as G      # the seeded generator and the CPU count of the GPU tests


def _assert_scores_equal(gt, pred, N, void=None):
    counts = G.cpu_counts(gt, pred, N, void=void)
    j, f = M.jf_from_counts(counts)
    assert j.shape == f.shape == counts.shape[:2] and j.dtype == f.dtype == np.float64
    for t in range(gt.shape[0]):
        v = None if void is None else void[t]
        for o in range(1, N + 1):
            assert j[t, o - 1] == M.db_eval_iou(gt[t] == o, pred[t] == o, v), (t, o)
            assert f[t, o - 1] == M.f_measure(pred[t] == o, gt[t] == o, v), (t, o)
    return counts, j, f


@pytest.mark.parametrize('T,H,W,N', [(2, 480, 854, 3), (2, 200, 200, 2), (2, 33, 70, 2), (2, 65, 129, 2), (2, 7, 5, 1), (2, 1, 300, 1),
                                     (2, 300, 1, 1)], ids=lambda v: str(v))
def test_scores_from_counts_equal_the_cpu_metric(T, H, W, N):
    gt, pred = G.make_maps(T, H, W, N, seed=3, roll=(min(2, H - 1), -min(3, W - 1)))
    _assert_scores_equal(gt, pred, N)


def test_scores_from_counts_flagship_case_and_void():
    gt, pred = G.flagship_case()
    counts, j, f = _assert_scores_equal(gt[1:4], pred[1:4], 3)          # the frames with the absent objects
    assert (counts[..., 2] == 0).any() and (counts[..., 3] == 0).any()
    void = np.zeros_like(gt[:2])
    void[:, 200:260, 300:500] = 1
    _assert_scores_equal(gt[:2], pred[:2], 3, void=void)


def test_degenerate_branches():
    """f_measure's four branches and db_eval_iou's empty union, on counts and on masks that produce them."""
    H, W = 40, 60
    blob = np.zeros((H, W), np.uint8)
    blob[10:30, 20:45] = 1
    empty = np.zeros((H, W), np.uint8)
    far = np.zeros((H, W), np.uint8)
    far[0:3, 0:3] = 1
    cases = [(blob, empty), (empty, blob), (empty, empty), (blob, blob), (blob, far)]       # (gt, pred)
    gt = np.stack([c[0] for c in cases])
    pred = np.stack([c[1] for c in cases])
    counts, j, f = _assert_scores_equal(gt, pred, 1)
    n_fg, n_gt = counts[:, 0, 2], counts[:, 0, 3]
    assert n_fg[0] == 0 < n_gt[0] and n_fg[1] > 0 == n_gt[1] and n_fg[2] == 0 == n_gt[2] and counts[2, 0, 1] == 0
    assert f[:, 0].tolist() == [0, 0, 1, 1, 0] and j[:, 0].tolist() == [0, 0, 1, 1, 0]     # (far: precision + recall == 0)
    # the same straight from integers, any leading shape
    j, f = M.jf_from_counts(np.array([[0, 5, 0, 7, 0, 0], [0, 5, 7, 0, 0, 0], [0, 0, 0, 0, 0, 0], [2, 6, 4, 8, 1, 2]], np.int32))
    assert j.tolist() == [0, 0, 1, 2 / 6] and f.tolist() == [0, 0, 1, 2 * (1 / 4.) * (2 / 8.) / ((1 / 4.) + (2 / 8.))]
    with pytest.raises(AssertionError):
        M.jf_from_counts(np.zeros((3, 5), np.int32))


def test_bound_pixels():
    assert M.bound_pixels((480, 854)) == 8 and M.bound_pixels((200, 200)) == 3 and M.bound_pixels((2160, 3840)) == 36
    assert M.bound_pixels((48, 80), 3) == 3 and isinstance(M.bound_pixels((48, 80), 3.0), int)
    with pytest.raises(ValueError):
        M.bound_pixels((48, 80), 2.5)


def test_entry_point_validates_before_any_hip_call(lib):
    T, N, H, W = 4, 2, 48, 80
    need = lib.swem_jf_workspace(T, N, H, W)
    assert need == T * N * 2 * H * 2 * 8
    assert 0 < lib.swem_jf_workspace(1, 1, 1, 1) < lib.swem_jf_workspace(2, 1, 1, 1) < lib.swem_jf_workspace(2, 3, 1, 1)
    assert lib.swem_jf_workspace(T, N, H, W) < lib.swem_jf_workspace(T + 1, N, H, W) < lib.swem_jf_workspace(T + 1, N + 1, H, W)
    d = 4096                                  # a dummy non-null, aligned address: never dereferenced by the checks
    call = lib.swem_jf_counts_u8
    assert call(None, None, None, None, None, T, N, H, W, 3, None, 0) == -4 and b'null pointer' in lib.swem_last_error()
    assert call(None, d, d, None, d, T, N, H, W, 3, None, need) == -4 and b'null pointer' in lib.swem_last_error()
    assert call(None, d, d, None, d, T, N, H, W, 65, d, need) == -1 and b'radius 65' in lib.swem_last_error()
    assert call(None, d, d, None, d, T, 256, H, W, 3, d, need) == -1 and b'N=256' in lib.swem_last_error()
    assert call(None, d, d, None, d, T, N, H, W, 3, d, need - 1) == -2 and b'workspace' in lib.swem_last_error()
    assert call(None, d, d, d, d, 0, N, H, W, 3, d, need) == -1
    assert isinstance(need, int) and lib.swem_jf_counts_u8.restype is ctypes.c_int

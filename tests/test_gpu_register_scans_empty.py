"""Empty clouds through both scan registrations on the device: bsgpu_register_scans (k_icp.hip) and bsgpu_register_scans_gicp
(k_gicp.hip) share the grid build of k_point_grid.hip, which knows nothing of a pair's state; each entry point sets its own.  A
target cloud without points has no grid cell, and a call in which every cloud is empty has no scan launch at all: the pairs' states
must be set all the same.  Each case is held to the shared header on the CPU, bit for bit (icp.h, gicp.h through their drivers).

Shapes: one call of two pairs, an empty target under 600 source points beside the 600-point scene; every target of the call empty
(600, 257 and 0 source points); for GICP also every cloud of the call empty.
"""
import numpy as np
import pytest

import gicp_ref
import icp_ref
import test_gicp
import test_gpu_register_scans as icp_dev
import test_gpu_register_scans_gicp as gicp_dev
import test_icp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def icp_core(tmp_path_factory):
    return test_icp._compile(tmp_path_factory, ["-O2"], "test_icp")


@pytest.fixture(scope="module")
def gicp_core(tmp_path_factory):
    return test_gicp._compile(tmp_path_factory, ["-O2"], "test_gicp")


def _icp_header(core, tmp_path, pairs):
    return [test_icp.parse_reg(tok) for tok in test_icp.run_program(core, [test_icp.reg_command(s, q) for s, q in pairs], tmp_path)]


def _gicp_header(core, tmp_path, pairs):
    """(a pair without any point: the driver prints no covariances)"""
    none = dict(ref_cov=np.zeros((0, 6)), tgt_cov=np.zeros((0, 6)))
    return [{**none, **want} for want in gicp_dev._header(core, tmp_path, [p + (gicp_ref.DEFAULTS,) for p in pairs])]


def _ended_at_once(out, too_few):
    return (out["status"], out["n_iters"], out["n_corr"]) == (too_few, 0, 0) and (out["T"] == icp_ref.EYE).all()


def test_icp_empty_target_beside_a_live_pair(icp_core, tmp_path):
    """The empty pair ends with TOO_FEW_CORRESPONDENCES, T = I and no iteration; its neighbour returns the bits of its lone call."""
    S, Q = icp_ref.scene(600)
    pairs = [(S, Q[:0]), (S, Q)]
    together = icp_dev._device(pairs)
    assert _ended_at_once(together[0], icp_ref.TOO_FEW)
    icp_dev._same_bits(together[1], icp_dev._device([pairs[1]])[0], "lone call")
    for k, want in enumerate(_icp_header(icp_core, tmp_path, pairs)):
        icp_dev._same_bits(together[k], want, k)


def test_icp_every_target_empty(icp_core, tmp_path):
    S, Q = icp_ref.scene(600)
    pairs = [(S, Q[:0]), (S[:257], Q[:0]), (S[:0], Q[:0])]
    got = icp_dev._device(pairs)
    for k, want in enumerate(_icp_header(icp_core, tmp_path, pairs)):
        assert _ended_at_once(got[k], icp_ref.TOO_FEW), k
        icp_dev._same_bits(got[k], want, k)


def test_gicp_empty_target_beside_a_live_pair(gicp_core, tmp_path):
    """The empty pair ends with TOO_FEW_CORRESPONDENCES, T = I and no iteration; its neighbour returns the bits of its lone call."""
    S, Q = icp_ref.scene(600)
    pairs = [(S, Q[:0]), (S, Q)]
    together = gicp_dev._device(pairs)
    assert _ended_at_once(together[0], gicp_ref.TOO_FEW)
    gicp_dev._same_bits(together[1], gicp_dev._device([pairs[1]])[0], "lone call")
    for k, want in enumerate(_gicp_header(gicp_core, tmp_path, pairs)):
        gicp_dev._same_bits(together[k], want, k)


@pytest.mark.parametrize("n_src", [600, 0])
def test_gicp_every_target_empty(n_src, gicp_core, tmp_path):
    """No pair is live and no iteration is enqueued; without source points either there is no cell, no scan and no covariance launch."""
    S, Q = icp_ref.scene(600)
    pairs = [(S[:n_src], Q[:0]), (S[:min(n_src, 257)], Q[:0])]
    got = gicp_dev._device(pairs)
    for k, want in enumerate(_gicp_header(gicp_core, tmp_path, pairs)):
        assert _ended_at_once(got[k], gicp_ref.TOO_FEW), k
        gicp_dev._same_bits(got[k], want, k)

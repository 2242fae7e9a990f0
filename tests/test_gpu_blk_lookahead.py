"""The four-wave schedule of the blocked H x H inverse (blk_sweep<NB, 4>, csrc/blk_inverse.hpp; up to 64 rows: look-ahead on the
diagonal blocks, one barrier per block step, new panels parked in the image's lower blocks; 128 rows: two barriers per step) against
the one-wave schedule (blk_sweep<NB, 1>) on the same LDS image, through vbmf_debug_blk_sweep.  Both perform the same fp64 operations
per 16 x 16 block on the same operands in the same order, so the upper blocks, the log-determinant and the bad-pivot flag must agree
BIT FOR BIT -- at every tier (16, 32, 64, 128 rows), with every count of blocks in use, with a partial last block, on a benign matrix,
on an ARD-like spectrum over 18 decades and when a non-positive pivot is met in the middle of the sweep (NaNs and infinities included:
equal_nan)."""
import numpy as np
import pytest

import __graft_entry__ as G

pytestmark = pytest.mark.gpu

ORDERS = [1, 15, 16,            # one block, partial and full
          17, 31, 32,           # two steps
          33, 48, 49, 64,       # NB = 4 with 3 and 4 blocks used
          65, 96, 113, 128]     # NB = 8 with 5 to 8 blocks used


@pytest.fixture(scope="module")
def capi():
    G.build()
    return G.load_package().capi


def _spd(H):
    """(a) seeded random SPD matrix with spectrum in [1, 100]"""
    rng = np.random.default_rng(4100 + H)
    Q, _ = np.linalg.qr(rng.standard_normal((H, H)))
    K = (Q * np.linspace(1.0, 100.0, H)) @ Q.T
    return 0.5 * (K + K.T)


def _ard(H):
    """(b) G G' / H + diag(10^(-8 .. 10)) in shuffled order: the ARD-like precision of the inverse's probe (scripts/r03_inv_probe.hip)"""
    rng = np.random.default_rng(4200 + H)
    Gm = rng.random((H, H)) - 0.5
    i = np.arange(H)
    dg = 10.0 ** (-8.0 + 18.0 * ((i * 7) % H) / max(1, H - 1))
    K = Gm @ Gm.T / H
    K = 0.5 * (K + K.T)
    K[i, i] += dg
    return K


def _bad(H):
    """(c) matrix (a) with one diagonal entry of the second-to-last block negative (the only block at H <= 16)"""
    K = _spd(H).copy()
    nb = (H + 15) // 16
    blk = max(0, nb - 2)
    i = min(16 * blk + 5, H - 1) if nb > 1 else H // 2
    K[i, i] = -K[i, i]
    return K


def _same(capi, K):
    img4, ld4, bad4 = capi.blk_sweep(K, waves=4)
    img1, ld1, bad1 = capi.blk_sweep(K, waves=1)
    assert img4.shape == img1.shape
    diff = ~((img4.view(np.uint64) == img1.view(np.uint64)) | (np.isnan(img4) & np.isnan(img1)))
    assert not diff.any(), (K.shape[0], int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert bad4 == bad1, (bad4, bad1)
    assert np.array_equal(np.float64(ld4), np.float64(ld1), equal_nan=True), (ld4, ld1)
    return img4, ld4, bad4


@pytest.mark.parametrize("H", ORDERS)
def test_four_waves_equal_one_wave_spd(capi, H):
    K = _spd(H)
    img, ld, bad = _same(capi, K)
    assert bad == 0
    # harness guard only (condition number <= 100, fp64: three orders of margin); the bitwise lines above are the test
    inv = -np.triu(img[:H, :H])
    inv = inv + np.triu(inv, 1).T
    assert np.abs(K @ inv - np.eye(H)).max() <= 1e-10


@pytest.mark.parametrize("H", ORDERS)
def test_four_waves_equal_one_wave_ard(capi, H):
    _same(capi, _ard(H))


@pytest.mark.parametrize("H", ORDERS)
def test_four_waves_equal_one_wave_bad_pivot(capi, H):
    img, ld, bad = _same(capi, _bad(H))
    assert bad != 0

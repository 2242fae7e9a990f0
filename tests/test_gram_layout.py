"""CPU checks of the test decoders of the Gram form's device layouts (tests/helpers.py): a matrix encoded with the kernels' own
store-index formulas, written out in numpy, must decode to itself.  gram_build_kernel (csrc/gram_kernels.hpp) stores the
upper tiles p <= q of G, each with its mirror; gram_prod_kernel stores the transposed product tile fragment-major.  The
encoders also count the stores, so a layout in which two stores collide or a slot is never written fails here."""
import numpy as np
import pytest

from tests.helpers import frag_to_rows, gram_frag_to_matrix


def _rho(r, half):
    """common.hpp rho: row of register r, lane-half `half`, in a 32 x 32 MFMA accumulator"""
    return (r & 3) + 8 * (r >> 2) + 4 * half


def _encode_gram(G, GT):
    """gram_build_kernel's stores of the 32 GT x 32 GT symmetric G: accumulator (p, q), p <= q, lane (half, c), register r holds
    G[32 p + rho(r, half)][32 q + c]; stored at its own fragment slot and, for p != q, at the mirror's."""
    KT = 2 * GT
    out = np.zeros(GT * KT * 64 * 8, dtype=np.float32)
    cnt = np.zeros(out.size, dtype=np.int64)
    p, q = np.triu_indices(GT)
    p, q = p[:, None, None, None], q[:, None, None, None]
    half = np.arange(2)[None, :, None, None]
    c = np.arange(32)[None, None, :, None]
    r = np.arange(16)[None, None, None, :]
    i = _rho(r, half)
    shape = np.broadcast_shapes(p.shape, half.shape, c.shape, r.shape)
    p, q, half, c, i = (np.broadcast_to(a, shape).ravel() for a in (p, q, half, c, i))
    v = G[32 * p + i, 32 * q + c]
    own = ((p * KT + 2 * q + (c >> 4)) * 64 + 32 * ((c >> 3) & 1) + i) * 8 + (c & 7)
    out[own] = v
    np.add.at(cnt, own, 1)
    m = p != q
    mir = ((q[m] * KT + 2 * p[m] + (i[m] >> 4)) * 64 + 32 * ((i[m] >> 3) & 1) + c[m]) * 8 + (i[m] & 7)
    out[mir] = v[m]
    np.add.at(cnt, mir, 1)
    return out, cnt


def _encode_frag(P, Hp):
    """gram_prod_kernel's stores of P (32 XT x Hp): accumulator (row tile p, h tile ht), lane (half, c), register r holds the
    transposed tile's P[32 p + c][32 ht + rho(r, half)], stored at ((p NH + ht) 64 + lane) 16 + r."""
    XT, NH = P.shape[0] // 32, Hp // 32
    out = np.zeros(XT * NH * 64 * 16, dtype=np.float32)
    cnt = np.zeros(out.size, dtype=np.int64)
    p, ht, half, c, r = np.meshgrid(np.arange(XT), np.arange(NH), np.arange(2), np.arange(32), np.arange(16), indexing="ij")
    p, ht, half, c, r = (a.ravel() for a in (p, ht, half, c, r))
    idx = ((p * NH + ht) * 64 + 32 * half + c) * 16 + r
    out[idx] = P[32 * p + c, 32 * ht + _rho(r, half)]
    np.add.at(cnt, idx, 1)
    return out, cnt


@pytest.mark.parametrize("GT", [16, 32])
def test_gram_decoder_roundtrip(GT):
    rng = np.random.default_rng(GT)
    X = rng.standard_normal((32 * GT, 32 * GT)).astype(np.float32)
    G = np.triu(X) + np.triu(X, 1).T                              # symmetric, every entry distinct
    F, cnt = _encode_gram(G, GT)
    assert np.all(cnt == 1), "every fragment slot is written exactly once (upper tiles plus mirrors)"
    assert np.array_equal(gram_frag_to_matrix(F, GT), G)
    # a slice of row tiles decodes to those rows
    KT = 2 * GT
    assert np.array_equal(gram_frag_to_matrix(F[3 * KT * 512:7 * KT * 512], GT), G[96:224])
    # without the mirror stores the lower tiles stay zero: the decoder sees it
    p = np.arange(GT)
    Fu = F.copy()
    Fu.reshape(GT, KT, 64, 8)[p[:, None] > (np.arange(KT)[None, :] >> 1)] = 0.0
    D = gram_frag_to_matrix(Fu, GT)
    tiles = np.arange(32 * GT) // 32
    assert np.array_equal(D[tiles[:, None] <= tiles[None, :]], G[tiles[:, None] <= tiles[None, :]])
    assert not np.any(D[tiles[:, None] > tiles[None, :]])


@pytest.mark.parametrize("XT,Hp", [(3, 32), (5, 64), (2, 128)])
def test_frag_decoder_roundtrip(XT, Hp):
    rng = np.random.default_rng(XT * Hp)
    P = rng.standard_normal((32 * XT, Hp)).astype(np.float32)
    F, cnt = _encode_frag(P, Hp)
    assert np.all(cnt == 1)
    M = 32 * XT - 7
    R = frag_to_rows(F, M, Hp)
    assert R.dtype == np.float64 and np.array_equal(R, P[:M].astype(np.float64))

"""grm_write_spectrum_orders: the spectrum by scattering order with its standard error, written from
the cell sums [N_ORDERS][cells][N_CELL_SUMS] (no GPU): against grm_write_spectrum's 37-column file
on the same sum wE, and against the sums themselves."""
import os

import numpy as np
import pytest

import grmonty_amd as G

CELLS = G.N_TH_BINS * G.N_E_BINS


@pytest.fixture(scope="module")
def written(model64, tmp_path_factory):
    d = tmp_path_factory.mktemp("orders")
    rng = np.random.default_rng(7)
    sums = np.zeros((G.N_ORDERS, CELLS, G.N_CELL_SUMS))
    n = rng.integers(0, 400, size=(G.N_ORDERS, CELLS)).astype(np.float64)
    n[rng.random((G.N_ORDERS, CELLS)) < 0.3] = 0.0   # empty (order, cell) entries
    n[:, 17] = 0.0                                   # a cell empty in every order
    n[:, 5 * G.N_E_BINS + 199] = 0.0                 # the last cell too
    w = 10.0 ** rng.uniform(20, 40, size=n.shape)
    e = 10.0 ** rng.uniform(-10, 2, size=n.shape)
    sums[..., 0] = n
    sums[..., 1] = n * w
    sums[..., 2] = n * w * w
    sums[..., 3] = n * w * e
    sums[..., 4] = n * (w * e) ** 2 * rng.uniform(1.0, 3.0, size=n.shape)
    po = os.path.join(d, "spectrum.orders")
    model64.write_spectrum_orders(sums, po)
    spec = np.zeros(CELLS, dtype=G.SPECTRUM_CELL)
    spec["de_dle"] = sums[..., 3].sum(axis=0)
    spec["dn_dle"] = sums[..., 1].sum(axis=0)
    ps = os.path.join(d, "spectrum.txt")
    model64.write_spectrum(spec, ps)
    return sums, po, ps


def _load_orders(path):
    lines = open(path).read().splitlines()
    head = [ln for ln in lines if ln.startswith("#")]
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    return head, rows


def test_shape_and_header(written):
    _, po, _ = written
    head, rows = _load_orders(po)
    assert len(head) == 1 and open(po).readline().startswith("#")
    assert len(rows) == G.N_E_BINS
    assert all(len(r) == 1 + G.N_TH_BINS * G.N_ORDERS * 3 == 73 for r in rows)


def test_against_37_column_file_and_sums(written):
    sums, po, ps = written
    _, rows = _load_orders(po)
    a = np.array(rows, dtype=np.float64)
    assert a.shape == (G.N_E_BINS, 73)
    body = a[:, 1:].reshape(G.N_E_BINS, G.N_TH_BINS, G.N_ORDERS, 3)   # [i_e, theta, order, (nuLnu, sigma, n)]
    ref = np.loadtxt(ps)
    assert ref.shape == (G.N_E_BINS, 37)
    # the energy axis, to the 37-column file's five digits
    np.testing.assert_allclose(a[:, 0], ref[:, 0], rtol=1e-4)
    nulnu_37 = ref[:, 1::6]                                          # [i_e, theta]
    np.testing.assert_allclose(body[..., 0].sum(axis=2), nulnu_37, rtol=1e-4, atol=0.0)
    s = sums.reshape(G.N_ORDERS, G.N_TH_BINS, G.N_E_BINS, G.N_CELL_SUMS).transpose(2, 1, 0, 3)  # [i_e, theta, order]
    # n exactly
    assert np.array_equal(body[..., 2], s[..., 0])
    # sigma / nuLnu = sqrt(sum (wE)^2) / sum wE
    pos = s[..., 3] > 0
    assert pos.sum() > 1000
    got = body[..., 1][pos] / body[..., 0][pos]
    want = np.sqrt(s[..., 4][pos]) / s[..., 3][pos]
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0.0)
    # empty cells are zeros, not NaN
    empty = s[..., 0] == 0
    assert empty.sum() > 100
    assert np.all(body[empty] == 0.0)
    assert np.all(np.isfinite(body))


def test_rejects_wrong_shape(model64, tmp_path):
    with pytest.raises(ValueError):
        model64.write_spectrum_orders(np.zeros((CELLS, G.N_CELL_SUMS)), str(tmp_path / "x"))

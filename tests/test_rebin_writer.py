"""grm_write_spectrum_grid: the spectrum by scattering order on a caller-chosen (theta, E) grid,
written from a re-binned table [N_ORDERS][rows][n_e][N_CELL_SUMS] (no GPU).

1. the default grid gives grm_write_spectrum_orders' file, byte for byte from the second line on;
2. an unfolded grid whose south rows mirror its north rows gives the nuLnu columns of the folded
   file fed the doubled sums, to 4 ulp (the folded solid angle is twice the row's, the sums twice
   the row's: the two factors of two cancel, and a south row takes its mirror image's solid angle);
3. the column count, 1 + rows * 4 * 3;
4. grids outside the limits and null arguments are errors with a message naming the field."""
import ctypes as C
import os

import numpy as np
import pytest

import grmonty_amd as G


def random_sums(rng, shape):
    """[4][rows][n_e][5] with empty entries, as tests/test_cell_sums_writer.py builds them"""
    n = rng.integers(0, 400, size=shape).astype(np.float64)
    n[rng.random(shape) < 0.3] = 0.0
    w = 10.0 ** rng.uniform(20, 40, size=shape)
    e = 10.0 ** rng.uniform(-10, 2, size=shape)
    return np.stack([n, n * w, n * w * w, n * w * e, n * (w * e) ** 2 * rng.uniform(1.0, 3.0, size=shape)], axis=-1)


def load(path):
    lines = open(path).read().splitlines()
    head = [ln for ln in lines if ln.startswith("#")]
    rows = [ln.split() for ln in lines if not ln.startswith("#")]
    return head, rows


def test_default_grid_is_the_orders_file(model64, tmp_path):
    g = G.BinGrid()
    assert (g.n_th, g.n_e, g.fold, g.pad_) == (6, 200, 1, 0)
    assert g.l_e_0 == np.log(1e-12) and g.d_l_e == 0.25
    assert g.shape == (4, 6, 200, 5)
    sums = random_sums(np.random.default_rng(7), (4, 6, 200))
    po, pg = str(tmp_path / "orders"), str(tmp_path / "grid")
    model64.write_spectrum_orders(sums.reshape(4, 1200, 5), po)
    model64.write_spectrum_grid(g, sums, pg)
    a, b = open(po, "rb").read(), open(pg, "rb").read()
    assert a.startswith(b"#") and b.startswith(b"#")
    head = b.split(b"\n", 1)[0].decode()
    assert "n_th=6" in head and "n_e=200" in head and "fold=1" in head and "independent" in head
    assert a.split(b"\n", 1)[1] == b.split(b"\n", 1)[1]
    assert len(b.split(b"\n", 1)[1]) > 200 * 73 * 2


def test_unfolded_mirror_equals_folded_doubled(model64, tmp_path):
    n_th, n_e = 5, 37
    gu = G.BinGrid(n_th=n_th, n_e=n_e, fold=False, log10_e=(-9.0, 3.5))
    gf = G.BinGrid(n_th=n_th, n_e=n_e, fold=True, log10_e=(-9.0, 3.5))
    assert gu.rows == 10 and gf.rows == 5 and gu.d_l_e == gf.d_l_e and gu.l_e_0 == gf.l_e_0
    north = random_sums(np.random.default_rng(11), (4, n_th, n_e))
    unf = np.concatenate([north, north[:, ::-1]], axis=1)            # row 2 n_th - 1 - i mirrors row i
    pu, pf = str(tmp_path / "unfolded"), str(tmp_path / "folded")
    model64.write_spectrum_grid(gu, unf, pu)
    model64.write_spectrum_grid(gf, 2.0 * north, pf)
    u = np.array(load(pu)[1], dtype=np.float64)
    f = np.array(load(pf)[1], dtype=np.float64)
    assert u.shape == (n_e, 1 + 10 * 12) and f.shape == (n_e, 1 + 5 * 12)
    assert np.array_equal(u[:, 0], f[:, 0])
    ub = u[:, 1:].reshape(n_e, 10, 4, 3)
    fb = f[:, 1:].reshape(n_e, 5, 4, 3)
    assert (fb[..., 0] > 0).sum() > 300
    for half in (ub[:, :5], ub[:, :4:-1]):
        err = np.abs(half[..., 0] - fb[..., 0])
        assert (err <= 4 * np.spacing(fb[..., 0])).all(), float((err / np.maximum(np.spacing(fb[..., 0]), 1e-300)).max())
        assert np.array_equal(2.0 * half[..., 2], fb[..., 2])       # n: the folded file was fed the doubled sums
    # the energy axis: bin centres, l_e_0 + i d_l_e, in log10
    np.testing.assert_allclose(u[:, 0], (gu.l_e_0 + np.arange(n_e) * gu.d_l_e) / np.log(10.0), rtol=1e-15)
    np.testing.assert_allclose(u[0, 0] - 0.5 * gu.d_l_e / np.log(10.0), -9.0, rtol=1e-14)


@pytest.mark.parametrize("n_th,n_e,fold", [(18, 400, True), (3, 7, False)])
def test_column_count(model64, tmp_path, n_th, n_e, fold):
    g = G.BinGrid(n_th=n_th, n_e=n_e, fold=fold)
    rows = n_th if fold else 2 * n_th
    assert g.rows == rows and G.lib().grm_bin_grid_doubles(C.byref(g)) == 4 * rows * n_e * 5
    p = str(tmp_path / "grid")
    model64.write_spectrum_grid(g, random_sums(np.random.default_rng(3), (4, rows, n_e)), p)
    head, body = load(p)
    assert len(head) == 1 and open(p).readline().startswith("#")
    assert len(body) == n_e
    assert all(len(r) == 1 + rows * 4 * 3 for r in body)
    assert np.all(np.isfinite(np.array(body, dtype=np.float64)))


BAD = [
    (dict(n_th=0), "n_th"), (dict(n_th=-3), "n_th"), (dict(n_th=513), "n_th"),
    (dict(n_e=0), "n_e"), (dict(n_e=65537), "n_e"),
    (dict(d_l_e=0.0), "d_l_e"), (dict(d_l_e=-0.25), "d_l_e"), (dict(d_l_e=float("nan")), "d_l_e"),
    (dict(d_l_e=float("inf")), "d_l_e"),
    (dict(l_e_0=float("nan")), "l_e_0"), (dict(l_e_0=float("-inf")), "l_e_0"),
    (dict(fold=2), "fold"), (dict(fold=-1), "fold"),
    (dict(n_th=512, n_e=4096, fold=0), "GRM_REBIN_MAX_CELLS"),
]


@pytest.mark.parametrize("kw,field", BAD, ids=[f"{k}-{i}" for i, (_, k) in enumerate(BAD)])
def test_invalid_grids_are_errors(model64, tmp_path, kw, field):
    g = G.BinGrid()
    for k, v in kw.items():
        setattr(g, k, v)
    L = G.lib()
    msg = L.grm_bin_grid_check(C.byref(g))
    assert msg is not None and field in msg.decode()
    assert L.grm_bin_grid_doubles(C.byref(g)) == 0
    p = str(tmp_path / "never")
    rc = L.grm_write_spectrum_grid(model64.h, C.byref(g), np.zeros(8).ctypes.data_as(G.DP), p.encode())
    assert rc != 0 and field in L.grm_model_last_error().decode()
    assert not os.path.exists(p)
    with pytest.raises(IOError, match=field):
        model64.write_spectrum_grid(g, np.zeros(8), p)


def test_limits_are_accepted_and_null_arguments_refused(model64, tmp_path):
    L = G.lib()
    for kw in (dict(n_th=512, n_e=2048, fold=1), dict(n_th=512, n_e=1024, fold=0), dict(n_th=1, n_e=65536, fold=1),
               dict(n_th=1, n_e=1, fold=0)):
        g = G.BinGrid()
        for k, v in kw.items():
            setattr(g, k, v)
        assert L.grm_bin_grid_check(C.byref(g)) is None, kw
    assert L.grm_bin_grid_check(None) is not None and L.grm_bin_grid_doubles(None) == 0
    g = G.BinGrid()
    sums = np.zeros(g.shape)
    p = str(tmp_path / "x").encode()
    for args in ((None, C.byref(g), sums.ctypes.data_as(G.DP), p), (model64.h, None, sums.ctypes.data_as(G.DP), p),
                 (model64.h, C.byref(g), None, p), (model64.h, C.byref(g), sums.ctypes.data_as(G.DP), None)):
        assert L.grm_write_spectrum_grid(*args) != 0
        assert "null" in L.grm_model_last_error().decode()
    with pytest.raises(ValueError):
        model64.write_spectrum_grid(g, np.zeros((4, 6, 100, 5)), str(tmp_path / "y"))
    assert L.grm_sizeof(7) == C.sizeof(G.BinGrid) == 32

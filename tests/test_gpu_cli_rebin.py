"""The command-line driver's --rebin / --rebin_path (host/grm_main.cpp): the traced run's records
re-binned on the GPU on a grid given on the command line, beside --orders_path's cell sums, and
written by grm_write_spectrum_grid."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "cuda-grmonty_amd", "bin", "grmonty_amd")
U = 2.0 ** -53


def run(dump64, *args):
    cmd = [CLI, f"--harm_dump_path={dump64}", "--photon_n=2000", "--mass_unit=4e19", *args]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


def test_cli_default_grid_equals_orders_file(dump64, tmp_path):
    orders, rebin = tmp_path / "spectrum.orders", tmp_path / "spectrum.grid"
    # --batch=8000: three zone batches, both consumers fed and the trace rewound more than once
    r = run(dump64, f"--orders_path={orders}", "--rebin=6,200", f"--rebin_path={rebin}", "--batch=8000")
    assert r.returncode == 0, r.stderr
    recorded = int(re.search(r"recorded: (\d+)", r.stderr).group(1))
    a_bins = [int(x) for x in re.findall(r"Binned (\d+) trace records", r.stderr)]
    b_bins = [int(x) for x in re.findall(r"Re-binned (\d+) trace records", r.stderr)]
    assert len(a_bins) >= 2 and a_bins == b_bins
    lo, lg = orders.read_text().splitlines(), rebin.read_text().splitlines()
    assert lo[0].startswith("#") and lg[0].startswith("# grid n_th=6 n_e=200 fold=1")
    a = np.array([ln.split() for ln in lo[1:]], dtype=float)
    b = np.array([ln.split() for ln in lg[1:]], dtype=float)
    assert a.shape == b.shape == (200, 73)
    assert np.array_equal(a[:, 0], b[:, 0])
    ab, bb = a[:, 1:].reshape(200, 6, 4, 3), b[:, 1:].reshape(200, 6, 4, 3)
    n = ab[..., 2]
    assert np.array_equal(n, bb[..., 2]) and n.sum() == recorded
    # the same records summed in two orders: tests/test_gpu_cell_sums.py's (2 n + 4) 2^-53 per cell
    tol = (2.0 * n + 4.0) * U
    assert (np.abs(ab[..., 0] - bb[..., 0]) <= tol * ab[..., 0]).all()
    assert (np.abs(ab[..., 1] - bb[..., 1]) <= tol * ab[..., 1]).all()
    # the out-of-grid count is the escaped-unbinned photons of the engine's own grid
    m = re.search(r"Rebin: (\d+) escaped superphotons fell outside the grid", r.stderr)
    assert sum(a_bins) >= recorded + (int(m.group(1)) if m else 0)


def test_cli_wide_unfolded_grid(dump64, tmp_path):
    rebin = tmp_path / "spectrum.grid"
    r = run(dump64, "--rebin=18,400,-14,4,unfold", f"--rebin_path={rebin}")
    assert r.returncode == 0, r.stderr
    recorded = int(re.search(r"recorded: (\d+)", r.stderr).group(1))
    lines = rebin.read_text().splitlines()
    assert lines[0].startswith("# grid n_th=18 n_e=400 fold=0")
    b = np.array([ln.split() for ln in lines[1:]], dtype=float)
    assert b.shape == (400, 1 + 36 * 12)
    d = 18.0 / 400
    np.testing.assert_allclose(b[:, 0], -14.0 + d * (np.arange(400) + 0.5), rtol=1e-12)
    body = b[:, 1:].reshape(400, 36, 4, 3)
    assert body[..., 2].sum() >= recorded                       # the wider range holds at least the engine's
    assert body[:, :18, :, 2].sum() > 0 and body[:, 18:, :, 2].sum() > 0
    assert np.isfinite(body).all()


@pytest.mark.parametrize("args", [["--rebin=6,200"], ["--rebin_path=x.grid"], ["--rebin=6", "--rebin_path=x.grid"],
                                  ["--rebin=6,200,unfolded", "--rebin_path=x.grid"],
                                  ["--rebin=6,200,3,1", "--rebin_path=x.grid"],
                                  ["--rebin=0,200", "--rebin_path=x.grid"]])
def test_cli_usage_errors(dump64, tmp_path, args):
    r = subprocess.run([CLI, f"--harm_dump_path={dump64}", *args], capture_output=True, text=True, timeout=60,
                       cwd=tmp_path)
    assert r.returncode != 0
    assert "usage: --rebin=" in r.stderr
    assert not (tmp_path / "x.grid").exists()

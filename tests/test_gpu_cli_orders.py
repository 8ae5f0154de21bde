"""The command-line driver's --orders_path / --trace_cap (host/grm_main.cpp): a traced run whose
trace is binned on the GPU after every zone batch and written as the 73-column spectrum by
scattering order; a trace too small for a batch ends the run with the error and a non-zero status."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "cuda-grmonty_amd", "bin", "grmonty_amd")


def test_cli_orders(dump64, tmp_path):
    spec, orders = tmp_path / "spectrum", tmp_path / "spectrum.orders"
    # --batch=8000: three zone batches, so the trace is sized, binned and rewound more than once
    cmd = [CLI, f"--harm_dump_path={dump64}", f"--spectrum_path={spec}", f"--orders_path={orders}",
           "--photon_n=2000", "--mass_unit=4e19", "--batch=8000"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    recorded = int(re.search(r"recorded: (\d+)", r.stderr).group(1))
    binned = [int(x) for x in re.findall(r"Binned (\d+) trace records", r.stderr)]
    assert len(binned) >= 2 and sum(binned) > recorded
    lines = orders.read_text().splitlines()
    assert lines[0].startswith("#")
    a = np.array([ln.split() for ln in lines[1:]], dtype=float)
    assert a.shape == (200, 73)
    body = a[:, 1:].reshape(200, 6, 4, 3)                  # [i_e, theta, order, (nuLnu, sigma, n)]
    assert body[..., 2].sum() == recorded
    assert (body[..., 2].sum(axis=(0, 1)) > 0).all()       # every order recorded something
    ref = np.loadtxt(spec)
    np.testing.assert_allclose(body[..., 0].sum(axis=2), ref[:, 1::6], rtol=1e-4, atol=0.0)
    filled = body[..., 2] > 0
    assert (body[..., 1][filled] > 0).all() and (body[..., 1][filled] <= body[..., 0][filled] * (1 + 1e-12)).all()


def test_cli_orders_overflow_is_an_error(dump64, tmp_path):
    orders = tmp_path / "spectrum.orders"
    cmd = [CLI, f"--harm_dump_path={dump64}", f"--orders_path={orders}", "--trace_cap=1000", "--photon_n=2000",
           "--mass_unit=4e19"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "records were lost" in r.stderr and "1000" in r.stderr, r.stderr
    assert not orders.exists()

"""The trace re-binned on a caller-chosen (theta, E) grid (csrc/grm_rebin.hip, grm_engine_rebin_*):
the cell sums' five moments per (order, row, energy bin), with the cell of a record recomputed on
the device from its x2 and e.

Tolerance: tests/test_gpu_cell_sums.py's, derived there -- counts exact, (2 n + 4) 2^-53 relative
per cell for the four sums, n the cell's own count.

The numpy reference (ref_keys / ref_table) restates record_photon's two index expressions.  The
synthetic generator places x2 and ln e at bin-coordinate fractions in [0.1, 0.9], so the host's log
and the device's flog cannot disagree on a cell.

 1. the kernels alone (probe_rebin): record counts around the wave / workgroup / grid-stride edges;
 2. grids: one cell, unfolded, a row wider than a slice, cell counts around the slice size;
 3. one hot cell;  4. the corner cells of an unfolded grid;  5. records at the fold and the poles;
 6. out-of-grid records are skipped and counted once, ended ones (reasons 2-4) never;
 7. escaped-unbinned records (end_reason 1) that fit a wider grid are binned;
 8. a traced model64 job: the default grid equals the engine's cell sums and spectrum;
 9. refinement and unfolding of that job;  10. a second grid without tracking again;
11. a bounded trace buffer shared with the cell sums;  12. loud failures;  13. reset."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_cell_sums import TRACE_CAP, check, check_against_spectrum, restore, traced_job

pytestmark = pytest.mark.gpu

ORDERS_IN = (0, 1, 2, 3, 4, 1000)   # n_scatt values: the clamp to order 3


@pytest.fixture(scope="module")
def x2r(model64):
    """(x_start[2], x_stop[2]) of the model; the generator's north rows need x_start[2] = 0, as
    record_photon's x2 / dx2 does"""
    h = model64.header
    assert h.x_start[2] == 0.0 and h.x_stop[2] == 1.0
    return float(h.x_start[2]), float(h.x_stop[2])


def grid(n_th=6, n_e=200, fold=True, **kw):
    import grmonty_amd as G
    return G.BinGrid(n_th=n_th, n_e=n_e, fold=fold, **kw).check()


def coords(tr, g, x2r):
    """record_photon's bin coordinates: (north, t, u) with i = (int)t and i_e = (int)u - 2"""
    xs2, xe2 = x2r
    dx2 = (xe2 - xs2) / (2 * g.n_th)
    with np.errstate(all="ignore"):
        north = tr["x2"] < 0.5 * (xs2 + xe2)
        t = np.where(north, tr["x2"] / dx2, (xe2 - tr["x2"]) / dx2)
        u = (np.log(tr["e"]) - g.l_e_0) / g.d_l_e + 2.5
    return north, t, u


def ref_keys(tr, g, x2r):
    """(binned, out of grid, order, cell) per record"""
    north, t, u = coords(tr, g, x2r)
    escaped = (tr["end_reason"] == 0) | (tr["end_reason"] == 1)
    with np.errstate(invalid="ignore"):
        ok = (escaped & (tr["n_scatt"] >= 0) & ~np.isnan(tr["w"]) & ~np.isnan(tr["e"]) & ~np.isnan(tr["x2"])
              & (t > -1.0) & (t < g.n_th) & (u >= 2.0) & (u < g.n_e + 2.0))
    i = np.trunc(np.where(ok, t, 0.0)).astype(np.int64)
    i_e = np.trunc(np.where(ok, u, 2.0)).astype(np.int64) - 2
    row = i if g.fold else np.where(north, i, 2 * g.n_th - 1 - i)
    return ok, escaped & ~ok, np.minimum(tr["n_scatt"], 3), row * g.n_e + i_e


def ref_table(tr, g, x2r):
    """([4][rows * n_e][5], n_out_of_grid) by per-order np.bincount"""
    ok, out, order, cell = ref_keys(tr, g, x2r)
    cells = g.rows * g.n_e
    tab = np.zeros((4, cells, 5))
    for k in range(4):
        m = ok & (order == k)
        c, w = cell[m], tr["w"][m]
        we = w * tr["e"][m]
        tab[k, :, 0] = np.bincount(c, minlength=cells)
        for col, v in ((1, w), (2, w * w), (3, we), (4, we * we)):
            tab[k, :, col] = np.bincount(c, weights=v, minlength=cells)
    return tab, int(out.sum())


def synth(n, rng, g, x2r, rows=None, i_e=None, n_scatt=None, ended=0.3, unbinned=0.1):
    """n trace records at bin-coordinate fractions in [0.1, 0.9] of grid g: random (or the given)
    rows, energy bins and orders; a fraction `ended` of reasons 2-4 and a fraction `unbinned` of
    reason 1 (escaped; the re-binning takes them).  ix2 = i_e = -1 throughout: never read."""
    import grmonty_amd as G
    xs2, xe2 = x2r
    tr = np.zeros(n, dtype=G.TRACE)
    tr["id"] = np.arange(n)
    tr["w"] = 10.0 ** rng.uniform(20, 40, n)
    row = rng.integers(0, g.rows, n) if rows is None else rng.choice(rows, n)
    j = rng.integers(0, g.n_e, n) if i_e is None else rng.choice(i_e, n)
    if g.fold:
        north, i = rng.random(n) < 0.5, row
    else:
        north = row < g.n_th
        i = np.where(north, row, 2 * g.n_th - 1 - row)
    dx2 = (xe2 - xs2) / (2 * g.n_th)
    d = (i + rng.uniform(0.1, 0.9, n)) * dx2
    tr["x2"] = np.where(north, d, xe2 - d)
    tr["e"] = np.exp(g.l_e_0 + (j - 0.5 + rng.uniform(0.1, 0.9, n)) * g.d_l_e)
    tr["n_scatt"] = rng.choice(ORDERS_IN if n_scatt is None else n_scatt, n)
    r = rng.random(n)
    dead = r < ended
    tr["end_reason"][dead] = rng.integers(2, 5, int(dead.sum()))
    tr["end_reason"][(r >= ended) & (r < ended + unbinned)] = 1
    tr["ix2"] = -1
    tr["i_e"] = -1
    return tr


def run_probe(eng, tr, g, x2r, what, every_order=False):
    got, out = eng.probe_rebin(tr, g)
    assert got.shape == g.shape
    ref, ref_out = ref_table(tr, g, x2r)
    if every_order:
        assert (ref[:, :, 0].sum(axis=1) > 0).all()          # condition on the input
    check(got.reshape(ref.shape), ref, what=what)
    assert out == ref_out
    return got, out, ref


@pytest.fixture(scope="module")
def eng(model64):
    """the engine of the probe tests and of the one traced job that tests 8-10 re-bin"""
    import grmonty_amd as G
    e = G.Engine(model64, device=0)
    e.emit_setup(model64)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng2(model64):
    """the engine of the tests that run their own jobs"""
    import grmonty_amd as G
    e = G.Engine(model64, device=0)
    e.emit_setup(model64)
    yield e
    e.close()


# --- 1. the kernels alone: record counts ------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 100_003])
@pytest.mark.parametrize("g", [grid, lambda: grid(18, 400)], ids=["default", "18x400"])
def test_probe_record_counts(eng, x2r, g, n):
    g = g()
    tr = synth(n, np.random.default_rng(2000 + n), g, x2r)
    got, out, ref = run_probe(eng, tr, g, x2r, f"n={n}", every_order=n >= 257)
    assert out == 0
    assert got[..., 0].sum() == (tr["end_reason"] <= 1).sum()  # reason 1 in the grid is binned


# --- 2. grids ---------------------------------------------------------------------------------

def slice_grids():
    import grmonty_amd as G
    s = G.lib().grm_rebin_slice_cells()             # GRM_REBIN_SLICE_CELLS of the header
    assert s >= 16
    per_order = G.lib().grm_rebin_max_slices() // 4   # slices of one order at the threshold between the two paths
    assert 1 <= per_order <= 400
    return s, {
        "last-grid-on-slices": dict(n_th=per_order, n_e=s),
        "first-grid-on-direct-atomics": dict(n_th=per_order, n_e=s + 1),
        "direct-atomics-unfolded": dict(n_th=per_order, n_e=s + 3, fold=False),
        "1x1": dict(n_th=1, n_e=1),
        "12x200-unfolded": dict(n_th=12, n_e=200, fold=False),
        "7x1300-wide-row": dict(n_th=7, n_e=1300),
        "one-slice": dict(n_th=1, n_e=s),
        "one-slice-plus-1": dict(n_th=1, n_e=s + 1),
        "not-a-multiple": dict(n_th=3, n_e=s // 2 + 7),
        "two-slices-unfolded": dict(n_th=1, n_e=s, fold=False),
    }


@pytest.mark.parametrize("name", ["1x1", "12x200-unfolded", "7x1300-wide-row", "one-slice", "one-slice-plus-1",
                                  "not-a-multiple", "two-slices-unfolded", "last-grid-on-slices",
                                  "first-grid-on-direct-atomics", "direct-atomics-unfolded"])
def test_probe_grids(eng, x2r, name):
    s, grids = slice_grids()
    g = grid(**grids[name])
    cells = g.rows * g.n_e
    if name == "7x1300-wide-row":
        assert g.n_e > s
    if name == "one-slice":
        assert cells == s
    if name == "one-slice-plus-1":
        assert cells == s + 1
    if name == "not-a-multiple":
        assert cells > s and cells % s
    rng = np.random.default_rng(31)
    tr = np.concatenate([synth(19_883, rng, g, x2r), synth(64, rng, g, x2r, rows=[0], i_e=[0], ended=0.0),
                         synth(64, rng, g, x2r, rows=[g.rows - 1], i_e=[g.n_e - 1], ended=0.0)])
    assert len(tr) == 20_011
    got, out, ref = run_probe(eng, tr, g, x2r, name, every_order=True)
    assert out == 0
    assert (ref[:, 0, 0] > 0).all() and (ref[:, cells - 1, 0] > 0).all()   # the first and the last cell, every order
    if not g.fold:
        north, south = got[:, :g.n_th, :, 0].sum(), got[:, g.n_th:, :, 0].sum()
        assert north > 0 and south > 0


# --- 3. one hot cell --------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65, 100_003])
@pytest.mark.parametrize("n_th,n_e", [(18, 400), (64, 4096)], ids=["lds-slices", "direct-atomics"])
def test_probe_one_hot_cell(eng, x2r, n, n_th, n_e):
    """every record in one (order, cell): all atomics of a slice's workgroups (or, on the large
    grid, of the whole launch) on five addresses"""
    import grmonty_amd as G
    g = grid(n_th, n_e)
    assert (4 * -(-g.rows * g.n_e // G.lib().grm_rebin_slice_cells()) > G.lib().grm_rebin_max_slices()) == (n_th == 64)
    tr = synth(n, np.random.default_rng(7), g, x2r, rows=[11], i_e=[277], n_scatt=[1000], ended=0.0, unbinned=0.0)
    got, out, ref = run_probe(eng, tr, g, x2r, "hot cell")
    assert ref[3, 11 * n_e + 277, 0] == n and out == 0


# --- 4. corners -------------------------------------------------------------------------------

def test_probe_corner_cells_unfolded(eng, x2r):
    g = grid(9, 301, fold=False)
    tr = synth(4099, np.random.default_rng(11), g, x2r, rows=[0, 17], i_e=[0, 300])
    got, out, ref = run_probe(eng, tr, g, x2r, "corners", every_order=True)
    corners = [0, 300, 17 * 301, 17 * 301 + 300]
    for o in range(4):
        for c in corners:
            assert ref[o, c, 0] > 0
    assert ref[..., 0].sum() == ref[:, corners, 0].sum() and out == 0


# --- 5. the fold and the poles ----------------------------------------------------------------

def test_probe_edge_records(eng, x2r):
    import grmonty_amd as G
    xs2, xe2 = x2r
    mid = 0.5 * (xs2 + xe2)
    # x2 == mid takes the south branch (north is x2 < mid).  It lands in the grid only where
    # (xe2 - mid) / dx2 rounds below n_th: pick such an n_th (for the others it is out of grid,
    # as in the reference, whose ix2 == N_TH_BINS is not recorded)
    inside = [k for k in range(2, 200) if (xe2 - mid) / ((xe2 - xs2) / (2 * k)) < k]      # 93 is the first
    outside = [k for k in range(2, 200) if (xe2 - mid) / ((xe2 - xs2) / (2 * k)) >= k]
    assert inside and outside
    for n_th, lands in ((inside[0], True), (outside[0], False)):
        g = grid(n_th, 50, fold=False)
        dx2 = (xe2 - xs2) / (2 * n_th)
        tr = np.zeros(6, dtype=G.TRACE)
        tr["w"] = 1e30
        tr["e"] = np.exp(g.l_e_0 + 20.3 * g.d_l_e)
        tr["n_scatt"] = [0, 1, 2, 3, 0, 0]
        tr["x2"] = [mid, np.nextafter(mid, 0.0), -1e-3 * dx2, xe2 + 1e-3 * dx2, -1.5 * dx2, xe2 + 1.5 * dx2]
        got, out, ref = run_probe(eng, tr, g, x2r, f"edges n_th={n_th}")
        n = got[..., 0].reshape(4, g.rows, g.n_e)
        assert n[0, n_th, 20] == (1 if lands else 0)          # at the fold: the first south row, or out
        assert n[1, n_th - 1, 20] == 1                         # just north of it: the last north row
        assert n[2, 0, 20] == 1                                # slightly negative: truncated to row 0
        assert n[3, 2 * n_th - 1, 20] == 1                     # slightly past x_stop: the south pole's row
        assert out == (2 if lands else 3) and n.sum() == 6 - out


# --- 6. out of grid ---------------------------------------------------------------------------

def test_probe_out_of_grid_is_skipped_and_counted_once(eng, x2r):
    rng = np.random.default_rng(13)
    g = grid()
    tr = synth(6000, rng, g, x2r)
    esc = np.flatnonzero(tr["end_reason"] <= 1)
    bad = rng.choice(esc, 1300, replace=False)
    cases = [("e", 1e-13), ("e", 1e11), ("e", 0.0), ("e", np.nan), ("w", np.nan), ("x2", np.nan), ("x2", 1e300),
             ("x2", -1e300), ("n_scatt", -1), ("e", np.inf), ("e", -1.0), ("x2", -0.2), ("x2", 1.2)]
    for k, (field, v) in enumerate(cases):
        tr[field][bad[100 * k:100 * (k + 1)]] = v
    ended = np.flatnonzero(tr["end_reason"] >= 2)
    assert len(ended) > 1000
    for k, (field, v) in enumerate(cases):                    # the same poison in ended records: never counted
        tr[field][ended[50 * k:50 * (k + 1)]] = v
    good = tr.copy()
    good["end_reason"][bad] = 2
    got, out = eng.probe_rebin(tr, g)
    ref, ref_out = ref_table(tr, g, x2r)
    clean, clean_out = ref_table(good, g, x2r)
    assert ref_out == 1300 and clean_out == 0 and np.array_equal(ref, clean)
    check(got.reshape(ref.shape), clean, what="out of grid")
    assert out == 1300
    assert np.isfinite(got).all()


# --- 7. escaped-unbinned records on a wider grid -----------------------------------------------

def test_probe_reason_1_records_fit_a_wider_grid(eng, x2r):
    import grmonty_amd as G
    rng = np.random.default_rng(17)
    g0 = grid()
    wide = grid(6, 237, l_e_0=g0.l_e_0 - 37 * 0.25, d_l_e=0.25)   # starts four decades lower, same bin edges
    assert (g0.l_e_0 - wide.l_e_0) / np.log(10.0) > 4.0
    tr = synth(30_000, rng, g0, x2r, unbinned=0.0)
    low = synth(5_000, rng, wide, x2r, i_e=np.arange(0, 37), ended=0.0, unbinned=0.0)
    low["end_reason"] = 1                                       # the engine could not bin them
    tr = np.concatenate([tr, low])[rng.permutation(35_000)]
    assert (tr["e"][tr["end_reason"] == 1] < np.exp(g0.l_e_0 - 0.125)).all()
    got0, out0, ref0 = run_probe(eng, tr, g0, x2r, "default grid", every_order=True)
    assert out0 == 5_000 and got0[..., 0].sum() == (tr["end_reason"] == 0).sum()
    got1, out1, ref1 = run_probe(eng, tr, wide, x2r, "wide grid", every_order=True)
    assert out1 == 0 and got1[..., 0].sum() == (tr["end_reason"] <= 1).sum() == got0[..., 0].sum() + 5_000
    assert got1[:, :, :37, 0].sum() == 5_000
    assert np.array_equal(got1[:, :, 37:, 0], got0[..., 0])      # the shared bins: the same records
    assert isinstance(eng.L.grm_sizeof(7), int) and eng.L.grm_sizeof(7) == C.sizeof(G.BinGrid)


# --- 8. the default grid equals the engine ---------------------------------------------------

@pytest.fixture(scope="module")
def job(eng):
    """one traced model64 job on the lane loop; the trace stays in the engine's buffer, so every
    test re-bins it on its own grid (rebin_setup sets the re-binning's consumed mark to 0)"""
    try:
        tr, spec, st = traced_job(eng)
        yield tr, spec, st
    finally:
        eng.rebin_release()
        restore(eng)


def check_default_grid(eng, tr, spec):
    g = eng.rebin_setup()
    n_binned, ms = eng.rebin_accumulate()
    k, s = eng.rebin_ms()
    assert k > 0 and s > 0 and abs(k + s - ms) < 1e-9
    sums, out = eng.rebin()
    again = eng.rebin_accumulate()
    eng.cell_sums_accumulate()
    cs, skipped = eng.cell_sums()
    assert (g.n_th, g.n_e, g.fold) == (6, 200, 1) and sums.shape == (4, 6, 200, 5)
    assert n_binned == len(tr) and ms > 0 and again[0] == 0
    assert skipped == 0 and cs[..., 0].sum() > 0
    flat = sums.reshape(4, 1200, 5)
    check(flat, cs, what="rebin at the default grid against the cell sums")
    assert out == (tr["end_reason"] == 1).sum()
    check_against_spectrum(flat, spec)
    assert np.array_equal(eng.rebin()[0], sums)                 # the empty accumulate changed nothing
    assert eng.rebin_device_ptr() != 0
    return sums


def test_default_grid_equals_engine_lane_loop(eng, job):
    tr, spec, st = job
    print(f"lane loop: {len(tr)} records, {(tr['end_reason'] == 0).sum()} recorded, "
          f"{(tr['end_reason'] == 1).sum()} escaped unbinned")
    check_default_grid(eng, tr, spec)


def test_default_grid_equals_engine_lone_kernel(eng2):
    import grmonty_amd as G
    eng2.set_option(G.OPT_LONE, 2)
    try:
        tr, spec, st = traced_job(eng2)
        assert st["n_lone"] > 0
        check_default_grid(eng2, tr, spec)
    finally:
        eng2.rebin_release()
        restore(eng2)


# --- 9. refinement and fold ------------------------------------------------------------------

def rebin_on(eng, g):
    eng.rebin_setup(g)
    n, _ = eng.rebin_accumulate()
    sums, out = eng.rebin()
    return n, sums, out


def test_refinement_and_fold(eng, job, x2r):
    tr, spec, st = job
    _, base, out0 = rebin_on(eng, grid())
    # twice the theta rows: dx2 / 2 is exact, so adjacent row pairs are the default rows
    n, fine, out = rebin_on(eng, grid(12, 200))
    assert n == len(tr) and out == out0
    assert np.array_equal(fine[:, 0::2, :, 0] + fine[:, 1::2, :, 0], base[..., 0])
    assert (fine[:, 0::2, :, 0].sum() > 0) and (fine[:, 1::2, :, 0].sum() > 0)
    # unfolded: north + mirrored south is the folded table
    n, unf, out = rebin_on(eng, grid(6, 200, fold=False))
    assert n == len(tr) and out == out0 and unf.shape == (4, 12, 200, 5)
    assert unf[:, :6, :, 0].sum() > 0 and unf[:, 6:, :, 0].sum() > 0
    assert np.array_equal(unf[:, :6, :, 0] + unf[:, :5:-1, :, 0], base[..., 0])


def test_18x400_against_probe_and_numpy(eng, job, x2r):
    tr, spec, st = job
    g = grid(18, 400)
    n, acc, out = rebin_on(eng, g)
    got, pout = eng.probe_rebin(tr, g)
    assert n == len(tr) and out == pout
    assert np.array_equal(acc[..., 0], got[..., 0])
    assert (got[..., 0].sum(axis=(0, 2)) > 0).all()            # all 18 theta rows are filled
    print(f"18 x 400: {(got[..., 0].sum(axis=0) > 0).sum()} cells filled, largest {int(got[..., 0].max())}")
    # records within 1e-9 of a bin edge (in bin coordinates, either axis) are set aside on both sides
    _, t, u = coords(tr, g, x2r)
    with np.errstate(invalid="ignore"):
        near = (tr["end_reason"] <= 1) & ((np.abs(t - np.rint(t)) < 1e-9) | (np.abs(u - np.rint(u)) < 1e-9))
    assert near.sum() <= 3
    kept = tr.copy()
    kept["end_reason"][near] = 2
    run_probe(eng, kept, g, x2r, "18 x 400 against numpy", every_order=True)


# --- 10. a second grid without tracking again -------------------------------------------------

def test_second_grid_without_retracking(eng, job, x2r):
    tr, spec, st = job
    n1, a, _ = rebin_on(eng, grid(18, 400))
    tracked = eng.stats()["n_tracked"]
    g = grid(4, 90, fold=False, log10_e=(-14.0, 4.0))
    n2, b, out = rebin_on(eng, g)
    assert n1 == n2 == len(tr) == tracked                       # every record again, nothing tracked in between
    assert eng.rebin_grid().n_e == 90 and b.shape == (4, 8, 90, 5)
    got, pout = eng.probe_rebin(tr, g)
    assert np.array_equal(b[..., 0], got[..., 0]) and out == pout
    assert b[..., 0].sum() + out == (tr["end_reason"] <= 1).sum()


# --- 11. a bounded buffer shared with the cell sums -------------------------------------------

def test_bounded_buffer_two_consumers(eng2):
    import grmonty_amd as G
    try:
        _, _, st = traced_job(eng2)
        total = st["n_tracked"]
        cap = int(0.75 * total)
        eng2.reset()
        eng2.set_option(G.OPT_SEED, 123)
        eng2.set_option(G.OPT_TRACE_CAP, cap)
        eng2.rebin_setup()
        p, n = eng2.emit(seed=123)
        cuts = [0, n // 3, 2 * (n // 3), n]
        binned = [0, 0]
        for a, b in zip(cuts[:-1], cuts[1:]):
            eng2.set_option(G.OPT_ID_BASE, a)
            eng2.track_device(p + a * G.INIT_PHOTON.itemsize, b - a)
            k, _ = eng2.cell_sums_accumulate()
            with pytest.raises(RuntimeError, match="rebin"):
                eng2.trace_rewind()                             # only the cell sums have consumed
            k2, _ = eng2.rebin_accumulate()
            assert 0 < k == k2 <= cap
            binned[0] += k
            binned[1] += k2
            eng2.trace_rewind()
        assert binned[0] == binned[1] == eng2.stats()["n_tracked"] > cap
        sums, out = eng2.rebin()
        cs, skipped = eng2.cell_sums()
        spec = eng2.finish()[0].reshape(-1)
    finally:
        eng2.rebin_release()
        restore(eng2)
    assert skipped == 0 and spec["nph"].sum() > 0
    flat = sums.reshape(4, 1200, 5)
    check(flat, cs, what="bounded buffer")
    check_against_spectrum(flat, spec)


# --- 12. loud failures --------------------------------------------------------------------------

def test_failures_are_loud_and_leave_the_accumulator_alone(model64, eng2):
    import grmonty_amd as G
    e = G.Engine(model64, device=0)
    try:
        assert e.rebin_device_ptr() == 0
        nb, ms = C.c_uint64(7), C.c_double(7.0)
        assert e.L.grm_engine_rebin_accumulate(e.h, C.byref(nb), C.byref(ms)) == -1       # before a setup
        assert "setup" in e.L.grm_engine_last_error(e.h).decode() and nb.value == 0 and ms.value == 0.0
        with pytest.raises(RuntimeError, match="setup"):
            e.rebin()
        e.rebin_setup(grid(3, 10))
        assert e.rebin_device_ptr() != 0
        with pytest.raises(RuntimeError, match="trace is off"):
            e.rebin_accumulate()                                                          # the trace is off
        sums, out = e.rebin()
        assert sums.shape == (4, 3, 10, 5) and not sums.any() and out == 0
    finally:
        e.close()
    try:
        tr, _, _ = traced_job(eng2)
        g = eng2.rebin_setup(grid(5, 77))
        eng2.rebin_accumulate()
        before, out_before = eng2.rebin()
        assert before[..., 0].sum() > 0
        for kw, field in ((dict(n_th=0), "n_th"), (dict(n_e=10 ** 6), "n_e"), (dict(d_l_e=0.0), "d_l_e"),
                          (dict(l_e_0=float("inf")), "l_e_0"), (dict(fold=3), "fold")):
            bad = G.BinGrid()
            for k, v in kw.items():
                setattr(bad, k, v)
            with pytest.raises(RuntimeError, match=field):
                eng2.rebin_setup(bad)                                                     # a bad grid
        now = eng2.rebin_grid()
        assert (now.n_th, now.n_e, now.l_e_0, now.d_l_e) == (5, 77, g.l_e_0, g.d_l_e)
        small = np.zeros(before.size - 1)
        rc = eng2.L.grm_engine_rebin_read(eng2.h, small.ctypes.data_as(G.DP), small.size, None)  # a wrong size
        assert rc == -1 and str(before.size) in eng2.L.grm_engine_last_error(eng2.h).decode()
        assert not small.any()
        rc = eng2.L.grm_probe_rebin(eng2.h, C.byref(g), tr.ctypes.data_as(C.c_void_p), 10, small.ctypes.data_as(G.DP),
                                    small.size, None)                                      # the probe's too
        assert rc == -1 and str(before.size) in eng2.L.grm_engine_last_error(eng2.h).decode()
        after, out_after = eng2.rebin()
        assert np.array_equal(before, after) and out_before == out_after
        assert eng2.rebin_accumulate()[0] == 0                                            # the mark is where it was
        # an overflowed trace
        eng2.reset()
        eng2.set_option(G.OPT_SEED, 123)
        eng2.set_option(G.OPT_ID_BASE, 0)
        eng2.set_option(G.OPT_TRACE_CAP, 1000)
        p, n = eng2.emit(seed=123)
        eng2.track_device(p, n)
        tracked = eng2.stats()["n_tracked"]
        assert tracked > 1000
        nb, ms = C.c_uint64(), C.c_double()
        rc = eng2.L.grm_engine_rebin_accumulate(eng2.h, C.byref(nb), C.byref(ms))
        msg = eng2.L.grm_engine_last_error(eng2.h).decode()
        sums, out = eng2.rebin()
    finally:
        eng2.rebin_release()
        restore(eng2)
    assert rc == -1 and nb.value == 0
    assert str(tracked) in msg and "1000" in msg, msg
    assert not sums.any() and out == 0                          # reset() cleared it; the failure added nothing


# --- 13. reset ---------------------------------------------------------------------------------

def test_reset_probe_and_rewind(model64, eng2, x2r):
    import grmonty_amd as G
    try:
        tr, _, _ = traced_job(eng2)
        g = grid(18, 400)
        eng2.rebin_setup(g)
        eng2.rebin_accumulate()
        a, _ = eng2.rebin()
        assert a.any()
        eng2.probe_rebin(synth(1000, np.random.default_rng(3), grid(2, 9), x2r), grid(2, 9))
        b, _ = eng2.rebin()
        assert np.array_equal(a, b) and eng2.rebin_grid().n_th == 18   # a probe leaves engine state alone
        assert eng2.rebin_accumulate()[0] == 0
        eng2.rebin_reset()
        c, out = eng2.rebin()
        assert not c.any() and out == 0
        assert eng2.rebin_accumulate()[0] == 0                  # rebin_reset keeps the mark
        eng2.rebin_setup(g)
        eng2.rebin_accumulate()
        assert eng2.rebin()[0].any()
        eng2.reset()
        c, out = eng2.rebin()
        assert not c.any() and out == 0                         # reset() clears it, and the mark
        tr2, _, _ = traced_job(eng2, seed=124)
        n, _ = eng2.rebin_accumulate()
        d, _ = eng2.rebin()
        assert n == len(tr2)
        got, _ = eng2.probe_rebin(tr2, g)
        assert np.array_equal(d[..., 0], got[..., 0])           # nothing carried over
    finally:
        eng2.rebin_release()
        restore(eng2)
    # no re-binning set up: trace_rewind behaves as before; set up: the re-binning alone is asked
    e = G.Engine(model64, device=0)
    try:
        e.emit_setup(model64)
        e.trace_rewind()                                        # trace off: nothing to lose
        e.set_option(G.OPT_TRACE_CAP, TRACE_CAP)
        p, n = e.emit(seed=123)
        e.track_device(p, n // 8)
        with pytest.raises(RuntimeError, match="cell_sums_accumulate"):
            e.trace_rewind()
        e.cell_sums_accumulate()
        e.trace_rewind()
        assert e.trace(TRACE_CAP).size == 0
        e2 = G.Engine(model64, device=0)
        try:
            e2.emit_setup(model64)
            e2.set_option(G.OPT_TRACE_CAP, TRACE_CAP)
            e2.rebin_setup()
            p, n = e2.emit(seed=123)
            e2.track_device(p, n // 8)
            with pytest.raises(RuntimeError, match="rebin_accumulate"):
                e2.trace_rewind()
            assert e2.rebin_accumulate()[0] > 0
            e2.trace_rewind()                                   # the cell sums were never fed: not asked
        finally:
            e2.close()
    finally:
        e.close()

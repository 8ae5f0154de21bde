"""Cell sums by scattering order, binned on the device from the trace (csrc/grm_cellsums.hip,
grm_engine_cell_sums_*): n, sum w, sum w^2, sum wE, sum (wE)^2 per (order, theta, E) cell.

Tolerance, derived: every addend is positive, so two summation orders of a cell's n terms differ by
at most 2 (n - 1) 2^-53 relative, plus two roundings per term (the product wE and its square, or the
engine's fused w E + sum): rtol = (2 n + 4) 2^-53 with n the cell's own count.  Counts are exact.

1. the kernel alone (grm_probe_cell_sums) against a per-order np.bincount on synthetic records:
   wave / workgroup / grid-stride edges, one hot cell, the corner cells, the order clamp, unrecorded
   records (ix2 = i_e = -1) and recorded ones outside the grid (skipped and counted);
2. a whole traced model64 job on three transport paths: the accumulator against the numpy binning
   of the downloaded trace, and against the engine's own spectrum (nph, dn_dle, de_dle);
3. a trace buffer smaller than the job, accumulated and rewound after every track call;
4. an overflowed trace and a disabled one fail loudly and leave the accumulator alone;
5. reset() clears it and nothing carries over into the next job."""
import numpy as np
import pytest

from spectrum_stats import cell_sums_from_trace

pytestmark = pytest.mark.gpu

CELLS = 1200
U = 2.0 ** -53
ORDERS_IN = (0, 1, 2, 3, 4, 1000)   # n_scatt values: the clamp to order 3


def ref_sums(tr):
    """[4][1200][5] by per-order np.bincount (cell_sums_from_trace's columns)"""
    r = tr[tr["end_reason"] == 0]
    o = np.minimum(r["n_scatt"], 3)
    return np.stack([cell_sums_from_trace(r[o == k]) for k in range(4)])


def check(got, ref, n=None, what=""):
    """got, ref: [..., 5] (n, sum w, sum w^2, sum wE, sum (wE)^2); n: the counts the tolerance runs on"""
    assert got.shape == ref.shape
    assert np.array_equal(got[..., 0], ref[..., 0]), what + ": counts"
    n = ref[..., 0] if n is None else n
    tol = (2.0 * n + 4.0) * U
    for k in range(1, got.shape[-1]):
        err = np.abs(got[..., k] - ref[..., k])
        bad = err > tol * np.abs(ref[..., k])
        assert not bad.any(), (what, k, int(bad.sum()), float((err / np.maximum(np.abs(ref[..., k]), 1e-300)).max()))


def synth(n, rng, ix2=None, i_e=None, n_scatt=None, ended=0.3):
    """n trace records: recorded photons in random (or the given) cells and orders, and a fraction
    `ended` of unrecorded ones (end_reason 1-4, ix2 = i_e = -1 as the engine writes them)"""
    import grmonty_amd as G
    tr = np.zeros(n, dtype=G.TRACE)
    tr["id"] = np.arange(n)
    tr["w"] = 10.0 ** rng.uniform(20, 40, n)
    tr["e"] = 10.0 ** rng.uniform(-8, 2, n)
    tr["ix2"] = rng.integers(0, 6, n) if ix2 is None else rng.choice(ix2, n)
    tr["i_e"] = rng.integers(0, 200, n) if i_e is None else rng.choice(i_e, n)
    tr["n_scatt"] = rng.choice(ORDERS_IN if n_scatt is None else n_scatt, n)
    dead = rng.random(n) < ended
    tr["end_reason"][dead] = rng.integers(1, 5, int(dead.sum()))
    tr["ix2"][dead] = -1
    tr["i_e"][dead] = -1
    return tr


@pytest.fixture(scope="module")
def eng(model64):
    import grmonty_amd as G
    e = G.Engine(model64, device=0)
    e.emit_setup(model64)
    yield e
    e.close()


# --- 1. the kernel alone -------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 100_003])
def test_probe_mixed_records(eng, n):
    tr = synth(n, np.random.default_rng(1000 + n))
    got, skipped = eng.probe_cell_sums(tr)
    ref = ref_sums(tr)
    if n >= 257:
        assert (ref[:, :, 0].sum(axis=1) > 0).all()        # every order present
    check(got, ref, what=f"n={n}")
    assert skipped == 0                                    # unrecorded records are not "skipped"
    assert got[..., 0].sum() == (tr["end_reason"] == 0).sum()


@pytest.mark.parametrize("n", [65, 100_003])
@pytest.mark.parametrize("n_scatt", [0, 1000])
def test_probe_one_hot_cell(eng, n, n_scatt):
    """every record in one (order, cell): all LDS atomics of a workgroup on five addresses"""
    tr = synth(n, np.random.default_rng(7), ix2=[3], i_e=[77], n_scatt=[n_scatt], ended=0.0)
    got, skipped = eng.probe_cell_sums(tr)
    ref = ref_sums(tr)
    assert ref[min(n_scatt, 3), 3 * 200 + 77, 0] == n
    check(got, ref, what="hot cell")
    assert skipped == 0


def test_probe_corner_cells_and_clamp(eng):
    tr = synth(4099, np.random.default_rng(11), ix2=[0, 5], i_e=[0, 199])
    got, skipped = eng.probe_cell_sums(tr)
    ref = ref_sums(tr)
    for o in range(4):
        for c in (0, 199, 5 * 200, 5 * 200 + 199):
            assert ref[o, c, 0] > 0
    assert ref[..., 0].sum() == ref[:, [0, 199, 1000, 1199], 0].sum()
    # n_scatt 3, 4 and 1000 all land in order 3
    rec = tr[tr["end_reason"] == 0]
    assert ref[3, :, 0].sum() == (rec["n_scatt"] >= 3).sum() > (rec["n_scatt"] == 3).sum()
    check(got, ref, what="corners")
    assert skipped == 0


def test_probe_out_of_grid_is_skipped_and_counted(eng):
    """recorded photons with a cell or an order outside the table contribute nothing and are counted"""
    rng = np.random.default_rng(13)
    tr = synth(5000, rng)
    rec = np.flatnonzero(tr["end_reason"] == 0)
    bad = rng.choice(rec, 600, replace=False)
    tr["ix2"][bad[:100]] = 6
    tr["ix2"][bad[100:200]] = -1
    tr["i_e"][bad[200:300]] = 200
    tr["i_e"][bad[300:400]] = -7
    tr["n_scatt"][bad[400:500]] = -1
    tr["ix2"][bad[500:]] = 2 ** 31 - 1
    tr["i_e"][bad[500:]] = -2 ** 31
    good = tr.copy()
    good["end_reason"][bad] = 2                            # the reference simply leaves them out
    got, skipped = eng.probe_cell_sums(tr)
    check(got, ref_sums(good), what="skipped")
    assert skipped == 600


def test_probe_leaves_engine_state_alone(eng):
    eng.reset()
    eng.cell_sums_reset()
    eng.probe_cell_sums(synth(1000, np.random.default_rng(3)))
    sums, skipped = eng.cell_sums()
    assert not sums.any() and skipped == 0


# --- 2. a real job on three transport paths -------------------------------------------------

TRACE_CAP = 1_000_000


def traced_job(eng, seed=123):
    """emit + track the whole model64 job with the trace on; returns (trace, spectrum, stats)"""
    import grmonty_amd as G
    eng.reset()
    eng.set_option(G.OPT_SEED, seed)
    eng.set_option(G.OPT_ID_BASE, 0)
    eng.set_option(G.OPT_TRACE_CAP, TRACE_CAP)
    p, n = eng.emit(seed=seed)
    eng.track_device(p, n)
    st = eng.stats()
    assert st["n_dropped"] == 0 and st["n_abandoned"] == 0
    tr = eng.trace(TRACE_CAP)
    assert len(tr) == st["n_tracked"] < TRACE_CAP
    spec = eng.finish()[0].reshape(-1)
    return tr, spec, st


def restore(eng):
    import grmonty_amd as G
    eng.set_option(G.OPT_TRACE_CAP, 0)
    eng.set_option(G.OPT_LONE, 1)
    eng.set_option(G.OPT_EARLY_STEPS, 1500)
    eng.set_option(G.OPT_FLIGHT_RATIO, 96)
    eng.set_option(G.OPT_WARMUP, -2)


def check_against_spectrum(sums, spec):
    tot = sums.sum(axis=0)
    assert np.array_equal(tot[:, 0], spec["nph"])
    check(tot[:, [0, 1, 3]], np.stack([spec["nph"], spec["dn_dle"], spec["de_dle"]], axis=1), what="engine spectrum")


@pytest.mark.parametrize("path", ["lane-loop", "lone-kernel", "early-steps-40", "early-worker"])
def test_real_job(eng, path):
    """the default lane loop; every photon through the lone-photon kernel (GRM_OPT_LONE = 2); and
    GRM_OPT_EARLY_STEPS = 40.  A live-bias job this small runs on one workgroup and entirely inside
    the bias warm-up, where nothing is handed to the early worker, so "early-steps-40" changes the
    option alone and "early-worker" also takes the full grid and no warm-up -- the same photons on a
    live bias, now with hand-overs to the worker."""
    import grmonty_amd as G
    eng.set_option(G.OPT_LONE, 2 if path == "lone-kernel" else 1)
    eng.set_option(G.OPT_EARLY_STEPS, 40 if path.startswith("early") else 1500)
    if path == "early-worker":
        eng.set_option(G.OPT_FLIGHT_RATIO, 0)
        eng.set_option(G.OPT_WARMUP, 0)
    try:
        tr, spec, st = traced_job(eng)
        n_binned, ms = eng.cell_sums_accumulate()
        sums, skipped = eng.cell_sums()
        again = eng.cell_sums_accumulate()
        sums2, _ = eng.cell_sums()
    finally:
        restore(eng)
    if path == "lone-kernel":
        assert st["n_lone"] > 0
    if path == "early-worker":
        assert st["n_early"] > 0
    ref = ref_sums(tr)
    per_order = ref[:, :, 0].sum(axis=1)
    per_theta = ref[:, :, 0].sum(axis=0).reshape(6, 200).sum(axis=1)
    print(f"{path}: tracked {len(tr)}, recorded by order {per_order.astype(int).tolist()}, by theta bin "
          f"{per_theta.astype(int).tolist()}, largest cell {int(ref[..., 0].max())}, kernel {ms:.3f} ms")
    assert (per_order > 0).all() and (per_theta > 0).all()  # condition on the input
    assert n_binned == len(tr) and ms > 0
    assert skipped == 0
    check(sums, ref, what=path)
    check_against_spectrum(sums, spec)
    assert again[0] == 0 and np.array_equal(sums, sums2)    # nothing new: bins 0, changes nothing
    assert eng.cell_sums_device_ptr() != 0


# --- 3. a bounded buffer, rewound after every call -------------------------------------------

def test_bounded_buffer(eng):
    import grmonty_amd as G
    try:
        _, _, st = traced_job(eng)
        total = st["n_tracked"]
        cap = int(0.75 * total)                              # below the job's total, above a third's count
        eng.reset()
        eng.set_option(G.OPT_SEED, 123)
        eng.set_option(G.OPT_TRACE_CAP, cap)
        p, n = eng.emit(seed=123)
        cuts = [0, n // 3, 2 * (n // 3), n]
        binned = 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            eng.set_option(G.OPT_ID_BASE, a)
            eng.track_device(p + a * G.INIT_PHOTON.itemsize, b - a)
            if a == 0:
                with pytest.raises(RuntimeError, match="not consumed"):
                    eng.trace_rewind()                       # unconsumed records: refused
            k, _ = eng.cell_sums_accumulate()
            assert 0 < k <= cap
            binned += k
            eng.trace_rewind()
        assert binned == eng.stats()["n_tracked"] > cap      # the buffer served more than it holds
        sums, skipped = eng.cell_sums()
        spec = eng.finish()[0].reshape(-1)
        assert eng.cell_sums_accumulate()[0] == 0
        sums2, _ = eng.cell_sums()
    finally:
        restore(eng)
    assert skipped == 0
    assert spec["nph"].sum() > 0
    check_against_spectrum(sums, spec)
    assert np.array_equal(sums, sums2)


# --- 4. overflow and a disabled trace are loud ----------------------------------------------

def test_overflow_is_loud(eng):
    import ctypes as C
    import grmonty_amd as G
    try:
        eng.reset()
        eng.set_option(G.OPT_SEED, 123)
        eng.set_option(G.OPT_ID_BASE, 0)
        eng.set_option(G.OPT_TRACE_CAP, 1000)
        p, n = eng.emit(seed=123)
        eng.track_device(p, n)
        tracked = eng.stats()["n_tracked"]
        assert tracked > 1000
        nb, ms = C.c_uint64(), C.c_double()
        rc = eng.L.grm_engine_cell_sums_accumulate(eng.h, C.byref(nb), C.byref(ms))
        msg = eng.L.grm_engine_last_error(eng.h).decode()
        sums, skipped = eng.cell_sums()
    finally:
        restore(eng)
    assert rc == -1 and nb.value == 0
    assert str(tracked) in msg and "1000" in msg, msg
    assert not sums.any() and skipped == 0


def test_trace_off_is_loud(model64):
    import ctypes as C
    import grmonty_amd as G
    e = G.Engine(model64, device=0)
    try:
        assert e.cell_sums_device_ptr() == 0                 # nothing allocated before the first use
        rc = e.L.grm_engine_cell_sums_accumulate(e.h, None, None)
        msg = e.L.grm_engine_last_error(e.h).decode()
        assert rc == -1 and "trace" in msg
        with pytest.raises(RuntimeError):
            e.cell_sums_accumulate()
        sums, skipped = e.cell_sums()
        assert sums.shape == (G.N_ORDERS, CELLS, G.N_CELL_SUMS) and not sums.any() and skipped == 0
        assert e.cell_sums_device_ptr() == 0
        e.trace_rewind()                                     # trace off: nothing to lose
    finally:
        e.close()


# --- 5. reset --------------------------------------------------------------------------------

def test_reset_clears_and_nothing_carries_over(eng):
    try:
        traced_job(eng, seed=123)
        eng.cell_sums_accumulate()
        assert eng.cell_sums()[0].any()
        eng.reset()
        sums, skipped = eng.cell_sums()
        assert not sums.any() and skipped == 0
        tr, spec, _ = traced_job(eng, seed=124)
        n_binned, _ = eng.cell_sums_accumulate()
        sums, skipped = eng.cell_sums()
        eng.cell_sums_reset()
        cleared, _ = eng.cell_sums()
    finally:
        restore(eng)
    assert n_binned == len(tr) and skipped == 0
    check(sums, ref_sums(tr), what="after reset")
    check_against_spectrum(sums, spec)
    assert not cleared.any()

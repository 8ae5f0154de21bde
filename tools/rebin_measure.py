#!/usr/bin/env python3
"""Kernel times of the trace re-binning (csrc/grm_rebin.hip) beside cell_sums_kernel on the same
trace: one traced pass per seed at --grid^2, photon_n = --photon-n, then every grid of GRIDS binned
from the records in the trace buffer (rebin_setup sets the consumed mark to 0, so nothing is
tracked again).  Prints one JSON object; DESIGN.md §4.8 and profiles/rebin_measure.json hold a run.

    python tools/rebin_measure.py [--grid 192] [--photon-n 1e6] [--seeds 3] [--reps 3]
    GRMONTY_AMD_LIB=cuda-grmonty_amd/ab/libgrmonty_amd_vdirect.so python tools/rebin_measure.py
        (one accumulation shape forced for every grid: VFLAGS=-DGRM_REBIN_DIRECT_SLICES=0 tools/build_variant.sh
         direct, global atomics; VFLAGS=-DGRM_REBIN_DIRECT_SLICES=1000000 tools/build_variant.sh slices, LDS slices)
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cuda-grmonty_amd"))

import grmonty_amd as G  # noqa: E402
from grmonty_amd.synth_dump import write_dump  # noqa: E402

GRIDS = {"default_6x200": dict(), "18x400": dict(n_th=18, n_e=400), "7x1300": dict(n_th=7, n_e=1300),
         "18x400_unfolded": dict(n_th=18, n_e=400, fold=False), "16x1200": dict(n_th=16, n_e=1200),
         "36x800": dict(n_th=36, n_e=800), "64x4096": dict(n_th=64, n_e=4096)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=192)
    ap.add_argument("--photon-n", type=float, default=1e6)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace-cap", type=int, default=40_000_000)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="grmonty_rebin_") as td:
        path = write_dump(os.path.join(td, "synth.dump"), a.grid, a.grid)
        model = G.Model.load(path, photon_n=int(a.photon_n)).init(16, device=0)
        eng = G.Engine(model, device=0)
        eng.emit_setup(model)
        res = {"lib": os.path.basename(G.LIB_PATH), "grid": a.grid, "photon_n": int(a.photon_n), "seeds": [],
               "slice_cells": G.lib().grm_rebin_slice_cells()}
        # a small traced job first, so that no timed launch is a kernel's first
        eng.set_option(G.OPT_TRACE_CAP, a.trace_cap)
        p, n = eng.emit(seed=999)
        eng.track_device(p, min(n, 20_000))
        eng.cell_sums_accumulate()
        eng.rebin_setup(G.BinGrid())
        eng.rebin_accumulate()
        for s in range(a.seeds):
            seed = 1000 + s
            eng.reset()
            eng.set_option(G.OPT_SEED, seed)
            eng.set_option(G.OPT_ID_BASE, 0)
            eng.set_option(G.OPT_TRACE_CAP, a.trace_cap)
            p, n = eng.emit(seed=seed)
            eng.track_device(p, n)
            st = eng.stats()
            one = {"seed": seed, "primaries": n, "records": st["n_tracked"], "cell_sums_kernel_ms": [], "rebin": {}}
            nb, ms = eng.cell_sums_accumulate()   # once: its consumed mark cannot be set back
            assert nb == st["n_tracked"]
            one["cell_sums_kernel_ms"].append(ms)
            cs, _ = eng.cell_sums()
            for name, kw in GRIDS.items():
                g = G.BinGrid(**kw)
                key, sl = [], []
                for _ in range(a.reps):
                    eng.rebin_setup(g)
                    nb, ms = eng.rebin_accumulate()
                    assert nb == st["n_tracked"]
                    k, v = eng.rebin_ms()
                    key.append(k)
                    sl.append(v)
                sums, out = eng.rebin()
                one["rebin"][name] = {"key_pass_ms": key, "slice_passes_ms": sl, "out_of_grid": out,
                                      "binned": float(sums[..., 0].sum()),
                                      "cells_filled": int((sums[..., 0].sum(axis=0) > 0).sum()),
                                      "largest_cell": float(sums[..., 0].max())}
                if name == "default_6x200":
                    one["rebin"][name]["counts_equal_cell_sums"] = bool(
                        np.array_equal(sums[..., 0].reshape(4, -1), cs[..., 0]))
            eng.rebin_release()
            eng.set_option(G.OPT_TRACE_CAP, 0)
            res["seeds"].append(one)
        eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

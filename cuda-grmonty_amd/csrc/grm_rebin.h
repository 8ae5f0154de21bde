/*
 * grm_rebin.h -- launcher of the re-binning kernels (grm_rebin.hip), shared with the engine's
 * C-ABI entry points (grm_engine.hip).
 */
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/grmonty_amd.h"

/* a validated grm_bin_grid on one model's x2 range, as the kernels take it */
struct grm_rebin_grid {
    double x2_mid; /* 0.5 (xs2 + xe2): x2 below it is north */
    double xe2;
    double dx2;    /* (xe2 - xs2) / (2 n_th) */
    double l_e_0, d_l_e;
    int n_th, n_e, fold;
    unsigned cells; /* rows x n_e of one order */
};

/* a table of more slices than this (GRM_REBIN_SLICE_CELLS cells of one order each, all orders
 * together) is accumulated by direct global atomics instead of LDS slices */
int grm_rebin_direct_slices();

grm_rebin_grid grm_rebin_make(const grm_bin_grid &g, double xs2, double xe2);

/* adds the n trace records at d_rec (device memory) to d_sums, [GRM_N_ORDERS][g.cells]
 * [GRM_N_CELL_SUMS], and the out-of-grid records to *d_out (both device memory, not cleared here).
 * d_keys: device scratch of n 32-bit words, 16-byte aligned.  ev0 / ev1 / ev2 bracket the key pass
 * and the accumulation (slice passes or direct atomics) on stream s; ms[0] = key pass, ms[1] =
 * accumulation (ms may be null).  n = 0 launches nothing.  Synchronous; 0 = OK. */
int grm_rebin_launch(const grm_rebin_grid &g, const grm_trace *d_rec, size_t n, uint32_t *d_keys, double *d_sums,
                     unsigned long long *d_out, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, hipEvent_t ev2,
                     double ms[2], std::string &err);

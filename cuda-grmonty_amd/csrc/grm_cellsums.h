/*
 * grm_cellsums.h -- launcher of the cell-sum binning kernel (grm_cellsums.hip), shared with the
 * engine's C-ABI entry points (grm_engine.hip).
 */
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/grmonty_amd.h"

/* doubles of one accumulator, [GRM_N_ORDERS][GRM_N_TH_BINS * GRM_N_E_BINS][GRM_N_CELL_SUMS] */
constexpr size_t GRM_CELLSUMS_DOUBLES = (size_t)GRM_N_ORDERS * GRM_N_TH_BINS * GRM_N_E_BINS * GRM_N_CELL_SUMS;

/* adds the n trace records at d_rec (device memory) to d_sums and the records it had to skip to
 * *d_skipped (both device memory, not cleared here).  ev0 / ev1 bracket the kernel on stream s;
 * *ms = its time.  n = 0 launches nothing.  Synchronous; 0 = OK. */
int grm_cellsums_launch(const grm_trace *d_rec, size_t n, double *d_sums, unsigned long long *d_skipped, hipStream_t s,
                        hipEvent_t ev0, hipEvent_t ev1, double *ms, std::string &err);

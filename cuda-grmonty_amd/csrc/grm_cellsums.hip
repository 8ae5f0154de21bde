/*
 * grm_cellsums.hip -- the five moment sums per (theta, E) cell, split by scattering order, binned
 * on the device from the per-photon trace (grm_trace records, written by write_trace on every
 * transport path): n, sum w, sum w^2, sum wE, sum (wE)^2 of the recorded superphotons, the sums
 * every spectrum statistic starts from (KS on nuLnu, Kish effective N, standard errors).
 *
 * Layout: sums[order][cell][moment], order = min(n_scatt, 3), cell = ix2 * GRM_N_E_BINS + i_e.
 *
 * Kernel shape: the whole table is 4 x 1200 x 5 x 8 B = 192 KB, more than the CU's 160 KB of LDS,
 * so blockIdx.y picks one order and a workgroup keeps that order's 48 KB slice in LDS (three
 * workgroups per CU).  Every workgroup walks the records in a grid-stride loop (the grid is
 * bounded: a trace of 1e8 records is as good as one of 1e3), reads the record's end reason, cell and
 * order first and its weight and energy only if the record is a recorded photon of its order, adds
 * with LDS fp64 atomics, and at the end flushes its non-zero entries with one global fp64 atomic
 * add each.  No index read from memory is used unchecked: a recorded photon outside the grid, or of
 * a negative order, is skipped and counted (by the order-0 workgroups, so once).
 */
#include "grm_cellsums.h"

namespace {

constexpr int CS_BLOCK = 256;
constexpr int CS_CELLS = GRM_N_TH_BINS * GRM_N_E_BINS;
constexpr int CS_SLICE = CS_CELLS * GRM_N_CELL_SUMS; /* doubles of one order: 6000 = 48 KB */
constexpr unsigned CS_MAX_GRID = 256;                /* x blockIdx.y = 4 orders: 1,024 workgroups at most */
constexpr unsigned CS_RECS_PER_THREAD = 16;          /* below the grid bound: records a thread walks */

static_assert(sizeof(grm_trace) == 96, "grm_trace layout");
static_assert(CS_SLICE * sizeof(double) <= 64 * 1024, "static LDS of one workgroup");

__device__ __forceinline__ void lds_add(double *p, double v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__global__ __launch_bounds__(CS_BLOCK) void cell_sums_kernel(const grm_trace *__restrict__ rec, unsigned long long n,
                                                             double *__restrict__ sums,
                                                             unsigned long long *__restrict__ n_skipped) {
    __shared__ double acc[CS_SLICE];
    const int order = (int)blockIdx.y;
    for (int i = (int)threadIdx.x; i < CS_SLICE; i += CS_BLOCK) acc[i] = 0.0;
    __syncthreads();
    unsigned long long skipped = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * CS_BLOCK;
    for (unsigned long long i = (unsigned long long)blockIdx.x * CS_BLOCK + threadIdx.x; i < n; i += stride) {
        const grm_trace &r = rec[i];
        if (r.end_reason != 0) continue; /* not recorded: ix2 = i_e = -1, no contribution */
        const int ix2 = r.ix2, i_e = r.i_e, n_scatt = r.n_scatt;
        if ((unsigned)ix2 >= (unsigned)GRM_N_TH_BINS || (unsigned)i_e >= (unsigned)GRM_N_E_BINS || n_scatt < 0) {
            ++skipped;
            continue;
        }
        if ((n_scatt < GRM_N_ORDERS - 1 ? n_scatt : GRM_N_ORDERS - 1) != order) continue;
        const double w = r.w;
        const double we = w * r.e; /* rounded once; squared below: numpy's we = w * e; we * we */
        double *c = acc + (ix2 * GRM_N_E_BINS + i_e) * GRM_N_CELL_SUMS;
        lds_add(c + 0, 1.0);
        lds_add(c + 1, w);
        lds_add(c + 2, w * w);
        lds_add(c + 3, we);
        lds_add(c + 4, we * we);
    }
    __syncthreads();
    double *out = sums + (size_t)order * CS_SLICE;
    for (int i = (int)threadIdx.x; i < CS_SLICE; i += CS_BLOCK) {
        const double v = acc[i];
        if (v != 0.0) unsafeAtomicAdd(out + i, v); /* the hardware's fp64 add, not a compare-and-swap loop */
    }
    if (order == 0 && skipped) atomicAdd(n_skipped, skipped);
}

} /* namespace */

int grm_cellsums_launch(const grm_trace *d_rec, size_t n, double *d_sums, unsigned long long *d_skipped, hipStream_t s,
                        hipEvent_t ev0, hipEvent_t ev1, double *ms, std::string &err) {
    if (ms) *ms = 0.0;
    if (n == 0) return 0;
    if (!d_rec || !d_sums || !d_skipped) {
        err = "cell sums: null buffer";
        return -1;
    }
    const size_t per_block = (size_t)CS_BLOCK * CS_RECS_PER_THREAD;
    const size_t want = (n + per_block - 1) / per_block;
    const unsigned gx = want > CS_MAX_GRID ? CS_MAX_GRID : (unsigned)want;
    hipError_t st = hipEventRecord(ev0, s);
    if (st == hipSuccess) {
        hipLaunchKernelGGL(cell_sums_kernel, dim3(gx, GRM_N_ORDERS), dim3(CS_BLOCK), 0, s, d_rec, (unsigned long long)n,
                           d_sums, d_skipped);
        st = hipGetLastError();
    }
    if (st == hipSuccess) st = hipEventRecord(ev1, s);
    if (st == hipSuccess) st = hipEventSynchronize(ev1);
    float t = 0.f;
    if (st == hipSuccess) st = hipEventElapsedTime(&t, ev0, ev1);
    if (st != hipSuccess) {
        err = std::string("cell sums: ") + hipGetErrorString(st);
        return -1;
    }
    if (ms) *ms = t;
    return 0;
}

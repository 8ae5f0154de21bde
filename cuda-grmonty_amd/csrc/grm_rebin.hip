/*
 * grm_rebin.hip -- the trace re-binned on a caller-chosen (theta, E) grid: the cell sums' five
 * moments (n, sum w, sum w^2, sum wE, sum (wE)^2) per scattering order, with the cell of a record
 * recomputed from its x2 and e on a grm_bin_grid given at run time (include/grmonty_amd.h) instead
 * of read from the engine's own ix2 / i_e.  grm_cellsums.hip stays the kernel of the fixed grid.
 *
 * Layout: sums[order][cell][moment], order = min(n_scatt, 3), cell = row * n_e + i_e.
 *
 * Two passes:
 *  1. rebin_key_kernel, one lane per record in a bounded grid-stride loop: the record's cell by
 *     record_photon's two index expressions (grm_transport.h, the same flog), packed with its order
 *     into one 32-bit key = order * cells + cell; KEY_NONE for a record that did not escape
 *     (end_reason 2-4), KEY_OUT -- counted -- for one that escaped but is off the grid.  Every
 *     double is range-checked before it is converted to int, so no conversion is undefined.
 *  2. rebin_slice_kernel: the table has no fixed size (18 x 400 cells x 4 orders x 5 moments is
 *     1.15 MB), so it is cut into slices of GRM_REBIN_SLICE_CELLS cells of one order, 48 KB of
 *     doubles, the LDS block of grm_cellsums.hip (three workgroups per CU).  blockIdx.y picks the
 *     slice, blockIdx.x the workgroup's share of the records; a workgroup reads the keys, and w and
 *     e only of the records whose key is in its slice, adds with LDS fp64 atomics and flushes its
 *     non-zero entries with one hardware global fp64 add each.  The logarithm is taken once per
 *     record, not once per slice.  Every slice pass reads all the keys (four per lane and load), so
 *     the cost grows with the number of slices: a table of more than GRM_REBIN_DIRECT_SLICES slices
 *     is also too sparse for its cells to contend, and
 *  2'. rebin_direct_kernel adds every record's five moments straight to the table in HBM with the
 *     hardware's global fp64 add instead (one pass over the keys whatever the table's size).
 * The threshold is measured; -DGRM_REBIN_DIRECT_SLICES=0 / =1000000 (a variant
 * build, tools/build_variant.sh) force one shape or the other for such a measurement.
 */
#include "grm_rebin.h"

#include "grm_device.h"

namespace {

constexpr int RB_BLOCK = 256;
constexpr int RB_SLICE_CELLS = GRM_REBIN_SLICE_CELLS;
constexpr int RB_SLICE = RB_SLICE_CELLS * GRM_N_CELL_SUMS; /* doubles of one slice: 6000 = 48 KB */
constexpr unsigned RB_MAX_WGS = 1024;                      /* workgroups of a launch, all slices together */
constexpr unsigned RB_RECS_PER_THREAD = 16;                /* below the grid bound: records a thread walks */
#ifndef GRM_REBIN_DIRECT_SLICES
#define GRM_REBIN_DIRECT_SLICES 96 /* more slices than this (all orders together): direct global atomics */
#endif
constexpr uint32_t KEY_OUT = 0xffffffffu;  /* escaped, off the grid (counted) */
constexpr uint32_t KEY_NONE = 0xfffffffeu; /* did not escape: no contribution */

static_assert(sizeof(grm_trace) == 96, "grm_trace layout");
static_assert(RB_SLICE * sizeof(double) <= 64 * 1024, "static LDS of one workgroup");
static_assert((unsigned long long)GRM_N_ORDERS * GRM_REBIN_MAX_CELLS < KEY_NONE, "keys are 32 bits");
static_assert(2ll * GRM_REBIN_MAX_TH * GRM_REBIN_MAX_E < (1ll << 31) && GRM_REBIN_MAX_E < (1 << 30) - 2, "int cells");

__device__ __forceinline__ void lds_add(double *p, double v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

/* the key of one record; see the file comment */
__device__ __forceinline__ uint32_t rebin_key(const grm_trace &r, const grm_rebin_grid &g) {
    if ((unsigned)r.end_reason > 1u) return KEY_NONE;
    const int n_scatt = r.n_scatt;
    const double w = r.w, e = r.e, x2 = r.x2;
    if (n_scatt < 0 || isnan(w) || isnan(e) || isnan(x2)) return KEY_OUT;
    const bool north = x2 < g.x2_mid;
    const double t = north ? x2 / g.dx2 : (g.xe2 - x2) / g.dx2;
    /* (int)t truncates towards zero: row 0 for -1 < t < 1, as the reference's cast */
    if (!(t > -1.0 && t < (double)g.n_th)) return KEY_OUT;
    const int i = (int)t;
    const double u = (grm::flog(e) - g.l_e_0) / g.d_l_e + 2.5;
    /* i_e = (int)u - 2 in [0, n_e)  <=>  2 <= u < n_e + 2 (false for a NaN or infinite u) */
    if (!(u >= 2.0 && u < (double)(g.n_e + 2))) return KEY_OUT;
    const int i_e = (int)u - 2;
    const int row = (g.fold || north) ? i : 2 * g.n_th - 1 - i;
    const unsigned order = n_scatt < GRM_N_ORDERS - 1 ? (unsigned)n_scatt : (unsigned)(GRM_N_ORDERS - 1);
    return order * g.cells + (unsigned)(row * g.n_e + i_e);
}

__global__ __launch_bounds__(RB_BLOCK) void rebin_key_kernel(const grm_trace *__restrict__ rec, unsigned long long n,
                                                             grm_rebin_grid g, uint32_t *__restrict__ keys,
                                                             unsigned long long *__restrict__ n_out) {
    unsigned long long out = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * RB_BLOCK;
    for (unsigned long long i = (unsigned long long)blockIdx.x * RB_BLOCK + threadIdx.x; i < n; i += stride) {
        const uint32_t k = rebin_key(rec[i], g);
        out += k == KEY_OUT;
        keys[i] = k;
    }
    if (out) atomicAdd(n_out, out);
}

/* the five moments of record r into cell c (LDS or global) */
template <bool LDS>
__device__ __forceinline__ void add_record(double *c, const grm_trace &r) {
    const double w = r.w;
    const double we = w * r.e; /* rounded once; squared below: numpy's we = w * e; we * we */
    if (LDS) {
        lds_add(c + 0, 1.0);
        lds_add(c + 1, w);
        lds_add(c + 2, w * w);
        lds_add(c + 3, we);
        lds_add(c + 4, we * we);
    } else { /* the hardware's fp64 add, not a compare-and-swap loop */
        unsafeAtomicAdd(c + 0, 1.0);
        unsafeAtomicAdd(c + 1, w);
        unsafeAtomicAdd(c + 2, w * w);
        unsafeAtomicAdd(c + 3, we);
        unsafeAtomicAdd(c + 4, we * we);
    }
}

/* slice blockIdx.y = the cells [first, first + len) of the flat [order][cell] key space.  keys is
 * 16-byte aligned (the start of an allocation). */
__global__ __launch_bounds__(RB_BLOCK) void rebin_slice_kernel(const grm_trace *__restrict__ rec,
                                                               const uint32_t *__restrict__ keys, unsigned long long n,
                                                               unsigned cells, unsigned slices_per_order,
                                                               double *__restrict__ sums) {
    __shared__ double acc[RB_SLICE];
    const unsigned order = blockIdx.y / slices_per_order, sl = blockIdx.y - order * slices_per_order;
    const unsigned c0 = sl * RB_SLICE_CELLS;
    const unsigned len = cells - c0 < (unsigned)RB_SLICE_CELLS ? cells - c0 : (unsigned)RB_SLICE_CELLS;
    const unsigned first = order * cells + c0;
    const int doubles = (int)len * GRM_N_CELL_SUMS;
    for (int i = (int)threadIdx.x; i < doubles; i += RB_BLOCK) acc[i] = 0.0;
    __syncthreads();
    /* k wraps for a key below the slice, and for KEY_OUT / KEY_NONE stays >= len */
    auto take = [&](unsigned key, unsigned long long i) {
        const unsigned k = key - first;
        if (k < len) add_record<true>(acc + k * GRM_N_CELL_SUMS, rec[i]);
    };
    const unsigned long long stride = (unsigned long long)gridDim.x * RB_BLOCK;
    const unsigned long long t = (unsigned long long)blockIdx.x * RB_BLOCK + threadIdx.x;
    const unsigned long long n4 = n / 4;
    const uint4 *k4 = reinterpret_cast<const uint4 *>(keys);
    for (unsigned long long q = t; q < n4; q += stride) {
        const uint4 k = k4[q];
        take(k.x, 4 * q);
        take(k.y, 4 * q + 1);
        take(k.z, 4 * q + 2);
        take(k.w, 4 * q + 3);
    }
    for (unsigned long long i = 4 * n4 + t; i < n; i += stride) take(keys[i], i); /* the last n % 4 */
    __syncthreads();
    double *out = sums + (size_t)first * GRM_N_CELL_SUMS;
    for (int i = (int)threadIdx.x; i < doubles; i += RB_BLOCK) {
        const double v = acc[i];
        if (v != 0.0) unsafeAtomicAdd(out + i, v); /* the hardware's fp64 add, not a compare-and-swap loop */
    }
}

/* a table of many slices: every record adds its five moments to the table in HBM */
__global__ __launch_bounds__(RB_BLOCK) void rebin_direct_kernel(const grm_trace *__restrict__ rec,
                                                                const uint32_t *__restrict__ keys, unsigned long long n,
                                                                unsigned total_cells, double *__restrict__ sums) {
    const unsigned long long stride = (unsigned long long)gridDim.x * RB_BLOCK;
    for (unsigned long long i = (unsigned long long)blockIdx.x * RB_BLOCK + threadIdx.x; i < n; i += stride) {
        const unsigned k = keys[i];
        if (k < total_cells) add_record<false>(sums + (size_t)k * GRM_N_CELL_SUMS, rec[i]);
    }
}

} /* namespace */

int grm_rebin_direct_slices() { return GRM_REBIN_DIRECT_SLICES; }

grm_rebin_grid grm_rebin_make(const grm_bin_grid &g, double xs2, double xe2) {
    grm_rebin_grid r{};
    r.x2_mid = 0.5 * (xs2 + xe2);
    r.xe2 = xe2;
    r.dx2 = (xe2 - xs2) / (2.0 * g.n_th);
    r.l_e_0 = g.l_e_0;
    r.d_l_e = g.d_l_e;
    r.n_th = g.n_th;
    r.n_e = g.n_e;
    r.fold = g.fold;
    r.cells = (unsigned)(g.fold ? g.n_th : 2 * g.n_th) * (unsigned)g.n_e;
    return r;
}

int grm_rebin_launch(const grm_rebin_grid &g, const grm_trace *d_rec, size_t n, uint32_t *d_keys, double *d_sums,
                     unsigned long long *d_out, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, hipEvent_t ev2,
                     double ms[2], std::string &err) {
    if (ms) ms[0] = ms[1] = 0.0;
    if (n == 0) return 0;
    if (!d_rec || !d_keys || !d_sums || !d_out) {
        err = "rebin: null buffer";
        return -1;
    }
    if (g.cells == 0 || g.cells > (unsigned)GRM_REBIN_MAX_CELLS || !(g.dx2 > 0.0) || !(g.d_l_e > 0.0)) {
        err = "rebin: bad grid";
        return -1;
    }
    const size_t per_block = (size_t)RB_BLOCK * RB_RECS_PER_THREAD;
    const size_t want = (n + per_block - 1) / per_block;
    const unsigned gk = want > RB_MAX_WGS ? RB_MAX_WGS : (unsigned)want;
    hipError_t st = hipEventRecord(ev0, s);
    if (st == hipSuccess) {
        hipLaunchKernelGGL(rebin_key_kernel, dim3(gk), dim3(RB_BLOCK), 0, s, d_rec, (unsigned long long)n, g, d_keys,
                           d_out);
        st = hipGetLastError();
    }
    if (st == hipSuccess) st = hipEventRecord(ev1, s);
    if (st == hipSuccess) {
        /* at most GRM_REBIN_MAX_CELLS / RB_SLICE_CELLS + 1 = 874 slices per order: blockIdx.y < 65536 */
        const unsigned spo = (g.cells + RB_SLICE_CELLS - 1) / RB_SLICE_CELLS;
        const unsigned slices = spo * GRM_N_ORDERS;
        if (slices <= (unsigned)GRM_REBIN_DIRECT_SLICES) {
            unsigned gx = RB_MAX_WGS / slices;
            if (gx < 1) gx = 1;
            if (gx > want) gx = (unsigned)want;
            hipLaunchKernelGGL(rebin_slice_kernel, dim3(gx, slices), dim3(RB_BLOCK), 0, s, d_rec, d_keys,
                               (unsigned long long)n, g.cells, spo, d_sums);
        } else {
            hipLaunchKernelGGL(rebin_direct_kernel, dim3(gk), dim3(RB_BLOCK), 0, s, d_rec, d_keys,
                               (unsigned long long)n, g.cells * GRM_N_ORDERS, d_sums);
        }
        st = hipGetLastError();
    }
    if (st == hipSuccess) st = hipEventRecord(ev2, s);
    if (st == hipSuccess) st = hipEventSynchronize(ev2);
    float t0 = 0.f, t1 = 0.f;
    if (st == hipSuccess) st = hipEventElapsedTime(&t0, ev0, ev1);
    if (st == hipSuccess) st = hipEventElapsedTime(&t1, ev1, ev2);
    if (st != hipSuccess) {
        err = std::string("rebin: ") + hipGetErrorString(st);
        return -1;
    }
    if (ms) {
        ms[0] = t0;
        ms[1] = t1;
    }
    return 0;
}

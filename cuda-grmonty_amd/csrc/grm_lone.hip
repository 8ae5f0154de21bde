/*
 * grm_lone.hip -- the lone-photon kernels (lone_kernel, early_kernel) around the two-wave pipeline of
 * grm_lone_pipe.h, and their launch wrapper (grm_lone_launch, called by the engine's host code).
 *
 * Why a unit of their own, built with other flags than grm_engine.hip: the pipeline's geometry wave
 * is ONE wave on its SIMD, and a single wave issues one instruction of any kind (VALU, SALU, LDS) per
 * ~4 cycles, so its chain is bound by its instruction count.  grm_engine.hip is built with
 * -disable-machine-licm for the bulk kernel (two waves per SIMD, 256 VGPRs: hoisted constants would
 * cost it spills), which leaves every polynomial and physical constant rematerialised inside the
 * loop -- ~115 s_mov_b32 per geometry step beside ~535 VALU.  Here machine LICM stays on and fma_k
 * is a plain fma: the constants are hoisted into registers once per photon (the lone kernels run one
 * wave per SIMD), the step issues ~100 fewer instructions.  Same operations, same results.
 */
#define GRM_FMA_K_PLAIN 1
#include <cstring>

#include "grm_lone_pipe.h"

namespace {

__device__ __forceinline__ bool child_setup_body(const Params &P, const Ctl &C, LoneRec *r, int lane);

constexpr unsigned long long LK_STANDBY = 4; /* lone pairs that wait for children once their photon has ended */
#ifndef GRM_LK_SLEEP
#define GRM_LK_SLEEP 32
#endif

/* A lone pair after its own photon (GRM_OPT_EARLY_CHILDREN): the children the kernel's photons append
 * to lk_q, taken in order by whichever pair looks first, for as long as any pair still tracks a
 * photon (*lk_active), so that a long photon's child starts at once instead of in the relaunch after
 * the kernel.  A pair that finds the queue empty waits, up to LK_STANDBY pairs, or leaves.  Leaving
 * is safe whenever the queue is empty: a child is only appended by a pair that is tracking, and
 * every pair looks at the queue again when its photon ends.  Whole wave, uniform control. */
__device__ void lone_children(const Params &P, const Ctl &C, int lane, LonePair &pr, unsigned &gen,
                              unsigned long long n_handed) {
    bool standing = false;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (true) {
        /* every handed-over photon finished (its pair may not have started yet when a pair looks) */
        const bool orig_done =
            __hip_atomic_load(C.lk_orig, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= n_handed;
        const unsigned long long act = __hip_atomic_load(C.lk_active, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long taken = __hip_atomic_load(C.lk_taken, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        unsigned long long tail = __hip_atomic_load(C.lk_tail, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
        if (tail > C.lk_cap) tail = C.lk_cap;
        if (taken < tail) {
            /* counted as tracking before the claim, so that no waiting pair leaves in between */
            unsigned long long got = ~0ull;
            if (lane == 0) {
                atomicAdd(C.lk_active, 1ull);
                unsigned long long want = taken;
                if (__hip_atomic_compare_exchange_strong(C.lk_taken, &want, taken + 1, __ATOMIC_ACQ_REL,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    got = taken;
                else
                    atomicAdd(C.lk_active, ~0ull);
            }
            got = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(got >> 32)) << 32) |
                  (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)got);
            if (got == ~0ull) continue;
            if (standing && lane == 0) atomicAdd(C.lk_standby, ~0ull);
            standing = false;
            while (__hip_atomic_load(C.lk_ready + got, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != C.lk_tag)
                __builtin_amdgcn_s_sleep(1);
            LoneRec *r = C.lk_q + got;
            if (child_setup_body(P, C, r, lane)) lone_interact(P, C, *r, lane, pr, gen, 2);
            if (lane == 0) __hip_atomic_fetch_add(C.lk_active, ~0ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        if (act == 0 && orig_done) break; /* nothing queued or tracked, nothing to come: no child can */
        if (!standing) {
            unsigned long long sb = 0;
            if (lane == 0) sb = atomicAdd(C.lk_standby, 1ull);
            sb = (unsigned long long)__builtin_amdgcn_readfirstlane((int)sb);
            if (sb >= LK_STANDBY) {
                if (lane == 0) atomicAdd(C.lk_standby, ~0ull);
                return;
            }
            standing = true;
        }
        /* a guard, not a path: every tracked photon ends within its own watchdog */
        if (__builtin_amdgcn_s_memrealtime() - t0 > 2 * (C.watchdog_ticks ? C.watchdog_ticks : 6000000000ull)) {
            if (lane == 0) __hip_atomic_store(&C.ctr->abort, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        __builtin_amdgcn_s_sleep(GRM_LK_SLEEP);
    }
    if (standing && lane == 0) atomicAdd(C.lk_standby, ~0ull);
}

/* launched on lone_cap workgroups; the launch before handed over *C.lone_count photons, one to each of
 * the first workgroups; with GRM_OPT_EARLY_CHILDREN the next LK_STANDBY workgroups (as the grid
 * allows) start as standby pairs for the children, so that a launch of few photons -- a relaunch's
 * long photon -- does not track its photons' children one after another on their own pairs */
__global__ __launch_bounds__(128) void lone_kernel(Params P, Ctl C) {
    unsigned long long n_handed = __hip_atomic_load(C.lone_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_handed > C.lone_cap) n_handed = C.lone_cap;
    const bool extra = blockIdx.x >= n_handed;
    if (blockIdx.x >= C.lone_cap || (extra && (!C.lk_on || n_handed == 0 || blockIdx.x >= n_handed + LK_STANDBY)))
        return;
    const int wave = (int)(threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63);
    LonePair &pr = s_pair[0];
    if (threadIdx.x < 8) s_cnt[threadIdx.x >> 2][threadIdx.x & 3] = 0;
    if (threadIdx.x < LONE_RING) pr.ring[threadIdx.x].tag = 0;
    if (threadIdx.x == 0) {
        pr.ctl.cons = 0;
        pr.ctl.req = 0;
    }
    __syncthreads();
    if (wave == 1) {
        lone_geometry(P, C, lane, pr);
        return;
    }
    unsigned gen = 0;
    if (!extra) {
        if (C.lk_on && lane == 0) atomicAdd(C.lk_active, 1ull);
        lone_interact(P, C, C.lone[blockIdx.x], lane, pr, gen, C.lk_on ? 2 : 0);
        if (C.lk_on && lane == 0) {
            /* its children are queued before it counts as finished (release) */
            __hip_atomic_fetch_add(C.lk_orig, 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(C.lk_active, ~0ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (C.lk_on) lone_children(P, C, lane, pr, gen, n_handed);
    if (lane == 0) __hip_atomic_store(&pr.ctl.req, LONE_STOP, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

/* Concurrent worker for long photons (one workgroup of LONE_PAIRS two-wave pairs on a second
 * stream, beside the bulk launch): once it runs (early_live), a lane-loop photon that reaches early_steps steps is
 * handed over at the top of a step into the early queue (slot claimed by early_tail, published by
 * early_ready[slot] = early_tag); each pair's interaction wave claims slots in order (early_head),
 * waits for them to be published and tracks them with its geometry wave.  It exits once the bulk
 * launch has ended (early_done, set by its last workgroup) and every claimed slot is done.  Without
 * it such a photon would advance one step per lane-loop trip (~7 us) until the bulk ends. */
/* A child request in a queue slot r (queue_child_push) made a photon at the top of its first
 * step: scatter_super_photon's sampling and the set-up at the head of track_super_photon
 * (harm_model.cpp:1083-1215, 895-917) -- the lane loop's sample_child, init_photon and set-up trip,
 * with the same functions: dk/dlambda from the connection at x (its zero-length push), the fluid,
 * both coefficients and the bias at x -- written back into the slot as the LoneRec a hand-over would
 * be.  The whole wave, identical values in every lane; lane 0 writes.  false = an invalid child
 * (traced with reason 4, as in the lane loop). */
/* Inlined.  Out of line (a call) the early kernel's serial chain ran 1.299-1.307 us/step against
 * 1.306-1.313 inlined (tools/gpu_kids_ab.sh), but the same call from lone_kernel handed lone_interact
 * records whose weight came out NaN (every child of the lone kernel's photons; profiles/
 * r06_early_children/lk_debug.log) while the inlined body is photon-by-photon exact in both kernels. */
__device__ __forceinline__ bool child_setup_body(const Params &P, const Ctl &C, LoneRec *r, int lane) {
    SReq R;
    load_sreq(reinterpret_cast<const SReq *>(r), R);
    Rng rng;
    rng.k0 = C.key0;
    rng.k1 = C.key1;
    double x[4], k[4], w;
    Cold c;
    if (lane == 0) atomicAdd(&C.ctr->n_tracked, 1ull);
    bool ok = sample_child_core(P, R, rng, x, k, w, &c);
    ok = ok && !(isnan(x[0]) || isnan(x[1]) || isnan(x[2]) || isnan(x[3]) || isnan(k[0]) || isnan(k[1]) ||
                 isnan(k[2]) || isnan(k[3]) || w == 0.0);
    if (!ok) {
        /* both of the lane loop's invalid-child traces carry these values (id, weight, x of the
         * request, no steps) */
        if (lane == 0 && C.trace)
            write_trace(C, &c, R.id, R.w, R.x[1], R.x[2], R.x[3], 0.0, 0.0, R.n_scatt, 0, 4, -1, -1);
        return false;
    }
    Trig T;
    trig_at(P, x, T);
    Gcov G;
    gcov_from_trig(P, T, G);
    double dk[4];
    {
        Conn Cn;
        connection(P, T, Cn);
#pragma unroll
        for (int i = 0; i < 4; ++i) dk[i] = geo_rhs(Cn, i, k);
    }
    ZoneFetch Z;
    zone_fetch(P, x, Z);
    Fluid F;
    fluid_from(P, x, G, Z, F);
    const double nu = fluid_nu(k, F);
    double a_s = 0.0, a_a = 0.0;
    radiation_coeffs(P, k, F, nu, a_s, a_a); /* the set-up evaluates them whatever nu (transport_trip) */
    const double bf = bias_func(bias_den(P, C), F.theta_e, w);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            r->x[i] = x[i];
            r->k[i] = k[i];
            r->dk[i] = dk[i];
        }
        r->w = w;
        r->e_0_s = c.e;
        r->tau_abs = 0.0;
        r->tau_scatt = 0.0;
        r->a_si = a_s;
        r->a_ai = a_a;
        r->bi = bf;
        r->fl_ne = F.n_e;
        r->c = c;
        r->id = rng.id;
        r->ctr = rng.ctr;
        r->n_step = 0;
        r->n_scatt = R.n_scatt;
        r->pad = 0;
    }
    __threadfence(); /* the wave reads the record back (lone_interact) */
    return true;
}

/* the early worker's next queue slot for the calling interaction wave, or ~0 when none will come.
 * Out of line (it touches only global memory): the kernel's SGPR spills 344 -> 265 */
__device__ __attribute__((noinline)) unsigned long long early_claim(const Ctl &C, unsigned long long rt_start) {
    unsigned long long slot = 0;
    if ((threadIdx.x & 63) == 0) slot = atomicAdd(C.early_head, 1ull);
    slot = (unsigned long long)__builtin_amdgcn_readfirstlane((int)slot); /* < 2^31 */
    unsigned long long t_done = 0; /* when this wave first saw the bulk launch ended */
    while (true) {
        if (slot < C.early_cap &&
            __hip_atomic_load(C.early_ready + slot, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == C.early_tag)
            return slot;
        if (__hip_atomic_load(C.early_done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != 0) {
            /* the bulk launch has ended: every claimed hand-over is published, so a slot past the
             * claims (or past the queue) will never come -- unless a pair still tracking a photon may
             * append a child (queue_child_push).  Slots finish in any order, but while this slot is
             * unpublished every later one is too, so *early_fin >= slot says that every slot before
             * it is finished: nothing is left that could append.  *early_fin is read before the tail
             * (a pair appends before it counts its slot finished), and a pair that leaves counts its
             * own slot, so the pair holding the next one can leave in turn. */
            if (slot >= C.early_cap) return ~0ull;
            const unsigned long long fin =
                C.early_kids_on ? __hip_atomic_load(C.early_fin, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) : 0;
            const unsigned long long tail = __hip_atomic_load(C.early_tail, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
            if (slot >= tail && (!C.early_kids_on || fin >= slot)) {
                if (C.early_kids_on && (threadIdx.x & 63) == 0)
                    __hip_atomic_fetch_add(C.early_fin, 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                return ~0ull;
            }
            /* a guard, not a path: the other pair's photon ends within its own watchdog; a count
             * that never arrives (a bug) fails the call instead of keeping the GPU */
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            if (t_done == 0) t_done = now;
            if (now - t_done > 2 * (C.watchdog_ticks ? C.watchdog_ticks : 6000000000ull)) {
                if ((threadIdx.x & 63) == 0) __hip_atomic_store(&C.ctr->abort, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return ~0ull;
            }
        }
        if (__builtin_amdgcn_s_memrealtime() - rt_start > EARLY_ALONE_TICKS &&
            __builtin_amdgcn_readfirstlane(
                (int)__hip_atomic_load(C.bulk_live, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_AGENT)) == 0) {
            /* no bulk workgroup has started: the launches are serialised and this one runs first.
             * Close the queue, then leave unless a bulk workgroup started meanwhile (then reopen
             * it: a workgroup that read 1 after starting is seen here by the store-load order) */
            if ((threadIdx.x & 63) == 0) __hip_atomic_store(C.early_live, 2ull, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_AGENT);
            if (__builtin_amdgcn_readfirstlane(
                    (int)__hip_atomic_load(C.bulk_live, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_AGENT)) == 0)
                return ~0ull;
            if ((threadIdx.x & 63) == 0) __hip_atomic_store(C.early_live, 1ull, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_AGENT);
        }
        __builtin_amdgcn_s_sleep(64);
    }
}

__global__ __launch_bounds__(64 * 2 * LONE_PAIRS) void early_kernel(Params P, Ctl C) {
    const int wave = (int)(threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63);
    LonePair &pr = s_pair[wave >> 1];
    if (threadIdx.x < 4 * 2 * LONE_PAIRS) s_cnt[threadIdx.x >> 2][threadIdx.x & 3] = 0;
    if (lane < LONE_RING) pr.ring[lane].tag = 0;
    if (lane == 0) {
        pr.ctl.cons = 0;
        pr.ctl.req = 0;
    }
    __syncthreads();
    const unsigned long long rt_start = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) __hip_atomic_store(C.early_live, 1ull, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_AGENT);
    if (wave & 1) {
        /* one inlined copy per pair: the pair's LDS block at a constant address, as in lone_kernel
         * (with the block indexed by the wave the geometry step compiled to ~20 more instructions and
         * ran 1.39 us per step against the lone kernel's 1.29-1.31; now 1.32-1.37) */
        if (wave == 1)
            lone_geometry(P, C, lane, s_pair[0]);
        else
            lone_geometry(P, C, lane, s_pair[1]);
        return;
    }
    unsigned gen = 0;
    while (true) {
        const unsigned long long slot = early_claim(C, rt_start);
        if (slot == ~0ull) break;
        LoneRec *r = C.early_q + slot;
        /* a child request (pad = 1, wave-uniform) becomes a photon at the top of its first step */
        const bool go = r->pad != 1 || child_setup_body(P, C, r, lane);
        if (go) lone_interact(P, C, *r, lane, pr, gen, C.early_kids_on ? 1 : 0);
        if (C.early_kids_on && lane == 0)
            __hip_atomic_fetch_add(C.early_fin, 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane == 0) __hip_atomic_store(&pr.ctl.req, LONE_STOP, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

} /* namespace */

extern "C" hipError_t grm_lone_launch(int which, unsigned grid, hipStream_t s, const void *P, size_t p_size,
                                      const void *C, size_t c_size) {
    if (p_size != sizeof(grm::Params) || c_size != sizeof(Ctl)) return hipErrorInvalidValue; /* built apart */
    grm::Params p;
    Ctl c;
    memcpy(&p, P, sizeof p);
    memcpy(&c, C, sizeof c);
    if (which == 0)
        hipLaunchKernelGGL(lone_kernel, dim3(grid), dim3(128), 0, s, p, c);
    else
        hipLaunchKernelGGL(early_kernel, dim3(1), dim3(64 * 2 * LONE_PAIRS), 0, s, p, c);
    return hipGetLastError();
}

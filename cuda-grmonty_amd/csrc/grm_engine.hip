/*
 * grm_engine.hip -- persistent-wavefront superphoton transport for MI355X (gfx950):
 * the bulk kernel and the C-ABI engine entry points (include/grmonty_amd.h).
 *
 * Replaces the reference's 2-stream x 16384-slot lock-step pipeline of nine kernels
 * per geodesic step with host refills and host re-queueing of scattered photons
 * (super_photon.cu:505-1037).  Here ONE kernel launch tracks a whole batch:
 *
 *   - each lane owns one superphoton in VGPRs for its whole life
 *     (track_super_photon, harm_model.cpp:894-1069, CPU semantics);
 *   - idle lanes refill first from their own child stack, then from the batch pool
 *     with one wave-aggregated atomic per refill (ballot + popcount);
 *   - a scattering pushes the child onto the lane's private stack in HBM (no
 *     inter-lane synchronisation); a full stack spills to an overflow pool that
 *     the host relaunches over (double-buffered) until empty;
 *   - escaping photons are binned with fp64 global atomics (record_super_photon,
 *     harm_model.cpp:1291-1335); counters are u64 (fixes SURVEY Q7).
 *
 * RNG: Philox4x32-10 stream per photon id (key = seed); a child's stream id is a
 * function of its parent's id and draw counter, so results do not depend on lane
 * assignment or scheduling (bias mode FROZEN makes a batch fully reproducible).
 *
 * This file holds the bulk kernel (transport_trip, record_stuck, track_kernel), the utility kernels
 * (stash_kernel, job_counters_kernel, ctl_kernel with CtlOp) and the host engine with the C ABI.
 * The device code the bulk kernel shares with the other transport kernels is grm_transport.h; the
 * lone-photon kernels are grm_lone.hip (their two-wave pipeline: grm_lone_pipe.h), the role-split
 * bulk kernel of variant builds is grm_split.hip.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include <rccl/rccl.h>

#include "grm_transport.h"
#include "grm_cellsums.h"
#include "grm_rebin.h"
#include "grm_emit.h"

namespace {

/* One trip of the lane state machine = at most ONE geodesic push attempt, then, if that attempt
 * completed a step, the rest of the while-loop body of track_super_photon
 * (harm_model.cpp:919-1063).  A lane that has to halve its step (push_photon's recursion,
 * :1279-1285) spends extra trips while the other lanes of the wave keep stepping, instead of the
 * whole wave waiting for the deepest halving tree.  `walked`: halving_walk has just completed this
 * lane's push (its phase-0 block ran before it).  Returns false when the photon's life ended. */
__device__ bool transport_trip(const Params &P, const Ctl &C, Lane &L, Cold *cold, SReq *wstack, int *wtop,
                               const Slot &ph2, const Slot &bk, double bias_d, bool walked, bool &stepped) {
    if (L.phase == 0 && !trip_begin(P, C, L, cold, ph2)) return false;
    TSTAMP(8);
    /* one attempt of push_photon at the current node of the halving tree (:1217-1289).  A lane in
     * set-up (phase 3) makes a zero-length attempt instead: x and k stay, the corrector's first pass
     * leaves dk = dk/dlambda from the connection at x -- init_dkdlam (:915, :1571-1587) -- and T, G
     * are then at x for the fluid evaluation below. */
    const bool setup = L.phase == 3;
    Trig T;
    Gcov G;
    ZoneFetch Z;
    bool have_tg = false;
    TLANES(18, !walked && (setup || !(L.x[1] < P.xs1))); /* slots 18-19: push attempts */
    if (!walked && (setup || !(L.x[1] < P.xs1))) {
        if (L.depth > 0) {
            save_xkdk(bk, L);
        }
        double e_1;
        const bool fail = push_attempt(P, L.x, L.k, L.dk, L.e_0_s, ldexp(L.hlen, -L.depth), e_1, T, G);
        TSTAMP(9);
        if (setup) {
            /* restore x, k exactly (a non-finite dk must not leak into them through 0 * dk) */
#pragma unroll
            for (int i = 0; i < 3; ++i) L.x[1 + i] = ph2[i];
#pragma unroll
            for (int i = 0; i < 4; ++i) L.k[i] = ph2[3 + i];
        } else if (fail && L.depth < MAX_SUBDIV) {
            if (L.depth == 0) {
                load_ph2(ph2, L);
            } else {
                load_xkdk(bk, L);
            }
            ++L.depth;
            L.pend |= 1u << L.depth;
            return true;
        }
        if (!setup) L.e_0_s = e_1;
        have_tg = true;
    }
    if (L.pend) {
        L.depth = 31 - __builtin_clz(L.pend);
        L.pend &= ~(1u << L.depth);
        return true;
    }
    /* the push is complete.  Phase 1 = end of a geodesic step: stop test, then the interaction
     * block (:927-1056).  Phase 2 = back at the scattering point after the re-push (:1005-1055).
     * Both evaluate the fluid and the absorption/scattering coefficients at the new point; they share
     * ONE evaluation here so a wave with lanes in both phases runs that code once. */
    const bool at_scatter = L.phase == 2;
    if (!at_scatter && !setup) {
        stepped = true; /* counted per wave by the caller (a ballot), not per lane in LDS */
        if (stop_criterion(P, L)) {
            end_of_life(P, C, cold, L);
            return false;
        }
        /* A NaN position is absorbing: every later stop test is false, no interaction can fire
         * (bias * d_tau_scatt > x1 is false for NaN), and record_super_photon drops NaN photons
         * (harm_model.cpp:1291-1295), so the reference's loop only burns steps -- each a full
         * 255-attempt halving tree, since err is NaN -- until max_n_step (:1058-1063, no record :1066).  End it here
         * with the same (empty) outcome. */
        if (isnan(L.x[1])) {
            atomicAdd(&C.ctr->n_nan, 1ull);
            trace_end(C, cold, L, 3);
            return false;
        }
    }
    TSTAMP(10);
    TLANES(16, setup || at_scatter || L.alpha_absi() > 0.0 || L.alpha_scatti() > 0.0 || L.fl_ne() > 0.0);
    if (setup || at_scatter || L.alpha_absi() > 0.0 || L.alpha_scatti() > 0.0 || L.fl_ne() > 0.0) {
        if (!have_tg) {
            trig_at(P, L.x, T);
            gcov_from_trig(P, T, G);
        }
        zone_fetch(P, L.x, Z);
        Fluid F;
        fluid_from(P, L.x, G, Z, F);
        L.fl_ne() = F.n_e;
        TSTAMP(11);
        /* scatter_super_photon's parent-side check (:1076-1081) */
        if (at_scatter && F.n_e > 0.0 &&
            (L.k[0] > 1.0e5 || L.k[0] < 0.0 || isnan(L.k[0]) || isnan(L.k[1]) || isnan(L.k[3]))) {
            L.k[0] = fabs(L.k[0]);
            L.w = 0.0;
            trace_end(C, cold, L, 2);
            return false;
        }
        /* phase 1 skips the coefficients out of the fluid (bound_flag, :941-955); both skip them
         * for nu < 0 */
        const double nu = fluid_nu(L.k, F);
        const bool zero = !setup && (nu < 0.0 || (!at_scatter && F.n_e == 0.0));
        double a_s = 0.0, a_a = 0.0;
        if (!zero) {
            radiation_coeffs(P, L.k, F, nu, a_s, a_a);
        }
        const double bf = (zero && !at_scatter) ? 0.0 : bias_func(bias_d, F.theta_e, L.w);
        TSTAMP(12);
        if (setup) { /* the set-up's coefficients (:905-913); the loop starts on the next trip */
            L.alpha_scatti() = a_s;
            L.alpha_absi() = a_a;
            L.bi() = bf;
            L.phase = 0;
            return true;
        }
        if (at_scatter) {
            /* the child leaves as a scatter request; its stores go out after this trip's table
             * loads, so no load of the trip waits behind them (vmcnt is in order) */
            if (F.n_e > 0.0) {
                if (push_request(C, L.x, L.k, L.rng, L.n_scatt(), cold, F, L.p_wc(), wstack, wtop)) ++L.flight();
                ++L.c_children();
            }
            L.alpha_scatti() = a_s;
            L.alpha_absi() = a_a;
            L.bi() = bf;
            L.tau_abs() += L.p_dtau_abs();
            L.tau_scatt() += L.p_dtau_scatt();
        } else {
            /* trapezoid optical depths over the step (:957-975) */
            const double dl = L.dl;
            double d_tau_scatt, d_tau_abs, bias;
            if (zero) {
                d_tau_scatt = 0.5 * L.alpha_scatti() * P.d_tau_k * dl;
                d_tau_abs = 0.5 * L.alpha_absi() * P.d_tau_k * dl;
                bias = 0.0;
            } else {
                d_tau_scatt = 0.5 * (L.alpha_scatti() + a_s) * P.d_tau_k * dl;
                d_tau_abs = 0.5 * (L.alpha_absi() + a_a) * P.d_tau_k * dl;
                bias = 0.5 * (L.bi() + bf);
            }
            L.alpha_scatti() = a_s;
            L.alpha_absi() = a_a;
            L.bi() = bf;
            /* x1 = -log u (:983); the test bias * d_tau_scatt > x1 is settled without the logarithm
             * when bias * d_tau_scatt <= (1 - u)(1 - 2^-40) <= -log u (margin for the log's rounding) */
            const double u = uniform(L.rng);
            const double bdt = bias * d_tau_scatt;
            const bool may = bdt > (1.0 - u) * (1.0 - 0x1p-40);
            const double x1 = may ? -flog(u) : 0.0;
            const double wc = fdiv(L.w, bias);
            if (may && bdt > x1 && wc > WEIGHT_MIN) {
                const double frac = fdiv(x1, bias * d_tau_scatt);
                d_tau_abs *= frac;
                if (d_tau_abs > 100) {
                    trace_end(C, cold, L, 2);
                    return false; /* absorbed before scattering */
                }
                d_tau_scatt *= frac;
                const double d_tau = d_tau_abs + d_tau_scatt;
                if (d_tau_abs < 1.0e-3)
                    L.w *= (1.0 - d_tau * (1.0 / 24.0) * (24.0 - d_tau * (12.0 - d_tau * (4.0 - d_tau))));
                else
                    L.w *= fexp(-d_tau);
                /* re-push photon_2 by dl*frac to the scattering point (:1005), on later trips */
                load_ph2(ph2, L);
                L.e_0_s = L.ph2_e0s();
                L.hlen = dl * frac;
                L.depth = 0;
                L.pend = 0;
                L.phase = 2;
                L.p_dtau_abs() = d_tau_abs;
                L.p_dtau_scatt() = d_tau_scatt;
                L.p_wc() = wc;
                return true;
            }
            if (d_tau_abs > 100) {
                trace_end(C, cold, L, 2);
                return false; /* absorbed */
            }
            const double d_tau = d_tau_abs + d_tau_scatt;
            if (d_tau < 1.0e-3)
                L.w *= (1.0 - d_tau * (1.0 / 24.0) * (24.0 - d_tau * (12.0 - d_tau * (4.0 - d_tau))));
            else
                L.w *= fexp(-d_tau);
            L.tau_abs() += d_tau_abs;
            L.tau_scatt() += d_tau_scatt;
        }
    }
    TSTAMP(13);
    L.phase = 0;
    ++L.n_step;
    if (L.n_step > MAX_N_STEP) {
        trace_end(C, cold, L, 3);
        return false;
    }
    return true;
}

/* watchdog record of a photon abandoned mid-flight: id, n_step, phase, depth, pend, w, e_0_s, dl, x, k */
__device__ void record_stuck(const Ctl &C, const Lane &L) {
    const unsigned long long slot = atomicAdd(C.stuck_count, 1ull);
    if (slot >= C.stuck_cap) return;
    double *r = C.stuck + slot * STUCK_WORDS;
    r[0] = (double)L.rng.id;
    r[1] = L.n_step;
    r[2] = L.phase;
    r[3] = L.depth;
    r[4] = L.pend;
    r[5] = L.w;
    r[6] = L.e_0_s;
    r[7] = L.dl;
    for (int i = 0; i < 4; ++i) {
        r[8 + i] = L.x[i];
        r[12 + i] = L.k[i];
    }
}

__global__ __launch_bounds__(BLOCK, MIN_WAVES_PER_SIMD) void track_kernel(Params P_, Ctl C_) {
    KArgsK *const ka = kargs();
    const Ctl &C0 = C_;
    const Params &P0 = P_;
#ifdef GRM_TIMING
    const unsigned long long t_start = __builtin_amdgcn_s_memtime();
    if ((threadIdx.x & 63) < 24) g_tlds[threadIdx.x >> 6][threadIdx.x & 63] = (threadIdx.x & 63) == 15 ? t_start : 0;
#endif
    __shared__ double lds[2 * LDS_DOUBLES_PER_LANE * BLOCK];
    const Slot ph2{lds + threadIdx.x, BLOCK};
    const Slot bk{lds + LDS_DOUBLES_PER_LANE * BLOCK + threadIdx.x, BLOCK};
    const unsigned lane_id = threadIdx.x & 63;
    const uint64_t gtid = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const int wave = threadIdx.x >> 6;
    SReq *wstack = C0.stack + (gtid >> 6) * WSTACK_CAP;
    __shared__ int s_wtop[BLOCK / 64];
    int *wtop = s_wtop + wave;
    if (lane_id == 0) *wtop = 0;
    if (lane_id == 0) s_recn[wave] = 0;
    if (lane_id < 4) s_cnt[wave][lane_id] = 0;
    if (threadIdx.x == 0 && C0.early_q) __hip_atomic_store(C0.bulk_live, 1ull, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_AGENT);
    /* a multi-rank warm-up: this rank's launch is resident (the job's start barrier) */
    if (threadIdx.x == 0 && C0.n_peers > 1 && C0.admit_n != 0) atomicOr(C0.in_flight, WARM_STARTED);
    __syncthreads();
    Cold *cold = C0.cold + gtid;
    const unsigned long long rt_start = __builtin_amdgcn_s_memrealtime();
    unsigned long long wave_trips = 0;
    Lane L;
    L.rng.k0 = C0.key0;
    L.rng.k1 = C0.key1;
    bool active = false;
    /* a failed argument check ends the wave at its first trip (the exit path uses C0 only) */
    const bool karg_bad = !kargs_check(ka, P0, C0);
    if (karg_bad && lane_id == 0) atomicAdd(&C0.ctr->karg_bad, 1ull);
    bool pool_done = karg_bad;   /* wave-uniform */
    unsigned long long res_next = 0, res_end = 0; /* wave-uniform: reserved claim positions */
    bool head_done = false;      /* wave-uniform: the pool head has passed pos_end */
    bool warm = !karg_bad && C0.admit_n != 0; /* wave-uniform: warm-up admission in force */
    /* wave-uniform: every rank of the job has started this pass (or the wait gave up); one GPU: true */
    bool started_all = !(C0.n_peers > 1 && C0.admit_n != 0 && C0.start_wait_ticks != 0);
    unsigned wait_trips = 0;     /* consecutive trips idle waiting for admission */
    L.flight() = 0;
    /* wave-uniform; refreshed every trip during the warm-up and every REFRESH_TRIPS trips after it
     * (the device-coherent counters cost a cross-die round trip; past the warm-up they move by
     * parts per million between refreshes) */
    double bias_d = bias_den(P0, C0);
    unsigned trip = 1;
    /* per-lane launch counters, 32-bit in the loop (a lane makes < 2^32 steps per launch), widened
     * for the wave reduction at exit */
    L.c_tracked() = L.c_primaries() = L.c_children() = 0;
    unsigned long long wave_steps = 0; /* wave-uniform: transport steps the wave's lanes completed */
    L.c_nstep_max() = L.c_long() = 0; /* longest photon life; lives > 100k steps */
    const unsigned long long lt_mask = (lane_id == 0) ? 0ull : (~0ull >> (64 - lane_id));

    while (true) {
        KArgsK *const kt = karg_fresh(ka); /* one opaque pointer for both (two would both spill) */
        const Params &P = karg_params(kt);
        const Ctl &C = karg_ctl(kt);
        ++wave_trips;
        TCOUNT(4);
        if (warm && (blockIdx.x >= WARM_BLOCKS || (unsigned)wave >= WARM_WAVES)) {
            /* the warm-up's admission batches are small: the waves of the first WARM_BLOCKS
             * workgroups take them, the rest wait here without touching the counters (their polling
             * would contend with the warm-up's own counter traffic) until the admission is over */
            unsigned long long end = 0;
            if (lane_id == 0) end = __hip_atomic_load(C.admit_end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__builtin_amdgcn_readfirstlane((int)(end >> 32)) != -1 ||
                __builtin_amdgcn_readfirstlane((int)end) != -1) {
#pragma unroll
                for (int z = 0; z < GRM_PARK_SLEEPS; ++z) __builtin_amdgcn_s_sleep(127);
                continue;
            }
            warm = false;
            if (!C.bias_frozen) bias_d = bias_den(P, C);
        }
        if ((trip++ & (REFRESH_TRIPS - 1)) == 0 || warm) {
            flush_counters(C);
            if (!C.bias_frozen) bias_d = bias_den(P, C);
            if (C.watchdog_ticks) {
                bool stop = __hip_atomic_load(&C.ctr->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
                if (!stop && __builtin_amdgcn_s_memrealtime() - rt_start > C.watchdog_ticks) {
                    stop = true;
                    if (lane_id == 0) __hip_atomic_store(&C.ctr->abort, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (stop) { /* abandon: drop the lane photons, the wave's stack and the pool; exit */
                    /* end the admission too, so that waves parked for it wake up and exit */
                    if (lane_id == 0) __hip_atomic_store(C.admit_end, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (lane_id == 0 && C.n_peers > 1) atomicOr(C.in_flight, WARM_DONE);
                    if (active) {
                        record_stuck(C, L);
                        atomicAdd(&C.ctr->n_abandoned, 1ull);
                        active = false;
                    }
                    pool_done = true;
                    warm = false;
                    if (lane_id == 0) *wtop = 0;
                }
            }
            TSTAMP(7);
        }
        if (__builtin_amdgcn_readfirstlane(s_recn[wave]) >= RECBUF_FLUSH) flush_records(C);
        /* Refill (converged point).  A primary needs only its loads here (its set-up runs in the
         * trip, phase 3), so idle lanes take primaries as soon as refill_min of them are idle.  A
         * child needs the divergent scattering sampling (sample_child), so children go in batches:
         * once child_min wait on the wave's stack, the wave stops taking primaries until as many
         * lanes are idle and samples them together (stack order: depth-first, like the reference's
         * recursion, harm_model.cpp:1023).  With no lane active, or once the pool is drained, the
         * wave refills whatever it can. */
        const unsigned long long idle = __ballot(!active);
        if (idle) {
            int top = *wtop;
            if (top > WSTACK_CAP) top = WSTACK_CAP;
            const int n_idle = __popcll(idle);
            const bool none_active = idle == __ballot(1);
            const bool child_due = top >= C.child_min || (pool_done && top > 0);
            int k_child = 0, k_pool = 0;
            bool go;
            if (none_active || child_due) {
                k_child = n_idle < top ? n_idle : top;
                k_pool = pool_done ? 0 : n_idle - k_child;
                go = none_active || n_idle >= min(C.child_min, top);
            } else {
                k_pool = pool_done ? 0 : n_idle;
                go = k_pool >= C.refill_min;
            }
            if (go) {
                const int r = __popcll(idle & lt_mask);
                unsigned long long base = 0;
                if (k_pool > 0) {
                    if (warm) {
                        /* warm-up: claim only inside the admitted batch (CAS); once it is claimed and
                         * nothing is in flight, one wave admits the next batch.  In a multi-rank job
                         * the gate is the job's: every rank's flight against every rank's admitted
                         * photons (warm_job), so the ranks' batches interleave as one GPU's would
                         * (each rank gating on its own flight let the job run ahead of its history:
                         * +5 % recorded at 8 ranks) */
                        long long got = 0;
                        int off = 0;
                        const bool job = C.n_peers > 1;
                        unsigned long long j_hist = 0;
                        long long j_flight = 0;
                        if (job) warm_job(C, j_hist, j_flight);
                        if (!started_all)
                            started_all = job_started(C) || __builtin_amdgcn_s_memrealtime() - rt_start > C.start_wait_ticks;
                        const unsigned long long unit = job ? WARM_HIST + 1 : 1; /* admitted + in flight */
                        if (lane_id == 0) {
                            const unsigned long long end =
                                __hip_atomic_load(C.admit_end, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (end == ~0ull) {
                                off = 1;
                            } else if (!started_all) {
                                /* the job's start barrier: no claim until every rank's launch runs */
                            } else {
                                const unsigned long long head =
                                    __hip_atomic_load(C.pool_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                base = head;
                                if (head < end) {
                                    unsigned long long want = min((unsigned long long)k_pool, end - head);
                                    if (C.admit_spread) want = min(want, C.admit_spread);
                                    atomicAdd(C.in_flight, want * unit); /* before the claim is visible */
                                    if (atomicCAS(C.pool_head, head, head + want) == head)
                                        got = (long long)want;
                                    else
                                        atomicAdd(C.in_flight, (unsigned long long)(-(long long)(want * unit)));
                                } else if (job ? (unsigned long long)j_flight <= (j_hist >> C.admit_slack)
                                               : __hip_atomic_load(C.in_flight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <=
                                                     ((C.admit_h0 + end) >> C.admit_slack)) {
                                    /* the next batch once all but a straggler fraction of the history
                                     * has ended: the counters then hold nearly all of it, and one
                                     * long-lived photon does not hold the warm-up up */
                                    /* one GPU: the batch doubles the history, up to admit_lim.  A job
                                     * (n_peers ranks): this rank's share of a batch that doubles the JOB's
                                     * admitted photons, and the admission ends for every rank when the job's
                                     * reach admit_lim (= n_peers x one GPU's); sized from its own history, a
                                     * rank that won a few gate openings ran its batches ahead of the others
                                     * and left the warm-up early, on a history far shorter than the job's
                                     * in flight (+4-5 % recorded at 2-8 emulated ranks, round 4) */
                                    const unsigned long long h = job ? j_hist : C.admit_h0 + end;
                                    const unsigned long long grow =
                                        job ? min(h, C.admit_lim - min(h, C.admit_lim)) / (unsigned long long)C.n_peers
                                            : min(h, C.admit_lim - h);
                                    const unsigned long long next =
                                        (end >= C.admit_n || (job && h >= C.admit_lim))
                                            ? ~0ull
                                            : min(C.admit_n, end + max(C.admit_b0, grow));
                                    const bool opened = atomicCAS(C.admit_end, end, next) == end;
                                    if (opened && next == ~0ull && job) atomicOr(C.in_flight, WARM_DONE);
                                    if (opened && C.phases) {
                                        const unsigned long long t = __builtin_amdgcn_s_memrealtime();
                                        if (next == ~0ull) C.phases[0] = t;
                                        /* the admission log: [3 + 2k] when batch k + 1 opened, [4 + 2k]
                                         * the photons then in flight */
                                        const unsigned long long k = atomicAdd(C.phases + 2, 1ull);
                                        if (k < (PHASE_LOG - 3) / 2) {
                                            C.phases[3 + 2 * k] = t;
                                            /* photons in flight: a multi-rank pass block packs them into
                                             * the signed low word of its warm-up state (see DevCounters) */
                                            const unsigned long long f =
                                                __hip_atomic_load(C.in_flight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                            const long long fl = job ? (long long)(int)(unsigned)f : (long long)f;
                                            C.phases[4 + 2 * k] = (unsigned long long)(fl < 0 ? 0 : fl);
                                        }
                                    }
                                }
                            }
                        }
                        if (__shfl(off, 0)) {
                            warm = false; /* admission over: plain claims from here on */
                        } else {
                            base = __shfl(base, 0);
                            k_pool = (int)__shfl(got, 0);
                            if (k_pool > 0 && base + k_pool >= C.pos_end) pool_done = true;
                        }
                    }
                    if (!warm) {
                        /* the wave's reservation of claim positions: one global atomic per RES_CHUNK
                         * positions instead of one per refill (2048 waves refilling a few lanes every
                         * ~20 trips would queue on the pool head's single address) */
                        if (res_next >= res_end) {
                            unsigned long long b = 0;
                            if (lane_id == 0) b = atomicAdd(C.pool_head, (unsigned long long)RES_CHUNK);
                            b = __shfl(b, 0);
                            res_next = b;
                            res_end = min(b + RES_CHUNK, C.pos_end);
                            head_done = b + RES_CHUNK >= C.pos_end;
                            if (C.phases && lane_id == 0 && b < C.pos_end && head_done)
                                C.phases[1] = __builtin_amdgcn_s_memrealtime(); /* the one wave of the last chunk */
                        }
                        base = res_next;
                        k_pool = res_end > res_next ? (int)min((unsigned long long)k_pool, res_end - res_next) : 0;
                        res_next += k_pool;
                        if (head_done && res_next >= res_end) pool_done = true;
                    }
                }
                if (lane_id == 0) *wtop = top - k_child;
#ifdef GRM_TIMING
                if (k_child) TCOUNT(5);
                if (k_pool) TCOUNT(6);
#endif
                TSTAMP(14);
                bool has = false, ok = true;
                if (!active && r < k_child) {
                    SReq R;
                    load_sreq(wstack + (top - 1 - r), R);
                    ok = sample_child(P, C, R, L, cold);
                    if (!ok && C.trace)
                        write_trace(C, cold, R.id, R.w, R.x[1], R.x[2], R.x[3], 0.0, 0.0, R.n_scatt, 0, 4, -1, -1);
                    has = true;
                }
                TSTAMP(0);
                if (!active && r >= k_child && r - k_child < k_pool) {
                    const unsigned long long pos = base + (unsigned long long)(r - k_child);
                    const unsigned long long idx =
                        (pos & ((1ull << C.pool_sh) - 1)) * C.pool_m + (pos >> C.pool_sh);
                    if (pos < C.pos_end && idx >= C.n_pool) --L.flight(); /* a hole: claimed, ends at once */
                    if (pos < C.pos_end && idx < C.n_pool) {
                        if (C.pool_kind == 0) {
                            load_primary(C, idx, L, cold);
                            ++L.c_primaries();
                        } else {
                            SReq R;
                            load_sreq(reinterpret_cast<const SReq *>(C.pool) + idx, R);
                            ok = sample_child(P, C, R, L, cold);
                            if (!ok && C.trace)
                                write_trace(C, cold, R.id, R.w, R.x[1], R.x[2], R.x[3], 0.0, 0.0, R.n_scatt, 0, 4,
                                            -1, -1);
                        }
                        has = true;
                    }
                }
                if (has) {
                    ++L.c_tracked();
                    if (ok) active = init_photon(C, cold, L, ph2);
                    if (!active) --L.flight(); /* started and ended at once (invalid) */
                }
                TSTAMP(1);
            }
        }
        if (!__any(active)) {
            if (warm) {
                int d = L.flight(); /* flush before waiting: the barrier needs everyone's ends */
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
                if (lane_id == 0 && d) atomicAdd(C.in_flight, (unsigned long long)(long long)d);
                L.flight() = 0;
            }
            if (pool_done && *wtop == 0) break;
            if (warm) {
                /* waiting for the next batch; a barrier that never opens (it cannot, short of a
                 * counting bug) must not hang the GPU: after ~1 s give the warm-up up for all */
                if (++wait_trips > (1u << 21) && lane_id == 0) {
                    __hip_atomic_store(C.admit_end, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (C.n_peers > 1) atomicOr(C.in_flight, WARM_DONE);
                }
                __builtin_amdgcn_s_sleep(16);
            }
            continue;
        }
        wait_trips = 0;
        /* a photon that has run early_steps steps goes to the concurrent early_kernel at the top of
         * a step (one lane-loop trip is ~7 us per step for it, the pair ~1.8 us) */
        if (C.early_q && !warm) {
            const bool early = active && L.phase == 0 && L.n_step >= C.early_steps;
            /* a full queue is read, not claimed: past early_cap every such lane would add to the one
             * tail word on every trip for the rest of the launch */
            if (__ballot(early) && __hip_atomic_load(C.early_live, __ATOMIC_SEQ_CST, __HIP_MEMORY_SCOPE_AGENT) == 1 &&
                __hip_atomic_load(C.early_tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < C.early_cap && early) {
                const unsigned long long slot = atomicAdd(C.early_tail, 1ull);
                if (slot < C.early_cap) {
                    export_lone(C.early_q + slot, L, cold);
                    __threadfence();
                    __hip_atomic_store(C.early_ready + slot, C.early_tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    active = false;
                }
            }
        }
        /* the tail: this wave's only work left is one photon -- hand it to the lone-photon kernel at
         * the top of a step (in the test mode GRM_OPT_LONE = 2: every photon at the top of its
         * first step); halving_walk finishes a push already in progress with the whole wave */
        bool walked = false, ended = false;
        const bool tail = pool_done && !warm;
        if (tail || C.lone_all) {
            const unsigned long long act = __ballot(active);
            const int n_act = __popcll(act);
            const bool alone = n_act == 1 && *wtop == 0;
            if (C.lone && (alone || C.lone_all)) {
                /* a full hand-over queue is read, not claimed, and the photons stay in the lane loop
                 * (claiming past the cap and skipping the trip would retry forever) */
                const bool hand = active && L.phase == 0 &&
                                  __hip_atomic_load(C.lone_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < C.lone_cap;
                if (__ballot(hand)) {
                    unsigned long long slot = ~0ull;
                    if (hand) slot = atomicAdd(C.lone_count, 1ull);
                    const bool handed = hand && slot < C.lone_cap;
                    if (handed) {
                        export_lone(C.lone + slot, L, cold);
                        active = false;
                    }
                    if (__ballot(handed)) continue; /* the rest reach the top of a step on later trips */
                }
            }
            if (tail && alone) {
                const int owner = __ffsll((long long)act) - 1;
                int walk = 0;
                if (active) {
                    if (L.phase == 0 && !trip_begin(P, C, L, cold, ph2))
                        ended = true;
                    else
                        walk = (L.phase == 1 || L.phase == 2) ? 1 : 0;
                }
                if (__builtin_amdgcn_readlane(walk, owner)) {
                    halving_walk(P, L, owner);
                    walked = true;
                }
            }
        }
        bool stepped = false;
        if (active) {
            active = !ended && transport_trip(P, C, L, cold, wstack, wtop, ph2, bk, bias_d, walked, stepped);
            if (!active) {
                L.c_nstep_max() = max((int)L.c_nstep_max(), L.n_step);
                L.c_long() += L.n_step > 100000 ? 1 : 0;
                --L.flight();
            }
        }
        wave_steps += (unsigned long long)__popcll(__ballot(stepped)); /* scalar: no LDS round trip per step */
        if (warm) {
            int d = L.flight();
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
            if (lane_id == 0 && d) atomicAdd(C.in_flight, (unsigned long long)(long long)d);
            L.flight() = 0;
        }
        TSTAMP(2);
    }
#ifdef GRM_TIMING
    if (lane_id == 0) {
        g_tlds[threadIdx.x >> 6][3] = __builtin_amdgcn_s_memtime() - t_start;
        for (int r = 0; r < 15; ++r) atomicAdd(C0.timing + r, g_tlds[threadIdx.x >> 6][r]);
        for (int r = 16; r < 24; ++r) atomicAdd(C0.timing + 16 + r, g_tlds[threadIdx.x >> 6][r]);
    }
#endif
    const Ctl &C = C0;
    /* counters, the buffered records, then the workgroup's spectrum, to the global accumulators */
    flush_counters(C);
    flush_records(C);
    __syncthreads();
    double *slice = spec_slice(C);
    for (int i = threadIdx.x; i < SPEC_LDS; i += BLOCK) {
        /* the slice was accumulated by memory-side atomics; read it there and leave it zero for the
         * next launch (padding fields 12..15 stay zero) */
        if ((i & (SPEC_CELL - 1)) >= SPEC_FIELDS) continue;
        const double v = __hip_atomic_load(slice + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v != 0.0) slice[i] = 0.0;
        if (v != 0.0) unsafeAtomicAdd(reinterpret_cast<double *>(C.spec + i / SPEC_CELL) + (i & (SPEC_CELL - 1)), v);
    }
    /* wave-reduce the lane counters, one atomic per wave */
    unsigned long long w_tracked = (unsigned)L.c_tracked();
    unsigned long long w_primaries = (unsigned)L.c_primaries(), w_children = (unsigned)L.c_children();
    unsigned long long w_long = (unsigned)L.c_long(), w_nstep_max = (unsigned)L.c_nstep_max();
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        w_tracked += __shfl_xor(w_tracked, off);
        w_primaries += __shfl_xor(w_primaries, off);
        w_children += __shfl_xor(w_children, off);
        w_long += __shfl_xor(w_long, off);
        w_nstep_max = max(w_nstep_max, (unsigned long long)__shfl_xor(w_nstep_max, off));
    }
    if (lane_id == 0) {
        atomicAdd(&C.ctr->n_steps, wave_steps);
        atomicAdd(&C.ctr->n_tracked, w_tracked);
        atomicAdd(&C.ctr->n_primaries, w_primaries);
        atomicAdd(&C.ctr->n_children, w_children);
        if (w_long) atomicAdd(&C.ctr->n_long, w_long);
        atomicMax(&C.ctr->max_nstep, w_nstep_max);
        if (C.waves) {
            unsigned long long *wr = C.waves + (gtid >> 6) * 4;
            wr[0] = rt_start;
            wr[1] = __builtin_amdgcn_s_memrealtime();
            wr[2] = wave_trips;
            wr[3] = w_tracked;
        }
    }
    if (C.early_q) { /* the last workgroup out tells early_kernel that no hand-over will follow */
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence();
            if (atomicAdd(C.wg_exit, 1ull) == gridDim.x - 1)
                __hip_atomic_store(C.early_done, 1ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

/* Stream-ordered control of the small device words, so that a pass needs no copy or fill
 * (ROCclr blit) kernels: one workgroup sets the words a launch starts from (and, on a reset, the
 * counters and the whole spectrum, grid-stride), then mirrors the counters and the small words into
 * host-mapped memory, which the host reads after the stream synchronises. */
struct CtlOp {
    DevCounters *ctr;
    unsigned long long *small; /* grm_engine::d_small */
    double *spec;              /* zeroed on a reset (n_spec doubles) */
    size_t n_spec;
    DevCounters *h_ctr;        /* host-mapped mirrors (null: no mirror) */
    unsigned long long *h_small;
    unsigned long long val[16]; /* small[i] = val[i] for the bits of set */
    unsigned set;
    int reset, clear_abort;
    unsigned long long max_tau_init_bits;
    int set_warm;                  /* ctr->warm = warm_val (a multi-rank job's warm-up start) */
    unsigned long long warm_val;
};

/* one pass's results into slot `slot` of the stash (grm_engine_stash): the spectrum, then the
 * counters split by their reduction (sum: recorded, scattered, steps, tracked, children, overflow,
 * dropped, primaries, lives > 1e5; max: max tau_scatt bits, longest life) */
constexpr int STASH_SUMS = 9, STASH_MAXS = 2;
__global__ __launch_bounds__(256) void stash_kernel(const double *spec, const DevCounters *ctr, double *st_spec,
                                                    unsigned long long *st_sum, unsigned long long *st_max, int slot,
                                                    int ncell) {
    double *dst = st_spec + (size_t)slot * ncell;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < ncell; i += gridDim.x * 256) dst[i] = spec[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        unsigned long long *s = st_sum + (size_t)slot * STASH_SUMS, *m = st_max + (size_t)slot * STASH_MAXS;
        s[0] = ctr->n_recorded;
        s[1] = ctr->n_scatt;
        s[2] = ctr->n_steps;
        s[3] = ctr->n_tracked;
        s[4] = ctr->n_children;
        s[5] = ctr->n_overflow;
        s[6] = ctr->n_dropped;
        s[7] = ctr->n_primaries;
        s[8] = ctr->n_long;
        m[0] = ctr->max_tau_bits;
        m[1] = ctr->max_nstep;
    }
}

/* the job's bias counters as bias_den forms them (grm_engine_job_counters; tests of the peer mapping) */
__global__ __launch_bounds__(64) void job_counters_kernel(Params P, Ctl C, double *out) {
    const double den = bias_den(P, C);
    unsigned long long sc = 0, rc = 0, mt = 0;
    const int lane = (int)threadIdx.x;
    if (lane < C.n_peers) {
        const DevCounters *pc = C.peers[lane] + C.ctr_slot;
        sc = __hip_atomic_load(&pc->n_scatt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        rc = __hip_atomic_load(&pc->n_recorded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        mt = __hip_atomic_load(&pc->max_tau_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sc += __shfl_xor(sc, o);
        rc += __shfl_xor(rc, o);
        mt = max(mt, (unsigned long long)__shfl_xor(mt, o));
    }
    if (lane == 0) {
        out[0] = den;
        out[1] = (double)sc;
        out[2] = (double)rc;
        out[3] = __longlong_as_double((long long)mt);
    }
}

__global__ __launch_bounds__(256) void ctl_kernel(CtlOp op) {
    if (op.reset)
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < op.n_spec; i += (size_t)gridDim.x * 256)
            op.spec[i] = 0.0;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (op.reset) {
        unsigned long long *c = reinterpret_cast<unsigned long long *>(op.ctr);
        for (int i = 0; i < 16; ++i) c[i] = 0;
        op.ctr->max_tau_bits = op.max_tau_init_bits;
    }
    if (op.clear_abort) op.ctr->abort = 0;
    if (op.set_warm) op.ctr->warm = op.warm_val;
    for (int i = 0; i < 16; ++i)
        if ((op.set >> i) & 1u) op.small[i * SMALL_STRIDE] = op.val[i];
    if (op.h_ctr) {
        const unsigned long long *c = reinterpret_cast<const unsigned long long *>(op.ctr);
        unsigned long long *h = reinterpret_cast<unsigned long long *>(op.h_ctr);
        for (int i = 0; i < 16; ++i) h[i] = c[i];
        for (int i = 0; i < 16; ++i) op.h_small[i] = op.small[i * SMALL_STRIDE];
        __threadfence_system();
    }
}

} /* namespace */

/* lone_kernel / early_kernel live in grm_lone.hip (a unit compiled without
 * -disable-machine-licm, see there); Params and Ctl cross as bytes */
extern "C" hipError_t grm_lone_launch(int which, unsigned grid, hipStream_t s, const void *P, size_t p_size,
                                      const void *C, size_t c_size);
#ifdef GRM_WITH_SPLIT
/* split_kernel lives in grm_split.hip (the bulk transport with geometry and interaction waves): an
 * experiment that lost, built only into variant libraries (tools/build_variant.sh) */
extern "C" hipError_t grm_split_launch(unsigned grid, hipStream_t s, const void *P, size_t p_size, const void *C,
                                       size_t c_size);
#endif

/* ========================================================================= */
/* engine object + C ABI                                                      */
/* ========================================================================= */
struct grm_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
    Params P{};
    double *d_zones = nullptr, *d_hot = nullptr, *d_k2 = nullptr;
    DevCounters *d_ctr = nullptr;       /* the counter block in use: d_ctr_own, or a pass slot */
    DevCounters *d_ctr_own = nullptr;   /* allocated with the engine */
    DevCounters *d_ctr_slots = nullptr; /* per-pass blocks (grm_engine_stash_reserve), shared with peers */
    int n_ctr_slots = 0, ctr_slot = -1;
    const DevCounters **d_peers = nullptr; /* device array: every rank's d_ctr_slots */
    int n_peers = 0;
    std::vector<void *> ipc_open;           /* peers' blocks opened by IPC (closed at destroy) */
    grm_spectrum_cell *d_spec = nullptr;
    SReq *d_stack = nullptr;
    Cold *d_cold = nullptr;
    size_t lanes = 0;
    int grid = 0;
    SReq *d_ovf[2] = {nullptr, nullptr};
    unsigned long long ovf_cap = 0;
    unsigned long long *d_small = nullptr; /* [0] pool head, [1..2] ovf counts, [3] trace count,
                                              [4] warm-up in flight, [5] warm-up admitted end */
    grm_init_photon *d_batch = nullptr;
    size_t batch_cap = 0;
    grm_trace *d_trace = nullptr;
    unsigned long long trace_cap = 0;
    /* cell sums binned from the trace (grm_engine_cell_sums_*): records [0, trace_consumed) are in
     * the accumulator, GRM_CELLSUMS_DOUBLES doubles and then the skipped-record word; allocated by
     * the first accumulate */
    unsigned long long trace_consumed = 0;
    double *d_cellsums = nullptr;
    /* the trace re-binned on a caller's grid (grm_engine_rebin_*): records [0, rebin_consumed) are in
     * d_rebin, rebin_doubles doubles and then the out-of-grid word; d_rebin_keys: the key pass's
     * scratch, one word per record of the trace buffer (allocated by the first accumulate) */
    bool rebin_on = false;
    grm_bin_grid rebin_grid{};
    double *d_rebin = nullptr;
    size_t rebin_doubles = 0;
    unsigned long long rebin_consumed = 0;
    uint32_t *d_rebin_keys = nullptr;
    unsigned long long rebin_keys_cap = 0;
    double rebin_ms[2] = {0.0, 0.0}; /* key pass, slice passes of the last accumulate */
    uint64_t seed = 123;
    int bias_mode = 0;
    uint64_t id_base = 0;
    int grid_override = 0;
    int64_t flight_ratio = 96; /* GRM_OPT_FLIGHT_RATIO: a live-bias call of n photons runs on <= n / this lanes */
    int split = 0;             /* GRM_OPT_SPLIT: the bulk launch is split_kernel (grm_split.hip) */
    int split_thr = 48, split_spin = 4, split_gthr = 24; /* GRM_OPT_SPLIT_THR / _SPIN / _GTHR (profiles/r05_split) */
    int split_batch = 1; /* GRM_OPT_SPLIT_BATCH */
    double max_tau_init = 0.0;
    bool frozen_set = false;
    /* photons; -1 = lanes; -2 (default) = auto: lanes for a call of fewer than WARMUP_AUTO_RATIO x lanes
     * photons, else WARMUP_PHOTONS (profiles/r03d_warmup_rank_sweep_1e5.log) */
    int64_t warmup = -2;
    int warmup_slack = -1; /* log2; -1 (default) = auto: 4 when the warm-up ramps to a grid of lanes, else 1 */
    int refill_min = 2;      /* primaries: set-up is in the trip (phase 3), so refill early */
    int child_min = 8;       /* children: batch the divergent scattering sampling */
    uint64_t history = 0;    /* primaries tracked since reset */
    double fz_scatt = 0.0, fz_rec = 0.0, fz_maxtau = 0.0;
    grm_stats stats{};
    grm_init_photon *d_upload = nullptr;
    size_t upload_cap = 0;
    ncclComm_t comm = nullptr;
    /* deferred reduction of a job's passes (grm_engine_stash*): per slot the spectrum, 9 summed
     * counters and 2 max counters */
    double *d_stash_spec = nullptr;
    unsigned long long *d_stash_sum = nullptr, *d_stash_max = nullptr;
    int stash_cap = 0;
    unsigned long long *d_timing = nullptr;
    unsigned long long *d_waves = nullptr; /* [lanes / 64][4] per-wave record of the last launch */
    int64_t watchdog_ms = 60000;           /* per-launch watchdog (GRM_OPT_WATCHDOG_MS; 0 = off) */
    double *d_stuck = nullptr;             /* [STUCK_CAP][STUCK_WORDS] abandoned-photon records */
    double *d_spec_blocks = nullptr;       /* per-workgroup spectrum slices */
    LoneRec *d_lone = nullptr;             /* photons handed over to lone_kernel */
    unsigned long long lone_cap = 0;
    int lone = 1;                          /* GRM_OPT_LONE */
    /* early hand-over of long photons to early_kernel on a second stream (GRM_OPT_EARLY_STEPS): 1,500
     * (~100 photons a bench pass) rather than 5,000 (~1): frozen-bias replays of the tail passes end
     * 14-48 ms sooner, the others unchanged; 1,000 fills the 1,024-slot queue */
    int early_steps = 1500;
    /* GRM_OPT_JOB_START_WAIT_MS: default 0.  Ranks of a real multi-GPU job run their passes back to back
     * without a host barrier between passes (bench.py), so a rank held up by a long photon would stall
     * every other rank's next warm-up; the one-GPU emulation of N ranks, whose launches queue behind
     * each other, sets it (tests/multirank_emu.py) */
    int64_t job_start_wait_ms = 0;
    /* The queue has EARLY_CAP slots, claimed once per launch.  The photons reaching S steps fall off
     * steeply with S (per 14.5 M-photon bench pass: ~680 at 1,200 steps, ~110 at 1,500, ~10 at
     * 2,000, ~1 at 5,000 -- about S^-8.5), so a call of many more photons (a configs[3] shard, 1.8e8
     * in one call) would fill the queue at 1,500 and keep its later long photons in the lane loop.
     * The threshold therefore grows with the call past 16 M photons as (n / 16 M)^(1/8.5): the same
     * expected hand-overs per call (~100-150) as a bench pass, 1,500 -> ~2,000 for a 1.8e8 shard. */
    static int early_steps_for(int base, size_t n) {
        const double ref = 16.0e6;
        if (base <= 0 || (double)n <= ref) return base;
        const double s = (double)base * std::pow((double)n / ref, 1.0 / 8.5);
        return s > (double)(1 << 30) ? (1 << 30) : (int)s;
    }
    bool early_serial = false; /* test: the worker ahead of the main launch on its stream */
    int early_children = 1;    /* GRM_OPT_EARLY_CHILDREN: the worker tracks its photons' children itself */
    int karg_test = 0;         /* test: GRM_OPT_KARG_TEST */
    static constexpr unsigned long long EARLY_CAP = 1024;
    LoneRec *d_early = nullptr;
    unsigned long long *d_early_ready = nullptr;
    /* the lone kernel's children queue (Ctl::lk_*): LK_CAP slots, their ready tags, and the five words
     * tail, taken, active, standby, originals finished (one per SMALL_STRIDE), cleared before every
     * lone launch */
    static constexpr unsigned long long LK_CAP = 4096;
    LoneRec *d_lk = nullptr;
    unsigned long long *d_lk_ready = nullptr, *d_lk_words = nullptr; /* words: 5 x SMALL_STRIDE */
    unsigned long long launch_seq = 0;
    size_t waves_rows = 0; /* rows of d_waves the last recorded launch wrote */
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_pre = nullptr, ev_w = nullptr;
    unsigned long long warmup_b0 = 64;     /* GRM_OPT_WARMUP_BATCH */
    /* GRM_OPT_WARMUP_SPREAD: 4 photons per wave claim spread a batch over 4-16x more waves, so the
     * families of its photons (the first photons' bias is large: long scattering cascades, each on
     * its wave's stack) get more lanes each -- the warm-up of a photon_n = 1e6 pass ends at ~28 ms
     * instead of ~49, recorded unchanged within 1.3 % (12 passes per setting, profiles/r03_ab/
     * r03p_warmup_spread_*.log; 1: 41 ms, 2: 32, 8: 29, 16: 31).  -1 (default) = auto: 4 for the
     * WARMUP_PHOTONS warm-up; none for the ramp to a grid of lanes (its batches outnumber the
     * warm-up's lanes) */
    int64_t warmup_spread = -1;
    /* host-mapped control block: ctl_kernel mirrors the counters and the small words here (ctr,
     * small) and the emission scan writes its total (word[4]); the host reads them after a stream
     * synchronisation, so a pass runs without copy or fill kernels (see ctl_kernel) */
    struct Pinned {
        DevCounters ctr;
        unsigned long long small[16];
        unsigned long long word[8];
    } *pin = nullptr;
    /* device emission: zone table, emission tables, zone offsets, emitted photons */
    grm_emit_zone *d_ezones = nullptr;
    double *d_eweight = nullptr, *d_ef = nullptr;
    unsigned long long *d_eoff = nullptr;
    int64_t n_ezones = 0;
    grm_init_photon *d_emit = nullptr;
    size_t emit_cap = 0;
    std::string err;
};

namespace {

bool hip_ok(grm_engine *e, hipError_t st, const char *what) {
    if (st == hipSuccess) return true;
    if (e) e->err = std::string(what) + ": " + hipGetErrorString(st);
    return false;
}

#define HIPCHK(e, call)                                   \
    do {                                                  \
        if (!hip_ok((e), (call), #call)) return -1;       \
    } while (0)

/* one ctl_kernel launch on the engine stream (op: the words to set; the mirror is always made) */
int ctl(grm_engine *e, CtlOp op, bool sync) {
    op.ctr = e->d_ctr;
    op.small = e->d_small;
    op.h_ctr = &e->pin->ctr;
    op.h_small = e->pin->small;
    unsigned blocks = 1;
    if (op.reset) {
        op.spec = reinterpret_cast<double *>(e->d_spec);
        op.n_spec = sizeof(grm_spectrum_cell) / sizeof(double) * N_TH_BINS * N_E_BINS;
        blocks = (unsigned)((op.n_spec + 255) / 256);
        std::memcpy(&op.max_tau_init_bits, &e->max_tau_init, sizeof(double));
    }
    hipLaunchKernelGGL(ctl_kernel, dim3(blocks), dim3(256), 0, e->stream, op);
    HIPCHK(e, hipGetLastError());
    if (sync) HIPCHK(e, hipStreamSynchronize(e->stream));
    return 0;
}

/* the device counters, through the host-mapped mirror */
int read_counters(grm_engine *e, DevCounters &h) {
    if (ctl(e, CtlOp{}, true)) return -1;
    h = e->pin->ctr; /* written by the device before the synchronisation returned */
    return 0;
}

int alloc_lanes(grm_engine *e) {
    int n_cu = 0;
    HIPCHK(e, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, e->device));
    int per_cu = 0;
    HIPCHK(e, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, track_kernel, BLOCK, 0));
    if (per_cu < 1) per_cu = 1;
    int grid = e->grid_override > 0 ? e->grid_override : n_cu * per_cu;
    if (grid < 1) grid = 1;
    const size_t lanes = (size_t)grid * BLOCK;
    if (lanes != e->lanes) {
        if (e->d_stack) (void)hipFree(e->d_stack);
        if (e->d_cold) (void)hipFree(e->d_cold);
        e->d_stack = nullptr;
        e->d_cold = nullptr;
        HIPCHK(e, hipMalloc(&e->d_stack, lanes * STACK_DEPTH * sizeof(SReq)));
        HIPCHK(e, hipMalloc(&e->d_cold, lanes * sizeof(Cold)));
        if (e->d_waves) (void)hipFree(e->d_waves);
        e->d_waves = nullptr;
        /* + PHASE_LOG words: the launch's phase stamps (grm_engine_debug_phases / _admissions) */
        HIPCHK(e, hipMalloc(&e->d_waves, (lanes / 64 * 4 + PHASE_LOG) * sizeof(unsigned long long)));
        if (e->d_spec_blocks) (void)hipFree(e->d_spec_blocks);
        e->d_spec_blocks = nullptr;
        HIPCHK(e, hipMalloc(&e->d_spec_blocks, (size_t)grid * SPEC_LDS * sizeof(double)));
        HIPCHK(e, hipMemset(e->d_spec_blocks, 0, (size_t)grid * SPEC_LDS * sizeof(double)));
        /* at most one hand-over per wave per launch (one per lane and launch's photon in the test
         * mode GRM_OPT_LONE = 2, sized in run_passes) */
        if (e->d_lone) (void)hipFree(e->d_lone);
        e->d_lone = nullptr;
        e->lone_cap = lanes / 64;
        HIPCHK(e, hipMalloc(&e->d_lone, e->lone_cap * sizeof(LoneRec)));
        e->lanes = lanes;
    }
    e->grid = grid;
    return 0;
}

int ensure_ovf(grm_engine *e, unsigned long long cap) {
    if (cap <= e->ovf_cap) return 0;
    for (int i = 0; i < 2; ++i) {
        if (e->d_ovf[i]) hipFree(e->d_ovf[i]);
        e->d_ovf[i] = nullptr;
        HIPCHK(e, hipMalloc(&e->d_ovf[i], cap * sizeof(SReq)));
    }
    e->ovf_cap = cap;
    return 0;
}

/* Live-bias warm-up size (GRM_OPT_WARMUP = -2, the default).  The counters bias_func reads lag the
 * claims by the photons in flight (~lanes): while the history is short against that, photons start
 * on a bias the serial reference never had.  A call of fewer than WARMUP_AUTO_RATIO x lanes photons
 * (photon_n = 1e5 on one GPU: 11 x lanes) ramps admission until the history reaches a grid's worth
 * of lanes: recorded +6.1 % -> +1.8 % against the oracle at 192^2, photon_n = 1e5, for +73 ms per
 * pass (16 seeds, profiles/r03d_warmup_rank_sweep_1e5.log; 16 k and 64 k photons did not move it).
 * A larger call (the bench's photon_n = 1e6: 110 x lanes) keeps WARMUP_PHOTONS: its lag is ~1 % of
 * the pass, and the ramp would cost ~15 % of it. */
constexpr uint64_t WARMUP_AUTO_RATIO = 32, WARMUP_PHOTONS = 4096;
/* The barrier before each admission batch waits until in-flight <= history / 2^slack.  Slack 1
 * (1/2) instead of 4 (1/16) shortened a photon_n = 1e6 launch by ~30 ms, the recorded count within
 * the oracle's spread (17.6 / 17.0 M against 17.64 +- 0.55 M; profiles/r03_ab/r3k_*).  The
 * admission log (grm_engine_debug_admissions, profiles/r03_ab/r03o_*) then shows batches 2-7
 * opening within 0.3 ms and the end of the warm-up at ~48 ms: the last batch waits for the
 * scattering families of its photons (the first photons' bias is large), each on its own wave's
 * stack -- hence WARMUP_SPREAD photons per wave claim (~28 ms).  The ramp of small passes (above)
 * keeps 1/16: there the history it builds is the point. */
constexpr int WARMUP_SLACK_LARGE = 1;
constexpr unsigned long long WARMUP_SPREAD = 4;

/* one launch (+ overflow relaunches) over claim positions [pos0, pos1) of a batch of n primaries
 * interleaved as 2^sh runs of m (Ctl.pos_end) */
int run_passes(grm_engine *e, const grm_init_photon *d_batch, size_t n, int sh, uint64_t m, uint64_t pos0,
               uint64_t pos1, int grid) {
    if (pos1 <= pos0) return 0;
    /* overflow pool: children rarely spill (a 1,024-deep stack per wave): a few hundred per
     * photon_n = 1e6 pass, 213-238 for the 1.8e8-photon shard of BASELINE configs[3]; size
     * max(1M, n/32) -- 2 x 1.1 GB for that shard, so eight such engines fit one GPU (n/4 took
     * 2 x 8.8 GB each).  A child that fits nowhere is counted and fails the call (n_dropped). */
    if (ensure_ovf(e, std::max<unsigned long long>(1ull << 20, (pos1 - pos0) / 32))) return -1;
    if (e->lone == 2 && e->lone_cap < e->ovf_cap + n) { /* test mode: every photon may be handed over */
        if (e->d_lone) (void)hipFree(e->d_lone);
        e->d_lone = nullptr;
        e->lone_cap = e->ovf_cap + n;
        HIPCHK(e, hipMalloc(&e->d_lone, e->lone_cap * sizeof(LoneRec)));
    }
    Ctl C{};
    C.pool = d_batch;
    C.pool_kind = 0;
    C.n_pool = n;
    C.pos_end = pos1;
    C.pool_m = m;
    C.pool_sh = sh;
    C.pool_head = e->d_small + (0) * SMALL_STRIDE;
    C.id_base = e->id_base;
    C.key0 = (uint32_t)e->seed;
    C.key1 = (uint32_t)(e->seed >> 32);
    C.stack = e->d_stack;
    C.cold = e->d_cold;
    C.ovf_cap = e->ovf_cap;
    C.spec = e->d_spec;
    C.spec_blocks = e->d_spec_blocks;
    C.ctr = e->d_ctr;
    C.peers = e->d_peers;
    C.n_peers = (e->ctr_slot >= 0 && e->d_peers) ? e->n_peers : 0;
    C.ctr_slot = e->ctr_slot;
    C.trace = e->trace_cap ? e->d_trace : nullptr;
    C.trace_cap = e->trace_cap;
    C.trace_count = e->d_small + (3) * SMALL_STRIDE;
    C.timing = e->d_timing;
    C.refill_min = e->refill_min;
    C.child_min = e->child_min;
    C.lanes = (int)e->lanes;
    C.bias_frozen = e->bias_mode;
    /* a multi-rank job's flight goes to the pass block, where the other ranks' gates read it */
    C.in_flight = C.n_peers > 1 ? &e->d_ctr->warm : e->d_small + (4) * SMALL_STRIDE;
    C.admit_end = e->d_small + (5) * SMALL_STRIDE;
    C.watchdog_ticks = (unsigned long long)std::max<int64_t>(e->watchdog_ms, 0) * 100000ull; /* 100 MHz */
    C.start_wait_ticks = (unsigned long long)e->job_start_wait_ms * 100000ull;
    C.stuck = e->d_stuck;
    C.stuck_cap = STUCK_CAP;
    C.stuck_count = e->d_small + (6) * SMALL_STRIDE;
    C.lone = e->lone ? e->d_lone : nullptr;
    C.lone_cap = e->lone_cap;
    C.lone_count = e->d_small + (7) * SMALL_STRIDE;
    C.lone_all = e->lone == 2;
    C.karg_test = e->karg_test;
    C.split_thr = e->split_thr;
    C.split_spin = e->split_spin;
    C.split_gthr = e->split_gthr;
    C.split_mode = e->split;
    C.split_batch = e->split_batch;
    {
        /* live-bias warm-up (GRM_OPT_WARMUP): the first photons after a reset start as the
         * counters' history doubles, as the serial reference's bias_func sees them */
        const uint64_t n_call = pos1 - pos0;
        const uint64_t lanes = (uint64_t)grid * BLOCK; /* this call's launch */
        const bool small = n_call < WARMUP_AUTO_RATIO * lanes;
        const uint64_t limit = e->warmup == -2 ? (small ? lanes : WARMUP_PHOTONS)
                               : e->warmup < 0 ? lanes
                                               : (uint64_t)e->warmup;
        /* a multi-rank job ramps the job's history to n_peers x one GPU's warm-up (see the kernel) */
        const uint64_t lim = C.n_peers > 1 ? limit * (uint64_t)C.n_peers : limit;
        C.admit_n = (!e->bias_mode && e->history < lim && pos0 == 0) ? std::min<uint64_t>(pos1, lim - e->history) : 0;
        C.admit_h0 = e->history;
        C.admit_lim = lim;
        /* slack: 1/16 for the small-call ramp and for a multi-rank job (its ranks' batches interleave
         * in 1/N shares; emulated 8-rank jobs, 48 each against the oracle at photon_n = 1e5: +4.1 to
         * +5.5 % recorded at 1/2 over five sessions, +2.3 / +2.4 / +3.1 % at 1/16 with warm-ups of 4 k /
         * 16 k / 64 k photons per rank, profiles/r04r_emu_sweep.log, r04y_emu.log) */
        C.admit_slack = e->warmup_slack >= 0 ? e->warmup_slack
                                              : ((e->warmup == -2 && small) || C.n_peers > 1 ? 4 : WARMUP_SLACK_LARGE);
        /* With the job's counters (n_peers ranks), every rank ramps at once: its batches are 1/n_peers
         * of a single GPU's, so that the JOB admits 64, 64, 128, ... photons against the job-wide
         * history as one GPU does (each rank at full batches would start n_peers x 64 photons on the
         * empty history, and so on at every doubling) */
        C.admit_b0 = C.n_peers > 1 ? std::max<unsigned long long>(1ull, e->warmup_b0 / (unsigned long long)C.n_peers)
                                   : e->warmup_b0;
        C.admit_spread = e->warmup_spread >= 0 ? (unsigned long long)e->warmup_spread
                                               : (e->warmup == -2 && small ? 0ull : WARMUP_SPREAD);
    }
    if (e->bias_mode && e->frozen_set) {
        C.f_scatt = e->fz_scatt;
        C.f_rec = e->fz_rec;
        C.f_maxtau = e->fz_maxtau;
    } else if (e->bias_mode) {
        DevCounters h;
        if (read_counters(e, h)) return -1;
        C.f_scatt = (double)h.n_scatt;
        C.f_rec = (double)h.n_recorded;
        double mt;
        std::memcpy(&mt, &h.max_tau_bits, sizeof(mt));
        C.f_maxtau = mt;
    }
    unsigned long long steps_before = 0;
    {
        DevCounters h;
        if (read_counters(e, h)) return -1;
        steps_before = h.n_steps;
    }
    double ms_total = 0.0;
    unsigned long long steps_pass = steps_before;
    int src = -1, dst = 0;
    unsigned long long n_pool = pos1 - pos0;
    for (int pass = 0; n_pool > 0; ++pass) {
        /* the words this launch starts from: [0] pool head (the first claim position), [1 + dst] its
         * overflow count (and that of the pool it drains), [4] in flight and [5] the end of the first
         * warm-up batch, [7] hand-overs; the abort flag cleared */
        CtlOp op{};
        op.clear_abort = 1;
        op.set = (1u << 0) | (1u << 1) | (1u << 2) | (1u << 7);
        op.val[0] = pass == 0 ? pos0 : 0;
        if (pass == 0 && C.admit_n) {
            const unsigned long long h = C.admit_h0;
            op.set |= (1u << 4) | (1u << 5);
            op.val[4] = 0;
            const unsigned long long n_r = C.n_peers > 1 ? (unsigned long long)C.n_peers : 1ull;
            op.val[5] = std::min<unsigned long long>(C.admit_n, std::max<unsigned long long>(
                                                                    C.admit_b0, std::min(h, C.admit_lim - h) / n_r));
            /* the job's gate counts this rank's earlier calls as admitted history */
            op.set_warm = C.n_peers > 1;
            op.warm_val = h * WARM_HIST;
        }
        /* the main launch runs the early worker beside it: [8] early tail, [9] head, [10] done,
         * [11] workgroups exited, [12] worker running / closed, [13] bulk started, [14] slots
         * finished, [15] the worker's children in its queue */
        const bool early = pass == 0 && C.pool_kind == 0 && e->early_steps > 0 && !C.lone_all && grid > 1;
        if (early) op.set |= 0xff00u;
        if (ctl(e, op, false)) return -1;
        if (early) {
            C.early_q = e->d_early;
            C.early_ready = e->d_early_ready;
            C.early_cap = grm_engine::EARLY_CAP;
            C.early_tag = ++e->launch_seq;
            C.early_tail = e->d_small + (8) * SMALL_STRIDE;
            C.early_head = e->d_small + (9) * SMALL_STRIDE;
            C.early_done = e->d_small + (10) * SMALL_STRIDE;
            C.wg_exit = e->d_small + (11) * SMALL_STRIDE;
            C.early_live = e->d_small + (12) * SMALL_STRIDE;
            C.bulk_live = e->d_small + (13) * SMALL_STRIDE;
            C.early_steps = grm_engine::early_steps_for(e->early_steps, n);
            C.early_kids_on = e->early_children;
            C.early_fin = e->d_small + (14) * SMALL_STRIDE;
            C.early_kids = e->d_small + (15) * SMALL_STRIDE;
        } else {
            C.early_q = nullptr;
            C.early_kids_on = 0;
        }
        C.ovf = e->d_ovf[dst];
        C.ovf_count = e->d_small + (1 + dst) * SMALL_STRIDE;
        /* the per-wave record is kept of the first launch (the bulk of a call) */
        C.waves = pass == 0 ? e->d_waves : nullptr;
        C.phases = C.waves ? e->d_waves + (size_t)(e->lanes / 64) * 4 : nullptr;
        if (C.phases) HIPCHK(e, hipMemsetAsync(C.phases, 0, PHASE_LOG * sizeof(unsigned long long), e->stream));
        if (C.waves) e->waves_rows = (size_t)grid * (BLOCK / 64);
        if (pass > 0) {
            C.pool = e->d_ovf[src];
            C.pool_kind = 1;
            C.n_pool = n_pool;
            C.pos_end = n_pool;
            C.pool_m = n_pool;
            C.pool_sh = 0;
            C.admit_n = 0;
            /* a small relaunch (the children of the hand-overs, a few hundred) is a tail from its
             * start: every photon goes to a two-wave pair at the top of its first step (~1.5 us per
             * step against ~4 us in a sparse lane loop) */
            C.lone_all = e->lone == 2 || (e->lone == 1 && n_pool <= e->lone_cap / 2);
        }
        if (early && e->early_serial) { /* test: serialised ahead of the main launch */
            HIPCHK(e, grm_lone_launch(1, 1, e->stream, &e->P, sizeof(Params), &C, sizeof(Ctl)));
            HIPCHK(e, hipEventRecord(e->ev_w, e->stream));
        } else if (early) { /* after the control words are set; one workgroup, all of its pairs */
            HIPCHK(e, hipEventRecord(e->ev_pre, e->stream));
            HIPCHK(e, hipStreamWaitEvent(e->stream2, e->ev_pre, 0));
            HIPCHK(e, grm_lone_launch(1, 1, e->stream2, &e->P, sizeof(Params), &C, sizeof(Ctl)));
            HIPCHK(e, hipEventRecord(e->ev_w, e->stream2));
        }
        HIPCHK(e, hipEventRecord(e->ev0, e->stream));
        /* one workgroup per CU.  The early worker takes one CU too: workgroups are dealt to the XCDs
         * round-robin, so with the worker's XCD full one bulk workgroup waits and starts (to find
         * the pool empty) as the bulk drains -- 255 run either way, and a full grid needs no guess
         * which XCD the worker lands on */
#ifdef GRM_WITH_SPLIT
        if (e->split) {
            HIPCHK(e, grm_split_launch((unsigned)grid, e->stream, &e->P, sizeof(Params), &C, sizeof(Ctl)));
        } else
#endif
        {
            hipLaunchKernelGGL(track_kernel, dim3(grid), dim3(BLOCK), 0, e->stream, e->P, C);
            HIPCHK(e, hipGetLastError());
        }
        HIPCHK(e, hipEventRecord(e->ev1, e->stream));
        /* the photons the launch handed over (a count on the device), one wave pair each; their
         * children join this launch's overflow pool */
        if (C.lone) {
            /* the lone pairs track the children of their photons themselves (GRM_OPT_EARLY_CHILDREN) */
            C.lk_on = e->early_children;
            C.lk_q = e->d_lk;
            C.lk_ready = e->d_lk_ready;
            C.lk_cap = grm_engine::LK_CAP;
            C.lk_tag = ++e->launch_seq;
            C.lk_tail = e->d_lk_words + 0 * SMALL_STRIDE;
            C.lk_taken = e->d_lk_words + 1 * SMALL_STRIDE;
            C.lk_active = e->d_lk_words + 2 * SMALL_STRIDE;
            C.lk_standby = e->d_lk_words + 3 * SMALL_STRIDE;
            C.lk_orig = e->d_lk_words + 4 * SMALL_STRIDE;
            if (C.lk_on)
                HIPCHK(e, hipMemsetAsync(e->d_lk_words, 0, 5 * SMALL_STRIDE * sizeof(unsigned long long), e->stream));
            HIPCHK(e, hipEventRecord(e->ev2, e->stream));
            HIPCHK(e, grm_lone_launch(0, (unsigned)e->lone_cap, e->stream, &e->P, sizeof(Params), &C, sizeof(Ctl)));
            HIPCHK(e, hipEventRecord(e->ev3, e->stream));
        }
        if (early) HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev_w, 0)); /* its photons' counters too */
        DevCounters hp;
        if (read_counters(e, hp)) return -1; /* synchronises */
        float ms = 0.f;
        HIPCHK(e, hipEventElapsedTime(&ms, e->ev0, e->ev1));
        ms_total += ms;
        const unsigned long long n_lone = std::min<unsigned long long>(e->pin->small[7], e->lone_cap);
        if (early) { /* the published slots: hand-overs and the worker's own children */
            const unsigned long long kids = e->pin->small[15];
            e->stats.n_early += std::min<unsigned long long>(e->pin->small[8], grm_engine::EARLY_CAP) - kids;
            e->stats.n_early_children += kids;
        }
        if (early && !e->early_serial) { /* ev_pre (engine stream, before the bulk) .. ev_w (after the worker) */
            float ms_e = 0.f;
            HIPCHK(e, hipEventElapsedTime(&ms_e, e->ev_pre, e->ev_w));
            if (ms_e > e->stats.early_ms) e->stats.early_ms = ms_e;
        }
        if (C.lone) {
            float ms_l = 0.f;
            HIPCHK(e, hipEventElapsedTime(&ms_l, e->ev2, e->ev3));
            ms_total += ms_l;
            e->stats.lone_ms += ms_l;
            e->stats.n_lone += n_lone;
            if (C.lk_on) {
                unsigned long long lk_tail = 0;
                HIPCHK(e, hipMemcpy(&lk_tail, e->d_lk_words, sizeof(lk_tail), hipMemcpyDeviceToHost));
                e->stats.n_lone_children += std::min<unsigned long long>(lk_tail, grm_engine::LK_CAP);
            }
            if (n_lone) e->stats.n_launches++;
        }
        const unsigned long long cnt = e->pin->small[1 + dst];
        if (ms > e->stats.max_launch_ms) { /* the dominant launch of this transport call */
            e->stats.max_launch_ms = ms;
            e->stats.max_launch_steps = hp.n_steps - steps_pass;
        }
        steps_pass = hp.n_steps;
        e->stats.n_launches++;
        e->stats.n_nan_photons = hp.n_nan;
        if (hp.karg_bad) {
            e->err = "track_kernel: the kernel-argument segment does not hold the launch's arguments in the "
                     "layout of struct KArgs (" + std::to_string(hp.karg_bad) +
                     " waves); no photon was tracked -- results of this call are invalid";
            return -1;
        }
        if (hp.abort) {
            e->stats.n_abandoned = hp.n_abandoned;
            e->err = "watchdog: a transport launch ran longer than " + std::to_string(e->watchdog_ms) + " ms; " +
                     std::to_string(hp.n_abandoned) +
                     " photons abandoned (their state: grm_engine_debug_stuck); results of this call are incomplete";
            return -1;
        }
        n_pool = std::min(cnt, e->ovf_cap);
        src = dst;
        dst ^= 1;
        if (pass > 64) {
            e->err = "overflow relaunch did not converge";
            return -1;
        }
    }
    DevCounters h;
    if (read_counters(e, h)) return -1;
    if (h.n_dropped) {
        /* a scattered child that fit neither the wave stack nor the overflow pool is lost: the
         * spectrum of this call would be incomplete, so the call fails */
        e->err = std::to_string(h.n_dropped) + " scattered children dropped (overflow pool of " +
                 std::to_string(e->ovf_cap) + " full); results of this call are incomplete";
        return -1;
    }
    e->stats.kernel_ms += ms_total;
    e->stats.last_kernel_ms += ms_total;
    e->stats.last_steps += h.n_steps - steps_before;
    e->history += pos1 - pos0;
    return 0;
}

/* One transport call = one persistent launch (+ overflow relaunches); the live-bias warm-up is
 * admission control inside the launch (Ctl.admit_n).
 *
 * Claim order.  The batch is in zone-walk order (emission, harm_model.cpp:673-704), and the
 * adaptive bias (bias_func, :1391-1404) is driven by the counters of RECORDED photons.  The inner
 * zones' photons fall into the hole and never record, so a zone-ordered claim sequence would start
 * ~lanes photons of the zones where escape begins all at once on the bias of an empty history --
 * where the serial reference adapts after the first few records -- and their scattering cascades
 * would inflate the recorded / scattered counts ~2x (measured: 5.1 M vs the reference's 2.3 M at
 * 192^2, photon_n = 1e5).  Claims therefore interleave 2^CLAIM_SH evenly spaced runs of the batch:
 * claim position q takes photon (q mod 2^CLAIM_SH) * m + q / 2^CLAIM_SH, so every admission batch
 * and every stretch of the bulk samples the whole zone range, records start at once and the
 * counters evolve as in the serial run (photon ids, and so the Philox streams, stay the batch
 * index: results depend on the order only through the bias). */
constexpr int CLAIM_SH = 12;

int run_transport(grm_engine *e, const grm_init_photon *d_batch, size_t n) {
    if (alloc_lanes(e)) return -1;
    e->stats.last_kernel_ms = 0.0;
    e->stats.last_steps = 0;
    e->stats.max_launch_ms = 0.0;
    e->stats.max_launch_steps = 0;
    if (n == 0) return 0;
    const int sh = n >= (2ull << CLAIM_SH) ? CLAIM_SH : 0;
    const uint64_t m = (n + (1ull << sh) - 1) >> sh, n_pos = m << sh;
    /* one launch: the live-bias warm-up (the first positions in admission batches) is admission
     * control inside it, and the claims run free as soon as it is over, while the warm-up's own
     * long-lived photons are still in flight.  With the live bias the launch has at most
     * n / flight_ratio lanes (GRM_OPT_FLIGHT_RATIO): the counters bias_func reads trail the claims
     * by the photons in flight, and a call of 1.45 M photons (photon_n = 1e5) on 131 k lanes moved
     * recorded / scattered / steps +4.4 / +5.9 / +4.2 % against the serial reference, +1.0 / +1.1 /
     * +0.9 % on 16 k lanes (96 seeds each, profiles/r04h_grid_sweep96.jsonl) -- for 1.6x the pass
     * time at that size; a bench pass (14.5 M photons) keeps the full grid.  The lag matters against
     * the history the counters already hold, so the cap counts the photons tracked since the reset
     * too: a pass fed in chunks (INTEGRATION.md path (a), 4 M photons per call) runs its later
     * chunks on the full grid */
    int grid = e->grid;
    if (!e->bias_mode && e->flight_ratio > 0) {
        /* A multi-rank job's small calls run on half those lanes: with the job's counters the ranks'
         * concurrent launches lag the job's history more than one GPU's launch with as many lanes
         * (emulated 8-rank jobs at photon_n = 1e5, 96 each, the same seeds: recorded +2.97 % at ratio
         * 96, +1.42 % at 192; one GPU +1.00 / +0.92 %, the serial reference on the same streams +0.85 %;
         * DESIGN.md §7).  Large calls (>= WARMUP_AUTO_RATIO x the full grid's lanes: the bench's 1e6
         * per rank, a configs[3] shard) keep the ratio, so the cap does not bind there. */
        const bool job = e->ctr_slot >= 0 && e->d_peers && e->n_peers > 1;
        const uint64_t full = (uint64_t)e->grid * BLOCK;
        const uint64_t ratio = (uint64_t)e->flight_ratio * ((job && e->history + n < WARMUP_AUTO_RATIO * full) ? 2 : 1);
        const uint64_t cap_wg = (e->history + n) / (ratio * BLOCK);
        grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)grid, cap_wg));
    }
    e->stats.last_grid = grid;
    if (run_passes(e, d_batch, n, sh, m, 0, n_pos, grid)) return -1;
    e->id_base += n;
    return 0;
}

/* records the trace has counted (more than trace_cap: the excess was lost) */
int trace_count(grm_engine *e, unsigned long long &cnt) {
    HIPCHK(e, hipMemcpyAsync(&cnt, e->d_small + (3) * SMALL_STRIDE, sizeof(cnt), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return 0;
}

/* the cell-sum accumulator and its skipped-record word behind it */
constexpr size_t CELLSUMS_BYTES = GRM_CELLSUMS_DOUBLES * sizeof(double) + sizeof(unsigned long long);
/* a re-binning table of `doubles` doubles and its out-of-grid word */
constexpr size_t rebin_bytes(size_t doubles) { return doubles * sizeof(double) + sizeof(unsigned long long); }

int reset_counters(grm_engine *e) {
    CtlOp op{};
    op.reset = 1;
    op.set = 0xffffu; /* every small word 0 */
    return ctl(e, op, true);
}

} /* namespace */

/* probe entry point lives in grm_probe.hip */
extern "C" int grm_probe_impl(const Params &P, hipStream_t s, int which, const double *in, int in_stride, double *out,
                              int out_stride, size_t n, std::string &err);

extern "C" {

int grm_engine_create(const grm_header *h, const double *const fields[8], const grm_units *u, const double *hotcross,
                      const double *k2, const double scalars[4], int device, grm_engine **out) {
    if (!h || !fields || !u || !hotcross || !k2 || !scalars || !out) return -1;
    *out = nullptr;
    if (h->n[0] < 2 || h->n[1] < 2) return -2;
    grm_engine *e = new grm_engine();
    e->device = device;
    auto fail = [&](void) {
        *out = e; /* hand back for last_error; caller destroys */
        return -1;
    };
    if (!hip_ok(e, hipSetDevice(device), "hipSetDevice")) return fail();
    if (!hip_ok(e, hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking), "stream")) return fail();
    if (!hip_ok(e, hipEventCreate(&e->ev0), "event") || !hip_ok(e, hipEventCreate(&e->ev1), "event") ||
        !hip_ok(e, hipEventCreate(&e->ev2), "event") || !hip_ok(e, hipEventCreate(&e->ev3), "event") ||
        !hip_ok(e, hipEventCreate(&e->ev_pre), "event") || /* timed: stats.early_ms */
        !hip_ok(e, hipEventCreate(&e->ev_w), "event") ||
        !hip_ok(e, hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking), "stream") ||
        !hip_ok(e, hipMalloc(&e->d_early, grm_engine::EARLY_CAP * sizeof(LoneRec)), "early queue") ||
        !hip_ok(e, hipMalloc(&e->d_early_ready, grm_engine::EARLY_CAP * sizeof(unsigned long long)), "early queue") ||
        !hip_ok(e, hipMemset(e->d_early_ready, 0, grm_engine::EARLY_CAP * sizeof(unsigned long long)), "early queue") ||
        !hip_ok(e, hipMalloc(&e->d_lk, grm_engine::LK_CAP * sizeof(LoneRec)), "lone children queue") ||
        !hip_ok(e, hipMalloc(&e->d_lk_ready, grm_engine::LK_CAP * sizeof(unsigned long long)), "lone children queue") ||
        !hip_ok(e, hipMemset(e->d_lk_ready, 0, grm_engine::LK_CAP * sizeof(unsigned long long)), "lone children queue") ||
        !hip_ok(e, hipMalloc(&e->d_lk_words, 5 * SMALL_STRIDE * sizeof(unsigned long long)), "lone children queue"))
        return fail();
    if (!hip_ok(e, hipHostMalloc(reinterpret_cast<void **>(&e->pin), sizeof(grm_engine::Pinned),
                                 hipHostMallocMapped | hipHostMallocCoherent),
                "host-mapped control block"))
        return fail();
    std::memset(e->pin, 0, sizeof(grm_engine::Pinned));
    {
        /* the kernels write the block through the host pointer: it must be the device address too */
        void *dp = nullptr;
        if (!hip_ok(e, hipHostGetDevicePointer(&dp, e->pin, 0), "hipHostGetDevicePointer")) return fail();
        if (dp != (void *)e->pin) {
            e->err = "host-mapped control block: device address differs from the host address";
            return fail();
        }
    }
    const size_t nz = (size_t)h->n[0] * h->n[1];
    std::vector<double> zones(nz * 8);
    for (size_t z = 0; z < nz; ++z)
        for (int f = 0; f < 8; ++f) zones[z * 8 + f] = fields[f][z];
    const size_t nhot = (size_t)(GRM_HC_N_W + 1) * (GRM_HC_N_T + 1);
    if (!hip_ok(e, hipMalloc(&e->d_zones, nz * 8 * sizeof(double)), "zones") ||
        !hip_ok(e, hipMalloc(&e->d_hot, nhot * sizeof(double)), "hotcross") ||
        !hip_ok(e, hipMalloc(&e->d_k2, (GRM_N_E_SAMP + 1) * sizeof(double)), "k2") ||
        !hip_ok(e, hipMalloc(&e->d_ctr_own, sizeof(DevCounters)), "counters") ||
        !hip_ok(e, hipMalloc(&e->d_spec, sizeof(grm_spectrum_cell) * N_TH_BINS * N_E_BINS), "spectrum") ||
        !hip_ok(e, hipMalloc(&e->d_small, 16 * SMALL_STRIDE * sizeof(unsigned long long)), "small") ||
        !hip_ok(e, hipMalloc(&e->d_stuck, STUCK_CAP * STUCK_WORDS * sizeof(double)), "stuck") ||
        !hip_ok(e, hipMemset(e->d_small, 0, 16 * SMALL_STRIDE * sizeof(unsigned long long)), "small"))
        return fail();
    if (!hip_ok(e, hipMemcpy(e->d_zones, zones.data(), nz * 8 * sizeof(double), hipMemcpyHostToDevice), "H2D") ||
        !hip_ok(e, hipMemcpy(e->d_hot, hotcross, nhot * sizeof(double), hipMemcpyHostToDevice), "H2D") ||
        !hip_ok(e, hipMemcpy(e->d_k2, k2, (GRM_N_E_SAMP + 1) * sizeof(double), hipMemcpyHostToDevice), "H2D"))
        return fail();
    Params &P = e->P;
    P.n1 = h->n[0];
    P.n2 = h->n[1];
    P.xs1 = h->x_start[1];
    P.xs2 = h->x_start[2];
    P.xe1 = h->x_stop[1];
    P.xe2 = h->x_stop[2];
    P.dx1 = h->dx[1];
    P.dx2 = h->dx[2];
    P.a = h->a;
    P.h_slope = h->h_slope;
    P.r0 = h->r_0;
    P.n_e_unit = u->n_e_unit;
    P.theta_e_unit = u->theta_e_unit;
    P.b_unit = u->b_unit;
    P.bias_norm = scalars[0];
    P.x1_min = scalars[1];
    e->max_tau_init = scalars[2];
    P.d_tau_k = scalars[3];
    /* derived table constants, host libm (consts.hpp:33-157) */
    P.x1_max = std::log(100.0);
    P.hc_l_min_w = std::log10(1.0e-12);
    P.hc_l_min_t = std::log10(1.0e-4);
    P.hc_d_l_w = std::log10(1.0e6 / 1.0e-12) / GRM_HC_N_W;
    P.hc_d_l_t = std::log10(1.0e4 / 1.0e-4) / GRM_HC_N_T;
    P.jnu_l_min_t = std::log(0.3);
    P.jnu_d_l_t = std::log(1.0e2 / 0.3) / GRM_N_E_SAMP;
    P.spec_l_e_0 = std::log(1.0e-12);
    P.th_dx2 = (h->x_stop[2] - h->x_start[2]) / (2.0 * N_TH_BINS);
    P.i_dx1 = 1.0 / P.dx1;
    P.i_dx2 = 1.0 / P.dx2;
    P.hc_i_d_l_w = 1.0 / P.hc_d_l_w;
    P.hc_i_d_l_t = 1.0 / P.hc_d_l_t;
    P.jnu_i_d_l_t = 1.0 / P.jnu_d_l_t;
    params_metric(P);
    P.zones = e->d_zones;
    P.hotcross = e->d_hot;
    P.k2 = e->d_k2;
    e->d_ctr = e->d_ctr_own;
    if (!hip_ok(e, hipMalloc(&e->d_timing, 48 * sizeof(unsigned long long)), "timing") ||
        !hip_ok(e, hipMemset(e->d_timing, 0, 48 * sizeof(unsigned long long)), "timing"))
        return fail();
    if (reset_counters(e)) return fail();
    *out = e;
    return 0;
}

void grm_engine_destroy(grm_engine *e) {
    if (!e) return;
    hipSetDevice(e->device);
    if (e->stream) hipStreamSynchronize(e->stream);
    if (e->stream2) hipStreamSynchronize(e->stream2); /* early_kernel uses d_small, d_ctr, d_early ... */
    hipFree(e->d_zones);
    hipFree(e->d_hot);
    hipFree(e->d_k2);
    hipFree(e->d_ctr_own);
    for (void *p : e->ipc_open) hipIpcCloseMemHandle(p);
    hipFree(e->d_ctr_slots);
    hipFree(e->d_peers);
    hipFree(e->d_spec);
    hipFree(e->d_stack);
    hipFree(e->d_cold);
    hipFree(e->d_ovf[0]);
    hipFree(e->d_ovf[1]);
    hipFree(e->d_small);
    hipFree(e->d_stuck);
    hipFree(e->d_spec_blocks);
    hipFree(e->d_lone);
    if (e->pin) hipHostFree(e->pin);
    hipFree(e->d_batch);
    hipFree(e->d_trace);
    hipFree(e->d_cellsums);
    hipFree(e->d_rebin);
    hipFree(e->d_rebin_keys);
    hipFree(e->d_upload);
    hipFree(e->d_timing);
    hipFree(e->d_waves);
    hipFree(e->d_ezones);
    hipFree(e->d_eweight);
    hipFree(e->d_ef);
    hipFree(e->d_eoff);
    hipFree(e->d_emit);
    if (e->comm) ncclCommDestroy(e->comm);
    hipFree(e->d_stash_spec);
    hipFree(e->d_stash_sum);
    hipFree(e->d_stash_max);
    if (e->ev0) hipEventDestroy(e->ev0);
    if (e->ev1) hipEventDestroy(e->ev1);
    if (e->ev2) hipEventDestroy(e->ev2);
    if (e->ev3) hipEventDestroy(e->ev3);
    if (e->ev_pre) hipEventDestroy(e->ev_pre);
    if (e->ev_w) hipEventDestroy(e->ev_w);
    if (e->stream2) hipStreamDestroy(e->stream2);
    hipFree(e->d_early);
    hipFree(e->d_early_ready);
    hipFree(e->d_lk);
    hipFree(e->d_lk_ready);
    hipFree(e->d_lk_words);
    if (e->stream) hipStreamDestroy(e->stream);
    delete e;
}

const char *grm_engine_last_error(const grm_engine *e) { return e ? e->err.c_str() : "null engine"; }

int grm_engine_set_option(grm_engine *e, int opt, int64_t v) {
    if (!e) return -1;
    hipSetDevice(e->device);
    switch (opt) {
    case GRM_OPT_SEED: e->seed = (uint64_t)v; return 0;
    case GRM_OPT_BIAS_MODE: e->bias_mode = v ? 1 : 0; return 0;
    case GRM_OPT_TRACE_CAP:
        /* the records counted so far are those of the old buffer (or of none): never binned */
        if (trace_count(e, e->trace_consumed)) return -1;
        e->rebin_consumed = e->trace_consumed;
        if (e->d_trace) hipFree(e->d_trace);
        e->d_trace = nullptr;
        e->trace_cap = 0;
        if (v > 0) {
            HIPCHK(e, hipMalloc(&e->d_trace, (size_t)v * sizeof(grm_trace)));
            e->trace_cap = (unsigned long long)v;
        }
        return 0;
    case GRM_OPT_GRID_BLOCKS: e->grid_override = (int)v; return 0;
    case GRM_OPT_FLIGHT_RATIO: e->flight_ratio = v < 0 ? 0 : v; return 0;
    case GRM_OPT_JOB_START_WAIT_MS: e->job_start_wait_ms = v < 0 ? 0 : (v > 10000 ? 10000 : v); return 0;
    case GRM_OPT_ID_BASE: e->id_base = (uint64_t)v; return 0;
    case GRM_OPT_FROZEN_SCATT: e->fz_scatt = (double)v; e->frozen_set = true; return 0;
    case GRM_OPT_FROZEN_REC: e->fz_rec = (double)v; e->frozen_set = true; return 0;
    case GRM_OPT_FROZEN_MAXTAU: std::memcpy(&e->fz_maxtau, &v, sizeof(double)); e->frozen_set = true; return 0;
    case GRM_OPT_WARMUP: e->warmup = v; return 0;
    case GRM_OPT_REFILL_MIN: e->refill_min = v < 1 ? 1 : (v > 64 ? 64 : (int)v); return 0;
    case GRM_OPT_CHILD_MIN: e->child_min = v < 1 ? 1 : (v > 64 ? 64 : (int)v); return 0;
    case GRM_OPT_WARMUP_SLACK: e->warmup_slack = v < 0 ? -1 : (v > 30 ? 30 : (int)v); return 0;
    case GRM_OPT_LONE: e->lone = v < 0 ? 0 : (v > 2 ? 2 : (int)v); return 0;
    case GRM_OPT_WARMUP_BATCH: e->warmup_b0 = v < 1 ? 1 : (unsigned long long)v; return 0;
    case GRM_OPT_WARMUP_SPREAD: e->warmup_spread = v < 0 ? -1 : v; return 0;
    case GRM_OPT_EARLY_STEPS: e->early_steps = v < 0 ? 0 : (v > (1 << 30) ? (1 << 30) : (int)v); return 0;
    case GRM_OPT_EARLY_SERIAL: e->early_serial = v != 0; return 0;
    case GRM_OPT_EARLY_CHILDREN: e->early_children = v != 0; return 0;
    case GRM_OPT_KARG_TEST: e->karg_test = (int)v; return 0;
    case GRM_OPT_WATCHDOG_MS: e->watchdog_ms = v < 0 ? 0 : v; return 0;
#ifdef GRM_WITH_SPLIT
    case GRM_OPT_SPLIT: e->split = v < 0 ? 0 : (v > 2 ? 2 : (int)v); return 0;
    case GRM_OPT_SPLIT_THR: e->split_thr = v < 1 ? 1 : (v > 64 ? 64 : (int)v); return 0;
    case GRM_OPT_SPLIT_SPIN: e->split_spin = v < 0 ? 0 : (v > 1 << 20 ? 1 << 20 : (int)v); return 0;
    case GRM_OPT_SPLIT_GTHR: e->split_gthr = v < 0 ? 0 : (v > 64 ? 64 : (int)v); return 0;
    case GRM_OPT_SPLIT_BATCH: e->split_batch = v < 1 ? 1 : (v > 3 ? 3 : (int)v); return 0;
#else
    case GRM_OPT_SPLIT:
        if (v == 0) return 0; /* track_kernel: the only bulk kernel of this build */
        e->err = "split_kernel is not in this library (a variant build: VFLAGS=-DGRM_WITH_SPLIT tools/build_variant.sh)";
        return -1;
    case GRM_OPT_SPLIT_THR: case GRM_OPT_SPLIT_SPIN: case GRM_OPT_SPLIT_GTHR: case GRM_OPT_SPLIT_BATCH:
        e->err = "split_kernel options need a variant build with -DGRM_WITH_SPLIT";
        return -1;
#endif
    case 18: case 20: case 21: e->err = "retired option " + std::to_string(opt); return -1;
    default: e->err = "unknown option"; return -1;
    }
}

int grm_engine_track(grm_engine *e, const grm_init_photon *batch, size_t n) {
    if (!e || (!batch && n)) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    if (n > e->batch_cap) { /* 1/8 headroom, as the emission buffer (grm_emit.hip) */
        if (e->d_batch) hipFree(e->d_batch);
        e->d_batch = nullptr;
        HIPCHK(e, hipMalloc(&e->d_batch, (n + n / 8) * sizeof(grm_init_photon)));
        e->batch_cap = n + n / 8;
    }
    HIPCHK(e, hipMemcpyAsync(e->d_batch, batch, n * sizeof(grm_init_photon), hipMemcpyHostToDevice, e->stream));
    return run_transport(e, e->d_batch, n);
}

int grm_engine_track_device(grm_engine *e, const grm_init_photon *dev_batch, size_t n) {
    if (!e || (!dev_batch && n)) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    return run_transport(e, dev_batch, n);
}

int grm_engine_finish(grm_engine *e, grm_spectrum_cell *spec, uint64_t *n_rec, uint64_t *n_scatt, double *max_tau) {
    if (!e) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    DevCounters h;
    if (spec)
        HIPCHK(e, hipMemcpyAsync(spec, e->d_spec, sizeof(grm_spectrum_cell) * N_TH_BINS * N_E_BINS,
                                 hipMemcpyDeviceToHost, e->stream));
    if (read_counters(e, h)) return -1;
    if (n_rec) *n_rec = h.n_recorded;
    if (n_scatt) *n_scatt = h.n_scatt;
    if (max_tau) std::memcpy(max_tau, &h.max_tau_bits, sizeof(double));
    e->stats.n_steps = h.n_steps;
    e->stats.n_tracked = h.n_tracked;
    e->stats.n_children = h.n_children;
    e->stats.n_overflow = h.n_overflow;
    e->stats.n_dropped = h.n_dropped;
    e->stats.n_primaries = h.n_primaries;
    e->stats.max_photon_steps = h.max_nstep;
    e->stats.n_long_photons = h.n_long;
    return 0;
}

int grm_engine_reset(grm_engine *e) {
    if (!e) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    const double ms = e->stats.kernel_ms;
    const uint64_t launches = e->stats.n_launches;
    std::memset(&e->stats, 0, sizeof(e->stats));
    e->stats.kernel_ms = ms;
    e->stats.n_launches = launches;
    e->history = 0;
    e->trace_consumed = 0; /* reset_counters zeroes the trace count */
    if (e->d_cellsums) HIPCHK(e, hipMemsetAsync(e->d_cellsums, 0, CELLSUMS_BYTES, e->stream));
    e->rebin_consumed = 0;
    if (e->d_rebin) HIPCHK(e, hipMemsetAsync(e->d_rebin, 0, rebin_bytes(e->rebin_doubles), e->stream));
    return reset_counters(e);
}

int grm_engine_stats(const grm_engine *e, grm_stats *out) {
    if (!e || !out) return -1;
    grm_engine *m = const_cast<grm_engine *>(e);
    if (grm_engine_finish(m, nullptr, nullptr, nullptr, nullptr)) return -1;
    *out = e->stats;
    return 0;
}

void *grm_engine_spectrum_device_ptr(grm_engine *e) { return e ? (void *)e->d_spec : nullptr; }

int64_t grm_engine_trace(grm_engine *e, grm_trace *out, size_t cap) {
    if (!e || !e->d_trace) return -1;
    hipSetDevice(e->device);
    unsigned long long cnt = 0;
    if (hipMemcpy(&cnt, e->d_small + (3) * SMALL_STRIDE, sizeof(cnt), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    const size_t avail = std::min<unsigned long long>(cnt, e->trace_cap);
    const size_t k = std::min(avail, cap);
    if (k && out && hipMemcpy(out, e->d_trace, k * sizeof(grm_trace), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)cnt;
}

int grm_engine_cell_sums_accumulate(grm_engine *e, uint64_t *n_binned, double *ms) {
    if (!e) return -1;
    if (n_binned) *n_binned = 0;
    if (ms) *ms = 0.0;
    HIPCHK(e, hipSetDevice(e->device));
    if (!e->trace_cap) {
        e->err = "cell sums: the trace is off (GRM_OPT_TRACE_CAP)";
        return -1;
    }
    unsigned long long cnt = 0;
    if (trace_count(e, cnt)) return -1;
    if (cnt > e->trace_cap) {
        e->err = "cell sums: the trace counted " + std::to_string(cnt) + " records but holds " +
                 std::to_string(e->trace_cap) + " (GRM_OPT_TRACE_CAP): records were lost, nothing binned";
        return -1;
    }
    if (!e->d_cellsums) {
        HIPCHK(e, hipMalloc(&e->d_cellsums, CELLSUMS_BYTES));
        HIPCHK(e, hipMemsetAsync(e->d_cellsums, 0, CELLSUMS_BYTES, e->stream));
    }
    const unsigned long long c0 = std::min(e->trace_consumed, cnt);
    double t = 0.0;
    if (grm_cellsums_launch(e->d_trace + c0, (size_t)(cnt - c0), e->d_cellsums,
                            reinterpret_cast<unsigned long long *>(e->d_cellsums + GRM_CELLSUMS_DOUBLES), e->stream,
                            e->ev0, e->ev1, &t, e->err))
        return -1;
    e->trace_consumed = cnt;
    if (n_binned) *n_binned = cnt - c0;
    if (ms) *ms = t;
    return 0;
}

int grm_engine_cell_sums_read(grm_engine *e, double *out, uint64_t *n_skipped) {
    if (!e || !out) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    unsigned long long sk = 0;
    if (!e->d_cellsums) {
        std::memset(out, 0, GRM_CELLSUMS_DOUBLES * sizeof(double));
    } else {
        HIPCHK(e, hipMemcpyAsync(out, e->d_cellsums, GRM_CELLSUMS_DOUBLES * sizeof(double), hipMemcpyDeviceToHost,
                                 e->stream));
        HIPCHK(e, hipMemcpyAsync(&sk, e->d_cellsums + GRM_CELLSUMS_DOUBLES, sizeof(sk), hipMemcpyDeviceToHost,
                                 e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
    }
    if (n_skipped) *n_skipped = sk;
    return 0;
}

int grm_engine_cell_sums_reset(grm_engine *e) {
    if (!e) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    if (e->d_cellsums) {
        HIPCHK(e, hipMemsetAsync(e->d_cellsums, 0, CELLSUMS_BYTES, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
    }
    return 0;
}

int grm_engine_trace_rewind(grm_engine *e) {
    if (!e) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    unsigned long long cnt = 0;
    if (trace_count(e, cnt)) return -1;
    /* with a re-binning set up, the cell sums are a consumer only once they have been accumulated:
     * a run that re-bins alone need not feed them.  With none, exactly as before. */
    if (e->trace_cap && cnt > e->trace_consumed && (!e->rebin_on || e->d_cellsums)) {
        e->err = "trace rewind: " + std::to_string(cnt - e->trace_consumed) +
                 " records are not consumed yet (grm_engine_cell_sums_accumulate); a rewind would drop them";
        return -1;
    }
    if (e->trace_cap && e->rebin_on && cnt > e->rebin_consumed) {
        e->err = "trace rewind: " + std::to_string(cnt - e->rebin_consumed) +
                 " records are not consumed yet by the rebin (grm_engine_rebin_accumulate); a rewind would drop them";
        return -1;
    }
    CtlOp op{};
    op.set = 1u << 3; /* the trace count */
    op.val[3] = 0;
    if (ctl(e, op, true)) return -1;
    e->trace_consumed = 0;
    e->rebin_consumed = 0;
    return 0;
}

/* --- the trace re-binned on a caller's grid (csrc/grm_rebin.hip) --- */
int grm_engine_rebin_setup(grm_engine *e, const grm_bin_grid *grid) {
    if (!e) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    if (!grid) { /* release */
        if (e->d_rebin) HIPCHK(e, hipFree(e->d_rebin));
        e->d_rebin = nullptr;
        e->rebin_doubles = 0;
        e->rebin_on = false;
        e->rebin_consumed = 0;
        return 0;
    }
    if (const char *bad = grm_bin_grid_check(grid)) {
        e->err = std::string("rebin setup: ") + bad;
        return -1;
    }
    const size_t doubles = grm_bin_grid_doubles(grid);
    if (doubles != e->rebin_doubles) {
        double *d = nullptr;
        HIPCHK(e, hipMalloc(&d, rebin_bytes(doubles))); /* a failure leaves the old table in force */
        if (e->d_rebin) (void)hipFree(e->d_rebin);
        e->d_rebin = d;
        e->rebin_doubles = doubles;
    }
    e->rebin_grid = *grid;
    e->rebin_grid.pad_ = 0;
    e->rebin_on = true;
    e->rebin_consumed = 0;
    HIPCHK(e, hipMemsetAsync(e->d_rebin, 0, rebin_bytes(doubles), e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return 0;
}

int grm_engine_rebin_accumulate(grm_engine *e, uint64_t *n_binned, double *ms) {
    if (!e) return -1;
    if (n_binned) *n_binned = 0;
    if (ms) *ms = 0.0;
    HIPCHK(e, hipSetDevice(e->device));
    if (!e->rebin_on) {
        e->err = "rebin: no grid set up (grm_engine_rebin_setup)";
        return -1;
    }
    if (!e->trace_cap) {
        e->err = "rebin: the trace is off (GRM_OPT_TRACE_CAP)";
        return -1;
    }
    unsigned long long cnt = 0;
    if (trace_count(e, cnt)) return -1;
    if (cnt > e->trace_cap) {
        e->err = "rebin: the trace counted " + std::to_string(cnt) + " records but holds " +
                 std::to_string(e->trace_cap) + " (GRM_OPT_TRACE_CAP): records were lost, nothing binned";
        return -1;
    }
    if (e->rebin_keys_cap < e->trace_cap) {
        if (e->d_rebin_keys) (void)hipFree(e->d_rebin_keys);
        e->d_rebin_keys = nullptr;
        e->rebin_keys_cap = 0;
        HIPCHK(e, hipMalloc(&e->d_rebin_keys, (size_t)e->trace_cap * sizeof(uint32_t)));
        e->rebin_keys_cap = e->trace_cap;
    }
    const unsigned long long c0 = std::min(e->rebin_consumed, cnt);
    double t[2] = {0.0, 0.0};
    if (grm_rebin_launch(grm_rebin_make(e->rebin_grid, e->P.xs2, e->P.xe2), e->d_trace + c0, (size_t)(cnt - c0),
                         e->d_rebin_keys, e->d_rebin,
                         reinterpret_cast<unsigned long long *>(e->d_rebin + e->rebin_doubles), e->stream, e->ev0,
                         e->ev1, e->ev2, t, e->err))
        return -1;
    e->rebin_consumed = cnt;
    e->rebin_ms[0] = t[0];
    e->rebin_ms[1] = t[1];
    if (n_binned) *n_binned = cnt - c0;
    if (ms) *ms = t[0] + t[1];
    return 0;
}

int grm_engine_rebin_read(grm_engine *e, double *out, size_t out_doubles, uint64_t *n_out_of_grid) {
    if (!e) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    if (!e->rebin_on) {
        e->err = "rebin: no grid set up (grm_engine_rebin_setup)";
        return -1;
    }
    if (!out || out_doubles != e->rebin_doubles) {
        e->err = "rebin read: the grid in force has " + std::to_string(e->rebin_doubles) + " doubles, the caller gave " +
                 std::to_string(out ? out_doubles : 0);
        return -1;
    }
    unsigned long long og = 0;
    HIPCHK(e, hipMemcpyAsync(out, e->d_rebin, e->rebin_doubles * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(&og, e->d_rebin + e->rebin_doubles, sizeof(og), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (n_out_of_grid) *n_out_of_grid = og;
    return 0;
}

int grm_engine_rebin_reset(grm_engine *e) {
    if (!e) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    if (e->d_rebin) {
        HIPCHK(e, hipMemsetAsync(e->d_rebin, 0, rebin_bytes(e->rebin_doubles), e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
    }
    return 0;
}

int grm_engine_rebin_grid(grm_engine *e, grm_bin_grid *out) {
    if (!e || !out) return -1;
    if (!e->rebin_on) {
        e->err = "rebin: no grid set up (grm_engine_rebin_setup)";
        return -1;
    }
    *out = e->rebin_grid;
    return 0;
}

void *grm_engine_rebin_device_ptr(grm_engine *e) { return e ? (void *)e->d_rebin : nullptr; }

int grm_engine_debug_rebin_ms(grm_engine *e, double out[2]) {
    if (!e || !out) return -1;
    out[0] = e->rebin_ms[0];
    out[1] = e->rebin_ms[1];
    return 0;
}

int grm_rebin_slice_cells(void) { return GRM_REBIN_SLICE_CELLS; }

int grm_rebin_max_slices(void) { return grm_rebin_direct_slices(); }

int grm_probe_rebin(grm_engine *e, const grm_bin_grid *grid, const grm_trace *host_records, size_t n, double *out,
                    size_t out_doubles, uint64_t *n_out_of_grid) {
    if (!e) return -1;
    if (!grid || !out || (!host_records && n)) {
        e->err = "grm_probe_rebin: null argument";
        return -1;
    }
    if (const char *bad = grm_bin_grid_check(grid)) {
        e->err = std::string("grm_probe_rebin: ") + bad;
        return -1;
    }
    const size_t doubles = grm_bin_grid_doubles(grid);
    if (out_doubles != doubles) {
        e->err = "grm_probe_rebin: the grid has " + std::to_string(doubles) + " doubles, the caller gave " +
                 std::to_string(out_doubles);
        return -1;
    }
    HIPCHK(e, hipSetDevice(e->device));
    grm_trace *d_rec = nullptr;
    uint32_t *d_keys = nullptr;
    double *d_acc = nullptr;
    unsigned long long og = 0;
    int rc = 0;
    hipError_t st = hipMalloc(&d_acc, rebin_bytes(doubles));
    if (st == hipSuccess && n) st = hipMalloc(&d_rec, n * sizeof(grm_trace));
    if (st == hipSuccess && n) st = hipMalloc(&d_keys, n * sizeof(uint32_t));
    if (st == hipSuccess) st = hipMemsetAsync(d_acc, 0, rebin_bytes(doubles), e->stream);
    if (st == hipSuccess && n)
        st = hipMemcpyAsync(d_rec, host_records, n * sizeof(grm_trace), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess)
        rc = grm_rebin_launch(grm_rebin_make(*grid, e->P.xs2, e->P.xe2), d_rec, n, d_keys, d_acc,
                              reinterpret_cast<unsigned long long *>(d_acc + doubles), e->stream, e->ev0, e->ev1, e->ev2,
                              nullptr, e->err);
    if (st == hipSuccess && rc == 0)
        st = hipMemcpyAsync(out, d_acc, doubles * sizeof(double), hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess && rc == 0)
        st = hipMemcpyAsync(&og, d_acc + doubles, sizeof(og), hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
    hipFree(d_rec);
    hipFree(d_keys);
    hipFree(d_acc);
    if (st != hipSuccess) {
        e->err = std::string("grm_probe_rebin: ") + hipGetErrorString(st);
        return -1;
    }
    if (rc) return -1;
    if (n_out_of_grid) *n_out_of_grid = og;
    return 0;
}

void *grm_engine_cell_sums_device_ptr(grm_engine *e) { return e ? (void *)e->d_cellsums : nullptr; }

int grm_probe_cell_sums(grm_engine *e, const grm_trace *host_records, size_t n, double *out, uint64_t *n_skipped) {
    if (!e || !out || (!host_records && n)) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    grm_trace *d_rec = nullptr;
    double *d_acc = nullptr;
    unsigned long long sk = 0;
    int rc = 0;
    hipError_t st = hipMalloc(&d_acc, CELLSUMS_BYTES);
    if (st == hipSuccess && n) st = hipMalloc(&d_rec, n * sizeof(grm_trace));
    if (st == hipSuccess) st = hipMemsetAsync(d_acc, 0, CELLSUMS_BYTES, e->stream);
    if (st == hipSuccess && n)
        st = hipMemcpyAsync(d_rec, host_records, n * sizeof(grm_trace), hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess)
        rc = grm_cellsums_launch(d_rec, n, d_acc, reinterpret_cast<unsigned long long *>(d_acc + GRM_CELLSUMS_DOUBLES),
                                 e->stream, e->ev0, e->ev1, nullptr, e->err);
    if (st == hipSuccess && rc == 0)
        st = hipMemcpyAsync(out, d_acc, GRM_CELLSUMS_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess && rc == 0)
        st = hipMemcpyAsync(&sk, d_acc + GRM_CELLSUMS_DOUBLES, sizeof(sk), hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
    hipFree(d_rec);
    hipFree(d_acc);
    if (st != hipSuccess) {
        e->err = std::string("grm_probe_cell_sums: ") + hipGetErrorString(st);
        return -1;
    }
    if (rc) return -1;
    if (n_skipped) *n_skipped = sk;
    return 0;
}

int grm_engine_upload(grm_engine *e, const grm_init_photon *batch, size_t n, grm_init_photon **dev_out) {
    if (!e || !dev_out || (!batch && n)) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    if (n > e->upload_cap) {
        if (e->d_upload) (void)hipFree(e->d_upload);
        e->d_upload = nullptr;
        e->upload_cap = 0;
        HIPCHK(e, hipMalloc(&e->d_upload, n * sizeof(grm_init_photon)));
        e->upload_cap = n;
    }
    HIPCHK(e, hipMemcpy(e->d_upload, batch, n * sizeof(grm_init_photon), hipMemcpyHostToDevice));
    *dev_out = e->d_upload;
    return 0;
}

int grm_engine_emit_setup(grm_engine *e, const grm_emit_zone *zones, int64_t n_zones, const double *weight,
                          const double *f) {
    if (!e) return -1;
    if (!zones || !weight || !f || n_zones != (int64_t)e->P.n1 * e->P.n2) {
        e->err = "grm_engine_emit_setup: need the zone table of all n1*n2 zones and both emission tables";
        return -1;
    }
    HIPCHK(e, hipSetDevice(e->device));
    hipFree(e->d_ezones);
    hipFree(e->d_eweight);
    hipFree(e->d_ef);
    hipFree(e->d_eoff);
    e->d_ezones = nullptr;
    e->d_eweight = e->d_ef = nullptr;
    e->d_eoff = nullptr;
    e->n_ezones = 0;
    const size_t nt = GRM_N_E_SAMP + 1;
    HIPCHK(e, hipMalloc(&e->d_ezones, (size_t)n_zones * sizeof(grm_emit_zone)));
    HIPCHK(e, hipMalloc(&e->d_eweight, nt * sizeof(double)));
    HIPCHK(e, hipMalloc(&e->d_ef, nt * sizeof(double)));
    HIPCHK(e, hipMalloc(&e->d_eoff, ((size_t)n_zones + 1) * sizeof(unsigned long long)));
    HIPCHK(e, hipMemcpy(e->d_ezones, zones, (size_t)n_zones * sizeof(grm_emit_zone), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->d_eweight, weight, nt * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->d_ef, f, nt * sizeof(double), hipMemcpyHostToDevice));
    e->n_ezones = n_zones;
    return 0;
}

int grm_engine_emit(grm_engine *e, uint64_t seed, int64_t z0, int64_t z1, grm_init_photon **dev_out,
                    uint64_t *n_out) {
    return grm_engine_emit_strided(e, seed, z0, z1, 1, dev_out, n_out);
}

int grm_engine_emit_strided(grm_engine *e, uint64_t seed, int64_t z0, int64_t z1, int64_t stride,
                            grm_init_photon **dev_out, uint64_t *n_out) {
    if (!e || !dev_out || !n_out) return -1;
    if (stride < 1) {
        e->err = "grm_engine_emit_strided: stride < 1";
        return -1;
    }
    if (!e->d_ezones) {
        e->err = "grm_engine_emit: no zone table (grm_engine_emit_setup)";
        return -1;
    }
    HIPCHK(e, hipSetDevice(e->device));
    if (z1 < 0 || z1 > e->n_ezones) z1 = e->n_ezones;
    if (z0 < 0) z0 = 0;
    if (z0 > z1) z0 = z1;
    const uint64_t n_zones = (uint64_t)((z1 - z0 + stride - 1) / stride);
    /* consts.hpp:33-157 emission constants, host libm like the host model's */
    EmitParams E;
    E.zones = e->d_ezones;
    E.weight = e->d_eweight;
    E.f = e->d_ef;
    E.l_nu_min = std::log(1.0e9);
    const double l_nu_max = std::log(1.0e16);
    E.n_l_n = l_nu_max - E.l_nu_min;
    E.d_l_nu = (l_nu_max - E.l_nu_min) / GRM_N_E_SAMP;
    E.jnu_l_min_k = std::log(0.002);
    E.jnu_d_l_k = std::log(1.0e7 / 0.002) / GRM_N_E_SAMP;
    E.k0 = (uint32_t)seed;
    E.k1 = (uint32_t)(seed >> 32);
    HIPCHK(e, hipEventRecord(e->ev0, e->stream));
    uint64_t n = 0;
    if (grm_emit_launch(e->P, E, (uint64_t)z0, (uint64_t)stride, n_zones, e->d_eoff, e->stream, &e->pin->word[4], &e->d_emit,
                        &e->emit_cap, &n, e->err))
        return -1;
    HIPCHK(e, hipEventRecord(e->ev1, e->stream));
    HIPCHK(e, hipEventSynchronize(e->ev1));
    float ms = 0.f;
    HIPCHK(e, hipEventElapsedTime(&ms, e->ev0, e->ev1));
    e->stats.last_emit_ms = ms;
    *dev_out = e->d_emit;
    *n_out = n;
    return 0;
}

int grm_engine_download(grm_engine *e, const grm_init_photon *dev, size_t n, grm_init_photon *host_out) {
    if (!e || (n && (!dev || !host_out))) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    if (n) HIPCHK(e, hipMemcpy(host_out, dev, n * sizeof(grm_init_photon), hipMemcpyDeviceToHost));
    return 0;
}

int grm_engine_debug_timing(grm_engine *e, uint64_t out[48], int reset) {
    if (!e || !out) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipMemcpy(out, e->d_timing, 48 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(e, hipMemset(e->d_timing, 0, 48 * sizeof(unsigned long long)));
#ifdef GRM_TIMING
    return 1;
#else
    return 0;
#endif
}

int64_t grm_engine_debug_waves(grm_engine *e, uint64_t *out, size_t cap) {
    if (!e || !e->d_waves) return -1;
    if (hipSetDevice(e->device) != hipSuccess) return -1;
    const size_t n = std::min(e->lanes / 64, e->waves_rows);
    const size_t k = std::min(n, cap);
    if (k && out && hipMemcpy(out, e->d_waves, k * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return (int64_t)n;
}

int grm_engine_debug_phases(grm_engine *e, uint64_t out[4]) {
    if (!e || !out) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    DevCounters h;
    if (read_counters(e, h)) return -1; /* mirrors the small words */
    unsigned long long lo = ~0ull, hi = 0;
    const size_t n = std::min(e->lanes / 64, e->waves_rows);
    if (n) {
        std::vector<unsigned long long> w(n * 4);
        HIPCHK(e, hipMemcpy(w.data(), e->d_waves, n * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            lo = std::min(lo, w[i * 4]);
            hi = std::max(hi, w[i * 4 + 1]);
        }
    }
    unsigned long long ph[2] = {0, 0};
    if (n) HIPCHK(e, hipMemcpy(ph, e->d_waves + (e->lanes / 64) * 4, sizeof(ph), hipMemcpyDeviceToHost));
    out[0] = n ? lo : 0;
    out[1] = ph[0];
    out[2] = ph[1];
    out[3] = hi;
    return 0;
}

int64_t grm_engine_debug_admissions(grm_engine *e, uint64_t *out, size_t cap) {
    if (!e || !e->d_waves || !e->waves_rows) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    unsigned long long ph[PHASE_LOG];
    HIPCHK(e, hipMemcpy(ph, e->d_waves + (e->lanes / 64) * 4, sizeof(ph), hipMemcpyDeviceToHost));
    const size_t k = std::min<size_t>(ph[2], (PHASE_LOG - 3) / 2);
    for (size_t i = 0; i < k && i < cap; ++i) {
        out[2 * i] = ph[3 + 2 * i];
        out[2 * i + 1] = ph[4 + 2 * i];
    }
    return (int64_t)k;
}

int grm_engine_debug_counters(grm_engine *e, uint64_t out[16]) {
    if (!e || !out) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    DevCounters h;
    if (read_counters(e, h)) return -1;
    std::memcpy(out, &h, sizeof(h));
    return 0;
}

int64_t grm_engine_debug_stuck(grm_engine *e, double *out, size_t cap) {
    if (!e || !e->d_small) return -1;
    if (hipSetDevice(e->device) != hipSuccess) return -1;
    unsigned long long cnt = 0;
    if (hipMemcpy(&cnt, e->d_small + (6) * SMALL_STRIDE, sizeof(cnt), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    const size_t n = std::min<size_t>(cnt, STUCK_CAP), k = std::min(n, cap);
    if (k && out && hipMemcpy(out, e->d_stuck, k * STUCK_WORDS * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    return (int64_t)n;
}

int grm_rccl_unique_id(uint8_t id_out[128]) {
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return -1;
    std::memcpy(id_out, &id, sizeof(id));
    return 0;
}

int grm_engine_comm_init(grm_engine *e, const uint8_t id_in[128], int nranks, int rank) {
    if (!e || !id_in) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    ncclUniqueId id;
    std::memcpy(&id, id_in, sizeof(id));
    const ncclResult_t r = ncclCommInitRank(&e->comm, nranks, id, rank);
    if (r != ncclSuccess) {
        e->err = std::string("ncclCommInitRank: ") + ncclGetErrorString(r);
        e->comm = nullptr;
        return -1;
    }
    return 0;
}

int grm_engine_allreduce(grm_engine *e) {
    if (!e) return -1;
    if (!e->comm) {
        e->err = "grm_engine_allreduce: no communicator (grm_engine_comm_init)";
        return -1;
    }
    HIPCHK(e, hipSetDevice(e->device));
    const size_t ncell = (size_t)N_TH_BINS * N_E_BINS * (sizeof(grm_spectrum_cell) / sizeof(double));
    unsigned long long *c = reinterpret_cast<unsigned long long *>(e->d_ctr);
    ncclResult_t r = ncclGroupStart();
    if (r == ncclSuccess) r = ncclAllReduce(e->d_spec, e->d_spec, ncell, ncclFloat64, ncclSum, e->comm, e->stream);
    /* DevCounters: [0..1] n_recorded n_scatt (sum), [2] max_tau bits (max; tau >= 0 orders as u64),
     * [3..8] steps/tracked/children/overflow/dropped/primaries (sum) */
    if (r == ncclSuccess) r = ncclAllReduce(c, c, 2, ncclUint64, ncclSum, e->comm, e->stream);
    if (r == ncclSuccess) r = ncclAllReduce(c + 2, c + 2, 1, ncclUint64, ncclMax, e->comm, e->stream);
    if (r == ncclSuccess) r = ncclAllReduce(c + 3, c + 3, 6, ncclUint64, ncclSum, e->comm, e->stream);
    const ncclResult_t r2 = ncclGroupEnd();
    if (r == ncclSuccess) r = r2;
    if (r != ncclSuccess) {
        e->err = std::string("RCCL all-reduce: ") + ncclGetErrorString(r);
        return -1;
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return 0;
}

int grm_engine_stash_reserve(grm_engine *e, int n_slots) {
    if (!e || n_slots < 0) return -1;
    if (n_slots <= e->stash_cap) return 0;
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const size_t ncell = (size_t)N_TH_BINS * N_E_BINS * (sizeof(grm_spectrum_cell) / sizeof(double));
    hipFree(e->d_stash_spec);
    hipFree(e->d_stash_sum);
    hipFree(e->d_stash_max);
    e->d_stash_spec = nullptr;
    e->d_stash_sum = e->d_stash_max = nullptr;
    e->stash_cap = 0;
    HIPCHK(e, hipMalloc(&e->d_stash_spec, (size_t)n_slots * ncell * sizeof(double)));
    HIPCHK(e, hipMalloc(&e->d_stash_sum, (size_t)n_slots * STASH_SUMS * sizeof(unsigned long long)));
    HIPCHK(e, hipMalloc(&e->d_stash_max, (size_t)n_slots * STASH_MAXS * sizeof(unsigned long long)));
    e->stash_cap = n_slots;
    /* per-pass counter blocks (grm_engine_begin_pass); a new allocation unlinks the peers */
    if (e->ctr_slot >= 0) e->d_ctr = e->d_ctr_own;
    e->ctr_slot = -1;
    hipFree(e->d_ctr_slots);
    e->d_ctr_slots = nullptr;
    e->n_ctr_slots = 0;
    hipFree(e->d_peers);
    e->d_peers = nullptr;
    e->n_peers = 0;
    HIPCHK(e, hipMalloc(&e->d_ctr_slots, (size_t)n_slots * sizeof(DevCounters)));
    HIPCHK(e, hipMemset(e->d_ctr_slots, 0, (size_t)n_slots * sizeof(DevCounters)));
    e->n_ctr_slots = n_slots;
    return 0;
}

int grm_engine_begin_pass(grm_engine *e, int slot) {
    if (!e) return -1;
    if (slot >= e->n_ctr_slots) {
        e->err = "grm_engine_begin_pass: slot " + std::to_string(slot) + " outside the reserved " +
                 std::to_string(e->n_ctr_slots) + " (grm_engine_stash_reserve)";
        return -1;
    }
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->ctr_slot = slot < 0 ? -1 : slot;
    e->d_ctr = slot < 0 ? e->d_ctr_own : e->d_ctr_slots + slot;
    return grm_engine_reset(e);
}

int grm_engine_counters_ipc_handle(grm_engine *e, uint8_t out[64]) {
    if (!e || !out) return -1;
    if (!e->d_ctr_slots) {
        e->err = "grm_engine_counters_ipc_handle: no pass slots (grm_engine_stash_reserve first)";
        return -1;
    }
    HIPCHK(e, hipSetDevice(e->device));
    hipIpcMemHandle_t h;
    HIPCHK(e, hipIpcGetMemHandle(&h, e->d_ctr_slots));
    static_assert(sizeof(h) <= 64, "IPC handle size");
    std::memset(out, 0, 64);
    std::memcpy(out, &h, sizeof(h));
    return 0;
}

namespace {
int upload_peers(grm_engine *e, const std::vector<const DevCounters *> &tab) {
    hipFree(e->d_peers);
    e->d_peers = nullptr;
    e->n_peers = 0;
    if (tab.size() < 2) return 0;
    HIPCHK(e, hipMalloc(&e->d_peers, tab.size() * sizeof(DevCounters *)));
    HIPCHK(e, hipMemcpy(e->d_peers, tab.data(), tab.size() * sizeof(DevCounters *), hipMemcpyHostToDevice));
    e->n_peers = (int)tab.size();
    return 0;
}
} /* namespace */

int grm_engine_set_peers(grm_engine *e, const uint8_t *handles, int n, int rank) {
    if (!e || n < 0 || (n > 1 && (!handles || rank < 0 || rank >= n))) return -1;
    if (n > 64) {
        e->err = "grm_engine_set_peers: at most 64 ranks";
        return -1;
    }
    HIPCHK(e, hipSetDevice(e->device));
    for (void *p : e->ipc_open) hipIpcCloseMemHandle(p);
    e->ipc_open.clear();
    std::vector<const DevCounters *> tab;
    if (n > 1) {
        if (!e->d_ctr_slots) {
            e->err = "grm_engine_set_peers: no pass slots (grm_engine_stash_reserve first)";
            return -1;
        }
        for (int r = 0; r < n; ++r) {
            if (r == rank) {
                tab.push_back(e->d_ctr_slots);
                continue;
            }
            hipIpcMemHandle_t h;
            std::memcpy(&h, handles + (size_t)r * 64, sizeof(h));
            void *p = nullptr;
            const hipError_t st = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
            if (st != hipSuccess) {
                for (void *q : e->ipc_open) hipIpcCloseMemHandle(q);
                e->ipc_open.clear();
                e->err = std::string("grm_engine_set_peers: hipIpcOpenMemHandle of rank ") + std::to_string(r) + ": " +
                         hipGetErrorString(st);
                upload_peers(e, {});
                return -1;
            }
            e->ipc_open.push_back(p);
            tab.push_back(reinterpret_cast<const DevCounters *>(p));
        }
    }
    return upload_peers(e, tab);
}

int grm_device_peer_ok(int device, int peer) {
    if (device == peer) return 1;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, device, peer) != hipSuccess) return 0;
    return can ? 1 : 0;
}

int grm_engine_link_peers(grm_engine *const *engines, int n) {
    if (!engines || n < 1) return -1;
    std::vector<const DevCounters *> tab;
    for (int r = 0; r < n; ++r) {
        if (!engines[r] || !engines[r]->d_ctr_slots || engines[r]->device != engines[0]->device) return -1;
        tab.push_back(engines[r]->d_ctr_slots);
    }
    for (int r = 0; r < n; ++r) {
        grm_engine *e = engines[r];
        HIPCHK(e, hipSetDevice(e->device));
        if (upload_peers(e, n > 1 ? tab : std::vector<const DevCounters *>{})) return -1;
    }
    return 0;
}

int grm_engine_job_counters(grm_engine *e, double out[4]) {
    if (!e || !out) return -1;
    HIPCHK(e, hipSetDevice(e->device));
    Ctl C{};
    C.ctr = e->d_ctr;
    C.peers = e->d_peers;
    C.n_peers = (e->ctr_slot >= 0 && e->d_peers) ? e->n_peers : 0;
    C.ctr_slot = e->ctr_slot;
    double *d = nullptr;
    HIPCHK(e, hipMalloc(&d, 4 * sizeof(double)));
    hipLaunchKernelGGL(job_counters_kernel, dim3(1), dim3(64), 0, e->stream, e->P, C, d);
    hipError_t st = hipGetLastError();
    if (st == hipSuccess) st = hipMemcpyAsync(out, d, 4 * sizeof(double), hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
    (void)hipFree(d);
    return hip_ok(e, st, "job counters") ? 0 : -1;
}

int grm_engine_stash(grm_engine *e, int slot) {
    if (!e) return -1;
    if (slot < 0 || slot >= e->stash_cap) {
        e->err = "grm_engine_stash: slot " + std::to_string(slot) + " outside the reserved " +
                 std::to_string(e->stash_cap) + " (grm_engine_stash_reserve)";
        return -1;
    }
    HIPCHK(e, hipSetDevice(e->device));
    const int ncell = N_TH_BINS * N_E_BINS * (int)(sizeof(grm_spectrum_cell) / sizeof(double));
    hipLaunchKernelGGL(stash_kernel, dim3(8), dim3(256), 0, e->stream, reinterpret_cast<const double *>(e->d_spec),
                       e->d_ctr, e->d_stash_spec, e->d_stash_sum, e->d_stash_max, slot, ncell);
    HIPCHK(e, hipGetLastError());
    return 0;
}

int grm_engine_allreduce_stash(grm_engine *e, int first, int n_slots) {
    if (!e) return -1;
    if (first < 0 || n_slots < 0 || first + n_slots > e->stash_cap) {
        e->err = "grm_engine_allreduce_stash: slots outside the reserved stash";
        return -1;
    }
    if (!e->comm) {
        e->err = "grm_engine_allreduce_stash: no communicator (grm_engine_comm_init)";
        return -1;
    }
    if (n_slots == 0) return 0;
    HIPCHK(e, hipSetDevice(e->device));
    const size_t ncell = (size_t)N_TH_BINS * N_E_BINS * (sizeof(grm_spectrum_cell) / sizeof(double));
    ncclResult_t r = ncclGroupStart();
    if (r == ncclSuccess)
        r = ncclAllReduce(e->d_stash_spec + (size_t)first * ncell, e->d_stash_spec + (size_t)first * ncell,
                          (size_t)n_slots * ncell, ncclFloat64, ncclSum, e->comm, e->stream);
    if (r == ncclSuccess)
        r = ncclAllReduce(e->d_stash_sum + (size_t)first * STASH_SUMS, e->d_stash_sum + (size_t)first * STASH_SUMS,
                          (size_t)n_slots * STASH_SUMS, ncclUint64, ncclSum, e->comm, e->stream);
    if (r == ncclSuccess)
        r = ncclAllReduce(e->d_stash_max + (size_t)first * STASH_MAXS, e->d_stash_max + (size_t)first * STASH_MAXS,
                          (size_t)n_slots * STASH_MAXS, ncclUint64, ncclMax, e->comm, e->stream);
    const ncclResult_t r2 = ncclGroupEnd();
    if (r == ncclSuccess) r = r2;
    if (r != ncclSuccess) {
        e->err = std::string("RCCL all-reduce (stash): ") + ncclGetErrorString(r);
        return -1;
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return 0;
}

int grm_engine_stash_read(grm_engine *e, int slot, grm_spectrum_cell *spec, uint64_t *n_rec, uint64_t *n_scatt,
                          double *max_tau, uint64_t *n_steps) {
    if (!e) return -1;
    if (slot < 0 || slot >= e->stash_cap) {
        e->err = "grm_engine_stash_read: slot outside the reserved stash";
        return -1;
    }
    HIPCHK(e, hipSetDevice(e->device));
    const size_t ncell = (size_t)N_TH_BINS * N_E_BINS * (sizeof(grm_spectrum_cell) / sizeof(double));
    unsigned long long sums[STASH_SUMS], maxs[STASH_MAXS];
    if (spec)
        HIPCHK(e, hipMemcpyAsync(spec, e->d_stash_spec + (size_t)slot * ncell, ncell * sizeof(double),
                                 hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(sums, e->d_stash_sum + (size_t)slot * STASH_SUMS, sizeof(sums), hipMemcpyDeviceToHost,
                             e->stream));
    HIPCHK(e, hipMemcpyAsync(maxs, e->d_stash_max + (size_t)slot * STASH_MAXS, sizeof(maxs), hipMemcpyDeviceToHost,
                             e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (n_rec) *n_rec = sums[0];
    if (n_scatt) *n_scatt = sums[1];
    if (n_steps) *n_steps = sums[2];
    if (max_tau) std::memcpy(max_tau, &maxs[0], sizeof(double));
    return 0;
}

int grm_engine_stash_raw(grm_engine *e, int first, int n_slots, double *spec, uint64_t *sums, uint64_t *maxs,
                         int write) {
    if (!e) return -1;
    if (first < 0 || n_slots < 0 || first + n_slots > e->stash_cap) {
        e->err = "grm_engine_stash_raw: slots outside the reserved stash";
        return -1;
    }
    if (n_slots == 0) return 0;
    HIPCHK(e, hipSetDevice(e->device));
    const size_t ncell = (size_t)N_TH_BINS * N_E_BINS * (sizeof(grm_spectrum_cell) / sizeof(double));
    const hipMemcpyKind k = write ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    struct Part {
        void *dev, *host;
        size_t bytes;
    } parts[3] = {{e->d_stash_spec + (size_t)first * ncell, spec, (size_t)n_slots * ncell * sizeof(double)},
                  {e->d_stash_sum + (size_t)first * STASH_SUMS, sums, (size_t)n_slots * STASH_SUMS * sizeof(uint64_t)},
                  {e->d_stash_max + (size_t)first * STASH_MAXS, maxs, (size_t)n_slots * STASH_MAXS * sizeof(uint64_t)}};
    for (const Part &q : parts) {
        if (!q.host) continue;
        if (write)
            HIPCHK(e, hipMemcpyAsync(q.dev, q.host, q.bytes, k, e->stream));
        else
            HIPCHK(e, hipMemcpyAsync(q.host, q.dev, q.bytes, k, e->stream));
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return 0;
}

int grm_stash_words(int which) {
    switch (which) {
    case 0: return N_TH_BINS * N_E_BINS * (int)(sizeof(grm_spectrum_cell) / sizeof(double));
    case 1: return STASH_SUMS;
    case 2: return STASH_MAXS;
    default: return -1;
    }
}

int grm_probe(grm_engine *e, int which, const double *in, int in_stride, double *out, int out_stride, size_t n) {
    if (!e) return -1;
    hipSetDevice(e->device);
    return grm_probe_impl(e->P, e->stream, which, in, in_stride, out, out_stride, n, e->err);
}

size_t grm_sizeof(int which) {
    switch (which) {
    case 0: return sizeof(grm_header);
    case 1: return sizeof(grm_units);
    case 2: return sizeof(grm_init_photon);
    case 3: return sizeof(grm_spectrum_cell);
    case 4: return sizeof(grm_trace);
    case 5: return sizeof(grm_stats);
    case 6: return sizeof(grm_emit_zone);
    case 7: return sizeof(grm_bin_grid);
    default: return 0;
    }
}

const char *grm_version(void) { return "grmonty_amd 0.1.0 (gfx950)"; }

} /* extern "C" */

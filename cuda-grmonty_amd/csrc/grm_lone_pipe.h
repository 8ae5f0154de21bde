/*
 * grm_lone_pipe.h -- the two-wave lone-photon pipeline: the ring between a pair's geometry and
 * interaction waves (LoneSlot, LoneCtl, LonePair, s_pair), the geometry wave (lone_geometry) and the
 * interaction wave (lone_draw, lone_stop, lone_interact).  Used by the lone kernels (grm_lone.hip)
 * and by tools/microbench/geom_only.hip, which times the geometry wave alone.
 */
#ifndef GRM_LONE_PIPE_H
#define GRM_LONE_PIPE_H

#include "grm_transport.h"

namespace {

/* Two waves per handed-over photon, pipelined: the geometry wave (wave 1) runs the photon's
 * geodesic ahead -- photon_2, step size, push as a halving walk over its lanes (:920-930) -- into a
 * ring of LONE_RING steps in LDS; the interaction wave (wave 0) consumes them in order and does
 * everything else of the loop body: the stop criteria with their roulette draws, fluid, absorption
 * and scattering coefficients, bias, the scattering decision, the weight (:919, :932-1063).  The
 * geodesic does not depend on the interactions except at a scattering, where the photon continues
 * from photon_2 pushed to the scattering point (:1005-1010): the interaction wave makes that push
 * itself and restarts the geometry wave from it (a new generation; steps of the old one are
 * discarded by their tag).  Both halves of a step then run at once on two SIMDs. */
constexpr int LONE_RING = 32, LONE_BATCH = 16;
constexpr unsigned long long LONE_STOP = ~0ull;
struct alignas(16) LoneSlot {
    double out[13], dl;     /* the state after the push (x, k, dk/dlambda, e_0_s) and the step size */
    unsigned long long tag; /* (generation << 32) | (step index + 1), stored last */
};
struct alignas(16) LoneCtl {
    double rs[13];                /* restart state: photon_2 of the generation's first step */
    unsigned long long cons, req; /* steps consumed; restart request (generation << 32 | step) or LONE_STOP */
};
/* one photon's two-wave pipeline state (a geometry wave + an interaction wave) */
struct LonePair {
    LoneSlot ring[LONE_RING];
    LoneCtl ctl;
};
constexpr int LONE_PAIRS = 2; /* pairs of the concurrent worker (early_kernel: 4 waves, one per SIMD, up to 512 VGPRs) */
/* early_kernel dispatches its geometry waves to s_pair[0] / s_pair[1] by a constant index (one inlined
 * copy per pair): more pairs need more arms there, or a pair's interaction wave waits forever */
static_assert(LONE_PAIRS == 2, "early_kernel's geometry dispatch assumes two pairs");
/* early_kernel waits this long (s_memrealtime, 100 MHz) for the bulk launch to start before it
 * takes the launches for serialised and leaves */
constexpr unsigned long long EARLY_ALONE_TICKS = 100000; /* 1 ms */
__shared__ LonePair s_pair[LONE_PAIRS];

constexpr bool GEO_QUAD = true; /* the geometry wave pushes with quad-parallel corrector rows (§4.2:
                                   * the plain push 1.41-1.42 us/step against 1.36-1.37, s3e) */

/* The geometry wave of a pair (see above): runs photon after photon -- each begins as a restart
 * request from the interaction wave -- until LONE_STOP. */
__device__ void lone_geometry(const Params &P_, const Ctl &C, int lane, LonePair &pr) {
    Params P = P_;
    push_params_vgpr(P);
    unsigned gen = 0;
    unsigned long long p = 0, cur = 0, cons = 0; /* cons: the last value read of pr.ctl.cons */
    bool spec = false; /* speculate the halving depths on this step's push (the last one halved) */
    double x[4], k[4], dk[4], e_0_s;
    {
        /* a photon starts as a restart (generation, step 0) from its hand-over state in rs */
        unsigned long long r0;
        while ((r0 = __hip_atomic_load(&pr.ctl.req, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP)) == 0)
            __builtin_amdgcn_s_sleep(2);
        if (r0 == LONE_STOP) return;
        cur = r0;
        gen = (unsigned)(r0 >> 32);
        p = r0 & 0xffffffffull;
        cons = p;
        unpack13(pr.ctl.rs, x, k, dk, e_0_s);
    }
    const double *ph2src = pr.ctl.rs; /* where the current step's start state (photon_2) is kept */
#ifdef GRM_TIMING
    unsigned long long g_last = __builtin_amdgcn_s_memtime();
    unsigned long long tg[6] = {0, 0, 0, 0, 0, 0}; /* steps, rounds, walk, step size, rest, halved */
#endif
    while (true) {
        if (p + 1 >= cons + LONE_RING) { /* the slot of step p and that of p - 1 must be consumed */
            cons = __hip_atomic_load(&pr.ctl.cons, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (p + 1 >= cons + LONE_RING) {
#ifdef GRM_TIMING
                const unsigned long long t0 = __builtin_amdgcn_s_memtime();
                __builtin_amdgcn_s_sleep(1); /* the ring is full */
                if (lane == 0) atomicAdd(C.timing + 31, __builtin_amdgcn_s_memtime() - t0);
#else
                __builtin_amdgcn_s_sleep(1); /* the ring is full */
#endif
                if (__hip_atomic_load(&pr.ctl.req, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == cur) continue;
            }
        }
        /* the restart request (stop folded in as LONE_STOP): read once per step and looked at
         * after the push, so that its LDS latency hides behind it; a step computed while a
         * restart was pending is dropped (and one published just before a restart carries the
         * old generation's tag, which the interaction wave skips) */
        const unsigned long long req = __hip_atomic_load(&pr.ctl.req, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#ifdef GRM_TIMING
        const unsigned long long g0 = __builtin_amdgcn_s_memtime();
#endif
        const double dl = step_size(P, x, k);
#ifdef GRM_TIMING
        const unsigned long long g1 = __builtin_amdgcn_s_memtime();
#endif
        /* Most steps pass their first attempt: then every lane makes that same attempt, the
         * state stays identical over the wave and needs no broadcast.  A step that halves
         * continues as a halving walk, and the next step speculates from the start. */
        int rounds = 1;
        {
            if (!spec) {
                bool fail = false;
                if (!(x[1] < P.xs1)) {
                    double e_1;
                    Trig T;
                    Gcov G;
                    /* every quad of lanes makes the attempt, lane q contracting connection row q */
                    fail = GEO_QUAD ? push_attempt_quad(P, x, k, dk, e_0_s, dl, e_1, T, G, lane & 3)
                                    : push_attempt(P, x, k, dk, e_0_s, dl, e_1, T, G);
                    if (fail) { /* depth 0 failed: the serial walk goes on at depth 1 (:1279-1285) */
                        /* from the step's start state, photon_2: the slot published last (or the
                         * generation's restart state) -- no register copy on every step for the ~2 %
                         * that fail (the copy cost ~24 moves per step of the serial chain) */
                        double e_r;
                        unpack13(ph2src, x, k, dk, e_r);
                        rounds += walk_push<GEO_QUAD>(P, x, k, dk, e_0_s, dl, 1, 2u, GEO_QUAD ? lane >> 2 : lane, 0);
                    } else {
                        e_0_s = e_1;
                    }
                }
                spec = fail;
            } else {
                rounds = walk_push<GEO_QUAD>(P, x, k, dk, e_0_s, dl, 0, 0u, GEO_QUAD ? lane >> 2 : lane, 0);
                spec = rounds > 1;
            }
        }
        if (req != cur) {
            if (req == LONE_STOP) {
#ifdef GRM_TIMING
                /* slots 16-21: photons of > 1e5 steps (the tail), 22-27: the others */
                if (lane == 0)
                    for (int r = 0; r < 6; ++r) atomicAdd(C.timing + (tg[0] > 100000 ? 16 : 22) + r, tg[r]);
#endif
                break;
            }
            /* restart from the scattering point (this step, if computed, is on the old geodesic) */
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); /* rs was written before req */
            cur = req;
            gen = (unsigned)(req >> 32);
            p = req & 0xffffffffull;
            cons = p; /* what the interaction wave has consumed when it requests a restart at p */
            unpack13(pr.ctl.rs, x, k, dk, e_0_s);
            ph2src = pr.ctl.rs;
            spec = false;
            continue;
        }
#ifdef GRM_TIMING
        const unsigned long long g2 = __builtin_amdgcn_s_memtime();
        tg[0] += 1;
        tg[1] += (unsigned long long)rounds;
        tg[2] += g2 - g1;
        tg[3] += g1 - g0;
        tg[4] += g0 - g_last;
        tg[5] += spec ? 1ull : 0ull;
        g_last = g2;
#endif
        if (lane == 0) {
            LoneSlot &S = pr.ring[p % LONE_RING];
            pack13(S.out, x, k, dk, e_0_s);
            S.dl = dl;
            /* LDS operations of a wave complete in order: the slot is written before its tag
             * (a compiler barrier keeps the stores in program order; no wait for completion) */
            __asm__ volatile("" ::: "memory");
            __hip_atomic_store(&S.tag, ((unsigned long long)gen << 32) | (p + 1), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        ph2src = pr.ring[p % LONE_RING].out; /* lane 0's stores precede this wave's later loads */
        ++p;
    }
}

/* The draws of a lone photon come from a window of 64 consecutive Philox counters evaluated at once
 * (lane i: counter wbase + i; the same block and bits as uniform(), so the same numbers in the same
 * order): a serial draw is then two v_readlane instead of a 10-round Philox chain. */
__device__ __forceinline__ double lone_draw(Rng &rng, double &win, uint32_t &wbase, int lane) {
    if (rng.ctr - wbase >= 64u) { /* wave-uniform */
        wbase = rng.ctr;
        Rng g = rng;
        g.ctr = wbase + (uint32_t)lane;
        win = uniform(g);
    }
    const double u = bcast(win, (int)(rng.ctr - wbase));
    ++rng.ctr;
    return u;
}

/* stop_criterion (harm_model.cpp:1589-1616) with the windowed draws */
__device__ __forceinline__ bool lone_stop(const Params &P, double x1, double &w, Rng &rng, double &win,
                                          uint32_t &wbase, int lane) {
    if (x1 < P.x1_min) return true;
    if (x1 > P.x1_max) {
        if (w < WEIGHT_MIN) {
            if (lone_draw(rng, win, wbase, lane) <= 1.0 / ROULETTE)
                w *= ROULETTE;
            else
                w = 0.0;
        }
        return true;
    }
    if (w < WEIGHT_MIN) {
        if (lone_draw(rng, win, wbase, lane) <= 1.0 / ROULETTE) {
            w *= ROULETTE;
        } else {
            w = 0.0;
            return true;
        }
    }
    return false;
}

/* The interaction wave of a pair: one handed-over photon, from its record to its end (the
 * geometry wave is started on it with a restart request: generation gen + 1, step 0). */
/* kids: where the photon's scattered children go -- 0 the overflow pool, 1 the early worker's queue,
 * 2 the lone kernel's (queue_child_push) */
__device__ void lone_interact(const Params &P, const Ctl &C, const LoneRec &R, int lane, LonePair &pr, unsigned &gen_io,
                              int kids) {
    double x1 = R.x[1];
    unsigned gen = gen_io + 1;
    if (lane == 0) {
        double x[4], k[4], dk[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[i] = R.x[i];
            k[i] = R.k[i];
            dk[i] = R.dk[i];
        }
        pack13(pr.ctl.rs, x, k, dk, R.e_0_s); /* the state before step 0 */
        pr.ctl.cons = 0;
        __hip_atomic_store(&pr.ctl.req, (unsigned long long)gen << 32, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    const bool own = lane == 0;
    const int rank = lane;
    double w = R.w;
    double tau_abs = R.tau_abs, tau_scatt = R.tau_scatt, a_si = R.a_si, a_ai = R.a_ai, bi = R.bi, fl_ne = R.fl_ne;
    const Cold *cold = &R.c;
    int n_step = R.n_step;
    const int n_scatt = R.n_scatt;
    Rng rng;
    rng.k0 = C.key0;
    rng.k1 = C.key1;
    rng.id = R.id;
    rng.ctr = R.ctr;
    rng.ctr_hi = 0;
    double win = 0.0;
    uint32_t wbase = rng.ctr - 64u; /* empty window */
    double bias_d = bias_den(P, C);
    const unsigned long long rt_start = __builtin_amdgcn_s_memrealtime();
    unsigned long long steps = 0, children = 0;
    bool ended = false, abandoned = false;
    int reason = -1; /* ended without a record: trace reason */
    unsigned long long gen_start = 0; /* the generation's first step */
    unsigned long long si = 0;        /* index of the next step */
    /* the step whose end state is the photon's state (LONE_STOP: the restart state in rs) */
    unsigned long long cur = LONE_STOP;
    unsigned since = 0; /* steps since the last counter flush / bias refresh / watchdog look */
    bool done = false;
#ifdef GRM_TIMING
    unsigned long long ti[4] = {0, 0, 0, 0}; /* batches, steps in them, batch-evaluation cycles, serial cycles */
#endif
    while (!done) {
        /* A batch: the consecutive steps the geometry wave has ready (at least one, at most
         * LONE_BATCH).  Lane j evaluates step si + j at once: the fluid and the absorption /
         * scattering coefficients at its end point (these depend on the geodesic only), and from
         * them -- taking the previous step's coefficients from lane j - 1, as the serial recurrence
         * has them whenever step j interacts -- its optical depths, the weight factor of a step
         * without scattering and the weight-independent part of bias_func.  The steps then run in
         * order, each taking its lane's values; a scattering discards the rest of the batch (the
         * photon continues elsewhere). */
        if (since >= REFRESH_TRIPS) { /* at a batch boundary, so that bias_d is fixed over a batch */
            since = 0;
            flush_counters(C);
            if (!C.bias_frozen) bias_d = bias_den(P, C);
            if (C.watchdog_ticks) {
                bool stop = __hip_atomic_load(&C.ctr->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
                if (!stop && __builtin_amdgcn_s_memrealtime() - rt_start > C.watchdog_ticks) {
                    stop = true;
                    if (own) __hip_atomic_store(&C.ctr->abort, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                if (stop) {
                    abandoned = true;
                    break;
                }
            }
        }
        const unsigned long long base = si;
        {
            LoneSlot &S0 = pr.ring[base % LONE_RING];
            const unsigned long long want = ((unsigned long long)gen << 32) | (base + 1);
#ifdef GRM_TIMING
            const unsigned long long tw0 = __builtin_amdgcn_s_memtime();
#endif
            while (__hip_atomic_load(&S0.tag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != want)
                __builtin_amdgcn_s_sleep(1);
#ifdef GRM_TIMING
            if (own) atomicAdd(C.timing + 30, __builtin_amdgcn_s_memtime() - tw0);
#endif
        }
        const unsigned long long qj = base + (lane < LONE_BATCH ? lane : 0);
        const bool ready = lane < LONE_BATCH && __hip_atomic_load(&pr.ring[qj % LONE_RING].tag, __ATOMIC_ACQUIRE,
                                                                  __HIP_MEMORY_SCOPE_WORKGROUP) ==
                                                    (((unsigned long long)gen << 32) | (qj + 1));
        const unsigned long long rb = __ballot(ready);
        const int nb = rb == ~0ull ? 64 : __ffsll((long long)~rb) - 1; /* leading run of ready steps (>= 1) */
#ifdef GRM_TIMING
        const unsigned long long tb0 = __builtin_amdgcn_s_memtime();
#endif
        double l_x1, l_ne, l_as = 0.0, l_aa = 0.0, l_dts, l_dta, l_b0, l_fac;
        int l_zero;
        {
            const LoneSlot &Sj = pr.ring[(base + (lane < nb ? lane : 0)) % LONE_RING];
            double xj[4], kj[4], dkj[4], ej;
            unpack13(Sj.out, xj, kj, dkj, ej);
            const double dl = Sj.dl;
            Trig T;
            Gcov G;
            ZoneFetch Z;
            zone_fetch(P, xj, Z);
            trig_at(P, xj, T);
            gcov_from_trig(P, T, G);
            Fluid F;
            fluid_from(P, xj, G, Z, F);
            const double nu = fluid_nu(kj, F);
            l_zero = (nu < 0.0 || F.n_e == 0.0) ? 1 : 0; /* bound_flag (:941-955) or nu < 0 */
            if (!l_zero) radiation_coeffs(P, kj, F, nu, l_as, l_aa);
            l_x1 = xj[1];
            l_ne = F.n_e;
            /* the coefficients the step starts from: the step before's (lane j - 1), or the carried
             * (the shuffles outside the conditional: with lane 0 masked off, lane 1 would read 0) */
            const double up_as = __shfl_up(l_as, 1), up_aa = __shfl_up(l_aa, 1);
            const double p_as = lane == 0 ? a_si : up_as, p_aa = lane == 0 ? a_ai : up_aa;
            if (l_zero) {
                l_dts = 0.5 * p_as * P.d_tau_k * dl;
                l_dta = 0.5 * p_aa * P.d_tau_k * dl;
                l_b0 = 0.0;
            } else {
                l_dts = 0.5 * (p_as + l_as) * P.d_tau_k * dl;
                l_dta = 0.5 * (p_aa + l_aa) * P.d_tau_k * dl;
                /* bias_func up to its weight cap (same operations) */
                l_b0 = fdiv(100.0 * F.theta_e * F.theta_e, bias_d);
                if (l_b0 < TP_OVER_TE) l_b0 = TP_OVER_TE;
            }
            const double d_tau = l_dta + l_dts;
            l_fac = d_tau < 1.0e-3 ? (1.0 - d_tau * (1.0 / 24.0) * (24.0 - d_tau * (12.0 - d_tau * (4.0 - d_tau))))
                                   : fexp(-d_tau);
        }
#ifdef GRM_TIMING
        const unsigned long long tb1 = __builtin_amdgcn_s_memtime();
        ti[0] += 1;
        ti[1] += (unsigned long long)nb;
        ti[2] += tb1 - tb0;
#endif
        /* The batch's leading run of PLAIN steps is committed at once: a step that interacts,
         * neither stops, roulettes, scatters nor is absorbed changes the state only by w *= fac,
         * tau += d_tau, one draw and the coefficients it leaves -- every lane decides its step from
         * the weight before it (the sequential product, in the serial order, so bit-identical) and
         * the draw at its counter; the first lane that is not plain ends the run, and its step (and
         * the rest of the batch) goes through the serial code below. */
        int bj0 = 0;
        {
            /* weight and optical depths before step j (lane j), and after all nb steps (lane nb) */
            double w_run = w, ta_run = tau_abs, ts_run = tau_scatt;
            double w_j = w, ta_j = tau_abs, ts_j = tau_scatt;
            for (int j = 0; j < nb; ++j) {
                if (lane == j) {
                    w_j = w_run;
                    ta_j = ta_run;
                    ts_j = ts_run;
                }
                w_run = w_run * bcast(l_fac, j);
                ta_run = ta_run + bcast(l_dta, j);
                ts_run = ts_run + bcast(l_dts, j);
            }
            if (lane == nb) {
                w_j = w_run;
                ta_j = ta_run;
                ts_j = ts_run;
            }
            /* the window of draws must hold counters rng.ctr .. rng.ctr + nb - 1 */
            if (rng.ctr - wbase + (uint32_t)nb > 64u) {
                wbase = rng.ctr;
                Rng g = rng;
                g.ctr = wbase + (uint32_t)lane;
                win = uniform(g);
            }
            const double u = __shfl(win, (int)(rng.ctr - wbase) + (lane < nb ? lane : 0));
            /* the state before step j: lane j - 1's results, or the carried ones for j = 0 */
            const double up_x1 = __shfl_up(l_x1, 1), up_ne = __shfl_up(l_ne, 1);
            const double up_as = __shfl_up(l_as, 1), up_aa = __shfl_up(l_aa, 1);
            const double x1_prev = lane == 0 ? x1 : up_x1;
            const double ne_prev = lane == 0 ? fl_ne : up_ne, as_prev = lane == 0 ? a_si : up_as,
                         aa_prev = lane == 0 ? a_ai : up_aa;
            /* bias_func with the weight cap (:1391-1404) and the interaction's bias (:977) */
            double bf = 0.0;
            if (!l_zero) {
                const double max = w_j * (0.5 / WEIGHT_MIN);
                double b = l_b0;
                if (b > max) b = max;
                bf = b * (1.0 / TP_OVER_TE);
            }
            const double up_bf = __shfl_up(bf, 1);
            const double bi_prev = lane == 0 ? bi : up_bf;
            const double bias = l_zero ? 0.0 : 0.5 * (bi_prev + bf);
            const double bdt = bias * l_dts;
            const bool may = bdt > (1.0 - u) * (1.0 - 0x1p-40);
            const double lx = may ? -flog(u) : 0.0;
            bool scatter = may && bdt > lx;
            if (scatter) scatter = fdiv(w_j, bias) > WEIGHT_MIN;
            const bool plain = lane < nb && !(x1_prev < P.x1_min) && !(x1_prev > P.x1_max) && !(w_j < WEIGHT_MIN) &&
                               !(l_x1 < P.x1_min) && !(l_x1 > P.x1_max) && !isnan(l_x1) &&
                               (aa_prev > 0.0 || as_prev > 0.0 || ne_prev > 0.0) && !scatter && !(l_dta > 100) &&
                               n_step + lane + 1 <= MAX_N_STEP;
            const unsigned long long np = __ballot(!plain);
            bj0 = np ? __ffsll((long long)np) - 1 : 64; /* lanes >= nb are not plain: bj0 <= nb */
            if (bj0 > 0) {
                const int l = bj0 - 1;
                w = bcast(w_j, bj0);
                tau_abs = bcast(ta_j, bj0);
                tau_scatt = bcast(ts_j, bj0);
                x1 = bcast(l_x1, l);
                fl_ne = bcast(l_ne, l);
                a_si = bcast(l_as, l);
                a_ai = bcast(l_aa, l);
                bi = bcast(bf, l);
                rng.ctr += (uint32_t)bj0;
                n_step += bj0;
                steps += (unsigned long long)bj0;
                since += (unsigned)bj0;
                cur = base + (unsigned long long)l;
                si = base + (unsigned long long)bj0;
                if (own) __hip_atomic_store(&pr.ctl.cons, si, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        for (int bj = bj0; bj < nb; ++bj) {
            ++since;
            /* while (!stop_criterion(photon)) (:919) */
            if (lone_stop(P, x1, w, rng, win, wbase, lane)) {
                ended = done = true;
                break;
            }
            /* photon_2, step size and push of this step: from the geometry wave */
            cur = base + bj;
            x1 = bcast(l_x1, bj);
            ++steps;
            if (lone_stop(P, x1, w, rng, win, wbase, lane)) { /* :932-934 */
                ended = done = true;
                break;
            }
            if (isnan(x1)) { /* a NaN position is absorbing (see transport_trip) */
                if (own) atomicAdd(&C.ctr->n_nan, 1ull);
                ended = done = true;
                reason = 3;
                break;
            }
            if (a_ai > 0.0 || a_si > 0.0 || fl_ne > 0.0) { /* :937 */
                const bool zero = __builtin_amdgcn_readlane(l_zero, bj) != 0;
                fl_ne = bcast(l_ne, bj);
                double d_tau_scatt = bcast(l_dts, bj), d_tau_abs = bcast(l_dta, bj), bf = 0.0, bias = 0.0;
                if (!zero) { /* bias_func's weight cap (:1391-1404) */
                    const double max = w * (0.5 / WEIGHT_MIN);
                    double b = bcast(l_b0, bj);
                    if (b > max) b = max;
                    bf = b * (1.0 / TP_OVER_TE);
                    bias = 0.5 * (bi + bf);
                }
                a_si = bcast(l_as, bj);
                a_ai = bcast(l_aa, bj);
                bi = bf;
                /* x1 = -log u, settled without the logarithm when possible (as in transport_trip) */
                const double u = lone_draw(rng, win, wbase, lane);
                const double bdt = bias * d_tau_scatt;
                const bool may = bdt > (1.0 - u) * (1.0 - 0x1p-40);
                const double lx = may ? -flog(u) : 0.0;
                bool scatter = may && bdt > lx;
                double wc = 0.0;
                if (scatter) { /* w / bias only when it decides (:985) */
                    wc = fdiv(w, bias);
                    scatter = wc > WEIGHT_MIN;
                }
                if (scatter) { /* :985 */
                    const double frac = fdiv(lx, bias * d_tau_scatt);
                    d_tau_abs *= frac;
                    if (d_tau_abs > 100) { /* absorbed before scattering */
                        ended = done = true;
                        reason = 2;
                        break;
                    }
                    d_tau_scatt *= frac;
                    const double d_tau = d_tau_abs + d_tau_scatt;
                    if (d_tau_abs < 1.0e-3)
                        w *= (1.0 - d_tau * (1.0 / 24.0) * (24.0 - d_tau * (12.0 - d_tau * (4.0 - d_tau))));
                    else
                        w *= fexp(-d_tau);
                    /* photon_2 pushed to the scattering point (:1005-1010), by this wave */
                    double x[4], k[4], dk[4], e_0_s;
                    /* photon_2 of this step: the state after the step before, or the restart state */
                    unpack13(base + bj == gen_start ? pr.ctl.rs : pr.ring[(base + bj - 1) % LONE_RING].out, x, k, dk,
                             e_0_s);
                    walk_push(P, x, k, dk, e_0_s, pr.ring[(base + bj) % LONE_RING].dl * frac, 0, 0u, rank, 0);
                    Trig T;
                    Gcov G;
                    ZoneFetch Z;
                    zone_fetch(P, x, Z);
                    trig_at(P, x, T);
                    gcov_from_trig(P, T, G);
                    Fluid F;
                    fluid_from(P, x, G, Z, F);
                    fl_ne = F.n_e;
                    x1 = x[1];
                    cur = LONE_STOP; /* the state is the restart state from here on */
                    if (F.n_e > 0.0 && (k[0] > 1.0e5 || k[0] < 0.0 || isnan(k[0]) || isnan(k[1]) || isnan(k[3]))) {
                        /* scatter_super_photon's parent-side check (:1076-1081, :1018-1021) */
                        k[0] = fabs(k[0]);
                        w = 0.0;
                        if (own) pack13(pr.ctl.rs, x, k, dk, e_0_s);
                        ended = done = true;
                        reason = 2;
                        break;
                    }
                    const double nu2 = fluid_nu(k, F);
                    double a_s2 = 0.0, a_a2 = 0.0;
                    if (!(nu2 < 0.0)) radiation_coeffs(P, k, F, nu2, a_s2, a_a2);
                    const double bf2 = bias_func(bias_d, F.theta_e, w);
                    if (F.n_e > 0.0) {
                        /* the child (:1015-1024): on the early worker into its queue, tracked by the
                         * next free pair; else to the overflow pool, tracked by the relaunch */
                        if (own) {
                            if (kids)
                                queue_child_push(C, kids, x, k, rng, n_scatt, cold, F, wc);
                            else
                                push_overflow(C, x, k, rng, n_scatt, cold, F, wc);
                        }
                        ++children;
                    }
                    a_si = a_s2;
                    a_ai = a_a2;
                    bi = bf2;
                    /* the photon goes on from the scattering point: restart the geometry wave there */
                    ++gen;
                    gen_start = base + bj + 1;
                    if (own) {
                        pack13(pr.ctl.rs, x, k, dk, e_0_s);
                        __hip_atomic_store(&pr.ctl.req, ((unsigned long long)gen << 32) | (base + bj + 1),
                                           __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                    /* the end of the step here, and the end of the batch (the rest of it is on the old
                     * geodesic): the batch's lane values are dead on this path */
                    tau_abs += d_tau_abs;
                    tau_scatt += d_tau_scatt;
                    ++n_step; /* :1058-1063 */
                    if (n_step > MAX_N_STEP) {
                        ended = done = true;
                        reason = 3;
                        break;
                    }
                    si = base + bj + 1;
                    if (own) __hip_atomic_store(&pr.ctl.cons, si, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                    break;
                } else {
                    if (d_tau_abs > 100) { /* absorbed */
                        ended = done = true;
                        reason = 2;
                        break;
                    }
                    w *= bcast(l_fac, bj);
                }
                tau_abs += d_tau_abs;
                tau_scatt += d_tau_scatt;
            }
            ++n_step; /* :1058-1063 */
            if (n_step > MAX_N_STEP) {
                ended = done = true;
                reason = 3;
                break;
            }
            si = base + bj + 1;
            if (own) __hip_atomic_store(&pr.ctl.cons, si, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
#ifdef GRM_TIMING
        ti[3] += __builtin_amdgcn_s_memtime() - tb1;
#endif
    }
#ifdef GRM_TIMING
    /* slots 36-39: photons of > 1e5 steps, 40-43: the others */
    if (own)
        for (int r = 0; r < 4; ++r) atomicAdd(C.timing + (steps > 100000 ? 36 : 40) + r, ti[r]);
#endif
    gen_io = gen;
    if (own) {
        /* the photon's state: the end of step cur (its ring slot is not overwritten before this wave
         * consumes the step after it), or the restart state */
        double x[4], k[4], dk[4], e_0_s;
        unpack13(cur == LONE_STOP ? pr.ctl.rs : pr.ring[cur % LONE_RING].out, x, k, dk, e_0_s);
        if (abandoned) {
            const unsigned long long slot = atomicAdd(C.stuck_count, 1ull);
            if (slot < C.stuck_cap) {
                double *r = C.stuck + slot * STUCK_WORDS;
                r[0] = (double)rng.id;
                r[1] = n_step;
                r[2] = r[3] = r[4] = r[7] = 0.0;
                r[5] = w;
                r[6] = e_0_s;
                for (int i = 0; i < 4; ++i) {
                    r[8 + i] = x[i];
                    r[12 + i] = k[i];
                }
            }
            atomicAdd(&C.ctr->n_abandoned, 1ull);
        } else if (ended) {
            /* record_criterion (:1066) when the stop criterion ended it, else the reason's trace */
            if (reason < 0 && x[1] > P.x1_max && n_step <= MAX_N_STEP)
                record_photon(P, C, cold, rng.id, w, x[1], x[2], x[3], tau_abs, tau_scatt, n_scatt, n_step,
                              reinterpret_cast<double *>(C.spec), (int)(sizeof(grm_spectrum_cell) / sizeof(double)));
            else if (C.trace)
                write_trace(C, cold, rng.id, w, x[1], x[2], x[3], tau_abs, tau_scatt, n_scatt, n_step,
                            reason < 0 ? 2 : reason, -1, -1);
        }
        flush_counters(C);
        atomicAdd(&C.ctr->n_steps, steps);
        if (children) atomicAdd(&C.ctr->n_children, children);
        atomicMax(&C.ctr->max_nstep, (unsigned long long)n_step);
        if (n_step > 100000) atomicAdd(&C.ctr->n_long, 1ull);
    }
}

} /* namespace */

#endif /* GRM_LONE_PIPE_H */

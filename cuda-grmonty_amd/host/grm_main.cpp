/*
 * grm_main.cpp -- command-line driver with the reference's flags and run sequence
 * (m-torhan/cuda-grmonty main.cpp:20-53, HARMModel::run_simulation harm_model.cpp:340-414):
 *
 *   grmonty_amd --harm_dump_path=DUMP --spectrum_path=OUT [--photon_n=5000000]
 *               [--mass_unit=4e19] [--verbosity=info] [--device=0] [--seed=123]
 *               [--batch=67108864] [--threads=0] [--host_emit] [--stats_path=OUT.stats]
 *               [--orders_path=OUT.orders] [--trace_cap=N]
 *               [--rebin=N_TH,N_E[,LOG10_E_MIN,LOG10_E_MAX][,unfold] --rebin_path=OUT.grid]
 *
 * read_file -> init -> run_simulation (zone batches emitted and tracked on the GPU; --host_emit:
 * emitted on host threads, batch b+1 overlapping the transport of batch b) -> report_spectrum.
 * --orders_path: the spectrum by scattering order with standard errors (grm_write_spectrum_orders);
 * the run then keeps the per-photon trace, bins it on the GPU after every zone batch
 * (grm_engine_cell_sums_accumulate) and rewinds it.  --trace_cap: trace records per batch (default:
 * TRACE_PER_PHOTON x the batch's emitted photons); a batch that needs more ends the run with an error.
 * --rebin with --rebin_path: the same spectrum on a (theta, E) grid chosen here -- N_TH theta bins per
 * hemisphere (folded about the equator, or with "unfold" 2 N_TH rows pole to pole) and N_E energy bins
 * over the default range (1e-12 upward, 200 x 0.25 in ln E) or over [LOG10_E_MIN, LOG10_E_MAX] --
 * re-binned on the GPU from the same trace (grm_engine_rebin_accumulate, grm_write_spectrum_grid).
 * "Final rate" = created superphotons / wall time of run_simulation, as in the reference.
 */
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/grmonty_amd.h"

namespace {

int g_verbose = 1; /* 0 warn, 1 info, 2 debug */

void info(const char *msg) {
    if (g_verbose >= 1) std::fprintf(stderr, "[info] %s\n", msg);
}

template <typename... A>
__attribute__((format(printf, 1, 0))) void info(const char *fmt, A... a) {
    if (g_verbose >= 1) {
        std::fprintf(stderr, "[info] ");
        std::fprintf(stderr, fmt, a...);
        std::fprintf(stderr, "\n");
    }
}

bool flag(int argc, char **argv, int &i, const char *name, std::string &val) {
    const size_t n = std::strlen(name);
    const char *a = argv[i];
    if (std::strncmp(a, "--", 2) != 0 || std::strncmp(a + 2, name, n) != 0) return false;
    if (a[2 + n] == '=') {
        val = a + 3 + n;
        return true;
    }
    if (a[2 + n] == 0 && i + 1 < argc) {
        val = argv[++i];
        return true;
    }
    return false;
}

/* Default trace capacity of a zone batch, in records per emitted photon: twice the largest
 * tracked / primaries ratio measured -- 4.39 at 64^2, photon_n = 2000; 2.54 at 192^2, 1e5; 2.23 at
 * 192^2, 1e6 (profiles/cell_sums_measure.json).  The ratio grows as photon_n
 * shrinks (the adaptive bias scatters more per photon) and in the first batch of a job cut into
 * many: such a run says how many records it needed and wants --trace_cap. */
constexpr double TRACE_PER_PHOTON = 8.8;

/* --rebin=N_TH,N_E[,LOG10_E_MIN,LOG10_E_MAX][,unfold]; false for a malformed list */
bool parse_rebin(const std::string &v, grm_bin_grid &g) {
    std::vector<std::string> f;
    size_t a = 0;
    for (;;) {
        const size_t b = v.find(',', a);
        f.push_back(v.substr(a, b == std::string::npos ? b : b - a));
        if (b == std::string::npos) break;
        a = b + 1;
    }
    grm_bin_grid_default(&g);
    if (!f.empty() && f.back() == "unfold") {
        g.fold = 0;
        f.pop_back();
    }
    if (f.size() != 2 && f.size() != 4) return false;
    double x[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t i = 0; i < f.size(); ++i) {
        char *end = nullptr;
        x[i] = std::strtod(f[i].c_str(), &end);
        if (f[i].empty() || *end || !std::isfinite(x[i])) return false;
    }
    if (x[0] < 1.0 || x[0] > 1e9 || x[0] != std::floor(x[0]) || x[1] < 1.0 || x[1] > 1e9 || x[1] != std::floor(x[1]))
        return false;
    /* the range edge to edge: the default grid's, or the one given; bin 0 is centred half a bin in */
    double lo = g.l_e_0 - 0.5 * g.d_l_e, span = g.d_l_e * g.n_e;
    if (f.size() == 4) {
        if (!(x[3] > x[2])) return false;
        const double ln10 = std::log(10.0);
        lo = x[2] * ln10;
        span = (x[3] - x[2]) * ln10;
    }
    g.n_th = (int32_t)x[0];
    g.n_e = (int32_t)x[1];
    g.d_l_e = span / g.n_e;
    g.l_e_0 = lo + 0.5 * g.d_l_e;
    return true;
}

} /* namespace */

int main(int argc, char **argv) {
    long long photon_n = 5000000; /* main.cpp:20 */
    double mass_unit = 4e19;      /* main.cpp:21 */
    std::string dump, spec_path, stats_path, orders_path, rebin_arg, rebin_path, verbosity = "info";
    int device = 0, threads = 0;
    unsigned long long seed = 123; /* consts.hpp:14 */
    long long batch = 1ll << 26; /* photons per zone batch (8.6 GB of emitted photons) */
    bool host_emit = false;
    long long trace_cap = 0; /* --trace_cap; 0 = TRACE_PER_PHOTON x the batch */
    for (int i = 1; i < argc; ++i) {
        std::string v;
        if (flag(argc, argv, i, "photon_n", v)) photon_n = std::atoll(v.c_str());
        else if (flag(argc, argv, i, "mass_unit", v)) mass_unit = std::atof(v.c_str());
        else if (flag(argc, argv, i, "harm_dump_path", v)) dump = v;
        else if (flag(argc, argv, i, "spectrum_path", v)) spec_path = v;
        else if (flag(argc, argv, i, "verbosity", v)) verbosity = v;
        else if (flag(argc, argv, i, "stats_path", v)) stats_path = v;
        else if (flag(argc, argv, i, "orders_path", v)) orders_path = v;
        else if (flag(argc, argv, i, "rebin_path", v)) rebin_path = v;
        else if (flag(argc, argv, i, "rebin", v)) rebin_arg = v;
        else if (flag(argc, argv, i, "trace_cap", v)) trace_cap = std::atoll(v.c_str());
        else if (flag(argc, argv, i, "device", v)) device = std::atoi(v.c_str());
        else if (flag(argc, argv, i, "seed", v)) seed = std::strtoull(v.c_str(), nullptr, 10);
        else if (flag(argc, argv, i, "batch", v)) batch = std::atoll(v.c_str());
        else if (flag(argc, argv, i, "threads", v)) threads = std::atoi(v.c_str());
        else if (std::strcmp(argv[i], "--host_emit") == 0) host_emit = true;
        else {
            std::fprintf(stderr, "unknown argument %s\n", argv[i]);
            return 2;
        }
    }
    const bool rebin = !rebin_arg.empty() || !rebin_path.empty();
    grm_bin_grid grid;
    grm_bin_grid_default(&grid);
    if (rebin) {
        const char *bad = nullptr;
        if (rebin_arg.empty() || rebin_path.empty()) bad = "--rebin and --rebin_path go together";
        else if (!parse_rebin(rebin_arg, grid)) bad = "malformed --rebin list";
        else bad = grm_bin_grid_check(&grid);
        if (bad) {
            std::fprintf(stderr, "%s\nusage: --rebin=N_TH,N_E[,LOG10_E_MIN,LOG10_E_MAX][,unfold] --rebin_path=FILE\n", bad);
            return 2;
        }
    }
    g_verbose = verbosity == "debug" || verbosity == "trace" ? 2 : (verbosity == "warn" || verbosity == "error" ? 0 : 1);
    info("Parameters:");
    info("\tphoton_n: %lld", photon_n);
    info("\tmass_unit: %g", mass_unit);
    info("\tharm_dump_path: %s", dump.c_str());
    info("\tspectrum_path: %s", spec_path.c_str());

    grm_model *m = nullptr;
    info("Reading file %s", dump.c_str());
    if (grm_model_load(dump.c_str(), (int)photon_n, mass_unit, &m)) {
        std::fprintf(stderr, "[error] %s\n", grm_model_last_error());
        return 1;
    }
    info("Initializing HARM model (tables)");
    if (grm_model_init(m, threads)) {
        std::fprintf(stderr, "[error] %s\n", grm_model_last_error());
        return 1;
    }
    grm_engine *e = nullptr;
    if (grm_engine_create_from_model(m, device, &e)) {
        std::fprintf(stderr, "[error] engine: %s\n", e ? grm_engine_last_error(e) : grm_model_last_error());
        grm_engine_destroy(e);
        return 1;
    }
    grm_engine_set_option(e, GRM_OPT_SEED, (int64_t)seed);

    /* run_simulation: zone-range batches (bounded HBM for the emitted photons), each emitted on the
     * GPU from the zone table and tracked there; --host_emit keeps the host emitter (batch b+1
     * emitted on host threads while batch b is tracked) */
    if (!host_emit && grm_engine_emit_setup_from_model(e, m)) {
        std::fprintf(stderr, "[error] emission setup: %s %s\n", grm_engine_last_error(e), grm_model_last_error());
        return 1;
    }
    info("Starting main loop");
    const auto t0 = std::chrono::steady_clock::now();
    grm_header h;
    grm_model_header(m, &h);
    const long long nzones = (long long)h.n[0] * h.n[1];
    std::vector<double> zw((size_t)nzones);
    grm_model_zone_weights(m, zw.data());
    /* cut the zone walk into ranges of ~batch expected photons */
    std::vector<long long> cuts{0};
    double acc = 0.0;
    for (long long z = 0; z < nzones; ++z) {
        acc += zw[(size_t)z];
        if (acc >= (double)batch) {
            cuts.push_back(z + 1);
            acc = 0.0;
        }
    }
    if (cuts.back() != nzones) cuts.push_back(nzones);
    unsigned long long created = 0;
    std::vector<grm_init_photon> cur, nxt;
    auto emit = [&](size_t b, std::vector<grm_init_photon> &buf) {
        const int64_t n = grm_model_emit(m, seed, cuts[b], cuts[b + 1], nullptr, 0, threads);
        buf.resize((size_t)std::max<int64_t>(n, 0));
        if (n > 0) grm_model_emit(m, seed, cuts[b], cuts[b + 1], buf.data(), buf.size(), threads);
    };
    /* --orders_path / --rebin: size the trace for the batch about to be tracked, and bin + rewind it after */
    const bool orders = !orders_path.empty();
    const bool traced = orders || rebin;
    if (rebin && grm_engine_rebin_setup(e, &grid)) {
        std::fprintf(stderr, "[error] rebin: %s\n", grm_engine_last_error(e));
        return 1;
    }
    long long cap_now = 0;
    auto trace_for = [&](size_t n) {
        const long long want = trace_cap > 0 ? trace_cap : (long long)(TRACE_PER_PHOTON * (double)n) + 1024;
        if (want <= cap_now) return 0;
        cap_now = want;
        return grm_engine_set_option(e, GRM_OPT_TRACE_CAP, want);
    };
    auto bin_trace = [&]() {
        uint64_t nb = 0;
        double ms = 0.0;
        if (orders) {
            if (grm_engine_cell_sums_accumulate(e, &nb, &ms)) return -1;
            info("Binned %llu trace records by scattering order in %.3f ms", (unsigned long long)nb, ms);
        }
        if (rebin) {
            if (grm_engine_rebin_accumulate(e, &nb, &ms)) return -1;
            info("Re-binned %llu trace records on the %d x %d grid in %.3f ms", (unsigned long long)nb,
                 grid.fold ? grid.n_th : 2 * grid.n_th, grid.n_e, ms);
        }
        return grm_engine_trace_rewind(e) ? -1 : 0;
    };
    if (host_emit) emit(0, cur);
    for (size_t b = 0; b + 1 < cuts.size(); ++b) {
        if (host_emit) {
            std::thread prod;
            if (b + 2 < cuts.size()) prod = std::thread(emit, b + 1, std::ref(nxt));
            if (traced && !cur.empty() && trace_for(cur.size())) {
                std::fprintf(stderr, "[error] trace: %s\n", grm_engine_last_error(e));
                if (prod.joinable()) prod.join();
                return 1;
            }
            if (!cur.empty() && grm_engine_track(e, cur.data(), cur.size())) {
                std::fprintf(stderr, "[error] transport: %s\n", grm_engine_last_error(e));
                if (prod.joinable()) prod.join();
                return 1;
            }
            created += cur.size();
            if (prod.joinable()) prod.join();
            std::swap(cur, nxt);
            nxt.clear();
        } else {
            grm_init_photon *d_ph = nullptr;
            uint64_t n = 0;
            if (grm_engine_emit(e, seed, cuts[b], cuts[b + 1], &d_ph, &n) || (traced && n && trace_for(n)) ||
                (n && grm_engine_track_device(e, d_ph, n))) {
                std::fprintf(stderr, "[error] emission/transport: %s\n", grm_engine_last_error(e));
                return 1;
            }
            created += n;
        }
        if (traced && cap_now && bin_trace()) {
            std::fprintf(stderr, "[error] trace binning: %s\n", grm_engine_last_error(e));
            return 1;
        }
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        info("Rate %.2f ph/s, zone batch %zu/%zu", created / el, b + 1, cuts.size() - 1);
    }
    std::vector<grm_spectrum_cell> spec(GRM_N_TH_BINS * GRM_N_E_BINS);
    uint64_t n_rec = 0, n_scatt = 0;
    double max_tau = 0.0;
    if (grm_engine_finish(e, spec.data(), &n_rec, &n_scatt, &max_tau)) {
        std::fprintf(stderr, "[error] spectrum readback: %s\n", grm_engine_last_error(e));
        return 1;
    }
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    info("Final rate %.2f ph/s", created / el);
    info("Super photons:");
    info("\tcreated: %llu", created);
    info("\tscattered: %llu", (unsigned long long)n_scatt);
    info("\trecorded: %llu", (unsigned long long)n_rec);
    grm_stats st;
    if (grm_engine_stats(e, &st)) {
        std::fprintf(stderr, "[error] engine stats: %s\n", grm_engine_last_error(e));
        return 1;
    }
    info("\ttransport steps: %llu (%.3g steps/s in kernel)", (unsigned long long)st.n_steps,
         st.n_steps / (st.kernel_ms * 1e-3 + 1e-30));
    if (!spec_path.empty()) {
        info("Writing spectrum to file %s", spec_path.c_str());
        double lm[2];
        if (grm_write_spectrum(m, spec.data(), spec_path.c_str(), lm)) {
            std::fprintf(stderr, "[error] %s\n", grm_model_last_error());
            return 1;
        }
        info("\tlumosity: %g", lm[0]);
        info("\tmax_tau_scatt: %g", lm[1]);
    }
    if (!stats_path.empty() && grm_write_spectrum_stats(m, spec.data(), stats_path.c_str())) {
        std::fprintf(stderr, "[error] %s\n", grm_model_last_error());
        return 1;
    }
    if (orders) {
        std::vector<double> sums((size_t)GRM_N_ORDERS * GRM_N_TH_BINS * GRM_N_E_BINS * GRM_N_CELL_SUMS);
        uint64_t skipped = 0;
        if (grm_engine_cell_sums_read(e, sums.data(), &skipped)) {
            std::fprintf(stderr, "[error] cell sums: %s\n", grm_engine_last_error(e));
            return 1;
        }
        if (skipped) std::fprintf(stderr, "[warn] cell sums: %llu recorded photons outside the grid skipped\n",
                                  (unsigned long long)skipped);
        info("Writing spectrum by scattering order to file %s", orders_path.c_str());
        if (grm_write_spectrum_orders(m, sums.data(), orders_path.c_str())) {
            std::fprintf(stderr, "[error] %s\n", grm_model_last_error());
            return 1;
        }
    }
    if (rebin) {
        std::vector<double> sums(grm_bin_grid_doubles(&grid));
        uint64_t out_of_grid = 0;
        if (grm_engine_rebin_read(e, sums.data(), sums.size(), &out_of_grid)) {
            std::fprintf(stderr, "[error] rebin: %s\n", grm_engine_last_error(e));
            return 1;
        }
        if (out_of_grid) info("Rebin: %llu escaped superphotons fell outside the grid", (unsigned long long)out_of_grid);
        info("Writing the re-binned spectrum to file %s", rebin_path.c_str());
        if (grm_write_spectrum_grid(m, &grid, sums.data(), rebin_path.c_str())) {
            std::fprintf(stderr, "[error] %s\n", grm_model_last_error());
            return 1;
        }
    }
    grm_engine_destroy(e);
    grm_model_free(m);
    return 0;
}

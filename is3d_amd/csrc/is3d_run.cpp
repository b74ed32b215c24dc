// is3d_run.cpp -- IS3D::run_particlization (/root/reference/src/cpp/iS3D.cpp:74-192) behind the C ABI: the driver layer
// shared by the command line tool (is3d_main.cpp) and the embedding class (include/iS3D_amd.hpp).
//
// Runs in a directory laid out like the reference's run directory; it reads the same hard-coded
// CWD-relative files IS3D::run_particlization reads (/root/reference/src/cpp/iS3D.cpp:74-192):
//   iS3D_parameters.dat, input/surface.dat, PDG/pdg-urqmd_v3.3+.dat | PDG/pdg_smash.dat,
//   PDG/chosen_particles.dat, deltaf_coefficients/vh/<eos>/{c0,c2,F,betabulk,betapi}.dat,
//   tables/pT_gauss_legendre_table.dat, tables/phi_gauss_legendre_table.dat,
//   tables/y_trapezoid_table_21pt.dat, tables/eta/eta_trapezoid_table_241pt.dat
// and writes what EmissionFunctionArray::calculate_spectra writes for operation = 1
// (emissionfunction.cpp:1678-1686) into results/ (which must exist, README.md:34) plus
// average_thermodynamic_quantities.dat (readindata.cpp:464-466).
// operation = 2 (particle sampler; df_mode 1-4, fast in {0, 1}, include_baryon = 1 with df_mode 1-3) writes
// results/particle_list_osc.dat (write_particle_list_OSC, emissionfunction.cpp:863-901) and results/dN_dy_*.dat is skipped.
// mode = 2 (anisotropic hydro, P_L matching; BASELINE config 5): operation = 1 (or 0, below) with df_mode = 4 -- the combination for which the
// reference allocates the per-cell c0..c4 (emissionfunction.cpp:1397-1418) and the CUDA tree loads the VAH tables
// (src/cuda/deltafReader.cu:74-81) -- reads input/surface.dat with read_surf_VAH_PLMatch and deltaf_coefficients/vah/c{0..4}_vah1.dat,
// runs what the commented-out call site would (emissionfunction.cpp:1650-1654) and writes the same three result files.  With a device list
// that was spelled out (the list of is3d_run_particlization_on, --devices, IS3D_DEVICES) the cells are sharded over it
// (is3d_smooth_spectra_vah_multi, the run's reduce); without one, or with a bare device count, the first device computes alone -- the rule of
// mode 5 below -- so that a mode-2 run does not depend on how many devices a machine shows.
// operation = 0 (smooth spacetime distributions, calculate_dN_dX; emissionfunction.cpp:1510-1516): mode in {0, 1, 4, 5, 6, 7}, df_mode in
// {1, 2}, include_baryon in {0, 1}, dimension 2 or 3, the per-cell stage sharded over the run's device list and one bin stage on its first
// device (is3d_spacetime_distributions_multi); reads tau_min ... r_bins (:216-222), writes
// results/spacetime_distribution/{dN_taudtaudy, dN_twopirdrdy, dN_twopitaurdtaudrdy}_<id>.dat and dN_dydeta_<id>_<n>pt.dat (the directory must
// exist) and prints one "dN_dy = %lf" line per species; no momentum-spectra file (those are written for operation = 1 only, :1678).  df_mode 3 / 4
// (calculate_dN_dX_feqmod) with those modes is refused before anything is written.  mode = 2 with df_mode = 4 runs the anisotropic-hydro form
// (is3d_spacetime_distributions_vah; the reference has none): the same parameters, files and lines from the mode-2 surface and the
// deltaf_coefficients/vah tables, on the first device of the run's list.
// do_resonance_decays = 1 (optional key): with operation = 1 and hrg_eos = 1 or 2, the thermal files are written as without it, then the
// feed-down (is3d_resonance_decays) runs on the spectrum on the first device of the run's list and results/dN_pTdpTdphidy_resonance_decays.dat
// and dN_dpTdphidy_resonance_decays.dat are appended (emissionfunction.cpp:1689-1698); the embedding result keeps the thermal spectrum.
// Operations 0 and 2 and hrg_eos = 3 (no decay data) refuse the key.
// decay_sampled_hadrons = 1 (optional key, default 0): with operation = 2, test_sampler = 0 and hrg_eos = 1 or 2 (either sampler family)
// results/particle_list_osc.dat is written as without it, then the list is decayed to stable particles by Monte Carlo (is3d_decay_particles:
// the sampler's seed, lifetime = 0, the first device of the run's list) and results/particle_list_osc_decayed.dat written with the decay
// table's ids; one line of stats is printed and the embedding result keeps the thermal list.  Every other combination refuses the key before
// anything is written (do_resonance_decays = 1 stays refused with operation = 2: it names the smooth feed-down).
// deltaf_dir = DIR (optional key, absent by default): the coefficient tables are read from DIR instead of deltaf_coefficients/vh/<eos>/ --
// a directory written by `iS3D_amd --generate-df DIR` (is3d_main.cpp) for an edited list or another (T, mu_B) grid.
// test_sampler_on_device = 1 (optional key, default 0): with operation = 2 and test_sampler = 1 the hadrons are sampled ONCE and binned per event
// batch on the device (is3d_sample_binned_multi), never held as a list; the same files are written from the integer histograms
// (is3d_write_sampler_tests_binned; vn/ to the fixed point) and the same lines printed, plus ms_bin.  test_sampler = 0, other operations and
// the embedding entry (which returns the list) refuse the key.
// test_sampler_fused = 1 (optional key, default 0): with operation = 2, test_sampler = 1 and a viscous mode every hadron is binned where it is
// sampled (is3d_sample_fused; is3d_sample_fused_multi over a device list that was spelled out) -- one pass per event batch, no list and no
// particle workspace.  The files of the test_sampler_on_device = 1 run are written (is3d_write_sampler_tests_binned, the same mean_yield) and
// its lines printed, plus ms_bin; test_sampler_on_device may be 0 or 1 beside it, and oversample = 1 works.  Other operations,
// test_sampler = 0, mode = 2 (it has vah_sampler_on_device) and the embedding entry refuse the key before anything is written.
// vah_oversample = 1 (optional key, default 0): with mode = 2, operation = 2, df_mode = 4 and vah_sampler = 1 the anisotropic-hydro mean yield
// (is3d_total_yield_vah: first device of the run's list, the file's y_cut, the deltaf_coefficients/vah tables, the sampler's Gauss-Laguerre file)
// is printed as the viscous path prints its own and sizes the run, Nevents = is3d_oversample_events(min_num_hadrons, yield, max_num_samples); a
// yield <= 0 (the linear delta-f of a large residual bulk pressure) stops the run before anything is written.  Every other combination refuses
// the key; oversample = 1 stays refused with mode = 2.
// vah_sampler_on_device = 1 (optional key, default 0): with mode = 2, operation = 2, df_mode = 4, vah_sampler = 1 and test_sampler = 1 the
// anisotropic-hydro sampler's hadrons are sampled ONCE and binned where they are sampled (is3d_sample_binned_vah; is3d_sample_binned_vah_multi over
// a device list that was spelled out), never held as a list: the files of the host-binned run are written from the integer histograms
// (is3d_write_sampler_tests_binned, with the same mean_yield; vn/ to the fixed point), the same lines printed plus ms_bin, no particle list.  Works
// together with vah_oversample = 1.  Every other combination and the embedding entry (which returns the list) refuse the key before anything is
// written; test_sampler_on_device = 1 stays refused with mode = 2 (it names the viscous route).
// mode = 5: every run, whatever its operation, ends with the spin polarization from the surface's thermal vorticity (calculate_spin_polzn,
// emissionfunction.cpp:1675) and appends results/St.dat, Sx.dat, Sy.dat, Sn.dat (write_polzn_vector_toFile, :1701), with T from the averages
// file just written or T_switch when set_FO_temperature = 1; the embedding entry has no vorticity and says so.  With a device list that was
// spelled out (the list of is3d_run_particlization_on, --devices, IS3D_DEVICES) the cells are sharded over it (is3d_spin_polarization_multi:
// one shard per entry, the class sums added in shard order on the first device); without one, or with a bare device count, the first device
// computes alone, so that the S files do not depend on how many devices a machine shows.
// Scope: operation in {0, 1, 2}, mode in {0, 1, 4, 5, 6, 7}, df_mode in {1, 2, 3} with include_baryon in {0, 1}, df_mode 4
// (modified equilibrium; also reads tables/gla_roots_weights_32_points.txt, deta_min, mass_pion0 and the surface
// averages it has just written, as the reference does) with include_baryon = 0.  Anything else is refused
// with a message instead of silently doing something different from the reference.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <fstream>
#include <iomanip>
#include <string>
#include <thread>
#include <vector>

#include <cstdarg>

#include "../../include/is3d_amd.h"
#include "errors.h"

static double now_s()
{
    using namespace std::chrono;
    return duration<double>(steady_clock::now().time_since_epoch()).count();
}

// print like the reference does before exit(-1), but return a code and keep the text for is3d_last_error()
static int die(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static int die(const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    fprintf(stderr, "iS3D-amd: %s\n", buf);
    return is3d::set_error(IS3D_EINVAL, "%s", buf);
}
#define DIE(...) return die(__VA_ARGS__)

static int get_param(const char *name, double *v, bool required = true)
{
    int rc = is3d_param_get("iS3D_parameters.dat", name, v);
    if (rc && required) fprintf(stderr, "iS3D-amd: %s\n", is3d_last_error());
    return rc;
}

// an optional key whose value is text (deltaf_dir): the line rules of is3d_param_get -- '#' starts a comment, blanks and tabs are removed, the
// name is lower-cased, later lines overwrite -- with the right-hand side taken verbatim.  False when the key is absent.
static bool get_param_text(const char *name, std::string &value)
{
    std::ifstream f("iS3D_parameters.dat");
    bool found = false;
    for (std::string line; std::getline(f, line);) {
        line = line.substr(0, line.find('#'));
        line.erase(std::remove_if(line.begin(), line.end(), [](char c) { return c == ' ' || c == '\t' || c == '\r'; }), line.end());
        const size_t eq = line.find('=');
        if (eq == std::string::npos) continue;
        std::string lhs = line.substr(0, eq);
        for (char &c : lhs) c = (char)tolower((unsigned char)c);
        if (lhs == name) { value = line.substr(eq + 1); found = true; }
    }
    return found;
}

static int read_table(const char *path, std::vector<double> &col1, std::vector<double> &col2)
{
    int64_t rows;
    int32_t cols;
    if (is3d_table_read(path, &rows, &cols, nullptr, 0)) return 1;
    std::vector<double> d((size_t)rows * cols);
    if (is3d_table_read(path, &rows, &cols, d.data(), (int64_t)d.size())) return 1;
    col1.resize(rows);
    col2.assign(rows, 0.0);
    for (int64_t r = 0; r < rows; r++) {
        col1[r] = d[r * cols];
        if (cols > 1) col2[r] = d[r * cols + 1];
    }
    return 0;
}

// surface-volume weighted averages of T, E, P, muB, nB as the readers accumulate them (readindata.cpp:422-466)
static void surface_averages(const is3d_cells *c, double avg[5])
{
    double num[5] = {0, 0, 0, 0, 0}, den = 0.0;
    for (int64_t i = 0; i < c->n_cells; i++) {
        const double tau = c->tau[i], ux = c->ux[i], uy = c->uy[i], un = c->un[i];
        const double ut = std::sqrt(1.0 + ux * ux + uy * uy + tau * tau * un * un);
        const double dat = c->dat[i], dax = c->dax[i], day = c->day[i], dan = c->dan[i];
        const double uds = ut * dat + ux * dax + uy * day + un * dan;
        const double dsds = dat * dat - dax * dax - day * day - dan * dan / (tau * tau);
        const double w = std::fabs(uds) + std::sqrt(std::fabs(uds * uds - dsds));
        num[0] += c->T[i] * w; num[1] += c->E[i] * w; num[2] += c->P[i] * w;
        if (c->muB) num[3] += c->muB[i] * w;
        if (c->nB) num[4] += c->nB[i] * w;
        den += w;
    }
    for (int k = 0; k < 5; k++) avg[k] = den > 0.0 ? num[k] / den : 0.0;
}

// devices of the run: an explicit list, else the environment (IS3D_DEVICES = "0,2,3" | "all"; IS3D_REDUCE = "ordered" | "rccl"),
// else every visible device
struct RunDevices {
    std::vector<int32_t> list;   // empty: all visible
    int32_t reduce = IS3D_REDUCE_ORDERED;
    bool named = false;          // the list was spelled out (the entry's list, --devices, IS3D_DEVICES), not a bare count of ordinals
};

static int parse_run_devices(const int32_t *devices, int32_t n_devices, int32_t reduce, RunDevices &rd)
{
    rd.reduce = reduce;
    if (devices && n_devices > 0) {
        rd.list.assign(devices, devices + n_devices);
        rd.named = true;
        return IS3D_OK;
    }
    if (n_devices > 0) {
        for (int32_t i = 0; i < n_devices; i++) rd.list.push_back(i);
        return IS3D_OK;
    }
    if (const char *e = getenv("IS3D_REDUCE")) {
        if (!strcmp(e, "rccl")) rd.reduce = IS3D_REDUCE_RCCL;
        else if (!strcmp(e, "ordered")) rd.reduce = IS3D_REDUCE_ORDERED;
        else return die("IS3D_REDUCE = %s: ordered | rccl", e);
    }
    if (const char *e = getenv("IS3D_DEVICES")) {
        if (strcmp(e, "all") && *e) {
            const char *p = e;
            while (*p) {
                char *end = nullptr;
                long v = strtol(p, &end, 10);
                if (end == p || v < 0) return die("IS3D_DEVICES = %s: a comma separated list of HIP device ordinals, or all", e);
                rd.list.push_back((int32_t)v);
                p = (*end == ',') ? end + 1 : end;
                if (*end && *end != ',') return die("IS3D_DEVICES = %s: a comma separated list of HIP device ordinals, or all", e);
            }
            rd.named = !rd.list.empty();
        }
    }
    return IS3D_OK;
}

static int run_impl(const is3d_cells *mem, const double *mem_x, const double *mem_y, int variant, const RunDevices &rd, is3d_run_result *res)
{
    printf("iS3D-amd: MI355X-native smooth Cooper-Frye spectra (%s)\n", is3d_version());
    double v;
    int operation, mode, hrg_eos, dimension, df_mode, include_baryon, include_bulk, include_shear, include_diff, regulate, outflow;
#define GET(var, name)                           \
    if (get_param(name, &v)) return IS3D_EINVAL; \
    var = (int)v;
    GET(operation, "operation");
    GET(mode, "mode");
    GET(hrg_eos, "hrg_eos");
    GET(dimension, "dimension");
    GET(df_mode, "df_mode");
    GET(include_baryon, "include_baryon");
    GET(include_bulk, "include_bulk_deltaf");
    GET(include_shear, "include_shear_deltaf");
    GET(include_diff, "include_baryondiff_deltaf");
    GET(regulate, "regulate_deltaf");
    GET(outflow, "outflow");
#undef GET
    if (operation != 0 && operation != 1 && operation != 2)
        DIE("operation = %d: operation = 0 (smooth spacetime distributions), 1 (smooth momentum spectra) and 2 (particle sampler) are on this path", operation);
    if (operation == 0) {
        // mode = 2 (anisotropic hydro; df_mode = 4 is checked below) has its own routine, is3d_spacetime_distributions_vah
        if ((df_mode == 3 || df_mode == 4) && !(!mem && mode == 2))
            DIE("operation = 0 with df_mode = %d (calculate_dN_dX_feqmod) is not run by this driver yet (the library entry is3d_spacetime_distributions_feqmod has it): set df_mode = 1 or 2", df_mode);
        if (mem && (!mem_x || !mem_y)) DIE("operation = 0 needs the cells' x and y positions (NULL given)");
    }
    bool do_decays = false;
    {
        double decays = 0.0;   // optional key here; the reference runs do_resonance_decays() after the spectra (emissionfunction.cpp:1689-1698)
        if (get_param("do_resonance_decays", &decays, false) == IS3D_OK && (int)decays) {
            if (operation != 1)
                DIE("do_resonance_decays = 1 with operation = %d: the feed-down follows the momentum spectra (operation = 1) only; set do_resonance_decays = 0", operation);
            if (hrg_eos == 3)
                DIE("do_resonance_decays = 1 with hrg_eos = 3: PDG/pdg_box.dat carries no decay data (smash box: no decay info, iS3D_parameters.dat); use hrg_eos = 1 or 2");
            do_decays = true;
        }
    }
    // optional key decay_sampled_hadrons = 1: the sampled list decayed to stable particles on the device (is3d_decay_particles)
    bool decay_sampled = false;
    {
        double key = 0.0, test_sampler = 0.0;
        if (get_param("decay_sampled_hadrons", &key, false) == IS3D_OK && (int)key) {
            if (operation != 2)
                DIE("decay_sampled_hadrons = 1 with operation = %d: it decays the sampler's particle list (operation = 2); set decay_sampled_hadrons = 0", operation);
            if (hrg_eos != 1 && hrg_eos != 2)
                DIE("decay_sampled_hadrons = 1 with hrg_eos = %d: PDG/pdg_box.dat carries no decay data (smash box: no decay info, iS3D_parameters.dat); use hrg_eos = 1 or 2", hrg_eos);
            if (get_param("test_sampler", &test_sampler)) return IS3D_EINVAL;
            if ((int)test_sampler)
                DIE("decay_sampled_hadrons = 1 with test_sampler = 1: that run bins the thermal hadrons and writes no particle list to decay; set decay_sampled_hadrons = 0");
            decay_sampled = true;
        }
    }
    bool bin_on_device = false;
    {
        double on_device = 0.0, test_sampler = 0.0;   // optional key: the test_sampler = 1 distributions binned on the device, no particle list
        if (get_param("test_sampler_on_device", &on_device, false) == IS3D_OK && (int)on_device) {
            if (operation != 2)
                DIE("test_sampler_on_device = 1 with operation = %d: it bins the sampler's hadrons (operation = 2); set test_sampler_on_device = 0", operation);
            if (get_param("test_sampler", &test_sampler)) return IS3D_EINVAL;
            if (!(int)test_sampler)
                DIE("test_sampler_on_device = 1 with test_sampler = 0: the particle list is the output of that run and is not kept on this path; set test_sampler_on_device = 0");
            if (res)
                DIE("test_sampler_on_device = 1: the embedding entry returns the particle list, which this path never holds; set test_sampler_on_device = 0");
            bin_on_device = true;
        }
    }
    const bool vah = !mem && mode == 2;
    // optional key test_sampler_fused = 1: the viscous sampler's hadrons binned where they are sampled (is3d_sample_fused), no particle list
    bool bin_fused = false;
    {
        double key = 0.0, test_sampler = 0.0;
        if (get_param("test_sampler_fused", &key, false) == IS3D_OK && (int)key) {
            if (operation != 2)
                DIE("test_sampler_fused = 1 with operation = %d: it bins the sampler's hadrons (operation = 2); set test_sampler_fused = 0", operation);
            if (get_param("test_sampler", &test_sampler)) return IS3D_EINVAL;
            if (!(int)test_sampler)
                DIE("test_sampler_fused = 1 with test_sampler = 0: the particle list is the output of that run and is never held on this path; set test_sampler_fused = 0");
            if (vah)
                DIE("test_sampler_fused = 1 with mode = 2: it names the viscous-hydro sampler; the anisotropic-hydro one has vah_sampler_on_device; set test_sampler_fused = 0");
            if (res)
                DIE("test_sampler_fused = 1: the embedding entry returns the particle list, which this path never holds; set test_sampler_fused = 0");
            bin_fused = true;
        }
    }
    // optional key vah_oversample = 1: the anisotropic-hydro mean yield (is3d_total_yield_vah) sizes the run of this library's own VAH sampler
    bool vah_oversample = false;
    {
        double key = 0.0, sampler = 0.0;
        if (get_param("vah_oversample", &key, false) == IS3D_OK && (int)key) {
            const bool own_sampler = get_param("vah_sampler", &sampler, false) == IS3D_OK && (int)sampler;
            if (!(vah && operation == 2 && df_mode == 4 && own_sampler))
                DIE("vah_oversample = 1 with mode = %d, operation = %d, df_mode = %d, vah_sampler = %d: the anisotropic-hydro mean yield sizes this library's own "
                    "anisotropic-hydro sampler only (mode = 2, operation = 2, df_mode = 4, vah_sampler = 1); set vah_oversample = 0", mode, operation, df_mode,
                    (int)own_sampler);
            vah_oversample = true;
        }
    }
    // optional key vah_sampler_on_device = 1: the VAH sampler's hadrons binned where they are sampled (is3d_sample_binned_vah), no particle list
    bool vah_bin_on_device = false;
    {
        double key = 0.0, sampler = 0.0, test_sampler = 0.0;
        if (get_param("vah_sampler_on_device", &key, false) == IS3D_OK && (int)key) {
            const bool own_sampler = get_param("vah_sampler", &sampler, false) == IS3D_OK && (int)sampler;
            const bool tests = get_param("test_sampler", &test_sampler, false) == IS3D_OK && (int)test_sampler;
            if (!(vah && operation == 2 && df_mode == 4 && own_sampler && tests))
                DIE("vah_sampler_on_device = 1 with mode = %d, operation = %d, df_mode = %d, vah_sampler = %d, test_sampler = %d: it bins the hadrons of this "
                    "library's own anisotropic-hydro sampler on the device and keeps no particle list (mode = 2, operation = 2, df_mode = 4, vah_sampler = 1, "
                    "test_sampler = 1; the viscous-hydro route has test_sampler_on_device); set vah_sampler_on_device = 0", mode, operation, df_mode,
                    (int)own_sampler, (int)tests);
            if (res)
                DIE("vah_sampler_on_device = 1: the embedding entry returns the particle list, which this path never holds; set vah_sampler_on_device = 0");
            vah_bin_on_device = true;
        }
    }
    if (vah) {
        if (operation == 2) {
            // optional key vah_sampler = 1: this library's own VAH sampler (is3d_sample_particles_vah; the reference has none)
            double vah_sampler = 0.0, oversample = 0.0;
            if (!(get_param("vah_sampler", &vah_sampler, false) == IS3D_OK && (int)vah_sampler))
                DIE("mode = 2 (anisotropic hydro): operation = 0 or 1; the reference's VAH sampler is an empty stub (emissionfunction_sampling_kernels.cpp:1231-1239); "
                    "set vah_sampler = 1 for this library's own anisotropic-hydro sampler (is3d_sample_particles_vah)");
            if (bin_on_device)
                DIE("test_sampler_on_device = 1 with mode = 2: the anisotropic-hydro sampler's hadrons are binned on the host (test_sampler = 1); set test_sampler_on_device = 0");
            if (get_param("oversample", &oversample)) return IS3D_EINVAL;
            if ((int)oversample)
                DIE("oversample = 1 with mode = 2: the mean yield that sizes an oversampled run (calculate_total_yield) is viscous-hydro only; set oversample = 0 "
                    "(max_num_samples events are sampled), and vah_oversample = 1 for the anisotropic-hydro mean yield (is3d_total_yield_vah) to size the run");
        }
        if (df_mode != 4) DIE("mode = 2 (anisotropic hydro) needs df_mode = 4: the per-cell 14-moment coefficients c0..c4 exist for that combination only (emissionfunction.cpp:1410-1418)");
    }
    if (!mem && !vah && mode != 0 && mode != 1 && mode != 4 && mode != 5 && mode != 6 && mode != 7)
        DIE("mode = %d: the smooth path reads the viscous-hydro surface formats 0, 1, 4, 5, 6, 7 and the anisotropic-hydro format 2 (3 = VAH P_L, P_T matching has no kernel in the reference: emissionfunction.cpp:1328-1681)", mode);
    if (df_mode < 1 || df_mode > 4) DIE("df_mode = %d: 1 (14-moment), 2 (Chapman-Enskog), 3 (modified equilibrium, Mike), 4 (Jonah)", df_mode);
    const bool feqmod = !vah && (df_mode == 3 || df_mode == 4);
    if (df_mode == 4 && include_baryon && !vah)   // deltafReader.cpp:470-474
        DIE("Bilinear interpolation error: Jonah df doesn't work for nonzero muB (df_mode = 4 with include_baryon = 1)");
    const char *pdg_path, *df_dir;
    if (hrg_eos == 1) { pdg_path = "PDG/pdg-urqmd_v3.3+.dat"; df_dir = "deltaf_coefficients/vh/urqmd/"; }
    else if (hrg_eos == 2) { pdg_path = "PDG/pdg_smash.dat"; df_dir = "deltaf_coefficients/vh/smash/"; }
    else if (hrg_eos == 3) { pdg_path = "PDG/pdg_box.dat"; df_dir = "deltaf_coefficients/vh/smash_box/"; }   // readindata.h:219, deltafReader.h:29
    else DIE("hrg_eos = %d: please choose hrg_eos = (1,2,3)", hrg_eos);
    // optional key deltaf_dir: the coefficient tables come from that directory (one written by `iS3D_amd --generate-df DIR`, say) instead
    std::string df_dir_key;
    if (get_param_text("deltaf_dir", df_dir_key)) {
        if (df_dir_key.empty()) DIE("deltaf_dir is empty: name the directory that holds c0.dat ... betapi.dat, or remove the key");
        if (df_dir_key.back() != '/') df_dir_key += '/';
        df_dir = df_dir_key.c_str();
        printf("df coefficient tables from %s (deltaf_dir)\n", df_dir);
    }

    double t0 = now_s();
    // the device contexts are created while the surface is being parsed (joined before the first device call)
    std::vector<int> warm_list(rd.list.begin(), rd.list.end());
    std::thread warm([&warm_list] { is3d::warm_devices(warm_list.empty() ? nullptr : warm_list.data(), (int)warm_list.size()); });
    struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } warm_joiner{warm};
    // ---- surface (iS3D.cpp:90-98) ----
    int64_t n_cells = 0;
    double *ptr[23] = {nullptr};
    double avg[5] = {0, 0, 0, 0, 0};
    // the text surface: one read + one parse, or the binary sidecar input/surface.dat.is3dcache of an earlier run on the same file
    // (is3d_surface_open; IS3D_NO_CACHE=1 disables); the arrays are the library's until the end of this function
    is3d_surface *surf = nullptr;
    struct SurfCloser { is3d_surface *&s; ~SurfCloser() { if (s) is3d_surface_close(s); } } surf_closer{surf};
    const double *sa[32] = {nullptr};     // modes 0-7 except 2: cell_arrays23 + x, y; mode 2: arrays32
    if (vah) {
        if (is3d_surface_open("input/surface.dat", 2, 0, 0, dimension, 1, &surf)) DIE("%s", is3d_last_error());
        n_cells = is3d_surface_cells(surf);
        if (is3d_surface_arrays(surf, sa, 32, nullptr)) DIE("%s", is3d_last_error());
        if (is3d_surface_from_sidecar(surf))
            printf("surface: %lld cells from the binary sidecar input/surface.dat.is3dcache (IS3D_NO_CACHE=1 to re-parse the text)\n", (long long)n_cells);
    } else if (mem) {
        // iS3D.cpp:100-134: the surface comes from the caller's vectors, already in GeV / fm units (no hbar*c conversion)
        printf("Reading in freezeout surface from memory \n");
        n_cells = mem->n_cells;
        const double *src[23] = {mem->T, mem->P, mem->E, mem->tau, mem->eta, mem->ux, mem->uy, mem->un, mem->dat, mem->dax, mem->day, mem->dan,
                                 mem->pixx, mem->pixy, mem->pixn, mem->piyy, mem->piyn, mem->bulkPi, mem->muB, mem->nB, mem->Vx, mem->Vy, mem->Vn};
        for (int a = 0; a < 23; a++) ptr[a] = const_cast<double *>(src[a]);
        for (int a = 0; a < 18; a++)
            if (!ptr[a] && !(a == 4 && dimension == 2)) DIE("in-memory surface: a required array is NULL");
        if (n_cells > 0) surface_averages(mem, avg);
    } else {
        if (is3d_surface_open("input/surface.dat", mode, include_baryon, include_diff, dimension, 1, &surf)) DIE("%s", is3d_last_error());
        n_cells = is3d_surface_cells(surf);
        if (is3d_surface_arrays(surf, sa, 25, avg)) DIE("%s", is3d_last_error());
        // said BEFORE the spectra are computed: a user who did not expect the cache sees it while the run can still be stopped
        if (is3d_surface_from_sidecar(surf))
            printf("surface: %lld cells from the binary sidecar input/surface.dat.is3dcache (its key -- size, mtime, ctime, inode, content hash -- matches "
                   "input/surface.dat; IS3D_NO_CACHE=1 to re-parse the text)\n", (long long)n_cells);
        for (int a = 0; a < 23; a++) ptr[a] = const_cast<double *>(sa[a]);   // read-only from here on
    }
    if (!vah) {   // read_surf_VAH_PLMatch accumulates no averages (readindata.cpp:813-928)
        std::ofstream f("average_thermodynamic_quantities.dat", std::ios_base::out);
        f << std::setprecision(15) << avg[0] << "\n" << avg[1] << "\n" << avg[2] << "\n" << avg[3] << "\n" << avg[4];
    }
    // ---- species (iS3D.cpp:138-140, 156; emissionfunction.cpp:336-351, 1293-1307) ----
    int32_t npdg = 0;
    const auto pdg_read = (hrg_eos == 3) ? is3d_pdg_read_box : is3d_pdg_read;   // read_resonances: conventional | smash box (readindata.cpp:1687-1713)
    if (pdg_read(pdg_path, &npdg, nullptr, nullptr, nullptr, nullptr, nullptr, 0)) DIE("%s", is3d_last_error());
    std::vector<int64_t> pid(npdg);
    std::vector<double> pmass(npdg), pg(npdg), pb(npdg), ps(npdg);
    if (pdg_read(pdg_path, &npdg, pid.data(), pmass.data(), pg.data(), pb.data(), ps.data(), npdg)) DIE("%s", is3d_last_error());
    std::vector<double> chosen, dummy;
    if (read_table("PDG/chosen_particles.dat", chosen, dummy)) DIE("%s", is3d_last_error());
    std::vector<int64_t> mcid;
    std::vector<double> mass, sign, deg, bar;
    for (double c : chosen) {
        int id = (int)c;
        bool found = false;
        for (int n = 0; n < npdg; n++)
            if (pid[n] == id) {
                mcid.push_back(pid[n]); mass.push_back(pmass[n]); sign.push_back(ps[n]); deg.push_back(pg[n]); bar.push_back(pb[n]);
                found = true;
                break;
            }
        if (!found) DIE("chosen particle %d is not in %s", id, pdg_path);
    }
    // ---- grids (iS3D.cpp:161-167) ----
    std::vector<double> pT, pTw, phi, phiw, y, yw, eta, etaw;
    if (read_table("tables/pT_gauss_legendre_table.dat", pT, pTw) || read_table("tables/phi_gauss_legendre_table.dat", phi, phiw) ||
        read_table("tables/y_trapezoid_table_21pt.dat", y, yw))
        DIE("%s", is3d_last_error());
    // the eta table: 241 points for the smooth spectra; the reference opens the 41-point one when it samples (iS3D.cpp:164-167) and never uses it
    // there (nor does the sampler here): a run directory made for either operation is accepted
    if (operation == 2) {
        // neither there: the reference fails on its missing table (readBlockData, arsenal.cpp:406-413) -- a mis-built run directory must not pass silently
        if (read_table("tables/eta/eta_trapezoid_table_41pt.dat", eta, etaw) && read_table("tables/eta/eta_trapezoid_table_241pt.dat", eta, etaw))
            DIE("operation 2 opens tables/eta/eta_trapezoid_table_41pt.dat (or tables/eta/eta_trapezoid_table_241pt.dat): neither can be read (%s)", is3d_last_error());
    } else if (read_table("tables/eta/eta_trapezoid_table_241pt.dat", eta, etaw))
        DIE("%s", is3d_last_error());
    // ---- delta-f coefficient tables (iS3D.cpp:144-145) ----
    //      include_baryon = 0: the mu_B = 0 rows; include_baryon = 1: the full (mu_B, T) grids (deltafReader.cpp:134)
    const char *names[10] = {"c0.dat", "c1.dat", "c2.dat", "c3.dat", "c4.dat", "F.dat", "G.dat", "betabulk.dat", "betaV.dat", "betapi.dat"};
    std::vector<double> Tk, Bk, tab[10];
    for (int t = 0; t < 10 && !vah; t++) {
        std::string p = std::string(df_dir) + names[t];
        int32_t nT = 0, nB = 0;
        const bool spline_table = (t == 0 || t == 2 || t == 5 || t == 7 || t == 9);   // c0 c2 F betabulk betapi
        if (!include_baryon && !spline_table) continue;   // only the bilinear branch looks at c1 c3 c4 G betaV
        if (is3d_df_table_read_full(p.c_str(), &nT, &nB, nullptr, nullptr, nullptr, 0)) DIE("%s", is3d_last_error());
        if (!include_baryon) {
            Tk.resize(nT);
            Bk.assign(1, 0.0);
            tab[t].resize(nT);
            if (is3d_df_table_read(p.c_str(), &nT, Tk.data(), tab[t].data(), nT)) DIE("%s", is3d_last_error());
        } else {
            Tk.resize(nT);
            Bk.resize(nB);
            tab[t].resize((size_t)nT * nB);
            if (is3d_df_table_read_full(p.c_str(), &nT, &nB, Tk.data(), Bk.data(), tab[t].data(), (int64_t)tab[t].size())) DIE("%s", is3d_last_error());
        }
    }
    if (warm.joinable()) warm.join();
    double t1 = now_s();
    printf("Total number of freezeout cells: %lld\nNumber of chosen particles: %zu\n", (long long)n_cells, mcid.size());

    is3d_cells cells{};
    cells.n_cells = n_cells;
    cells.T = ptr[0]; cells.P = ptr[1]; cells.E = ptr[2]; cells.tau = ptr[3]; cells.eta = ptr[4];
    cells.ux = ptr[5]; cells.uy = ptr[6]; cells.un = ptr[7];
    cells.dat = ptr[8]; cells.dax = ptr[9]; cells.day = ptr[10]; cells.dan = ptr[11];
    cells.pixx = ptr[12]; cells.pixy = ptr[13]; cells.pixn = ptr[14]; cells.piyy = ptr[15]; cells.piyn = ptr[16];
    cells.bulkPi = ptr[17];
    cells.muB = ptr[18]; cells.nB = ptr[19]; cells.Vx = ptr[20]; cells.Vy = ptr[21]; cells.Vn = ptr[22];
    is3d_species sp{(int32_t)mcid.size(), mass.data(), sign.data(), deg.data(), bar.data()};
    is3d_grid grid{(int32_t)pT.size(), pT.data(), (int32_t)phi.size(), phi.data(), (int32_t)y.size(), y.data(),
                   (int32_t)eta.size(), eta.data(), etaw.data()};
    is3d_df_tables df{(int32_t)Tk.size(), Tk.data(), (int32_t)Bk.size(), Bk.data(), tab[0].data(), tab[1].data(), tab[2].data(),
                      tab[3].data(), tab[4].data(), tab[5].data(), tab[6].data(), tab[7].data(), tab[8].data(), tab[9].data()};
    is3d_options opts{};
    opts.dimension = dimension; opts.df_mode = df_mode; opts.include_baryon = include_baryon;
    opts.include_bulk_deltaf = include_bulk; opts.include_shear_deltaf = include_shear; opts.include_baryondiff_deltaf = include_diff;
    opts.regulate_deltaf = regulate; opts.outflow = outflow;
    opts.accumulate = 0; opts.device = rd.list.empty() ? -1 : rd.list[0]; opts.kernel_variant = variant;
    // ---- mode 5: every run ends with the spin polarization from the surface's thermal vorticity (emissionfunction.cpp:1675, :1701) ----
    auto polarization = [&]() -> int {
        if (mode != 5 || vah) return IS3D_OK;
        if (mem) {
            printf("mode = 5: the spin polarization needs the thermal vorticity, which only the file reader (input/surface.dat) provides; no S*.dat written\n");
            return IS3D_OK;
        }
        // Plasma::temperature: the first line of the averages file this run wrote, or T_switch (emissionfunction.cpp:1318-1321)
        double Tp = 0.0, set_T = 0.0;
        {
            FILE *tf = fopen("average_thermodynamic_quantities.dat", "r");
            if (!tf || fscanf(tf, "%lf", &Tp) != 1) {
                if (tf) fclose(tf);
                DIE("Error opening average thermodynamic file");
            }
            fclose(tf);
        }
        if (get_param("set_fo_temperature", &set_T, false) == IS3D_OK && (int)set_T && get_param("t_switch", &Tp)) return IS3D_EINVAL;
        const double *w[6];
        if (is3d_surface_vorticity(surf, w)) DIE("%s", is3d_last_error());
        is3d_vorticity vort{w[0], w[1], w[2], w[3], w[4], w[5]};
        is3d_options po{};
        po.dimension = dimension;
        po.device = rd.list.empty() ? -1 : rd.list[0];
        const size_t np = mcid.size() * pT.size() * phi.size() * (size_t)((dimension == 2) ? 1 : y.size());
        std::vector<double> pS[5];
        for (auto &v : pS) v.assign(np, 0.0);
        is3d_polarization_out po_out{pS[0].data(), pS[1].data(), pS[2].data(), pS[3].data(), pS[4].data()};
        is3d_polarization_stats pst{};
        printf("Calculating spin polarization vector (T = %.6f GeV)...\n", Tp);
        // a device list the user spelled out shards the cells like the run's other cell sums do.  Without one the first device computes alone:
        // the sum's association depends on the shard count, and the S files (eight digits) must not depend on how many cards a machine shows
        std::vector<is3d_polarization_stats> pss(rd.named ? rd.list.size() : 0);
        const int rcp = rd.named ? is3d_spin_polarization_multi(&cells, &vort, &sp, &grid, Tp, &po, rd.list.data(), (int32_t)rd.list.size(), &po_out,
                                                                &pst, pss.data())
                                 : is3d_spin_polarization(&cells, &vort, &sp, &grid, Tp, &po, &po_out, &pst);
        if (rcp) {
            const std::string msg = is3d_last_error();
            DIE("%s failed (%d): %s", rd.named ? "is3d_spin_polarization_multi" : "is3d_spin_polarization", rcp, msg.c_str());
        }
        printf("Writing polarization vector to file...\n");
        if (is3d_write_polarization("results", dimension, sp.n, grid.n_pT, pT.data(), grid.n_phi, phi.data(), grid.n_y, y.data(), &po_out))
            DIE("%s", is3d_last_error());
        printf("polarization: species classes evaluated: %d of %d; device time: cells %.3f ms, reduce %.3f ms\n", pst.n_classes, sp.n,
               pst.ms_cells, pst.ms_reduce);
        if (rd.named) printf("polarization: %d shard%s; slowest shard's cells %.3f ms\n", (int)pss.size(), pss.size() == 1 ? "" : "s", pst.ms_cells);
        return IS3D_OK;
    };
    // ---- mode 2: the surface's cell arrays and the deltaf_coefficients/vah tables (what src/cuda/deltafReader.cu:224-278 would have put into the surface) ----
    std::vector<double> vah_L, vah_aL, vah_c;
    is3d_vah_df_tables vt{};
    is3d_vah_cells vc{};
    if (vah) {
        int32_t nL = 0, naL = 0;
        if (is3d_vah_df_read("deltaf_coefficients/vah", &nL, &naL, nullptr, nullptr, nullptr, 0)) DIE("%s", is3d_last_error());
        vah_L.resize((size_t)nL); vah_aL.resize((size_t)naL); vah_c.resize((size_t)5 * nL * naL);
        if (is3d_vah_df_read("deltaf_coefficients/vah", &nL, &naL, vah_L.data(), vah_aL.data(), vah_c.data(), (int64_t)vah_c.size())) DIE("%s", is3d_last_error());
        const size_t tn = (size_t)nL * naL;
        vt = is3d_vah_df_tables{nL, naL, vah_L.data(), vah_aL.data(), vah_c.data(), vah_c.data() + tn, vah_c.data() + 2 * tn, vah_c.data() + 3 * tn,
                                vah_c.data() + 4 * tn};
        vc.n_cells = n_cells;
        const double **vf[25] = {&vc.tau, &vc.eta, &vc.ux, &vc.uy, &vc.un, &vc.dat, &vc.dax, &vc.day, &vc.dan, &vc.T, &vc.pitt, &vc.pitx, &vc.pity,
                                 &vc.pitn, &vc.pixx, &vc.pixy, &vc.pixn, &vc.piyy, &vc.piyn, &vc.pinn, &vc.bulkPi, &vc.Wx, &vc.Wy, &vc.Lambda, &vc.aL};
        for (int a = 0; a < 25; a++) *vf[a] = sa[a];
    }
    const int ny_eff = (dimension == 2) ? 1 : (int)y.size();
    std::vector<double> dN(mcid.size() * pT.size() * phi.size() * (size_t)ny_eff, 0.0);
    if (operation == 2) {
        // ---- emissionfunction.cpp:1522-1545: number of events, sampling, OSCAR list ----
        double oversample, min_num_hadrons, max_num_samples, sampler_seed, y_cut, fast, test_sampler, set_T, T_switch = 0.0;
        if (get_param("oversample", &oversample) || get_param("min_num_hadrons", &min_num_hadrons) || get_param("max_num_samples", &max_num_samples) ||
            get_param("sampler_seed", &sampler_seed) || get_param("y_cut", &y_cut) || get_param("fast", &fast) || get_param("test_sampler", &test_sampler) ||
            get_param("set_fo_temperature", &set_T))
            return IS3D_EINVAL;
        if ((int)set_T && get_param("t_switch", &T_switch)) return IS3D_EINVAL;
        is3d_sampler_test_bins bins{};
        if ((int)test_sampler) {                                                  // emissionfunction.cpp:205-222
            double yb, ec, eb, pl, pu, pb, t0b, t1b, tb, r0b, r1b, rb;
            if (get_param("y_bins", &yb) || get_param("eta_cut", &ec) || get_param("eta_bins", &eb) || get_param("pt_lower_cut", &pl) ||
                get_param("pt_upper_cut", &pu) || get_param("pt_bins", &pb) || get_param("tau_min", &t0b) || get_param("tau_max", &t1b) ||
                get_param("tau_bins", &tb) || get_param("r_min", &r0b) || get_param("r_max", &r1b) || get_param("r_bins", &rb))
                return IS3D_EINVAL;
            bins.y_cut = y_cut; bins.eta_cut = ec; bins.pT_lower_cut = pl; bins.pT_upper_cut = pu; bins.tau_min = t0b; bins.tau_max = t1b;
            bins.r_min = r0b; bins.r_max = r1b;
            bins.y_bins = (int)yb; bins.eta_bins = (int)eb; bins.pT_bins = (int)pb; bins.tau_bins = (int)tb; bins.r_bins = (int)rb;
        }
        // cell positions: columns 1, 2 of every supported surface format (readindata.cpp:343-346 etc.)
        std::vector<double> xs((size_t)n_cells, 0.0), ys((size_t)n_cells, 0.0);
        if (mem) {
            if (mem_x) xs.assign(mem_x, mem_x + n_cells);
            if (mem_y) ys.assign(mem_y, mem_y + n_cells);
        } else if (n_cells > 0) {   // they came with the surface (is3d_surface_arrays: arrays 23, 24; mode 2: 30, 31)
            xs.assign(sa[vah ? 30 : 23], sa[vah ? 30 : 23] + n_cells);
            ys.assign(sa[vah ? 31 : 24], sa[vah ? 31 : 24] + n_cells);
        }
        int32_t n_alpha = 0, n_pts = 0;
        const char *gla_path = "tables/gla_roots_weights_32_points.txt";
        if (is3d_gla_read(gla_path, &n_alpha, &n_pts, nullptr, nullptr, 0)) DIE("%s", is3d_last_error());
        if (n_alpha < 3) DIE("%s: needs alpha = 0, 1, 2", gla_path);
        std::vector<double> groot((size_t)n_alpha * n_pts), gweight((size_t)n_alpha * n_pts);
        if (is3d_gla_read(gla_path, &n_alpha, &n_pts, groot.data(), gweight.data(), (int64_t)groot.size())) DIE("%s", is3d_last_error());
        is3d_sampler_inputs si{};
        si.n_events = 1; si.n_gla = n_pts;
        si.seed = sampler_seed < 0 ? (uint64_t)std::chrono::system_clock::now().time_since_epoch().count() : (uint64_t)sampler_seed;   // :842-844
        si.y_cut = y_cut; si.first_cell = 0; si.x = xs.data(); si.y = ys.data();
        si.root1 = groot.data() + n_pts; si.weight1 = gweight.data() + n_pts;
        // df_mode 3 / 4 and fast mode: emissionfunction.cpp:1309-1321, sampling_kernels.cpp:852-869
        double T_avg_file = 0.0, E_avg_file = 0.0, P_avg_file = 0.0, muB_avg_file = 0.0;   // Plasma::load_thermodynamic_averages
        if (!vah) {   // (the mode-2 reader writes no averages and the anisotropic-hydro sampler takes none)
            FILE *tf = fopen("average_thermodynamic_quantities.dat", "r");
            if (!tf || fscanf(tf, "%lf %lf %lf %lf", &T_avg_file, &E_avg_file, &P_avg_file, &muB_avg_file) != 4) DIE("Error opening average thermodynamic file");
            fclose(tf);
        }
        is3d_feqmod_tables fqs{};
        if (feqmod || (int)fast) {
            double deta_min, mass_pion0;
            if (get_param("deta_min", &deta_min) || get_param("mass_pion0", &mass_pion0)) return IS3D_EINVAL;
            fqs.n_gla = n_pts;
            fqs.root1 = si.root1; fqs.weight1 = si.weight1;
            fqs.root2 = groot.data() + 2 * (size_t)n_pts; fqs.weight2 = gweight.data() + 2 * (size_t)n_pts;
            fqs.n_pdg = npdg; fqs.pdg_mass = pmass.data(); fqs.pdg_degeneracy = pg.data(); fqs.pdg_sign = ps.data();
            fqs.T_avg = T_avg_file; fqs.deta_min = deta_min; fqs.mass_pion0 = mass_pion0;
            si.feqmod = &fqs;
        }
        si.fast = (int)fast != 0;
        si.muB_avg = muB_avg_file;                                                // Plasma::baryon_chemical_potential, :858
        si.T_avg = T_avg_file;
        si.T_avg_switch = (int)set_T ? T_switch : T_avg_file;                     // :856
        if (si.fast) printf("Using fast mode: (Tavg, muBavg) = (%lf, %lf)\n", si.T_avg_switch, muB_avg_file);
        printf("iS3D Sampling Seed : %llu\n", (unsigned long long)si.seed);
        is3d_sampler_stats ss{};
        int64_t count = 0;
        double mean_yield = 0.0;   // calculate_total_yield's member mean_yield (:828), written by write_yield_list_toFile
        if ((int)oversample) {
            // emissionfunction.cpp:1524-1533: the analytic mean yield (calculate_total_yield) sizes the run
            double E_avg = 0.0, P_avg = 0.0, nB_avg = 0.0;
            {
                FILE *tf = fopen("average_thermodynamic_quantities.dat", "r");
                double t_, m_;
                if (!tf || fscanf(tf, "%lf %lf %lf %lf %lf", &t_, &E_avg, &P_avg, &m_, &nB_avg) != 5) DIE("Error opening average thermodynamic file");
                fclose(tf);
            }
            if (n_alpha < 4) DIE("%s: the yield estimate needs alpha = 0, 1, 2, 3", gla_path);
            is3d_feqmod_tables fqy = fqs;
            if (!si.feqmod) {   // the alpha = 2 nodes enter every df_mode's bulk density (J20)
                fqy.n_gla = n_pts;
                fqy.root1 = si.root1; fqy.weight1 = si.weight1;
                fqy.root2 = groot.data() + 2 * (size_t)n_pts; fqy.weight2 = gweight.data() + 2 * (size_t)n_pts;
            }
            is3d_sampler_inputs sy = si;
            sy.feqmod = &fqy;
            is3d_yield_inputs yi{T_avg_file, E_avg, P_avg, muB_avg_file, nB_avg, groot.data() + 3 * (size_t)n_pts, gweight.data() + 3 * (size_t)n_pts};
            double Ntotal = 0.0;
            printf("Total particle yield: ");
            int rc1 = is3d_total_yield(&cells, &sp, &df, &sy, &yi, &opts, &Ntotal, nullptr);
            if (rc1) DIE("is3d_total_yield failed (%d): %s", rc1, is3d_last_error());
            if (dimension == 2) printf("dN_dy ~ %lf\n\n", Ntotal / (2.0 * y_cut));
            printf("%lf\n", Ntotal);
            mean_yield = Ntotal;
            Ntotal = (double)fabsf((float)Ntotal);                                  // "prevent overflow", :1528
            // Nevents = min((int)ceil(MIN_NUM_HADRONS / Ntotal), MAX_NUM_SAMPLES); at least one event is sampled here
            si.n_events = (int32_t)std::max(1.0, std::min(std::ceil(min_num_hadrons / Ntotal), (double)(int)max_num_samples));
        }
        if (vah) si.n_events = (int32_t)std::max(1.0, (double)(int)max_num_samples);   // without vah_oversample no mean yield sizes the run: MAX_NUM_SAMPLES events
        if (vah_oversample) {
            // the anisotropic-hydro mean yield on the first device of the run's list (opts.device), with the sampler's tables, nodes and y_cut
            double Ntotal = 0.0;
            printf("Total particle yield: ");
            const int rc1 = is3d_total_yield_vah(&vc, &sp, &vt, &si, &opts, &Ntotal, nullptr, nullptr);
            if (rc1) DIE("is3d_total_yield_vah failed (%d): %s", rc1, is3d_last_error());
            if (dimension == 2) printf("dN_dy ~ %lf\n\n", Ntotal / (2.0 * y_cut));
            printf("%lf\n", Ntotal);
            if (!(Ntotal > 0.0))
                DIE("vah_oversample = 1: the linear delta-f has driven the mean yield of the surface non-positive (%g), which sizes no run (the residual bulk "
                    "pressure is outside the range of the linear correction); set vah_oversample = 0 (max_num_samples events are sampled)", Ntotal);
            mean_yield = Ntotal;
            if (is3d_oversample_events(min_num_hadrons, Ntotal, (int32_t)max_num_samples, &si.n_events)) DIE("%s", is3d_last_error());
        }
        printf("Sampling %d event(s)\n", si.n_events);
        if (df_mode == 1) printf("Sampling particles with Grad 14 moment df...\n");                    // emissionfunction.cpp:1540-1541, :1602-1603
        if (df_mode == 2) printf("Sampling particles with Chapman Enskog df...\n");
        if (df_mode == 3) printf("Sampling particles with Mike's modified distribution...\n");
        if (df_mode == 4 && !vah) printf("Sampling particles with Jonah's modified distribution...\n");
        if (vah) printf("Sampling particles from vahydro (P_L matching) with df...\n");
        if (bin_on_device || vah_bin_on_device || bin_fused) {
            // one pass: every event batch is binned on its device and dropped (anisotropic hydro: every hadron binned where it is sampled); the
            // integer histograms of the shards are added on the host
            const size_t S = (size_t)sp.n, plane = (size_t)IS3D_SAMPLER_VN_HARMONICS * S * bins.pT_bins;
            std::vector<int64_t> h_dy(S * bins.y_bins), h_de(S * bins.eta_bins), h_dp(S * bins.pT_bins), h_dt(S * bins.tau_bins), h_dr(S * bins.r_bins),
                h_vr(plane), h_vi(plane), h_yield((size_t)si.n_events);
            const is3d_sampler_hist hist{h_dy.data(), h_de.data(), h_dp.data(), h_dt.data(), h_dr.data(), h_vr.data(), h_vi.data(), h_yield.data()};
            // anisotropic hydro: a device list the user spelled out shards the cells; without one the first device samples alone
            const int rcb = bin_fused
                                ? (rd.named ? is3d_sample_fused_multi(&cells, &sp, &df, &si, &opts, rd.list.data(), (int32_t)rd.list.size(), &bins, &hist, &count, &ss)
                                            : is3d_sample_fused(&cells, &sp, &df, &si, &opts, &bins, &hist, &count, &ss))
                            : vah_bin_on_device
                                ? (rd.named ? is3d_sample_binned_vah_multi(&vc, &sp, &vt, &si, &opts, rd.list.data(), (int32_t)rd.list.size(), &bins, &hist, &count, &ss)
                                            : is3d_sample_binned_vah(&vc, &sp, &vt, &si, &opts, &bins, &hist, &count, &ss))
                                : is3d_sample_binned_multi(&cells, &sp, &df, &si, &opts, rd.list.empty() ? nullptr : rd.list.data(), (int32_t)rd.list.size(),
                                                           &bins, &hist, &count, &ss);
            if (rcb) DIE("%s failed (%d): %s", bin_fused ? "is3d_sample_fused" : vah_bin_on_device ? "is3d_sample_binned_vah" : "is3d_sample_binned", rcb, is3d_last_error());
            double t2s = now_s();
            printf("\nMomentum sampling efficiency = %f %%\n", 100.0 * (double)ss.n_acceptances / (double)std::max<int64_t>(ss.n_momentum_samples, 1));
            if (feqmod) printf("feqmod breaks down for %lld cells\n", (long long)ss.n_cells_breakdown);
            printf("Writing the binned sampler test distributions...\n");
            if (is3d_write_sampler_tests_binned("results", &bins, si.n_events, sp.n, mcid.data(), &hist, mean_yield)) DIE("%s", is3d_last_error());
            double t3s = now_s();
            printf("particles: %lld in %d event(s); hadrons drawn %lld; cells skipped (u.dsigma <= 0): %lld\n", (long long)count, si.n_events,
                   (long long)ss.n_hadrons_drawn, (long long)ss.n_cells_skipped);
            printf("device time: prep %.3f ms, count %.3f ms, fill %.3f ms; h2d %.3f ms\n", ss.ms_prep, ss.ms_count, ss.ms_fill, ss.ms_h2d);
            if (vah_bin_on_device || bin_fused) printf("binned where sampled on the device: ms_bin %.3f ms (sampling and binning, one pass), no particle workspace\n", ss.ms_bin);
            else printf("binned on the device: ms_bin %.3f ms, particle workspace %lld bytes (one event batch)\n", ss.ms_bin, (long long)ss.particle_workspace_bytes);
            printf("wall: read %.3f s, sampling %.3f s, write %.3f s\n", t1 - t0, t2s - t1, t3s - t2s);
            if (int rcp = polarization()) return rcp;
            printf("Done sampling particles. Output stored in results folder. Goodbye!\n");
            return IS3D_OK;
        }
        // count, then fill a list of that size: the viscous-hydro sampler, or (mode 2) the anisotropic-hydro one on the mode-2 cells and tables
        auto sample = [&](is3d_particle *list, int64_t capacity) {
            const int32_t *dl = rd.list.empty() ? nullptr : rd.list.data();
            if (vah) return is3d_sample_particles_vah_multi(&vc, &sp, &vt, &si, &opts, dl, (int32_t)rd.list.size(), list, capacity, &count, &ss);
            return is3d_sample_particles_multi(&cells, &sp, &df, &si, &opts, dl, (int32_t)rd.list.size(), list, capacity, &count, &ss);
        };
        const char *sampler_name = vah ? "is3d_sample_particles_vah" : "is3d_sample_particles";
        int rc2 = sample(nullptr, 0);
        if (rc2) DIE("%s failed (%d): %s", sampler_name, rc2, is3d_last_error());
        std::vector<is3d_particle> plist((size_t)std::max<int64_t>(count, 1));
        rc2 = sample(plist.data(), count);
        if (rc2) DIE("%s failed (%d): %s", sampler_name, rc2, is3d_last_error());
        double t2s = now_s();
        printf("\nMomentum sampling efficiency = %f %%\n", 100.0 * (double)ss.n_acceptances / (double)std::max<int64_t>(ss.n_momentum_samples, 1));
        if (feqmod) printf("feqmod breaks down for %lld cells\n", (long long)ss.n_cells_breakdown);
        if ((int)test_sampler) {                                                  // emissionfunction.cpp:1545-1554
            printf("Writing the binned sampler test distributions...\n");
            if (is3d_write_sampler_tests("results", &bins, si.n_events, sp.n, mcid.data(), count, plist.data(), mean_yield)) DIE("%s", is3d_last_error());
        } else {
            printf("Writing sampled particles list to OSCAR File...\n");
            if (is3d_write_particle_list_osc("results/particle_list_osc.dat", si.n_events, count, plist.data(), mcid.data())) DIE("%s", is3d_last_error());
        }
        if (decay_sampled) {
            // the thermal list decayed to stable particles, on the first device of the run's list; its species index the decay table
            printf("Decaying the sampled hadrons to stable particles...\n");
            int32_t nd = 0, nc = 0;
            if (is3d_pdg_read_decays(pdg_path, &nd, &nc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0)) DIE("%s", is3d_last_error());
            std::vector<int64_t> did((size_t)nd), dau((size_t)nc * 5);
            std::vector<double> dm((size_t)nd), dw((size_t)nd), dbr((size_t)nc);
            std::vector<int32_t> dst((size_t)nd), dnc((size_t)nd), dnp((size_t)nc);
            if (is3d_pdg_read_decays(pdg_path, &nd, &nc, did.data(), dm.data(), dw.data(), dst.data(), dnc.data(), dnp.data(), dbr.data(), dau.data(), nd, nc))
                DIE("%s", is3d_last_error());
            const is3d_decay_table tab{nd, did.data(), dm.data(), dw.data(), dst.data(), dnc.data(), dnp.data(), dbr.data(), dau.data()};
            const is3d_decay_mc_inputs mi{si.seed, 0, 0, rd.list.empty() ? -1 : rd.list[0]};
            is3d_decay_mc_stats ms{};
            int64_t n_final = 0;
            const double t4 = now_s();
            int rcd = is3d_decay_particles(&tab, sp.n, mcid.data(), &mi, count, plist.data(), nullptr, nullptr, 0, &n_final, &ms);
            std::vector<is3d_particle> decayed((size_t)std::max<int64_t>(n_final, 1));
            if (!rcd) rcd = is3d_decay_particles(&tab, sp.n, mcid.data(), &mi, count, plist.data(), decayed.data(), nullptr, n_final, &n_final, &ms);
            if (rcd) {
                const std::string msg = is3d_last_error();
                DIE("is3d_decay_particles failed (%d): %s", rcd, msg.c_str());
            }
            if (is3d_write_particle_list_osc("results/particle_list_osc_decayed.dat", si.n_events, n_final, decayed.data(), did.data())) DIE("%s", is3d_last_error());
            printf("decays: %lld primaries, %lld decays, %lld final particles (%lld without an open channel), %lld phase-space proposals (%lld exhausted); "
                   "device time: count %.3f ms, fill %.3f ms; wall %.3f s\n", (long long)ms.n_primaries, (long long)ms.n_decays, (long long)ms.n_final,
                   (long long)ms.n_stuck, (long long)ms.n_trials, (long long)ms.n_exhausted, ms.ms_count, ms.ms_fill, now_s() - t4);
        }
        double t3s = now_s();
        printf("particles: %lld in %d event(s); hadrons drawn %lld; cells skipped (u.dsigma <= 0): %lld\n", (long long)count, si.n_events,
               (long long)ss.n_hadrons_drawn, (long long)ss.n_cells_skipped);
        printf("device time: prep %.3f ms, count %.3f ms, fill %.3f ms; h2d %.3f ms\n", ss.ms_prep, ss.ms_count, ss.ms_fill, ss.ms_h2d);
        printf("wall: read %.3f s, sampling %.3f s, write %.3f s\n", t1 - t0, t2s - t1, t3s - t2s);
        if (res) {
            // iS3D.cpp:178-184: the event lists go back to the caller (final_particles_)
            res->operation = 2; res->n_events = si.n_events; res->n_species = sp.n; res->n_particles = count;
            res->particles = (is3d_particle *)malloc(sizeof(is3d_particle) * (size_t)std::max<int64_t>(count, 1));
            res->mc_id = (int64_t *)malloc(sizeof(int64_t) * (size_t)sp.n);
            res->mass = (double *)malloc(sizeof(double) * (size_t)sp.n);
            if (!res->particles || !res->mc_id || !res->mass) return is3d::set_error(IS3D_ENOMEM, "out of memory for the particle list");
            memcpy(res->particles, plist.data(), sizeof(is3d_particle) * (size_t)count);
            memcpy(res->mc_id, mcid.data(), sizeof(int64_t) * (size_t)sp.n);
            memcpy(res->mass, mass.data(), sizeof(double) * (size_t)sp.n);
        }
        if (int rcp = polarization()) return rcp;
        printf("Done sampling particles. Output stored in results folder. Goodbye!\n");
        return IS3D_OK;
    }
    if (operation == 0) {
        // ---- emissionfunction.cpp:1510-1516 -> calculate_dN_dX (smooth_kernels.cpp:1000-1446) ----
        double t0b, t1b, tb, r0b, r1b, rb;
        if (get_param("tau_min", &t0b) || get_param("tau_max", &t1b) || get_param("tau_bins", &tb) || get_param("r_min", &r0b) ||
            get_param("r_max", &r1b) || get_param("r_bins", &rb))
            return IS3D_EINVAL;
        is3d_spacetime_bins bins{t0b, t1b, r0b, r1b, (int32_t)tb, (int32_t)rb};
        // x and y: arrays 23, 24 of the viscous-hydro surfaces, the last two of is3d_surface_read_vah's 32
        const double *xp = mem ? mem_x : sa[vah ? 30 : 23], *yp = mem ? mem_y : sa[vah ? 31 : 24];
        std::vector<double> zero(1, 0.0);
        if (n_cells == 0) xp = yp = zero.data();
        const int S = sp.n, n_eta_eff = dimension == 3 ? 1 : (int)eta.size();
        std::vector<double> o_dy((size_t)S), o_t((size_t)S * bins.tau_bins), o_r((size_t)S * bins.r_bins),
            o_tr((size_t)S * bins.tau_bins * bins.r_bins), o_eta((size_t)S * n_eta_eff);
        is3d_spacetime_out out{o_dy.data(), o_t.data(), o_r.data(), o_tr.data(), o_eta.data(), nullptr};
        for (int ip = 0; ip < S; ip++) printf("Starting spacetime distribution %lld\n", (long long)mcid[ip]);   // :1100
        is3d_spacetime_stats sst{};
        int rc0;
        if (vah) {
            // anisotropic hydro: the first device of the run's list computes alone (opts.device), whatever the list holds
            printf("computing spacetime distributions from vahydro (P_L matching) with df...\n");
            rc0 = is3d_spacetime_distributions_vah(&vc, xp, yp, &sp, &grid, pTw.data(), phiw.data(), &vt, &opts, &bins, &out, &sst);
        } else {
            // the per-cell stage on cell-axis shards over the run's devices, one bin stage on the first (is3d_spacetime_distributions_multi)
            rc0 = is3d_spacetime_distributions_multi(&cells, xp, yp, &sp, &grid, pTw.data(), phiw.data(), &df, nullptr, &opts,
                                                     rd.list.empty() ? nullptr : rd.list.data(), (int32_t)rd.list.size(), &bins, &out, &sst, nullptr);
            const int nd = rd.list.empty() ? is3d_device_count() : (int)rd.list.size();
            printf("devices: %d (cell-axis shards of ~%lld cells%s)\n", nd, (long long)((n_cells + nd - 1) / std::max(nd, 1)),
                   nd > 1 ? ", one bin stage over the assembled per-cell values" : "");
        }
        if (rc0) {
            const std::string msg = is3d_last_error();
            DIE("%s failed (%d): %s", vah ? "is3d_spacetime_distributions_vah" : "is3d_spacetime_distributions_multi", rc0, msg.c_str());
        }
        // the reference prints an error line per cell with a negative bin index (:1391-1392); one line with the counts here
        if (sst.n_tau_negative || sst.n_r_negative)
            printf("Error: %lld cells with a negative tau bin index, %lld with a negative r bin index. Adjust the tau_min / r_min parameters\n",
                   (long long)sst.n_tau_negative, (long long)sst.n_r_negative);
        // 3+1D: the single eta point is eta_fo of the surface's last cell (etaValues[0], assigned at :1155 before the skip test)
        const double *eta_fo = vah ? vc.eta : cells.eta;
        std::vector<double> eta_vals = dimension == 3 ? std::vector<double>(1, n_cells > 0 ? eta_fo[n_cells - 1] : 0.0) : eta;
        if (is3d_write_spacetime("results/spacetime_distribution", &bins, S, mcid.data(), n_eta_eff, eta_vals.data(), &out))
            DIE("%s", is3d_last_error());
        for (int ip = 0; ip < S; ip++) printf("dN_dy = %lf\n", o_dy[ip]);   // :1438-1441
        printf("species classes evaluated: %d of %d; cells skipped (u.dsigma <= 0): %lld; outside the tau / r bins: %lld / %lld\n", sst.n_classes, S,
               (long long)sst.n_cells_skipped, (long long)sst.n_tau_outside, (long long)sst.n_r_outside);
        printf("device time: prep %.3f ms, per-cell %.3f ms, bins %.3f ms; h2d %.3f ms, d2h %.3f ms\n", sst.ms_prep, sst.ms_cells, sst.ms_bins,
               sst.ms_h2d, sst.ms_d2h);
        if (res) {
            res->operation = 0; res->n_species = S;
            res->mc_id = (int64_t *)malloc(sizeof(int64_t) * (size_t)S);
            res->mass = (double *)malloc(sizeof(double) * (size_t)S);
            if (!res->mc_id || !res->mass) return is3d::set_error(IS3D_ENOMEM, "out of memory");
            memcpy(res->mc_id, mcid.data(), sizeof(int64_t) * (size_t)S);
            memcpy(res->mass, mass.data(), sizeof(double) * (size_t)S);
        }
        if (int rcp = polarization()) return rcp;
        printf("Done calculating spacetime distributions. Output stored in results/spacetime_distribution. Goodbye!\n");
        return IS3D_OK;
    }
    is3d_status st{};
    int rc;
    if (vah) {
        // the call the reference has commented out (emissionfunction.cpp:1650-1654), with the coefficients the CUDA tree's reader
        // would have put into the surface (src/cuda/deltafReader.cu:224-278)
        printf("computing thermal spectra from vahydro (P_L matching) with df...\n");
        // a device list the user spelled out shards the cells; without one the first device computes alone, whatever the machine shows
        if (rd.named) {
            rc = is3d_smooth_spectra_vah_multi(&vc, &sp, &grid, &vt, &opts, rd.list.data(), (int32_t)rd.list.size(), rd.reduce, dN.data(), &st, nullptr);
            const int nd = (int)rd.list.size();
            printf("devices: %d (cell-axis shards of ~%lld cells%s)\n", nd, (long long)((n_cells + nd - 1) / std::max(nd, 1)),
                   nd > 1 ? (rd.reduce == IS3D_REDUCE_RCCL ? ", RCCL all-reduce of the spectrum" : ", shard-ordered device sum of the spectrum") : "");
        } else {
            rc = is3d_smooth_spectra_vah_df(&vc, &sp, &grid, &vt, &opts, dN.data(), &st);
        }
    } else if (feqmod) {
        printf("computing thermal spectra from vhydro with feqmod...\n");
        // emissionfunction.cpp:1309-1319: Gauss-Laguerre tables, Plasma::load_thermodynamic_averages (the file written
        // above, read back as text), parameters deta_min and mass_pion0 (:184, :188)
        int32_t n_alpha = 0, n_pts = 0;
        const char *gla_path = "tables/gla_roots_weights_32_points.txt";
        if (is3d_gla_read(gla_path, &n_alpha, &n_pts, nullptr, nullptr, 0)) DIE("%s", is3d_last_error());
        if (n_alpha < 3) DIE("%s: needs alpha = 0, 1, 2", gla_path);
        std::vector<double> groot((size_t)n_alpha * n_pts), gweight((size_t)n_alpha * n_pts);
        if (is3d_gla_read(gla_path, &n_alpha, &n_pts, groot.data(), gweight.data(), (int64_t)groot.size())) DIE("%s", is3d_last_error());
        double deta_min, mass_pion0, T_avg = 0.0;
        if (get_param("deta_min", &deta_min) || get_param("mass_pion0", &mass_pion0)) return IS3D_EINVAL;
        {
            FILE *tf = fopen("average_thermodynamic_quantities.dat", "r");
            if (!tf || fscanf(tf, "%lf", &T_avg) != 1) DIE("Error opening average thermodynamic file");
            fclose(tf);
        }
        is3d_feqmod_tables fq{};
        fq.n_gla = n_pts;
        fq.root1 = groot.data() + n_pts; fq.weight1 = gweight.data() + n_pts;
        fq.root2 = groot.data() + 2 * (size_t)n_pts; fq.weight2 = gweight.data() + 2 * (size_t)n_pts;
        fq.n_pdg = npdg; fq.pdg_mass = pmass.data(); fq.pdg_degeneracy = pg.data(); fq.pdg_sign = ps.data();
        fq.T_avg = T_avg; fq.deta_min = deta_min; fq.mass_pion0 = mass_pion0;
        rc = is3d_smooth_spectra_multi(&cells, &sp, &grid, &df, &fq, &opts, rd.list.empty() ? nullptr : rd.list.data(), (int32_t)rd.list.size(),
                                       rd.reduce, dN.data(), &st, nullptr);
    } else {
        printf("computing thermal spectra from vhydro with df...\n");
        rc = is3d_smooth_spectra_multi(&cells, &sp, &grid, &df, nullptr, &opts, rd.list.empty() ? nullptr : rd.list.data(), (int32_t)rd.list.size(),
                                       rd.reduce, dN.data(), &st, nullptr);
    }
    if (!vah) {
        const int nd = rd.list.empty() ? is3d_device_count() : (int)rd.list.size();
        printf("devices: %d (cell-axis shards of ~%lld cells%s)\n", nd, (long long)((n_cells + nd - 1) / std::max(nd, 1)),
               nd > 1 ? (rd.reduce == IS3D_REDUCE_RCCL ? ", RCCL all-reduce of the spectrum" : ", shard-ordered device sum of the spectrum") : "");
    }
    if (rc) {
        const std::string msg = is3d_last_error();
        DIE("is3d_smooth_spectra failed (%d): %s", rc, msg.c_str());
    }
    if (feqmod && !vah) printf("\nfeqmod breaks down for %lld cells\n\n", (long long)st.n_cells_breakdown);   // smooth_kernels.cpp:989
    double t2 = now_s();
    if (is3d_write_results("results", dimension, sp.n, mcid.data(), grid.n_pT, pT.data(), pTw.data(), grid.n_phi, phi.data(),
                           phiw.data(), grid.n_y, y.data(), dN.data()))
        DIE("%s", is3d_last_error());
    double t3 = now_s();
    printf("species classes evaluated: %d of %d; cells skipped (u.dsigma <= 0): %lld\n", st.n_classes, sp.n, (long long)st.n_cells_skipped);
    printf("device time: prep %.3f ms, main %.3f ms (kernel variant %d), finalize %.3f ms; h2d %.3f ms, d2h %.3f ms\n", st.ms_prep,
           st.ms_main, st.kernel_variant, st.ms_finalize, st.ms_h2d, st.ms_d2h);
    const int src_kind = surf ? is3d_surface_source(surf) : -1;
    printf("wall: read %.3f s, spectra %.3f s, write %.3f s\n", t1 - t0, t2 - t1, t3 - t2);
    if (src_kind >= 0)
        printf("surface: %s\n", src_kind == 2 ? "binary sidecar input/surface.dat.is3dcache (matches the text file; IS3D_NO_CACHE=1 to ignore)"
                                 : src_kind == 1 ? "text parsed, sidecar input/surface.dat.is3dcache written for the next run" : "text parsed");
    if (res) {
        res->operation = 1; res->n_species = sp.n; res->n_spectrum = (int64_t)dN.size();
        res->spectrum = (double *)malloc(sizeof(double) * dN.size());
        res->mc_id = (int64_t *)malloc(sizeof(int64_t) * (size_t)sp.n);
        res->mass = (double *)malloc(sizeof(double) * (size_t)sp.n);
        if (!res->spectrum || !res->mc_id || !res->mass) return is3d::set_error(IS3D_ENOMEM, "out of memory for the spectrum");
        memcpy(res->spectrum, dN.data(), sizeof(double) * dN.size());
        memcpy(res->mc_id, mcid.data(), sizeof(int64_t) * (size_t)sp.n);
        memcpy(res->mass, mass.data(), sizeof(double) * (size_t)sp.n);
    }
    if (do_decays) {
        // emissionfunction.cpp:1689-1698: the feed-down of the thermal spectrum, then its two files; on the first device of the run's list
        printf("Starting resonance decays...\n");
        int32_t nd = 0, nc = 0;
        if (is3d_pdg_read_decays(pdg_path, &nd, &nc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0)) DIE("%s", is3d_last_error());
        std::vector<int64_t> did((size_t)nd), dau((size_t)nc * 5);
        std::vector<double> dm((size_t)nd), dw((size_t)nd), dbr((size_t)nc);
        std::vector<int32_t> dst((size_t)nd), dnc((size_t)nd), dnp((size_t)nc);
        if (is3d_pdg_read_decays(pdg_path, &nd, &nc, did.data(), dm.data(), dw.data(), dst.data(), dnc.data(), dnp.data(), dbr.data(), dau.data(), nd, nc))
            DIE("%s", is3d_last_error());
        const is3d_decay_table tab{nd, did.data(), dm.data(), dw.data(), dst.data(), dnc.data(), dnp.data(), dbr.data(), dau.data()};
        std::vector<double> fed(dN);
        is3d_decay_stats dst_{};
        const double t4 = now_s();
        const int rcd = is3d_resonance_decays(&tab, sp.n, mcid.data(), &grid, dimension, rd.list.empty() ? -1 : rd.list[0], fed.data(), &dst_);
        if (rcd) {
            const std::string msg = is3d_last_error();
            DIE("is3d_resonance_decays failed (%d): %s", rcd, msg.c_str());
        }
        printf("Writing thermal + resonance decays spectra to file...\n");
        if (is3d_write_results_decays("results", dimension, sp.n, grid.n_pT, pT.data(), grid.n_phi, phi.data(), grid.n_y, y.data(), fed.data()))
            DIE("%s", is3d_last_error());
        printf("resonance decays: %d parents, %d channels integrated (%d with adjusted masses), %lld acos clamps; device time: tables %.3f ms, "
               "feed-down %.3f ms; wall %.3f s\n", dst_.n_parents, dst_.n_channels, dst_.n_adjusted, (long long)dst_.n_clamps, dst_.ms_tables,
               dst_.ms_feed, now_s() - t4);
    }
    if (int rcp = polarization()) return rcp;
    printf("Done calculating particle spectra. Output stored in results folder. Goodbye!\n");
    return IS3D_OK;
}

extern "C" int is3d_run_particlization(const is3d_cells *surface, const double *x, const double *y, int32_t kernel_variant,
                                       is3d_run_result *result)
{
    return is3d_run_particlization_on(surface, x, y, kernel_variant, nullptr, 0, IS3D_REDUCE_ORDERED, result);
}

extern "C" int is3d_run_particlization_on(const is3d_cells *surface, const double *x, const double *y, int32_t kernel_variant,
                                          const int32_t *devices, int32_t n_devices, int32_t reduce, is3d_run_result *result)
{
    if (result) memset(result, 0, sizeof *result);
    RunDevices rd;
    if (int rc = parse_run_devices(devices, n_devices, reduce, rd)) return rc;
    return run_impl(surface, x, y, kernel_variant, rd, result);
}

extern "C" void is3d_run_result_free(is3d_run_result *r)
{
    if (!r) return;
    free(r->particles); free(r->mc_id); free(r->mass); free(r->spectrum);
    memset(r, 0, sizeof *r);
}

// is3d_run.cpp -- IS3D::run_particlization (src/cpp/iS3D.cpp:74-192 of the reference) behind the C ABI: the driver layer shared by the command
// line tool (is3d_main.cpp) and the embedding class (include/iS3D_amd.hpp).  What every parameter and optional key selects, what is refused and
// what each operation prints and writes: INTEGRATION.md, section 1 ("The driver's optional keys").  Runs in an iS3D run directory.
// Reads: iS3D_parameters.dat; input/surface.dat (or its sidecar input/surface.dat.is3dcache); PDG/pdg-urqmd_v3.3+.dat | pdg_smash.dat | pdg_box.dat;
//   PDG/chosen_particles.dat; tables/{pT,phi}_gauss_legendre_table.dat, tables/y_trapezoid_table_21pt.dat, tables/eta/eta_trapezoid_table_241pt.dat
//   (operation 2: the 41pt one first); deltaf_coefficients/vh/<eos>/{c0..c4,F,G,betabulk,betaV,betapi}.dat, or those names under deltaf_dir;
//   deltaf_coefficients/vah/c{0..4}_vah1.dat (mode 2); tables/gla_roots_weights_32_points.txt (df_mode 3 / 4, operation 2); its own averages file.
// Writes: average_thermodynamic_quantities.dat (not in mode 2); input/surface.dat.is3dcache; in results/, which must exist -- operation 1:
//   dN_pTdpTdphidy*.dat, dN_dpTdphidy.dat, dN_dy_*.dat, vn_continuous/vn_*.dat, *_resonance_decays.dat; operation 0: spacetime_distribution/*.dat;
//   operation 2: particle_list_osc.dat, particle_list_osc_decayed.dat, or the binned test files (test_sampler = 1; with test_sampler_decayed = 1
//   also under results/decayed/; with test_sampler_flow = 1 the flow cumulants and multiplicities under results/flow/ (and, with
//   test_sampler_flow_diff = 1, the differential flow against pT beside them); with test_sampler_pairs = 1
//   the two-particle correlations under results/pairs/; with test_sampler_hbt = 1 the HBT correlation functions and radii under results/hbt/);
//   mode 5: S{t,x,y,n}.dat.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <string>
#include <thread>
#include <vector>

#include <sys/stat.h>

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

// The parameter file, read and parsed once (is3d::param_pairs: the line rules of is3d_param_get).  A later line overwrites an earlier one.
class RunParams {
public:
    explicit RunParams(const char *path) : path_(path), rc_(is3d::param_pairs(path, pairs_)), error_(rc_ ? is3d_last_error() : "") {}
    // a key the run cannot do without: is3d_param_get's message behind "iS3D-amd: " when it is absent or the file cannot be used
    int required(const char *name, double *v) const
    {
        if (rc_) {
            is3d::set_error(rc_, "%s", error_.c_str());
            fprintf(stderr, "iS3D-amd: %s\n", error_.c_str());
            return IS3D_EINVAL;
        }
        return optional(name, v) ? IS3D_OK : die("parameter with name %s not found in %s", name, path_.c_str());
    }
    // false, and *v untouched, when the key is absent; the value is strtod of the right-hand side
    bool optional(const char *name, double *v) const
    {
        std::string rhs;
        if (!text(name, &rhs)) return false;
        *v = strtod(rhs.c_str(), nullptr);
        return true;
    }
    // the right-hand side as text: blanks and tabs are gone already, '\r' goes here
    bool text(const char *name, std::string *s) const
    {
        bool found = false;
        for (const auto &p : pairs_)
            if (p.first == name) { *s = p.second; found = true; }
        s->erase(std::remove(s->begin(), s->end(), '\r'), s->end());
        return found;
    }

private:
    std::string path_;
    std::vector<std::pair<std::string, std::string>> pairs_;
    int rc_;
    std::string error_;
};

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
    const int32_t *data() const { return list.empty() ? nullptr : list.data(); }
    int32_t size() const { return (int32_t)list.size(); }
    int32_t first() const { return list.empty() ? -1 : list[0]; }
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

// the embedding entry's surface: the caller's arrays, already in GeV / fm units, and the cells' positions (either may be NULL)
struct MemSurface { const is3d_cells *cells; const double *x, *y; };

// what iS3D_parameters.dat asks for, after every check that needs nothing but that file
struct RunConfig {
    int operation, mode, hrg_eos, dimension, df_mode, include_baryon, include_bulk, include_shear, include_diff, regulate, outflow;
    // optional keys (absent: 0); an `is set` flag here has passed its checks
    bool do_decays, decay_sampled, bin_on_device, bin_fused, vah_oversample, vah_bin_on_device, vah_sampler, test_sampler, bin_decayed, flow, flow_diff, pairs, hbt;
    is3d_hbt_bins hbt_bins;     // test_sampler_hbt = 1: hbt_y_cut, hbt_pT_min, hbt_pT_max, hbt_kT_min, hbt_kT_max, hbt_kT_bins, hbt_q_max, hbt_q_bins (defaults 0.5, 0.1, 1.5, 0.1, 0.9, 4, 0.1, 20)
    is3d_pair_bins pair_bins;   // test_sampler_pairs = 1: pairs_y_cut, pairs_pT_min, pairs_pT_max, pairs_y_bins, pairs_phi_bins (defaults 2.0, 0.2, 3.0, 32, 32)
    is3d_flow_cuts flow_cuts;   // test_sampler_flow = 1: flow_y_cut, flow_y_gap, flow_pT_min, flow_pT_max (defaults 1.0, 0.5, 0.2, 3.0)
    // test_sampler_flow_diff = 1 (beside test_sampler_flow = 1): flow_diff_pt_bins uniform bins from flow_pT_min to flow_diff_pt_max (defaults 14, 3.0)
    std::vector<double> flow_diff_edges;
    bool vah;               // mode 2 from files: the anisotropic-hydro surface, tables and routines
    bool feqmod;            // df_mode 3 / 4 of viscous hydro: the modified-equilibrium kernels
    const char *pdg_path;
    std::string df_dir;     // with its trailing '/'
};

// Reads every key that decides whether the run is accepted and makes every refusal, in a fixed order: a file with two things wrong gets the
// message of the earlier check.  Touches no device and writes no file (its one line on stdout names deltaf_dir).  mem: NULL for a run from files.
static int parse_config(const RunParams &p, const MemSurface *mem, bool wants_result, RunConfig &c)
{
    double v = 0.0;
    const struct { int *var; const char *name; } required[11] = {
        {&c.operation, "operation"}, {&c.mode, "mode"}, {&c.hrg_eos, "hrg_eos"}, {&c.dimension, "dimension"}, {&c.df_mode, "df_mode"},
        {&c.include_baryon, "include_baryon"}, {&c.include_bulk, "include_bulk_deltaf"}, {&c.include_shear, "include_shear_deltaf"},
        {&c.include_diff, "include_baryondiff_deltaf"}, {&c.regulate, "regulate_deltaf"}, {&c.outflow, "outflow"}};
    for (const auto &r : required) {
        if (p.required(r.name, &v)) return IS3D_EINVAL;
        *r.var = (int)v;
    }
    const auto is_set = [&p](const char *name) { double key = 0.0; return p.optional(name, &key) && (int)key != 0; };
    c.do_decays = is_set("do_resonance_decays"); c.decay_sampled = is_set("decay_sampled_hadrons"); c.bin_on_device = is_set("test_sampler_on_device");
    c.bin_fused = is_set("test_sampler_fused"); c.vah_sampler = is_set("vah_sampler"); c.vah_oversample = is_set("vah_oversample");
    c.vah_bin_on_device = is_set("vah_sampler_on_device"); c.bin_decayed = is_set("test_sampler_decayed");
    c.flow = is_set("test_sampler_flow");
    c.flow_diff = is_set("test_sampler_flow_diff");
    c.pairs = is_set("test_sampler_pairs");
    c.hbt = is_set("test_sampler_hbt");
    // test_sampler is a sampler key: optional where a check only looks at it, required (with the missing-key message) where a key depends on it
    const bool has_test_sampler = p.optional("test_sampler", &v);
    c.test_sampler = has_test_sampler && (int)v != 0;
    const auto need_test_sampler = [&] { return has_test_sampler ? IS3D_OK : p.required("test_sampler", &v); };
    const int operation = c.operation, mode = c.mode, df_mode = c.df_mode, hrg_eos = c.hrg_eos;
    const bool vah = c.vah = !mem && mode == 2;
    // operation: 0 smooth spacetime distributions, 1 smooth momentum spectra, 2 particle sampler
    if (operation != 0 && operation != 1 && operation != 2)
        DIE("operation = %d: operation = 0 (smooth spacetime distributions), 1 (smooth momentum spectra) and 2 (particle sampler) are on this path", operation);
    if (operation == 0) {
        // df_mode 3 / 4 of viscous hydro (calculate_dN_dX_feqmod) is a library entry only; mode 2 with df_mode 4 has is3d_spacetime_distributions_vah
        if ((df_mode == 3 || df_mode == 4) && !vah)
            DIE("operation = 0 with df_mode = %d (calculate_dN_dX_feqmod) is not run by this driver yet (the library entry is3d_spacetime_distributions_feqmod has it): set df_mode = 1 or 2", df_mode);
        if (mem && (!mem->x || !mem->y)) DIE("operation = 0 needs the cells' x and y positions (NULL given)");
    }
    // do_resonance_decays = 1: the feed-down runs after the momentum spectra (emissionfunction.cpp:1689-1698) and needs a list with decay data
    if (c.do_decays) {
        if (operation != 1)
            DIE("do_resonance_decays = 1 with operation = %d: the feed-down follows the momentum spectra (operation = 1) only; set do_resonance_decays = 0", operation);
        if (hrg_eos == 3)
            DIE("do_resonance_decays = 1 with hrg_eos = 3: PDG/pdg_box.dat carries no decay data (smash box: no decay info, iS3D_parameters.dat); use hrg_eos = 1 or 2");
    }
    // decay_sampled_hadrons = 1: the sampled list decayed to stable particles (is3d_decay_particles): operation 2 writing its list, hrg_eos 1 | 2
    if (c.decay_sampled) {
        if (operation != 2)
            DIE("decay_sampled_hadrons = 1 with operation = %d: it decays the sampler's particle list (operation = 2); set decay_sampled_hadrons = 0", operation);
        if (hrg_eos != 1 && hrg_eos != 2)
            DIE("decay_sampled_hadrons = 1 with hrg_eos = %d: PDG/pdg_box.dat carries no decay data (smash box: no decay info, iS3D_parameters.dat); use hrg_eos = 1 or 2", hrg_eos);
        if (need_test_sampler()) return IS3D_EINVAL;
        if (c.test_sampler)
            DIE("decay_sampled_hadrons = 1 with test_sampler = 1: that run bins the thermal hadrons and writes no particle list to decay; set decay_sampled_hadrons = 0");
    }
    // test_sampler_on_device = 1: the test_sampler = 1 distributions binned on the device, no particle list -- so not for the embedding entry
    if (c.bin_on_device) {
        if (operation != 2)
            DIE("test_sampler_on_device = 1 with operation = %d: it bins the sampler's hadrons (operation = 2); set test_sampler_on_device = 0", operation);
        if (need_test_sampler()) return IS3D_EINVAL;
        if (!c.test_sampler)
            DIE("test_sampler_on_device = 1 with test_sampler = 0: the particle list is the output of that run and is not kept on this path; set test_sampler_on_device = 0");
        if (wants_result)
            DIE("test_sampler_on_device = 1: the embedding entry returns the particle list, which this path never holds; set test_sampler_on_device = 0");
    }
    // test_sampler_fused = 1: the viscous sampler's hadrons binned where they are sampled (is3d_sample_fused), no particle list
    if (c.bin_fused) {
        if (operation != 2)
            DIE("test_sampler_fused = 1 with operation = %d: it bins the sampler's hadrons (operation = 2); set test_sampler_fused = 0", operation);
        if (need_test_sampler()) return IS3D_EINVAL;
        if (!c.test_sampler)
            DIE("test_sampler_fused = 1 with test_sampler = 0: the particle list is the output of that run and is never held on this path; set test_sampler_fused = 0");
        if (vah)
            DIE("test_sampler_fused = 1 with mode = 2: it names the viscous-hydro sampler; the anisotropic-hydro one has vah_sampler_on_device; set test_sampler_fused = 0");
        if (wants_result)
            DIE("test_sampler_fused = 1: the embedding entry returns the particle list, which this path never holds; set test_sampler_fused = 0");
    }
    // vah_oversample = 1: the anisotropic-hydro mean yield (is3d_total_yield_vah) sizes the run of this library's own VAH sampler, and no other
    if (c.vah_oversample && !(vah && operation == 2 && df_mode == 4 && c.vah_sampler))
        DIE("vah_oversample = 1 with mode = %d, operation = %d, df_mode = %d, vah_sampler = %d: the anisotropic-hydro mean yield sizes this library's own "
            "anisotropic-hydro sampler only (mode = 2, operation = 2, df_mode = 4, vah_sampler = 1); set vah_oversample = 0", mode, operation, df_mode,
            (int)c.vah_sampler);
    // vah_sampler_on_device = 1: the VAH sampler's hadrons binned where they are sampled (is3d_sample_binned_vah), no particle list
    if (c.vah_bin_on_device) {
        if (!(vah && operation == 2 && df_mode == 4 && c.vah_sampler && c.test_sampler))
            DIE("vah_sampler_on_device = 1 with mode = %d, operation = %d, df_mode = %d, vah_sampler = %d, test_sampler = %d: it bins the hadrons of this "
                "library's own anisotropic-hydro sampler on the device and keeps no particle list (mode = 2, operation = 2, df_mode = 4, vah_sampler = 1, "
                "test_sampler = 1; the viscous-hydro route has test_sampler_on_device); set vah_sampler_on_device = 0", mode, operation, df_mode,
                (int)c.vah_sampler, (int)c.test_sampler);
        if (wants_result)
            DIE("vah_sampler_on_device = 1: the embedding entry returns the particle list, which this path never holds; set vah_sampler_on_device = 0");
    }
    if (vah) {
        if (operation == 2) {
            // vah_sampler = 1 selects this library's own VAH sampler (is3d_sample_particles_vah; the reference has none); it has keys of its own
            if (!c.vah_sampler)
                DIE("mode = 2 (anisotropic hydro): operation = 0 or 1; the reference's VAH sampler is an empty stub (emissionfunction_sampling_kernels.cpp:1231-1239); "
                    "set vah_sampler = 1 for this library's own anisotropic-hydro sampler (is3d_sample_particles_vah)");
            if (c.bin_on_device)
                DIE("test_sampler_on_device = 1 with mode = 2: the anisotropic-hydro sampler's hadrons are binned on the host (test_sampler = 1); set test_sampler_on_device = 0");
            if (p.required("oversample", &v)) return IS3D_EINVAL;
            if ((int)v)
                DIE("oversample = 1 with mode = 2: the mean yield that sizes an oversampled run (calculate_total_yield) is viscous-hydro only; set oversample = 0 "
                    "(max_num_samples events are sampled), and vah_oversample = 1 for the anisotropic-hydro mean yield (is3d_total_yield_vah) to size the run");
        }
        // the per-cell c0..c4 exist for df_mode 4 only
        if (df_mode != 4) DIE("mode = 2 (anisotropic hydro) needs df_mode = 4: the per-cell 14-moment coefficients c0..c4 exist for that combination only (emissionfunction.cpp:1410-1418)");
    }
    // mode: a surface format with a reader here (the embedding entry brings its own cells)
    if (!mem && !vah && mode != 0 && mode != 1 && mode != 4 && mode != 5 && mode != 6 && mode != 7)
        DIE("mode = %d: the smooth path reads the viscous-hydro surface formats 0, 1, 4, 5, 6, 7 and the anisotropic-hydro format 2 (3 = VAH P_L, P_T matching has no kernel in the reference: emissionfunction.cpp:1328-1681)", mode);
    if (df_mode < 1 || df_mode > 4) DIE("df_mode = %d: 1 (14-moment), 2 (Chapman-Enskog), 3 (modified equilibrium, Mike), 4 (Jonah)", df_mode);
    c.feqmod = !vah && (df_mode == 3 || df_mode == 4);
    if (df_mode == 4 && c.include_baryon && !vah)   // deltafReader.cpp:470-474
        DIE("Bilinear interpolation error: Jonah df doesn't work for nonzero muB (df_mode = 4 with include_baryon = 1)");
    // hrg_eos: the particle list and its coefficient directory (readindata.h:219, deltafReader.h:29)
    if (hrg_eos == 1) { c.pdg_path = "PDG/pdg-urqmd_v3.3+.dat"; c.df_dir = "deltaf_coefficients/vh/urqmd/"; }
    else if (hrg_eos == 2) { c.pdg_path = "PDG/pdg_smash.dat"; c.df_dir = "deltaf_coefficients/vh/smash/"; }
    else if (hrg_eos == 3) { c.pdg_path = "PDG/pdg_box.dat"; c.df_dir = "deltaf_coefficients/vh/smash_box/"; }
    else DIE("hrg_eos = %d: please choose hrg_eos = (1,2,3)", hrg_eos);
    // deltaf_dir: the coefficient tables come from that directory (one written by `iS3D_amd --generate-df DIR`, say) instead
    std::string dir;
    if (p.text("deltaf_dir", &dir)) {
        if (dir.empty()) DIE("deltaf_dir is empty: name the directory that holds c0.dat ... betapi.dat, or remove the key");
        if (dir.back() != '/') dir += '/';
        c.df_dir = dir;
        printf("df coefficient tables from %s (deltaf_dir)\n", c.df_dir.c_str());
    }
    // test_sampler_decayed = 1: beside the thermal distributions of a test_sampler_on_device run, those of the hadrons after their Monte Carlo
    // decays, binned on the device batch by batch (is3d_sample_decayed_binned).  Behind every other check: no earlier message or order changes.
    if (c.bin_decayed) {
        if (operation != 2)
            DIE("test_sampler_decayed = 1 with operation = %d: it decays and bins the sampler's hadrons (operation = 2); set test_sampler_decayed = 0", operation);
        if (need_test_sampler()) return IS3D_EINVAL;
        if (!c.test_sampler)
            DIE("test_sampler_decayed = 1 with test_sampler = 0: it writes the test_sampler distributions of the decayed hadrons beside the thermal ones; set test_sampler_decayed = 0");
        if (vah)
            DIE("test_sampler_decayed = 1 with mode = 2: it decays the viscous-hydro sampler's hadrons; the anisotropic-hydro sampler has no such entry; set test_sampler_decayed = 0");
        if (wants_result)
            DIE("test_sampler_decayed = 1: the embedding entry returns the particle list, which this path never holds; set test_sampler_decayed = 0");
        if (!c.bin_on_device)
            DIE("test_sampler_decayed = 1 with test_sampler_on_device = 0: the hadrons are decayed where each event batch is binned, on the device "
                "(test_sampler_on_device = 1); set test_sampler_decayed = 0");
        if (c.bin_fused)
            DIE("test_sampler_decayed = 1 with test_sampler_fused = 1: the fused pass never holds the batch of hadrons that is decayed; set test_sampler_decayed = 0");
        if (hrg_eos != 1 && hrg_eos != 2)
            DIE("test_sampler_decayed = 1 with hrg_eos = %d: PDG/pdg_box.dat carries no decay data (smash box: no decay info, iS3D_parameters.dat); use hrg_eos = 1 or 2, "
                "or set test_sampler_decayed = 0", hrg_eos);
    }
    // test_sampler_flow = 1: beside the distributions of a test_sampler_on_device run, the per-event flow records of its hadrons (and, with
    // test_sampler_decayed = 1, of their decay products) as cumulants and multiplicities under results/flow/ (results/decayed/flow/).  Behind
    // every other check, and the one check here that looks at the file system: the directories must exist before anything is written.
    if (c.flow) {
        if (operation != 2)
            DIE("test_sampler_flow = 1 with operation = %d: it records the flow vectors of the sampler's hadrons (operation = 2); set test_sampler_flow = 0", operation);
        if (need_test_sampler()) return IS3D_EINVAL;
        if (!c.test_sampler)
            DIE("test_sampler_flow = 1 with test_sampler = 0: it writes the flow cumulants beside the test_sampler distributions; set test_sampler_flow = 0");
        if (vah)
            DIE("test_sampler_flow = 1 with mode = 2: it records the viscous-hydro sampler's hadrons; the anisotropic-hydro sampler has no such entry; set test_sampler_flow = 0");
        if (wants_result)
            DIE("test_sampler_flow = 1: the embedding entry returns the particle list, which this path never holds; set test_sampler_flow = 0");
        if (!c.bin_on_device)
            DIE("test_sampler_flow = 1 with test_sampler_on_device = 0: the flow records are made where each event batch is binned, on the device "
                "(test_sampler_on_device = 1); set test_sampler_flow = 0");
        if (c.bin_fused)
            DIE("test_sampler_flow = 1 with test_sampler_fused = 1: the fused pass never holds the batch of hadrons that is recorded; set test_sampler_flow = 0");
        is3d_flow_cuts &f = c.flow_cuts;
        f = is3d_flow_cuts{1.0, 0.5, 0.2, 3.0, 0};
        p.optional("flow_y_cut", &f.y_cut); p.optional("flow_y_gap", &f.y_gap); p.optional("flow_pt_min", &f.pT_min); p.optional("flow_pt_max", &f.pT_max);
        if (!(f.y_cut > 0.0 && f.y_gap >= 0.0 && f.y_gap < 2.0 * f.y_cut && f.pT_min >= 0.0 && f.pT_max > f.pT_min))
            DIE("test_sampler_flow = 1 with flow_y_cut = %g, flow_y_gap = %g, flow_pT_min = %g, flow_pT_max = %g: the cuts need flow_y_cut > 0, "
                "0 <= flow_y_gap < 2 flow_y_cut and flow_pT_max > flow_pT_min >= 0; set test_sampler_flow = 0", f.y_cut, f.y_gap, f.pT_min, f.pT_max);
        for (const char *dir : {"results/flow", "results/decayed/flow"}) {
            if (dir[8] == 'd' && !c.bin_decayed) continue;
            struct stat sb;
            if (stat(dir, &sb) != 0 || !S_ISDIR(sb.st_mode))
                DIE("test_sampler_flow = 1: the directory %s is missing; create it or set test_sampler_flow = 0", dir);
        }
    }
    // test_sampler_flow_diff = 1: beside the flow cumulants of a test_sampler_flow = 1 run, v_n{2}, v_n{4} and v_n{2,gap} against pT in
    // uniform bins from flow_pT_min to flow_diff_pt_max, under the same directories (which the check above has found).  Every edge is
    // computed here, once: flow_pT_min + k (flow_diff_pt_max - flow_pT_min) / bins, the last one flow_diff_pt_max exactly.
    if (c.flow_diff) {
        if (!c.flow)
            DIE("test_sampler_flow_diff = 1 with test_sampler_flow = 0: it writes the differential flow beside the flow cumulants of test_sampler_flow = 1; "
                "set test_sampler_flow_diff = 0");
        double bins = 14.0, top = 3.0;
        p.optional("flow_diff_pt_bins", &bins); p.optional("flow_diff_pt_max", &top);
        const double lo = c.flow_cuts.pT_min;
        const bool whole = bins >= 1.0 && bins <= (double)IS3D_FLOW_DIFF_MAX_BINS && bins == (double)(int)bins;
        const int n = whole ? (int)bins : 0;
        c.flow_diff_edges.assign((size_t)n + 1, lo);
        for (int k = 1; k <= n; k++) c.flow_diff_edges[(size_t)k] = k == n ? top : lo + (double)k * (top - lo) / (double)n;
        bool rising = whole && top > lo && top <= 1.7976931348623157e308;
        for (int k = 1; k <= n && rising; k++) rising = c.flow_diff_edges[(size_t)k] > c.flow_diff_edges[(size_t)k - 1];
        if (!rising)
            DIE("test_sampler_flow_diff = 1 with flow_diff_pt_bins = %g, flow_diff_pt_max = %g, flow_pT_min = %g: the bins need a whole 1 <= flow_diff_pt_bins <= %d "
                "and a finite flow_diff_pt_max > flow_pT_min that leaves every bin a width; set test_sampler_flow_diff = 0", bins, top, lo, IS3D_FLOW_DIFF_MAX_BINS);
    }
    // test_sampler_pairs = 1: the two-particle (delta y, delta phi) correlations of the same hadrons under results/pairs/
    // (results/decayed/pairs/), refused in the situations that refuse test_sampler_flow, and for bad bins and missing directories
    if (c.pairs) {
        if (operation != 2)
            DIE("test_sampler_pairs = 1 with operation = %d: it correlates the sampler's hadrons (operation = 2); set test_sampler_pairs = 0", operation);
        if (need_test_sampler()) return IS3D_EINVAL;
        if (!c.test_sampler)
            DIE("test_sampler_pairs = 1 with test_sampler = 0: it writes the pair correlations beside the test_sampler distributions; set test_sampler_pairs = 0");
        if (vah)
            DIE("test_sampler_pairs = 1 with mode = 2: it correlates the viscous-hydro sampler's hadrons; the anisotropic-hydro sampler has no such entry; set test_sampler_pairs = 0");
        if (wants_result)
            DIE("test_sampler_pairs = 1: the embedding entry returns the particle list, which this path never holds; set test_sampler_pairs = 0");
        if (!c.bin_on_device)
            DIE("test_sampler_pairs = 1 with test_sampler_on_device = 0: the occupancies are made where each event batch is binned, on the device "
                "(test_sampler_on_device = 1); set test_sampler_pairs = 0");
        if (c.bin_fused)
            DIE("test_sampler_pairs = 1 with test_sampler_fused = 1: the fused pass never holds the batch of hadrons that is counted; set test_sampler_pairs = 0");
        is3d_pair_bins &b = c.pair_bins;
        b = is3d_pair_bins{2.0, 0.2, 3.0, 32, 32};
        double ny = 32.0, nphi = 32.0;
        p.optional("pairs_y_cut", &b.y_cut); p.optional("pairs_pt_min", &b.pT_min); p.optional("pairs_pt_max", &b.pT_max);
        p.optional("pairs_y_bins", &ny); p.optional("pairs_phi_bins", &nphi);
        const bool whole = ny >= 1.0 && ny <= 64.0 && ny == (double)(int)ny && nphi >= 4.0 && nphi <= 64.0 && nphi == (double)(int)nphi && (int)nphi % 4 == 0;
        b.n_y = whole ? (int32_t)ny : 0;
        b.n_phi = whole ? (int32_t)nphi : 0;
        // the library's own rule decides (the rapidity edges must come out finite and increasing): an empty list through is3d_pairs_list
        std::vector<int64_t> w(whole ? (size_t)(2 * (2 * b.n_y - 1) * b.n_phi + 1) : 3);
        const is3d_pair_hist probe{w.data(), w.data() + (w.size() - 1) / 2, w.data() + w.size() - 1};
        const int32_t none = -1;
        if (!whole || is3d_pairs_list(&b, 1, 1, &none, 1, 0, nullptr, &probe) != IS3D_OK)
            DIE("test_sampler_pairs = 1 with pairs_y_cut = %g, pairs_pT_min = %g, pairs_pT_max = %g, pairs_y_bins = %g, pairs_phi_bins = %g: the bins need "
                "pairs_y_cut > 0, pairs_pT_max > pairs_pT_min >= 0, 1 <= pairs_y_bins <= 64 and pairs_phi_bins a multiple of 4 in 4..64; set test_sampler_pairs = 0",
                b.y_cut, b.pT_min, b.pT_max, ny, nphi);
        for (const char *dir : {"results/pairs", "results/decayed/pairs"}) {
            if (dir[8] == 'd' && !c.bin_decayed) continue;
            struct stat sb;
            if (stat(dir, &sb) != 0 || !S_ISDIR(sb.st_mode))
                DIE("test_sampler_pairs = 1: the directory %s is missing; create it or set test_sampler_pairs = 0", dir);
        }
    }
    // test_sampler_hbt = 1: the HBT correlation functions and radii of the same hadrons under results/hbt/ (results/decayed/hbt/), refused in
    // the situations that refuse test_sampler_pairs, and for bad bins and missing directories
    if (c.hbt) {
        if (operation != 2)
            DIE("test_sampler_hbt = 1 with operation = %d: it correlates the sampler's hadrons (operation = 2); set test_sampler_hbt = 0", operation);
        if (need_test_sampler()) return IS3D_EINVAL;
        if (!c.test_sampler)
            DIE("test_sampler_hbt = 1 with test_sampler = 0: it writes the HBT correlations beside the test_sampler distributions; set test_sampler_hbt = 0");
        if (vah)
            DIE("test_sampler_hbt = 1 with mode = 2: it correlates the viscous-hydro sampler's hadrons; the anisotropic-hydro sampler has no such entry; set test_sampler_hbt = 0");
        if (wants_result)
            DIE("test_sampler_hbt = 1: the embedding entry returns the particle list, which this path never holds; set test_sampler_hbt = 0");
        if (!c.bin_on_device)
            DIE("test_sampler_hbt = 1 with test_sampler_on_device = 0: the pairs are formed where each event batch is binned, on the device "
                "(test_sampler_on_device = 1); set test_sampler_hbt = 0");
        if (c.bin_fused)
            DIE("test_sampler_hbt = 1 with test_sampler_fused = 1: the fused pass never holds the batch of hadrons that is paired; set test_sampler_hbt = 0");
        is3d_hbt_bins &b = c.hbt_bins;
        b = is3d_hbt_bins{0.5, 0.1, 1.5, 0.1, 0.9, 4, 0.1, 20, 0};
        double nk = 4.0, nq = 20.0;
        p.optional("hbt_y_cut", &b.y_cut); p.optional("hbt_pt_min", &b.pT_min); p.optional("hbt_pt_max", &b.pT_max);
        p.optional("hbt_kt_min", &b.kT_min); p.optional("hbt_kt_max", &b.kT_max); p.optional("hbt_q_max", &b.q_max);
        p.optional("hbt_kt_bins", &nk); p.optional("hbt_q_bins", &nq);
        const bool whole = nk >= 1.0 && nk <= 16.0 && nk == (double)(int)nk && nq >= 2.0 && nq <= 64.0 && nq == (double)(int)nq;
        b.n_kT = whole ? (int32_t)nk : 0;
        b.n_q = whole ? (int32_t)nq : 0;
        // the library's own rule decides: an empty list through is3d_hbt_list
        std::vector<int64_t> w(whole ? (size_t)(2 * b.n_kT * b.n_q * b.n_q * b.n_q + 1) : 3);
        const is3d_hbt_hist probe{w.data(), w.data() + (w.size() - 1) / 2, w.data() + w.size() - 1};
        const int32_t none = -1;
        if (!whole || is3d_hbt_list(&b, 1, 1, &none, 1, 0, nullptr, &probe) != IS3D_OK)
            DIE("test_sampler_hbt = 1 with hbt_y_cut = %g, hbt_pT_min = %g, hbt_pT_max = %g, hbt_kT_min = %g, hbt_kT_max = %g, hbt_kT_bins = %g, hbt_q_max = %g, "
                "hbt_q_bins = %g: the bins need hbt_y_cut > 0, hbt_pT_max > hbt_pT_min >= 0, hbt_kT_max > hbt_kT_min >= 0, 1 <= hbt_kT_bins <= 16, "
                "hbt_q_max > 0 and 2 <= hbt_q_bins <= 64; set test_sampler_hbt = 0",
                b.y_cut, b.pT_min, b.pT_max, b.kT_min, b.kT_max, nk, b.q_max, nq);
        for (const char *dir : {"results/hbt", "results/decayed/hbt"}) {
            if (dir[8] == 'd' && !c.bin_decayed) continue;
            struct stat sb;
            if (stat(dir, &sb) != 0 || !S_ISDIR(sb.st_mode))
                DIE("test_sampler_hbt = 1: the directory %s is missing; create it or set test_sampler_hbt = 0", dir);
        }
    }
    return IS3D_OK;
}

// Everything the run reads before it computes.  The structs the library takes point into the vectors and into the surface, which is the
// library's (is3d_surface_open) until this object goes: it is neither copied nor moved.
struct RunInputs {
    RunInputs() = default;
    RunInputs(const RunInputs &) = delete;
    ~RunInputs() { if (surf) is3d_surface_close(surf); }
    is3d_surface *surf = nullptr;              // NULL for the embedding entry's surface
    bool from_memory = false;
    int64_t n_cells = 0;
    const double *x = nullptr, *y = nullptr;   // the cells' positions: with the surface file, or the caller's (which may be NULL)
    is3d_cells cells{};                        // viscous hydro
    is3d_vah_cells vc{};                       // mode 2
    std::vector<int64_t> pdg_id, mcid;         // the whole particle list (the modified equilibrium needs it), then the chosen species
    std::vector<double> pdg_mass, pdg_g, pdg_b, pdg_s, mass, sign, deg, bar;
    std::vector<double> pT, pTw, phi, phiw, yv, yw, eta, etaw;
    std::vector<double> Tk, Bk, tab[10], vah_L, vah_aL, vah_c;
    is3d_species sp{};
    is3d_grid grid{};
    is3d_df_tables df{};
    is3d_vah_df_tables vt{};
    is3d_options opts{};
    double t_start = 0.0, t_loaded = 0.0;      // wall clock around the reads
};

// ---- surface (iS3D.cpp:90-134): the text file (one read + one parse) or its binary sidecar of an earlier run, or the caller's vectors ----
static int load_surface(const RunConfig &cfg, const MemSurface *mem, RunInputs &in, double avg[5])
{
    if (mem) {
        // iS3D.cpp:100-134: the surface comes from the caller's vectors, already in GeV / fm units (no hbar*c conversion)
        printf("Reading in freezeout surface from memory \n");
        in.from_memory = true;
        in.cells = *mem->cells;
        in.n_cells = in.cells.n_cells;
        in.x = mem->x; in.y = mem->y;
        const is3d_cells &m = in.cells;
        const double *need[18] = {m.T, m.P, m.E, m.tau, m.eta, m.ux, m.uy, m.un, m.dat, m.dax, m.day, m.dan, m.pixx, m.pixy, m.pixn, m.piyy, m.piyn, m.bulkPi};
        for (int a = 0; a < 18; a++)
            if (!need[a] && !(a == 4 && cfg.dimension == 2)) DIE("in-memory surface: a required array is NULL");
        if (in.n_cells > 0) surface_averages(&in.cells, avg);
    } else {
        // modes 0-7 except 2: the 23 cell arrays, x, y and the averages; mode 2: is3d_surface_read_vah's 32 arrays, x and y last, no averages
        const double *sa[32] = {nullptr};
        const int n_arrays = cfg.vah ? 32 : 25;
        if (is3d_surface_open("input/surface.dat", cfg.vah ? 2 : cfg.mode, cfg.vah ? 0 : cfg.include_baryon, cfg.vah ? 0 : cfg.include_diff, cfg.dimension, 1, &in.surf))
            DIE("%s", is3d_last_error());
        in.n_cells = is3d_surface_cells(in.surf);
        if (is3d_surface_arrays(in.surf, sa, n_arrays, cfg.vah ? nullptr : avg)) DIE("%s", is3d_last_error());
        // said BEFORE the spectra are computed: a user who did not expect the cache sees it while the run can still be stopped
        if (is3d_surface_from_sidecar(in.surf))
            printf("surface: %lld cells from the binary sidecar input/surface.dat.is3dcache (%sIS3D_NO_CACHE=1 to re-parse the text)\n", (long long)in.n_cells,
                   cfg.vah ? "" : "its key -- size, mtime, ctime, inode, content hash -- matches input/surface.dat; ");
        is3d_cells &c = in.cells;
        is3d_vah_cells &v = in.vc;   // both in the order of is3d_surface_arrays
        const double **cf[23] = {&c.T, &c.P, &c.E, &c.tau, &c.eta, &c.ux, &c.uy, &c.un, &c.dat, &c.dax, &c.day, &c.dan, &c.pixx, &c.pixy, &c.pixn, &c.piyy,
                                 &c.piyn, &c.bulkPi, &c.muB, &c.nB, &c.Vx, &c.Vy, &c.Vn};
        const double **vf[25] = {&v.tau, &v.eta, &v.ux, &v.uy, &v.un, &v.dat, &v.dax, &v.day, &v.dan, &v.T, &v.pitt, &v.pitx, &v.pity, &v.pitn, &v.pixx, &v.pixy,
                                 &v.pixn, &v.piyy, &v.piyn, &v.pinn, &v.bulkPi, &v.Wx, &v.Wy, &v.Lambda, &v.aL};
        for (int a = 0; a < (cfg.vah ? 25 : 23); a++) *(cfg.vah ? vf[a] : cf[a]) = sa[a];
        in.x = sa[n_arrays - 2]; in.y = sa[n_arrays - 1];
    }
    in.cells.n_cells = in.vc.n_cells = in.n_cells;
    return IS3D_OK;
}

// The reads, and the one write (the surface's averages), of a run before it computes; the warm-up is joined once the viscous-hydro inputs are in.
static int load_inputs(const RunConfig &cfg, const RunDevices &rd, int variant, const MemSurface *mem, std::thread &warm, RunInputs &in)
{
    double avg[5] = {0, 0, 0, 0, 0};
    if (int rc = load_surface(cfg, mem, in, avg)) return rc;
    if (!cfg.vah) {   // read_surf_VAH_PLMatch accumulates no averages (readindata.cpp:813-928)
        std::ofstream f("average_thermodynamic_quantities.dat", std::ios_base::out);
        f << std::setprecision(15) << avg[0] << "\n" << avg[1] << "\n" << avg[2] << "\n" << avg[3] << "\n" << avg[4];
    }
    // ---- species (iS3D.cpp:138-140, 156; emissionfunction.cpp:336-351, 1293-1307) ----
    int32_t npdg = 0;
    const auto pdg_read = (cfg.hrg_eos == 3) ? is3d_pdg_read_box : is3d_pdg_read;   // read_resonances: conventional | smash box (readindata.cpp:1687-1713)
    if (pdg_read(cfg.pdg_path, &npdg, nullptr, nullptr, nullptr, nullptr, nullptr, 0)) DIE("%s", is3d_last_error());
    in.pdg_id.resize(npdg); in.pdg_mass.resize(npdg); in.pdg_g.resize(npdg); in.pdg_b.resize(npdg); in.pdg_s.resize(npdg);
    if (pdg_read(cfg.pdg_path, &npdg, in.pdg_id.data(), in.pdg_mass.data(), in.pdg_g.data(), in.pdg_b.data(), in.pdg_s.data(), npdg)) DIE("%s", is3d_last_error());
    std::vector<double> chosen, dummy;
    if (read_table("PDG/chosen_particles.dat", chosen, dummy)) DIE("%s", is3d_last_error());
    for (double c : chosen) {
        const int id = (int)c;
        const auto at = std::find(in.pdg_id.begin(), in.pdg_id.end(), (int64_t)id);
        if (at == in.pdg_id.end()) DIE("chosen particle %d is not in %s", id, cfg.pdg_path);
        const size_t n = (size_t)(at - in.pdg_id.begin());
        in.mcid.push_back(in.pdg_id[n]); in.mass.push_back(in.pdg_mass[n]); in.sign.push_back(in.pdg_s[n]); in.deg.push_back(in.pdg_g[n]); in.bar.push_back(in.pdg_b[n]);
    }
    // ---- grids (iS3D.cpp:161-167) ----
    if (read_table("tables/pT_gauss_legendre_table.dat", in.pT, in.pTw) || read_table("tables/phi_gauss_legendre_table.dat", in.phi, in.phiw) ||
        read_table("tables/y_trapezoid_table_21pt.dat", in.yv, in.yw))
        DIE("%s", is3d_last_error());
    // the eta table: 241 points for the smooth spectra; the reference opens the 41-point one when it samples (iS3D.cpp:164-167) and never uses it
    // there (nor does the sampler here): a run directory made for either operation is accepted
    if (cfg.operation == 2) {
        // neither there: the reference fails on its missing table (readBlockData, arsenal.cpp:406-413) -- a mis-built run directory must not pass silently
        if (read_table("tables/eta/eta_trapezoid_table_41pt.dat", in.eta, in.etaw) && read_table("tables/eta/eta_trapezoid_table_241pt.dat", in.eta, in.etaw))
            DIE("operation 2 opens tables/eta/eta_trapezoid_table_41pt.dat (or tables/eta/eta_trapezoid_table_241pt.dat): neither can be read (%s)", is3d_last_error());
    } else if (read_table("tables/eta/eta_trapezoid_table_241pt.dat", in.eta, in.etaw))
        DIE("%s", is3d_last_error());
    // ---- delta-f coefficient tables (iS3D.cpp:144-145): include_baryon = 0: the mu_B = 0 rows; 1: the full (mu_B, T) grids (deltafReader.cpp:134) ----
    const char *names[10] = {"c0.dat", "c1.dat", "c2.dat", "c3.dat", "c4.dat", "F.dat", "G.dat", "betabulk.dat", "betaV.dat", "betapi.dat"};
    std::vector<double> &Tk = in.Tk, &Bk = in.Bk, *tab = in.tab;
    for (int t = 0; t < 10 && !cfg.vah; t++) {
        std::string p = cfg.df_dir + names[t];
        int32_t nT = 0, nB = 0;
        const bool spline_table = (t == 0 || t == 2 || t == 5 || t == 7 || t == 9);   // c0 c2 F betabulk betapi
        if (!cfg.include_baryon && !spline_table) continue;   // only the bilinear branch looks at c1 c3 c4 G betaV
        if (is3d_df_table_read_full(p.c_str(), &nT, &nB, nullptr, nullptr, nullptr, 0)) DIE("%s", is3d_last_error());
        Tk.resize(nT);
        if (!cfg.include_baryon) {
            Bk.assign(1, 0.0);
            tab[t].resize(nT);
            if (is3d_df_table_read(p.c_str(), &nT, Tk.data(), tab[t].data(), nT)) DIE("%s", is3d_last_error());
        } else {
            Bk.resize(nB);
            tab[t].resize((size_t)nT * nB);
            if (is3d_df_table_read_full(p.c_str(), &nT, &nB, Tk.data(), Bk.data(), tab[t].data(), (int64_t)tab[t].size())) DIE("%s", is3d_last_error());
        }
    }
    in.df = is3d_df_tables{(int32_t)Tk.size(), Tk.data(), (int32_t)Bk.size(), Bk.data(), tab[0].data(), tab[1].data(), tab[2].data(),
                           tab[3].data(), tab[4].data(), tab[5].data(), tab[6].data(), tab[7].data(), tab[8].data(), tab[9].data()};
    if (warm.joinable()) warm.join();
    in.t_loaded = now_s();
    printf("Total number of freezeout cells: %lld\nNumber of chosen particles: %zu\n", (long long)in.n_cells, in.mcid.size());
    in.sp = is3d_species{(int32_t)in.mcid.size(), in.mass.data(), in.sign.data(), in.deg.data(), in.bar.data()};
    in.grid = is3d_grid{(int32_t)in.pT.size(), in.pT.data(), (int32_t)in.phi.size(), in.phi.data(), (int32_t)in.yv.size(), in.yv.data(),
                        (int32_t)in.eta.size(), in.eta.data(), in.etaw.data()};
    is3d_options &o = in.opts;
    o.dimension = cfg.dimension; o.df_mode = cfg.df_mode; o.include_baryon = cfg.include_baryon;
    o.include_bulk_deltaf = cfg.include_bulk; o.include_shear_deltaf = cfg.include_shear; o.include_baryondiff_deltaf = cfg.include_diff;
    o.regulate_deltaf = cfg.regulate; o.outflow = cfg.outflow;
    o.accumulate = 0; o.device = rd.first(); o.kernel_variant = variant;
    // ---- mode 2: the deltaf_coefficients/vah tables (what src/cuda/deltafReader.cu:224-278 would have put into the surface) ----
    if (cfg.vah) {
        int32_t nL = 0, naL = 0;
        if (is3d_vah_df_read("deltaf_coefficients/vah", &nL, &naL, nullptr, nullptr, nullptr, 0)) DIE("%s", is3d_last_error());
        in.vah_L.resize((size_t)nL); in.vah_aL.resize((size_t)naL); in.vah_c.resize((size_t)5 * nL * naL);
        if (is3d_vah_df_read("deltaf_coefficients/vah", &nL, &naL, in.vah_L.data(), in.vah_aL.data(), in.vah_c.data(), (int64_t)in.vah_c.size())) DIE("%s", is3d_last_error());
        const size_t tn = (size_t)nL * naL;
        const double *c = in.vah_c.data();
        in.vt = is3d_vah_df_tables{nL, naL, in.vah_L.data(), in.vah_aL.data(), c, c + tn, c + 2 * tn, c + 3 * tn, c + 4 * tn};
    }
    return IS3D_OK;
}

// tables/gla_roots_weights_32_points.txt: the Gauss-Laguerre nodes, one row of n_pts per alpha
struct GaussLaguerre {
    const char *path = "tables/gla_roots_weights_32_points.txt";
    int32_t n_alpha = 0, n_pts = 0;
    std::vector<double> root, weight;
    const double *r(int alpha) const { return root.data() + (size_t)alpha * n_pts; }
    const double *w(int alpha) const { return weight.data() + (size_t)alpha * n_pts; }
};

// reads the table and points fq's alpha = 1 and alpha = 2 rules at it (emissionfunction.cpp:1309-1312)
static int read_gauss_laguerre(GaussLaguerre &g, is3d_feqmod_tables &fq)
{
    if (is3d_gla_read(g.path, &g.n_alpha, &g.n_pts, nullptr, nullptr, 0)) DIE("%s", is3d_last_error());
    if (g.n_alpha < 3) DIE("%s: needs alpha = 0, 1, 2", g.path);
    g.root.resize((size_t)g.n_alpha * g.n_pts); g.weight.resize(g.root.size());
    if (is3d_gla_read(g.path, &g.n_alpha, &g.n_pts, g.root.data(), g.weight.data(), (int64_t)g.root.size())) DIE("%s", is3d_last_error());
    fq.n_gla = g.n_pts;
    fq.root1 = g.r(1); fq.weight1 = g.w(1); fq.root2 = g.r(2); fq.weight2 = g.w(2);
    return IS3D_OK;
}

// Plasma::load_thermodynamic_averages: the first n numbers (T, E, P, muB, nB) of the averages file this run wrote, read back as text
static int read_averages(int n, double *v)
{
    FILE *tf = fopen("average_thermodynamic_quantities.dat", "r");
    int got = 0;
    while (tf && got < n && fscanf(tf, "%lf", &v[got]) == 1) got++;
    if (tf) fclose(tf);
    if (got != n) DIE("Error opening average thermodynamic file");
    return IS3D_OK;
}

// the rest of what the modified equilibrium takes: the whole particle list, deta_min, mass_pion0 and the surface's average temperature
static int fill_feqmod(const RunInputs &in, const RunParams &params, double T_avg, is3d_feqmod_tables &fq)
{
    if (params.required("deta_min", &fq.deta_min) || params.required("mass_pion0", &fq.mass_pion0)) return IS3D_EINVAL;
    fq.n_pdg = (int32_t)in.pdg_id.size(); fq.pdg_mass = in.pdg_mass.data(); fq.pdg_degeneracy = in.pdg_g.data(); fq.pdg_sign = in.pdg_s.data();
    fq.T_avg = T_avg;
    return IS3D_OK;
}

// the decay table of a particle list, owning its arrays
struct DecayTable {
    std::vector<int64_t> id, daughters;
    std::vector<double> mass, width, branch_ratio;
    std::vector<int32_t> stable, n_channels, n_part;
    is3d_decay_table view{};
};

static int read_decay_table(const char *path, DecayTable &t)
{
    int32_t nd = 0, nc = 0;
    if (is3d_pdg_read_decays(path, &nd, &nc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0)) DIE("%s", is3d_last_error());
    t.id.resize((size_t)nd); t.daughters.resize((size_t)nc * 5); t.mass.resize((size_t)nd); t.width.resize((size_t)nd); t.branch_ratio.resize((size_t)nc);
    t.stable.resize((size_t)nd); t.n_channels.resize((size_t)nd); t.n_part.resize((size_t)nc);
    if (is3d_pdg_read_decays(path, &nd, &nc, t.id.data(), t.mass.data(), t.width.data(), t.stable.data(), t.n_channels.data(), t.n_part.data(),
                             t.branch_ratio.data(), t.daughters.data(), nd, nc))
        DIE("%s", is3d_last_error());
    t.view = is3d_decay_table{nd, t.id.data(), t.mass.data(), t.width.data(), t.stable.data(), t.n_channels.data(), t.n_part.data(), t.branch_ratio.data(),
                              t.daughters.data()};
    return IS3D_OK;
}

// What goes back to the embedding caller (iS3D.cpp:178-184): the species, and the operation's own product -- the spectrum or the particle list.
static int copy_result(is3d_run_result *res, int operation, const RunInputs &in, const std::vector<double> *spectrum, const is3d_particle *list, int64_t count)
{
    if (!res) return IS3D_OK;
    const size_t S = (size_t)in.sp.n;
    res->operation = operation; res->n_species = in.sp.n;
    if (list) { res->n_particles = count; res->particles = (is3d_particle *)malloc(sizeof(is3d_particle) * (size_t)std::max<int64_t>(count, 1)); }
    if (spectrum) { res->n_spectrum = (int64_t)spectrum->size(); res->spectrum = (double *)malloc(sizeof(double) * spectrum->size()); }
    res->mc_id = (int64_t *)malloc(sizeof(int64_t) * S);
    res->mass = (double *)malloc(sizeof(double) * S);
    if ((list && !res->particles) || (spectrum && !res->spectrum) || !res->mc_id || !res->mass)
        return is3d::set_error(IS3D_ENOMEM, "out of memory%s", list ? " for the particle list" : spectrum ? " for the spectrum" : "");
    if (list) memcpy(res->particles, list, sizeof(is3d_particle) * (size_t)count);
    if (spectrum) memcpy(res->spectrum, spectrum->data(), sizeof(double) * spectrum->size());
    memcpy(res->mc_id, in.mcid.data(), sizeof(int64_t) * S);
    memcpy(res->mass, in.mass.data(), sizeof(double) * S);
    return IS3D_OK;
}

// the line of a stage that shards the cells over the run's devices; `how` says what becomes of the shards' results (NULL: the run's reduce of the spectrum)
static void print_devices(const RunDevices &rd, int64_t n_cells, const char *how)
{
    const int nd = rd.list.empty() ? is3d_device_count() : (int)rd.list.size();
    if (!how) how = rd.reduce == IS3D_REDUCE_RCCL ? ", RCCL all-reduce of the spectrum" : ", shard-ordered device sum of the spectrum";
    printf("devices: %d (cell-axis shards of ~%lld cells%s)\n", nd, (long long)((n_cells + nd - 1) / std::max(nd, 1)), nd > 1 ? how : "");
}

// a sampler run as set up from the parameter file and the tables, before anything is sampled
struct SamplerRun {
    is3d_sampler_inputs si{};
    is3d_sampler_test_bins bins{};
    GaussLaguerre gla;
    is3d_feqmod_tables fq{};
    std::vector<double> xs, ys;
    double oversample = 0.0, min_num_hadrons = 0.0, max_num_samples = 0.0, y_cut = 0.0, avg[5] = {0, 0, 0, 0, 0};
    double mean_yield = 0.0;   // calculate_total_yield's member mean_yield (:828), written by write_yield_list_toFile
};

// the sampler's lines after the sampling: what the momentum sampling accepted ...
static void print_sampling_efficiency(const RunConfig &cfg, const is3d_sampler_stats &ss)
{
    printf("\nMomentum sampling efficiency = %f %%\n", 100.0 * (double)ss.n_acceptances / (double)std::max<int64_t>(ss.n_momentum_samples, 1));
    if (cfg.feqmod) printf("feqmod breaks down for %lld cells\n", (long long)ss.n_cells_breakdown);
}

// ... and its closing lines, after the files are written; t_sampled and t_written are the clock at those two points
static void print_sampler_summary(const RunConfig &cfg, const RunInputs &in, const SamplerRun &s, const is3d_sampler_stats &ss, int64_t count, double t_sampled,
                                  double t_written)
{
    printf("particles: %lld in %d event(s); hadrons drawn %lld; cells skipped (u.dsigma <= 0): %lld\n", (long long)count, s.si.n_events,
           (long long)ss.n_hadrons_drawn, (long long)ss.n_cells_skipped);
    printf("device time: prep %.3f ms, count %.3f ms, fill %.3f ms; h2d %.3f ms\n", ss.ms_prep, ss.ms_count, ss.ms_fill, ss.ms_h2d);
    if (cfg.vah_bin_on_device || cfg.bin_fused) printf("binned where sampled on the device: ms_bin %.3f ms (sampling and binning, one pass), no particle workspace\n", ss.ms_bin);
    else if (cfg.bin_on_device) printf("binned on the device: ms_bin %.3f ms, particle workspace %lld bytes (one event batch)\n", ss.ms_bin, (long long)ss.particle_workspace_bytes);
    printf("wall: read %.3f s, sampling %.3f s, write %.3f s\n", in.t_loaded - in.t_start, t_sampled - in.t_loaded, t_written - t_sampled);
}

// ---- emissionfunction.cpp:205-222, 1309-1321, sampling_kernels.cpp:842-869: the sampler's parameters, cell positions, nodes and averages ----
static int setup_sampler(const RunConfig &cfg, const RunInputs &in, const RunParams &params, SamplerRun &s)
{
    double sampler_seed, fast, test_sampler, set_T, T_switch = 0.0;
    if (params.required("oversample", &s.oversample) || params.required("min_num_hadrons", &s.min_num_hadrons) ||
        params.required("max_num_samples", &s.max_num_samples) || params.required("sampler_seed", &sampler_seed) || params.required("y_cut", &s.y_cut) ||
        params.required("fast", &fast) || params.required("test_sampler", &test_sampler) || params.required("set_fo_temperature", &set_T))
        return IS3D_EINVAL;
    if ((int)set_T && params.required("t_switch", &T_switch)) return IS3D_EINVAL;
    is3d_sampler_test_bins &b = s.bins;
    if (cfg.test_sampler) {                                                   // emissionfunction.cpp:205-222
        double yb, eb, pb, tb, rb;
        if (params.required("y_bins", &yb) || params.required("eta_cut", &b.eta_cut) || params.required("eta_bins", &eb) ||
            params.required("pt_lower_cut", &b.pT_lower_cut) || params.required("pt_upper_cut", &b.pT_upper_cut) || params.required("pt_bins", &pb) ||
            params.required("tau_min", &b.tau_min) || params.required("tau_max", &b.tau_max) || params.required("tau_bins", &tb) ||
            params.required("r_min", &b.r_min) || params.required("r_max", &b.r_max) || params.required("r_bins", &rb))
            return IS3D_EINVAL;
        b.y_cut = s.y_cut;
        b.y_bins = (int)yb; b.eta_bins = (int)eb; b.pT_bins = (int)pb; b.tau_bins = (int)tb; b.r_bins = (int)rb;
    }
    // cell positions: columns 1, 2 of every supported surface format (readindata.cpp:343-346 etc.); zeros where the embedding caller gave none
    s.xs.assign((size_t)in.n_cells, 0.0); s.ys.assign((size_t)in.n_cells, 0.0);
    if (in.n_cells > 0 && in.x) s.xs.assign(in.x, in.x + in.n_cells);
    if (in.n_cells > 0 && in.y) s.ys.assign(in.y, in.y + in.n_cells);
    if (int rc = read_gauss_laguerre(s.gla, s.fq)) return rc;
    is3d_sampler_inputs &si = s.si;
    si.n_events = 1; si.n_gla = s.gla.n_pts;
    si.seed = sampler_seed < 0 ? (uint64_t)std::chrono::system_clock::now().time_since_epoch().count() : (uint64_t)sampler_seed;   // :842-844
    si.y_cut = s.y_cut; si.first_cell = 0; si.x = s.xs.data(); si.y = s.ys.data();
    si.root1 = s.gla.r(1); si.weight1 = s.gla.w(1);
    if (int rc = cfg.vah ? IS3D_OK : read_averages(4, s.avg)) return rc;   // (the mode-2 reader writes no averages and the VAH sampler takes none)
    const double T_avg = s.avg[0], muB_avg = s.avg[3];
    if (cfg.feqmod || (int)fast) {   // df_mode 3 / 4 and fast mode: emissionfunction.cpp:1309-1321, sampling_kernels.cpp:852-869
        if (int rc = fill_feqmod(in, params, T_avg, s.fq)) return rc;
        si.feqmod = &s.fq;
    }
    si.fast = (int)fast != 0;
    si.T_avg = T_avg; si.muB_avg = muB_avg;                                   // Plasma::baryon_chemical_potential, :858
    si.T_avg_switch = (int)set_T ? T_switch : T_avg;                          // :856
    if (si.fast) printf("Using fast mode: (Tavg, muBavg) = (%lf, %lf)\n", si.T_avg_switch, muB_avg);
    printf("iS3D Sampling Seed : %llu\n", (unsigned long long)si.seed);
    return IS3D_OK;
}

// ---- emissionfunction.cpp:1524-1533: the number of events, from the analytic mean yield where one sizes the run ----
static int size_sampler_run(const RunConfig &cfg, RunInputs &in, SamplerRun &s)
{
    is3d_sampler_inputs &si = s.si;
    const size_t n_pts = (size_t)s.gla.n_pts;
    const auto print_yield = [&](double N) { if (cfg.dimension == 2) printf("dN_dy ~ %lf\n\n", N / (2.0 * s.y_cut)); printf("%lf\n", N); };
    if ((int)s.oversample) {
        if (int rc = read_averages(5, s.avg)) return rc;   // calculate_total_yield also takes E, P and nB
        if (s.gla.n_alpha < 4) DIE("%s: the yield estimate needs alpha = 0, 1, 2, 3", s.gla.path);
        is3d_feqmod_tables fqy = s.fq;   // the alpha = 2 nodes enter every df_mode's bulk density (J20)
        is3d_sampler_inputs sy = si;
        sy.feqmod = &fqy;
        is3d_yield_inputs yi{s.avg[0], s.avg[1], s.avg[2], s.avg[3], s.avg[4], s.gla.root.data() + 3 * n_pts, s.gla.weight.data() + 3 * n_pts};
        double Ntotal = 0.0;
        printf("Total particle yield: ");
        int rc1 = is3d_total_yield(&in.cells, &in.sp, &in.df, &sy, &yi, &in.opts, &Ntotal, nullptr);
        if (rc1) DIE("is3d_total_yield failed (%d): %s", rc1, is3d_last_error());
        print_yield(Ntotal);
        s.mean_yield = Ntotal;
        Ntotal = (double)fabsf((float)Ntotal);                                  // "prevent overflow", :1528
        // Nevents = min((int)ceil(MIN_NUM_HADRONS / Ntotal), MAX_NUM_SAMPLES); at least one event is sampled here
        si.n_events = (int32_t)std::max(1.0, std::min(std::ceil(s.min_num_hadrons / Ntotal), (double)(int)s.max_num_samples));
    }
    if (cfg.vah) si.n_events = (int32_t)std::max(1.0, (double)(int)s.max_num_samples);   // without vah_oversample no mean yield sizes the run: MAX_NUM_SAMPLES events
    if (cfg.vah_oversample) {
        // the anisotropic-hydro mean yield on the first device of the run's list (opts.device), with the sampler's tables, nodes and y_cut
        double Ntotal = 0.0;
        printf("Total particle yield: ");
        const int rc1 = is3d_total_yield_vah(&in.vc, &in.sp, &in.vt, &si, &in.opts, &Ntotal, nullptr, nullptr);
        if (rc1) DIE("is3d_total_yield_vah failed (%d): %s", rc1, is3d_last_error());
        print_yield(Ntotal);
        if (!(Ntotal > 0.0))
            DIE("vah_oversample = 1: the linear delta-f has driven the mean yield of the surface non-positive (%g), which sizes no run (the residual bulk "
                "pressure is outside the range of the linear correction); set vah_oversample = 0 (max_num_samples events are sampled)", Ntotal);
        s.mean_yield = Ntotal;
        if (is3d_oversample_events(s.min_num_hadrons, Ntotal, (int32_t)s.max_num_samples, &si.n_events)) DIE("%s", is3d_last_error());
    }
    printf("Sampling %d event(s)\n", si.n_events);
    if (cfg.df_mode == 1) printf("Sampling particles with Grad 14 moment df...\n");                    // emissionfunction.cpp:1540-1541, :1602-1603
    if (cfg.df_mode == 2) printf("Sampling particles with Chapman Enskog df...\n");
    if (cfg.df_mode == 3) printf("Sampling particles with Mike's modified distribution...\n");
    if (cfg.df_mode == 4 && !cfg.vah) printf("Sampling particles with Jonah's modified distribution...\n");
    if (cfg.vah) printf("Sampling particles from vahydro (P_L matching) with df...\n");
    return IS3D_OK;
}

// test_sampler_on_device | test_sampler_fused | vah_sampler_on_device: one pass, every event batch binned on its device and dropped (anisotropic
// hydro and the fused route: every hadron binned where it is sampled); the integer histograms of the shards are added on the host
static int run_sampler_binned(const RunConfig &cfg, RunInputs &in, const RunDevices &rd, SamplerRun &s)
{
    const is3d_sampler_test_bins &bins = s.bins;
    const size_t S = (size_t)in.sp.n, plane = (size_t)IS3D_SAMPLER_VN_HARMONICS * S * bins.pT_bins;
    std::vector<int64_t> h_dy(S * bins.y_bins), h_de(S * bins.eta_bins), h_dp(S * bins.pT_bins), h_dt(S * bins.tau_bins), h_dr(S * bins.r_bins),
        h_vr(plane), h_vi(plane), h_yield((size_t)s.si.n_events);
    const is3d_sampler_hist hist{h_dy.data(), h_de.data(), h_dp.data(), h_dt.data(), h_dr.data(), h_vr.data(), h_vi.data(), h_yield.data()};
    is3d_sampler_stats ss{};
    int64_t count = 0;
    // anisotropic hydro and the fused route: a device list the user spelled out shards the cells; without one the first device samples alone
    const int rcb = cfg.bin_fused
                        ? (rd.named ? is3d_sample_fused_multi(&in.cells, &in.sp, &in.df, &s.si, &in.opts, rd.list.data(), rd.size(), &bins, &hist, &count, &ss)
                                    : is3d_sample_fused(&in.cells, &in.sp, &in.df, &s.si, &in.opts, &bins, &hist, &count, &ss))
                    : cfg.vah_bin_on_device
                        ? (rd.named ? is3d_sample_binned_vah_multi(&in.vc, &in.sp, &in.vt, &s.si, &in.opts, rd.list.data(), rd.size(), &bins, &hist, &count, &ss)
                                    : is3d_sample_binned_vah(&in.vc, &in.sp, &in.vt, &s.si, &in.opts, &bins, &hist, &count, &ss))
                        : is3d_sample_binned_multi(&in.cells, &in.sp, &in.df, &s.si, &in.opts, rd.data(), rd.size(), &bins, &hist, &count, &ss);
    if (rcb) DIE("%s failed (%d): %s", cfg.bin_fused ? "is3d_sample_fused" : cfg.vah_bin_on_device ? "is3d_sample_binned_vah" : "is3d_sample_binned", rcb, is3d_last_error());
    const double t_sampled = now_s();
    print_sampling_efficiency(cfg, ss);
    printf("Writing the binned sampler test distributions...\n");
    if (is3d_write_sampler_tests_binned("results", &bins, s.si.n_events, in.sp.n, in.mcid.data(), &hist, s.mean_yield)) DIE("%s", is3d_last_error());
    print_sampler_summary(cfg, in, s, ss, count, t_sampled, now_s());
    return IS3D_OK;
}

// decay_sampled_hadrons = 1: the thermal list decayed to stable particles, on the first device of the run's list; its species index the decay table
static int decay_sampled_list(const RunConfig &cfg, const RunInputs &in, const RunDevices &rd, const SamplerRun &s, const std::vector<is3d_particle> &plist, int64_t count)
{
    printf("Decaying the sampled hadrons to stable particles...\n");
    DecayTable tab;
    if (int rc = read_decay_table(cfg.pdg_path, tab)) return rc;
    const is3d_decay_mc_inputs mi{s.si.seed, 0, 0, rd.first()};
    is3d_decay_mc_stats ms{};
    int64_t n_final = 0;
    const double t4 = now_s();
    int rcd = is3d_decay_particles(&tab.view, in.sp.n, in.mcid.data(), &mi, count, plist.data(), nullptr, nullptr, 0, &n_final, &ms);
    std::vector<is3d_particle> decayed((size_t)std::max<int64_t>(n_final, 1));
    if (!rcd) rcd = is3d_decay_particles(&tab.view, in.sp.n, in.mcid.data(), &mi, count, plist.data(), decayed.data(), nullptr, n_final, &n_final, &ms);
    if (rcd) {
        const std::string msg = is3d_last_error();
        DIE("is3d_decay_particles failed (%d): %s", rcd, msg.c_str());
    }
    if (is3d_write_particle_list_osc("results/particle_list_osc_decayed.dat", s.si.n_events, n_final, decayed.data(), tab.id.data())) DIE("%s", is3d_last_error());
    printf("decays: %lld primaries, %lld decays, %lld final particles (%lld without an open channel), %lld phase-space proposals (%lld exhausted); "
           "device time: count %.3f ms, fill %.3f ms; wall %.3f s\n", (long long)ms.n_primaries, (long long)ms.n_decays, (long long)ms.n_final,
           (long long)ms.n_stuck, (long long)ms.n_trials, (long long)ms.n_exhausted, ms.ms_count, ms.ms_fill, now_s() - t4);
    return IS3D_OK;
}

// test_sampler_decayed = 1: the run of test_sampler_on_device on the first device of the run's list, every event batch binned as there and then
// decayed and binned again (is3d_sample_decayed_binned); results/ as without the key, results/decayed/ the same files for the chosen species
// that are stable in the decay table, in chosen order
static int run_sampler_decayed_binned(const RunConfig &cfg, RunInputs &in, const RunDevices &rd, SamplerRun &s)
{
    static const char *const subdirs[5] = {"dN_dy", "dN_deta", "momentum_distribution", "vn", "spacetime_distribution"};
    for (const char *d : subdirs) {
        const std::string path = std::string("results/decayed/") + d;
        struct stat sb;
        if (stat(path.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode))
            DIE("test_sampler_decayed = 1: the directory %s is missing (results/decayed/ needs the five directories of results/); create it or set test_sampler_decayed = 0",
                path.c_str());
    }
    DecayTable tab;
    if (int rc = read_decay_table(cfg.pdg_path, tab)) return rc;
    std::vector<int32_t> slot((size_t)tab.view.n, -1);
    std::vector<int64_t> slot_id;
    for (int ip = 0; ip < in.sp.n; ip++)
        for (int32_t e = 0; e < tab.view.n; e++)
            if (tab.id[(size_t)e] == in.mcid[(size_t)ip]) {          // first match, as the library's chosen -> entry map
                if (tab.stable[(size_t)e] && slot[(size_t)e] < 0) { slot[(size_t)e] = (int32_t)slot_id.size(); slot_id.push_back(tab.id[(size_t)e]); }
                break;
            }
    if (slot_id.empty())
        DIE("test_sampler_decayed = 1: no chosen particle is stable in %s, so nothing would be binned; set test_sampler_decayed = 0", cfg.pdg_path);
    const is3d_sampler_test_bins &bins = s.bins;
    const auto sizes = [&bins](size_t S) {
        return std::vector<size_t>{S * bins.y_bins, S * bins.eta_bins, S * bins.pT_bins, S * bins.tau_bins, S * bins.r_bins,
                                   (size_t)IS3D_SAMPLER_VN_HARMONICS * S * bins.pT_bins, (size_t)IS3D_SAMPLER_VN_HARMONICS * S * bins.pT_bins};
    };
    std::vector<std::vector<int64_t>> ht, hd;
    for (size_t n : sizes((size_t)in.sp.n)) ht.emplace_back(n);
    for (size_t n : sizes(slot_id.size())) hd.emplace_back(n);
    std::vector<int64_t> yt((size_t)s.si.n_events), yd((size_t)s.si.n_events);
    const is3d_sampler_hist hist{ht[0].data(), ht[1].data(), ht[2].data(), ht[3].data(), ht[4].data(), ht[5].data(), ht[6].data(), yt.data()};
    const is3d_sampler_hist hist_d{hd[0].data(), hd[1].data(), hd[2].data(), hd[3].data(), hd[4].data(), hd[5].data(), hd[6].data(), yd.data()};
    is3d_sampler_stats ss{};
    is3d_decay_mc_stats ms{};
    int64_t count = 0, n_final = 0, n_unbinned = 0;
    is3d_options opts = in.opts;
    opts.device = rd.first();
    const int rcb = is3d_sample_decayed_binned(&in.cells, &in.sp, &in.df, &s.si, &opts, &bins, &hist, &tab.view, in.mcid.data(), slot.data(),
                                               (int32_t)slot_id.size(), s.si.seed, 0, &hist_d, &count, &n_final, &n_unbinned, &ss, &ms);
    if (rcb) DIE("is3d_sample_decayed_binned failed (%d): %s", rcb, is3d_last_error());
    const double t_sampled = now_s();
    print_sampling_efficiency(cfg, ss);
    printf("Writing the binned sampler test distributions...\n");
    if (is3d_write_sampler_tests_binned("results", &bins, s.si.n_events, in.sp.n, in.mcid.data(), &hist, s.mean_yield)) DIE("%s", is3d_last_error());
    printf("Writing the binned sampler test distributions of the decayed hadrons (%d species)...\n", (int)slot_id.size());
    if (is3d_write_sampler_tests_binned("results/decayed", &bins, s.si.n_events, (int32_t)slot_id.size(), slot_id.data(), &hist_d, s.mean_yield))
        DIE("%s", is3d_last_error());
    printf("decayed and binned on the device: n_final %lld, n_unbinned %lld, n_decays %lld, n_stuck %lld, n_exhausted %lld, ms_bin %.3f ms\n",
           (long long)n_final, (long long)n_unbinned, (long long)ms.n_decays, (long long)ms.n_stuck, (long long)ms.n_exhausted, ms.ms_bin);
    print_sampler_summary(cfg, in, s, ss, count, t_sampled, now_s());
    return IS3D_OK;
}

// labels and the slot of an mc_id, in the order the ids come: a slot of its own for each id of `named`, one further slot "other" for the rest,
// made when the first such id comes
struct NamedSlots {
    std::vector<int64_t> named;
    std::vector<std::string> label;
    int other = -1;
    int of(int64_t id)
    {
        for (int64_t k : named)
            if (id == k) {
                const std::string l = std::to_string((long long)id);
                for (size_t j = 0; j < label.size(); j++)
                    if (label[j] == l) return (int)j;
                label.push_back(l);
                return (int)label.size() - 1;
            }
        if (other < 0) { other = (int)label.size(); label.push_back("other"); }
        return other;
    }
};
// the slot maps of a run: thermal over the chosen species; decayed (table read when asked) over the chosen species that are stable in the table
static int named_slot_maps(const RunConfig &cfg, const RunInputs &in, NamedSlots &th, NamedSlots &de, std::vector<int32_t> &slot,
                           std::vector<int32_t> &slot_d, DecayTable &tab)
{
    slot.assign((size_t)in.sp.n, -1);
    for (int ip = 0; ip < in.sp.n; ip++) slot[(size_t)ip] = th.of(in.mcid[(size_t)ip]);
    if (cfg.bin_decayed) {
        if (int rc = read_decay_table(cfg.pdg_path, tab)) return rc;
        slot_d.assign((size_t)tab.view.n, -1);
        for (int ip = 0; ip < in.sp.n; ip++)
            for (int32_t e = 0; e < tab.view.n; e++)
                if (tab.id[(size_t)e] == in.mcid[(size_t)ip]) {          // first match, as the library's chosen -> entry map
                    if (tab.stable[(size_t)e] && slot_d[(size_t)e] < 0) slot_d[(size_t)e] = de.of(tab.id[(size_t)e]);
                    break;
                }
    }
    return IS3D_OK;
}

// test_sampler_flow = 1: after the binned run has written its files, the sampler runs once more on the first device of the run's list with the
// same seed (the same hadrons: every stream is counter-based) and each event batch goes through cf_sampler_flow -- and, with
// test_sampler_decayed = 1, through cf_decay_mc_flow with the decay seed of that run.  Slots: pi+, K+, p (211, 321, 2212) where chosen, everything
// else in one further slot; "all" is written from the merge.  Decayed: the same rule over the chosen species that are stable in the table.
static int run_sampler_flow(const RunConfig &cfg, RunInputs &in, const RunDevices &rd, SamplerRun &s)
{
    NamedSlots th{{211, 321, 2212}}, de{{211, 321, 2212}};
    std::vector<int32_t> slot, slot_d;
    DecayTable tab;
    if (int rc = named_slot_maps(cfg, in, th, de, slot, slot_d, tab)) return rc;
    const bool decayed = cfg.bin_decayed && !de.label.empty();
    const int32_t E = s.si.n_events, S = (int32_t)th.label.size(), Sd = (int32_t)de.label.size();
    struct Block {
        std::vector<int64_t> M, re, im;
        is3d_flow_records view;
        Block(int32_t events, int32_t slots)
            : M((size_t)events * slots * 3), re(M.size() * IS3D_FLOW_HARMONICS), im(re.size()), view{M.data(), re.data(), im.data()} {}
    } rt(E, S), rdec(E, std::max(Sd, 1)), all_t(E, 1), all_d(E, 1);
    is3d_sampler_stats ss{};
    is3d_decay_mc_stats ms{};
    int64_t count = 0, n_final = 0, n_unbinned = 0;
    is3d_options opts = in.opts;
    opts.device = rd.first();
    const int rcf = is3d_sample_flow(&in.cells, &in.sp, &in.df, &s.si, &opts, &cfg.flow_cuts, slot.data(), S, &rt.view, decayed ? &tab.view : nullptr,
                                     in.mcid.data(), slot_d.data(), Sd, s.si.seed, 0, &rdec.view, &count, &n_final, &n_unbinned, &ss, &ms);
    if (rcf) DIE("is3d_sample_flow failed (%d): %s", rcf, is3d_last_error());
    const auto write = [E](const char *dir, Block &b, Block &all, const std::vector<std::string> &label) {
        std::vector<const char *> names;
        for (const std::string &l : label) names.push_back(l.c_str());
        const std::vector<int32_t> group(label.size(), 0);
        const char *const all_name = "all";
        if (is3d_write_flow(dir, &b.view, E, (int32_t)label.size(), names.data())) return 1;
        if (is3d_flow_merge(&b.view, E, (int32_t)label.size(), group.data(), 1, &all.view)) return 1;
        return is3d_write_flow(dir, &all.view, E, 1, &all_name) ? 1 : 0;
    };
    printf("Writing the flow cumulants and multiplicities (%d slots and all)...\n", (int)S);
    if (write("results", rt, all_t, th.label)) DIE("%s", is3d_last_error());
    if (decayed) {
        printf("Writing the flow cumulants and multiplicities of the decayed hadrons (%d slots and all)...\n", (int)Sd);
        if (write("results/decayed", rdec, all_d, de.label)) DIE("%s", is3d_last_error());
    }
    printf("flow records on the device: %lld hadrons, ms_bin %.3f ms", (long long)count, ss.ms_bin);
    if (decayed) printf("; decayed: n_final %lld, n_unbinned %lld, ms_bin %.3f ms", (long long)n_final, (long long)n_unbinned, ms.ms_bin);
    printf("\n");
    return IS3D_OK;
}

// test_sampler_flow_diff = 1: as run_sampler_flow, once more with the same seed, each event batch through cf_sampler_flow_diff (and
// cf_decay_mc_flow on the differential sink) with the slots of run_sampler_flow and the pT bins of the config; the cuts are those of the
// flow run with pT_max = flow_diff_pt_max.  differential_<label>.dat per slot and, from the integer sums over the slots, for "all"; the
// reference of every file is all slots over all bins.
static int run_sampler_flow_diff(const RunConfig &cfg, RunInputs &in, const RunDevices &rd, SamplerRun &s)
{
    NamedSlots th{{211, 321, 2212}}, de{{211, 321, 2212}};
    std::vector<int32_t> slot, slot_d;
    DecayTable tab;
    if (int rc = named_slot_maps(cfg, in, th, de, slot, slot_d, tab)) return rc;
    const bool decayed = cfg.bin_decayed && !de.label.empty();
    const int32_t E = s.si.n_events, S = (int32_t)th.label.size(), Sd = (int32_t)de.label.size(), B = (int32_t)cfg.flow_diff_edges.size() - 1;
    struct Block {
        std::vector<int64_t> m, re, im;
        is3d_flow_diff_records view;
        Block(int32_t events, int32_t slots, int32_t bins)
            : m((size_t)events * slots * bins * 3), re(m.size() * IS3D_FLOW_HARMONICS), im(re.size()), view{m.data(), re.data(), im.data()} {}
    } rt(E, S, B), rdec(E, std::max(Sd, 1), B), all(E, 1, B);
    is3d_flow_cuts cuts = cfg.flow_cuts;
    cuts.pT_max = cfg.flow_diff_edges.back();
    is3d_sampler_stats ss{};
    is3d_decay_mc_stats ms{};
    int64_t count = 0, n_final = 0, n_unbinned = 0;
    is3d_options opts = in.opts;
    opts.device = rd.first();
    const int rcf = is3d_sample_flow_diff(&in.cells, &in.sp, &in.df, &s.si, &opts, &cuts, B, cfg.flow_diff_edges.data(), slot.data(), S, &rt.view,
                                          decayed ? &tab.view : nullptr, in.mcid.data(), slot_d.data(), Sd, s.si.seed, 0, &rdec.view, &count, &n_final,
                                          &n_unbinned, &ss, &ms);
    if (rcf) DIE("is3d_sample_flow_diff failed (%d): %s", rcf, is3d_last_error());
    const auto write = [&](const char *dir, Block &b, const std::vector<std::string> &label) {
        std::vector<const char *> names;
        for (const std::string &l : label) names.push_back(l.c_str());
        const int32_t n = (int32_t)label.size();
        const std::vector<int32_t> every((size_t)n, 1);
        if (is3d_write_flow_diff(dir, &b.view, E, n, B, cfg.flow_diff_edges.data(), every.data(), 0, B, names.data())) return 1;
        // "all": the integer sums over the slots, per (event, bin, region)
        const size_t rec = (size_t)B * 3;
        for (std::vector<int64_t> Block::*a : {&Block::m, &Block::re, &Block::im}) {
            const size_t w = rec * (a == &Block::m ? 1 : IS3D_FLOW_HARMONICS);
            std::fill((all.*a).begin(), (all.*a).end(), 0);
            for (int32_t e = 0; e < E; e++)
                for (int32_t k = 0; k < n; k++)
                    for (size_t j = 0; j < w; j++) (all.*a)[(size_t)e * w + j] += (b.*a)[((size_t)e * n + (size_t)k) * w + j];
        }
        const char *const all_name = "all";
        const int32_t one = 1;
        return is3d_write_flow_diff(dir, &all.view, E, 1, B, cfg.flow_diff_edges.data(), &one, 0, B, &all_name) ? 1 : 0;
    };
    printf("Writing the differential flow (%d slots and all, %d pT bins)...\n", (int)S, (int)B);
    if (write("results", rt, th.label)) DIE("%s", is3d_last_error());
    if (decayed) {
        printf("Writing the differential flow of the decayed hadrons (%d slots and all, %d pT bins)...\n", (int)Sd, (int)B);
        if (write("results/decayed", rdec, de.label)) DIE("%s", is3d_last_error());
    }
    printf("differential flow records on the device: %lld hadrons, ms_bin %.3f ms", (long long)count, ss.ms_bin);
    if (decayed) printf("; decayed: n_final %lld, n_unbinned %lld, ms_bin %.3f ms", (long long)n_final, (long long)n_unbinned, ms.ms_bin);
    printf("\n");
    return IS3D_OK;
}

// test_sampler_pairs = 1: as run_sampler_flow, the sampler runs once more with the same seed and each event batch goes through cf_pair_cells
// -- and, with test_sampler_decayed = 1, through cf_decay_mc_pairs -- into occupancies that cf_pair_correlate turns into the same-event and
// mixed-event histograms after the last batch.  Slots: pi+, pi-, K+, p (211, -211, 321, 2212) where chosen, everything else in one further slot.
static int run_sampler_pairs(const RunConfig &cfg, RunInputs &in, const RunDevices &rd, SamplerRun &s)
{
    NamedSlots th{{211, -211, 321, 2212}}, de{{211, -211, 321, 2212}};
    std::vector<int32_t> slot, slot_d;
    DecayTable tab;
    if (int rc = named_slot_maps(cfg, in, th, de, slot, slot_d, tab)) return rc;
    const bool decayed = cfg.bin_decayed && !de.label.empty();
    const int32_t E = s.si.n_events, S = (int32_t)th.label.size(), Sd = (int32_t)de.label.size();
    const is3d_pair_bins &b = cfg.pair_bins;
    struct Block {
        std::vector<int64_t> same, mixed, M;
        is3d_pair_hist view;
        Block(const is3d_pair_bins &b, int32_t events, int32_t slots)
            : same((size_t)slots * (slots + 1) / 2 * (2 * b.n_y - 1) * b.n_phi), mixed(same.size()), M((size_t)events * slots),
              view{same.data(), mixed.data(), M.data()} {}
    } ht(b, E, S), hd(b, E, std::max(Sd, 1));
    is3d_sampler_stats ss{};
    is3d_decay_mc_stats ms{};
    int64_t count = 0, n_final = 0, n_unbinned = 0;
    is3d_options opts = in.opts;
    opts.device = rd.first();
    const int rcp = is3d_sample_pairs(&in.cells, &in.sp, &in.df, &s.si, &opts, &b, slot.data(), S, &ht.view, decayed ? &tab.view : nullptr,
                                      in.mcid.data(), slot_d.data(), Sd, s.si.seed, 0, &hd.view, &count, &n_final, &n_unbinned, &ss, &ms);
    if (rcp) DIE("is3d_sample_pairs failed (%d): %s", rcp, is3d_last_error());
    const auto write = [&b](const char *dir, Block &h, const std::vector<std::string> &label) {
        std::vector<const char *> names;
        for (const std::string &l : label) names.push_back(l.c_str());
        return is3d_write_pairs(dir, &b, &h.view, (int32_t)label.size(), names.data());
    };
    printf("Writing the pair correlations (%d slots, %d classes)...\n", (int)S, (int)(S * (S + 1) / 2));
    if (write("results", ht, th.label)) DIE("%s", is3d_last_error());
    if (decayed) {
        printf("Writing the pair correlations of the decayed hadrons (%d slots, %d classes)...\n", (int)Sd, (int)(Sd * (Sd + 1) / 2));
        if (write("results/decayed", hd, de.label)) DIE("%s", is3d_last_error());
    }
    printf("pair correlations on the device: %lld hadrons, ms_bin %.3f ms", (long long)count, ss.ms_bin);
    if (decayed) printf("; decayed: n_final %lld, n_unbinned %lld, ms_bin %.3f ms", (long long)n_final, (long long)n_unbinned, ms.ms_bin);
    printf("\n");
    return IS3D_OK;
}

// test_sampler_hbt = 1: as run_sampler_pairs, the sampler runs once more with the same seed and each event batch is selected and paired on
// the device (cf_hbt_select, cf_hbt_pairs) -- and, with test_sampler_decayed = 1, decayed with lifetimes (the halo of long-lived resonances is
// what lowers lambda) into records that are paired.  Slots: pi+, pi-, K+, K- (211, -211, 321, -321) where chosen; every other species is dropped.
static int run_sampler_hbt(const RunConfig &cfg, RunInputs &in, const RunDevices &rd, SamplerRun &s)
{
    static const int64_t named[4] = {211, -211, 321, -321};
    struct Slots {
        std::vector<std::string> label;
        int of(int64_t id)
        {
            for (int64_t k : named)
                if (id == k) {
                    const std::string l = std::to_string((long long)id);
                    for (size_t j = 0; j < label.size(); j++)
                        if (label[j] == l) return (int)j;
                    label.push_back(l);
                    return (int)label.size() - 1;
                }
            return -1;
        }
    } th, de;
    std::vector<int32_t> slot((size_t)in.sp.n), slot_d;
    for (int ip = 0; ip < in.sp.n; ip++) slot[(size_t)ip] = th.of(in.mcid[(size_t)ip]);
    DecayTable tab;
    if (cfg.bin_decayed) {
        if (int rc = read_decay_table(cfg.pdg_path, tab)) return rc;
        slot_d.assign((size_t)tab.view.n, -1);
        for (int ip = 0; ip < in.sp.n; ip++)
            for (int e = 0; e < tab.view.n; e++)
                if (tab.view.mc_id[e] == in.mcid[(size_t)ip]) {
                    if (tab.view.stable[e]) slot_d[(size_t)e] = de.of(in.mcid[(size_t)ip]);
                    break;
                }
    }
    if (th.label.empty()) {
        printf("HBT correlations: none of 211, -211, 321, -321 is chosen; nothing written\n");
        return IS3D_OK;
    }
    const bool decayed = cfg.bin_decayed && !de.label.empty();
    const int32_t E = s.si.n_events, S = (int32_t)th.label.size(), Sd = (int32_t)de.label.size();
    const is3d_hbt_bins &b = cfg.hbt_bins;
    struct Block {
        std::vector<int64_t> num, den, M;
        is3d_hbt_hist view;
        Block(const is3d_hbt_bins &b, int32_t events, int32_t slots)
            : num((size_t)slots * b.n_kT * b.n_q * b.n_q * b.n_q), den(num.size()), M((size_t)events * slots), view{num.data(), den.data(), M.data()} {}
    } ht(b, E, S), hd(b, E, std::max(Sd, 1));
    is3d_sampler_stats ss{};
    is3d_decay_mc_stats ms{};
    int64_t count = 0, n_final = 0, n_unbinned = 0;
    is3d_options opts = in.opts;
    opts.device = rd.first();
    const int rcp = is3d_sample_hbt(&in.cells, &in.sp, &in.df, &s.si, &opts, &b, slot.data(), S, &ht.view, decayed ? &tab.view : nullptr,
                                    in.mcid.data(), slot_d.data(), Sd, s.si.seed, 1, &hd.view, &count, &n_final, &n_unbinned, &ss, &ms);
    if (rcp) DIE("is3d_sample_hbt failed (%d): %s", rcp, is3d_last_error());
    const auto write = [&b](const char *dir, Block &h, const std::vector<std::string> &label) {
        std::vector<const char *> names;
        for (const std::string &l : label) names.push_back(l.c_str());
        return is3d_write_hbt(dir, &b, &h.view, (int32_t)label.size(), names.data(), 20, 0.05);
    };
    printf("Writing the HBT correlations (%d slots, %d kT bins)...\n", (int)S, (int)b.n_kT);
    if (write("results", ht, th.label)) DIE("%s", is3d_last_error());
    if (decayed) {
        printf("Writing the HBT correlations of the decayed hadrons (%d slots, %d kT bins)...\n", (int)Sd, (int)b.n_kT);
        if (write("results/decayed", hd, de.label)) DIE("%s", is3d_last_error());
    }
    printf("HBT correlations on the device: %lld hadrons, ms_bin %.3f ms", (long long)count, ss.ms_bin);
    if (decayed) printf("; decayed: n_final %lld, n_unbinned %lld, ms_bin %.3f ms", (long long)n_final, (long long)n_unbinned, ms.ms_bin);
    printf("\n");
    return IS3D_OK;
}

// ---- operation 2 (emissionfunction.cpp:1522-1554): number of events, sampling, the OSCAR list or the binned test distributions ----
static int run_sampler(const RunConfig &cfg, RunInputs &in, const RunDevices &rd, RunParams &params, is3d_run_result *res)
{
    SamplerRun s;
    if (int rc = setup_sampler(cfg, in, params, s)) return rc;
    if (int rc = size_sampler_run(cfg, in, s)) return rc;
    if (cfg.bin_decayed || cfg.bin_on_device || cfg.vah_bin_on_device || cfg.bin_fused) {
        if (int rc = cfg.bin_decayed ? run_sampler_decayed_binned(cfg, in, rd, s) : run_sampler_binned(cfg, in, rd, s)) return rc;
        if (cfg.flow)
            if (int rc = run_sampler_flow(cfg, in, rd, s)) return rc;
        if (cfg.flow_diff)
            if (int rc = run_sampler_flow_diff(cfg, in, rd, s)) return rc;
        if (cfg.pairs)
            if (int rc = run_sampler_pairs(cfg, in, rd, s)) return rc;
        return cfg.hbt ? run_sampler_hbt(cfg, in, rd, s) : IS3D_OK;
    }
    // count, then fill a list of that size: the viscous-hydro sampler, or (mode 2) the anisotropic-hydro one on the mode-2 cells and tables
    is3d_sampler_stats ss{};
    int64_t count = 0;
    auto sample = [&](is3d_particle *list, int64_t capacity) {
        if (cfg.vah) return is3d_sample_particles_vah_multi(&in.vc, &in.sp, &in.vt, &s.si, &in.opts, rd.data(), rd.size(), list, capacity, &count, &ss);
        return is3d_sample_particles_multi(&in.cells, &in.sp, &in.df, &s.si, &in.opts, rd.data(), rd.size(), list, capacity, &count, &ss);
    };
    const char *sampler_name = cfg.vah ? "is3d_sample_particles_vah" : "is3d_sample_particles";
    int rc2 = sample(nullptr, 0);
    if (rc2) DIE("%s failed (%d): %s", sampler_name, rc2, is3d_last_error());
    std::vector<is3d_particle> plist((size_t)std::max<int64_t>(count, 1));
    rc2 = sample(plist.data(), count);
    if (rc2) DIE("%s failed (%d): %s", sampler_name, rc2, is3d_last_error());
    const double t_sampled = now_s();
    print_sampling_efficiency(cfg, ss);
    if (cfg.test_sampler) {                                                   // emissionfunction.cpp:1545-1554
        printf("Writing the binned sampler test distributions...\n");
        if (is3d_write_sampler_tests("results", &s.bins, s.si.n_events, in.sp.n, in.mcid.data(), count, plist.data(), s.mean_yield)) DIE("%s", is3d_last_error());
    } else {
        printf("Writing sampled particles list to OSCAR File...\n");
        if (is3d_write_particle_list_osc("results/particle_list_osc.dat", s.si.n_events, count, plist.data(), in.mcid.data())) DIE("%s", is3d_last_error());
    }
    if (int rc = cfg.decay_sampled ? decay_sampled_list(cfg, in, rd, s, plist, count) : IS3D_OK) return rc;
    print_sampler_summary(cfg, in, s, ss, count, t_sampled, now_s());
    if (res) res->n_events = s.si.n_events;   // iS3D.cpp:178-184: the event lists go back to the caller (final_particles_)
    return copy_result(res, 2, in, nullptr, plist.data(), count);
}

// ---- operation 0 (emissionfunction.cpp:1510-1516 -> calculate_dN_dX, smooth_kernels.cpp:1000-1446) ----
static int run_spacetime(const RunConfig &cfg, RunInputs &in, const RunDevices &rd, RunParams &params, is3d_run_result *res)
{
    double t0b, t1b, tb, r0b, r1b, rb;
    if (params.required("tau_min", &t0b) || params.required("tau_max", &t1b) || params.required("tau_bins", &tb) || params.required("r_min", &r0b) ||
        params.required("r_max", &r1b) || params.required("r_bins", &rb))
        return IS3D_EINVAL;
    is3d_spacetime_bins bins{t0b, t1b, r0b, r1b, (int32_t)tb, (int32_t)rb};
    const double *xp = in.x, *yp = in.y;
    std::vector<double> zero(1, 0.0);
    if (in.n_cells == 0) xp = yp = zero.data();
    const int S = in.sp.n, n_eta_eff = cfg.dimension == 3 ? 1 : (int)in.eta.size();
    std::vector<double> o_dy((size_t)S), o_t((size_t)S * bins.tau_bins), o_r((size_t)S * bins.r_bins),
        o_tr((size_t)S * bins.tau_bins * bins.r_bins), o_eta((size_t)S * n_eta_eff);
    is3d_spacetime_out out{o_dy.data(), o_t.data(), o_r.data(), o_tr.data(), o_eta.data(), nullptr};
    for (int ip = 0; ip < S; ip++) printf("Starting spacetime distribution %lld\n", (long long)in.mcid[ip]);   // :1100
    is3d_spacetime_stats sst{};
    int rc0;
    if (cfg.vah) {
        // anisotropic hydro: the first device of the run's list computes alone (opts.device), whatever the list holds
        printf("computing spacetime distributions from vahydro (P_L matching) with df...\n");
        rc0 = is3d_spacetime_distributions_vah(&in.vc, xp, yp, &in.sp, &in.grid, in.pTw.data(), in.phiw.data(), &in.vt, &in.opts, &bins, &out, &sst);
    } else {
        // the per-cell stage on cell-axis shards over the run's devices, one bin stage on the first (is3d_spacetime_distributions_multi)
        rc0 = is3d_spacetime_distributions_multi(&in.cells, xp, yp, &in.sp, &in.grid, in.pTw.data(), in.phiw.data(), &in.df, nullptr, &in.opts, rd.data(),
                                                 rd.size(), &bins, &out, &sst, nullptr);
        print_devices(rd, in.n_cells, ", one bin stage over the assembled per-cell values");
    }
    if (rc0) {
        const std::string msg = is3d_last_error();
        DIE("%s failed (%d): %s", cfg.vah ? "is3d_spacetime_distributions_vah" : "is3d_spacetime_distributions_multi", rc0, msg.c_str());
    }
    // the reference prints an error line per cell with a negative bin index (:1391-1392); one line with the counts here
    if (sst.n_tau_negative || sst.n_r_negative)
        printf("Error: %lld cells with a negative tau bin index, %lld with a negative r bin index. Adjust the tau_min / r_min parameters\n",
               (long long)sst.n_tau_negative, (long long)sst.n_r_negative);
    // 3+1D: the single eta point is eta_fo of the surface's last cell (etaValues[0], assigned at :1155 before the skip test)
    const double *eta_fo = cfg.vah ? in.vc.eta : in.cells.eta;
    std::vector<double> eta_vals = cfg.dimension == 3 ? std::vector<double>(1, in.n_cells > 0 ? eta_fo[in.n_cells - 1] : 0.0) : in.eta;
    if (is3d_write_spacetime("results/spacetime_distribution", &bins, S, in.mcid.data(), n_eta_eff, eta_vals.data(), &out))
        DIE("%s", is3d_last_error());
    for (int ip = 0; ip < S; ip++) printf("dN_dy = %lf\n", o_dy[ip]);   // :1438-1441
    printf("species classes evaluated: %d of %d; cells skipped (u.dsigma <= 0): %lld; outside the tau / r bins: %lld / %lld\n", sst.n_classes, S,
           (long long)sst.n_cells_skipped, (long long)sst.n_tau_outside, (long long)sst.n_r_outside);
    printf("device time: prep %.3f ms, per-cell %.3f ms, bins %.3f ms; h2d %.3f ms, d2h %.3f ms\n", sst.ms_prep, sst.ms_cells, sst.ms_bins,
           sst.ms_h2d, sst.ms_d2h);
    return copy_result(res, 0, in, nullptr, nullptr, 0);
}

// do_resonance_decays = 1 (emissionfunction.cpp:1689-1698): the feed-down of the thermal spectrum, then its two files; on the first device of the run's list
static int feed_down(const RunConfig &cfg, const RunInputs &in, const RunDevices &rd, const std::vector<double> &dN)
{
    printf("Starting resonance decays...\n");
    DecayTable tab;
    if (int rc = read_decay_table(cfg.pdg_path, tab)) return rc;
    std::vector<double> fed(dN);
    is3d_decay_stats ds{};
    const double t4 = now_s();
    const int rcd = is3d_resonance_decays(&tab.view, in.sp.n, in.mcid.data(), &in.grid, cfg.dimension, rd.first(), fed.data(), &ds);
    if (rcd) {
        const std::string msg = is3d_last_error();
        DIE("is3d_resonance_decays failed (%d): %s", rcd, msg.c_str());
    }
    printf("Writing thermal + resonance decays spectra to file...\n");
    if (is3d_write_results_decays("results", cfg.dimension, in.sp.n, in.grid.n_pT, in.pT.data(), in.grid.n_phi, in.phi.data(), in.grid.n_y, in.yv.data(), fed.data()))
        DIE("%s", is3d_last_error());
    printf("resonance decays: %d parents, %d channels integrated (%d with adjusted masses), %lld acos clamps; device time: tables %.3f ms, "
           "feed-down %.3f ms; wall %.3f s\n", ds.n_parents, ds.n_channels, ds.n_adjusted, (long long)ds.n_clamps, ds.ms_tables, ds.ms_feed, now_s() - t4);
    return IS3D_OK;
}

// ---- operation 1 (emissionfunction.cpp:1556-1698): the smooth momentum spectra, their files, the decay feed-down ----
static int run_spectra(const RunConfig &cfg, RunInputs &in, const RunDevices &rd, RunParams &params, is3d_run_result *res)
{
    const int ny_eff = (cfg.dimension == 2) ? 1 : (int)in.yv.size();
    std::vector<double> dN(in.mcid.size() * in.pT.size() * in.phi.size() * (size_t)ny_eff, 0.0);
    is3d_status st{};
    int rc;
    if (cfg.vah) {
        // the call the reference has commented out (emissionfunction.cpp:1650-1654), with the coefficients the CUDA tree's reader
        // would have put into the surface (src/cuda/deltafReader.cu:224-278)
        printf("computing thermal spectra from vahydro (P_L matching) with df...\n");
        // a device list the user spelled out shards the cells; without one the first device computes alone, whatever the machine shows
        if (rd.named) {
            rc = is3d_smooth_spectra_vah_multi(&in.vc, &in.sp, &in.grid, &in.vt, &in.opts, rd.list.data(), rd.size(), rd.reduce, dN.data(), &st, nullptr);
            print_devices(rd, in.n_cells, nullptr);
        } else {
            rc = is3d_smooth_spectra_vah_df(&in.vc, &in.sp, &in.grid, &in.vt, &in.opts, dN.data(), &st);
        }
    } else {
        GaussLaguerre gla;
        is3d_feqmod_tables fq{};
        fputs(cfg.feqmod ? "computing thermal spectra from vhydro with feqmod...\n" : "computing thermal spectra from vhydro with df...\n", stdout);
        if (cfg.feqmod) {
            // emissionfunction.cpp:1309-1319: Gauss-Laguerre tables, parameters deta_min and mass_pion0 (:184, :188), Plasma::load_thermodynamic_averages
            double T_avg = 0.0;
            if (int rcg = read_gauss_laguerre(gla, fq)) return rcg;
            if (fill_feqmod(in, params, 0.0, fq)) return IS3D_EINVAL;
            if (int rca = read_averages(1, &T_avg)) return rca;
            fq.T_avg = T_avg;
        }
        rc = is3d_smooth_spectra_multi(&in.cells, &in.sp, &in.grid, &in.df, cfg.feqmod ? &fq : nullptr, &in.opts, rd.data(), rd.size(), rd.reduce, dN.data(),
                                       &st, nullptr);
        print_devices(rd, in.n_cells, nullptr);
    }
    if (rc) {
        const std::string msg = is3d_last_error();
        DIE("is3d_smooth_spectra failed (%d): %s", rc, msg.c_str());
    }
    if (cfg.feqmod) printf("\nfeqmod breaks down for %lld cells\n\n", (long long)st.n_cells_breakdown);   // smooth_kernels.cpp:989
    const double t2 = now_s();
    if (is3d_write_results("results", cfg.dimension, in.sp.n, in.mcid.data(), in.grid.n_pT, in.pT.data(), in.pTw.data(), in.grid.n_phi, in.phi.data(),
                           in.phiw.data(), in.grid.n_y, in.yv.data(), dN.data()))
        DIE("%s", is3d_last_error());
    const double t3 = now_s();
    printf("species classes evaluated: %d of %d; cells skipped (u.dsigma <= 0): %lld\n", st.n_classes, in.sp.n, (long long)st.n_cells_skipped);
    printf("device time: prep %.3f ms, main %.3f ms (kernel variant %d), finalize %.3f ms; h2d %.3f ms, d2h %.3f ms\n", st.ms_prep,
           st.ms_main, st.kernel_variant, st.ms_finalize, st.ms_h2d, st.ms_d2h);
    const int src_kind = in.surf ? is3d_surface_source(in.surf) : -1;
    printf("wall: read %.3f s, spectra %.3f s, write %.3f s\n", in.t_loaded - in.t_start, t2 - in.t_loaded, t3 - t2);
    if (src_kind >= 0)
        printf("surface: %s\n", src_kind == 2 ? "binary sidecar input/surface.dat.is3dcache (matches the text file; IS3D_NO_CACHE=1 to ignore)"
                                 : src_kind == 1 ? "text parsed, sidecar input/surface.dat.is3dcache written for the next run" : "text parsed");
    if (int rcr = copy_result(res, 1, in, &dN, nullptr, 0)) return rcr;   // the embedding result keeps the thermal spectrum
    return cfg.do_decays ? feed_down(cfg, in, rd, dN) : IS3D_OK;
}

// ---- mode 5: every run ends with the spin polarization from the surface's thermal vorticity (emissionfunction.cpp:1675, :1701) ----
static int run_polarization(const RunConfig &cfg, RunInputs &in, const RunDevices &rd, RunParams &params, is3d_run_result *)
{
    if (cfg.mode != 5 || cfg.vah) return IS3D_OK;
    if (in.from_memory) {
        printf("mode = 5: the spin polarization needs the thermal vorticity, which only the file reader (input/surface.dat) provides; no S*.dat written\n");
        return IS3D_OK;
    }
    // Plasma::temperature: the first line of the averages file this run wrote, or T_switch (emissionfunction.cpp:1318-1321)
    double Tp = 0.0, set_T = 0.0;
    if (int rc = read_averages(1, &Tp)) return rc;
    if (params.optional("set_fo_temperature", &set_T) && (int)set_T && params.required("t_switch", &Tp)) return IS3D_EINVAL;
    const double *w[6];
    if (is3d_surface_vorticity(in.surf, w)) DIE("%s", is3d_last_error());
    is3d_vorticity vort{w[0], w[1], w[2], w[3], w[4], w[5]};
    is3d_options po{};
    po.dimension = cfg.dimension;
    po.device = rd.first();
    const size_t np = in.mcid.size() * in.pT.size() * in.phi.size() * (size_t)((cfg.dimension == 2) ? 1 : in.yv.size());
    std::vector<double> pS[5];
    for (auto &v : pS) v.assign(np, 0.0);
    is3d_polarization_out po_out{pS[0].data(), pS[1].data(), pS[2].data(), pS[3].data(), pS[4].data()};
    is3d_polarization_stats pst{};
    printf("Calculating spin polarization vector (T = %.6f GeV)...\n", Tp);
    // a device list the user spelled out shards the cells like the run's other cell sums do.  Without one the first device computes alone:
    // the sum's association depends on the shard count, and the S files (eight digits) must not depend on how many cards a machine shows
    std::vector<is3d_polarization_stats> pss(rd.named ? rd.list.size() : 0);
    const int rcp = rd.named ? is3d_spin_polarization_multi(&in.cells, &vort, &in.sp, &in.grid, Tp, &po, rd.list.data(), rd.size(), &po_out, &pst, pss.data())
                             : is3d_spin_polarization(&in.cells, &vort, &in.sp, &in.grid, Tp, &po, &po_out, &pst);
    if (rcp) {
        const std::string msg = is3d_last_error();
        DIE("%s failed (%d): %s", rd.named ? "is3d_spin_polarization_multi" : "is3d_spin_polarization", rcp, msg.c_str());
    }
    printf("Writing polarization vector to file...\n");
    if (is3d_write_polarization("results", cfg.dimension, in.sp.n, in.grid.n_pT, in.pT.data(), in.grid.n_phi, in.phi.data(), in.grid.n_y, in.yv.data(), &po_out))
        DIE("%s", is3d_last_error());
    printf("polarization: species classes evaluated: %d of %d; device time: cells %.3f ms, reduce %.3f ms\n", pst.n_classes, in.sp.n,
           pst.ms_cells, pst.ms_reduce);
    if (rd.named) printf("polarization: %d shard%s; slowest shard's cells %.3f ms\n", (int)pss.size(), pss.size() == 1 ? "" : "s", pst.ms_cells);
    return IS3D_OK;
}

static int run_impl(const MemSurface *mem, int variant, const RunDevices &rd, is3d_run_result *res)
{
    printf("iS3D-amd: MI355X-native smooth Cooper-Frye spectra (%s)\n", is3d_version());
    RunParams params("iS3D_parameters.dat");
    RunConfig cfg{};
    if (int rc = parse_config(params, mem, res != nullptr, cfg)) return rc;
    RunInputs in;
    in.t_start = now_s();
    // the device contexts are created while the surface is being parsed (load_inputs joins before the first device call)
    std::vector<int> warm_list(rd.list.begin(), rd.list.end());
    std::thread warm([&warm_list] { is3d::warm_devices(warm_list.empty() ? nullptr : warm_list.data(), (int)warm_list.size()); });
    struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } warm_joiner{warm};
    if (int rc = load_inputs(cfg, rd, variant, mem, warm, in)) return rc;
    const auto stage = cfg.operation == 2 ? run_sampler : cfg.operation == 0 ? run_spacetime : run_spectra;
    if (int rc = stage(cfg, in, rd, params, res)) return rc;
    if (int rc = run_polarization(cfg, in, rd, params, res)) return rc;
    fputs(cfg.operation == 2   ? "Done sampling particles. Output stored in results folder. Goodbye!\n"
          : cfg.operation == 0 ? "Done calculating spacetime distributions. Output stored in results/spacetime_distribution. Goodbye!\n"
                               : "Done calculating particle spectra. Output stored in results folder. Goodbye!\n", stdout);
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
    const MemSurface mem{surface, x, y};
    return run_impl(surface ? &mem : nullptr, kernel_variant, rd, result);
}

extern "C" void is3d_run_result_free(is3d_run_result *r)
{
    if (!r) return;
    free(r->particles); free(r->mc_id); free(r->mass); free(r->spectrum);
    memset(r, 0, sizeof *r);
}

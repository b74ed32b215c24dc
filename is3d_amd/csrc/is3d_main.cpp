// is3d_main.cpp -- `iS3D`-compatible command line driver: run it inside an iS3D run directory (iS3D_parameters.dat, input/,
// PDG/, tables/, deltaf_coefficients/, results/).  Everything happens in is3d_run_particlization (is3d_run.cpp), the
// counterpart of RuniS3D.cpp -> IS3D::run_particlization(1) (/root/reference/src/cpp/RuniS3D.cpp, iS3D.cpp:74-192).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/is3d_amd.h"

// --generate-df DIR: the coefficient generator (generate_delta_f_coefficients/<list>/df_vh_dimensionless in the reference, a separate offline
// program there) for the list hrg_eos names, on the device.  Reads iS3D_parameters.dat (hrg_eos), the PDG file and
// tables/gla_roots_weights_<N>_points.txt; writes the ten tables into DIR and nothing else.  No surface is read.
struct DfRange { double lo, hi; int n; };
static int generate_df(const char *dir, int gla_points, DfRange Tr, DfRange Br)
{
    const auto fail = [](const char *what) { fprintf(stderr, "iS3D-amd: %s\n", what); return 1; };
    if (FILE *f = fopen((std::string(dir) + "/c0.dat").c_str(), "r")) {   // the writer's own refusal, before anything is computed
        fclose(f);
        fprintf(stderr, "iS3D-amd: %s/c0.dat exists: coefficient tables are never overwritten; choose another directory\n", dir);
        return 1;
    }
    double v = 0.0;
    if (is3d_param_get("iS3D_parameters.dat", "hrg_eos", &v)) return fail(is3d_last_error());
    const int hrg_eos = (int)v;
    const char *pdg_path = hrg_eos == 1 ? "PDG/pdg-urqmd_v3.3+.dat" : hrg_eos == 2 ? "PDG/pdg_smash.dat" : hrg_eos == 3 ? "PDG/pdg_box.dat" : nullptr;
    if (!pdg_path) { fprintf(stderr, "iS3D-amd: hrg_eos = %d: please choose hrg_eos = (1,2,3)\n", hrg_eos); return 1; }
    const auto pdg_read = (hrg_eos == 3) ? is3d_pdg_read_box : is3d_pdg_read;
    int32_t n = 0;
    if (pdg_read(pdg_path, &n, nullptr, nullptr, nullptr, nullptr, nullptr, 0)) return fail(is3d_last_error());
    std::vector<int64_t> id(n);
    std::vector<double> mass(n), gspin(n), baryon(n), sign(n);
    if (pdg_read(pdg_path, &n, id.data(), mass.data(), gspin.data(), baryon.data(), sign.data(), n)) return fail(is3d_last_error());
    const std::string gla_path = "tables/gla_roots_weights_" + std::to_string(gla_points) + "_points.txt";
    int32_t n_alpha = 0, n_gla = 0;
    if (is3d_gla_read(gla_path.c_str(), &n_alpha, &n_gla, nullptr, nullptr, 0)) return fail(is3d_last_error());
    if (n_alpha < 5) {
        fprintf(stderr, "iS3D-amd: %s carries alpha = 0..%d; the coefficient integrals need the rules for alpha = 1, 2, 3 and 4 (five alphas)\n",
                gla_path.c_str(), n_alpha - 1);
        return 1;
    }
    std::vector<double> root((size_t)n_alpha * n_gla), weight(root.size());
    if (is3d_gla_read(gla_path.c_str(), &n_alpha, &n_gla, root.data(), weight.data(), (int64_t)root.size())) return fail(is3d_last_error());
    const double *r4[4], *w4[4];
    for (int a = 0; a < 4; a++) { r4[a] = root.data() + (size_t)(a + 1) * n_gla; w4[a] = weight.data() + (size_t)(a + 1) * n_gla; }
    // the grid as deltaf_table.cpp:58-71 builds it: x[0] = lo, x[i] = lo + i * (hi - lo) / (n - 1)
    const auto grid = [](DfRange r) {
        std::vector<double> x(r.n, r.lo);
        const double d = r.n > 1 ? (r.hi - r.lo) / (double)(r.n - 1) : 0.0;
        for (int i = 1; i < r.n; i++) x[i] = r.lo + (double)i * d;
        return x;
    };
    const std::vector<double> T = grid(Tr), muB = grid(Br);
    std::vector<double> tables((size_t)10 * T.size() * muB.size());
    const is3d_hadron_list list = {n, mass.data(), gspin.data(), baryon.data(), sign.data()};
    is3d_dfgen_stats st;
    const auto t0 = std::chrono::steady_clock::now();
    if (is3d_df_generate(&list, n_gla, r4, w4, (int32_t)T.size(), T.data(), (int32_t)muB.size(), muB.data(), -1, tables.data(), nullptr, &st))
        return fail(is3d_last_error());
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (is3d_df_tables_write(dir, (int32_t)T.size(), T.data(), (int32_t)muB.size(), muB.data(), tables.data())) return fail(is3d_last_error());
    printf("df coefficients: %s (%d entries, %d massive), %d-point Gauss-Laguerre, %zu T x %zu muB points -> %s\n"
           "device time: kernel %.3f ms, upload %.3f ms, copy back %.3f ms (whole call %.3f ms)\n",
           pdg_path, n, st.n_massive, n_gla, T.size(), muB.size(), dir, st.ms_kernel, st.ms_h2d, st.ms_d2h, ms);
    return 0;
}

static bool parse_range(char **a, DfRange &r)
{
    char *e1 = nullptr, *e2 = nullptr, *e3 = nullptr;
    r.lo = strtod(a[0], &e1);
    r.hi = strtod(a[1], &e2);
    const long n = strtol(a[2], &e3, 10);
    r.n = (int)n;
    return e1 != a[0] && !*e1 && e2 != a[1] && !*e2 && e3 != a[2] && !*e3 && n >= 1 && n <= 100000;
}

int main(int argc, char **argv)
{
    int variant = 0, reduce = -1;
    std::vector<int32_t> devices;
    const char *df_out = nullptr;
    int gla_points = 64;                                         // carries alpha up to 4; deltaf_table.cpp:48
    DfRange Tr = {0.1, 0.2, 101}, Br = {0.0, 0.8, 81};           // deltaf_table.cpp:39-46
    for (int i = 1; i < argc; i++) {
        if (!strcmp(argv[i], "--variant") && i + 1 < argc) variant = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--generate-df") && i + 1 < argc) df_out = argv[++i];
        else if (!strcmp(argv[i], "--gla-points") && i + 1 < argc) {
            gla_points = atoi(argv[++i]);
            if (gla_points < 1) { fprintf(stderr, "--gla-points N: a positive number of Gauss-Laguerre nodes\n"); return 2; }
        } else if ((!strcmp(argv[i], "--T-range") || !strcmp(argv[i], "--muB-range")) && i + 3 < argc) {
            const bool isT = !strcmp(argv[i], "--T-range");
            if (!parse_range(argv + i + 1, isT ? Tr : Br) || (isT && !(Tr.lo > 0.0))) {
                fprintf(stderr, "%s lo hi n: two numbers in GeV (T > 0) and a point count >= 1\n", argv[i]);
                return 2;
            }
            i += 3;
        }
        else if (!strcmp(argv[i], "--devices") && i + 1 < argc) {
            // "0,1,2": one cell-axis shard per entry (an ordinal may repeat); default: IS3D_DEVICES, else every visible device
            for (const char *p = argv[++i]; *p;) {
                char *end = nullptr;
                const long v = strtol(p, &end, 10);
                if (end == p || v < 0 || (*end && *end != ',')) { fprintf(stderr, "--devices: a comma separated list of HIP device ordinals\n"); return 2; }
                devices.push_back((int32_t)v);
                p = *end ? end + 1 : end;
            }
        } else if (!strcmp(argv[i], "--reduce") && i + 1 < argc) {
            ++i;
            if (!strcmp(argv[i], "rccl")) reduce = IS3D_REDUCE_RCCL;
            else if (!strcmp(argv[i], "ordered")) reduce = IS3D_REDUCE_ORDERED;
            else { fprintf(stderr, "--reduce ordered|rccl\n"); return 2; }
        } else if (!strcmp(argv[i], "--help")) {
            printf("usage: %s [--variant 1|2|3|4] [--devices 0,1,...] [--reduce ordered|rccl]   (run inside an iS3D run directory)\n"
                   "       %s --generate-df DIR [--gla-points N] [--T-range lo hi n] [--muB-range lo hi n]\n"
                   "  --generate-df writes the ten df coefficient tables of the hrg_eos list into DIR (default grid: T 0.1..0.2 GeV x 101,\n"
                   "  muB 0..0.8 GeV x 81, 64 Gauss-Laguerre nodes) and does nothing else; the optional parameter deltaf_dir = DIR makes a run read them\n"
                   "  operation = 1 shards the freezeout cells over the devices (default: every visible GPU; IS3D_DEVICES, IS3D_REDUCE)\n"
                   "  mode = 5 shards the spin polarization over a device list given by --devices or IS3D_DEVICES (default: the first device alone)\n"
                   "  mode = 2 shards the anisotropic-hydro spectra over such a list in the same way (default: the first device alone)\n", argv[0], argv[0]);
            return 0;
        }
    }
    if (df_out) return generate_df(df_out, gla_points, Tr, Br);
    if (devices.empty() && reduce < 0) return is3d_run_particlization(NULL, NULL, NULL, variant, NULL) == IS3D_OK ? 0 : 1;
    if (devices.empty()) {   // --reduce alone: every visible device, as a count -- no list was spelled out (mode 5: the polarization is not sharded)
        const int n = is3d_device_count() > 0 ? is3d_device_count() : 1;
        return is3d_run_particlization_on(NULL, NULL, NULL, variant, NULL, n, reduce, NULL) == IS3D_OK ? 0 : 1;
    }
    return is3d_run_particlization_on(NULL, NULL, NULL, variant, devices.data(), (int32_t)devices.size(),
                                      reduce < 0 ? IS3D_REDUCE_ORDERED : reduce, NULL) == IS3D_OK ? 0 : 1;
}

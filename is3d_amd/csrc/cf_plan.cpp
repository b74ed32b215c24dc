// cf_plan.cpp -- plan object and C ABI of the device path (include/is3d_amd.h).
//
// Host-side counterpart of EmissionFunctionArray's packing/dispatch for the smooth path
// (/root/reference/src/cpp/emissionfunction.cpp:1282-1307 species scalars, :1503-1521 dispatch):
// groups species into (mass, sign) classes, builds the lane table, the natural cubic splines of
// Deltaf_Data::construct_cubic_splines (deltafReader.cpp:300-322) and drives prep -> main -> finalize.
// There is no CPU compute path in this file: without a HIP device every entry fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/is3d_amd.h"
#include "cf_feqmod.h"
#include "cf_host.h"
#include "cf_launch.h"
#include "cf_plan_geometry.h"
#include "cf_spacetime.h"
#include "errors.h"
#include "jonah.h"
#include "spline.h"

#define fail is3d::set_error

using is3d::DevBuf;

struct is3d_plan {
    is3d_options opts{};
    int device = 0;
    int npart = 0, ncls = 0, npT = 0, J = 0, K = 0, Kacc = 0, ny_eff = 0;
    int L = 0, Lpad = 0;      // L: lane slots in use (bins x split), Lpad: padded to whole waves
    int Lbins = 0, split = 1; // momentum bins (classes x pT); lane slots per bin (unit-strided lanes, 2+1D variant 7)
    DevBuf<int32_t> d_lane_sub;
    int variant = 2, JT = 1, KT = 1, jtiles = 1, ktiles = 1;
    bool dim3 = true, ce = false;
    int64_t max_cells = 0, pass_cells = 0, nout = 0;
    int nch_max = 1;
    size_t bytes_per_cell = 0;
    double prefactor = 0;
    double mTmax = 0, pTmax = 0;   // over the lane table: bound of |p.dsigma| for the stream's power-of-two scale
    double kmin = 0, kmax = 0, gw2d = 1;   // y range (3+1D) / max_k w_k cosh(eta_k) (2+1D) for the same bound

    DevBuf<double> d_mT, d_pT, d_sign, d_lane_b, d_degeneracy, d_cosphi, d_sinphi, d_kgrid, d_kweight, d_kch, d_ksh;
    DevBuf<double> d_bilT, d_bilB, d_biltab[5];
    DevBuf<double> d_coskphi, d_sinkphi, d_phiw, d_pTw;   // derived observables
    is3d::BilinearDev bil{};
    bool baryon = false, baryondiff = false;
    DevBuf<int> d_cls;
    DevBuf<int32_t> d_lane_pe;      // per lane: max(mT/mTmax, pT/pTmax) < 2^pe
    DevBuf<double> d_cull_floor;    // zero_skip 3 (cf_main_tile3e): [jtiles * ktiles][Lpad] threshold floors from the chunks that ran first
    DevBuf<double> d_splx, d_sply[3], d_splc[3];
    DevBuf<double> d_S1, d_S2, d_S3, d_TS, d_partial;
    DevBuf<double> d_TE, d_pTgrid;   // variant 5: E2 table stream (cf_device.h), the pT grid for cf_prep
    DevBuf<int32_t> d_lane_ipT;      // variant 5: lane -> index of its pT
    bool e2tab = false;
    int ub3e = 0;
    int rblocks = 1, upc = 1;   // row blocks of the tiled stream; units per cell within a stream
    int wpb = 4;                // waves per workgroup of the main kernel
    DevBuf<unsigned long long> d_status, d_sticky;   // d_sticky: {min bad cell, min fast cell} over the executes since the last is3d_plan_check
    is3d::SplineDev spl{};

    // modified equilibrium (df_mode 3, 4)
    bool feqmod = false;
    int nj = 0, ngl = 0;
    double bp_max = 0.0, detA_min = 0.0, mass_pion0 = 0.0;
    DevBuf<double> d_gl, d_jonah, d_cls_mass, d_cls_sign, d_cls_baryon, d_lane_mass, d_RN, d_CR, d_FB;
    DevBuf<int32_t> d_lane_cls, d_flag, d_list, d_count;

    // operation 0 (is3d_plan_execute_spacetime): host copies of the species classes, the lane tables of cf_st_cells and its workspaces,
    // made on the first such execute
    std::vector<int32_t> sp_cls;
    std::vector<double> cls_mass, cls_sign, cls_bar, pT_grid, sp_deg;
    is3d::StState st;   // lane tables, weights and workspaces (cf_spacetime.h)

    bool timing = false;
    std::vector<hipEvent_t> ev_list;  // [pass][0..3]: start, after prep, after main; last: after finalize
    int last_passes = 0;
    int64_t workspace = 0;

    ~is3d_plan()
    {
        for (hipEvent_t e : ev_list)
            if (e) (void)hipEventDestroy(e);
    }
};

static int validate(const is3d_species *sp, const is3d_grid *g, const is3d_df_tables *df, const is3d_feqmod_tables *fq,
                    const is3d_options *o)
{
    if (!sp || !g || !df || !o) return fail(IS3D_EINVAL, "null argument");
    if (o->dimension != 2 && o->dimension != 3) return fail(IS3D_EINVAL, "dimension must be 2 or 3 (got %d)", o->dimension);
    if (fq) {
        if (o->df_mode != 3 && o->df_mode != 4) return fail(IS3D_EINVAL, "the feqmod entries take df_mode 3 or 4 (got %d)", o->df_mode);
        if (o->include_baryon && o->df_mode == 4)   // the reference: "Jonah df doesn't work for nonzero muB. Exiting..", deltafReader.cpp:470-474
            return fail(IS3D_EINVAL, "df_mode 4 does not work with include_baryon = 1 (the reference exits there too)");
        if (o->kernel_variant == 1) return fail(IS3D_EINVAL, "df_mode 3/4 runs on the tile kernel only (kernel_variant 0, 2-4)");
        if (fq->n_gla < 1 || fq->n_gla > 256 || !fq->root1 || !fq->weight1 || !fq->root2 || !fq->weight2)
            return fail(IS3D_EINVAL, "df_mode 3/4 needs the Gauss-Laguerre roots and weights for alpha = 1, 2");
        if (!df->betapi) return fail(IS3D_EINVAL, "df_mode 3/4 needs the betapi table");
        if (o->df_mode == 3 && (!df->F || !df->betabulk)) return fail(IS3D_EINVAL, "df_mode 3 needs the F and betabulk tables");
        if (o->df_mode == 4 && (fq->n_pdg < 1 || !fq->pdg_mass || !fq->pdg_degeneracy || !fq->pdg_sign || !(fq->T_avg > 0.0)))
            return fail(IS3D_EINVAL, "df_mode 4 needs the full PDG list and the surface-averaged temperature");
    } else if (o->df_mode != 1 && o->df_mode != 2)
        return fail(IS3D_EINVAL, "df_mode must be 1 (14-moment) or 2 (Chapman-Enskog) on this entry (got %d); 3 and 4 go through is3d_*_feqmod", o->df_mode);
    if (o->include_baryon) {
        if (o->kernel_variant == 1) return fail(IS3D_EINVAL, "include_baryon = 1 runs on the tile kernel only (kernel_variant 2-4)");
        if (!sp->baryon) return fail(IS3D_EINVAL, "include_baryon = 1 needs the species' baryon numbers");
        if (df->n_muB < 2 || !df->muB) return fail(IS3D_EINVAL, "include_baryon = 1 needs the full (T, muB) coefficient tables");
        for (int i = 1; i < df->n_muB; i++)
            if (!(df->muB[i] > df->muB[i - 1])) return fail(IS3D_EINVAL, "coefficient table muB values must ascend");
        if (o->df_mode == 1 && (!df->c1 || !df->c3 || !df->c4)) return fail(IS3D_EINVAL, "include_baryon = 1, df_mode 1 needs c0..c4 tables");
        if ((o->df_mode == 2 || o->df_mode == 3) && (!df->G || !df->betaV)) return fail(IS3D_EINVAL, "include_baryon = 1, df_mode 2 needs F, G, betabulk, betaV, betapi tables");
    }
    if (sp->n < 1 || !sp->mass || !sp->sign || !sp->degeneracy) return fail(IS3D_EINVAL, "empty species list");
    if (g->n_pT < 1 || g->n_phi < 1 || !g->pT || !g->phi) return fail(IS3D_EINVAL, "empty pT/phi grid");
    if (o->dimension == 3 && (g->n_y < 1 || !g->y)) return fail(IS3D_EINVAL, "dimension 3 needs a y grid");
    if (o->dimension == 2 && (g->n_eta < 1 || !g->eta || !g->eta_w)) return fail(IS3D_EINVAL, "dimension 2 needs an eta table");
    if (df->n_T < 3 || !df->T) return fail(IS3D_EINVAL, "coefficient table needs >= 3 temperatures");
    if (o->df_mode == 1 && (!df->c0 || !df->c2)) return fail(IS3D_EINVAL, "df_mode 1 needs c0 and c2 tables");
    if (o->df_mode == 2 && (!df->F || !df->betabulk || !df->betapi)) return fail(IS3D_EINVAL, "df_mode 2 needs F, betabulk, betapi tables");
    for (int i = 1; i < df->n_T; i++)
        if (!(df->T[i] > df->T[i - 1])) return fail(IS3D_EINVAL, "coefficient table temperatures must ascend");
    return IS3D_OK;
}

extern "C" const char *is3d_version(void) { return is3d::kDevBuild ? "is3d_amd 0.1 (gfx950) DEV BUILD" : "is3d_amd 0.1 (gfx950)"; }
extern "C" int is3d_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// The stages of plan_create_impl, in its order.  What they decide without the device is in cf_plan_geometry.h.

// ---- choose kernel: the variant, whether it reads the E2 table stream, lane slots per momentum bin ----
// Defaults per mode (A/B on MI355X):
//   3+1D delta-f, pT grid <= 32: variant 6 -- 8 x 7 tile, phi-side exponentials from the E2 table stream, rows tested for liveness before
//     their exponential (config 3: 354 ms against 404 ms for variant 3), with or without baryon slots;
//   3+1D otherwise: 8 x 7 (modified equilibrium, with or without the baryon slots -- its records do not grow with them: 1005 vs 1028 ms for
//     6 x 7; 247.1 against 260.5 ms per 3e5 cells), 6 x 7 for delta-f with the baryon slots;
//   2+1D: variant 7 -- 8 x 31 tile with unit-strided lanes (delta-f, config 2, 96 bins: 31.4 ms against 38.7 ms for 8 x 61; 305 species, one
//     slot per bin: 96.0 against 101.0 ms per 2e4 cells; modified equilibrium: rows tested against the unit's threshold from the beta minimum
//     they carry, the default since round 4).
// The shipped library holds the kernels these defaults reach (cf_kernels.hip::launch_variant, cf_feqmod.hip) and one explicit choice, the 8 x 7
// tile without the E2 table stream (3) for a 3+1D delta-f surface without baryon slots; any other request runs the default.  The A/B forms of
// rounds 1-5 exist in the developer build (make DEV=1), where tests/test_gpu_devlib.py runs their parity tests.
static void plan_choose_kernel(is3d_plan &P, const is3d_grid *g, const is3d_options *o)
{
    const bool fq = P.feqmod;
    const is3d::VariantChoice vc = is3d::choose_variant(o->dimension, fq, o->include_baryon != 0, g->n_pT <= is3d::kE2Stride, o->kernel_variant, is3d::kDevBuild);
    P.variant = vc.variant;
    P.e2tab = vc.e2tab;
    // unit-strided lanes (2+1D, variants 7 and 8): S lane slots per bin so that the slots fill whole waves; S divides the units per cell
    P.split = 1;
    if (P.variant == 7 || P.variant == 8) {
        int JT7 = 0, R7 = 0;
        is3d::main_tile_shape(7, 0, &JT7, &R7);
        P.split = is3d::lane_split(P.Lbins, (g->n_eta + R7 - 1) / R7);
    }
    if (fq && o->dimension == 2 && P.variant != 7) {
        // modified equilibrium, 2+1D, the 61-row tiles (A/B): the same lane slots on the kernel's own tile -- S = 2 when it divides the units per cell and
        // the units per LDS batch (cf_main_feqmod stages 1536 / REC units) and fills the two-wave workgroups better
        int JTf = 0, Rf = 0;
        is3d::main_tile_shape(P.variant, 0, &JTf, &Rf);
        const int recf = 4 * JTf + Rf * (4 + JTf), ubf = std::max(1, 1536 / recf), rblocksf = (g->n_eta + Rf - 1) / Rf;
        const int nb = P.Lbins;
        const double waste1 = 1.0 - (double)nb / (double)(((nb + 63) / 64) * 64);
        const double waste2 = 1.0 - (double)(2 * nb) / (double)(((2 * nb + 63) / 64) * 64);
        if (rblocksf % 2 == 0 && ubf % 2 == 0 && waste2 < waste1 - 0.05) P.split = 2;
    }
}

// ---- lanes and grids: the lane table, the species map, the phi and y / eta grids, uploaded ----
static int plan_lanes_and_grids(is3d_plan &P, const is3d_grid *g, const is3d_options *o, const is3d::SpeciesClasses &k)
{
    // dev A/B (IS3D_LANE_INTERLEAVE=1, developer build): the two waves of a workgroup take the even and the odd slots of their 128-slot span of
    // the mT order instead of its lower and upper half -- both then cover the same mT range, cull the same units and rows, and meet at the
    // per-batch barrier with (nearly) the same work done
    static const bool inter = is3d::dev_env("IS3D_LANE_INTERLEAVE") != nullptr;
    const is3d::LaneTable lt = is3d::lane_table(k, g->pT, P.npT, P.split, inter && o->dimension == 3 && !P.feqmod);
    P.L = lt.L;
    P.Lpad = lt.Lpad;
    // what is uploaded: the table's slots in use, the padding slots as copies of the last of them (they never change a cull vote of their wave)
    const is3d::LaneArrays la = is3d::lane_arrays(lt, k, P.npT);
    P.mTmax = la.mTmax;
    P.pTmax = la.pTmax;
    std::vector<double> cosphi(P.J), sinphi(P.J);
    for (int j = 0; j < P.J; j++) { cosphi[j] = std::cos(g->phi[j]); sinphi[j] = std::sin(g->phi[j]); }  // :43-48
    std::vector<double> kgrid(P.K), kweight(P.K, 1.0);
    for (int k2 = 0; k2 < P.K; k2++) {
        kgrid[k2] = P.dim3 ? g->y[k2] : g->eta[k2];
        if (!P.dim3) kweight[k2] = g->eta_w[k2];
    }
    P.kmin = *std::min_element(kgrid.begin(), kgrid.end());
    P.kmax = *std::max_element(kgrid.begin(), kgrid.end());
    if (!P.dim3) {
        P.gw2d = 0.0;
        for (int k2 = 0; k2 < P.K; k2++) P.gw2d = std::max(P.gw2d, std::fabs(kweight[k2]) * std::cosh(kgrid[k2]));
    }
    HIP_TRY(P.d_mT.upload(la.mT));
    HIP_TRY(P.d_pT.upload(la.pT));
    HIP_TRY(P.d_sign.upload(la.sign));
    HIP_TRY(P.d_lane_b.upload(la.b));
    HIP_TRY(P.d_lane_sub.upload(la.sub));
    if (P.e2tab) {
        HIP_TRY(P.d_lane_ipT.upload(la.ipT));
        HIP_TRY(P.d_pTgrid.upload(P.pT_grid));
        for (int i = 0; i < P.npT; i++)
            if (!(g->pT[i] >= 0.0)) return fail(IS3D_EINVAL, "kernel_variant 5 needs pT >= 0 (pT Dmax must be the maximum of pT D_j)");
    }
    HIP_TRY(P.d_degeneracy.upload(P.sp_deg));
    HIP_TRY(P.d_cls.upload(lt.lane_of));
    HIP_TRY(P.d_lane_pe.upload(la.pe));
    if (P.feqmod) {   // modified equilibrium: the slots' class and its mass
        HIP_TRY(P.d_lane_mass.upload(la.mass));
        HIP_TRY(P.d_lane_cls.upload(la.cls));
    }
    HIP_TRY(P.d_cosphi.upload(cosphi));
    HIP_TRY(P.d_sinphi.upload(sinphi));
    HIP_TRY(P.d_kgrid.upload(kgrid));
    HIP_TRY(P.d_kweight.upload(kweight));
    {
        std::vector<double> kch(P.K), ksh(P.K);
        for (int k2 = 0; k2 < P.K; k2++) { kch[k2] = std::cosh(0.0 - kgrid[k2]); ksh[k2] = std::sinh(0.0 - kgrid[k2]); }   // smooth_kernels.cpp:279-280 with y = 0
        HIP_TRY(P.d_kch.upload(kch));
        HIP_TRY(P.d_ksh.upload(ksh));
    }
    std::vector<double> ck, sk;
    is3d::vn_harmonics(g->phi, P.J, ck, sk);
    HIP_TRY(P.d_coskphi.upload(ck));
    HIP_TRY(P.d_sinkphi.upload(sk));
    HIP_TRY(P.d_phiw.alloc(P.J));
    HIP_TRY(P.d_pTw.alloc(P.npT));
    return IS3D_OK;
}

// ---- coefficient tables: splines in T (deltafReader.cpp:300-322), and with baryon slots the full (mu_B, T) grids of the bilinear branch ----
static int plan_coefficient_tables(is3d_plan &P, const is3d_df_tables *df, const is3d_options *o)
{
    const double *tabs[3] = {nullptr, nullptr, nullptr};
    int nspl;
    if (P.feqmod) {
        // df_mode 3: F, betabulk, betapi; df_mode 4 reads betapi only (the other two slots mirror it, unused)
        tabs[0] = (o->df_mode == 3) ? df->F : df->betapi;
        tabs[1] = (o->df_mode == 3) ? df->betabulk : df->betapi;
        tabs[2] = df->betapi;
        nspl = 3;
    } else if (!P.ce) { tabs[0] = df->c0; tabs[1] = df->c2; nspl = 2; }
    else { tabs[0] = df->F; tabs[1] = df->betabulk; tabs[2] = df->betapi; nspl = 3; }
    std::vector<double> xs(df->T, df->T + df->n_T);
    HIP_TRY(P.d_splx.upload(xs));
    P.spl.n = df->n_T;
    P.spl.x = P.d_splx.p;
    P.spl.nspl = nspl;
    for (int s = 0; s < 3; s++) { P.spl.y[s] = nullptr; P.spl.c[s] = nullptr; }
    for (int s = 0; s < nspl; s++) {
        std::vector<double> ys(tabs[s], tabs[s] + df->n_T), cs;
        if (!is3d::natural_cspline_init(xs, ys, cs)) return fail(IS3D_EINVAL, "spline construction failed");
        HIP_TRY(P.d_sply[s].upload(ys));
        HIP_TRY(P.d_splc[s].upload(cs));
        P.spl.y[s] = P.d_sply[s].p;
        P.spl.c[s] = P.d_splc[s].p;
    }
    if (P.baryon) {
        // full (mu_B, T) grids for the bilinear branch (deltafReader.cpp:412-484)
        const double *t5[5];
        if (!P.ce && !P.feqmod) { t5[0] = df->c0; t5[1] = df->c1; t5[2] = df->c2; t5[3] = df->c3; t5[4] = df->c4; }
        else { t5[0] = df->F; t5[1] = df->G; t5[2] = df->betabulk; t5[3] = df->betaV; t5[4] = df->betapi; }
        std::vector<double> bs(df->muB, df->muB + df->n_muB);
        HIP_TRY(P.d_bilT.upload(xs));
        HIP_TRY(P.d_bilB.upload(bs));
        P.bil.nT = df->n_T; P.bil.nB = df->n_muB;
        P.bil.swap = o->reference_bilinear_indexing != 0;
        P.bil.T = P.d_bilT.p; P.bil.muB = P.d_bilB.p;
        for (int k = 0; k < 5; k++) {
            std::vector<double> tv(t5[k], t5[k] + (size_t)df->n_T * df->n_muB);
            HIP_TRY(P.d_biltab[k].upload(tv));
            P.bil.tab[k] = P.d_biltab[k].p;
        }
    }
    return IS3D_OK;
}

// ---- modified-equilibrium tables: Gauss-Laguerre nodes, the df_mode 4 splines in bulkPi/Peq, the class tables (the lane -> class tables go up with the lanes) ----
static int plan_feqmod_tables(is3d_plan &P, const is3d_feqmod_tables *fq, const is3d_options *o, const is3d::SpeciesClasses &k)
{
    P.ngl = fq->n_gla;
    P.detA_min = fq->deta_min;
    P.mass_pion0 = fq->mass_pion0;
    std::vector<double> gl((size_t)4 * P.ngl);
    for (int i = 0; i < P.ngl; i++) {
        gl[i] = fq->root1[i]; gl[P.ngl + i] = fq->weight1[i]; gl[2 * P.ngl + i] = fq->root2[i]; gl[3 * P.ngl + i] = fq->weight2[i];
    }
    HIP_TRY(P.d_gl.upload(gl));
    std::vector<double> jon;
    if (o->df_mode == 4) {
        std::vector<double> bp, l2, zz, cl, cz;
        is3d::jonah_tables(fq, bp, l2, zz, P.bp_max);
        // gsl_spline_init on (bulkPi_over_Peq, lambda_squared) and (bulkPi_over_Peq, z), deltafReader.cpp:311-320
        if (!is3d::natural_cspline_init(bp, l2, cl) || !is3d::natural_cspline_init(bp, zz, cz))
            return fail(IS3D_EINVAL, "df_mode 4: bulkPi/Peq(lambda) is not ascending at T_avg = %.6g GeV (GSL would abort here)", fq->T_avg);
        P.nj = (int)bp.size();
        for (const auto *v : {&bp, &l2, &zz, &cl, &cz}) jon.insert(jon.end(), v->begin(), v->end());
    } else {
        P.nj = 2;   // unused placeholder so that the prep kernel's LDS layout stays valid
        jon.assign(10, 0.0);
        jon[1] = 1.0;
    }
    HIP_TRY(P.d_jonah.upload(jon));
    HIP_TRY(P.d_cls_mass.upload(k.cmass));
    HIP_TRY(P.d_cls_sign.upload(k.csign));
    if (P.baryon) HIP_TRY(P.d_cls_baryon.upload(k.cbar));
    return IS3D_OK;
}

// ---- tiling and pass / chunk sizing: the tile grid, bytes of streams per cell, cells per pass, waves per workgroup, chunks ----
static int plan_tiling_and_sizing(is3d_plan &P, const is3d_df_tables *df, const is3d_options *o, int64_t max_cells)
{
    is3d::main_tile_shape(P.variant, P.dim3 ? 1 : 0, &P.JT, &P.KT);
    P.jtiles = (P.J + P.JT - 1) / P.JT;
    const bool tiled = P.variant != 1;
    if (!P.feqmod && is3d::prep_lds_bytes(df->n_T, P.spl.nspl, P.J, P.K, P.baryon ? 1 : 0, tiled ? is3d::unit_rec_doubles(P.JT, P.KT, P.baryon ? 1 : 0) : 0, P.dim3 ? 1 : 0,
                                    (tiled && P.dim3) ? P.jtiles * ((P.K + P.KT - 1) / P.KT) : 0) > 160 * 1024)
        return fail(IS3D_EINVAL, "grids too large for the prep kernel's LDS staging");
    P.rblocks = tiled ? (P.K + P.KT - 1) / P.KT : 1;
    P.ktiles = P.dim3 ? (P.K + P.KT - 1) / P.KT : 1;   // k tiles are separate tasks only in 3+1D
    P.upc = (tiled && !P.dim3) ? P.rblocks : 1;            // 2+1D: eta blocks are consecutive units of one stream
    if (P.feqmod && is3d::prep_feqmod_lds_bytes(df->n_T, P.nj, P.ngl, P.J, P.K, P.jtiles, P.rblocks, is3d::unit_rec_doubles(P.JT, P.KT, 0)) > 160 * 1024)
        return fail(IS3D_EINVAL, "grids too large for the prep kernel's LDS staging");
    if (tiled)
        P.bytes_per_cell = sizeof(double) * (size_t)P.jtiles * P.rblocks * is3d::unit_rec_doubles(P.JT, P.KT, (P.baryon && !P.feqmod) ? 1 : 0);
    else
        P.bytes_per_cell = sizeof(double) * ((size_t)P.K * is3d::kS1Rec + (size_t)P.J * is3d::kS2Rec + (size_t)P.J * P.K);
    if (P.e2tab) P.bytes_per_cell += sizeof(double) * (size_t)P.jtiles * is3d::kE2Stride * P.JT;
    if (P.feqmod)   // fallback record, flag, list entry; df_mode 3: cell record + |renorm| per class
        P.bytes_per_cell += sizeof(double) * is3d::kFbRec + 2 * sizeof(int32_t) +
                             (o->df_mode == 3 ? sizeof(double) * ((size_t)is3d::kCrRec + P.ncls) : 0);
    // cap on the derived streams of one pass: the caller's, else 16 GiB or 45 % of the device's TOTAL memory, whichever is larger (288 GB of
    // HBM: a 1e6-cell surface with baryon slots -- 20.6 KB per cell -- stays a single pass; only what max_cells needs is allocated).  The
    // total, not what happens to be free: the pass count, the chunk count and with them the summation order of a surface that needs several
    // passes must not depend on what else occupies the GPU at the moment (the partial slab below adds up to 12 GiB on top; an allocation that
    // does not fit is reported as IS3D_ENOMEM with the sizes, and opts.workspace_bytes sets the cap explicitly)
    const int64_t ws = is3d::default_stream_cap_bytes(o->workspace_bytes);   // cf_launch.h: one rule for every plan
    int64_t pc = ws / (int64_t)P.bytes_per_cell;
    if (pc < 1) pc = 1;
    if (pc > max_cells) pc = max_cells;
    if (pc > 0x7fff0000LL) pc = 0x7fff0000LL;
    P.pass_cells = pc;
    P.max_cells = max_cells;

    const int lane_waves = P.Lpad / 64;
    P.wpb = 4;
    if (tiled) {
        P.wpb = is3d::waves_per_group(lane_waves, o->waves_per_group);
        if (o->waves_per_group == 1 && P.e2tab) P.wpb = 1;   // cf_main_tile3e: one-wave workgroups (no barrier partner)
        if (P.variant == 9) P.wpb = 1;                       // cf_main_tile3s: a workgroup IS one wave
        // cf_main_feqmod, 3+1D 8 x 7 without baryon slots: one-wave workgroups (cf_feqmod.hip, LDSD); the pipelined A/B form (variant 5) keeps two
        // -- the default there since round 4 (486 against 501 ms on the config-3 surface, profiles/r04_ab_feqmod.log); waves_per_group = 2 keeps the pair
        if (P.feqmod && P.dim3 && (P.variant == 3 || P.variant == 6) && (o->waves_per_group == 1 || o->waves_per_group == 0)) P.wpb = 1;
    }
    // Chunk count (is3d::chunk_count): ~12 rounds of the chip (24 until the end of round 3 -- on a 125 000-cell shard 144 instead of 288 chunks run
    // the same 43.1 ms and reduce 0.3 ms less) and chunks of at most ~1152 cells: the fabric / HBM-side traffic of the main kernel drops 3x (config 3:
    // FETCH_SIZE 1.82e8 -> 5.99e7 KiB per launch) at an unchanged step time (the main kernel gains what the 1.3 ms of extra partial-slab reduction
    // cost; 1.0 point less culling because every chunk warms its thresholds up anew).  Partial slabs: one 9.8 MB slab per chunk on config 3,
    // 869 chunks = 8.5 GB under the 12 GiB cap (it was 2 GiB = 219 chunks until round 3).
    static const int64_t kChunkRounds = [] { const char *e = is3d::dev_env("IS3D_CHUNK_ROUNDS"); const int v = e ? atoi(e) : 0; return (int64_t)(v > 0 ? v : 12); }();   // dev A/B
    P.nch_max = is3d::chunk_count(kChunkRounds, (int64_t)lane_waves * P.jtiles * P.ktiles, pc, o->cell_chunks, (int64_t)P.J * P.Kacc * P.Lpad * (int64_t)sizeof(double));
    return IS3D_OK;
}

// one stream or slab of the plan: out of device memory is reported with the sizes that decide it
static int plan_big_alloc(is3d_plan &P, DevBuf<double> &buf, size_t count, const char *what)
{
    const hipError_t e = buf.alloc(count);
    if (e == hipErrorOutOfMemory) return is3d::oom_report(what, count * sizeof(double), P.pass_cells, P.bytes_per_cell, P.nch_max);
    if (e != hipSuccess) return fail(IS3D_ENODEVICE, "hipMalloc(%s) failed: %s", what, hipGetErrorString(e));
    return IS3D_OK;
}

// ---- allocation: the streams of one pass, the partial slabs, the status words, the modified-equilibrium workspaces ----
static int plan_allocate(is3d_plan &P, const is3d_options *o)
{
    const size_t pc = (size_t)P.pass_cells;
    if (P.variant != 1) {
        // unpredicated direct-to-LDS staging over-reads a short last batch (cf_main_tile3e, cf_main_tile variant 8)
        const size_t slack = (size_t)is3d::tile3e_stream_slack_doubles(P.JT, P.KT) + 16 * (size_t)is3d::unit_rec_doubles(P.JT, P.KT, 1);
        if (int rc = plan_big_alloc(P, P.d_TS, pc * P.jtiles * P.rblocks * is3d::unit_rec_doubles(P.JT, P.KT, (P.baryon && !P.feqmod) ? 1 : 0) + slack, "the unit-record stream")) return rc;
        if (P.e2tab) {
            if (int rc = plan_big_alloc(P, P.d_TE, pc * P.jtiles * is3d::kE2Stride * P.JT + slack, "the E2 table stream")) return rc;
            P.ub3e = is3d::tile3e_units_per_batch(P.JT, P.KT, P.npT, P.wpb, P.baryon ? 1 : 0, P.variant == 10 ? 1 : P.variant == 12 ? 2 : 0);
            if (P.ub3e < 1) return fail(IS3D_EINVAL, "kernel_variant 5: a unit record plus its %d x %d E2 table does not fit the LDS budget", P.npT, P.JT);
        }
    } else {
        HIP_TRY(P.d_S1.alloc(pc * P.K * is3d::kS1Rec));
        HIP_TRY(P.d_S2.alloc(pc * P.J * is3d::kS2Rec));
        HIP_TRY(P.d_S3.alloc(pc * P.J * P.K));
    }
    if (int rc = plan_big_alloc(P, P.d_partial, (size_t)(P.nch_max + is3d::kTaperExtra /* the tapered tail: chunk_plan */) * P.J * P.Kacc * P.Lpad, "the per-chunk partial spectra")) return rc;
    if (P.e2tab) HIP_TRY(P.d_cull_floor.alloc((size_t)P.jtiles * P.ktiles * P.Lpad));
    HIP_TRY(P.d_status.alloc(8));
    HIP_TRY(P.d_sticky.upload(std::vector<unsigned long long>{~0ULL, ~0ULL}));
    if (P.feqmod) {
        HIP_TRY(P.d_FB.alloc(pc * is3d::kFbRec));
        HIP_TRY(P.d_flag.alloc(pc));
        HIP_TRY(P.d_list.alloc(pc));
        HIP_TRY(P.d_count.alloc(1));
        if (o->df_mode == 3) {
            HIP_TRY(P.d_CR.alloc(pc * is3d::kCrRec));
            HIP_TRY(P.d_RN.alloc(pc * P.ncls));
        }
    }
    P.workspace = (int64_t)(P.d_S1.n + P.d_S2.n + P.d_S3.n + P.d_TS.n + P.d_TE.n + P.d_partial.n + P.d_FB.n + P.d_CR.n + P.d_RN.n) * (int64_t)sizeof(double) +
                  (int64_t)(P.d_flag.n + P.d_list.n) * (int64_t)sizeof(int32_t);
    return IS3D_OK;
}

static int plan_create_impl(is3d_plan **out, const is3d_species *sp, const is3d_grid *g, const is3d_df_tables *df,
                            const is3d_feqmod_tables *fq, const is3d_options *o, int64_t max_cells)
{
    if (!out) return fail(IS3D_EINVAL, "null plan pointer");
    *out = nullptr;
    int rc = validate(sp, g, df, fq, o);
    if (rc) return rc;
    if (max_cells < 1) max_cells = 1;
    if (max_cells > (int64_t)1 << 40) return fail(IS3D_EINVAL, "max_cells too large");
    if (is3d_device_count() < 1) return fail(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");

    std::unique_ptr<is3d_plan> P(new is3d_plan);
    is3d::count_resource(0);
    P->opts = *o;
    if (o->device >= 0) HIP_TRY(hipSetDevice(o->device));
    HIP_TRY(hipGetDevice(&P->device));
    P->dim3 = (o->dimension == 3);
    P->ce = (o->df_mode == 2);
    P->feqmod = fq != nullptr;
    P->npart = sp->n;
    P->npT = g->n_pT;
    P->J = g->n_phi;
    P->K = P->dim3 ? g->n_y : g->n_eta;
    P->Kacc = P->dim3 ? P->K : 1;
    P->ny_eff = P->Kacc;
    P->nout = (int64_t)P->npart * P->npT * P->J * P->ny_eff;
    P->prefactor = std::pow(2.0 * M_PI * is3d::kHbarC, -3);  // smooth_kernels.cpp:36
    // species classes: identical (mass, sign) => identical integrand up to the degeneracy; with include_baryon the baryon number enters f_eq
    // and delta-f, so it is part of the class key
    P->baryon = o->include_baryon != 0;
    P->baryondiff = P->baryon && o->include_baryondiff_deltaf != 0;
    const is3d::SpeciesClasses k = is3d::species_classes(sp->mass, sp->sign, P->baryon ? sp->baryon : nullptr, sp->n, o->collapse_species != 2);
    P->ncls = (int)k.cmass.size();
    P->sp_cls = k.cls;
    P->cls_mass = k.cmass; P->cls_sign = k.csign; P->cls_bar = k.cbar;
    P->pT_grid.assign(g->pT, g->pT + g->n_pT);
    P->sp_deg.assign(sp->degeneracy, sp->degeneracy + sp->n);
    P->Lbins = P->ncls * P->npT;

    plan_choose_kernel(*P, g, o);
    if ((rc = plan_lanes_and_grids(*P, g, o, k))) return rc;
    if ((rc = plan_coefficient_tables(*P, df, o))) return rc;
    if (fq && (rc = plan_feqmod_tables(*P, fq, o, k))) return rc;
    if ((rc = plan_tiling_and_sizing(*P, df, o, max_cells))) return rc;
    if ((rc = plan_allocate(*P, o))) return rc;
    *out = P.release();
    return IS3D_OK;
}

extern "C" int is3d_plan_create(is3d_plan **out, const is3d_species *sp, const is3d_grid *g, const is3d_df_tables *df,
                                const is3d_options *o, int64_t max_cells)
{
    return plan_create_impl(out, sp, g, df, nullptr, o, max_cells);
}

extern "C" int is3d_plan_create_feqmod(is3d_plan **out, const is3d_species *sp, const is3d_grid *g, const is3d_df_tables *df,
                                       const is3d_feqmod_tables *fq, const is3d_options *o, int64_t max_cells)
{
    if (!fq) return fail(IS3D_EINVAL, "null feqmod tables");
    return plan_create_impl(out, sp, g, df, fq, o, max_cells);
}

extern "C" int is3d_probe_shader_clock(int32_t device, double seconds, double *ghz)
{
    if (!ghz || !(seconds > 0.0) || seconds > 10.0) return fail(IS3D_EINVAL, "is3d_probe_shader_clock: ghz == NULL or seconds outside (0, 10]");
    *ghz = 0.0;
    HIP_TRY(hipSetDevice(device));
    int khz = 0;
    HIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device));
    if (khz <= 0) return fail(IS3D_ENODEVICE, "is3d_probe_shader_clock: the device reports no wall clock rate");
    hipStream_t st;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    unsigned long long *d = nullptr, h[16] = {0};
    is3d::count_resource(1);
    hipError_t e = hipMalloc(&d, sizeof h);
    if (e == hipSuccess) e = hipMemsetAsync(d, 0, sizeof h, st);
    if (e == hipSuccess) e = is3d::launch_clock_probe((unsigned long long)(seconds * khz * 1e3), d, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (d) (void)hipFree(d);
    (void)hipStreamDestroy(st);
    if (e != hipSuccess) return fail(IS3D_ENODEVICE, "is3d_probe_shader_clock: %s", hipGetErrorString(e));
    double sum = 0.0;
    int n = 0;
    for (int i = 0; i < 8; i++)
        if (h[2 * i + 1]) { sum += (double)h[2 * i] / (double)h[2 * i + 1]; n++; }
    const double ratio = n ? sum / n : 0.0;                 // shader ticks per reference tick
    *ghz = (ratio > 1.001 || ratio < 0.999) ? ratio * khz * 1e-6 : 0.0;
    return IS3D_OK;
}

extern "C" int is3d_math_probe(int32_t which, int64_t n, const double *x, double *y, int32_t device)
{
    const int arity = is3d::math_probe_arity(which);
    if (arity < 1 || n < 0 || (n > 0 && (!x || !y))) return fail(IS3D_EINVAL, "is3d_math_probe: which in 0..16, n >= 0, non-null arrays");
    if (n % arity) return fail(IS3D_EINVAL, "is3d_math_probe: function %d reads records of %d doubles, n = %lld is no multiple of that", (int)which, arity, (long long)n);
    if (is3d_device_count() < 1) return fail(IS3D_ENODEVICE, "no HIP device visible; this library has no CPU path");
    if (n == 0) return IS3D_OK;
    if (device >= 0) HIP_TRY(hipSetDevice(device));
    DevBuf<double> dx, dy;
    HIP_TRY(dx.alloc((size_t)n));
    HIP_TRY(dy.alloc((size_t)n));
    HIP_TRY(hipMemcpy(dx.p, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(is3d::launch_math_probe(which, n, dx.p, dy.p, nullptr));
    HIP_TRY(hipMemcpy(y, dy.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return IS3D_OK;
}

extern "C" int64_t is3d_plan_output_size(const is3d_plan *P) { return P ? P->nout : 0; }
extern "C" int64_t is3d_plan_workspace_bytes(const is3d_plan *P) { return P ? P->workspace : 0; }
extern "C" const char *is3d_plan_main_kernel_name(const is3d_plan *P)
{
    if (P && P->feqmod) return "cf_main_feqmod";
    return is3d::main_kernel_name(P ? P->variant : 2);
}
extern "C" int is3d_plan_tile_shape(const is3d_plan *P, int32_t *JT, int32_t *R)
{
    if (!P || !JT || !R) return fail(IS3D_EINVAL, "null argument");
    *JT = P->JT;
    *R = P->KT;
    return IS3D_OK;
}
extern "C" int is3d_plan_set_timing(is3d_plan *P, int32_t enable)
{
    if (!P) return fail(IS3D_EINVAL, "null plan");
    P->timing = enable != 0;
    return IS3D_OK;
}
namespace is3d {
int plan_accumulate(const is3d_plan *P) { return P && P->opts.accumulate != 0; }
int plan_device(const is3d_plan *P) { return P ? P->device : -1; }
}
extern "C" void is3d_plan_destroy(is3d_plan *P)
{
    if (!P) return;
    (void)hipSetDevice(P->device);
    delete P;
}

static int chunks_for(const is3d_plan *P, int64_t n)
{
    int64_t by_cells = std::max<int64_t>(1, n / 64);
    return (int)std::max<int64_t>(1, std::min<int64_t>(P->nch_max, by_cells));
}

// ... with the tapered tail of the cell partition (cf_device.h: chunk_cells, chunk_taper): the grid of the main kernel drains in quarter-length
// tasks -- the fixed ~2.7 ms a launch cost beyond its per-cell time (profiles/r04_shard_sizes.json: 329.0 / 166.2 / 85.5 / 43.5 ms main at 1e6 /
// 5e5 / 2.5e5 / 1.25e5 cells; profiles/r04_ab_chunk_taper.log)
static void chunk_plan(const is3d_plan *P, int64_t n, int &nch, int &nsmall)
{
    nch = chunks_for(P, n);
    nsmall = is3d::chunk_taper(n, P->opts.cell_chunks, nch);
}

// cf_prep's parameters for the cells [c0, c0 + nc) of a pass; the caller sets tiled, pds_bound and TE
static is3d::PrepParams fill_prep(const is3d_plan *P, const is3d_cells *cells, int64_t c0, int32_t nc)
{
    const is3d_options &o = P->opts;
    is3d::PrepParams pp{};
    pp.cells = is3d::cell_ptrs(*cells);
    pp.cell0 = c0;
    pp.n_cells = nc;
    pp.J = P->J; pp.K = P->K;
    pp.dim3 = P->dim3; pp.ce = P->ce;
    pp.include_bulk = o.include_bulk_deltaf != 0;
    pp.include_shear = o.include_shear_deltaf != 0;
    pp.baryon = P->baryon; pp.baryondiff = P->baryondiff;
    pp.bil = P->bil;
    pp.cosphi = P->d_cosphi.p; pp.sinphi = P->d_sinphi.p;
    pp.kgrid = P->d_kgrid.p; pp.kweight = P->d_kweight.p; pp.kch = P->d_kch.p; pp.ksh = P->d_ksh.p;
    pp.spl = P->spl;
    pp.S1 = P->d_S1.p; pp.S2 = P->d_S2.p; pp.S3 = P->d_S3.p;
    pp.JT = P->JT; pp.R = P->KT; pp.jtiles = P->jtiles; pp.rblocks = P->rblocks;
    pp.TS = P->d_TS.p;
    pp.mTmax = P->mTmax; pp.kmin = P->kmin; pp.kmax = P->kmax;
    pp.pTmax = P->pTmax; pp.gw2d = P->gw2d;
    pp.status = P->d_status.p;
    pp.pTgrid = P->d_pTgrid.p; pp.npT = P->npT;
    return pp;
}

// the status words of an execute (cf_device.h): [0] min bad cell, [1..5] counters, [6] the |p.dsigma| bound, [7] min cell whose p.u/T can exceed 1e9
static hipError_t status_begin(is3d_plan *P, hipStream_t st)
{
    static const unsigned long long init[8] = {~0ULL, 0ULL, 0ULL, 0ULL, 0ULL, 0ULL, 0ULL, ~0ULL};
    return hipMemcpyAsync(P->d_status.p, init, sizeof init, hipMemcpyHostToDevice, st);
}

// the words read back after the execute: *bad_cell, and IS3D_EDOMAIN (also in *code) for a cell out of the table or of the exponent range
static int status_finish(const is3d_plan *P, const unsigned long long h[8], int64_t *bad_cell, int32_t *code)
{
    *bad_cell = (h[0] == ~0ULL) ? -1 : (int64_t)h[0];
    if (h[7] != ~0ULL && (*bad_cell < 0 || (int64_t)h[7] < *bad_cell)) {
        *bad_cell = (int64_t)h[7];
        *code = IS3D_EDOMAIN;
        return fail(IS3D_EDOMAIN, "cell %lld: p.u/T can exceed 1e9 for the momentum grid (flow velocity / temperature outside the "
                    "kernel's exponent range; the reference's exp() overflows to inf there), or |p.dsigma| can exceed 1e300 (outside the range of "
                    "the power-of-two scale behind the outflow cut)", (long long)*bad_cell);
    }
    if (*bad_cell >= 0) {
        *code = IS3D_EDOMAIN;
        return fail(IS3D_EDOMAIN, "cell %lld: T%s outside the coefficient table (the reference aborts in gsl_spline_eval here)",
                    (long long)*bad_cell, (P->feqmod && P->opts.df_mode == 4) ? " (or bulkPi/P)" : "");
    }
    return IS3D_OK;
}

// one pass of is3d_plan_execute over the cells [c0, c0 + nc), modified equilibrium: prep (+ renormalisation in df_mode 3), the main kernel, then the
// flagged cells with the linearised delta-f; nch / nch_small: the chunk partition of the first pass (chunk_plan)
static int exec_pass_feqmod(is3d_plan *P, const is3d_cells *cells, hipStream_t st, int pass, int64_t c0, int32_t nc, int nch_used, int nch_small)
{
    const is3d_options &o = P->opts;
    is3d::FqPrepParams fp{};
    fp.cells = is3d::cell_ptrs(*cells);
    fp.baryon = P->baryon; fp.baryondiff = P->baryondiff; fp.bil = P->bil;
    fp.cell0 = c0; fp.n_cells = nc; fp.J = P->J; fp.K = P->K;
    fp.dim3 = P->dim3; fp.mode = o.df_mode;
    fp.include_bulk = o.include_bulk_deltaf != 0; fp.include_shear = o.include_shear_deltaf != 0;
    fp.cosphi = P->d_cosphi.p; fp.sinphi = P->d_sinphi.p; fp.kgrid = P->d_kgrid.p; fp.kweight = P->d_kweight.p;
    fp.spl = P->spl;
    fp.nj = P->nj;
    fp.jx = P->d_jonah.p; fp.jl2 = fp.jx + P->nj; fp.jz = fp.jx + 2 * P->nj; fp.jcl = fp.jx + 3 * P->nj; fp.jcz = fp.jx + 4 * P->nj;
    fp.bp_max = P->bp_max;
    fp.mTmax = P->mTmax; fp.kmin = P->kmin; fp.kmax = P->kmax;
    fp.pTmax = P->pTmax; fp.scale_rows = (o.df_mode == 4 && o.outflow != 0) ? 1 : 0;   // cf_main_feqmod's CLAMP instantiations
    fp.ngl = P->ngl; fp.gl = P->d_gl.p;
    fp.detA_min = P->detA_min; fp.mass_pion0 = P->mass_pion0;
    fp.JT = P->JT; fp.R = P->KT; fp.jtiles = P->jtiles; fp.rblocks = P->rblocks;
    fp.TS = P->d_TS.p; fp.CR = P->d_CR.p; fp.FB = P->d_FB.p; fp.flag = P->d_flag.p;
    fp.status = P->d_status.p;
    if (P->timing) HIP_TRY(hipEventRecord(P->ev_list[pass * 3 + 0], st));
    HIP_TRY(is3d::launch_prep_feqmod(fp, st));
    if (o.df_mode == 3)
        HIP_TRY(is3d::launch_feqmod_renorm(P->d_CR.p, P->d_gl.p, P->ngl, P->d_cls_mass.p, P->d_cls_sign.p,
                                           P->baryon ? P->d_cls_baryon.p : nullptr, P->ncls, nc, fp.include_bulk, P->dim3,
                                           P->d_RN.p, st));
    if (P->timing) HIP_TRY(hipEventRecord(P->ev_list[pass * 3 + 1], st));
    is3d::FqMainArgs a{};
    a.TS = P->d_TS.p; a.lane_mT = P->d_mT.p; a.lane_pT = P->d_pT.p; a.lane_sign = P->d_sign.p;
    a.RN = P->d_RN.p; a.lane_cls = P->d_lane_cls.p; a.ncls = P->ncls;
    a.lane_sub = P->d_lane_sub.p; a.g.split = P->split;
    a.lane_b = P->baryon ? P->d_lane_b.p : nullptr;
    a.partial = P->d_partial.p; a.stats = P->d_status.p;
    a.g.upc = P->upc; a.g.zskip = (o.zero_skip == 2) ? 0 : (o.zero_skip == 1 ? 1 : 2); a.g.baryon = 0;
    a.g.n_cells = nc; a.g.J = P->J; a.g.K = P->K; a.g.Lpad = P->Lpad; a.g.wpb = P->wpb;
    a.g.G = (P->Lpad / 64 + P->wpb - 1) / P->wpb;
    a.g.jtiles = P->jtiles; a.g.ktiles = P->ktiles; a.g.nch = nch_used; a.g.nch_small = nch_small;
    a.g.NT = P->jtiles * P->ktiles * nch_used; a.g.Kacc = P->Kacc; a.g.first_pass = (pass == 0);
    HIP_TRY(is3d::launch_main_feqmod(P->variant, P->dim3, o.outflow != 0, o.df_mode == 3, P->baryon ? 1 : 0, a, st));
    // flagged cells (breakdown, narrow rows): ordered list, then the linearised delta-f on top of chunk 0
    HIP_TRY(is3d::launch_feqmod_compact(P->d_flag.p, nc, P->d_list.p, P->d_count.p, P->d_status.p, st));
    is3d::FqLinearArgs la{};
    la.FB = P->d_FB.p; la.list = P->d_list.p; la.count = P->d_count.p;
    la.lane_mT = P->d_mT.p; la.lane_pT = P->d_pT.p; la.lane_sign = P->d_sign.p; la.lane_mass = P->d_lane_mass.p;
    la.lane_b = P->baryon ? P->d_lane_b.p : nullptr;
    la.cosphi = P->d_cosphi.p; la.sinphi = P->d_sinphi.p; la.kgrid = P->d_kgrid.p; la.kweight = P->d_kweight.p;
    la.partial = P->d_partial.p;
    la.J = P->J; la.K = P->K; la.Kacc = P->Kacc; la.Lpad = P->Lpad; la.dim3 = P->dim3; la.mode = o.df_mode; la.Lbins = P->Lbins;
    la.outflow = o.outflow != 0; la.regulate = o.regulate_deltaf != 0;
    HIP_TRY(is3d::launch_feqmod_linear(la, st));
    if (P->timing) HIP_TRY(hipEventRecord(P->ev_list[pass * 3 + 2], st));
    return IS3D_OK;
}

// the same pass for delta-f (df_mode 1, 2): prep, the main kernel -- in two launches around the cull floors with zero_skip 3
static int exec_pass_deltaf(is3d_plan *P, const is3d_cells *cells, hipStream_t st, int pass, int64_t c0, int32_t nc, int nch_used, int nch_small, bool use_scale)
{
    const is3d_options &o = P->opts;
    is3d::PrepParams pp = fill_prep(P, cells, c0, nc);
    pp.tiled = (P->variant != 1);
    pp.pds_bound = use_scale ? P->d_status.p + 6 : nullptr;
    pp.TE = P->e2tab ? P->d_TE.p : nullptr;
    if (P->timing) HIP_TRY(hipEventRecord(P->ev_list[pass * 3 + 0], st));
    HIP_TRY(is3d::launch_prep(pp, st));
    if (P->timing) HIP_TRY(hipEventRecord(P->ev_list[pass * 3 + 1], st));

    is3d::MainArgs a{};
    a.S1 = P->d_S1.p; a.S2 = P->d_S2.p; a.S3 = P->d_S3.p; a.TS = P->d_TS.p;
    a.g.upc = P->upc;
    a.g.zskip = (o.zero_skip == 2) ? 0 : (o.zero_skip == 1 ? 1 : 2);   // 0 default: exact-zero + accumulator-relative culling; 3: + surface-relative floors (below)
    a.lane_mT = P->d_mT.p; a.lane_pT = P->d_pT.p; a.lane_sign = P->d_sign.p; a.lane_b = P->d_lane_b.p;
    a.g.baryon = P->baryon;
    a.lane_pe = P->d_lane_pe.p;
    a.partial = P->d_partial.p;
    a.stats = P->d_status.p;
    a.g.n_cells = nc;
    a.g.J = P->J; a.g.K = P->K;
    a.g.Lpad = P->Lpad;
    a.g.wpb = P->wpb;
    a.g.G = (P->Lpad / 64 + P->wpb - 1) / P->wpb;
    a.g.jtiles = P->jtiles; a.g.ktiles = P->ktiles;
    a.g.nch = nch_used; a.g.nch_small = nch_small;
    a.g.NT = P->jtiles * P->ktiles * nch_used;
    a.g.Kacc = P->Kacc;
    a.g.first_pass = (pass == 0);
    a.TE = P->e2tab ? P->d_TE.p : nullptr; a.lane_ipT = P->d_lane_ipT.p; a.g.npT = P->npT; a.g.ub = P->ub3e; a.pTgrid = P->e2tab ? P->d_pTgrid.p : nullptr;
    a.g.split = P->split; a.lane_sub = P->d_lane_sub.p;
    // zero_skip 3, surface-relative cull (cf_main_tile3e with outflow && regulate_deltaf; include/is3d_amd.h): an eighth of the chunks
    // runs first with the accumulator-relative rule; their partial spectrum is a lower bound of the final one (all terms >= 0) and
    // floors the row-cull thresholds of the other chunks, which would otherwise each start from an empty accumulator
    static const int surf_den = [] { const char *e = is3d::dev_env("IS3D_SURFCULL_DEN"); const int v = e ? atoi(e) : 0; return v >= 2 ? v : 8; }();
    const bool surf = o.zero_skip == 3 && P->e2tab && o.outflow != 0 && o.regulate_deltaf != 0 && nch_used >= 2 * surf_den;
    if (surf) {
        const int nA = nch_used / surf_den;
        a.g.ch0 = 0; a.g.nch_run = nA;
        HIP_TRY(is3d::launch_main(P->variant, P->ce, P->dim3, true, true, a, st));
        HIP_TRY(is3d::launch_cull_floor(P->d_partial.p, nA, P->J, P->K, P->Kacc, P->Lpad, P->JT, P->KT, P->jtiles, P->ktiles, P->d_lane_pe.p,
                                        2.0, P->d_cull_floor.p, st));
        a.g.ch0 = nA; a.g.nch_run = nch_used - nA;
        a.cull_floor = P->d_cull_floor.p;
        HIP_TRY(is3d::launch_main(P->variant, P->ce, P->dim3, true, true, a, st));
    } else {
        HIP_TRY(is3d::launch_main(P->variant, P->ce, P->dim3, o.outflow != 0, o.regulate_deltaf != 0, a, st));
    }
    if (P->timing) HIP_TRY(hipEventRecord(P->ev_list[pass * 3 + 2], st));
    return IS3D_OK;
}

extern "C" int is3d_plan_execute(is3d_plan *P, const is3d_cells *cells, double *dN_out, void *hip_stream, is3d_status *status)
{
    if (!P || !cells || !dN_out) return fail(IS3D_EINVAL, "null argument");
    if (status) { memset(status, 0, sizeof *status); status->bad_cell = -1; }
    const int64_t n = cells->n_cells;
    if (n < 0 || n > P->max_cells) return fail(IS3D_EINVAL, "n_cells = %lld exceeds the plan's max_cells = %lld", (long long)n, (long long)P->max_cells);
    const is3d_options &o = P->opts;
    if (int rc = is3d::check_cells(cells, P->dim3, o, P->baryondiff)) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(P->device));

    const int npasses = n == 0 ? 0 : (int)((n + P->pass_cells - 1) / P->pass_cells);
    if (P->timing) {
        size_t need = (size_t)npasses * 3 + 1;
        while (P->ev_list.size() < need) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            P->ev_list.push_back(e);
        }
    }
    P->last_passes = npasses;
    HIP_TRY(status_begin(P, st));

    int nch_used = 1, nch_small = 0;
    // tiled delta-f stream: p.dsigma travels times 2^-e (status[6] = bits of the bound, cf_device.h)
    const bool use_scale = !P->feqmod && P->variant != 1;
    if (n == 0) {
        // empty surface: spectrum is zero (reference: loops do not execute)
        if (!o.accumulate) HIP_TRY(hipMemsetAsync(dN_out, 0, (size_t)P->nout * sizeof(double), st));
    } else {
        // all passes use the chunk count of the first (largest) pass so that partial slots line up
        chunk_plan(P, std::min<int64_t>(n, P->pass_cells), nch_used, nch_small);
        if (use_scale) {
            HIP_TRY(is3d::launch_pds_bound(is3d::cell_ptrs(*cells), n, P->dim3, P->kmin, P->kmax, P->gw2d, P->mTmax, P->pTmax, P->d_status.p + 6, st));
        }
        for (int pass = 0; pass < npasses; pass++) {
            const int64_t c0 = (int64_t)pass * P->pass_cells;
            const int32_t nc = (int32_t)std::min<int64_t>(P->pass_cells, n - c0);
            const int rc = P->feqmod ? exec_pass_feqmod(P, cells, st, pass, c0, nc, nch_used, nch_small)
                                     : exec_pass_deltaf(P, cells, st, pass, c0, nc, nch_used, nch_small, use_scale);
            if (rc) return rc;
        }
        HIP_TRY(is3d::launch_finalize(P->d_partial.p, P->d_cls.p, P->d_degeneracy.p, dN_out, P->nout, P->npart, P->npT, P->J,
                                      P->Kacc, P->Lpad, nch_used, P->prefactor, o.accumulate != 0,
                                      use_scale ? P->d_status.p + 6 : nullptr, st, P->split, P->Lbins));
        if (P->timing) HIP_TRY(hipEventRecord(P->ev_list[npasses * 3], st));
    }

    // executes that return their domain errors through `status` do not leave them for a later is3d_plan_check as well
    if (n > 0 && !status) HIP_TRY(is3d::launch_fold_status(P->d_status.p, P->d_sticky.p, st));
    if (status) {
        unsigned long long h[8];
        HIP_TRY(hipMemcpyAsync(h, P->d_status.p, sizeof h, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        status->n_classes = P->ncls;
        status->n_passes = npasses;
        status->kernel_variant = P->variant;
        status->n_cells_skipped = (int64_t)h[1];
        status->n_wave_rows = (int64_t)h[2];
        status->n_wave_rows_culled = (int64_t)h[3];
        status->n_cells_breakdown = (int64_t)h[4];
        status->n_cells_narrow = (int64_t)h[5];
        return status_finish(P, h, &status->bad_cell, &status->code);
    }
    return IS3D_OK;
}

extern "C" int is3d_plan_check(is3d_plan *P, void *hip_stream, int64_t *bad_cell)
{
    if (!P) return fail(IS3D_EINVAL, "null plan");
    if (bad_cell) *bad_cell = -1;
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(P->device));
    unsigned long long h[2], reset[2] = {~0ULL, ~0ULL};
    HIP_TRY(hipMemcpyAsync(h, P->d_sticky.p, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(P->d_sticky.p, reset, sizeof reset, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    const unsigned long long first = std::min(h[0], h[1]);
    if (first == ~0ULL) return IS3D_OK;
    if (bad_cell) *bad_cell = (int64_t)first;
    if (h[1] <= h[0])
        return fail(IS3D_EDOMAIN, "cell %llu (of an execute since the last check): p.u/T can exceed 1e9 for the momentum grid (the reference's exp() "
                    "overflows to inf there), or |p.dsigma| can exceed 1e300; the cell was left out of the spectrum", first);
    return fail(IS3D_EDOMAIN, "cell %llu (of an execute since the last check): T%s outside the coefficient table; the cell was left out of the "
                "spectrum (the reference aborts in gsl_spline_eval here)", first, (P->feqmod && P->opts.df_mode == 4) ? " (or bulkPi/P)" : "");
}

extern "C" int is3d_plan_observables(is3d_plan *P, const double *dN_dev, const double *pT_w, const double *phi_w, double *dNdy_dev,
                                     double *dN2pipTdpTdy_dev, double *vn_dev, void *hip_stream)
{
    if (!P || !dN_dev || !phi_w) return fail(IS3D_EINVAL, "null argument");
    if (dNdy_dev && !pT_w) return fail(IS3D_EINVAL, "dN/dy needs the pT weights");
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(P->device));
    HIP_TRY(hipMemcpyAsync(P->d_phiw.p, phi_w, (size_t)P->J * sizeof(double), hipMemcpyHostToDevice, st));
    if (pT_w) HIP_TRY(hipMemcpyAsync(P->d_pTw.p, pT_w, (size_t)P->npT * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_TRY(is3d::launch_observables(dN_dev, P->d_phiw.p, P->d_pTw.p, P->d_coskphi.p, P->d_sinkphi.p, dNdy_dev, dN2pipTdpTdy_dev,
                                     vn_dev, P->npart, P->npT, P->J, P->ny_eff, st));
    return IS3D_OK;
}

extern "C" int is3d_plan_timings(is3d_plan *P, is3d_status *status)
{
    if (!P || !status) return fail(IS3D_EINVAL, "null argument");
    status->ms_prep = status->ms_main = status->ms_finalize = 0.0;
    if (!P->timing || P->last_passes == 0) return IS3D_OK;
    HIP_TRY(hipSetDevice(P->device));
    HIP_TRY(hipEventSynchronize(P->ev_list[P->last_passes * 3]));
    for (int pass = 0; pass < P->last_passes; pass++) {
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, P->ev_list[pass * 3 + 0], P->ev_list[pass * 3 + 1]));
        HIP_TRY(hipEventElapsedTime(&b, P->ev_list[pass * 3 + 1], P->ev_list[pass * 3 + 2]));
        status->ms_prep += a;
        status->ms_main += b;
    }
    float c = 0;
    HIP_TRY(hipEventElapsedTime(&c, P->ev_list[(P->last_passes - 1) * 3 + 2], P->ev_list[P->last_passes * 3]));
    status->ms_finalize = c;
    status->n_passes = P->last_passes;
    status->kernel_variant = P->variant;
    status->n_classes = P->ncls;
    return IS3D_OK;
}

// ---------------------------------------------------------------------------------------------
// one-shot host entry
// ---------------------------------------------------------------------------------------------
static int smooth_spectra_impl(const is3d_cells *cells, const is3d_species *species, const is3d_grid *grid,
                               const is3d_df_tables *df, const is3d_feqmod_tables *fq, const is3d_options *opts, double *dN_out,
                               is3d_status *status)
{
    if (!cells || !dN_out) return fail(IS3D_EINVAL, "null argument");
    is3d_plan *P = nullptr;
    int rc = plan_create_impl(&P, species, grid, df, fq, opts, std::max<int64_t>(cells->n_cells, 1));
    if (rc) { if (status) { memset(status, 0, sizeof *status); status->code = rc; status->bad_cell = -1; } return rc; }
    struct Guard { is3d_plan *p; ~Guard() { is3d_plan_destroy(p); } } guard{P};
    (void)is3d_plan_set_timing(P, 1);

    const int64_t n = cells->n_cells;
    const bool diff = opts->include_baryon && opts->include_baryondiff_deltaf;
    const auto keep = [diff](int a) { return a < 18 || diff; };   // the diffusion arrays only when they are read
    DevBuf<double> dcell, dout;
    HIP_TRY(dcell.alloc((size_t)std::max<int64_t>(n, 1) * is3d::kCellArrays));
    HIP_TRY(dout.alloc((size_t)P->nout));
    hipEvent_t e0, e1, e2, e3;
    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); HIP_TRY(hipEventCreate(&e2)); HIP_TRY(hipEventCreate(&e3));
    struct EvGuard { hipEvent_t e[4]; ~EvGuard() { for (auto x : e) (void)hipEventDestroy(x); } } evg{{e0, e1, e2, e3}};
    HIP_TRY(hipEventRecord(e0, nullptr));
    is3d_cells dc;
    HIP_TRY(is3d::stage_cells(*cells, keep, 0, n, dcell.p, nullptr, &dc));
    if (opts->accumulate) HIP_TRY(hipMemcpyAsync(dout.p, dN_out, (size_t)P->nout * sizeof(double), hipMemcpyHostToDevice, nullptr));
    HIP_TRY(hipEventRecord(e1, nullptr));
    is3d_status st{};
    rc = is3d_plan_execute(P, &dc, dout.p, nullptr, &st);
    if (rc) { if (status) *status = st; return rc; }
    HIP_TRY(hipEventRecord(e2, nullptr));
    HIP_TRY(hipMemcpyAsync(dN_out, dout.p, (size_t)P->nout * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipEventRecord(e3, nullptr));
    HIP_TRY(hipEventSynchronize(e3));
    (void)is3d_plan_timings(P, &st);
    float h2d = 0, d2h = 0;
    HIP_TRY(hipEventElapsedTime(&h2d, e0, e1));
    HIP_TRY(hipEventElapsedTime(&d2h, e2, e3));
    st.ms_h2d = h2d;
    st.ms_d2h = d2h;
    st.code = IS3D_OK;
    if (status) *status = st;
    return IS3D_OK;
}

extern "C" int is3d_smooth_spectra(const is3d_cells *cells, const is3d_species *species, const is3d_grid *grid,
                                   const is3d_df_tables *df, const is3d_options *opts, double *dN_out, is3d_status *status)
{
    return smooth_spectra_impl(cells, species, grid, df, nullptr, opts, dN_out, status);
}

extern "C" int is3d_smooth_spectra_feqmod(const is3d_cells *cells, const is3d_species *species, const is3d_grid *grid,
                                          const is3d_df_tables *df, const is3d_feqmod_tables *fq, const is3d_options *opts,
                                          double *dN_out, is3d_status *status)
{
    if (!fq) return fail(IS3D_EINVAL, "null feqmod tables");
    return smooth_spectra_impl(cells, species, grid, df, fq, opts, dN_out, status);
}

// ---------------------------------------------------------------------------------------------
// operation 0: smooth spacetime distributions (calculate_dN_dX, emissionfunction_smooth_kernels.cpp:1000-1446), cf_spacetime.hip
// ---------------------------------------------------------------------------------------------
static int st_check(const is3d_spacetime_bins *b, const double *x, const double *y, int df_mode, bool feqmod = false)
{
    if (!feqmod && (df_mode == 3 || df_mode == 4))
        return fail(IS3D_EINVAL, "operation 0 with df_mode %d is calculate_dN_dX_feqmod: use is3d_spacetime_distributions_feqmod / "
                    "is3d_plan_execute_spacetime_feqmod (this entry takes df_mode 1 or 2)", df_mode);
    if (feqmod && df_mode != 3 && df_mode != 4)
        return fail(IS3D_EINVAL, "the feqmod entries of operation 0 take df_mode 3 or 4 (got %d)", df_mode);
    return is3d::spacetime_check_bins(b, x, y);
}

// the 2+1D eta rows' share of LDS: the feqmod kernel keeps 16 KiB of the 64 for its staged records
static size_t st_lds_cap(bool feqmod) { return (feqmod ? 48 : 64) * 1024; }

// the breakdown cells' workgroup slots of cf_st_fq_linear (2+1D: eta partial slots after the chunks')
static int st_linear_slots(int64_t nc) { return (int)std::max<int64_t>(1, std::min<int64_t>(64, nc)); }

// one pass of df_mode 1 / 2: before the first, the |p.dsigma| bound of the surface; the records; the per-cell stage
static int st_pass_viscous(is3d_plan *P, const is3d_cells *cells, is3d::StSplit *split, hipStream_t st, int pass, int64_t c0, int32_t nc, int nch,
                           const is3d::StMark &mark)
{
    const is3d_options &o = P->opts;
    const is3d::StState &S = P->st;
    const int K = P->K;
    if (pass == 0) {
        HIP_TRY(is3d::launch_pds_bound(is3d::cell_ptrs(*cells), cells->n_cells, P->dim3, P->kmin, P->kmax, P->gw2d, P->mTmax, P->pTmax,
                                       P->d_status.p + 6, st));
        if (split && split->exchange) {
            // a shard: the records take the scale of the WHOLE surface, so that they -- and D -- are the single-device ones bit for bit
            unsigned long long mine = 0, all = 0;
            HIP_TRY(hipMemcpyAsync(&mine, P->d_status.p + 6, sizeof mine, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (int rc = split->exchange(mine, &all)) return rc;
            HIP_TRY(hipMemcpyAsync(P->d_status.p + 6, &all, sizeof all, hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));   // `all` goes out of scope
        }
    }
    is3d::PrepParams pp = fill_prep(P, cells, c0, nc);
    pp.tiled = 1;
    pp.pds_bound = P->d_status.p + 6;
    pp.TE = nullptr;   // the E2 tables of cf_main_tile3e are not needed here
    HIP_TRY(is3d::launch_prep(pp, st));
    HIP_TRY(mark(0));

    is3d::StCellArgs a{};
    a.TS = P->d_TS.p; a.nc = nc; a.J = P->J; a.K = K; a.jtiles = P->jtiles; a.rblocks = P->rblocks;
    a.ncls = P->ncls; a.npTp = S.npTp; a.nlw = S.nlw; a.G = (S.nlw + 3) / 4; a.nch = (int)std::min<int64_t>(nch, nc);
    a.outflow = o.outflow != 0; a.regulate = o.regulate_deltaf != 0; a.zskip = o.zero_skip != 2;
    a.lane_mT = S.d_mT.p; a.lane_pT = S.d_pT.p; a.lane_sign = S.d_sign.p; a.lane_b = S.d_b.p; a.lane_wpT = S.d_wpT.p;
    a.wphi = S.d_wphi.p; a.pds_bound = P->d_status.p + 6;
    a.D = S.d_D.p; a.eta_slab = P->dim3 ? nullptr : S.d_slab.p;
    HIP_TRY(is3d::launch_spacetime_cells(a, P->ce, P->dim3, P->baryon, P->JT, P->KT, st));
    if (!P->dim3) HIP_TRY(is3d::launch_spacetime_eta_reduce(S.d_slab.p, a.nch, (int64_t)P->ncls * K, pass == 0, S.d_eta.p, st));
    HIP_TRY(mark(1));
    return IS3D_OK;
}

// one pass of df_mode 3 / 4: the feqmod records (operation 0's form; they carry p.dsigma unscaled), df_mode 3 renormalisation, per-cell stage,
// breakdown cells
static int st_pass_feqmod(is3d_plan *P, const is3d_cells *cells, hipStream_t st, int pass, int64_t c0, int32_t nc, int nch, const is3d::StMark &mark)
{
    const is3d_options &o = P->opts;
    const is3d::StState &S = P->st;
    const int K = P->K, G = (S.nlw + 3) / 4, GL = st_linear_slots(S.pass);
    is3d::FqPrepParams fp{};
    fp.cells = is3d::cell_ptrs(*cells);
    fp.baryon = P->baryon; fp.baryondiff = P->baryondiff; fp.bil = P->bil;
    fp.cell0 = c0; fp.n_cells = nc; fp.J = P->J; fp.K = K;
    fp.dim3 = P->dim3; fp.mode = o.df_mode;
    fp.include_bulk = o.include_bulk_deltaf != 0; fp.include_shear = o.include_shear_deltaf != 0;
    fp.cosphi = P->d_cosphi.p; fp.sinphi = P->d_sinphi.p; fp.kgrid = P->d_kgrid.p; fp.kweight = P->d_kweight.p;
    fp.spl = P->spl;
    fp.nj = P->nj;
    fp.jx = P->d_jonah.p; fp.jl2 = fp.jx + P->nj; fp.jz = fp.jx + 2 * P->nj; fp.jcl = fp.jx + 3 * P->nj; fp.jcz = fp.jx + 4 * P->nj;
    fp.bp_max = P->bp_max;
    fp.mTmax = P->mTmax; fp.kmin = P->kmin; fp.kmax = P->kmax;
    fp.pTmax = P->pTmax; fp.scale_rows = 0;   // D holds the unscaled value: no power-of-two row scale
    fp.ngl = P->ngl; fp.gl = P->d_gl.p;
    fp.detA_min = P->detA_min; fp.mass_pion0 = P->mass_pion0;
    fp.JT = P->JT; fp.R = P->KT; fp.jtiles = P->jtiles; fp.rblocks = P->rblocks;
    fp.TS = P->d_TS.p; fp.CR = P->d_CR.p; fp.FB = P->d_FB.p; fp.flag = P->d_flag.p;
    fp.status = P->d_status.p;
    HIP_TRY(is3d::launch_prep_feqmod(fp, st, true));
    HIP_TRY(mark(0));
    if (o.df_mode == 3) {
        HIP_TRY(is3d::launch_feqmod_renorm(P->d_CR.p, P->d_gl.p, P->ngl, P->d_cls_mass.p, P->d_cls_sign.p,
                                           P->baryon ? P->d_cls_baryon.p : nullptr, P->ncls, nc, fp.include_bulk, P->dim3,
                                           P->d_RN.p, st, P->d_status.p + 2));
        HIP_TRY(mark(3));
    }
    is3d::StFqCellArgs a{};
    a.TS = P->d_TS.p; a.nc = nc; a.J = P->J; a.K = K; a.jtiles = P->jtiles; a.rblocks = P->rblocks;
    a.ncls = P->ncls; a.npTp = S.npTp; a.nlw = S.nlw; a.G = G; a.nch = (int)std::min<int64_t>(nch, nc);
    a.zskip = o.zero_skip != 2;
    a.lane_mT = S.d_mT.p; a.lane_pT = S.d_pT.p; a.lane_sign = S.d_sign.p; a.lane_b = S.d_b.p; a.lane_wpT = S.d_wpT.p;
    a.wphi = S.d_wphi.p; a.RN = o.df_mode == 3 ? P->d_RN.p : nullptr;
    a.D = S.d_D.p; a.eta_slab = P->dim3 ? nullptr : S.d_slab.p;
    HIP_TRY(is3d::launch_spacetime_feqmod_cells(a, P->dim3, o.df_mode == 3, P->baryon, o.outflow != 0, P->JT, P->KT, st));
    HIP_TRY(mark(1));
    HIP_TRY(is3d::launch_feqmod_compact(P->d_flag.p, nc, P->d_list.p, P->d_count.p, P->d_status.p, st));
    is3d::StFqLinearArgs la{};
    la.FB = P->d_FB.p; la.list = P->d_list.p; la.count = P->d_count.p;
    la.lane_mT = S.d_mT.p; la.lane_pT = S.d_pT.p; la.lane_sign = S.d_sign.p; la.lane_mass = S.d_mass.p;
    la.lane_b = P->baryon ? S.d_b.p : nullptr; la.lane_wpT = S.d_wpT.p;
    la.cosphi = P->d_cosphi.p; la.sinphi = P->d_sinphi.p; la.wphi = S.d_wphi.p; la.kgrid = P->d_kgrid.p; la.kweight = P->d_kweight.p;
    la.RN = o.df_mode == 3 ? P->d_RN.p : nullptr;
    la.nc = nc; la.J = P->J; la.K = K; la.ncls = P->ncls; la.npTp = S.npTp; la.nlw = S.nlw; la.G = G; la.GL = GL; la.nch = a.nch;
    la.dim3 = P->dim3; la.mode = o.df_mode; la.outflow = o.outflow != 0; la.regulate = o.regulate_deltaf != 0;
    la.D = S.d_D.p; la.eta_slab = P->dim3 ? nullptr : S.d_slab.p;
    HIP_TRY(is3d::launch_spacetime_feqmod_linear(la, st));
    if (!P->dim3) HIP_TRY(is3d::launch_spacetime_eta_reduce(S.d_slab.p, a.nch + GL, (int64_t)P->ncls * K, pass == 0, S.d_eta.p, st));
    HIP_TRY(mark(4));
    return IS3D_OK;
}

static int st_execute(is3d_plan *P, const is3d_cells *cells, const double *x, const double *y, const double *pT_w, const double *phi_w,
                      const is3d_spacetime_bins *bins, const is3d_spacetime_out *out, void *hip_stream, is3d_spacetime_stats *stats,
                      is3d_spacetime_feqmod_stats *fstats, is3d::StSplit *split = nullptr)
{
    if (stats) { memset(stats, 0, sizeof *stats); stats->bad_cell = -1; }
    if (fstats) { memset(fstats, 0, sizeof *fstats); fstats->first_cell_out_of_range = -1; }
    // the halves of an execute (cf_spacetime.h): a shard's per-cell stage into the assembled D, or the bin stage over it
    const bool do_cells = !split || split->role == is3d::ST_CELLS, do_bins = !split || split->role == is3d::ST_BINS;
    if (!P || !cells || (do_bins && !out) || (do_cells && (!pT_w || !phi_w))) return fail(IS3D_EINVAL, "null argument");
    if (split && (!split->D_full || split->n_total < cells->n_cells + split->c_off || split->c_off < 0)) return fail(IS3D_EINVAL, "bad split");
    int rc = do_bins ? st_check(bins, x, y, P->opts.df_mode, P->feqmod) : IS3D_OK;
    if (rc) return rc;
    if (P->feqmod ? !is3d::spacetime_feqmod_shape_supported(P->dim3, P->JT, P->KT) : !is3d::spacetime_shape_supported(P->dim3, P->JT, P->KT))
        return fail(IS3D_EINVAL, "operation 0 runs on the plan's unit records of the default tile shapes (this plan: kernel variant %d, %d x %d "
                    "records for %d %s nodes)", P->variant, P->JT, P->KT, P->K, P->dim3 ? "y" : "eta");
    rc = is3d::spacetime_check_grid(P->dim3, st_lds_cap(P->feqmod), P->npT, P->K);
    if (!rc && do_bins) rc = is3d::spacetime_check_out(out);
    if (rc) return rc;
    const int64_t n = cells->n_cells;
    if (n < 0 || (do_cells && n > P->max_cells)) return fail(IS3D_EINVAL, "n_cells = %lld exceeds the plan's max_cells = %lld", (long long)n, (long long)P->max_cells);
    if (n > 0x7fff0000LL) return fail(IS3D_EINVAL, "operation 0 takes up to 2^31 cells");
    const is3d_options &o = P->opts;
    rc = do_cells ? is3d::check_cells(cells, P->dim3, o, P->baryondiff) : IS3D_OK;
    if (rc) return rc;
    hipStream_t st = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(P->device));
    is3d::StSetup su{};
    su.ncls = P->ncls; su.npT = P->npT; su.J = P->J; su.K = P->K; su.dim3 = P->dim3; su.jtiles = P->jtiles; su.JT = P->JT; su.npart = P->npart;
    su.cls_mass = P->cls_mass.data(); su.cls_sign = P->cls_sign.data(); su.cls_bar = P->cls_bar.data();
    su.pT_grid = P->pT_grid.data(); su.sp_deg = P->sp_deg.data(); su.sp_cls = P->sp_cls.data();
    su.prefactor = P->prefactor;
    su.bytes_per_cell = (int64_t)P->bytes_per_cell; su.pass_cells = P->pass_cells; su.workspace_bytes = o.workspace_bytes;
    su.mass_lanes = P->feqmod; su.b_lanes = true; su.pad = is3d::ST_PAD_UNIT;
    rc = is3d::spacetime_setup(P->st, su);
    // an execute with the same weights and stats == NULL does not block the host
    if (!rc && do_cells) rc = is3d::spacetime_upload_weights(P->st, pT_w, phi_w, st);
    if (rc) return rc;

    unsigned long long h[8];
    is3d::StRun r{};
    r.bs.tau = cells->tau; r.bs.ux = cells->ux; r.bs.uy = cells->uy; r.bs.un = cells->un;
    r.bs.dat = cells->dat; r.bs.dax = cells->dax; r.bs.day = cells->day; r.bs.dan = cells->dan; r.bs.x = x; r.bs.y = y;
    r.bs.n = n; r.bs.bins = bins; r.bs.out = out; r.bs.all_cells = 0;
    r.linear_slots = P->feqmod ? st_linear_slots(P->st.pass) : 0;
    r.kweight = P->d_kweight.p; r.device = P->device; r.split = split; r.stream = st;
    r.d_status = P->d_status.p; r.d_sticky = P->d_sticky.p; r.status = h; r.stats = stats;
    if (fstats) { r.ms_renorm = &fstats->ms_renorm; r.ms_linear = &fstats->ms_linear; }
    r.pass = [=](int pass, int64_t c0, int32_t nc, int nch, const is3d::StMark &mark) {
        return P->feqmod ? st_pass_feqmod(P, cells, st, pass, c0, nc, nch, mark) : st_pass_viscous(P, cells, split, st, pass, c0, nc, nch, mark);
    };
    rc = is3d::spacetime_run(P->st, r);
    if (rc || !stats) return rc;
    if (fstats && n > 0) {
        fstats->n_cells_breakdown = (int64_t)h[4];
        fstats->n_renorm_skipped = (int64_t)h[2] * (o.df_mode == 4 ? P->ncls : 1);   // df_mode 4: whole cells (cf_prep_feqmod)
        fstats->first_cell_out_of_range = h[7] == ~0ULL ? -1 : (int64_t)h[7];
    }
    stats->n_cells_skipped = n == 0 ? 0 : (int64_t)h[1];
    return status_finish(P, h, &stats->bad_cell, &stats->code);
}

extern "C" int is3d_plan_execute_spacetime(is3d_plan *P, const is3d_cells *cells, const double *x, const double *y, const double *pT_w,
                                           const double *phi_w, const is3d_spacetime_bins *bins, const is3d_spacetime_out *out, void *hip_stream,
                                           is3d_spacetime_stats *stats)
{
    return st_execute(P, cells, x, y, pT_w, phi_w, bins, out, hip_stream, stats, nullptr);
}

extern "C" int is3d_plan_execute_spacetime_feqmod(is3d_plan *P, const is3d_cells *cells, const double *x, const double *y, const double *pT_w,
                                                  const double *phi_w, const is3d_spacetime_bins *bins, const is3d_spacetime_out *out,
                                                  void *hip_stream, is3d_spacetime_stats *stats, is3d_spacetime_feqmod_stats *fstats)
{
    if (P && !P->feqmod) {
        if (stats) { memset(stats, 0, sizeof *stats); stats->bad_cell = -1; }
        if (fstats) { memset(fstats, 0, sizeof *fstats); fstats->first_cell_out_of_range = -1; }
        return fail(IS3D_EINVAL, "is3d_plan_execute_spacetime_feqmod needs a plan of is3d_plan_create_feqmod (df_mode 3 or 4)");
    }
    // the counters need the stream's status words: an execute with fstats reports them as one with stats does
    is3d_spacetime_stats local{};
    return st_execute(P, cells, x, y, pT_w, phi_w, bins, out, hip_stream, stats ? stats : (fstats ? &local : nullptr), fstats);
}

// the argument checks of the one-shot entries (and of the entry that shards the cells over devices, cf_multi.hip) that need no plan, in the
// order of their refusals: bins, grid, what plan creation would refuse, outputs.  No device is touched
static int st_check_args(const is3d_species *species, const is3d_grid *grid, const is3d_df_tables *df, const is3d_feqmod_tables *fq,
                         const is3d_options *opts, const is3d_spacetime_bins *bins, const double *x, const double *y, const is3d_spacetime_out *out)
{
    int rc = st_check(bins, x, y, opts->df_mode, fq != nullptr);
    if (!rc && fq && opts->include_baryon && opts->df_mode == 4)
        rc = fail(IS3D_EINVAL, "df_mode 4 does not work with include_baryon = 1 (the reference exits there too)");
    if (!rc && fq) rc = validate(species, grid, df, fq, opts);
    if (!rc && grid && (opts->dimension == 2 || opts->dimension == 3))
        rc = is3d::spacetime_check_grid(opts->dimension == 3, st_lds_cap(fq != nullptr), grid->n_pT, grid->n_eta);
    if (!rc && !fq) rc = validate(species, grid, df, nullptr, opts);
    return rc ? rc : is3d::spacetime_check_out(out);
}

static int st_oneshot(const is3d_cells *cells, const double *x, const double *y, const is3d_species *species, const is3d_grid *grid,
                      const double *pT_w, const double *phi_w, const is3d_df_tables *df, const is3d_feqmod_tables *fq, const is3d_options *opts,
                      const is3d_spacetime_bins *bins, is3d_spacetime_out *out, is3d_spacetime_stats *stats, is3d_spacetime_feqmod_stats *fstats)
{
    if (stats) { memset(stats, 0, sizeof *stats); stats->bad_cell = -1; }
    if (fstats) { memset(fstats, 0, sizeof *fstats); fstats->first_cell_out_of_range = -1; }
    if (!cells || !out || !opts || !pT_w || !phi_w) return fail(IS3D_EINVAL, "null argument");
    int rc = st_check_args(species, grid, df, fq, opts, bins, x, y, out);
    if (rc) { if (stats) stats->code = rc; return rc; }
    is3d_plan *P = nullptr;
    rc = plan_create_impl(&P, species, grid, df, fq, opts, std::max<int64_t>(cells->n_cells, 1));
    if (rc) { if (stats) stats->code = rc; return rc; }
    struct Guard { is3d_plan *p; ~Guard() { is3d_plan_destroy(p); } } guard{P};
    const bool diff = opts->include_baryon && opts->include_baryondiff_deltaf;
    return is3d::spacetime_oneshot(*cells, x, y, [diff](int a) { return a < 18 || diff; }, P->npart, P->dim3 ? 1 : P->K, bins, out, stats,
                                   [&](const is3d_cells &dc, const double *dx, const double *dy, const is3d_spacetime_out &dev,
                                       is3d_spacetime_stats *stt) { return st_execute(P, &dc, dx, dy, pT_w, phi_w, bins, &dev, nullptr, stt, fstats); });
}

namespace is3d {
int spacetime_check_args(const is3d_cells *cells, const double *x, const double *y, const is3d_species *species, const is3d_grid *grid,
                         const double *pT_w, const double *phi_w, const is3d_df_tables *df, const is3d_feqmod_tables *fq, const is3d_options *opts,
                         const is3d_spacetime_bins *bins, const is3d_spacetime_out *out)
{
    if (!cells || !out || !opts || !pT_w || !phi_w) return fail(IS3D_EINVAL, "null argument");
    if (int rc = st_check_args(species, grid, df, fq, opts, bins, x, y, out)) return rc;
    if (cells->n_cells < 0) return fail(IS3D_EINVAL, "n_cells < 0");
    if (cells->n_cells > 0x7fff0000LL) return fail(IS3D_EINVAL, "operation 0 takes up to 2^31 cells");
    return check_cells(cells, opts->dimension == 3, *opts, opts->include_baryon && opts->include_baryondiff_deltaf);
}
int spacetime_execute_split(is3d_plan *plan, const is3d_cells *cells, const double *x, const double *y, const double *pT_w, const double *phi_w,
                            const is3d_spacetime_bins *bins, const is3d_spacetime_out *out, void *hip_stream, is3d_spacetime_stats *stats,
                            StSplit *split)
{
    if (!split || (split->role != ST_CELLS && split->role != ST_BINS)) return fail(IS3D_EINVAL, "bad split");
    return st_execute(plan, cells, x, y, pT_w, phi_w, bins, out, hip_stream, stats, nullptr, split);
}
int plan_classes(const is3d_plan *P) { return P ? P->ncls : 0; }
double *plan_st_eta(const is3d_plan *P) { return P ? P->st.d_eta.p : nullptr; }
}  // namespace is3d

extern "C" int is3d_spacetime_distributions(const is3d_cells *cells, const double *x, const double *y, const is3d_species *species,
                                            const is3d_grid *grid, const double *pT_w, const double *phi_w, const is3d_df_tables *df,
                                            const is3d_options *opts, const is3d_spacetime_bins *bins, is3d_spacetime_out *out,
                                            is3d_spacetime_stats *stats)
{
    return st_oneshot(cells, x, y, species, grid, pT_w, phi_w, df, nullptr, opts, bins, out, stats, nullptr);
}

extern "C" int is3d_spacetime_distributions_feqmod(const is3d_cells *cells, const double *x, const double *y, const is3d_species *species,
                                                   const is3d_grid *grid, const double *pT_w, const double *phi_w, const is3d_df_tables *df,
                                                   const is3d_feqmod_tables *fq, const is3d_options *opts, const is3d_spacetime_bins *bins,
                                                   is3d_spacetime_out *out, is3d_spacetime_stats *stats, is3d_spacetime_feqmod_stats *fstats)
{
    if (!fq) {
        if (stats) { memset(stats, 0, sizeof *stats); stats->bad_cell = -1; stats->code = IS3D_EINVAL; }
        if (fstats) { memset(fstats, 0, sizeof *fstats); fstats->first_cell_out_of_range = -1; }
        return fail(IS3D_EINVAL, "null feqmod tables");
    }
    return st_oneshot(cells, x, y, species, grid, pT_w, phi_w, df, fq, opts, bins, out, stats, fstats);
}

/*
 * is3d_amd.h -- C ABI of the MI355X-native smooth Cooper-Frye spectra path.
 *
 * The reference (derekeverett/iS3D) has no FFI layer; the boundary this library is a drop-in for
 * is the C++ method
 *
 *   void EmissionFunctionArray::calculate_dN_pTdpTdphidy(double *Mass, double *Sign,
 *        double *Degeneracy, double *Baryon, double *T_fo, double *P_fo, double *E_fo,
 *        double *tau_fo, double *eta_fo, double *ux_fo, double *uy_fo, double *un_fo,
 *        double *dat_fo, double *dax_fo, double *day_fo, double *dan_fo, double *pixx_fo,
 *        double *pixy_fo, double *pixn_fo, double *piyy_fo, double *piyn_fo, double *bulkPi_fo,
 *        double *muB_fo, double *nB_fo, double *Vx_fo, double *Vy_fo, double *Vn_fo,
 *        Deltaf_Data *df_data)
 *   declared  src/cpp/emissionfunction.h:179, defined src/cpp/emissionfunction_smooth_kernels.cpp:28-393,
 *   called    src/cpp/emissionfunction.cpp:1519,
 *
 * whose implicit inputs are members of the object (FO_length, number_of_chosen_particles, the
 * pT/phi/y/eta Tables, DIMENSION, DF_MODE, OUTFLOW, REGULATE_DELTAF, INCLUDE_* --
 * src/cpp/emissionfunction.h:73-90, :139-142) and whose output is the member array
 * dN_pTdpTdphidy (emissionfunction.h:142), index
 *   iS3D = ipart + npart * (ipT + npT * (iphip + nphi * iy))      (smooth_kernels.cpp:363)
 * Every implicit input is an explicit argument here.  Plain pointers and sizes only.
 *
 * Conventions
 *   - all functions return IS3D_OK (0) or a negative IS3D_E* code; nothing calls exit()/abort()
 *     (reference: printf + exit(-1), GSL abort);  is3d_last_error() has the text;
 *   - the caller owns every buffer; the library never frees or keeps caller memory past a call
 *     (a plan keeps its own device copies of species/grid/tables);
 *   - pointers for disabled corrections (muB, nB, Vx, Vy, Vn; eta in 2+1D) may be NULL and are
 *     never dereferenced (reference passes uninitialised pointers there, emissionfunction.cpp:1357-1378);
 *   - dN_out has n_species * n_pT * n_phi * n_y_eff doubles, n_y_eff = (dimension == 2) ? 1 : n_y,
 *     species fastest; it is OVERWRITTEN unless opts->accumulate (reference semantics: +=, :375);
 *   - thread-safe for distinct plans; one plan serves one call at a time;
 *   - there is NO CPU fallback: without a HIP device every compute entry returns IS3D_ENODEVICE.
 */
#ifndef IS3D_AMD_H
#define IS3D_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IS3D_OK 0
#define IS3D_EINVAL (-1)     /* bad argument / unsupported option combination            */
#define IS3D_ENODEVICE (-2)  /* no HIP device, or a HIP runtime error (see last_error)    */
#define IS3D_EDOMAIN (-3)    /* a non-skipped cell's T is outside the coefficient table, */
                             /* or its flow is so fast that p.u/T can exceed 1e9         */
                             /* (reference: GSL domain error -> abort, deltafReader.cpp:339) */
#define IS3D_ENOMEM (-4)
#define IS3D_EIO (-5)        /* host reader/writer failure                               */
#define IS3D_EPEER (-6)      /* multi-GPU: another rank's execute failed before the all-reduce; the sum is incomplete */

/* Freezeout cells, structure of arrays, fp64, length n_cells each.  Replaces the *_fo pointer
 * arguments of calculate_dN_pTdpTdphidy (emissionfunction.h:179).  Units as after the reader's
 * hbar*c conversion (GeV, GeV/fm^3; readindata.cpp:367-410). */
typedef struct {
    int64_t n_cells;                    /* FO_length (emissionfunction.h:139) */
    const double *tau, *eta;            /* eta unused (may be NULL) when dimension == 2 */
    const double *dat, *dax, *day, *dan; /* covariant dsigma_mu */
    const double *ux, *uy, *un;         /* contravariant u^mu; u^tau recomputed (:133) */
    const double *T, *P, *E;
    const double *pixx, *pixy, *pixn, *piyy, *piyn; /* other components reconstructed (:166-170) */
    const double *bulkPi;
    const double *muB, *nB, *Vx, *Vy, *Vn; /* only read if include_baryon && include_baryondiff_deltaf (:186-197) */
} is3d_cells;

/* Replaces Mass, Sign, Degeneracy, Baryon (emissionfunction.cpp:1293-1307) */
typedef struct {
    int32_t n;                          /* number_of_chosen_particles */
    const double *mass, *sign, *degeneracy, *baryon;
} is3d_species;

/* Replaces pT_tab, phi_tab, y_tab, eta_tab column 1 (and eta weights, column 2)
 * (smooth_kernels.cpp:40-92).  cos/sin(phi) are formed inside, as the reference does. */
typedef struct {
    int32_t n_pT;  const double *pT;
    int32_t n_phi; const double *phi;
    int32_t n_y;   const double *y;     /* used when dimension == 3 */
    int32_t n_eta; const double *eta, *eta_w; /* used when dimension == 2 */
} is3d_grid;

/* Replaces Deltaf_Data: the coefficient tables as loaded by load_df_coefficient_data
 * (deltafReader.cpp:120-197), still carrying their temperature scaling (c0*T^4, c1*T^3, c2*T^4, c3*T^4,
 * c4*T^5, F/T, G, betabulk/T^4, betaV/T^3, betapi/T^4).  Every table is [n_muB][n_T], T fastest, row 0 =
 * the lowest mu_B (= 0 in the shipped files).
 *   include_baryon = 0: only row 0 of c0, c2 (df_mode 1) or F, betabulk, betapi (df_mode 2) is read
 *     (n_muB may be 1, the other pointers NULL); natural cubic splines in T are built inside
 *     (construct_cubic_splines, deltafReader.cpp:300-322; cubic_spline, :325-395).
 *   include_baryon = 1: bilinear interpolation in (T, mu_B) over the full grids of c0..c4 (df_mode 1) or
 *     F, G, betabulk, betaV, betapi (df_mode 2) (bilinear_interpolation, :412-484) -- with the intended
 *     [imuB][iT] indexing; the reference's calculate_bilinear swaps the two indices (:404-407). */
typedef struct {
    int32_t n_T;
    const double *T;                    /* GeV, ascending, uniform */
    int32_t n_muB;
    const double *muB;                  /* GeV, ascending, uniform; may be NULL when include_baryon = 0 */
    const double *c0, *c1, *c2, *c3, *c4;           /* df_mode 1 */
    const double *F, *G, *betabulk, *betaV, *betapi; /* df_mode 2 */
} is3d_df_tables;

/* Extra inputs of the modified-equilibrium path (df_mode 3, 4): replaces the Gauss_Laguerre *laguerre argument of
 * calculate_dN_ptdptdphidy_feqmod (emissionfunction.h:182), the PDG/Plasma inputs of
 * Deltaf_Data::compute_jonah_coefficients (deltafReader.cpp:222-297) and the members DETA_MIN, MASS_PION0
 * (emissionfunction.cpp:184, :188). */
typedef struct {
    int32_t n_gla;                      /* Gauss-Laguerre points per alpha (32 in tables/gla_roots_weights_32_points.txt) */
    const double *root1, *weight1;      /* alpha = 1 (Gauss_Laguerre::load_roots_and_weights, readindata.cpp:24-53) */
    const double *root2, *weight2;      /* alpha = 2 */
    int32_t n_pdg;                      /* ALL species of the PDG file (df_mode 4: the z(Pi/P), lambda(Pi/P) tables sum over them) */
    const double *pdg_mass, *pdg_degeneracy, *pdg_sign;
    double T_avg;                       /* Plasma::temperature: the surface average as read back from
                                           average_thermodynamic_quantities.dat (df_mode 4) */
    double deta_min;                    /* parameter deta_min */
    double mass_pion0;                  /* parameter mass_pion0 */
} is3d_feqmod_tables;

typedef struct {
    int32_t dimension;                  /* 2 | 3                      DIMENSION  */
    int32_t df_mode;                    /* 1 14-moment | 2 Chapman-Enskog | 3 modified equilibrium (Mike) | 4 (Jonah);
                                           3 and 4 only through the *_feqmod entries; 4 needs include_baryon = 0, as in the
                                           reference (deltafReader.cpp:470-474)                             DF_MODE */
    int32_t include_baryon;             /* 1: mu_B/T in f_eq, bilinear (T, mu_B) coefficients (muB_fo; with
                                           include_baryondiff_deltaf also nB_fo, Vx_fo, Vy_fo, Vn_fo) */
    int32_t include_bulk_deltaf;
    int32_t include_shear_deltaf;
    int32_t include_baryondiff_deltaf;  /* ignored unless include_baryon */
    int32_t regulate_deltaf;
    int32_t outflow;
    int32_t accumulate;                 /* 0: dN_out = result; 1: dN_out += result (reference) */
    int32_t device;                     /* HIP device ordinal; -1 = current device */
    /* tuning; 0 = library default */
    int32_t kernel_variant;             /* 0 default: 6 in 3+1D (pT grids of up to 32 values: the 8x7 tile with the phi-side exponentials read
                                           from a table stream and the rows of a unit tested for liveness before their exponentials; larger pT
                                           grids: 3, the 8x7 tile without the table -- 2, 6x7, with baryon slots), 7 in 2+1D (8x31 tile, unit-strided
                                           lanes); modified equilibrium (df_mode 3, 4): 3 in 3+1D, 7 in 2+1D.  The shipped library holds these
                                           kernels and honours one explicit choice -- 3 for a 3+1D delta-f surface without baryon slots; ANY other
                                           request runs the default, and status.kernel_variant says which kernel ran.  The A/B forms of rounds 1-5
                                           (1 direct kernel | 2, 4 other tile shapes | 5 hand-pipelined rows | 8 register-staged LDS copy | 9 unit
                                           records on the scalar path | 10 E2 column from global memory | 11 raw header values as FMA operands | 12 E2 tables built per workgroup in LDS | modified equilibrium: 5, 6 other row
                                           walks, 2-4 the 61-row tiles) exist only in the developer build of the library (make DEV=1) */
    int32_t cell_chunks;                /* number of cell chunks the main kernel grid is split into; 0 (default): the library's count, with
                                           a tapered tail (the last chunks a quarter of the size of the others); > 0: that many equal chunks */
    int64_t workspace_bytes;            /* cap on the derived-coefficient workspace per pass; 0: max(16 GiB, 45 % of the device's TOTAL memory) --
                                           the total, not what is free at the moment, so that the pass / chunk count (and with it the
                                           summation order) of a large surface does not depend on the GPU's other tenants.  An
                                           allocation that does not fit returns IS3D_ENOMEM naming the sizes */
    int32_t collapse_species;           /* 0 default(on) | 1 on | 2 off: evaluate one representative per
                                           distinct (mass, sign) and scale by degeneracy */
    int32_t zero_skip;                  /* wave-level culling of rows that cannot change the result (bitwise-identical spectra
                                           in all three settings): 1: rows whose exp(-p.u/T) is exactly +0; 0 (default): also
                                           rows whose every term is below half an ulp of every accumulator it would be added to
                                           (delta-f tile kernel with outflow && regulate_deltaf); 2: off; 3: as 0, and in the 3+1D
                                           delta-f kernel (cf_main_tile3e, outflow && regulate_deltaf, >= 16 cell chunks) an eighth of
                                           the chunks runs first and its partial spectrum -- a lower bound of the final one, every term
                                           being >= 0 -- floors the thresholds of the rest.  NOT bitwise: a skipped term is below 2^-57 of
                                           the final value of every bin it belongs to, the spectrum can lose at most n_cells 2^-57 of a
                                           bin (7e-12 at 1e6 cells), one-sided.  Measured on BASELINE config 3: 59.5 instead of 57.3 % of
                                           the wave-rows culled, main kernel -2.2 %, 6 of 4.9e6 bins differ by one ulp */
    int32_t waves_per_group;            /* 0 default | 2, 4, 8: lane-waves per workgroup of the tile kernel (they share
                                           one LDS-staged coefficient stream) | 1: one-wave workgroups, no barrier partner
                                           (variants 5, 6 only) */
    int32_t reference_bilinear_indexing; /* include_baryon = 1 only.  0 (default): the (T, mu_B) coefficient tables are read [imuB][iT], as they
                                           are stored.  1: bug-compatible with the reference's calculate_bilinear, which reads f_data[iT][imuB]
                                           (deltafReader.cpp:404-407) from arrays allocated [points_muB][points_T] (:36-61): the value at
                                           (mu_B row iT, T column imuB).  Reproduced wherever that read is inside the allocation
                                           (iT + 1 < n_muB, i.e. T < T[n_muB - 1] = 0.18 GeV on the shipped 101 x 81 grids); a live cell
                                           beyond it gives IS3D_EDOMAIN (the reference reads past its row pointers there: undefined) */
    int32_t reserved[4];
} is3d_options;

typedef struct {
    int32_t code;                       /* same as the return value */
    int32_t n_classes;                  /* distinct (mass, sign) classes actually evaluated */
    int64_t n_cells_skipped;            /* cells with u.dsigma <= 0 (contribute 0, :137) */
    int64_t bad_cell;                   /* first cell index with T outside the table, or -1 */
    int32_t n_passes;                   /* workspace passes over the cell axis */
    int32_t kernel_variant;             /* variant that ran */
    double ms_prep, ms_main, ms_finalize; /* device time of the three kernels (HIP events), summed over passes;
                                             filled by is3d_plan_timings / the host entry, else 0 */
    double ms_h2d, ms_d2h;              /* host entry only */
    int64_t n_wave_rows;                /* (cell, row, wave) triples the tile kernel visited ...          */
    int64_t n_wave_rows_culled;         /* ... and how many it skipped as exactly zero (zero_skip)        */
    int64_t n_cells_breakdown;          /* df_mode 3: cells where feqmod breaks down (linearised delta-f used, the count
                                           the reference prints, smooth_kernels.cpp:983-986)              */
    int64_t n_cells_narrow;             /* df_mode 3, 4 in 3+1D: cells with detA < 0.01, whose rows |y - eta| < detA use
                                           the linearised delta-f (:807-813)                               */
} is3d_status;

typedef struct is3d_plan is3d_plan;

const char *is3d_last_error(void);
const char *is3d_version(void);
/* number of visible HIP devices (>= 0), never fails */
int is3d_device_count(void);

/*
 * One-shot host entry: what a maintainer calls from calculate_dN_pTdpTdphidy.  All pointers are
 * HOST memory.  Uploads the cell arrays, runs prep -> main -> finalize on the device, downloads
 * the spectrum.
 */
int is3d_smooth_spectra(const is3d_cells *cells, const is3d_species *species, const is3d_grid *grid,
                        const is3d_df_tables *df, const is3d_options *opts, double *dN_out,
                        is3d_status *status);

/* The same for df_mode 3 / 4: what a maintainer calls from calculate_dN_ptdptdphidy_feqmod
 * (emissionfunction.h:182, smooth_kernels.cpp:396-996, call site emissionfunction.cpp:1584).  df needs betapi
 * (df_mode 4) or F, betabulk, betapi (df_mode 3), row 0. */
int is3d_smooth_spectra_feqmod(const is3d_cells *cells, const is3d_species *species, const is3d_grid *grid,
                               const is3d_df_tables *df, const is3d_feqmod_tables *fq, const is3d_options *opts,
                               double *dN_out, is3d_status *status);

/*
 * Device-resident API.  A plan holds the species classes, grids and spline tables on the device and
 * the workspaces sized for up to max_cells cells per execute.
 */
int is3d_plan_create(is3d_plan **plan, const is3d_species *species, const is3d_grid *grid,
                     const is3d_df_tables *df, const is3d_options *opts, int64_t max_cells);
/* plan for df_mode 3 / 4; execute, observables, timings as for any plan.  df_mode 4 builds the 301-point
 * lambda(Pi/P), z(Pi/P) tables on the host here (deltafReader.cpp:222-297), ~0.1 s. */
int is3d_plan_create_feqmod(is3d_plan **plan, const is3d_species *species, const is3d_grid *grid,
                            const is3d_df_tables *df, const is3d_feqmod_tables *fq, const is3d_options *opts,
                            int64_t max_cells);
/* length of dN_out in doubles */
int64_t is3d_plan_output_size(const is3d_plan *plan);
/* cells->* and dN_out are DEVICE pointers on the plan's device; hip_stream is a hipStream_t (NULL =
 * default stream).  Asynchronous with respect to the host except for the final status read-back
 * when status != NULL (then the stream is synchronised). */
int is3d_plan_execute(is3d_plan *plan, const is3d_cells *cells, double *dN_out, void *hip_stream,
                      is3d_status *status);
/* Domain errors of executes that ran with status == NULL (fully asynchronous: nothing is read back, a cell whose T leaves the
 * coefficient table is left out of the spectrum and the call returns IS3D_OK).  The plan keeps the lowest offending cell index of
 * all executes since the last check; this call synchronises hip_stream, returns IS3D_EDOMAIN (and *bad_cell, index within its
 * execute's cells; may be NULL) if there was one, and clears the record.  The reference aborts on such a cell (GSL domain error /
 * exit(-1)): a caller that skips the status must ask here before trusting the spectrum. */
int is3d_plan_check(is3d_plan *plan, void *hip_stream, int64_t *bad_cell);
/* Derived observables from a device-resident spectrum of this plan's shape (what the reference's writers reduce on
 * the host: emissionfunction.cpp:639-677, :729-772, :1053-1136).  pT_w / phi_w: HOST arrays of the quadrature weights
 * (column 2 of the pT / phi tables).  Outputs are DEVICE arrays, any may be NULL:
 *   dNdy          [n_species][n_y_eff]            sum_phi sum_pT w_phi w_pT dN
 *   dN2pipTdpTdy  [n_species][n_y_eff][n_pT]      sum_phi w_phi dN / (2 pi)
 *   vn            [n_species][n_y_eff][n_pT][7]   |sum_phi w_phi e^{i k phi} dN| / sum_phi w_phi dN, k = 1..7 (0 if the
 *                                                 denominator is below 1e-15)
 * Asynchronous on hip_stream. */
int is3d_plan_observables(is3d_plan *plan, const double *dN_dev, const double *pT_w, const double *phi_w, double *dNdy,
                          double *dN2pipTdpTdy, double *vn, void *hip_stream);
/* Enable (1) / disable (0) HIP-event timing of the three kernels on subsequent executes. */
int is3d_plan_set_timing(is3d_plan *plan, int32_t enable);
/* Synchronises the recorded events of the last execute and fills status->ms_*. */
int is3d_plan_timings(is3d_plan *plan, is3d_status *status);

/* Diagnostic (no reference counterpart): the shader clock a kernel actually runs at.  Launches one idle wave per XCD on a
 * private non-blocking stream of `device`; each reads the shader-clock counter (s_memtime) and the constant-rate counter
 * (s_memrealtime) `seconds` apart and the call returns the mean ratio in GHz.  Called from a second host thread while a
 * spectra kernel runs on another stream, it gives the clock that kernel's fp64 roofline should be priced at
 * (bench.py: roofline_valu.shader_clock_ghz).  *ghz = 0 if the two counters tick at the same rate on this device. */
int is3d_probe_shader_clock(int32_t device, double seconds, double *ghz);
/* Diagnostic (no reference counterpart): the elementary functions the kernels are built from (is3d_amd/csrc/cf_math.h), evaluated on the
 * device, y[i] = f(x[i]) for HOST arrays of n doubles -- so that their accuracy is a tested number, not a comment.  which: 0 exp_full
 * (Cody-Waite, degree 10) | 1 exp_p9 (one-fma reduction, degree 9; |x| < 1.4e9) | 2 exp_p9_sat | 3 exp_full_sat (|x| up to ~1e45) | 4 sqrt_g1 (v_rsq_f64 +
 * one Goldschmidt step) | 5 sqrt_nr | 6 rcp_nr1 (v_rcp_f64 + one Newton step) | 7 rcp_nr (two steps) | 8 exp_p9_scaled with e = 5 (32 e^x: the
 * power-of-two factor cf_main_feqmod takes out of p.dsigma comes back through the exponential's shift constant).
 * Functions of several arguments read records of `arity` consecutive doubles from x and write one result per record slot; n must be a
 * multiple of the arity (IS3D_EINVAL otherwise).  9 add_clamp01 (a, b) | 10 fma_clamp01 (a, b, c) | 11 fma_clamp01_half (a, b): the add / fma
 * with the VOP3 clamp modifier that forms max(p.dsigma 2^-e, 0), min(max(fl(a b + c), 0), 1) with NaN -> 0, the value repeated over the
 * record | 12 exp_p9_scaled (v, e): 2^e exp_p9(v) for an integer e, repeated over the record | 13, 14, 15, 16 rcp_batch<RB> with RB = 2, 3,
 * 4, 8: slot i of a record gets 1 / x_i from the batch's one shared reciprocal. */
int is3d_math_probe(int32_t which, int64_t n, const double *x, double *y, int32_t device);
/* Diagnostic (no reference counterpart): process-wide counts of the plans this library has created (is3d_plan_create*, the per-shard plans of
 * is3d_multi_plan_create and of the one-shot entries) and of the device allocations (hipMalloc) it has made, since the library was loaded.  What a
 * persistent plan promises -- a second execute creates nothing and allocates nothing -- is checked with these, not with a wall clock.  Either
 * pointer may be NULL. */
int is3d_resource_counters(int64_t *plans_created, int64_t *device_allocations);
/* Name of the dominant kernel as it appears in rocprofv3 traces, for the variant in use. */
const char *is3d_plan_main_kernel_name(const is3d_plan *plan);
/* tile of the main kernel: *JT phi's x *R rows (y's in 3+1D, eta nodes in 2+1D) */
int is3d_plan_tile_shape(const is3d_plan *plan, int32_t *JT, int32_t *R);
/* bytes of device workspace the plan holds */
int64_t is3d_plan_workspace_bytes(const is3d_plan *plan);
void is3d_plan_destroy(is3d_plan *plan);

/* ---------------------------------------------------------------------------------------------
 * Multi-GPU.  The reference is single-process; its spectrum is a plain sum over freezeout cells
 * (src/cpp/emissionfunction_smooth_kernels.cpp:363-375: dN_pTdpTdphidy[iS3D] += chunk sum), so the cell axis shards:
 * contiguous blocks of cells per GPU, no data-path collective, one sum of the n_species x n_bins spectrum at the end.
 * Two forms:
 *   (1) one process, several devices: is3d_smooth_spectra_multi -- one host thread + stream per shard;
 *   (2) one process per GPU (MPI / torchrun style hosts): an is3d_comm (RCCL communicator) + is3d_plan_execute_allreduce.
 * RCCL (librccl.so.1) is loaded on first use; a host that never asks for it does not need it installed.
 * --------------------------------------------------------------------------------------------- */
#define IS3D_REDUCE_ORDERED 0   /* shard spectra are added pairwise in a fixed binary tree by a device kernel (the partner's spectrum
                                   read over hipMemcpyPeer): round r adds shard i + 2^r into shard i for every i that is a multiple of
                                   2^(r+1) -- ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)) for eight shards -- the pairs of a round
                                   run concurrently on their own devices.  Bitwise reproducible for a given shard count, whatever
                                   the devices; a device may be listed more than once */
#define IS3D_REDUCE_RCCL 1      /* ncclAllReduce(ncclDouble, ncclSum) over a communicator of the listed devices (distinct) */

/* Host entry over several devices: what is3d_smooth_spectra / is3d_smooth_spectra_feqmod (fq != NULL: df_mode 3, 4) compute,
 * with the cells split into n_devices contiguous shards (sizes differ by at most one cell), shard s on devices[s].
 *   devices == NULL: ordinals 0 .. n_devices-1;  n_devices <= 0: every visible device.  opts->device is ignored.
 *   Every in-process multi-device entry reads its list by this one rule: more than 1024 shards, a negative ordinal and n_devices beyond the
 *   visible count with devices == NULL are IS3D_EINVAL before any device is used (so with or without one), then no visible device is
 *   IS3D_ENODEVICE, then an ordinal beyond the visible count IS3D_EINVAL; the message names devices[i] or n_devices.
 *   status (may be NULL): counters summed over the shards, bad_cell = lowest global cell index, ms_prep / ms_main / ms_finalize /
 *   ms_h2d = the slowest shard's, ms_d2h = reduction + download;  shard_status (may be NULL): n_devices entries, one per shard
 *   (bad_cell is shard-local there).
 * All shards run concurrently.  With one shard and IS3D_REDUCE_ORDERED this is is3d_smooth_spectra on devices[0]. */
int is3d_smooth_spectra_multi(const is3d_cells *cells, const is3d_species *species, const is3d_grid *grid,
                              const is3d_df_tables *df, const is3d_feqmod_tables *fq, const is3d_options *opts,
                              const int32_t *devices, int32_t n_devices, int32_t reduce, double *dN_out,
                              is3d_status *status, is3d_status *shard_status);
/* shard [*lo, *hi) of `rank` among n_ranks contiguous shards of n_cells cells (the split is3d_smooth_spectra_multi uses) */
int is3d_shard_bounds(int64_t n_cells, int32_t rank, int32_t n_ranks, int64_t *lo, int64_t *hi);

/* RCCL communicator for one-process-per-GPU hosts.  Rank 0 calls is3d_comm_unique_id and ships the 128 bytes to the other
 * ranks by whatever the host already has (MPI_Bcast, a torch.distributed store, a file); then every rank calls
 * is3d_comm_create (collective: ncclCommInitRank) with its HIP device. */
typedef struct is3d_comm is3d_comm;
#define IS3D_COMM_ID_BYTES 128
int is3d_comm_unique_id(uint8_t id[IS3D_COMM_ID_BYTES]);
int is3d_comm_create(is3d_comm **comm, const uint8_t id[IS3D_COMM_ID_BYTES], int32_t n_ranks, int32_t rank, int32_t device);
int is3d_comm_rank(const is3d_comm *comm, int32_t *rank, int32_t *n_ranks);
/* in-place sum over all ranks of n doubles at dN_dev (DEVICE pointer on the communicator's device), asynchronous on hip_stream:
 * the "+=" of smooth_kernels.cpp:375 across shards (ncclAllReduce, ncclDouble, ncclSum). */
int is3d_comm_allreduce(is3d_comm *comm, double *dN_dev, int64_t n, void *hip_stream);
void is3d_comm_destroy(is3d_comm *comm);
/* is3d_plan_execute on this rank's shard of the cells, then the sum of dN_out over the ranks on the same stream (ncclAllReduce):
 * every rank ends with the spectrum of the whole surface.  comm == NULL: plain is3d_plan_execute.  The plan must have been created
 * with opts.accumulate = 0 (the old contents would be summed n_ranks times): IS3D_EINVAL otherwise.
 * Failures.  A one-double error word is summed next to the spectrum (same RCCL group):
 *   - a rank whose execute fails in a way that leaves its stream usable (IS3D_EDOMAIN; IS3D_EINVAL for a bad shard or plan option)
 *     still joins -- after a domain error with the cells it could evaluate, after an argument error with zeros -- with its error word
 *     set, and returns its own error code;
 *   - the other ranks learn of it: with status != NULL (the call synchronises anyway) they return IS3D_EPEER; with status == NULL
 *     (fully asynchronous) at the next is3d_comm_check;
 *   - a rank that cannot join (dN_out or plan NULL, a HIP error) calls ncclCommAbort on its OWN communicator before it returns
 *     (unusable afterwards: every call returns IS3D_ENODEVICE) and its host should exit non-zero so that the launcher ends the job.
 *     Its abort is local: RCCL enqueues an all-reduce and returns at once, and nothing tells the peers' kernels that a rank will never
 *     arrive.  What protects the PEERS is their own deadline: every host-side wait the library makes behind a collective
 *     (the status read-back of this call, is3d_comm_check, is3d_comm_timings, is3d_comm_synchronize) polls the stream together with
 *     ncclCommGetAsyncError and, on an asynchronous RCCL error or after the communicator's timeout (is3d_comm_set_timeout; default 300 s,
 *     or IS3D_COMM_TIMEOUT_S at is3d_comm_create), aborts this rank's communicator and returns IS3D_ENODEVICE instead of blocking for ever.
 *     A host that synchronises the stream itself (hipStreamSynchronize) has no such deadline: use is3d_comm_synchronize. */
int is3d_plan_execute_allreduce(is3d_plan *plan, const is3d_cells *shard, double *dN_out, is3d_comm *comm, void *hip_stream,
                                is3d_status *status);
/* Error words of the collectives since the last check (waits for hip_stream, with the communicator's deadline): IS3D_OK, or IS3D_EPEER with
 * *n_failed (may be NULL) = how many rank-executes had failed before their all-reduce -- this rank's own failures included; IS3D_ENODEVICE
 * when the wait hit an asynchronous RCCL error or the deadline (the communicator is aborted then). */
int is3d_comm_check(is3d_comm *comm, void *hip_stream, int32_t *n_failed);
/* ncclCommAbort on this rank's communicator: for a host that has to leave a job.  Local -- the other ranks find out through their own
 * deadline (see is3d_plan_execute_allreduce), not through this call. */
int is3d_comm_abort(is3d_comm *comm);
/* Deadline, in seconds, of the host-side waits behind this communicator's collectives (default 300).  What it times (round 5): with ONE collective
 * enqueued since the last completed wait -- the usual step: execute, all-reduce, wait -- the clock starts when the stream REACHES the collective
 * (an event recorded just before it), so this rank's own kernels queued ahead of it do not count, however long they run.  With several collectives
 * queued before one wait, and as a backstop while the collective has not been reached, the wait gives up 20 x `seconds` after it was entered: a caller
 * that queues many steps before it waits must choose `seconds` above 1/20 of the compute it queues. */
int is3d_comm_set_timeout(is3d_comm *comm, double seconds);
/* hipStreamSynchronize(hip_stream) with that deadline and with ncclCommGetAsyncError polled beside it: IS3D_OK when everything enqueued on
 * the stream has finished, IS3D_ENODEVICE (communicator aborted) on an asynchronous RCCL error or when the deadline passes. */
int is3d_comm_synchronize(is3d_comm *comm, void *hip_stream);
/* Device time of the last collective on this rank (HIP events on its stream around the RCCL group; it includes the wait for the
 * slowest rank).  Waits for the closing event (with the communicator's deadline). */
int is3d_comm_timings(is3d_comm *comm, double *ms_allreduce);

/* Persistent form of is3d_smooth_spectra_multi: one plan, one workspace, one stream, the device blocks for cells and spectrum and
 * (IS3D_REDUCE_RCCL) the communicator set per shard are created ONCE; every execute then only uploads its cells, runs the shards concurrently and sums the
 * spectra.  max_cells bounds cells->n_cells of any execute.  The result of an execute is bitwise the one is3d_smooth_spectra_multi
 * returns for the same arguments. */
typedef struct is3d_multi_plan is3d_multi_plan;
int is3d_multi_plan_create(is3d_multi_plan **mplan, const is3d_species *species, const is3d_grid *grid, const is3d_df_tables *df,
                           const is3d_feqmod_tables *fq, const is3d_options *opts, const int32_t *devices, int32_t n_devices,
                           int32_t reduce, int64_t max_cells);
int is3d_multi_plan_execute(is3d_multi_plan *mplan, const is3d_cells *cells, double *dN_out, is3d_status *status,
                            is3d_status *shard_status);
int32_t is3d_multi_plan_shards(const is3d_multi_plan *mplan);
int64_t is3d_multi_plan_output_size(const is3d_multi_plan *mplan);
void is3d_multi_plan_destroy(is3d_multi_plan *mplan);

/* ---------------------------------------------------------------------------------------------
 * Anisotropic hydro (VAH, P_L matching): replaces EmissionFunctionArray::calculate_dN_pTdpTdphidy_VAH_PL
 * (src/cpp/emissionfunction.h, src/cpp/emissionfunction_smooth_kernels.cpp:2140-2393).  The reference never calls it (call
 * site commented out, emissionfunction.cpp:1650-1654) and src/cpp never loads the VAH coefficient tables: the per-cell
 * 14-moment coefficients c0..c4 are inputs, as in the method's own signature.  All ten pi_perp^{mu nu} components are inputs
 * too (this kernel does not reconstruct them); T is accepted and unused.  No outflow cut, no skipped cells.  opts: dimension,
 * include_bulk_deltaf, include_shear_deltaf, regulate_deltaf, accumulate, device, workspace_bytes, cell_chunks, collapse_species,
 * zero_skip (exact zeros only on this path: 0 and 1 are the same), kernel_variant (0 default = 3 in 3+1D: factored exponent on the 8 x 7
 * tile, cf_main_vah3, and the same kernel on 8 x 31 records with unit-strided lanes in 2+1D | 2: the round-1 kernel on the 6 x 7 / 8 x 61 tile,
 * kept for A/B in the developer build of the library -- the shipped one runs the default for it).  A cell whose E_a/Lambda could exceed 1e9 for the momentum grid returns IS3D_EDOMAIN (the reference's exp overflows there).
 * HOST pointers; dN_out as for is3d_smooth_spectra.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
    int64_t n_cells;
    const double *tau, *eta;            /* eta unused (may be NULL) when dimension == 2 */
    const double *ux, *uy, *un;
    const double *dat, *dax, *day, *dan;
    const double *T;                    /* unused (only FORCE_F0 reads it in the reference, :2295-2298); may be NULL */
    const double *pitt, *pitx, *pity, *pitn, *pixx, *pixy, *pixn, *piyy, *piyn, *pinn;   /* pi_perp^{mu nu} */
    const double *bulkPi;               /* residual bulk pressure */
    const double *Wx, *Wy;              /* W_perp^mu; W^tau, W^eta reconstructed (:2244-2245) */
    const double *Lambda, *aL;          /* anisotropic variables */
    const double *c0, *c1, *c2, *c3, *c4;
} is3d_vah_cells;

int is3d_smooth_spectra_vah(const is3d_vah_cells *cells, const is3d_species *species, const is3d_grid *grid,
                            const is3d_options *opts, double *dN_out, is3d_status *status);

/* The anisotropic-hydro 14-moment coefficient tables deltaf_coefficients/vah/c{0..4}_vah1.dat.  src/cpp never loads them; the
 * loader the reference has is the CUDA tree's load_df_coefficient_data, "df_mode == 4 // va hydro PL matching 14 moment"
 * (src/cuda/deltafReader.cu:60-82 file names, :104-112 "n_Lambda\nn_alphaL\n" + one label line, :196-213 rows
 * "Lambda [fm^-1]  alpha_L  value", alpha_L outer, Lambda inner).  Every table is [n_aL][n_L], Lambda fastest, file units. */
typedef struct {
    int32_t n_L, n_aL;
    const double *L;                    /* Lambda nodes, fm^-1, ascending */
    const double *aL;                   /* alpha_L nodes, ascending */
    const double *c0, *c1, *c2, *c3, *c4;
} is3d_vah_df_tables;
/* Reads <dir>/c0_vah1.dat ... c4_vah1.dat (dir = "deltaf_coefficients/vah" in a run directory).  Two-call pattern: L == NULL ->
 * only *n_L, *n_aL; otherwise L[n_L], aL[n_aL], c[5 * n_aL * n_L] (table k at c + k n_aL n_L), capacity in doubles of `c`.
 * The node arrays are what the reference's scan leaves in L_array / aL_array (each row overwrites its entries; the c4 file is
 * scanned last).  IS3D_EIO: a file is missing or short; IS3D_EINVAL: the five headers disagree or the nodes do not ascend. */
int is3d_vah_df_read(const char *dir, int32_t *n_L, int32_t *n_aL, double *L, double *aL, double *c, int64_t capacity);
/* Per-cell coefficients as src/cuda/deltafReader.cu:224-278 sets them, evaluated on the device (HOST pointers in and out; Lambda in
 * GeV as the surface reader stores it, :228): the first alpha_L node i2 >= 1 with aL < aL[i2] and the first Lambda node i1 >= 1 with
 * Lambda/hbarc < L[i1] select the cell of the grid; bilinear interpolation in (Lambda, alpha_L) -- which below the first node
 * extrapolates, as the reference does -- and every coefficient divided by hbarc^3 (:262-266).  A cell with Lambda/hbarc >= L[n_L - 1]
 * or aL >= aL[n_aL - 1] (or a NaN) finds no node: the reference leaves its c0..c4 unset there; this call returns IS3D_EDOMAIN with
 * *bad_cell (may be NULL) = the lowest such index, and stores zeros for it.  c0..c4: n doubles each. */
int is3d_vah_coefficients(const is3d_vah_df_tables *tab, int64_t n, const double *Lambda, const double *aL, double *c0, double *c1,
                          double *c2, double *c3, double *c4, int32_t device, int64_t *bad_cell);
/* is3d_smooth_spectra_vah with the coefficients taken from the tables: cells->c0..c4 are ignored (may be NULL), a device kernel
 * interpolates them from (Lambda, aL) into the arrays the prep kernel reads.  IS3D_EDOMAIN + status->bad_cell for a cell outside
 * the grid (see is3d_vah_coefficients).  tab == NULL: is3d_smooth_spectra_vah. */
int is3d_smooth_spectra_vah_df(const is3d_vah_cells *cells, const is3d_species *species, const is3d_grid *grid,
                               const is3d_vah_df_tables *tab, const is3d_options *opts, double *dN_out, is3d_status *status);

/* Device-resident form (bench.py --workload config5, hosts whose surface is already in HBM): the plan holds the lane tables, the
 * coefficient tables (tab may be NULL: cells->c0..c4 are then inputs) and the workspaces for up to max_cells cells per execute;
 * cells->* and dN_out are DEVICE pointers on the plan's device, hip_stream a hipStream_t.  Asynchronous except for the status
 * read-back when status != NULL.  is3d_vah_plan_timings: device time of the last execute's kernels (coefficients + prep in ms_prep,
 * cf_main_vah in ms_main, reduction + species scatter in ms_finalize) when timing is enabled. */
typedef struct is3d_vah_plan is3d_vah_plan;
int is3d_vah_plan_create(is3d_vah_plan **plan, const is3d_species *species, const is3d_grid *grid, const is3d_vah_df_tables *tab,
                         const is3d_options *opts, int64_t max_cells);
int64_t is3d_vah_plan_output_size(const is3d_vah_plan *plan);
int64_t is3d_vah_plan_workspace_bytes(const is3d_vah_plan *plan);
int is3d_vah_plan_execute(is3d_vah_plan *plan, const is3d_vah_cells *cells, double *dN_out, void *hip_stream, is3d_status *status);
int is3d_vah_plan_set_timing(is3d_vah_plan *plan, int32_t enable);
int is3d_vah_plan_timings(is3d_vah_plan *plan, is3d_status *status);
int is3d_vah_plan_tile_shape(const is3d_vah_plan *plan, int32_t *JT, int32_t *R);
/* "cf_main_vah3" (3+1D, opts.kernel_variant 0 | 3: factored exponent, 8 x 7 tile) or "cf_main_vah" (2+1D; 3+1D with kernel_variant 2: the
 * round-1 kernel on the 6 x 7 tile, kept for A/B) as it appears in rocprofv3 traces */
const char *is3d_vah_plan_main_kernel_name(const is3d_vah_plan *plan);
/* is3d_plan_observables for a device-resident spectrum of this plan's shape (dN/dy, dN/2 pi pT dpT dy, v_n; the same arguments, the same
 * kernels, this plan's species and grid): a VAH caller that wants a dN/dy does not take the spectrum to the host.  Asynchronous on hip_stream. */
int is3d_vah_plan_observables(is3d_vah_plan *plan, const double *dN_dev, const double *pT_w, const double *phi_w, double *dNdy,
                              double *dN2pipTdpTdy, double *vn, void *hip_stream);
void is3d_vah_plan_destroy(is3d_vah_plan *plan);

/* is3d_smooth_spectra_vah_df over several devices (tab == NULL: c0..c4 from the cells): the cells in n_devices contiguous shards
 * (is3d_shard_bounds), shard s on devices[s] with a host thread, a non-blocking stream and an is3d_vah_plan of its own; the device list,
 * reduce, status and shard_status as for is3d_smooth_spectra_multi (IS3D_REDUCE_ORDERED: the fixed binary tree, bitwise reproducible for a
 * given shard count, an ordinal may repeat; IS3D_REDUCE_RCCL: distinct devices).  A shard uploads only its own cells; with tab its
 * coefficients are interpolated on its own device.  One shard with IS3D_REDUCE_ORDERED is is3d_smooth_spectra_vah_df on devices[0].
 * opts->accumulate = 1 adds the combined result to dN_out on the host.  Shards without cells contribute zeros.  A failed shard does not stop
 * the others; the first failed shard's code comes back with "shard i (device d): ..." and, for IS3D_EDOMAIN, the cell's index in the whole
 * surface (also status->bad_cell; shard_status[i].bad_cell is shard-local).  NULL arguments, n_cells < 0, a NULL cell array that is read, a bad
 * reduce and what the list alone decides are IS3D_EINVAL before any device is used. */
int is3d_smooth_spectra_vah_multi(const is3d_vah_cells *cells, const is3d_species *species, const is3d_grid *grid,
                                  const is3d_vah_df_tables *tab, const is3d_options *opts, const int32_t *devices, int32_t n_devices,
                                  int32_t reduce, double *dN_out, is3d_status *status, is3d_status *shard_status);

/* FO_data_reader::read_surf_VAH_PLMatch (mode 2; src/cpp/readindata.cpp:813-928): 31 numbers per cell -- tau x y eta | dat dax day
 * dan | ut ux uy un | E T P PL | pitt pitx pity pitn pixx pixy pixn piyy piyn pinn | Wt Wx Wy Wn | bulkPi -- E, T, P, PL, pi, W and
 * bulkPi multiplied by hbar*c, and the anisotropic variables inferred per cell: aL = aL_fit(PL/P), Lambda = T / (aL R200(aL) / 2)^(1/4)
 * (src/cpp/arsenal.cpp:999-1065), Lambda stored in GeV.  PL/P >= 3 is fatal in the reference ("pl is too large", exit(-1)):
 * IS3D_EINVAL naming the cell.  Two-call pattern as is3d_surface_read_vh (arrays == NULL -> only *n_cells).  arrays32: caller-allocated,
 * in the order of is3d_vah_cells' first 25 members -- tau eta ux uy un dat dax day dan T pitt pitx pity pitn pixx pixy pixn piyy piyn
 * pinn bulkPi Wx Wy Lambda aL -- then E P PL Wt Wn x y; the last seven may be NULL. */
int is3d_surface_read_vah(const char *path, int32_t dimension, int64_t *n_cells, double *const *arrays32);

/* ---------------------------------------------------------------------------------------------
 * Particle sampler (operation = 2): replaces EmissionFunctionArray::sample_dN_pTdpTdphidy
 * (src/cpp/emissionfunction.h:208-210, emissionfunction_sampling_kernels.cpp:833-1225, call sites emissionfunction.cpp:1543,
 * :1606) for viscous hydro, df_mode 1-4, fast = 0 | 1; include_baryon = 1 with df_mode 1-3.  The reference's serial
 * std::default_random_engine streams are replaced by counter-based Philox4x32-10 streams keyed by (seed, stream, global cell
 * index, event) -- same five stream roles and the same distributions; particle lists agree with the reference statistically,
 * not draw by draw (the construction is written out in cf_sampler.hip and DESIGN.md section 3c).
 * --------------------------------------------------------------------------------------------- */
typedef struct {                        /* Sampled_Particle (src/cpp/particle.h), 96 bytes */
    int64_t cell;                       /* global cell index: first_cell + index in the call */
    int32_t event;
    int32_t species;                    /* index into the species list (mc_id, mass: caller's arrays) */
    double tau, x, y, eta, t, z;        /* t = tau cosh(eta), z = tau sinh(eta) */
    double E, px, py, pz;
} is3d_particle;

typedef struct {
    int32_t n_events;                   /* Nevents (emissionfunction.cpp:202, :1531) */
    int32_t n_gla;                      /* Gauss-Laguerre points */
    uint64_t seed;                      /* sampler_seed */
    double y_cut;                       /* 2+1D: hadrons get a uniform rapidity in +-y_cut (Y_CUT); 3+1D: unused (y_max = 0.5) */
    int64_t first_cell;                 /* global index of cells[0]: a shard of a surface samples what the whole surface would */
    const double *x, *y;                /* cell positions x_fo, y_fo copied into the particles; may be NULL */
    const double *root1, *weight1;      /* Gauss-Laguerre alpha = 1 (equilibrium densities, max_particle_number) */
    const is3d_feqmod_tables *feqmod;   /* df_mode 3, 4 (and fast = 1 with df_mode 2): alpha = 2 nodes, PDG list, T_avg of the
                                           Jonah tables, deta_min, mass_pion0; NULL otherwise */
    int32_t fast;                       /* FAST: species densities at the surface-average temperature (:1044-1056) */
    int32_t batch_events;               /* tuning: events per count/scan/fill batch; 0 = as many as fit 2^25 (event, cell) threads.
                                           The particle list does not depend on it. */
    double T_avg;                       /* fast: Plasma::temperature as read back from average_thermodynamic_quantities.dat */
    double T_avg_switch;                /* fast, df_mode 3: the same after `if (SET_T_SWITCH) temperature = T_SWITCH` (:856);
                                           0 = T_avg */
    double muB_avg;                     /* fast with include_baryon: Plasma::baryon_chemical_potential (deltafReader.cpp:545, :858) */
} is3d_sampler_inputs;

typedef struct {
    int64_t n_cells_skipped;            /* u.dsigma <= 0 (:899) */
    int64_t n_hadrons_drawn;            /* sum of the Poisson numbers (before the flux / viscous keep test) */
    int64_t n_momentum_samples, n_acceptances;   /* "Momentum sampling efficiency" (:1224) */
    int32_t n_classes, reserved;
    int64_t n_cells_breakdown;          /* df_mode 3: cells sampled with the linear delta-f instead (:1038) */
    double ms_h2d, ms_prep, ms_count, ms_fill;   /* device time: upload, densities + cell records, count pass + scan, fill pass */
    double ms_density;                  /* part of ms_prep: cf_sampler_density (the Gauss-Laguerre density integrals per (cell, class)) */
    double ms_poisson;                  /* part of ms_count: cf_sampler_poisson + the compaction of the emitting (event, cell) pairs */
    double ms_bin;                      /* is3d_sampler_plan_execute_binned: cf_sampler_bins over all batches (0 for the list entries);
                                           is3d_sample_binned_vah, is3d_sample_fused: the fused sample-and-bin passes (ms_count = ms_fill = 0
                                           there) */
    int64_t particle_workspace_bytes;   /* is3d_sampler_plan_execute_binned: the plan-owned particle workspace (one batch); 0 otherwise */
} is3d_sampler_stats;

/* All pointers HOST memory; opts: dimension, df_mode (1-4), include_bulk_deltaf, include_shear_deltaf, device.  Particles
 * come ordered by (event, cell, draw).  particles == NULL (or capacity 0): only *n_particles is computed.  If the buffer is
 * too small the first `capacity` particles are stored, *n_particles is the full count and IS3D_ENOMEM is returned. */
int is3d_sample_particles(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df,
                          const is3d_sampler_inputs *in, const is3d_options *opts, is3d_particle *particles,
                          int64_t capacity, int64_t *n_particles, is3d_sampler_stats *stats);
/* Device-resident, persistent form (what bench.py --workload config5-sampler times; is3d_sample_particles is create + upload + execute +
 * download + destroy, so the two give the same list bit for bit): the species classes, splines / bilinear grids, Jonah tables and fast-mode
 * densities are set up once from (species, df, in, opts) -- `in` as for is3d_sample_particles; its n_events, seed, first_cell, x, y and
 * batch_events are execute-time arguments here -- and the workspaces (8 B x classes + 360 B per cell, + 8 B x species per cell for the running sums of the
 * species weights unless df_mode = 3; 25 B per (event, cell) of a batch) are
 * allocated at the first execute of a shape and kept.  execute: cells->* and x, y are DEVICE arrays on the plan's device (x, y may be NULL),
 * particles a DEVICE buffer of `capacity` entries (NULL: count only); runs on the null stream and returns when the list is complete.
 * stats->ms_h2d is 0 (nothing is uploaded).  Return codes as is3d_sample_particles; cells->n_cells > max_cells: IS3D_EINVAL. */
typedef struct is3d_sampler_plan is3d_sampler_plan;
int is3d_sampler_plan_create(is3d_sampler_plan **plan, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                             const is3d_options *opts, int64_t max_cells);
int is3d_sampler_plan_execute(is3d_sampler_plan *plan, const is3d_cells *cells_dev, const double *x_dev, const double *y_dev, int32_t n_events,
                              uint64_t seed, int64_t first_cell, int32_t batch_events, is3d_particle *particles_dev, int64_t capacity,
                              int64_t *n_particles, is3d_sampler_stats *stats);
void is3d_sampler_plan_destroy(is3d_sampler_plan *plan);
/* is3d_sample_particles over several devices: the same contiguous cell shards, shard s on devices[s] with first_cell advanced to
 * the shard's first cell -- the counter-based streams are keyed by the GLOBAL cell index, so the hadrons are exactly those one device
 * samples; the shard lists are merged into the single-device order (event, cell, draw).  No collective at all.  Same calling
 * pattern and return codes as is3d_sample_particles; stats are summed (times: the slowest shard's).  opts->device is ignored. */
int is3d_sample_particles_multi(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df,
                                const is3d_sampler_inputs *in, const is3d_options *opts, const int32_t *devices, int32_t n_devices,
                                is3d_particle *particles, int64_t capacity, int64_t *n_particles, is3d_sampler_stats *stats);

/* Particle sampler for anisotropic hydro (mode 2, operation 2).  The reference's sample_dN_pTdpTdphidy_VAH_PL is an empty stub, so THIS is
 * the definition: the VAH analogue of sample_dN_pTdpTdphidy in regular mode (fast = 0).  The leading-order distribution f_a is an equilibrium
 * distribution at the stretched momentum p' = (p_x, p_y, p_z / alpha_L) of the local rest frame, so the sampler is the reference's df_mode-4
 * construction -- sample isotropically, map the momentum linearly -- with the residual delta-f of is3d_smooth_spectra_vah as a viscous weight.
 * Per cell, with the basis, the dsigma boost and ds_max = |dsigma_t| + |dsigma_space| (local rest frame) of is3d_sample_particles:
 *   - u.dsigma <= 0: skipped, counted in stats->n_cells_skipped.
 *   - Lambda or alpha_L not finite and > 0, or (with tab) a cell beyond the last node of the tables: a bad cell (so are a Lambda above 1e4
 *     times a boson's mass, where the momentum sampler's rejection bound ends, and a mean hadron number >= 2^31).  IS3D_EDOMAIN naming the
 *     lowest global index ("cell N: ..."); the other cells are sampled all the same and the list, *n_particles and stats are returned with
 *     the error.  No rejection loop is entered with such a scale.
 *   - bound density per species dn_s = 2 alpha_L g_s Lambda^3 / (2 pi^2 hbarc^3) GaussThermal(neq_int; m_s / Lambda, sign_s): the 14-moment
 *     bound 2 n_eq with T -> Lambda, alpha_L the Jacobian d^3p = alpha_L d^3p'; species added in list order;
 *     dn_tot = (sum_s dn_s) 2 y_max ds_max, y_max = y_cut (2+1D) | 0.5 (3+1D).
 *   - draws: the Poisson number, the species and the momentum from the counter-based streams of is3d_sample_particles (same key, same five
 *     roles); p' = sample_momentum(m, sign, T = Lambda, chem = 0); local-rest-frame momentum (p'_x, p'_y, alpha_L p'_z), E = sqrt(m^2 + p^2),
 *     boosted to the lab frame as there.
 *   - weights: w_flux = max(0, E dsigma_t - p.dsigma_space) / (E ds_max) with the stretched momentum; w_visc = (1 + clamp(fbar_a df, -1, 1)) / 2
 *     with df = c3 (p.z)(W.p) + c4 pi_perp^{mu nu} p_mu p_nu (include_shear_deltaf) + (c0 m^2 + c1 (p.z)^2 + c2 (p.u)^2) Pi
 *     (include_bulk_deltaf) at the hadron's momentum and fbar_a = 1 - sign f_a, E_a = E' (the energy of p'); kept when u_keep < w_flux w_visc.
 *   - the 2+1D rapidity draw, eta, t, z, x, y and the is3d_particle fields: as is3d_sample_particles.
 * The expected number of kept hadrons of species s is the integral of d^3p / E max(p.dsigma, 0) f_a (1 + clamp(fbar_a df)): the smooth VAH
 * spectrum with regulate_deltaf = 1 and an outflow cut, integrated over momentum.
 * HOST pointers.  tab == NULL: c0..c4 from the cells; else they are interpolated on the device (is3d_vah_coefficients) and cells->c0..c4 may be
 * NULL.  cells->T is not read; eta only in 3+1D; pi_perp, Wx, Wy only with include_shear_deltaf; bulkPi only with include_bulk_deltaf.
 * Calling pattern, ordering (event, cell, draw), IS3D_ENOMEM rule and stats: is3d_sample_particles.  in->fast != 0, a non-NULL in->feqmod,
 * a NULL cell array that would be read, n_events < 1 and n_gla outside 1..256 are IS3D_EINVAL before any device use; a good call without a
 * device is IS3D_ENODEVICE. */
int is3d_sample_particles_vah(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab,
                              const is3d_sampler_inputs *in, const is3d_options *opts, is3d_particle *particles, int64_t capacity,
                              int64_t *n_particles, is3d_sampler_stats *stats);
/* is3d_sample_particles_vah over several devices, as is3d_sample_particles_multi: contiguous cell shards, first_cell advanced per shard, the
 * lists merged into the single-device order; no collective.  The same refusals, before any device use; opts->device is ignored. */
int is3d_sample_particles_vah_multi(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab,
                                    const is3d_sampler_inputs *in, const is3d_options *opts, const int32_t *devices, int32_t n_devices,
                                    is3d_particle *particles, int64_t capacity, int64_t *n_particles, is3d_sampler_stats *stats);

/* EmissionFunctionArray::calculate_total_yield (src/cpp/emissionfunction_sampling_kernels.cpp:653-830; call sites
 * emissionfunction.cpp:1527, :1591): the mean particle yield of the surface, from which an oversampled run takes its number of
 * events, Nevents = min(ceil(min_num_hadrons / |yield|), max_num_samples) (emissionfunction.cpp:1524-1533).  Species densities
 * as Deltaf_Data::compute_particle_densities forms them at the surface averages (deltafReader.cpp:536-650), per-cell terms as
 * estimate_mean_particle_number (:200-236); 2+1D: times 2 y_cut (:822-826).  Deterministic (no random numbers).
 * in: n_gla, root1, weight1, y_cut and feqmod (the alpha = 2 nodes for every df_mode; df_mode 4 also the PDG list and T_avg of
 * the Jonah tables).  opts: dimension, df_mode, include_bulk_deltaf, include_baryon, include_baryondiff_deltaf, device.
 * densities (may be NULL): 3 * species->n doubles {Equilibrium_Density, Bulk_Density, Diffusion_Density} (emissionfunction.cpp:1289-1306). */
typedef struct {
    double T, E, P, muB, nB;            /* Plasma::load_thermodynamic_averages: the five lines of average_thermodynamic_quantities.dat */
    const double *root3, *weight3;      /* Gauss-Laguerre alpha = 3 (df_mode 1: J30, J31, deltafReader.cpp:596-600); NULL otherwise */
} is3d_yield_inputs;
int is3d_total_yield(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                     const is3d_yield_inputs *avg, const is3d_options *opts, double *mean_yield, double *densities);

/* The mean yield of an anisotropic-hydro surface: what sizes an oversampled run of is3d_sample_particles_vah.  The reference has nothing to
 * match (calculate_total_yield is viscous-hydro only and works at the surface-average temperature; there is no surface average of
 * (Lambda, alpha_L) and mode 2 writes no averages file), so THIS is the definition.
 * *mean_yield is the mean number of hadrons the surface emits: the momentum integral of the smooth VAH integrand (is3d_smooth_spectra_vah) with
 * the LINEAR residual delta-f (regulate_deltaf = 0) and no outflow cut, over the cells with u.dsigma > 0 -- the cells the sampler does not
 * skip -- in the convention of calculate_total_yield: backflow included; 3+1D: the whole rapidity range; 2+1D: times 2 y_cut.
 * f_a is an equilibrium distribution at the stretched momentum p' = (p_x, p_y, p_z / alpha_L), so in the local rest frame the integral reduces
 * to three radial ones.  For a cell with Lambda, alpha = alpha_L and a species (m, sign, g), mbar = m / Lambda, on the alpha = 1 Gauss-Laguerre
 * nodes (r_k, w_k) = (in->root1, in->weight1), E_k = sqrt(r_k^2 + mbar^2):
 *     N0 = sum_k w_k r_k   e^{r_k}       / (e^{E_k} + sign)
 *     A0 = sum_k w_k r_k   e^{r_k + E_k} / (e^{E_k} + sign)^2
 *     A2 = sum_k w_k r_k^3 e^{r_k + E_k} / (e^{E_k} + sign)^2
 *     K_m = [include_bulk_deltaf] Pi (c0 + c2)
 *     K_p = ([include_bulk_deltaf] Pi (c1 alpha^2 + c2 (2 + alpha^2)) + [include_shear_deltaf] c4 (pi_XX + pi_YY + alpha^2 pi_ZZ)) / 3
 *     N_{cell,s} = (u.dsigma) alpha g Lambda^3 / (2 pi^2 hbarc^3) (N0 + K_m m^2 A0 + K_p Lambda^2 A2)
 * with pi_AB = A_mu B_nu pi_perp^{mu nu} on the basis (X, Y, Z) of is3d_sample_particles_vah (covariant basis components, metric
 * (+, -, -, -tau^2)).  yield_by_species[s] = sum_cells N_{cell,s} (times 2 y_cut in 2+1D); *mean_yield = their sum in list order.
 * Where the terms come from: the angular averages <p_z^2> = alpha^2 p'^2 / 3, <p_x^2> = <p_y^2> = p'^2 / 3, <E^2> = m^2 + p'^2 (2 + alpha^2) / 3;
 * every term odd in a momentum component integrates to zero -- the c3 (p.z)(W.p) term (W.z = 0 by the way W^tau and W^eta are reconstructed)
 * and the spatial flux p^i dsigma_i.  The components of pi_perp along u are NOT read: they vanish on every surface whose pi_perp is orthogonal
 * to u (file surfaces, synthetic ones); on any other input tensor the yield differs from the smooth spectrum's integral by those terms.  For
 * alpha_L = 1 and a traceless pi_perp the shear term vanishes; for alpha_L != 1 it does not ((alpha^2 - 1) pi_ZZ).  With a large residual bulk
 * pressure the linear delta-f can drive a yield negative: the caller decides what that means (is3d_oversample_events takes the magnitude).
 * Bad cells: Lambda or alpha_L not finite and > 0, or (tab != NULL) a cell beyond the last node of the tables -- IS3D_EDOMAIN naming
 * in->first_cell + the lowest index ("cell N: ..."), the outputs holding the sum over the other cells.  u.dsigma <= 0: skipped, counted.
 * HOST pointers.  in: n_gla (1..256), root1, weight1, y_cut (2+1D: > 0), first_cell; fast must be 0 and feqmod NULL.  opts: dimension,
 * include_bulk_deltaf, include_shear_deltaf, device.  tab == NULL: the coefficients from the cells.  Arrays read: tau, u, dsigma, Lambda, aL;
 * pi_perp (and c4 without tab) only with include_shear_deltaf; bulkPi (and c0..c2 without tab) only with include_bulk_deltaf; never T, eta,
 * Wx, Wy, c3.  A NULL argument, a NULL array that would be read and the values above are IS3D_EINVAL before any device use; a good call
 * without a device is IS3D_ENODEVICE; n_cells = 0 gives 0.  Deterministic: per-(cell tile, class) partial sums added in a fixed order (no
 * floating-point atomics), the tiling a function of n_cells only -- the same bits from run to run and device to device.
 * stats: device time of the upload, of the per-cell kernel (with the coefficient interpolation) and of the per-(cell, class) integrals. */
typedef struct {
    int64_t n_cells_skipped;            /* u.dsigma <= 0 */
    int32_t n_classes, reserved;        /* species classes (mass, sign) the radial integrals were done for */
    double ms_h2d, ms_cells, ms_classes;
} is3d_yield_vah_stats;
int is3d_total_yield_vah(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab /* NULL: c0..c4 from the cells */,
                         const is3d_sampler_inputs *in /* n_gla, root1, weight1, y_cut, first_cell */, const is3d_options *opts,
                         double *mean_yield, double *yield_by_species /* may be NULL */, is3d_yield_vah_stats *stats /* may be NULL */);
/* The number of events of an oversampled run (emissionfunction.cpp:1524-1533, with at least one event):
 * max(1, min(ceil(min_num_hadrons / |(float) mean_yield|), max_num_samples)).  min_num_hadrons not > 0 or max_num_samples < 1: IS3D_EINVAL;
 * a yield that is 0 or not finite: IS3D_EDOMAIN. */
int is3d_oversample_events(double min_num_hadrons, double mean_yield, int32_t max_num_samples, int32_t *n_events);

/* write_particle_list_OSC (src/cpp/emissionfunction.cpp:863-901): results/particle_list_osc.dat, "# N" per non-empty event
 * then "mcid t x y z E px py pz" rows; particles ordered by event. */
int is3d_write_particle_list_osc(const char *path, int32_t n_events, int64_t n_particles, const is3d_particle *particles,
                                 const int64_t *mc_id);

/* test_sampler = 1: the binned self-consistency outputs (sample_dN_dy ... sample_dN_dX, sampling_kernels.cpp:31-152; writers
 * emissionfunction.cpp:903-1257) from a particle list: <dir>/dN_dy/, dN_deta/, momentum_distribution/, vn/,
 * spacetime_distribution/ (must exist), mean_yield.dat, yield_list.dat.  Bins = the parameters y_cut, y_bins, eta_cut, eta_bins,
 * pT_lower_cut, pT_upper_cut, pT_bins, tau_min, tau_max, tau_bins, r_min, r_max, r_bins (emissionfunction.cpp:205-222). */
typedef struct {
    double y_cut, eta_cut, pT_lower_cut, pT_upper_cut, tau_min, tau_max, r_min, r_max;
    int32_t y_bins, eta_bins, pT_bins, tau_bins, r_bins;
    int32_t kernel_form;                /* tuning, device binning only: 0 = the measured choice (workgroup-private histograms where they
                                           fit the LDS, global atomics otherwise), 1 = global atomics, 2 = workgroup-private (IS3D_EINVAL
                                           if they do not fit).  The histograms do not depend on it. */
} is3d_sampler_test_bins;
int is3d_write_sampler_tests(const char *results_dir, const is3d_sampler_test_bins *bins, int32_t n_events, int32_t n_species,
                             const int64_t *mc_id, int64_t n_particles, const is3d_particle *particles, double mean_yield);

/* The same distributions as raw integer histograms, so that the sampler can bin on the device and never hold the list (S = number of
 * species; every array caller-owned):
 *   dN_dy [S * y_bins], dN_deta [S * eta_bins], dN_pT [S * pT_bins], dN_tau [S * tau_bins], dN_r [S * r_bins]   counts, [species][bin]
 *   vn_re, vn_im [7 * S * pT_bins]     [k][species][bin]: the sums of cos((k+1) phi), sin((k+1) phi) over the hadrons of dN_pT's bin
 *   yield [n_events]                   hadrons per event
 * dN_pT is the one count that both sample_dN_2pipTdpTdy and sample_vn keep.  The harmonic sums are FIXED POINT: every term is added as
 * llrint(term * 2^32) (IS3D_SAMPLER_VN_SCALE), so that all sums are integer sums -- independent of the order of arrival, and with it of
 * launch geometry, event batching and cell sharding, bit for bit.  One term is off by at most 2^-33; a sum of N terms is below N 2^32 in
 * magnitude, so no bin overflows up to IS3D_SAMPLER_VN_MAX_COUNT = 2^31 - 1 entries: the device entries check dN_pT afterwards and
 * return IS3D_EDOMAIN beyond that.  The per-particle rule is csrc/cf_sampler_bins.h, shared by host and device. */
#define IS3D_SAMPLER_VN_HARMONICS 7
#define IS3D_SAMPLER_VN_SCALE 4294967296.0
#define IS3D_SAMPLER_VN_MAX_COUNT 2147483647LL
typedef struct {
    int64_t *dN_dy, *dN_deta, *dN_pT, *dN_tau, *dN_r, *vn_re, *vn_im, *yield;
} is3d_sampler_hist;
/* list -> histograms on the host (step 1 of is3d_write_sampler_tests; the CPU yardstick of the device kernel).  hist is overwritten. */
int is3d_sampler_bin_list(const is3d_sampler_test_bins *bins, int32_t n_events, int32_t n_species, int64_t n_particles,
                          const is3d_particle *particles, const is3d_sampler_hist *hist);
/* list -> histograms on the DEVICE: a caller's HOST list (any order, any length) is uploaded, binned by cf_sampler_bins in the form
 * bins->kernel_form, and the histograms copied to hist (HOST arrays, overwritten) as is3d_sampler_plan_execute_binned does.  A particle
 * whose species is outside [0, n_species) or whose event is outside [0, n_events) adds nothing (is3d_sampler_bin_list refuses such a
 * list): *n_skipped = n_particles - sum(yield) counts them.  Checked before any device use: the bins and kernel_form as for
 * is3d_sampler_plan_execute_binned (kernel_form = 2 on a block that does not fit the LDS included), n_events >= 1, n_species >= 1,
 * n_particles >= 0, particles non-null when n_particles > 0: IS3D_EINVAL.  n_particles = 0: zero histograms, no launch.  A dN_pT bin
 * above IS3D_SAMPLER_VN_MAX_COUNT: IS3D_EDOMAIN.  device < 0: the current device. */
int is3d_sampler_bin_list_device(const is3d_sampler_test_bins *bins, int32_t n_events, int32_t n_species, int64_t n_particles,
                                 const is3d_particle *particles, const is3d_sampler_hist *hist, int64_t *n_skipped, int32_t device);
/* histograms -> the files of is3d_write_sampler_tests (step 2); every file but vn/ is byte for byte the list writer's, vn/ agrees to
 * the fixed point (2^-32 absolute in v_n before the 7 printed digits). */
int is3d_write_sampler_tests_binned(const char *results_dir, const is3d_sampler_test_bins *bins, int32_t n_events, int32_t n_species,
                                    const int64_t *mc_id, const is3d_sampler_hist *hist, double mean_yield);
/* is3d_sampler_plan_execute with the list binned per event batch on the device and discarded: fill into a plan-owned particle workspace
 * (grown to the largest batch seen: stats->particle_workspace_bytes), cf_sampler_bins into device-resident histograms, and after the last
 * batch one copy to hist_host (HOST arrays, overwritten).  No buffer is sized by the total number of hadrons, and the sampler runs once.
 * The histograms are those of is3d_sampler_bin_list on the list of is3d_sampler_plan_execute: counts and yields exactly; vn_re, vn_im
 * within one unit per entry of the bin (device and host libm).  Bad bins (a count < 1, pT_upper_cut <= pT_lower_cut, an empty y, eta,
 * tau or r range): IS3D_EINVAL before any launch; a dN_pT bin above IS3D_SAMPLER_VN_MAX_COUNT: IS3D_EDOMAIN. */
int is3d_sampler_plan_execute_binned(is3d_sampler_plan *plan, const is3d_cells *cells_dev, const double *x_dev, const double *y_dev,
                                     int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events,
                                     const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist_host, int64_t *n_particles,
                                     is3d_sampler_stats *stats);
/* host-pointer one-shot (create + upload + execute_binned + destroy; in->first_cell is honoured), and the same over the cell shards of
 * is3d_sample_particles_multi, one per entry of devices, the integer histograms added on the host: equal to the single-device result
 * bit for bit. */
int is3d_sample_binned(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                       const is3d_options *opts, const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int64_t *n_particles,
                       is3d_sampler_stats *stats);
int is3d_sample_binned_multi(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                             const is3d_options *opts, const int32_t *devices, int32_t n_devices, const is3d_sampler_test_bins *bins,
                             const is3d_sampler_hist *hist, int64_t *n_particles, is3d_sampler_stats *stats);
/* The viscous sampler with its hadrons binned where they are sampled (cf_sampler_fused), in one pass and without a list: the arguments,
 * the persistent plan and the refusals of the binned entries above.  Definition:
 *   the histograms are those of is3d_sampler_bin_list on the list that is3d_sample_particles (is3d_sampler_plan_execute) returns for the
 *   same arguments -- counts and yields exactly; vn_re, vn_im within one unit per entry of the dN_pT bin (device and host libm).
 *   *n_particles = the sum of the yields = the length of that list.
 * How: per event batch the Poisson numbers and the compaction of the emitting (event, cell) pairs as in the list route, then ONE pass,
 * thread <-> pair, that replays the list route's streams and loop (df_mode 1-4, fast, include_baryon) and gives every kept hadron's
 * is3d_particle, built in registers, to the rule of csrc/cf_sampler_bins.h.  The adds are the 64-bit integer adds of cf_sampler_bins, so the
 * result depends neither on the order of arrival nor on bins->kernel_form (0 = workgroup-private histograms in LDS where they fit 64 KiB,
 * 1 = global atomics, 2 = private or IS3D_EINVAL), batch_events, first_cell sharding or the device count, bit for bit.
 * Device memory: the histograms (8 B per word of is3d_sampler_hist), the per-cell records and tables of the plan, and 9 B per (event, cell)
 * pair of ONE batch (Poisson number, emit flag, pair list; batches of <= 2^25 pairs, or batch_events events) with the compaction's temporary
 * storage.  Nothing is sized by the number of hadrons: no particle workspace, no counts, no offsets, no scan.
 * stats: ms_bin is the time of the fused passes; ms_count, ms_fill and particle_workspace_bytes are 0; the rest is the list route's.
 * A plan may serve is3d_sampler_plan_execute, _execute_binned and _execute_fused in any order.  Refused with IS3D_EINVAL before any device
 * use, in the order of the binned entries: a NULL, n_events < 1, bad bins, a NULL histogram array, kernel_form outside 0..2, kernel_form = 2
 * on a block that does not fit the LDS (beside the three words of the run-wide tallies).  IS3D_EDOMAIN: a cell outside the coefficient
 * table (named by its global index, as is3d_sample_binned does), a dN_pT bin above IS3D_SAMPLER_VN_MAX_COUNT. */
int is3d_sampler_plan_execute_fused(is3d_sampler_plan *plan, const is3d_cells *cells_dev, const double *x_dev, const double *y_dev,
                                    int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events,
                                    const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist_host, int64_t *n_particles,
                                    is3d_sampler_stats *stats);
/* host-pointer one-shot (create + upload + execute_fused + destroy), and the same over the cell shards of is3d_sample_binned_multi: the
 * integer histograms are added on the host, so the result equals the single-device one bit for bit. */
int is3d_sample_fused(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                      const is3d_options *opts, const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int64_t *n_particles,
                      is3d_sampler_stats *stats);
int is3d_sample_fused_multi(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                            const is3d_options *opts, const int32_t *devices, int32_t n_devices, const is3d_sampler_test_bins *bins,
                            const is3d_sampler_hist *hist, int64_t *n_particles, is3d_sampler_stats *stats);
/* The anisotropic-hydro sampler with its hadrons binned where they are sampled (cf_sampler_fused), in one pass and without a list.  As for
 * is3d_sample_particles_vah the reference has nothing to match, so THIS is the definition:
 *   the histograms are those of is3d_sampler_bin_list on the list that is3d_sample_particles_vah returns for the same arguments -- counts
 *   and yields exactly; vn_re, vn_im within one unit per entry of the dN_pT bin (device and host libm; against is3d_sampler_bin_list_device
 *   of that list, which runs the same device arithmetic, they are expected to be identical).  *n_particles = the sum of the yields = the
 *   length of that list.
 * How: per event batch the Poisson numbers and the compaction of the emitting (event, cell) pairs as in the list route, then ONE pass, thread
 * <-> pair, that replays the list route's streams and loop and gives every kept hadron's is3d_particle (built in registers) to the rule of
 * csrc/cf_sampler_bins.h; the adds are the 64-bit integer adds of cf_sampler_bins, so the result depends neither on the order of arrival
 * nor on bins->kernel_form (0 = workgroup-private histograms in LDS where they fit 64 KiB, 1 = global atomics, 2 = private or IS3D_EINVAL),
 * in->batch_events, in->first_cell sharding or the device count, bit for bit.  "Fit" is the rule of is3d_sample_fused: the kernel keeps the
 * three words of the run-wide tallies in LDS beside the block, so a private block has at most 8189 words; on a block of 8190-8192 words
 * kernel_form = 0 takes the global form and kernel_form = 2 is refused (the list kernel of is3d_sample_binned still holds 8192).
 * Device memory: the histograms (8 B per word of is3d_sampler_hist), the per-cell records of is3d_sample_particles_vah and 9 B per
 * (event, cell) pair of ONE batch (Poisson number, emit flag, pair list; batches of <= 2^25 pairs, or in->batch_events events) with the
 * compaction's temporary storage -- nothing is sized by the number of hadrons: no particle workspace, no counts, no offsets, no scan.
 * stats: ms_bin is the time of the fused sample-and-bin passes; ms_count, ms_fill and particle_workspace_bytes are 0; ms_h2d, ms_prep,
 * ms_density, ms_poisson, n_momentum_samples, n_acceptances, n_hadrons_drawn and n_cells_skipped are those of is3d_sample_particles_vah.
 * HOST pointers; hist is overwritten.  Refused with IS3D_EINVAL before any device use, in this order: everything is3d_sample_particles_vah
 * refuses, then what is3d_sample_fused refuses of bins and hist (a NULL, bad bins, kernel_form outside 0..2, kernel_form = 2 on a block
 * that does not fit the LDS beside the three tally words).  A good call without a device is IS3D_ENODEVICE, an empty surface included (the plan comes first, as for
 * is3d_sample_particles_vah); with a device n_cells = 0 gives zero histograms, *n_particles = 0 and IS3D_OK without a launch.
 * A bad cell (is3d_sample_particles_vah): IS3D_EDOMAIN naming the lowest global index, with the histograms of the other cells, *n_particles
 * and stats returned.  A dN_pT bin above IS3D_SAMPLER_VN_MAX_COUNT: IS3D_EDOMAIN. */
int is3d_sample_binned_vah(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab /* NULL: c0..c4 from the cells */,
                           const is3d_sampler_inputs *in, const is3d_options *opts, const is3d_sampler_test_bins *bins,
                           const is3d_sampler_hist *hist, int64_t *n_particles, is3d_sampler_stats *stats /* may be NULL */);
/* is3d_sample_binned_vah over contiguous cell shards, shard s on devices[s] with first_cell advanced to the shard's first cell (the
 * shards of is3d_sample_particles_vah_multi); the shards' integer histograms are added on the host, so the result equals the single-device
 * one bit for bit.  The same refusals, before any device use; opts->device is ignored; a bad cell is named by its index in the whole
 * surface (the lowest one), with the sum of all shards' histograms returned.  stats are summed (times: the slowest shard's). */
int is3d_sample_binned_vah_multi(const is3d_vah_cells *cells, const is3d_species *species, const is3d_vah_df_tables *tab,
                                 const is3d_sampler_inputs *in, const is3d_options *opts, const int32_t *devices, int32_t n_devices,
                                 const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist, int64_t *n_particles,
                                 is3d_sampler_stats *stats);

/* ---------------------------------------------------------------------------------------------
 * Operation 0: smooth Cooper-Frye spacetime distributions, df_mode 1 / 2 -- the drop-in for calculate_dN_dX
 * (emissionfunction_smooth_kernels.cpp:1000-1446, dispatched at emissionfunction.cpp:1510-1516).  Per cell
 *   dN_dy_cell = sum_pT sum_phi sum_(y | eta) w_pT w_phi prefactor g p.dsigma f        (:1370; the 3+1D y sum has NO weights)
 * with the spectra path's integrand, cell skipping and coefficients (the same cf_prep records); then per species
 *   dN_dy = the sum over all cells, dN_taudtaudy[itau], dN_twopirdrdy[ir], dN_twopitaurdtaudrdy[itau][ir] = the sums over the cells of a bin,
 *   itau = floor((tau - tau_min) / dtau), ir = floor((r - r_min) / dr), r = sqrt(x^2 + y^2), dtau = (tau_max - tau_min) / tau_bins (:1382-1398);
 *   a cell outside [0, bins) of one index counts toward dN_dy and the other histogram only.
 * Every sum is left to right over the cells in ascending index, each term pg_s * D_class(s)(cell) with pg_s = prefactor * g_s (one rounding
 * each): bitwise reproducible, and a bin equals the running sum of dN_dy_cell over its cells.  The values are RAW sums (not divided by bin
 * widths; is3d_write_spacetime normalises).  dN_dydeta: 2+1D, per eta node k of the eta table, sum w_pT w_phi prefactor g p.dsigma f / w_k (:1365);
 * 3+1D one point (n_eta_eff = 1): the species' total (the reference's etaValues[0] is eta_fo of the LAST cell, :1155).  pT_w, phi_w: the
 * weights of pT_tab, phi_tab (column 2), HOST memory.  df_mode 3 / 4 (calculate_dN_dX_feqmod) goes through the *_feqmod entries below;
 * the entries without feqmod tables refuse it with IS3D_EINVAL.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
    double tau_min, tau_max, r_min, r_max;  /* parameters tau_min ... r_bins (emissionfunction.cpp:216-222) */
    int32_t tau_bins, r_bins;
} is3d_spacetime_bins;

typedef struct {                        /* S = number of species; device pointers for the plan entry, host pointers for the one-shot */
    double *dN_dy;                      /* [S]                         */
    double *dN_taudtaudy;               /* [S][tau_bins]               */
    double *dN_twopirdrdy;              /* [S][r_bins]                 */
    double *dN_twopitaurdtaudrdy;       /* [S][tau_bins][r_bins]       */
    double *dN_dydeta;                  /* [S][n_eta_eff], n_eta_eff = n_eta (2+1D) | 1 (3+1D) */
    double *dN_dy_cell;                 /* [S][n_cells], may be NULL   */
} is3d_spacetime_out;

typedef struct {
    int32_t code;
    int32_t n_classes;
    int64_t n_cells_skipped;            /* u.dsigma <= 0 (:1170): contribute 0 */
    int64_t n_tau_outside, n_r_outside; /* non-skipped cells whose tau (r) bin index is outside [0, bins) */
    int64_t n_tau_negative, n_r_negative; /* ... of them below 0 (the reference prints an error line per such cell) */
    int64_t bad_cell;                   /* first cell with T outside the table, or -1 */
    int32_t n_passes, reserved;
    double ms_prep, ms_cells, ms_bins;  /* device time of the record writer, the per-cell kernel, the binning (keys, sort, sums) */
    double ms_h2d, ms_d2h;              /* one-shot entry only */
} is3d_spacetime_stats;

/* one-shot host entry; the argument checks (df_mode 3 / 4, NULL x or y, bins < 1, tau_max <= tau_min, r_max <= r_min) precede any device use */
int is3d_spacetime_distributions(const is3d_cells *cells, const double *x, const double *y, const is3d_species *species, const is3d_grid *grid,
                                 const double *pT_w, const double *phi_w, const is3d_df_tables *df, const is3d_options *opts,
                                 const is3d_spacetime_bins *bins, is3d_spacetime_out *out, is3d_spacetime_stats *stats);
/* the same on an existing plan (species classes, grids, splines shared with is3d_plan_execute): cells, x, y and out are DEVICE pointers;
 * the plan's workspace_bytes cap bounds the passes.  stats != NULL synchronises the stream and reports IS3D_EDOMAIN as is3d_plan_execute does */
int is3d_plan_execute_spacetime(is3d_plan *plan, const is3d_cells *cells, const double *x, const double *y, const double *pT_w,
                                const double *phi_w, const is3d_spacetime_bins *bins, const is3d_spacetime_out *out, void *hip_stream,
                                is3d_spacetime_stats *stats);
/* the four files per species under <results_dir> (emissionfunction_smooth_kernels.cpp:1100-1127, :1403-1434), "%.6e" as the reference's
 * setprecision(6) << scientific: dN_taudtaudy_<id>.dat (tau_mid, v / (tau_mid dtau)), dN_twopirdrdy_<id>.dat (r_mid, v / (2 pi r_mid dr)),
 * dN_twopitaurdtaudrdy_<id>.dat (tau_mid, r_mid, v / (2 pi tau_mid r_mid dtau dr), r outer, tau inner), dN_dydeta_<id>_<n_eta_eff>pt.dat
 * (eta_values[k], v).  IS3D_EIO if the directory is missing. */
int is3d_write_spacetime(const char *results_dir, const is3d_spacetime_bins *bins, int32_t n_species, const int64_t *mc_id, int32_t n_eta_eff,
                         const double *eta_values, const is3d_spacetime_out *out);

/* Operation 0 with the modified equilibrium, df_mode 3 / 4 -- the drop-in for calculate_dN_dX_feqmod (emissionfunction_smooth_kernels.cpp:1449-2135):
 * the same outputs, binning and order of additions as above; the per-cell integrand is that of is3d_smooth_spectra_feqmod (the linearised
 * delta-f where feqmod breaks down, df_mode 3) except in three places the routine differs from the spectra one:
 *   1. 3+1D: no switch to the linear delta-f for the rows |y - eta| < detA of cells with detA < 0.01 (:1926-1934 is commented out);
 *   2. 2+1D: the eta nodes are stretched by detA whenever detA > deta_min (:1847-1849; the spectra path also requires detA < 1); weights and
 *      the eta values written to the file are unchanged;
 *   3. the nan / inf test is on renorm / detA in both dimensions (:1881), before the breakdown branch: a (cell, species) that fails it adds 0,
 *      broken down or not.  p.dsigma keeps dsigma_eta inside the eta weight (:1943, :2010).
 * include_baryon = 1 with df_mode 3 only (df_mode 4 exits in the reference). */
typedef struct {
    int64_t n_cells_breakdown;          /* cells where feqmod breaks down (df_mode 3; the reference prints a running count over species x cells) */
    int64_t n_renorm_skipped;           /* (cell, species class) pairs that failed the test of point 3: they add 0 */
    int64_t first_cell_out_of_range;    /* first cell left out because E_mod / T_mod can exceed 1e9 (IS3D_EDOMAIN, as the spectra path), or -1 */
    double ms_renorm, ms_linear;        /* device time of the df_mode 3 renormalisation and of the linearised delta-f of the breakdown cells */
} is3d_spacetime_feqmod_stats;

/* one-shot host entry, the arguments of is3d_spacetime_distributions plus the feqmod tables; every argument check (NULL fq, df_mode 1 / 2,
 * df_mode 4 with include_baryon, the bins, NULL x or y) precedes any device use */
int is3d_spacetime_distributions_feqmod(const is3d_cells *cells, const double *x, const double *y, const is3d_species *species,
                                        const is3d_grid *grid, const double *pT_w, const double *phi_w, const is3d_df_tables *df,
                                        const is3d_feqmod_tables *fq, const is3d_options *opts, const is3d_spacetime_bins *bins,
                                        is3d_spacetime_out *out, is3d_spacetime_stats *stats, is3d_spacetime_feqmod_stats *fstats);
/* is3d_plan_execute_spacetime on a plan of is3d_plan_create_feqmod (which that entry also accepts), with the extra counters */
int is3d_plan_execute_spacetime_feqmod(is3d_plan *plan, const is3d_cells *cells, const double *x, const double *y, const double *pT_w,
                                       const double *phi_w, const is3d_spacetime_bins *bins, const is3d_spacetime_out *out, void *hip_stream,
                                       is3d_spacetime_stats *stats, is3d_spacetime_feqmod_stats *fstats);

/* Operation 0 for anisotropic hydro (mode 2, P_L matching).  The reference has no such routine -- calculate_dN_dX knows viscous hydro only --
 * so THIS is the definition: the VAH analogue of calculate_dN_dX, with the integrand, the options and the domain rule of
 * is3d_smooth_spectra_vah[_df] above: f_a (1 + fbar_a delta-f), include_bulk_deltaf, include_shear_deltaf, regulate_deltaf; NO outflow cut and
 * NO skipped cells (a cell with u.dsigma <= 0 contributes its negative value and is binned); IS3D_EDOMAIN + stats->bad_cell for a cell whose
 * E_a/Lambda can exceed 1e9 for the momentum grid or, with tables, whose (Lambda, alpha_L) lies beyond them.  Everything else is operation 0
 * as stated above for df_mode 1 / 2:
 *   dN_dy_cell[s][c] = pg_s D[class(s)][c],  D = sum_pT w_pT sum_phi w_phi sum_(y | eta) p.dsigma f;  the 3+1D y sum has no weights, the 2+1D eta
 *   sum carries the VAH kernel's own weights eta_w[k] (eta[1] - eta[0]) (smooth_kernels.cpp:2175-2185);
 *   dN_dy and the three histograms are the left-to-right sums of dN_dy_cell over the cells in ascending index (the same bin rule, RAW sums);
 *   dN_dydeta: 3+1D one point, the species' total; 2+1D per eta node k that node's term of the sum divided by eta_w[k] (eta[1] - eta[0]).
 * stats: n_cells_skipped is always 0; n_tau_outside, n_r_outside, n_tau_negative, n_r_negative count ALL cells outside a histogram (the
 * df_mode 1 - 4 entries count the u.dsigma > 0 ones); bad_cell as above.  opts: dimension, include_bulk_deltaf, include_shear_deltaf,
 * regulate_deltaf, device, workspace_bytes, collapse_species, zero_skip (exact zeros only: every value gives the same bits), kernel_variant 0 | 3
 * (the per-cell kernel reads the default variant's records).  Several devices are not offered for this entry.
 *
 * One-shot, HOST pointers.  tab == NULL: c0..c4 come from the cells; otherwise they are interpolated on the device and cells->c0..c4 are ignored.
 * Every argument check -- NULL x, y or weights, bins < 1, empty ranges, more than 64 pT values or an eta table beyond the per-cell kernel's LDS,
 * kernel_variant other than 0 / 3, a NULL cell array that is read -- precedes any device use or plan creation (is3d_resource_counters is unchanged
 * by a refusal); a good call without a device is IS3D_ENODEVICE. */
int is3d_spacetime_distributions_vah(const is3d_vah_cells *cells, const double *x, const double *y, const is3d_species *species,
                                     const is3d_grid *grid, const double *pT_w, const double *phi_w, const is3d_vah_df_tables *tab,
                                     const is3d_options *opts, const is3d_spacetime_bins *bins, is3d_spacetime_out *out,
                                     is3d_spacetime_stats *stats);
/* the same on an is3d_vah_plan (with or without its coefficient tables; species classes, grids and the record stream shared with
 * is3d_vah_plan_execute): cells, x, y and out are DEVICE pointers, pT_w and phi_w HOST memory; the plan's workspace_bytes cap bounds the passes
 * (stats->n_passes).  Asynchronous on hip_stream; stats != NULL synchronises it and reports IS3D_EDOMAIN with stats->bad_cell. */
int is3d_vah_plan_execute_spacetime(is3d_vah_plan *plan, const is3d_vah_cells *cells, const double *x, const double *y, const double *pT_w,
                                    const double *phi_w, const is3d_spacetime_bins *bins, const is3d_spacetime_out *out, void *hip_stream,
                                    is3d_spacetime_stats *stats);

/* Operation 0 over several devices (one process): the cells are cut into the contiguous blocks of is3d_shard_bounds, shard s runs on
 * devices[s], all shards concurrently with one host thread and one stream each.  A shard uploads its cells, writes its records and runs the
 * per-cell stage (df_mode 3 / 4: with the renormalisation and the linearised delta-f of its own breakdown cells) on a plan of its own; its
 * D slice lands in one [class][n_cells] array on devices[0] at the shard's cell offset (a copy on the device, hipMemcpyPeer from another
 * one).  devices[0] then runs the bin stage ONCE over the whole D and the whole surface's tau, x, y and skip flags -- keys, stable sort,
 * left-to-right segment sums, the dN_dy walk -- exactly as the single-device entries do.  All pointers are HOST pointers.
 *   fq:       NULL = df_mode 1 / 2 (is3d_spacetime_distributions), else df_mode 3 / 4 (is3d_spacetime_distributions_feqmod).
 *   devices:  as is3d_smooth_spectra_multi: NULL = the ordinals 0 .. n_devices - 1, n_devices <= 0 = every visible device, an ordinal may
 *             repeat; opts->device is ignored.  More shards than cells: the shards without cells contribute nothing (no error).
 * Contract:
 *   - one shard: the result is that of is3d_spacetime_distributions(_feqmod) on devices[0] bit for bit, dN_dydeta included;
 *   - any shard count, any device list: dN_dy, dN_taudtaudy, dN_twopirdrdy, dN_twopitaurdtaudrdy, dN_dy_cell (the assembled D expanded to
 *     species) and, in 3+1D, dN_dydeta are BITWISE the single-device result -- a cell's D depends on that cell alone, and every sum runs
 *     over the assembled D in global cell order.  The df_mode 1 / 2 records carry a power-of-two p.dsigma scale taken over the execute: the
 *     shards exchange their bounds before the records are written and all use the whole surface's, so the records themselves are the
 *     single-device ones;
 *   - 2+1D dN_dydeta: every shard reduces its per-chunk eta slabs in chunk order as a single device does, and a kernel on devices[0] adds the
 *     shards' rows in shard order 0, 1, 2, ... (no floating-point atomics): bitwise reproducible for a given shard count whatever the devices;
 *     it differs from the single-device value by the association of its additions only;
 *   - the workspace_bytes passes inside a shard change nothing of the above.
 * stats: the counters summed over the shards (n_tau_* / n_r_* come from the one bin stage), bad_cell the lowest GLOBAL cell index, ms_prep /
 * ms_cells the slowest shard's, ms_bins the one bin stage's, ms_h2d the slowest shard's upload plus the bin stage's, ms_d2h the D placement
 * (slowest shard) plus the read-back.  shard_stats: NULL or one entry per shard (n_devices of them; is3d_device_count() for n_devices <= 0),
 * bad_cell shard-local.
 * Errors: the argument checks of the two one-shot entries (NULL x or y, bins < 1, empty ranges, the grid bounds, an fq that contradicts
 * df_mode), n_devices beyond the visible count with devices == NULL and a negative ordinal are refused with IS3D_EINVAL BEFORE any device
 * is used or plan created (is3d_resource_counters is unchanged by them); a cell outside the coefficient table in any shard gives
 * IS3D_EDOMAIN for the whole call. */
int is3d_spacetime_distributions_multi(const is3d_cells *cells, const double *x, const double *y, const is3d_species *species,
                                       const is3d_grid *grid, const double *pT_w, const double *phi_w, const is3d_df_tables *df,
                                       const is3d_feqmod_tables *fq, const is3d_options *opts, const int32_t *devices, int32_t n_devices,
                                       const is3d_spacetime_bins *bins, is3d_spacetime_out *out, is3d_spacetime_stats *stats,
                                       is3d_spacetime_stats *shard_stats);

/* ---------------------------------------------------------------------------------------------
 * Spin polarization from thermal vorticity (mode 5) -- what EmissionFunctionArray::calculate_spin_polzn computes
 * (src/cpp/emissionfunction_polzn_kernels.cpp:27-265; writer write_polzn_vector_toFile, emissionfunction.cpp:775-821).  For every species s
 * and (pT, phi, y), summed over ALL cells (no u.dsigma test, no outflow cut, no degeneracy, no (2 pi hbar c)^-3):
 *   pt = mT cosh(y - eta), pn = mT / tau sinh(y - eta), px = pT cos(phi), py = pT sin(phi), ut = sqrt(|1 + ux^2 + uy^2 + tau^2 un^2|),
 *   f0 = 1 / (exp(p.u / T) + sign), pref = -(1 / (8 m)) (1 - sign f0),
 *   spin_t = 2 pref (wxy pn - wxn py + wyn px),   spin_x = 2 pref (wyn pt - wtn py + wty pn),
 *   spin_y = 2 pref (-wxn pt + wtn px - wtx pn),  spin_n = 2 pref (wtx py + wxy pt - wty px),
 *   S_mu += w p.dsigma f0 spin_mu,  Snorm += w p.dsigma f0.
 * T is ONE temperature for the whole surface (Plasma::temperature: the first line of average_thermodynamic_quantities.dat, or T_switch
 * when set_FO_temperature = 1; emissionfunction.cpp:1318-1321).  3+1D: the y grid, eta = the cell's eta, w = 1.  2+1D: y = 0, the sum over
 * the eta grid with w = eta_w[k] (eta[1] - eta[0]).  Outputs in the spectrum layout s + S (ipT + n_pT (iphi + n_phi iy)).
 * The vorticity is indexed by the GLOBAL cell index (the reference reads wtx_fo[icell] with the index inside its 10 000-cell chunk, so every
 * chunk after the first reuses the first chunk's vorticity).  Species of the same (mass, sign) share one evaluation;
 * degeneracy and baryon number do not enter.  Deterministic: per-chunk partial sums reduced in a fixed order, no floating-point atomics.
 * Options honoured: dimension, device, workspace_bytes (cap on the per-chunk partial sums; 0: 16 GiB).  The argument checks (a NULL
 * vorticity or cell array the dimension needs, T <= 0 or not finite, a mass <= 0, fewer than 2 eta nodes in 2+1D) precede any device use.
 * --------------------------------------------------------------------------------------------- */
typedef struct {                        /* thermal vorticity varpi_{mu nu} as read from a mode-5 surface (readindata.cpp:470-551), no unit conversion */
    const double *wtx, *wty, *wtn, *wxy, *wxn, *wyn;
} is3d_vorticity;

typedef struct {                        /* each [n_species][n_pT][n_phi][n_y_eff] in the spectrum layout; host (one-shot) or device (plan) */
    double *St, *Sx, *Sy, *Sn, *Snorm;
} is3d_polarization_out;

typedef struct {
    int32_t code;
    int32_t n_classes;                  /* distinct (mass, sign) classes evaluated */
    int32_t n_chunks;                   /* cell chunks of the partial sums (reduced in chunk order) */
    int32_t reserved;
    double ms_cells, ms_reduce;         /* device time of the per-chunk kernel and of the chunk reduction */
    double ms_h2d, ms_d2h;              /* one-shot entry only */
} is3d_polarization_stats;

/* one-shot host entry: cells (tau, eta in 3+1D, ux, uy, un, dat, dax, day, dan are read) and vorticity are HOST arrays of cells->n_cells */
int is3d_spin_polarization(const is3d_cells *cells, const is3d_vorticity *vorticity, const is3d_species *species, const is3d_grid *grid,
                           double T, const is3d_options *opts, is3d_polarization_out *out, is3d_polarization_stats *stats);
/* device-resident form: species classes, grids and lane tables on the device at create; execute takes DEVICE cell and vorticity arrays and
 * DEVICE outputs on hip_stream (a hipStream_t, NULL = default).  stats != NULL synchronises the stream and fills the times.  The one-shot is
 * create + upload + execute + download, so the two agree bit for bit. */
typedef struct is3d_polarization_plan is3d_polarization_plan;
int is3d_polarization_plan_create(is3d_polarization_plan **plan, const is3d_species *species, const is3d_grid *grid, const is3d_options *opts,
                                  int64_t max_cells);
int is3d_polarization_plan_execute(is3d_polarization_plan *plan, const is3d_cells *cells, const is3d_vorticity *vorticity, double T,
                                   const is3d_polarization_out *out, void *hip_stream, is3d_polarization_stats *stats);
void is3d_polarization_plan_destroy(is3d_polarization_plan *plan);
/* The spin polarization over several devices (one process): the cells are cut into the contiguous blocks of is3d_shard_bounds, shard s runs
 * on devices[s], all shards concurrently with one host thread, one is3d_polarization_plan and one stream each.  A shard uploads its own cell
 * slice and the same slice of the six vorticity arrays (the vorticity stays indexed by the GLOBAL cell index), runs the per-chunk kernel with
 * the chunk count of ITS cell count and adds its chunks in chunk order into one class-lane array V_s (not expanded to species, not scaled:
 * the v of the single-device reduction before its scale).  The V_s of the shards that have cells are placed next to each other on devices[0]
 * (a copy on the device, hipMemcpyPeer from another one) and one kernel there forms out = scale x ((V_0 + V_1) + V_2 ...) per (species, pT,
 * bin), in shard order.  No floating-point atomics, no collective.  All pointers are HOST pointers.
 *   devices:  as is3d_spacetime_distributions_multi: NULL = the ordinals 0 .. n_devices - 1, n_devices <= 0 = every visible device, an ordinal
 *             may repeat; opts->device is ignored.  More shards than cells: the shards without cells contribute nothing; no cells at all:
 *             the five outputs are zeros.
 * Contract:
 *   - one shard: the result is that of is3d_spin_polarization on devices[0] bit for bit;
 *   - N shards: the result is bitwise scale x ((V_0 + V_1) + V_2 ...), so bitwise reproducible for a given shard count whatever the device
 *     list; two calls give the same bits;
 *   - against the single device it differs by the association of the additions only.  The single-device chunk partition is a function of
 *     the whole surface's size, a shard's of the shard's size, so bitwise equality with the single device is NOT promised.
 * stats: n_classes; n_chunks summed over the shards; ms_cells the slowest shard's; ms_reduce the slowest shard's class sums plus the
 * combine on devices[0]; ms_h2d the slowest shard's upload; ms_d2h the placement of the class sums on devices[0] plus the read-back.
 * shard_stats: NULL or one entry per shard (n_devices of them; is3d_device_count() for n_devices <= 0); ms_reduce its class sums, ms_d2h the
 * placement of its class sums on devices[0].
 * Errors: every argument check of is3d_spin_polarization, a negative ordinal and n_devices beyond the visible count with devices == NULL are
 * refused with IS3D_EINVAL BEFORE any device is used or plan created (is3d_resource_counters is unchanged by them); with no device present
 * IS3D_ENODEVICE.  A shard's failure is returned, with its message, after all threads have joined; the lowest failing shard wins. */
int is3d_spin_polarization_multi(const is3d_cells *cells, const is3d_vorticity *vorticity, const is3d_species *species,
                                 const is3d_grid *grid, double T, const is3d_options *opts,
                                 const int32_t *devices, int32_t n_devices,
                                 is3d_polarization_out *out, is3d_polarization_stats *stats, is3d_polarization_stats *shard_stats);
/* write_polzn_vector_toFile (emissionfunction.cpp:775-821): APPENDS to <results_dir>/St.dat, Sx.dat, Sy.dat, Sn.dat one line per point,
 * "y\tphip\tpT\tS/Snorm" (scientific, setprecision(8), setw(5)), species outer, then y, phi, pT, a blank line after each phi block.  The
 * ratio is formed here, in C++, so 0/0 and +-inf print as the reference's would.  2+1D: y = 0 (y may be NULL).  IS3D_EIO if a file cannot
 * be opened. */
int is3d_write_polarization(const char *results_dir, int32_t dimension, int32_t n_species, int32_t n_pT, const double *pT, int32_t n_phi,
                            const double *phi, int32_t n_y, const double *y, const is3d_polarization_out *out);

/* ---------------------------------------------------------------------------------------------
 * Resonance decay feed-down -- what EmissionFunctionArray::do_resonance_decays (src/cpp/emissionfunction_resonance_decays.cpp:124-2158)
 * computes if its exit(-1) at entry (:128-129) is taken away.  Parents: the unstable chosen species, chosen-list order from the LAST to
 * index 1; each parent's log dN is taken from the spectrum as it stands at its turn (so it holds the feed-down of every parent before it).
 * Its 2-body (adjusted-mass loop :243-258) and 3-body (Q factor, 12-point s integral) channels, in file order, feed the daughters that are
 * in the chosen list (same-type daughters grouped, multiplicity as weight); 1- and 4-body channels add nothing.  The (v, zeta) integrands
 * use 12 x 12 Gauss-Legendre points and read the parent by bilinear interpolation of log dN in (Phi, M_T) (2+1D; 3+1D: also linear in Y)
 * up to the M_T switch, and the exponential M_T fit of each (y, phi) row above it.  Divergences from the reference:
 * the switch is the minimum over rows of M_T at the last pT index before the row's first non-positive value (the reference's MTmax, the
 * last node, for a positive spectrum); the 2-body recoil mass is the partner's (the reference takes particle_2's for every group) and the
 * channel's adjusted masses are used throughout; the acos argument is clamped to [-1, 1] (counted in n_clamps); what the reference exits
 * on is a return code.  The spectrum is [n_chosen][n_pT][n_phi][n_y_eff] in the library's layout, species fastest (n_y_eff = 1 in 2+1D).
 * Deterministic: each (daughter, bin) has one writer per parent that adds the parent's channels in channel order; no floating-point atomics.
 * --------------------------------------------------------------------------------------------- */
typedef struct {                        /* is3d_pdg_read_decays' output: entries in file order with the synthesised antibaryon entries */
    int32_t n;
    const int64_t *mc_id;
    const double *mass, *width;
    const int32_t *stable;              /* decays_Npart[0] == 1 (readindata.cpp:1487) */
    const int32_t *n_channels;          /* per entry; entry i's channels follow those of entries 0 .. i-1 */
    const int32_t *npart;               /* per channel, as in the file (|npart| products; negative values occur) */
    const double *branch_ratio;         /* per channel */
    const int64_t *daughters;           /* [channel][5], 0 = none */
} is3d_decay_table;

typedef struct {
    int32_t code;
    int32_t n_parents;                  /* unstable chosen parents visited */
    int32_t n_channels;                 /* 2- and 3-body channels with at least one chosen daughter (integrated) */
    int32_t n_adjusted;                 /* ... of which 2-body channels whose masses the adjustment loop changed */
    int64_t n_clamps;                   /* quadrature points whose cos(Phi~) was clamped to [-1, 1] */
    int64_t n_points;                   /* quadrature points per execute: bins x (144 | 1728) summed over every (parent, daughter, channel group) */
    double ms_tables, ms_feed;          /* device time of the per-parent table kernels (log, fit, switch) and of the feed-down kernels */
    double ms_h2d, ms_d2h;              /* one-shot entry only */
} is3d_decay_stats;

/* PDG_Data::read_resonances_conventional (readindata.cpp:1440-1568) in full, for hrg_eos = 1, 2.  Two-call pattern: mc_id == NULL returns
 * *n (the entries is3d_pdg_read counts) and *n_channels_total.  Antibaryon entries copy their baryon's channels with every daughter negated
 * unless it has baryon = charge = strangeness = 0 (:1510-1535).  More than 50 channels or 5 products, a truncated or non-numeric record, or a
 * daughter of an unstable antibaryon channel that cannot be found: IS3D_EIO. */
int is3d_pdg_read_decays(const char *path, int32_t *n, int32_t *n_channels_total, int64_t *mc_id, double *mass, double *width,
                         int32_t *stable, int32_t *n_channels, int32_t *npart, double *branch_ratio, int64_t *daughters, int32_t capacity,
                         int32_t channel_capacity);
/* calculate_Q_factor (:99-121): the 3-body phase-space normalisation, 24-point Gauss-Legendre.  Host only. */
double is3d_decay_q_factor(double mass_parent, double mass_1, double mass_2, double mass_3);
/* one-shot: dN_inout is a HOST spectrum, fed down in place.  chosen_mc_id: the chosen list in its order (each must be in the table).
 * EINVAL: fewer than 2 chosen species, a chosen or daughter id missing from the table, a 5-body channel, a daughter mass driven negative by
 * the adjustment.  EDOMAIN: a pT / phi (/ y) grid that does not ascend (or pT <= 0); a (y, phi) row of a parent with fewer than 2 points for
 * the M_T fit (the message names the parent's mc_id and the row).  On EDOMAIN from the fit the device spectrum of the plan entry holds the
 * feed-down of the parents before the failing one. */
int is3d_resonance_decays(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id, const is3d_grid *grid,
                          int32_t dimension, int32_t device, double *dN_inout, is3d_decay_stats *stats);
/* device-resident form: the schedule, groups, E*, p*, Q, s nodes and M_T nodes go to the device at create; execute feeds down the DEVICE
 * spectrum dN_inout on hip_stream (NULL = default) and synchronises it (a failed fit is reported by the return code).  stats != NULL times
 * every kernel.  The one-shot is create + upload + execute + download: the two agree bit for bit. */
typedef struct is3d_decay_plan is3d_decay_plan;
int is3d_decay_plan_create(is3d_decay_plan **plan, const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                           const is3d_grid *grid, int32_t dimension, int32_t device);
int64_t is3d_decay_plan_output_size(const is3d_decay_plan *plan);
int is3d_decay_plan_execute(is3d_decay_plan *plan, double *dN_inout, void *hip_stream, is3d_decay_stats *stats);
void is3d_decay_plan_destroy(is3d_decay_plan *plan);
/* write_dN_pTdpTdphidy_with_resonance_decays_toFile and write_dN_dpTdphidy_with_resonance_decays_toFile (emissionfunction.cpp:452-488,
 * :555-590): APPEND to <results_dir>/dN_pTdpTdphidy_resonance_decays.dat ("y\tphip\tpT\tdN", scientific, setprecision(8), species outer, then
 * y, phi, pT, a blank line after each phi block) and <results_dir>/dN_dpTdphidy_resonance_decays.dat (a header line, then the same with
 * dN x pT).  2+1D: y = 0 (y may be NULL).  IS3D_EIO if a file cannot be opened. */
int is3d_write_results_decays(const char *results_dir, int32_t dimension, int32_t n_species, int32_t n_pT, const double *pT, int32_t n_phi,
                              const double *phi, int32_t n_y, const double *y, const double *dN);

/* ---------------------------------------------------------------------------------------------
 * Monte Carlo decays of a sampled particle list to stable particles (the reference has none: this comment is the definition; DESIGN.md
 * section 3p).  Thread <-> primary; a primary's whole decay tree draws from ONE Philox stream, Rng(seed, 5, lo32(g), hi32(g)) with
 * g = first_particle + i (streams 0-4 are the samplers'), so a list decayed in pieces gives the bits of the whole.
 * Per particle of table entry e (lab momentum P, position (t, x, y, z), mass table->mass[e]), depth-first, first daughter next:
 *   - stable[e]: final.  A channel has n = |npart| products and is OPEN when the left-to-right sum of its daughters' table masses is < the
 *     parent's mass; no open channel: final as itself, counted in n_stuck.
 *   - channel: u_ch; the first open channel j with u_ch * c_last < c_j, c_j the running sum of the open channels' branch_ratio in file order
 *     (the last open channel otherwise): renormalised over the open channels.
 *   - lifetime != 0: u_tau is drawn at every decay; width > 0: the parent moves by (P / m) tau*, tau* = -(hbarc / width) log1p(-u_tau), and
 *     tau = sqrt(t^2 - z^2), eta = atanh(z / t) are recomputed; width <= 0: it decays where it is.
 *   - cluster masses, flat n-body phase space by mass generation with rejection: T = M - sum m_i; n - 2 uniforms sorted ascending to
 *     r_1 .. r_{n-2}; mu_k = sum_{i<=k} m_i + r_k T (r_0 = 0, r_{n-1} = 1); w = prod_{k=1}^{n-1} p*(mu_k; mu_{k-1}, m_k) with
 *     p*(a; b, c) = sqrt(max((a-b-c)(a+b+c)(a+b-c)(a-b+c), 0)) / (2a); n > 2: u_acc, accepted when u_acc w_max < w, w_max =
 *     prod_{k=1}^{n-1} p*(T + sum_{i<=k} m_i; sum_{i<k} m_i, m_k) (GENBOD's bound); after IS3D_DECAY_MC_MAX_TRIALS proposals the last one
 *     is taken and counted in n_exhausted.  n = 2: no rejection, no draw.
 *   - momenta, top-down from the cluster Pc = P: for k = n-1 .. 1, u_cos then u_phi (cos theta = 2 u_cos - 1, phi = 2 pi u_phi); in the
 *     cluster's rest frame particle k gets (sqrt(p^2 + m_k^2), p d) and the remainder (sqrt(p^2 + mu_{k-1}^2), -p d), p = p*(mu_k; mu_{k-1}, m_k);
 *     both go to the lab by one pure boost with beta = Pc_vec / Pc_0 (beta = 0: unchanged); the remainder becomes Pc, after k = 1 particle 0.
 * All pointers HOST memory.  particles[i].species indexes chosen_mc_id (as the samplers return it); out[k].species indexes the TABLE
 * (daughters need not be chosen species: table->mc_id is the mc_id argument of is3d_write_particle_list_osc); out[k].cell and .event are the
 * primary's, origin[k] (may be NULL) its index in particles.  Order: primaries in input order, within one the final particles in depth-first
 * pre-order over each channel's daughters in file order.  out == NULL counts only; with a list, capacity < *n_out returns IS3D_ENOMEM with
 * the full count in *n_out and nothing written.  IS3D_EINVAL before any device use: a NULL argument, n_particles < 0, a species outside
 * [0, n_chosen), a chosen or daughter id missing from the table, a channel of an unstable entry with more than IS3D_DECAY_MC_MAX_BODIES (or
 * fewer than 2) products, a decay graph with a cycle, a worst-case pending stack beyond IS3D_DECAY_MC_MAX_STACK (need(e) = 1 for a final
 * entry, else the maximum of need(d_i) + (n - 1 - i) over its channels' daughters d_i).  n_particles = 0: OK, *n_out = 0, no launch.  A good
 * call without a device is IS3D_ENODEVICE (no CPU path).  Two runs agree bit for bit.
 * --------------------------------------------------------------------------------------------- */
#define IS3D_DECAY_MC_MAX_BODIES 5
#define IS3D_DECAY_MC_MAX_STACK  16
#define IS3D_DECAY_MC_MAX_TRIALS 4096
typedef struct {
    uint64_t seed;
    int64_t  first_particle;  /* global index of particles[0]: a list decayed in pieces gives the bits of the whole */
    int32_t  lifetime;        /* 0: daughters are born where the parent was; 1: the parent first flies a proper time drawn from exp(-t Gamma / hbarc) */
    int32_t  device;          /* < 0: the current device */
} is3d_decay_mc_inputs;
typedef struct {
    int64_t n_primaries, n_decays, n_final, n_stuck, n_trials, n_exhausted;
    int32_t max_stack, max_depth;       /* static, from the table */
    int32_t n_closed_channels, reserved;
    double ms_h2d, ms_count, ms_fill, ms_d2h;
    double ms_bin;                      /* the binned entries below: the one decay-and-bin pass (ms_count = ms_fill = 0 there); 0 for the list entry */
} is3d_decay_mc_stats;
int is3d_decay_particles(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                         const is3d_decay_mc_inputs *in, int64_t n_particles, const is3d_particle *particles,
                         is3d_particle *out, int64_t *origin /* may be NULL */, int64_t capacity,
                         int64_t *n_out, is3d_decay_mc_stats *stats /* may be NULL */);

/* The table as the decay kernels read it, resident on one device (device < 0: the current one): the host analysis and the upload that
 * is3d_decay_particles performs on every call -- the open channels with their running sums, the chosen -> entry map, the cycle check,
 * max_stack and max_depth -- done once for a caller that keeps its primaries on the device.  Every refusal of the table that
 * is3d_decay_particles makes (IS3D_EINVAL, same messages) is made here before any device use; a good table without a device is
 * IS3D_ENODEVICE.  A table serves any number of calls and may outlive them; destroy(NULL) is allowed. */
typedef struct is3d_decay_mc_table is3d_decay_mc_table;
int is3d_decay_mc_table_create(is3d_decay_mc_table **table_dev, const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                               int32_t device);
void is3d_decay_mc_table_destroy(is3d_decay_mc_table *table_dev);

/* The test_sampler distributions of a list AFTER its Monte Carlo decays, without the decayed list.  Definition:
 *   the histograms are those of is3d_sampler_bin_list(bins, n_events, n_slots, ...) on the list that is3d_decay_particles returns for the
 *   same (table, chosen_mc_id, in, particles), with every particle's species (a TABLE entry e) replaced by slot[e] and the particles with
 *   slot[e] = -1 dropped -- counts and yields exactly; vn_re, vn_im within one unit per entry of the dN_pT bin (device and host libm).
 *   *n_final is the length of that list before the drop, *n_unbinned = *n_final - sum(yield) the number dropped.
 * How: ONE pass, thread <-> primary, over the same decay loop and stream (Rng(seed, 5, first_particle + i)): every final particle is built
 * in registers as the fill pass stores it and goes to the rule of csrc/cf_sampler_bins.h at once -- no counts, offsets, scan or output
 * list; device memory holds the primaries and the histograms.  The adds are the 64-bit integer adds of cf_sampler_bins, so the histograms
 * do not depend on bins->kernel_form (0 = workgroup-private histograms in LDS where the block and six tally words fit 64 KiB, 1 = global
 * atomics, 2 = private or IS3D_EINVAL), on the launch geometry, or on the pieces a list is decayed in (first_particle; integer histograms
 * added by the caller), bit for bit.  slot: int32[table->n].  All pointers HOST memory; hist is overwritten.
 * stats: the tallies and static fields of is3d_decay_particles; ms_count = ms_fill = 0, ms_bin is the pass.
 * IS3D_EINVAL before any device use: every refusal of is3d_decay_particles; n_slots < 1; the bins, NULL histogram arrays and kernel_form
 * as for is3d_sampler_bin_list_device; a NULL slot map or a slot outside [-1, n_slots); kernel_form = 2 on a block that does not fit; a
 * primary whose event is outside [0, n_events).  n_particles = 0: zero histograms, no launch.  A dN_pT bin above
 * IS3D_SAMPLER_VN_MAX_COUNT: IS3D_EDOMAIN.  A good call without a device: IS3D_ENODEVICE. */
int is3d_decay_particles_binned(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                                const is3d_decay_mc_inputs *in, int64_t n_particles, const is3d_particle *particles,
                                const int32_t *slot, int32_t n_slots, const is3d_sampler_test_bins *bins, int32_t n_events,
                                const is3d_sampler_hist *hist, int64_t *n_final, int64_t *n_unbinned,
                                is3d_decay_mc_stats *stats /* may be NULL */);
/* is3d_sampler_plan_execute_binned with every event batch decayed and binned a second time from the plan's particle workspace: after a
 * batch's fill, cf_sampler_bins bins the thermal hadrons into hist_host exactly as _execute_binned does (the same bits), then
 * cf_decay_mc_bins decays the batch with first_particle = the number of hadrons of the batches before it and bins the products into
 * hist_decayed (n_slots species).  hist_decayed is what is3d_decay_particles_binned gives for the whole list of is3d_sampler_plan_execute
 * with first_particle = 0, seed = decay_seed: independent of batch_events, kernel_form and launch geometry, bit for bit.  table_dev: on
 * the plan's device, created for the plan's species list as chosen list.  Device memory beyond _execute_binned's: the second histogram
 * block and the slot map, sized at first use and kept by the plan; nothing is sized by the number of final particles or of events' hadrons.
 * *n_particles: thermal hadrons; *n_final, *n_unbinned, decay_stats (may be NULL; n_primaries = *n_particles, ms_bin = the decay passes):
 * as above.  IS3D_EINVAL before any device use: the refusals of _execute_binned, n_slots < 1, a NULL array of hist_decayed, a bad slot map,
 * kernel_form = 2 on a decayed block that does not fit, a table of another chosen count or device. */
int is3d_sampler_plan_execute_decayed_binned(is3d_sampler_plan *plan, const is3d_cells *cells_dev, const double *x_dev, const double *y_dev,
                                             int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events,
                                             const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist_host,
                                             const is3d_decay_mc_table *table_dev, const int32_t *slot, int32_t n_slots, uint64_t decay_seed,
                                             int32_t lifetime, const is3d_sampler_hist *hist_decayed, int64_t *n_particles, int64_t *n_final,
                                             int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats);
/* host-pointer one-shot for the viscous sampler (df_mode 1-4, fast, include_baryon): plan and table create, upload, execute, destroy.
 * chosen_mc_id: the mc_id of species[0 .. n), which the table must hold.  The table's refusals come first, then is3d_sample_binned's. */
int is3d_sample_decayed_binned(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                               const is3d_options *opts, const is3d_sampler_test_bins *bins, const is3d_sampler_hist *hist,
                               const is3d_decay_table *table, const int64_t *chosen_mc_id, const int32_t *slot, int32_t n_slots,
                               uint64_t decay_seed, int32_t lifetime, const is3d_sampler_hist *hist_decayed, int64_t *n_particles,
                               int64_t *n_final, int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats);

/* Per-event flow vectors and cumulants of a particle list: what varies from event to event and what correlates the
 * particles of one event, which no event-averaged histogram above holds.  Per (event, slot) a record keeps the multiplicity M and the flow
 * vectors Q_n = sum e^{i n phi}, n = 1 .. IS3D_FLOW_HARMONICS, in three regions: 0 the full acceptance, 1 sub-event A, 2 sub-event B.
 * The rule for one particle (csrc/cf_sampler_flow.h, shared by host and device), with ratio = (E + pz) / (E - pz) = e^{2y}:
 *   accepted   E - pz > 0, exp(-2 y_cut) <= ratio <= exp(2 y_cut) and pT_min <= pT < pT_max, pT = sqrt(px^2 + py^2)
 *   A          accepted and ratio < exp(-y_gap)   (y < -y_gap / 2)
 *   B          accepted and ratio > exp(y_gap)    (y > +y_gap / 2): A and B are y_gap apart in rapidity
 * An accepted particle adds to region 0; one in A or B adds to that region as well.  What it adds: 1 to M, and llrint(cos(n phi) 2^32),
 * llrint(sin(n phi) 2^32) with phi = atan2(py, px) to Q_re, Q_im -- the fixed point of vn_re / vn_im (IS3D_SAMPLER_VN_SCALE), so every
 * word is an integer sum: independent of the order of arrival, the kernel form, the launch geometry and the pieces a list is processed in,
 * bit for bit (records of pieces add).  No region decision goes through log or atan2: host and device agree on M exactly; a Q word of the
 * device differs from the host's by at most M units (device and host libm).  Eight harmonics serve the two-particle cumulants for n <= 8
 * and the four-particle ones for n <= 4.  Cuts are valid when y_cut > 0, 0 <= y_gap < 2 y_cut and pT_max > pT_min >= 0.
 * Records (caller-owned): M [n_events][n_slots][3], Q_re and Q_im [n_events][n_slots][3][8].  M above IS3D_SAMPLER_VN_MAX_COUNT in any
 * record: IS3D_EDOMAIN from the device entry after the run. */
#define IS3D_FLOW_HARMONICS 8
typedef struct {
    double y_cut, y_gap, pT_min, pT_max;
    int32_t kernel_form;                /* tuning, device entries only: 0 = the measured choice, 1 = global atomics after a per-wave combine,
                                           2 = a workgroup-private window of events in LDS (IS3D_EINVAL when the records of one event,
                                           n_slots * 51 words, do not fit 64 KiB).  The records do not depend on it. */
} is3d_flow_cuts;
typedef struct {
    int64_t *M, *Q_re, *Q_im;
} is3d_flow_records;
/* list -> records on the host: THE definition, no device use.  slot: int32[n_species], species -> slot in [0, n_slots), or -1: dropped.
 * A particle whose species is outside [0, n_species) or whose event is outside [0, n_events) is refused (IS3D_EINVAL), as a NULL, n_events
 * or n_slots < 1, bad cuts, a slot outside [-1, n_slots) and kernel_form outside 0..2 are.  records is overwritten. */
int is3d_flow_list(const is3d_flow_cuts *cuts, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                   int64_t n_particles, const is3d_particle *particles, const is3d_flow_records *records);
/* list -> records on the DEVICE: a caller's HOST list (any order, any length) is uploaded and passed through cf_sampler_flow in the form
 * cuts->kernel_form.  A particle whose species or event is out of range adds nothing and is counted in *n_skipped.  The refusals above
 * and kernel_form = 2 on records that do not fit come before any device use; a good call without a device is IS3D_ENODEVICE.
 * n_particles = 0: zero records, no launch.  device < 0: the current device. */
int is3d_flow_list_device(const is3d_flow_cuts *cuts, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                          int64_t n_particles, const is3d_particle *particles, const is3d_flow_records *records, int64_t *n_skipped,
                          int32_t device);
/* Integer sums of slots: out (n_groups slots) receives, per event and region, the sums of the records whose slot s has group[s] = g
 * (group: int32[n_slots], -1: left out).  M and Q are additive, so "all hadrons" is the merge of the identified slots. */
int is3d_flow_merge(const is3d_flow_records *records, int32_t n_events, int32_t n_slots, const int32_t *group, int32_t n_groups,
                    const is3d_flow_records *out);
/* Q-cumulants (Bilandzic, Snellings, Voloshin, Phys. Rev. C 83, 044913) per slot from region 0 and the sub-events, n = 1..8 (index n - 1),
 * with Q = Q_n / 2^32, all in double from the exact integers, events in order -- deterministic on the host:
 *   <2>     = (|Q_n|^2 - M) / (M (M - 1)),                                                            event weight M (M - 1)
 *   <4>     = [|Q_n|^4 + |Q_2n|^2 - 2 Re(Q_2n Q_n*^2) - 4 (M - 2) |Q_n|^2 + 2 M (M - 3)] / W4,  n <= 4,   W4 = M (M - 1)(M - 2)(M - 3)
 *   <2>_gap = Re(Q_n^A Q_n^B*) / (M_A M_B),                                                           event weight M_A M_B
 * An event whose weight for a quantity is zero is left out of it; n_used_* count the events that were not.  <<.>> is the weighted event
 * average (0 when no event was used).
 *   c2 = <<2>>, avg4 = <<4>>, c4 = <<4>> - 2 <<2>>^2, c2_gap = <<2>_gap>
 *   v2 = sgn(c2) |c2|^(1/2), v4 = sgn(-c4) |c4|^(1/4), v2_gap = sgn(c2_gap) |c2_gap|^(1/2)
 *   v_rp = sum Re Q_n / sum M: the flow about the fixed reaction plane (0 when sum M = 0)
 *   mean_M, var_M: mean and population variance of M over all n_events events */
typedef struct {
    double c2[IS3D_FLOW_HARMONICS], c2_gap[IS3D_FLOW_HARMONICS], v2[IS3D_FLOW_HARMONICS], v2_gap[IS3D_FLOW_HARMONICS], v_rp[IS3D_FLOW_HARMONICS];
    double avg4[4], c4[4], v4[4];
    double mean_M, var_M;
    int64_t n_used_2, n_used_4, n_used_gap, n_events;
} is3d_flow_result;
int is3d_flow_cumulants(const is3d_flow_records *records, int32_t n_events, int32_t n_slots, is3d_flow_result *out /* [n_slots] */);
/* Writes, per slot s, <results_dir>/flow/cumulants_<labels[s]>.dat (two comment lines, then a row per n = 1..8: n, c_n{2}, c_n{4}, c_n{2,gap},
 * v_n{2}, v_n{4}, v_n{2,gap}, reaction-plane v_n, tab separated; the four-particle columns are 0 for n > 4) and
 * <results_dir>/flow/multiplicity_<labels[s]>.dat (two comment lines, the first with the mean and the variance of M, then a row per event: event, M, M_A, M_B).  Doubles are printed by
 * std::to_chars(scientific, 8) as the other writers' values.  The flow/ directory must exist (IS3D_EIO otherwise); a NULL, an empty label or
 * one with a '/', n_events < 1 and n_slots < 1 are IS3D_EINVAL. */
int is3d_write_flow(const char *results_dir, const is3d_flow_records *records, int32_t n_events, int32_t n_slots, const char *const *labels);
/* The flow records of a list AFTER its Monte Carlo decays, without the decayed list: the one-pass analogue of is3d_decay_particles_binned.
 * Definition: the records are those of is3d_flow_list(cuts, n_events, n_slots, slot, table->n, ...) on the list that is3d_decay_particles
 * returns for the same (table, chosen_mc_id, in, particles), whose species are TABLE entries -- M exactly, every Q word within M units
 * (device and host libm).  *n_final is the length of that list, *n_unbinned = *n_final - sum of M over region 0: the final particles that
 * added to no record (slot -1, or outside the cuts).  How: cf_decay_mc_flow, thread <-> primary over the decay loop and stream of
 * is3d_decay_particles (Rng(seed, 5, first_particle + i)); every final particle's momentum is built in registers and goes to the rule of
 * csrc/cf_sampler_flow.h at once.  A primary's products share its event, so the workgroup-private form keeps a window of events in LDS
 * along the primaries' order (kernel_form as for is3d_flow_list_device, the window beside six tally words).  The records do not depend on
 * kernel_form, on the launch geometry or on the pieces a list is decayed in (first_particle; records added by the caller), bit for bit.
 * slot: int32[table->n].  All pointers HOST memory; records is overwritten.  stats as for is3d_decay_particles_binned (ms_bin: the pass).
 * IS3D_EINVAL before any device use: every refusal of is3d_decay_particles; the refusals of is3d_flow_list_device with the table's entries as
 * species; a primary whose event is outside [0, n_events).  n_particles = 0: zero records, no launch.  M above IS3D_SAMPLER_VN_MAX_COUNT:
 * IS3D_EDOMAIN.  A good call without a device: IS3D_ENODEVICE. */
int is3d_decay_particles_flow(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                              const is3d_decay_mc_inputs *in, int64_t n_particles, const is3d_particle *particles,
                              const int32_t *slot, int32_t n_slots, const is3d_flow_cuts *cuts, int32_t n_events,
                              const is3d_flow_records *records, int64_t *n_final, int64_t *n_unbinned,
                              is3d_decay_mc_stats *stats /* may be NULL */);

/* is3d_sampler_plan_execute with the list of each event batch turned into flow records on the device and discarded: fill into the plan's
 * particle workspace, cf_sampler_flow into device-resident records (slot: int32 per species of the plan) and, with table_dev != NULL,
 * cf_decay_mc_flow of the same batch with first_particle = the number of hadrons of the batches before it (slot_decayed: int32 per table
 * entry), exactly as is3d_sampler_plan_execute_decayed_binned does; one copy of each block to the caller's HOST arrays after the last batch.
 *   records          = is3d_flow_list of the list is3d_sampler_plan_execute returns for the same arguments
 *   records_decayed  = is3d_decay_particles_flow of that list with first_particle = 0, seed = decay_seed
 * (M exactly, Q within M units), independent of batch_events, kernel_form and launch geometry, bit for bit.  The plan keeps the record
 * blocks and slot maps (sized at first use) and serves its other entries in any order, as before.  table_dev == NULL: slot_decayed,
 * records_decayed, n_final, n_unbinned and decay_stats are not used.  *n_particles: thermal hadrons; *n_final, *n_unbinned, decay_stats as
 * for is3d_decay_particles_flow.  IS3D_EINVAL before any device use: the refusals of is3d_flow_list_device for either set of records, a
 * table of another chosen count or device.  Not offered: the fused sample-and-bin pass, the anisotropic-hydro sampler, several devices
 * (thermal records of cell shards may be added by the caller; decayed ones may not, since first_particle depends on the shards before). */
int is3d_sampler_plan_execute_flow(is3d_sampler_plan *plan, const is3d_cells *cells_dev, const double *x_dev, const double *y_dev,
                                   int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events, const is3d_flow_cuts *cuts,
                                   const int32_t *slot, int32_t n_slots, const is3d_flow_records *records_host,
                                   const is3d_decay_mc_table *table_dev /* may be NULL */, const int32_t *slot_decayed, int32_t n_slots_decayed,
                                   uint64_t decay_seed, int32_t lifetime, const is3d_flow_records *records_decayed, int64_t *n_particles,
                                   int64_t *n_final, int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats);
/* host-pointer one-shot for the viscous sampler: plan and table create, upload, execute, destroy.  table may be NULL; otherwise chosen_mc_id
 * holds the mc_id of species[0 .. n), which the table must hold.  The cuts' and the table's refusals come first, then the plan's. */
int is3d_sample_flow(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                     const is3d_options *opts, const is3d_flow_cuts *cuts, const int32_t *slot, int32_t n_slots,
                     const is3d_flow_records *records, const is3d_decay_table *table /* may be NULL */, const int64_t *chosen_mc_id,
                     const int32_t *slot_decayed, int32_t n_slots_decayed, uint64_t decay_seed, int32_t lifetime,
                     const is3d_flow_records *records_decayed, int64_t *n_particles, int64_t *n_final, int64_t *n_unbinned,
                     is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats);

/* Differential flow: the flow records above with a second key, the pT bin, and from them v_n{2}(pT), v_n{4}(pT) and
 * v_n{2,gap}(pT) against a reference made of the same records.  The pT bins are a caller's edge table pT_edges[n_pT + 1]: HOST doubles,
 * finite, strictly ascending, pT_edges[0] >= 0, 1 <= n_pT <= IS3D_FLOW_DIFF_MAX_BINS, handed to the kernels as bits.  The table IS the
 * acceptance in pT: cuts->pT_min and cuts->pT_max must equal pT_edges[0] and pT_edges[n_pT] bit for bit (IS3D_EINVAL otherwise), so the
 * rule of is3d_flow_list decides acceptance and region unchanged.  An accepted particle's bin is the b with pT_edges[b] <= pT <
 * pT_edges[b + 1], pT = sqrt(px^2 + py^2) as in that rule, found by bisection with comparisons only (csrc/cf_sampler_flow_diff.h, shared by
 * host and device: no division by a width, no libm in any decision).  It adds what it adds to a flow record, to region 0 and its
 * sub-event of (event, slot, bin): m (the count) and p_re, p_im (the fixed-point terms).  So the records summed over the bins ARE the
 * is3d_flow_list records of the same cuts, word for word, and everything said there about order, pieces, kernel form and the device's
 * agreement with the host (m exactly, a p word within m units) holds here.
 * Records (caller-owned): m [n_events][n_slots][n_pT][3], p_re and p_im [n_events][n_slots][n_pT][3][8].  kernel_form = 2 is IS3D_EINVAL
 * when the records of one event, n_slots * n_pT * 51 words, do not fit 64 KiB beside the IS3D_FLOW_DIFF_MAX_BINS + 2 words kept for the staged
 * edges (and the six tally words of the decay pass).  m above IS3D_SAMPLER_VN_MAX_COUNT: IS3D_EDOMAIN from a device entry after the run.
 * Not offered: the fused sample-and-bin pass, the anisotropic-hydro sampler, several devices. */
#define IS3D_FLOW_DIFF_MAX_BINS 64
typedef struct {
    int64_t *m, *p_re, *p_im;
} is3d_flow_diff_records;
/* list -> records on the host: THE definition, no device use.  Refusals: those of is3d_flow_list, and the edge-table checks above. */
int is3d_flow_diff_list(const is3d_flow_cuts *cuts, int32_t n_pT, const double *pT_edges, int32_t n_events, int32_t n_slots, const int32_t *slot,
                        int32_t n_species, int64_t n_particles, const is3d_particle *particles, const is3d_flow_diff_records *records);
/* list -> records on the DEVICE through cf_sampler_flow_diff, as is3d_flow_list_device (n_skipped, n_particles = 0, device < 0). */
int is3d_flow_diff_list_device(const is3d_flow_cuts *cuts, int32_t n_pT, const double *pT_edges, int32_t n_events, int32_t n_slots,
                               const int32_t *slot, int32_t n_species, int64_t n_particles, const is3d_particle *particles,
                               const is3d_flow_diff_records *records, int64_t *n_skipped, int32_t device);
/* The reference flow vectors: out (flow records of ONE slot, n_events events) receives, per event and region, the integer sums of the
 * differential records over the slots s with ref_slot[s] != 0 (int32[n_slots], 0 or 1) and the bins in [ref_bin_lo, ref_bin_hi).
 * IS3D_EINVAL: a NULL, sizes < 1, n_pT outside 1..64, ref_slot outside {0, 1}, not 0 <= ref_bin_lo < ref_bin_hi <= n_pT. */
int is3d_flow_diff_reference(const is3d_flow_diff_records *records, int32_t n_events, int32_t n_slots, int32_t n_pT, const int32_t *ref_slot,
                             int32_t ref_bin_lo, int32_t ref_bin_hi, const is3d_flow_records *out);
/* Differential Q-cumulants (Bilandzic, Snellings, Voloshin, Phys. Rev. C 83, 044913, section IV) per (slot, bin), in double from the exact
 * integers, events in order.  Q, M: the reference of region 0 (is3d_flow_diff_reference); p, m_p: the record of (slot, bin) in region 0;
 * q, m_q: that record again if the slot and the bin belong to the reference, 0 otherwise; all vectors / 2^32:
 *   <2'>     = (Re(p_n Q_n*) - m_q) / (m_p M - m_q),                                   event weight the denominator, n = 1..8
 *   <4'>     = Re[p_n Q_n Q_n* Q_n* - q_2n Q_n* Q_n* - p_n Q_n Q_2n* - 2 M p_n Q_n* - 2 m_q |Q_n|^2 + 7 q_n Q_n* - Q_n q_n* + q_2n Q_2n*
 *                 + 2 p_n Q_n* + 2 m_q M - 6 m_q] / [(m_p M - 3 m_q)(M - 1)(M - 2)],  event weight the denominator, n = 1..4
 *   <2'>_gap = [Re(p_n^A Q_n^B*) + Re(p_n^B Q_n^A*)] / (m_p^A M^B + m_p^B M^A),        event weight the denominator
 * An event whose weight for a quantity is zero is left out of it, and an event with M < 4 out of the four-particle one; n_used_* count
 * the events that were not.  <<.>> is the weighted event average (0 when no event was used).  With c2 = <<2>>, c4 and c2_gap those of
 * is3d_flow_cumulants on the reference records:
 *   d2 = <<2'>>, avg4 = <<4'>>, d4 = <<4'>> - 2 <<2'>> <<2>>, d2_gap = <<2'>_gap>
 *   v2 = d2 / sqrt(c2) (0 unless c2 > 0), v4 = -d4 / (-c4)^(3/4) (0 unless c4 < 0), v2_gap = d2_gap / sqrt(c2_gap) (0 unless c2_gap > 0)
 *   v_rp = sum Re p_n / sum m_p (0 when sum m_p = 0); sum_m = sum m_p over the events, mean_m = sum_m / n_events
 * out: [n_slots][n_pT].  Refusals as for is3d_flow_diff_reference. */
typedef struct {
    double d2[IS3D_FLOW_HARMONICS], d2_gap[IS3D_FLOW_HARMONICS], v2[IS3D_FLOW_HARMONICS], v2_gap[IS3D_FLOW_HARMONICS], v_rp[IS3D_FLOW_HARMONICS];
    double avg4[4], d4[4], v4[4];
    double mean_m, sum_m;
    int64_t n_used_2, n_used_4, n_used_gap, n_events;
} is3d_flow_diff_result;
int is3d_flow_diff_cumulants(const is3d_flow_diff_records *records, int32_t n_events, int32_t n_slots, int32_t n_pT, const int32_t *ref_slot,
                             int32_t ref_bin_lo, int32_t ref_bin_hi, is3d_flow_diff_result *out /* [n_slots][n_pT] */);
/* Writes, per slot s, <results_dir>/flow/differential_<labels[s]>.dat: two comment lines, then a row per (bin, n), n = 1..8: bin, edge_lo,
 * edge_hi, n, d_n{2}, d_n{4}, d_n{2,gap}, v_n{2}, v_n{4}, v_n{2,gap}, reaction-plane v_n, sum m_p, tab separated (the four-particle
 * columns are 0 for n > 4); doubles by std::to_chars(scientific, 8), integers in full.  The flow/ directory must exist (IS3D_EIO otherwise);
 * the refusals of is3d_flow_diff_cumulants and of the edge table, a NULL, an empty label or one with a '/' are IS3D_EINVAL. */
int is3d_write_flow_diff(const char *results_dir, const is3d_flow_diff_records *records, int32_t n_events, int32_t n_slots, int32_t n_pT,
                         const double *pT_edges, const int32_t *ref_slot, int32_t ref_bin_lo, int32_t ref_bin_hi, const char *const *labels);
/* is3d_decay_particles_flow with the pT bin as a second key: the records are those of is3d_flow_diff_list on the list is3d_decay_particles
 * returns (m exactly, every p word within m units), in one pass of cf_decay_mc_flow on the differential sink; n_final, n_unbinned, stats,
 * pieces (first_particle) and refusals as there, with the edge-table checks. */
int is3d_decay_particles_flow_diff(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                                   const is3d_decay_mc_inputs *in, int64_t n_particles, const is3d_particle *particles,
                                   const int32_t *slot, int32_t n_slots, const is3d_flow_cuts *cuts, int32_t n_pT, const double *pT_edges,
                                   int32_t n_events, const is3d_flow_diff_records *records, int64_t *n_final, int64_t *n_unbinned,
                                   is3d_decay_mc_stats *stats /* may be NULL */);
/* is3d_sampler_plan_execute_flow with differential records (both sets on the same edge table): thermal records = is3d_flow_diff_list of
 * the list is3d_sampler_plan_execute returns, decayed ones = is3d_decay_particles_flow_diff of that list; independent of batch_events,
 * kernel_form and launch geometry, bit for bit.  The plan serves its other entries afterwards as before. */
int is3d_sampler_plan_execute_flow_diff(is3d_sampler_plan *plan, const is3d_cells *cells_dev, const double *x_dev, const double *y_dev,
                                        int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events, const is3d_flow_cuts *cuts,
                                        int32_t n_pT, const double *pT_edges, const int32_t *slot, int32_t n_slots,
                                        const is3d_flow_diff_records *records_host, const is3d_decay_mc_table *table_dev /* may be NULL */,
                                        const int32_t *slot_decayed, int32_t n_slots_decayed, uint64_t decay_seed, int32_t lifetime,
                                        const is3d_flow_diff_records *records_decayed, int64_t *n_particles, int64_t *n_final,
                                        int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats);
/* host-pointer one-shot, as is3d_sample_flow */
int is3d_sample_flow_diff(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                          const is3d_options *opts, const is3d_flow_cuts *cuts, int32_t n_pT, const double *pT_edges, const int32_t *slot,
                          int32_t n_slots, const is3d_flow_diff_records *records, const is3d_decay_table *table /* may be NULL */,
                          const int64_t *chosen_mc_id, const int32_t *slot_decayed, int32_t n_slots_decayed, uint64_t decay_seed,
                          int32_t lifetime, const is3d_flow_diff_records *records_decayed, int64_t *n_particles, int64_t *n_final,
                          int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats);

/* Two-particle (delta y, delta phi) correlations of a particle list: how the pairs of ONE event are distributed in
 * relative rapidity and azimuth, beside the same distribution of pairs from neighbouring events.  The flow records above hold the delta phi
 * harmonics of that and nothing in delta y.  A particle maps to a cell (iy, iphi) of an n_y x n_phi grid or to nothing, by the rule of
 * csrc/cf_sampler_pairs.h, shared by host and device, with ratio = (E + pz) / (E - pz) = e^{2y} (one division):
 *   accepted   E - pz > 0, edge[0] <= ratio < edge[n_y], pT_min <= pT < pT_max and pT > 0, pT = sqrt(px^2 + py^2)
 *   iy         the largest k with edge[k] <= ratio, edge[k] = exp(2 (-y_cut + k (2 y_cut / n_y))), by bisection
 *   iphi       the quadrant from the signs of px and py; inside it the largest k with dir[k].x py - dir[k].y px >= 0 (two rounded products,
 *              one subtraction), by bisection, dir[k] = (cos, sin)(2 pi k / n_phi) with the four axis directions exact
 * The tables are computed once on the host and handed to the kernels as bits; no decision goes through log or atan2, so host and device
 * reach the same cell from the same particle bits and every count below is equal on both, bit for bit.
 * Bins are valid when y_cut > 0, pT_max > pT_min >= 0, 1 <= n_y <= 64, n_phi is a multiple of 4 in 4..64 and the edges come out finite and
 * strictly increasing (NaN: invalid).
 * Result (caller-owned): same and mixed [n_classes][2 n_y - 1][n_phi], n_classes = n_slots (n_slots + 1) / 2, class (a <= b) at index
 * a n_slots - a (a - 1) / 2 + (b - a); M [n_events][n_slots], the accepted multiplicities.
 *   same    every ordered pair (i, j), i != j, of one event, both accepted, slot_i <= slot_j, adds 1 to
 *           same[class(slot_i, slot_j)][iy_j - iy_i + n_y - 1][(iphi_j - iphi_i) mod n_phi]
 *   mixed   n_events >= 2: the same with i from event e and j from event (e + 1) mod n_events, without the i != j condition; one event: zero
 * M[e][s] above IS3D_SAMPLER_VN_MAX_COUNT: IS3D_EDOMAIN from the device entries after the run. */
typedef struct {
    double y_cut, pT_min, pT_max;
    int32_t n_y, n_phi;
} is3d_pair_bins;
typedef struct {
    int64_t *same, *mixed, *M;
} is3d_pair_hist;
/* list -> histograms on the host, as the explicit double loop over the pairs: THE definition, no device use, O(M^2) per event.  slot:
 * int32[n_species], species -> slot in [0, n_slots), or -1: dropped.  IS3D_EINVAL: a NULL, n_events, n_slots or n_species < 1, bad bins, a
 * slot outside [-1, n_slots), a particle whose species or event is out of range.  hist is overwritten. */
int is3d_pairs_list(const is3d_pair_bins *bins, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                    int64_t n_particles, const is3d_particle *particles, const is3d_pair_hist *hist);
/* list -> histograms on the DEVICE, without a loop over pairs: a caller's HOST list (any order, any length) is uploaded; cf_pair_cells
 * (thread <-> particle) adds every accepted particle to a 32-bit occupancy block occ[event][slot][iy][iphi]; cf_pair_correlate (workgroup
 * <-> (event, class)) forms the cross-correlation of the occupancy grids in 64-bit integers, which IS the pair histogram.  Its cost does
 * not depend on M^2.  A particle whose species or event is out of range adds nothing and is counted in *n_skipped.  The refusals above
 * (but that one) come before any device use; a good call without a device is IS3D_ENODEVICE; an occupancy block that cannot be allocated
 * is IS3D_ENOMEM naming its size.  n_particles = 0: zero histograms, no launch.  device < 0: the current device. */
int is3d_pairs_list_device(const is3d_pair_bins *bins, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                           int64_t n_particles, const is3d_particle *particles, const is3d_pair_hist *hist, int64_t *n_skipped,
                           int32_t device);
/* The correlation function of every class from the exact integers, in double, on the host.  Per class c:
 *   n_same, n_mixed   the totals of same and mixed over all bins
 *   C[c][dy][dphi]    (same / n_same) / (mixed / n_mixed) where mixed > 0, else 0
 *   C_phi[c][dphi]    the same ratio of the sums over the rows dy with |dy - (n_y - 1)| >= gap_bins (0 where that sum of mixed is 0):
 *                     the delta phi projection with a rapidity gap of gap_bins bins
 *   V[n - 1]          sum C_phi cos(2 pi n dphi / n_phi) / sum C_phi, n = 1..4 (0 when sum C_phi = 0)
 * hist->M is not read.  IS3D_EINVAL: a NULL (C and C_phi may each be NULL: not returned), bad bins, n_slots < 1, gap_bins outside [0, n_y). */
typedef struct {
    int64_t n_same, n_mixed;
    double V[4];
} is3d_pair_result;
int is3d_pairs_correlation(const is3d_pair_bins *bins, const is3d_pair_hist *hist, int32_t n_slots, int32_t gap_bins,
                           double *C /* [n_classes][2 n_y - 1][n_phi] */, double *C_phi /* [n_classes][n_phi] */,
                           is3d_pair_result *out /* [n_classes] */);
/* Writes, per class (a <= b), <results_dir>/pairs/correlation_<labels[a]>_<labels[b]>.dat: two comment lines (the bins; the totals), then a
 * row per bin: delta y (the centre (dy - (n_y - 1)) 2 y_cut / n_y), delta phi (dphi 2 pi / n_phi), same, mixed, C, tab separated.  Doubles
 * are printed by std::to_chars(scientific, 8) as the other writers' values, integers in full.  The pairs/ directory must exist (IS3D_EIO
 * otherwise); a NULL, an empty label or one with a '/', bad bins and n_slots < 1 are IS3D_EINVAL. */
int is3d_write_pairs(const char *results_dir, const is3d_pair_bins *bins, const is3d_pair_hist *hist, int32_t n_slots,
                     const char *const *labels);
/* The pair histograms of a list AFTER its Monte Carlo decays, without the decayed list.  Definition: is3d_pairs_list(bins, n_events,
 * n_slots, slot, table->n, ...) on the list that is3d_decay_particles returns for the same (table, chosen_mc_id, in, particles), whose
 * species are TABLE entries -- equal bit for bit.  *n_final is the length of that list, *n_unbinned = *n_final - sum of M.  How:
 * cf_decay_mc_pairs, thread <-> primary over the decay loop and stream of is3d_decay_particles; every final particle's momentum goes to the
 * rule at once and makes ONE occupancy add; then cf_pair_correlate.  The occupancies do not depend on the launch geometry or on the pieces a
 * list is decayed in (first_particle), but the histograms are not additive over pieces of one event: a caller who decays in pieces
 * passes the whole list's occupancies through one correlate, which this entry does for its list.  slot: int32[table->n].  All pointers
 * HOST memory; hist is overwritten.  stats as for is3d_decay_particles_binned (ms_bin: the decay pass).  IS3D_EINVAL before any device
 * use: every refusal of is3d_decay_particles; the refusals of is3d_pairs_list_device with the table's entries as species; a primary whose
 * event is outside [0, n_events).  n_particles = 0: zero histograms, no launch.  A good call without a device: IS3D_ENODEVICE. */
int is3d_decay_particles_pairs(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                               const is3d_decay_mc_inputs *in, int64_t n_particles, const is3d_particle *particles,
                               const int32_t *slot, int32_t n_slots, const is3d_pair_bins *bins, int32_t n_events,
                               const is3d_pair_hist *hist, int64_t *n_final, int64_t *n_unbinned,
                               is3d_decay_mc_stats *stats /* may be NULL */);
/* is3d_sampler_plan_execute with the list of each event batch turned into occupancies on the device and discarded: fill into the plan's
 * particle workspace, cf_pair_cells into a device-resident occupancy block (zeroed once per run, kept across batches; slot: int32 per
 * species of the plan) and, with table_dev != NULL, cf_decay_mc_pairs of the same batch with first_particle = the number of hadrons of the
 * batches before it (slot_decayed: int32 per table entry) into a second block; after the last batch cf_pair_correlate for each block and
 * one copy to the caller's HOST arrays.
 *   hist          = is3d_pairs_list of the list is3d_sampler_plan_execute returns for the same arguments
 *   hist_decayed  = is3d_decay_particles_pairs of that list with first_particle = 0, seed = decay_seed
 * independent of batch_events and launch geometry, bit for bit.  The plan keeps the blocks and slot maps (sized at first use) and serves
 * its other entries in any order, as before.  table_dev == NULL: slot_decayed, hist_decayed, n_final, n_unbinned and decay_stats are not
 * used.  IS3D_EINVAL before any device use: the refusals of is3d_pairs_list_device for either result, a table of another chosen count or
 * device.  Not offered: the fused sample-and-bin pass, the anisotropic-hydro sampler, several devices. */
int is3d_sampler_plan_execute_pairs(is3d_sampler_plan *plan, const is3d_cells *cells_dev, const double *x_dev, const double *y_dev,
                                    int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events, const is3d_pair_bins *bins,
                                    const int32_t *slot, int32_t n_slots, const is3d_pair_hist *hist_host,
                                    const is3d_decay_mc_table *table_dev /* may be NULL */, const int32_t *slot_decayed, int32_t n_slots_decayed,
                                    uint64_t decay_seed, int32_t lifetime, const is3d_pair_hist *hist_decayed, int64_t *n_particles,
                                    int64_t *n_final, int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats);
/* host-pointer one-shot for the viscous sampler: plan and table create, upload, execute, destroy.  table may be NULL; otherwise chosen_mc_id
 * holds the mc_id of species[0 .. n), which the table must hold.  The bins' and the table's refusals come first, then the plan's. */
int is3d_sample_pairs(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                      const is3d_options *opts, const is3d_pair_bins *bins, const int32_t *slot, int32_t n_slots,
                      const is3d_pair_hist *hist, const is3d_decay_table *table /* may be NULL */, const int64_t *chosen_mc_id,
                      const int32_t *slot_decayed, int32_t n_slots_decayed, uint64_t decay_seed, int32_t lifetime,
                      const is3d_pair_hist *hist_decayed, int64_t *n_particles, int64_t *n_final, int64_t *n_unbinned,
                      is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats);

/* HBT (femtoscopic) correlation functions of a particle list: the one observable above that reads the freeze-out
 * POSITIONS (t, x, y, z) of the sampled hadrons.  Identical-particle pairs of ONE event are binned in the pair momentum KT and the
 * out-side-long components of the relative momentum in the longitudinally comoving frame, and each pair adds cos(q . dx / hbarc) to a
 * numerator.  This is a true O(M^2) loop per event: the weight depends on both positions.  The rule is csrc/cf_sampler_hbt.h, ONE
 * statement for host and device, compiled with contraction off; every decision uses only + - * / sqrt and comparisons on numbers the host
 * computes once (lo = exp(-2 y_cut), hi = exp(2 y_cut), dkT = (kT_max - kT_min) / n_kT, dq = 2 q_max / n_q) and hands over as bits.
 * Bins are valid when y_cut > 0, pT_max > pT_min >= 0, kT_max > kT_min >= 0, 1 <= n_kT <= 16, q_max > 0, 2 <= n_q <= 64 and lo, hi, dkT,
 * dq come out finite and positive (NaN: invalid).
 *   single particle  accepted when E - pz > 0, lo <= (E + pz) / (E - pz) <= hi (one division), pT_min <= sqrt(px^2 + py^2) < pT_max and
 *                    slot[species] >= 0
 *   ordered pair     (i, j), i != j, same event, same slot, both accepted; products are rounded one by one, in this order:
 *     K = (p_i + p_j) / 2, q = p_i - p_j (four components each), KT = sqrt(Kx^2 + Ky^2); rejected unless KT > 0 and kT_min <= KT < kT_max
 *     ikT = (int)((KT - kT_min) / dkT), clamped to n_kT - 1
 *     q_o = (qx Kx + qy Ky) / KT, q_s = (qx Ky - qy Kx) / KT
 *     beta = Kz / K0, g2 = 1 - beta beta; rejected unless g2 > 0; q_l = (qz - beta q0) / sqrt(g2)
 *     u = (q + q_max) / dq for each of q_o, q_s, q_l; rejected unless 0 <= u < n_q for all three; io, is, il = (int)u
 *     den[slot][ikT][io][is][il] += 1
 *     num[slot][ikT][io][is][il] += llrint(cos(phi) 2^32), phi = (((q0 dt - qx dx) - qy dy) - qz dz) / hbarc, dx = x_i - x_j
 *   M[event][slot]   the accepted single-particle multiplicity
 * All words are int64, so the sums do not depend on order, batching or kernel form.  cos is the one libm call: it feeds a term, never a
 * decision, and device and host may differ by one unit per pair there.  A den word above IS3D_SAMPLER_VN_MAX_COUNT is IS3D_EDOMAIN; below
 * that bound num cannot overflow.  The histograms are NOT additive over pieces of one event (pairs across the pieces are missing).
 * kernel_form (device entries; the host entries ignore it): 0 the measured choice, 1 global atomics, 2 a workgroup-private histogram of
 * one slot's n_kT n_q^3 bins in LDS, refused with IS3D_EINVAL naming the word count when it does not fit; every form gives the same bits. */
typedef struct {
    double y_cut, pT_min, pT_max, kT_min, kT_max;
    int32_t n_kT;
    double q_max;
    int32_t n_q, kernel_form;
} is3d_hbt_bins;
typedef struct {
    int64_t *num, *den, *M;   /* num, den [n_slots][n_kT][n_q (out)][n_q (side)][n_q (long)]; M [n_events][n_slots] */
} is3d_hbt_hist;
/* list -> histograms on the host, as the explicit double loop over the pairs: THE definition, no device use.  slot: int32[n_species],
 * species -> slot in [0, n_slots), or -1: dropped.  IS3D_EINVAL: a NULL, n_events, n_slots or n_species < 1, bad bins, a slot outside
 * [-1, n_slots), a particle whose species or event is out of range.  hist is overwritten. */
int is3d_hbt_list(const is3d_hbt_bins *bins, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                  int64_t n_particles, const is3d_particle *particles, const is3d_hbt_hist *hist);
/* list -> histograms on the DEVICE: a caller's HOST list (any order) is uploaded; cf_hbt_select (thread <-> particle) applies the
 * single-particle rule and writes the accepted particles as compact 64-byte records (E, px, py, pz, t, x, y, z) into per-(event, slot)
 * segments (count, scan, fill with a per-segment cursor); cf_hbt_pairs (workgroup <-> (segment, tile of 256 i, run of j tiles); a thread
 * owns one i, the j tiles are staged in LDS) applies the pair rule.  A particle whose species or event is out of range adds nothing and
 * is counted in *n_skipped.  The refusals above (but that one) and kernel_form come before any device use; a good call without a device
 * is IS3D_ENODEVICE; a block that cannot be allocated is IS3D_ENOMEM naming its size.  n_particles = 0: zero histograms, no launch.
 * device < 0: the current device. */
int is3d_hbt_list_device(const is3d_hbt_bins *bins, int32_t n_events, int32_t n_slots, const int32_t *slot, int32_t n_species,
                         int64_t n_particles, const is3d_particle *particles, const is3d_hbt_hist *hist, int64_t *n_skipped,
                         int32_t device);
/* Radii from the exact integers, on the host.  Per (slot, kT bin): c = num / (den 2^32) in every q bin with den >= min_pairs and
 * c >= c_min > 0; a weighted linear least-squares fit (weights den c^2, normal equations in long double) of
 *   ln c = ln lambda - (R_o^2 q_o^2 + R_s^2 q_s^2 + R_l^2 q_l^2 + 2 R_os^2 q_o q_s + 2 R_ol^2 q_o q_l + 2 R_sl^2 q_s q_l) / hbarc^2
 * at the bin centres q = -q_max + (k + 1/2) dq.  R2 holds R_o^2, R_s^2, R_l^2, R_os^2, R_ol^2, R_sl^2 in fm^2 (not their roots), n_bins the
 * number of bins used; singular = 1 (lambda and R2 zero) when the 7 x 7 system has no solution (fewer than 7 bins among them).
 * hist->M is not read.  IS3D_EINVAL: a NULL, bad bins, n_slots < 1, min_pairs < 1, c_min not > 0. */
typedef struct {
    double lambda, R2[6];
    int32_t n_bins, singular;
} is3d_hbt_radii_result;
int is3d_hbt_radii(const is3d_hbt_bins *bins, const is3d_hbt_hist *hist, int32_t n_slots, int64_t min_pairs, double c_min,
                   is3d_hbt_radii_result *out /* [n_slots][n_kT] */);
/* Writes, per slot s and kT bin k, <results_dir>/hbt/correlation_<labels[s]>_kT<k>.dat: two comment lines (the bins; the kT range and the
 * totals), then a row per q bin: the q_o, q_s, q_l centres, den, C = 1 + num / (den 2^32) (1 where den is 0), tab separated; and per slot
 * <results_dir>/hbt/radii_<labels[s]>.dat: a row per kT bin: the kT centre, lambda, the six R^2, n_bins, singular (the fit of
 * is3d_hbt_radii with min_pairs and c_min).  Doubles by std::to_chars(scientific, 8), integers in full.  The hbt/ directory must exist
 * (IS3D_EIO otherwise); a NULL, an empty label or one with a '/', bad bins and n_slots < 1 are IS3D_EINVAL. */
int is3d_write_hbt(const char *results_dir, const is3d_hbt_bins *bins, const is3d_hbt_hist *hist, int32_t n_slots,
                   const char *const *labels, int64_t min_pairs, double c_min);
/* The HBT histograms of a list AFTER its Monte Carlo decays, without the decayed list.  Definition: is3d_hbt_list(bins, n_events, n_slots,
 * slot, table->n, ...) on the list that is3d_decay_particles returns for the same (table, chosen_mc_id, in, particles): den and M equal,
 * num within one unit per pair.  How: the decay loop runs twice over the same counter-based stream, first with a sink that counts the
 * accepted finals per (event, slot), then with a sink that writes their compact records; then cf_hbt_pairs.  Device memory holds the
 * accepted records, never the decayed list.  With in->lifetime = 1 a parent flies before its daughters are born, which is what the
 * positions record.  slot: int32[table->n].  *n_final is the length of the decayed list, *n_unbinned = *n_final - sum of M.  IS3D_EINVAL
 * before any device use: every refusal of is3d_decay_particles; the refusals of is3d_hbt_list_device with the table's entries as species; a
 * primary whose event is outside [0, n_events).  n_particles = 0: zero histograms, no launch. */
int is3d_decay_particles_hbt(const is3d_decay_table *table, int32_t n_chosen, const int64_t *chosen_mc_id,
                             const is3d_decay_mc_inputs *in, int64_t n_particles, const is3d_particle *particles,
                             const int32_t *slot, int32_t n_slots, const is3d_hbt_bins *bins, int32_t n_events,
                             const is3d_hbt_hist *hist, int64_t *n_final, int64_t *n_unbinned,
                             is3d_decay_mc_stats *stats /* may be NULL */);
/* is3d_sampler_plan_execute with the list of each event batch selected and paired on the device and discarded: an event lies whole in one
 * batch, so each batch is complete for its events; the histograms stay on the device across batches and are copied once at the end.
 *   hist          = is3d_hbt_list of the list is3d_sampler_plan_execute returns for the same arguments
 *   hist_decayed  = is3d_decay_particles_hbt of that list with first_particle = 0, seed = decay_seed
 * independent of batch_events, bit for bit.  table_dev == NULL: slot_decayed, hist_decayed, n_final, n_unbinned and decay_stats are not
 * used.  The plan serves its other entries in any order, as before.  IS3D_EINVAL before any device use: the refusals of
 * is3d_hbt_list_device for either result, a table of another chosen count or device.  Not offered: the fused sample-and-bin pass, the
 * anisotropic-hydro sampler, several devices. */
int is3d_sampler_plan_execute_hbt(is3d_sampler_plan *plan, const is3d_cells *cells_dev, const double *x_dev, const double *y_dev,
                                  int32_t n_events, uint64_t seed, int64_t first_cell, int32_t batch_events, const is3d_hbt_bins *bins,
                                  const int32_t *slot, int32_t n_slots, const is3d_hbt_hist *hist_host,
                                  const is3d_decay_mc_table *table_dev /* may be NULL */, const int32_t *slot_decayed, int32_t n_slots_decayed,
                                  uint64_t decay_seed, int32_t lifetime, const is3d_hbt_hist *hist_decayed, int64_t *n_particles,
                                  int64_t *n_final, int64_t *n_unbinned, is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats);
/* host-pointer one-shot for the viscous sampler: plan and table create, upload, execute, destroy.  table may be NULL. */
int is3d_sample_hbt(const is3d_cells *cells, const is3d_species *species, const is3d_df_tables *df, const is3d_sampler_inputs *in,
                    const is3d_options *opts, const is3d_hbt_bins *bins, const int32_t *slot, int32_t n_slots,
                    const is3d_hbt_hist *hist, const is3d_decay_table *table /* may be NULL */, const int64_t *chosen_mc_id,
                    const int32_t *slot_decayed, int32_t n_slots_decayed, uint64_t decay_seed, int32_t lifetime,
                    const is3d_hbt_hist *hist_decayed, int64_t *n_particles, int64_t *n_final, int64_t *n_unbinned,
                    is3d_sampler_stats *stats, is3d_decay_mc_stats *decay_stats);

/* ---------------------------------------------------------------------------------------------
 * Driver: IS3D::run_particlization (src/cpp/iS3D.cpp:74-192; class IS3D, src/cpp/iS3D.h:19-96).  Reads iS3D_parameters.dat,
 * PDG/, tables/, deltaf_coefficients/ from the current directory and writes results/ exactly as the command line tool does
 * (which is this call with surface = NULL).  surface != NULL is the embedding path (read_fo_surf_from_memory +
 * run_particlization(0), iS3D.cpp:27-72, :100-134): HOST arrays already in GeV / fm units, x and y the cell positions (may be
 * NULL).  result may be NULL; otherwise it receives library-allocated copies -- operation 2: the sampled particles ordered
 * by event (what the reference returns in final_particles_, :178-184); operation 1: the spectrum -- to be released with
 * is3d_run_result_free.  include/iS3D_amd.hpp wraps this in a class with the reference's member names.
 * --------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t operation, n_events, n_species, reserved;
    int64_t n_particles;
    is3d_particle *particles;           /* operation 2 */
    int64_t *mc_id;                     /* [n_species] chosen particles, order of PDG/chosen_particles.dat */
    double *mass;                       /* [n_species] */
    int64_t n_spectrum;
    double *spectrum;                   /* operation 1: dN_pTdpTdphidy, species fastest */
} is3d_run_result;

int is3d_run_particlization(const is3d_cells *surface, const double *x, const double *y, int32_t kernel_variant,
                            is3d_run_result *result);
/* The same on an explicit device list (operation 1: the cells are sharded over the devices as is3d_smooth_spectra_multi does;
 * operation 2 samples the shards on their devices and merges the lists, is3d_sample_particles_multi).  devices == NULL && n_devices > 0: ordinals 0 .. n_devices-1.  n_devices <= 0 is what
 * is3d_run_particlization and the command line tool do: the environment decides -- IS3D_DEVICES = "0,2,3" | "all" (default:
 * every visible device), IS3D_REDUCE = "ordered" (default) | "rccl".  mode = 5: a list that was spelled out (devices != NULL here, or
 * IS3D_DEVICES) also shards the spin polarization (is3d_spin_polarization_multi); a bare count (devices == NULL) or no list leaves it on the
 * first device, so that the S files do not depend on how many devices a machine shows. */
int is3d_run_particlization_on(const is3d_cells *surface, const double *x, const double *y, int32_t kernel_variant,
                               const int32_t *devices, int32_t n_devices, int32_t reduce, is3d_run_result *result);
void is3d_run_result_free(is3d_run_result *result);

/* ---------------------------------------------------------------------------------------------
 * Host I/O in the reference's file formats (C++ implementation, C ABI so that tests and other
 * hosts can reach it).  All paths are explicit; the CLI driver passes the reference's hard-coded
 * CWD-relative names.
 * --------------------------------------------------------------------------------------------- */

/* ParameterReader::readFromFile + getVal (src/cpp/ParameterReader.cpp:38-155): `name = value # comment`.
 * Returns IS3D_EIO if the file cannot be read, IS3D_EINVAL if `name` is absent (reference: exit). */
int is3d_param_get(const char *path, const char *name, double *value);

/* Table(filename) (src/cpp/Table.cpp:179-195, arsenal.cpp:406-453): n-column numeric text.  Two-call
 * pattern: data == NULL returns the shape; otherwise fills data[row * n_cols + col] (capacity in
 * doubles).  A last line without a trailing newline is dropped, as in the reference. */
int is3d_table_read(const char *path, int64_t *n_rows, int32_t *n_cols, double *data, int64_t capacity);

/* FO_data_reader::read_surf_VH (mode 1; src/cpp/readindata.cpp:320-468).  Two-call pattern as above
 * (cells == NULL -> only *n_cells).  Fills caller-allocated arrays named in `cells` (non-NULL
 * members of at least n_cells doubles; x,y positions are not kept).  Also returns the
 * surface-volume-weighted averages {T, E, P, muB, nB} (readindata.cpp:422-466) in avg5 if non-NULL. */
int is3d_surface_read_vh(const char *path, int32_t include_baryon, int32_t include_baryondiff_deltaf,
                         int32_t dimension, int64_t *n_cells, double *const *cell_arrays23, double *avg5);

/* FO_data_reader::read_surf_switch (src/cpp/readindata.cpp:133-144) for the viscous-hydro surface formats the
 * smooth path accepts: mode 0 read_surf_VH_old (:148-318), 1 read_surf_VH (:320-468), 4 read_surf_VH_MUSIC (:552-668),
 * 5 read_surf_VH_Vorticity (:470-551: the mode-1 columns, V^tau inside the diffusion block, six thermal-vorticity columns that the
 * viscous-hydro kernels calculate_spectra runs on such a surface do not read; unlike the reference's reader this one also returns the
 * surface averages), 6 read_surf_VH_MUSIC_New (:671-810), 7 read_surf_VH_hiceventgen (:1059-1196).  Same calling pattern and array order
 * as is3d_surface_read_vh; every format is converted to the kernel's conventions the way the reference does (tau
 * Jacobians, hbar*c, p = T s - e, u = gamma v); muB is stored whenever the array is given (modes 4, 6, 7 always
 * carry it), nB and V^mu are zero in modes 4, 6, 7.  Other modes: IS3D_EINVAL. */
int is3d_surface_read(const char *path, int32_t mode, int32_t include_baryon, int32_t include_baryondiff_deltaf,
                      int32_t dimension, int64_t *n_cells, double *const *cell_arrays23, double *avg5);

/* The same readers (modes 0, 1, 4, 5, 6, 7 and the anisotropic-hydro mode 2) behind ONE read and ONE parse of the text, the arrays owned by
 * the library, and a binary sidecar next to the text so that a second run on the same surface skips the parse (no reference counterpart: the
 * reference re-parses `input/surface.dat` with operator>> on every run, readindata.cpp:320-468; the drop-in keeps its result, not its cost).
 *   cache = 0: parse the text, touch nothing else | 1: use `<path>.is3dcache` when it matches the text file as it is now -- size, mtime (ns), a
 *   hash of sampled blocks of its contents, the parse parameters (mode, include_baryon, include_baryondiff_deltaf, dimension) and the sidecar's
 *   own length -- else parse the text and (re)write it (temp file + rename, on a thread of the library's while the caller computes; a directory
 *   that cannot be written to is not an error) | 2: as 1 with a hash of the WHOLE text (reads the text: slower, for the wary).
 *   IS3D_NO_CACHE=1 in the environment forces 0.  The cached arrays and averages are bit for bit what the text parse produced.
 * is3d_surface_arrays: modes 0-7 except 2: n_arrays = 25 -- cell_arrays23 order (T P E tau eta ux uy un dat dax day dan pixx pixy pixn piyy
 * piyn bulkPi muB nB Vx Vy Vn; NULL for the ones the flags leave out) then the positions x, y (columns 2, 3: the sampler's) -- and avg5 as
 * is3d_surface_read; mode 2: n_arrays = 32, the arrays32 of is3d_surface_read_vah, avg5 untouched.  Pointers stay valid until is3d_surface_close.
 *   The sidecar's key (round 5): the text's size, mtime, CHANGE time, inode and device, the sampled (or whole-file) content hash and the parse
 *   parameters -- an edit that restores size and mtime (cp -p, rsync -t, utime) still changes the inode's ctime and is re-parsed.
 * is3d_surface_source: 0 the text was parsed, no sidecar written | 1 parsed, sidecar written (waits for the writer) | 2 loaded from the sidecar.
 * is3d_surface_from_sidecar: 1 when the arrays came from the sidecar, else 0; known when is3d_surface_open returns, never waits. */
typedef struct is3d_surface is3d_surface;
int is3d_surface_open(const char *path, int32_t mode, int32_t include_baryon, int32_t include_baryondiff_deltaf, int32_t dimension,
                      int32_t cache, is3d_surface **surface);
int64_t is3d_surface_cells(const is3d_surface *surface);
int32_t is3d_surface_source(is3d_surface *surface);
int32_t is3d_surface_from_sidecar(const is3d_surface *surface);
int is3d_surface_arrays(const is3d_surface *surface, const double **arrays, int32_t n_arrays, double avg5[5]);
void is3d_surface_close(is3d_surface *surface);
/* the six thermal-vorticity arrays of a mode-5 surface (w: wtx wty wtn wxy wxn wyn, as read, no unit conversion; valid until
 * is3d_surface_close).  A mode-5 sidecar carries them too (one written without them is re-parsed).  IS3D_EINVAL for any other mode. */
int is3d_surface_vorticity(const is3d_surface *surface, const double *w[6]);

/* PDG_Data::read_resonances_conventional (src/cpp/readindata.cpp:1440-1568), reduced to what the
 * smooth path uses.  Two-call pattern (mc_id == NULL -> only *n).  Arrays of capacity entries. */
int is3d_pdg_read(const char *path, int32_t *n, int64_t *mc_id, double *mass, double *gspin,
                  double *baryon, double *sign, int32_t capacity);

/* PDG_Data::read_resonances_smash_box with read_mcid (src/cpp/readindata.cpp:1571-1685, :1201-1418): the line-oriented list of hrg_eos = 3
 * (PDG/pdg_box.dat: "name mass width parity id [id...]", '#' comments) -- degeneracy, baryon number, statistics and the antiparticle
 * entries follow from the digits of the Monte-Carlo ids.  Same outputs and two-call pattern as is3d_pdg_read. */
int is3d_pdg_read_box(const char *path, int32_t *n, int64_t *mc_id, double *mass, double *gspin,
                      double *baryon, double *sign, int32_t capacity);

/* Deltaf_Data::load_df_coefficient_data (src/cpp/deltafReader.cpp:65-219) for one file, mu_B = 0 row.
 * Two-call pattern (T == NULL -> only *n_T). */
int is3d_df_table_read(const char *path, int32_t *n_T, double *T, double *value, int32_t capacity);
/* The same file with every mu_B row (include_baryon = 1): value[iB * n_T + iT].  Two-call pattern
 * (T == NULL -> only *n_T, *n_muB); capacity in doubles of `value`. */
int is3d_df_table_read_full(const char *path, int32_t *n_T, int32_t *n_muB, double *T, double *muB, double *value,
                            int64_t capacity);

/* Gauss_Laguerre::load_roots_and_weights (src/cpp/readindata.cpp:24-53; tables/gla_roots_weights_32_points.txt).
 * Two-call pattern (root == NULL -> only the shape); root/weight[alpha * n_points + k], capacity in doubles each. */
int is3d_gla_read(const char *path, int32_t *n_alpha, int32_t *n_points, double *root, double *weight, int64_t capacity);

/* The df-coefficient generator (generate_delta_f_coefficients/<list>/df_vh_dimensionless/src/deltaf_table.cpp:137-248, :296-395) on the device:
 * the ten tables of deltaf_coefficients/vh/<list>/ for any hadron list, Gauss-Laguerre rule and (T, mu_B) grid.
 *   list      every entry as is3d_pdg_read / is3d_pdg_read_box return it; entries with mass == 0 (the photon) are skipped as in the reference
 *   root, weight   [4][n_gla]: the Gauss-Laguerre rules for alpha = 1, 2, 3, 4 (rows 1..4 of is3d_gla_read's arrays), any n_gla >= 1
 *   T, muB    [n_T], [n_muB] in GeV, any order; T > 0
 *   tables    [10][n_muB][n_T]: c0 T^4, c1 T^3, c2 T^4, c3 T^4, c4 T^5, F / T, G, betabulk / T^4, betaV / T^3, betapi / T^4 -- the numbers the
 *             generator prints (:240-244, :387-391)
 *   integrals NULL, or [20][n_muB][n_T]: J20 J21 J40 J41 N10 N30 N31 M20 M21 A20 A21 B10 nB e p J30 J32 N20 M10 M11 in the generator's units
 * Every sum has a fixed order that depends on n_gla and list->n alone (csrc/cf_dfgen.hip): a point's numbers are bitwise the same from run to
 * run and in whatever grid the point is computed; `integrals` changes no bit of `tables`.
 * Arguments are checked before any device use: null pointers, n <= 0, n_gla <= 0, n_T or n_muB <= 0, T <= 0, a root <= 0, a negative mass and
 * non-finite values are IS3D_EINVAL; a good call without a device is IS3D_ENODEVICE (no CPU path).  Where the reference calls exit(-1) --
 * exp(E/T - b muB/T) + sign <= 0 at a node (thermal_integrands.cpp:18-23), a zero bulk or diffusion denominator (deltaf_table.cpp:228-237), a
 * zero betapi, betabulk or betaV (:370-384) -- and where an output is not finite, the call returns IS3D_EDOMAIN; is3d_last_error() names T, mu_B
 * and the condition(s) of the first such point in grid order (and the list entry for the first case).  `tables` is filled nevertheless. */
typedef struct {
    int32_t n;
    const double *mass, *gspin, *baryon, *sign;
} is3d_hadron_list;
typedef struct {
    double ms_kernel, ms_h2d, ms_d2h;   /* device time of the kernel (events); wall time of the uploads and of the copies back */
    int32_t n_massive;                  /* entries with mass != 0 */
    int32_t reserved;
} is3d_dfgen_stats;
int is3d_df_generate(const is3d_hadron_list *list, int32_t n_gla, const double *const root[4], const double *const weight[4],
                     int32_t n_T, const double *T, int32_t n_muB, const double *muB, int32_t device, double *tables,
                     double *integrals, is3d_dfgen_stats *stats);
/* Writes <dir>/{c0,c1,c2,c3,c4,F,G,betabulk,betaV,betapi}.dat in the generator's format (the two count lines, the label line of
 * deltaf_table.cpp:129-133 / :288-292, then rows `fixed`, setw(8), mu_B outer, T inner), which is3d_df_table_read[_full] read back.  tables as
 * is3d_df_generate fills it.  <dir> is created if missing (one level); an existing <dir>/c0.dat is never overwritten: IS3D_EINVAL.  A value
 * that is not finite is IS3D_EINVAL; IS3D_EIO if a file cannot be written. */
int is3d_df_tables_write(const char *dir, int32_t n_T, const double *T, int32_t n_muB, const double *muB, const double *tables);

/* Writers (src/cpp/emissionfunction.cpp:381-450, :729-772, :1053-1136): append to
 * <dir>/dN_pTdpTdphidy.dat, <dir>/dN_pTdpTdphidy_<mcid>.dat, <dir>/dN_dy_<mcid>.dat,
 * <dir>/vn_continuous/vn_<mcid>.dat in the reference's formatting.  pT/phi/y carry nodes and
 * weights (w may be NULL for write_spectra only). */
int is3d_write_results(const char *results_dir, int32_t dimension, int32_t n_species, const int64_t *mc_id,
                       int32_t n_pT, const double *pT, const double *pT_w, int32_t n_phi, const double *phi,
                       const double *phi_w, int32_t n_y, const double *y, const double *dN);

#ifdef __cplusplus
}
#endif
#endif /* IS3D_AMD_H */

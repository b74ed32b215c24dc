"""ctypes binding of include/is3d_amd.h (lib/libis3d_amd.so) -- plumbing, not the product.

The compute entry points run HIP kernels only; there is no CPU fallback here or in the library:
without the built extension `load()` raises, without a GPU the library returns IS3D_ENODEVICE.
PyTorch is used by callers for device memory and streams; this module itself needs only ctypes+numpy.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# IS3D_USE_DEV_LIB=1: the developer build (`make -C is3d_amd/csrc DEV=1`: A/B switches and cycle-accounting kernels, csrc/errors.h) for tools/
DEV_LIB = os.environ.get("IS3D_USE_DEV_LIB", "") == "1"
LIB_PATH = os.path.join(_HERE, "lib_dev" if DEV_LIB else "lib", "libis3d_amd.so")
CLI_PATH = os.path.join(_HERE, "bin_dev" if DEV_LIB else "bin", "iS3D_amd")

IS3D_OK, IS3D_EINVAL, IS3D_ENODEVICE, IS3D_EDOMAIN, IS3D_ENOMEM, IS3D_EIO = 0, -1, -2, -3, -4, -5

_dp = C.POINTER(C.c_double)

CELL_FIELDS = ["tau", "eta", "dat", "dax", "day", "dan", "ux", "uy", "un", "T", "P", "E",
               "pixx", "pixy", "pixn", "piyy", "piyn", "bulkPi", "muB", "nB", "Vx", "Vy", "Vn"]
# order of the cell_arrays23 argument of is3d_surface_read_vh
SURFACE_READ_ORDER = ["T", "P", "E", "tau", "eta", "ux", "uy", "un", "dat", "dax", "day", "dan",
                      "pixx", "pixy", "pixn", "piyy", "piyn", "bulkPi", "muB", "nB", "Vx", "Vy", "Vn"]


class Cells(C.Structure):
    _fields_ = [("n_cells", C.c_int64)] + [(n, C.c_void_p) for n in CELL_FIELDS]


class Species(C.Structure):
    _fields_ = [("n", C.c_int32), ("mass", _dp), ("sign", _dp), ("degeneracy", _dp), ("baryon", _dp)]


class Grid(C.Structure):
    _fields_ = [("n_pT", C.c_int32), ("pT", _dp), ("n_phi", C.c_int32), ("phi", _dp), ("n_y", C.c_int32), ("y", _dp),
                ("n_eta", C.c_int32), ("eta", _dp), ("eta_w", _dp)]


class DfTables(C.Structure):
    _fields_ = [("n_T", C.c_int32), ("T", _dp), ("n_muB", C.c_int32), ("muB", _dp)] + \
               [(n, _dp) for n in ["c0", "c1", "c2", "c3", "c4", "F", "G", "betabulk", "betaV", "betapi"]]


class FeqmodTables(C.Structure):
    _fields_ = [("n_gla", C.c_int32), ("root1", _dp), ("weight1", _dp), ("root2", _dp), ("weight2", _dp), ("n_pdg", C.c_int32),
                ("pdg_mass", _dp), ("pdg_degeneracy", _dp), ("pdg_sign", _dp), ("T_avg", C.c_double), ("deta_min", C.c_double),
                ("mass_pion0", C.c_double)]


class Particle(C.Structure):
    _fields_ = [("cell", C.c_int64), ("event", C.c_int32), ("species", C.c_int32)] + \
               [(n, C.c_double) for n in ["tau", "x", "y", "eta", "t", "z", "E", "px", "py", "pz"]]


PARTICLE_DTYPE = np.dtype([("cell", "<i8"), ("event", "<i4"), ("species", "<i4")] +
                          [(n, "<f8") for n in ["tau", "x", "y", "eta", "t", "z", "E", "px", "py", "pz"]])


class SamplerInputs(C.Structure):
    _fields_ = [("n_events", C.c_int32), ("n_gla", C.c_int32), ("seed", C.c_uint64), ("y_cut", C.c_double), ("first_cell", C.c_int64),
                ("x", _dp), ("y", _dp), ("root1", _dp), ("weight1", _dp), ("feqmod", C.POINTER(FeqmodTables)), ("fast", C.c_int32),
                ("batch_events", C.c_int32), ("T_avg", C.c_double), ("T_avg_switch", C.c_double), ("muB_avg", C.c_double)]


class SamplerStats(C.Structure):
    _fields_ = [("n_cells_skipped", C.c_int64), ("n_hadrons_drawn", C.c_int64), ("n_momentum_samples", C.c_int64),
                ("n_acceptances", C.c_int64), ("n_classes", C.c_int32), ("reserved", C.c_int32), ("n_cells_breakdown", C.c_int64),
                ("ms_h2d", C.c_double),
                ("ms_prep", C.c_double), ("ms_count", C.c_double), ("ms_fill", C.c_double), ("ms_density", C.c_double), ("ms_poisson", C.c_double),
                ("ms_bin", C.c_double), ("particle_workspace_bytes", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Options(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ["dimension", "df_mode", "include_baryon", "include_bulk_deltaf",
                                         "include_shear_deltaf", "include_baryondiff_deltaf", "regulate_deltaf", "outflow",
                                         "accumulate", "device", "kernel_variant", "cell_chunks"]] + \
               [("workspace_bytes", C.c_int64), ("collapse_species", C.c_int32), ("zero_skip", C.c_int32), ("waves_per_group", C.c_int32), ("reference_bilinear_indexing", C.c_int32),
                ("reserved", C.c_int32 * 4)]


class Status(C.Structure):
    _fields_ = [("code", C.c_int32), ("n_classes", C.c_int32), ("n_cells_skipped", C.c_int64), ("bad_cell", C.c_int64),
                ("n_passes", C.c_int32), ("kernel_variant", C.c_int32), ("ms_prep", C.c_double), ("ms_main", C.c_double),
                ("ms_finalize", C.c_double), ("ms_h2d", C.c_double), ("ms_d2h", C.c_double), ("n_wave_rows", C.c_int64),
                ("n_wave_rows_culled", C.c_int64), ("n_cells_breakdown", C.c_int64), ("n_cells_narrow", C.c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


EXPORTS = ["is3d_last_error", "is3d_version", "is3d_device_count", "is3d_smooth_spectra", "is3d_smooth_spectra_feqmod", "is3d_plan_create",
           "is3d_plan_create_feqmod",
           "is3d_probe_shader_clock", "is3d_plan_output_size", "is3d_plan_execute", "is3d_plan_set_timing", "is3d_plan_timings", "is3d_plan_observables",
           "is3d_plan_main_kernel_name", "is3d_plan_tile_shape", "is3d_plan_workspace_bytes", "is3d_plan_destroy", "is3d_param_get",
           "is3d_table_read", "is3d_surface_read_vh", "is3d_surface_read", "is3d_pdg_read", "is3d_pdg_read_box", "is3d_df_table_read", "is3d_df_table_read_full",
           "is3d_gla_read", "is3d_write_results", "is3d_sample_particles", "is3d_write_particle_list_osc",
           "is3d_run_particlization", "is3d_run_result_free", "is3d_write_sampler_tests", "is3d_smooth_spectra_vah",
           "is3d_smooth_spectra_multi", "is3d_shard_bounds", "is3d_comm_unique_id", "is3d_comm_create", "is3d_comm_rank",
           "is3d_comm_allreduce", "is3d_comm_destroy", "is3d_plan_execute_allreduce", "is3d_run_particlization_on", "is3d_total_yield", "is3d_plan_check", "is3d_sample_particles_multi",
           "is3d_comm_check", "is3d_comm_abort", "is3d_comm_timings", "is3d_comm_set_timeout", "is3d_comm_synchronize", "is3d_surface_open", "is3d_surface_cells", "is3d_surface_source", "is3d_surface_from_sidecar",
           "is3d_surface_arrays", "is3d_surface_close", "is3d_sampler_plan_create", "is3d_sampler_plan_execute", "is3d_sampler_plan_destroy", "is3d_multi_plan_create", "is3d_multi_plan_execute",
           "is3d_multi_plan_shards", "is3d_multi_plan_output_size", "is3d_multi_plan_destroy",
           "is3d_vah_df_read", "is3d_vah_coefficients", "is3d_smooth_spectra_vah_df", "is3d_vah_plan_create", "is3d_vah_plan_output_size",
           "is3d_vah_plan_workspace_bytes", "is3d_vah_plan_execute", "is3d_vah_plan_set_timing", "is3d_vah_plan_timings",
           "is3d_vah_plan_tile_shape", "is3d_vah_plan_destroy", "is3d_surface_read_vah", "is3d_vah_plan_main_kernel_name", "is3d_math_probe", "is3d_resource_counters",
           "is3d_spacetime_distributions", "is3d_plan_execute_spacetime", "is3d_write_spacetime",
           "is3d_spacetime_distributions_feqmod", "is3d_plan_execute_spacetime_feqmod", "is3d_spacetime_distributions_multi",
           "is3d_spin_polarization", "is3d_polarization_plan_create", "is3d_polarization_plan_execute", "is3d_polarization_plan_destroy",
           "is3d_write_polarization", "is3d_surface_vorticity", "is3d_spin_polarization_multi",
           "is3d_pdg_read_decays", "is3d_decay_q_factor", "is3d_resonance_decays", "is3d_decay_plan_create", "is3d_decay_plan_output_size",
           "is3d_decay_plan_execute", "is3d_decay_plan_destroy", "is3d_write_results_decays", "is3d_decay_particles",
           "is3d_decay_mc_table_create", "is3d_decay_mc_table_destroy", "is3d_decay_particles_binned", "is3d_sampler_plan_execute_decayed_binned",
           "is3d_sample_decayed_binned",
           "is3d_sampler_bin_list", "is3d_write_sampler_tests_binned", "is3d_sampler_plan_execute_binned", "is3d_sample_binned", "is3d_sample_binned_multi",
           "is3d_sampler_plan_execute_fused", "is3d_sample_fused", "is3d_sample_fused_multi",
           "is3d_sampler_bin_list_device", "is3d_df_generate", "is3d_df_tables_write",
           "is3d_flow_list", "is3d_flow_list_device", "is3d_flow_merge", "is3d_flow_cumulants", "is3d_decay_particles_flow",
           "is3d_sampler_plan_execute_flow", "is3d_sample_flow", "is3d_write_flow",
           "is3d_flow_diff_list", "is3d_flow_diff_list_device", "is3d_flow_diff_reference", "is3d_flow_diff_cumulants", "is3d_write_flow_diff",
           "is3d_decay_particles_flow_diff", "is3d_sampler_plan_execute_flow_diff", "is3d_sample_flow_diff",
           "is3d_pairs_list", "is3d_pairs_list_device", "is3d_pairs_correlation", "is3d_write_pairs", "is3d_decay_particles_pairs",
           "is3d_sampler_plan_execute_pairs", "is3d_sample_pairs",
           "is3d_hbt_list", "is3d_hbt_list_device", "is3d_hbt_radii", "is3d_write_hbt", "is3d_decay_particles_hbt",
           "is3d_sampler_plan_execute_hbt", "is3d_sample_hbt",
           "is3d_smooth_spectra_vah_multi", "is3d_vah_plan_observables",
           "is3d_spacetime_distributions_vah", "is3d_vah_plan_execute_spacetime",
           "is3d_sample_particles_vah", "is3d_sample_particles_vah_multi", "is3d_sample_binned_vah", "is3d_sample_binned_vah_multi",
           "is3d_total_yield_vah", "is3d_oversample_events"]

VORTICITY_FIELDS = ["wtx", "wty", "wtn", "wxy", "wxn", "wyn"]
POLARIZATION_OUTPUTS = ["St", "Sx", "Sy", "Sn", "Snorm"]


class Vorticity(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in VORTICITY_FIELDS]


class PolarizationOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in POLARIZATION_OUTPUTS]


class PolarizationStats(C.Structure):
    _fields_ = [("code", C.c_int32), ("n_classes", C.c_int32), ("n_chunks", C.c_int32), ("reserved", C.c_int32),
                ("ms_cells", C.c_double), ("ms_reduce", C.c_double), ("ms_h2d", C.c_double), ("ms_d2h", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}

class DecayTable(C.Structure):
    _fields_ = [("n", C.c_int32), ("mc_id", C.c_void_p), ("mass", C.c_void_p), ("width", C.c_void_p), ("stable", C.c_void_p),
                ("n_channels", C.c_void_p), ("npart", C.c_void_p), ("branch_ratio", C.c_void_p), ("daughters", C.c_void_p)]


class DecayStats(C.Structure):
    _fields_ = [("code", C.c_int32), ("n_parents", C.c_int32), ("n_channels", C.c_int32), ("n_adjusted", C.c_int32), ("n_clamps", C.c_int64), ("n_points", C.c_int64),
                ("ms_tables", C.c_double), ("ms_feed", C.c_double), ("ms_h2d", C.c_double), ("ms_d2h", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DecayMcInputs(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("first_particle", C.c_int64), ("lifetime", C.c_int32), ("device", C.c_int32)]


class DecayMcStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ["n_primaries", "n_decays", "n_final", "n_stuck", "n_trials", "n_exhausted"]] + \
               [(n, C.c_int32) for n in ["max_stack", "max_depth", "n_closed_channels", "reserved"]] + \
               [(n, C.c_double) for n in ["ms_h2d", "ms_count", "ms_fill", "ms_d2h", "ms_bin"]]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class SpacetimeBins(C.Structure):
    _fields_ = [("tau_min", C.c_double), ("tau_max", C.c_double), ("r_min", C.c_double), ("r_max", C.c_double),
                ("tau_bins", C.c_int32), ("r_bins", C.c_int32)]


class SpacetimeOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ["dN_dy", "dN_taudtaudy", "dN_twopirdrdy", "dN_twopitaurdtaudrdy", "dN_dydeta", "dN_dy_cell"]]


class SpacetimeStats(C.Structure):
    _fields_ = [("code", C.c_int32), ("n_classes", C.c_int32), ("n_cells_skipped", C.c_int64), ("n_tau_outside", C.c_int64),
                ("n_r_outside", C.c_int64), ("n_tau_negative", C.c_int64), ("n_r_negative", C.c_int64), ("bad_cell", C.c_int64),
                ("n_passes", C.c_int32), ("reserved", C.c_int32), ("ms_prep", C.c_double), ("ms_cells", C.c_double), ("ms_bins", C.c_double),
                ("ms_h2d", C.c_double), ("ms_d2h", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if n != "reserved"}


class SpacetimeFeqmodStats(C.Structure):
    _fields_ = [("n_cells_breakdown", C.c_int64), ("n_renorm_skipped", C.c_int64), ("first_cell_out_of_range", C.c_int64),
                ("ms_renorm", C.c_double), ("ms_linear", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


SPACETIME_OUTPUTS = ["dN_dy", "dN_taudtaudy", "dN_twopirdrdy", "dN_twopitaurdtaudrdy", "dN_dydeta", "dN_dy_cell"]


def _spacetime_bins(bins):
    return SpacetimeBins(float(bins["tau_min"]), float(bins["tau_max"]), float(bins["r_min"]), float(bins["r_max"]), int(bins["tau_bins"]),
                         int(bins["r_bins"]))


def spacetime_shapes(n_species, n_cells, bins, dimension, n_eta):
    """Shapes of the operation-0 outputs (include/is3d_amd.h, is3d_spacetime_out)."""
    tb, rb = int(bins["tau_bins"]), int(bins["r_bins"])
    return dict(dN_dy=(n_species,), dN_taudtaudy=(n_species, tb), dN_twopirdrdy=(n_species, rb), dN_twopitaurdtaudrdy=(n_species, tb, rb),
                dN_dydeta=(n_species, 1 if dimension == 3 else n_eta), dN_dy_cell=(n_species, n_cells))


REDUCE_ORDERED, REDUCE_RCCL = 0, 1
IS3D_EPEER = -6
COMM_ID_BYTES = 128


class HadronList(C.Structure):
    _fields_ = [("n", C.c_int32), ("mass", _dp), ("gspin", _dp), ("baryon", _dp), ("sign", _dp)]


class DfgenStats(C.Structure):
    _fields_ = [("ms_kernel", C.c_double), ("ms_h2d", C.c_double), ("ms_d2h", C.c_double), ("n_massive", C.c_int32), ("reserved", C.c_int32)]


DFGEN_INTEGRALS = ["J20", "J21", "J40", "J41", "N10", "N30", "N31", "M20", "M21", "A20", "A21", "B10", "nB", "e", "p", "J30", "J32", "N20", "M10", "M11"]


class Is3dError(RuntimeError):
    def __init__(self, code, msg, bad_cell=None):
        super().__init__("is3d_amd error %d: %s" % (code, msg))
        self.code = code
        self.bad_cell = bad_cell


_LIB = None


def build(verbose=False):
    """Compile the HIP library and the CLI in-tree (hipcc --offload-arch=gfx950)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"], stdout=out)
    return LIB_PATH


def load():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: the HIP extension is not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C is3d_amd/csrc`).  There is no CPU fallback." % LIB_PATH)
    try:
        # torch bundles its own libamdhip64.so.7; if our library pulled in /opt/rocm's copy first, the
        # process would hold two HIP runtimes and the second one finds no GPU.  Importing torch first
        # makes the loader resolve our DT_NEEDED libamdhip64.so.7 to the copy that is already mapped.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    L.is3d_last_error.restype = C.c_char_p
    L.is3d_version.restype = C.c_char_p
    L.is3d_plan_main_kernel_name.restype = C.c_char_p
    L.is3d_plan_main_kernel_name.argtypes = [C.c_void_p]
    L.is3d_smooth_spectra.argtypes = [C.POINTER(Cells), C.POINTER(Species), C.POINTER(Grid), C.POINTER(DfTables),
                                      C.POINTER(Options), _dp, C.POINTER(Status)]
    L.is3d_plan_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Species), C.POINTER(Grid), C.POINTER(DfTables),
                                   C.POINTER(Options), C.c_int64]
    L.is3d_smooth_spectra_feqmod.argtypes = [C.POINTER(Cells), C.POINTER(Species), C.POINTER(Grid), C.POINTER(DfTables),
                                             C.POINTER(FeqmodTables), C.POINTER(Options), _dp, C.POINTER(Status)]
    L.is3d_plan_create_feqmod.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Species), C.POINTER(Grid), C.POINTER(DfTables),
                                          C.POINTER(FeqmodTables), C.POINTER(Options), C.c_int64]
    L.is3d_probe_shader_clock.argtypes = [C.c_int32, C.c_double, C.POINTER(C.c_double)]
    L.is3d_plan_output_size.restype = C.c_int64
    L.is3d_plan_output_size.argtypes = [C.c_void_p]
    L.is3d_plan_workspace_bytes.restype = C.c_int64
    L.is3d_plan_workspace_bytes.argtypes = [C.c_void_p]
    L.is3d_plan_tile_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.is3d_plan_execute.argtypes = [C.c_void_p, C.POINTER(Cells), C.c_void_p, C.c_void_p, C.POINTER(Status)]
    L.is3d_plan_observables.argtypes = [C.c_void_p, C.c_void_p, _dp, _dp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.is3d_plan_set_timing.argtypes = [C.c_void_p, C.c_int32]
    L.is3d_plan_timings.argtypes = [C.c_void_p, C.POINTER(Status)]
    L.is3d_plan_destroy.argtypes = [C.c_void_p]
    L.is3d_plan_destroy.restype = None
    L.is3d_param_get.argtypes = [C.c_char_p, C.c_char_p, _dp]
    L.is3d_table_read.argtypes = [C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), _dp, C.c_int64]
    L.is3d_surface_read_vh.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64),
                                       C.POINTER(_dp), _dp]
    L.is3d_surface_read.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int64),
                                    C.POINTER(_dp), _dp]
    L.is3d_pdg_read.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64), _dp, _dp, _dp, _dp, C.c_int32]
    L.is3d_df_table_read.argtypes = [C.c_char_p, C.POINTER(C.c_int32), _dp, _dp, C.c_int32]
    L.is3d_df_table_read_full.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, _dp, _dp, C.c_int64]
    # the host-pointer sampler entries: a head per family, a tail per kind, the device list between them in the _multi form
    heads = dict(viscous=[C.POINTER(Cells), C.POINTER(Species), C.POINTER(DfTables), C.POINTER(SamplerInputs), C.POINTER(Options)],
                 vah=[C.POINTER(VahCells), C.POINTER(Species), C.POINTER(VahDfTables), C.POINTER(SamplerInputs), C.POINTER(Options)])
    tails = dict(list=[C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(SamplerStats)],
                 binned=[C.POINTER(SamplerTestBins), C.POINTER(SamplerHist), C.POINTER(C.c_int64), C.POINTER(SamplerStats)])
    for name, (family, kind) in SAMPLER_ENTRIES.items():
        getattr(L, name).argtypes = heads[family] + tails[kind]
        getattr(L, name + "_multi").argtypes = heads[family] + [C.POINTER(C.c_int32), C.c_int32] + tails[kind]
    L.is3d_write_particle_list_osc.argtypes = [C.c_char_p, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]
    L.is3d_gla_read.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, _dp, C.c_int64]
    L.is3d_write_results.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int32, _dp, _dp,
                                     C.c_int32, _dp, _dp, C.c_int32, _dp, _dp]
    L.is3d_smooth_spectra_multi.argtypes = [C.POINTER(Cells), C.POINTER(Species), C.POINTER(Grid), C.POINTER(DfTables),
                                            C.POINTER(FeqmodTables), C.POINTER(Options), C.POINTER(C.c_int32), C.c_int32, C.c_int32,
                                            _dp, C.POINTER(Status), C.POINTER(Status)]
    L.is3d_shard_bounds.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.is3d_comm_unique_id.argtypes = [C.c_char_p]
    L.is3d_comm_create.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_int32, C.c_int32, C.c_int32]
    L.is3d_comm_rank.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.is3d_comm_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.is3d_comm_destroy.argtypes = [C.c_void_p]
    L.is3d_comm_destroy.restype = None
    L.is3d_plan_execute_allreduce.argtypes = [C.c_void_p, C.POINTER(Cells), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Status)]
    L.is3d_comm_check.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]
    L.is3d_comm_abort.argtypes = [C.c_void_p]
    L.is3d_comm_timings.argtypes = [C.c_void_p, _dp]
    L.is3d_plan_check.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    L.is3d_multi_plan_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Species), C.POINTER(Grid), C.POINTER(DfTables),
                                         C.POINTER(FeqmodTables), C.POINTER(Options), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int64]
    L.is3d_multi_plan_execute.argtypes = [C.c_void_p, C.POINTER(Cells), _dp, C.POINTER(Status), C.POINTER(Status)]
    L.is3d_multi_plan_shards.argtypes = [C.c_void_p]
    L.is3d_multi_plan_output_size.argtypes = [C.c_void_p]
    L.is3d_multi_plan_output_size.restype = C.c_int64
    L.is3d_multi_plan_destroy.argtypes = [C.c_void_p]
    L.is3d_multi_plan_destroy.restype = None
    L.is3d_spacetime_distributions.argtypes = [C.POINTER(Cells), _dp, _dp, C.POINTER(Species), C.POINTER(Grid), _dp, _dp, C.POINTER(DfTables),
                                               C.POINTER(Options), C.POINTER(SpacetimeBins), C.POINTER(SpacetimeOut), C.POINTER(SpacetimeStats)]
    L.is3d_plan_execute_spacetime.argtypes = [C.c_void_p, C.POINTER(Cells), C.c_void_p, C.c_void_p, _dp, _dp, C.POINTER(SpacetimeBins),
                                              C.POINTER(SpacetimeOut), C.c_void_p, C.POINTER(SpacetimeStats)]
    L.is3d_spacetime_distributions_feqmod.argtypes = [C.POINTER(Cells), _dp, _dp, C.POINTER(Species), C.POINTER(Grid), _dp, _dp,
                                                      C.POINTER(DfTables), C.POINTER(FeqmodTables), C.POINTER(Options), C.POINTER(SpacetimeBins),
                                                      C.POINTER(SpacetimeOut), C.POINTER(SpacetimeStats), C.POINTER(SpacetimeFeqmodStats)]
    L.is3d_spacetime_distributions_multi.argtypes = [C.POINTER(Cells), _dp, _dp, C.POINTER(Species), C.POINTER(Grid), _dp, _dp,
                                                     C.POINTER(DfTables), C.POINTER(FeqmodTables), C.POINTER(Options), C.POINTER(C.c_int32),
                                                     C.c_int32, C.POINTER(SpacetimeBins), C.POINTER(SpacetimeOut), C.POINTER(SpacetimeStats),
                                                     C.POINTER(SpacetimeStats)]
    L.is3d_plan_execute_spacetime_feqmod.argtypes = [C.c_void_p, C.POINTER(Cells), C.c_void_p, C.c_void_p, _dp, _dp, C.POINTER(SpacetimeBins),
                                                     C.POINTER(SpacetimeOut), C.c_void_p, C.POINTER(SpacetimeStats), C.POINTER(SpacetimeFeqmodStats)]
    L.is3d_write_spacetime.argtypes = [C.c_char_p, C.POINTER(SpacetimeBins), C.c_int32, C.POINTER(C.c_int64), C.c_int32, _dp,
                                       C.POINTER(SpacetimeOut)]
    L.is3d_spin_polarization.argtypes = [C.POINTER(Cells), C.POINTER(Vorticity), C.POINTER(Species), C.POINTER(Grid), C.c_double,
                                         C.POINTER(Options), C.POINTER(PolarizationOut), C.POINTER(PolarizationStats)]
    L.is3d_spin_polarization_multi.argtypes = [C.POINTER(Cells), C.POINTER(Vorticity), C.POINTER(Species), C.POINTER(Grid), C.c_double,
                                               C.POINTER(Options), C.POINTER(C.c_int32), C.c_int32, C.POINTER(PolarizationOut),
                                               C.POINTER(PolarizationStats), C.POINTER(PolarizationStats)]
    L.is3d_polarization_plan_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Species), C.POINTER(Grid), C.POINTER(Options), C.c_int64]
    L.is3d_polarization_plan_execute.argtypes = [C.c_void_p, C.POINTER(Cells), C.POINTER(Vorticity), C.c_double, C.POINTER(PolarizationOut),
                                                 C.c_void_p, C.POINTER(PolarizationStats)]
    L.is3d_polarization_plan_destroy.argtypes = [C.c_void_p]
    L.is3d_polarization_plan_destroy.restype = None
    L.is3d_write_polarization.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, _dp,
                                          C.POINTER(PolarizationOut)]
    L.is3d_surface_vorticity.argtypes = [C.c_void_p, C.POINTER(_dp)]
    _i32p, _i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    L.is3d_pdg_read_decays.argtypes = [C.c_char_p, _i32p, _i32p, _i64p, _dp, _dp, _i32p, _i32p, _i32p, _dp, _i64p, C.c_int32, C.c_int32]
    L.is3d_decay_q_factor.restype = C.c_double
    L.is3d_decay_q_factor.argtypes = [C.c_double] * 4
    L.is3d_resonance_decays.argtypes = [C.POINTER(DecayTable), C.c_int32, _i64p, C.POINTER(Grid), C.c_int32, C.c_int32, _dp,
                                        C.POINTER(DecayStats)]
    L.is3d_decay_plan_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(DecayTable), C.c_int32, _i64p, C.POINTER(Grid), C.c_int32, C.c_int32]
    L.is3d_decay_plan_output_size.restype = C.c_int64
    L.is3d_decay_plan_output_size.argtypes = [C.c_void_p]
    L.is3d_decay_plan_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DecayStats)]
    L.is3d_decay_plan_destroy.argtypes = [C.c_void_p]
    L.is3d_decay_plan_destroy.restype = None
    L.is3d_write_results_decays.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, _dp, C.c_int32, _dp, C.c_int32, _dp, _dp]
    L.is3d_df_generate.argtypes = [C.POINTER(HadronList), C.c_int32, C.POINTER(_dp), C.POINTER(_dp), C.c_int32, _dp, C.c_int32, _dp, C.c_int32,
                                   _dp, _dp, C.POINTER(DfgenStats)]
    L.is3d_df_tables_write.argtypes = [C.c_char_p, C.c_int32, _dp, C.c_int32, _dp, _dp]
    L.is3d_smooth_spectra_vah_multi.argtypes = [C.POINTER(VahCells), C.POINTER(Species), C.POINTER(Grid), C.POINTER(VahDfTables),
                                                C.POINTER(Options), C.POINTER(C.c_int32), C.c_int32, C.c_int32, _dp, C.POINTER(Status),
                                                C.POINTER(Status)]
    L.is3d_vah_plan_observables.argtypes = [C.c_void_p, C.c_void_p, _dp, _dp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.is3d_spacetime_distributions_vah.argtypes = [C.POINTER(VahCells), _dp, _dp, C.POINTER(Species), C.POINTER(Grid), _dp, _dp,
                                                   C.POINTER(VahDfTables), C.POINTER(Options), C.POINTER(SpacetimeBins), C.POINTER(SpacetimeOut),
                                                   C.POINTER(SpacetimeStats)]
    L.is3d_vah_plan_execute_spacetime.argtypes = [C.c_void_p, C.POINTER(VahCells), C.c_void_p, C.c_void_p, _dp, _dp, C.POINTER(SpacetimeBins),
                                                  C.POINTER(SpacetimeOut), C.c_void_p, C.POINTER(SpacetimeStats)]
    _LIB = L
    return L


def _check(rc):
    if rc != 0:
        raise Is3dError(rc, load().is3d_last_error().decode())


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(_dp)


DF_NAMES_2D = ["c0", "c1", "c2", "c3", "c4", "F", "G", "betabulk", "betaV", "betapi"]

DEFAULT_OPTS = dict(dimension=3, df_mode=1, include_baryon=0, include_bulk_deltaf=1, include_shear_deltaf=1,
                    include_baryondiff_deltaf=0, regulate_deltaf=1, outflow=1, accumulate=0, device=-1,
                    kernel_variant=0, cell_chunks=0, workspace_bytes=0, collapse_species=0, zero_skip=0, waves_per_group=0,
                    reference_bilinear_indexing=0)


def _pack_common(species, grid, df, opts):
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    keep = {}
    sp = {k: _f64(species[k]) for k in ["mass", "sign", "degeneracy", "baryon"]}
    g = {k: _f64(grid[k]) for k in ["pT", "phi", "y", "eta", "eta_w"]}
    d = {k: _f64(df[k]) for k in ["T", "c0", "c2", "F", "betabulk", "betapi"]}
    keep.update(sp=sp, g=g, d=d)
    full = None
    if "2d" in df:   # full (mu_B, T) grids: needed (and used) only with include_baryon = 1
        full = {k: _f64(df["2d"][k]) for k in DF_NAMES_2D}
        full["muB"] = _f64(df["muB"])
        keep["full"] = full
    sps = Species(len(sp["mass"]), _p(sp["mass"]), _p(sp["sign"]), _p(sp["degeneracy"]), _p(sp["baryon"]))
    gs = Grid(len(g["pT"]), _p(g["pT"]), len(g["phi"]), _p(g["phi"]), len(g["y"]), _p(g["y"]), len(g["eta"]),
              _p(g["eta"]), _p(g["eta_w"]))
    ds = DfTables()
    ds.n_T, ds.T = len(d["T"]), _p(d["T"])
    if full is not None:
        ds.n_muB, ds.muB = len(full["muB"]), _p(full["muB"])
        for k in DF_NAMES_2D:
            assert full[k].shape == (ds.n_muB, ds.n_T), k
            setattr(ds, k, _p(full[k]))
    else:
        ds.n_muB = 1
        for k in ["c0", "c2", "F", "betabulk", "betapi"]:
            setattr(ds, k, _p(d[k]))
    os_ = Options()
    for k, v in o.items():
        setattr(os_, k, int(v))
    ny_eff = 1 if o["dimension"] == 2 else len(g["y"])
    nout = len(sp["mass"]) * len(g["pT"]) * len(g["phi"]) * ny_eff
    return sps, gs, ds, os_, nout, keep


VAH_FIELDS = ["tau", "eta", "ux", "uy", "un", "dat", "dax", "day", "dan", "T", "pitt", "pitx", "pity", "pitn", "pixx", "pixy", "pixn",
              "piyy", "piyn", "pinn", "bulkPi", "Wx", "Wy", "Lambda", "aL", "c0", "c1", "c2", "c3", "c4"]


class VahCells(C.Structure):
    _fields_ = [("n_cells", C.c_int64)] + [(f, _dp) for f in VAH_FIELDS]


class VahDfTables(C.Structure):
    _fields_ = [("n_L", C.c_int32), ("n_aL", C.c_int32), ("L", _dp), ("aL", _dp), ("c0", _dp), ("c1", _dp), ("c2", _dp), ("c3", _dp), ("c4", _dp)]


def _pack_vah_tables(tab, keep):
    """is3d_vah_df_tables from the dict of is3d_amd.inputs.vah_df_tables() / vah_df_read()."""
    a = {k: _f64(tab[k]) for k in ("L", "aL", "c0", "c1", "c2", "c3", "c4")}
    for k in ("c0", "c1", "c2", "c3", "c4"):
        assert a[k].shape == (len(a["aL"]), len(a["L"])), k
    keep["vah_tab"] = a
    return VahDfTables(len(a["L"]), len(a["aL"]), _p(a["L"]), _p(a["aL"]), _p(a["c0"]), _p(a["c1"]), _p(a["c2"]), _p(a["c3"]), _p(a["c4"]))


_VAH_DUMMY_DF = dict(T=[0.1, 0.15, 0.2], c0=[0, 0, 0], c2=[0, 0, 0], F=[0, 0, 0], betabulk=[1, 1, 1], betapi=[1, 1, 1])


def _vah_cells_struct(cells, held, device=False):
    cs = VahCells()
    if device:
        cs.n_cells = int(cells["n_cells"])
        for f in VAH_FIELDS:
            p = cells.get(f)
            if p:
                setattr(cs, f, C.cast(C.c_void_p(int(p)), _dp))
        return cs
    n = len(cells["tau"])
    cs.n_cells = n
    for f in VAH_FIELDS:
        a = cells.get(f)
        if a is not None:
            a = _f64(a)
            assert a.shape == (n,), f
            held.append(a)
            setattr(cs, f, _p(a))
    return cs


def smooth_spectra_vah(cells, species, grid, opts=None, out=None, tab=None):
    """is3d_smooth_spectra_vah (the drop-in for calculate_dN_pTdpTdphidy_VAH_PL).  cells: dict of host arrays per VAH_FIELDS.
    tab (dict L, aL, c0..c4): is3d_smooth_spectra_vah_df -- the cells' c0..c4 are ignored, the coefficients come from the
    (Lambda, alpha_L) tables (src/cuda/deltafReader.cu:224-278)."""
    L = load()
    sps, gs, _, os_, nout, keep = _pack_common(species, grid, _VAH_DUMMY_DF, opts)
    held = []
    if tab is not None:
        cells = {k: v for k, v in cells.items() if k not in ("c0", "c1", "c2", "c3", "c4")}
    cs = _vah_cells_struct(cells, held)
    if out is None:
        out = np.zeros(nout)
    st = Status()
    L.is3d_smooth_spectra_vah.argtypes = [C.POINTER(VahCells), C.POINTER(Species), C.POINTER(Grid), C.POINTER(Options), _dp, C.POINTER(Status)]
    L.is3d_smooth_spectra_vah_df.argtypes = [C.POINTER(VahCells), C.POINTER(Species), C.POINTER(Grid), C.POINTER(VahDfTables), C.POINTER(Options), _dp,
                                             C.POINTER(Status)]
    if tab is not None:
        ts = _pack_vah_tables(tab, keep)
        rc = L.is3d_smooth_spectra_vah_df(C.byref(cs), C.byref(sps), C.byref(gs), C.byref(ts), C.byref(os_), _p(out), C.byref(st))
    else:
        rc = L.is3d_smooth_spectra_vah(C.byref(cs), C.byref(sps), C.byref(gs), C.byref(os_), _p(out), C.byref(st))
    if rc != 0:
        raise Is3dError(rc, L.is3d_last_error().decode(), bad_cell=st.bad_cell)
    return out, st.as_dict()


def vah_coefficients(tab, Lambda, aL, device=-1):
    """is3d_vah_coefficients: per-cell c0..c4 (divided by hbarc^3) from the tables, evaluated on the device.  Lambda in GeV.
    Raises Is3dError(IS3D_EDOMAIN) with .bad_cell and .values (zeros at the offending cells) for a cell beyond the last node."""
    L = load()
    keep = {}
    ts = _pack_vah_tables(tab, keep)
    lam, al = _f64(Lambda), _f64(aL)
    n = len(lam)
    out = [np.zeros(n) for _ in range(5)]
    bad = C.c_int64(-1)
    L.is3d_vah_coefficients.argtypes = [C.POINTER(VahDfTables), C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int32, C.POINTER(C.c_int64)]
    rc = L.is3d_vah_coefficients(C.byref(ts), n, _p(lam), _p(al), *[_p(x) for x in out], int(device), C.byref(bad))
    vals = {"c%d" % k: out[k] for k in range(5)}
    if rc != 0:
        e = Is3dError(rc, L.is3d_last_error().decode(), bad_cell=bad.value)
        e.values = vals
        raise e
    return vals


def vah_df_read(directory):
    """is3d_vah_df_read: <dir>/c{0..4}_vah1.dat -> dict L, aL, c0..c4 ([n_aL][n_L])."""
    L = load()
    nL, naL = C.c_int32(), C.c_int32()
    L.is3d_vah_df_read.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, _dp, _dp, C.c_int64]
    _check(L.is3d_vah_df_read(directory.encode(), C.byref(nL), C.byref(naL), None, None, None, 0))
    Lg, ag, c = np.zeros(nL.value), np.zeros(naL.value), np.zeros((5, naL.value, nL.value))
    _check(L.is3d_vah_df_read(directory.encode(), C.byref(nL), C.byref(naL), _p(Lg), _p(ag), _p(c), c.size))
    d = dict(L=Lg, aL=ag)
    for k in range(5):
        d["c%d" % k] = c[k].copy()
    return d


VAH_SURFACE_ORDER = VAH_FIELDS[:25] + ["E", "P", "PL", "Wt", "Wn", "x", "y"]


def surface_read_vah(path, dimension=3):
    """is3d_surface_read_vah (mode 2, read_surf_VAH_PLMatch) -> dict of the 32 arrays of VAH_SURFACE_ORDER."""
    L = load()
    n = C.c_int64(0)
    L.is3d_surface_read_vah.argtypes = [C.c_char_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(_dp)]
    _check(L.is3d_surface_read_vah(path.encode(), int(dimension), C.byref(n), None))
    arrs = {f: np.zeros(n.value) for f in VAH_SURFACE_ORDER}
    ptrs = (_dp * 32)(*[_p(arrs[f]) for f in VAH_SURFACE_ORDER])
    if n.value > 0:
        _check(L.is3d_surface_read_vah(path.encode(), int(dimension), C.byref(n), ptrs))
    return arrs


def spacetime_distributions_vah(cells, species, grid, bins, opts=None, per_cell=False, tab=None):
    """Operation 0 for anisotropic hydro (is3d_spacetime_distributions_vah): cells is a dict of host arrays per VAH_FIELDS plus "x" and "y";
    grid needs pT_w and phi_w.  Returns the dict of spacetime_distributions -- the RAW bin sums dN_dy, dN_taudtaudy, dN_twopirdrdy,
    dN_twopitaurdtaudrdy, dN_dydeta, with per_cell also dN_dy_cell -- and "stats".  tab (dict L, aL, c0..c4): the cells' c0..c4 are ignored,
    the coefficients come from the (Lambda, alpha_L) tables.  Is3dError carries .bad_cell for IS3D_EDOMAIN."""
    L = load()
    sps, gs, _, os_, _, keep = _pack_common(species, grid, _VAH_DUMMY_DF, opts)
    held = []
    fields = {k: v for k, v in cells.items() if k in VAH_FIELDS and not (tab is not None and k in ("c0", "c1", "c2", "c3", "c4"))}
    cs = _vah_cells_struct(fields, held)
    n = cs.n_cells
    xa = None if cells.get("x") is None else _f64(cells["x"])
    ya = None if cells.get("y") is None else _f64(cells["y"])
    pw, fw = _f64(grid["pT_w"]), _f64(grid["phi_w"])
    shapes = spacetime_shapes(len(keep["sp"]["mass"]), n, bins, os_.dimension, len(keep["g"]["eta"]))
    res = {k: np.zeros(v) for k, v in shapes.items() if k != "dN_dy_cell" or per_cell}
    so = SpacetimeOut(*[res[k].ctypes.data if k in res else None for k in SPACETIME_OUTPUTS])
    b = _spacetime_bins(bins)
    st = SpacetimeStats()
    ts = _pack_vah_tables(tab, keep) if tab is not None else None
    rc = L.is3d_spacetime_distributions_vah(C.byref(cs), _p(xa) if xa is not None else None, _p(ya) if ya is not None else None, C.byref(sps),
                                            C.byref(gs), _p(pw), _p(fw), C.byref(ts) if ts is not None else None, C.byref(os_), C.byref(b),
                                            C.byref(so), C.byref(st))
    if rc != 0:
        raise Is3dError(rc, L.is3d_last_error().decode(), bad_cell=st.bad_cell)
    res["stats"] = st.as_dict()
    return res


class VahPlan:
    """Device-resident VAH plan (is3d_vah_plan_*): cell arrays and the output are device pointers (ints); with `tab` the
    coefficients are interpolated on the device from (Lambda, aL) and c0..c4 need not be given."""

    def __init__(self, species, grid, opts=None, tab=None, max_cells=1):
        L = load()
        sps, gs, _, os_, self.output_size, self._keep = _pack_common(species, grid, _VAH_DUMMY_DF, opts)
        ts = _pack_vah_tables(tab, self._keep) if tab is not None else None
        L.is3d_vah_plan_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Species), C.POINTER(Grid), C.POINTER(VahDfTables), C.POINTER(Options), C.c_int64]
        L.is3d_vah_plan_execute.argtypes = [C.c_void_p, C.POINTER(VahCells), C.c_void_p, C.c_void_p, C.POINTER(Status)]
        L.is3d_vah_plan_timings.argtypes = [C.c_void_p, C.POINTER(Status)]
        L.is3d_vah_plan_set_timing.argtypes = [C.c_void_p, C.c_int32]
        L.is3d_vah_plan_tile_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.is3d_vah_plan_output_size.argtypes = [C.c_void_p]
        L.is3d_vah_plan_output_size.restype = C.c_int64
        L.is3d_vah_plan_workspace_bytes.argtypes = [C.c_void_p]
        L.is3d_vah_plan_workspace_bytes.restype = C.c_int64
        L.is3d_vah_plan_destroy.argtypes = [C.c_void_p]
        L.is3d_vah_plan_destroy.restype = None
        self._h = C.c_void_p()
        _check(L.is3d_vah_plan_create(C.byref(self._h), C.byref(sps), C.byref(gs), C.byref(ts) if ts is not None else None, C.byref(os_), int(max_cells)))
        assert L.is3d_vah_plan_output_size(self._h) == self.output_size
        self.workspace_bytes = L.is3d_vah_plan_workspace_bytes(self._h)
        jt, r = C.c_int32(), C.c_int32()
        L.is3d_vah_plan_tile_shape(self._h, C.byref(jt), C.byref(r))
        self.tile_shape = (jt.value, r.value)
        L.is3d_vah_plan_main_kernel_name.argtypes = [C.c_void_p]
        L.is3d_vah_plan_main_kernel_name.restype = C.c_char_p
        self.main_kernel_name = L.is3d_vah_plan_main_kernel_name(self._h).decode()

    def set_timing(self, enable=True):
        _check(load().is3d_vah_plan_set_timing(self._h, 1 if enable else 0))

    def execute(self, n_cells, cell_ptrs, out_ptr, stream=0, want_status=True):
        cs = _vah_cells_struct(dict(cell_ptrs, n_cells=n_cells), None, device=True)
        st = Status()
        rc = load().is3d_vah_plan_execute(self._h, C.byref(cs), C.c_void_p(int(out_ptr)), C.c_void_p(int(stream or 0)), C.byref(st) if want_status else None)
        if rc != 0:
            raise Is3dError(rc, load().is3d_last_error().decode(), bad_cell=st.bad_cell)
        return st.as_dict() if want_status else None

    def observables(self, dN_ptr, pT_w, phi_w, dndy_ptr=0, spec2pi_ptr=0, vn_ptr=0, stream=0):
        """is3d_vah_plan_observables: as Plan.observables -- device pointers (ints) in and out, host weight arrays (pT_w may be None when
        dN/dy is not asked for)."""
        pw, fw = None if pT_w is None else _f64(pT_w), _f64(phi_w)
        _check(load().is3d_vah_plan_observables(self._h, C.c_void_p(int(dN_ptr)), None if pw is None else _p(pw), _p(fw), C.c_void_p(int(dndy_ptr or 0)),
                                                C.c_void_p(int(spec2pi_ptr or 0)), C.c_void_p(int(vn_ptr or 0)), C.c_void_p(int(stream or 0))))

    def execute_spacetime(self, n_cells, cell_ptrs, x_ptr, y_ptr, pT_w, phi_w, bins, out_ptrs, stream=0, want_stats=True):
        """is3d_vah_plan_execute_spacetime: as Plan.execute_spacetime -- cell arrays, x, y and the outputs (dict per SPACETIME_OUTPUTS,
        dN_dy_cell optional) are device pointers (ints), the weights host arrays."""
        cs = _vah_cells_struct(dict(cell_ptrs, n_cells=n_cells), None, device=True)
        pw, fw = _f64(pT_w), _f64(phi_w)
        so = SpacetimeOut(*[C.c_void_p(int(out_ptrs[k])) if out_ptrs.get(k) else None for k in SPACETIME_OUTPUTS])
        b = _spacetime_bins(bins)
        st = SpacetimeStats()
        rc = load().is3d_vah_plan_execute_spacetime(self._h, C.byref(cs), C.c_void_p(int(x_ptr or 0)), C.c_void_p(int(y_ptr or 0)), _p(pw), _p(fw),
                                                    C.byref(b), C.byref(so), C.c_void_p(int(stream or 0)), C.byref(st) if want_stats else None)
        if rc != 0:
            raise Is3dError(rc, load().is3d_last_error().decode(), bad_cell=st.bad_cell)
        return st.as_dict() if want_stats else None

    def timings(self):
        st = Status()
        _check(load().is3d_vah_plan_timings(self._h, C.byref(st)))
        return st.as_dict()

    def close(self):
        if self._h:
            load().is3d_vah_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pack_feqmod(fq, keep):
    """is3d_feqmod_tables from the dict of is3d_amd.inputs.feqmod_tables()."""
    a = {k: _f64(fq[k]) for k in ["root1", "weight1", "root2", "weight2", "pdg_mass", "pdg_degeneracy", "pdg_sign"]}
    keep["fq"] = a
    return FeqmodTables(len(a["root1"]), _p(a["root1"]), _p(a["weight1"]), _p(a["root2"]), _p(a["weight2"]), len(a["pdg_mass"]),
                        _p(a["pdg_mass"]), _p(a["pdg_degeneracy"]), _p(a["pdg_sign"]), float(fq["T_avg"]), float(fq["deta_min"]),
                        float(fq["mass_pion0"]))


def smooth_spectra(cells, species, grid, df, opts=None, out=None, fq=None):
    """Host-pointer entry is3d_smooth_spectra (the drop-in for calculate_dN_pTdpTdphidy); with fq (df_mode 3, 4)
    is3d_smooth_spectra_feqmod (the drop-in for calculate_dN_ptdptdphidy_feqmod).
    cells: dict of numpy arrays (host).  Returns (dN flat numpy array, status dict)."""
    L = load()
    sps, gs, ds, os_, nout, keep = _pack_common(species, grid, df, opts)
    n = len(cells["tau"])
    cs = Cells()
    cs.n_cells = n
    held = []
    for f in CELL_FIELDS:
        a = cells.get(f)
        if a is not None:
            a = _f64(a)
            assert a.shape == (n,), f
            held.append(a)
            setattr(cs, f, a.ctypes.data)
    if out is None:
        out = np.zeros(nout)
    assert out.dtype == np.float64 and out.size == nout and out.flags.c_contiguous
    st = Status()
    if fq is not None:
        fqs = _pack_feqmod(fq, keep)
        rc = L.is3d_smooth_spectra_feqmod(C.byref(cs), C.byref(sps), C.byref(gs), C.byref(ds), C.byref(fqs), C.byref(os_), _p(out), C.byref(st))
    else:
        rc = L.is3d_smooth_spectra(C.byref(cs), C.byref(sps), C.byref(gs), C.byref(ds), C.byref(os_), _p(out), C.byref(st))
    _check(rc)
    return out, st.as_dict()


def spacetime_distributions(cells, species, grid, df, bins, opts=None, per_cell=False, x=None, y=None, fq=None):
    """Operation 0 (is3d_spacetime_distributions, the drop-in for calculate_dN_dX): host arrays in, a dict of numpy arrays out -- the RAW bin
    sums dN_dy [S], dN_taudtaudy [S][tau_bins], dN_twopirdrdy [S][r_bins], dN_twopitaurdtaudrdy [S][tau_bins][r_bins], dN_dydeta
    [S][n_eta | 1], with per_cell also dN_dy_cell [S][n_cells] -- and "stats".  grid needs pT_w and phi_w; x, y default to cells["x"], cells["y"];
    bins: dict tau_min, tau_max, tau_bins, r_min, r_max, r_bins.  With fq (df_mode 3, 4): is3d_spacetime_distributions_feqmod (the drop-in for
    calculate_dN_dX_feqmod), and "feqmod_stats" as well."""
    L = load()
    sps, gs, ds, os_, _, keep = _pack_common(species, grid, df, opts)
    n = len(cells["tau"])
    cs = Cells()
    cs.n_cells = n
    held = []
    for f in CELL_FIELDS:
        a = cells.get(f)
        if a is not None:
            a = _f64(a)
            assert a.shape == (n,), f
            held.append(a)
            setattr(cs, f, a.ctypes.data)
    x = cells.get("x") if x is None else x
    y = cells.get("y") if y is None else y
    xa = None if x is None else _f64(x)
    ya = None if y is None else _f64(y)
    pw, fw = _f64(grid["pT_w"]), _f64(grid["phi_w"])
    dim = os_.dimension
    shapes = spacetime_shapes(len(keep["sp"]["mass"]), n, bins, dim, len(keep["g"]["eta"]))
    res = {k: np.zeros(v) for k, v in shapes.items() if k != "dN_dy_cell" or per_cell}
    so = SpacetimeOut(*[res[k].ctypes.data if k in res else None for k in SPACETIME_OUTPUTS])
    b = _spacetime_bins(bins)
    st = SpacetimeStats()
    xp, yp = (_p(xa) if xa is not None else None), (_p(ya) if ya is not None else None)
    if fq is not None:
        fqs = _pack_feqmod(fq, keep)
        fst = SpacetimeFeqmodStats()
        rc = L.is3d_spacetime_distributions_feqmod(C.byref(cs), xp, yp, C.byref(sps), C.byref(gs), _p(pw), _p(fw), C.byref(ds), C.byref(fqs),
                                                   C.byref(os_), C.byref(b), C.byref(so), C.byref(st), C.byref(fst))
        _check(rc)
        res["feqmod_stats"] = fst.as_dict()
    else:
        rc = L.is3d_spacetime_distributions(C.byref(cs), xp, yp, C.byref(sps), C.byref(gs), _p(pw), _p(fw), C.byref(ds), C.byref(os_), C.byref(b),
                                            C.byref(so), C.byref(st))
        _check(rc)
    res["stats"] = st.as_dict()
    return res


def _pack_devices(devices):
    """The devices argument of the multi-device wrappers -> (c_int32 array or None, n_devices, n_stats): None or an int n means no list and that
    count (None or 0: every visible device; n: the ordinals 0 .. n - 1), a sequence its entries; n_stats: the shards the library reports on."""
    if devices is None or isinstance(devices, (int, np.integer)):
        nd, dv = int(devices or 0), None
    else:
        nd = len(devices)
        dv = (C.c_int32 * max(nd, 1))(*[int(d) for d in devices])
    return dv, nd, nd if nd > 0 else max(load().is3d_device_count(), 1)


def spacetime_distributions_multi(cells, species, grid, df, bins, opts=None, devices=None, fq=None, per_cell=False, x=None, y=None):
    """is3d_spacetime_distributions_multi: operation 0 with the per-cell stage on one contiguous cell shard per entry of devices (an ordinal may
    repeat; an int n means the ordinals 0 .. n - 1; None or 0 every visible device) and ONE bin stage on devices[0].  Arguments and result as
    spacetime_distributions (fq: df_mode 3, 4), plus "shard_stats", one dict per shard.  Everything but the 2+1D dN_dydeta is bitwise the
    single-device result for any shard count; that one is reproducible for a given shard count.  An Is3dError raised here carries bad_cell
    (global), stats and shard_stats."""
    L = load()
    sps, gs, ds, os_, _, keep = _pack_common(species, grid, df, opts)
    n = len(cells["tau"])
    cs = Cells()
    cs.n_cells = n
    held = []
    for f in CELL_FIELDS:
        a = cells.get(f)
        if a is not None:
            a = _f64(a)
            assert a.shape == (n,), f
            held.append(a)
            setattr(cs, f, a.ctypes.data)
    x = cells.get("x") if x is None else x
    y = cells.get("y") if y is None else y
    xa = None if x is None else _f64(x)
    ya = None if y is None else _f64(y)
    pw, fw = _f64(grid["pT_w"]), _f64(grid["phi_w"])
    shapes = spacetime_shapes(len(keep["sp"]["mass"]), n, bins, os_.dimension, len(keep["g"]["eta"]))
    res = {k: np.zeros(v) for k, v in shapes.items() if k != "dN_dy_cell" or per_cell}
    so = SpacetimeOut(*[res[k].ctypes.data if k in res else None for k in SPACETIME_OUTPUTS])
    b = _spacetime_bins(bins)
    dv, nd, n_stats = _pack_devices(devices)
    st = SpacetimeStats()
    sst = (SpacetimeStats * n_stats)()
    fqs = _pack_feqmod(fq, keep) if fq is not None else None
    xp, yp = (_p(xa) if xa is not None else None), (_p(ya) if ya is not None else None)
    rc = L.is3d_spacetime_distributions_multi(C.byref(cs), xp, yp, C.byref(sps), C.byref(gs), _p(pw), _p(fw), C.byref(ds),
                                              C.byref(fqs) if fqs is not None else None, C.byref(os_), dv, nd, C.byref(b), C.byref(so),
                                              C.byref(st), sst)
    stats, shard_stats = st.as_dict(), [sst[i].as_dict() for i in range(n_stats)]
    if rc != 0:
        err = Is3dError(rc, L.is3d_last_error().decode(), bad_cell=stats["bad_cell"])
        err.stats, err.shard_stats = stats, shard_stats
        raise err
    res["stats"] = stats
    res["shard_stats"] = shard_stats
    return res


def write_spacetime(results_dir, bins, mc_id, eta_values, res):
    """is3d_write_spacetime: the four files per species of calculate_dN_dX from the raw sums of spacetime_distributions."""
    L = load()
    mc = np.ascontiguousarray(mc_id, dtype=np.int64)
    ev = _f64(np.atleast_1d(eta_values))
    arrs = {k: _f64(res[k]) for k in SPACETIME_OUTPUTS[1:5]}
    so = SpacetimeOut(*[arrs[k].ctypes.data if k in arrs else None for k in SPACETIME_OUTPUTS])
    b = _spacetime_bins(bins)
    _check(L.is3d_write_spacetime(results_dir.encode(), C.byref(b), len(mc), mc.ctypes.data_as(C.POINTER(C.c_int64)), len(ev), _p(ev),
                                  C.byref(so)))


def _polzn_pack(species, grid, opts):
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    keep = {}
    sp = {k: _f64(species[k]) for k in ["mass", "sign", "degeneracy", "baryon"]}
    g = {k: _f64(grid[k]) for k in ["pT", "phi", "y", "eta", "eta_w"]}
    keep.update(sp=sp, g=g)
    sps = Species(len(sp["mass"]), _p(sp["mass"]), _p(sp["sign"]), _p(sp["degeneracy"]), _p(sp["baryon"]))
    gs = Grid(len(g["pT"]), _p(g["pT"]), len(g["phi"]), _p(g["phi"]), len(g["y"]), _p(g["y"]), len(g["eta"]), _p(g["eta"]), _p(g["eta_w"]))
    os_ = Options()
    for k, v in o.items():
        setattr(os_, k, int(v))
    ny_eff = 1 if o["dimension"] == 2 else len(g["y"])
    nout = len(sp["mass"]) * len(g["pT"]) * len(g["phi"]) * ny_eff
    return sps, gs, os_, nout, keep


def _host_cells(cells, held):
    n = len(next(v for f in CELL_FIELDS for v in [cells.get(f)] if v is not None))
    cs = Cells()
    cs.n_cells = n
    for f in CELL_FIELDS:
        a = cells.get(f)
        if a is not None:
            a = _f64(a)
            assert a.shape == (n,), f
            held.append(a)
            setattr(cs, f, a.ctypes.data)
    return cs


def _host_vorticity(vorticity, n_cells, held):
    if vorticity is None:
        return None
    vs = Vorticity()
    for f in VORTICITY_FIELDS:
        a = vorticity.get(f)
        if a is not None:
            a = _f64(a)
            assert a.shape == (n_cells,), f
            held.append(a)
            setattr(vs, f, a.ctypes.data)
    return vs


def spin_polarization(cells, vorticity, species, grid, T, opts=None):
    """is3d_spin_polarization (mode 5, the drop-in for calculate_spin_polzn with the vorticity read at the global cell index): host arrays
    in -> dict St, Sx, Sy, Sn, Snorm (flat, spectrum layout) and "stats".  vorticity: dict of VORTICITY_FIELDS arrays (None: refused by the
    library); T: the surface's single temperature; opts: dimension, device, workspace_bytes."""
    L = load()
    sps, gs, os_, nout, keep = _polzn_pack(species, grid, opts)
    held = []
    cs = _host_cells(cells, held)
    vs = _host_vorticity(vorticity, cs.n_cells, held)
    res = {k: np.zeros(nout) for k in POLARIZATION_OUTPUTS}
    po = PolarizationOut(*[res[k].ctypes.data for k in POLARIZATION_OUTPUTS])
    st = PolarizationStats()
    _check(L.is3d_spin_polarization(C.byref(cs), C.byref(vs) if vs is not None else None, C.byref(sps), C.byref(gs), float(T), C.byref(os_),
                                    C.byref(po), C.byref(st)))
    res["stats"] = st.as_dict()
    return res


def spin_polarization_multi(cells, vorticity, species, grid, T, opts=None, devices=None):
    """is3d_spin_polarization_multi: the spin polarization with one contiguous cell shard per entry of devices (an ordinal may repeat; an int n
    means the ordinals 0 .. n - 1; None or 0 every visible device), the shards' class sums added in shard order on devices[0].  Arguments and
    result as spin_polarization, plus "shard_stats", one dict per shard.  One shard is spin_polarization on devices[0] bit for bit; N shards
    are bitwise reproducible for that shard count and differ from the single device by the association of the additions only.  An Is3dError
    raised here carries stats and shard_stats."""
    L = load()
    sps, gs, os_, nout, keep = _polzn_pack(species, grid, opts)
    held = []
    cs = _host_cells(cells, held)
    vs = _host_vorticity(vorticity, cs.n_cells, held)
    res = {k: np.zeros(nout) for k in POLARIZATION_OUTPUTS}
    po = PolarizationOut(*[res[k].ctypes.data for k in POLARIZATION_OUTPUTS])
    dv, nd, n_stats = _pack_devices(devices)
    st = PolarizationStats()
    sst = (PolarizationStats * n_stats)()
    rc = L.is3d_spin_polarization_multi(C.byref(cs), C.byref(vs) if vs is not None else None, C.byref(sps), C.byref(gs), float(T), C.byref(os_),
                                        dv, nd, C.byref(po), C.byref(st), sst)
    stats, shard_stats = st.as_dict(), [sst[i].as_dict() for i in range(n_stats)]
    if rc != 0:
        err = Is3dError(rc, L.is3d_last_error().decode())
        err.stats, err.shard_stats = stats, shard_stats
        raise err
    res["stats"] = stats
    res["shard_stats"] = shard_stats
    return res


class PolarizationPlan:
    """Device-resident spin polarization (is3d_polarization_plan_*): cell and vorticity arrays and the five outputs are device pointers (ints),
    e.g. torch tensors' data_ptr(); `stream` a hipStream_t handle."""

    def __init__(self, species, grid, opts=None, max_cells=1):
        L = load()
        sps, gs, os_, nout, _ = _polzn_pack(species, grid, opts)
        self._h = C.c_void_p()
        _check(L.is3d_polarization_plan_create(C.byref(self._h), C.byref(sps), C.byref(gs), C.byref(os_), int(max_cells)))
        self.output_size = nout

    def execute(self, n_cells, cell_ptrs, vort_ptrs, T, out_ptrs, stream=0, want_stats=True):
        """cell_ptrs / vort_ptrs: dict field -> device pointer (vort_ptrs None: refused); out_ptrs: dict St, Sx, Sy, Sn, Snorm -> device pointer."""
        cs = Cells()
        cs.n_cells = int(n_cells)
        for f in CELL_FIELDS:
            p = cell_ptrs.get(f)
            if p:
                setattr(cs, f, int(p))
        vs = None
        if vort_ptrs is not None:
            vs = Vorticity(*[int(vort_ptrs[f]) if vort_ptrs.get(f) else None for f in VORTICITY_FIELDS])
        po = PolarizationOut(*[int(out_ptrs[k]) if out_ptrs.get(k) else None for k in POLARIZATION_OUTPUTS])
        st = PolarizationStats()
        _check(load().is3d_polarization_plan_execute(self._h, C.byref(cs), C.byref(vs) if vs is not None else None, float(T), C.byref(po),
                                                     C.c_void_p(int(stream or 0)), C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def close(self):
        if self._h:
            load().is3d_polarization_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_polarization(results_dir, dimension, pT, phi, y, res, n_species=None):
    """is3d_write_polarization: appends St.dat, Sx.dat, Sy.dat, Sn.dat under results_dir from the five arrays of spin_polarization (the
    ratios S / Snorm are formed in the library).  y may be None in 2+1D."""
    L = load()
    pT, phi = _f64(pT), _f64(phi)
    yv = _f64(y if y is not None else [0.0])
    arrs = {k: _f64(res[k]) for k in POLARIZATION_OUTPUTS}
    ny_eff = 1 if dimension == 2 else len(yv)
    if n_species is None:
        n_species = arrs["St"].size // (len(pT) * len(phi) * ny_eff)
    po = PolarizationOut(*[arrs[k].ctypes.data for k in POLARIZATION_OUTPUTS])
    _check(L.is3d_write_polarization(results_dir.encode(), int(dimension), int(n_species), len(pT), _p(pT), len(phi), _p(phi),
                                     len(yv), _p(yv), C.byref(po)))


def pdg_read_decays(path):
    """is3d_pdg_read_decays (hrg_eos 1, 2): dict of per-entry mc_id, mass, width, stable, n_channels and per-channel npart, branch_ratio,
    daughters [n_channels_total, 5] (entry i's channels follow those of the entries before it)."""
    L = load()
    n, nc = C.c_int32(0), C.c_int32(0)
    _check(L.is3d_pdg_read_decays(path.encode(), C.byref(n), C.byref(nc), None, None, None, None, None, None, None, None, 0, 0))
    t = dict(mc_id=np.zeros(n.value, np.int64), mass=np.zeros(n.value), width=np.zeros(n.value), stable=np.zeros(n.value, np.int32),
             n_channels=np.zeros(n.value, np.int32), npart=np.zeros(nc.value, np.int32), branch_ratio=np.zeros(nc.value),
             daughters=np.zeros((nc.value, 5), np.int64))
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))  # noqa: E731
    _check(L.is3d_pdg_read_decays(path.encode(), C.byref(n), C.byref(nc), i64(t["mc_id"]), _p(t["mass"]), _p(t["width"]), i32(t["stable"]),
                                  i32(t["n_channels"]), i32(t["npart"]), _p(t["branch_ratio"]), i64(t["daughters"]), n.value, nc.value))
    return t


def decay_q_factor(mass_parent, m1, m2, m3):
    """is3d_decay_q_factor: calculate_Q_factor, the 3-body normalisation (host)."""
    return load().is3d_decay_q_factor(float(mass_parent), float(m1), float(m2), float(m3))


def _decay_pack(table, chosen_mc_id, grid):
    keep = dict(mc_id=np.ascontiguousarray(table["mc_id"], np.int64), mass=_f64(table["mass"]), width=_f64(table["width"]),
                stable=np.ascontiguousarray(table["stable"], np.int32), n_channels=np.ascontiguousarray(table["n_channels"], np.int32),
                npart=np.ascontiguousarray(table["npart"], np.int32), branch_ratio=_f64(table["branch_ratio"]),
                daughters=np.ascontiguousarray(table["daughters"], np.int64).reshape(-1))
    ts = DecayTable(len(keep["mc_id"]), *[keep[k].ctypes.data for k in ["mc_id", "mass", "width", "stable", "n_channels", "npart",
                                                                         "branch_ratio", "daughters"]])
    ch = np.ascontiguousarray(chosen_mc_id, np.int64)
    g = {k: _f64(grid[k]) if grid.get(k) is not None else _f64([0.0]) for k in ["pT", "phi", "y"]}
    gs = Grid(len(g["pT"]), _p(g["pT"]), len(g["phi"]), _p(g["phi"]), len(g["y"]), _p(g["y"]), 0, None, None)
    keep.update(ch=ch, g=g)
    return ts, ch, gs, keep


def resonance_decays(table, chosen_mc_id, grid, dN, dimension=2, device=-1):
    """is3d_resonance_decays: the feed-down of a host spectrum (flat, species fastest, n_y_eff = 1 in 2+1D).  Returns (fed-down copy, stats).
    table: pdg_read_decays' dict; chosen_mc_id: the chosen list in its order; grid: dict pT, phi (and y in 3+1D)."""
    L = load()
    ts, ch, gs, keep = _decay_pack(table, chosen_mc_id, grid)
    out = np.array(dN, dtype=np.float64, copy=True).reshape(-1)
    st = DecayStats()
    _check(L.is3d_resonance_decays(C.byref(ts), len(ch), ch.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(gs), int(dimension), int(device),
                                   _p(out), C.byref(st)))
    return out, st.as_dict()


class DecayPlan:
    """Device-resident feed-down (is3d_decay_plan_*): execute(dN_ptr) feeds down a DEVICE spectrum in place, e.g. a torch tensor's data_ptr()."""

    def __init__(self, table, chosen_mc_id, grid, dimension=2, device=-1):
        L = load()
        ts, ch, gs, _ = _decay_pack(table, chosen_mc_id, grid)
        self._h = C.c_void_p()
        _check(L.is3d_decay_plan_create(C.byref(self._h), C.byref(ts), len(ch), ch.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(gs),
                                        int(dimension), int(device)))
        self.output_size = L.is3d_decay_plan_output_size(self._h)

    def execute(self, dN_ptr, stream=0, want_stats=True):
        st = DecayStats()
        _check(load().is3d_decay_plan_execute(self._h, C.c_void_p(int(dN_ptr)), C.c_void_p(int(stream or 0)),
                                              C.byref(st) if want_stats else None))
        return st.as_dict() if want_stats else None

    def close(self):
        if self._h:
            load().is3d_decay_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_results_decays(results_dir, dimension, pT, phi, y, dN, n_species=None):
    """is3d_write_results_decays: appends dN_pTdpTdphidy_resonance_decays.dat and dN_dpTdphidy_resonance_decays.dat under results_dir."""
    L = load()
    pT, phi = _f64(pT), _f64(phi)
    yv = _f64(y if y is not None else [0.0])
    d = _f64(dN).reshape(-1)
    ny_eff = 1 if dimension == 2 else len(yv)
    if n_species is None:
        n_species = d.size // (len(pT) * len(phi) * ny_eff)
    _check(L.is3d_write_results_decays(results_dir.encode(), int(dimension), int(n_species), len(pT), _p(pT), len(phi), _p(phi), len(yv),
                                       _p(yv), _p(d)))


def decay_particles(table, chosen_mc_id, particles, seed=1, first_particle=0, lifetime=0, device=-1, capacity=None):
    """is3d_decay_particles: a sampled list (PARTICLE_DTYPE, species indexing chosen_mc_id) decayed to stable particles by Monte Carlo on the
    device.  Returns (out, origin, stats): out[k]["species"] indexes the TABLE (table["mc_id"] is the id list of write_particle_list_osc),
    origin[k] is the primary's index in `particles`.  capacity = None sizes the buffers from a count-only first call."""
    L = load()
    ts, ch, _, keep = _decay_pack(table, chosen_mc_id, dict(pT=[1.0], phi=[0.0], y=[0.0]))
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    inp = DecayMcInputs(int(seed), int(first_particle), int(lifetime), int(device))
    st, cnt = DecayMcStats(), C.c_int64(0)
    L.is3d_decay_particles.argtypes = [C.POINTER(DecayTable), C.c_int32, C.POINTER(C.c_int64), C.POINTER(DecayMcInputs), C.c_int64, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(DecayMcStats)]
    head = (C.byref(ts), len(ch), ch.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(inp), len(particles), particles.ctypes.data)
    if capacity is None:
        _check(L.is3d_decay_particles(*head, None, None, 0, C.byref(cnt), C.byref(st)))
        capacity = int(cnt.value)
    out = np.zeros(max(int(capacity), 1), dtype=PARTICLE_DTYPE)
    origin = np.zeros(max(int(capacity), 1), dtype=np.int64)
    _check(L.is3d_decay_particles(*head, out.ctypes.data, origin.ctypes.data, int(capacity), C.byref(cnt), C.byref(st)))
    n = int(cnt.value)
    return out[:n], origin[:n], st.as_dict()


def _check_decayed(rc, st, nf, nu, **extra):
    """A decayed-and-binned entry's return code: an Is3dError carries the decay stats (.stats) and whatever else the entry had in hand."""
    d = st.as_dict()
    d["n_final"], d["n_unbinned"] = int(nf.value), int(nu.value)
    if rc != 0:
        e = Is3dError(rc, load().is3d_last_error().decode())
        e.stats = d
        for k, v in extra.items():
            setattr(e, k, v)
        raise e
    return d


def _slot_map(table, slot):
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    assert slot.shape == (len(table["mc_id"]),), (slot.shape, len(table["mc_id"]))
    return slot


def stable_slots(table, mc_ids=None):
    """The slot map of a decayed-and-binned run: (int32[table entries], the slots' mc_id).  mc_ids = None: every stable entry of the table in
    table order; otherwise those of mc_ids that are stable in the table, in the order given (the run driver's rule for its chosen list)."""
    ids, stable = np.asarray(table["mc_id"], np.int64), np.asarray(table["stable"]) != 0
    slot = np.full(len(ids), -1, np.int32)
    if mc_ids is None:
        keep = np.nonzero(stable)[0]
    else:
        first = {}
        for e, i in enumerate(ids):
            first.setdefault(int(i), e)
        keep = [first[int(i)] for i in mc_ids if int(i) in first and stable[first[int(i)]]]
    for k, e in enumerate(keep):
        slot[e] = k
    return slot, ids[np.asarray(keep, np.int64)] if len(keep) else np.zeros(0, np.int64)


class DecayMcTable:
    """is3d_decay_mc_table_*: the decay table as the Monte Carlo kernels read it, analysed once and resident on `device`.  Every refusal of the
    table is raised here (Is3dError, IS3D_EINVAL) before any device use.  .stats: max_stack, max_depth, n_closed_channels come with a run."""

    def __init__(self, table, chosen_mc_id, device=-1):
        L = load()
        ts, ch, _, self._keep = _decay_pack(table, chosen_mc_id, dict(pT=[1.0], phi=[0.0], y=[0.0]))
        self.table, self.n_entries, self.n_chosen = table, len(table["mc_id"]), len(ch)
        L.is3d_decay_mc_table_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(DecayTable), C.c_int32, C.POINTER(C.c_int64), C.c_int32]
        L.is3d_decay_mc_table_destroy.argtypes = [C.c_void_p]
        L.is3d_decay_mc_table_destroy.restype = None
        self._h = C.c_void_p()
        _check(L.is3d_decay_mc_table_create(C.byref(self._h), C.byref(ts), len(ch), ch.ctypes.data_as(C.POINTER(C.c_int64)), int(device)))

    def close(self):
        if self._h:
            load().is3d_decay_mc_table_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decay_particles_binned(table, chosen_mc_id, particles, slot, n_slots, bins, n_events, seed=1, first_particle=0, lifetime=0, device=-1):
    """is3d_decay_particles_binned: a sampled list decayed on the device with every final particle binned at once -- the histograms of
    sampler_bin_list on decay_particles' list with species -> slot[species], slot -1 dropped.  slot: int32 per table entry.  Returns
    (dict of int64 histograms of n_slots species, stats dict with n_final, n_unbinned and the tallies of decay_particles)."""
    L = load()
    ts, ch, _, keep = _decay_pack(table, chosen_mc_id, dict(pT=[1.0], phi=[0.0], y=[0.0]))
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    slot = _slot_map(table, slot)
    inp = DecayMcInputs(int(seed), int(first_particle), int(lifetime), int(device))
    b = _pack_bins(bins)
    h, out = _hist_arrays(bins, n_events, n_slots)
    st, nf, nu = DecayMcStats(), C.c_int64(0), C.c_int64(0)
    L.is3d_decay_particles_binned.argtypes = [C.POINTER(DecayTable), C.c_int32, C.POINTER(C.c_int64), C.POINTER(DecayMcInputs), C.c_int64, C.c_void_p,
                                              C.c_void_p, C.c_int32, C.POINTER(SamplerTestBins), C.c_int32, C.POINTER(SamplerHist),
                                              C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(DecayMcStats)]
    rc = L.is3d_decay_particles_binned(C.byref(ts), len(ch), ch.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(inp), len(particles),
                                       particles.ctypes.data, slot.ctypes.data, int(n_slots), C.byref(b), int(n_events), C.byref(h), C.byref(nf),
                                       C.byref(nu), C.byref(st))
    return out, _check_decayed(rc, st, nf, nu, hist=out)


def decay_particles_flow(table, chosen_mc_id, particles, slot, n_slots, cuts, n_events, seed=1, first_particle=0, lifetime=0, device=-1):
    """is3d_decay_particles_flow: a sampled list decayed on the device with every final particle added to the per-event flow records at
    once -- the records of flow_list on decay_particles' list (species = table entries) with the same slot map.  slot: int32 per table
    entry.  Returns (records dict, stats dict with n_final, n_unbinned and the tallies of decay_particles)."""
    L = load()
    ts, ch, _, keep = _decay_pack(table, chosen_mc_id, dict(pT=[1.0], phi=[0.0], y=[0.0]))
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    slot = _slot_map(table, slot)
    inp = DecayMcInputs(int(seed), int(first_particle), int(lifetime), int(device))
    c = _pack_cuts(cuts)
    r, out = _flow_arrays(n_events, n_slots)
    st, nf, nu = DecayMcStats(), C.c_int64(0), C.c_int64(0)
    L.is3d_decay_particles_flow.argtypes = [C.POINTER(DecayTable), C.c_int32, C.POINTER(C.c_int64), C.POINTER(DecayMcInputs), C.c_int64, C.c_void_p,
                                            C.c_void_p, C.c_int32, C.POINTER(FlowCuts), C.c_int32, C.POINTER(FlowRecords),
                                            C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(DecayMcStats)]
    rc = L.is3d_decay_particles_flow(C.byref(ts), len(ch), ch.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(inp), len(particles),
                                     particles.ctypes.data, slot.ctypes.data, int(n_slots), C.byref(c), int(n_events), C.byref(r), C.byref(nf),
                                     C.byref(nu), C.byref(st))
    return out, _check_decayed(rc, st, nf, nu, records=out)


def decay_particles_flow_diff(table, chosen_mc_id, particles, slot, n_slots, cuts, pT_edges, n_events, seed=1, first_particle=0, lifetime=0,
                              device=-1):
    """is3d_decay_particles_flow_diff: decay_particles_flow with the pT bin as a second key -- the records of flow_diff_list on
    decay_particles' list.  Returns (differential records dict, stats dict with n_final, n_unbinned and the tallies of decay_particles)."""
    L = load()
    ts, ch, _, keep = _decay_pack(table, chosen_mc_id, dict(pT=[1.0], phi=[0.0], y=[0.0]))
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    slot = _slot_map(table, slot)
    inp = DecayMcInputs(int(seed), int(first_particle), int(lifetime), int(device))
    c = _pack_cuts(cuts)
    edges = np.ascontiguousarray(pT_edges, dtype=np.float64)
    r, out = _flow_diff_arrays(n_events, n_slots, len(edges) - 1)
    st, nf, nu = DecayMcStats(), C.c_int64(0), C.c_int64(0)
    L.is3d_decay_particles_flow_diff.argtypes = [C.POINTER(DecayTable), C.c_int32, C.POINTER(C.c_int64), C.POINTER(DecayMcInputs), C.c_int64,
                                                 C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(FlowCuts), C.c_int32, C.c_void_p, C.c_int32,
                                                 C.POINTER(FlowDiffRecords), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(DecayMcStats)]
    rc = L.is3d_decay_particles_flow_diff(C.byref(ts), len(ch), ch.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(inp), len(particles),
                                          particles.ctypes.data, slot.ctypes.data, int(n_slots), C.byref(c), len(edges) - 1, edges.ctypes.data,
                                          int(n_events), C.byref(r), C.byref(nf), C.byref(nu), C.byref(st))
    return out, _check_decayed(rc, st, nf, nu, records=out)


def decay_particles_pairs(table, chosen_mc_id, particles, slot, n_slots, bins, n_events, seed=1, first_particle=0, lifetime=0, device=-1):
    """is3d_decay_particles_pairs: a sampled list decayed on the device with every final particle added to the pair occupancies at once,
    then correlated -- the histograms of pairs_list on decay_particles' list (species = table entries) with the same slot map, bit for bit.
    slot: int32 per table entry.  Returns (hist dict, stats dict with n_final, n_unbinned and the tallies of decay_particles)."""
    L = load()
    ts, ch, _, keep = _decay_pack(table, chosen_mc_id, dict(pT=[1.0], phi=[0.0], y=[0.0]))
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    slot = _slot_map(table, slot)
    inp = DecayMcInputs(int(seed), int(first_particle), int(lifetime), int(device))
    b = _pack_pair_bins(bins)
    h, out = _pair_arrays(b, n_events, n_slots)
    st, nf, nu = DecayMcStats(), C.c_int64(0), C.c_int64(0)
    L.is3d_decay_particles_pairs.argtypes = [C.POINTER(DecayTable), C.c_int32, C.POINTER(C.c_int64), C.POINTER(DecayMcInputs), C.c_int64, C.c_void_p,
                                             C.c_void_p, C.c_int32, C.POINTER(PairBins), C.c_int32, C.POINTER(PairHist),
                                             C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(DecayMcStats)]
    rc = L.is3d_decay_particles_pairs(C.byref(ts), len(ch), ch.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(inp), len(particles),
                                      particles.ctypes.data, slot.ctypes.data, int(n_slots), C.byref(b), int(n_events), C.byref(h), C.byref(nf),
                                      C.byref(nu), C.byref(st))
    return out, _check_decayed(rc, st, nf, nu, hist=out)


def decay_particles_hbt(table, chosen_mc_id, particles, slot, n_slots, bins, n_events, seed=1, first_particle=0, lifetime=0, device=-1):
    """is3d_decay_particles_hbt: a sampled list decayed on the device twice over one stream (count, fill) into compact records of the accepted
    final particles, which are paired -- the histograms of hbt_list on decay_particles' list (species = table entries) with the same slot
    map: den and M equal, num within one unit per pair.  slot: int32 per table entry.  Returns (hist dict, stats dict with n_final,
    n_unbinned and the tallies of decay_particles)."""
    L = load()
    ts, ch, _, keep = _decay_pack(table, chosen_mc_id, dict(pT=[1.0], phi=[0.0], y=[0.0]))
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    slot = _slot_map(table, slot)
    inp = DecayMcInputs(int(seed), int(first_particle), int(lifetime), int(device))
    b = _pack_hbt_bins(bins)
    h, out = _hbt_arrays(b, n_events, n_slots)
    st, nf, nu = DecayMcStats(), C.c_int64(0), C.c_int64(0)
    L.is3d_decay_particles_hbt.argtypes = [C.POINTER(DecayTable), C.c_int32, C.POINTER(C.c_int64), C.POINTER(DecayMcInputs), C.c_int64, C.c_void_p,
                                           C.c_void_p, C.c_int32, C.POINTER(HbtBins), C.c_int32, C.POINTER(HbtHist),
                                           C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(DecayMcStats)]
    rc = L.is3d_decay_particles_hbt(C.byref(ts), len(ch), ch.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(inp), len(particles),
                                    particles.ctypes.data, slot.ctypes.data, int(n_slots), C.byref(b), int(n_events), C.byref(h), C.byref(nf),
                                    C.byref(nu), C.byref(st))
    return out, _check_decayed(rc, st, nf, nu, hist=out)


def shard_bounds(n_cells, rank, n_ranks):
    """is3d_shard_bounds: the contiguous cell shard [lo, hi) of `rank` (what is3d_smooth_spectra_multi uses)."""
    lo, hi = C.c_int64(), C.c_int64()
    _check(load().is3d_shard_bounds(int(n_cells), int(rank), int(n_ranks), C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def smooth_spectra_multi(cells, species, grid, df, opts=None, devices=None, reduce=REDUCE_ORDERED, out=None, fq=None):
    """is3d_smooth_spectra_multi: the host entry with the cells sharded over `devices` (list of HIP ordinals, one shard per
    entry, an ordinal may repeat; None = every visible device).  Returns (dN, aggregate status dict, [per-shard status dicts])."""
    L = load()
    sps, gs, ds, os_, nout, keep = _pack_common(species, grid, df, opts)
    n = len(cells["tau"])
    cs = Cells()
    cs.n_cells = n
    held = []
    for f in CELL_FIELDS:
        a = cells.get(f)
        if a is not None:
            a = _f64(a)
            assert a.shape == (n,), f
            held.append(a)
            setattr(cs, f, a.ctypes.data)
    if out is None:
        out = np.zeros(nout)
    assert out.dtype == np.float64 and out.size == nout and out.flags.c_contiguous
    dv, nd, n_stats = _pack_devices(devices)
    st = Status()
    sst = (Status * n_stats)()
    fqs = _pack_feqmod(fq, keep) if fq is not None else None
    rc = L.is3d_smooth_spectra_multi(C.byref(cs), C.byref(sps), C.byref(gs), C.byref(ds), C.byref(fqs) if fqs is not None else None,
                                     C.byref(os_), dv, nd, int(reduce), _p(out), C.byref(st), sst)
    _check(rc)
    return out, st.as_dict(), [sst[i].as_dict() for i in range(n_stats)]


def smooth_spectra_vah_multi(cells, species, grid, opts=None, devices=None, reduce=REDUCE_ORDERED, out=None, tab=None):
    """is3d_smooth_spectra_vah_multi: smooth_spectra_vah with the cells sharded over `devices` (as smooth_spectra_multi: a list of HIP
    ordinals, one shard per entry, an ordinal may repeat; an int n means the ordinals 0 .. n - 1; None every visible device).  Returns
    (dN, status dict); status["shards"] holds one status dict per shard (bad_cell shard-local there).  An Is3dError raised here carries
    bad_cell (an index of the whole surface) and that status."""
    L = load()
    sps, gs, _, os_, nout, keep = _pack_common(species, grid, _VAH_DUMMY_DF, opts)
    held = []
    if tab is not None:
        cells = {k: v for k, v in cells.items() if k not in ("c0", "c1", "c2", "c3", "c4")}
    cs = _vah_cells_struct(cells, held)
    if out is None:
        out = np.zeros(nout)
    assert out.dtype == np.float64 and out.size == nout and out.flags.c_contiguous
    ts = _pack_vah_tables(tab, keep) if tab is not None else None
    dv, nd, n_stats = _pack_devices(devices)
    st = Status()
    sst = (Status * n_stats)()
    rc = L.is3d_smooth_spectra_vah_multi(C.byref(cs), C.byref(sps), C.byref(gs), C.byref(ts) if ts is not None else None, C.byref(os_),
                                         dv, nd, int(reduce), _p(out), C.byref(st), sst)
    status = st.as_dict()
    status["shards"] = [sst[i].as_dict() for i in range(n_stats)]
    if rc != 0:
        err = Is3dError(rc, L.is3d_last_error().decode(), bad_cell=status["bad_cell"])
        err.status = status
        raise err
    return out, status


class MultiPlan:
    """is3d_multi_plan_*: the persistent form of smooth_spectra_multi -- per-shard plans, workspaces, streams, pinned staging and the
    communicator set are created once; execute(cells) only uploads, runs and sums."""

    def __init__(self, species, grid, df, opts=None, devices=None, reduce=REDUCE_ORDERED, max_cells=1, fq=None):
        L = load()
        sps, gs, ds, os_, self.output_size, self._keep = _pack_common(species, grid, df, opts)
        dv, nd, _ = _pack_devices(devices)
        fqs = _pack_feqmod(fq, self._keep) if fq is not None else None
        self._h = C.c_void_p()
        _check(L.is3d_multi_plan_create(C.byref(self._h), C.byref(sps), C.byref(gs), C.byref(ds), C.byref(fqs) if fqs is not None else None,
                                        C.byref(os_), dv, nd, int(reduce), int(max_cells)))
        self.n_shards = L.is3d_multi_plan_shards(self._h)
        assert L.is3d_multi_plan_output_size(self._h) == self.output_size

    def execute(self, cells, out=None):
        """cells: dict of host numpy arrays.  Returns (dN, aggregate status dict, [per-shard status dicts])."""
        n = len(cells["tau"])
        cs = Cells()
        cs.n_cells = n
        held = []
        for f in CELL_FIELDS:
            a = cells.get(f)
            if a is not None:
                a = _f64(a)
                assert a.shape == (n,), f
                held.append(a)
                setattr(cs, f, a.ctypes.data)
        if out is None:
            out = np.zeros(self.output_size)
        assert out.dtype == np.float64 and out.size == self.output_size and out.flags.c_contiguous
        st = Status()
        sst = (Status * self.n_shards)()
        _check(load().is3d_multi_plan_execute(self._h, C.byref(cs), _p(out), C.byref(st), sst))
        return out, st.as_dict(), [sst[i].as_dict() for i in range(self.n_shards)]

    def close(self):
        if self._h:
            load().is3d_multi_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """is3d_comm: the library's RCCL communicator for one-process-per-GPU hosts.  Rank 0 makes the id (Comm.unique_id()),
    the host ships the 128 bytes to the other ranks, every rank constructs Comm(id, n_ranks, rank, device)."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _check(load().is3d_comm_unique_id(buf))
        return buf.raw

    def __init__(self, uid, n_ranks, rank, device=-1):
        assert len(uid) == COMM_ID_BYTES
        self._h = C.c_void_p()
        _check(load().is3d_comm_create(C.byref(self._h), C.create_string_buffer(uid, COMM_ID_BYTES), int(n_ranks), int(rank), int(device)))
        self.n_ranks, self.rank = int(n_ranks), int(rank)

    def allreduce(self, dev_ptr, n, stream=0):
        _check(load().is3d_comm_allreduce(self._h, C.c_void_p(int(dev_ptr)), int(n), C.c_void_p(int(stream or 0))))

    def rank_seen(self):
        """(rank, n_ranks) as the library's communicator reports them (is3d_comm_rank)."""
        r, n = C.c_int32(-1), C.c_int32(-1)
        _check(load().is3d_comm_rank(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def check(self, stream=0):
        """is3d_comm_check: raises Is3dError(IS3D_EPEER) if a rank's execute had failed before one of the all-reduces since the
        last check (its n_failed attribute says how many); synchronises the stream."""
        k = C.c_int32(0)
        rc = load().is3d_comm_check(self._h, C.c_void_p(int(stream or 0)), C.byref(k))
        if rc != 0:
            e = Is3dError(rc, load().is3d_last_error().decode())
            e.n_failed = k.value
            raise e

    def abort(self):
        _check(load().is3d_comm_abort(self._h))

    def set_timeout(self, seconds):
        """Deadline of the library's host-side waits behind this communicator's collectives (is3d_comm_set_timeout)."""
        L = load()
        L.is3d_comm_set_timeout.argtypes = [C.c_void_p, C.c_double]
        _check(L.is3d_comm_set_timeout(self._h, float(seconds)))

    def synchronize(self, stream=0):
        """hipStreamSynchronize with that deadline (is3d_comm_synchronize): raises Is3dError(IS3D_ENODEVICE) instead of blocking for ever
        behind a collective a peer never joined."""
        _check(load().is3d_comm_synchronize(self._h, C.c_void_p(int(stream or 0))))

    def allreduce_ms(self):
        """Device time of the last collective on this rank (is3d_comm_timings)."""
        ms = C.c_double(0.0)
        _check(load().is3d_comm_timings(self._h, C.byref(ms)))
        return ms.value

    def close(self):
        if self._h:
            load().is3d_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


MATH_FUNCS = dict(exp_full=0, exp_p9=1, exp_p9_sat=2, exp_full_sat=3, sqrt_g1=4, sqrt_nr=5, rcp_nr1=6, rcp_nr=7, exp_p9_x32=8,
                  add_clamp01=9, fma_clamp01=10, fma_clamp01_half=11, exp_p9_scaled=12, rcp_batch2=13, rcp_batch3=14, rcp_batch4=15, rcp_batch8=16)
# functions of several arguments: doubles per record (is3d_amd.h); the others take one
MATH_ARITY = dict(add_clamp01=2, fma_clamp01=3, fma_clamp01_half=2, exp_p9_scaled=2, rcp_batch2=2, rcp_batch3=3, rcp_batch4=4, rcp_batch8=8)


def resource_counters():
    """is3d_resource_counters: (plans created, device allocations made) by the library in this process so far."""
    L = load()
    a, b = C.c_int64(0), C.c_int64(0)
    L.is3d_resource_counters.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    _check(L.is3d_resource_counters(C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


def math_probe(which, x, device=-1):
    """is3d_math_probe: the device's elementary function `which` (a key of MATH_FUNCS) at the host array x.  A function of several arguments
    (MATH_ARITY) takes x as [records][arity] and returns [records] -- the rcp_batch functions [records][arity], one quotient per slot."""
    xs = _f64(x)
    y = np.zeros_like(xs)
    L = load()
    L.is3d_math_probe.argtypes = [C.c_int32, C.c_int64, _dp, _dp, C.c_int32]
    _check(L.is3d_math_probe(MATH_FUNCS[which], xs.size, _p(xs), _p(y), int(device)))
    arity = MATH_ARITY.get(which, 1)
    if arity > 1:
        y = y.reshape(-1, arity)
        if not which.startswith("rcp_batch"):
            y = np.ascontiguousarray(y[:, 0])
    return y


def probe_shader_clock(seconds=0.3, device=0):
    """Shader clock in GHz averaged over `seconds`, sampled by idle waves on a private stream (0.0: the device's two counters
    tick at the same rate, nothing to measure).  Call it from a second thread while a kernel runs to price that kernel."""
    ghz = C.c_double(0.0)
    _check(load().is3d_probe_shader_clock(int(device), float(seconds), C.byref(ghz)))
    return ghz.value


class Plan:
    """Device-resident plan (is3d_plan_*).  Cell arrays and the output are device pointers (ints),
    e.g. torch tensors' data_ptr(); `stream` is a hipStream_t handle (torch.cuda.current_stream().cuda_stream)."""

    def __init__(self, species, grid, df, opts=None, max_cells=1, fq=None):
        L = load()
        sps, gs, ds, os_, nout, keep = _pack_common(species, grid, df, opts)
        self._h = C.c_void_p()
        if fq is not None:
            fqs = _pack_feqmod(fq, keep)
            _check(L.is3d_plan_create_feqmod(C.byref(self._h), C.byref(sps), C.byref(gs), C.byref(ds), C.byref(fqs), C.byref(os_), int(max_cells)))
        self.feqmod = fq is not None
        if fq is None:
            _check(L.is3d_plan_create(C.byref(self._h), C.byref(sps), C.byref(gs), C.byref(ds), C.byref(os_), int(max_cells)))
        self.output_size = int(L.is3d_plan_output_size(self._h))
        assert self.output_size == nout
        self.workspace_bytes = int(L.is3d_plan_workspace_bytes(self._h))
        self.main_kernel_name = L.is3d_plan_main_kernel_name(self._h).decode()
        jt, r = C.c_int32(), C.c_int32()
        _check(L.is3d_plan_tile_shape(self._h, C.byref(jt), C.byref(r)))
        self.tile_shape = (jt.value, r.value)

    def set_timing(self, enable=True):
        _check(load().is3d_plan_set_timing(self._h, 1 if enable else 0))

    def execute(self, n_cells, cell_ptrs, out_ptr, stream=0, want_status=True):
        """cell_ptrs: dict field -> device pointer (int)."""
        cs = Cells()
        cs.n_cells = int(n_cells)
        for f in CELL_FIELDS:
            p = cell_ptrs.get(f)
            if p:
                setattr(cs, f, int(p))
        st = Status()
        rc = load().is3d_plan_execute(self._h, C.byref(cs), C.c_void_p(int(out_ptr)), C.c_void_p(int(stream or 0)),
                                      C.byref(st) if want_status else None)
        _check(rc)
        return st.as_dict() if want_status else None

    def execute_allreduce(self, n_cells, cell_ptrs, out_ptr, comm=None, stream=0, want_status=True):
        """is3d_plan_execute_allreduce: execute on this rank's shard, then the RCCL all-reduce of the spectrum over `comm`
        (a Comm, or None for a single rank) on the same stream."""
        cs = Cells()
        cs.n_cells = int(n_cells)
        for f in CELL_FIELDS:
            p = cell_ptrs.get(f)
            if p:
                setattr(cs, f, int(p))
        st = Status()
        rc = load().is3d_plan_execute_allreduce(self._h, C.byref(cs), C.c_void_p(int(out_ptr)), comm._h if comm is not None else None,
                                                C.c_void_p(int(stream or 0)), C.byref(st) if want_status else None)
        _check(rc)
        return st.as_dict() if want_status else None

    def observables(self, dN_ptr, pT_w, phi_w, dndy_ptr=0, spec2pi_ptr=0, vn_ptr=0, stream=0):
        """is3d_plan_observables: device pointers (ints) in and out, host weight arrays."""
        pw, fw = _f64(pT_w), _f64(phi_w)
        _check(load().is3d_plan_observables(self._h, C.c_void_p(int(dN_ptr)), _p(pw), _p(fw), C.c_void_p(int(dndy_ptr or 0)),
                                            C.c_void_p(int(spec2pi_ptr or 0)), C.c_void_p(int(vn_ptr or 0)), C.c_void_p(int(stream or 0))))

    def execute_spacetime(self, n_cells, cell_ptrs, x_ptr, y_ptr, pT_w, phi_w, bins, out_ptrs, stream=0, want_stats=True):
        """is3d_plan_execute_spacetime (operation 0): cell_ptrs, x_ptr, y_ptr and out_ptrs (dict name -> device pointer, SPACETIME_OUTPUTS;
        dN_dy_cell optional) are device pointers, pT_w / phi_w host weight arrays.  On a plan made with fq (df_mode 3, 4):
        is3d_plan_execute_spacetime_feqmod, whose counters come back under "feqmod" in the stats dict."""
        cs = Cells()
        cs.n_cells = int(n_cells)
        for f in CELL_FIELDS:
            p = cell_ptrs.get(f)
            if p:
                setattr(cs, f, int(p))
        pw, fw = _f64(pT_w), _f64(phi_w)
        so = SpacetimeOut(*[int(out_ptrs[k]) if out_ptrs.get(k) else None for k in SPACETIME_OUTPUTS])
        b = _spacetime_bins(bins)
        st = SpacetimeStats()
        if self.feqmod:
            fst = SpacetimeFeqmodStats()
            rc = load().is3d_plan_execute_spacetime_feqmod(self._h, C.byref(cs), C.c_void_p(int(x_ptr or 0)), C.c_void_p(int(y_ptr or 0)), _p(pw),
                                                           _p(fw), C.byref(b), C.byref(so), C.c_void_p(int(stream or 0)),
                                                           C.byref(st) if want_stats else None, C.byref(fst) if want_stats else None)
            _check(rc)
            return dict(st.as_dict(), feqmod=fst.as_dict()) if want_stats else None
        rc = load().is3d_plan_execute_spacetime(self._h, C.byref(cs), C.c_void_p(int(x_ptr or 0)), C.c_void_p(int(y_ptr or 0)), _p(pw), _p(fw),
                                                C.byref(b), C.byref(so), C.c_void_p(int(stream or 0)), C.byref(st) if want_stats else None)
        _check(rc)
        return st.as_dict() if want_stats else None

    def check(self, stream=0):
        """is3d_plan_check: raises Is3dError(IS3D_EDOMAIN) if an execute since the last check (status-less ones included) met a
        cell outside the coefficient table; synchronises the stream."""
        bad = C.c_int64(-1)
        rc = load().is3d_plan_check(self._h, C.c_void_p(int(stream or 0)), C.byref(bad))
        if rc != 0:
            raise Is3dError(rc, load().is3d_last_error().decode(), bad_cell=bad.value)

    def timings(self):
        st = Status()
        _check(load().is3d_plan_timings(self._h, C.byref(st)))
        return st.as_dict()

    def close(self):
        if self._h:
            load().is3d_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- host I/O wrappers -------------------------------------------------------------------------
def param_get(path, name):
    v = C.c_double()
    _check(load().is3d_param_get(path.encode(), name.encode(), C.byref(v)))
    return v.value


def table_read(path):
    L = load()
    rows, cols = C.c_int64(), C.c_int32()
    _check(L.is3d_table_read(path.encode(), C.byref(rows), C.byref(cols), None, 0))
    data = np.zeros((rows.value, cols.value))
    _check(L.is3d_table_read(path.encode(), C.byref(rows), C.byref(cols), _p(data), data.size))
    return data


def surface_read_vh(path, include_baryon=0, include_baryondiff_deltaf=0, dimension=3):
    L = load()
    n = C.c_int64(0)
    _check(L.is3d_surface_read_vh(path.encode(), include_baryon, include_baryondiff_deltaf, dimension, C.byref(n), None, None))
    arrs = {f: np.zeros(n.value) for f in SURFACE_READ_ORDER}
    ptrs = (_dp * 23)(*[_p(arrs[f]) for f in SURFACE_READ_ORDER])
    avg = np.zeros(5)
    if n.value > 0:
        _check(L.is3d_surface_read_vh(path.encode(), include_baryon, include_baryondiff_deltaf, dimension, C.byref(n), ptrs, _p(avg)))
    return arrs, avg


def surface_read(path, mode, include_baryon=0, include_baryondiff_deltaf=0, dimension=3):
    """is3d_surface_read: modes 0, 1, 4, 5, 6, 7 -> (dict of the 23 arrays, averages)."""
    L = load()
    n = C.c_int64(0)
    _check(L.is3d_surface_read(path.encode(), mode, include_baryon, include_baryondiff_deltaf, dimension, C.byref(n), None, None))
    arrs = {f: np.zeros(n.value) for f in SURFACE_READ_ORDER}
    ptrs = (_dp * 23)(*[_p(arrs[f]) for f in SURFACE_READ_ORDER])
    avg = np.zeros(5)
    if n.value > 0:
        _check(L.is3d_surface_read(path.encode(), mode, include_baryon, include_baryondiff_deltaf, dimension, C.byref(n), ptrs, _p(avg)))
    return arrs, avg


def surface_open(path, mode=1, include_baryon=0, include_baryondiff_deltaf=0, dimension=3, cache=1):
    """is3d_surface_open / _arrays / _source / _close: one read and one parse of the text, or the binary sidecar `<path>.is3dcache` when it
    matches -> (dict of arrays [copies], averages or None, source) with source 0 text parsed | 1 text parsed + sidecar written | 2 sidecar.
    Modes 0, 1, 4, 5, 6, 7: the 23 arrays of SURFACE_READ_ORDER (absent ones None) + x, y; mode 2: the 32 arrays of VAH_SURFACE_ORDER."""
    L = load()
    L.is3d_surface_open.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.is3d_surface_cells.argtypes = [C.c_void_p]
    L.is3d_surface_cells.restype = C.c_int64
    L.is3d_surface_source.argtypes = [C.c_void_p]
    L.is3d_surface_arrays.argtypes = [C.c_void_p, C.POINTER(_dp), C.c_int32, _dp]
    L.is3d_surface_close.argtypes = [C.c_void_p]
    L.is3d_surface_close.restype = None
    h = C.c_void_p()
    _check(L.is3d_surface_open(path.encode(), int(mode), int(include_baryon), int(include_baryondiff_deltaf), int(dimension), int(cache), C.byref(h)))
    try:
        n = L.is3d_surface_cells(h)
        names = list(VAH_SURFACE_ORDER) if mode == 2 else list(SURFACE_READ_ORDER) + ["x", "y"]
        ptrs = (_dp * len(names))()
        avg = np.zeros(5)
        _check(L.is3d_surface_arrays(h, ptrs, len(names), _p(avg)))
        if n > 0:
            arrs = {f: (np.ctypeslib.as_array(ptrs[i], shape=(n,)).copy() if ptrs[i] else None) for i, f in enumerate(names)}
        else:
            arrs = {f: np.zeros(0) for f in names}
        L.is3d_surface_from_sidecar.argtypes = [C.c_void_p]
        early = L.is3d_surface_from_sidecar(h)                 # known at open, never waits for the writer
        source = L.is3d_surface_source(h)
        assert early == (1 if source == 2 else 0)
    finally:
        L.is3d_surface_close(h)
    return arrs, (None if mode == 2 else avg), source


def surface_vorticity(path, include_baryon=0, include_baryondiff_deltaf=0, dimension=3, cache=1):
    """is3d_surface_open (mode 5) + is3d_surface_vorticity: the six thermal-vorticity arrays of a mode-5 surface (copies), dict
    VORTICITY_FIELDS -> array, and the source (0 text parsed | 1 text parsed + sidecar written | 2 sidecar)."""
    L = load()
    L.is3d_surface_open.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.is3d_surface_cells.argtypes = [C.c_void_p]
    L.is3d_surface_cells.restype = C.c_int64
    L.is3d_surface_source.argtypes = [C.c_void_p]
    L.is3d_surface_close.argtypes = [C.c_void_p]
    L.is3d_surface_close.restype = None
    h = C.c_void_p()
    _check(L.is3d_surface_open(path.encode(), 5, int(include_baryon), int(include_baryondiff_deltaf), int(dimension), int(cache), C.byref(h)))
    try:
        n = L.is3d_surface_cells(h)
        ptrs = (_dp * 6)()
        _check(L.is3d_surface_vorticity(h, ptrs))
        w = {f: (np.ctypeslib.as_array(ptrs[i], shape=(n,)).copy() if n > 0 else np.zeros(0)) for i, f in enumerate(VORTICITY_FIELDS)}
        source = L.is3d_surface_source(h)
    finally:
        L.is3d_surface_close(h)
    return w, source


def pdg_read(path, box=False):
    """is3d_pdg_read (hrg_eos 1, 2: the conventional token-stream files) | box = True: is3d_pdg_read_box (hrg_eos 3: PDG/pdg_box.dat)."""
    L = load()
    f = L.is3d_pdg_read_box if box else L.is3d_pdg_read
    n = C.c_int32(0)
    _check(f(path.encode(), C.byref(n), None, None, None, None, None, 0))
    ids = np.zeros(n.value, dtype=np.int64)
    mass, gspin, baryon, sign = (np.zeros(n.value) for _ in range(4))
    _check(f(path.encode(), C.byref(n), ids.ctypes.data_as(C.POINTER(C.c_int64)), _p(mass), _p(gspin), _p(baryon), _p(sign), n.value))
    return dict(mc_id=ids, mass=mass, gspin=gspin, baryon=baryon, sign=sign)


def df_table_read(path):
    L = load()
    n = C.c_int32(0)
    _check(L.is3d_df_table_read(path.encode(), C.byref(n), None, None, 0))
    T, v = np.zeros(n.value), np.zeros(n.value)
    _check(L.is3d_df_table_read(path.encode(), C.byref(n), _p(T), _p(v), n.value))
    return T, v


def df_table_read_full(path):
    L = load()
    nT, nB = C.c_int32(0), C.c_int32(0)
    _check(L.is3d_df_table_read_full(path.encode(), C.byref(nT), C.byref(nB), None, None, None, 0))
    T, B, v = np.zeros(nT.value), np.zeros(nB.value), np.zeros((nB.value, nT.value))
    _check(L.is3d_df_table_read_full(path.encode(), C.byref(nT), C.byref(nB), _p(T), _p(B), _p(v), v.size))
    return T, B, v


def df_generate(pdg, root, weight, T, muB, device=-1, with_integrals=False):
    """is3d_df_generate: the ten coefficient tables of deltaf_coefficients/vh/<list>/ for the hadron list `pdg` (as pdg_read returns it) on the
    (T, muB) grid, computed on the device.  root, weight: the Gauss-Laguerre arrays as gla_read returns them (row alpha; rows 1..4 are used).
    Returns (tables [10][n_muB][n_T] in the order of DF_NAMES_2D, integrals [20][n_muB][n_T] in the order of DFGEN_INTEGRALS or None, stats)."""
    L = load()
    cols = [_f64(pdg[k]) for k in ("mass", "gspin", "baryon", "sign")]
    n = len(cols[0])
    if any(len(c) != n for c in cols):
        raise ValueError("the hadron list's arrays differ in length")
    root, weight = np.asarray(root, dtype=np.float64), np.asarray(weight, dtype=np.float64)
    if root.ndim != 2 or root.shape != weight.shape or root.shape[0] < 5:
        raise ValueError("root and weight must be [n_alpha >= 5][n_points] (alpha = 1..4 are used)")
    rows = [_f64(root[a]) for a in range(1, 5)] + [_f64(weight[a]) for a in range(1, 5)]
    r4, w4 = (_dp * 4)(*[_p(a) for a in rows[:4]]), (_dp * 4)(*[_p(a) for a in rows[4:]])
    T, muB = _f64(np.atleast_1d(T)), _f64(np.atleast_1d(muB))
    hl = HadronList(n, *[_p(c) for c in cols])
    tables = np.zeros((10, len(muB), len(T)))
    integrals = np.zeros((20, len(muB), len(T))) if with_integrals else None
    st = DfgenStats()
    _check(L.is3d_df_generate(C.byref(hl), root.shape[1], r4, w4, len(T), _p(T), len(muB), _p(muB), device, _p(tables),
                              _p(integrals) if with_integrals else None, C.byref(st)))
    return tables, integrals, dict(ms_kernel=st.ms_kernel, ms_h2d=st.ms_h2d, ms_d2h=st.ms_d2h, n_massive=st.n_massive)


def df_tables_write(directory, T, muB, tables):
    """is3d_df_tables_write: the ten files of a coefficient directory in the generator's format; refuses to overwrite an existing c0.dat."""
    T, muB, tables = _f64(np.atleast_1d(T)), _f64(np.atleast_1d(muB)), _f64(tables)
    if tables.shape != (10, len(muB), len(T)):
        raise ValueError("tables must be [10][n_muB][n_T]")
    _check(load().is3d_df_tables_write(str(directory).encode(), len(T), _p(T), len(muB), _p(muB), _p(tables)))


def _pack_sampler(cells, species, df, gla, opts, n_events, seed, y_cut, first_cell, fq, fast, T_avg, T_avg_switch, batch_events, muB_avg):
    """The C structs of the host-pointer sampler entries: (Cells, Species, DfTables, SamplerInputs, Options, what must stay alive)."""
    grid_dummy = dict(pT=[1.0], phi=[0.0], y=[0.0], eta=[0.0], eta_w=[1.0])
    sps, _, ds, os_, _, keep = _pack_common(species, grid_dummy, df, opts)
    n = len(cells["tau"])
    cs = Cells()
    cs.n_cells = n
    held = [keep]
    for f in CELL_FIELDS:
        a = cells.get(f)
        if a is not None:
            a = _f64(a)
            assert a.shape == (n,), f
            held.append(a)
            setattr(cs, f, a.ctypes.data)
    si = _sampler_inputs(cells, gla, n_events, seed, y_cut, first_cell, fq, fast, batch_events, held, T_avg, T_avg_switch, muB_avg)
    return cs, sps, ds, si, os_, held


def _sampler_inputs(cells, gla, n_events, seed, y_cut, first_cell, fq, fast, batch_events, held, T_avg=0.0, T_avg_switch=0.0, muB_avg=0.0):
    """SamplerInputs for both sampler families (anisotropic hydro has no averages: 0.0).  held: what must stay alive, appended to; held[0] is
    the list _pack_common keeps."""
    r1, w1 = _f64(gla["root1"]), _f64(gla["weight1"])
    xs = _f64(cells["x"]) if cells.get("x") is not None else None
    ys = _f64(cells["y"]) if cells.get("y") is not None else None
    fqs = _pack_feqmod(fq, held[0]) if fq is not None else None
    held += [r1, w1, xs, ys, fqs]
    return SamplerInputs(int(n_events), len(r1), int(seed), float(y_cut), int(first_cell), _p(xs) if xs is not None else None,
                         _p(ys) if ys is not None else None, _p(r1), _p(w1), C.pointer(fqs) if fqs is not None else None, int(fast), int(batch_events),
                         float(T_avg), float(T_avg_switch), float(muB_avg))


# the host-pointer sampler entries, each with a _multi form: name -> (family, kind); load() builds their argtypes from this
SAMPLER_ENTRIES = dict(is3d_sample_particles=("viscous", "list"), is3d_sample_binned=("viscous", "binned"), is3d_sample_fused=("viscous", "binned"),
                       is3d_sample_particles_vah=("vah", "list"), is3d_sample_binned_vah=("vah", "binned"))


def _sampler_call(name, head, devices, edomain_keeps_rest, *tail):
    """One call of the entry `name` (devices = None) or of name_multi (one cell shard per listed device; an ordinal may repeat).  An error
    raises; with edomain_keeps_rest IS3D_EDOMAIN, which comes with the other cells' result, is returned instead."""
    if devices is None:
        rc = getattr(load(), name)(*head, *tail)
    else:
        dv, nd, _ = _pack_devices(devices)
        rc = getattr(load(), name + "_multi")(*head, dv, nd, *tail)
    if not (edomain_keeps_rest and rc == IS3D_EDOMAIN):
        _check(rc)
    return rc


def _sampler_result(rc, st, cnt, **result):
    """(result, stats dict with n_particles) of a sampler call; rc = IS3D_EDOMAIN, bad cells: Is3dError with .bad_cell (the index the text
    names), .stats and the partial result under its keyword."""
    (key, value), = result.items()
    d = st.as_dict()
    d["n_particles"] = int(cnt.value)
    if rc:
        msg = load().is3d_last_error().decode()
        m = re.search(r"cell (\d+):", msg)
        e = Is3dError(rc, msg, bad_cell=int(m.group(1)) if m else None)
        setattr(e, key, value)
        e.stats = d
        raise e
    return value, d


def _sample_list(name, head, devices, capacity, edomain_keeps_rest):
    """The list entries' protocol: capacity = None sizes the buffer from a count-only first call; -> (the list, stats dict).
    edomain_keeps_rest: IS3D_EDOMAIN carries the other cells' hadrons (.particles, .stats)."""
    st, cnt = SamplerStats(), C.c_int64(0)
    if capacity is None:
        _sampler_call(name, head, devices, edomain_keeps_rest, None, 0, C.byref(cnt), C.byref(st))
        capacity = int(cnt.value)
    out = np.zeros(max(int(capacity), 1), dtype=PARTICLE_DTYPE)
    assert out.dtype.itemsize == C.sizeof(Particle)
    rc = _sampler_call(name, head, devices, edomain_keeps_rest, out.ctypes.data, int(capacity), C.byref(cnt), C.byref(st))
    return _sampler_result(rc, st, cnt, particles=out[:min(int(cnt.value), int(capacity))])


def _sample_binned(name, head, devices, bins, n_events, n_species, edomain_keeps_rest):
    """The binned entries: -> (dict of int64 histograms, stats dict).  edomain_keeps_rest: IS3D_EDOMAIN carries the other cells' histograms
    (.hist, .stats)."""
    b = _pack_bins(bins)
    h, out = _hist_arrays(bins, n_events, n_species)
    st, cnt = SamplerStats(), C.c_int64(0)
    rc = _sampler_call(name, head, devices, edomain_keeps_rest, C.byref(b), C.byref(h), C.byref(cnt), C.byref(st))
    return _sampler_result(rc, st, cnt, hist=out)


def sample_particles(cells, species, df, gla, opts=None, n_events=1, seed=1, y_cut=0.5, first_cell=0, capacity=None, fq=None, fast=0,
                     T_avg=0.0, T_avg_switch=0.0, batch_events=0, muB_avg=0.0, devices=None):
    """is3d_sample_particles (the drop-in for sample_dN_pTdpTdphidy, df_mode 1-4).  cells: dict of host arrays (x, y optional);
    gla: dict with root1, weight1; fq: the feqmod tables (df_mode 3, 4; fast mode with df_mode 2).  Returns (numpy structured array of PARTICLE_DTYPE, stats dict); capacity = None sizes the
    buffer from a count-only first call.  devices: is3d_sample_particles_multi, one cell shard per listed device (an ordinal may repeat)."""
    cs, sps, ds, si, os_, _held = _pack_sampler(cells, species, df, gla, opts, n_events, seed, y_cut, first_cell, fq, fast, T_avg, T_avg_switch,
                                                batch_events, muB_avg)
    return _sample_list("is3d_sample_particles", (C.byref(cs), C.byref(sps), C.byref(ds), C.byref(si), C.byref(os_)), devices, capacity, False)


def _pack_sampler_vah(cells, species, gla, opts, tab, n_events, seed, y_cut, first_cell, batch_events, fast, fq):
    """The arguments the anisotropic-hydro sampler entries share: (VahCells, Species, tables pointer | None, SamplerInputs, Options, held)."""
    sps, _, _, os_, _, keep = _pack_common(species, dict(pT=[1.0], phi=[0.0], y=[0.0], eta=[0.0], eta_w=[1.0]), _VAH_DUMMY_DF, opts)
    held = [keep]
    if tab is not None:
        cells = {k: v for k, v in cells.items() if k not in ("c0", "c1", "c2", "c3", "c4")}
    cs = _vah_cells_struct(cells, held)
    ts = _pack_vah_tables(tab, keep) if tab is not None else None
    held.append(ts)
    si = _sampler_inputs(cells, gla, n_events, seed, y_cut, first_cell, fq, fast, batch_events, held)
    return cs, sps, (C.byref(ts) if ts is not None else None), si, os_, held


def sample_particles_vah(cells, species, gla, opts=None, tab=None, n_events=1, seed=1, y_cut=0.5, first_cell=0, capacity=None, batch_events=0,
                         devices=None, fast=0, fq=None):
    """is3d_sample_particles_vah: the particle sampler for anisotropic hydro (mode 2, operation 2).  cells: dict of host arrays per VAH_FIELDS
    (x, y optional); gla: dict with root1, weight1; tab (dict L, aL, c0..c4): the coefficients come from the (Lambda, alpha_L) tables and the
    cells' c0..c4 are ignored.  devices: is3d_sample_particles_vah_multi, one cell shard per listed device (an ordinal may repeat).  Returns
    (numpy structured array of PARTICLE_DTYPE, stats dict); capacity = None sizes the buffer from a count-only first call.  A bad cell raises
    Is3dError(IS3D_EDOMAIN) with .bad_cell (the lowest global index), .particles and .stats: the other cells are sampled all the same.
    fast, fq: passed on only so that the entry's refusals can be reached."""
    cs, sps, tp, si, os_, _held = _pack_sampler_vah(cells, species, gla, opts, tab, n_events, seed, y_cut, first_cell, batch_events, fast, fq)
    return _sample_list("is3d_sample_particles_vah", (C.byref(cs), C.byref(sps), tp, C.byref(si), C.byref(os_)), devices, capacity, True)


def sample_particles_vah_multi(cells, species, gla, opts=None, devices=(0,), **kw):
    """is3d_sample_particles_vah_multi: one cell shard per entry of devices (an ordinal may repeat); the list equals sample_particles_vah's."""
    return sample_particles_vah(cells, species, gla, opts, devices=list(devices), **kw)


class SamplerPlan:
    """is3d_sampler_plan_*: the device-resident, persistent form of is3d_sample_particles.  Tables, species classes and (after the first
    execute of a shape) the workspaces live on the device; execute takes DEVICE pointers for the cell arrays (dict field -> int), an optional
    DEVICE particle buffer (PARTICLE_DTYPE entries) and returns (n_particles, stats).  The list is the one is3d_sample_particles gives."""

    def __init__(self, species, df, gla, opts=None, max_cells=1, fq=None, fast=0, T_avg=0.0, T_avg_switch=0.0, muB_avg=0.0, y_cut=0.5):
        L = load()
        grid_dummy = dict(pT=[1.0], phi=[0.0], y=[0.0], eta=[0.0], eta_w=[1.0])
        sps, _, ds, os_, _, self._keep = _pack_common(species, grid_dummy, df, opts)
        r1, w1 = _f64(gla["root1"]), _f64(gla["weight1"])
        fqs = _pack_feqmod(fq, self._keep) if fq is not None else None
        si = SamplerInputs(1, len(r1), 0, float(y_cut), 0, None, None, _p(r1), _p(w1), C.pointer(fqs) if fqs is not None else None, int(fast), 0,
                           float(T_avg), float(T_avg_switch), float(muB_avg))
        L.is3d_sampler_plan_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(Species), C.POINTER(DfTables), C.POINTER(SamplerInputs), C.POINTER(Options), C.c_int64]
        L.is3d_sampler_plan_execute.argtypes = [C.c_void_p, C.POINTER(Cells), C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, C.c_void_p,
                                                C.c_int64, C.POINTER(C.c_int64), C.POINTER(SamplerStats)]
        L.is3d_sampler_plan_destroy.argtypes = [C.c_void_p]
        L.is3d_sampler_plan_destroy.restype = None
        self._h = C.c_void_p()
        _check(L.is3d_sampler_plan_create(C.byref(self._h), C.byref(sps), C.byref(ds), C.byref(si), C.byref(os_), int(max_cells)))

    def execute(self, n_cells, dev_ptrs, n_events, seed, particles_ptr=0, capacity=0, x_ptr=0, y_ptr=0, first_cell=0, batch_events=0):
        cs = Cells()
        cs.n_cells = int(n_cells)
        for f in CELL_FIELDS:
            if dev_ptrs.get(f):
                setattr(cs, f, int(dev_ptrs[f]))
        cnt, st = C.c_int64(0), SamplerStats()
        rc = load().is3d_sampler_plan_execute(self._h, C.byref(cs), C.c_void_p(int(x_ptr) or None), C.c_void_p(int(y_ptr) or None), int(n_events), int(seed),
                                              int(first_cell), int(batch_events), C.c_void_p(int(particles_ptr) or None), int(capacity), C.byref(cnt), C.byref(st))
        _check(rc)
        d = st.as_dict()
        d["n_particles"] = int(cnt.value)
        return int(cnt.value), d

    def execute_binned(self, n_cells, dev_ptrs, n_events, seed, bins, n_species, x_ptr=0, y_ptr=0, first_cell=0, batch_events=0, _fused=False):
        """is3d_sampler_plan_execute_binned: -> (dict of int64 histograms, stats); n_species: the length of the plan's species list."""
        cs = Cells()
        cs.n_cells = int(n_cells)
        for f in CELL_FIELDS:
            if dev_ptrs.get(f):
                setattr(cs, f, int(dev_ptrs[f]))
        b = _pack_bins(bins)
        h, out = _hist_arrays(bins, n_events, n_species)
        cnt, st = C.c_int64(0), SamplerStats()
        L = load()
        fn = L.is3d_sampler_plan_execute_fused if _fused else L.is3d_sampler_plan_execute_binned
        fn.argtypes = [C.c_void_p, C.POINTER(Cells), C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int64, C.c_int32,
                       C.POINTER(SamplerTestBins), C.POINTER(SamplerHist), C.POINTER(C.c_int64), C.POINTER(SamplerStats)]
        _check(fn(self._h, C.byref(cs), C.c_void_p(int(x_ptr) or None), C.c_void_p(int(y_ptr) or None), int(n_events),
                  int(seed), int(first_cell), int(batch_events), C.byref(b), C.byref(h), C.byref(cnt), C.byref(st)))
        d = st.as_dict()
        d["n_particles"] = int(cnt.value)
        return out, d

    def execute_decayed_binned(self, n_cells, dev_ptrs, n_events, seed, bins, n_species, table, slot, n_slots, decay_seed=None, lifetime=0,
                               x_ptr=0, y_ptr=0, first_cell=0, batch_events=0):
        """is3d_sampler_plan_execute_decayed_binned: execute_binned with every event batch also decayed (table: a DecayMcTable on the plan's
        device, created for the plan's species list) and its final particles binned by slot.  decay_seed = None: the sampler's seed.
        -> (thermal histograms, decayed histograms of n_slots species, sampler stats, decay stats with n_final and n_unbinned)."""
        cs = Cells()
        cs.n_cells = int(n_cells)
        for f in CELL_FIELDS:
            if dev_ptrs.get(f):
                setattr(cs, f, int(dev_ptrs[f]))
        b = _pack_bins(bins)
        h, out = _hist_arrays(bins, n_events, n_species)
        hd, outd = _hist_arrays(bins, n_events, n_slots)
        slot = _slot_map(table.table, slot)
        cnt, st, dst, nf, nu = C.c_int64(0), SamplerStats(), DecayMcStats(), C.c_int64(0), C.c_int64(0)
        fn = load().is3d_sampler_plan_execute_decayed_binned
        fn.argtypes = [C.c_void_p, C.POINTER(Cells), C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int64, C.c_int32,
                       C.POINTER(SamplerTestBins), C.POINTER(SamplerHist), C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int32,
                       C.POINTER(SamplerHist), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(SamplerStats),
                       C.POINTER(DecayMcStats)]
        rc = fn(self._h, C.byref(cs), C.c_void_p(int(x_ptr) or None), C.c_void_p(int(y_ptr) or None), int(n_events), int(seed), int(first_cell),
                int(batch_events), C.byref(b), C.byref(h), table._h, slot.ctypes.data, int(n_slots), int(seed if decay_seed is None else decay_seed),
                int(lifetime), C.byref(hd), C.byref(cnt), C.byref(nf), C.byref(nu), C.byref(st), C.byref(dst))
        d = st.as_dict()
        d["n_particles"] = int(cnt.value)
        dd = _check_decayed(rc, dst, nf, nu, hist=out, hist_decayed=outd, sampler_stats=d)
        return out, outd, d, dd

    def execute_flow(self, n_cells, dev_ptrs, n_events, seed, cuts, slot, n_slots, table=None, slot_decayed=None, n_slots_decayed=0,
                     decay_seed=None, lifetime=0, x_ptr=0, y_ptr=0, first_cell=0, batch_events=0):
        """is3d_sampler_plan_execute_flow: the per-event flow records of the list execute returns (slot: int32 per species of the plan) and,
        with table (a DecayMcTable on the plan's device), of its Monte Carlo decay products (slot_decayed: int32 per table entry).
        -> (records, sampler stats) | (records, decayed records, sampler stats, decay stats with n_final and n_unbinned)."""
        cs = Cells()
        cs.n_cells = int(n_cells)
        for f in CELL_FIELDS:
            if dev_ptrs.get(f):
                setattr(cs, f, int(dev_ptrs[f]))
        c = _pack_cuts(cuts)
        slot = np.ascontiguousarray(slot, dtype=np.int32)
        r, out = _flow_arrays(n_events, n_slots)
        rd, outd = _flow_arrays(n_events, n_slots_decayed if table is not None else 0)
        sd = _slot_map(table.table, slot_decayed) if table is not None else None
        cnt, st, dst, nf, nu = C.c_int64(0), SamplerStats(), DecayMcStats(), C.c_int64(0), C.c_int64(0)
        fn = load().is3d_sampler_plan_execute_flow
        fn.argtypes = [C.c_void_p, C.POINTER(Cells), C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, C.POINTER(FlowCuts),
                       C.c_void_p, C.c_int32, C.POINTER(FlowRecords), C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int32,
                       C.POINTER(FlowRecords), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(SamplerStats),
                       C.POINTER(DecayMcStats)]
        rc = fn(self._h, C.byref(cs), C.c_void_p(int(x_ptr) or None), C.c_void_p(int(y_ptr) or None), int(n_events), int(seed), int(first_cell),
                int(batch_events), C.byref(c), slot.ctypes.data, int(n_slots), C.byref(r), table._h if table is not None else None,
                sd.ctypes.data if sd is not None else None, int(n_slots_decayed), int(seed if decay_seed is None else decay_seed), int(lifetime),
                C.byref(rd) if table is not None else None, C.byref(cnt), C.byref(nf), C.byref(nu), C.byref(st), C.byref(dst))
        d = st.as_dict()
        d["n_particles"] = int(cnt.value)
        if table is None:
            _check(rc)
            return out, d
        dd = _check_decayed(rc, dst, nf, nu, records=out, records_decayed=outd, sampler_stats=d)
        return out, outd, d, dd

    def execute_flow_diff(self, n_cells, dev_ptrs, n_events, seed, cuts, pT_edges, slot, n_slots, table=None, slot_decayed=None,
                          n_slots_decayed=0, decay_seed=None, lifetime=0, x_ptr=0, y_ptr=0, first_cell=0, batch_events=0):
        """is3d_sampler_plan_execute_flow_diff: execute_flow with the pT bin of the edge table pT_edges as a second key of both sets of records.
        -> (records, sampler stats) | (records, decayed records, sampler stats, decay stats with n_final and n_unbinned)."""
        cs = Cells()
        cs.n_cells = int(n_cells)
        for f in CELL_FIELDS:
            if dev_ptrs.get(f):
                setattr(cs, f, int(dev_ptrs[f]))
        c = _pack_cuts(cuts)
        edges = np.ascontiguousarray(pT_edges, dtype=np.float64)
        slot = np.ascontiguousarray(slot, dtype=np.int32)
        r, out = _flow_diff_arrays(n_events, n_slots, len(edges) - 1)
        rd, outd = _flow_diff_arrays(n_events, n_slots_decayed if table is not None else 0, len(edges) - 1)
        sd = _slot_map(table.table, slot_decayed) if table is not None else None
        cnt, st, dst, nf, nu = C.c_int64(0), SamplerStats(), DecayMcStats(), C.c_int64(0), C.c_int64(0)
        fn = load().is3d_sampler_plan_execute_flow_diff
        fn.argtypes = [C.c_void_p, C.POINTER(Cells), C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, C.POINTER(FlowCuts),
                       C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(FlowDiffRecords), C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64,
                       C.c_int32, C.POINTER(FlowDiffRecords), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                       C.POINTER(SamplerStats), C.POINTER(DecayMcStats)]
        rc = fn(self._h, C.byref(cs), C.c_void_p(int(x_ptr) or None), C.c_void_p(int(y_ptr) or None), int(n_events), int(seed), int(first_cell),
                int(batch_events), C.byref(c), len(edges) - 1, edges.ctypes.data, slot.ctypes.data, int(n_slots), C.byref(r),
                table._h if table is not None else None, sd.ctypes.data if sd is not None else None, int(n_slots_decayed),
                int(seed if decay_seed is None else decay_seed), int(lifetime), C.byref(rd) if table is not None else None, C.byref(cnt),
                C.byref(nf), C.byref(nu), C.byref(st), C.byref(dst))
        d = st.as_dict()
        d["n_particles"] = int(cnt.value)
        if table is None:
            _check(rc)
            return out, d
        dd = _check_decayed(rc, dst, nf, nu, records=out, records_decayed=outd, sampler_stats=d)
        return out, outd, d, dd

    def execute_pairs(self, n_cells, dev_ptrs, n_events, seed, bins, slot, n_slots, table=None, slot_decayed=None, n_slots_decayed=0,
                      decay_seed=None, lifetime=0, x_ptr=0, y_ptr=0, first_cell=0, batch_events=0):
        """is3d_sampler_plan_execute_pairs: the pair histograms of the list execute returns (slot: int32 per species of the plan) and, with
        table (a DecayMcTable on the plan's device), of its Monte Carlo decay products (slot_decayed: int32 per table entry).
        -> (hist, sampler stats) | (hist, decayed hist, sampler stats, decay stats with n_final and n_unbinned)."""
        cs = Cells()
        cs.n_cells = int(n_cells)
        for f in CELL_FIELDS:
            if dev_ptrs.get(f):
                setattr(cs, f, int(dev_ptrs[f]))
        b = _pack_pair_bins(bins)
        slot = np.ascontiguousarray(slot, dtype=np.int32)
        h, out = _pair_arrays(b, n_events, n_slots)
        hd, outd = _pair_arrays(b, n_events, n_slots_decayed if table is not None else 0)
        sd = _slot_map(table.table, slot_decayed) if table is not None else None
        cnt, st, dst, nf, nu = C.c_int64(0), SamplerStats(), DecayMcStats(), C.c_int64(0), C.c_int64(0)
        fn = load().is3d_sampler_plan_execute_pairs
        fn.argtypes = [C.c_void_p, C.POINTER(Cells), C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, C.POINTER(PairBins),
                       C.c_void_p, C.c_int32, C.POINTER(PairHist), C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int32,
                       C.POINTER(PairHist), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(SamplerStats),
                       C.POINTER(DecayMcStats)]
        rc = fn(self._h, C.byref(cs), C.c_void_p(int(x_ptr) or None), C.c_void_p(int(y_ptr) or None), int(n_events), int(seed), int(first_cell),
                int(batch_events), C.byref(b), slot.ctypes.data, int(n_slots), C.byref(h), table._h if table is not None else None,
                sd.ctypes.data if sd is not None else None, int(n_slots_decayed), int(seed if decay_seed is None else decay_seed), int(lifetime),
                C.byref(hd) if table is not None else None, C.byref(cnt), C.byref(nf), C.byref(nu), C.byref(st), C.byref(dst))
        d = st.as_dict()
        d["n_particles"] = int(cnt.value)
        if table is None:
            _check(rc)
            return out, d
        dd = _check_decayed(rc, dst, nf, nu, hist=out, hist_decayed=outd, sampler_stats=d)
        return out, outd, d, dd

    def execute_hbt(self, n_cells, dev_ptrs, n_events, seed, bins, slot, n_slots, table=None, slot_decayed=None, n_slots_decayed=0,
                    decay_seed=None, lifetime=0, x_ptr=0, y_ptr=0, first_cell=0, batch_events=0):
        """is3d_sampler_plan_execute_hbt: the HBT histograms of the list execute returns (slot: int32 per species of the plan) and, with
        table (a DecayMcTable on the plan's device), of its Monte Carlo decay products (slot_decayed: int32 per table entry).
        -> (hist, sampler stats) | (hist, decayed hist, sampler stats, decay stats with n_final and n_unbinned)."""
        cs = Cells()
        cs.n_cells = int(n_cells)
        for f in CELL_FIELDS:
            if dev_ptrs.get(f):
                setattr(cs, f, int(dev_ptrs[f]))
        b = _pack_hbt_bins(bins)
        slot = np.ascontiguousarray(slot, dtype=np.int32)
        h, out = _hbt_arrays(b, n_events, n_slots)
        hd, outd = _hbt_arrays(b, n_events, n_slots_decayed if table is not None else 0)
        sd = _slot_map(table.table, slot_decayed) if table is not None else None
        cnt, st, dst, nf, nu = C.c_int64(0), SamplerStats(), DecayMcStats(), C.c_int64(0), C.c_int64(0)
        fn = load().is3d_sampler_plan_execute_hbt
        fn.argtypes = [C.c_void_p, C.POINTER(Cells), C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int64, C.c_int32, C.POINTER(HbtBins),
                       C.c_void_p, C.c_int32, C.POINTER(HbtHist), C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_int32,
                       C.POINTER(HbtHist), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(SamplerStats),
                       C.POINTER(DecayMcStats)]
        rc = fn(self._h, C.byref(cs), C.c_void_p(int(x_ptr) or None), C.c_void_p(int(y_ptr) or None), int(n_events), int(seed), int(first_cell),
                int(batch_events), C.byref(b), slot.ctypes.data, int(n_slots), C.byref(h), table._h if table is not None else None,
                sd.ctypes.data if sd is not None else None, int(n_slots_decayed), int(seed if decay_seed is None else decay_seed), int(lifetime),
                C.byref(hd) if table is not None else None, C.byref(cnt), C.byref(nf), C.byref(nu), C.byref(st), C.byref(dst))
        d = st.as_dict()
        d["n_particles"] = int(cnt.value)
        if table is None:
            _check(rc)
            return out, d
        dd = _check_decayed(rc, dst, nf, nu, hist=out, hist_decayed=outd, sampler_stats=d)
        return out, outd, d, dd

    def execute_fused(self, n_cells, dev_ptrs, n_events, seed, bins, n_species, x_ptr=0, y_ptr=0, first_cell=0, batch_events=0):
        """is3d_sampler_plan_execute_fused: execute_binned's arguments and result, every hadron binned where it is sampled (no list, no
        particle workspace: stats["particle_workspace_bytes"] == 0)."""
        return self.execute_binned(n_cells, dev_ptrs, n_events, seed, bins, n_species, x_ptr, y_ptr, first_cell, batch_events, _fused=True)

    def close(self):
        if self._h:
            load().is3d_sampler_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class YieldInputs(C.Structure):
    _fields_ = [(n, C.c_double) for n in ["T", "E", "P", "muB", "nB"]] + [("root3", _dp), ("weight3", _dp)]


def total_yield(cells, species, df, gla, avg5, opts=None, y_cut=0.5, fq=None):
    """is3d_total_yield (the drop-in for calculate_total_yield): mean particle yield of the surface.  gla: dict with root1, weight1,
    root2, weight2 (+ root3, weight3 for df_mode 1), e.g. is3d_amd.inputs.feqmod_tables(); avg5 = (T, E, P, muB, nB) surface
    averages; fq: the feqmod tables for df_mode 4 (defaults to gla).  Returns (yield, densities[3][n_species])."""
    L = load()
    grid_dummy = dict(pT=[1.0], phi=[0.0], y=[0.0], eta=[0.0], eta_w=[1.0])
    sps, _, ds, os_, _, keep = _pack_common(species, grid_dummy, df, opts)
    n = len(cells["tau"])
    cs = Cells()
    cs.n_cells = n
    held = []
    for f in CELL_FIELDS:
        a = cells.get(f)
        if a is not None:
            a = _f64(a)
            assert a.shape == (n,), f
            held.append(a)
            setattr(cs, f, a.ctypes.data)
    r1, w1 = _f64(gla["root1"]), _f64(gla["weight1"])
    fqs = _pack_feqmod(fq if fq is not None else dict(gla, T_avg=gla.get("T_avg", avg5[0]), deta_min=gla.get("deta_min", 1e-5),
                                                      mass_pion0=gla.get("mass_pion0", 0.138)), keep)
    si = SamplerInputs(1, len(r1), 0, float(y_cut), 0, None, None, _p(r1), _p(w1), C.pointer(fqs), 0, 0, 0.0, 0.0, 0.0)
    r3 = _f64(gla["root3"]) if "root3" in gla else None
    w3 = _f64(gla["weight3"]) if "weight3" in gla else None
    yi = YieldInputs(float(avg5[0]), float(avg5[1]), float(avg5[2]), float(avg5[3]), float(avg5[4]), _p(r3) if r3 is not None else None,
                     _p(w3) if w3 is not None else None)
    out = C.c_double(0.0)
    dens = np.zeros((3, sps.n))
    L.is3d_total_yield.argtypes = [C.POINTER(Cells), C.POINTER(Species), C.POINTER(DfTables), C.POINTER(SamplerInputs), C.POINTER(YieldInputs),
                                   C.POINTER(Options), C.POINTER(C.c_double), _dp]
    _check(L.is3d_total_yield(C.byref(cs), C.byref(sps), C.byref(ds), C.byref(si), C.byref(yi), C.byref(os_), C.byref(out), _p(dens)))
    return out.value, dens


class YieldVahStats(C.Structure):
    _fields_ = [("n_cells_skipped", C.c_int64), ("n_classes", C.c_int32), ("reserved", C.c_int32), ("ms_h2d", C.c_double), ("ms_cells", C.c_double),
                ("ms_classes", C.c_double)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def total_yield_vah(cells, species, gla, opts=None, tab=None, y_cut=0.5, first_cell=0, fast=0, fq=None):
    """is3d_total_yield_vah: the mean number of hadrons an anisotropic-hydro surface emits (linear delta-f, no outflow cut, the cells with
    u.dsigma > 0), which sizes an oversampled run of sample_particles_vah.  cells: dict of host arrays per VAH_FIELDS; gla: dict with root1,
    weight1; tab (dict L, aL, c0..c4): the coefficients come from the (Lambda, alpha_L) tables and the cells' c0..c4 are ignored.  Returns
    (mean_yield, yield_by_species, stats dict).  A bad cell raises Is3dError(IS3D_EDOMAIN) with .bad_cell (the lowest global index),
    .mean_yield, .yield_by_species and .stats: the sums over the other cells.  fast, fq: passed on only so that the entry's refusals can be
    reached."""
    L = load()
    sps, _, _, os_, _, keep = _pack_common(species, dict(pT=[1.0], phi=[0.0], y=[0.0], eta=[0.0], eta_w=[1.0]), _VAH_DUMMY_DF, opts)
    held = [keep]
    if tab is not None:
        cells = {k: v for k, v in cells.items() if k not in ("c0", "c1", "c2", "c3", "c4")}
    cs = _vah_cells_struct(cells, held)
    ts = _pack_vah_tables(tab, keep) if tab is not None else None
    r1, w1 = _f64(gla["root1"]), _f64(gla["weight1"])
    fqs = _pack_feqmod(fq, keep) if fq is not None else None
    si = SamplerInputs(1, len(r1), 0, float(y_cut), int(first_cell), None, None, _p(r1), _p(w1), C.pointer(fqs) if fqs is not None else None,
                       int(fast), 0, 0.0, 0.0, 0.0)
    st = YieldVahStats()
    out = C.c_double(0.0)
    by = np.zeros(sps.n)
    L.is3d_total_yield_vah.argtypes = [C.POINTER(VahCells), C.POINTER(Species), C.POINTER(VahDfTables), C.POINTER(SamplerInputs), C.POINTER(Options),
                                       C.POINTER(C.c_double), _dp, C.POINTER(YieldVahStats)]
    rc = L.is3d_total_yield_vah(C.byref(cs), C.byref(sps), C.byref(ts) if ts is not None else None, C.byref(si), C.byref(os_), C.byref(out), _p(by),
                                C.byref(st))
    if rc == IS3D_EDOMAIN:
        msg = L.is3d_last_error().decode()
        m = re.search(r"cell (\d+):", msg)
        e = Is3dError(rc, msg, bad_cell=int(m.group(1)) if m else None)
        e.mean_yield, e.yield_by_species, e.stats = out.value, by, st.as_dict()
        raise e
    _check(rc)
    return out.value, by, st.as_dict()


def oversample_events(min_num_hadrons, mean_yield, max_num_samples):
    """is3d_oversample_events: max(1, min(ceil(min_num_hadrons / |(float) mean_yield|), max_num_samples)), the number of events of an
    oversampled run (emissionfunction.cpp:1524-1533)."""
    L = load()
    L.is3d_oversample_events.argtypes = [C.c_double, C.c_double, C.c_int32, C.POINTER(C.c_int32)]
    n = C.c_int32(0)
    _check(L.is3d_oversample_events(float(min_num_hadrons), float(mean_yield), int(max_num_samples), C.byref(n)))
    return int(n.value)


def write_particle_list_osc(path, n_events, particles, mc_id):
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    ids = np.ascontiguousarray(mc_id, dtype=np.int64)
    _check(load().is3d_write_particle_list_osc(path.encode(), int(n_events), len(particles), particles.ctypes.data,
                                               ids.ctypes.data_as(C.POINTER(C.c_int64))))


class SamplerTestBins(C.Structure):
    _fields_ = [(n, C.c_double) for n in ["y_cut", "eta_cut", "pT_lower_cut", "pT_upper_cut", "tau_min", "tau_max", "r_min", "r_max"]] + \
               [(n, C.c_int32) for n in ["y_bins", "eta_bins", "pT_bins", "tau_bins", "r_bins", "kernel_form"]]


def write_sampler_tests(results_dir, bins, n_events, mc_id, particles, mean_yield=0.0):
    """is3d_write_sampler_tests: the test_sampler = 1 binned outputs from a particle list."""
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    ids = np.ascontiguousarray(mc_id, dtype=np.int64)
    b = SamplerTestBins()
    for k, v in bins.items():
        setattr(b, k, v)
    L = load()
    L.is3d_write_sampler_tests.argtypes = [C.c_char_p, C.POINTER(SamplerTestBins), C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.c_int64,
                                           C.c_void_p, C.c_double]
    _check(L.is3d_write_sampler_tests(results_dir.encode(), C.byref(b), int(n_events), len(ids), ids.ctypes.data_as(C.POINTER(C.c_int64)),
                                      len(particles), particles.ctypes.data, float(mean_yield)))


class SamplerHist(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_int64)) for n in ["dN_dy", "dN_deta", "dN_pT", "dN_tau", "dN_r", "vn_re", "vn_im", "yield"]]


VN_HARMONICS = 7          # IS3D_SAMPLER_VN_HARMONICS
VN_SCALE = 2.0 ** 32      # IS3D_SAMPLER_VN_SCALE: vn_re, vn_im hold the sums of llrint(term * 2^32)


def _pack_bins(bins):
    b = SamplerTestBins()
    for k, v in bins.items():
        setattr(b, k, v)
    return b


def _hist_arrays(bins, n_events, n_species, hist=None):
    """is3d_sampler_hist over numpy int64 arrays: (struct, dict).  hist = None: fresh zero arrays of the shapes [species][bin],
    vn_re / vn_im [7][species][pT bin], yield [event]; otherwise the caller's arrays are checked and used."""
    S, E, nb = int(n_species), int(n_events), {k: max(int(bins[k]), 0) for k in ("y_bins", "eta_bins", "pT_bins", "tau_bins", "r_bins")}
    shapes = dict(dN_dy=(S, nb["y_bins"]), dN_deta=(S, nb["eta_bins"]), dN_pT=(S, nb["pT_bins"]), dN_tau=(S, nb["tau_bins"]), dN_r=(S, nb["r_bins"]),
                  vn_re=(VN_HARMONICS, S, nb["pT_bins"]), vn_im=(VN_HARMONICS, S, nb["pT_bins"]))
    shapes["yield"] = (max(E, 0),)
    out = {}
    for k, shp in shapes.items():
        if hist is None:
            out[k] = np.zeros(shp, dtype=np.int64)
        else:
            out[k] = np.ascontiguousarray(hist[k], dtype=np.int64)
            assert out[k].shape == shp, (k, out[k].shape, shp)
    h = SamplerHist(*[out[k].ctypes.data_as(C.POINTER(C.c_int64)) for k, _ in SamplerHist._fields_])
    return h, out


def sampler_bin_list(bins, n_events, n_species, particles):
    """is3d_sampler_bin_list: a particle list -> dict of int64 histograms (the CPU yardstick of the device binning)."""
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    b = _pack_bins(bins)
    h, out = _hist_arrays(bins, n_events, n_species)
    L = load()
    L.is3d_sampler_bin_list.argtypes = [C.POINTER(SamplerTestBins), C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(SamplerHist)]
    _check(L.is3d_sampler_bin_list(C.byref(b), int(n_events), int(n_species), len(particles), particles.ctypes.data, C.byref(h)))
    return out


def sampler_bin_list_device(bins, n_events, n_species, particles, device=0):
    """is3d_sampler_bin_list_device: a host particle list binned by the device kernel (form bins["kernel_form"]).  Returns (dict of int64
    histograms, n_skipped); n_skipped counts the particles whose species or event is out of range, which add nothing."""
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    b = _pack_bins(bins)
    h, out = _hist_arrays(bins, n_events, n_species)
    skipped = C.c_int64(0)
    L = load()
    L.is3d_sampler_bin_list_device.argtypes = [C.POINTER(SamplerTestBins), C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(SamplerHist),
                                               C.POINTER(C.c_int64), C.c_int32]
    _check(L.is3d_sampler_bin_list_device(C.byref(b), int(n_events), int(n_species), len(particles), particles.ctypes.data, C.byref(h),
                                          C.byref(skipped), int(device)))
    return out, int(skipped.value)


FLOW_HARMONICS = 8        # IS3D_FLOW_HARMONICS
FLOW_CUTS = dict(y_cut=1.0, y_gap=0.5, pT_min=0.2, pT_max=3.0)   # the run driver's defaults


class FlowCuts(C.Structure):
    _fields_ = [(n, C.c_double) for n in ["y_cut", "y_gap", "pT_min", "pT_max"]] + [("kernel_form", C.c_int32)]


class FlowRecords(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_int64)) for n in ["M", "Q_re", "Q_im"]]


class FlowResult(C.Structure):
    _fields_ = [(n, C.c_double * FLOW_HARMONICS) for n in ["c2", "c2_gap", "v2", "v2_gap", "v_rp"]] + \
               [(n, C.c_double * 4) for n in ["avg4", "c4", "v4"]] + [("mean_M", C.c_double), ("var_M", C.c_double)] + \
               [(n, C.c_int64) for n in ["n_used_2", "n_used_4", "n_used_gap", "n_events"]]


def _pack_cuts(cuts):
    c = FlowCuts()
    for k, v in cuts.items():
        setattr(c, k, v)
    return c


def _flow_arrays(n_events, n_slots, records=None):
    """is3d_flow_records over numpy int64 arrays: (struct, dict).  records = None: fresh zero arrays M [event][slot][3], Q_re / Q_im
    [event][slot][3][8] (region 0 full acceptance, 1 sub-event A, 2 sub-event B); otherwise the caller's arrays are checked and used."""
    E, S = max(int(n_events), 0), max(int(n_slots), 0)
    shapes = dict(M=(E, S, 3), Q_re=(E, S, 3, FLOW_HARMONICS), Q_im=(E, S, 3, FLOW_HARMONICS))
    out = {}
    for k, shp in shapes.items():
        if records is None:
            out[k] = np.zeros(shp, dtype=np.int64)
        else:
            out[k] = np.ascontiguousarray(records[k], dtype=np.int64)
            assert out[k].shape == shp, (k, out[k].shape, shp)
    r = FlowRecords(*[out[k].ctypes.data_as(C.POINTER(C.c_int64)) for k, _ in FlowRecords._fields_])
    return r, out


def flow_list(cuts, n_events, n_slots, slot, particles):
    """is3d_flow_list: a particle list -> the per-event flow records on the host (the definition; no device use).  slot: int32 per species,
    -1 drops the species.  Returns a dict of int64 arrays M, Q_re, Q_im."""
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    c = _pack_cuts(cuts)
    r, out = _flow_arrays(n_events, n_slots)
    L = load()
    L.is3d_flow_list.argtypes = [C.POINTER(FlowCuts), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(FlowRecords)]
    _check(L.is3d_flow_list(C.byref(c), int(n_events), int(n_slots), slot.ctypes.data, len(slot), len(particles), particles.ctypes.data, C.byref(r)))
    return out


def flow_list_device(cuts, n_events, n_slots, slot, particles, device=0):
    """is3d_flow_list_device: a host particle list through the device kernel cf_sampler_flow (form cuts["kernel_form"]).  Returns (records,
    n_skipped); n_skipped counts the particles whose species or event is out of range, which add nothing."""
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    c = _pack_cuts(cuts)
    r, out = _flow_arrays(n_events, n_slots)
    skipped = C.c_int64(0)
    L = load()
    L.is3d_flow_list_device.argtypes = [C.POINTER(FlowCuts), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(FlowRecords),
                                        C.POINTER(C.c_int64), C.c_int32]
    _check(L.is3d_flow_list_device(C.byref(c), int(n_events), int(n_slots), slot.ctypes.data, len(slot), len(particles), particles.ctypes.data,
                                   C.byref(r), C.byref(skipped), int(device)))
    return out, int(skipped.value)


def flow_merge(records, group, n_groups):
    """is3d_flow_merge: the integer sums of the slots s with group[s] = g, per event and region (group -1: left out)."""
    group = np.ascontiguousarray(group, dtype=np.int32)
    n_events, n_slots = np.shape(records["M"])[:2]
    r, _keep = _flow_arrays(n_events, n_slots, records)
    o, out = _flow_arrays(n_events, n_groups)
    L = load()
    L.is3d_flow_merge.argtypes = [C.POINTER(FlowRecords), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(FlowRecords)]
    assert len(group) == n_slots, (len(group), n_slots)
    _check(L.is3d_flow_merge(C.byref(r), n_events, n_slots, group.ctypes.data, int(n_groups), C.byref(o)))
    return out


def flow_cumulants(records):
    """is3d_flow_cumulants: the Q-cumulants of every slot.  Returns a dict of arrays with the slot as first axis: c2, c2_gap, v2, v2_gap,
    v_rp [slot][8]; avg4, c4, v4 [slot][4]; mean_M, var_M, n_used_2, n_used_4, n_used_gap, n_events [slot]."""
    n_events, n_slots = np.shape(records["M"])[:2]
    r, _keep = _flow_arrays(n_events, n_slots, records)
    res = (FlowResult * max(n_slots, 1))()
    L = load()
    L.is3d_flow_cumulants.argtypes = [C.POINTER(FlowRecords), C.c_int32, C.c_int32, C.POINTER(FlowResult)]
    _check(L.is3d_flow_cumulants(C.byref(r), n_events, n_slots, res))
    return {k: np.array([np.array(getattr(res[s], k)) for s in range(n_slots)]) for k, _ in FlowResult._fields_}


def write_flow(results_dir, records, labels):
    """is3d_write_flow: <results_dir>/flow/cumulants_<label>.dat and multiplicity_<label>.dat for every slot of the records."""
    n_events, n_slots = np.shape(records["M"])[:2]
    assert len(labels) == n_slots, (len(labels), n_slots)
    r, _keep = _flow_arrays(n_events, n_slots, records)
    names = (C.c_char_p * n_slots)(*[str(x).encode() for x in labels])
    L = load()
    L.is3d_write_flow.argtypes = [C.c_char_p, C.POINTER(FlowRecords), C.c_int32, C.c_int32, C.POINTER(C.c_char_p)]
    _check(L.is3d_write_flow(results_dir.encode(), C.byref(r), n_events, n_slots, names))


FLOW_DIFF_MAX_BINS = 64   # IS3D_FLOW_DIFF_MAX_BINS


class FlowDiffRecords(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_int64)) for n in ["m", "p_re", "p_im"]]


class FlowDiffResult(C.Structure):
    _fields_ = [(n, C.c_double * FLOW_HARMONICS) for n in ["d2", "d2_gap", "v2", "v2_gap", "v_rp"]] + \
               [(n, C.c_double * 4) for n in ["avg4", "d4", "v4"]] + [("mean_m", C.c_double), ("sum_m", C.c_double)] + \
               [(n, C.c_int64) for n in ["n_used_2", "n_used_4", "n_used_gap", "n_events"]]


def flow_diff_edges(pT_min, pT_max, n_pT):
    """The run driver's uniform edge table: pT_min + k (pT_max - pT_min) / n_pT, the last edge pT_max exactly."""
    e = np.array([pT_min + k * (pT_max - pT_min) / n_pT for k in range(n_pT + 1)], dtype=np.float64)
    e[-1] = pT_max
    return e


def _flow_diff_arrays(n_events, n_slots, n_pT, records=None):
    """is3d_flow_diff_records over numpy int64 arrays: (struct, dict).  records = None: fresh zero arrays m [event][slot][bin][3], p_re /
    p_im [event][slot][bin][3][8]; otherwise the caller's arrays are checked and used."""
    E, S, B = max(int(n_events), 0), max(int(n_slots), 0), max(int(n_pT), 0)
    shapes = dict(m=(E, S, B, 3), p_re=(E, S, B, 3, FLOW_HARMONICS), p_im=(E, S, B, 3, FLOW_HARMONICS))
    out = {}
    for k, shp in shapes.items():
        if records is None:
            out[k] = np.zeros(shp, dtype=np.int64)
        else:
            out[k] = np.ascontiguousarray(records[k], dtype=np.int64)
            assert out[k].shape == shp, (k, out[k].shape, shp)
    r = FlowDiffRecords(*[out[k].ctypes.data_as(C.POINTER(C.c_int64)) for k, _ in FlowDiffRecords._fields_])
    return r, out


def flow_diff_list(cuts, pT_edges, n_events, n_slots, slot, particles):
    """is3d_flow_diff_list: a particle list -> the differential flow records on the host (the definition; no device use).  pT_edges: the
    n_pT + 1 bin edges, whose ends must equal cuts pT_min / pT_max bit for bit.  Returns a dict of int64 arrays m, p_re, p_im."""
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    edges = np.ascontiguousarray(pT_edges, dtype=np.float64)
    c = _pack_cuts(cuts)
    r, out = _flow_diff_arrays(n_events, n_slots, len(edges) - 1)
    L = load()
    L.is3d_flow_diff_list.argtypes = [C.POINTER(FlowCuts), C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p,
                                      C.POINTER(FlowDiffRecords)]
    _check(L.is3d_flow_diff_list(C.byref(c), len(edges) - 1, edges.ctypes.data, int(n_events), int(n_slots), slot.ctypes.data, len(slot),
                                 len(particles), particles.ctypes.data, C.byref(r)))
    return out


def flow_diff_list_device(cuts, pT_edges, n_events, n_slots, slot, particles, device=0):
    """is3d_flow_diff_list_device: a host particle list through the device kernel cf_sampler_flow_diff (form cuts["kernel_form"]).  Returns
    (records, n_skipped); n_skipped counts the particles whose species or event is out of range, which add nothing."""
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    edges = np.ascontiguousarray(pT_edges, dtype=np.float64)
    c = _pack_cuts(cuts)
    r, out = _flow_diff_arrays(n_events, n_slots, len(edges) - 1)
    skipped = C.c_int64(0)
    L = load()
    L.is3d_flow_diff_list_device.argtypes = [C.POINTER(FlowCuts), C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64,
                                             C.c_void_p, C.POINTER(FlowDiffRecords), C.POINTER(C.c_int64), C.c_int32]
    _check(L.is3d_flow_diff_list_device(C.byref(c), len(edges) - 1, edges.ctypes.data, int(n_events), int(n_slots), slot.ctypes.data, len(slot),
                                        len(particles), particles.ctypes.data, C.byref(r), C.byref(skipped), int(device)))
    return out, int(skipped.value)


def _flow_diff_ref(records, ref_slot, ref_bins):
    n_events, n_slots, n_pT = np.shape(records["m"])[:3]
    ref_slot = np.ascontiguousarray(np.ones(n_slots) if ref_slot is None else ref_slot, dtype=np.int32)
    assert len(ref_slot) == n_slots, (len(ref_slot), n_slots)
    lo, hi = (0, n_pT) if ref_bins is None else ref_bins
    return n_events, n_slots, n_pT, ref_slot, int(lo), int(hi)


def flow_diff_reference(records, ref_slot=None, ref_bins=None):
    """is3d_flow_diff_reference: the reference flow records (one slot) of the differential records -- the integer sums over the slots with
    ref_slot[s] = 1 (None: all) and the bins [ref_bins[0], ref_bins[1]) (None: all).  Returns a dict M, Q_re, Q_im as flow_list's."""
    n_events, n_slots, n_pT, ref_slot, lo, hi = _flow_diff_ref(records, ref_slot, ref_bins)
    r, _keep = _flow_diff_arrays(n_events, n_slots, n_pT, records)
    o, out = _flow_arrays(n_events, 1)
    L = load()
    L.is3d_flow_diff_reference.argtypes = [C.POINTER(FlowDiffRecords), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                           C.POINTER(FlowRecords)]
    _check(L.is3d_flow_diff_reference(C.byref(r), n_events, n_slots, n_pT, ref_slot.ctypes.data, lo, hi, C.byref(o)))
    return out


def flow_diff_cumulants(records, ref_slot=None, ref_bins=None):
    """is3d_flow_diff_cumulants: the differential Q-cumulants of every (slot, bin) against the reference of flow_diff_reference.  Returns a
    dict of arrays with (slot, bin) as first axes: d2, d2_gap, v2, v2_gap, v_rp [slot][bin][8]; avg4, d4, v4 [slot][bin][4]; mean_m, sum_m,
    n_used_2, n_used_4, n_used_gap, n_events [slot][bin]."""
    n_events, n_slots, n_pT, ref_slot, lo, hi = _flow_diff_ref(records, ref_slot, ref_bins)
    r, _keep = _flow_diff_arrays(n_events, n_slots, n_pT, records)
    res = (FlowDiffResult * max(n_slots * n_pT, 1))()
    L = load()
    L.is3d_flow_diff_cumulants.argtypes = [C.POINTER(FlowDiffRecords), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                           C.POINTER(FlowDiffResult)]
    _check(L.is3d_flow_diff_cumulants(C.byref(r), n_events, n_slots, n_pT, ref_slot.ctypes.data, lo, hi, res))
    return {k: np.array([[np.array(getattr(res[s * n_pT + b], k)) for b in range(n_pT)] for s in range(n_slots)]) for k, _ in FlowDiffResult._fields_}


def write_flow_diff(results_dir, records, pT_edges, labels, ref_slot=None, ref_bins=None):
    """is3d_write_flow_diff: <results_dir>/flow/differential_<label>.dat for every slot of the records."""
    n_events, n_slots, n_pT, ref_slot, lo, hi = _flow_diff_ref(records, ref_slot, ref_bins)
    assert len(labels) == n_slots, (len(labels), n_slots)
    edges = np.ascontiguousarray(pT_edges, dtype=np.float64)
    assert len(edges) == n_pT + 1, (len(edges), n_pT)
    r, _keep = _flow_diff_arrays(n_events, n_slots, n_pT, records)
    names = (C.c_char_p * n_slots)(*[str(x).encode() for x in labels])
    L = load()
    L.is3d_write_flow_diff.argtypes = [C.c_char_p, C.POINTER(FlowDiffRecords), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_int32, C.POINTER(C.c_char_p)]
    _check(L.is3d_write_flow_diff(results_dir.encode(), C.byref(r), n_events, n_slots, n_pT, edges.ctypes.data, ref_slot.ctypes.data, lo, hi, names))


PAIR_BINS = dict(y_cut=2.0, pT_min=0.2, pT_max=3.0, n_y=32, n_phi=32)   # the run driver's defaults


class PairBins(C.Structure):
    _fields_ = [(n, C.c_double) for n in ["y_cut", "pT_min", "pT_max"]] + [("n_y", C.c_int32), ("n_phi", C.c_int32)]


class PairHist(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_int64)) for n in ["same", "mixed", "M"]]


class PairResult(C.Structure):
    _fields_ = [("n_same", C.c_int64), ("n_mixed", C.c_int64), ("V", C.c_double * 4)]


def _pack_pair_bins(bins):
    if isinstance(bins, PairBins):
        return bins
    b = PairBins()
    for k, v in bins.items():
        setattr(b, k, v)
    return b


def pair_classes(n_slots):
    """The number of slot pairs (a <= b) of n_slots slots; class (a, b) has index a n_slots - a (a - 1) / 2 + (b - a)."""
    return n_slots * (n_slots + 1) // 2


def pair_class(a, b, n_slots):
    assert 0 <= a <= b < n_slots, (a, b, n_slots)
    return a * n_slots - a * (a - 1) // 2 + (b - a)


def _pair_arrays(b, n_events, n_slots, hist=None):
    """is3d_pair_hist over numpy int64 arrays: (struct, dict).  hist = None: fresh zero arrays same and mixed [class][2 n_y - 1][n_phi] and
    M [event][slot] (shaped for valid bins; a refusal never writes them); otherwise the caller's arrays are checked and used."""
    E, S = max(int(n_events), 0), max(int(n_slots), 0)
    ny, nphi = min(max(int(b.n_y), 1), 64), min(max(int(b.n_phi), 1), 64)
    shapes = dict(same=(pair_classes(S), 2 * ny - 1, nphi), mixed=(pair_classes(S), 2 * ny - 1, nphi), M=(E, S))
    out = {}
    for k, shp in shapes.items():
        if hist is None:
            out[k] = np.zeros(shp, dtype=np.int64)
        else:
            out[k] = np.ascontiguousarray(hist[k], dtype=np.int64)
            assert out[k].shape == shp, (k, out[k].shape, shp)
    h = PairHist(*[out[k].ctypes.data_as(C.POINTER(C.c_int64)) for k, _ in PairHist._fields_])
    return h, out


def pairs_list(bins, n_events, n_slots, slot, particles):
    """is3d_pairs_list: a particle list -> the same-event and mixed-event (delta y, delta phi) pair histograms on the host, as the explicit
    double loop (the definition; no device use; O(M^2) per event).  slot: int32 per species, -1 drops the species.  Returns a dict of int64
    arrays same, mixed [class][2 n_y - 1][n_phi] and M [event][slot]."""
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    b = _pack_pair_bins(bins)
    h, out = _pair_arrays(b, n_events, n_slots)
    L = load()
    L.is3d_pairs_list.argtypes = [C.POINTER(PairBins), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(PairHist)]
    _check(L.is3d_pairs_list(C.byref(b), int(n_events), int(n_slots), slot.ctypes.data, len(slot), len(particles), particles.ctypes.data, C.byref(h)))
    return out


def pairs_list_device(bins, n_events, n_slots, slot, particles, device=0):
    """is3d_pairs_list_device: a host particle list through the device kernels cf_pair_cells and cf_pair_correlate (no loop over pairs).
    Returns (hist, n_skipped); n_skipped counts the particles whose species or event is out of range, which add nothing."""
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    b = _pack_pair_bins(bins)
    h, out = _pair_arrays(b, n_events, n_slots)
    skipped = C.c_int64(0)
    L = load()
    L.is3d_pairs_list_device.argtypes = [C.POINTER(PairBins), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(PairHist),
                                         C.POINTER(C.c_int64), C.c_int32]
    _check(L.is3d_pairs_list_device(C.byref(b), int(n_events), int(n_slots), slot.ctypes.data, len(slot), len(particles), particles.ctypes.data,
                                    C.byref(h), C.byref(skipped), int(device)))
    return out, int(skipped.value)


def pairs_correlation(bins, hist, gap_bins=0):
    """is3d_pairs_correlation: per class, C = (same / n_same) / (mixed / n_mixed) (0 where mixed is 0), its delta phi projection over the
    rows at least gap_bins from delta y = 0 and V_n-delta, n = 1..4.  Returns a dict: C [class][2 n_y - 1][n_phi], C_phi [class][n_phi],
    V [class][4], n_same, n_mixed [class]."""
    b = _pack_pair_bins(bins)
    n_classes = np.shape(hist["same"])[0]
    n_slots = int(round((np.sqrt(8 * n_classes + 1) - 1) / 2))
    assert pair_classes(n_slots) == n_classes, n_classes
    n_events = np.shape(hist["M"])[0]
    h, _keep = _pair_arrays(b, n_events, n_slots, hist)
    Cc = np.zeros(np.shape(hist["same"]), dtype=np.float64)
    Cp = np.zeros((n_classes, int(b.n_phi)), dtype=np.float64)
    res = (PairResult * max(n_classes, 1))()
    L = load()
    L.is3d_pairs_correlation.argtypes = [C.POINTER(PairBins), C.POINTER(PairHist), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(PairResult)]
    _check(L.is3d_pairs_correlation(C.byref(b), C.byref(h), n_slots, int(gap_bins), Cc.ctypes.data, Cp.ctypes.data, res))
    return dict(C=Cc, C_phi=Cp, V=np.array([list(res[c].V) for c in range(n_classes)]).reshape(n_classes, 4),
                n_same=np.array([res[c].n_same for c in range(n_classes)], dtype=np.int64),
                n_mixed=np.array([res[c].n_mixed for c in range(n_classes)], dtype=np.int64))


def write_pairs(results_dir, bins, hist, labels):
    """is3d_write_pairs: <results_dir>/pairs/correlation_<A>_<B>.dat for every class (A <= B) of the histograms."""
    b = _pack_pair_bins(bins)
    n_slots = len(labels)
    n_events = np.shape(hist["M"])[0]
    h, _keep = _pair_arrays(b, n_events, n_slots, hist)
    names = (C.c_char_p * n_slots)(*[str(x).encode() for x in labels])
    L = load()
    L.is3d_write_pairs.argtypes = [C.c_char_p, C.POINTER(PairBins), C.POINTER(PairHist), C.c_int32, C.POINTER(C.c_char_p)]
    _check(L.is3d_write_pairs(results_dir.encode(), C.byref(b), C.byref(h), n_slots, names))


HBT_BINS = dict(y_cut=0.5, pT_min=0.1, pT_max=1.5, kT_min=0.1, kT_max=0.9, n_kT=4, q_max=0.1, n_q=20, kernel_form=0)   # the run driver's defaults


class HbtBins(C.Structure):
    _fields_ = [(n, C.c_double) for n in ["y_cut", "pT_min", "pT_max", "kT_min", "kT_max"]] + [("n_kT", C.c_int32), ("q_max", C.c_double),
                                                                                              ("n_q", C.c_int32), ("kernel_form", C.c_int32)]


class HbtHist(C.Structure):
    _fields_ = [(n, C.POINTER(C.c_int64)) for n in ["num", "den", "M"]]


class HbtRadii(C.Structure):
    _fields_ = [("lambda_", C.c_double), ("R2", C.c_double * 6), ("n_bins", C.c_int32), ("singular", C.c_int32)]


HBT_R2 = ("oo", "ss", "ll", "os", "ol", "sl")   # the order of R2


def _pack_hbt_bins(bins):
    if isinstance(bins, HbtBins):
        return bins
    b = HbtBins()
    for k, v in bins.items():
        setattr(b, k, v)
    return b


def _hbt_arrays(b, n_events, n_slots, hist=None):
    """is3d_hbt_hist over numpy int64 arrays: (struct, dict).  hist = None: fresh zero arrays num and den [slot][n_kT][n_q][n_q][n_q] and
    M [event][slot] (shaped for valid bins; a refusal never writes them); otherwise the caller's arrays are checked and used."""
    E, S = max(int(n_events), 0), max(int(n_slots), 0)
    nk, nq = min(max(int(b.n_kT), 1), 16), min(max(int(b.n_q), 1), 64)
    shapes = dict(num=(S, nk, nq, nq, nq), den=(S, nk, nq, nq, nq), M=(E, S))
    out = {}
    for k, shp in shapes.items():
        if hist is None:
            out[k] = np.zeros(shp, dtype=np.int64)
        else:
            out[k] = np.ascontiguousarray(hist[k], dtype=np.int64)
            assert out[k].shape == shp, (k, out[k].shape, shp)
    h = HbtHist(*[out[k].ctypes.data_as(C.POINTER(C.c_int64)) for k, _ in HbtHist._fields_])
    return h, out


def hbt_list(bins, n_events, n_slots, slot, particles):
    """is3d_hbt_list: a particle list -> the HBT histograms on the host, as the explicit double loop over the ordered identical-particle
    pairs of each event (the definition; no device use).  slot: int32 per species, -1 drops the species.  Returns a dict of int64 arrays
    num, den [slot][n_kT][n_q out][n_q side][n_q long] and M [event][slot]; the correlation is c = num / (den 2^32)."""
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    b = _pack_hbt_bins(bins)
    h, out = _hbt_arrays(b, n_events, n_slots)
    L = load()
    L.is3d_hbt_list.argtypes = [C.POINTER(HbtBins), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(HbtHist)]
    _check(L.is3d_hbt_list(C.byref(b), int(n_events), int(n_slots), slot.ctypes.data, len(slot), len(particles), particles.ctypes.data, C.byref(h)))
    return out


def hbt_list_device(bins, n_events, n_slots, slot, particles, device=0):
    """is3d_hbt_list_device: a host particle list through the device kernels cf_hbt_select and cf_hbt_pairs (form bins["kernel_form"]).
    Returns (hist, n_skipped); n_skipped counts the particles whose species or event is out of range, which add nothing."""
    particles = np.ascontiguousarray(particles, dtype=PARTICLE_DTYPE)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    b = _pack_hbt_bins(bins)
    h, out = _hbt_arrays(b, n_events, n_slots)
    skipped = C.c_int64(0)
    L = load()
    L.is3d_hbt_list_device.argtypes = [C.POINTER(HbtBins), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(HbtHist),
                                       C.POINTER(C.c_int64), C.c_int32]
    _check(L.is3d_hbt_list_device(C.byref(b), int(n_events), int(n_slots), slot.ctypes.data, len(slot), len(particles), particles.ctypes.data,
                                  C.byref(h), C.byref(skipped), int(device)))
    return out, int(skipped.value)


def hbt_radii(bins, hist, min_pairs=1, c_min=1e-3):
    """is3d_hbt_radii: per (slot, kT bin) the weighted log-linear fit of c = num / (den 2^32) over the bins with den >= min_pairs and
    c >= c_min.  Returns a dict: lambda [slot][n_kT], R2 [slot][n_kT][6] in fm^2 in the order HBT_R2, n_bins and singular [slot][n_kT]."""
    b = _pack_hbt_bins(bins)
    n_slots = np.shape(hist["den"])[0]
    h, _keep = _hbt_arrays(b, np.shape(hist["M"])[0], n_slots, hist)
    n = max(n_slots * int(b.n_kT), 1)
    res = (HbtRadii * n)()
    L = load()
    L.is3d_hbt_radii.argtypes = [C.POINTER(HbtBins), C.POINTER(HbtHist), C.c_int32, C.c_int64, C.c_double, C.POINTER(HbtRadii)]
    _check(L.is3d_hbt_radii(C.byref(b), C.byref(h), n_slots, int(min_pairs), float(c_min), res))
    shp = (n_slots, int(b.n_kT))
    return {"lambda": np.array([r.lambda_ for r in res][:shp[0] * shp[1]]).reshape(shp),
            "R2": np.array([list(r.R2) for r in res][:shp[0] * shp[1]]).reshape(shp + (6,)),
            "n_bins": np.array([r.n_bins for r in res][:shp[0] * shp[1]], dtype=np.int64).reshape(shp),
            "singular": np.array([r.singular for r in res][:shp[0] * shp[1]], dtype=np.int64).reshape(shp)}


def write_hbt(results_dir, bins, hist, labels, min_pairs=1, c_min=1e-3):
    """is3d_write_hbt: <results_dir>/hbt/correlation_<label>_kT<k>.dat per slot and kT bin and radii_<label>.dat per slot."""
    b = _pack_hbt_bins(bins)
    n_slots = len(labels)
    h, _keep = _hbt_arrays(b, np.shape(hist["M"])[0], n_slots, hist)
    names = (C.c_char_p * n_slots)(*[str(x).encode() for x in labels])
    L = load()
    L.is3d_write_hbt.argtypes = [C.c_char_p, C.POINTER(HbtBins), C.POINTER(HbtHist), C.c_int32, C.POINTER(C.c_char_p), C.c_int64, C.c_double]
    _check(L.is3d_write_hbt(results_dir.encode(), C.byref(b), C.byref(h), n_slots, names, int(min_pairs), float(c_min)))


def write_sampler_tests_binned(results_dir, bins, n_events, mc_id, hist, mean_yield=0.0):
    """is3d_write_sampler_tests_binned: the test_sampler = 1 files from a dict of int64 histograms."""
    ids = np.ascontiguousarray(mc_id, dtype=np.int64)
    b = _pack_bins(bins)
    h, _keep = _hist_arrays(bins, n_events, len(ids), hist)
    L = load()
    L.is3d_write_sampler_tests_binned.argtypes = [C.c_char_p, C.POINTER(SamplerTestBins), C.c_int32, C.c_int32, C.POINTER(C.c_int64),
                                                  C.POINTER(SamplerHist), C.c_double]
    _check(L.is3d_write_sampler_tests_binned(results_dir.encode(), C.byref(b), int(n_events), len(ids), ids.ctypes.data_as(C.POINTER(C.c_int64)),
                                             C.byref(h), float(mean_yield)))


def sample_binned(cells, species, df, gla, bins, opts=None, n_events=1, seed=1, y_cut=0.5, first_cell=0, fq=None, fast=0, T_avg=0.0,
                  T_avg_switch=0.0, batch_events=0, muB_avg=0.0, devices=None, _fused=False):
    """is3d_sample_binned (devices = None) | is3d_sample_binned_multi: the sampler with every event batch binned on the device and dropped.
    Arguments as sample_particles; bins: dict of is3d_sampler_test_bins fields.  Returns (dict of int64 histograms, stats dict)."""
    cs, sps, ds, si, os_, _held = _pack_sampler(cells, species, df, gla, opts, n_events, seed, y_cut, first_cell, fq, fast, T_avg, T_avg_switch,
                                                batch_events, muB_avg)
    return _sample_binned("is3d_sample_fused" if _fused else "is3d_sample_binned", (C.byref(cs), C.byref(sps), C.byref(ds), C.byref(si), C.byref(os_)),
                          devices, bins, n_events, sps.n, False)


def sample_decayed_binned(cells, species, df, gla, bins, table, chosen_mc_id, slot, n_slots, opts=None, n_events=1, seed=1, decay_seed=None,
                          lifetime=0, y_cut=0.5, first_cell=0, fq=None, fast=0, T_avg=0.0, T_avg_switch=0.0, batch_events=0, muB_avg=0.0):
    """is3d_sample_decayed_binned: the viscous sampler with every event batch binned (as sample_binned) and, decayed on the device, binned
    again by slot.  chosen_mc_id: the mc_id of the species list.  Returns (thermal histograms, decayed histograms, sampler stats, decay stats
    with n_final and n_unbinned)."""
    cs, sps, ds, si, os_, _held = _pack_sampler(cells, species, df, gla, opts, n_events, seed, y_cut, first_cell, fq, fast, T_avg, T_avg_switch,
                                                batch_events, muB_avg)
    ts, ch, _, keep = _decay_pack(table, chosen_mc_id, dict(pT=[1.0], phi=[0.0], y=[0.0]))
    assert len(ch) == sps.n, (len(ch), sps.n)
    b = _pack_bins(bins)
    h, out = _hist_arrays(bins, n_events, sps.n)
    hd, outd = _hist_arrays(bins, n_events, n_slots)
    slot = _slot_map(table, slot)
    cnt, st, dst, nf, nu = C.c_int64(0), SamplerStats(), DecayMcStats(), C.c_int64(0), C.c_int64(0)
    fn = load().is3d_sample_decayed_binned
    fn.argtypes = [C.POINTER(Cells), C.POINTER(Species), C.POINTER(DfTables), C.POINTER(SamplerInputs), C.POINTER(Options),
                   C.POINTER(SamplerTestBins), C.POINTER(SamplerHist), C.POINTER(DecayTable), C.POINTER(C.c_int64), C.c_void_p, C.c_int32,
                   C.c_uint64, C.c_int32, C.POINTER(SamplerHist), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                   C.POINTER(SamplerStats), C.POINTER(DecayMcStats)]
    rc = fn(C.byref(cs), C.byref(sps), C.byref(ds), C.byref(si), C.byref(os_), C.byref(b), C.byref(h), C.byref(ts),
            ch.ctypes.data_as(C.POINTER(C.c_int64)), slot.ctypes.data, int(n_slots), int(seed if decay_seed is None else decay_seed), int(lifetime),
            C.byref(hd), C.byref(cnt), C.byref(nf), C.byref(nu), C.byref(st), C.byref(dst))
    d = st.as_dict()
    d["n_particles"] = int(cnt.value)
    dd = _check_decayed(rc, dst, nf, nu, hist=out, hist_decayed=outd, sampler_stats=d)
    return out, outd, d, dd


def sample_flow(cells, species, df, gla, cuts, slot, n_slots, opts=None, table=None, chosen_mc_id=None, slot_decayed=None, n_slots_decayed=0,
                n_events=1, seed=1, decay_seed=None, lifetime=0, y_cut=0.5, first_cell=0, fq=None, fast=0, T_avg=0.0, T_avg_switch=0.0,
                batch_events=0, muB_avg=0.0):
    """is3d_sample_flow: the viscous sampler with every event batch turned into per-event flow records on the device (slot: int32 per
    species) and, with table (pdg_read_decays' dict; chosen_mc_id: the mc_id of the species list), decayed and recorded again by
    slot_decayed (int32 per table entry).  Returns (records, sampler stats) | (records, decayed records, sampler stats, decay stats)."""
    cs, sps, ds, si, os_, _held = _pack_sampler(cells, species, df, gla, opts, n_events, seed, y_cut, first_cell, fq, fast, T_avg, T_avg_switch,
                                                batch_events, muB_avg)
    c = _pack_cuts(cuts)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    assert len(slot) == sps.n, (len(slot), sps.n)
    r, out = _flow_arrays(n_events, n_slots)
    rd, outd = _flow_arrays(n_events, n_slots_decayed if table is not None else 0)
    ts = ch = sd = None
    if table is not None:
        ts, ch, _, keep = _decay_pack(table, chosen_mc_id, dict(pT=[1.0], phi=[0.0], y=[0.0]))
        assert len(ch) == sps.n, (len(ch), sps.n)
        sd = _slot_map(table, slot_decayed)
    cnt, st, dst, nf, nu = C.c_int64(0), SamplerStats(), DecayMcStats(), C.c_int64(0), C.c_int64(0)
    fn = load().is3d_sample_flow
    fn.argtypes = [C.POINTER(Cells), C.POINTER(Species), C.POINTER(DfTables), C.POINTER(SamplerInputs), C.POINTER(Options), C.POINTER(FlowCuts),
                   C.c_void_p, C.c_int32, C.POINTER(FlowRecords), C.POINTER(DecayTable), C.POINTER(C.c_int64), C.c_void_p, C.c_int32, C.c_uint64,
                   C.c_int32, C.POINTER(FlowRecords), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(SamplerStats),
                   C.POINTER(DecayMcStats)]
    rc = fn(C.byref(cs), C.byref(sps), C.byref(ds), C.byref(si), C.byref(os_), C.byref(c), slot.ctypes.data, int(n_slots), C.byref(r),
            C.byref(ts) if ts is not None else None, ch.ctypes.data_as(C.POINTER(C.c_int64)) if ch is not None else None,
            sd.ctypes.data if sd is not None else None, int(n_slots_decayed), int(seed if decay_seed is None else decay_seed), int(lifetime),
            C.byref(rd) if table is not None else None, C.byref(cnt), C.byref(nf), C.byref(nu), C.byref(st), C.byref(dst))
    d = st.as_dict()
    d["n_particles"] = int(cnt.value)
    if table is None:
        _check(rc)
        return out, d
    dd = _check_decayed(rc, dst, nf, nu, records=out, records_decayed=outd, sampler_stats=d)
    return out, outd, d, dd


def sample_flow_diff(cells, species, df, gla, cuts, pT_edges, slot, n_slots, opts=None, table=None, chosen_mc_id=None, slot_decayed=None,
                     n_slots_decayed=0, n_events=1, seed=1, decay_seed=None, lifetime=0, y_cut=0.5, first_cell=0, fq=None, fast=0, T_avg=0.0,
                     T_avg_switch=0.0, batch_events=0, muB_avg=0.0):
    """is3d_sample_flow_diff: sample_flow with the pT bin of the edge table pT_edges as a second key of both sets of records.  Returns
    (records, sampler stats) | (records, decayed records, sampler stats, decay stats)."""
    cs, sps, ds, si, os_, _held = _pack_sampler(cells, species, df, gla, opts, n_events, seed, y_cut, first_cell, fq, fast, T_avg, T_avg_switch,
                                                batch_events, muB_avg)
    c = _pack_cuts(cuts)
    edges = np.ascontiguousarray(pT_edges, dtype=np.float64)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    assert len(slot) == sps.n, (len(slot), sps.n)
    r, out = _flow_diff_arrays(n_events, n_slots, len(edges) - 1)
    rd, outd = _flow_diff_arrays(n_events, n_slots_decayed if table is not None else 0, len(edges) - 1)
    ts = ch = sd = None
    if table is not None:
        ts, ch, _, keep = _decay_pack(table, chosen_mc_id, dict(pT=[1.0], phi=[0.0], y=[0.0]))
        assert len(ch) == sps.n, (len(ch), sps.n)
        sd = _slot_map(table, slot_decayed)
    cnt, st, dst, nf, nu = C.c_int64(0), SamplerStats(), DecayMcStats(), C.c_int64(0), C.c_int64(0)
    fn = load().is3d_sample_flow_diff
    fn.argtypes = [C.POINTER(Cells), C.POINTER(Species), C.POINTER(DfTables), C.POINTER(SamplerInputs), C.POINTER(Options), C.POINTER(FlowCuts),
                   C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(FlowDiffRecords), C.POINTER(DecayTable), C.POINTER(C.c_int64), C.c_void_p,
                   C.c_int32, C.c_uint64, C.c_int32, C.POINTER(FlowDiffRecords), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                   C.POINTER(SamplerStats), C.POINTER(DecayMcStats)]
    rc = fn(C.byref(cs), C.byref(sps), C.byref(ds), C.byref(si), C.byref(os_), C.byref(c), len(edges) - 1, edges.ctypes.data, slot.ctypes.data,
            int(n_slots), C.byref(r), C.byref(ts) if ts is not None else None, ch.ctypes.data_as(C.POINTER(C.c_int64)) if ch is not None else None,
            sd.ctypes.data if sd is not None else None, int(n_slots_decayed), int(seed if decay_seed is None else decay_seed), int(lifetime),
            C.byref(rd) if table is not None else None, C.byref(cnt), C.byref(nf), C.byref(nu), C.byref(st), C.byref(dst))
    d = st.as_dict()
    d["n_particles"] = int(cnt.value)
    if table is None:
        _check(rc)
        return out, d
    dd = _check_decayed(rc, dst, nf, nu, records=out, records_decayed=outd, sampler_stats=d)
    return out, outd, d, dd


def sample_pairs(cells, species, df, gla, bins, slot, n_slots, opts=None, table=None, chosen_mc_id=None, slot_decayed=None, n_slots_decayed=0,
                 n_events=1, seed=1, decay_seed=None, lifetime=0, y_cut=0.5, first_cell=0, fq=None, fast=0, T_avg=0.0, T_avg_switch=0.0,
                 batch_events=0, muB_avg=0.0):
    """is3d_sample_pairs: the viscous sampler with every event batch turned into pair occupancies on the device (slot: int32 per species)
    and, with table (pdg_read_decays' dict; chosen_mc_id: the mc_id of the species list), decayed and counted again by slot_decayed (int32
    per table entry); the occupancies are correlated after the last batch.  Returns (hist, sampler stats) | (hist, decayed hist, sampler
    stats, decay stats)."""
    cs, sps, ds, si, os_, _held = _pack_sampler(cells, species, df, gla, opts, n_events, seed, y_cut, first_cell, fq, fast, T_avg, T_avg_switch,
                                                batch_events, muB_avg)
    b = _pack_pair_bins(bins)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    assert len(slot) == sps.n, (len(slot), sps.n)
    h, out = _pair_arrays(b, n_events, n_slots)
    hd, outd = _pair_arrays(b, n_events, n_slots_decayed if table is not None else 0)
    ts = ch = sd = None
    if table is not None:
        ts, ch, _, keep = _decay_pack(table, chosen_mc_id, dict(pT=[1.0], phi=[0.0], y=[0.0]))
        assert len(ch) == sps.n, (len(ch), sps.n)
        sd = _slot_map(table, slot_decayed)
    cnt, st, dst, nf, nu = C.c_int64(0), SamplerStats(), DecayMcStats(), C.c_int64(0), C.c_int64(0)
    fn = load().is3d_sample_pairs
    fn.argtypes = [C.POINTER(Cells), C.POINTER(Species), C.POINTER(DfTables), C.POINTER(SamplerInputs), C.POINTER(Options), C.POINTER(PairBins),
                   C.c_void_p, C.c_int32, C.POINTER(PairHist), C.POINTER(DecayTable), C.POINTER(C.c_int64), C.c_void_p, C.c_int32, C.c_uint64,
                   C.c_int32, C.POINTER(PairHist), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(SamplerStats),
                   C.POINTER(DecayMcStats)]
    rc = fn(C.byref(cs), C.byref(sps), C.byref(ds), C.byref(si), C.byref(os_), C.byref(b), slot.ctypes.data, int(n_slots), C.byref(h),
            C.byref(ts) if ts is not None else None, ch.ctypes.data_as(C.POINTER(C.c_int64)) if ch is not None else None,
            sd.ctypes.data if sd is not None else None, int(n_slots_decayed), int(seed if decay_seed is None else decay_seed), int(lifetime),
            C.byref(hd) if table is not None else None, C.byref(cnt), C.byref(nf), C.byref(nu), C.byref(st), C.byref(dst))
    d = st.as_dict()
    d["n_particles"] = int(cnt.value)
    if table is None:
        _check(rc)
        return out, d
    dd = _check_decayed(rc, dst, nf, nu, hist=out, hist_decayed=outd, sampler_stats=d)
    return out, outd, d, dd


def sample_hbt(cells, species, df, gla, bins, slot, n_slots, opts=None, table=None, chosen_mc_id=None, slot_decayed=None, n_slots_decayed=0,
               n_events=1, seed=1, decay_seed=None, lifetime=0, y_cut=0.5, first_cell=0, fq=None, fast=0, T_avg=0.0, T_avg_switch=0.0,
               batch_events=0, muB_avg=0.0):
    """is3d_sample_hbt: the viscous sampler with every event batch selected and paired on the device (slot: int32 per species) and, with
    table (pdg_read_decays' dict; chosen_mc_id: the mc_id of the species list), decayed and paired again by slot_decayed (int32 per table
    entry).  Returns (hist, sampler stats) | (hist, decayed hist, sampler stats, decay stats)."""
    cs, sps, ds, si, os_, _held = _pack_sampler(cells, species, df, gla, opts, n_events, seed, y_cut, first_cell, fq, fast, T_avg, T_avg_switch,
                                                batch_events, muB_avg)
    b = _pack_hbt_bins(bins)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    assert len(slot) == sps.n, (len(slot), sps.n)
    h, out = _hbt_arrays(b, n_events, n_slots)
    hd, outd = _hbt_arrays(b, n_events, n_slots_decayed if table is not None else 0)
    ts = ch = sd = None
    if table is not None:
        ts, ch, _, keep = _decay_pack(table, chosen_mc_id, dict(pT=[1.0], phi=[0.0], y=[0.0]))
        assert len(ch) == sps.n, (len(ch), sps.n)
        sd = _slot_map(table, slot_decayed)
    cnt, st, dst, nf, nu = C.c_int64(0), SamplerStats(), DecayMcStats(), C.c_int64(0), C.c_int64(0)
    fn = load().is3d_sample_hbt
    fn.argtypes = [C.POINTER(Cells), C.POINTER(Species), C.POINTER(DfTables), C.POINTER(SamplerInputs), C.POINTER(Options), C.POINTER(HbtBins),
                   C.c_void_p, C.c_int32, C.POINTER(HbtHist), C.POINTER(DecayTable), C.POINTER(C.c_int64), C.c_void_p, C.c_int32, C.c_uint64,
                   C.c_int32, C.POINTER(HbtHist), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(SamplerStats),
                   C.POINTER(DecayMcStats)]
    rc = fn(C.byref(cs), C.byref(sps), C.byref(ds), C.byref(si), C.byref(os_), C.byref(b), slot.ctypes.data, int(n_slots), C.byref(h),
            C.byref(ts) if ts is not None else None, ch.ctypes.data_as(C.POINTER(C.c_int64)) if ch is not None else None,
            sd.ctypes.data if sd is not None else None, int(n_slots_decayed), int(seed if decay_seed is None else decay_seed), int(lifetime),
            C.byref(hd) if table is not None else None, C.byref(cnt), C.byref(nf), C.byref(nu), C.byref(st), C.byref(dst))
    d = st.as_dict()
    d["n_particles"] = int(cnt.value)
    if table is None:
        _check(rc)
        return out, d
    dd = _check_decayed(rc, dst, nf, nu, hist=out, hist_decayed=outd, sampler_stats=d)
    return out, outd, d, dd


def sample_binned_multi(cells, species, df, gla, bins, opts=None, devices=(0,), **kw):
    """is3d_sample_binned_multi: one cell shard per entry of devices (an ordinal may repeat); the result equals sample_binned's bit for bit."""
    return sample_binned(cells, species, df, gla, bins, opts, devices=list(devices), **kw)


def sample_fused(cells, species, df, gla, bins, opts=None, **kw):
    """is3d_sample_fused (devices = None) | is3d_sample_fused_multi: sample_binned's arguments and result with every hadron binned where it
    is sampled -- one pass per event batch, no list, no particle workspace.  Counts and yields equal sample_binned's; so do the harmonics."""
    return sample_binned(cells, species, df, gla, bins, opts, _fused=True, **kw)


def sample_fused_multi(cells, species, df, gla, bins, opts=None, devices=(0,), **kw):
    """is3d_sample_fused_multi: one cell shard per entry of devices (an ordinal may repeat); the result equals sample_fused's bit for bit."""
    return sample_fused(cells, species, df, gla, bins, opts, devices=list(devices), **kw)


def sample_binned_vah(cells, species, gla, bins, opts=None, tab=None, n_events=1, seed=1, y_cut=0.5, first_cell=0, batch_events=0, devices=None,
                      fast=0, fq=None):
    """is3d_sample_binned_vah (devices = None) | is3d_sample_binned_vah_multi: the anisotropic-hydro sampler with every hadron binned where it
    is sampled, in one pass and without a list.  Arguments as sample_particles_vah; bins: dict of is3d_sampler_test_bins fields.  Returns
    (dict of int64 histograms, stats dict): the histograms of sampler_bin_list on sample_particles_vah's list.  A bad cell raises
    Is3dError(IS3D_EDOMAIN) with .bad_cell (the lowest global index), .hist and .stats: the other cells are binned all the same."""
    cs, sps, tp, si, os_, _held = _pack_sampler_vah(cells, species, gla, opts, tab, n_events, seed, y_cut, first_cell, batch_events, fast, fq)
    return _sample_binned("is3d_sample_binned_vah", (C.byref(cs), C.byref(sps), tp, C.byref(si), C.byref(os_)), devices, bins, n_events, sps.n, True)


def sample_binned_vah_multi(cells, species, gla, bins, opts=None, devices=(0,), **kw):
    """is3d_sample_binned_vah_multi: one cell shard per entry of devices (an ordinal may repeat); the result equals sample_binned_vah's bit
    for bit."""
    return sample_binned_vah(cells, species, gla, bins, opts, devices=list(devices), **kw)


def gla_read(path):
    """is3d_gla_read -> (root[n_alpha][n_points], weight[n_alpha][n_points])"""
    L = load()
    na, npts = C.c_int32(), C.c_int32()
    _check(L.is3d_gla_read(path.encode(), C.byref(na), C.byref(npts), None, None, 0))
    r, w = np.zeros((na.value, npts.value)), np.zeros((na.value, npts.value))
    _check(L.is3d_gla_read(path.encode(), C.byref(na), C.byref(npts), _p(r), _p(w), r.size))
    return r, w


def write_results(results_dir, dimension, mc_id, pT, pT_w, phi, phi_w, y, dN):
    L = load()
    mc = np.ascontiguousarray(mc_id, dtype=np.int64)
    pT, pT_w, phi, phi_w, y, dN = (_f64(a) for a in (pT, pT_w, phi, phi_w, y, dN))
    _check(L.is3d_write_results(results_dir.encode(), dimension, len(mc), mc.ctypes.data_as(C.POINTER(C.c_int64)), len(pT),
                                _p(pT), _p(pT_w), len(phi), _p(phi), _p(phi_w), len(y), _p(y), _p(dN)))

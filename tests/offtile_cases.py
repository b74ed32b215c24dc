"""The off-tile cases of operation 0 (cf_spacetime.hip, cf_spacetime_feqmod.hip, cf_spacetime_vah.hip), the spin polarization
(cf_polzn.hip) and the decay feed-down (cf_decays.hip): a fixed table of small named shapes, each chosen to reach one branch that the shipped
32 x 24 x 21 | 241 grid never reaches -- padded pT lanes (npT below its power of two npTp, npTp = 1 and 64), the last phi tile's clamped
copies, padded y / eta rows, partly filled workgroups (lane-wave counts that are no multiple of 4), the 2+1D LDS bound, and interpolation on
non-uniform and two-node grids; for anisotropic hydro also dead row blocks and more than one cell per chunk.  tests/test_offtile_cases.py
checks the table and its references on the CPU, tests/test_gpu_offtile.py and tests/test_gpu_spacetime_vah_offtile.py run it on the GPU.

Grids (make_grid): pT sorted random in [0.05, 3] GeV, phi sorted random in [0, 2 pi), y sorted random in [-2, 2], eta uniform in
[-2.5, 2.5] with trapezoid weights, pT_w and phi_w random in [0.5, 1.5] (a weight read at the wrong index shows; constant weights would
hide it).  The ranges keep every value far from the denormal tail: the cases test layout, not underflow.
Shapes are written (npT, n_phi, n_y | n_eta)."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from is3d_amd import inputs, synth


def make_grid(npT, nphi, ny, neta, seed):
    rng = np.random.default_rng(seed)
    pT = np.sort(rng.uniform(0.05, 3.0, npT))
    phi = np.sort(rng.uniform(0.0, 2.0 * np.pi, nphi))
    y = np.sort(rng.uniform(-2.0, 2.0, ny))
    pT_w, phi_w = rng.uniform(0.5, 1.5, npT), rng.uniform(0.5, 1.5, nphi)
    eta = np.linspace(-2.5, 2.5, neta)
    eta_w = np.full(neta, eta[1] - eta[0])
    eta_w[[0, -1]] *= 0.5
    return dict(pT=pT, phi=phi, y=y, eta=eta, eta_w=eta_w, pT_w=pT_w, phi_w=phi_w)


def plain(grid):
    """the grid without the reduction weights (what the plans and the spectra entries take)"""
    return {k: grid[k] for k in ("pT", "phi", "y", "eta", "eta_w")}


# ---- what the kernels derive from a shape (cf_spacetime_host.cpp: spacetime_setup, spacetime_check_grid; the plan's tile choice; cf_polzn.hip) ----
def npTp_of(npT):
    p = 1
    while p < npT:
        p *= 2
    return p


def n_classes(sp, baryon):
    """species classes: identical (mass, sign[, baryon number]) share one"""
    return len({(float(m), float(s), float(b) if baryon else 0.0) for m, s, b in zip(sp["mass"], sp["sign"], sp["baryon"])})


def nlw_of(ncls, npT):
    return (ncls * npTp_of(npT) + 63) // 64


def op0_tile(dim, npT, baryon, feqmod):
    """(phi tile width, row block) of the unit records operation 0 runs on: 3+1D 8 x 7, or 6 x 7 with baryon slots on a pT grid of more
    than 32 values (no E2 table stream there); 2+1D 8 x 31"""
    if dim == 2:
        return 8, 31
    return (6 if (baryon and npT > 32 and not feqmod) else 8), 7


def op0_lds_max_eta(npT, feqmod):
    """the largest 2+1D eta count of spacetime_check_grid: 4 waves x (64 / npTp) classes x K doubles within 64 KiB (feqmod: 48 KiB)"""
    return ((48 if feqmod else 64) * 1024) // (8 * 4 * (64 // npTp_of(npT)))


POLZN_TILE = {3: (4, 3), 2: (8, 1)}   # kPolznJT3 x kPolznKT3, kPolznJT2


def polzn_chunks(ncls, npT, nphi, nk, dim, n):
    """cf_polzn.hip::polzn_chunks without the workspace cap (16 GiB: far away)"""
    jt, kt = POLZN_TILE[dim]
    waves = nlw_of(ncls, npT) * ((nphi + jt - 1) // jt) * (((nk + kt - 1) // kt) if dim == 3 else 1)
    return min(max(1, (8192 + waves - 1) // waves), max(1, n // 256), 64)


# ---- operation 0 ----
PAIR = [211, -211, 321, 2212, -2212]           # pi+ / pi- and p / pbar share a class (without baryon slots): 3 classes
TWO = [211, 2212]
THREE = [211, 321, 2212]
FIVE = [211, 321, 2212, 3122, 3312]
EIGHT = [211, 321, 2212, -2212, 3122, -3122, 3312, 111]   # 6 classes
BARYON3 = [211, 2212, -2212]                   # 3 classes with baryon slots

Op0 = namedtuple("Op0", "name dim shape df_mode species n_cells opts breakdown")
SIGNED = dict(outflow=0, regulate_deltaf=0)
BAR = dict(include_baryon=1, include_baryondiff_deltaf=1)

OP0_DF = [
    # 3+1D (npT, n_phi, n_y)
    Op0("3d-npT1-phi5-y6-pair-1cell", 3, (1, 5, 6), 1, PAIR, 1, {}, False),
    Op0("3d-npT3-phi7-y8-2cells-3chunks", 3, (3, 7, 8), 2, EIGHT, 2, dict(cell_chunks=3), False),
    Op0("3d-npT5-phi9-y15-signed-5chunks", 3, (5, 9, 15), 1, THREE, 37, dict(SIGNED, cell_chunks=5), False),
    Op0("3d-npT33-phi13-y1-nlw5", 3, (33, 13, 1), 2, FIVE, 37, {}, False),
    Op0("3d-npT64-phi1-y6-nlw2", 3, (64, 1, 6), 1, TWO, 2, {}, False),
    Op0("3d-npT33-phi5-y8-baryon-6wide-nlw3", 3, (33, 5, 8), 1, BARYON3, 37, dict(BAR), False),
    Op0("3d-npT5-phi13-y15-baryon", 3, (5, 13, 15), 2, PAIR, 2, dict(BAR), False),
    # 2+1D (npT, n_phi | n_eta)
    Op0("2d-npT1-phi5-eta2-pair-1cell", 2, (1, 5, 2), 1, PAIR, 1, {}, False),
    Op0("2d-npT3-phi7-eta30-2cells-3chunks", 2, (3, 7, 30), 2, EIGHT, 2, dict(cell_chunks=3), False),
    Op0("2d-npT5-phi9-eta241", 2, (5, 9, 241), 1, THREE, 2, {}, False),
    Op0("2d-npT33-phi13-eta32-nlw5", 2, (33, 13, 32), 2, FIVE, 37, {}, False),
    Op0("2d-npT64-phi1-eta33-signed-nlw2-5chunks", 2, (64, 1, 33), 1, TWO, 37, dict(SIGNED, cell_chunks=5), False),
    Op0("2d-npT5-phi5-eta62-baryon", 2, (5, 5, 62), 1, PAIR, 2, dict(BAR), False),
    Op0("2d-npT3-phi13-eta63-baryon", 2, (3, 13, 63), 2, BARYON3, 37, dict(BAR), False),
    # the largest eta count the LDS bound admits
    Op0("2d-npT1-phi3-eta%d-lds-max" % op0_lds_max_eta(1, False), 2, (1, 3, op0_lds_max_eta(1, False)), 2, THREE, 2, {}, False),
    Op0("2d-npT2-phi3-eta%d-lds-max" % op0_lds_max_eta(2, False), 2, (2, 3, op0_lds_max_eta(2, False)), 1, THREE, 2, {}, False),
]

OP0_FQ = [
    Op0("3d-npT1-phi7-y15-pair", 3, (1, 7, 15), 4, PAIR, 37, {}, False),
    Op0("3d-npT3-phi13-y1-breakdown-3chunks", 3, (3, 13, 1), 3, EIGHT, 2, dict(cell_chunks=3), True),
    Op0("3d-npT33-phi5-y6-nlw5-5chunks", 3, (33, 5, 6), 4, FIVE, 37, dict(cell_chunks=5), False),
    Op0("3d-npT64-phi9-y8-breakdown-signed-nlw2", 3, (64, 9, 8), 3, TWO, 37, dict(SIGNED), True),
    Op0("3d-npT5-phi1-y8-1cell", 3, (5, 1, 8), 4, TWO, 1, {}, False),
    Op0("2d-npT1-phi7-eta2-pair", 2, (1, 7, 2), 4, PAIR, 2, {}, False),
    Op0("2d-npT3-phi9-eta33-breakdown", 2, (3, 9, 33), 3, EIGHT, 37, {}, True),
    Op0("2d-npT33-phi5-eta62-nlw5-5chunks", 2, (33, 5, 62), 4, FIVE, 37, dict(cell_chunks=5), False),
    Op0("2d-npT64-phi13-eta63-breakdown-nlw3-3chunks", 2, (64, 13, 63), 3, THREE, 2, dict(cell_chunks=3), True),
    Op0("2d-npT5-phi1-eta32-signed-1cell", 2, (5, 1, 32), 4, TWO, 1, dict(SIGNED), False),
    # a request for the 61-row tiles: the shipped library maps it onto the 8 x 31 records operation 0 supports
    Op0("2d-npT5-phi5-eta30-variant2", 2, (5, 5, 30), 3, THREE, 2, dict(kernel_variant=2), False),
    Op0("2d-npT1-phi3-eta%d-lds-max" % op0_lds_max_eta(1, True), 2, (1, 3, op0_lds_max_eta(1, True)), 4, THREE, 2, {}, False),
    Op0("2d-npT2-phi3-eta%d-lds-max" % op0_lds_max_eta(2, True), 2, (2, 3, op0_lds_max_eta(2, True)), 3, THREE, 2, {}, True),
]

# refused by spacetime_check_grid before a plan exists: (name, dim, shape, df_mode)
OP0_REFUSED = [
    ("2d-npT1-eta%d-df" % (op0_lds_max_eta(1, False) + 1), 2, (1, 3, op0_lds_max_eta(1, False) + 1), 1),
    ("2d-npT2-eta%d-df" % (op0_lds_max_eta(2, False) + 1), 2, (2, 3, op0_lds_max_eta(2, False) + 1), 2),
    ("2d-npT1-eta%d-feqmod" % (op0_lds_max_eta(1, True) + 1), 2, (1, 3, op0_lds_max_eta(1, True) + 1), 4),
    ("2d-npT2-eta%d-feqmod" % (op0_lds_max_eta(2, True) + 1), 2, (2, 3, op0_lds_max_eta(2, True) + 1), 3),
    ("3d-npT65-df", 3, (65, 3, 2), 1),
    ("2d-npT65-df", 2, (65, 3, 5), 2),
    ("3d-npT65-feqmod", 3, (65, 3, 2), 4),
]


def _seed(name):
    return 1000 + sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 9000


def bins_for(cells):
    """test_gpu_spacetime.surface_bins (bins narrower than the surface: some cells fall outside), kept valid for one or two cells"""
    r = np.sqrt(cells["x"] ** 2 + cells["y"] ** 2)
    tau_min = float(cells["tau"].min()) - 0.01
    return dict(tau_min=tau_min, tau_max=max(float(cells["tau"].max()) * 0.9, tau_min + 0.25), tau_bins=7, r_min=0.0,
                r_max=max(float(r.max()) * 0.8, 0.5), r_bins=5)


@lru_cache(maxsize=None)
def _df(baryon):
    return inputs.df_tables_full() if baryon else inputs.df_tables()


def op0_inputs(dim, shape, df_mode, species, n_cells, opts, breakdown, seed):
    npT, nphi, nk = shape
    g = make_grid(npT, nphi, nk if dim == 3 else 3, nk if dim == 2 else 3, seed)
    baryon = int(opts.get("include_baryon", 0))
    cells = synth.synth_surface(n_cells, dim, seed=seed + 1, baryon=bool(baryon))
    cells = {k: v.copy() for k, v in cells.items()}
    if dim == 3:
        cells["eta"] *= 0.5   # inside the y grid's range
    if breakdown:
        cells["bulkPi"][::7] = -5.0 * cells["P"][::7]   # df_mode 3: the linearised delta-f (cf_st_fq_linear)
    o = dict(dimension=dim, df_mode=df_mode, **opts)
    fq = inputs.feqmod_tables(inputs.surface_average_T(cells)) if df_mode >= 3 else None
    return dict(cells=cells, sp=inputs.species(species), grid=g, df=_df(baryon), opts=o, bins=bins_for(cells), fq=fq)


def build_op0(case):
    return op0_inputs(case.dim, case.shape, case.df_mode, case.species, case.n_cells, case.opts, case.breakdown, _seed(case.name))


def op0_derived(case):
    """npTp, nlw, (phi remainder, phi tile width), (row remainder, row block) of a case"""
    npT, nphi, nk = case.shape
    baryon = int(case.opts.get("include_baryon", 0))
    jt, r = op0_tile(case.dim, npT, baryon, case.df_mode >= 3)
    return dict(npTp=npTp_of(npT), nlw=nlw_of(n_classes(inputs.species(case.species), baryon), npT), phi=(nphi % jt, jt), rows=(nk % r, r))


# ---- operation 0 for anisotropic hydro (cf_spacetime_vah.hip; host side: cf_vah.hip on cf_spacetime_host.cpp's grid check, setup and chunk rule) ----
VAH_TILE = {3: (8, 7), 2: (8, 31)}   # (phi tile, row block) of the "F" unit records the per-cell kernel reads


def vah_lds_max_eta(npT):
    """the largest 2+1D eta count of spacetime_check_grid for this path: 4 waves x (64 / npTp) classes x K doubles within 64 KiB"""
    return (64 * 1024) // (8 * 4 * (64 // npTp_of(npT)))


def vah_record_doubles(dim):
    """REC of an "F" unit record: 4 header values per phi column, then per row 4 (3+1D) / 6 (2+1D) scalars and the tile's columns"""
    jt, r = VAH_TILE[dim]
    return 4 * jt + r * ((4 if dim == 3 else 6) + jt)


def vah_pass_cells(ncls, nphi, nk, n, dim, workspace_bytes):
    """cells per pass of spacetime_setup: the plan's record stream plus D (8 bytes per class and cell) within opts.workspace_bytes; without that
    option the cap is 16 GiB or more, which every surface here fits into"""
    if not workspace_bytes:
        return n
    jt, r = VAH_TILE[dim]
    stream = 8 * ((nphi + jt - 1) // jt) * ((nk + r - 1) // r) * vah_record_doubles(dim)
    return max(1, min(n, workspace_bytes // stream, workspace_bytes // (stream + 8 * ncls)))


def vah_chunk_bounds(ncls, npT, n, dim, K):
    """[(c0, c1)] of every chunk (one workgroup column) of a pass of n cells: is3d_vah_plan_execute_spacetime's nch -- at most 16384 // G
    chunks, G = ceil(nlw / 4) workgroups per chunk, in 2+1D also the 256 MiB cap of the eta slab -- and cf_st_vah_cells' c0 / c1.
    opts.cell_chunks is not read on this path."""
    G = (nlw_of(ncls, npT) + 3) // 4
    nch = min(n, max(1, 16384 // G))
    if dim == 2:
        nch = max(1, min(nch, (256 << 20) // (8 * ncls * K)))
    return [((ch * n) // nch, ((ch + 1) * n) // nch) for ch in range(nch)]


def vah_cells_per_chunk(ncls, npT, n, dim, K):
    """the chunk sizes that occur in a pass of n cells, ascending"""
    return sorted({c1 - c0 for c0, c1 in vah_chunk_bounds(ncls, npT, n, dim, K)})


# grid: "random" make_grid | "dead-y" 7 y nodes in [-1, 1] then 7 in [9, 10] (3+1D: the second row block is dead at unit level) |
# "dead-eta" a uniform eta table on [-16, 16] (2+1D, 124 nodes: blocks 0 and 3 dead at unit level, blocks 1 and 2 hold dead and live rows).
# species: a list of the table above, or "classes" -- one species of each (mass, sign) class of the urqmd list.
# tab: the coefficients come from the VAH tables (else from the cells).  workspace: opts.workspace_bytes (0: the default).
Op0Vah = namedtuple("Op0Vah", "name dim shape species n_cells opts tab workspace grid")
VAH_MANY = 1000   # cells of the many-cell cases: more than the 862 chunks of 75 classes x 64 lane slots, so chunks of 1 and of 2 cells
UNREG = dict(regulate_deltaf=0)


def _vah(name, dim, shape, species, n_cells, opts=None, tab=False, workspace=0, grid="random"):
    return Op0Vah(name, dim, shape, species, n_cells, opts or {}, tab, workspace, grid)


OP0_VAH = [
    # 3+1D (npT, n_phi, n_y)
    _vah("3d-npT1-phi5-y6-pair-1cell", 3, (1, 5, 6), PAIR, 1, tab=True),
    _vah("3d-npT3-phi7-y8-unregulated", 3, (3, 7, 8), EIGHT, 2, UNREG),
    _vah("3d-npT5-phi9-y15-passes", 3, (5, 9, 15), THREE, 37, tab=True, workspace=100000),
    _vah("3d-npT33-phi13-y1-nlw5", 3, (33, 13, 1), FIVE, 37),
    _vah("3d-npT64-phi1-y7-nlw2-full-block", 3, (64, 1, 7), TWO, 2, tab=True),
    _vah("3d-npT5-phi5-y14-dead-rows", 3, (5, 5, 14), EIGHT, 37, grid="dead-y"),
    # 2+1D (npT, n_phi | n_eta)
    _vah("2d-npT1-phi5-eta2-pair-1cell", 2, (1, 5, 2), PAIR, 1),
    _vah("2d-npT1-phi3-eta%d-lds-max" % vah_lds_max_eta(1), 2, (1, 3, vah_lds_max_eta(1)), THREE, 2, tab=True),
    _vah("2d-npT2-phi3-eta%d-lds-max" % vah_lds_max_eta(2), 2, (2, 3, vah_lds_max_eta(2)), THREE, 2),
    _vah("2d-npT3-phi7-eta30-unregulated", 2, (3, 7, 30), EIGHT, 2, UNREG, tab=True),
    _vah("2d-npT5-phi9-eta31-full-block", 2, (5, 9, 31), THREE, 2),
    _vah("2d-npT33-phi13-eta32-nlw5-passes", 2, (33, 13, 32), FIVE, 37, tab=True, workspace=200000),
    _vah("2d-npT64-phi1-eta33-nlw2", 2, (64, 1, 33), TWO, 37),
    _vah("2d-npT5-phi5-eta62-pair-full-blocks", 2, (5, 5, 62), PAIR, 2, tab=True),
    _vah("2d-npT3-phi13-eta63", 2, (3, 13, 63), THREE, 37),
    _vah("2d-npT5-phi9-eta241", 2, (5, 9, 241), THREE, 2, tab=True),
    _vah("2d-npT5-phi5-eta124-dead-rows", 2, (5, 5, 124), EIGHT, 37, tab=True, grid="dead-eta"),
]

# more than one cell per chunk: 75 classes x 33 pT values (64 lane slots each) are nlw = 75 lane waves, G = 19, 862 chunks
OP0_VAH_MANY = [
    _vah("3d-npT33-phi3-y8-75classes-1000cells", 3, (33, 3, 8), "classes", VAH_MANY, tab=True),
    _vah("2d-npT33-phi1-eta33-75classes-1000cells", 2, (33, 1, 33), "classes", VAH_MANY),
]

# refused by spacetime_check_grid before a plan exists (the one-shot entry) or before anything is allocated (the plan entry): (name, dim, shape)
OP0_VAH_REFUSED = [
    ("2d-npT1-eta%d" % (vah_lds_max_eta(1) + 1), 2, (1, 3, vah_lds_max_eta(1) + 1)),
    ("2d-npT2-eta%d" % (vah_lds_max_eta(2) + 1), 2, (2, 3, vah_lds_max_eta(2) + 1)),
    ("3d-npT65", 3, (65, 3, 2)),
    ("2d-npT65", 2, (65, 3, 5)),
]

VAH_DEAD_Y_NEAR = 7   # "dead-y": the first 7 y nodes are near the cells, the other 7 far
VAH_COEF = ("c0", "c1", "c2", "c3", "c4")


def vah_species(which):
    if which != "classes":
        return inputs.species(which)
    sp = inputs.species("urqmd")
    first = {}
    for i, key in enumerate(zip(sp["mass"], sp["sign"])):
        first.setdefault(key, i)
    idx = sorted(first.values())
    return {k: v[idx] for k, v in sp.items()}


def vah_n_classes(sp):
    """the (mass, sign) classes of a VAH plan (cf_vah.hip: no baryon slots on this path)"""
    return n_classes(sp, 0)


def vah_grid(case):
    npT, nphi, nk = case.shape
    seed = _seed(case.name)
    g = make_grid(npT, nphi, nk if case.dim == 3 else 3, nk if case.dim == 2 else 3, seed)
    rng = np.random.default_rng(seed + 7)
    if case.grid == "dead-y":
        near, far = rng.uniform(-1.0, 1.0, VAH_DEAD_Y_NEAR), rng.uniform(9.0, 10.0, nk - VAH_DEAD_Y_NEAR)
        g["y"] = np.concatenate([np.sort(near), np.sort(far)])
    elif case.grid == "dead-eta":
        g["eta"] = np.linspace(-16.0, 16.0, nk)
        g["eta_w"] = np.full(nk, g["eta"][1] - g["eta"][0])
        g["eta_w"][[0, -1]] *= 0.5
    return g


def vah_uds(cells):
    ut = np.sqrt(1.0 + cells["ux"] ** 2 + cells["uy"] ** 2 + cells["tau"] ** 2 * cells["un"] ** 2)
    return ut * cells["dat"] + cells["ux"] * cells["dax"] + cells["uy"] * cells["day"] + cells["un"] * cells["dan"]


def build_op0_vah(case):
    """cells (c0..c4 from the VAH tables through the oracle's interpolation: what the reference routes read), species, grid, bins, opts, tab
    (the tables the library is given, or None: it then reads the cells' c0..c4) and neg, the cell whose dat is negated (None: a one-cell case)"""
    from oracle import oracle
    seed = _seed(case.name)
    cells = {k: v.copy() for k, v in synth.synth_vah_surface(case.n_cells, case.dim, seed=seed + 1).items()}
    if case.dim == 3:
        cells["eta"] *= 0.5   # inside the y grid's range
    neg = None
    if case.n_cells > 1:
        # u.dsigma < 0, which this path must not skip: the cell whose time-like term leads by most, so that negating dat flips the sign
        ut = np.sqrt(1.0 + cells["ux"] ** 2 + cells["uy"] ** 2 + cells["tau"] ** 2 * cells["un"] ** 2)
        space = cells["ux"] * cells["dax"] + cells["uy"] * cells["day"] + cells["un"] * cells["dan"]
        neg = int(np.argmax(ut * cells["dat"] - np.abs(space)))
        cells["dat"][neg] *= -1.0
    tab = inputs.vah_df_tables()
    coef, found = oracle.vah_coefficients(tab, cells["Lambda"], cells["aL"])
    cells.update(coef)
    o = dict(dimension=case.dim, **case.opts)
    if case.workspace:
        o["workspace_bytes"] = case.workspace
    return dict(cells=cells, found=found, sp=vah_species(case.species), grid=vah_grid(case), bins=bins_for(cells), opts=o,
                tab=tab if case.tab else None, neg=neg)


def vah_derived(case):
    """npTp, ncls, nlw, (phi remainder, tile), (row remainder, block), the cells per pass and the chunk sizes of a full pass and of the last"""
    npT, nphi, nk = case.shape
    jt, r = VAH_TILE[case.dim]
    ncls = vah_n_classes(vah_species(case.species))
    pc = vah_pass_cells(ncls, nphi, nk, case.n_cells, case.dim, case.workspace)
    sizes = set(vah_cells_per_chunk(ncls, npT, pc, case.dim, nk))
    if case.n_cells % pc:
        sizes |= set(vah_cells_per_chunk(ncls, npT, case.n_cells % pc, case.dim, nk))
    return dict(npTp=npTp_of(npT), ncls=ncls, nlw=nlw_of(ncls, npT), phi=(nphi % jt, jt), rows=(nk % r, r), pass_cells=pc,
                n_passes=(case.n_cells + pc - 1) // pc, chunk_sizes=sorted(sizes))


def vah_many_subset(case, neg):
    """the cells of a many-cell case that meet the per-cell oracle: both cells of every seventh two-cell chunk, the first and the last chunk
    and the negated cell (fewer than 150)"""
    npT, nphi, nk = case.shape
    ncls = vah_n_classes(vah_species(case.species))
    bounds = vah_chunk_bounds(ncls, npT, case.n_cells, case.dim, nk)
    two = [b for b in bounds if b[1] - b[0] == 2]
    pick = [bounds[0], bounds[-1]] + two[::7]
    cells = {c for c0, c1 in pick for c in range(c0, c1)} | {neg}
    return sorted(cells), two[::7]


def vah_dead_split(case, g):
    """(far, near) grids of a dead-row case: the rows no cell reaches (every exp(-E_a/Lambda) is +0 there) and the others.  2+1D: whole row
    blocks 0 and 3 against blocks 1 and 2; both parts start with two adjacent nodes, so eta[1] - eta[0] is the table's spacing in each."""
    if case.dim == 3:
        return dict(g, y=g["y"][VAH_DEAD_Y_NEAR:]), dict(g, y=g["y"][:VAH_DEAD_Y_NEAR])
    r = VAH_TILE[2][1]
    far = np.r_[0:r, 3 * r:4 * r]
    near = np.r_[r:3 * r]
    return dict(g, eta=g["eta"][far], eta_w=g["eta_w"][far]), dict(g, eta=g["eta"][near], eta_w=g["eta_w"][near])


def vah_eta_node_grid(g, k):
    """the two-node eta table [eta_k, eta_k + deta] with weights [w_k, 0]: the oracle's eta sum on it is node k's term of the sum on g"""
    deta = g["eta"][1] - g["eta"][0]
    return dict(g, eta=np.array([g["eta"][k], g["eta"][k] + deta]), eta_w=np.array([g["eta_w"][k], 0.0]))


def vah_eta_check_nodes(K):
    """node 0, the last node of each 31-row block, the first of the next, and K - 1"""
    r = VAH_TILE[2][1]
    return sorted({0, K - 1} | {k for b in range(r, K, r) for k in (b - 1, b)})


@lru_cache(maxsize=None)
def vah_reference(name):
    """(inputs, per-cell oracle values [S][n]) of a case of OP0_VAH, computed once and never written to"""
    from test_gpu_spacetime_vah import oracle_cells_vah
    case = next(c for c in OP0_VAH if c.name == name)
    b = build_op0_vah(case)
    ref = oracle_cells_vah(b["cells"], b["sp"], b["grid"], b["opts"])
    ref.setflags(write=False)
    return b, ref


@lru_cache(maxsize=None)
def vah_dead_eta_nodes(name, regulate=1, warm=1.0):
    """[K] bool of a 2+1D case: the eta nodes whose term of the oracle's eta sum is exactly 0 in every bin.  With regulate_deltaf = 0 those
    are the nodes where every exp(-E_a/Lambda) underflows; the regulated delta-f adds nodes next to them, where the exponentials that do
    not underflow meet a factor 1 + fbar delta-f clamped to 0.  warm: Lambda multiplied by it (E_a/Lambda divided)."""
    from oracle import oracle
    b, _ = vah_reference(name)
    K = len(b["grid"]["eta"])
    cells, o = dict(b["cells"], Lambda=warm * b["cells"]["Lambda"]), dict(b["opts"], regulate_deltaf=regulate)
    dead = np.array([np.all(oracle.dN_pTdpTdphidy_vah(cells, b["sp"], vah_eta_node_grid(b["grid"], k), o) == 0.0) for k in range(K)])
    dead.setflags(write=False)
    return dead


@lru_cache(maxsize=None)
def vah_many_reference(name):
    """(inputs, subset, its two-cell chunks, per-cell oracle values of the subset [S][len(subset)]) of a case of OP0_VAH_MANY"""
    from test_gpu_spacetime_vah import oracle_cells_vah
    case = next(c for c in OP0_VAH_MANY if c.name == name)
    b = build_op0_vah(case)
    subset, two = vah_many_subset(case, b["neg"])
    ref = oracle_cells_vah({k: v[subset] for k, v in b["cells"].items()}, b["sp"], b["grid"], b["opts"])
    ref.setflags(write=False)
    return b, subset, two, ref


# ---- mode 5 ----
Polzn = namedtuple("Polzn", "name dim shape n_cells kinds")
POLZN_MANY = 512   # the smallest cell count with more than one chunk (polzn_chunks: at least 256 cells per chunk)

POLZN = [
    Polzn("3d-npT1-phi5-y2-1cell", 3, (1, 5, 2), 1, (1, -1)),
    Polzn("3d-npT3-phi3-y4", 3, (3, 3, 4), POLZN_MANY, (1, -1)),
    Polzn("3d-npT33-phi9-y7", 3, (33, 9, 7), POLZN_MANY, (-1,)),
    Polzn("3d-npT64-phi1-y1-1cell", 3, (64, 1, 1), 1, (1,)),
    Polzn("2d-npT3-phi1-eta2-1cell", 2, (3, 1, 2), 1, (1, -1)),
    Polzn("2d-npT1-phi7-eta5", 2, (1, 7, 5), POLZN_MANY, (1, -1)),
    Polzn("2d-npT33-phi9-eta33", 2, (33, 9, 33), POLZN_MANY, (1,)),
]
POLZN_T = 0.1503


def build_polzn(case):
    from test_gpu_polarization import mixed_cells, pick_species
    npT, nphi, nk = case.shape
    seed = _seed(case.name)
    g = make_grid(npT, nphi, nk if case.dim == 3 else 3, nk if case.dim == 2 else 3, seed)
    sp = pick_species(3 if len(case.kinds) == 2 else 6, case.kinds)
    cells = mixed_cells(case.n_cells, case.dim, seed=seed + 1)
    w = synth.synth_vorticity(case.n_cells, seed=seed + 2)
    return dict(cells=cells, w=w, sp=sp, grid=plain(g), T=POLZN_T, dim=case.dim)


def polzn_derived(case):
    npT, nphi, nk = case.shape
    sp = build_polzn(case)["sp"]
    ncls = len({(float(m), float(s)) for m, s in zip(sp["mass"], sp["sign"])})
    jt, kt = POLZN_TILE[case.dim]
    return dict(npTp=npTp_of(npT), ncls=ncls, phi=(nphi % jt, jt), rows=(nk % kt, kt) if case.dim == 3 else (0, 1),
                chunks=polzn_chunks(ncls, npT, nphi, nk, case.dim, case.n_cells))


# ---- decay feed-down ----
DECAY_CHOSEN = [211, -211, 111, 321, -321, 311, 113, 223, 313, 333]   # test_gpu_decays.test_parity_3d_chain_and_3body
DECAY_PDG = "pdg-urqmd_v3.3+.dat"
Decay = namedtuple("Decay", "name dim shape y_ends")

DECAYS = [
    Decay("3d-7x5x4-nonuniform-y-1.3-to-0.9", 3, (7, 5, 4), (-1.3, 0.9)),
    Decay("3d-7x2x2-two-node-axes", 3, (7, 2, 2), (-0.7, 1.1)),   # (the last y node is Y_max: it must be above 0)
    Decay("2d-9x3", 2, (9, 3, 1), None),
]


def decay_grid(case):
    """make_grid with the top pT node at 3 GeV (the M_T fit of a parent takes the nodes above sqrt(1.73) M: 1.34 GeV for the phi(1020))"""
    npT, nphi, ny = case.shape
    g = make_grid(npT, nphi, ny, 241, _seed(case.name))
    g["pT"][-1] = 3.0
    if case.y_ends:
        g["y"] = np.sort(np.random.default_rng(_seed(case.name) + 5).uniform(case.y_ends[0], case.y_ends[1], ny))
        g["y"][0], g["y"][-1] = case.y_ends
    fx = inputs.grid()
    g["eta"], g["eta_w"] = fx["eta"], fx["eta_w"]   # the thermal input's 2+1D eta table: the shipped one
    return g


def decay_surface(case):
    return synth.synth_surface(48 if case.dim == 2 else 24, case.dim, seed=_seed(case.name) + 1)


def decay_species(pdg, chosen=DECAY_CHOSEN):
    """the chosen list's species from api.pdg_read's dict"""
    ids = list(pdg["mc_id"])
    k = [ids.index(c) for c in chosen]
    return dict(mass=pdg["mass"][k], sign=pdg["sign"][k], degeneracy=pdg["gspin"][k], baryon=pdg["baryon"][k])


DECAY_OPTS = dict(df_mode=2)

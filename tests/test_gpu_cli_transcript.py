"""GPU (-m gpu): the run driver's stdout, line for line.  The other tests/test_gpu_cli*.py files check what a run writes and look for single
lines; this one holds the order of all of them: for one run of every stage (momentum spectra with delta-f and with modified equilibrium plus the
decay feed-down, spacetime distributions, the sampler writing its list and decaying it, the fused and the anisotropic-hydro binned samplers
sized by their mean yields, mode 5's polarization; the last two also on a spelled-out device list) stdout with every number replaced by "#"
equals the transcript in tests/golden/run_transcripts.json, and a second directory of the same contents gives the same result files byte for
byte.  Three input errors that are met while the inputs load keep their messages.

The golden is the output of commit e664bc7 (before the driver was split into parse_config / load_inputs / one routine per operation) on an
MI355X, in fresh directories -- so the surface is parsed from text -- with fixed seeds; `python tests/test_gpu_cli_transcript.py OUT.json`
records it from the build in the tree."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_transcripts.json")
IDS = [211, 321, 2212, -2212]
DECAY_IDS = [211, -211, 321, 113]            # a resonance and its daughters, for the two decay keys
N_CELLS = 37
NUMBER = re.compile(r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?")


def viscous_dir(root, reference, params, keys=(), ids=IDS, shipped_pdg=None, big_cells=False):
    import refformat
    from is3d_amd import synth
    dim = params.get("dimension", 3)
    cells = dict(synth.synth_surface(N_CELLS, dim, seed=300 + dim))
    if big_cells:                           # a sampler run on 37 cells: cells large enough to emit some hundred hadrons
        for k in ("dat", "dax", "day", "dan"):
            cells[k] = 200.0 * cells[k]
    refformat.make_run_dir(root, cells, ids, params)
    if shipped_pdg:                         # the shipped list: the toy one of make_run_dir has no usable decay data
        shutil.copy(os.path.join(reference, "PDG", shipped_pdg), os.path.join(root, "PDG", shipped_pdg))
    with open(os.path.join(root, "iS3D_parameters.dat"), "a") as f:       # the template of make_run_dir has no line for an optional key
        for k, v in keys:
            f.write("%s\t\t= %s\n" % (k, v))
    return root


def mode5_dir(root, reference):
    import refformat
    from is3d_amd import synth
    from test_polarization_io import write_mode5
    cells = synth.synth_surface(N_CELLS, 3, seed=811)
    refformat.make_run_dir(root, cells, IDS, dict(mode=5, dimension=3, operation=1, df_mode=2))
    write_mode5(os.path.join(root, "input", "surface.dat"), cells, synth.synth_vorticity(N_CELLS, seed=812))
    return root


def vah_dir(root, reference):
    import pathlib
    from test_gpu_cli_sampler_vah_bins import vah_run
    p = pathlib.Path(root)
    return vah_run(p.parent, p.name, 3, keys=(("vah_sampler", 1), ("vah_oversample", 1), ("vah_sampler_on_device", 1), ("min_num_hadrons", 2000.0)))


SAMPLER = dict(operation=2, dimension=3, df_mode=2, oversample=1, min_num_hadrons=2000, sampler_seed=17)
CASES = {
    "spectra-14-moment": lambda root, ref: viscous_dir(root, ref, dict(operation=1, dimension=3, df_mode=1)),
    "spectra-feqmod-decays": lambda root, ref: viscous_dir(root, ref, dict(operation=1, dimension=2, df_mode=3, hrg_eos=2),
                                                           (("do_resonance_decays", 1),), DECAY_IDS, "pdg_smash.dat"),
    "spacetime": lambda root, ref: viscous_dir(root, ref, dict(operation=0, dimension=3, df_mode=2)),
    "sampler-list-decayed": lambda root, ref: viscous_dir(root, ref, SAMPLER, (("decay_sampled_hadrons", 1),), DECAY_IDS, "pdg-urqmd_v3.3+.dat", True),
    "sampler-fused": lambda root, ref: viscous_dir(root, ref, dict(SAMPLER, test_sampler=1), (("test_sampler_fused", 1),), big_cells=True),
    "vah-sampler-binned": vah_dir,
    "mode-5": mode5_dir,
}
RUNS = [(name, "0") for name in CASES] + [("vah-sampler-binned", "0,0"), ("mode-5", "0,0")]


def run(root, devices):
    from is3d_amd import api
    return subprocess.run([api.CLI_PATH], cwd=root, capture_output=True, text=True, timeout=600, env=dict(os.environ, IS3D_DEVICES=devices))


def result_files(root):
    found = {}
    for d, _, names in os.walk(os.path.join(root, "results")):
        for n in names:
            path = os.path.join(d, n)
            found[os.path.relpath(path, root)] = open(path, "rb").read()
    return found


def transcript(stdout):
    return NUMBER.sub("#", stdout)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["stdout"]


@pytest.mark.parametrize("name,devices", RUNS, ids=["%s-on-%s" % r for r in RUNS])
def test_stdout_keeps_its_lines_and_their_order(tmp_path, reference, golden, name, devices):
    first, second = CASES[name](str(tmp_path / "first"), reference), CASES[name](str(tmp_path / "second"), reference)
    r1, r2 = run(first, devices), run(second, devices)
    assert r1.returncode == 0, r1.stdout[-3000:] + r1.stderr[-3000:]
    assert r2.returncode == 0, r2.stdout[-3000:] + r2.stderr[-3000:]
    assert transcript(r1.stdout) == golden["%s-on-%s" % (name, devices)]
    assert r1.stderr == ""
    files = result_files(first)
    assert len(files) >= 2 and all(files.values()) and files == result_files(second)


def _bad_chosen(root):
    with open(os.path.join(root, "PDG", "chosen_particles.dat"), "a") as f:
        f.write("\t9999999\n")


def _no_eta_table(root):
    os.remove(os.path.join(root, "tables", "eta", "eta_trapezoid_table_241pt.dat"))


def _empty_averages(root):
    # the run writes this file and the sampler reads it back: a link to the null device swallows the write, so the read-back meets an empty
    # file without any race against the run
    os.symlink(os.devnull, os.path.join(root, "average_thermodynamic_quantities.dat"))


@pytest.mark.parametrize("spoil,message", [
    (_bad_chosen, "iS3D-amd: chosen particle 9999999 is not in PDG/pdg-urqmd_v3.3+.dat\n"),
    (_no_eta_table, "operation 2 opens tables/eta/eta_trapezoid_table_41pt.dat (or tables/eta/eta_trapezoid_table_241pt.dat): neither can be read ("),
    (_empty_averages, "iS3D-amd: Error opening average thermodynamic file\n"),
], ids=["chosen-not-in-pdg", "no-eta-table", "empty-averages-file"])
def test_input_errors_keep_their_messages(tmp_path, reference, spoil, message):
    root = viscous_dir(str(tmp_path / "run"), reference, dict(SAMPLER, oversample=0), big_cells=True)
    spoil(root)
    r = run(root, "0")
    assert r.returncode == 1 and message in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stderr.count("\n") == 1 and "Goodbye" not in r.stdout
    assert not os.path.exists(os.path.join(root, "results", "particle_list_osc.dat"))


def record(out_path):
    """writes the golden from the build in the tree (run it on the commit the file is to describe, on the GPU); a run that fails is reported
    and ends the recording"""
    import pathlib
    import tempfile
    from conftest import unpack_reference_data
    got = {}
    with tempfile.TemporaryDirectory() as d:
        reference = unpack_reference_data(os.path.join(d, "reference"))
        for k, (name, devices) in enumerate(RUNS):
            root = CASES[name](str(pathlib.Path(d) / ("run%d" % k)), reference)
            r = run(root, devices)
            print("==== %s on %s: exit %d\n%s%s" % (name, devices, r.returncode, r.stdout, r.stderr), flush=True)
            if r.returncode != 0:
                return 1
            got["%s-on-%s" % (name, devices)] = transcript(r.stdout)
    with open(out_path, "w") as f:
        json.dump(dict(commit="e664bc7", stdout=got), f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.exit(record(sys.argv[1]))

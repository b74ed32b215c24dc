"""CPU: the register report of the 3+1D default kernel since round 13 -- cf_main_tile3e<.., SH8>, D'_j and gamma_j in SGPRs and one reciprocal
per row of 8 (is3d_amd/csrc/isa_counts.json, tools/count_isa.py; the plain cf_main_tile3e keys hold the round-5 form the developer build keeps)."""
import json
import os

from conftest import ROOT


def test_sh8_kernels_hold_their_register_budget():
    d = json.load(open(os.path.join(ROOT, "is3d_amd", "csrc", "isa_counts.json")))
    for ce in (0, 1):
        new = d["cf_main_tile3e_sh8:CE=%d,OUTFLOW=1,REG=1,JT=8,R=7,MODE=1" % ce]
        old = d["cf_main_tile3e:CE=%d,OUTFLOW=1,REG=1,JT=8,R=7,MODE=1" % ce]
        assert new["evals_counted_from_isa"] and new["evals_in_loop"] == 56 and new["evals_per_rcp"] == 8 == new["evals_per_rcp_template"]
        assert new["histogram"]["v_rcp_f64"] == 7 and old["histogram"]["v_rcp_f64"] == 14
        assert new["scratch_in_loop"] == 0 and new["scratch_in_kernel"] == 0 and new["scratch_bytes_per_lane"] == 0
        assert new["vgprs"] <= 256 and new["occupancy_waves_per_simd"] >= 2
        # no SGPR spill code in the counted loop (v_writelane / v_readlane beyond the four the round-5 form has for its wave votes)
        assert new["histogram"].get("v_writelane_b32", 0) == 0
        assert new["histogram"].get("v_readlane_b32", 0) <= old["histogram"].get("v_readlane_b32", 0)
        assert new["issue_cycles_per_eval"] < old["issue_cycles_per_eval"]

"""LightGlue's float64 forward (tests/lg_f64.py) pinned to the reference's own runs, and the oracle measured against it.  No GPU:
runs under -m "not gpu"."""
import json

import numpy as np
import pytest
import torch

import lg_f64
from helpers import (LGF64_PAIRS, Golden, close_and_record, la_bound, la_bound_f64, lg_inputs, lgf64_pair,
                     lgf64_shipped_state_dict, record_flips, state_dict_for)

LG = Golden("lg")
LGCAL = Golden("lgcal")
LGCFG = Golden("lgcfg")


def _lg_case(name):
    c = dict(LG.cases[name])
    sd = state_dict_for(dict(c, state_keys=json.loads(bytes(LG[f"{name}.state_keys"]).decode())))
    return c, sd


@pytest.mark.parametrize("name", ["d256", "d128", "full"])
def test_float64_forward_equals_the_reference_in_float64(name):
    """two float64 evaluations of the same model on the same inputs (lgcal.npz `lg.<name>.la_f64`, `full` stored every 37th row /
    41st column): equal to 1e-8"""
    c, sd = _lg_case(name)
    d0, d1, k0, k1 = lg_inputs(c)
    la = lg_f64.forward(sd, k0, d0, k1, d1)["log_assignment"]
    assert la.shape == (c["n"] + 1, c["m"] + 1)
    if name == "full":
        la = la[::37, ::41]
    close_and_record(f"lgf64.{name}.float64 vs reference in float64", la, LGCAL[f"lg.{name}.la_f64"], atol=1e-8)


@pytest.mark.parametrize("name", ["d256", "d128", "full"])
def test_float32_forward_equals_the_reference_fp32(name):
    c, sd = _lg_case(name)
    d0, d1, k0, k1 = lg_inputs(c)
    r = lg_f64.forward(sd, k0, d0, k1, d1, dtype=torch.float32)
    la = r["log_assignment"]
    if f"{name}.la" in LG:
        close_and_record(f"lgf64.{name}.float32 vs reference", la, LG[f"{name}.la"][0], atol=la_bound(f"lg.{name}"))
    else:
        close_and_record(f"lgf64.{name}.float32 vs reference", la[::37, ::41], LG[f"{name}.la_probe"], atol=la_bound(f"lg.{name}"))
    assert record_flips(f"lgf64.{name}.float32 matches0 vs reference", r["matches0"], LG[f"{name}.matches0"]) == 0
    assert record_flips(f"lgf64.{name}.float32 matches1 vs reference", r["matches1"], LG[f"{name}.matches1"]) == 0


@pytest.mark.parametrize("name", list(LGCFG.cases))
def test_float32_forward_equals_the_reference_fp32_other_widths(name):
    """every lgcfg width / head count / layer count / input_proj: the restatement is the reference's model"""
    c = LGCFG.cases[name]
    sd = state_dict_for(dict(c, state_keys=json.loads(bytes(LGCFG[f"{name}.state_keys"]).decode())))
    d0, d1, k0, k1 = lg_inputs(c)
    r = lg_f64.forward(sd, k0, d0, k1, d1, dtype=torch.float32)
    assert len(r["layers"]) == c["n_layers"] and r["layers"][-1][0].shape == (c["n"], c["descriptor_dim"])
    close_and_record(f"lgf64.lgcfg.{name}.float32 vs reference", r["log_assignment"], LGCFG[f"{name}.la"][0],
                     atol=la_bound(f"lgcfg.{name}"))
    assert record_flips(f"lgf64.lgcfg.{name}.float32 matches0 vs reference", r["matches0"], LGCFG[f"{name}.matches0"]) == 0
    assert record_flips(f"lgf64.lgcfg.{name}.float32 matches1 vs reference", r["matches1"], LGCFG[f"{name}.matches1"]) == 0


def test_filter_decision_follows_the_fp32_rule():
    """exp of the row maximum in fp32: kept through the subnormal band below -87.3, dropped once it rounds to 0 (about -103.97)"""
    la = torch.full((5, 5), -200.0, dtype=torch.float64)  # [n+1, m+1]: 4 x 4 and the dustbins
    for i, v in enumerate((-87.0, -95.0, -103.9, -104.1)):
        la[i, i] = v
    m0, m1, s0, _, _ = lg_f64.filter_matches(la, 0.0)
    assert m0[:3].tolist() == [0, 1, 2] and m0[3] == -1 and m1.tolist() == m0.tolist()
    assert s0[3] > 0  # the float64 score itself does not underflow: only the decision is fp32


SINGLE = [f"{n}x{m}" for n, m in LGF64_PAIRS]


@pytest.mark.parametrize("shape", SINGLE)
def test_oracle_and_float32_vs_float64_on_single_pairs(oracle, shape):
    """the two fp32 peers on the GPU sweep's single-pair shapes (tests/test_lightglue_f64_gpu.py): each within the f64 bound the
    GPU is held to -- which the larger of the two sets -- and the oracle's assignments equal to the float64 ones outside the
    near-tie / filter-edge rows"""
    n, m = map(int, shape.split("x"))
    sd = lgf64_shipped_state_dict(801)
    d0, d1, k0, k1 = lgf64_pair(8000 + n + 7 * m, n, m)
    ex = lg_f64.forward(sd, k0, d0, k1, d1)
    f32 = lg_f64.forward(sd, k0, d0, k1, d1, dtype=torch.float32)
    orc = oracle.lightglue(sd, k0, d0, k1, d1, capture_layers=range(9))
    la = ex["log_assignment"]
    e_orc = float(np.abs(orc["log_assignment"] - la).max())
    e_f32 = float(np.abs(f32["log_assignment"] - la).max())
    bound = la_bound_f64([e_orc, e_f32], np.abs(la).max())
    tag = f"lgf64.single.{shape}"
    close_and_record(f"{tag}.log_assignment oracle vs float64", orc["log_assignment"], la, atol=bound)
    close_and_record(f"{tag}.log_assignment float32 vs float64", f32["log_assignment"], la, atol=bound)
    for i in range(9):
        for s in range(2):
            x = ex["layers"][i][s]
            np.testing.assert_allclose(orc["layers"][i][s], x, atol=la_bound_f64([np.abs(orc["layers"][i][s] - x).max(),
                                                                                np.abs(f32["layers"][i][s] - x).max()], np.abs(x).max()))
    allow = (ex["row_gap"] < bound) | (ex["edge_dist"] < bound)
    bad = np.nonzero(orc["matches0"] != ex["matches0"])[0]
    record_flips(f"{tag}.matches0 oracle vs float64", orc["matches0"], ex["matches0"], la)
    assert all(allow[i] or ex["col_gap"][max(orc["matches0"][i], ex["matches0"][i])] < bound for i in bad), bad

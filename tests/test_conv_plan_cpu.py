"""CPU-only: the conv dispatcher's selection (einx_conv_plan: the selection code of einx_conv_block without the launch) against the
coverage table tests/conv_plan_cases.py.  Every instantiation the dispatcher can name has a case (the GPU suite runs each of them
bit for bit: test_conv_gpu.py::test_every_conv_instantiation_bit_exact), and every case selects the kernel it says it does."""
import itertools
import re

import pytest

from conv_plan_cases import CONV_PLAN_CASES, CONV_PLAN_NAMES, case_id, plan_args, plan_name
from helpers import ROOT, load_pkg

pkg = load_pkg()
L = pkg.native.lib()

NET_MAPS = [(264, 352), (132, 176), (66, 88), (33, 44), (260, 346)]
SMALL = [1, 2, 3, 4, 5, 8, 11, 12, 13, 16, 22, 24, 31, 32, 33, 47, 64, 96]
SWEEP_B = [1, 2, 3, 8, 32, 64, 256, 384]
SWEEP_CIN = [1, 2, 5, 6, 7, 8, 12, 16, 20, 32, 64, 128, 256]
SWEEP_COUT = [1, 7, 64, 65, 128, 130, 256]


@pytest.mark.parametrize("case", CONV_PLAN_CASES, ids=case_id)
def test_case_plans_to_its_name_within_the_size_limit(case):
    B, cin, cout, H, W, ks, _relu, _bn, pool, fold, name = case
    assert plan_name(L, *plan_args(case)) == name
    Hs, Ws = (fold[2], fold[3]) if fold else (H, W)
    if fold:  # padding on every side, inside the logical map
        assert fold[0] > 0 and fold[1] > 0 and fold[0] + Hs < H and fold[1] + Ws < W
    Ho, Wo = (H // 2, W // 2) if pool else (H, W)
    assert 4 * B * (cin * Hs * Ws + cout * Ho * Wo) <= 64 << 20


def _sweep_names():
    seen = set()
    maps = NET_MAPS + list(itertools.product(SMALL, SMALL))
    for B, cin, cout, (H, W), ks, pool, fold in itertools.product(SWEEP_B, SWEEP_CIN, SWEEP_COUT, maps, (1, 3), (0, 1), (0, 1)):
        if ks == 1 and (pool or fold):
            continue  # refused by einx_conv_block
        if pool and (H % 2 or W % 2):
            continue
        h0, w0, Hs, Ws = (1, 2, H - 3, W - 3) if fold else (0, 0, H, W)
        if Hs < 1 or Ws < 1:
            continue
        name = plan_name(L, cin, cout, ks, pool, B, Hs, Ws, h0, w0, H, W)
        if name is not None:
            seen.add(name)
    return seen


@pytest.fixture(scope="module")
def sweep_names():
    return _sweep_names()


def test_every_name_the_sweep_reaches_has_a_case(sweep_names):
    """B x cin x cout x map x ks x pool x fold through the plan query (nothing launches): a name outside the table is an
    instantiation without a test."""
    missing = sorted(sweep_names - set(CONV_PLAN_NAMES))
    assert not missing, f"instantiations without a row in tests/conv_plan_cases.py: {missing}"


def test_every_table_name_is_reached(sweep_names):
    own = {plan_name(L, *plan_args(c)) for c in CONV_PLAN_CASES}
    assert set(CONV_PLAN_NAMES) <= sweep_names | own
    # the table covers the whole sweep and nothing else: a row whose kernel the dispatcher no longer selects is stale
    assert set(CONV_PLAN_NAMES) == own


def test_every_instantiation_named_in_the_source_is_in_the_table():
    """The dispatcher's list of conv_block_kernel variants (EINX_CONV_BLOCK_VARIANTS) and its three other kernels, read from
    conv.hip: each one is a name of the table, so none of them is dead code and none lacks a case."""
    import os
    src = open(os.path.join(ROOT, pkg.__name__, "csrc", "conv.hip")).read()
    rows = re.findall(r"^\s*X\(CB_\w+,\s*([^)]*)\)", src, flags=re.M)
    assert rows, "EINX_CONV_BLOCK_VARIANTS not found in conv.hip"
    names = set()
    for r in rows:
        f = [v.strip() for v in r.split(",")]
        names.add(f"conv_block_kernel<{','.join(f[:9])}>")
        if f[9] == "true":
            names.add(f"conv_block_kernel<{','.join(f[:9])}> (3 per CU)")
    names.add("conv_block_kernel<1,1,128,1,4,2,1,32,false,xtra>")
    names |= {f"conv16_1x1_kernel<{n}>" for n in (1, 2, 4)}
    names |= {f"conv16_kernel<{p},8,{n}>" for p in ("true", "false") for n in (1, 2, 4)}
    assert names == set(CONV_PLAN_NAMES), names ^ set(CONV_PLAN_NAMES)


def test_plan_refuses_what_the_dispatcher_refuses():
    assert plan_name(L, 8, 8, 2, 0, 1, 8, 8, 0, 0, 8, 8) is None   # kernel size
    assert plan_name(L, 8, 8, 3, 1, 1, 7, 8, 0, 0, 7, 8) is None   # pooling an odd map
    assert plan_name(L, 8, 8, 1, 1, 1, 8, 8, 0, 0, 8, 8) is None   # pooled 1x1
    assert plan_name(L, 8, 8, 1, 0, 1, 7, 8, 1, 0, 8, 8) is None   # folded 1x1
    assert plan_name(L, 8, 8, 3, 0, 0, 8, 8, 0, 0, 8, 8) is None   # empty batch
    assert plan_name(L, 1 << 12, 8, 3, 0, 1, 512, 512, 0, 0, 512, 512) is None  # 2^30 elements per image
    assert plan_name(L, 8, 8, 3, 0, 1, 8, 8, 0, 0, 8, 8) == "conv16_kernel<false,8,1>"


def _network_layers(ext, B, H, W):
    """(cin, cout, ks, pool, B, Hs, Ws, h0, w0, H, W) of every einx_conv_block call einx_extract can make for this extractor: the
    backbone (replicate padding folded into the first layer), both heads, and at B = 1 the two heads' first layers as one."""
    w0, w1, h0, h1 = pkg.native.padder_pads(H, W, ext.cell_size)
    h, w = H + h0 + h1, W + w0 + w1
    bb, det, desc = ext._stacks()
    out = []
    for i, (block, pool) in enumerate(bb):
        conv = ext._spec(block)[0]
        ks = conv.kernel_size[0]
        out.append((conv.in_channels, conv.out_channels, ks, int(pool), B) + ((H, W, h0, w0) if i == 0 else (h, w, 0, 0)) + (h, w))
        if pool:
            h, w = h // 2, w // 2
    for head in (det, desc):
        for block in head:
            conv = ext._spec(block)[0]
            out.append((conv.in_channels, conv.out_channels, conv.kernel_size[0], 0, B, h, w, 0, 0, h, w))
    if B == 1 and len(det) == 2 and len(desc) == 2:
        a, b = ext._spec(det[0])[0], ext._spec(desc[0])[0]
        out.append((a.in_channels, a.out_channels + b.out_channels, a.kernel_size[0], 0, B, h, w, 0, 0, h, w))
    return out


@pytest.mark.parametrize("cfg_name,bench_batch", [("SP_MNN", 32), ("SP_LG", 64), ("SiLK_MNN", 32)])
def test_shipped_networks_run_only_tabled_instantiations(cfg_name, bench_batch):
    """The layer lists of the shipped configurations (event and image extractor: backbone and both heads) at a single pair and at
    the benchmark's batch, 346x260 inputs: every kernel they would launch has a case in the table."""
    model = pkg.EIM(pkg.default_config(cfg_name, event_channels=5), device="cpu")
    planned = {}
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        for B in (1, bench_batch):
            layers = _network_layers(ext, B, 260, 346)
            assert len(layers) >= 10
            for a in layers:
                name = plan_name(L, *a)
                assert name is not None, a
                planned.setdefault(name, a)
    missing = {n: a for n, a in planned.items() if n not in CONV_PLAN_NAMES}
    assert not missing, missing
    assert len(planned) >= 4

"""Shared fixtures-as-functions of the GPU test modules (test_*_gpu.py): device helpers, golden files, model builders, oracle
runners.  Not collected by pytest (no test_ prefix); the component modules import what they use by name."""
import numpy as np
import pytest
import torch
import json
import os
import sys
import statistics
import subprocess
import time
from importlib import import_module

from helpers import (GOLDEN, Golden, close_and_record, la_bound, la_bound_e2e, load_pkg, record_flips, state_dict_for, sub_dict,
                     synth)
pkg = load_pkg()
FTOL = 1e-4
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ conv blocks vs oracle (bit exact)
CONV_SHAPES = [
    # cin, cout, H, W, ks, relu, bn, pool, fold(h0,w0,Hs,Ws) or None        # the kernel the dispatcher selects at the test's B = 2
    # (comments checked against einx_conv_plan; test_conv_block_bit_exact asserts launch == plan.  Per-instantiation coverage is
    # conv_plan_cases.CONV_PLAN_CASES, not this table: 13 of its 18 entries are small grids that land on the conv16 kernels)
    (1, 64, 40, 48, 3, True, False, False, (1, 2, 37, 45)),  # generic 12x16 (thin layer, CK = 8), fold
    (5, 64, 40, 48, 3, True, True, False, (1, 2, 37, 45)),   # generic 12x16 (thin layer), fold
    (16, 64, 24, 64, 3, True, True, False, None),            # conv16_kernel<false,8,1>
    (64, 64, 40, 64, 3, True, True, True, None),             # conv16_kernel<true,8,1>
    (64, 64, 24, 32, 3, True, False, True, None),            # conv16_kernel<true,8,1>
    (64, 128, 22, 24, 3, True, True, False, None),           # conv16_kernel<false,8,1>
    (128, 128, 44, 16, 3, True, True, True, None),           # conv16_kernel<true,8,1>
    (128, 128, 33, 44, 3, True, True, False, None),          # conv16_kernel<false,8,1>
    (128, 256, 33, 44, 3, True, False, False, None),         # conv16_kernel<false,8,1>
    (256, 65, 33, 44, 1, False, False, False, None),         # conv16_1x1_kernel<1>
    (256, 256, 5, 6, 1, False, True, False, None),           # conv16_1x1_kernel<1>
    (128, 1, 37, 45, 1, False, True, False, None),           # conv16_1x1_kernel<1>
    (6, 7, 9, 10, 3, False, True, False, None),              # generic 11x11 (thin layer); ragged everything
    (64, 256, 132, 176, 3, True, True, False, None),         # generic 12x16, un-pooled (exact tiling, 968 workgroups)
    (64, 64, 132, 176, 3, True, False, True, None),          # generic 12x16 pooled
    (8, 64, 16, 16, 3, True, True, False, None),             # conv16_kernel<false,8,1>, one chunk
    (256, 64, 33, 44, 1, False, True, False, None),          # conv16_1x1_kernel<1>
    (256, 130, 120, 90, 1, True, False, False, None),        # conv16_1x1_kernel<4>, ragged cout
]


CONV16_SHAPES = [
    # B, cin, cout, H, W, relu, bn, pool, expected N-tiles per wave
    (1, 128, 128, 33, 44, True, True, False, 1),   # the single-pair 33x44 layers
    (1, 128, 256, 33, 44, True, False, False, 1),  # head hidden layer, four output-channel tiles
    (1, 128, 128, 66, 88, True, True, True, 1),    # pooled, 726 workgroups
    (1, 64, 64, 132, 176, True, True, True, 2),    # two N-tiles per wave, pooled across lanes j^1 / j^8
    (1, 64, 64, 132, 176, True, False, False, 2),
    (2, 8, 20, 5, 13, False, True, False, 1),      # one chunk, ragged channels, odd size (masked halo and stores)
    (3, 16, 70, 10, 18, True, True, True, 1),      # ragged output channels across two channel tiles, pooled
    (1, 8, 64, 128, 256, True, False, True, 4),    # four N-tiles per wave (exactly 8192 MFMA tiles, 512 workgroups)
]


CONV16_1X1_SHAPES = [
    # B, cin, cout, H, W, relu, bn, N-tiles per wave
    (1, 256, 65, 33, 44, False, True, 1),    # detector head's 1x1 at a single pair: 65 channels over two channel tiles
    (1, 256, 256, 33, 44, False, True, 1),   # descriptor head's 1x1
    (1, 256, 65, 33, 44, False, False, 1),   # SuperPoint's convPb (no BN)
    (2, 32, 20, 5, 13, True, False, 1),      # one round, ragged pixel run (65 pixels) and ragged channels, ReLU
    (3, 64, 130, 9, 31, True, True, 1),      # three channel tiles, last with two channels
    (1, 128, 128, 130, 173, False, True, 4), # cell-1 heads at a quarter-size map: four N-tiles per wave, ragged last tile
    (1, 128, 1, 60, 80, False, True, 1),     # SiLK's one-channel detector output
    (2, 64, 128, 60, 80, True, True, 2),     # two N-tiles per wave
]


# ------------------------------------------------------------------ detector post-processing
POST = Golden("post")


# ------------------------------------------------------------------ descriptors
DESC = Golden("desc")


# ------------------------------------------------------------------ MNN
MNN = Golden("mnn")


# ------------------------------------------------------------------ whole extractors / EIM
CONV = Golden("conv")
E2E = Golden("e2e")


def _build(c, G):
    cfg = pkg.configs.to_attr(c["cfg"])
    model = pkg.EIM(cfg, device=DEV)
    sd = state_dict_for(c, G)
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith("descriptor_scale_factor") for k in missing), (missing, unexpected)
    return model.eval(), sd


def _inputs(c):
    H, W = c.get("H", 260), c.get("W", 346)
    ev, mask = synth.synth_events(c["iseed"], c["B"], c["ce"], H, W)
    img = synth.synth_image(c["iseed"], c["B"], H, W)
    return ev, mask, img


def _oracle_feats(oracle, c, sd, ev, mask, img, dense=False):
    cfg = c["cfg"]
    et, it = cfg["event_extractor"]["type"], cfg["image_extractor"]["type"]
    ecfg, icfg = cfg["event_extractor"][et], cfg["image_extractor"][it]
    ef = oracle.extractor_forward(et, sub_dict(sd, "event_extractor.extractor."), ev.copy(), mask, top_k=ecfg["detection_top_k"],
                                  radius=ecfg["nms_radius"], border=ecfg["remove_borders"], det_thr=ecfg["detection_threshold"],
                                  scale=ecfg["descriptor_scale_factor"], dense=dense)
    imf = oracle.extractor_forward(it, sub_dict(sd, "image_extractor.extractor."), img.copy(), None, top_k=icfg["detection_top_k"],
                                   radius=icfg["nms_radius"], border=icfg["remove_borders"], det_thr=icfg["detection_threshold"],
                                   scale=icfg["descriptor_scale_factor"], dense=dense)
    return ef, imf


def _assert_feats_equal_oracle(got, exp, dense=False):
    keys = ["backbone_feats", "logits", "raw_descriptors", "probability", "score", "nms"]
    if "coarse_descriptors" in exp:
        keys.append("coarse_descriptors")
    if dense:
        keys.append("normalized_descriptors")
    for k in keys:
        assert np.array_equal(_np(got[k]), exp[k]), f"{k} differs from the oracle"
    assert [int(p.shape[0]) for p in got["sparse_positions"]] == [len(p) for p in exp["sparse_positions"]]
    for b in range(len(exp["sparse_positions"])):
        assert np.array_equal(_np(got["sparse_positions"][b]), exp["sparse_positions"][b])
        assert np.array_equal(_np(got["sparse_descriptors"][b]), exp["sparse_descriptors"][b])
    assert [tuple(_np(s)) for s in got["image_size"]] == [tuple(s) for s in exp["image_size"]]


# ------------------------------------------------------------------ LightGlue
LG = Golden("lg")
LGCAL = Golden("lgcal")
# Float tolerances of the LightGlue path, next to what is MEASURED (helpers.close_and_record / record_flips print the maxima and
# the assignment-flip counts at the end of the session; profiles/r04_parity_errors.json keeps the round's table):
#   matching_scores, ref_descriptors, matched keypoints: the north_star's 1e-4 absolute.
#   log_assignment: the reference does not reproduce ITSELF to 1e-4 -- with its keypoints permuted it moves by 1.8e-4 .. 4.3e-4,
#   and it is 1.7e-4 .. 3.7e-4 away from its own float64 evaluation (tests/golden/lgcal.npz `noise`, generated by
#   gen_golden.py::lg_noise_floor).  Bound = helpers.la_bound(fixture) = 2 x that floor + 8 ulp of the largest value for comparisons on identical inputs;
#   end-to-end comparisons against the reference add the reference's measured response to +-2e-6 of input-descriptor noise
#   (helpers.la_bound_e2e).  The float64 results are stored too, so the kernels are also held to the same bound against the
#   exact answer.  Match ASSIGNMENTS are compared exactly and every comparison's flip count is recorded (target 0).


def _lg_model(c):
    import json
    cc = dict(c)
    cc["state_keys"] = json.loads(bytes(LG[f"{c['name']}.state_keys"]).decode())
    sd = state_dict_for(cc)
    lg = pkg.LightGlue({"input_dim": c["input_dim"]}).to(DEV)
    lg.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return lg.eval(), sd


# ------------------------------------------------------------------ event representation (next row 8f-2)
EVENTS = Golden("events")


# ------------------------------------------------------------------ evaluation metrics (next row 8f-1)
METRICS = Golden("metrics")


# ------------------------------------------------------------------ un-frozen Matcher branch
TRAIN = Golden("train")


def _unfrozen_matcher(name, L):
    import json
    c = dict(TRAIN.cases[name])
    cfg = pkg.default_config("SP_MNN" if c["matcher"] == "MNN" else "SP_LG", event_channels=5)
    cfg.matcher.freeze = False
    cfg.matcher.max_points_num = L
    mm = pkg.Matcher(cfg, device=DEV)
    sd = None
    if c["wseed"] is not None:
        c["state_keys"] = json.loads(bytes(TRAIN[f"{name}.state_keys"]).decode())
        sd = state_dict_for(c)
        mm.matcher.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert mm.matcher.training  # Matchers.py:47-48: an un-frozen matcher is put in train mode
    return mm, sd
# log_assignment: bounded by a multiple of the reference's OWN summation-order / rounding noise on the matching fixture
# (helpers.la_bound, tests/golden/lgcal.npz), not by a hand-picked number

_Z = np.load(os.path.join(GOLDEN, "r2.npz"))
_META = json.loads(bytes(_Z["meta"]).decode())
TIES = {c["name"]: c for c in _META["tie_cases"]}
MNNS = {c["name"]: c for c in _META["mnn_cases"]}
REPS = {c["name"]: c for c in _META["rep_cases"]}
TIED = ("alleq", "dup", "zero", "ratio_dup")


# ------------------------------------------------------------------ BASELINE batch sizes vs per-pair oracle
def _bench_like_model(cfg_name, seed=11, event_channels=5):
    cfg = pkg.default_config(cfg_name, event_channels=event_channels)
    model = pkg.EIM(cfg, device=DEV).eval()
    sd = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        ext.dense_outputs = False
    return cfg, model, sd


def _calibrate(model, sd, ev, img, mask):
    """bench.py's descriptor-bias calibration (distinct descriptors -> tens of matches per pair)"""
    ef, imf, _ = model(ev, img.clone(), mask)
    msd = model.state_dict()
    over = {}
    for prefix, feats in (("event_extractor.extractor.", ef), ("image_extractor.extractor.", imf)):
        mean = feats["raw_descriptors"].mean(dim=(0, 2, 3))
        key = [k for k in msd if k.startswith(prefix) and (k.endswith("convDb.bias") or k.endswith("_desH2.1.bias"))]
        assert len(key) == 1
        over[key[0]] = (msd[key[0]] - mean).detach().cpu()
    model.load_state_dict(over, strict=False)
    for k, v in over.items():
        sd[k] = v.numpy()


def _oracle_pair(oracle, cfg, sd, ev, mask, img, b):
    et, it = cfg.event_extractor.type, cfg.image_extractor.type
    oe = oracle.extractor_forward(et, sub_dict(sd, "event_extractor.extractor."), ev[b:b + 1].copy(), mask[b:b + 1], top_k=1024,
                                  scale=cfg.event_extractor[et].descriptor_scale_factor)
    oi = oracle.extractor_forward(it, sub_dict(sd, "image_extractor.extractor."), img[b:b + 1].copy(), None, top_k=1024,
                                  scale=cfg.image_extractor[it].descriptor_scale_factor)
    return oe, oi


def _calibrate_lightglue(model, sd, ef, imf):
    """synth.lightglue_calibration from the final descriptors of pair 0 (the same rule as tests/golden/lgcal.npz and bench.py)"""
    one = lambda f: {"sparse_positions": f["sparse_positions"][0][None], "sparse_descriptors": f["sparse_descriptors"][0][None],  # noqa: E731
                     "image_size": [f["image_size"][0]]}
    r = model.matcher.matcher(one(ef), one(imf))
    x = np.concatenate([_np(r["ref_descriptors0"])[0, 0], _np(r["ref_descriptors1"])[0, 0]], 0)
    over, _ = synth.lightglue_calibration(sd, x, prefix="matcher.matcher.")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in over.items()}, strict=False)
    sd.update(over)


# ------------------------------------------------------------------ r2 fixtures: MNN thresholds / exact ties
def _mnn_feats(d0, d1, k0, k1):
    size = torch.tensor([260, 346])
    f0 = {"sparse_descriptors": _t(d0)[None], "sparse_positions": _t(k0)[None], "image_size": [size]}
    f1 = {"sparse_descriptors": _t(d1)[None], "sparse_positions": _t(k1)[None], "image_size": [size]}
    return f0, f1


# ------------------------------------------------------------------ padding=0 networks (cell 1)
PAD0 = {c["name"]: c for c in _META["pad0_cases"]}


def _sp_mnn_model(dense_event=False):
    cfg = pkg.default_config("SP_MNN", event_channels=5)
    model = pkg.EIM(cfg, device=DEV).eval()
    sd = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=11)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    model.event_extractor.extractor.dense_outputs = dense_event
    model.image_extractor.extractor.dense_outputs = False
    return model


def _four_pairs(seed):
    ev, mask = synth.synth_events(seed, 4, 5)
    img = synth.synth_image(seed, 4)
    return ev, mask, img


def _tiled(a, B):
    return np.concatenate([a] * (B // a.shape[0]), axis=0)


def _need_free_gb(gb):
    free = torch.cuda.mem_get_info()[0] / 2**30
    if free < gb:
        pytest.skip(f"needs {gb} GB of free device memory, {free:.0f} GB available")


def _ramp(H, W):
    s = (np.arange(W, dtype=np.float32)[None, :] + 1) / np.float32(W + 1)
    return np.broadcast_to(s, (H, W)).copy()[None, None]


def _serpentine(H, W):
    """values increasing along a boustrophedon path through EVERY pixel: each maximum is decided only after the one that
    follows it on the path, 380 passes on 96x96"""
    m = np.zeros((H, W), np.float32)
    v = 1
    for y in range(2, H - 2):
        for x in (range(W) if y % 2 == 0 else range(W - 1, -1, -1)):
            m[y, x] = np.float32(v) / np.float32((H - 4) * W + 1)
            v += 1
    return m[None, None]
LGCFG = Golden("lgcfg")


def _conf(c):
    return {k: c[k] for k in ("input_dim", "descriptor_dim", "num_heads", "n_layers")}


def _lgcfg_model(c, keys=None):
    lg = pkg.LightGlue(_conf(c)).to(DEV)
    shapes = keys if keys is not None else {k: list(v.shape) for k, v in lg.state_dict().items()}
    sd = state_dict_for(dict(c, state_keys=shapes))
    lg.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return lg.eval(), sd


BATCH_CASES = [
    # (conf, B, cap0, cap1): caps of 1024 with B >= 3 take the persistent 128x128-tile linears (>= 256 tiles), the small ones the
    # 64x64-tile kernels; d = 192 has a partial 128-column tile per q | k | v block; unequal caps run the two sides unstacked
    (dict(input_dim=256, descriptor_dim=256, num_heads=8, n_layers=2), 3, 1024, 1024),
    (dict(input_dim=128, descriptor_dim=192, num_heads=3, n_layers=2), 4, 1024, 1024),
    (dict(input_dim=256, descriptor_dim=512, num_heads=4, n_layers=1), 3, 1024, 640),
    (dict(input_dim=128, descriptor_dim=128, num_heads=4, n_layers=2), 5, 130, 130),
    (dict(input_dim=64, descriptor_dim=64, num_heads=2, n_layers=2), 2, 70, 200),
]


def _rng(seed):
    return np.random.default_rng(seed)  # shapes only; tensor contents come from synth (platform independent)


CONV_SEEDS = list(range(24))


def _eim_model(cfg_name, seed, **kw):
    cfg = pkg.default_config(cfg_name, event_channels=5)
    model = pkg.EIM(cfg, device=DEV, **kw).eval()
    sd = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return cfg, model, sd

RGB = Golden("rgb")


def _with_layout(x):
    """device tensor with the numpy view's shape AND strides (its memory layout is what the test is about)"""
    base = x if x.base is None else x.base
    while base.base is not None:
        base = base.base
    off = (x.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // 4
    flat = torch.from_numpy(np.ascontiguousarray(base).reshape(-1)).to(DEV) if base.flags["C_CONTIGUOUS"] else None
    assert flat is not None
    return flat.as_strided(x.shape, tuple(s // 4 for s in x.strides), off)


def _feats_equal_oracle(got, exp):
    for k in ("backbone_feats", "logits", "raw_descriptors", "probability", "score", "nms", "coarse_descriptors"):
        assert np.array_equal(_np(got[k]), exp[k]), f"{k} differs from the oracle"
    for b in range(len(exp["sparse_positions"])):
        assert np.array_equal(_np(got["sparse_positions"][b]), exp["sparse_positions"][b])
        assert np.array_equal(_np(got["sparse_descriptors"][b]), exp["sparse_descriptors"][b])

#!/usr/bin/env python3
"""Golden-vector generator: runs the REFERENCE implementation (read-only at
/root/reference, imported with the dependency shims of _ref_stubs.py) on
deterministic synthetic inputs/weights and stores inputs' recipes + expected
outputs as small .npz fixtures next to this file.

Run ONLY in the build container (the reference does not exist on the GPU box):

    python tests/golden/gen_golden.py [group ...]     # groups: train metrics events post desc mnn conv lg e2e r2 ii lgcal mnnstab rgb cfgsweep lgcfg

The fixtures are data (recipes, shapes, expected outputs); no reference source
text is stored.  torch version and seeds are recorded in each file's `meta`.
Inputs and weights come from ei-nexus_official_amd/synth.py (integer-hash based,
platform independent), so tests regenerate them instead of storing them.
"""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"

sys.path.insert(0, HERE)
sys.path.insert(0, REF)
import _ref_stubs  # noqa: E402

_ref_stubs.install()

import torch  # noqa: E402
import yaml  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)

_spec = importlib.util.spec_from_file_location("einx_synth", os.path.join(REPO, "ei-nexus_official_amd", "synth.py"))
synth = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(synth)

import core.modules.image_extractors.superpoint_extractor as ref_sp  # noqa: E402
import core.modules.image_extractors.silk_extractor as ref_silk  # noqa: E402
from core.modules.utils import detector_util as ref_det  # noqa: E402
from core.modules.utils import descriptor_util as ref_desc  # noqa: E402
from core.modules.matchers.MNN import NearestNeighborMatcher  # noqa: E402
from core.modules.matchers.lightglue import LightGlue  # noqa: E402
from core.modules.EIM import EIM  # noqa: E402

# --- neutralise weight downloads / checkpoint loads (weights are synthetic) ---------------
ref_sp.torch.hub.load_state_dict_from_url = lambda *a, **k: None
_orig_sp_load = ref_sp.SuperPointv1.load_state_dict


def _sp_load(self, sd, *a, **k):
    if sd is None:
        return None
    return _orig_sp_load(self, sd, *a, **k)


ref_sp.SuperPointv1.load_state_dict = _sp_load
ref_silk.load_model_from_checkpoint = lambda model, **kw: model.eval()


def meta(**kw):
    kw["torch"] = torch.__version__
    kw["numpy"] = np.__version__
    return np.frombuffer(json.dumps(kw).encode(), dtype=np.uint8)


def load_synth_weights(module, seed):
    sd = module.state_dict()
    new = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in sd.items()], seed)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in new.items()}, strict=False)
    return {k: list(v.shape) for k, v in sorted(new.items())}


MAX_FIXTURE_BYTES = 1000 * 1024  # no committed file reaches 1 MiB


def save(name, **arrays):
    """name.npz; a fixture that would reach MAX_FIXTURE_BYTES is split by keys, in order, into name.npz (with `meta`),
    name.1.npz, ... of about equal raw size (tests/helpers.py::Golden reads the parts as one)."""
    import glob
    base = os.path.join(HERE, name[:-4])
    for old in glob.glob(base + ".[0-9]*.npz"):
        os.remove(old)
    keys = sorted(arrays, key=lambda k: k != "meta")  # `meta` goes to name.npz (helpers.lg_noise reads it there)
    n = 1
    while True:
        target = sum(np.asarray(v).nbytes for v in arrays.values()) / n
        groups, acc = [[]], 0.0
        for k in keys:
            if groups[-1] and acc + np.asarray(arrays[k]).nbytes > target and len(groups) < n:
                groups.append([])
                acc = 0.0
            groups[-1].append(k)
            acc += np.asarray(arrays[k]).nbytes
        paths = [base + (".npz" if i == 0 else f".{i}.npz") for i in range(len(groups))]
        for path, g in zip(paths, groups):
            np.savez_compressed(path, **{k: arrays[k] for k in g})
        if all(os.path.getsize(p) < MAX_FIXTURE_BYTES for p in paths) or n >= len(keys):
            break
        n += 1
    for p in paths:
        print(f"wrote {os.path.basename(p)}: {os.path.getsize(p) / 1024:.1f} KiB")


# =========================================================================================
# post: detector post-processing (border, fast_nms, top-k threshold, positions)
# =========================================================================================
def score_map(recipe):
    kind, seed, B, H, W = recipe["kind"], recipe["seed"], recipe["B"], recipe["H"], recipe["W"]
    u = synth.uniform01(seed, (B, 1, H, W))
    if kind == "rand":
        return u
    if kind == "quant":  # many exact ties
        return np.floor(u * np.float32(8.0)) / np.float32(8.0)
    if kind == "peaky":
        return (u ** 8).astype(np.float32)
    if kind == "sparse":
        keep = synth.uniform01(seed + 7, (B, 1, H, W)) < np.float32(0.01)
        return np.where(keep, u, np.float32(0)).astype(np.float32)
    raise ValueError(kind)


POST_CASES = [
    dict(name="rand64x88", kind="rand", seed=11, B=2, H=64, W=88, k=50, radius=4, border=4, thr=1.0),
    dict(name="ties40x48", kind="quant", seed=12, B=2, H=40, W=48, k=30, radius=4, border=4, thr=1.0),
    dict(name="few40x48", kind="sparse", seed=13, B=1, H=40, W=48, k=1024, radius=4, border=4, thr=1.0),
    dict(name="kgeN16x24", kind="rand", seed=14, B=1, H=16, W=24, k=1024, radius=4, border=4, thr=1.0),
    dict(name="full264x352", kind="peaky", seed=15, B=1, H=264, W=352, k=1024, radius=4, border=4, thr=1.0),
    dict(name="nonms24x32", kind="rand", seed=16, B=1, H=24, W=32, k=20, radius=0, border=4, thr=1.0),
    dict(name="detthr64x88", kind="rand", seed=17, B=2, H=64, W=88, k=50, radius=4, border=4, thr=0.9),
    dict(name="rank33x45", kind="rand", seed=18, B=1, H=33, W=45, k=100, radius=2, border=1, thr=1.0),
    dict(name="rank50x70", kind="rand", seed=19, B=3, H=50, W=70, k=300, radius=1, border=0, thr=1.0),
    dict(name="rank260x346", kind="peaky", seed=20, B=1, H=260, W=346, k=1024, radius=4, border=4, thr=1.0),
    dict(name="silk60x80", kind="rand", seed=21, B=4, H=60, W=80, k=0, radius=4, border=4, thr=0.0),
    dict(name="xy64x88", kind="rand", seed=22, B=1, H=64, W=88, k=40, radius=3, border=2, thr=1.0, ordering="xy"),
]


def gen_post():
    out = {"meta": meta(cases=POST_CASES)}
    for c in POST_CASES:
        score = torch.from_numpy(score_map(c).copy())
        nms = ref_det.prob_map_to_points_map(
            score, prob_thresh=c["thr"], nms_dist=c["radius"], border_dist=c["border"],
            use_fast_nms=True, top_k=(c["k"] or None))
        pos = ref_det.prob_map_to_positions_with_prob(nms, threshold=0.0, ordering=c.get("ordering", "yx"))
        n = c["name"]
        out[f"{n}.counts"] = np.array([p.shape[0] for p in pos], np.int64)
        out[f"{n}.positions"] = torch.cat(pos, 0).numpy()
        flat = nms.reshape(-1)
        nz = torch.nonzero(flat).squeeze(1)
        out[f"{n}.nms_idx"] = nz.numpy()
        out[f"{n}.nms_val"] = flat[nz].numpy()
        # score after in-place border removal (observable side effect, A10)
        sflat = score.reshape(-1)
        out[f"{n}.score_sum"] = np.array([float(sflat.double().sum())])
        if c["name"] == "silk60x80":
            # property of the reference's vendored utils_test.py:31-63 (fast == original)
            sc2 = torch.from_numpy(score_map(c).copy())
            slow = ref_det.prob_map_to_points_map(sc2, 0.0, 4, 4, use_fast_nms=False)
            assert torch.equal(slow, nms), "fast_nms != original_nms in the reference itself"
        print(n, out[f"{n}.counts"])
    save("post.npz", **out)


# =========================================================================================
# desc: sparse descriptor sampling
# =========================================================================================
def gen_desc():
    out = {}
    cases = []
    # low-resolution (cell 8) bilinear grid_sample path
    for name, seed, D, hc, wc, n in [("low_d32", 31, 32, 9, 12, 64), ("low_d256", 32, 256, 5, 6, 40)]:
        Hp, Wp = hc * 8, wc * 8
        raw = synth.normalish(seed, (2, D, hc, wc))
        pos_list = []
        for b in range(2):
            ys = np.floor(synth.uniform01(seed + 1 + b, (n,)) * np.float32(Hp)).astype(np.float32)
            xs = np.floor(synth.uniform01(seed + 3 + b, (n,)) * np.float32(Wp)).astype(np.float32)
            # force a few onto the extreme border rows/cols
            ys[:4] = [0, Hp - 1, 0, Hp - 1]
            xs[:4] = [0, 0, Wp - 1, Wp - 1]
            p = np.stack([ys + 0.5, xs + 0.5, synth.uniform01(seed + 5 + b, (n,))], 1).astype(np.float32)
            pos_list.append(p)
        pos_list[1] = pos_list[1][:0]  # n == 0 edge case for the second image
        res = ref_desc.sparsify_low_resolution_descriptors(
            torch.from_numpy(raw), [torch.from_numpy(p) for p in pos_list], (Hp, Wp), scale_factor=1.0)
        coarse = ref_desc.normalize_descriptors(torch.from_numpy(raw), scale_factor=1.0)
        out[f"{name}.desc0"] = res[0].numpy()
        out[f"{name}.desc1_shape"] = np.array(res[1].shape, np.int64)
        out[f"{name}.coarse"] = coarse.numpy()
        cases.append(dict(name=name, seed=seed, D=D, hc=hc, wc=wc, n=n, kind="low", scale=1.0))
    # full-resolution (cell 1) gather path, scale 1.41
    name, seed, D, H, W, n = "full_d128", 41, 128, 20, 24, 50
    raw = synth.normalish(seed, (1, D, H, W))
    ys = np.floor(synth.uniform01(seed + 1, (n,)) * np.float32(H)).astype(np.float32)
    xs = np.floor(synth.uniform01(seed + 3, (n,)) * np.float32(W)).astype(np.float32)
    p = np.stack([ys + 0.5, xs + 0.5, synth.uniform01(seed + 5, (n,))], 1).astype(np.float32)
    res = ref_desc.sparsify_full_resolution_descriptors(
        torch.from_numpy(raw), (torch.from_numpy(p),), scale_factor=torch.tensor(1.41))
    out[f"{name}.desc0"] = res[0].numpy()
    cases.append(dict(name=name, seed=seed, D=D, H=H, W=W, n=n, kind="full", scale=1.41))
    # dense upsample + normalise (K10) on a small map
    name, seed, D, hc, wc = "dense_d16", 45, 16, 3, 4
    raw = synth.normalish(seed, (1, D, hc, wc))
    up = ref_desc.upsample_descriptors(torch.from_numpy(raw), (hc * 8, wc * 8), scale_factor=1.0)
    out[f"{name}.up"] = up.numpy()
    cases.append(dict(name=name, seed=seed, D=D, hc=hc, wc=wc, kind="dense", scale=1.0))
    out["meta"] = meta(cases=cases)
    save("desc.npz", **out)


# =========================================================================================
# mnn: mutual nearest neighbour matcher
# =========================================================================================
def mnn_inputs(c):
    d0 = synth.synth_unit_descriptors(c["seed"], c["n"], c["D"], c["scale"])
    d1 = synth.synth_unit_descriptors(c["seed"] + 1, c["m"], c["D"], c["scale"])
    if c.get("shared", 0):
        # make `shared` rows of d1 noisy copies of rows of d0 so that real mutual matches exist
        s = c["shared"]
        perm = np.argsort(synth.uniform01(c["seed"] + 2, (c["m"],)))[:s]
        src = np.argsort(synth.uniform01(c["seed"] + 3, (c["n"],)))[:s]
        mix = d0[src] + np.float32(0.25) * d1[perm]
        mix = mix / np.sqrt((mix.astype(np.float64) ** 2).sum(-1, keepdims=True)).astype(np.float32)
        d1[perm] = (mix * np.float32(c["scale"])).astype(np.float32)
    k0 = np.concatenate([synth.uniform(c["seed"] + 4, (c["n"], 2), 0, 260), synth.uniform01(c["seed"] + 5, (c["n"], 1))], 1)
    k1 = np.concatenate([synth.uniform(c["seed"] + 6, (c["m"], 2), 0, 260), synth.uniform01(c["seed"] + 7, (c["m"], 1))], 1)
    return d0, d1, k0.astype(np.float32), k1.astype(np.float32)


MNN_CASES = [
    dict(name="d256", seed=51, n=257, m=300, D=256, scale=1.0, shared=120),
    dict(name="d128", seed=52, n=300, m=257, D=128, scale=1.41, shared=90),
    dict(name="full1024", seed=53, n=1024, m=1021, D=256, scale=1.0, shared=600),
    dict(name="tiny", seed=54, n=5, m=3, D=256, scale=1.0, shared=2),
]


def gen_mnn():
    out = {"meta": meta(cases=MNN_CASES)}
    mm = NearestNeighborMatcher(ratio_thresh=False, distance_thresh=False, mutual_check=True)
    for c in MNN_CASES:
        d0, d1, k0, k1 = mnn_inputs(c)
        f0 = {"sparse_descriptors": torch.from_numpy(d0)[None], "sparse_positions": torch.from_numpy(k0)[None]}
        f1 = {"sparse_descriptors": torch.from_numpy(d1)[None], "sparse_positions": torch.from_numpy(k1)[None]}
        r = mm(f0, f1)
        n = c["name"]
        out[f"{n}.matches0"] = r["matches0"].numpy()
        out[f"{n}.matches1"] = r["matches1"].numpy()
        out[f"{n}.mscores0"] = r["matching_scores0"].numpy()
        out[f"{n}.mscores1"] = r["matching_scores1"].numpy()
        out[f"{n}.matched_kpts0"] = r["matched_kpts0"].numpy()
        out[f"{n}.matched_kpts1"] = r["matched_kpts1"].numpy()
        la = r["log_assignment"]
        if c["n"] <= 300:
            out[f"{n}.la"] = la.numpy()
        else:
            out[f"{n}.la_probe"] = la[0, ::37, ::41].numpy()
            out[f"{n}.la_sum"] = np.array([float(la.double().sum())])
        # margin of the row/col arg-max decisions (gap between best and second best)
        sim = r["similarity"][0]
        t2 = sim.topk(2, dim=1).values
        out[f"{n}.row_gap_min"] = np.array([float((t2[:, 0] - t2[:, 1]).min())])
        print(n, int((r["matches0"] > -1).sum()), "matches; min row gap", out[f"{n}.row_gap_min"])
    save("mnn.npz", **out)


# =========================================================================================
# conv / e2e: whole extractors and EIM.forward with synthetic weights
# =========================================================================================
def model_cfg(event_type="vgg", image_type="superpointv1", matcher="MNN", ce=5, k=1024, lg_input_dim=None):
    with open(os.path.join(REF, "configs/model/SP_MNN.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["event_extractor"]["type"] = event_type
    cfg["event_extractor"]["freeze"] = True
    cfg["event_extractor"]["vgg"]["in_channels"] = ce
    cfg["event_extractor"]["vgg_np"]["in_channels"] = ce
    cfg["image_extractor"]["type"] = image_type
    cfg["matcher"]["type"] = matcher
    for sec in ("vgg", "vgg_np"):
        cfg["event_extractor"][sec]["detection_top_k"] = k
    for sec in ("superpointv1", "silk"):
        cfg["image_extractor"][sec]["detection_top_k"] = k
    if lg_input_dim is not None:
        cfg["matcher"]["LightGlue"]["input_dim"] = lg_input_dim
    return cfg


def feats_summary(prefix, feats, out, full=False):
    B = len(feats["sparse_positions"])
    out[f"{prefix}.counts"] = np.array([p.shape[0] for p in feats["sparse_positions"]], np.int64)
    out[f"{prefix}.positions"] = torch.cat(list(feats["sparse_positions"]), 0).numpy()
    sd = torch.cat(list(feats["sparse_descriptors"]), 0)
    out[f"{prefix}.sparse_desc"] = sd.numpy() if full else sd[:, :8].numpy()
    for key in ("backbone_feats", "logits", "raw_descriptors", "score", "nms"):
        t = feats[key]
        if full and t.numel() <= 70000:
            out[f"{prefix}.{key}"] = t.numpy()
        elif full:
            # too large to store whole: every 7th element of the flattened tensor + sums
            tf = t.reshape(-1)
            out[f"{prefix}.{key}.stride7"] = tf[::7].numpy()
            out[f"{prefix}.{key}.sums"] = np.array([float(tf.double().sum()), float((tf.double() ** 2).sum())])
        else:
            tf = t.reshape(-1).double()
            idx = (torch.arange(64, dtype=torch.int64) * (tf.numel() - 1)) // 63
            out[f"{prefix}.{key}.probe"] = tf[idx].float().numpy()
            out[f"{prefix}.{key}.sums"] = np.array([float(tf.sum()), float((tf * tf).sum())])
        out[f"{prefix}.{key}.shape"] = np.array(t.shape, np.int64)
    # top-k boundary margin per image: relative gap between kth and (k+1)th surviving score
    gaps = []
    for b in range(B):
        sc = feats["sparse_positions"][b][:, 2]
        gaps.append(float(sc.min()) if sc.numel() else 0.0)
    out[f"{prefix}.min_kept_score"] = np.array(gaps)
    out[f"{prefix}.keys"] = np.frombuffer(json.dumps(sorted(feats.keys())).encode(), dtype=np.uint8)


def match_summary(prefix, m, out):
    for key in ("matches0", "matches1", "matching_scores0", "matching_scores1", "matched_kpts0", "matched_kpts1"):
        vals = m[key]
        out[f"{prefix}.{key}"] = torch.cat([v.reshape(-1, v.shape[-1]) if v.dim() > 1 else v[None] for v in vals], 0).numpy() \
            if key.startswith("matched") else torch.cat([v.reshape(-1) for v in vals], 0).numpy()
        out[f"{prefix}.{key}.lens"] = np.array([v.shape[0] if key.startswith("matched") else v.numel() for v in vals], np.int64)
    la = m["log_assignment"]
    out[f"{prefix}.la_probe"] = torch.stack([x[0, ::97, ::89][:8, :8] for x in la]).numpy()
    out[f"{prefix}.la_shapes"] = np.array([list(x.shape) for x in la], np.int64)


CONV_CASES = [
    dict(name="vgg5_small", event_type="vgg", image_type="superpointv1", ce=5, H=37, W=45, B=2, k=20, wseed=1, iseed=3),
    dict(name="vgg16_small", event_type="vgg", image_type="superpointv1", ce=16, H=40, W=48, B=1, k=20, wseed=2, iseed=4),
    dict(name="np_small", event_type="vgg_np", image_type="silk", ce=5, H=37, W=45, B=2, k=30, wseed=3, iseed=5),
]


def build_eim(cfg, wseed):
    model = EIM(_ref_stubs.to_attr(cfg), device="cpu")
    keys = load_synth_weights(model, wseed)
    model.eval()
    return model, keys


def calibrate(model, ev, mask, img):
    """Random-weight ReLU stacks emit descriptors dominated by a per-channel constant (all
    keypoints look alike, ~1 mutual match in 1024).  Centre the raw descriptor maps by moving
    the per-channel spatial mean into the last bias of each descriptor head.  The resulting
    bias vectors are stored in the fixture as `override.<state_dict key>` (data), and the tests
    apply them on top of the name-synthesised weights."""
    overrides = {}
    sd = model.state_dict()
    with torch.no_grad():
        ef = model.event_extractor(torch.from_numpy(ev), torch.from_numpy(mask))
        imf = model.image_extractor(torch.from_numpy(img.copy()), None)
    for prefix, feats in (("event_extractor.extractor.", ef), ("image_extractor.extractor.", imf)):
        mean = feats["raw_descriptors"].mean(dim=(0, 2, 3))
        cands = [k for k in sd if k.startswith(prefix) and (k.endswith("convDb.bias") or k.endswith("_desH2.1.bias"))]
        assert len(cands) == 1, cands
        key = cands[0]
        overrides[key] = (sd[key] - mean).numpy()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in overrides.items()}, strict=False)
    return overrides


def gen_conv():
    out = {}
    for c in CONV_CASES:
        cfg = model_cfg(c["event_type"], c["image_type"], "MNN", c["ce"], c["k"])
        model, keys = build_eim(cfg, c["wseed"])
        ev, mask = synth.synth_events(c["iseed"], c["B"], c["ce"], c["H"], c["W"])
        img = synth.synth_image(c["iseed"], c["B"], c["H"], c["W"])
        for k_, v_ in calibrate(model, ev, mask, img).items():
            out[f"{c['name']}.override.{k_}"] = v_
        with torch.no_grad():
            ef = model.event_extractor(torch.from_numpy(ev), torch.from_numpy(mask))
            imf = model.image_extractor(torch.from_numpy(img.copy()), None)
        feats_summary(f"{c['name']}.ev", ef, out, full=True)
        feats_summary(f"{c['name']}.im", imf, out, full=True)
        c["cfg"] = cfg
        c["state_keys"] = keys
        print(c["name"], out[f"{c['name']}.ev.counts"], out[f"{c['name']}.im.counts"])
    out["meta"] = meta(cases=CONV_CASES)
    save("conv.npz", **out)


E2E_CASES = [
    dict(name="sp_mnn", event_type="vgg", image_type="superpointv1", matcher="MNN", ce=5, B=2, wseed=11, iseed=21),
    dict(name="sp_mnn16", event_type="vgg", image_type="superpointv1", matcher="MNN", ce=16, B=1, wseed=12, iseed=22),
    dict(name="sp_lg", event_type="vgg", image_type="superpointv1", matcher="LightGlue", ce=5, B=1, wseed=13, iseed=23),
    dict(name="silk_mnn", event_type="vgg_np", image_type="silk", matcher="MNN", ce=5, B=1, wseed=14, iseed=24),
    # configs/model/test/EI_SiLK_LG.yaml: 128-d SiLK descriptors through LightGlue's input_proj (lightglue.py:451-454)
    dict(name="silk_lg", event_type="vgg_np", image_type="silk", matcher="LightGlue", ce=5, B=1, wseed=15, iseed=25),
]


def gen_e2e(only=None):
    out = {}
    cases = []
    for c in E2E_CASES:
        if only and c["name"] not in only:
            continue
        cfg = model_cfg(c["event_type"], c["image_type"], c["matcher"], c["ce"], 1024,
                        lg_input_dim=(128 if c["image_type"] == "silk" else 256))
        model, keys = build_eim(cfg, c["wseed"])
        ev, mask = synth.synth_events(c["iseed"], c["B"], c["ce"])
        img = synth.synth_image(c["iseed"], c["B"])
        for k_, v_ in calibrate(model, ev, mask, img).items():
            out[f"{c['name']}.override.{k_}"] = v_
        with torch.no_grad():
            ef, imf, m = model(torch.from_numpy(ev), torch.from_numpy(img.copy()), torch.from_numpy(mask))
        feats_summary(f"{c['name']}.ev", ef, out)
        feats_summary(f"{c['name']}.im", imf, out)
        match_summary(f"{c['name']}.m", m, out)
        c = dict(c)
        c["cfg"] = cfg
        c["state_keys"] = keys
        cases.append(c)
        print(c["name"], out[f"{c['name']}.ev.counts"], out[f"{c['name']}.im.counts"], out[f"{c['name']}.m.matched_kpts0.lens"])
    out["meta"] = meta(cases=cases)
    save("e2e.npz", **out)


# =========================================================================================
# lg: LightGlue alone with synthetic weights and synthetic keypoints/descriptors
# =========================================================================================
LG_CASES = [
    dict(name="d256", seed=61, n=200, m=233, input_dim=256, wseed=5, shared=100),
    dict(name="d128", seed=62, n=150, m=140, input_dim=128, wseed=6, shared=70),
    dict(name="full", seed=63, n=1024, m=1023, input_dim=256, wseed=7, shared=500),
]


def lg_inputs(c):
    mc = dict(seed=c["seed"], n=c["n"], m=c["m"], D=c["input_dim"], scale=1.0, shared=c["shared"])
    d0, d1, k0, k1 = mnn_inputs(mc)
    # keypoints in (y,x,score) with y<260, x<346
    k0[:, 1] = k0[:, 1] * np.float32(346.0 / 260.0)
    k1[:, 1] = k1[:, 1] * np.float32(346.0 / 260.0)
    return d0, d1, k0, k1


def gen_lg():
    out = {"meta": meta(cases=LG_CASES)}
    for c in LG_CASES:
        conf = _ref_stubs.to_attr({"input_dim": c["input_dim"], "ratio_thresh": False, "distance_thresh": False})
        lg = LightGlue(conf)
        keys = load_synth_weights(lg, c["wseed"])
        lg.eval()
        d0, d1, k0, k1 = lg_inputs(c)
        size = torch.tensor([260, 346])
        f0 = {"sparse_descriptors": torch.from_numpy(d0)[None], "sparse_positions": torch.from_numpy(k0)[None], "image_size": [size]}
        f1 = {"sparse_descriptors": torch.from_numpy(d1)[None], "sparse_positions": torch.from_numpy(k1)[None], "image_size": [size]}
        layer_out = {}

        def hook(i):
            def fn(mod, inp, outp):
                layer_out[i] = (outp[0].detach().clone(), outp[1].detach().clone())
            return fn

        hs = [lg.transformers[i].register_forward_hook(hook(i)) for i in (0, 1, 8)]
        with torch.no_grad():
            r = lg(f0, f1)
        for h in hs:
            h.remove()
        n = c["name"]
        for i in (0, 1, 8):
            a, b = layer_out[i]
            out[f"{n}.l{i}.desc0"] = a[0, ::max(1, c["n"] // 16), ::16].numpy()
            out[f"{n}.l{i}.desc1"] = b[0, ::max(1, c["m"] // 16), ::16].numpy()
        with torch.no_grad():
            enc = lg.posenc(torch.from_numpy((k0[None, :, :2] - np.array([130.0, 173.0], np.float32)) / np.float32(173.0)))
        out[f"{n}.enc0"] = enc[:, 0, 0, ::max(1, c["n"] // 16), :].numpy()
        out[f"{n}.matches0"] = r["matches0"].numpy()
        out[f"{n}.matches1"] = r["matches1"].numpy()
        out[f"{n}.mscores0"] = r["matching_scores0"].numpy()
        out[f"{n}.mscores1"] = r["matching_scores1"].numpy()
        out[f"{n}.matched_kpts0"] = r["matched_kpts0"].numpy()
        out[f"{n}.matched_kpts1"] = r["matched_kpts1"].numpy()
        la = r["log_assignment"]
        if c["n"] <= 300:
            out[f"{n}.la"] = la.numpy()
        else:
            out[f"{n}.la_probe"] = la[0, ::37, ::41].numpy()
        out[f"{n}.ref_desc0_probe"] = r["ref_descriptors0"][0, 0, ::max(1, c["n"] // 16), ::16].numpy()
        out[f"{n}.state_keys"] = np.frombuffer(json.dumps(keys).encode(), dtype=np.uint8)
        # decision margin: gap between best and second best of scores rows
        sc = la[0, :-1, :-1]
        t2 = sc.topk(2, dim=1).values
        out[f"{n}.row_gap_min"] = np.array([float((t2[:, 0] - t2[:, 1]).min())])
        print(n, int((r["matches0"] > -1).sum()), "matches; min row gap", out[f"{n}.row_gap_min"])
    save("lg.npz", **out)


# =========================================================================================
# events: raw events -> voxel grid and events mask (datasets/representations.py, visualize.py)
# =========================================================================================
EVENT_CASES = [
    dict(name="int_p01", seed=71, n=3000, H=40, W=48, bins=5, frac=False, pneg=False),
    dict(name="frac_pm1", seed=72, n=2500, H=37, W=45, bins=16, frac=True, pneg=True),
    dict(name="full", seed=73, n=60000, H=260, W=346, bins=5, frac=False, pneg=False),
    # round 5: fractional coordinates and +-1 polarities at the size that matters (all eight corners non-zero)
    dict(name="full_frac", seed=74, n=60000, H=260, W=346, bins=5, frac=True, pneg=True),
]


def synth_raw_events(c):
    n, H, W = c["n"], c["H"], c["W"]
    u = synth.uniform01(c["seed"], (n,)).astype(np.float64)
    t = 1.5e9 + np.cumsum(u * 1e-4 + 1e-6)  # increasing float64 timestamps
    x = synth.uniform01(c["seed"] + 1, (n,)) * np.float32(W - 1)
    y = synth.uniform01(c["seed"] + 2, (n,)) * np.float32(H - 1)
    if not c["frac"]:
        x, y = np.floor(x), np.floor(y)
    # cluster a share of the events so that the accumulation image has a wide count range
    hot = synth.uniform01(c["seed"] + 4, (n,)) < np.float32(0.3)
    x = np.where(hot, np.float32(W // 2) + np.floor(x / 8), x).astype(np.float32)
    y = np.where(hot, np.float32(H // 2) + np.floor(y / 8), y).astype(np.float32)
    p = (synth.uniform01(c["seed"] + 3, (n,)) < np.float32(0.5)).astype(np.float32)
    if c["pneg"]:
        p = 2 * p - 1
    return {"x": x.astype(np.float32), "y": y.astype(np.float32), "t": t, "p": p.astype(np.float32)}


def gen_events():
    # the reference's `datasets/` has no __init__.py and would lose against the installed
    # HuggingFace `datasets` package, so load its two files by path
    def _load(name):
        sp = importlib.util.spec_from_file_location("ref_" + name, os.path.join(REF, "datasets", name + ".py"))
        mod = importlib.util.module_from_spec(sp)
        sp.loader.exec_module(mod)
        return mod
    sys.modules.setdefault("matplotlib.pyplot", __import__("types").ModuleType("matplotlib.pyplot"))
    ref_rep = _load("representations")
    draw_events_accumulation_image = _load("visualize").draw_events_accumulation_image
    # Round 5: ONE torch thread.  `put_(accumulate=True)` adds serially (corner major, then event order) with one thread at
    # every size; with 8 threads it switches to unordered atomic adds from 32768 elements on, which made the 60k-event
    # fixtures of rounds 1-4 order-dependent (they could only be compared with a tolerance).
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    out = {"meta": meta(cases=EVENT_CASES, torch_threads=1)}
    for c in EVENT_CASES:
        ev = synth_raw_events(c)
        grid = ref_rep.events_to_voxel_grid({k: v.copy() for k, v in ev.items()}, (c["bins"], c["H"], c["W"]), normalize=True)
        raw = ref_rep.events_to_voxel_grid({k: v.copy() for k, v in ev.items()}, (c["bins"], c["H"], c["W"]), normalize=False)
        raw2 = ref_rep.events_to_voxel_grid({k: v.copy() for k, v in ev.items()}, (c["bins"], c["H"], c["W"]), normalize=False)
        assert torch.equal(raw, raw2), "the reference is not reproducible run to run with one thread"
        img = draw_events_accumulation_image({k: v.copy() for k, v in ev.items()}, (c["W"], c["H"]))
        n = c["name"]
        if grid.numel() <= 70000:
            out[f"{n}.grid"] = grid.numpy()
            out[f"{n}.raw"] = raw.numpy()
        else:
            # every bit of the un-normalised grid: per (bin, row) the 64-bit sum and the xor of the row's fp32 bit patterns
            # (the whole tensor would be 1.8 MB per case); plus every 7th value of both grids for a readable comparison
            bits = raw.numpy().view(np.uint32).reshape(c["bins"] * c["H"], c["W"])
            out[f"{n}.raw.rowsum"] = bits.astype(np.uint64).sum(1)
            out[f"{n}.raw.rowxor"] = np.bitwise_xor.reduce(bits, axis=1)
            out[f"{n}.grid.stride7"] = grid.reshape(-1)[::7].numpy()
            out[f"{n}.raw.stride7"] = raw.reshape(-1)[::7].numpy()
        out[f"{n}.mask"] = np.packbits(img > 0)
        out[f"{n}.mask_count"] = np.array([int((img > 0).sum())])
        print(n, float(grid.abs().sum()), int((img > 0).sum()))
    torch.set_num_threads(threads)
    save("events.npz", **out)


# =========================================================================================
# metrics: MatchingRatio, MeanMatchingAccuracy, ValidDescriptorsDistance (core/metrics)
# =========================================================================================
METRIC_CASES = [
    dict(name="identity", seed=81, n=300, m=280, D=64, hom=None),
    dict(name="homography", seed=82, n=400, m=350, D=256, hom=[1.02, 0.015, -3.0, -0.01, 0.98, 2.5, 1e-5, -2e-5, 1.0]),
    dict(name="nomatch", seed=83, n=50, m=60, D=32, hom=None, M=0),
    # round 5: the conventions / edge cases of matching_metrics.py:84-156 and keypoints_metrics.py:170-290
    dict(name="xy_rows", warped_copies=True, seed=84, n=260, m=300, D=64, hom=[0.99, 0.02, 2.0, -0.015, 1.01, -1.5, 2e-5, 1e-5, 1.0], order="xy"),  # (x, y, score) rows
    dict(name="two_sizes", warped_copies=True, seed=85, n=320, m=240, D=128, hom=[0.9, 0.0, 4.0, 0.0, 0.9, 3.0, 0.0, 0.0, 1.0], size0=[260, 346], size1=[240, 320]),
    dict(name="off_image", warped_copies=True, seed=86, n=300, m=300, D=64, hom=[1.0, 0.0, 150.0, 0.0, 1.0, -90.0, 0.0, 0.0, 1.0]),  # most points leave the other image
    dict(name="all_out", warped_copies=True, seed=87, n=120, m=90, D=32, hom=[1.0, 0.0, 1000.0, 0.0, 1.0, 1000.0, 0.0, 0.0, 1.0]),   # nothing survives the visibility filter
    dict(name="empty0", seed=88, n=0, m=80, D=32, hom=None, M=0),
    dict(name="empty1", seed=89, n=70, m=0, D=32, hom=None, M=0),
    dict(name="thr135", warped_copies=True, seed=90, n=400, m=380, D=256, hom=[1.01, -0.02, 1.0, 0.02, 0.99, -2.0, -1e-5, 2e-5, 1.0], thr=[1, 3, 5]),
    dict(name="perspective", warped_copies=True, seed=91, n=350, m=350, D=64, hom=[0.95, 0.05, 6.0, -0.04, 1.05, -4.0, 3e-4, -2e-4, 1.0], thr=[1, 3, 5]),
    dict(name="xy_two_sizes", warped_copies=True, seed=92, n=200, m=260, D=64, hom=[1.1, 0.0, -5.0, 0.0, 1.1, -4.0, 0.0, 0.0, 1.0], order="xy", size0=[180, 240], size1=[260, 346]),
]


def metric_inputs(c):
    n, m, D = c["n"], c["m"], c["D"]
    H, W = c.get("size0", [260, 346])
    k0 = np.stack([synth.uniform(c["seed"], (n,), 4, H - 4), synth.uniform(c["seed"] + 1, (n,), 4, W - 4), synth.uniform01(c["seed"] + 2, (n,))], 1)
    # image-1 keypoints: noisy copies of a share of image-0 keypoints (so neighbours within 1-3 px exist) plus random ones
    share = min(n, m) * 2 // 3
    k1 = np.stack([synth.uniform(c["seed"] + 3, (m,), 4, H - 4), synth.uniform(c["seed"] + 4, (m,), 4, W - 4), synth.uniform01(c["seed"] + 5, (m,))], 1)
    k1[:share, :2] = k0[:share, :2] + synth.uniform(c["seed"] + 6, (share, 2), -2.5, 2.5)
    if c.get("hom") is not None and c.get("warped_copies"):
        # round-5 cases (`warped_copies`): image-1 copies sit where the homography sends the image-0 keypoints (+ the same noise), so that
        # MMA / VDD see real correspondences under a non-trivial warp; (y, x) rows -> (x, y) -> warp -> back
        Hm = np.array(c["hom"], np.float64).reshape(3, 3)
        xy1 = np.stack([k0[:share, 1], k0[:share, 0], np.ones(share)], 0).astype(np.float64)
        w = Hm @ xy1
        k1[:share, 0] = (w[1] / w[2]).astype(np.float32) + (k1[:share, 0] - k0[:share, 0])
        k1[:share, 1] = (w[0] / w[2]).astype(np.float32) + (k1[:share, 1] - k0[:share, 1])
    d0 = synth.synth_unit_descriptors(c["seed"] + 7, n, D)
    d1 = synth.synth_unit_descriptors(c["seed"] + 8, m, D)
    d1[:share] = d0[:share] * np.float32(0.8) + d1[:share] * np.float32(0.6)
    M = c.get("M", share // 2)
    mk0 = k0[:M].copy()
    mk1 = k1[:M].copy()
    if c.get("order", "yx") == "xy":  # rows as (x, y, score)
        k0, k1, mk0, mk1 = [a[:, [1, 0, 2]] for a in (k0, k1, mk0, mk1)]
    return [np.ascontiguousarray(a.astype(np.float32)) for a in (k0, k1, d0, d1, mk0, mk1)]


def metric_names(c):
    thr = c.get("thr", [1, 3])
    return ["MR"] + [f"MMA@{t}" for t in thr] + [f"VDD_{p}@{t}" for t in thr for p in ("Repeatability", "ValidDistance", "Angle")]


def gen_metrics():
    from core.metrics.keypoints_metrics import ValidDescriptorsDistance
    from core.metrics.matching_metrics import MatchingRatio, MeanMatchingAccuracy
    out = {"meta": meta(cases=METRIC_CASES)}
    for c in METRIC_CASES:
        k0, k1, d0, d1, mk0, mk1 = [torch.from_numpy(a) for a in metric_inputs(c)]
        Hm = torch.eye(3) if c["hom"] is None else torch.tensor(c["hom"], dtype=torch.float32).reshape(3, 3)
        thr = c.get("thr", [1, 3])
        xy = c.get("order", "yx") == "xy"
        s0, s1 = tuple(c.get("size0", [260, 346])), tuple(c.get("size1", [260, 346]))
        vals = {}
        vals.update(MatchingRatio("MR").update_one(mk0, mk1, k0, k1))
        for t in thr:
            vals.update(MeanMatchingAccuracy(f"MMA@{t}", threshold=t, ordering="xy" if xy else "yx").update_one(mk0, mk1, Hm))
        # ValidDescriptorsDistance's ordering names the OPPOSITE convention (keypoints_metrics.py:193-198): "xy" swaps the columns
        vals.update(ValidDescriptorsDistance("VDD", thr, ordering="yx" if xy else "xy").update_one(k0, k1, d0, d1, s0, s1, Hm))
        names = metric_names(c)
        out[f"{c['name']}.values"] = np.array([vals[k] for k in names], np.float64)
        print(c["name"], {k: round(vals[k], 5) for k in names})
    save("metrics.npz", **out)


# =========================================================================================
# train: forward pass of the un-frozen Matcher branch (Matchers.py:67-149,204-222): random padding
# to max_points_num, stacking, ONE batched matcher call (MNN b>1 / LightGlue b>1 in training mode)
# =========================================================================================
TRAIN_CASES = [
    dict(name="mnn", matcher="MNN", seed=81, counts0=[70, 96, 120], counts1=[96, 60, 101], L=96, D=256, tseed=1234, wseed=None),
    dict(name="lg", matcher="LightGlue", seed=82, counts0=[80, 96, 110], counts1=[90, 50, 96], L=96, D=256, tseed=4321, wseed=8),
]


def train_inputs(c):
    """per-sample ragged features: lists of [n_i,3] positions (y,x,score) and [n_i,D] descriptors"""
    f = []
    for side, counts in ((0, c["counts0"]), (1, c["counts1"])):
        pos, desc = [], []
        for i, n in enumerate(counts):
            sd = c["seed"] * 100 + side * 10 + i
            mc = dict(seed=sd, n=n, m=n, D=c["D"], scale=1.0, shared=0)
            d0, _, k0, _ = mnn_inputs(mc)
            k0[:, 1] = k0[:, 1] * np.float32(346.0 / 260.0)
            pos.append(k0)
            desc.append(d0)
        f.append((pos, desc))
    # make side 1 share structure with side 0 so that real matches exist: first rows are noisy copies
    (p0, d0), (p1, d1) = f
    for i in range(len(d0)):
        s = min(len(d0[i]), len(d1[i])) // 2
        mix = d0[i][:s] + np.float32(0.3) * d1[i][:s]
        mix = mix / np.sqrt((mix.astype(np.float64) ** 2).sum(-1, keepdims=True)).astype(np.float32)
        d1[i][:s] = mix.astype(np.float32)
    return p0, d0, p1, d1


def gen_train():
    from core.modules.Matchers import Matcher as RefMatcher
    out = {"meta": meta(cases=TRAIN_CASES)}
    for c in TRAIN_CASES:
        cfg = model_cfg(matcher=c["matcher"])
        cfg["matcher"]["freeze"] = False
        cfg["matcher"]["max_points_num"] = c["L"]
        mm = RefMatcher(_ref_stubs.to_attr(cfg), logger=None, device="cpu")
        keys = {}
        if c["wseed"] is not None:
            keys = load_synth_weights(mm.matcher, c["wseed"])
        assert mm.matcher.training
        p0, d0, p1, d1 = train_inputs(c)
        size = torch.tensor([260, 346])
        B = len(p0)
        f0 = {"sparse_positions": [torch.from_numpy(a) for a in p0], "sparse_descriptors": [torch.from_numpy(a) for a in d0],
              "image_size": [size] * B}
        f1 = {"sparse_positions": [torch.from_numpy(a) for a in p1], "sparse_descriptors": [torch.from_numpy(a) for a in d1],
              "image_size": [size] * B}
        torch.manual_seed(c["tseed"])
        with torch.no_grad():
            r = mm(f0, f1)
        n = c["name"]
        out[f"{n}.in_pos0"] = r["input_feats0"]["sparse_positions"].numpy()
        out[f"{n}.in_desc0"] = r["input_feats0"]["sparse_descriptors"].numpy()
        out[f"{n}.in_pos1"] = r["input_feats1"]["sparse_positions"].numpy()
        out[f"{n}.in_desc1"] = r["input_feats1"]["sparse_descriptors"].numpy()
        for k in ("matches0", "matches1", "matching_scores0", "matching_scores1", "log_assignment"):
            out[f"{n}.{k}"] = r[k].numpy()
        for b in range(B):
            out[f"{n}.matched_kpts0.{b}"] = r["matched_kpts0"][b].numpy()
            out[f"{n}.matched_kpts1.{b}"] = r["matched_kpts1"][b].numpy()
        if "similarity" in r:
            out[f"{n}.similarity"] = r["similarity"].numpy()
        if "ref_descriptors0" in r:
            out[f"{n}.ref_shape"] = np.array(r["ref_descriptors0"].shape)
            out[f"{n}.ref0_probe"] = r["ref_descriptors0"][:, :, ::8, ::16].numpy()
            out[f"{n}.ref1_probe"] = r["ref_descriptors1"][:, :, ::8, ::16].numpy()
            out[f"{n}.prune0"] = r["prune0"].numpy()
        out[f"{n}.state_keys"] = np.frombuffer(json.dumps(keys).encode(), dtype=np.uint8)
        sc = r["log_assignment"][:, :-1, :-1]
        t2 = sc.topk(2, dim=2).values
        out[f"{n}.row_gap_min"] = np.array([float((t2[..., 0] - t2[..., 1]).min())])
        print(n, [int((r["matches0"][b] > -1).sum()) for b in range(B)], "matches; min row gap", out[f"{n}.row_gap_min"],
              "keys", sorted(r.keys()))
    save("train.npz", **out)


GROUPS = {"train": gen_train, "metrics": gen_metrics, "events": gen_events, "post": gen_post, "desc": gen_desc, "mnn": gen_mnn, "conv": gen_conv, "lg": gen_lg, "e2e": gen_e2e}

# =========================================================================================
# r2 (round 2): cases the first fixture set did not pin
#   - NMS tie maps WITH survivors (first-max-wins of fast_nms, detector_util.py:286-335)
#   - degenerate descriptors into MNN (topk(1) tie behaviour, MNN.py:12-14,88-101)
#   - find_nn's ratio / distance thresholds (MNN.py:12-22)
#   - Repeatability (core/metrics/keypoints_metrics.py:54-157)
# =========================================================================================
def tie_map(c):
    """quantised maps: `levels` distinct values -> many exact ties inside every 9x9 window"""
    u = synth.uniform01(c["seed"], (c["B"], 1, c["H"], c["W"]))
    return (np.floor(u * np.float32(c["levels"])) / np.float32(c["levels"])).astype(np.float32)


R2_TIE_CASES = [
    dict(name="tie8_40x48", seed=112, B=2, H=40, W=48, levels=8, k=0, radius=4, border=4, thr=0.0),
    dict(name="tie4_64x88", seed=113, B=3, H=64, W=88, levels=4, k=0, radius=4, border=4, thr=0.0),
    dict(name="tie16_r2_50x70", seed=114, B=2, H=50, W=70, levels=16, k=0, radius=2, border=1, thr=0.0),
    dict(name="tie64_k_264x352", seed=115, B=1, H=264, W=352, levels=64, k=1024, radius=4, border=4, thr=1.0),
    dict(name="tie256_k_64x88", seed=116, B=2, H=64, W=88, levels=256, k=40, radius=4, border=4, thr=1.0),
]


def r2_mnn_inputs(c):
    kind, n, m, D = c["kind"], c["n"], c["m"], c["D"]
    if kind == "alleq":  # every descriptor is the same unit vector on both sides
        v = synth.synth_unit_descriptors(c["seed"], 1, D)
        return np.repeat(v, n, 0).copy(), np.repeat(v, m, 0).copy()
    if kind == "dup":  # duplicated rows inside each side and exact copies across sides
        d0 = synth.synth_unit_descriptors(c["seed"], n, D)
        d1 = synth.synth_unit_descriptors(c["seed"] + 1, m, D)
        d0[n // 2:] = d0[:n - n // 2]          # row i + n/2 == row i
        d1[:m // 3] = d0[:m // 3]              # exact copies of side-0 rows (which are themselves duplicated)
        d1[m // 3:2 * (m // 3)] = d1[:m // 3]  # and duplicated once more inside side 1
        return d0, d1
    if kind == "zero":  # all-zero descriptors: sim == 0 everywhere
        return np.zeros((n, D), np.float32), np.zeros((m, D), np.float32)
    d0, d1, _, _ = mnn_inputs(dict(seed=c["seed"], n=n, m=m, D=D, scale=c.get("scale", 1.0), shared=c.get("shared", 0)))
    return d0, d1


R2_MNN_CASES = [
    dict(name="alleq", kind="alleq", seed=121, n=40, m=37, D=256),
    dict(name="dup", kind="dup", seed=122, n=64, m=48, D=128),
    dict(name="zero", kind="zero", seed=123, n=9, m=12, D=64),
    dict(name="ratio", kind="rand", seed=124, n=200, m=180, D=64, shared=90, ratio=0.9, dist=None),
    dict(name="dist", kind="rand", seed=125, n=150, m=170, D=128, shared=70, ratio=None, dist=0.7),
    dict(name="both", kind="rand", seed=126, n=257, m=300, D=256, shared=120, ratio=0.95, dist=0.75),
    dict(name="ratio_dup", kind="dup", seed=127, n=64, m=48, D=128, ratio=0.8, dist=None),
]

R2_REP_CASES = [
    dict(name="rep_identity", seed=131, n=300, m=280, hom=None, ordering="yx"),
    dict(name="rep_homography", seed=132, n=400, m=350, hom=[1.02, 0.015, -3.0, -0.01, 0.98, 2.5, 1e-5, -2e-5, 1.0], ordering="yx"),
    dict(name="rep_xy", seed=133, n=120, m=90, hom=[0.99, -0.02, 4.0, 0.015, 1.01, -3.5, -1e-5, 1e-5, 1.0], ordering="xy"),
    dict(name="rep_empty1", seed=134, n=0, m=40, hom=None, ordering="yx"),
]


R2_PAD0_CASES = [
    dict(name="pad0", event_type="vgg_np", image_type="silk", ce=5, H=52, W=60, B=2, k=30, wseed=9, iseed=7),
]


def gen_r2_pad0(out):
    """padding=0 (un-padded 3x3 convolutions, keypoints mapped back by +9): SiLKModel and VGGExtractorNP
    (silk_extractor.py:142-152, EventExtractors.py:319-329); the event extractor is called without a mask (with one the
    reference fails on the shape mismatch of `score[~score_mask] = 0`)."""
    for c in R2_PAD0_CASES:
        cfg = model_cfg(c["event_type"], c["image_type"], "MNN", c["ce"], c["k"])
        cfg["event_extractor"]["vgg_np"]["padding"] = 0
        cfg["image_extractor"]["silk"]["padding"] = 0
        model, keys = build_eim(cfg, c["wseed"])
        ev, mask = synth.synth_events(c["iseed"], c["B"], c["ce"], c["H"], c["W"])
        img = synth.synth_image(c["iseed"], c["B"], c["H"], c["W"])
        # As shipped, the reference cannot finish a padding=0 forward: filter_sparse_feats returns LISTS and
        # mapping_positions only recurses into tuples, so `positions[..., 0]` raises TypeError (EventExtractors.py:326,
        # silk_extractor.py:149).  Recorded here; the expected values below are the reference's own arithmetic with
        # mapping_positions applied per list element (the evident intent: +9 on both coordinates).
        raised = []
        for ext, args in ((model.event_extractor, (torch.from_numpy(ev), None)), (model.image_extractor, (torch.from_numpy(img.copy()), None))):
            try:
                with torch.no_grad():
                    ext(*args)
                raised.append(0)
            except TypeError as e:
                raised.append(1)
                print("unpatched reference raises:", str(e))
        out[f"{c['name']}.reference_raises_typeerror"] = np.array(raised)
        for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
            cls = type(ext)
            if not getattr(cls, "_einx_list_fix", False):
                orig = cls.mapping_positions

                def mp(self, positions, _orig=orig):
                    if isinstance(positions, list):
                        return [_orig(self, p_) for p_ in positions]
                    return _orig(self, positions)
                cls.mapping_positions = mp
                cls._einx_list_fix = True
        with torch.no_grad():
            ef = model.event_extractor(torch.from_numpy(ev), None)
            imf = model.image_extractor(torch.from_numpy(img.copy()), None)
        feats_summary(f"{c['name']}.ev", ef, out, full=True)
        feats_summary(f"{c['name']}.im", imf, out, full=True)
        out[f"{c['name']}.ev.dense_positions_probe"] = ef["dense_positions"][0][::97].numpy()
        out[f"{c['name']}.im.dense_positions_probe"] = imf["dense_positions"][0][::97].numpy()
        try:
            with torch.no_grad():
                model.event_extractor(torch.from_numpy(ev), torch.from_numpy(mask))
            out[f"{c['name']}.mask_raises"] = np.array([0])
        except (IndexError, RuntimeError) as e:
            out[f"{c['name']}.mask_raises"] = np.array([1])
            print("with a mask the reference raises:", str(e)[:80])
        c["cfg"] = cfg
        c["state_keys"] = keys
        print(c["name"], out[f"{c['name']}.ev.counts"], out[f"{c['name']}.im.counts"], tuple(ef["score"].shape), tuple(ef["backbone_feats"].shape))


def gen_r2():
    from core.metrics.keypoints_metrics import Repeatability
    out = {}
    gen_r2_pad0(out)
    out["meta"] = meta(tie_cases=R2_TIE_CASES, mnn_cases=R2_MNN_CASES, rep_cases=R2_REP_CASES, pad0_cases=R2_PAD0_CASES)
    for c in R2_TIE_CASES:
        score = torch.from_numpy(tie_map(c).copy())
        nms = ref_det.prob_map_to_points_map(score, prob_thresh=c["thr"], nms_dist=c["radius"], border_dist=c["border"],
                                             use_fast_nms=True, top_k=(c["k"] or None))
        pos = ref_det.prob_map_to_positions_with_prob(nms, threshold=0.0, ordering="yx")
        n = c["name"]
        out[f"{n}.counts"] = np.array([p.shape[0] for p in pos], np.int64)
        out[f"{n}.positions"] = torch.cat(pos, 0).numpy()
        flat = nms.reshape(-1)
        nz = torch.nonzero(flat).squeeze(1)
        out[f"{n}.nms_idx"] = nz.numpy()
        out[f"{n}.nms_val"] = flat[nz].numpy()
        if c["k"] == 0 and c["H"] * c["W"] <= 64 * 88:
            sc2 = torch.from_numpy(tie_map(c).copy())
            slow = ref_det.prob_map_to_points_map(sc2, c["thr"], c["radius"], c["border"], use_fast_nms=False)
            out[f"{n}.original_nms_equal"] = np.array([int(torch.equal(slow, nms))])
        print(n, out[f"{n}.counts"])
        assert out[f"{n}.counts"].sum() > 0, "tie case must keep survivors"
    for c in R2_MNN_CASES:
        d0, d1 = r2_mnn_inputs(c)
        k0 = np.concatenate([synth.uniform(c["seed"] + 4, (c["n"], 2), 0, 260), synth.uniform01(c["seed"] + 5, (c["n"], 1))], 1).astype(np.float32)
        k1 = np.concatenate([synth.uniform(c["seed"] + 6, (c["m"], 2), 0, 260), synth.uniform01(c["seed"] + 7, (c["m"], 1))], 1).astype(np.float32)
        mm = NearestNeighborMatcher(ratio_thresh=c.get("ratio") or False, distance_thresh=c.get("dist") or False, mutual_check=True)
        f0 = {"sparse_descriptors": torch.from_numpy(d0)[None], "sparse_positions": torch.from_numpy(k0)[None]}
        f1 = {"sparse_descriptors": torch.from_numpy(d1)[None], "sparse_positions": torch.from_numpy(k1)[None]}
        n = c["name"]
        try:
            r = mm(f0, f1)
        except RuntimeError as e:  # zero matches: torch.stack([]) (MNN.py:126-127)
            out[f"{n}.raises"] = np.frombuffer(str(e).encode()[:60], dtype=np.uint8)
            print(n, "raises", str(e)[:60])
            # the match vectors up to the failing stack are still defined by find_nn + mutual_check
            sim = torch.einsum("bnd,bmd->bnm", f0["sparse_descriptors"], f1["sparse_descriptors"])
            from core.modules.matchers.MNN import find_nn, mutual_check
            m0 = find_nn(sim, mm.ratio_thresh, mm.distance_thresh)
            m1 = find_nn(sim.transpose(1, 2), mm.ratio_thresh, mm.distance_thresh)
            m0, m1 = mutual_check(m0, m1)
            out[f"{n}.matches0"], out[f"{n}.matches1"] = m0.numpy(), m1.numpy()
            continue
        out[f"{n}.matches0"] = r["matches0"].numpy()
        out[f"{n}.matches1"] = r["matches1"].numpy()
        out[f"{n}.matched_kpts0"] = r["matched_kpts0"].numpy()
        out[f"{n}.matched_kpts1"] = r["matched_kpts1"].numpy()
        print(n, int((r["matches0"] > -1).sum()), "matches of", c["n"])
    for c in R2_REP_CASES:
        mc = dict(c, D=8)
        if c["n"] == 0:
            mc["n"] = 10
        k0, k1, _, _, _, _ = metric_inputs(mc)
        if c["n"] == 0:
            k0 = k0[:0]
        if c["ordering"] == "xy":  # rows (x, y): swap the (y, x) recipe columns
            k0, k1 = k0[:, [1, 0, 2]].copy(), k1[:, [1, 0, 2]].copy()
        Hm = torch.eye(3) if c["hom"] is None else torch.tensor(c["hom"], dtype=torch.float32).reshape(3, 3)
        vals = []
        for t in (1, 3):
            d = Repeatability(f"repeatability@{t}", distance_thresh=t, ordering=c["ordering"]).update_one(
                torch.from_numpy(k0[:, :2].copy()), torch.from_numpy(k1[:, :2].copy()), (260, 346), (260, 346), Hm)
            vals.append(d.get(f"repeatability@{t}", float("nan")))
        out[f"{c['name']}.values"] = np.array(vals, np.float64)
        print(c["name"], vals)
    save("r2.npz", **out)


GROUPS["r2"] = gen_r2


# =========================================================================================
# ii: ImageImageMatcher (core/modules/ImageImageMatcher.py:75-82): the image extractor on both images, a score mask on the
# first one only (superpoint_extractor.py:411-412: no dilation on the image side), then the matcher.
# =========================================================================================
II_CASES = [
    dict(name="ii_sp_mnn", image_type="superpointv1", matcher="MNN", H=120, W=152, B=2, k=300, wseed=31, iseed=77, mseed=78),
    dict(name="ii_silk_mnn", image_type="silk", matcher="MNN", H=60, W=76, B=2, k=200, wseed=32, iseed=79, mseed=80),
]


def ii_inputs(c):
    img0 = synth.synth_image(c["iseed"], c["B"], c["H"], c["W"])
    img1 = synth.synth_image(c["iseed"] + 1000, c["B"], c["H"], c["W"])
    mask0 = synth.uniform01(c["mseed"], (c["B"], 1, c["H"], c["W"])) < np.float32(0.7)
    return img0, img1, mask0


def gen_ii():
    from core.modules.ImageImageMatcher import ImageImageMatcher
    out, cases = {}, []
    for c in II_CASES:
        with open(os.path.join(REF, "configs/model/SuperpointMatcher.yaml")) as f:
            cfg = yaml.safe_load(f)
        with open(os.path.join(REF, "configs/model/SiLKMatcher.yaml")) as f:
            cfg["image_extractor"]["silk"] = yaml.safe_load(f)["image_extractor"]["silk"]
        cfg["image_extractor"]["type"] = c["image_type"]
        cfg["image_extractor"]["freeze"] = True
        cfg["image_extractor"][c["image_type"]]["detection_top_k"] = c["k"]
        cfg["matcher"]["type"] = c["matcher"]
        cfg["matcher"]["freeze"] = True
        for st in ("pretrain_stage1", "pretrain_stage2"):
            cfg[st]["model_path"] = None
        model = ImageImageMatcher(_ref_stubs.to_attr(cfg), device="cpu")
        keys = load_synth_weights(model, c["wseed"])
        model.eval()
        img0, img1, mask0 = ii_inputs(c)
        # descriptor-bias calibration as in `calibrate` (image extractor only, statistics of the first image batch)
        sd = model.state_dict()
        with torch.no_grad():
            f = model.image_extractor(torch.from_numpy(img0.copy()), None)
        key = [k for k in sd if k.endswith("convDb.bias") or k.endswith("_desH2.1.bias") or "descriptor_head" in k and k.endswith("1.bias")]
        key = [k for k in key if sd[k].shape[0] == f["raw_descriptors"].shape[1]][-1:]
        assert len(key) == 1, key
        ov = (sd[key[0]] - f["raw_descriptors"].mean(dim=(0, 2, 3))).numpy()
        model.load_state_dict({key[0]: torch.from_numpy(ov)}, strict=False)
        out[f"{c['name']}.override.{key[0]}"] = ov
        with torch.no_grad():
            f0, f1, m = model(torch.from_numpy(img0.copy()), torch.from_numpy(img1.copy()), mask=torch.from_numpy(mask0))
        feats_summary(f"{c['name']}.f0", f0, out)
        feats_summary(f"{c['name']}.f1", f1, out)
        match_summary(f"{c['name']}.m", m, out)
        c = dict(c)
        c["cfg"], c["state_keys"], c["override_key"] = cfg, keys, key[0]
        cases.append(c)
        print(c["name"], out[f"{c['name']}.f0.counts"], out[f"{c['name']}.f1.counts"], out[f"{c['name']}.m.matched_kpts0.lens"])
    out["meta"] = meta(cases=cases)
    save("ii.npz", **out)


GROUPS["ii"] = gen_ii


# =========================================================================================
# lgcal (round 4): LightGlue end to end in a NON-degenerate regime + the reference's own float noise floor.
#   * "same scene" pairs (synth.twin_overrides / twin_events: the event extractor is the image extractor's twin, events =
#     image / 255 + sparse perturbation) -> ~700 mutual nearest neighbours of 1024 on the input descriptors;
#   * LightGlue's assignment head calibrated like the descriptor heads were (synth.lightglue_calibration: final_proj centred
#     and scaled, matchability shifted) -> hundreds of matches per pair with matching_scores spread over 0.01 .. 0.95;
#   * noise floor: the SAME reference model on the SAME inputs with (a) 1 instead of 8 torch threads and (b) the keypoints of
#     both sides permuted (LightGlue is permutation-equivariant; outputs are un-permuted before comparing).  What differs is
#     pure summation order inside the reference -- the tests bound log_assignment by a multiple of it instead of a hand-picked
#     tolerance, and count assignment flips against it.
# =========================================================================================
LGCAL_CASES = [
    dict(name="sp_lg_twin", event_type="vgg", image_type="superpointv1", matcher="LightGlue", ce=5, B=2, wseed=41, iseed=51),
    dict(name="silk_lg_twin", event_type="vgg_np", image_type="silk", matcher="LightGlue", ce=5, B=1, wseed=42, iseed=52),
]
LG_TEMPERATURE = 32.0


def _one(f, b):
    return {k: f[k][b][None] for k in ("sparse_positions", "sparse_descriptors", "image_size")}


def _perm(seed, n):
    return np.argsort(synth.uniform01(seed, (n,)), kind="stable")


COND_EPS = 2e-6


def lg_noise_floor(lg, f0, f1, seed, n_perm=3):
    """f0/f1: single-pair feature dicts ([1,n,*]).  Returns (differences, float64 result): the reference-vs-reference
    differences described above (maxima over `n_perm` keypoint permutations) and the fp32 reference's distance from the SAME
    reference module evaluated in float64 on the same fp32 inputs (`*_f64`: its own rounding error)."""
    import copy
    n, m = f0["sparse_positions"].shape[1], f1["sparse_positions"].shape[1]
    with torch.no_grad():
        base = lg(f0, f1)
        torch.set_num_threads(1)
        one = lg(f0, f1)
        torch.set_num_threads(8)
        dbl = lambda f: {k: (v.double() if torch.is_tensor(v) else v) for k, v in f.items()}  # noqa: E731
        r64 = copy.deepcopy(lg).double()(dbl(f0), dbl(f1))
        # conditioning: the reference on descriptors that differ by +-COND_EPS (uniform) -- the size at which extractor outputs
        # of two correct fp32 implementations differ; what an END-TO-END comparison of log_assignment inherits from upstream
        jit = lambda t, s_: t + torch.from_numpy(synth.uniform(s_, tuple(t.shape), -COND_EPS, COND_EPS))  # noqa: E731
        rc = lg(dict(f0, sparse_descriptors=jit(f0["sparse_descriptors"], seed + 50)), dict(f1, sparse_descriptors=jit(f1["sparse_descriptors"], seed + 51)))
    la_b, m0_b, ms_b = base["log_assignment"][0], base["matches0"][0], base["matching_scores0"][0]
    sc = la_b[:-1, :-1]
    t2r = sc.topk(2, dim=1).values
    t2c = sc.topk(2, dim=0).values
    out = {
        "la_threads": float((one["log_assignment"][0] - la_b).abs().max()),
        "ms_threads": float((one["matching_scores0"][0] - ms_b).abs().max()),
        "flips_threads": int((one["matches0"][0] != m0_b).sum()),
        "la_perm": 0.0, "ms_perm": 0.0, "ref_perm": 0.0, "flips_perm": 0,
        "la_f64": float((la_b.double() - r64["log_assignment"][0]).abs().max()),
        "ms_f64": float((ms_b.double() - r64["matching_scores0"][0]).abs().max()),
        "ref_f64": float((base["ref_descriptors0"].double() - r64["ref_descriptors0"]).abs().max()),
        "flips_f64": int((r64["matches0"][0] != m0_b).sum()),
        "la_cond": float((rc["log_assignment"][0] - la_b).abs().max()), "ms_cond": float((rc["matching_scores0"][0] - ms_b).abs().max()),
        "flips_cond": int((rc["matches0"][0] != m0_b).sum()), "cond_eps": COND_EPS,
        "la_absmax": float(la_b.abs().max()),
        "min_row_gap": float((t2r[:, 0] - t2r[:, 1]).min()),
        "min_col_gap": float((t2c[0] - t2c[1]).min()),
        "matches": int((m0_b > -1).sum()),
    }
    for j in range(n_perm):
        p0, p1 = torch.from_numpy(_perm(seed + 2 * j, n)), torch.from_numpy(_perm(seed + 2 * j + 1, m))
        g0 = dict(f0, sparse_positions=f0["sparse_positions"][:, p0], sparse_descriptors=f0["sparse_descriptors"][:, p0])
        g1 = dict(f1, sparse_positions=f1["sparse_positions"][:, p1], sparse_descriptors=f1["sparse_descriptors"][:, p1])
        with torch.no_grad():
            pr = lg(g0, g1)
        inv0, inv1 = torch.empty_like(p0), torch.empty_like(p1)
        inv0[p0] = torch.arange(n)
        inv1[p1] = torch.arange(m)
        # un-permute: row i of the permuted run is keypoint p0[i]; the dustbin row / column stays last
        r0 = torch.cat([inv0, torch.tensor([n])])
        r1 = torch.cat([inv1, torch.tensor([m])])
        la_p = pr["log_assignment"][0][r0][:, r1]
        m0_p = pr["matches0"][0][inv0]
        m0_p = torch.where(m0_p > -1, p1[m0_p.clamp(min=0)], m0_p)
        out["la_perm"] = max(out["la_perm"], float((la_p - la_b).abs().max()))
        out["ms_perm"] = max(out["ms_perm"], float((pr["matching_scores0"][0][inv0] - ms_b).abs().max()))
        out["ref_perm"] = max(out["ref_perm"], float((pr["ref_descriptors0"][0, 0][inv0] - base["ref_descriptors0"][0, 0]).abs().max()))
        out["flips_perm"] = max(out["flips_perm"], int((m0_b != m0_p).sum()))
    return out, r64


def gen_lgcal():
    out, cases, noise = {}, [], {}
    for c in LGCAL_CASES:
        cfg = model_cfg(c["event_type"], c["image_type"], c["matcher"], c["ce"], 1024,
                        lg_input_dim=(128 if c["image_type"] == "silk" else 256))
        model, keys = build_eim(cfg, c["wseed"])
        sd = {k: v.numpy().copy() for k, v in model.state_dict().items()}
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.twin_overrides(sd).items()}, strict=False)
        ev, mask = synth.synth_events(c["iseed"], c["B"], c["ce"])
        img = synth.synth_image(c["iseed"], c["B"])
        ev = synth.twin_events(ev, img)
        for k_, v_ in calibrate(model, ev, mask, img).items():
            out[f"{c['name']}.override.{k_}"] = v_
        lg = model.matcher.matcher
        with torch.no_grad():
            ef = model.event_extractor(torch.from_numpy(ev), torch.from_numpy(mask))
            imf = model.image_extractor(torch.from_numpy(img.copy()), None)
            r = lg(_one(ef, 0), _one(imf, 0))
        x = np.concatenate([r["ref_descriptors0"][0, 0].numpy(), r["ref_descriptors1"][0, 0].numpy()], 0)
        lsd = {k: v.numpy().copy() for k, v in lg.state_dict().items()}
        over, scale = synth.lightglue_calibration(lsd, x, temperature=LG_TEMPERATURE)
        lg.load_state_dict({k: torch.from_numpy(v) for k, v in over.items()}, strict=False)
        for k_, v_ in over.items():
            if "final_proj" not in k_:  # final_proj.{weight,bias} are the synthesised ones * float32(lgscale): a rule, not data
                out[f"{c['name']}.override.matcher.matcher.{k_}"] = v_
        out[f"{c['name']}.lgscale"] = np.array([scale], np.float32)
        with torch.no_grad():
            ef, imf, m = model(torch.from_numpy(ev), torch.from_numpy(img.copy()), torch.from_numpy(mask))
        feats_summary(f"{c['name']}.ev", ef, out)
        feats_summary(f"{c['name']}.im", imf, out)
        match_summary(f"{c['name']}.m", m, out)
        out[f"{c['name']}.m.la_probe2"] = torch.stack([x_[0, ::31, ::29] for x_ in m["log_assignment"]]).numpy()
        for b in range(c["B"]):
            nf, r64 = lg_noise_floor(lg, _one(ef, b), _one(imf, b), 900 + b)
            noise[f"{c['name']}.{b}"] = nf
            out[f"{c['name']}.m.la_probe2_f64.{b}"] = r64["log_assignment"][0, ::31, ::29].numpy()  # float64
            out[f"{c['name']}.m.matching_scores0_f64.{b}"] = r64["matching_scores0"][0].numpy()
            v = m["matching_scores0"][b].reshape(-1)[m["matches0"][b].reshape(-1) > -1].numpy()
            print(c["name"], b, "matches", nf["matches"], "scores q10/50/90", np.quantile(v, [0.1, 0.5, 0.9]).round(3), nf)
        c = dict(c)
        c["cfg"], c["state_keys"], c["temperature"] = cfg, keys, LG_TEMPERATURE
        cases.append(c)
    # noise floor of the fixtures that already exist (lg.npz stand-alone cases, e2e.npz LightGlue cases): same models, same inputs
    for c in LG_CASES:
        lg = LightGlue(_ref_stubs.to_attr({"input_dim": c["input_dim"], "ratio_thresh": False, "distance_thresh": False}))
        load_synth_weights(lg, c["wseed"])
        lg.eval()
        d0, d1, k0, k1 = lg_inputs(c)
        size = torch.tensor([260, 346])
        f0 = {"sparse_descriptors": torch.from_numpy(d0)[None], "sparse_positions": torch.from_numpy(k0)[None], "image_size": [size]}
        f1 = {"sparse_descriptors": torch.from_numpy(d1)[None], "sparse_positions": torch.from_numpy(k1)[None], "image_size": [size]}
        noise[f"lg.{c['name']}"], r64 = lg_noise_floor(lg, f0, f1, 910)
        la64 = r64["log_assignment"][0]
        out[f"lg.{c['name']}.la_f64"] = (la64 if c["n"] <= 300 else la64[::37, ::41]).numpy()  # same probes as lg.npz, float64
        print("lg." + c["name"], noise[f"lg.{c['name']}"])
    for c in E2E_CASES:
        if c["matcher"] != "LightGlue":
            continue
        cfg = model_cfg(c["event_type"], c["image_type"], c["matcher"], c["ce"], 1024,
                        lg_input_dim=(128 if c["image_type"] == "silk" else 256))
        model, _ = build_eim(cfg, c["wseed"])
        ev, mask = synth.synth_events(c["iseed"], c["B"], c["ce"])
        img = synth.synth_image(c["iseed"], c["B"])
        calibrate(model, ev, mask, img)
        with torch.no_grad():
            ef = model.event_extractor(torch.from_numpy(ev), torch.from_numpy(mask))
            imf = model.image_extractor(torch.from_numpy(img.copy()), None)
        noise[f"e2e.{c['name']}"], r64 = lg_noise_floor(model.matcher.matcher, _one(ef, 0), _one(imf, 0), 920)
        out[f"e2e.{c['name']}.la_probe_f64"] = r64["log_assignment"][0, ::97, ::89][:8, :8].numpy()
        print("e2e." + c["name"], noise[f"e2e.{c['name']}"])
    out["meta"] = meta(cases=cases, noise=noise)
    save("lgcal.npz", **out)


GROUPS["lgcal"] = gen_lgcal


# =========================================================================================
# mnnstab: which match rows of the MNN end-to-end cases are UNSTABLE IN THE REFERENCE ITSELF (VERDICT r5 "next" 1).
# The same reference model on the same inputs is evaluated in other, equally valid ways -- 1 instead of 8 torch threads,
# oneDNN convolutions off (torch's native fp32 kernels), the B = 2 case one sample at a time, the whole model in float64,
# and its NearestNeighborMatcher alone on its own fp32 descriptors with the keypoints permuted / in float64 -- and every row
# of matches0 / matches1 whose value differs from the stored e2e.npz result in ANY variant is recorded (row, variant, the
# value the variant gave).  The GPU tests then need no tolerance and no flip budget: a row that differs from e2e.npz must be
# in this set.  Stored: e2e-case name -> {key: rows, variants (bit mask per row), alternative values}; nothing is re-derived.
# =========================================================================================
MNNSTAB_VARIANTS = ["threads1", "onednn_off", "per_sample", "float64", "matcher_perm", "matcher_float64", "matcher_threads1"]


def _cat_matches(m, key):
    return torch.cat([v.reshape(-1) for v in m[key]], 0).numpy().astype(np.int64)


def gen_mnnstab():
    from core.modules.matchers.MNN import NearestNeighborMatcher as RefMNN
    e2e = np.load(os.path.join(HERE, "e2e.npz"))
    out, cases, summary = {}, [], {}
    for c in E2E_CASES:
        if c["matcher"] != "MNN":
            continue
        name = c["name"]
        cfg = model_cfg(c["event_type"], c["image_type"], c["matcher"], c["ce"], 1024, lg_input_dim=(128 if c["image_type"] == "silk" else 256))
        model, keys = build_eim(cfg, c["wseed"])
        ev, mask = synth.synth_events(c["iseed"], c["B"], c["ce"])
        img = synth.synth_image(c["iseed"], c["B"])
        calibrate(model, ev, mask, img)
        run = lambda mdl=model, e=ev, i=img, k=mask: mdl(torch.from_numpy(e), torch.from_numpy(i.copy()), torch.from_numpy(k))  # noqa: E731
        with torch.no_grad():
            ef, imf, base = run()
        lens = {key: [v.numel() for v in base[key]] for key in ("matches0", "matches1")}
        for key in lens:  # the run at hand IS the stored fixture
            assert np.array_equal(_cat_matches(base, key), e2e[f"{name}.m.{key}"]), (name, key)
        variants = {}
        with torch.no_grad():
            torch.set_num_threads(1)
            variants["threads1"] = run()[2]
            torch.set_num_threads(8)
            with torch.backends.mkldnn.flags(enabled=False):
                variants["onednn_off"] = run()[2]
            if c["B"] > 1:
                per = [run(e=ev[b:b + 1], i=img[b:b + 1], k=mask[b:b + 1])[2] for b in range(c["B"])]
                variants["per_sample"] = {key: [p[key][0] for p in per] for key in lens}
            import copy
            m64 = copy.deepcopy(model).double()
            _q = torch.Tensor.quantile  # the reference hands quantile an fp32 `q` tensor, which torch refuses beside a float64 input
            torch.Tensor.quantile = lambda x, q, *a, **k: _q(x, q.to(x.dtype) if torch.is_tensor(q) else q, *a, **k)
            try:
                r64 = m64(torch.from_numpy(ev).double(), torch.from_numpy(img.copy()).double(), torch.from_numpy(mask))
                variants["float64"] = r64[2]
                # only meaningful where the float64 model finds the same keypoints (it does on these cases: asserted)
                for f32, f64 in ((ef, r64[0]), (imf, r64[1])):
                    for b in range(c["B"]):
                        assert torch.equal(f32["sparse_positions"][b][:, :2], f64["sparse_positions"][b][:, :2].float()), (name, "float64 keypoints")
            except Exception as e:  # recorded, not hidden
                variants.pop("float64", None)
                summary.setdefault(name, {})["float64_error"] = f"{type(e).__name__}: {e}"[:200]
            finally:
                torch.Tensor.quantile = _q
            # the matcher alone on the reference's own fp32 descriptors
            mnn = RefMNN()
            perm_runs, f64_runs, t1_runs = {k: [] for k in lens}, {k: [] for k in lens}, {k: [] for k in lens}
            for b in range(c["B"]):
                f0, f1 = _one(ef, b), _one(imf, b)
                n, m_ = f0["sparse_positions"].shape[1], f1["sparse_positions"].shape[1]
                alt0 = [None] * 3
                for j in range(3):
                    p0, p1 = torch.from_numpy(_perm(700 + 2 * j, n)), torch.from_numpy(_perm(701 + 2 * j, m_))
                    g0 = dict(f0, sparse_positions=f0["sparse_positions"][:, p0], sparse_descriptors=f0["sparse_descriptors"][:, p0])
                    g1 = dict(f1, sparse_positions=f1["sparse_positions"][:, p1], sparse_descriptors=f1["sparse_descriptors"][:, p1])
                    pr = mnn(g0, g1)
                    inv0, inv1 = torch.empty_like(p0), torch.empty_like(p1)
                    inv0[p0] = torch.arange(n)
                    inv1[p1] = torch.arange(m_)
                    a0 = pr["matches0"][0][inv0]
                    a0 = torch.where(a0 > -1, p1[a0.clamp(min=0)], a0)
                    a1 = pr["matches1"][0][inv1]
                    a1 = torch.where(a1 > -1, p0[a1.clamp(min=0)], a1)
                    alt0[j] = (a0, a1)
                perm_runs["matches0"].append([a[0] for a in alt0])
                perm_runs["matches1"].append([a[1] for a in alt0])
                d = lambda f: {k: (v.double() if torch.is_tensor(v) else v) for k, v in f.items()}  # noqa: E731
                r = mnn(d(f0), d(f1))
                torch.set_num_threads(1)
                r1 = mnn(f0, f1)
                torch.set_num_threads(8)
                for key in lens:
                    f64_runs[key].append(r[key][0])
                    t1_runs[key].append(r1[key][0])
        rec = {}
        for key in lens:
            b_all = _cat_matches(base, key)
            flags = np.zeros(b_all.shape, np.int64)
            alts = {}

            def note(vi, arr):
                arr = np.asarray(arr, np.int64)
                for r_ in np.nonzero(arr != b_all)[0]:
                    flags[r_] |= 1 << vi
                    alts.setdefault(int(r_), set()).add(int(arr[r_]))
            for vname, res in variants.items():
                note(MNNSTAB_VARIANTS.index(vname), torch.cat([v.reshape(-1) for v in res[key]], 0).numpy())
            for j in range(3):
                note(MNNSTAB_VARIANTS.index("matcher_perm"), torch.cat([perm_runs[key][b][j] for b in range(c["B"])], 0).numpy())
            note(MNNSTAB_VARIANTS.index("matcher_float64"), torch.cat(f64_runs[key], 0).numpy())
            note(MNNSTAB_VARIANTS.index("matcher_threads1"), torch.cat(t1_runs[key], 0).numpy())
            rows = np.nonzero(flags)[0]
            out[f"{name}.{key}.ref_unstable_rows"] = rows.astype(np.int64)          # index into the per-case concatenation
            out[f"{name}.{key}.ref_unstable_variants"] = flags[rows]               # bit i = MNNSTAB_VARIANTS[i] differs there
            width = max([len(v) for v in alts.values()] + [1])
            alt = np.full((rows.size, width), -2, np.int64)                        # the values the variants gave (-2 = padding)
            for i, r_ in enumerate(rows):
                vals = sorted(alts[int(r_)])
                alt[i, :len(vals)] = vals
            out[f"{name}.{key}.ref_unstable_alt"] = alt
            out[f"{name}.{key}.lens"] = np.array(lens[key], np.int64)
            rec[key] = {"rows": rows.tolist(), "variants": flags[rows].tolist(), "base": b_all[rows].tolist(), "alt": [sorted(alts[int(r_)]) for r_ in rows]}
        summary.setdefault(name, {}).update(rec)
        print(name, json.dumps(summary[name]))
        cases.append(dict(name=name))
    out["meta"] = meta(cases=cases, variants=MNNSTAB_VARIANTS, summary=summary)
    save("mnnstab.npz", **out)


GROUPS["mnnstab"] = gen_mnnstab


# =========================================================================================
# rgb: what SuperPointv1 accepts beside contiguous grayscale (superpoint_extractor.py:372-376): 3-channel images (scaled in
# place, then kornia's rgb_to_grayscale -- restated from kornia 0.7.1 in _ref_stubs.py, the package is absent here) and
# non-contiguous tensors (`image /= 255.0` works through the strides).  Stored: the extractor's outputs and the caller's
# tensor as the call leaves it.
# =========================================================================================
RGB_CASES = [
    dict(name="rgb_small", layout="rgb", H=37, W=45, B=2, k=20, wseed=71, iseed=81, mask=False),
    dict(name="rgb_channels_last", layout="rgb_cl", H=40, W=48, B=1, k=20, wseed=72, iseed=82, mask=False),
    dict(name="gray_strided", layout="gray_view", H=37, W=45, B=2, k=20, wseed=73, iseed=83, mask=False),
    dict(name="rgb_full_mask", layout="rgb", H=260, W=346, B=1, k=1024, wseed=74, iseed=84, mask=True),
]


def rgb_input(c):
    """numpy array with the case's memory layout (helpers.rgb_input rebuilds the same)"""
    B, H, W = c["B"], c["H"], c["W"]
    if c["layout"] == "gray_view":
        big = np.zeros((B, 1, H + 3, W + 5), np.float32)
        big[:, :, 1:H + 1, 2:W + 2] = synth.synth_image(c["iseed"], B, H, W)
        return big[:, :, 1:H + 1, 2:W + 2]  # a view: rows W + 5 apart
    chans = [synth.synth_image(c["iseed"] + 10 * ch, B, H, W)[:, 0] for ch in range(3)]
    if c["layout"] == "rgb_cl":
        return np.ascontiguousarray(np.stack(chans, -1)).transpose(0, 3, 1, 2)  # [B,H,W,3] memory seen as [B,3,H,W]
    return np.ascontiguousarray(np.stack(chans, 1))


def gen_rgb():
    out, cases = {}, []
    for c in RGB_CASES:
        cfg = model_cfg("vgg", "superpointv1", "MNN", 5, c["k"])
        model, keys = build_eim(cfg, c["wseed"])
        x = rgb_input(c)
        t = torch.from_numpy(x)  # shares memory and strides with x
        assert t.stride() == tuple(s_ // 4 for s_ in x.strides)
        mask = None
        if c["mask"]:
            _, mk = synth.synth_events(c["iseed"], c["B"], 5, c["H"], c["W"])
            mask = torch.from_numpy(mk)
        with torch.no_grad():
            imf = model.image_extractor(t, mask)
        feats_summary(f"{c['name']}.im", imf, out, full=c["H"] < 100)
        after = t.numpy()
        out[f"{c['name']}.after"] = np.ascontiguousarray(after) if after.size < 70000 else np.ascontiguousarray(after).reshape(-1)[::7]
        c = dict(c)
        c["cfg"], c["state_keys"] = cfg, keys
        cases.append(c)
        print(c["name"], out[f"{c['name']}.im.counts"], "input after the call: max", float(after.max()))
    out["meta"] = meta(cases=cases, kornia="0.7.1 rgb_to_grayscale restated in _ref_stubs.py (package absent)")
    save("rgb.npz", **out)


GROUPS["rgb"] = gen_rgb


# =========================================================================================
# cfgsweep: every model YAML the reference ships (configs/model/**), built by the reference's own classes on the CPU:
# which class the scripts use for it (EIM when it has an event_extractor section, else ImageImageMatcher), the module tree
# as state_dict names -> shapes, and the attributes the evaluation scripts read.  The YAML text is not stored; the test
# parses the files where they lie (this container only).
# =========================================================================================
def gen_cfgsweep():
    import glob
    from core.modules.ImageImageMatcher import ImageImageMatcher
    cases = []
    for path in sorted(glob.glob(os.path.join(REF, "configs/model/*.yaml")) + glob.glob(os.path.join(REF, "configs/model/test/*.yaml"))):
        with open(path) as f:
            cfg = yaml.safe_load(f)
        cls = EIM if "event_extractor" in cfg else ImageImageMatcher
        for st in ("pretrain_stage1", "pretrain_stage2"):  # checkpoint files are not available: build with fresh weights
            cfg[st]["model_path"] = None
        model = cls(_ref_stubs.to_attr(cfg), device="cpu")
        keys = {k: list(v.shape) for k, v in sorted(model.state_dict().items())}
        inner = model.matcher.matcher
        case = {"file": os.path.relpath(path, REF), "name": cfg.get("name"), "cls": cls.__name__, "state_keys": keys,
                "matcher_cls": type(inner).__name__ if inner is not None else None,
                "image_ordering": model.image_extractor.extractor.ordering,
                "event_ordering": model.event_extractor.extractor.ordering if cls is EIM else None,
                "trainable": sorted(k for k, p_ in model.named_parameters() if p_.requires_grad)}
        cases.append(case)
        print(case["file"], case["cls"], len(keys), "tensors,", len(case["trainable"]), "trainable,", case["matcher_cls"])
    save("cfgsweep.npz", meta=meta(group="cfgsweep"), cases=np.frombuffer(json.dumps(cases).encode(), dtype=np.uint8))


GROUPS["cfgsweep"] = gen_cfgsweep


# =========================================================================================
# lgcfg (round 5): LightGlue configurations other than 256 = 4 x 64 -- the reference derives head_dim = descriptor_dim //
# num_heads (lightglue.py:246-248, 456-461) and takes n_layers / input_dim from the conf; plus what add_scale_ori=True does
# =========================================================================================
LGCFG_CASES = [
    dict(name="h8_d256", seed=161, n=200, m=233, input_dim=256, descriptor_dim=256, num_heads=8, n_layers=9, wseed=15, shared=100),
    dict(name="h2_d256", seed=162, n=150, m=140, input_dim=256, descriptor_dim=256, num_heads=2, n_layers=4, wseed=16, shared=70),
    dict(name="h4_d128", seed=163, n=170, m=190, input_dim=128, descriptor_dim=128, num_heads=4, n_layers=5, wseed=17, shared=80),
    dict(name="h3_d192", seed=164, n=260, m=131, input_dim=128, descriptor_dim=192, num_heads=3, n_layers=3, wseed=18, shared=60),
    dict(name="h4_d512", seed=165, n=140, m=150, input_dim=256, descriptor_dim=512, num_heads=4, n_layers=2, wseed=19, shared=60),
    dict(name="h1_d64", seed=166, n=90, m=300, input_dim=64, descriptor_dim=64, num_heads=1, n_layers=3, wseed=20, shared=40),
    # round 6: head widths that are not 32 / 64 / 128 (lightglue.py:456-461 takes any descriptor_dim // num_heads)
    dict(name="h2_d96", seed=167, n=180, m=150, input_dim=96, descriptor_dim=96, num_heads=2, n_layers=3, wseed=21, shared=70),      # 2 x 48
    dict(name="h4_d64", seed=168, n=130, m=170, input_dim=128, descriptor_dim=64, num_heads=4, n_layers=3, wseed=22, shared=60),     # 4 x 16
    dict(name="h3_d240", seed=169, n=150, m=200, input_dim=240, descriptor_dim=240, num_heads=3, n_layers=2, wseed=23, shared=70),   # 3 x 80, d % 32 != 0
    dict(name="h2_d200", seed=170, n=140, m=120, input_dim=200, descriptor_dim=200, num_heads=2, n_layers=2, wseed=24, shared=50),   # 2 x 100
    dict(name="h1_d256", seed=171, n=120, m=150, input_dim=256, descriptor_dim=256, num_heads=1, n_layers=2, wseed=25, shared=60),   # 1 x 256 (the widest head the kernels take)
    dict(name="h2_d384", seed=172, n=100, m=90, input_dim=128, descriptor_dim=384, num_heads=2, n_layers=2, wseed=26, shared=40),    # 2 x 192 through input_proj
]


def gen_lgcfg():
    out, noise = {}, {}
    size = torch.tensor([260, 346])
    for c in LGCFG_CASES:
        conf = _ref_stubs.to_attr({k: c[k] for k in ("input_dim", "descriptor_dim", "num_heads", "n_layers")})
        lg = LightGlue(conf)
        keys = load_synth_weights(lg, c["wseed"])
        lg.eval()
        d0, d1, k0, k1 = lg_inputs(c)
        f0 = {"sparse_descriptors": torch.from_numpy(d0)[None], "sparse_positions": torch.from_numpy(k0)[None], "image_size": [size]}
        f1 = {"sparse_descriptors": torch.from_numpy(d1)[None], "sparse_positions": torch.from_numpy(k1)[None], "image_size": [size]}
        layer_out = {}

        def hook(i):
            def fn(mod, inp, outp):
                layer_out[i] = (outp[0].detach().clone(), outp[1].detach().clone())
            return fn

        probes = (0, c["n_layers"] - 1)
        hs = [lg.transformers[i].register_forward_hook(hook(i)) for i in probes]
        with torch.no_grad():
            r = lg(f0, f1)
        for h in hs:
            h.remove()
        n = c["name"]
        sn, sm = max(1, c["n"] // 16), max(1, c["m"] // 16)
        for i in probes:
            a, b = layer_out[i]
            out[f"{n}.l{i}.desc0"] = a[0, ::sn, ::8].numpy()
            out[f"{n}.l{i}.desc1"] = b[0, ::sm, ::8].numpy()
        with torch.no_grad():
            enc = lg.posenc(torch.from_numpy((k0[None, :, :2] - np.array([130.0, 173.0], np.float32)) / np.float32(173.0)))
        out[f"{n}.enc0"] = enc[:, 0, 0, ::sn, :].numpy()
        for key, short in (("matches0", "matches0"), ("matches1", "matches1"), ("matching_scores0", "mscores0"), ("matching_scores1", "mscores1"),
                           ("matched_kpts0", "matched_kpts0"), ("matched_kpts1", "matched_kpts1"), ("log_assignment", "la")):
            out[f"{n}.{short}"] = r[key].numpy()
        out[f"{n}.ref_desc0_probe"] = r["ref_descriptors0"][0, 0, ::sn, ::8].numpy()
        out[f"{n}.prune0"] = r["prune0"].numpy()
        out[f"{n}.state_keys"] = np.frombuffer(json.dumps(keys).encode(), dtype=np.uint8)
        noise[n], _ = lg_noise_floor(lg, f0, f1, 1300 + c["seed"])
        print(n, int((r["matches0"] > -1).sum()), "matches;", json.dumps(noise[n]))
    # add_scale_ori=True: what the reference's forward does (the scale / orientation inputs are commented out, :540-560)
    lg = LightGlue(_ref_stubs.to_attr({"input_dim": 256, "add_scale_ori": True}))
    aso = {"state_keys": {k: list(v.shape) for k, v in sorted(lg.state_dict().items()) if k.startswith("posenc")}}
    c = LG_CASES[0]
    d0, d1, k0, k1 = lg_inputs(c)
    f0 = {"sparse_descriptors": torch.from_numpy(d0)[None], "sparse_positions": torch.from_numpy(k0)[None], "image_size": [size]}
    f1 = {"sparse_descriptors": torch.from_numpy(d1)[None], "sparse_positions": torch.from_numpy(k1)[None], "image_size": [size]}
    try:
        with torch.no_grad():
            lg.eval()(f0, f1)
        aso["raises"] = None
    except Exception as e:  # noqa: BLE001
        aso["raises"] = type(e).__name__
        aso["message"] = str(e)
    aso["n"] = c["n"]
    print("add_scale_ori:", aso)
    save("lgcfg.npz", meta=meta(cases=LGCFG_CASES, noise=noise, add_scale_ori=aso), **out)


GROUPS["lgcfg"] = gen_lgcfg


if __name__ == "__main__":
    names = sys.argv[1:] or list(GROUPS)
    for g in names:
        GROUPS[g]()

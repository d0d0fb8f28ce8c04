#!/usr/bin/env python3
"""Fixture of the extractor losses, generated from the reference (build container only):
    python tests/golden/gen_losses.py <reference checkout>   ->  tests/golden/losses.npz, tests/golden/train_loss_configs.json
Runs the reference's core/loss/extractor_loss.py on the CPU -- the file is imported by path, because core/loss/__init__ pulls in
omegaconf -- on the inputs of tests/loss_ref.py (synth recipes: the fixture stores none) and stores OUTPUTS only:

  <case>.ref    the reference's value (float32, as its `loss_info` reports it)
  <case>.f64    the float64 restatement of tests/loss_ref.py on the same inputs
  <case>.floor  |ref - f64|: the reference's own float32 summation noise on this case
  meta          torch version, the exception type and message of every case the reference refuses, the in-place edit that
                ScoreLoss mse-whole makes to gt_feats["score"], what build_losses does for an unknown feature_loss.type

The `loss` sections of the three shipped train configs (settings only) are copied to train_loss_configs.json for
tests/test_loss_cpu.py::test_build_losses_on_the_shipped_train_configs."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import loss_ref as R  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ["EINX_REFERENCE"]


def by_path(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = by_path("ref_extractor_loss", "core/loss/extractor_loss.py")
Padder = by_path("ref_util", "core/modules/utils/util.py").Padder
torch.set_num_threads(1)
KEYS = {"desc": "normalized_descriptors", "score": "score", "logits": "logits", "feat": "backbone_feats"}


def call(case, d):
    cls, kw, key, mkey, padded = case
    mod = getattr(ref, cls)(**kw)
    pred = {KEYS[key]: torch.from_numpy(d[key + "_pred"].copy())}
    gt = {KEYS[key]: torch.from_numpy(d[key + "_gt"].copy())}
    mask = None if mkey is None else torch.from_numpy(d[mkey].copy())
    if cls == "FeatureLoss":
        loss, info = mod(pred, gt)
    elif cls == "DescriptorsLoss":
        loss, info = mod(pred, gt, mask)
    else:
        loss, info = mod(pred, gt, mask, padder=Padder((R.H, R.W), R.CELL) if padded else None)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and len(info) == 1
    return loss, info, gt[KEYS[key]].numpy()


def main():
    d = R.inputs()
    assert Padder((R.H, R.W), R.CELL).padding_size == R.PADS
    out, meta = {}, {"torch": torch.__version__, "cases": [], "info_keys": {}, "raises": {}}
    for name, case in R.VALUE_CASES.items():
        loss, info, gt_after = call(case, d)
        f64 = float(R.restate(name, d))
        v = float(loss)
        out[f"{name}.ref"] = np.float32(v)
        out[f"{name}.f64"] = np.float64(f64)
        out[f"{name}.floor"] = np.float64(abs(v - f64)) if np.isfinite(f64) else np.float64(0.0)
        assert np.isfinite(v) == np.isfinite(f64), name
        meta["cases"].append({"name": name})
        meta["info_keys"][name] = list(info)[0]
        if name == "score_whole_mask":
            before = d["score_gt"]
            meta["mse_whole_in_place"] = {"changed": int((gt_after != before).sum()),
                                          "zeroed_where_masked": bool((gt_after[d["mask"]] == 0).all()),
                                          "kept_elsewhere": bool((gt_after[~d["mask"]] == before[~d["mask"]]).all())}
        print(f"{name:28s} ref {v:.9g}  f64 {f64:.17g}  floor {abs(v - f64):.3e}")
    for name, case in R.RAISE_CASES.items():
        try:
            call(case, d)
        except Exception as e:  # noqa: BLE001
            meta["raises"][name] = {"type": type(e).__name__, "message": str(e)}
            print(f"{name:28s} {type(e).__name__}: {e}")
        else:
            raise SystemExit(f"{name}: the reference did not raise")
    # build_losses with feature_loss.type != "FeatureLoss": the function's own structure, run on its source with the names it needs
    src = open(os.path.join(REF, "core/loss/__init__.py")).read()
    src = "\n".join(ln for ln in src.splitlines() if not ln.startswith(("from omegaconf", "from .")))
    ns = {"DictConfig": object}
    for n in ("ScoreLoss", "LogitsLoss", "DescriptorsLoss", "FeatureLoss"):
        ns[n] = getattr(ref, n)
    ns["MNNLoss"] = ns["NLLLoss"] = lambda **kw: None
    exec(compile(src, "core/loss/__init__.py", "exec"), ns)

    class A(dict):
        __getattr__ = dict.__getitem__

    def attr(o):
        return A({k: attr(v) for k, v in o.items()}) if isinstance(o, dict) else o

    configs = {}
    for f in ("train_stage1.yaml", "train_stage2.yaml", "train_default.yaml"):
        with open(os.path.join(REF, "configs/train", f)) as fh:
            configs[f] = yaml.safe_load(fh)["loss"]
        # (two of the three files have no feature_loss section: the reference's build_losses cannot complete on them, whatever
        # the config class does for a missing key; recorded, and the drop-in gives those a Pass)
        try:
            built = ns["build_losses"](attr(configs[f]))
            meta.setdefault("built", {})[f] = {k: type(v).__name__ for k, v in built.items()}
        except (KeyError, AttributeError) as e:
            meta.setdefault("built", {})[f] = {"raises": type(e).__name__, "missing": str(e).strip("'")}
    bad = json.loads(json.dumps(configs["train_stage1.yaml"]))
    bad["feature_loss"]["type"] = "none"
    try:
        ns["build_losses"](attr(bad))
    except Exception as e:  # noqa: BLE001
        meta["raises"]["build_losses_unknown_feature_loss"] = {"type": type(e).__name__, "message": str(e)}
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "losses.npz"), **out)
    with open(os.path.join(HERE, "train_loss_configs.json"), "w") as fh:
        json.dump(configs, fh, indent=1, sort_keys=True)
    print(json.dumps(meta["raises"], indent=1), json.dumps(meta["built"]), meta.get("mse_whole_in_place"))


if __name__ == "__main__":
    main()

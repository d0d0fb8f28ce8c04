"""CPU-only: the opt-in fp16 convolutions where no device is needed -- the dispatcher's plan query over the shipped
networks, the new symbols, the Python switch, and the float64 restatement the GPU tests judge with."""
import copy

import pytest
import torch
import torch.nn.functional as F

import conv_f16_ref as R
from helpers import load_pkg, synth

pkg = load_pkg()
L = pkg.native.lib()

MAPS = [(264, 352), (132, 176), (66, 88), (33, 44)]
NAMES = {"conv_f16_kernel<3,8,32,16,false>", "conv_f16_kernel<3,8,32,16,true>", "conv_f16_kernel<1,1,256,64,false>"}


def _model(name):
    cfg = pkg.default_config(name, event_channels=5)
    model = pkg.EIM(cfg, device="cpu").eval()
    sd = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=3)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return model


@pytest.fixture(scope="module")
def extractors():
    sp, silk = _model("SP_MNN"), _model("SiLK_MNN")
    return {"superpointv1": sp.image_extractor.extractor, "vgg": sp.event_extractor.extractor, "silk": silk.image_extractor.extractor}


def _plan(cin, cout, ks, pool, B, H, W):
    s = L.einx_conv_f16_plan(cin, cout, ks, int(pool), B, H, W)
    return None if s is None else s.decode()


def _layers(ext):
    """(cin, cout, ks, pool, first) of every layer of an extractor"""
    bb, det, desc = ext._stacks()
    out = []
    for i, (block, pool) in enumerate(bb):
        c = ext._spec(block)[0]
        out.append((c.in_channels, c.out_channels, c.kernel_size[0], bool(pool), i == 0))
    for block in list(det) + list(desc):
        c = ext._spec(block)[0]
        out.append((c.in_channels, c.out_channels, c.kernel_size[0], False, False))
    return out


@pytest.mark.parametrize("kind", ["superpointv1", "vgg", "silk"])
def test_plan_names_a_kernel_for_every_covered_layer(extractors, kind):
    layers = _layers(extractors[kind])
    assert layers[0][4] and not R.covered(layers[0][0], True)
    n = 0
    for cin, cout, ks, pool, first in layers:
        if not R.covered(cin, first):
            continue
        for H, W in MAPS:
            if pool and (H % 2 or W % 2):
                continue
            for B in (1, 32):
                name = _plan(cin, cout, ks, pool, B, H, W)
                assert name in NAMES, (kind, cin, cout, ks, pool, B, H, W, name)
                assert ("<1," in name) == (ks == 1) and name.endswith("true>") == pool
                n += 1
    assert n >= 4 * (len(layers) - 4)


def test_plan_refuses_what_the_entry_refuses():
    for cin in (1, 5, 12):
        assert _plan(cin, 64, 3, False, 2, 40, 48) is None
        assert b"cin must be a multiple of 8" in L.einx_last_error()
    assert _plan(64, 64, 5, False, 2, 40, 48) is None and b"kernel size must be 1 or 3" in L.einx_last_error()
    for H, W in ((33, 44), (44, 33)):
        assert _plan(64, 64, 3, True, 2, H, W) is None and b"pooling needs even H and W" in L.einx_last_error()
    assert _plan(64, 64, 3, True, 2, 44, 32) is not None
    # the names are the new dispatcher's own: the fp32 plan never reports them
    assert L.einx_conv_plan(64, 64, 3, 0, 32, 264, 352, 0, 0, 264, 352).decode() not in NAMES


def test_new_symbols_and_abi_version():
    for sym in ("einx_conv_weight_elems_f16", "einx_conv_repack_f16", "einx_conv_block_f16", "einx_conv_f16_plan", "einx_conv_f16_last_kernel",
                "einx_extractor_set_conv_f16"):
        assert hasattr(L, sym), sym
    assert L.einx_abi_version() == 6
    # [cout tile][chunk][64][tap][ck]: ck 16 (3x3) / 64 (1x1), cin and cout padded up
    assert L.einx_conv_weight_elems_f16(64, 64, 3) == 64 * 9 * 64
    assert L.einx_conv_weight_elems_f16(72, 96, 3) == 2 * 5 * 64 * 9 * 16
    assert L.einx_conv_weight_elems_f16(256, 65, 1) == 2 * 4 * 64 * 64
    assert L.einx_conv_weight_elems_f16(64, 64, 5) == 0


def test_switch_defaults_off_and_reads_fp32_on_the_cpu(extractors):
    from importlib import import_module
    base = import_module(pkg.__name__ + ".core.modules._base")
    assert base.NativeExtractor.half_precision is False
    for ext in extractors.values():
        assert ext.half_precision is False and ext.conv_mode == "fp32"
        ext.half_precision = True
        try:
            assert ext.conv_mode == "fp32"  # parameters on the CPU
        finally:
            del ext.half_precision
        assert ext.half_precision is False


def _plain_f64(ext, x):
    """the stack through torch's own modules in float64 (BatchNorm unfused)"""
    bb, det, desc = ext._stacks()

    def run(t, block, pool):
        conv, bn, relu = ext._spec(block)
        t = copy.deepcopy(conv).double()(t)
        if relu:
            t = F.relu(t)
        if bn is not None:
            t = copy.deepcopy(bn).double().eval()(t)
        return F.max_pool2d(t, 2, 2) if pool else t

    t = x.double()
    for block, pool in bb:
        t = run(t, block, pool)
    outs = []
    for head in (det, desc):
        h = t
        for block in head:
            h = run(h, block, False)
        outs.append(h)
    return t, outs[0], outs[1]


@pytest.mark.parametrize("kind", ["superpointv1", "vgg"])
def test_restatement_without_rounding_is_the_plain_float64_stack(extractors, kind):
    ext = extractors[kind]
    cin = _layers(ext)[0][0]
    x = torch.from_numpy(synth.synth_image(7, 1, 16, 24)).float().repeat(1, cin, 1, 1) * (1.0 / 255 if kind == "superpointv1" else 1.0)
    with torch.no_grad():
        got = R.stack_forward(ext, x, R.spec, rounding=False)
        want = _plain_f64(ext, x)
        rounded = R.stack_forward(ext, x, R.spec, rounding=True)
    for g, w in zip(got, want):
        assert g.dtype == torch.float64 and g.shape == w.shape
        # SuperPointv1 has no BatchNorm: the same float64 operations up to where the bias joins the sum (K 2^-53 per layer, K <= 2304,
        # ten layers deep: 1e-11 with room); the VGG's affine is folded in fp32 (einx_bn_fold's arithmetic: 2^-24 per layer)
        tol = (1e-11 if kind == "superpointv1" else 1e-5) * float(w.abs().max())
        assert float((g - w).abs().max()) <= tol
    assert any(float((g - r).abs().max()) > 0 for g, r in zip(got, rounded))  # and the rounding is not a no-op

"""LightGlue `flash: True`, the parts that need no GPU: the contract's restatement (tests/lg_flash_ref.py) is
self-consistent -- without rounding it is lg_f64.forward, its two float peers lie near its float64 form --, the package's switch,
the pruning gate, and the C ABI's new symbols, size query and argument checks."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

import lg_f64
import lg_flash_ref as FR
from helpers import close_and_record, la_bound_f64, lgf64_pair, lgf64_shipped_state_dict, load_pkg

pkg = load_pkg()
LIB = import_module(pkg.__name__ + "._lib")
L = pkg.native.lib()

H16 = 2.0 ** -11  # unit roundoff of binary16


def _sd(seed, layers=2):
    """the shipped parameter tree cut to its first `layers` layers (lg_f64 counts the layers it finds)"""
    sd = lgf64_shipped_state_dict(seed)
    return {k: v for k, v in sd.items() if k.split(".")[0] not in ("transformers", "log_assignment", "token_confidence") or int(k.split(".")[1]) < layers}


def _pair(seed, n, m):
    d0, d1, k0, k1 = lgf64_pair(seed, n, m)
    return k0, d0, k1, d1


def test_rn16_is_tensor_half():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.9, 65520.0, 1e-8, 2.0 ** -25, -3.3], dtype=torch.float64)
    want = [1.0, 1.0, 1.0 + 2.0 ** -9, 65504.0, 65504.0, float("inf"), 0.0, 0.0, float(np.float16(-3.3))]  # ties to even, overflow to inf
    assert FR.rn16(x).tolist() == want
    assert torch.equal(FR.rn16(x.float()), x.float().half().float())


def test_exact_mode_is_lg_f64_forward():
    sd = _sd(11)
    pair = _pair(21, 37, 40)
    a, b = FR.forward(sd, *pair, mode="exact"), lg_f64.forward(sd, *pair)
    assert np.array_equal(a["matches0"], b["matches0"]) and np.array_equal(a["matches1"], b["matches1"])
    # the cross block scales the product instead of both factors: rounding-level differences in float64
    assert np.abs(a["log_assignment"] - b["log_assignment"]).max() < 1e-11
    for (x0, x1), (y0, y1) in zip(a["layers"], b["layers"]):
        assert np.abs(x0 - y0).max() < 1e-12 and np.abs(x1 - y1).max() < 1e-12
    assert lg_f64.self_block.__module__ == "lg_f64" and lg_f64.cross_block.__module__ == "lg_f64"  # restored


def test_spec_rounds_and_differs_from_float64():
    sd = _sd(12)
    pair = _pair(22, 33, 29)
    spec, ex = FR.forward(sd, *pair), lg_f64.forward(sd, *pair)
    d = np.abs(spec["log_assignment"] - ex["log_assignment"]).max()
    assert 1e-6 < d < 1.0, d  # binary16 inputs move the result far beyond float64 rounding, and not wildly


@pytest.mark.parametrize("n,m", [(1, 1), (7, 40), (33, 31), (40, 40)])
def test_attention_peers_against_spec(n, m):
    """one attention call: the context is an fp16 value of magnitude |o|; each peer may round to a neighbouring fp16 value, so it
    lies within one binary16 spacing (2 H16 |o|, at the binade's top) plus its fp32 / fp16-P noise of the spec"""
    rng = np.random.default_rng(100 * n + m)
    Q, K, V = (rng.standard_normal((4, r, 64)) * s for r, s in ((n, 1.5), (m, 1.5), (m, 1.0)))
    spec = FR.attention_np(Q, K, V, "spec")
    assert np.array_equal(spec, spec.astype(np.float16).astype(np.float64))
    absmax = np.abs(spec).max()
    bound = 2 * (2 * H16 * absmax)  # two spacings: a neighbour, and head-room for a value that crosses a binade
    for mode in ("peer_a", "peer_b"):
        got = FR.attention_np(Q.astype(np.float32), K.astype(np.float32), V.astype(np.float32), mode)
        assert np.array_equal(got, got.astype(np.float16).astype(np.float64)), mode
        close_and_record(f"lgflash.cpu.attention.{n}x{m} {mode} vs spec", got, spec, atol=bound)


@pytest.mark.parametrize("n,m", [(1, 1), (40, 37), (33, 40)])
def test_forward_peers_against_spec(n, m):
    """whole forward, 2 layers.  The yardstick is the contract's own effect: the spec differs from the unrounded float64 forward by
    the binary16 rounding of q, k, v and the context.  A peer differs from the spec by no more than about that -- roundings of the
    same values that fall the other way behind fp32 arithmetic (both) and one more binary16 operand, the probabilities (peer_b) --
    so each lies within helpers.la_bound_f64 of it: twice that distance plus ulps.  An implementation of another contract (a scale in the wrong
    place, q / k rounded before the rotary step) is one to two orders of magnitude outside.  The measured distances are recorded:
    they are what bounds the kernel in tests/test_lg_flash_gpu.py."""
    sd = _sd(13)
    pair = _pair(300 + n, n, m)
    spec, ex = FR.forward(sd, *pair), lg_f64.forward(sd, *pair)
    peers = {mode: FR.forward(sd, *pair, mode=mode) for mode in ("peer_a", "peer_b")}
    la = spec["log_assignment"]
    bound = la_bound_f64([np.abs(ex["log_assignment"] - la).max()], np.abs(la).max())
    for mode, r in peers.items():
        close_and_record(f"lgflash.cpu.forward.{n}x{m}.log_assignment {mode} vs spec", r["log_assignment"], la, atol=bound)
        for i, xs in enumerate(spec["layers"]):
            for s, x in enumerate(xs):
                b = la_bound_f64([np.abs(ex["layers"][i][s] - x).max()], np.abs(x).max())
                close_and_record(f"lgflash.cpu.forward.{n}x{m}.descriptors layer {i} {mode} vs spec", r["layers"][i][s], x, atol=b)


def test_package_switch_and_pruning_gate():
    lg = pkg.LightGlue({})
    assert lg.attention_mode == "fp32" and lg.conf.flash is False
    assert lg.pruning_min_kpts("cuda") == 1024 and lg.pruning_min_kpts("cuda:1") == 1024 and lg.pruning_min_kpts("cpu") == -1
    fl = pkg.LightGlue({"flash": True})
    assert fl.attention_mode == "fp16"
    assert fl.pruning_min_kpts("cuda") == 1536 and fl.pruning_min_kpts(torch.device("cuda", 0)) == 1536
    assert fl.pruning_min_kpts("cpu") == -1  # the reference's gate: flash only on a GPU
    fl.pruning_keypoint_thresholds["flash"] = 7
    assert fl.pruning_min_kpts("cuda") == 7
    fl.conf["flash"] = False  # read at every call, like the other switches
    assert fl.attention_mode == "fp32" and fl.pruning_min_kpts("cuda") == 1024
    assert set(fl.state_dict()) == set(lg.state_dict())  # the switch adds no parameter


def test_new_symbols_and_size_query():
    assert L.einx_abi_version() == 6  # additive symbols only
    for name in ("einx_lightglue_flash", "einx_lightglue_flash_ws_bytes", "einx_lg_attention_f16"):
        assert name in LIB.SIGNATURES and hasattr(L, name), name
    q, ad, base = L.einx_lightglue_flash_ws_bytes, L.einx_lightglue_adaptive_ws_bytes, L.einx_lg_ws_bytes_heads
    # the kernel needs no region of its own: the query is the adaptive carve (the largest of the three runs it can make) ...
    for shape in ((1, 5, 33, 256, 4, 256, 9), (5, 130, 130, 256, 4, 256, 9), (64, 2048, 2048, 256, 4, 256, 9), (3, 40, 48, 128, 2, 128, 3),
                  (2, 64, 64, 96, 3, 96, 4), (1, 7, 7, 1024, 4, 1024, 2), (2, 64, 64, 256, 4, 256, 32)):
        assert q(*shape) == ad(*shape) > base(*shape[:6]) > 0, shape
    # ... and the plain carve for a layer count that only the plain run takes
    for shape in ((2, 64, 64, 256, 4, 256, 33), (2, 64, 64, 256, 4, 256, 0)):
        assert ad(*shape) == 0 and q(*shape) == base(*shape[:6]) > 0, shape
    for bad in ((0, 64, 64, 256, 4, 256, 9), (2, 0, 64, 256, 4, 256, 9), (2, 64, 0, 256, 4, 256, 9), (2, 64, 64, 250, 4, 256, 9),
                (2, 64, 64, 256, 3, 256, 9), (2, 64, 64, 2048, 4, 256, 9)):
        assert q(*bad) == 0, bad


def test_c_abi_argument_checks():
    """argument checks come before any launch: no device is needed"""
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)

    def attn(Q=p, O=p, nq=p, capq=8, capk=8, B=2, heads=4, dh=64, ld=256, kv_shift=0):
        return L.einx_lg_attention_f16(Q, p, p, O, nq, p, capq, capk, B, heads, dh, ld, kv_shift, None)

    for kw, word in ((dict(Q=None), b"null pointer"), (dict(O=None), b"null pointer"), (dict(nq=None), b"null pointer"),
                     (dict(capq=0), b"bad shape"), (dict(capk=-1), b"bad shape"), (dict(B=0), b"bad shape"),
                     (dict(heads=0), b"head_dim"), (dict(dh=0), b"head_dim"), (dict(dh=30, ld=120), b"head_dim"), (dict(dh=260, ld=1040), b"head_dim"),
                     (dict(ld=252), b"ld must"), (dict(ld=258), b"ld must"), (dict(kv_shift=2), b"kv_shift"), (dict(kv_shift=-1), b"kv_shift")):
        assert attn(**kw) == -1 and word in L.einx_last_error() and b"einx_lg_attention_f16" in L.einx_last_error(), (kw, L.einx_last_error())

    w = LIB.LgWeights()
    w.n_layers = 2
    heads = (LIB.LgHead * 2)()
    hs = ctypes.sizeof(LIB.LgHead)

    def rc(heads_=heads, head_size=hs, depth=-1.0, width=-1.0, la=None, live=p, stop=p, ref_layers=1, wp=ctypes.byref(w)):
        return L.einx_lightglue_flash(wp, heads_, head_size, depth, width, 0, *([None] * 3), 64, *([None] * 3), 64, 2, 1.0, 1.0, 1.0, 1.0, p,
                                      *([None] * 4), la, None, None, ref_layers, stop, p, p, p, p, live, None)

    # width_confidence > 0: the adaptive entry's rules, reported under the flash entry's name
    for kw, word in ((dict(width=0.5, live=None), b"null pointer"), (dict(width=0.5, head_size=hs + 8), b"head_size"),
                     (dict(width=1.5), b"width_confidence"), (dict(width=0.5, la=p), b"log_assignment"), (dict(width=0.5, ref_layers=2), b"ref_layers"),
                     (dict(width=0.5), b"log_assignment head")):
        assert rc(**kw) == -1 and word in L.einx_last_error() and b"einx_lightglue_flash" in L.einx_last_error(), (kw, L.einx_last_error())
    # depth_confidence > 0 alone: the early-stop entry's
    for kw, word in ((dict(depth=0.9, stop=None), b"null pointer"), (dict(depth=0.9, heads_=None), b"null pointer"),
                     (dict(depth=0.9, ref_layers=2), b"ref_layers"), (dict(depth=0.9), b"log_assignment head")):
        assert rc(**kw) == -1 and word in L.einx_last_error() and b"einx_lightglue_flash" in L.einx_last_error(), (kw, L.einx_last_error())
    # neither: the plain run, which reads no head: the shared body's own checks (kpts0 is null)
    assert rc(heads_=None, stop=None, live=None) == -1 and b"null pointer" in L.einx_last_error()
    assert rc(wp=None) == -1 and b"null pointer" in L.einx_last_error()

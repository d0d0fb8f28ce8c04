"""LightGlue `mp: True`, the parts that need no GPU: the contract's restatement (tests/lg_mp_ref.py) is
self-consistent -- without rounding it is lg_f64.forward, its two fp32 peers lie near its float64 form, it composes with the flash
contract --, the package's switch, and the C ABI's new symbols, size query and argument checks."""
import ctypes
from importlib import import_module

import numpy as np
import pytest
import torch

import lg_f64
import lg_flash_ref as FR
import lg_mp_ref as MR
from helpers import close_and_record, la_bound_f64, lgf64_pair, lgf64_shipped_state_dict, load_pkg

pkg = load_pkg()
LIB = import_module(pkg.__name__ + "._lib")
L = pkg.native.lib()


def _sd(seed, layers=2):
    """the shipped parameter tree cut to its first `layers` layers (lg_f64 counts the layers it finds)"""
    sd = lgf64_shipped_state_dict(seed)
    return {k: v for k, v in sd.items() if k.split(".")[0] not in ("transformers", "log_assignment", "token_confidence") or int(k.split(".")[1]) < layers}


def _pair(seed, n, m):
    d0, d1, k0, k1 = lgf64_pair(seed, n, m)
    return k0, d0, k1, d1


def test_exact_mode_is_lg_f64_forward():
    sd = _sd(11)
    pair = _pair(21, 37, 40)
    a, b = MR.forward(sd, *pair, mode="exact"), lg_f64.forward(sd, *pair)
    assert np.array_equal(a["log_assignment"], b["log_assignment"])  # the same expression on the same tensors
    assert np.array_equal(a["matches0"], b["matches0"]) and np.array_equal(a["matches1"], b["matches1"])
    for (x0, x1), (y0, y1) in zip(a["layers"], b["layers"]):
        assert np.array_equal(x0, y0) and np.array_equal(x1, y1)
    assert lg_f64._linear is MR._PLAIN  # restored
    # with the flash contract on top, unrounded: lg_flash_ref's own "exact"
    c, e = MR.forward(sd, *pair, mode="exact", flash=True), FR.forward(sd, *pair, mode="exact")
    assert np.array_equal(c["log_assignment"], e["log_assignment"])
    assert lg_f64._linear is MR._PLAIN and lg_f64.self_block.__module__ == "lg_f64" and lg_f64.cross_block.__module__ == "lg_f64"


def test_only_the_layers_linears_are_rounded():
    """the hook replaces the nine layer linears and nothing else: input_proj, final_proj, matchability and the token head keep
    lg_f64's expression under every mode"""
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((5, 8)))
    sd = {p + k: rng.standard_normal(s) for p in ("input_proj.", "log_assignment.0.final_proj.", "token_confidence.0.token.0.",
                                                   "transformers.0.self_attn.Wqkv.", "transformers.1.cross_attn.ffn.0.")
          for k, s in (("weight", (4, 8)), ("bias", (4,)))}
    with MR.linears("spec"):
        for prefix, key in (("", "input_proj"), ("log_assignment.0.", "final_proj"), ("token_confidence.0.", "token.0")):
            assert torch.equal(lg_f64._linear(x, sd, prefix, key, torch.float64), MR._PLAIN(x, sd, prefix, key, torch.float64))
        for prefix, key in (("transformers.0.self_attn.", "Wqkv"), ("transformers.1.cross_attn.", "ffn.0")):
            got = lg_f64._linear(x, sd, prefix, key, torch.float64)
            want = MR.rn16(x) @ MR.rn16(torch.from_numpy(sd[prefix + key + ".weight"])).T + torch.from_numpy(sd[prefix + key + ".bias"])
            assert torch.equal(got, want) and not torch.equal(got, MR._PLAIN(x, sd, prefix, key, torch.float64))


def test_linear_modes_on_exact_inputs_agree_bit_for_bit():
    """integers times multiples of 1/16: every partial sum is representable, so every accumulation order gives the same bits, and
    the output is not rounded to binary16 (a sum of 300 products of magnitude up to 8 needs more than 11 bits)"""
    rng = np.random.default_rng(5)
    X = rng.integers(-8, 9, (7, 300)).astype(np.float64)
    W = rng.integers(-16, 17, (9, 300)) / 16.0
    b = rng.integers(-16, 17, 9) / 16.0
    want = X @ W.T + b
    for mode in ("spec", "exact", "peer_a", "peer_b"):
        assert np.array_equal(MR.linear_np(X, W, b, mode), want), mode
    assert not np.array_equal(want, want.astype(np.float16).astype(np.float64))


def test_rounding_is_tensor_half():
    x = torch.tensor([[1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), -(1.0 + 3 * 2.0 ** -11), 65519.0, 1e-9]], dtype=torch.float64)
    eye, zero = torch.eye(6, dtype=torch.float64), torch.zeros(6, dtype=torch.float64)
    assert MR.linear(x, eye, zero, "spec").tolist() == [[1.0, 1.0 + 2.0 ** -9, -1.0, -(1.0 + 2.0 ** -9), 65504.0, 0.0]]
    big = torch.tensor([[65520.0, 1.0]], dtype=torch.float32)
    assert MR.linear(big, torch.ones((1, 2)), torch.zeros(1), "peer_b").item() == float("inf")  # overflow to infinity, not saturation


@pytest.mark.parametrize("flash", [False, True])
@pytest.mark.parametrize("n,m", [(1, 40), (40, 37), (33, 40)])
def test_forward_peers_against_spec(n, m, flash):
    """Whole forward, 2 layers.  The peers differ from the spec by fp32 accumulation and by binary16 roundings of the same values
    that fall the other way behind it; the yardstick for both is the contract's own effect, the distance of the spec from the
    unrounded float64 forward (helpers.la_bound_f64 of it).  The measured distances are recorded: they are what bounds the kernel in
    tests/test_lg_mp_gpu.py.  Also recorded, as a number and not a gate: how far the spec sits from the fp32 forward."""
    sd = _sd(13)
    pair = _pair(300 + n, n, m)
    tag = f"lgmp.cpu.forward{'.flash' if flash else ''}.{n}x{m}"
    spec, ex = MR.forward(sd, *pair, flash=flash), lg_f64.forward(sd, *pair)
    f32 = lg_f64.forward(sd, *pair, dtype=torch.float32)
    peers = {mode: MR.forward(sd, *pair, mode=mode, flash=flash) for mode in ("peer_a", "peer_b")}
    la = spec["log_assignment"]
    d = np.abs(la - ex["log_assignment"]).max()
    assert 1e-6 < d < 1.0, d  # binary16 operands move the result far beyond float64 rounding, and not wildly
    close_and_record(f"{tag}.log_assignment spec vs the fp32 forward (not a gate)", la, f32["log_assignment"], atol=np.inf)
    bound = la_bound_f64([d], np.abs(la).max())
    for mode, r in peers.items():
        close_and_record(f"{tag}.log_assignment {mode} vs spec", r["log_assignment"], la, atol=bound)
        for i, xs in enumerate(spec["layers"]):
            for s, x in enumerate(xs):
                b = la_bound_f64([np.abs(ex["layers"][i][s] - x).max()], np.abs(x).max())
                close_and_record(f"{tag}.descriptors layer {i} {mode} vs spec", r["layers"][i][s], x, atol=b)
    assert not np.array_equal(peers["peer_a"]["log_assignment"], peers["peer_b"]["log_assignment"])  # two accumulation orders


def test_package_switch_defaults_off():
    plain, off, on = pkg.LightGlue({}), pkg.LightGlue({"mp": False}), pkg.LightGlue({"mp": True})
    for lg in (plain, off, on):
        lg.eval()
        assert lg.mixed_precision is False and lg.linear_mode == "fp32" and not lg.mixed_precision_active()
    assert plain.conf.mp is False and on.conf.mp is True
    off.mixed_precision = True  # the attribute alone is not enough either
    assert off.linear_mode == "fp32"
    on.mixed_precision = True  # key and attribute, eval mode -- but the model is on the CPU: the mode needs a GPU
    assert on.linear_mode == "fp32" and not on.mixed_precision_active()
    assert set(on.state_dict()) == set(plain.state_dict())  # the switch adds no parameter
    # (the switch on a device -- read at every call, eval mode only, independent of flash -- is tests/test_lg_mp_gpu.py's)


def test_new_symbols_and_size_query():
    assert L.einx_abi_version() == 6  # additive symbols, fields appended under the struct_size guard
    for name in ("einx_lightglue_mp", "einx_lightglue_mp_ws_bytes", "einx_lg_linear_f16"):
        assert name in LIB.SIGNATURES and hasattr(L, name), name
    assert LIB.LgLayer._names[-10:] == ("Wqkv_h", "Wo_h", "sf0_h", "sf3_h", "Wqk_h", "Wv_h", "Wco_h", "cf0_h", "cf3_h", "Wqk_v_h")
    q, fl, ad, base = L.einx_lightglue_mp_ws_bytes, L.einx_lightglue_flash_ws_bytes, L.einx_lightglue_adaptive_ws_bytes, L.einx_lg_ws_bytes_heads
    # the kernel needs no region of its own: the call walks the carve of the run it makes, the query is the largest of them
    for shape in ((1, 5, 33, 256, 4, 256, 9), (5, 130, 130, 256, 4, 256, 9), (64, 2048, 2048, 256, 4, 256, 9), (3, 40, 48, 128, 2, 128, 3),
                  (2, 64, 64, 96, 3, 96, 4), (2, 64, 64, 256, 4, 256, 32)):
        assert q(*shape) == fl(*shape) == ad(*shape) > base(*shape[:6]) > 0, shape
    for shape in ((2, 64, 64, 256, 4, 256, 33), (2, 64, 64, 256, 4, 256, 0)):
        assert q(*shape) == base(*shape[:6]) > 0, shape
    for bad in ((0, 64, 64, 256, 4, 256, 9), (2, 0, 64, 256, 4, 256, 9), (2, 64, 64, 250, 4, 256, 9), (2, 64, 64, 2048, 4, 256, 9)):
        assert q(*bad) == 0, bad


def test_c_abi_argument_checks():
    """argument checks come before any launch: no device is needed"""
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)

    def lin(X=p, X2=None, Ksplit=0, K=64, W=p, bias=p, N=64, Y=p, ldy=64, resid=None, cnt=p, cap=8, B=2, epi=0):
        return L.einx_lg_linear_f16(X, X2, Ksplit, K, W, bias, N, Y, ldy, resid, cnt, cap, B, epi, None)

    for kw, word in ((dict(X=None), b"null pointer"), (dict(W=None), b"null pointer"), (dict(bias=None), b"null pointer"), (dict(Y=None), b"null pointer"),
                     (dict(K=62), b"multiple of 4"), (dict(K=0), b"bad shape"), (dict(N=0), b"bad shape"),
                     (dict(cap=-1), b"bad shape"), (dict(cap=0), b"bad shape"), (dict(B=-2), b"bad shape"), (dict(B=0), b"bad shape"),
                     (dict(ldy=60), b"ldy"),
                     (dict(X2=p, Ksplit=16), b"Ksplit"), (dict(X2=p, Ksplit=48), b"Ksplit"), (dict(X2=p, Ksplit=0), b"Ksplit"), (dict(X2=p, Ksplit=64), b"Ksplit"),
                     (dict(epi=2), b"epi"), (dict(epi=-1), b"epi"), (dict(epi=1, resid=p + 4), b"resid"), (dict(epi=0, resid=p), b"resid")):
        assert lin(**kw) == -1 and word in L.einx_last_error() and b"einx_lg_linear_f16" in L.einx_last_error(), (kw, L.einx_last_error())

    layers = (LIB.LgLayer * 2)()
    w = LIB.LgWeights()
    w.struct_size, w.layer_size = ctypes.sizeof(LIB.LgWeights), ctypes.sizeof(LIB.LgLayer)
    w.n_layers, w.layers = 2, ctypes.cast(layers, ctypes.POINTER(LIB.LgLayer))
    heads = (LIB.LgHead * 2)()
    hs = ctypes.sizeof(LIB.LgHead)

    def rc(mode=2, heads_=heads, head_size=hs, depth=-1.0, width=-1.0, la=None, live=p, stop=p, ref_layers=1, wp=ctypes.byref(w)):
        return L.einx_lightglue_mp(wp, heads_, head_size, depth, width, 0, *([None] * 3), 64, *([None] * 3), 64, 2, 1.0, 1.0, 1.0, 1.0, p,
                                   *([None] * 4), la, None, None, ref_layers, stop, p, p, p, p, live, mode, None)

    named = lambda: b"einx_lightglue_mp" in L.einx_last_error()  # noqa: E731
    assert rc(wp=None) == -1 and b"null pointer" in L.einx_last_error() and named()
    for mode in (4, -1, 7):
        assert rc(mode=mode) == -1 and b"mode" in L.einx_last_error() and named()
    # EINX_LG_LIN_F16: the pack must be unfolded and carry the binary16 images
    assert rc() == -1 and b"unfolded" in L.einx_last_error() and named()
    for lay in layers:
        lay.Wo = lay.bo = lay.Wco = lay.bco = p
    assert rc() == -1 and b"binary16 image" in L.einx_last_error() and named()
    for lay in layers[:1]:
        for name in LIB.LgLayer._names[-10:]:
            setattr(lay, name, p)
    assert rc() == -1 and b"binary16 image" in L.einx_last_error() and named()  # (the second layer)
    w.layer_size -= 8
    assert rc() == -1 and b"layer_size" in L.einx_last_error() and named()
    w.layer_size += 8
    for name in LIB.LgLayer._names[-10:-1]:  # (Wqk_v_h is optional)
        setattr(layers[1], name, p)
    # from here the entries' own rules, reported under this entry's name
    for kw, word in ((dict(width=0.5, live=None), b"null pointer"), (dict(width=0.5, head_size=hs + 8), b"head_size"),
                     (dict(width=1.5), b"width_confidence"), (dict(width=0.5, la=p), b"log_assignment"), (dict(width=0.5, ref_layers=2), b"ref_layers"),
                     (dict(width=0.5), b"log_assignment head"), (dict(depth=0.9, stop=None), b"null pointer"),
                     (dict(depth=0.9, ref_layers=2), b"ref_layers"), (dict(depth=0.9), b"log_assignment head")):
        for mode in (2, 3):
            assert rc(mode=mode, **kw) == -1 and word in L.einx_last_error() and named(), (kw, L.einx_last_error())
    assert rc(heads_=None, stop=None, live=None) == -1 and b"null pointer" in L.einx_last_error()  # the plain run: kpts0 is null


@pytest.mark.parametrize("flash", [False, True])
@pytest.mark.parametrize("adaptive", ["prune", "stop", "both"])
def test_adaptive_cases_are_out_of_the_roundings_reach(adaptive, flash):
    """the model and pairs tests/test_lg_mp_gpu.py runs with early stopping and point pruning (those of tests/test_lg_flash_gpu.py,
    biases chosen there): under this contract too the two peers take the spec's decisions with the margins lg_mp_ref.safe_refs
    asks for, so that no case has to be left out on the GPU; and something stops / is pruned in every case"""
    WIDTH, DEPTH, MSHIFT, TSHIFT, LAYERS = 0.99, 0.9, {1: -5.4918}, {5: 5.0}, 9  # tests/test_lg_flash_gpu.py
    prune, stop = adaptive != "stop", adaptive != "prune"
    sd = lgf64_shipped_state_dict(7)
    for i, s in (MSHIFT if prune else {}).items():
        sd[f"log_assignment.{i}.matchability.bias"] = sd[f"log_assignment.{i}.matchability.bias"] + np.float32(s)
    for i, s in (TSHIFT if stop else {}).items():
        sd[f"token_confidence.{i}.token.0.bias"] = sd[f"token_confidence.{i}.token.0.bias"] + np.float32(s)
    did = 0
    for seed, n, m in ((11, 31, 33), (11, 64, 64)):
        spec = MR.safe_refs(adaptive, sd, _pair(seed, n, m), WIDTH if prune else -1, DEPTH if stop else -1, flash)["spec"]
        did += bool(stop and spec["stop"] < LAYERS) + bool(prune and (spec["live"][0] < n or spec["live"][1] < m))
    assert did > 0

"""The refusal contract of the LightGlue C ABI: for each of the five run entries (einx_lightglue, _early_stop, _adaptive, _flash,
_mp) and the two test hooks (einx_lg_linear_f16, einx_lg_attention_f16) a fixed list of bad calls, each with the return code and the
COMPLETE einx_last_error() string it gives.  The strings were recorded from the library before the entries were moved onto one call
record (LgCall): the text, the entry a message is reported under and the order in which the checks fire are part of
the ABI.  Several calls are wrong in two ways at once, so that the order is visible.  Every check comes before any launch: no GPU."""
import ctypes
from importlib import import_module

import pytest

from helpers import load_pkg

pkg = load_pkg()
LIB = import_module(pkg.__name__ + "._lib")
L = pkg.native.lib()

_one = ctypes.c_float(0)
P = ctypes.addressof(_one)  # a non-null pointer nothing reads: every call below is refused before it is used
HS = ctypes.sizeof(LIB.LgHead)
N_LAYERS = 2


def _weights(kw):
    """a complete einx_lg_weights (d = 256, 4 heads, 2 layers, every layer pointer set), then the call's faults"""
    layers = (LIB.LgLayer * N_LAYERS)()
    for lay in layers:
        for name in LIB.LgLayer._names:
            setattr(lay, name, P)
        for name in kw.get("layer_null", ()):
            setattr(lay, name, None)
    w = LIB.LgWeights()
    w.struct_size, w.layer_size = ctypes.sizeof(LIB.LgWeights) + kw.get("struct_size_off", 0), ctypes.sizeof(LIB.LgLayer)
    w.n_layers, w.heads, w.d, w.input_dim = kw.get("n_layers", N_LAYERS), 4, kw.get("d", 256), kw.get("input_dim", 256)
    w.in_w = kw.get("in_w")
    w.layers = layers
    heads = (LIB.LgHead * N_LAYERS)()
    for h in heads:
        for name, _ in LIB.LgHead._fields_:
            setattr(h, name, P)
        for name in kw.get("head_null", ()):
            setattr(h, name, None)
    return w, layers, heads


def _run(entry, kw):
    w, layers, heads = _weights(kw)
    a = dict(w=ctypes.byref(w), heads=heads, head_size=HS, depth=0.0, width=0.0, min_kpts=0, kpts0=P, cap0=64, B=2, ws=P, la=None, ref_layers=0,
             stop=P, live=P, mode=0)
    a.update({k: v for k, v in kw.items() if k in a})
    pair = (a["kpts0"], P, P, a["cap0"], P, P, P, 64, a["B"], 1.0, 1.0, 1.0, 1.0, a["ws"], P, P, P, P, a["la"], None, None)
    es = (a["w"], a["heads"], a["head_size"], a["depth"])
    prune = (a["stop"], P, P, P, P, a["live"])
    if entry == "einx_lightglue":
        rc = L.einx_lightglue(a["w"], *pair, a["ref_layers"], None)
    elif entry == "einx_lightglue_early_stop":
        rc = L.einx_lightglue_early_stop(*es, *pair, a["stop"], None)
    elif entry == "einx_lightglue_adaptive":
        rc = L.einx_lightglue_adaptive(*es, a["width"], a["min_kpts"], *pair, *prune, None)
    elif entry == "einx_lightglue_flash":
        rc = L.einx_lightglue_flash(*es, a["width"], a["min_kpts"], *pair, a["ref_layers"], *prune, None)
    else:
        rc = L.einx_lightglue_mp(*es, a["width"], a["min_kpts"], *pair, a["ref_layers"], *prune, a["mode"], None)
    return rc, L.einx_last_error().decode()


def _linear_f16(kw):
    a = dict(X=P, X2=None, Ksplit=0, K=64, W16=P, bias=P, N=64, Y=P, ldy=64, resid=None, cnt=None, cap=8, B=1, epi=0)
    a.update(kw)
    rc = L.einx_lg_linear_f16(*[a[k] for k in ("X", "X2", "Ksplit", "K", "W16", "bias", "N", "Y", "ldy", "resid", "cnt", "cap", "B", "epi")], None)
    return rc, L.einx_last_error().decode()


def _attention_f16(kw):
    a = dict(Q=P, K=P, V=P, O=P, nq=P, nk=P, capq=8, capk=8, B=2, heads=4, dh=64, ld=256, kv_shift=0)
    a.update(kw)
    rc = L.einx_lg_attention_f16(*[a[k] for k in ("Q", "K", "V", "O", "nq", "nk", "capq", "capk", "B", "heads", "dh", "ld", "kv_shift")], None)
    return rc, L.einx_last_error().decode()


NULL = "null pointer"
ABI = "einx_lg_weights::struct_size / layer_size do not match this library (header / library ABI mismatch)"
HEAD_SIZE = "head_size does not match this library's einx_lg_head (header / library ABI mismatch)"
NO_LA = "log_assignment is not produced with point pruning (DESIGN.md 8j): la must be null"
REF_PRUNE = "point pruning returns the surviving rows, not every layer's: ref_layers must be 0 or 1"
REF_STOP = "early stopping returns the rows the stopping head read: ref_layers must be 0 or 1"
TOKEN = "every layer but the last needs its token_confidence head"
IMAGES = ("Wqkv_h",)

# (entry, the call's faults, return code, the message after "<reporting function>: ", the reporting function when it is not the entry)
RUN_CASES = [
    # the shared body's checks, in their order (reported under lg_run)
    ("einx_lightglue", dict(kpts0=None), -1, NULL, "lg_run"),
    ("einx_lightglue", dict(w=None), -1, NULL, "lg_run"),
    ("einx_lightglue", dict(kpts0=None, B=0), -1, NULL, "lg_run"),
    ("einx_lightglue", dict(d=250), -1, "descriptor_dim must be num_heads x head_dim with head_dim a multiple of 4, at most 256", "lg_run"),
    ("einx_lightglue", dict(d=250, struct_size_off=8), -1, "descriptor_dim must be num_heads x head_dim with head_dim a multiple of 4, at most 256", "lg_run"),
    ("einx_lightglue", dict(struct_size_off=8, n_layers=0), -1, ABI, "lg_run"),
    ("einx_lightglue", dict(n_layers=0, B=0), -1, "no layers", "lg_run"),
    ("einx_lightglue", dict(B=0, input_dim=6), -1, "bad shape", "lg_run"),
    ("einx_lightglue", dict(cap0=0), -1, "bad shape", "lg_run"),
    ("einx_lightglue", dict(input_dim=6, in_w=P), -1, "input_dim must be a multiple of 4", "lg_run"),
    ("einx_lightglue", dict(in_w=P, ref_layers=5), -1, "input_proj must be given exactly when input_dim != d", "lg_run"),
    ("einx_lightglue", dict(input_dim=128), -1, "input_proj must be given exactly when input_dim != d", "lg_run"),
    ("einx_lightglue", dict(ref_layers=5), -1, "ref_layers must be 0/1 (last layer) or n_layers", "lg_run"),
    # early stopping: its own checks under the entry, then the shared body
    ("einx_lightglue_early_stop", dict(stop=None, head_size=HS + 8), -1, NULL, None),
    ("einx_lightglue_early_stop", dict(heads=None), -1, NULL, None),
    ("einx_lightglue_early_stop", dict(head_size=HS + 8, n_layers=33), -1, HEAD_SIZE, None),
    ("einx_lightglue_early_stop", dict(n_layers=33, head_null=("proj_w",)), -1, "early stopping takes 1..32 layers", None),
    ("einx_lightglue_early_stop", dict(head_null=("match_b", "token_w")), -1, "every layer needs its log_assignment head", None),
    ("einx_lightglue_early_stop", dict(head_null=("token_b",), kpts0=None), -1, TOKEN, None),
    ("einx_lightglue_early_stop", dict(kpts0=None), -1, NULL, "lg_run"),
    ("einx_lightglue_early_stop", dict(ws=None, B=0), -1, NULL, "lg_run"),
    # point pruning
    ("einx_lightglue_adaptive", dict(width=0.5, live=None, head_size=HS + 8), -1, NULL, None),
    ("einx_lightglue_adaptive", dict(width=0.5, head_size=HS + 8, la=P), -1, HEAD_SIZE, None),
    ("einx_lightglue_adaptive", dict(width=0.5, n_layers=33, la=P), -1, "point pruning takes 1..32 layers", None),
    ("einx_lightglue_adaptive", dict(width=1.5, la=P), -1, "width_confidence must be in (0, 1]", None),
    ("einx_lightglue_adaptive", dict(width=0.0), -1, "width_confidence must be in (0, 1]", None),
    ("einx_lightglue_adaptive", dict(width=0.5, la=P, head_null=("proj_b",)), -1, NO_LA, None),
    ("einx_lightglue_adaptive", dict(width=0.5, head_null=("proj_b",)), -1, "every layer needs its log_assignment head", None),
    ("einx_lightglue_adaptive", dict(width=0.5, depth=0.5, head_null=("token_w",)), -1, "with depth_confidence > 0 " + TOKEN, None),
    ("einx_lightglue_adaptive", dict(width=0.5, depth=-1.0, head_null=("token_w",), kpts0=None), -1, NULL, "lg_run"),
    ("einx_lightglue_adaptive", dict(width=0.5, stop=None, cap0=0), -1, "bad shape", "lg_run"),
    # flash: the dispatch's own refusals, then those of the run it picks, all under einx_lightglue_flash
    ("einx_lightglue_flash", dict(width=0.5, ref_layers=2, live=None), -1, REF_PRUNE, None),
    ("einx_lightglue_flash", dict(width=0.5, head_size=HS + 8, la=P), -1, HEAD_SIZE, None),
    ("einx_lightglue_flash", dict(width=0.5, live=None), -1, NULL, None),
    ("einx_lightglue_flash", dict(width=0.5, depth=0.5, la=P), -1, NO_LA, None),
    ("einx_lightglue_flash", dict(depth=0.5, ref_layers=2, stop=None), -1, REF_STOP, None),
    ("einx_lightglue_flash", dict(depth=0.5, stop=None), -1, NULL, None),
    ("einx_lightglue_flash", dict(depth=0.5, ref_layers=1, head_null=("token_w",)), -1, TOKEN, None),
    ("einx_lightglue_flash", dict(ref_layers=5, heads=None, stop=None, live=None), -1, "ref_layers must be 0/1 (last layer) or n_layers", "lg_run"),
    ("einx_lightglue_flash", dict(w=None), -1, NULL, "lg_run"),
    ("einx_lightglue_flash", dict(width=0.5, w=None), -1, NULL, None),
    # mp: its own checks first
    ("einx_lightglue_mp", dict(w=None, mode=4), -1, NULL, None),
    ("einx_lightglue_mp", dict(mode=4, struct_size_off=8), -1, "mode takes EINX_LG_ATTN_F16 | EINX_LG_LIN_F16 only", None),
    ("einx_lightglue_mp", dict(mode=2, struct_size_off=8, n_layers=0), -1, ABI, None),
    ("einx_lightglue_mp", dict(mode=3, n_layers=0), -1, "no layers", None),
    ("einx_lightglue_mp", dict(mode=2, layer_null=("Wo", "Wqkv_h")), -1, "linears in fp16 take unfolded weights: every layer needs Wo / bo / Wco / bco", None),
    ("einx_lightglue_mp", dict(mode=2, layer_null=IMAGES, width=0.5, ref_layers=2), -1, "linears in fp16 need the binary16 image of every layer's nine weights", None),
    ("einx_lightglue_mp", dict(mode=2, layer_null=("Wqk_v_h",), width=0.5, ref_layers=2), -1, REF_PRUNE, None),
    ("einx_lightglue_mp", dict(mode=1, layer_null=IMAGES, depth=0.5, ref_layers=2), -1, REF_STOP, None),
    ("einx_lightglue_mp", dict(mode=1, struct_size_off=8, n_layers=0, kpts0=None), -1, NULL, "lg_run"),
    ("einx_lightglue_mp", dict(mode=3, width=0.5, head_size=HS + 8, la=P), -1, HEAD_SIZE, None),
    ("einx_lightglue_mp", dict(mode=0, depth=0.5, stop=None), -1, NULL, None),
    ("einx_lightglue_mp", dict(mode=1, n_layers=33, depth=0.5), -1, "early stopping takes 1..32 layers", None),  # (mode 2 would walk 33 layers)
]

K_MSG = "bad shape (K must be a multiple of 4)"
HOOK_CASES = [
    (_linear_f16, "einx_lg_linear_f16", dict(X=None, K=6), -1, NULL),
    (_linear_f16, "einx_lg_linear_f16", dict(W16=None), -1, NULL),
    (_linear_f16, "einx_lg_linear_f16", dict(K=6, ldy=8), -1, K_MSG),
    (_linear_f16, "einx_lg_linear_f16", dict(B=0), -1, K_MSG),
    (_linear_f16, "einx_lg_linear_f16", dict(ldy=63, epi=2), -1, "ldy must be at least N"),
    (_linear_f16, "einx_lg_linear_f16", dict(X2=P, Ksplit=16, epi=2), -1, "Ksplit must be a multiple of the 32-deep K slab inside (0, K)"),
    (_linear_f16, "einx_lg_linear_f16", dict(X2=P, Ksplit=64), -1, "Ksplit must be a multiple of the 32-deep K slab inside (0, K)"),
    (_linear_f16, "einx_lg_linear_f16", dict(epi=2, resid=P), -1, "epi must be 0 (bias) or 1 (bias + residual)"),
    (_linear_f16, "einx_lg_linear_f16", dict(epi=0, resid=P), -1, "resid is read by epi 1 only: with epi 0 it must be null"),
    (_linear_f16, "einx_lg_linear_f16", dict(epi=1, resid=P + 4), -1, "the residual is accumulated in place: resid must be Y (or null)"),
    (_attention_f16, "einx_lg_attention_f16", dict(nk=None, B=0), -1, NULL),
    (_attention_f16, "einx_lg_attention_f16", dict(capk=0, dh=6), -1, "bad shape"),
    (_attention_f16, "einx_lg_attention_f16", dict(dh=6, ld=8), -1, "head_dim must be a multiple of 4, at most 256"),
    (_attention_f16, "einx_lg_attention_f16", dict(dh=260), -1, "head_dim must be a multiple of 4, at most 256"),
    (_attention_f16, "einx_lg_attention_f16", dict(heads=0), -1, "head_dim must be a multiple of 4, at most 256"),
    (_attention_f16, "einx_lg_attention_f16", dict(ld=252, kv_shift=2), -1, "ld must be a multiple of 4, at least heads x head_dim"),
    (_attention_f16, "einx_lg_attention_f16", dict(ld=258), -1, "ld must be a multiple of 4, at least heads x head_dim"),
    (_attention_f16, "einx_lg_attention_f16", dict(kv_shift=2), -1, "kv_shift must be in [0, B)"),
    (_attention_f16, "einx_lg_attention_f16", dict(kv_shift=-1), -1, "kv_shift must be in [0, B)"),
]


@pytest.mark.parametrize("case", RUN_CASES, ids=lambda c: f"{c[0]}-{'+'.join(c[1])}")
def test_run_entries_refuse_in_the_recorded_order_with_the_recorded_text(case):
    entry, faults, rc, msg, reported = case
    assert _run(entry, faults) == (rc, f"{reported or entry}: {msg}")


@pytest.mark.parametrize("case", HOOK_CASES, ids=lambda c: f"{c[1]}-{'+'.join(c[2])}")
def test_hooks_refuse_in_the_recorded_order_with_the_recorded_text(case):
    call, entry, faults, rc, msg = case
    assert call(faults) == (rc, f"{entry}: {msg}")


def test_every_entry_and_hook_is_covered_and_the_two_double_faults_are_there():
    assert {c[0] for c in RUN_CASES} == {"einx_lightglue", "einx_lightglue_early_stop", "einx_lightglue_adaptive", "einx_lightglue_flash",
                                         "einx_lightglue_mp"}
    assert {c[1] for c in HOOK_CASES} == {"einx_lg_linear_f16", "einx_lg_attention_f16"}
    assert ("einx_lightglue_mp", dict(w=None, mode=4), -1, NULL, None) in RUN_CASES  # null w plus bad mode
    assert any(c[1] == dict(width=0.5, head_size=HS + 8, la=P) for c in RUN_CASES)  # bad head_size plus la set with pruning

"""GPU tests (-m gpu), component: the opt-in fp16 convolutions (conv_f16_kernel, einx_conv_block_f16, `half_precision`).
The judge is the contract's float64 restatement (tests/conv_f16_ref.py `spec`).  The kernel alone first: bit for bit against the
oracle-exact einx_conv_block on inputs whose answer is exact in every accumulation order, on values that tell the rounding modes
apart, and on random inputs under the a-priori bound of K fp32 additions.  Then the switch: off is today's forward bit for bit, on
follows the contract within the project's rule (twice the worse of two independent fp32 peers against the spec, plus 4 ulp)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import conv_f16_ref as R
from gpu_support import DEV, _eim_model, _np, _t, pkg
from helpers import synth, synth_raw_events

pytestmark = pytest.mark.gpu
N = pkg.native
LIB = pkg._lib
GUARD = 256  # elements before and behind every buffer (a multiple of 8: the buffers stay 16-byte aligned)
MARK = -77.0


# ------------------------------------------------------------------------------------------------ the kernel hook
class Guarded:
    """`n` elements on the device between two guard zones of MARK"""

    def __init__(self, n, dtype=torch.float32, fill=None):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), MARK, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]
        if fill is not None:
            self.t.copy_(fill.reshape(-1).to(DEV).to(dtype)) if torch.is_tensor(fill) else self.t.fill_(fill)

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool((self.buf[:GUARD].float() == MARK).all()) and bool((self.buf[GUARD + self.n:].float() == MARK).all())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Hook:
    """one layer on the device behind guard zones; run() -> out [B,cout,Ho,Wo] (CPU), NaN where the kernel did not write"""

    def __init__(self, x, w, bias=None, scale=None, shift=None, relu=False, pool=False):
        L = N.lib()
        self.B, self.cin, self.H, self.W = x.shape
        self.cout, _, self.ks, _ = w.shape
        self.relu, self.pool = relu, pool
        self.x = Guarded(x.numel(), fill=x)
        w_src = Guarded(w.numel(), fill=w)
        self.w16 = Guarded(L.einx_conv_weight_elems_f16(self.cin, self.cout, self.ks), torch.float16)
        rc = L.einx_conv_repack_f16(w_src.ptr(), self.cin, self.cout, self.ks, self.w16.ptr(), _stream())
        assert rc == 0, L.einx_last_error()
        torch.cuda.synchronize()
        assert w_src.intact() and self.w16.intact(), "repack wrote outside the image"
        g = lambda v: None if v is None else Guarded(v.numel(), fill=v)  # noqa: E731
        self.bias, self.scale, self.shift = g(bias), g(scale), g(shift)
        p = lambda v: None if v is None else v.t.data_ptr()  # noqa: E731
        self.desc = LIB.ConvDescF16(ctypes.sizeof(LIB.ConvDescF16), self.w16.t.data_ptr(), p(self.bias), p(self.scale), p(self.shift),
                                    self.cin, self.cout, self.ks, int(relu), int(pool))
        self.Ho, self.Wo = (self.H // 2, self.W // 2) if pool else (self.H, self.W)
        self.out = Guarded(self.B * self.cout * self.Ho * self.Wo)

    def launch(self):
        L = N.lib()
        rc = L.einx_conv_block_f16(self.x.ptr(), self.B, self.H, self.W, ctypes.byref(self.desc), self.out.ptr(), _stream())
        assert rc == 0, L.einx_last_error()

    def buffers(self):
        return [b for b in (self.x, self.w16, self.bias, self.scale, self.shift, self.out) if b is not None]

    def result(self, tag):
        torch.cuda.synchronize()
        assert all(b.intact() for b in self.buffers()), (tag, "a guard zone was written")
        return self.out.t.view(self.B, self.cout, self.Ho, self.Wo).cpu()

    def run(self, tag=None):
        self.out.t.fill_(float("nan"))
        self.launch()
        return self.result(tag)

    def run_graph(self, tag=None):
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            self.launch()  # warm-up on the capture stream
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            self.launch()
        self.out.t.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        return self.result(tag)


def _fp32(x, w, bias, scale, shift, relu, pool):
    """einx_conv_block on the same operands, and the name it launched"""
    out = R.peer_b(N, x, w, bias, scale, shift, relu, pool, rounding=False, dev=DEV)
    return out, N.lib().einx_conv_last_kernel().decode()


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _exact_operands(rng, B, cin, cout, H, W, ks):
    """integers in [-4, 4] and multiples of 1/16 in [-1, 1]: every partial sum is a multiple of 1/16 below 2^14, exact in fp32 in any
    order, and every operand is a binary16 value; the affine's scales are signed powers of two"""
    x = torch.from_numpy(rng.integers(-4, 5, (B, cin, H, W)).astype(np.float32))
    w = torch.from_numpy((rng.integers(-16, 17, (cout, cin, ks, ks)) / 16.0).astype(np.float32))
    bias = torch.from_numpy((rng.integers(-64, 65, cout) / 16.0).astype(np.float32))
    scale = torch.from_numpy((rng.choice([0.5, 1.0, 2.0, -1.0, -0.25], cout)).astype(np.float32))
    shift = torch.from_numpy((rng.integers(-64, 65, cout) / 16.0).astype(np.float32))
    return x, w, bias, scale, shift


def _plan(cin, cout, ks, pool, B, H, W):
    s = N.lib().einx_conv_f16_plan(cin, cout, ks, int(pool), B, H, W)
    return None if s is None else s.decode()


def _check_exact(tag, B, cin, cout, H, W, ks, relu, bn, pool, graph):
    rng = np.random.default_rng(abs(hash((B, cin, cout, H, W, ks))) % (2 ** 31))
    x, w, bias, scale, shift = _exact_operands(rng, B, cin, cout, H, W, ks)
    if not bn:
        scale = shift = None
    want, name32 = _fp32(x, w, bias, scale, shift, relu, pool)
    h = Hook(x, w, bias, scale, shift, relu, pool)
    a = h.run(tag)
    assert N.lib().einx_conv_f16_last_kernel().decode() == _plan(cin, cout, ks, pool, B, H, W) and "conv_f16" not in name32
    assert not torch.isnan(a).any(), (tag, "outputs left unwritten")
    assert _bits_equal(a, want), (tag, int((a != want).sum()), float((a - want).abs().max()))
    assert _bits_equal(h.run(tag), a), (tag, "second run differs")
    if graph:
        assert _bits_equal(h.run_graph(tag), a), (tag, "graph replay differs")


EXACT_CASES = [
    # B, cin, cout, H, W, ks, pool allowed
    (2, 8, 64, 10, 12, 3, True),      # half a chunk of channels
    (1, 64, 64, 24, 40, 3, True),     # pooled backbone layer shape, two tile columns
    (3, 64, 128, 33, 44, 3, False),   # odd map, two channel tiles
    (1, 128, 256, 33, 44, 3, False),  # eight chunks, four channel tiles
    (1, 256, 65, 33, 44, 1, False),   # the detector's 65 channels on two channel tiles
    (1, 256, 256, 7, 9, 1, False),    # a quarter of a pixel run
    (1, 72, 96, 17, 70, 3, False),    # ragged cin against the 16-channel chunk, ragged cout against 64
]


@pytest.mark.parametrize("case", EXACT_CASES, ids=lambda c: "x".join(str(v) for v in c[:6]))
def test_exact_inputs_bit_for_bit(case):
    """einx_conv_block_f16 == einx_conv_block on operands where no order of summation and neither rounding can matter; ReLU, BN and
    pool crossed; NaN prefill fully overwritten, guard zones before and behind all six buffers untouched; twice and on graph replay"""
    B, cin, cout, H, W, ks, pool_ok = case
    for relu, bn, pool in itertools.product((False, True), (False, True), (False, True) if pool_ok else (False,)):
        if case[:6] == (1, 256, 65, 33, 44, 1) and relu:
            continue  # the issue's case: no ReLU
        _check_exact(("exact", case, relu, bn, pool), B, cin, cout, H, W, ks, relu, bn, pool, graph=(relu and bn))
    if case[:6] == (1, 256, 65, 33, 44, 1):
        _check_exact(("exact", case, "graph"), B, cin, cout, H, W, ks, False, False, False, graph=True)


TILE_EDGES = [(3, False, [7, 8, 9], [31, 32, 33]), (3, True, [6, 8, 10], [30, 32, 34]), (1, False, [1], [255, 256, 257])]


@pytest.mark.parametrize("ks,pool,Hs,Ws", TILE_EDGES, ids=["3x3 8x32", "3x3 8x32 pool", "1x1 256"])
def test_every_tile_shape_below_at_and_above_the_tile(ks, pool, Hs, Ws):
    """the dispatcher names three instantiations: the 8x32 tile plain and pooled (pooled: the nearest even sizes) and the 256-pixel
    run; H and W one less than, equal to and one more than the tile"""
    names = set()
    for H, W in itertools.product(Hs, Ws):
        _check_exact(("edge", ks, pool, H, W), 2, 16, 64, H, W, ks, True, True, pool, graph=False)
        names.add(N.lib().einx_conv_f16_last_kernel().decode())
    assert len(names) == 1 and names == {_plan(16, 64, ks, pool, 2, Hs[0], Ws[0])}


def _tie_values():
    e = 2.0 ** -11
    vals = [1 + e, 1 + 3 * e, -(1 + e), -(1 + 3 * e), 1 + e + 2.0 ** -20, 1 + e - 2.0 ** -20, 2048 + 1, 2048 + 3, 65519.0, -65519.0, 65504.0, 0.0]
    rng = np.random.default_rng(5)
    for ex in range(-14, 16):  # every normal binade of binary16, both signs
        vals += list(((1 + rng.random(6)) * 2.0 ** ex * rng.choice([-1, 1], 6)))
    return np.asarray(vals, np.float32)


def test_the_rounding_is_nearest_even_with_overflow_to_infinity():
    """1x1, 8 inputs, 0/1 selection weights: the output is the rounded input, bit for bit x.half().float().  1 + 2^-11 is a tie and goes
    to the even 1; 1 + 3 2^-11 is a tie and goes to the even 1 + 2^-9 (round toward zero gives 1 + 2^-10); 65519 is below the
    overflow threshold and gives 65504, 65520 is the threshold and gives +inf.  The same for the weights, with an input of 1."""
    v = _tie_values()
    n = (len(v) + 7) // 8 * 8
    x = torch.zeros(1, 8, 1, n // 8 + 2)
    x[0, :, 0, :n // 8] = torch.from_numpy(np.resize(v, n)).view(n // 8, 8).t()
    got = Hook(x, torch.eye(8).view(8, 8, 1, 1)).run("rounding x")
    assert _bits_equal(got, x.half().float())
    assert float(R.rh(torch.tensor(1 + 2.0 ** -11))) == 1.0 and float(R.rh(torch.tensor(1 + 3 * 2.0 ** -11))) == 1 + 2.0 ** -9
    # overflow: one nonzero input channel under all-ones weights (a 0 weight would meet the infinity: 0 x inf = NaN)
    x = torch.zeros(1, 8, 1, 4)
    x[0, 0, 0] = torch.tensor([65519.0, 65520.0, -65520.0, 70000.0])
    got = Hook(x, torch.ones(8, 8, 1, 1)).run("overflow x")
    assert got[0, :, 0].tolist() == [[65504.0, float("inf"), float("-inf"), float("inf")]] * 8
    # the weights: input 1 in channel 0 only, the values down column 0 of W
    vw = np.concatenate([v, np.asarray([65520.0, -65520.0], np.float32)])
    w = torch.zeros(len(vw), 8, 1, 1)
    w[:, 0, 0, 0] = torch.from_numpy(vw)
    x = torch.zeros(1, 8, 1, 3)
    x[0, 0] = 1.0
    got = Hook(x, w).run("rounding w")
    want = torch.from_numpy(vw).half().float()
    assert torch.isinf(want[-2:]).all() and all(_bits_equal(got[0, :, 0, i], want) for i in range(3))


def test_probe_operands_below_the_normal_range_recorded_not_gated():
    """Outside the contract (as 8l): inputs of 2^-15, 2^-24, 3 x 2^-24 and 1023 x 2^-24 under a 0/1 selection weight, and
    a weight of 2^-20 under inputs of 1024, both signs.  Recorded at every run: the distance from x.half().float() (0 = binary16
    subnormals are produced by the convert and kept by the instruction).  Nothing is asserted about the values."""
    v = torch.tensor([2.0 ** -15, 2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24, -(2.0 ** -15), -(2.0 ** -24), -3 * 2.0 ** -24, -1023 * 2.0 ** -24])
    x = torch.zeros(1, 8, 1, 2)
    x[0, :, 0, 0] = v
    got = Hook(x, torch.eye(8).view(8, 8, 1, 1)).run("subnormal x")[0, :, 0, 0]
    d_in = float((got - v.half().float()).abs().max())
    w = torch.zeros(8, 8, 1, 1)
    w[:, 0, 0, 0] = torch.tensor([2.0 ** -20, -(2.0 ** -20)] * 4)
    x = torch.zeros(1, 8, 1, 2)
    x[0, 0] = 1024.0
    got = Hook(x, w).run("subnormal w")[0, :, 0, 0]
    d_w = float((got - w[:, 0, 0, 0].half().float() * 1024.0).abs().max())
    print(f"conv_f16 operands below 2^-14: distance from x.half().float(): inputs {d_in:.3e}, weights {d_w:.3e} (0 = subnormals kept)")
    assert torch.isfinite(got).all()


RANDOM_CASES = [(2, 64, 64, 24, 40, True), (1, 128, 128, 33, 44, False)]


@pytest.mark.parametrize("case", RANDOM_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_random_inputs_against_the_spec(case):
    """|kernel - spec| <= K 2^-24 sum|x w| (K = 9 cin fp32 additions in any order), carried through the affine by |scale|, + 4 ulp of
    the value; against peer B (einx_conv_block on the pre-rounded operands: the same exact products in another order) twice that.
    Measured share of the bound on an MI355X: 0.0031 / 0.0013 against the spec, 0.0039 / 0.0019 of twice the bound against peer B."""
    B, cin, cout, H, W, pool = case
    rng = np.random.default_rng(100 + cin)
    x = torch.from_numpy(rng.standard_normal((B, cin, H, W)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32))
    bias = torch.from_numpy(rng.standard_normal(cout).astype(np.float32))
    scale = torch.from_numpy((0.5 + rng.random(cout)).astype(np.float32) * rng.choice([-1, 1], cout).astype(np.float32))
    shift = torch.from_numpy(rng.standard_normal(cout).astype(np.float32))
    got = Hook(x, w, bias, scale, shift, True, pool).run("random").double()
    want = R.spec(x, w, bias, scale, shift, True, pool)
    peer = R.peer_b(N, x, w, bias, scale, shift, True, pool, dev=DEV).double()
    bnd = R.bound(x, w, want, scale, pool)
    share_spec, share_peer = float(((got - want).abs() / bnd).max()), float(((got - peer).abs() / (2 * bnd)).max())
    print(f"conv_f16 random {case}: share of the bound {share_spec:.4f} (spec), {share_peer:.4f} (peer B, twice the bound); "
          f"max |err| {float((got - want).abs().max()):.3e}")
    assert share_spec <= 1.0 and share_peer <= 1.0


def test_refusals_by_name():
    L = N.lib()
    x, w = torch.zeros(1, 16, 8, 8), torch.zeros(64, 16, 3, 3)
    h = Hook(x, w)

    def refused(what, desc=None, inp=True, out=True, H=8, W=8):
        d = h.desc if desc is None else desc
        rc = L.einx_conv_block_f16(h.x.ptr() if inp else None, 1, H, W, ctypes.byref(d) if d is not False else None, h.out.ptr() if out else None,
                                   _stream())
        assert rc != 0 and what.encode() in L.einx_last_error(), (what, rc, L.einx_last_error())

    def desc(**kw):
        d = LIB.ConvDescF16.from_buffer_copy(h.desc)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    refused("cin must be a multiple of 8", desc(cin=12))
    refused("kernel size must be 1 or 3", desc(ks=5))
    refused("pooling needs even H and W", desc(pool=1), H=7, W=8)
    refused("pooling needs even H and W", desc(pool=1), H=8, W=7)
    refused("null pointer", inp=False)
    refused("null pointer", out=False)
    refused("null pointer", desc=False)
    refused("null pointer", desc(w_f16=None))
    refused("struct_size", desc(struct_size=ctypes.sizeof(LIB.ConvDescF16) - 8))
    torch.cuda.synchronize()
    assert all(b.intact() for b in h.buffers())


# ------------------------------------------------------------------------------------------------ the switch
H_, W_, B_ = 40, 48, 2


def _model(seed=21):
    cfg, model, sd = _eim_model("SP_MNN", seed)
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        ext.detection_top_k = 64
    return model


def _inputs(seed=31):
    ev, mask = synth.synth_events(seed, B_, 5, H_, W_)
    img = synth.synth_image(seed, B_, H_, W_)
    return _t(ev), _t(mask), img


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(u, v) for u, v in zip(a, b))
    return a == b


def _forward(model, ev, mask, img):
    ef, imf, m = model(ev, _t(img.copy()), mask)
    names = (N.lib().einx_conv_last_kernel().decode(), N.lib().einx_conv_f16_last_kernel().decode())
    return dict(ef.items()), dict(imf.items()), m, names


def test_off_is_off():
    """attribute false, attribute switched on and off again (and, for the network without BatchNorm, on in train mode: not active),
    and never set: every key of both dicts and the matches torch.equal, the same fp32 instantiation launched last"""
    ev, mask, img = _inputs()
    never = _model()
    base = _forward(never, ev, mask, img)
    off = _model()
    toggled = _model()
    for ext in (off.event_extractor.extractor, off.image_extractor.extractor):
        ext.half_precision = False
    for ext in (toggled.event_extractor.extractor, toggled.image_extractor.extractor):
        ext.half_precision = True
    assert toggled.image_extractor.extractor.conv_mode == "fp16"
    on = _forward(toggled, ev, mask, img)
    assert not torch.equal(on[1]["logits"], base[1]["logits"])
    sp = toggled.image_extractor.extractor
    sp.train()
    assert sp.conv_mode == "fp32"  # not in eval mode: the fp32 forward
    bf = sp(_t(img.copy()))
    assert torch.equal(bf["logits"], base[1]["logits"])
    sp.eval()
    for ext in (toggled.event_extractor.extractor, toggled.image_extractor.extractor):
        ext.half_precision = False
        assert ext.conv_mode == "fp32"
    for model in (off, toggled):
        got = _forward(model, ev, mask, img)
        for side in (0, 1):
            assert set(got[side]) == set(base[side])
            for k in base[side]:
                assert _same(got[side][k], base[side][k]), (side, k)
        assert set(got[2]) == set(base[2]) and all(_same(got[2][k], base[2][k]) for k in base[2])
        assert got[3][0] == base[3][0] and ("conv_block_kernel" in got[3][0] or "conv16" in got[3][0])


def _network_io(ext, kind, ev, img):
    """the tensor the network reads (SuperPointv1 scales its image by 1/255 in fp32; 40x48 needs no padding)"""
    return torch.from_numpy(img.copy()) / 255.0 if kind == "image" else ev.cpu()


def test_on_follows_the_contract():
    """logits and raw_descriptors of both extractors against the float64 restatement of the layer rule, within 2 x the larger peer
    distance + 4 ulp of the value.  Measured on an MI355X (distance from the spec: kernel / peer A / peer B):
      event VGG     logits 7.0e-03 / 6.3e-03 / 9.1e-03, raw_descriptors 5.8e-03 / 7.4e-03 / 8.3e-03
      SuperPointv1  logits 1.0e-03 / 1.2e-03 / 1.1e-03, raw_descriptors 1.2e-03 / 1.2e-03 / 1.4e-03
    (not fp32-summation distances: an fp32 activation that differs from the float64 one in the last place and straddles a binary16
    tie moves the next layer's operand by a whole binary16 spacing, as in 8l.)  Keypoints are decisions: counted against the fp32
    run, not gated (all 64 per image coincide on both sides at this size)."""
    ev, mask, img = _inputs()
    model = _model()
    ef32, if32, _, _ = _forward(model, ev, mask, img)
    exts = {"event": model.event_extractor.extractor, "image": model.image_extractor.extractor}
    for ext in exts.values():
        ext.half_precision = True
        assert ext.conv_mode == "fp16"
    ef, imf, m, names = _forward(model, ev, mask, img)
    assert names[1].startswith("conv_f16_kernel<")
    ef2, imf2, m2, _ = _forward(model, ev, mask, img)
    for kind, got, again, f32 in (("event", ef, ef2, ef32), ("image", imf, imf2, if32)):
        ext = exts[kind]
        x = _network_io(ext, kind, ev, img)
        with torch.no_grad():
            spec = R.stack_forward(ext, x, R.spec)
            pa = R.stack_forward(ext, x, R.peer_a)
            pb = R.stack_forward(ext, x, lambda *a: R.peer_b(N, *a, dev=DEV))
        for idx, key in ((1, "logits"), (2, "raw_descriptors")):
            want = spec[idx]
            da, db = float((pa[idx].double() - want).abs().max()), float((pb[idx].double() - want).abs().max())
            g = got[key].cpu().double()
            dk = float((g - want).abs().max())
            print(f"conv_f16 {kind} {key}: distance from the spec: kernel {dk:.3e}, peer A {da:.3e}, peer B {db:.3e}")
            assert bool(((g - want).abs() <= 2 * max(da, db) + 4 * 2.0 ** -23 * want.abs()).all()), (kind, key, dk, da, db)
        # the decisions: inside their invariants, and the same twice
        cap = 64
        score = got["score"]
        same = 0
        for b in range(B_):
            pos, desc = got["sparse_positions"][b], got["sparse_descriptors"][b]
            assert pos.shape[0] <= cap and desc.shape[0] == pos.shape[0]
            yx = pos[:, :2].floor().long()  # pixel centres: index + 0.5
            assert bool(((yx >= 0) & (yx < torch.tensor([H_, W_], device=DEV))).all())
            assert torch.equal(score[b, 0, yx[:, 0], yx[:, 1]], pos[:, 2])
            assert bool(((desc.norm(dim=1) - 1).abs() < 1e-5).all())
            assert torch.equal(pos, again["sparse_positions"][b]) and torch.equal(desc, again["sparse_descriptors"][b])
            a = {tuple(r) for r in pos[:, :2].long().tolist()}
            same += len(a & {tuple(r) for r in f32["sparse_positions"][b][:, :2].long().tolist()}) / max(len(a), 1)
        assert torch.equal(got["logits"], again["logits"]) and torch.equal(got["raw_descriptors"], again["raw_descriptors"])
        print(f"conv_f16 {kind}: {100 * same / B_:.0f} % of the keypoints coincide with the fp32 run (recorded, not gated)")
    assert all(_same(m[k], m2[k]) for k in m)


def test_single_image_merged_head_equals_its_row_of_the_batch():
    """B == 1 runs the two heads' first layers as ONE merged layer (its own binary16 image, einx_extractor_set_conv_f16's last
    argument): every output is the same chunk-by-chunk, tap-by-tap sum as in the two launches of a batch, so the maps are bit-equal"""
    ev, mask, img = _inputs()
    model = _model()
    for ext in (model.event_extractor.extractor, model.image_extractor.extractor):
        ext.half_precision = True
    ef, imf, _, _ = _forward(model, ev, mask, img)
    ef1, imf1, _, names = _forward(model, ev[:1].contiguous(), mask[:1].contiguous(), img[:1])
    assert names[1].startswith("conv_f16_kernel<")
    for one, both in ((ef1, ef), (imf1, imf)):
        for k in ("backbone_feats", "logits", "raw_descriptors"):
            assert torch.equal(one[k][0], both[k][0]), k


def test_a_data_edit_reaches_the_fp16_image():
    ev, mask, img = _inputs()
    model = _model()
    sp = model.image_extractor.extractor
    sp.half_precision = True
    first = sp(_t(img.copy()))["logits"].clone()
    sp.conv3a.weight.data.mul_(0.5)  # through `.data`: only the content watch sees it
    second = sp(_t(img.copy()))["logits"].clone()
    assert not torch.equal(first, second)
    fresh = _model().image_extractor.extractor
    with torch.no_grad():
        fresh.conv3a.weight.mul_(0.5)
    fresh.half_precision = True
    assert torch.equal(second, fresh(_t(img.copy()))["logits"])


def test_forward_graph_replays_the_graph_of_the_mode():
    ev, mask, img = _inputs()
    model = _model()
    exts = (model.event_extractor.extractor, model.image_extractor.extractor)
    keys = ("logits", "raw_descriptors", "score")

    def snap(res):
        return [{k: res[s][k].clone() for k in keys} for s in (0, 1)]

    eager32 = snap(model(ev, _t(img.copy()), mask))
    for e in exts:
        e.half_precision = True
    eager16 = snap(model(ev, _t(img.copy()), mask))
    assert not torch.equal(eager16[1]["logits"], eager32[1]["logits"])
    seen = []
    for half, want in ((False, eager32), (True, eager16), (False, eager32), (True, eager16)):
        for e in exts:
            e.half_precision = half
        got = snap(model.forward_graph(ev, _t(img.copy()), mask))
        seen.append(len(model._graphs))
        assert all(torch.equal(got[s][k], want[s][k]) for s in (0, 1) for k in keys), half
    assert seen == [1, 2, 2, 2]  # one capture per mode, then replays


def test_evaluator_runs_with_the_mode_on():
    Hh, Wd, B, bins = 260, 346, 2, 5
    cfg, model, _ = _eim_model("SP_MNN", 23)
    evs = [synth_raw_events(dict(seed=840 + b, n=8000, H=Hh, W=Wd, bins=bins, frac=False, pneg=False)) for b in range(B)]
    img = synth.synth_image(98, B, Hh, Wd)
    ev32 = pkg.SameTimeEvaluator(model, bins=bins, resolution=(Wd, Hh))
    ev32.step(evs, _t(img.copy()))
    want = ev32.result()
    for e in (model.event_extractor.extractor, model.image_extractor.extractor):
        e.half_precision = True
    ev16 = pkg.SameTimeEvaluator(model, bins=bins, resolution=(Wd, Hh))
    ev16.step(evs, _t(img.copy()))
    assert N.lib().einx_conv_f16_last_kernel().decode().startswith("conv_f16_kernel<")
    got = ev16.result()
    assert list(got) == list(want)  # the result keys are unchanged

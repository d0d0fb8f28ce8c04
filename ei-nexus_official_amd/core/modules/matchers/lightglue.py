"""LightGlue matcher, native on MI355X (csrc/lightglue.hip).

Drop-in for LightGlue (reference core/modules/matchers/lightglue.py:421-716), inference path:
same `conf` handling (merged over `default_conf`), same parameter tree (`posenc.Wr`,
`transformers.{i}.self_attn|cross_attn.*`, `log_assignment.{i}.*`, `token_confidence.{i}.*`,
optional `input_proj`) and the same output dict.  `matcher_metrics` (:17-63) runs on the device
(csrc/gt_matches.hip).  `LightGlue.loss` in eval mode (:751-800 with one layer of
ref_descriptors: one assignment head, one NLL, row_norm, matcher_metrics) runs on the device without
a dense matrix (einx_lg_assign_nll); `NLLLoss` (:66-133) is the dense restatement in
torch operators.  Training mode (the layer loop, the token-confidence loss :190-203, autograd) is
out of scope.
Early stopping / point pruning are commented out in the reference (:606-652).  Early stopping (per-pair adaptive depth) is
available here as an opt-in, `LightGlue.early_stop`, and so is point pruning (per-pair, per-side adaptive width),
`LightGlue.point_pruning`.
"""
import ctypes

import numpy as np
import torch
from torch import nn

from ...._native import on_input_device
from .... import _lib
from .... import _native as N
from ._batched import from_feats, materialize_matches, stacked_outputs


@torch.no_grad()
def matcher_metrics(pred, data, prefix="", prefix_gt=None):
    """match_recall, match_precision, accuracy and average_precision of pred[f"{prefix}matches0"] (ranked by
    pred[f"{prefix}matching_scores0"]) against data[f"gt_{prefix_gt}matches0"], one value per pair: the reference's keys in and out
    (lightglue.py:17-63), computed by einx_match_pr.  average_precision is the closed form precision * (recall - r_first) of the
    reference's expression, the highest score's row taken at the lowest index on a tie."""
    from ...metrics._native_metrics import MATCH_PR_NAMES, match_pr
    if prefix_gt is None:
        prefix_gt = prefix
    rows = match_pr(pred[f"{prefix}matches0"], data[f"gt_{prefix_gt}matches0"], scores0=pred[f"{prefix}matching_scores0"]).float()
    return {f"{prefix}{name}": rows[:, i] for i, name in enumerate(MATCH_PR_NAMES)}


LOSS_KEYS = ("total", "last", "assignment_nll", "nll_pos", "nll_neg", "num_matchable", "num_unmatchable", "row_norm")


def nll_size_error(B, n, m):
    """What the reference's NLLLoss.nll_loss raises on stacked [B,n] / [B,m] labels with n != m: it writes the m column negatives
    into `weights[:, -1, :n]` (:132), a slice of min(n, m + 1) of the m + 1 columns.  None when that assignment goes through
    (n == m, or m == 1, which broadcasts)."""
    t = min(n, m + 1)
    if t == m or m == 1:
        return None
    return RuntimeError(f"The expanded size of the tensor ({t}) must match the existing size ({m}) at non-singleton dimension 1.  "
                        f"Target sizes: [{B}, {t}].  Tensor sizes: [{B}, {m}]")


def weight_loss(log_assignment, weights, gamma=0.0):
    """lightglue.py:66-85 on dense [B,n+1,m+1] tensors"""
    n, m = log_assignment.shape[1] - 1, log_assignment.shape[2] - 1
    loss_sc = log_assignment * weights
    num_neg0 = weights[:, :n, -1].sum(-1).clamp(min=1.0)
    num_neg1 = weights[:, -1, :m].sum(-1).clamp(min=1.0)
    num_pos = weights[:, :n, :m].sum((-1, -2)).clamp(min=1.0)
    nll_pos = -loss_sc[:, :n, :m].sum((-1, -2)) / num_pos
    nll_neg = (-loss_sc[:, :n, -1].sum(-1) - loss_sc[:, -1, :m].sum(-1)) / (num_neg0 + num_neg1)
    return nll_pos, nll_neg, num_pos, (num_neg0 + num_neg1) / 2.0


class NLLLoss(nn.Module):
    """The reference's NLLLoss (:88-133) on DENSE tensors with plain torch operators, on whatever device they live on: the
    restatement next to the device op, off the hot path like the dense `assignment` and `reward` of the ground-truth dict
    (LightGlue.loss does not go through it).  Forward values; pred["log_assignment"] [B,n+1,m+1]."""
    default_conf = {"nll_balancing": 0.5, "gamma_f": 0.0}

    def __init__(self, conf):
        super().__init__()
        self.conf = _merge(self.default_conf, conf if conf is not None else {})
        self.loss_fn = self.nll_loss

    def forward(self, pred, data, weights=None):
        log_assignment = pred["log_assignment"]
        if weights is None:
            weights = self.loss_fn(log_assignment, data)
        nll_pos, nll_neg, num_pos, num_neg = weight_loss(log_assignment, weights, gamma=self.conf.gamma_f)
        nll = self.conf.nll_balancing * nll_pos + (1 - self.conf.nll_balancing) * nll_neg
        return nll, weights, {"assignment_nll": nll, "nll_pos": nll_pos, "nll_neg": nll_neg, "num_matchable": num_pos,
                              "num_unmatchable": num_neg}

    def nll_loss(self, log_assignment, data):
        n, m = data["gt_matches0"].size(-1), data["gt_matches1"].size(-1)
        weights = torch.zeros_like(log_assignment)
        weights[:, :n, :m] = data["gt_assignment"].to(log_assignment.dtype)
        weights[:, :n, -1] = (data["gt_matches0"] == -1).to(log_assignment.dtype)
        weights[:, -1, :n] = (data["gt_matches1"] == -1).to(log_assignment.dtype)  # `:n` as the reference writes it (:132): n == m, or it raises
        return weights


class _Conf(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def _merge(base, over):
    out = _Conf(base)
    for k in (over.keys() if hasattr(over, "keys") else []):
        out[k] = over[k]
    return out


class LearnableFourierPositionalEncoding(nn.Module):
    def __init__(self, M, dim, F_dim=None, gamma=1.0):
        super().__init__()
        F_dim = F_dim if F_dim is not None else dim
        self.gamma = gamma
        self.Wr = nn.Linear(M, F_dim // 2, bias=False)
        nn.init.normal_(self.Wr.weight.data, mean=0, std=self.gamma ** -2)


def _ffn(d):
    return nn.Sequential(nn.Linear(2 * d, 2 * d), nn.LayerNorm(2 * d, elementwise_affine=True), nn.GELU(), nn.Linear(2 * d, d))


class SelfBlock(nn.Module):
    def __init__(self, embed_dim, num_heads, flash=False, bias=True):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.Wqkv = nn.Linear(embed_dim, 3 * embed_dim, bias=bias)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.ffn = _ffn(embed_dim)


class CrossBlock(nn.Module):
    def __init__(self, embed_dim, num_heads, flash=False, bias=True):
        super().__init__()
        self.heads = num_heads
        self.to_qk = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.to_v = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.to_out = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.ffn = _ffn(embed_dim)


class TransformerLayer(nn.Module):
    def __init__(self, *args, **kwargs):
        super().__init__()
        self.self_attn = SelfBlock(*args, **kwargs)
        self.cross_attn = CrossBlock(*args, **kwargs)


class MatchAssignment(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim
        self.matchability = nn.Linear(dim, 1, bias=True)
        self.final_proj = nn.Linear(dim, dim, bias=True)


class TokenConfidence(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.token = nn.Sequential(nn.Linear(dim, 1), nn.Sigmoid())


class LightGlue(nn.Module):
    """Early stopping.  The reference accepts `depth_confidence` and carries the trained token_confidence / log_assignment heads
    of every layer, but its forward IGNORES the key: the branch is commented out (:606-636) and the list its helpers read,
    `confidence_thresholds`, is never created, so every pair runs every layer.  This class does the same by default.  Setting
    `early_stop = True` (with conf.depth_confidence > 0, in eval mode) runs the branch on the device, per pair
    (einx_lightglue_early_stop): results then DIFFER from the reference's for every pair that stops, which is
    why the switch is opt-in rather than driven by the config key alone.  Outputs gain "stop" (layers run per pair).

    Point pruning.  The same holds for `width_confidence`: the reference's branch is commented out (:608-617, 637-652, 658-670),
    `get_pruning_mask` / `pruning_min_kpts` are live, the dict they read, `pruning_keypoint_thresholds`, is never created.
    `point_pruning = True` (with conf.width_confidence > 0, in eval mode) runs the branch on the device, per pair and per side
    (einx_lightglue_adaptive): after every non-final layer a side with more than `pruning_min_kpts(device)` rows
    drops the rows its matchability head calls unmatchable.  matches / scores stay in original indexing, prune0/1 hold the real
    counts, outputs gain kept0/1 (the survivors' original indices), ref_descriptors hold the survivors' rows, and
    "log_assignment" is absent.  A side pruned to zero rows finishes its pair without matches (upstream raises there).

    Half-precision attention.  `flash: True` is honoured as the reference honours it on a GPU (:206-230, :293-314): q, k, v of every
    self and cross attention are rounded to binary16, the attention runs on the f16 matrix-core instruction with fp32 accumulation
    and its context is rounded to binary16 again; everything else stays fp32 (einx_lightglue_flash).
    `attention_mode` reads "fp16" then; the default `flash: False` runs the fp32 kernels, unchanged.

    Half-precision linears.  The reference declares `mp` (:430) and its forward never reads it: upstream's
    torch.autocast(enabled=conf.mp) is gone, only `if torch.is_autocast_enabled(): desc0 = desc0.half()` is left (:568-570).  This
    class does the same by default.  `mixed_precision = True` (with conf.mp true, in eval mode, on a GPU) runs the nine nn.Linear of
    every transformer layer on the f16 matrix-core instruction (einx_lightglue_mp): inputs and weights rounded to
    binary16, products accumulated in fp32, fp32 bias, fp32 result.  Unlike autocast no output is rounded and the residual stream
    stays fp32; input_proj, rotary, LayerNorm, GELU, the heads, every decision and (unless `flash`) the attention stay fp32.  The
    weights are then packed without the out_proj / to_out fold, whatever `fold_message_projection` says, so that each weight is
    rounded as written.  `linear_mode` reads "fp16" then.  Independent of `flash`, early stopping and point pruning."""
    default_conf = {
        "name": "lightglue", "input_dim": 256, "add_scale_ori": False, "descriptor_dim": 256, "n_layers": 9, "num_heads": 4,
        "flash": False, "mp": False, "depth_confidence": -1, "width_confidence": -1, "filter_threshold": 0.0,
        "checkpointed": False, "weights": "superpoint", "weights_from_version": "v0.1_arxiv",
        "loss": {"gamma": 1.0, "fn": "nll", "nll_balancing": 0.5},
    }

    def __init__(self, conf):
        super().__init__()
        self.conf = conf = _merge(self.default_conf, conf)
        conf["loss"] = _merge(self.default_conf["loss"], conf["loss"])
        self.loss_fn = NLLLoss(conf.loss)
        # widths as the reference derives them (lightglue.py:246-248, 456-461): any num_heads dividing descriptor_dim.  The
        # attention kernel is instantiated for 32-, 64- and 128-wide heads (256 = 4 x 64, every EI-Nexus YAML, runs its own
        # instantiation); other widths run the next larger one on zero-padded heads.  What is left out: head widths that are
        # not a multiple of 4 (a head's rows are read 16 bytes at a time) or wider than 256.
        assert conf.descriptor_dim % conf.num_heads == 0
        hd = conf.descriptor_dim // conf.num_heads
        if hd % 4 or hd > 256:
            raise NotImplementedError("einx LightGlue: descriptor_dim // num_heads must be a multiple of 4, at most 256 "
                                      f"(got {conf.descriptor_dim} // {conf.num_heads})")
        if conf.input_dim != conf.descriptor_dim:
            self.input_proj = nn.Linear(conf.input_dim, conf.descriptor_dim, bias=True)
        else:
            self.input_proj = nn.Identity()
        head_dim = conf.descriptor_dim // conf.num_heads
        # add_scale_ori: the reference builds a 4-input encoding (:457-459) but its forward never appends scales / orientations
        # (:540-560 are commented out), so every forward fails in posenc.Wr on the 2-column keypoints; mirrored in forward()
        self.posenc = LearnableFourierPositionalEncoding(2 + 2 * bool(conf.add_scale_ori), head_dim, head_dim)
        h, n, d = conf.num_heads, conf.n_layers, conf.descriptor_dim
        self.transformers = nn.ModuleList([TransformerLayer(d, h, conf.flash) for _ in range(n)])
        self.log_assignment = nn.ModuleList([MatchAssignment(d) for _ in range(n)])
        self.token_confidence = nn.ModuleList([TokenConfidence(d) for _ in range(n - 1)])
        self.want_log_assignment = True
        self.fold_message_projection = True  # inference-time weight folding (see _pack); False = layer by layer as written
        self.merge_qk_v = True  # CrossBlock.to_qk and to_v as one launch over a merged weight image (same results); False = two launches
        # what the reference's confidence_threshold reads and never creates (:718-722, 468-470 commented out)
        self.confidence_thresholds = [self.confidence_threshold(i) for i in range(conf.n_layers)]
        self.early_stop = False  # opt-in: the reference ignores depth_confidence (see the class docstring)
        self.point_pruning = False  # opt-in: the reference ignores width_confidence (see the class docstring)
        self.mixed_precision = False  # opt-in: the reference ignores mp (see the class docstring)
        # what the reference's pruning_min_kpts reads and never creates (:745-749): upstream LightGlue's published values, quoted
        # (upstream is not at hand to check them against).  A side is pruned only while it has MORE rows than this.
        self.pruning_keypoint_thresholds = {"cpu": -1, "mps": -1, "cuda": 1024, "flash": 1536}
        self._packed = self._packed_mp = self._watch = None
        self._sig = None
        self._sig_tensors = None
        # also reached when a parent module's load_state_dict recurses into this one
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.refresh())

    def _apply(self, fn, *a, **k):
        self._packed = self._packed_mp = self._watch = self._sig_tensors = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._packed = self._packed_mp = self._watch = self._sig_tensors = None
        return super().load_state_dict(*a, **k)

    def confidence_threshold(self, layer_index):
        """scaled confidence threshold of a layer (lightglue.py:718-722)"""
        threshold = 0.8 + 0.1 * np.exp(-4.0 * layer_index / self.conf.n_layers)
        return float(np.clip(threshold, 0, 1))

    def early_stop_active(self):
        """whether the next eval-mode forward stops pairs early; depth_confidence is read at every call, like filter_threshold"""
        if not self.early_stop:
            return False
        if float(self.conf.width_confidence) > 0 and not self.point_pruning:
            raise NotImplementedError("einx LightGlue: early_stop with width_confidence > 0 asks for point pruning, which is not "
                                      "implemented (DESIGN.md 8h); set point_pruning = True to run it (DESIGN.md 8j)")
        return not self.training and float(self.conf.depth_confidence) > 0

    def point_pruning_active(self):
        """whether the next eval-mode forward prunes points; width_confidence is read at every call, like depth_confidence"""
        return bool(self.point_pruning) and not self.training and float(self.conf.width_confidence) > 0

    def pruning_min_kpts(self, device):
        """the gate (lightglue.py:745-749): a side is pruned only while it has more rows than this; with conf.flash on a GPU the
        "flash" entry, as the reference chooses"""
        kind = torch.device(device).type
        if self.conf.flash and kind == "cuda":
            return self.pruning_keypoint_thresholds["flash"]
        return self.pruning_keypoint_thresholds[kind]

    @property
    def attention_mode(self):
        """ "fp16": conf.flash is set and every attention of a device forward rounds q, k, v and its context to binary16 and runs
        on the f16 matrix-core instruction (einx_lightglue_flash); "fp32" (the default): the fp32 kernels"""
        return "fp16" if self.conf.flash else "fp32"

    def mixed_precision_active(self):
        """whether the next forward runs the layers' linears in fp16: the attribute, conf.mp (read at every call, like
        depth_confidence), eval mode, and the parameters on a GPU (the kernels take inputs and parameters on one HIP device, so
        that is where the inputs are); a model on the CPU reports "fp32"."""
        if not (bool(self.mixed_precision) and not self.training and bool(self.conf.mp)):
            return False
        return self.posenc.Wr.weight.device.type == "cuda"

    @property
    def linear_mode(self):
        """ "fp16": `mixed_precision` and conf.mp are set and the nine linears of every layer of an eval-mode device forward round
        their inputs and weights to binary16 and run on the f16 matrix-core instruction with fp32 accumulation (einx_lightglue_mp,
        DESIGN.md 8l); "fp32" (the default): the fp32 kernels"""
        return "fp16" if self.mixed_precision_active() else "fp32"

    def get_pruning_mask(self, confidences, scores, layer_index):
        """which points stay (lightglue.py:723-730), in the float32 arithmetic of DESIGN.md 8j: the restatement of what the
        device decides, on tensors of sigmoid outputs"""
        keep = scores > float(np.float32(1.0 - float(self.conf.width_confidence)))
        if confidences is not None:  # low-confidence points are never pruned
            keep = keep | (confidences <= float(np.float32(self.confidence_thresholds[layer_index])))
        return keep

    def refresh(self):
        """Drop the packed / folded weight images.  REQUIRED after edits through `p.data` (an alias with its own version
        counter: `p._version`, which `_pack` keys on, does not move) or after replacing Parameter objects."""
        self._packed = self._packed_mp = self._watch = self._sig_tensors = None

    def _pack(self, mp=False):
        """ctypes image of the parameter pointers (weights stay in their nn.Parameter storage).  mp: the image einx_lightglue_mp
        reads under EINX_LG_LIN_F16 -- no out_proj / to_out fold, and the binary16 image `w.half()` of each layer's nine weights
        (DESIGN.md 8l); kept beside the fp32 image and dropped with it."""
        if self._sig_tensors is None:
            self._sig_tensors = list(self.parameters())
        sig = tuple((t.data_ptr(), t._version) for t in self._sig_tensors)
        if sig != self._sig:  # in-place parameter edits and moves drop the folded weight images too
            self._packed, self._packed_mp, self._watch, self._sig = None, None, None, sig
        cached = self._packed_mp if mp else self._packed
        if cached is not None:
            return cached
        c = self.conf
        keep = []

        def p(t):
            t = t.detach()
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device.type != "cuda":
                raise RuntimeError("einx LightGlue: parameters must be contiguous fp32 tensors on a HIP device")
            keep.append(t)
            return t.data_ptr()

        def half(t):
            """the contract's rounding of a weight: IEEE binary16, round to nearest even (made once, on the device)"""
            t = t.detach().half().contiguous()
            keep.append(t)
            return t.data_ptr()

        d = c.descriptor_dim

        def fold(ffn0, proj):
            """ffn0(cat[x, proj(ctx)]) == cat[x, ctx] @ [W0a | W0b Wp]^T + (b0 + W0b bp): fold the message
            projection into the FFN's first Linear once, at load time (saves one GEMM per block)."""
            W0, b0 = ffn0.weight.detach(), ffn0.bias.detach()
            W0b = W0[:, d:].contiguous()
            Wf = W0.clone()
            zero = torch.zeros(d, dtype=torch.float32, device=W0.device)
            Wf[:, d:] = N.linear(W0b, proj.weight.detach().t().contiguous(), zero)  # W0b @ Wp
            bf = b0.clone().reshape(-1, 1).contiguous()
            N.linear(W0b, proj.bias.detach().reshape(1, -1).contiguous(), zero[:1], out=bf, accumulate=True)  # b0 + W0b @ bp
            return Wf.contiguous(), bf.reshape(-1).contiguous()

        layers = (_lib.LgLayer * c.n_layers)()
        for i, tl in enumerate(self.transformers):
            s, x, L = tl.self_attn, tl.cross_attn, layers[i]
            L.Wqkv, L.bqkv = p(s.Wqkv.weight), p(s.Wqkv.bias)
            L.Wqk, L.bqk, L.Wv, L.bv = p(x.to_qk.weight), p(x.to_qk.bias), p(x.to_v.weight), p(x.to_v.bias)
            if self.merge_qk_v and c.descriptor_dim == 256 and c.num_heads == 4:  # one launch for to_qk | to_v (copies, like the folds)
                L.Wqk_v = p(torch.cat([x.to_qk.weight.detach(), x.to_v.weight.detach()], 0).contiguous())
                L.bqk_v = p(torch.cat([x.to_qk.bias.detach(), x.to_v.bias.detach()], 0).contiguous())
            else:
                L.Wqk_v, L.bqk_v = None, None
            if mp:
                L.Wqkv_h, L.Wo_h, L.sf0_h, L.sf3_h = half(s.Wqkv.weight), half(s.out_proj.weight), half(s.ffn[0].weight), half(s.ffn[3].weight)
                L.Wqk_h, L.Wv_h, L.Wco_h = half(x.to_qk.weight), half(x.to_v.weight), half(x.to_out.weight)
                L.cf0_h, L.cf3_h = half(x.ffn[0].weight), half(x.ffn[3].weight)
                L.Wqk_v_h = half(torch.cat([x.to_qk.weight.detach(), x.to_v.weight.detach()], 0)) if L.Wqk_v else None
            if self.fold_message_projection and not mp:
                sw, sb = fold(s.ffn[0], s.out_proj)
                xw, xb = fold(x.ffn[0], x.to_out)
                L.Wo, L.bo, L.Wco, L.bco = None, None, None, None
                L.sf0_w, L.sf0_b, L.cf0_w, L.cf0_b = p(sw), p(sb), p(xw), p(xb)
            else:
                L.Wo, L.bo, L.Wco, L.bco = p(s.out_proj.weight), p(s.out_proj.bias), p(x.to_out.weight), p(x.to_out.bias)
                L.sf0_w, L.sf0_b, L.cf0_w, L.cf0_b = p(s.ffn[0].weight), p(s.ffn[0].bias), p(x.ffn[0].weight), p(x.ffn[0].bias)
            L.sln_g, L.sln_b = p(s.ffn[1].weight), p(s.ffn[1].bias)
            L.sf3_w, L.sf3_b = p(s.ffn[3].weight), p(s.ffn[3].bias)
            L.cln_g, L.cln_b = p(x.ffn[1].weight), p(x.ffn[1].bias)
            L.cf3_w, L.cf3_b = p(x.ffn[3].weight), p(x.ffn[3].bias)
        w = _lib.LgWeights()
        w.struct_size, w.layer_size = ctypes.sizeof(_lib.LgWeights), ctypes.sizeof(_lib.LgLayer)
        if isinstance(self.input_proj, nn.Linear):
            w.in_w, w.in_b = p(self.input_proj.weight), p(self.input_proj.bias)
        else:
            w.in_w, w.in_b = None, None
        la = self.log_assignment[c.n_layers - 1]
        w.Wr = p(self.posenc.Wr.weight)
        w.proj_w, w.proj_b = p(la.final_proj.weight), p(la.final_proj.bias)
        w.match_w, w.match_b = p(la.matchability.weight), p(la.matchability.bias)
        w.n_layers, w.heads, w.d, w.input_dim = c.n_layers, c.num_heads, c.descriptor_dim, c.input_dim
        w.filter_threshold = float(c.filter_threshold)
        w.layers = ctypes.cast(layers, ctypes.POINTER(_lib.LgLayer))
        heads = (_lib.LgHead * c.n_layers)()  # every layer's heads, for early stopping (the same storage, the same watch)
        for i, (hd, a) in enumerate(zip(heads, self.log_assignment)):
            hd.proj_w, hd.proj_b = p(a.final_proj.weight), p(a.final_proj.bias)
            hd.match_w, hd.match_b = p(a.matchability.weight), p(a.matchability.bias)
            if i < c.n_layers - 1:
                tok = self.token_confidence[i].token[0]
                hd.token_w, hd.token_b = p(tok.weight), p(tok.bias)
            else:
                hd.token_w, hd.token_b = None, None
        # `.data` edits are seen by content at the next forward (round 4).  ONE watch per set of images: it is built with the first
        # image after a drop and takes its reference then; the other mode's image, packed later, is judged against that same
        # reference, so an edit made between the two packs raises the flag and drops both.  It also keeps the
        # buffers a captured graph of the first mode reads alive while the second mode packs.
        if self._watch is None:
            self._watch = N.ParamWatch(self._sig_tensors)
        packed = (w, layers, keep, heads)
        if mp:
            self._packed_mp = packed
        else:
            self._packed = packed
        return packed

    def _add_scale_ori_error(self, feats0):
        """What the reference's forward raises with add_scale_ori=True (recorded from the reference, tests/golden/lgcfg.json): the
        descriptor-width assert comes first (:562-563), then posenc.Wr -- Linear(4, head_dim/2) -- meets [b, n, 2] keypoints (:565)."""
        pos, desc = feats0["sparse_positions"], feats0["sparse_descriptors"]
        pos = pos if torch.is_tensor(pos) else pos[0][None]
        desc = desc if torch.is_tensor(desc) else desc[0][None]
        if desc.shape[-1] != self.conf.input_dim:
            raise AssertionError("descriptor dimension does not match conf.input_dim")
        rows = pos.shape[0] * pos.shape[1] if pos.dim() == 3 else pos.shape[0]
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({rows}x2 and 4x{self.posenc.Wr.weight.shape[0]})")

    @on_input_device
    def match_batched(self, pb0, pb1, all_layers=False):
        if self.conf.add_scale_ori:
            raise RuntimeError("einx LightGlue: add_scale_ori=True has no working forward in the reference (lightglue.py:540-565)")
        if pb0.desc.shape[-1] != self.conf.input_dim or pb1.desc.shape[-1] != self.conf.input_dim:
            raise AssertionError("descriptor dimension does not match conf.input_dim")
        mp = self.mixed_precision_active()  # read at every call
        w, _, _, heads = self._pack(mp)
        w.filter_threshold = float(self.conf.filter_threshold)  # read at every call like the reference's filter_matches call (lightglue.py:656)
        stale = self._watch.check()
        es = (heads, float(self.conf.depth_confidence)) if self.early_stop_active() else None
        pr = None
        if self.point_pruning_active():
            pr = (heads, float(self.conf.width_confidence), int(self.pruning_min_kpts(pb0.desc.device)))
        r = N.lightglue(w, pb0, pb1, want_la=self.want_log_assignment, want_ref=True, all_layers=all_layers, early_stop=es, pruning=pr,
                        flash=bool(self.conf.flash), mp=mp)
        r.stale = stale
        return N.gather_matches(r, pb0.kpts, pb1.kpts, pb0.counts, 2)

    @torch.no_grad()
    @on_input_device
    def forward(self, feats0, feats1):
        """B == 1: the per-pair dict (matched keypoints in pixel coordinates, lightglue.py:689-698).
        B > 1 (stacked [B,n,*] inputs): whole-batch tensors and per-pair matched keypoints in
        *normalised* coordinates, as lightglue.py:675-687 returns them.  In training mode
        (`self.training`) ref_descriptors hold every layer's output [B,L,n,d] (:626-629,709-710);
        forward values only -- autograd / the loss are outside this build."""
        pos0, pos1 = feats0["sparse_positions"], feats1["sparse_positions"]
        if self.conf.add_scale_ori:
            self._add_scale_ori_error(feats0)
        stacked = torch.is_tensor(pos0) and pos0.dim() == 3 and torch.is_tensor(pos1) and pos1.dim() == 3
        if stacked:
            if feats0["sparse_descriptors"].shape[-1] != self.conf.input_dim or feats1["sparse_descriptors"].shape[-1] != self.conf.input_dim:
                raise AssertionError("descriptor dimension does not match conf.input_dim")
            if pos0.shape[0] > 1 and (pos0.numel() == 0 or pos1.numel() == 0):
                f = feats0["sparse_descriptors"]
                B, n, m = pos0.shape[0], pos0.shape[1], pos1.shape[1]
                print("No keypoints found in either image")
                return {"matches0": f.new_full((B, n), -1), "matches1": f.new_full((B, m), -1), "matching_scores0": f.new_zeros((B, n)),
                        "matching_scores1": f.new_zeros((B, m)), "matched_kpts0": [f.new_zeros((n, 3))] * B,
                        "matched_kpts1": [f.new_zeros((m, 3))] * B, "similarity": f.new_zeros((B, n, m)),
                        "log_assignment": f.new_zeros((B, n + 1, m + 1))}
        pb0, pb1 = from_feats(feats0), from_feats(feats1)
        all_layers = bool(self.training)
        r = self.match_batched(pb0, pb1, all_layers=all_layers)
        # match counts + the weight watch in one read-back
        nm_all = torch.cat([r.nmatch, r.stale]).cpu().tolist() if r.stale is not None else r.nmatch.cpu().tolist() + [0]
        if nm_all[-1]:  # a weight was edited through `.data`: rebuild the images, match again
            self.refresh()
            r = self.match_batched(pb0, pb1, all_layers=all_layers)
            nm_all = r.nmatch.cpu().tolist() + [0]
        pruned = r.live is not None  # point pruning ran: real prune counts, kept0/1, no log_assignment
        n = pb0.counts_host or pb0.counts.cpu().tolist()
        m = pb1.counts_host or pb1.counts.cpu().tolist()
        L = self.conf.n_layers
        if pb0.B == 1:
            nm = nm_all[:-1]
            out = {k: v[0] for k, v in materialize_matches(r, n, m, nm, 2).items()}
            if n[0] and m[0]:
                ref0 = r.ref0 if all_layers else r.ref0[:, None]
                ref1 = r.ref1 if all_layers else r.ref1[:, None]
                out["ref_descriptors0"] = ref0[:, :, :n[0]]
                out["ref_descriptors1"] = ref1[:, :, :m[0]]
                out["prune0"] = r.prune0[:, :n[0]] if pruned else torch.ones_like(out["matching_scores0"]) * L
                out["prune1"] = r.prune1[:, :m[0]] if pruned else torch.ones_like(out["matching_scores1"]) * L
            if pruned:
                live = r.live.cpu().tolist()
                out["kept0"], out["kept1"] = r.kept0[:, :live[0]], r.kept1[:, :live[1]]
                out.pop("log_assignment", None)
            if r.stop is not None:
                out["stop"] = r.stop
            return out
        if not (stacked and len(set(n)) == 1 and len(set(m)) == 1):
            raise NotImplementedError("einx LightGlue.forward with B > 1 takes stacked [B,n,*] tensors (as the reference does); "
                                      "use Matcher for ragged batches")
        # b > 1: matched keypoints are gathered from the normalised coordinates (reference behaviour)
        k0 = N.normalize_keypoints(pb0.kpts, pb0.image_size, out_cols=3)
        k1 = N.normalize_keypoints(pb1.kpts, pb1.image_size, out_cols=3)
        N.gather_matches(r, k0, k1, pb0.counts, 2)
        out = stacked_outputs(r, r.nmatch.cpu().tolist(), 2)
        out["ref_descriptors0"] = r.ref0 if all_layers else r.ref0[:, None]
        out["ref_descriptors1"] = r.ref1 if all_layers else r.ref1[:, None]
        out["prune0"] = r.prune0 if pruned else torch.ones_like(r.scores0) * L
        out["prune1"] = r.prune1 if pruned else torch.ones_like(r.scores1) * L
        if pruned:
            out["kept0"], out["kept1"] = r.kept0, r.kept1
            out.pop("log_assignment", None)
        if r.stop is not None:
            out["stop"] = r.stop
        return out

    @torch.no_grad()
    @on_input_device
    def loss(self, pred, data):
        """The reference's `loss` (:751-800) as its validation loop calls it, after model.eval(): `pred` holds the
        forward's ref_descriptors0/1 [B,1,n,d] (and matches0 / matching_scores0 for the metrics), `data` gt_matches0 [B,n],
        gt_matches1 [B,m] and gt_assignment [B,n,m].  Returns (losses, metrics): losses = LOSS_KEYS, each float32 [B] on the
        device; metrics = matcher_metrics(pred, data).  Everything is enqueued; nothing is read back.  The NLL and row_norm come
        from einx_lg_assign_nll on the last head's weights: no log_assignment is recomputed and pred["log_assignment"] is not read.
        A gt_assignment that is still a lazy entry of gt_generation's dict is handed over as pos0 and stays lazy; a tensor is
        read as the dense 0/1 matrix it is.  The reference's failures are mirrored: stacked labels with n != m raise its
        RuntimeError, more than one layer of ref_descriptors raises KeyError('confidence'); m == 1 < n (a silent broadcast there)
        and training mode raise NotImplementedError.  A `pred` that carries "stop" (early stopping was on) or "kept0" (point pruning
        was on: its ref_descriptors are a subset of the rows) raises ValueError."""
        from ....core.geometry.gt_generation import lazy_pos0
        if self.training:
            raise NotImplementedError("einx LightGlue.loss: training mode (layerwise totals, the token-confidence loss and a backward "
                                      "pass) is out of scope, see DESIGN.md 8; call it after model.eval()")
        if "stop" in pred:
            raise ValueError("einx LightGlue.loss: `pred` comes from a forward with early stopping on (it carries \"stop\"): its "
                             "ref_descriptors are those of each pair's stopping layer, and the loss applies the LAST head (DESIGN.md 8h)")
        if "kept0" in pred:
            raise ValueError("einx LightGlue.loss: `pred` comes from a forward with point pruning on (it carries \"kept0\"): its "
                             "ref_descriptors hold only the surviving rows, and the labels are those of every keypoint (DESIGN.md 8j)")
        ref0, ref1 = pred["ref_descriptors0"], pred["ref_descriptors1"]
        if ref0.shape[1] > 1:
            raise KeyError("confidence")  # the reference's layer loop adds to a key that only training mode creates (:781)
        gt0, gt1 = data["gt_matches0"], data["gt_matches1"]
        B, n, m = ref0.shape[0], gt0.size(-1), gt1.size(-1)
        err = nll_size_error(B, n, m)
        if err is not None:
            raise err
        if m == 1 and n > 1:
            raise NotImplementedError("einx LightGlue.loss: with m == 1 < n the reference broadcasts the one column label over its "
                                      "dustbin row (lightglue.py:132) instead of failing; that value is not reproduced")
        if ref0.shape[2] != n or ref1.shape[2] != m:
            raise ValueError("einx LightGlue.loss: ref_descriptors and gt_matches differ in their keypoint counts")
        pos0 = lazy_pos0(data, "gt_assignment")
        assignment = None if pos0 is not None else data["gt_assignment"]
        w = self._pack()[0]
        rows = N.lg_assign_nll(w, ref0[:, -1].float().contiguous(), ref1[:, -1].float().contiguous(), gt0, gt1, pos0=pos0, assignment=assignment)
        vals, row_norm = N.lg_nll_values(rows, float(self.conf.loss.nll_balancing))
        vals, row_norm = vals.float(), row_norm.float()
        nll = vals[:, 0]
        losses = {"total": nll, "last": nll.clone(), "assignment_nll": nll, "nll_pos": vals[:, 1], "nll_neg": vals[:, 2],
                  "num_matchable": vals[:, 3], "num_unmatchable": vals[:, 4], "row_norm": row_norm}
        return losses, matcher_metrics(pred, data)

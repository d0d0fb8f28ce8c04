// extract.hip -- handle-level entry points: ONE call enqueues a whole extractor (SURVEY 8b's coarse ABI).
//
// einx_extractor_create copies the layer descriptors of one network (weights stay in caller-owned device
// memory, already repacked by einx_conv_repack / folded by einx_bn_fold); einx_extract then enqueues, on the
// given stream and without any host synchronisation,
//   [input /= 255]  ->  backbone convs (replicate pad folded into layer 1)  ->  detector head  ->  descriptor head
//   ->  [coarse-descriptor normalisation + channels-last raw copy]  ->  score map (softmax / sigmoid, pixel
//   shuffle, mask dilation, border)  ->  NMS fix-point + top-k + positions  ->  sparse descriptor sampling,
// i.e. everything VGGExtractor / VGGExtractorNP / SuperPointv1 / SiLKModel .forward does up to the output dict
// (reference core/modules/event_extractors/EventExtractors.py:517-624,:331-434,
// image_extractors/superpoint_extractor.py:345-480, image_extractors/silk_extractor.py:177-257).
// Intermediate activations live in a caller-provided workspace (two ping-pong buffers + the detector's
// workspace); every tensor of the reference's output dict is written to caller-provided outputs.
// The op-level entry points (einx_conv_block, einx_score_map, ...) stay exported for the unit tests; this file
// only sequences them, so a handle-level forward is bit-identical to the op-by-op forward.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <new>
#include <vector>

#include "einx_common.h"

struct einx_extractor {
  einx_extractor_desc d;
  std::vector<einx_conv_desc> backbone, det, desc;
  bool has_merged = false;  // det[0] + desc[0] as one layer (see einx_extractor_desc::merged_head0)
  einx_conv_desc merged;
  // opt-in binary16 images (einx_extractor_set_conv_f16), parallel to the lists above: w_f16 == nullptr leaves the layer on fp32
  std::vector<einx_conv_desc_f16> backbone16, det16, desc16;
  einx_conv_desc_f16 merged16 = {};
};

namespace {

struct Plan {
  int Hp, Wp, h0, w0;       // padded size, top/left pad
  int hc, wc;               // head resolution
  size_t buf_elems[2];      // ping-pong activation buffers (floats per image)
  size_t head_elems;        // scratch for the 3x3 head layers' outputs (floats per image)
};

// Small batches (the reference's own call pattern is one pair per forward): every launch after the backbone leaves most of
// the 256 CUs idle and the call is a chain of ~25 dependent kernels.  The descriptor branch (head convs, coarse
// normalisation) does not depend on the detector branch (head convs, score map, NMS passes, selection) until the sparse
// sampling, so it is enqueued on a second, library-owned stream between a fork and a join event: at B=1 ~90 us of ~540 per
// network leave the critical path.  The rule depends only on the arguments that size the workspace (a second head scratch).
// Round 5: the networks with 1/8-resolution heads fork at EVERY batch size -- at B = 32 the detector branch's latency-bound tail
// (score map, eight NMS passes, selection) then runs beside the descriptor head's convolutions of the same network as well as
// beside the other extractor: SP+MNN 8.52-8.60 -> 8.43-8.47 ms per step, SP+LightGlue B = 64 62.2 -> 61.6 (A/B on one box,
// alternating libraries).  The full-resolution networks (SiLK family) measured the same either way at B = 32 and keep the limit.
constexpr long kForkMaxCells = 8192;  // B x head pixels up to which the two head branches of a full-resolution network run concurrently
bool fork_heads(const einx_extractor* e, const Plan& pl, int B) { return e->d.cell == 8 || (long)B * pl.hc * pl.wc <= kForkMaxCells; }

// Padder.__init__ arithmetic (core/modules/utils/util.py:6-15)
void padder(int h, int w, int p, int* w0, int* w1, int* h0, int* h1) {
  const int hp = (((h / p) + 1) * p - h) % p;
  const int wp = (((w / p) + 1) * p - w) % p;
  *w0 = wp / 2;
  *w1 = wp - wp / 2;
  *h0 = hp / 2;
  *h1 = hp - hp / 2;
}

bool make_plan(const einx_extractor* e, int H, int W, Plan* pl) {
  int w0, w1, h0, h1;
  padder(H, W, e->d.cell, &w0, &w1, &h0, &h1);
  pl->Hp = H + h0 + h1;
  pl->Wp = W + w0 + w1;
  pl->h0 = h0;
  pl->w0 = w0;
  int h = pl->Hp, w = pl->Wp;
  pl->buf_elems[0] = pl->buf_elems[1] = 0;
  const int nb = (int)e->backbone.size();
  for (int i = 0; i < nb; ++i) {
    const einx_conv_desc& c = e->backbone[i];
    if (c.pool) {
      if ((h & 1) || (w & 1)) return false;
      h /= 2;
      w /= 2;
    }
    if (i + 1 < nb) {  // the last backbone layer writes the `backbone_feats` output, not a scratch buffer
      const size_t n = (size_t)c.cout * h * w;
      if (n > pl->buf_elems[i & 1]) pl->buf_elems[i & 1] = n;
    }
  }
  pl->hc = h;
  pl->wc = w;
  size_t he = 0;
  for (size_t i = 0; i + 1 < e->det.size(); ++i) he = std::max(he, (size_t)e->det[i].cout * h * w);
  for (size_t i = 0; i + 1 < e->desc.size(); ++i) he = std::max(he, (size_t)e->desc[i].cout * h * w);
  if (e->has_merged) he = std::max(he, (size_t)e->merged.cout * h * w);
  pl->head_elems = he;
  return h * e->d.cell == pl->Hp && w * e->d.cell == pl->Wp;
}

int topk_cap(int N, int top_k, float det_thr) {
  // rows a batch image can produce: N-1-lo for the quantile threshold of detection_top_k (see einx_detect), else N
  if (top_k <= 0 || top_k >= N || det_thr < 1.0f) return N;
  const float q = (float)(N - top_k) / (float)N;
  const float rank = q * (float)(N - 1);
  const int lo = (int)floorf(rank);
  return N - 1 - lo;
}

void detect_params(const einx_extractor* e, const Plan& pl, int B, int H, int W, int cap, int nms_iters, einx_detect_params* p) {
  p->B = B;
  p->Hp = pl.Hp;
  p->Wp = pl.Wp;
  p->H = H;
  p->W = W;
  p->h0 = pl.h0;
  p->w0 = pl.w0;
  p->radius = e->d.nms_radius;
  p->top_k = e->d.top_k;
  p->det_thr = e->d.det_thr;
  p->ordering_xy = e->d.ordering_xy;
  p->cap = cap;
  p->nms_iters = nms_iters;
}

}  // namespace

EINX_EXPORT einx_extractor* einx_extractor_create(const einx_extractor_desc* d) {
  if (!d) {
    einx_set_error("einx_extractor_create: null descriptor");
    return nullptr;
  }
  if (d->struct_size != sizeof(einx_extractor_desc)) {
    einx_set_error("einx_extractor_create: einx_extractor_desc::struct_size is %zu, this library's is %zu (header / library ABI mismatch: EINX_ABI_VERSION %d)",
                   (size_t)d->struct_size, sizeof(einx_extractor_desc), EINX_ABI_VERSION);
    return nullptr;
  }
  if (!d || !d->backbone || !d->det_head || !d->desc_head || d->n_backbone <= 0 || d->n_det <= 0 || d->n_desc <= 0) {
    einx_set_error("einx_extractor_create: null / empty layer lists");
    return nullptr;
  }
  if (d->cell != 8 && d->cell != 1) {
    einx_set_error("einx_extractor_create: cell must be 8 (SuperPoint-shaped) or 1 (SiLK-shaped)");
    return nullptr;
  }
  einx_extractor* e = new (std::nothrow) einx_extractor();
  if (!e) return nullptr;
  e->d = *d;
  e->backbone.assign(d->backbone, d->backbone + d->n_backbone);
  e->det.assign(d->det_head, d->det_head + d->n_det);
  e->desc.assign(d->desc_head, d->desc_head + d->n_desc);
  e->d.backbone = e->backbone.data();
  e->d.det_head = e->det.data();
  e->d.desc_head = e->desc.data();
  e->d.merged_head0 = nullptr;
  if (d->merged_head0) {
    const einx_conv_desc& m = *d->merged_head0;
    const einx_conv_desc &a = e->det.front(), &b = e->desc.front();
    if (e->det.size() != 2 || e->desc.size() != 2 || m.cin != a.cin || m.cin != b.cin || m.cout != a.cout + b.cout || m.ks != a.ks || m.ks != b.ks ||
        m.relu != a.relu || m.relu != b.relu || m.pool || a.pool || b.pool || !m.w_native || (m.scale == nullptr) != (a.scale == nullptr) ||
        (m.scale == nullptr) != (b.scale == nullptr) || a.cout % 64 != 0) {
      einx_set_error("einx_extractor_create: merged_head0 (cin %d cout %d ks %d relu %d pool %d bn %d) does not describe det_head[0] (%d layers; cin %d cout %d ks %d relu %d bn %d) + "
                     "desc_head[0] (%d layers; cin %d cout %d ks %d relu %d bn %d): two-layer heads of one structure, det_head[0].cout a multiple of 64",
                     m.cin, m.cout, m.ks, m.relu, m.pool, m.scale != nullptr, (int)e->det.size(), a.cin, a.cout, a.ks, a.relu, a.scale != nullptr,
                     (int)e->desc.size(), b.cin, b.cout, b.ks, b.relu, b.scale != nullptr);
      delete e;
      return nullptr;
    }
    e->merged = m;
    e->has_merged = true;
  }
  const int want = d->cell == 8 ? 65 : 1;
  if (e->det.back().cout != want || e->backbone.back().cout != e->det.front().cin || e->backbone.back().cout != e->desc.front().cin) {
    einx_set_error("einx_extractor_create: head shapes do not fit (detector head must end in %d channels)", want);
    delete e;
    return nullptr;
  }
  return e;
}

EINX_EXPORT void einx_extractor_destroy(einx_extractor* e) { delete e; }

EINX_EXPORT int einx_extractor_set_conv_f16(einx_extractor* e, const einx_conv_desc_f16* const* backbone, const einx_conv_desc_f16* const* det_head,
                                            const einx_conv_desc_f16* const* desc_head, const einx_conv_desc_f16* merged_head0) {
  EINX_CHECK_ARG(e, "null pointer");
  // checked whole before anything is stored: a refused call leaves the handle as it was
  auto fits = [](const einx_conv_desc_f16* h, const einx_conv_desc& c) {
    return h->struct_size == sizeof(einx_conv_desc_f16) && h->w_f16 && h->cin == c.cin && h->cout == c.cout && h->ks == c.ks && h->relu == c.relu &&
           h->pool == c.pool && h->cin % 8 == 0 && (h->scale == nullptr) == (c.scale == nullptr) && (h->scale == nullptr) == (h->shift == nullptr);
  };
  auto list_fits = [&](const einx_conv_desc_f16* const* src, const std::vector<einx_conv_desc>& L) {
    for (size_t i = 0; src && i < L.size(); ++i)
      if (src[i] && !fits(src[i], L[i])) return false;
    return true;
  };
  EINX_CHECK_ARG(list_fits(backbone, e->backbone) && list_fits(det_head, e->det) && list_fits(desc_head, e->desc) &&
                     (!merged_head0 || (e->has_merged && fits(merged_head0, e->merged))),
                 "a binary16 descriptor does not describe its layer (struct_size, image, cin % 8 == 0, cin / cout / ks / relu / pool / BN as created)");
  auto store = [](const einx_conv_desc_f16* const* src, size_t n, std::vector<einx_conv_desc_f16>& dst) {
    dst.assign(n, einx_conv_desc_f16{});
    for (size_t i = 0; src && i < n; ++i)
      if (src[i]) dst[i] = *src[i];
  };
  store(backbone, e->backbone.size(), e->backbone16);
  store(det_head, e->det.size(), e->det16);
  store(desc_head, e->desc.size(), e->desc16);
  e->merged16 = merged_head0 ? *merged_head0 : einx_conv_desc_f16{};
  return EINX_OK;
}

EINX_EXPORT int einx_extract_shapes(const einx_extractor* e, int H, int W, einx_extract_shapes_t* s) {
  EINX_CHECK_ARG(e && s, "null pointer");
  Plan pl;
  EINX_CHECK_ARG(H > 0 && W > 0 && make_plan(e, H, W, &pl), "image size does not fit the network's pooling / cell size");
  s->Hp = pl.Hp;
  s->Wp = pl.Wp;
  s->h0 = pl.h0;
  s->w0 = pl.w0;
  s->hc = pl.hc;
  s->wc = pl.wc;
  s->feat_channels = e->backbone.back().cout;
  s->det_channels = e->det.back().cout;
  s->desc_dim = e->desc.back().cout;
  s->cap = topk_cap(pl.Hp * pl.Wp, e->d.top_k, e->d.det_thr);
  return EINX_OK;
}

// nms_iters <= 0 means "the default pass budget" in BOTH the size query and the call (the detector's per-image flag array
// is B x nms_iters words of the workspace)
static inline int nms_budget(int nms_iters) { return nms_iters > 0 ? nms_iters : 8; }

namespace {
struct ExtractWs {
  float* buf[2];       // the backbone's ping-pong activations
  float *head, *head2; // scratch of the heads' hidden layers; head2 == head where the size holds one
  void* det_ws;        // the detector's workspace, nested: `det` is its carve
  EinxDetectWs det;
};

// einx_extract's workspace; einx_extract_ws_bytes walks it from a null base.  The second head scratch is a region whenever
// fork_heads() says so, which depends only on the arguments that size the workspace: whether a call then runs the descriptor
// branch beside the detector branch (and uses it) is decided at run time, and moves no region.
ExtractWs carve(WsCarver& c, const einx_extractor* e, const Plan& pl, const einx_detect_params* dp, int B) {
  ExtractWs w;
  w.buf[0] = c.take<float>(pl.buf_elems[0] * B);
  w.buf[1] = c.take<float>(pl.buf_elems[1] * B);
  w.head = c.take<float>(pl.head_elems * B);
  w.head2 = fork_heads(e, pl, B) ? c.take<float>(pl.head_elems * B) : w.head;
  w.det_ws = c.here();
  w.det = einx_detect_carve(c, dp);
  c.slack(256);
  return w;
}
}  // namespace

EINX_EXPORT size_t einx_extract_ws_bytes(const einx_extractor* e, int B, int H, int W, int cap, int nms_iters) {
  Plan pl;
  if (!e || B <= 0 || !make_plan(e, H, W, &pl)) return 0;
  einx_detect_params p;
  detect_params(e, pl, B, H, W, cap > 0 ? cap : 1, nms_budget(nms_iters), &p);
  WsCarver c{nullptr};
  carve(c, e, pl, &p, B);
  return c.bytes;
}

EINX_EXPORT int einx_extract(const einx_extractor* e, float* in, const uint8_t* mask, int B, int H, int W, int nms_iters, void* ws,
                             size_t ws_bytes, const einx_extract_out* o, void* stream) {
  return einx_extract_pad(e, in, mask, EINX_MASK_PAD_ZERO, B, H, W, nms_iters, ws, ws_bytes, o, nullptr, stream);
}

EINX_EXPORT int einx_extract_watch(const einx_extractor* e, float* in, const uint8_t* mask, int B, int H, int W, int nms_iters, void* ws,
                                   size_t ws_bytes, const einx_extract_out* o, const einx_weight_watch* ww, void* stream) {
  return einx_extract_pad(e, in, mask, EINX_MASK_PAD_ZERO, B, H, W, nms_iters, ws, ws_bytes, o, ww, stream);
}

EINX_EXPORT int einx_extract_pad(const einx_extractor* e, float* in, const uint8_t* mask, int mask_pad, int B, int H, int W, int nms_iters,
                                 void* ws, size_t ws_bytes, const einx_extract_out* o, const einx_weight_watch* ww, void* stream) {
  EINX_CHECK_ARG(e && in && ws && o, "null pointer");
  EINX_CHECK_ARG(mask_pad == EINX_MASK_PAD_ZERO || mask_pad == EINX_MASK_PAD_REPLICATE, "mask_pad must be EINX_MASK_PAD_ZERO or EINX_MASK_PAD_REPLICATE");
  EINX_CHECK_ARG(!ww || ww->struct_size == sizeof(einx_weight_watch), "einx_weight_watch::struct_size does not match this library (ABI mismatch)");
  EINX_CHECK_ARG(!ww || ww->n == 0 || (ww->n > 0 && ww->table && ww->ref && ww->scratch && ww->stale), "weight watch with null pointers");
  EINX_CHECK_ARG(o->feats && o->logits && o->raw && o->prob && o->score && o->positions && o->indices && o->counts && o->thr &&
                     o->not_converged && o->sparse_desc,
                 "null output pointer");
  EINX_CHECK_ARG(B > 0 && H > 0 && W > 0 && o->cap > 0, "bad shape");
  Plan pl;
  EINX_CHECK_ARG(make_plan(e, H, W, &pl), "image size does not fit the network's pooling / cell size");
  EINX_CHECK_ARG(e->d.cell == 1 || (o->coarse && o->raw_cl), "cell-8 networks need the coarse / raw_cl outputs");
  EINX_CHECK_ARG(ws_bytes >= einx_extract_ws_bytes(e, B, H, W, o->cap, nms_iters), "workspace smaller than einx_extract_ws_bytes for these arguments");
  einx_detect_params dp;
  detect_params(e, pl, B, H, W, o->cap, nms_budget(nms_iters), &dp);
  WsCarver c{(char*)ws};
  const ExtractWs wk = carve(c, e, pl, &dp, B);
  // (while einx_profile_enable(1) records per-launch times the branches stay in line: its numbers are kernels ALONE on the chip)
  bool fork = fork_heads(e, pl, B) && !einx_profile_active();
  {  // a fork nested inside a caller's own fork crashes hipStreamEndCapture (ROCm 7.2): under capture the branches stay in line
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (fork && hipStreamIsCapturing((hipStream_t)stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) fork = false;
  }
  float* const head2 = fork ? wk.head2 : wk.head;  // the descriptor head's own scratch when the two branches run concurrently
  int rc;
  if (e->d.input_div != 0.0f && e->d.input_div != 1.0f) {  // SuperPointv1: `image /= 255.0` in place on the caller's tensor
    rc = einx_div_inplace(in, (size_t)B * e->backbone.front().cin * H * W, e->d.input_div, stream);
    if (rc) return rc;
  }
  // one un-folded layer: through einx_conv_block_f16 exactly when a binary16 image is set for it and einx_conv_f16_plan covers the call
  auto use_f16 = [&](const einx_conv_desc_f16* c16, int hh, int ww) {
    return c16 && c16->w_f16 && einx_conv_f16_plan(c16->cin, c16->cout, c16->ks, c16->pool, B, hh, ww) != nullptr;
  };
  auto conv = [&](const float* x, int hh, int ww, const einx_conv_desc* c, const einx_conv_desc_f16* c16, float* out, void* st) -> int {
    if (use_f16(c16, hh, ww)) return einx_conv_block_f16(x, B, hh, ww, c16, out, st);
    return einx_conv_block(x, B, hh, ww, 0, 0, hh, ww, c, out, st);
  };
  auto f16_of = [](const std::vector<einx_conv_desc_f16>& L, size_t i) { return i < L.size() ? &L[i] : nullptr; };
  // ---- backbone
  const float* cur = in;
  int h = pl.Hp, w = pl.Wp;
  const int nb = (int)e->backbone.size();
  int first = 0;
  // the first two layers of a 1-channel network as one launch (large launches only: einx_conv_first_two_fused_ok); with a binary16
  // image set for the second layer they are two launches, the first one on the fp32 kernel
  if (nb >= 2 && !use_f16(f16_of(e->backbone16, 1), pl.Hp, pl.Wp) &&
      1 == einx_conv_first_two_fused_ok(&e->backbone[0], &e->backbone[1], B, pl.Hp, pl.Wp)) {
    float* out = (2 < nb) ? wk.buf[1] : o->feats;
    if ((rc = einx_conv_first_two_fused(in, B, H, W, pl.h0, pl.w0, pl.Hp, pl.Wp, &e->backbone[0], &e->backbone[1], out, stream))) return rc;
    if (e->backbone[1].pool) {
      h /= 2;
      w /= 2;
    }
    cur = out;
    first = 2;
  }
  for (int i = first; i < nb; ++i) {
    const einx_conv_desc& c = e->backbone[i];
    float* out = (i + 1 < nb) ? wk.buf[i & 1] : o->feats;
    if (i == 0) rc = einx_conv_block(cur, B, H, W, pl.h0, pl.w0, pl.Hp, pl.Wp, &c, out, stream);
    else rc = conv(cur, h, w, &c, f16_of(e->backbone16, i), out, stream);
    if (rc) return rc;
    if (c.pool) {
      h /= 2;
      w /= 2;
    }
    cur = out;
  }
  // ---- heads (the hidden 3x3 layer of each head goes through a scratch buffer)
  auto run_head = [&](const std::vector<einx_conv_desc>& L, const std::vector<einx_conv_desc_f16>& L16, float* scratch, float* final_out, void* st) -> int {
    const float* x = o->feats;
    for (size_t i = 0; i < L.size(); ++i) {
      float* out = (i + 1 < L.size()) ? scratch : final_out;
      const int r = conv(x, h, w, &L[i], f16_of(L16, i), out, st);
      if (r) return r;
      x = out;
    }
    return 0;
  };
  const int D = e->desc.back().cout;
  // single images: the two heads' first layers as one launch into `head` (det channels first); each head's second layer then reads
  // its slice (one image: a channel slice is contiguous)
  const bool merged = e->has_merged && B == 1;
  if (merged && (rc = conv(o->feats, h, w, &e->merged, &e->merged16, wk.head, stream))) return rc;
  const float* desc_in = wk.head + (size_t)e->det.front().cout * h * w;
  auto det_branch = [&](void* st) -> int {
    if (merged) return conv(wk.head, h, w, &e->det[1], f16_of(e->det16, 1), o->logits, st);
    return run_head(e->det, e->det16, wk.head, o->logits, st);
  };
  // descriptor branch: head convs + the dense by-product that depends on `raw` only
  auto desc_branch = [&](void* st) -> int {
    int r = merged ? conv(desc_in, h, w, &e->desc[1], f16_of(e->desc16, 1), o->raw, st) : run_head(e->desc, e->desc16, head2, o->raw, st);
    if (r) return r;
    if (e->d.cell == 8) r = einx_normalize_map(o->raw, B, D, h * w, e->d.desc_scale, o->coarse, o->raw_cl, st);
    return r;
  };
  std::unique_lock<std::mutex> side_lock;  // (held until the call returns)
  const EinxSide* sd = fork ? einx_side_acquire((hipStream_t)stream, &side_lock) : nullptr;
  if (sd) {  // fork: the descriptor branch runs beside the detector branch
    if (hipEventRecord(sd->fork, (hipStream_t)stream) != hipSuccess || hipStreamWaitEvent(sd->stream, sd->fork, 0) != hipSuccess) {
      einx_set_error("einx_extract: fork failed");
      return EINX_ERR_LAUNCH;
    }
    rc = desc_branch(sd->stream);
    // the join is enqueued even when a launch failed, so that the caller's stream never runs ahead of the side stream
    const bool ok = hipEventRecord(sd->join, sd->stream) == hipSuccess;
    if (rc) {
      (void)hipStreamWaitEvent((hipStream_t)stream, sd->join, 0);
      return rc;
    }
    if (!ok) {
      einx_set_error("einx_extract: join failed");
      return EINX_ERR_LAUNCH;
    }
    if ((rc = det_branch(stream))) {
      (void)hipStreamWaitEvent((hipStream_t)stream, sd->join, 0);
      return rc;
    }
  } else {
    if ((rc = det_branch(stream))) return rc;
    if ((rc = desc_branch(stream))) return rc;
  }
  // the score kernel also zeroes the detection's NMS pass flags (no memset launch) when it has a thread per flag word
  const int C_det = e->det.back().cout;
  const long score_threads = (long)(C_det == 65 ? einx_cdiv(B * h * w, 32) : einx_cdiv(B * h * w, 256)) * 256;
  const bool zero_in_score = wk.det.nflags > 0 && wk.det.nflags <= score_threads;
  rc = einx_score_map_zero(o->logits, B, C_det, h, w, mask, H, W, pl.h0, pl.w0, e->d.dilate_mask, mask_pad, e->d.border, o->prob, o->score,
                           zero_in_score ? wk.det.flags : nullptr, zero_in_score ? wk.det.nflags : 0, o->score_crop, stream);
  if (rc) {
    if (sd) (void)hipStreamWaitEvent((hipStream_t)stream, sd->join, 0);
    return rc;
  }
  // the cropped `nms` output is written by extra workgroups of the sampling launch below (one launch less): the detection only
  // reports which buffer holds the NMS fix-point
  const float* nms_map = nullptr;
  rc = einx_detect_prezeroed(o->score, &dp, wk.det_ws, o->nms, o->positions, o->indices, o->counts, o->thr, o->not_converged, zero_in_score ? 1 : 0,
                             o->nms ? &nms_map : nullptr, stream);
  if (sd && hipStreamWaitEvent((hipStream_t)stream, sd->join, 0) != hipSuccess && !rc) {  // join before the sampler reads `raw`
    einx_set_error("einx_extract: join failed");
    return EINX_ERR_LAUNCH;
  }
  if (rc) return rc;
  const bool bilinear = e->d.cell == 8;
  const bool use_cl = bilinear && D <= 512;
  EinxWatch watch;  // the weight watch rides on spare workgroups of the sampling kernel: no launch of its own
  const bool on = ww && ww->n > 0;
  watch.table = on ? ww->table : nullptr;
  watch.ref = on ? (const unsigned long long*)ww->ref : nullptr;
  watch.hash = on ? (unsigned long long*)ww->scratch : nullptr;
  watch.flag = on ? ww->stale : nullptr;
  watch.n = on ? ww->n : 0;
  watch.bit = 1;
  EinxCrop crop{};
  crop.map = o->nms ? nms_map : nullptr;
  crop.thr = o->thr;
  crop.out = o->nms;
  crop.Hp = pl.Hp;
  crop.Wp = pl.Wp;
  crop.h0 = pl.h0;
  crop.w0 = pl.w0;
  crop.H = H;
  crop.W = W;
  return einx_desc_sample_watch(use_cl ? o->raw_cl : o->raw, B, D, h, w, pl.Hp, pl.Wp, bilinear ? 1 : 0, use_cl ? 1 : 0, o->indices, o->counts,
                                o->cap, e->d.desc_scale, o->sparse_desc, watch, crop, stream);
}

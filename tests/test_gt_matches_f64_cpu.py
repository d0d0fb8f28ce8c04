"""The dense restatement of the ground-truth labelling and matcher_metrics (tests/gt_matches_f64.py) against the reference's fixture
and against the fp32 restatement (tests/gt_matches_ref.py), the exactness claim its GPU companion (test_gt_matches_f64_gpu.py) rests
on, and the conditions every GPU case must hold.  No GPU."""
import numpy as np
import pytest

import gt_matches_f64 as F
import gt_matches_ref as R
from helpers import Golden

G = Golden("gt_matches")
F32 = np.float32


def _same(a, b, what):
    assert np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True), what


def _grid_class(v):
    """'on' the half-integer grid, 'off' on an odd quarter, None otherwise (per coordinate, finite values)"""
    q = v * 4
    return np.where(q % 4 == 2, 1, np.where(q % 2 == 1, 2, 0))


def _wholly_on_or_off(xy):
    fin = np.isfinite(xy).all(1) & (np.abs(xy) < 1e6).all(1)
    cx, cy = _grid_class(xy[fin, 0].astype(np.float64)), _grid_class(xy[fin, 1].astype(np.float64))
    return bool((cx == cy).all() and (cx > 0).all())


# ------------------------------------------------------------------------------------------------ exactness
def test_fp32_evaluation_is_exact_for_every_gpu_case():
    """the claim test_gt_matches_f64_gpu.py relies on: evaluated in float32 -- every input, constant and intermediate -- the
    restatement gives the float64 result bit for bit, for every case and every output the GPU test compares"""
    for name in F.LABEL_CASES:
        c = F.label_case(name)
        for p in c.pairs:
            for a in (p.kp0, p.kp1, p.p01, p.p10, p.p01_h, p.p10_h):
                f = a[~np.isnan(a)].astype(np.float64)
                assert a.dtype == F32 and (f * 4 == np.round(f * 4)).all() and f.min(initial=1) >= 0 and f.max(initial=0) < 512, name
        for form in F.FORMS:
            for b, (e64, e32) in enumerate(zip(F.label_expected(name, form), F.label_expected(name, form, F32))):
                assert e64.keys() == e32.keys()
                for k in e64:
                    _same(e64[k], e32[k], (name, form, b, k))
    s = F.sampler_case()
    for b in range(s.B):
        for kp, dm in ((s.kp0[b], s.depth0[b]), (s.kp1[b], s.depth1[b])):
            (d64, v64, _), (d32, v32, _) = F.sample_depth(kp, dm), F.sample_depth(kp, dm, F32)
            assert d32.dtype == F32
            _same(d64, d32, ("sampler", b))
            _same(v64, v32, ("sampler", b))
    c = F.projection_case()
    for b in range(c.B):
        for pre in (None, c.pre[b]):
            for T10 in (c.T10[b], None):
                kw = dict(precomputed=pre) if pre else dict(depth0=c.depth0[b], depth1=c.depth1[b])
                e64 = F.project_pair(c.kp0[b], c.kp1[b], c.K0[b], c.K1[b], c.T01[b], T10, **kw)
                e32 = F.project_pair(c.kp0[b], c.kp1[b], c.K0[b], c.K1[b], c.T01[b], T10, dt=F32, **kw)
                for k in F.STAGE_A_KEYS:
                    _same(e64[k], e32[k], ("projection", b, pre is None, T10 is None, k))
                assert e32["proj_0to1"].dtype == F32
        _same(F.invert_pose(c.T01[b]), c.T10[b], "inverse pose")
        _same(F.invert_pose(c.T01[b], F32), c.T10[b], "inverse pose")
    for b, (e64, e32) in enumerate(zip(F.scene_expected(), F.scene_expected(F32))):
        for k in F.STAGE_A_KEYS + ("matches0", "matches1", "pos0", "dmin0", "dmin1", "near0", "near1"):
            _same(e64[k], e32[k], ("scene", b, k))


# ------------------------------------------------------------------------------------------------ coverage
def _label_conditions():
    seen = set()
    shapes = {}
    for c in F.LABEL_CASES.values():
        shapes.setdefault((c[0], c[1]), []).extend(c[2])
    assert (1030, 2049) in shapes[(1030, 2049)] and (2048, 1027) in shapes[(2048, 1027)] and (257, 1025) in shapes
    assert any(n == 1030 for n, _ in shapes[(1536, 1100)])  # cap 1536: the workgroups from row 1280 on are wholly past the count
    assert -(-1030 // 256) * 256 < 1536
    assert all(2 <= len(c[2]) <= 3 for c in F.LABEL_CASES.values())
    assert any(1 in nm for v in shapes.values() for nm in v) and any(0 in nm for v in shapes.values() for nm in v)
    assert any(c[4] < c[3] for c in F.LABEL_CASES.values())
    for name in F.LABEL_CASES:
        c = F.label_case(name)
        pose, hom = F.label_expected(name, "pose"), F.label_expected(name, "homography")
        for b, p in enumerate(c.pairs):
            e, h, tag = pose[b], hom[b], (name, b)
            assert not (p.vis0 & np.isnan(p.p01).any(1)).any() and not (p.vis1 & np.isnan(p.p10).any(1)).any(), tag  # the contract
            assert not (p.vis0 & ~p.valid0).any() and not (p.vis1 & ~p.valid1).any(), tag
            if p.n and p.m:
                nan0 = np.isnan(p.p01).any(1)
                assert (e["matches0"][nan0] == -2).all() and (e["matches1"][np.isnan(p.p10).any(1)] == -2).all(), tag
                if nan0.any():
                    seen.add("nan_projection")
            for kind, gadgets in p.info.items():
                for rows, cols in gadgets:
                    i, j = rows[0], cols[0]
                    if kind == "mutual":
                        assert e["matches0"][i] == j and e["matches1"][j] == i and h["matches0"][i] == j, tag
                        if i >= 1024 and j >= 1024:
                            seen.add("mutual_chunk3" if j >= 2048 else "mutual_chunk2")
                    elif kind == "col_tie":
                        for x in (e, h):
                            assert x["tied0"][i] and x["min0"][i] == cols[0] and x["last0"][i] == cols[-1] and x["matches0"][i] == cols[0], tag
                            assert x["matches1"][cols[0]] == i and (x["matches1"][cols[1:]] == -2).all() and (x["min1"][cols] == i).all(), tag
                        assert all(np.array_equal(p.kp1[cols[0]], p.kp1[k]) and np.array_equal(p.p10[cols[0]], p.p10[k]) for k in cols), tag
                        if cols[0] // 1024 != cols[-1] // 1024:
                            seen.add("col_tie_chunks")
                        if cols == [1022, 1023, 1024, 1025]:
                            seen.add("col_tie_boundary")
                        if cols[-1] >= 2048:
                            seen.add("col_tie_chunk3")
                    elif kind == "row_tie":
                        for x in (e, h):
                            assert x["tied1"][j] and x["min1"][j] == rows[0] and x["last1"][j] == rows[-1] and x["matches1"][j] == rows[0], tag
                            assert x["matches0"][rows[0]] == j and (x["matches0"][rows[1:]] == -2).all(), tag
                        if rows[0] // 1024 != rows[-1] // 1024:
                            seen.add("row_tie_chunks")
                        if rows == [1021, 1023, 1024, 1025]:
                            seen.add("row_tie_boundary")
                    elif kind == "pos_eq":  # (3, 0): dist == 9 is not positive (with neg_th = 2 it is negative)
                        lab = -2 if c.neg_th == 5 else -1
                        for x in (e, h):
                            assert x["dmin0"][i] == 9 and x["min0"][i] == j and x["min1"][j] == i and x["pos0"][i] == -1, tag
                            assert x["matches0"][i] == lab and x["matches1"][j] == lab, tag
                        seen.add(kind)
                    elif kind == "pos_in" and c.neg_th == 5:  # (2.75, 1): the neighbour just inside
                        assert e["dmin0"][i] == 8.5625 and e["matches0"][i] == j and e["matches1"][j] == i and h["matches0"][i] == j, tag
                        seen.add(kind)
                    elif kind == "neg_eq" and c.neg_th == 5:  # (3, 4): min dist0 == 25 is not negative
                        for x in (e, h):
                            assert x["near0"][i] == 25 and x["near1"][j] == 25 and x["matches0"][i] == -2 and x["matches1"][j] == -2, tag
                        seen.add(kind)
                    elif kind == "neg_out_valid" and c.neg_th == 5:
                        for x in (e, h):
                            assert x["near0"][i] == 27.0625 and x["matches0"][i] == -1 and x["matches1"][j] == -1, tag
                        seen.add(kind)
                    elif kind == "neg_out_invalid" and c.neg_th == 5:  # the same distance without a valid depth
                        assert e["near0"][i] == 27.0625 and not p.valid0[i] and e["matches0"][i] == -2 and e["matches1"][j] == -2, tag
                        assert h["matches0"][i] == -1 and h["matches1"][j] == -1, tag  # the homography form has no validity
                        seen.add(kind)
                    elif kind == "neg_eq_2" and c.neg_th == 2:  # neg_th < pos_th: min dist0 == 4 is not negative, and positive
                        assert e["near0"][i] == 4 and e["matches0"][i] == j and e["matches1"][j] == i, tag
                        seen.add(kind)
                    elif kind == "neg_out_2" and c.neg_th == 2:  # one lattice step further: negative wins over positive
                        assert e["near0"][i] == 4.0625 and e["pos0"][i] == j and e["matches0"][i] == -1 and e["matches1"][j] == -1, tag
                        seen.add(kind)
                    elif kind == "asymmetric":  # dist0 alone would take the first column
                        assert e["min0_dist0_only"][i] == cols[0] and e["matches0"][i] == cols[1] and e["matches1"][cols[1]] == i, tag
                        assert h["matches0"][i] == cols[1], tag
                        seen.add(kind)
                    elif kind == "invisible_nearest":
                        assert e["nearest0_any"][i] == cols[0] and not p.vis1[cols[0]] and e["near0"][i] == 0.25 and e["matches0"][i] == cols[1], tag
                        seen.add(kind)
                    elif kind == "invisible_nearest_far" and c.neg_th == 5:  # counted visible-only it would be 36 > 25: unmatched
                        assert e["near0"][i] == 1 and e["dmin0"][i] == 36 and p.valid0[i] and e["matches0"][i] == -2, tag
                        seen.add(kind)
                    elif kind == "origin_invisible":
                        assert (i, j) == (0, 0) and e["min0"][0] == 0 and e["min1"][0] == 0 and np.isinf(e["dmin0"][0]) and np.isinf(e["dmin1"][0]), tag
                        assert e["pos0"][0] == -1 and e["matches0"][0] == -2 and e["matches1"][0] == -2, tag
                        seen.add(kind)
                    elif kind == "nan_projection":
                        assert np.isnan(p.p01[i]).all() and np.isnan(p.p10[j]).all() and e["matches0"][i] == -2 and e["matches1"][j] == -2, tag
                        if i >= 1024 or j >= 1024:
                            seen.add("nan_projection_late")
            if p.n and p.m:
                if (e["matches0"] >= 2048).any() or (e["matches1"] >= 2048).any():
                    seen.add("match_2048")
                if (e["matches0"] >= 1024).any():
                    seen.add("matches0_1024")
                if (e["matches1"] >= 1024).any():
                    seen.add("matches1_1024")
                if (e["matches0"] != np.where(e["min0_dist0_only"] == e["min0"], e["matches0"], -3)).any():
                    seen.add("dist1_decides")
                if e["at_pos"] and e["at_neg"] and e["tied0"].any() and e["tied1"].any():
                    seen.add("background_equalities")
            else:
                assert (e["matches0"] == -1).all() and (e["matches1"] == -1).all() and (e["pos0"] == -1).all()
                seen.add("early_return")
    return seen


def test_gpu_cases_hold_what_the_gpu_test_needs():
    """every condition of the planted edges, asserted from the float64 restatement alone: a case that stops exercising its edge
    fails here, without a GPU"""
    need = {"mutual_chunk2", "mutual_chunk3", "col_tie_chunks", "col_tie_boundary", "col_tie_chunk3", "row_tie_chunks", "row_tie_boundary",
            "pos_eq", "pos_in", "neg_eq", "neg_out_valid", "neg_out_invalid", "neg_eq_2", "neg_out_2", "asymmetric", "invisible_nearest",
            "invisible_nearest_far", "origin_invisible", "nan_projection", "nan_projection_late", "match_2048", "matches0_1024",
            "matches1_1024", "dist1_decides", "background_equalities", "early_return"}
    seen = _label_conditions()
    assert need <= seen, need - seen

    # ---- the sampler
    s = F.sampler_case()
    assert s.size0 != s.size1 and s.n[1] < s.cap0 and s.m[1] < s.cap1
    for b in range(s.B):
        for kp, dm in ((s.kp0[b], s.depth0[b]), (s.kp1[b], s.depth1[b])):
            H, W = dm.shape
            assert _wholly_on_or_off(kp)
            assert (dm == 0).any() and (dm < 0).any() and np.isnan(dm).any()
            good = dm[dm > 0].astype(np.float64)
            assert (good * 64 == np.round(good * 64)).all()
            d, valid, info = F.sample_depth(kp, dm)
            x, y = kp[:, 0].astype(np.float64), kp[:, 1].astype(np.float64)
            fin = np.isfinite(x) & np.isfinite(y) & (np.abs(x) < 1e6) & (np.abs(y) < 1e6)
            on = fin & (_grid_class(np.where(fin, x, 0.5)) == 1)
            assert set(info["taps_outside"][fin].tolist()) == {0, 2, 3, 4}
            if len(kp) == len(F._sampler_points(H, W)):
                border = {(px, py) for px in range(W) for py in range(H) if px in (0, W - 1) or py in (0, H - 1)}
                assert border <= {(int(a - 0.5), int(c - 0.5)) for a, c in zip(x[on], y[on])}  # every border pixel, the corners
                for qx, qy in ((0.25, 0.25), (W - 0.25, 0.25), (0.25, H - 0.25), (W - 0.25, H - 0.25), (0.25, 3.25), (W - 0.25, 3.75),
                               (5.25, 0.25), (5.75, H - 0.25)):
                    assert ((x == qx) & (y == qy)).any()
                for qx, qy in ((1e10, 4.5), (-1e10, 4.5), (np.inf, 4.5), (5.5, np.inf)):
                    assert ((x == qx) & (y == qy)).any()
                assert (np.isnan(x) & (y == 4.5)).any() and ((x == 5.5) & np.isnan(y)).any()
            out = ~fin | (info["taps_outside"] == 4)
            assert out.sum() >= 20 and (d[out] == 0).all() and not valid[out].any()
            on_border = on & ((x == 0.5) | (x == W - 0.5) | (y == 0.5) | (y == H - 0.5))
            assert np.isnan(d[on_border]).any() and valid[on_border].any()  # a hole under the one tap of a border point
            off_fb = fin & ~on & info["fallback"] & (info["taps_outside"] < 4)
            assert set(info["nearest"][off_fb].tolist()) == {0, 1, 2}  # a weighted hole: nearest good / a hole / outside the map
            assert valid[off_fb & (info["nearest"] == 0)].all() and np.isnan(d[off_fb & (info["nearest"] == 1)]).all()
            assert (d[off_fb & (info["nearest"] == 2)] == 0).all()
            part = fin & ~on & ~info["fallback"] & np.isin(info["taps_outside"], (2, 3))
            assert valid[part].any()  # a zero-padded tap in a sum that stands

    # ---- the projection
    c = F.projection_case()
    eps, nxt = np.float64(F.EPS_Z), np.float64(np.nextafter(F.EPS_Z, F32(1)))
    tags = [set(), set()]
    for b in range(c.B):
        assert _wholly_on_or_off(c.kp0[b]) and _wholly_on_or_off(c.kp1[b])
        pre = F.project_pair(c.kp0[b], c.kp1[b], c.K0[b], c.K1[b], c.T01[b], c.T10[b], precomputed=c.pre[b])
        maps = F.project_pair(c.kp0[b], c.kp1[b], c.K0[b], c.K1[b], c.T01[b], c.T10[b], depth0=c.depth0[b], depth1=c.depth1[b])
        for side, (planted, Ko, kp, size) in enumerate(zip(c.planted[b], (c.K1[b], c.K0[b]), (c.kp0[b], c.kp1[b]), (c.size0, c.size1))):
            pk, vk = ("proj_0to1", "visible0") if side == 0 else ("proj_1to0", "visible1")
            wmax, hmax = 2 * float(Ko[0, 2]) - 1, 2 * float(Ko[1, 2]) - 1
            assert (kp[:, 0] >= 0.5).all() and (kp[:, 0] <= size[1] - 0.5).all() and (kp[:, 1] >= 0.5).all() and (kp[:, 1] <= size[0] - 0.5).all()
            assert not (maps[f"depth_keypoints{side}"] == 0).any()  # inside the map: 2, 1e-4 or NaN, never the 0 of zero padding
            for i, tag, uv in planted:
                inside = 0 <= uv[0] <= wmax and 0 <= uv[1] <= hmax
                assert inside == (tag[-1] not in "+-")
                exact = {"u0": uv[0] == 0, "umax": uv[0] == wmax, "v0": uv[1] == 0, "vmax": uv[1] == hmax, "u-": uv[0] == -0.25,
                         "u+": uv[0] == wmax + 0.25, "v-": uv[1] == -0.25, "v+": uv[1] == hmax + 0.25}
                assert exact.get(tag, True)
                for e in (pre, maps):
                    assert tuple(e[pk][i]) == uv and e[vk][i] == inside and e[f"side{side}"]["front"][i], (b, side, i)
                    assert e[f"side{side}"]["inside"][i] == inside
                tags[side].add(tag)
            assert pre[vk].any() and not pre[vk].all() and maps[vk].any() and np.isnan(maps[pk]).any()
            z = pre[f"side{side}"]["qz"]
            assert (np.log2(z) == np.round(np.log2(z)))[2 if b == 2 else 0:].all()  # every q.z a power of two
        if b == 2:  # the front boundary
            for e, zs in ((pre, ((eps, nxt), (eps, nxt))), (maps, ((eps, eps), (nxt, nxt)))):
                for side, Ko in ((0, c.K1[b]), (1, c.K0[b])):
                    pk, vk = ("proj_0to1", "visible0") if side == 0 else ("proj_1to0", "visible1")
                    for i in (0, 1):
                        assert e[f"side{side}"]["qz"][i] == zs[side][i] and e[f"side{side}"]["front"][i] == (zs[side][i] > eps)
                        assert tuple(e[pk][i]) == (Ko[0, 2], Ko[1, 2]) and e[vk][i] == (zs[side][i] > eps)
            assert not np.any(c.T01[b][:3, 3])
    for side in (0, 1):
        assert {"u0", "umax", "v0", "vmax", "u-", "u+", "v-", "v+"} <= tags[side], (side, tags[side])
    assert tags[0] | tags[1] >= {"c00", "cmm", "c0m", "cm0"}

    # ---- the whole scene
    c = F.scene_case()
    assert min(c.n + c.m) > 1024 and c.n[1] < c.cap0 and c.m[1] < c.cap1
    for b, e in enumerate(F.scene_expected()):
        assert _wholly_on_or_off(c.kp0[b]) and _wholly_on_or_off(c.kp1[b])
        assert (e["matches0"] >= 1024).sum() > 20 and (e["matches1"][1024:] >= 0).sum() > 20 and (e["matches0"] > -1).sum() > 200
        for k in ("matches0", "matches1"):
            assert {-2, -1} <= set(e[k].tolist())
        assert np.isnan(e["depth_keypoints0"]).any() and (~e["valid1"]).any() and e["sample0"]["fallback"].any()
        assert set(np.unique(e["depth_keypoints0"][e["valid0"]]).tolist()) == {F.PLANE}
        assert e["visible0"].mean() > 0.5 and (e["valid0"] & ~e["visible0"]).any()

    # ---- matcher_metrics
    for cap in F.PR_CAPS:
        m, gt, sc, n, names, ties = F.pr_case(cap)
        exp = F.pr_expected(cap)
        assert (n <= cap).all() and ((n < cap).sum() >= len(n) - 4 or cap == 1) and sc.dtype == F32
        assert np.isnan(exp[names.index("no_rows")]).all() and np.isfinite(np.delete(exp, names.index("no_rows"), 0)).all()
        for b, (lo, hi) in ties.items():  # the tied rows differ in correctness: the other order of equal scores moves AP
            nb = n[b]
            assert sc[b, lo] == sc[b, hi] == sc[b, :nb].max() and lo < hi < nb and (m[b, lo] == gt[b, lo]) != (m[b, hi] == gt[b, hi])
            other = F.matcher_metrics(m[b, :nb][::-1], gt[b, :nb][::-1], sc[b, :nb][::-1])
            assert np.array_equal(other[:3], exp[b, :3]) and abs(other[3] - exp[b, 3]) > 1e-6, (cap, names[b])
        if cap >= 130:
            assert ties[names.index("same_lane_low_right")] == (5, 69) and ties[names.index("same_lane_high_right")] == (5, 69)
            assert ties[names.index("higher_lane_low_right")] == (7, 70) and ties[names.index("higher_lane_high_right")] == (7, 70)
        if cap > 1:
            assert {names.index(k) for k in ("all_equal", "all_minus_inf", "higher_lane_low_right")} <= set(ties)
            b = names.index("past_count")
            assert n[b] < cap and sc[b, n[b]:].min() > sc[b, :n[b]].max() and (m[b, n[b]:] == gt[b, n[b]:]).all()
            assert np.isneginf(sc[names.index("all_minus_inf"), :n[names.index("all_minus_inf")]]).all()
            assert np.isposinf(sc[names.index("plus_inf_top")]).sum() == 1
        rows = lambda k: (gt[names.index(k), :n[names.index(k)]], m[names.index(k), :n[names.index(k)]])  # noqa: E731
        g, _ = rows("no_recall_rows")
        assert (g > -1).sum() == 0 and exp[names.index("no_recall_rows"), 0] == 0
        g, mm = rows("no_precision_rows")
        assert ((mm > -1) & (g >= -1)).sum() == 0 and exp[names.index("no_precision_rows"), 1] == 0
        g, _ = rows("no_accuracy_rows")
        assert (g >= -1).sum() == 0 and exp[names.index("no_accuracy_rows"), 2] == 0


# ------------------------------------------------------------------------------------------------ against the reference's fixture
def _close(got, exp, bound, what):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(exp)), f"{what}: NaN pattern"
    fin = ~np.isnan(exp)
    err = float(np.abs(got - exp)[fin].max()) if fin.any() else 0.0
    print(f"{what}: max |error| {err:.3e} (bound {bound:.3e})")
    assert err <= bound, what


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_restatement_equals_reference_fixture(name):
    """cases (a), (b), (d) of tests/golden/gt_matches.npz in float64: discrete outputs exactly, floats within the fixture's bounds"""
    c = G.cases[name]
    sc = R.POSE_CASES[name](c["seed"])
    for b in range(c["B"]):
        n, m = int(sc["n"][b]), int(sc["m"][b])
        exp = R.fixture_pair(G, f"{name}.{b}", n, m)
        kp0, kp1 = sc["kp0"][b, :n], sc["kp1"][b, :m]
        if exp is None:
            e = F.label(kp0, kp1, kp0, kp1, None, None, None, None, c["pos_th"], c["neg_th"])
            assert np.array_equal(e["matches0"], G[f"{name}.{b}.tuple.matches0"]) and np.array_equal(e["matches1"], G[f"{name}.{b}.tuple.matches1"])
            continue
        kw = dict(precomputed=R.precomputed_depths(sc, b)) if name == "b" else dict(depth0=sc["depth0"][b], depth1=sc["depth1"][b])
        e = F.project_pair(kp0, kp1, sc["K0"][b], sc["K1"][b], sc["T01"][b], sc["T10"][b], **kw)
        for side in "01":
            assert np.array_equal(e[f"visible{side}"], exp[f"visible{side}"]), (name, b, side)
            _close(e[f"depth_keypoints{side}"], exp[f"depth_keypoints{side}"], c["bounds"]["depth"], f"{name}.{b} depth{side}")
        _close(e["proj_0to1"], exp["proj_0to1"], c["bounds"]["proj"], f"{name}.{b} proj_0to1")
        _close(e["proj_1to0"], exp["proj_1to0"], c["bounds"]["proj"], f"{name}.{b} proj_1to0")
        lab = F.label(kp0, kp1, e["proj_0to1"], e["proj_1to0"], e["visible0"], e["visible1"], e["valid0"], e["valid1"], c["pos_th"], c["neg_th"],
                      keep=True)
        assert np.array_equal(lab["matches0"], exp["matches0"]) and np.array_equal(lab["matches1"], exp["matches1"]), (name, b)
        assert np.array_equal(lab["positive"], exp["assignment"]), (name, b)
        epi = R.epipolar_all(kp0, kp1, sc["K0"][b], sc["K1"][b], sc["T01"][b])  # not part of the labelling: the dense `reward` only
        reward = (lab["dist"] < c["pos_th"] ** 2).astype(F32) - (epi > c["neg_th"]).astype(F32)
        sure = np.ones(n * m, bool)
        sure[exp["reward_unsure"]] = False
        assert np.array_equal(reward.reshape(-1)[sure], exp["reward"].reshape(-1)[sure]) and sure.mean() > 0.999, (name, b)


@pytest.mark.parametrize("name", ["c", "c_neg_lt_pos"])
def test_restatement_equals_reference_fixture_homography_form(name):
    """case (c): the labelling of gt_generation.py:186-213 on the reference's own warps"""
    c = G.cases[name]
    sc = R.homography_scene(c["seed"], c["B"], c["n"], c["m"])
    B, n, m = c["B"], c["n"], c["m"]
    assignment = np.unpackbits(G[f"{name}.assignment"])[:B * n * m].reshape(B, n, m).astype(bool)
    for b in range(B):
        lab = F.label(sc["kp0"][b], sc["kp1"][b], G[f"{name}.proj_0to1"][b], G[f"{name}.proj_1to0"][b], None, None, None, None, c["pos_th"],
                      c["neg_th"], keep=True)
        assert np.array_equal(lab["matches0"], G[f"{name}.matches0"][b]) and np.array_equal(lab["matches1"], G[f"{name}.matches1"][b])
        assert np.array_equal(lab["positive"], assignment[b])
        reward = (lab["dist"] < c["pos_th"] ** 2).astype(F32) - (lab["dist"] > c["neg_th"] ** 2).astype(F32)
        assert np.array_equal(reward, G[f"{name}.reward"][b])


def test_restatement_equals_reference_fixture_matcher_metrics():
    """the long form of ranking_ap in float64 against the reference's float32 run: 1e-4 as test_gt_matches_cpu.py argues it"""
    for name, (m, gt, sc) in R.pr_cases().items():
        got = np.stack([F.matcher_metrics(m[b], gt[b], sc[b]) for b in range(len(m))])
        err = np.abs(got - G[f"pr.{name}"]).max()
        print(f"pr.{name}: max |float64 long form - reference| {err:.2e}")
        assert err <= 1e-4, name


# ------------------------------------------------------------------------------------------------ two texts, one answer
def test_restatement_equals_the_fp32_restatement():
    """gt_matches_ref.sample_depth / project_side / label / match_pr (written along the kernel's operation order) agree with the
    dense restatement (written from the reference's text) on the exact cases"""
    s = F.sampler_case()
    for b in range(s.B):
        for kp, dm in ((s.kp0[b], s.depth0[b]), (s.kp1[b], s.depth1[b])):
            far = ~(np.abs(kp) < 1e6).all(1)  # gt_matches_ref casts floor(ix) to int64: it takes no far, infinite or NaN coordinate
            d, v, _ = F.sample_depth(kp[~far], dm)
            rd, rv = R.sample_depth(kp[~far], dm)
            _same(d, rd, ("sampler", b))
            _same(v, rv, ("sampler", b))
    c = F.projection_case()
    for b in range(c.B):
        for pre in (None, c.pre[b]):
            kw = dict(precomputed=pre) if pre else dict(depth0=c.depth0[b], depth1=c.depth1[b])
            e = F.project_pair(c.kp0[b], c.kp1[b], c.K0[b], c.K1[b], c.T01[b], c.T10[b], **kw)
            for side, (kp, Ks, Ko, T) in enumerate(((c.kp0[b], c.K0[b], c.K1[b], c.T01[b]), (c.kp1[b], c.K1[b], c.K0[b], c.T10[b]))):
                r = R.project_side(kp, e[f"depth_keypoints{side}"].astype(F32), e[f"valid{side}"], Ks, Ko, T)
                _same(r["proj"], e["proj_0to1" if side == 0 else "proj_1to0"], ("projection", b, side))
                _same(r["visible"], e[f"visible{side}"], ("projection", b, side))
        _same(R.invert_pose_f32(c.T01[b]), c.T10[b], "inverse pose")
    for name in F.LABEL_CASES:
        c = F.label_case(name)
        for form in F.FORMS:
            for b, (p, e) in enumerate(zip(c.pairs, F.label_expected(name, form))):
                m0, m1, pos0 = R.label(*F.label_inputs(p, form), c.pos_th, c.neg_th)
                assert np.array_equal(m0, e["matches0"]) and np.array_equal(m1, e["matches1"]) and np.array_equal(pos0, e["pos0"]), (name, form, b)
    sc = F.scene_case()
    for b, e in enumerate(F.scene_expected()):
        one = dict(kp0=sc.kp0[b][None], kp1=sc.kp1[b][None], depth0=sc.depth0[b][None], depth1=sc.depth1[b][None], K0=sc.K0[b][None],
                   K1=sc.K1[b][None], T01=sc.T01[b][None], T10=sc.T10[b][None], n=[sc.n[b]], m=[sc.m[b]])
        r = R.project(one, 0)
        for k, rk in (("depth_keypoints0", "d0"), ("depth_keypoints1", "d1"), ("valid0", "valid0"), ("valid1", "valid1"), ("proj_0to1", "proj01"),
                      ("proj_1to0", "proj10"), ("visible0", "visible0"), ("visible1", "visible1")):
            _same(e[k], r[rk], ("scene", b, k))
        m0, m1, pos0 = R.label(sc.kp0[b], sc.kp1[b], r["proj01"], r["proj10"], r["visible0"], r["visible1"], r["valid0"], r["valid1"], sc.pos_th, sc.neg_th)
        assert np.array_equal(m0, e["matches0"]) and np.array_equal(m1, e["matches1"]) and np.array_equal(pos0, e["pos0"])
    worst = 0.0
    for cap in F.PR_CAPS:
        m, gt, s, n, names, _ = F.pr_case(cap)
        exp = F.pr_expected(cap)
        got = np.stack([R.match_pr(m[b, :n[b]], gt[b, :n[b]], s[b, :n[b]]) for b in range(len(n))])
        assert np.array_equal(got[:, :3], exp[:, :3], equal_nan=True), cap
        assert np.array_equal(np.isnan(got[:, 3]), np.isnan(exp[:, 3]))
        err = float(np.nanmax(np.abs(got[:, 3] - exp[:, 3])))
        worst = max(worst, err / (cap * 2.0 ** -52))
        print(f"match_pr cap {cap}: closed form vs long form {err:.3e} (bound {cap * 2.0 ** -52:.3e})")
        assert err <= cap * 2.0 ** -52, cap  # cap float64 roundings of terms of magnitude <= 1
    assert worst <= 1

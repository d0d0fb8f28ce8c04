"""GPU tests of the relative-pose refinement (csrc/pose.hip: pose_refine_kernel) against the float64 restatement
tests/pose_refine_f64.py on the fixed cases of tests/pose_refine_cases.py, whose bounds and margins tests/test_pose_refine_cpu.py
establishes on the restatement alone; certificates computed from the outputs alone; bit-for-bit independence of slot, batch size,
layout and run; the pass-through and degenerate inputs; the wiring up to the evaluator.  No case is pinned or exempted."""
from importlib import import_module

import numpy as np
import pytest
import torch

import pose_f64 as P
import pose_refine_cases as C
from gpu_support import DEV, _np, _t, pkg
from helpers import synth, synth_raw_events

pytestmark = pytest.mark.gpu
NM = import_module(pkg.__name__ + ".core.metrics._native_metrics")
MM = import_module(pkg.__name__ + ".core.metrics.matching_metrics")
POSE_GATE = 10 * C.REFINE_FLOOR   # device against the restatement (pose_distance)
CLEAN_GATE = 10 * C.CLEAN_WORST   # device against the true pose on the noise-free, outlier-free cases
NAMES = list(C.CASES)


def _stack(names, cap=C.CAP, cols=3, ordering="yx", nmatch=None, T=True, status=None, k64=None):
    """cases -> the arguments of refine_relative_pose: (mk0, mk1, nmatch, K0, K1, R, t, mask, status), T_0to1"""
    B = len(names)
    mk0, mk1 = np.zeros((B, cap, cols), np.float32), np.zeros((B, cap, cols), np.float32)
    nm, st = np.zeros(B, np.int32), np.zeros(B, np.int32)
    R, t, mask = np.zeros((B, 3, 3)), np.zeros((B, 3)), np.zeros((B, cap), bool)
    if k64 is None:
        k64 = any(C.scene(n)["K0"].dtype == np.float64 for n in names)
    assert all((C.scene(n)["K0"].dtype == np.float64) == k64 for n in names)  # a batch has one dtype of K
    for b, name in enumerate(names):
        s = C.scene(name)
        a0, a1 = s["kp0"].copy(), s["kp1"].copy()
        if ordering == "xy":
            a0[:, :2], a1[:, :2] = a0[:, 1::-1].copy(), a1[:, 1::-1].copy()
        n = min(len(a0), cap)
        mk0[b, :n], mk1[b, :n], nm[b] = a0[:n, :cols], a1[:n, :cols], len(a0)
        R[b], t[b], m, st[b] = C.initial(name)
        mask[b, :n] = m[:n]
    if nmatch is not None:
        nm = np.asarray(nmatch, np.int32)
    if status is not None:
        st = np.asarray(status, np.int32)
    args = (_t(mk0), _t(mk1), _t(nm), _t(np.stack([C.scene(n)["K0"] for n in names])), _t(np.stack([C.scene(n)["K1"] for n in names])),
            _t(R), _t(t), _t(mask), _t(st))
    return args, (_t(np.stack([C.scene(n)["T"] for n in names])) if T else None)


def _run(args, T, ordering="yx", **kw):
    out = [_np(x) for x in NM.refine_relative_pose(*args, T, ordering=ordering, **kw)]  # R, t, mask, info, rows, cost
    torch.cuda.synchronize()
    return out


def _same(x, y, msg=None):
    for a, b in zip(x, y):
        assert np.array_equal(a, b, equal_nan=True), msg


def _row(out, b):
    return [x[b] for x in out]


def _groups():
    """the cases grouped by what one call shares: the options and the dtype of K"""
    g = {}
    for n in NAMES:
        g.setdefault((tuple(sorted(C.kwargs(n).items())), C.scene(n)["K0"].dtype == np.float64), []).append(n)
    return g


@pytest.fixture(scope="module")
def results():
    """{case: its device outputs}, from one call per group of cases"""
    out = {}
    for (kw, _), names in _groups().items():
        args, T = _stack(names)
        got = _run(args, T, **dict(kw))
        for b, n in enumerate(names):
            out[n] = _row(got, b)
    return out


def _sampson_mask(R, t, name):
    s = C.scene(name)
    x1, x2 = P.normalize(s["kp0"][:, 1::-1], s["K0"]), P.normalize(s["kp1"][:, 1::-1], s["K1"])
    thr = P.ransac_threshold(C.kwargs(name)["thresh"], s["K0"], s["K1"])
    return P.sampson_f32(P.skew(t) @ R, x1, x2)[0] <= np.float32(thr * thr), x1, x2


# ------------------------------------------------------------------ against the restatement
def test_cases_match_the_restatement(results):
    worst, accepted = (0.0, None), {}
    for name in NAMES:
        ref, (R, t, mask, info, rows, cost) = C.ref(name), results[name]
        n = len(C.scene(name)["kp0"])
        assert (info[0], info[1], info[3]) == (ref["info"][0], ref["info"][1], ref["info"][3]), (name, info, ref["info"])
        assert np.array_equal(mask[:n], ref["mask"]) and not mask[n:].any(), name
        d = C.pose_distance(R, t, ref["R"], ref["t"])
        if d > worst[0]:
            worst = (d, name)
        assert d <= POSE_GATE, (name, d)
        want = np.array(ref["rows"])
        assert np.abs(rows[:3] - want[:3]).max() <= 1e-5 and rows[3] == want[3], (name, rows, want)  # degrees
        if info[2] != ref["info"][2]:
            accepted[name] = (int(info[2]), ref["info"][2])
        if info[1] > 0:
            assert np.allclose(cost, ref["cost"], rtol=1e-6, atol=0), (name, cost, ref["cost"])
        else:
            assert np.isnan(cost).all(), name
    print(f"worst pose distance from the restatement {worst[0]:.3e} ({worst[1]}; gate {POSE_GATE:.3e}); accepted steps that differ "
          f"(device, restatement; not gated): {accepted}")


# ------------------------------------------------------------------ certificates from the outputs alone
def test_certificates(results):
    for name in NAMES:
        R, t, mask, info, rows, cost = results[name]
        n = len(C.scene(name)["kp0"])
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0, name
        assert abs(np.linalg.norm(t) - 1.0) <= 1e-12, name
        if info[1] > 0:
            assert cost[1] <= cost[0], (name, cost)
        R0, t0, m0, _ = C.initial(name)
        if info[0] == 1:
            inl, x1, x2 = _sampson_mask(R, t, name)
            want = np.zeros(n, bool)
            sel = np.nonzero(inl)[0]
            want[sel] = P.triangulate_ok(R, t, x1[sel], x2[sel])
            assert np.array_equal(mask[:n], want), name
            assert np.count_nonzero(inl) >= np.count_nonzero(_sampson_mask(R0, t0, name)[0]), name  # the keep rule
            assert info[2] > 0, name
        else:
            assert np.array_equal(R, R0) and np.array_equal(t, t0) and np.array_equal(mask[:n], m0), name
        assert rows[3] == mask[:n].mean() and not mask[n:].any(), name
    assert {n for n in NAMES if results[n][3][0] == 0} == C.NOT_KEPT


def test_noise_free_cases_reach_the_truth(results):
    names = [n for n in NAMES if C.clean_case(n)]
    assert len(names) >= 4
    for name in names:
        assert C.CASES[name][4] == 0.5  # from the truth perturbed by half a degree
        d = C.pose_distance(results[name][0], results[name][1], *C.truth(name))
        assert d <= CLEAN_GATE, (name, d)


def test_refinement_improves_the_noisy_cases(results):
    names = [n for n in NAMES if C.noisy_case(n)]
    before = np.array([C.pose_err_before(n) for n in names])
    after = np.array([results[n][4][2] for n in names])
    print("mean pose_err before", before.mean(), "after", after.mean())
    assert after.mean() < before.mean()


# ------------------------------------------------------------------ bit for bit
BITS = ["n64_cams", "forward", "ransac_64", "ransac_255", "n1024", "n5", "few_inliers"]  # float32 K and the default options: one call


@pytest.fixture(scope="module")
def bits_batch():
    names = list(BITS)
    args, T = _stack(names)
    return names, args, T, _run(args, T)


def test_run_to_run_and_alone_and_reversed(bits_batch, results):
    names, args, T, out = bits_batch
    _same(_run(args, T), out, "repeat")
    rev = _run(*_stack(names[::-1]))
    for b, n in enumerate(names):
        _same(_row(out, b), results[n], ("against its group's batch", n))
        _same(_row(rev, len(names) - 1 - b), _row(out, b), ("reversed slots", n))
        _same(_row(_run(*_stack([n])), 0), _row(out, b), ("alone", n))


def test_layouts(bits_batch):
    names, args, T, out = bits_batch
    _same(_run(*_stack(names, cols=2)), out, "two columns")
    _same(_run(*_stack(names, ordering="xy"), ordering="xy"), out, "xy on swapped columns")
    a, T = _stack(["n1024", "ransac_64"])
    over = [C.CAP + 7, 64]
    got = _run(*_stack(["n1024", "ransac_64"], nmatch=over))
    _same(got, _run(a, T), "nmatch = cap + 7")


def test_batch_over_64_pairs():
    tile = ["n5", "n6_clean", "n64_clean", "ransac_64", "ransac_64_clean", "n64_cams", "few_inliers"]  # cap 64 holds them
    names = [tile[b % len(tile)] for b in range(130)]
    out = _run(*_stack(names, cap=64))
    for e, n in enumerate(tile):
        alone = _row(_run(*_stack([n], cap=64)), 0)
        for b in range(e, 130, len(tile)):
            _same(_row(out, b), alone, (n, b))
    assert len({names[b] for b in (63, 64, 65)}) == 3 and len({names[b] for b in (127, 128, 129)}) == 3


def test_graph_replay(bits_batch):
    names, args, T, out = bits_batch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        NM.refine_relative_pose(*args, T)  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = NM.refine_relative_pose(*args, T)
    g.replay()
    torch.cuda.synchronize()
    _same([_np(x) for x in res], out, "graph replay")


# ------------------------------------------------------------------ pass-through and degenerate inputs
def test_negative_status_passes_through():
    names = [C.NEGATIVE, "ransac_64", C.NEGATIVE]
    R, t, mask, info, rows, cost = _run(*_stack(names, status=[-2, 0, -1]))
    for b in (0, 2):
        assert not R[b].any() and not t[b].any() and not mask[b].any(), b
        assert np.array_equal(rows[b], [np.inf, np.inf, np.inf, 0.0]) and list(info[b]) == [-1, 0, 0, 0] and np.isnan(cost[b]).all(), b
    assert info[1][0] == 1  # its neighbours do not disturb the pair with a pose


def test_small_sets_return_the_input(results):
    for name in ("n5", "few_inliers"):
        R, t, mask, info, rows, cost = results[name]
        R0, t0, m0, _ = C.initial(name)
        n = len(m0)
        assert list(info) == [0, 0, 0, 0] and np.array_equal(R, R0) and np.array_equal(t, t0) and np.array_equal(mask[:n], m0), name
        assert np.isnan(cost).all() and rows[3] == m0.mean(), name
    assert list(results["rejected"][3][:2]) == [0, 2] and results["rejected"][3][2] > 0


def test_degenerate_scenes_are_finite_or_pass_through():
    names = list(C.DEGENERATE)
    args, T = _stack(names)
    R, t, mask, info, rows, cost = _run(args, T)
    for b, name in enumerate(names):
        R0, t0, m0, _ = C.initial(name)
        if info[b][0] == 1:
            assert np.isfinite(R[b]).all() and np.isfinite(t[b]).all(), name
            assert np.abs(R[b] @ R[b].T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.norm(t[b]) - 1.0) <= 1e-12, name
        else:
            assert np.array_equal(R[b], R0) and np.array_equal(t[b], t0) and np.array_equal(mask[b, :len(m0)], m0), name
        assert np.isfinite(rows[b][[0, 2, 3]]).all(), (name, rows[b])
        if name == "pure_rotation":  # t_gt = 0: 8b's rule, a NaN t_err and pose_err = R_err
            assert np.isnan(rows[b][1]) and rows[b][2] == rows[b][0]
        else:
            assert np.isfinite(rows[b][1]), name


def test_without_a_true_pose_only_the_error_rows_change(bits_batch):
    names, args, T, out = bits_batch
    got = _run(args, None)
    _same([got[i] for i in (0, 1, 2, 3, 5)], [out[i] for i in (0, 1, 2, 3, 5)])
    assert np.isnan(got[4][:, :3]).all() and np.array_equal(got[4][:, 3], out[4][:, 3])


# ------------------------------------------------------------------ wiring
@pytest.fixture(scope="module")
def ransac_batch():
    names = ["ransac_64", "n64_cams", "ransac_255", "n5", "forward"]
    args, T = _stack(names, cap=320)
    return names, args[:5], T


def test_relative_pose_refine_equals_the_two_calls(ransac_batch):
    _, head, T = ransac_batch
    kw = dict(max_iters=200)
    plain = NM.relative_pose(*head, T, **kw)
    by_hand = NM.refine_relative_pose(*head, *plain[:4], T)
    both = NM.relative_pose(*head, T, refine=True, **kw)
    off = NM.relative_pose(*head, T, refine=False, **kw)
    torch.cuda.synchronize()
    _same([_np(x) for x in off], [_np(x) for x in plain], "refine=False")
    _same([_np(x) for x in both], [_np(x) for x in (by_hand[0], by_hand[1], by_hand[2], plain[3], by_hand[4])], "refine=True")
    assert both[2].dtype == torch.bool and _np(by_hand[3])[:, 0].max() == 1  # some pair keeps its refinement
    other = NM.relative_pose(*head, T, refine=True, refine_rounds=1, refine_iters=3, **kw)
    _same([_np(x) for x in other[:2]], [_np(x) for x in NM.refine_relative_pose(*head, *plain[:4], T, rounds=1, lm_iters=3)[:2]])
    mr = type("MR", (), {"mk0": head[0], "mk1": head[1], "nmatch": head[2]})()
    _same([_np(x) for x in NM.batch_relative_pose(mr, head[3], head[4], T)], [_np(x) for x in NM.relative_pose(*head, T)])
    _same([_np(x) for x in NM.batch_relative_pose(mr, head[3], head[4], T, refine=True)], [_np(x) for x in NM.relative_pose(*head, T, refine=True)])


def test_metric_class_returns_the_refined_triple():
    s = C.scene("ransac_255")
    m0, m1 = MM.RelativePoseEstimation("RPE", (5, 10, 20)), MM.RelativePoseEstimation("RPE", (5, 10, 20), refine=True)
    kp0, kp1 = _t(s["kp0"]), _t(s["kp1"])
    plain = m0.estimate_pose(kp0, kp1, s["K0"], s["K1"], 1.0, 0.999)
    got = m1.estimate_pose(kp0, kp1, s["K0"], s["K1"], 1.0, 0.999)
    n = len(s["kp0"])
    mk0, mk1 = _t(s["kp0"][None]), _t(s["kp1"][None])
    nm, K0, K1 = _t(np.array([n], np.int32)), _t(s["K0"][None]), _t(s["K1"][None])
    want = NM.relative_pose(mk0, mk1, nm, K0, K1, refine=True)
    assert np.array_equal(got[0], _np(want[0])[0]) and np.array_equal(got[1], _np(want[1])[0]) and np.array_equal(got[2], _np(want[2])[0, :n])
    assert not np.array_equal(got[0], plain[0]) and got[2].sum() >= plain[2].sum()
    out = m1.update_one(kp0, kp1, s["K0"], s["K1"], s["T"])
    t_err, R_err = m1.relative_pose_error(s["T"], got[0], got[1])  # the class's own arithmetic on the float32 T
    assert out["RPE_inliers"] == got[2].mean() and out["RPE_pose_errs"] == max(R_err, t_err)
    assert abs(out["RPE_pose_errs"] - P.pose_errors(s["T"], got[0], got[1])[2]) <= 1e-4


def test_evaluator_keys():
    H, W, B, BINS = 260, 346, 2, 5
    model = pkg.EIM(pkg.default_config("SP_MNN", event_channels=BINS), device=DEV).eval()
    sdn = synth.synth_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], seed=31)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sdn.items()}, strict=False)
    K = _t(np.tile(np.array([[256.0, 0, W / 2], [0, 256.0, H / 2], [0, 0, 1]], np.float32), (B, 1, 1)))
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    T[:, 0, 3] = 1.0 / 8
    pose = (K, K, _t(T))
    plain = pkg.DifferentTimeEvaluator(model, bins=BINS, resolution=(W, H))
    off = pkg.DifferentTimeEvaluator(model, bins=BINS, resolution=(W, H), pose_refine=False)
    fine = pkg.DifferentTimeEvaluator(model, bins=BINS, resolution=(W, H), pose_refine=True)
    streamed = pkg.DifferentTimeEvaluator(model, bins=BINS, resolution=(W, H), pose_refine=True)
    rows, kept, items = [], [], []
    for step in range(2):
        evs = [synth_raw_events(dict(seed=830 + 2 * step + b, n=20000, H=H, W=W, bins=BINS, frac=False, pneg=False)) for b in range(B)]
        img = synth.synth_image(96 + step, B, H, W)
        items.append((evs, _t(img), None, pose))
        r0, _ = plain.step(evs, _t(img), None, pose=pose)
        off.step(evs, _t(img), None, pose=pose)
        r1, (ef, _, _) = fine.step(evs, _t(img), None, pose=pose)
        assert _np(r0).tobytes() == _np(r1).tobytes()  # the returned metric rows are unchanged
        mr = model._last_match
        first = NM.batch_relative_pose(mr, K, K, pose[2], ordering=ef._batched.ordering)
        by_hand = NM.refine_relative_pose(mr.mk0, mr.mk1, mr.nmatch, K, K, *first[:4], pose[2], ordering=ef._batched.ordering)
        rows.append(by_hand[4])
        kept.append(by_hand[3][:, :1].to(torch.float64))
        assert torch.equal(torch.nan_to_num(fine._pose_rows[-1], nan=-7.0), torch.nan_to_num(by_hand[4], nan=-7.0))
    list(streamed.run(items, depth=2))
    same = lambda a, b: a == b or (a != a and b != b)  # noqa: E731
    a, o, b, c = plain.result(), off.result(), fine.result(), streamed.result()
    assert list(o) == list(a) and all(same(a[k], o[k]) for k in a) and not off._pose_kept  # the default: today's keys and values
    assert list(b) == list(a) + ["RPE_refined_ratio"] and list(c) == list(b) and all(same(b[k], c[k]) for k in b)
    H_ = import_module(pkg.__name__ + ".harness")
    want = H_.rpe_summary(torch.cat(rows, 0), fine.pose_thresh)
    want.update(H_.refined_summary(torch.cat(kept, 0)))
    assert all(same(b[k], want[k]) for k in want) and set(want) <= set(b)
    assert all(same(a[k], b[k]) for k in a if not k.startswith("RPE"))

"""Contribution scores on the GPU (SPEC M11; include/msgs.h msgs_contrib_*): per Gaussian, over the pixels p of a
view with an optional weight map m_p, weight_sum = sum_p m_p w_ip, weight_max = max_p m_p w_ip and pixel_count = the number of
counted pixels, with w_ip = alpha_ip T_ip the blend weight (the weight of dL/dC in the colour gradient).

Two truths, both independent of the kernel under test:
  A  float64, from oracle/torch_oracle.py alone: tests/golden/contrib_truth.npz (scene F; generator and the CPU test that pins
     it: tests/golden/make_contrib_golden.py, tests/test_contrib_cpu.py).  The weight maps are zero on the pixels the oracle flags
     as borderline, on both sides.
  B  the op's own decomposition: one backward of a plain render per pixel with dL/dC = e_0 at that pixel; colors_precomp.grad[:, 0]
     is then w_ip of that pixel.  One whole-image backward with dL/dC = (m, 0, 0) must reproduce the weighted weight_sum.
Counts are compared exactly, sums and maxima with parity_utils.rel_err against BWD_RTOL, the project's gradient tolerance; the
measured maxima are printed (pytest -s) and recorded in profiles/contrib_notes.md.  Then: the invariants, accumulation over views,
equal bits on every run and behind every forward route, the untouched default path, the host layer and the guards.
The float64 truth here lives on one 3 x 2-tile picture; for the breadth (lists of several 256-entry batches, early termination,
filters with a fade, rigid poses, focal lengths, the scaling modifier, small models) see the seeded sweep of all opt-in outputs
against the same kind of truth: tests/test_replay_sweep_gpu.py, tests/replay_cases.py, tests/replay_truth.py."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import diff_gaussian_rasterization as dgr
import scenes
from parity_utils import BWD_RTOL, PIPE, rel_err, report, small_scene
from route_utils import PLAIN, assert_identical, reset_forward_state, result, slab_stats
from synthetic_model import SyntheticGaussians
from test_absgrad_gpu import BG, _env, _scene_b, _scene_f, _set_route
from test_depth_grad_gpu import ROUTES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _reset_routes():
    yield
    dgr._C.lib.msgs_set_backward_generation(0)
    dgr._C.lib.msgs_set_blend_granularity(0)


def _rasterizer(cam, pc, st=PLAIN):
    from gaussian_renderer import _settings
    return dgr.GaussianRasterizer(_settings(cam.to("cuda"), pc, PIPE, torch.tensor(BG).cuda(), 1.0, st["filter_small"],
                                            st["filter_large"], st["fade_size"]))


def _contrib(sc, cam, pixel_weights=None, into=None, pc=None, st=PLAIN):
    """GaussianRasterizer.contributions on the inputs render() hands to the op for this model"""
    pc = pc if pc is not None else SyntheticGaussians(sc, "cuda", requires_grad=False)
    s = _rasterizer(cam, pc, st).contributions(
        pc.get_xyz, pc.get_opacity, scales=pc.get_scaling, rotations=pc.get_rotation, max_pixel_sizes=pc.get_max_pixel_sizes,
        min_pixel_sizes=pc.get_min_pixel_sizes, base_mask=pc.get_base_mask, pixel_weights=pixel_weights, into=into)
    torch.cuda.synchronize()
    return s


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _weight_map(W, H, seed):
    """[H,W] float32 on the GPU: a quarter of the pixels 0, the others uniform in (0.25, 2.25)"""
    g = torch.Generator().manual_seed(seed)
    m = 0.25 + 2.0 * torch.rand(H, W, generator=g)
    return torch.where(torch.rand(H, W, generator=g) < 0.25, torch.zeros(H, W), m).cuda()


def _check_types(s, P):
    assert isinstance(s, dgr.ContributionScores)
    assert s.weight_sum.shape == s.weight_max.shape == s.pixel_count.shape == (P,)
    assert s.weight_sum.dtype == s.weight_max.dtype == torch.float32 and s.pixel_count.dtype == torch.int64
    assert s.weight_sum.is_cuda and s.weight_max.is_cuda and s.pixel_count.is_cuda


# ---------------------------------------------------------------------------------------------------------------------------
# 1. truth A: float64, independent of the op
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def truth_a():
    t = np.load(os.path.join(ROOT, "tests", "golden", "contrib_truth.npz"))
    assert t["borderline"].sum() <= 0.02 * t["borderline"].size         # the condition of the masking (scene F: 1 of 960)
    return {k: torch.from_numpy(t[k]) for k in t.files}


@pytest.mark.parametrize("route", list(ROUTES))
def test_scores_against_float64_truth(truth_a, route):
    from gaussian_renderer import render
    sc, cam, bg, _ = _scene_f()
    _set_route(route)
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    with torch.no_grad():
        radii = render(cam.to("cuda"), pc, PIPE, bg.cuda(), **PLAIN)["radii"]
    assert torch.equal((radii > 0).cpu(), truth_a["visible"])
    for name in ("plain", "weighted"):           # "plain": 1 everywhere but on the borderline pixels, handed over as a weight map
        s = _contrib(sc, cam, pixel_weights=truth_a["m_" + name].cuda(), pc=pc)
        _check_types(s, 200)
        assert torch.equal(s.pixel_count.cpu(), truth_a["count_" + name]), name
        for key, got in (("sum", s.weight_sum), ("max", s.weight_max)):
            e = rel_err(got, truth_a[f"{key}_{name}"])
            report(f"contrib truth A [{route}, {name}]", f"weight_{key} rel err", e)
            assert e <= BWD_RTOL, (name, key)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. truth B: the op's own per-pixel decomposition
# ---------------------------------------------------------------------------------------------------------------------------
def _per_pixel_truth(sc, cam, m):
    """(sum_p w, max_p w, #{w > 0}) per Gaussian in float64 from one backward per pixel of ONE plain render with colour leaves,
    the gradient of a whole-image backward with dL/dC = (m, 0, 0), the model"""
    from gaussian_renderer import render
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    P = pc.get_xyz.shape[0]
    col = torch.rand(P, 3, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_(True)
    out = render(cam.to("cuda"), pc, PIPE, torch.tensor(BG).cuda(), override_color=col, **PLAIN)
    img = out["render"]
    H, W = img.shape[1:]
    one = torch.zeros_like(img)
    tot = torch.zeros(P, dtype=torch.float64, device="cuda")
    mx = torch.zeros_like(tot)
    cnt = torch.zeros(P, dtype=torch.int64, device="cuda")
    for y in range(H):
        for x in range(W):
            one[0, y, x] = 1.0
            g, = torch.autograd.grad(img, [col], one, retain_graph=True)
            w = g[:, 0].double()
            tot += w
            mx = torch.maximum(mx, w)
            cnt += w > 0
            one[0, y, x] = 0.0
    seed = torch.zeros_like(img)
    seed[0] = m
    full, = torch.autograd.grad(img, [col], seed)
    torch.cuda.synchronize()
    return tot, mx, cnt, full[:, 0].double(), pc, out["radii"]


@pytest.mark.parametrize("kind", ["F", "deep", "opaque", "sparse"])
def test_scores_against_per_pixel_backwards(kind):
    sc, cam = _scene_b(kind)[:2]
    W, H = cam.image_width, cam.image_height
    m = _weight_map(W, H, 83)
    tot, mx, cnt, full, pc, radii = _per_pixel_truth(sc, cam, m)
    assert cnt.sum().item() > 0
    s = _contrib(sc, cam, pc=pc)
    _check_types(s, tot.shape[0])
    assert torch.equal(s.pixel_count, cnt)
    for key, got, ref in (("sum", s.weight_sum, tot), ("max", s.weight_max, mx)):
        e = rel_err(got, ref)
        report(f"contrib truth B [{kind}]", f"weight_{key} rel err", e)
        assert e <= BWD_RTOL, key
    assert torch.equal(s.pixel_count[radii == 0], torch.zeros_like(s.pixel_count[radii == 0]))
    # one whole-image backward with dL/dC = (m, 0, 0): the colour gradient IS the weighted sum.  Both sides add at most 256
    # positive float32 terms per tile in some order (relative error <= 256 * 2^-24 whatever the order), then exact double
    # adds, then one rounding to float32 each (2^-24 each)
    sw = _contrib(sc, cam, pixel_weights=m, pc=pc)
    assert full.max().item() > 0
    err = ((sw.weight_sum.double() - full).abs() / full.clamp_min(1e-300)).where(full > 0, (sw.weight_sum != 0).double())
    report(f"contrib truth B [{kind}]", "weighted weight_sum vs the colour gradient of dL = (m, 0, 0), worst row rel err",
           err.max().item())
    assert err.max().item() <= 256 * 2.0 ** -24 + 2.0 ** -23
    assert (sw.pixel_count <= s.pixel_count).all() and sw.pixel_count.sum().item() < s.pixel_count.sum().item()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. invariants
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["F", "opaque"])
def test_invariants(kind):
    from gaussian_renderer import render_with_alpha
    sc, cam = _scene_b(kind)[:2]
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    with torch.no_grad():
        out = render_with_alpha(cam.to("cuda"), pc, PIPE, torch.tensor(BG).cuda(), **PLAIN)
    s = _contrib(sc, cam, pc=pc)
    ws, wm, n = s
    seen = n > 0
    assert n.sum().item() > 0 and (n >= 0).all()
    assert torch.equal(seen, ws != 0) and torch.equal(seen, wm != 0)                       # zero together
    assert torch.isfinite(ws).all() and torch.isfinite(wm).all()
    report(f"contrib invariants [{kind}]", "largest weight_max", wm.max().item())
    assert (wm[seen] > 0).all() and (wm[seen] <= 0.99).all()
    assert (wm <= ws).all()
    assert (ws.double() <= n.double() * wm.double() * (1 + 2.0 ** -20)).all()
    gone = out["radii"] == 0
    assert not seen[gone].any()
    a = out["alpha"].double().sum().item()
    e = abs(ws.double().sum().item() - a) / a
    report(f"contrib invariants [{kind}]", "|sum_i weight_sum - sum_p alpha| / sum_p alpha", e)
    assert e <= BWD_RTOL


# ---------------------------------------------------------------------------------------------------------------------------
# 4. accumulation over views
# ---------------------------------------------------------------------------------------------------------------------------
def _ball(P=6000, W=104, H=72, V=3):
    sc = scenes.ball_scene(P, seed=12, log_s=-2.3)
    sc.opacities[::20] = 1e-4                 # below 1/255: in the lists of their tiles, never blended
    return sc, [scenes.ring_camera(v, 8, W, H) for v in range(V)]


def test_two_views_in_one_accumulator():
    sc, cams = _ball()
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    P = pc.get_xyz.shape[0]
    a, b = _contrib(sc, cams[0], pc=pc), _contrib(sc, cams[1], pc=pc)
    assert a.pixel_count.sum().item() > 0 and b.pixel_count.sum().item() > 0 and not torch.equal(a.pixel_count, b.pixel_count)
    acc = dgr.ContributionAccumulator(P, "cuda")
    assert _equal(acc.scores(), [torch.zeros_like(t) for t in a])                   # before the first view: zeros
    assert _contrib(sc, cams[0], into=acc, pc=pc) is None and _contrib(sc, cams[1], into=acc, pc=pc) is None
    assert acc.views == 2
    s = acc.scores()
    torch.cuda.synchronize()
    assert torch.equal(s.pixel_count, a.pixel_count + b.pixel_count)
    assert torch.equal(s.weight_max, torch.maximum(a.weight_max, b.weight_max))
    want = a.weight_sum.double() + b.weight_sum.double()
    assert ((s.weight_sum.double() - want).abs() <= 2.0 ** -23 * want).all()
    # reset(): the next view starts over
    acc.reset()
    _contrib(sc, cams[1], into=acc, pc=pc)
    assert _equal(acc.scores(), b)


def test_the_same_view_twice_and_clear_first():
    sc, cam = _scene_f()[:2]
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    one = _contrib(sc, cam, pc=pc)
    acc = dgr.ContributionAccumulator(200, "cuda")
    acc.buf.fill_(0xA5)                                   # clear_first really clears
    _contrib(sc, cam, into=acc, pc=pc)
    assert _equal(acc.scores(), one)
    _contrib(sc, cam, into=acc, pc=pc)
    two = acc.scores()
    torch.cuda.synchronize()
    assert torch.equal(two.pixel_count, 2 * one.pixel_count) and torch.equal(two.weight_max, one.weight_max)
    assert torch.equal(two.weight_sum, 2 * one.weight_sum)                          # doubling is exact


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the same bits on every run and behind every forward route
# ---------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_equal_bits():
    sc, cam = small_scene(3000, 150, 90, seed=11)
    m = _weight_map(150, 90, 84)
    for pw in (None, m):
        a, b = _contrib(sc, cam, pixel_weights=pw), _contrib(sc, cam, pixel_weights=pw)
        assert a.pixel_count.sum().item() > 0 and _equal(a, b)


def _compare_routes(what, got, a, b):
    assert got[a].pixel_count.sum().item() > 0
    assert torch.equal(got[a].pixel_count, got[b].pixel_count)
    for key in ("weight_sum", "weight_max"):
        e = rel_err(getattr(got[a], key), getattr(got[b], key))
        report(what, f"{key} rel err", e)
        assert e <= BWD_RTOL
    report(what, "equal bits (1 = yes)", float(_equal(got[a], got[b])))


def test_scores_behind_a_slab_forward():
    from test_slab_gpu import _dense_scene
    W, H = 960, 720
    sc, cam = _dense_scene(80_000, W, H, 9, opacity=(0.5, 0.99)), scenes.front_camera(W, H)
    got, seen = {}, []
    prev, dgr._contrib_probe = dgr._contrib_probe, lambda call, state: seen.append(types.SimpleNamespace(call=call, state=state))
    try:
        for policy in ("never", "0.12"):
            with _env(slab=policy):
                got[policy] = _contrib(sc, cam)
                assert slab_stats(seen[-1])["active"] == (policy != "never")
    finally:
        dgr._contrib_probe = prev
    _compare_routes("contrib slab 0.12 vs never", got, "0.12", "never")


def test_scores_behind_the_occlusion_cut_off():
    from test_occlusion_gpu import _giants_scene
    W, H = 420, 300
    sc, cam = _giants_scene(2500, W, H, 5, 60, giant_scale=1.2, giant_opacity=0.9), scenes.front_camera(W, H)
    got = {}
    for occ in (0, 1):
        with _env(occlusion=occ):
            got[occ] = _contrib(sc, cam)
    _compare_routes("contrib occlusion cut-off on vs off", got, 1, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the default path untouched
# ---------------------------------------------------------------------------------------------------------------------------
def test_a_call_between_forward_and_backward_changes_nothing():
    from gaussian_renderer import render
    W, H = 150, 90
    sc, cam = small_scene(3000, W, H, seed=11)
    cam, bg, dL = cam.to("cuda"), torch.tensor(BG).cuda(), scenes.grad_seed(W, H, 78).cuda()

    def sequence(with_call):
        """two render + backward rounds of the same view, the first with contributions() in between -> (results, routes)"""
        reset_forward_state()
        before = dict(dgr.forward_stats)
        res = []
        for it in range(2):
            pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
            out = render(cam, pc, PIPE, bg, **PLAIN)
            if with_call and it == 0:
                s = _contrib(sc, cam, pc=pc, pixel_weights=_weight_map(W, H, 85))
                assert s.pixel_count.sum().item() > 0
            out["render"].backward(dL)
            torch.cuda.synchronize()
            res.append(result(out, pc, out["render"].grad_fn, W, H))
        delta = {k: dgr.forward_stats[k] - before[k] for k in before}
        return res, delta, dict(dgr._last_instances), dict(dgr._instances_by_view)

    plain, d0, g0, v0 = sequence(False)
    mixed, d1, g1, v1 = sequence(True)
    assert_identical(plain[0], mixed[0], "contributions() between forward and backward")
    assert_identical(plain[1], mixed[1], "the render after a contributions() call")
    assert d1["forwards"] == d0["forwards"] + 1 and d1["non_speculative"] == d0["non_speculative"]     # its own forward, no redo
    assert g0 == g1 and v0 == v1                                                    # the instance guesses of the next forward


# ---------------------------------------------------------------------------------------------------------------------------
# 7. the host layer
# ---------------------------------------------------------------------------------------------------------------------------
def test_contribution_scores_over_cameras():
    from contribution import contribution_scores
    sc, cams = _ball()
    cams = [c.to("cuda") for c in cams]
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    bg = torch.tensor(BG).cuda()
    maps = [_weight_map(104, 72, 90 + v) if v != 1 else None for v in range(3)]
    calls = []

    def pixel_weights(i, cam):
        calls.append((i, cam))
        return maps[i]
    for pw, ms in ((None, [None] * 3), (pixel_weights, maps)):
        s = contribution_scores(cams, pc, PIPE, bg, pixel_weights=pw, **PLAIN)
        per = [_contrib(sc, c, pixel_weights=m, pc=pc) for c, m in zip(cams, ms)]
        assert torch.equal(s.pixel_count, per[0].pixel_count + per[1].pixel_count + per[2].pixel_count)
        assert torch.equal(s.weight_max, torch.maximum(torch.maximum(per[0].weight_max, per[1].weight_max), per[2].weight_max))
        want = sum(p.weight_sum.double() for p in per)
        assert ((s.weight_sum.double() - want).abs() <= 2 * 2.0 ** -23 * want).all()
        assert s.pixel_count.sum().item() > 0
    assert [c[0] for c in calls] == [0, 1, 2] and all(c[1] is cams[c[0]] for c in calls)


def test_prune_by_contribution_removes_rows_and_moments():
    from contribution import contribution_scores, prune_by_contribution
    from densify import prune_points
    from train_epilogue import FusedAdam
    sc, cams = _ball()
    cams = [c.to("cuda") for c in cams]
    bg = torch.tensor(BG).cuda()
    models, opts = [], []
    for _ in range(2):
        m = SyntheticGaussians(sc, "cuda")
        o = FusedAdam(m.training_setup(4), lr=0.0, eps=1e-15)
        g = torch.Generator().manual_seed(6)
        for n in m.LEAVES:
            p = getattr(m, n)
            o.state[p] = {"step": torch.tensor(7.0), "exp_avg": torch.randn(p.shape, generator=g).cuda(),
                          "exp_avg_sq": torch.rand(p.shape, generator=g).cuda()}
        models.append(m), opts.append(o)
    a, b = models
    P = a._xyz.shape[0]
    s = contribution_scores(cams, a, PIPE, bg, **PLAIN)
    never = (s.pixel_count == 0).cpu().numpy()
    n_remove = int(np.floor(0.25 * P))
    assert 0 < never.sum() < n_remove                     # never-seen Gaussians exist, and the cut reaches into the seen ones
    want = np.zeros(P, bool)
    want[np.argsort(s.weight_sum.cpu().numpy(), kind="stable")[:n_remove]] = True
    assert want[never].all()                              # never-seen Gaussians leave first
    mask = prune_by_contribution(a, s, optimizer=opts[0], fraction=0.25)
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), want)
    prune_points(b, torch.from_numpy(want).cuda(), optimizer=opts[1])
    torch.cuda.synchronize()
    assert a._xyz.shape[0] == P - n_remove
    for n in a.LEAVES:
        pa, pb = getattr(a, n), getattr(b, n)
        assert torch.equal(pa, pb), n
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opts[0].state[pa][k], opts[1].state[pb][k]), (n, k)
        assert opts[0].state[pa]["step"].item() == 7.0
    for k in ("xyz_gradient_accum", "denom", "max_radii2D", "max_pixel_sizes", "min_pixel_sizes", "base_gaussian_mask",
              "target_reso_lvl"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    keep = torch.from_numpy(~want).cuda()
    assert torch.equal(a._xyz.detach(), SyntheticGaussians(sc, "cuda")._xyz.detach()[keep])


# ---------------------------------------------------------------------------------------------------------------------------
# 8. guards
# ---------------------------------------------------------------------------------------------------------------------------
def test_verification_mode_refuses_before_any_launch():
    from contribution import contribution_scores
    sc, cam = _scene_f()[:2]
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    before = dgr.forward_stats["forwards"]
    prev = dgr.set_deterministic(True)
    try:
        with pytest.raises(ValueError, match="verification mode"):
            _contrib(sc, cam, pc=pc)
        with pytest.raises(ValueError, match="verification mode"):
            dgr.ContributionAccumulator(200, "cuda")
        with pytest.raises(ValueError, match="verification mode"):
            contribution_scores([cam.to("cuda")], pc, PIPE, torch.tensor(BG).cuda(), **PLAIN)
    finally:
        dgr.set_deterministic(prev)
    assert dgr.forward_stats["forwards"] == before


def test_no_gaussians_gives_empty_scores():
    rs = dgr.GaussianRasterizationSettings(24, 40, 0.5, 0.3, torch.tensor(BG).cuda(), 1.0, torch.eye(4).cuda(), torch.eye(4).cuda(),
                                           3, torch.zeros(3).cuda(), False, False)
    z = lambda *s: torch.zeros(*s, device="cuda")
    before = dgr.forward_stats["forwards"]
    s = dgr.GaussianRasterizer(rs).contributions(z(0, 3), z(0, 1), shs=z(0, 16, 3), scales=z(0, 3), rotations=z(0, 4),
                                                 pixel_weights=z(24, 40))
    _check_types(s, 0)
    acc = dgr.ContributionAccumulator(0, "cuda")
    assert dgr.GaussianRasterizer(rs).contributions(z(0, 3), z(0, 1), scales=z(0, 3), rotations=z(0, 4), into=acc) is None
    _check_types(acc.scores(), 0)
    assert dgr.forward_stats["forwards"] == before


def test_pixel_weights_and_accumulator_are_checked():
    sc, cam = _scene_f()[:2]
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    before = dgr.forward_stats["forwards"]
    ok = torch.ones(24, 40, device="cuda")
    for bad in (ok.double(), ok.half(), torch.ones(40, 24, device="cuda"), ok[None], ok[:, :39], ok.cpu(), ok.cpu().numpy()):
        with pytest.raises(ValueError, match="pixel_weights"):
            _contrib(sc, cam, pc=pc, pixel_weights=bad)
    for bad in (dgr.ContributionAccumulator(199, "cuda"), dgr.ContributionAccumulator(0, "cpu"), object()):
        with pytest.raises(ValueError, match="ContributionAccumulator"):
            _contrib(sc, cam, pc=pc, into=bad)
    assert dgr.forward_stats["forwards"] == before
    # a non-contiguous map of the right shape is taken (copied)
    t = torch.ones(40, 24, device="cuda").t()
    assert not t.is_contiguous() and _equal(_contrib(sc, cam, pc=pc, pixel_weights=t), _contrib(sc, cam, pc=pc, pixel_weights=ok))
    assert _equal(_contrib(sc, cam, pc=pc, pixel_weights=ok), _contrib(sc, cam, pc=pc))          # ones = no map


def test_negative_and_nan_weights_count_as_zero():
    sc, cam = _scene_f()[:2]
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    m = _weight_map(40, 24, 86)
    g = torch.Generator().manual_seed(7)
    pick = torch.rand(24, 40, generator=g).cuda()
    dirty = torch.where(pick < 0.1, torch.full_like(m, float("nan")), m)
    dirty = torch.where((pick >= 0.1) & (pick < 0.2), -m - 0.5, dirty)
    dirty = torch.where((pick >= 0.2) & (pick < 0.25), torch.full_like(m, -0.0), dirty)
    dirty = torch.where((pick >= 0.25) & (pick < 0.3), torch.full_like(m, float("-inf")), dirty)
    clean = torch.where(pick < 0.3, torch.zeros_like(m), m)
    assert torch.isnan(dirty).any() and (dirty < 0).any()
    a, b = _contrib(sc, cam, pc=pc, pixel_weights=dirty), _contrib(sc, cam, pc=pc, pixel_weights=clean)
    assert a.pixel_count.sum().item() > 0 and _equal(a, b)
    assert torch.isfinite(a.weight_sum).all() and torch.isfinite(a.weight_max).all()
    none = _contrib(sc, cam, pc=pc, pixel_weights=torch.zeros(24, 40, device="cuda"))
    assert not none.pixel_count.any() and not none.weight_sum.any() and not none.weight_max.any()


def test_c_entries_check_capacity_and_arguments():
    from gaussian_renderer import render
    sc, cam, bg, _ = _scene_f()
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    out = render(cam.to("cuda"), pc, PIPE, bg.cuda(), **PLAIN)
    ctx = out["render"].grad_fn
    geom, binning, image, D = dgr._resolve(ctx.state)
    lib, call, P = dgr._C.lib, ctx.call, ctx.call.P
    need = lib.msgs_contrib_scratch_bytes(P)
    GUARD = 256
    # guard words around the accumulator and the three outputs
    accbuf = torch.full((need + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    outs = [torch.full((P + 2 * GUARD,), v, dtype=dt, device="cuda") for v, dt in ((7.0, torch.float32), (7.0, torch.float32),
                                                                                     (7, torch.int64))]
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    acc_p = p(accbuf, GUARD)

    def accumulate(image_bytes=image.numel(), acc_bytes=need, acc=acc_p, n=P, g=p(geom), geom_bytes=geom.numel(), d=D,
                   binning_bytes=binning.numel(), view=call.view_ref, im=p(image)):
        return lib.msgs_contrib_accumulate(view, n, g, geom_bytes, d, p(binning), binning_bytes, im, image_bytes, None, acc,
                                           acc_bytes, 1, stream)

    def finish(acc=acc_p, acc_bytes=need, n=P, ws=p(outs[0], 4 * GUARD), wm=p(outs[1], 4 * GUARD), pcnt=p(outs[2], 8 * GUARD)):
        return lib.msgs_contrib_finish(n, acc, acc_bytes, ws, wm, pcnt, stream)
    assert accumulate(acc_bytes=need - 1) == -2                   # MSGS_ERR_CAPACITY
    assert accumulate(image_bytes=lib.msgs_image_bytes(40, 24) - 1) == -2
    assert accumulate(geom_bytes=lib.msgs_geom_bytes(P) - 1) == -2
    assert accumulate(binning_bytes=lib.msgs_binning_bytes(D, 40, 24) - 1) == -2
    assert accumulate(acc=None) == -1                             # MSGS_ERR_INVALID_ARG
    assert accumulate(acc=p(accbuf, GUARD + 4)) == -1
    assert accumulate(g=None) == -1 and accumulate(im=None) == -1 and accumulate(view=None) == -1
    assert accumulate(n=-1) == -1 and accumulate(d=-1) == -1
    assert finish(acc_bytes=need - 1) == -2
    assert finish(acc=None) == -1 and finish(ws=None) == -1 and finish(wm=None) == -1 and finish(pcnt=None) == -1
    assert finish(n=-1) == -1
    torch.cuda.synchronize()
    assert (accbuf == 0x5A).all()                                 # refused calls wrote nothing
    for t, v in zip(outs, (7.0, 7.0, 7)):
        assert (t == v).all()
    # no instance: only the clear runs (no geom / binning / image needed)
    assert lib.msgs_contrib_accumulate(call.view_ref, P, None, 0, 0, None, 0, None, 0, None, acc_p, need, 1, stream) == 0
    torch.cuda.synchronize()
    assert (accbuf[:GUARD] == 0x5A).all() and (accbuf[GUARD + need:] == 0x5A).all() and not accbuf[GUARD:GUARD + need].any()
    assert accumulate() == 0 and finish() == 0
    torch.cuda.synchronize()
    assert (accbuf[:GUARD] == 0x5A).all() and (accbuf[GUARD + need:] == 0x5A).all()
    for t, v in zip(outs, (7.0, 7.0, 7)):
        assert (t[:GUARD] == v).all() and (t[GUARD + P:] == v).all()
    # the entries are independent of the backward calls, and they are what the wrapper calls
    ref = _contrib(sc, cam, pc=pc)
    assert _equal([t[GUARD:GUARD + P] for t in outs], ref)

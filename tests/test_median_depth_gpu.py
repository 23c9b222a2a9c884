"""Median depth and Gaussian id on the GPU (SPEC M15; 4.15): GaussianRasterizer.with_median_depth().

Two independent truths:
  1  float64: tests/golden/median_depth_truth.npz (oracle/torch_oracle.preprocess + the blend loop restated by
     tests/replay_truth.pixel_weights + the definition, autograd of sum G * median_depth for means3D and a viewmatrix leaf) on
     scene F (every pixel crosses 1/2) and "thin" (empty, crossing and never-crossing pixels).  G is zero on the fixture's mask
     (the oracle's borderline pixels and pixels with a blended T_{i+1} within 1e-4 of 0.5), which is also left out of the map
     comparisons; the mask covers <= 2 % of the image (asserted).
  2  the op's own per-pixel decomposition: one backward of a plain render per pixel with dL/dC = e_0 gives w_ip; in float64
     T_i = 1 - sum_{j<i} w_j in list order gives m(p).  A pixel whose crossing has |T - 0.5| < 1e-4 may report either entry at
     the sides of the crossing; such pixels are <= 5 % on "deep" and <= 2 % elsewhere (asserted).
Tolerances are the project's own for quantities of the same kind (FWD_ATOL, BWD_RTOL of tests/parity_utils.py, LIN_TOL of
tests/test_depth_grad_gpu.py, CEIL of tests/test_camera_grad_gpu.py); ids are compared exactly.  The measured maxima are printed
(pytest -s) and recorded in profiles/median_depth_notes.md.  The forward-route section runs the scenes of the route tests of
tests/test_distortion_gpu.py (the smallest that reach a redo, forced slabs and closed occlusion blocks), forward only.
The float64 truth here lives on one 3 x 2-tile picture; for the breadth (lists of several 256-entry batches, early termination,
filters with a fade, rigid poses, focal lengths, the scaling modifier, small models) see the seeded sweep of all opt-in outputs
against the same kind of truth: tests/test_replay_sweep_gpu.py, tests/replay_cases.py, tests/replay_truth.py."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

import diff_gaussian_rasterization as dgr
import scenes
from parity_utils import BWD_RTOL, FWD_ATOL, PIPE, check_backward, report, small_scene
from route_utils import PLAIN, guesses_around, non_speculative, reset_forward_state, slab_stats
from synthetic_model import SyntheticGaussians
from test_absgrad_gpu import _scene_b, _scene_f
from test_camera_grad_gpu import CEIL as CAMERA_CEIL
from test_depth_grad_gpu import LIN_TOL, ROUTES, _view_z
from test_features_gpu import GRADS, _env, _equal_grads, _features, _grads, _rel, _seed_map, _set_route

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT5 = ("render", "acc_pixel_size", "depth", "radii", "pixel_sizes")
NEAR = 1e-4                  # |T - 0.5| at the crossing below which either neighbouring entry is accepted (truth 2)


@pytest.fixture(autouse=True)
def _reset_routes():
    yield
    dgr._C.lib.msgs_set_backward_generation(0)
    dgr._C.lib.msgs_set_blend_granularity(0)


def _generator():
    spec = importlib.util.spec_from_file_location("make_median_depth_golden", os.path.join(ROOT, "tests", "golden",
                                                                                           "make_median_depth_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _seed(h, w, seed=151):
    """G = dL/dmedian_depth [h,w] float32 on the GPU, seeded, uniform in (-0.5, 0.5)"""
    return (torch.rand(h, w, generator=torch.Generator().manual_seed(seed)) - 0.5).cuda()


def _rasterizer(cam, pc, bg, st=PLAIN, median=True, distortion=False, features=None, alpha=False, smod=1.0, pipe=PIPE):
    from gaussian_renderer import _settings
    st = {**PLAIN, **st}
    settings = _settings(cam, pc, pipe, bg, smod, st["filter_small"], st["filter_large"], st["fade_size"])
    return dgr.GaussianRasterizer(settings, return_alpha=alpha).with_features(features).with_distortion(distortion) \
        .with_median_depth(median)


def _render(cam, pc, bg, st=PLAIN, median=True, distortion=False, features=None, alpha=False, fused=False, smod=1.0, pipe=PIPE,
            rasterizer=None):
    """render() / render_fused() of the host layer with any of the opt-in outputs: the result dict plus "alpha" / "distortion" /
    "median_depth", "median_id" / "features" """
    from gaussian_renderer import RESULT_KEYS, _colour_inputs, _shape_inputs
    r = rasterizer or _rasterizer(cam, pc, bg, st, median, distortion, features, alpha, smod, pipe)
    kw = dict(max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes,
              occ_multiplier=pc.get_occ_multiplier, dc_delta=pc.get_dc_delta, base_mask=pc.get_base_mask)
    if fused:
        vs = torch.empty_like(pc._xyz, requires_grad=True)
        outs = r.forward_raw(pc._xyz, vs, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation, **kw)
    else:
        vs = torch.zeros_like(pc.get_xyz, requires_grad=True) + 0
        if vs.requires_grad:
            vs.retain_grad()
        outs = r(means3D=pc.get_xyz, means2D=vs, opacities=pc.get_opacity, **kw, **_colour_inputs(cam, pc, pipe, None),
                 **_shape_inputs(pc, pipe, smod))
    out = dict(zip(RESULT_KEYS, (*outs[:3], vs, outs[3] > 0, outs[3], outs[4])))
    rest = list(outs[5:])
    if r.return_alpha:
        out["alpha"] = rest.pop(0)
    if r.return_distortion:
        out["distortion"] = rest.pop(0)
    if r.return_median_depth:
        out["median_depth"], out["median_id"] = rest.pop(0), rest.pop(0)
    if r.features is not None:
        out["features"] = rest.pop(0)
    assert not rest
    return out


SEED_KEYS = (("dL", "render"), ("Gd", "depth"), ("Ga", "alpha"), ("Gx", "distortion"), ("Gm", "median_depth"), ("G", "features"))


def _loss(out, seeds):
    loss = 0.0
    for name, key in SEED_KEYS:
        if seeds.get(name) is not None:
            loss = loss + (out[key] * seeds[name]).sum()
    return loss


def _run(sc, cam, st=PLAIN, feats=None, fused=False, bg=None, median=True, **seeds):
    """one forward + backward on fresh leaves; the loss is the sum of the given seeds (dL, Gd, Ga, Gx, Gm, G) times their maps.
    Returns (out, {name: grad})"""
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    f = feats.detach().cuda().clone().requires_grad_(True) if feats is not None else None
    bg = torch.zeros(3, device="cuda") if bg is None else bg.cuda()
    out = _render(cam.to("cuda"), pc, bg, st, median, seeds.get("Gx") is not None, f, seeds.get("Ga") is not None, fused)
    _loss(out, seeds).backward()
    torch.cuda.synchronize()
    _run.last_pc = pc
    return out, _grads(pc, out)


def _maps(out):
    return out["median_depth"].detach(), out["median_id"]


def _check_maps(out, h, w):
    d, i = out["median_depth"], out["median_id"]
    assert d.shape == (h, w) and d.dtype == torch.float32 and i.shape == (h, w) and i.dtype == torch.int32
    assert not i.requires_grad and i.grad_fn is None


# ---------------------------------------------------------------------------------------------------------------------------
# 1. float64 truth, independent of the op: scene F and "thin", the four backward routes, plain and fused
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def truth():
    t = np.load(os.path.join(ROOT, "tests", "golden", "median_depth_truth.npz"))
    gen = _generator()
    out = {}
    for s in gen.SCENES:
        assert t[f"{s}_mask"].sum() <= 0.02 * t[f"{s}_mask"].size          # the condition of the masking (F: 4, thin: 2 of 960)
        out[s] = {k[len(s) + 1:]: torch.from_numpy(t[k]) for k in t.files if k.startswith(s + "_")}
        out[s]["scene"] = gen.scene(s)
    return out


def _zero_or_none(g):
    return g is None or not g.any()


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("kind", ["F", "thin"])
def test_maps_and_gradients_against_float64_truth(truth, kind, route, fused):
    t = truth[kind]
    sc, cam = t["scene"]
    keep = ~t["mask"]
    _set_route(route)
    out, g = _run(sc, cam, Gm=t["G"].cuda(), fused=fused)
    _check_maps(out, 24, 40)
    assert out["median_depth"].requires_grad
    D, I = out["median_depth"].detach().cpu(), out["median_id"].cpu()
    assert torch.equal((out["radii"] > 0).cpu(), t["visible"])
    name = f"median depth truth {kind} [{route}{', fused' if fused else ''}]"
    wrong = (I != t["id"]) & keep
    report(name, "pixels off the mask with another id", float(wrong.sum()))
    report(name, "masked pixels with another id", float(((I != t["id"]) & ~keep).sum()))
    assert not wrong.any()
    e = ((D.double() - t["depth"]).abs() * keep).max().item() / t["depth"].abs().max().item()
    report(name, "depth err / max depth", e)
    assert e <= FWD_ATOL
    empty = t["count"] == 0
    assert torch.equal(D[empty & keep], torch.zeros(int((empty & keep).sum()))) and (I[empty & keep] == -1).all()
    assert torch.equal(I == -1, D == 0) and ((I == -1) == empty)[keep].all()
    # the gradient reaches means3D alone
    pc = _run.last_pc
    P = sc.means3D.shape[0]
    for k in ("opacity", "scaling", "rotation", "viewspace", "dc", "rest"):
        assert _zero_or_none(g[k]), k
    vs = out["viewspace_points"].grad
    zeros = lambda *s: torch.zeros(*s, dtype=torch.float64)
    for leaf in (pc._opacity, pc._scaling, pc._rotation):                  # (None stands for zeros in check_backward's pairs)
        if leaf.grad is None:
            leaf.grad = torch.zeros_like(leaf)
    worst = check_backward(pc, vs if vs is not None else torch.zeros(P, 3, device="cuda"),
                           {"means3D": t["means3D"], "opacities": zeros(P, 1), "means2D": zeros(P, 3)}, name, rtol=BWD_RTOL)
    print(f"{name}: gradients {worst}")
    assert g["xyz"].abs().max() > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the op's own per-pixel decomposition
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["F", "deep", "opaque", "sparse"])
def test_maps_against_per_pixel_backwards(kind):
    """one backward of a plain render per pixel with dL/dC = e_0: colors_precomp.grad[:, 0] is w_ip of that pixel, non-zero
    exactly on its blended entries; in list order (depth, ties by index) and float64, T_i = 1 - sum_{j<i} w_j"""
    from gaussian_renderer import render
    sc, cam = _scene_b(kind)[:2]
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    P = pc.get_xyz.shape[0]
    col = torch.rand(P, 3, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_(True)
    plain = render(cam.to("cuda"), pc, PIPE, torch.zeros(3, device="cuda"), override_color=col, **PLAIN)
    img = plain["render"]
    h, w = img.shape[1:]
    z32 = _view_z(pc, cam).detach()
    order = torch.argsort(z32, stable=True)
    one = torch.zeros_like(img)
    first = torch.full((h, w), -1, dtype=torch.int64, device="cuda")      # m(p), as a model row
    second = torch.full((h, w), -1, dtype=torch.int64, device="cuda")     # the other accepted row of a near-threshold pixel
    near = torch.zeros(h, w, dtype=torch.bool, device="cuda")
    pos = torch.full((h, w), -1, dtype=torch.int64, device="cuda")        # position of m(p) among the pixel's blended entries
    crossing = torch.zeros(h, w, dtype=torch.bool, device="cuda")
    for y in range(h):
        for x in range(w):
            one[0, y, x] = 1.0
            g, = torch.autograd.grad(img, [col], one, retain_graph=True)
            one[0, y, x] = 0.0
            wl = g[:, 0].double()[order]
            b = torch.nonzero(wl != 0)[:, 0]                              # the blended entries, in list order
            if b.numel() == 0:
                continue
            wb = wl[b]
            T_before = 1.0 - (torch.cumsum(wb, 0) - wb)
            T_after = T_before - wb
            k = int((T_before > 0.5).sum().item()) - 1                    # T_before decreases: the candidates are a prefix
            first[y, x], pos[y, x] = order[b[k]], k
            crossing[y, x] = bool(T_after[k] <= 0.5)
            close = torch.nonzero((T_after - 0.5).abs() < NEAR)[:, 0]
            if close.numel():
                near[y, x] = True
                i = int(close[0].item())                                  # (alpha >= 1/255: T moves by > NEAR per entry near 0.5)
                a, bb = order[b[i]], order[b[min(i + 1, b.numel() - 1)]]
                second[y, x] = bb if first[y, x] == a else a
    with torch.no_grad():
        out = _render(cam.to("cuda"), pc, torch.zeros(3, device="cuda"))
    torch.cuda.synchronize()
    _check_maps(out, h, w)
    D, I = out["median_depth"], out["median_id"].long()
    name = f"median depth per-pixel decomposition [{kind}]"
    frac = near.float().mean().item()
    report(name, "near-threshold pixel fraction", frac)
    print(f"{name}: empty {(first < 0).sum().item()}  crossing {crossing.sum().item()}  never crossing "
          f"{((first >= 0) & ~crossing).sum().item()}  near {near.sum().item()} of {h * w}  median position among the blended "
          f"{pos[first >= 0].min().item() if (first >= 0).any() else -1} .. {pos.max().item()}")
    assert frac <= (0.05 if kind == "deep" else 0.02)
    assert torch.equal(I[~near], first[~near])
    assert ((I == first) | (I == second))[near].all()
    report(name, "near-threshold pixels that report the other entry", float((I != first).sum().item()))
    # every id is a rendered Gaussian of the model, -1 exactly where the pixel's weights are all zero
    assert torch.equal(I == -1, first == -1)
    got = I[I >= 0]
    assert (got < P).all() and (plain["radii"][got] > 0).all()
    # the depth is that Gaussian's view depth: the bits K1 stored, the same for every pixel of one id
    assert not D[I == -1].any()
    zg = z32[got]
    e = ((D[I >= 0] - zg).abs() / zg.abs()).max().item() if got.numel() else 0.0
    report(name, "depth vs the view depth of the id, rel", e)
    assert e <= 1e-6
    per_id = torch.zeros(P, dtype=torch.float32, device="cuda")
    per_id[got] = D[I >= 0]                                               # (any one pixel's value per id)
    assert torch.equal(per_id[got].view(torch.int32), D[I >= 0].view(torch.int32))
    if kind == "sparse":
        assert (first < 0).sum() > 200 and ((first >= 0) & ~crossing).sum() > 400


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the camera
# ---------------------------------------------------------------------------------------------------------------------------
def test_camera_gradient_against_float64(truth):
    """viewmatrix as a float64 leaf of the truth's generator against the op's gradient of the same loss; the map does not depend
    on projmatrix or campos: zero"""
    t = truth["F"]
    sc, cam = t["scene"]
    names = ("world_view_transform", "full_proj_transform", "camera_center")
    c = copy.copy(cam.to("cuda"))
    for n in names:
        setattr(c, n, getattr(c, n).clone().requires_grad_(True))
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    out = _render(c, pc, torch.zeros(3, device="cuda"))
    (out["median_depth"] * t["G"].cuda()).sum().backward()
    torch.cuda.synchronize()
    assert not c.full_proj_transform.grad.any() and not c.camera_center.grad.any()
    got, ref = c.world_view_transform.grad.double().cpu().reshape(-1), t["viewmatrix"].reshape(-1)
    e = ((got - ref).abs().max() / ref.abs().max()).item()
    report("median depth camera gradient vs float64", "viewmatrix", e)
    assert ref.abs().max() > 0 and e <= CAMERA_CEIL, e
    assert pc._xyz.grad.abs().max() > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 4. nothing else moves
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_default_path_is_untouched(fused, monkeypatch):
    sc, cam = _scene_f()[:2]
    dL, Gm = scenes.grad_seed(40, 24, 78).cuda(), _seed(24, 40)
    calls = []
    monkeypatch.setattr(dgr, "_median_probe", calls.append)
    out0, g0 = _run(sc, cam, dL=dL, fused=fused, median=False)
    assert calls == [] and "median_depth" not in out0             # a call without the flag never reaches msgs_median_depth_*
    # a loss that ignores the maps: today's backward, bit for bit; only the forward replay ran
    out1, g1 = _run(sc, cam, dL=dL, fused=fused)
    assert calls == ["msgs_median_depth_forward"]
    for k in OUT5:
        assert torch.equal(out0[k], out1[k]), k
    _equal_grads(g0, g1, "a colour-only loss with the flag on")
    # a loss that uses the map: the ordinary outputs and the maps are still the same bits, the backward entry ran
    del calls[:]
    out2, g2 = _run(sc, cam, dL=dL, Gm=Gm, fused=fused)
    assert calls == ["msgs_median_depth_forward", "msgs_median_depth_backward"]
    for k in OUT5:
        assert torch.equal(out0[k], out2[k]), k
    assert all(torch.equal(a, b) for a, b in zip(_maps(out1), _maps(out2)))
    assert not torch.equal(g2["xyz"], g0["xyz"])
    for k in GRADS:                                               # ... and only means3D moved (the depth variant of the
        if k != "xyz" and g0[k] is not None:                      # backward ran: another kernel, the same sums)
            assert _rel(g2[k], g0[k]) <= 1e-6, k


def test_absgrad_does_not_include_a_median_share():
    from gaussian_renderer import _colour_inputs, _settings, _shape_inputs
    sc, cam = _scene_f()[:2]
    camd, bg = cam.to("cuda"), torch.zeros(3, device="cuda")
    dL, Gm = scenes.grad_seed(40, 24, 78).cuda(), _seed(24, 40)
    got = []
    for use in (False, True):
        pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
        r = dgr.GaussianRasterizer(_settings(camd, pc, PIPE, bg, 1.0, False, False, 1.0), absgrad=True).with_median_depth()
        vs = torch.zeros_like(pc.get_xyz, requires_grad=True)
        outs = r(means3D=pc.get_xyz, means2D=vs, opacities=pc.get_opacity, **_colour_inputs(camd, pc, PIPE, None),
                 **_shape_inputs(pc, PIPE, 1.0))
        assert len(outs) == 7
        ((outs[0] * dL).sum() + ((outs[5] * Gm).sum() if use else 0.0)).backward()
        torch.cuda.synchronize()
        got.append((vs.absgrad.clone(), vs.grad.clone(), pc._xyz.grad.clone()))
    assert got[0][0].abs().max() > 0 and torch.equal(got[0][0], got[1][0]) and _rel(got[1][1], got[0][1]) <= 1e-6
    assert not torch.equal(got[0][2], got[1][2])


def test_host_entry_returns_the_render_dict_plus_the_maps():
    from gaussian_renderer import RESULT_KEYS, render, render_with_median_depth
    sc, cam = _scene_f()[:2]
    camd, bg = cam.to("cuda"), torch.tensor([0.2, 0.4, 0.1], device="cuda")
    for fused in (False, True):
        for alpha in (False, True):
            pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
            out = render_with_median_depth(camd, pc, PIPE, bg, fused=fused, alpha=alpha, **PLAIN)
            assert set(out) == set(RESULT_KEYS) | {"median_depth", "median_id"} | ({"alpha"} if alpha else set())
            ref = _render(camd, SyntheticGaussians(sc, "cuda", requires_grad=True), bg, alpha=alpha, fused=fused)
            assert all(torch.equal(a, b) for a, b in zip(_maps(out), _maps(ref)))
            assert torch.equal(out["render"], ref["render"]) and (not alpha or torch.equal(out["alpha"], ref["alpha"]))
            plain = render(camd, SyntheticGaussians(sc, "cuda", requires_grad=True), PIPE, bg, **PLAIN)
            assert fused or torch.equal(out["render"], plain["render"])
            out["median_depth"].mean().backward()
            assert pc._xyz.grad.abs().max() > 0
    with pytest.raises(ValueError, match="override_color"):
        render_with_median_depth(camd, pc, PIPE, bg, override_color=torch.zeros(sc.P, 3, device="cuda"), fused=True)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. linearity
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_colour_depth_alpha_distortion_median_features_is_linear(fused):
    sc, cam = _scene_f()[:2]
    h, w = 24, 40
    seeds = dict(dL=scenes.grad_seed(w, h, 78).cuda(), Gd=(scenes.grad_seed(w, h, 77)[0] * 0.1).cuda(),
                 Ga=scenes.grad_seed(w, h, 79)[1].cuda(), Gx=_seed(h, w, 131), Gm=_seed(h, w), G=_seed_map(5, h, w))
    feats = _features(sc.P, 5)
    bg = torch.tensor([0.1, 0.2, 0.3])
    parts = {}
    for name in seeds:
        _, parts[name] = _run(sc, cam, feats=feats if name == "G" else None, fused=fused, bg=bg, median=name == "Gm",
                              **{name: seeds[name]})
    # all six at once, twice over one graph
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    f = feats.cuda().clone().requires_grad_(True)
    out = _render(cam.to("cuda"), pc, bg.cuda(), distortion=True, features=f, alpha=True, fused=fused)
    loss = _loss(out, seeds)
    loss.backward(retain_graph=True)
    torch.cuda.synchronize()
    gs = _grads(pc, out)
    for k in GRADS:
        ref = sum(g[k] for g in parts.values() if g[k] is not None)
        e = _rel(gs[k], ref)
        report(f"median depth linearity fused={fused}", f"grad {k}", e)
        assert e <= LIN_TOL.get(k, 1e-6), f"grad {k} rel err {e:.3e}"
    gm = parts["Gm"]["xyz"]
    without = sum(g["xyz"] for n, g in parts.items() if n != "Gm")
    assert gm.abs().max() > 0 and _rel(gs["xyz"], without) > 1e-4          # the median's share is in it
    for leaf in (pc._xyz, pc._opacity, pc._scaling, pc._rotation, pc._features_dc, pc._features_rest, out["viewspace_points"], f):
        leaf.grad = None
    loss.backward()
    torch.cuda.synchronize()
    _equal_grads(_grads(pc, out), gs, "second backward over the retained graph")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. behind every forward route: the bits of the exact-buffer single pass
# ---------------------------------------------------------------------------------------------------------------------------
def _forward(sc, cam, fused=False):
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    out = _render(cam.to("cuda"), pc, torch.zeros(3, device="cuda"), fused=fused)
    torch.cuda.synchronize()
    return out


def _same_maps(a, b, what):
    assert (a["median_id"] >= 0).any(), what
    assert torch.equal(a["median_id"], b["median_id"]), (what, "id")
    assert torch.equal(a["median_depth"].detach().view(torch.int32), b["median_depth"].detach().view(torch.int32)), (what, "depth")
    assert torch.equal(a["render"], b["render"]), (what, "render")


def test_two_runs_and_both_granularities_give_equal_bits():
    sc, cam = _scene_f()[:2]
    reset_forward_state()
    ref = _forward(sc, cam)
    _same_maps(_forward(sc, cam), ref, "two runs")
    for route in ROUTES:
        _set_route(route)
        _same_maps(_forward(sc, cam), ref, route)
    sc, cam = _scene_b("deep")[:2]
    _set_route("default")
    ref = _forward(sc, cam)
    _set_route("fine")
    _same_maps(_forward(sc, cam), ref, "deep, fine")


@pytest.mark.parametrize("fused", [False, True])
def test_maps_behind_a_redone_stage2(fused):
    Wr, Hr = 320, 200
    sc, cam = small_scene(20000, Wr, Hr, seed=21)
    reset_forward_state()
    n0 = non_speculative()
    ref = _forward(sc, cam, fused)                                          # first call: exact buffers
    assert non_speculative() == n0 + 1
    D = dgr._resolve(ref["render"].grad_fn.state)[3]
    key = (torch.cuda.current_device(), sc.P, Wr, Hr, 0, 0)
    assert key in dgr._last_instances
    reset_forward_state()
    dgr._last_instances[key] = guesses_around(D)[0] // 2                    # its capacity is below D: the redo
    n0 = non_speculative()
    got = _forward(sc, cam, fused)
    assert non_speculative() == n0 + 1
    _same_maps(got, ref, "redo")
    n0 = non_speculative()
    got = _forward(sc, cam, fused)                                          # ... and the speculative stage 2 that stands
    assert non_speculative() == n0
    _same_maps(got, ref, "speculative")


def test_maps_in_forced_slabs():
    from test_slab_gpu import _dense_scene
    Ws, Hs = 960, 720
    sc, cam = _dense_scene(80_000, Ws, Hs, 9, opacity=(0.5, 0.99)), scenes.front_camera(Ws, Hs)
    got = {}
    for policy in ("never", "0.12"):
        with _env({"slab": policy}):
            got[policy] = _forward(sc, cam)
            assert slab_stats(got[policy]["render"].grad_fn)["active"] == (policy != "never")
    _same_maps(got["0.12"], got["never"], "slab 0.12 vs never")


def test_maps_behind_the_occlusion_cut_off():
    from test_occlusion_gpu import _giants_scene, _stats
    Wo, Ho = 420, 300
    sc, cam = _giants_scene(2500, Wo, Ho, 5, 60, giant_scale=1.2, giant_opacity=0.9), scenes.front_camera(Wo, Ho)
    got = {}
    for occ in (0, 1):
        with _env({"occlusion": occ}):
            got[occ] = _forward(sc, cam)
            if occ:
                assert _stats(got[occ]["render"].grad_fn)["closed_blocks"] > 0
    _same_maps(got[1], got[0], "occlusion cut-off on vs off")


# ---------------------------------------------------------------------------------------------------------------------------
# 7. composition and edges
# ---------------------------------------------------------------------------------------------------------------------------
def test_antialiased_maps_are_the_plain_maps_of_the_compensated_opacity():
    from gaussian_renderer import _colour_inputs, _settings, _shape_inputs
    sc, cam = _scene_f()[:2]
    camd, bg = cam.to("cuda"), torch.zeros(3, device="cuda")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    settings = _settings(camd, pc, PIPE, bg, 1.0, False, False, 1.0)
    shape = _shape_inputs(pc, PIPE, 1.0)
    kw = dict(means3D=pc.get_xyz, means2D=torch.zeros_like(pc.get_xyz), **_colour_inputs(camd, pc, PIPE, None), **shape)
    with torch.no_grad():
        base = dgr.GaussianRasterizer(settings)
        aa = base.with_antialiasing().with_median_depth()(opacities=pc.get_opacity, **kw)
        o_eff = dgr.screen_compensation(pc.get_xyz, pc.get_opacity, settings, **shape)
        ref = base.with_median_depth()(opacities=o_eff, **kw)
        plain = base.with_median_depth()(opacities=pc.get_opacity, **kw)
    torch.cuda.synchronize()
    assert len(aa) == 7 and all(torch.equal(a, b) for a, b in zip(aa, ref))
    assert not torch.equal(aa[0], plain[0])                               # (the compensation does something on this scene)


def test_no_gaussians_gives_empty_maps_and_zero_gradients():
    rs = dgr.GaussianRasterizationSettings(24, 40, 0.5, 0.3, torch.tensor([0.2, 0.4, 0.1]).cuda(), 1.0, torch.eye(4).cuda(),
                                           torch.eye(4).cuda(), 3, torch.zeros(3).cuda(), False, False)
    z = lambda *s: torch.zeros(*s, device="cuda")
    m3, m2, f = z(0, 3).requires_grad_(), z(0, 3).requires_grad_(), z(0, 7).requires_grad_()
    out = dgr.GaussianRasterizer(rs, return_alpha=True).with_features(f).with_distortion().with_median_depth()(
        means3D=m3, means2D=m2, opacities=z(0, 1), shs=z(0, 16, 3), scales=z(0, 3), rotations=z(0, 4))
    assert len(out) == 10 and [tuple(o.shape) for o in out[5:]] == [(24, 40)] * 4 + [(7, 24, 40)]
    assert out[7].dtype == torch.float32 and not out[7].any()
    assert out[8].dtype == torch.int32 and (out[8] == -1).all() and not out[8].requires_grad
    (out[7].sum() + out[0].sum()).backward()
    assert m3.grad.shape == (0, 3)


def test_an_empty_view_gives_empty_maps(monkeypatch):
    """a camera that looks away: Gaussians, but no instance — the forward fills 0 and -1, the backward launches nothing"""
    sc, cam = _scene_f()[:2]
    sc = copy.copy(sc)
    sc.means3D = sc.means3D * torch.tensor([1.0, 1.0, -1.0])            # all behind the camera
    calls = []
    monkeypatch.setattr(dgr, "_median_probe", calls.append)
    out, g = _run(sc, cam, Gm=_seed(24, 40), dL=scenes.grad_seed(40, 24, 78).cuda())
    assert calls == ["msgs_median_depth_forward"]
    assert not (out["radii"] > 0).any() and not out["median_depth"].detach().any() and (out["median_id"] == -1).all()
    assert not g["xyz"].any() and not g["opacity"].any()


def test_maps_with_two_views_in_flight():
    """inside deferred_forward a call with the maps resolves its own view before the replay: the serial bits"""
    Wv, Hv, nv = 40, 24, 2
    sc, cam = _scene_f()[:2]
    cams = [cam.to("cuda")] * nv
    Gm, dL = _seed(Hv, Wv), scenes.grad_seed(Wv, Hv, 78).cuda()
    bg = torch.zeros(3, device="cuda")
    reset_forward_state()
    serial = [_run(sc, cam, Gm=Gm, dL=dL) for cam in cams]
    reset_forward_state()
    pcs = [SyntheticGaussians(sc, "cuda", requires_grad=True) for _ in cams]
    with dgr.deferred_forward() as pending:
        outs = [_render(cam, pc, bg) for cam, pc in zip(cams, pcs)]
        assert len(pending) == nv
    for o, pc, (ro, rg) in zip(outs, pcs, serial):
        ((o["median_depth"] * Gm).sum() + (o["render"] * dL).sum()).backward()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(_maps(o), _maps(ro)))
        _equal_grads(_grads(pc, o), rg, "deferred")


def test_verification_mode_is_refused_before_any_launch(monkeypatch):
    sc, cam = _scene_f()[:2]
    camd, bg = cam.to("cuda"), torch.zeros(3, device="cuda")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    calls = []
    monkeypatch.setattr(dgr, "_median_probe", calls.append)
    before = dgr.forward_stats["forwards"]
    prev = dgr.set_deterministic(True)
    try:
        for fused in (False, True):
            with pytest.raises(ValueError, match="verification mode"):
                _render(camd, pc, bg, fused=fused)
    finally:
        dgr.set_deterministic(prev)
    assert dgr.forward_stats["forwards"] == before and calls == []


def test_c_entries_check_capacity_and_arguments():
    import ctypes as C
    from gaussian_renderer import render
    sc, cam = _scene_f()[:2]
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    out = render(cam.to("cuda"), pc, PIPE, torch.zeros(3, device="cuda"), **PLAIN)
    ctx = out["render"].grad_fn
    geom, binning, image, D = dgr._resolve(ctx.state)
    lib, P = dgr._C.lib, sc.P
    dmap = torch.full((24, 40), 7.0, device="cuda")
    imap = torch.full((24, 40), 7, dtype=torch.int32, device="cuda")
    G = _seed(24, 40)
    rec = torch.zeros(lib.msgs_backward_scratch_bytes(P), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(P=P, D=D, gb=None, o=dmap, i=imap):
        return lib.msgs_median_depth_forward(ctx.call.view_ref, P, p(geom), geom.numel() if gb is None else gb, D, p(binning),
                                             binning.numel(), p(image), image.numel(), p(o), p(i), stream)

    def bwd(P=P, i=imap, g=G, r=rec, rb=None):
        return lib.msgs_median_depth_backward(ctx.call.view_ref, P, p(i), p(g), p(r), rec.numel() if rb is None else rb, stream)
    assert fwd(P=-1) == -1 and fwd(o=None) == -1 and fwd(i=None) == -1 and fwd(gb=16) == -2
    assert bwd(P=-1) == -1 and bwd(i=None) == -1 and bwd(g=None) == -1 and bwd(r=None) == -1 and bwd(rb=rec.numel() - 1) == -2
    torch.cuda.synchronize()
    assert (dmap == 7.0).all() and (imap == 7).all() and not rec.any()              # refused calls wrote nothing
    prev = dgr.set_deterministic(True)
    try:
        assert fwd() == -1 and bwd() == -1                                          # not offered in the verification mode
    finally:
        dgr.set_deterministic(prev)
    # no instance: 0 and -1 everywhere; a map of -1 (and ids outside the model) adds nothing; P == 0 launches nothing
    assert fwd(D=0) == 0 and bwd() == 0 and bwd(P=0) == 0
    imap2 = torch.full((24, 40), P + 5, dtype=torch.int32, device="cuda")
    assert bwd(i=imap2) == 0
    torch.cuda.synchronize()
    assert not dmap.any() and (imap == -1).all() and not rec.any()
    # the real call: the maps of the Python layer; the records get slot 9 alone: the sum of G over each Gaussian's pixels
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = _render(cam.to("cuda"), SyntheticGaussians(sc, "cuda", requires_grad=False), torch.zeros(3, device="cuda"))
    assert torch.equal(dmap, ref["median_depth"]) and torch.equal(imap, ref["median_id"]) and (imap >= 0).all()
    slots = rec[:80 * P].view(torch.float64).view(P, 10)              # ten doubles per record (msgs_internal.h)
    assert not slots[:, :9].any()
    want = torch.zeros(P, dtype=torch.float64, device="cuda").index_add_(0, imap.view(-1).long(), G.view(-1).double())
    e = ((slots[:, 9] - want).abs().max() / want.abs().max()).item()
    report("median depth records", "slot 9 vs the per-Gaussian sum of G, rel", e)
    assert e <= 1e-6 and not slots[want == 0, 9].any()
    # it ADDS: a second call doubles the sums
    assert bwd() == 0
    torch.cuda.synchronize()
    assert ((slots[:, 9] - 2 * want).abs().max() / want.abs().max()).item() <= 1e-6

"""Depth distortion on the GPU (SPEC M13; include/msgs.h msgs_distortion_forward / msgs_distortion_backward):
    Dist_p = 2 sum_{j<i} w_ip w_jp (z_i - z_j),   w_ip = alpha_ip T_ip,   i = 1..n in tile-list order (front to back)
one more opt-in output [H,W] with gradients to the geometry and the camera.

References, none of them the kernels under test:
  1  float64, from oracle/torch_oracle.py's preprocess and its blend loop restated: tests/golden/distortion_truth.npz, scene F and
     "far" (the same picture from 2000 units away); generator and the CPU test that pins it: tests/golden/
     make_distortion_golden.py, tests/test_distortion_cpu.py.  Borderline pixels carry G = 0 on both sides and are left out of the
     map comparison.
  2  the op's own per-pixel decomposition: one backward of a plain render per pixel with dL/dC = e_0 gives w_ip; Dist is formed
     from those weights and the op's depths in float64.
Tolerances are the project's own for quantities of the same kind (BWD_RTOL, LIN_TOL of tests/test_depth_grad_gpu.py, CEIL of
tests/test_camera_grad_gpu.py); the far map is held to 1e-5 of its maximum — a tenth of what the unshifted float32 formulas
reach and thirty times what the shifted ones reach with exact weights (tests/test_distortion_cpu.py).  The measured maxima are
printed (pytest -s) and recorded in profiles/distortion_notes.md.
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
from parity_utils import BWD_RTOL, PIPE, check_backward, rel_err, report, small_scene
from route_utils import PLAIN, guesses_around, non_speculative, per_pixel, reset_forward_state, slab_stats
from synthetic_model import SyntheticGaussians
from test_absgrad_gpu import _scene_b, _scene_f
from test_alpha_grad_gpu import MS, _scene
from test_camera_grad_gpu import CEIL as CAMERA_CEIL
from test_depth_grad_gpu import LIN_TOL, ROUTES, _view_z
from test_features_gpu import GRADS, _env, _equal_grads, _features, _grads, _rel, _seed_map, _set_route

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT6 = ("render", "acc_pixel_size", "depth", "radii", "pixel_sizes", "alpha")


@pytest.fixture(autouse=True)
def _reset_routes():
    yield
    dgr._C.lib.msgs_set_backward_generation(0)
    dgr._C.lib.msgs_set_blend_granularity(0)


def _generator():
    spec = importlib.util.spec_from_file_location("make_distortion_golden", os.path.join(ROOT, "tests", "golden",
                                                                                         "make_distortion_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _seed(h, w, seed=131):
    """G = dL/dDist [h,w] float32 on the GPU, seeded, uniform in (-0.5, 0.5)"""
    return (torch.rand(h, w, generator=torch.Generator().manual_seed(seed)) - 0.5).cuda()


def _render(cam, pc, bg, st=PLAIN, distortion=True, features=None, alpha=False, fused=False, smod=1.0, pipe=PIPE):
    """render() / render_fused() of the host layer with any of the opt-in outputs: the result dict plus "alpha" / "distortion" /
    "features" """
    from gaussian_renderer import RESULT_KEYS, _colour_inputs, _settings, _shape_inputs
    st = {**PLAIN, **st}
    settings = _settings(cam, pc, pipe, bg, smod, st["filter_small"], st["filter_large"], st["fade_size"])
    r = dgr.GaussianRasterizer(settings, return_alpha=alpha).with_features(features).with_distortion(distortion)
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
    if alpha:
        out["alpha"] = rest.pop(0)
    if distortion:
        out["distortion"] = rest.pop(0)
    if features is not None:
        out["features"] = rest.pop(0)
    assert not rest
    return out


def _run(sc, cam, st=PLAIN, Gx=None, dL=None, Gd=None, Ga=None, feats=None, G=None, fused=False, smod=1.0, pipe=PIPE, bg=None,
         distortion=True):
    """one forward + backward on fresh leaves; the loss is the sum of the given seeds times their maps (Gx: the distortion
    map's).  Returns (out, {name: grad})"""
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    f = feats.detach().cuda().clone().requires_grad_(True) if feats is not None else None
    bg = torch.zeros(3, device="cuda") if bg is None else bg.cuda()
    out = _render(cam.to("cuda"), pc, bg, st, distortion, f, Ga is not None, fused, smod, pipe)
    loss = 0.0
    for seed, key in ((dL, "render"), (Gd, "depth"), (Ga, "alpha"), (Gx, "distortion"), (G, "features")):
        if seed is not None:
            loss = loss + (out[key] * seed).sum()
    loss.backward()
    torch.cuda.synchronize()
    _run.last_pc = pc
    return out, _grads(pc, out)


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2. float64 truth, independent of the op: scene F, and the same picture from 2000 units away
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def truth():
    t = np.load(os.path.join(ROOT, "tests", "golden", "distortion_truth.npz"))
    gen = _generator()
    out = {}
    for s in gen.SCENES:
        assert t[f"{s}_borderline"].sum() <= 0.02 * t[f"{s}_borderline"].size       # the condition of the masking (1 of 960)
        out[s] = {k[len(s) + 1:]: torch.from_numpy(t[k]) for k in t.files if k.startswith(s + "_")}
        out[s]["scene"] = gen.scene(s)
    return out


FAR_MAP_TOL = 1e-5           # of max Dist (the module docstring; tests/test_distortion_cpu.py measures both sides of it)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("kind", ["F", "far"])
def test_map_and_gradients_against_float64_truth(truth, kind, route, fused):
    """the map off the borderline pixel and every geometry gradient, on the four backward routes, plain and fused (measured
    maxima: profiles/distortion_notes.md)"""
    t = truth[kind]
    sc, cam = t["scene"]
    keep = ~t["borderline"]
    _set_route(route)
    out, _ = _run(sc, cam, Gx=t["G"].cuda(), fused=fused)
    D = out["distortion"].detach()
    assert D.shape == (24, 40) and D.dtype == torch.float32 and out["distortion"].requires_grad
    assert torch.equal((out["radii"] > 0).cpu(), t["visible"])
    name = f"distortion truth {kind} [{route}{', fused' if fused else ''}]"
    e = rel_err(D.cpu() * keep, t["map"] * keep)
    report(name, "map err / max Dist", e)
    print(f"{name}: map err / max Dist {e:.3e}")
    assert e <= (FAR_MAP_TOL if kind == "far" else BWD_RTOL)
    pc = _run.last_pc
    worst = check_backward(pc, out["viewspace_points"].grad, {k: t[k] for k in ("means3D", "opacities", "scales", "rotations",
                                                                                "means2D")}, name)
    print(f"{name}: gradients {worst}")
    for k in ("_features_dc", "_features_rest"):
        assert getattr(pc, k).grad is None or not getattr(pc, k).grad.any(), k


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the op's own per-pixel decomposition
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["F", "deep"])
def test_map_against_per_pixel_backwards(kind):
    """one backward of a plain render per pixel with dL/dC = e_0: colors_precomp.grad[:, 0] is w_ip of that pixel; with the
    op's depths in list order (depth, ties by index) the definition in float64 is the map"""
    from gaussian_renderer import render
    sc, cam = _scene_b(kind)[:2]
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    P = pc.get_xyz.shape[0]
    col = torch.rand(P, 3, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_(True)
    img = render(cam.to("cuda"), pc, PIPE, torch.zeros(3, device="cuda"), override_color=col, **PLAIN)["render"]
    h, w = img.shape[1:]
    z32 = _view_z(pc, cam).detach()
    order = torch.argsort(z32, stable=True)
    z = z32[order].double()
    one = torch.zeros_like(img)
    ref = torch.zeros(h, w, dtype=torch.float64, device="cuda")
    pairs = torch.zeros(h, w, dtype=torch.int64, device="cuda")
    for y in range(h):
        for x in range(w):
            one[0, y, x] = 1.0
            g, = torch.autograd.grad(img, [col], one, retain_graph=True)
            wgt = g[:, 0].double()[order]
            wz = wgt * z
            ref[y, x] = 2.0 * (wgt * (z * (torch.cumsum(wgt, 0) - wgt) - (torch.cumsum(wz, 0) - wz))).sum()
            pairs[y, x] = (wgt != 0).sum()
            one[0, y, x] = 0.0
    with torch.no_grad():
        D = _render(cam.to("cuda"), pc, torch.zeros(3, device="cuda"))["distortion"]
    torch.cuda.synchronize()
    assert (pairs >= 2).any()
    e = rel_err(D, ref)
    report(f"distortion per-pixel decomposition [{kind}]", "map rel err", e)
    print(f"distortion per-pixel decomposition [{kind}]: {e:.3e}; pixels with fewer than two pairs {(pairs < 2).sum().item()}")
    assert e <= BWD_RTOL
    assert not D[pairs < 2].any()                                    # exactly 0.0f with fewer than two counted pairs


# ---------------------------------------------------------------------------------------------------------------------------
# 4. invariants
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sparse", "opaque", "F", "deep"])
def test_map_is_non_negative_and_zero_without_a_pair(kind):
    """... and the backward on the same scenes ("deep": every tile list spans several staged batches, partial tiles in x and y;
    "sparse": whole tiles empty) repeats bit for bit — a batch read before it is staged, or staged before it is consumed,
    does not"""
    sc, cam = _scene_b(kind)[:2]
    Gx = _seed(cam.image_height, cam.image_width)
    out, g = _run(sc, cam, Gx=Gx)
    again, g2 = _run(sc, cam, Gx=Gx)
    assert torch.equal(out["distortion"].detach(), again["distortion"].detach())
    _equal_grads(g, g2, kind)
    assert g["xyz"].abs().max() > 0 or kind == "sparse"
    D = out["distortion"].detach()
    assert (D.max() > 0 or kind == "sparse") and D.min() >= -1e-6 * D.max()
    image = dgr._resolve(out["render"].grad_fn.state)[2]
    n_contrib = per_pixel(image, cam.image_width, cam.image_height)[1].view(torch.int32).view(D.shape)
    few = n_contrib < 2
    assert few.any() or kind != "sparse"
    assert not D[few].any()                                          # exactly 0.0f
    assert all(torch.isfinite(v).all() for v in g.values() if v is not None)


def test_equal_depths_give_an_exactly_zero_map():
    """all Gaussians on one plane z = const under the identity view matrix: every z~ is 0, so the map and every dDist/dw are
    exactly 0 and only dDist/dz_i = 2 w_i B_i is left — the signed form's slope at a tie, which reaches means3D's z alone.
    Everything that goes through the blend weights (opacity, scales, rotations, means2D, x and y of means3D) is held to 1e-6
    of the colour loss's gradient."""
    sc, cam = _scene_f()[:2]
    sc = copy.copy(sc)
    m = sc.means3D.clone()
    f = 3.0 / m[:, 2]
    sc.means3D = torch.stack([m[:, 0] * f, m[:, 1] * f, torch.full_like(f, 3.0)], 1)
    sc.scales = sc.scales * f[:, None]
    assert torch.equal(cam.world_view_transform[:3, :3], torch.eye(3))
    dL = scenes.grad_seed(40, 24, 78).cuda()
    _, gc = _run(sc, cam, dL=dL)
    out, g = _run(sc, cam, Gx=_seed(24, 40))
    assert (out["radii"] > 0).sum() >= 150
    assert not out["distortion"].detach().any()
    for k in ("opacity", "scaling", "rotation", "viewspace"):
        assert g[k].abs().max() <= 1e-6 * gc[k].abs().max(), k
    assert g["xyz"][:, :2].abs().max() <= 1e-6 * gc["xyz"].abs().max()
    assert g["xyz"][:, 2].abs().max() > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 5. linearity
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_colour_depth_alpha_distortion_is_linear(fused):
    sc, cam, st, smod, pipe, _ = _scene("C")
    h, w = cam.image_height, cam.image_width
    dL = scenes.grad_seed(w, h, 78).cuda()
    Gd = (scenes.grad_seed(w, h, 77)[0] * 0.1).cuda()
    Ga = scenes.grad_seed(w, h, 79)[1].cuda()
    Gx = _seed(h, w)
    bg = torch.tensor([0.1, 0.2, 0.3])
    _, gc = _run(sc, cam, st, dL=dL, fused=fused, bg=bg)
    _, gd = _run(sc, cam, st, Gd=Gd, fused=fused, bg=bg)
    _, ga = _run(sc, cam, st, Ga=Ga, fused=fused, bg=bg)
    _, gx = _run(sc, cam, st, Gx=Gx, fused=fused, bg=bg)
    _, gs = _run(sc, cam, st, Gx=Gx, dL=dL, Gd=Gd, Ga=Ga, fused=fused, bg=bg)
    for k in GRADS:
        ref = sum(g[k] for g in (gc, gd, ga, gx) if g[k] is not None)
        e = _rel(gs[k], ref)
        report(f"distortion linearity fused={fused}", f"grad {k}", e)
        assert e <= LIN_TOL.get(k, 1e-6), f"grad {k} rel err {e:.3e}"
    assert gx["xyz"].abs().max() > 0 and _rel(gs["xyz"], gc["xyz"] + gd["xyz"] + ga["xyz"]) > 1e-4   # the map's share is in it
    # ... and together with features: both helpers add to the same records in front of the main backward
    feats, G = _features(sc.P, 5), _seed_map(5, h, w)
    _, gf = _run(sc, cam, st, feats=feats, G=G, fused=fused, bg=bg, distortion=False)
    _, gb = _run(sc, cam, st, Gx=Gx, feats=feats, G=G, dL=dL, fused=fused, bg=bg)
    for k in GRADS:
        ref = sum(g[k] for g in (gc, gx, gf) if g[k] is not None)
        e = _rel(gb[k], ref)
        report(f"distortion + features linearity fused={fused}", f"grad {k}", e)
        assert e <= LIN_TOL.get(k, 1e-6), f"grad {k} rel err {e:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------
# 6. behind every forward route: the bits of the exact-buffer single pass
# ---------------------------------------------------------------------------------------------------------------------------
def _bits(sc, cam, Gx, dL, fused=False):
    return _run(sc, cam, PLAIN, Gx=Gx, dL=dL, fused=fused)


def _same_bits(a, b, what):
    (oa, ga), (ob, gb) = a, b
    assert oa["distortion"].abs().max() > 0, what
    assert torch.equal(oa["distortion"].detach(), ob["distortion"].detach()), (what, "map")
    _equal_grads(ga, gb, what)


def test_two_runs_give_equal_bits():
    sc, cam, st, *_ = _scene("A")
    Gx, dL = _seed(90, 150), scenes.grad_seed(150, 90, 78).cuda()
    reset_forward_state()
    _same_bits(_bits(sc, cam, Gx, dL), _bits(sc, cam, Gx, dL), "two runs")


@pytest.mark.parametrize("fused", [False, True])
def test_distortion_behind_a_redone_stage2(fused):
    Wr, Hr = 320, 200
    sc, cam = small_scene(20000, Wr, Hr, seed=21)
    Gx, dL = _seed(Hr, Wr), scenes.grad_seed(Wr, Hr, 78).cuda()
    reset_forward_state()
    n0 = non_speculative()
    ref = _bits(sc, cam, Gx, dL, fused)                                     # first call: exact buffers
    assert non_speculative() == n0 + 1
    D = dgr._resolve(ref[0]["render"].grad_fn.state)[3]
    key = (torch.cuda.current_device(), sc.P, Wr, Hr, 0, 0)
    assert key in dgr._last_instances
    reset_forward_state()
    dgr._last_instances[key] = guesses_around(D)[0] // 2                    # its capacity is below D: the redo
    n0 = non_speculative()
    got = _bits(sc, cam, Gx, dL, fused)
    assert non_speculative() == n0 + 1
    _same_bits(got, ref, "redo")
    n0 = non_speculative()
    got = _bits(sc, cam, Gx, dL, fused)                                     # ... and the speculative stage 2 that stands
    assert non_speculative() == n0
    _same_bits(got, ref, "speculative")


def test_distortion_in_forced_slabs():
    from test_slab_gpu import _dense_scene
    Ws, Hs = 960, 720
    sc, cam = _dense_scene(80_000, Ws, Hs, 9, opacity=(0.5, 0.99)), scenes.front_camera(Ws, Hs)
    Gx, dL = _seed(Hs, Ws), scenes.grad_seed(Ws, Hs, 78).cuda()
    got = {}
    for policy in ("never", "0.12"):
        with _env({"slab": policy}):
            got[policy] = _bits(sc, cam, Gx, dL)
            assert slab_stats(got[policy][0]["render"].grad_fn)["active"] == (policy != "never")
    _same_bits(got["0.12"], got["never"], "slab 0.12 vs never")


def test_distortion_behind_the_occlusion_cut_off():
    from test_occlusion_gpu import _giants_scene, _stats
    Wo, Ho = 420, 300
    sc, cam = _giants_scene(2500, Wo, Ho, 5, 60, giant_scale=1.2, giant_opacity=0.9), scenes.front_camera(Wo, Ho)
    Gx, dL = _seed(Ho, Wo), scenes.grad_seed(Wo, Ho, 78).cuda()
    got = {}
    for occ in (0, 1):
        with _env({"occlusion": occ}):
            got[occ] = _bits(sc, cam, Gx, dL)
            if occ:
                assert _stats(got[occ][0]["render"].grad_fn)["closed_blocks"] > 0
    _same_bits(got[1], got[0], "occlusion cut-off on vs off")


def test_distortion_with_two_views_in_flight():
    """inside deferred_forward a call with the map resolves its own view before the replay: the serial bits"""
    Wv, Hv, nv = 320, 200, 2
    sc = scenes.ball_scene(20000, seed=46, log_s=-3.0)
    cams = [scenes.ring_camera(v, 4, Wv, Hv).to("cuda") for v in range(nv)]
    Gx, dL = _seed(Hv, Wv), scenes.grad_seed(Wv, Hv, 78).cuda()
    bg = torch.zeros(3, device="cuda")
    reset_forward_state()
    serial = [_bits(sc, cam, Gx, dL) for cam in cams]
    reset_forward_state()
    pcs = [SyntheticGaussians(sc, "cuda", requires_grad=True) for _ in cams]
    with dgr.deferred_forward() as pending:
        outs = [_render(cam, pc, bg) for cam, pc in zip(cams, pcs)]
        assert len(pending) == nv
    for o, pc, ref in zip(outs, pcs, serial):
        ((o["distortion"] * Gx).sum() + (o["render"] * dL).sum()).backward()
        torch.cuda.synchronize()
        _same_bits((o, _grads(pc, o)), ref, "deferred")


# ---------------------------------------------------------------------------------------------------------------------------
# 7. nothing else moves
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_default_path_is_untouched(fused, monkeypatch):
    sc, cam, st, *_ = _scene("A")
    h, w = cam.image_height, cam.image_width
    dL = scenes.grad_seed(w, h, 78).cuda()
    Ga = scenes.grad_seed(w, h, 79)[1].cuda()
    Gx = _seed(h, w)
    calls = []
    monkeypatch.setattr(dgr, "_distortion_probe", calls.append)
    out0, g0 = _run(sc, cam, PLAIN, dL=dL, Ga=Ga, fused=fused, distortion=False)
    assert calls == [] and "distortion" not in out0              # a call without the flag never reaches msgs_distortion_*
    # a loss that ignores the map: today's backward, bit for bit; only the forward replay ran
    out1, g1 = _run(sc, cam, PLAIN, dL=dL, Ga=Ga, fused=fused)
    assert calls == ["msgs_distortion_forward"]
    for k in OUT6:
        assert torch.equal(out0[k], out1[k]), k
    _equal_grads(g0, g1, "a loss without the distortion map")
    # a loss that uses it: the ordinary outputs are still the same bits
    del calls[:]
    out2, g2 = _run(sc, cam, PLAIN, Gx=Gx, dL=dL, Ga=Ga, fused=fused)
    assert calls == ["msgs_distortion_forward", "msgs_distortion_backward"]
    for k in OUT6:
        assert torch.equal(out0[k], out2[k]), k
    assert torch.equal(out1["distortion"].detach(), out2["distortion"].detach())
    assert not torch.equal(g2["xyz"], g0["xyz"])
    # with features too: the feature map keeps its bits and its place at the end
    feats = _features(sc.P, 5)
    o3, _ = _run(sc, cam, PLAIN, dL=dL, Ga=Ga, feats=feats, fused=fused, distortion=False)
    o4, _ = _run(sc, cam, PLAIN, dL=dL, Ga=Ga, feats=feats, fused=fused)
    assert torch.equal(o3["features"], o4["features"]) and torch.equal(o4["distortion"].detach(), out1["distortion"].detach())


def test_absgrad_does_not_include_the_distortion_share():
    from gaussian_renderer import _colour_inputs, _settings, _shape_inputs
    sc, cam = _scene_f()[:2]
    camd, bg = cam.to("cuda"), torch.zeros(3, device="cuda")
    dL, Gx = scenes.grad_seed(40, 24, 78).cuda(), _seed(24, 40)
    got = []
    for use in (False, True):
        pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
        r = dgr.GaussianRasterizer(_settings(camd, pc, PIPE, bg, 1.0, False, False, 1.0), absgrad=True).with_distortion()
        vs = torch.zeros_like(pc.get_xyz, requires_grad=True)
        outs = r(means3D=pc.get_xyz, means2D=vs, opacities=pc.get_opacity, **_colour_inputs(camd, pc, PIPE, None),
                 **_shape_inputs(pc, PIPE, 1.0))
        assert len(outs) == 6
        ((outs[0] * dL).sum() + ((outs[5] * Gx).sum() if use else 0.0)).backward()
        torch.cuda.synchronize()
        got.append((vs.absgrad.clone(), vs.grad.clone()))
    assert got[0][0].abs().max() > 0 and torch.equal(got[0][0], got[1][0]) and not torch.equal(got[0][1], got[1][1])


def test_host_entry_returns_the_render_dict_plus_distortion():
    from gaussian_renderer import RESULT_KEYS, render, render_with_distortion
    sc, cam = _scene_f()[:2]
    camd, bg = cam.to("cuda"), torch.tensor([0.2, 0.4, 0.1], device="cuda")
    for fused in (False, True):
        for alpha in (False, True):
            pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
            out = render_with_distortion(camd, pc, PIPE, bg, fused=fused, alpha=alpha, **PLAIN)
            assert set(out) == set(RESULT_KEYS) | {"distortion"} | ({"alpha"} if alpha else set())
            ref = _render(camd, SyntheticGaussians(sc, "cuda", requires_grad=True), bg, alpha=alpha, fused=fused)
            assert out["distortion"].shape == (24, 40) and torch.equal(out["distortion"], ref["distortion"])
            assert torch.equal(out["render"], ref["render"]) and (not alpha or torch.equal(out["alpha"], ref["alpha"]))
            plain = render(camd, SyntheticGaussians(sc, "cuda", requires_grad=True), PIPE, bg, **PLAIN)
            assert fused or torch.equal(out["render"], plain["render"])
            out["distortion"].mean().backward()
            assert pc._xyz.grad.abs().max() > 0
    with pytest.raises(ValueError, match="override_color"):
        render_with_distortion(camd, pc, PIPE, bg, override_color=torch.zeros(sc.P, 3, device="cuda"), fused=True)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. the camera
# ---------------------------------------------------------------------------------------------------------------------------
def test_camera_gradient_against_float64():
    """viewmatrix and projmatrix as float64 leaves of the truth's generator (autograd through oracle/torch_oracle.preprocess and
    the restated loop) against the op's camera gradients of the same loss; campos reaches the image through SH alone: zero"""
    gen = _generator()
    sc, cam = gen.scene("F")
    leaves = {}

    def edit(view):
        leaves["V"] = view["viewmatrix"].to(torch.float64).clone().requires_grad_(True)
        leaves["PM"] = view["projmatrix"].to(torch.float64).clone().requires_grad_(True)
        view["viewmatrix"], view["projmatrix"] = leaves["V"], leaves["PM"]
    r = gen.restated("F", view_edit=edit)
    G = gen.seed_map() * (~r["borderline"]).to(torch.float32)
    (r["dist"] * G.double()).sum().backward()
    names = {"V": "world_view_transform", "PM": "full_proj_transform", "cp": "camera_center"}
    c = copy.copy(cam.to("cuda"))
    for n in names.values():
        setattr(c, n, getattr(c, n).clone().requires_grad_(True))
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    out = _render(c, pc, torch.zeros(3, device="cuda"))
    (out["distortion"] * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert not c.camera_center.grad.any()
    for k in ("V", "PM"):
        got, ref = getattr(c, names[k]).grad.double().cpu().reshape(-1), leaves[k].grad.reshape(-1)
        e = ((got - ref).abs().max() / ref.abs().max()).item()
        report("distortion camera gradient vs float64", k, e)
        print(f"distortion camera gradient {k}: {e:.3e}")
        assert ref.abs().max() > 0 and e <= 2 * CAMERA_CEIL, (k, e)


# ---------------------------------------------------------------------------------------------------------------------------
# 9. the optimizer step inside the backward
# ---------------------------------------------------------------------------------------------------------------------------
def test_optimizer_in_backward_with_a_distortion_loss():
    """set_optimizer_in_backward on a fused render with a colour + distortion loss: parameters and both moments bit-identical
    to FusedAdam.step() after the plain backward of the same loss"""
    from train_epilogue import FusedAdam
    Wt, Ht = 160, 128
    sc, cam = small_scene(6007, Wt, Ht, 23, multiscale=True, scale_k=0.004 * 1920.0 / Wt * 0.2)
    dL, Gx = scenes.grad_seed(Wt, Ht, 78).cuda(), _seed(Ht, Wt)
    bg, camd = torch.zeros(3).cuda(), cam.to("cuda")
    a, b = SyntheticGaussians(sc, "cuda"), SyntheticGaussians(sc, "cuda")
    oa = FusedAdam(a.training_setup(7, sc.target_reso_lvl), lr=0.0, eps=1e-15)
    ob = FusedAdam(b.training_setup(7, sc.target_reso_lvl), lr=0.0, eps=1e-15)
    for it in range(3):
        taken = getattr(oa, "steps_in_backward", 0)
        prev = dgr.set_optimizer_in_backward(oa)
        try:
            pa = _render(camd, a, bg, MS, fused=True)
        finally:
            dgr.set_optimizer_in_backward(prev)
        ((pa["render"] * dL).sum() + (pa["distortion"] * Gx).sum()).backward()
        assert getattr(oa, "steps_in_backward", 0) == taken + 1
        pb = _render(camd, b, bg, MS, fused=True)
        ((pb["render"] * dL).sum() + (pb["distortion"] * Gx).sum()).backward()
        ob.step()
        ob.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        assert all(getattr(a, n).grad is None for n in a.LEAVES)
        assert pa["distortion"].abs().max() > 0 and torch.equal(pa["distortion"], pb["distortion"]), it
    for n in a.LEAVES:
        p, q = getattr(a, n), getattr(b, n)
        assert torch.equal(p, q), n
        sa, sb = oa.state[p], ob.state[q]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), n
        assert sa["exp_avg"].abs().max().item() > 0, n


# ---------------------------------------------------------------------------------------------------------------------------
# 10. guards
# ---------------------------------------------------------------------------------------------------------------------------
def test_no_gaussians_gives_a_zero_map_and_zero_gradients():
    rs = dgr.GaussianRasterizationSettings(24, 40, 0.5, 0.3, torch.tensor([0.2, 0.4, 0.1]).cuda(), 1.0, torch.eye(4).cuda(),
                                           torch.eye(4).cuda(), 3, torch.zeros(3).cuda(), False, False)
    z = lambda *s: torch.zeros(*s, device="cuda")
    m3, m2, f = z(0, 3).requires_grad_(), z(0, 3).requires_grad_(), z(0, 7).requires_grad_()
    out = dgr.GaussianRasterizer(rs, return_alpha=True).with_features(f).with_distortion()(
        means3D=m3, means2D=m2, opacities=z(0, 1), shs=z(0, 16, 3), scales=z(0, 3), rotations=z(0, 4))
    assert len(out) == 8 and out[5].shape == (24, 40) and out[6].shape == (24, 40) and out[7].shape == (7, 24, 40)
    assert not out[6].any()
    (out[6].sum() + out[0].sum()).backward()
    assert m3.grad.shape == (0, 3)


def test_an_empty_view_gives_a_zero_map():
    """a camera that looks away: Gaussians, but no instance — the forward zero-fills, the backward launches nothing"""
    sc, cam = _scene_f()[:2]
    sc = copy.copy(sc)
    sc.means3D = sc.means3D * torch.tensor([1.0, 1.0, -1.0])            # all behind the camera
    out, g = _run(sc, cam, Gx=_seed(24, 40), dL=scenes.grad_seed(40, 24, 78).cuda())
    assert not (out["radii"] > 0).any() and not out["distortion"].detach().any()
    assert not g["xyz"].any() and not g["opacity"].any()


def test_verification_mode_is_refused_before_any_launch(monkeypatch):
    sc, cam = _scene_f()[:2]
    camd, bg = cam.to("cuda"), torch.zeros(3, device="cuda")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    calls = []
    monkeypatch.setattr(dgr, "_distortion_probe", calls.append)
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
    dmap, mom = torch.full((24, 40), 7.0, device="cuda"), torch.full((24, 40), 7.0, device="cuda")
    G = _seed(24, 40)
    rec = torch.zeros(lib.msgs_backward_scratch_bytes(P), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(P=P, D=D, gb=None, o=dmap, m=mom):
        return lib.msgs_distortion_forward(ctx.call.view_ref, P, p(geom), geom.numel() if gb is None else gb, D, p(binning),
                                           binning.numel(), p(image), image.numel(), p(o), p(m), stream)

    def bwd(P=P, D=D, m=mom, g=G, r=rec, rb=None):
        return lib.msgs_distortion_backward(ctx.call.view_ref, P, p(geom), geom.numel(), D, p(binning), binning.numel(), p(image),
                                            image.numel(), p(m), p(g), p(r), rec.numel() if rb is None else rb, stream)
    assert fwd(P=-1) == -1 and fwd(o=None) == -1 and fwd(m=None) == -1 and fwd(gb=16) == -2
    assert bwd(P=-1) == -1 and bwd(m=None) == -1 and bwd(g=None) == -1 and bwd(r=None) == -1 and bwd(rb=rec.numel() - 1) == -2
    torch.cuda.synchronize()
    assert (dmap == 7.0).all() and (mom == 7.0).all() and not rec.any()             # refused calls wrote nothing
    prev = dgr.set_deterministic(True)
    try:
        assert fwd() == -1 and bwd() == -1                                          # not offered in the verification mode
    finally:
        dgr.set_deterministic(prev)
    # no instance: the forward zero-fills both maps, the backward launches nothing
    assert fwd(D=0) == 0 and bwd(D=0) == 0 and bwd(P=0) == 0
    torch.cuda.synchronize()
    assert not dmap.any() and not mom.any() and not rec.any()
    # the real call: the map of the Python layer; the records get slots 0..5 and 9, zeros elsewhere
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = _render(cam.to("cuda"), SyntheticGaussians(sc, "cuda", requires_grad=False), torch.zeros(3, device="cuda"))
    assert torch.equal(dmap, ref["distortion"]) and dmap.max() > 0
    slots = rec[:80 * P].view(torch.float64).view(P, 10)              # ten doubles per record (msgs_internal.h)
    assert not rec[80 * P:].any() and slots[:, :6].abs().max() > 0 and slots[:, 9].abs().max() > 0 and not slots[:, 6:9].any()

"""Feature channels on the GPU (SPEC M12; include/msgs.h msgs_features_forward / msgs_features_backward): per-Gaussian
vectors f_i [C] splatted with the blend weights w_ip = alpha_ip T_ip of the colour render, F[c,p] = sum_i f_ic w_ip over
background 0, with gradients to the features and — as C more colour channels — to the geometry and the camera.

Three references, none of them the kernels under test:
  1  float64, from oracle/torch_oracle.py alone: tests/golden/features_truth.npz (scene F, C = 5; generator and the CPU test that
     pins it: tests/golden/make_features_golden.py, tests/test_features_cpu.py).  Borderline pixels carry G = 0 on both sides and
     are left out of the map comparison.
  2  the op's own per-pixel decomposition: one backward of a plain render per pixel with dL/dC = e_0 gives w_ip.
  3  the colour route: the same model rendered with override_color triples over background 0, one backward per triple.
Tolerances are the project's own for quantities of the same kind (BWD_RTOL, TOL and LIN_TOL of tests/test_depth_grad_gpu.py); the
measured maxima are printed (pytest -s) and recorded in profiles/features_notes.md.  Then: channel blocks, never-read rows,
linearity, the forward routes, the untouched default path, the other modes and the guards.
The float64 truth here lives on one 3 x 2-tile picture; for the breadth (lists of several 256-entry batches, early termination,
filters with a fade, rigid poses, focal lengths, the scaling modifier, small models) see the seeded sweep of all opt-in outputs
against the same kind of truth: tests/test_replay_sweep_gpu.py, tests/replay_cases.py, tests/replay_truth.py."""
import contextlib
import copy
import os

import numpy as np
import pytest
import torch

import diff_gaussian_rasterization as dgr
import scenes
from parity_utils import BWD_RTOL, PIPE, check_backward, rel_err, report, small_scene
from route_utils import PLAIN, guesses_around, non_speculative, reset_forward_state, slab_stats
from synthetic_model import SyntheticGaussians
from test_absgrad_gpu import _scene_b, _scene_f
from test_alpha_grad_gpu import MS, _scene
from test_camera_grad_gpu import CEIL as CAMERA_CEIL
from test_depth_grad_gpu import LIN_TOL, ROUTES, TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CB = 8                      # channels per launch (blend.hip FEAT_CB): the sizes of test 4 straddle it
GRADS = ("xyz", "opacity", "scaling", "rotation", "viewspace", "dc", "rest")


@pytest.fixture(autouse=True)
def _reset_routes():
    yield
    dgr._C.lib.msgs_set_backward_generation(0)
    dgr._C.lib.msgs_set_blend_granularity(0)


def _set_route(route):
    gen, gran = ROUTES[route]
    dgr._C.lib.msgs_set_backward_generation(gen)
    dgr._C.lib.msgs_set_blend_granularity(gran)


@contextlib.contextmanager
def _env(env):
    """slab policy / occlusion switch of a view, restored afterwards; the forced routes are taken from the first call on"""
    prev_slab = dgr.slab_policy
    prev_occ = dgr._C.lib.msgs_set_occlusion(env["occlusion"]) if "occlusion" in env else None
    dgr.slab_policy = env.get("slab", prev_slab)
    reset_forward_state()
    try:
        yield
    finally:
        dgr.slab_policy = prev_slab
        if prev_occ is not None:
            dgr._C.lib.msgs_set_occlusion(prev_occ)


def _features(P, C, seed=91):
    """[P,C] float32 on the CPU, seeded, uniform in [0, 1)"""
    return torch.rand(P, C, generator=torch.Generator().manual_seed(seed))


def _seed_map(C, h, w, seed=92):
    """G = dL/dF [C,h,w] float32 on the GPU, seeded, uniform in (-0.5, 0.5)"""
    return (torch.rand(C, h, w, generator=torch.Generator().manual_seed(seed)) - 0.5).cuda()


def _render(cam, pc, bg, st=PLAIN, features=None, alpha=False, fused=False, override_color=None, smod=1.0, pipe=PIPE):
    """render() / render_fused() of the host layer with any of the opt-in outputs: the result dict plus "alpha" / "features" """
    from gaussian_renderer import RESULT_KEYS, _colour_inputs, _settings, _shape_inputs
    st = {**PLAIN, **st}
    settings = _settings(cam, pc, pipe, bg, smod, st["filter_small"], st["filter_large"], st["fade_size"])
    r = dgr.GaussianRasterizer(settings, return_alpha=alpha).with_features(features)
    kw = dict(max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes,
              occ_multiplier=pc.get_occ_multiplier, dc_delta=pc.get_dc_delta, base_mask=pc.get_base_mask)
    if fused:
        vs = torch.empty_like(pc._xyz, requires_grad=True)
        outs = r.forward_raw(pc._xyz, vs, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation, **kw)
    else:
        vs = torch.zeros_like(pc.get_xyz, requires_grad=True) + 0
        if vs.requires_grad:
            vs.retain_grad()
        outs = r(means3D=pc.get_xyz, means2D=vs, opacities=pc.get_opacity, **kw, **_colour_inputs(cam, pc, pipe, override_color),
                 **_shape_inputs(pc, pipe, smod))
    image, acc_ps, depth, radii, pixel_sizes = outs[:5]
    out = dict(zip(RESULT_KEYS, (image, acc_ps, depth, vs, radii > 0, radii, pixel_sizes)))
    rest = list(outs[5:])
    if alpha:
        out["alpha"] = rest.pop(0)
    if features is not None and features.numel() > 0:
        out["features"] = rest.pop(0)
    assert not rest
    return out


def _grads(pc, out):
    g = {"xyz": pc._xyz.grad, "opacity": pc._opacity.grad, "scaling": pc._scaling.grad, "rotation": pc._rotation.grad,
         "viewspace": out["viewspace_points"].grad, "dc": pc._features_dc.grad, "rest": pc._features_rest.grad}
    return {k: (v.detach().clone() if v is not None else None) for k, v in g.items()}


def _run(sc, cam, st=PLAIN, feats=None, G=None, dL=None, Gd=None, Ga=None, fused=False, smod=1.0, pipe=PIPE, bg=None):
    """one forward + backward on fresh leaves; the loss is the sum of the given seeds times their maps (G with feats [P,C] on the
    CPU or the GPU).  Returns (out, {name: grad}, dL/dfeatures or None, the feature leaf or None)"""
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    f = feats.detach().cuda().clone().requires_grad_(True) if feats is not None else None
    bg = torch.zeros(3, device="cuda") if bg is None else bg.cuda()
    out = _render(cam.to("cuda"), pc, bg, st, features=f, alpha=Ga is not None, fused=fused, smod=smod, pipe=pipe)
    loss = 0.0
    for seed, key in ((dL, "render"), (Gd, "depth"), (Ga, "alpha"), (G, "features")):
        if seed is not None:
            loss = loss + (out[key] * seed).sum()
    loss.backward()
    torch.cuda.synchronize()
    _run.last_pc = pc
    return out, _grads(pc, out), (f.grad.detach().clone() if f is not None and f.grad is not None else None), f


def _colour_route(sc, cam, st, feats, G, smod=1.0, pipe=PIPE):
    """the reference of test 3: ceil(C / 3) renders with override_color triples over background 0 and their backwards, summed.
    Returns (map [C,H,W], {name: summed grad}, dL/dfeatures [P,C])"""
    from gaussian_renderer import render
    P, C = feats.shape
    total, maps, dfeat = None, [], torch.zeros(P, C, device="cuda")
    for c0 in range(0, C, 3):
        n = min(3, C - c0)
        col = torch.zeros(P, 3, device="cuda")
        col[:, :n] = feats[:, c0:c0 + n].cuda()
        col.requires_grad_(True)
        pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
        out = render(cam.to("cuda"), pc, pipe, torch.zeros(3, device="cuda"), scaling_modifier=smod, override_color=col, **st)
        (out["render"][:n] * G[c0:c0 + n]).sum().backward()
        torch.cuda.synchronize()
        maps.append(out["render"][:n].detach())
        dfeat[:, c0:c0 + n] = col.grad[:, :n]
        g = _grads(pc, out)
        total = g if total is None else {k: (total[k] + g[k] if g[k] is not None else total[k]) for k in g}
    return torch.cat(maps, 0), total, dfeat


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-20)).item()


def _equal_grads(ga, gb, what):
    for k in GRADS:
        assert (ga[k] is None) == (gb[k] is None), (what, k)
        if ga[k] is not None:
            assert torch.equal(ga[k], gb[k]), (what, k)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. float64 truth, independent of the op
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def truth():
    t = np.load(os.path.join(ROOT, "tests", "golden", "features_truth.npz"))
    assert t["borderline"].sum() <= 0.02 * t["borderline"].size         # the condition of the masking (scene F: 1 of 960)
    return {k: torch.from_numpy(t[k]) for k in t.files}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("route", list(ROUTES))
def test_map_and_gradients_against_float64_truth(truth, route, fused):
    sc, cam = _scene_f()[:2]
    keep = ~truth["borderline"]
    _set_route(route)
    out, _, dfeat, _ = _run(sc, cam, feats=truth["features"], G=truth["G"].cuda(), fused=fused)
    F = out["features"].detach()
    assert F.shape == (5, 24, 40) and F.dtype == torch.float32 and out["features"].requires_grad
    assert torch.equal((out["radii"] > 0).cpu(), truth["visible"])
    name = f"features truth [{route}{', fused' if fused else ''}]"
    e = rel_err(F.cpu() * keep[None], truth["map"] * keep[None])
    report(name, "map rel err", e)
    assert e <= BWD_RTOL
    e = rel_err(dfeat, truth["dfeatures"])
    report(name, "dL/dfeatures rel err", e)
    assert e <= BWD_RTOL
    assert not dfeat[~truth["visible"].cuda()].any()
    pc = _run.last_pc
    check_backward(pc, out["viewspace_points"].grad, {k: truth[k] for k in ("means3D", "opacities", "scales", "rotations",
                                                                            "means2D")}, name)
    for k in ("_features_dc", "_features_rest"):
        assert getattr(pc, k).grad is None or not getattr(pc, k).grad.any(), k


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the op's own per-pixel decomposition
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["F", "deep"])
def test_map_against_per_pixel_backwards(kind):
    """one backward of a plain render per pixel with dL/dC = e_0: colors_precomp.grad[:, 0] is w_ip of that pixel, and
    sum_i f_ic w_ip in float64 is the map"""
    from gaussian_renderer import render
    sc, cam = _scene_b(kind)[:2]
    C = 5
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    P = pc.get_xyz.shape[0]
    feats = _features(P, C)
    col = torch.rand(P, 3, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_(True)
    img = render(cam.to("cuda"), pc, PIPE, torch.zeros(3, device="cuda"), override_color=col, **PLAIN)["render"]
    h, w = img.shape[1:]
    one = torch.zeros_like(img)
    f64 = feats.cuda().double()
    ref = torch.zeros(C, h, w, dtype=torch.float64, device="cuda")
    counted = torch.zeros(h, w, dtype=torch.bool, device="cuda")
    for y in range(h):
        for x in range(w):
            one[0, y, x] = 1.0
            g, = torch.autograd.grad(img, [col], one, retain_graph=True)
            wgt = g[:, 0].double()
            ref[:, y, x] = wgt @ f64
            counted[y, x] = (wgt != 0).any()
            one[0, y, x] = 0.0
    with torch.no_grad():
        F = _render(cam.to("cuda"), pc, torch.zeros(3, device="cuda"), features=feats.cuda())["features"]
    torch.cuda.synchronize()
    assert counted.any()
    e = rel_err(F, ref)
    report(f"features per-pixel decomposition [{kind}]", "map rel err", e)
    report(f"features per-pixel decomposition [{kind}]", "pixels without a counted pair", float((~counted).sum().item()))
    assert e <= BWD_RTOL
    assert not F[:, ~counted].any()                                  # exactly 0.0f where nothing was blended


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the colour route
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,C", [("A", 5), ("C", 5), ("S", 5), ("E", 5), ("A", 19), ("deep", 5)])
@pytest.mark.parametrize("route", list(ROUTES))
def test_gradients_equal_the_colour_route(kind, C, route):
    # "deep" (test_absgrad_gpu._scene_b): every tile list spans several staged batches, partial tiles in x and y
    sc, cam, st, smod, pipe, _ = _scene_b(kind)[:2] + ({}, 1.0, PIPE, {}) if kind == "deep" else _scene(kind)
    st = st or PLAIN
    h, w = cam.image_height, cam.image_width
    feats, G = _features(sc.P, C), _seed_map(C, h, w)
    _set_route(route)
    out, g, dfeat, _ = _run(sc, cam, st, feats, G, smod=smod, pipe=pipe)
    ref_map, gr, dref = _colour_route(sc, cam, st, feats, G, smod, pipe)
    name = f"features = colour route {kind}/C={C}/{route}"
    report(name, "max |map - render| (reported)", (out["features"].detach() - ref_map).abs().max().item())
    # the features are positive: the colour route's pixel is 0 in every channel exactly where nothing was blended — 0.0f here too
    empty = (ref_map == 0).all(0)
    assert empty.any() or kind not in ("S", "E")
    assert not out["features"].detach()[:, empty].any() and (out["features"].detach()[:, ~empty] != 0).any()
    for k, tol in TOL.items():
        assert g[k] is not None and g[k].abs().max() > 0, k
        e = _rel(g[k], gr[k])
        report(name, f"grad {k}", e)
        assert e <= tol, f"{name}: grad {k} rel err {e:.3e} > {tol}"
    e = _rel(dfeat, dref)
    report(name, "dL/dfeatures against override_color.grad", e)
    assert dref.abs().max() > 0 and e <= TOL["opacity"], f"{name}: dL/dfeatures rel err {e:.3e}"
    for k in ("dc", "rest"):                                   # the features carry no colour gradient
        assert g[k] is None or not g[k].any(), k


# ---------------------------------------------------------------------------------------------------------------------------
# 4. channel blocks
# ---------------------------------------------------------------------------------------------------------------------------
def test_channel_blocks_are_independent():
    """a channel's arithmetic is one FMA per pair in the forward and one product per pair in the backward, whatever its
    neighbours hold: the first k channels of a wide call are BIT-equal to a call with only those k"""
    sc, cam, st, *_ = _scene("S")
    st = st or PLAIN
    h, w = cam.image_height, cam.image_width
    wide = 2 * CB + 3
    feats, G = _features(sc.P, wide), _seed_map(wide, h, w)
    out, _, dwide, _ = _run(sc, cam, st, feats, G)
    Fwide = out["features"].detach()
    assert Fwide.abs().max() > 0 and dwide.abs().max() > 0
    for k in (1, CB - 1, CB, CB + 1, wide):
        o, _, d, _ = _run(sc, cam, st, feats[:, :k].contiguous(), G[:k].contiguous())
        assert torch.equal(o["features"].detach(), Fwide[:k]), k
        assert torch.equal(d, dwide[:, :k]), k
    # scalar row loads: C % 4 != 0, and C % 4 == 0 on a base that is 4-byte but not 16-byte aligned — the same values
    for k in (CB - 1, CB):
        store = torch.zeros(sc.P * k + 1, device="cuda")
        f = store[1:].view(sc.P, k)
        f.copy_(feats[:, :k])
        assert f.data_ptr() % 16 == 4 and f.is_contiguous()
        f.requires_grad_(True)
        pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
        o = _render(cam.to("cuda"), pc, torch.zeros(3, device="cuda"), st, features=f)
        (o["features"] * G[:k]).sum().backward()
        torch.cuda.synchronize()
        assert torch.equal(o["features"].detach(), Fwide[:k]), k
        assert torch.equal(f.grad, dwide[:, :k]), k


# ---------------------------------------------------------------------------------------------------------------------------
# 5. never-read rows
# ---------------------------------------------------------------------------------------------------------------------------
def test_rows_of_gaussians_in_no_list_are_never_read():
    sc, cam, st, *_ = _scene("C")
    h, w = cam.image_height, cam.image_width
    C = CB + 2
    feats, G = _features(sc.P, C), _seed_map(C, h, w)
    out0, g0, d0, _ = _run(sc, cam, st, feats, G)
    gone = (out0["radii"] == 0).cpu()
    assert gone.any() and not gone.all()
    zeros, nans = feats.clone(), feats.clone()
    zeros[gone], nans[gone] = 0.0, float("nan")
    outz, gz, dz, _ = _run(sc, cam, st, zeros, G)
    outn, gn, dn, _ = _run(sc, cam, st, nans, G)
    assert torch.isfinite(outn["features"]).all()
    assert torch.equal(outn["features"].detach(), outz["features"].detach())
    assert torch.equal(outn["features"].detach(), out0["features"].detach())
    assert torch.equal(dn, dz) and not dn[gone.cuda()].any()
    _equal_grads(gn, gz, "NaN rows")


# ---------------------------------------------------------------------------------------------------------------------------
# 6. linearity
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_colour_depth_alpha_features_is_linear(fused):
    sc, cam, st, smod, pipe, _ = _scene("C")
    h, w = cam.image_height, cam.image_width
    dL = scenes.grad_seed(w, h, 78).cuda()
    Gd = (scenes.grad_seed(w, h, 77)[0] * 0.1).cuda()
    Ga = scenes.grad_seed(w, h, 79)[1].cuda()
    C = 5
    feats, G = _features(sc.P, C), _seed_map(C, h, w)
    bg = torch.tensor([0.1, 0.2, 0.3])
    _, gc, _, _ = _run(sc, cam, st, dL=dL, fused=fused, bg=bg)
    _, gd, _, _ = _run(sc, cam, st, Gd=Gd, fused=fused, bg=bg)
    _, ga, _, _ = _run(sc, cam, st, Ga=Ga, fused=fused, bg=bg)
    _, gf, df, _ = _run(sc, cam, st, feats, G, fused=fused, bg=bg)
    _, gs, ds, _ = _run(sc, cam, st, feats, G, dL=dL, Gd=Gd, Ga=Ga, fused=fused, bg=bg)
    for k in GRADS:
        ref = sum(g[k] for g in (gc, gd, ga, gf) if g[k] is not None)
        e = _rel(gs[k], ref)
        report(f"features linearity fused={fused}", f"grad {k}", e)
        assert e <= LIN_TOL.get(k, 1e-6), f"grad {k} rel err {e:.3e}"
    assert torch.equal(ds, df)                                                     # dL/dfeatures depends on G alone
    assert gf["xyz"].abs().max() > 0 and _rel(gs["xyz"], gc["xyz"] + gd["xyz"] + ga["xyz"]) > 1e-4     # the features' share is in it


# ---------------------------------------------------------------------------------------------------------------------------
# 7. behind every forward route: the bits of the exact-buffer single pass
# ---------------------------------------------------------------------------------------------------------------------------
def _bits(sc, cam, st, feats, G, dL, fused=False):
    out, g, d, _ = _run(sc, cam, st, feats, G, dL=dL, fused=fused)
    return out, g, d


def _same_bits(a, b, what):
    (oa, ga, da), (ob, gb, db) = a, b
    assert oa["features"].abs().max() > 0 and da.abs().max() > 0, what
    assert torch.equal(oa["features"].detach(), ob["features"].detach()), (what, "map")
    assert torch.equal(da, db), (what, "dL/dfeatures")
    _equal_grads(ga, gb, what)


def test_two_runs_give_equal_bits():
    sc, cam, st, *_ = _scene("A")
    feats, G = _features(sc.P, CB + 3), _seed_map(CB + 3, 90, 150)
    dL = scenes.grad_seed(150, 90, 78).cuda()
    reset_forward_state()
    _same_bits(_bits(sc, cam, PLAIN, feats, G, dL), _bits(sc, cam, PLAIN, feats, G, dL), "two runs")


@pytest.mark.parametrize("fused", [False, True])
def test_features_behind_a_redone_stage2(fused):
    Wr, Hr = 320, 200
    sc, cam = small_scene(20000, Wr, Hr, seed=21)
    feats, G, dL = _features(sc.P, 5), _seed_map(5, Hr, Wr), scenes.grad_seed(Wr, Hr, 78).cuda()
    reset_forward_state()
    n0 = non_speculative()
    ref = _bits(sc, cam, PLAIN, feats, G, dL, fused)                        # first call: exact buffers
    assert non_speculative() == n0 + 1
    D = dgr._resolve(ref[0]["render"].grad_fn.state)[3]
    key = (torch.cuda.current_device(), sc.P, Wr, Hr, 0, 0)
    assert key in dgr._last_instances
    reset_forward_state()
    dgr._last_instances[key] = guesses_around(D)[0] // 2                    # its capacity is below D: the redo
    n0 = non_speculative()
    got = _bits(sc, cam, PLAIN, feats, G, dL, fused)
    assert non_speculative() == n0 + 1
    _same_bits(got, ref, "redo")
    n0 = non_speculative()
    got = _bits(sc, cam, PLAIN, feats, G, dL, fused)                        # ... and the speculative stage 2 that stands
    assert non_speculative() == n0
    _same_bits(got, ref, "speculative")


def test_features_in_forced_slabs():
    from test_slab_gpu import _dense_scene
    Ws, Hs = 960, 720
    sc, cam = _dense_scene(80_000, Ws, Hs, 9, opacity=(0.5, 0.99)), scenes.front_camera(Ws, Hs)
    feats, G, dL = _features(sc.P, 5), _seed_map(5, Hs, Ws), scenes.grad_seed(Ws, Hs, 78).cuda()
    got = {}
    for policy in ("never", "0.12"):
        with _env({"slab": policy}):
            got[policy] = _bits(sc, cam, PLAIN, feats, G, dL)
            assert slab_stats(got[policy][0]["render"].grad_fn)["active"] == (policy != "never")
    _same_bits(got["0.12"], got["never"], "slab 0.12 vs never")


def test_features_behind_the_occlusion_cut_off():
    from test_occlusion_gpu import _giants_scene, _stats
    Wo, Ho = 420, 300
    sc, cam = _giants_scene(2500, Wo, Ho, 5, 60, giant_scale=1.2, giant_opacity=0.9), scenes.front_camera(Wo, Ho)
    feats, G, dL = _features(sc.P, 5), _seed_map(5, Ho, Wo), scenes.grad_seed(Wo, Ho, 78).cuda()
    got = {}
    for occ in (0, 1):
        with _env({"occlusion": occ}):
            got[occ] = _bits(sc, cam, PLAIN, feats, G, dL)
            if occ:
                assert _stats(got[occ][0]["render"].grad_fn)["closed_blocks"] > 0
    _same_bits(got[1], got[0], "occlusion cut-off on vs off")


def test_features_with_two_views_in_flight():
    """inside deferred_forward a call with features resolves its own view before the replay: the serial bits"""
    Wv, Hv, nv = 320, 200, 2
    sc = scenes.ball_scene(20000, seed=46, log_s=-3.0)
    cams = [scenes.ring_camera(v, 4, Wv, Hv).to("cuda") for v in range(nv)]
    feats, G, dL = _features(sc.P, 5), _seed_map(5, Hv, Wv), scenes.grad_seed(Wv, Hv, 78).cuda()
    bg = torch.zeros(3, device="cuda")
    reset_forward_state()
    serial = [_bits(sc, cam, PLAIN, feats, G, dL) for cam in cams]
    reset_forward_state()
    pcs = [SyntheticGaussians(sc, "cuda", requires_grad=True) for _ in cams]
    fs = [feats.cuda().clone().requires_grad_(True) for _ in cams]
    with dgr.deferred_forward() as pending:
        outs = [_render(cam, pc, bg, features=f) for cam, pc, f in zip(cams, pcs, fs)]
        assert len(pending) == nv
    for o, pc, f, ref in zip(outs, pcs, fs, serial):
        ((o["features"] * G).sum() + (o["render"] * dL).sum()).backward()
        torch.cuda.synchronize()
        _same_bits((o, _grads(pc, o), f.grad), ref, "deferred")


# ---------------------------------------------------------------------------------------------------------------------------
# 8. nothing else moves
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True])
def test_default_path_is_untouched(fused, monkeypatch):
    sc, cam, st, *_ = _scene("A")
    h, w = cam.image_height, cam.image_width
    feats, G = _features(sc.P, 5), _seed_map(5, h, w)
    dL = scenes.grad_seed(w, h, 78).cuda()
    Ga = scenes.grad_seed(w, h, 79)[1].cuda()
    calls = []
    monkeypatch.setattr(dgr, "_features_probe", calls.append)
    out0, g0, _, _ = _run(sc, cam, PLAIN, dL=dL, Ga=Ga, fused=fused)
    assert calls == [] and "features" not in out0                       # a call without features never reaches msgs_features_*
    # a loss that ignores the feature map: today's backward, bit for bit; only the forward replay ran
    out1, g1, d1, f1 = _run(sc, cam, PLAIN, feats, None, dL=dL, Ga=Ga, fused=fused)
    assert calls == ["msgs_features_forward"] and d1 is None
    for k in ("render", "acc_pixel_size", "depth", "radii", "pixel_sizes", "alpha"):
        assert torch.equal(out0[k], out1[k]), k
    _equal_grads(g0, g1, "a loss without the feature map")
    # a loss that uses it: the ordinary outputs are still the same bits
    del calls[:]
    out2, g2, d2, _ = _run(sc, cam, PLAIN, feats, G, dL=dL, Ga=Ga, fused=fused)
    assert calls == ["msgs_features_forward", "msgs_features_backward"]
    for k in ("render", "acc_pixel_size", "depth", "radii", "pixel_sizes", "alpha"):
        assert torch.equal(out0[k], out2[k]), k
    assert torch.equal(out1["features"].detach(), out2["features"].detach())
    assert d2.abs().max() > 0 and not torch.equal(g2["xyz"], g0["xyz"])


def test_host_entry_returns_the_render_dict_plus_features():
    from gaussian_renderer import RESULT_KEYS, render, render_with_features
    sc, cam = _scene_f()[:2]
    camd, bg = cam.to("cuda"), torch.tensor([0.2, 0.4, 0.1], device="cuda")
    feats = _features(sc.P, 5).cuda()
    for fused in (False, True):
        pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
        out = render_with_features(camd, pc, PIPE, bg, feats, fused=fused, **PLAIN)
        assert set(out) == set(RESULT_KEYS) | {"features"}
        ref = _render(camd, SyntheticGaussians(sc, "cuda", requires_grad=True), bg, features=feats, fused=fused)
        assert torch.equal(out["features"], ref["features"]) and torch.equal(out["render"], ref["render"])
        plain = render(camd, SyntheticGaussians(sc, "cuda", requires_grad=True), PIPE, bg, **PLAIN)
        assert fused or torch.equal(out["render"], plain["render"])
    with pytest.raises(ValueError, match="override_color"):
        render_with_features(camd, pc, PIPE, bg, feats, override_color=torch.zeros(sc.P, 3, device="cuda"), fused=True)


# ---------------------------------------------------------------------------------------------------------------------------
# 9. other modes
# ---------------------------------------------------------------------------------------------------------------------------
def test_retain_graph_gives_the_same_gradients_twice():
    sc, cam, st, *_ = _scene("A")
    feats, G = _features(sc.P, 5), _seed_map(5, 90, 150)
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    f = feats.cuda().requires_grad_(True)
    out = _render(cam.to("cuda"), pc, torch.zeros(3, device="cuda"), features=f)
    loss = (out["features"] * G).sum()
    loss.backward(retain_graph=True)
    torch.cuda.synchronize()
    g1, d1 = _grads(pc, out), f.grad.clone()
    for t in [f, out["viewspace_points"]] + [getattr(pc, n) for n in pc.LEAVES]:
        t.grad = None
    loss.backward()
    torch.cuda.synchronize()
    assert d1.abs().max() > 0 and torch.equal(f.grad, d1)
    _equal_grads(_grads(pc, out), g1, "second backward through the retained graph")


def test_camera_gradient_against_the_colour_route():
    sc, cam, st, *_ = _scene("A")
    C = 5
    feats, G = _features(sc.P, C), _seed_map(C, 90, 150)
    names = ("world_view_transform", "full_proj_transform", "camera_center")

    def leaf_camera():
        c = copy.copy(cam.to("cuda"))
        for n in names:
            setattr(c, n, getattr(c, n).clone().requires_grad_(True))
        return c
    c = leaf_camera()
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    out = _render(c, pc, torch.zeros(3, device="cuda"), features=feats.cuda())
    (out["features"] * G).sum().backward()
    got = [getattr(c, n).grad.clone() for n in names]
    ref = [torch.zeros_like(g) for g in got]
    for c0 in range(0, C, 3):
        n = min(3, C - c0)
        col = torch.zeros(sc.P, 3, device="cuda")
        col[:, :n] = feats[:, c0:c0 + n].cuda()
        c2 = leaf_camera()
        o = _render(c2, SyntheticGaussians(sc, "cuda", requires_grad=True), torch.zeros(3, device="cuda"), override_color=col)
        (o["render"][:n] * G[c0:c0 + n]).sum().backward()
        ref = [r + getattr(c2, k).grad for r, k in zip(ref, names)]
    torch.cuda.synchronize()
    # both sides are float32 evaluations of the same sum, each held to CEIL of the float64 truth by tests/test_camera_grad_gpu.py:
    # they differ by at most twice that
    for k, a, b in zip(names, got, ref):
        if k == "camera_center":        # the camera position reaches the image through the SH colours alone: nothing here
            assert not a.any() and not b.any()
            continue
        e = _rel(a, b)
        report("features camera gradient = colour route", k, e)
        assert b.abs().max() > 0 and e <= 2 * CAMERA_CEIL, (k, e)


def test_optimizer_in_backward_with_a_feature_loss():
    """set_optimizer_in_backward on a fused render with a colour + feature loss: parameters and both moments bit-identical to
    FusedAdam.step() after the plain backward of the same loss"""
    from train_epilogue import FusedAdam
    Wt, Ht = 160, 128
    sc, cam = small_scene(6007, Wt, Ht, 23, multiscale=True, scale_k=0.004 * 1920.0 / Wt * 0.2)
    dL = scenes.grad_seed(Wt, Ht, 78).cuda()
    feats, G = _features(sc.P, 5).cuda(), _seed_map(5, Ht, Wt)
    bg, camd = torch.zeros(3).cuda(), cam.to("cuda")
    a, b = SyntheticGaussians(sc, "cuda"), SyntheticGaussians(sc, "cuda")
    oa = FusedAdam(a.training_setup(7, sc.target_reso_lvl), lr=0.0, eps=1e-15)
    ob = FusedAdam(b.training_setup(7, sc.target_reso_lvl), lr=0.0, eps=1e-15)
    fa, fb = feats.clone().requires_grad_(True), feats.clone().requires_grad_(True)
    for it in range(3):
        taken = getattr(oa, "steps_in_backward", 0)
        prev = dgr.set_optimizer_in_backward(oa)
        try:
            pa = _render(camd, a, bg, MS, features=fa, fused=True)
        finally:
            dgr.set_optimizer_in_backward(prev)
        ((pa["render"] * dL).sum() + (pa["features"] * G).sum()).backward()
        assert getattr(oa, "steps_in_backward", 0) == taken + 1
        pb = _render(camd, b, bg, MS, features=fb, fused=True)
        ((pb["render"] * dL).sum() + (pb["features"] * G).sum()).backward()
        ob.step()
        ob.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        assert all(getattr(a, n).grad is None for n in a.LEAVES)
        assert torch.equal(pa["features"], pb["features"]), it
    assert fa.grad.abs().max() > 0 and torch.equal(fa.grad, fb.grad)
    for n in a.LEAVES:
        p, q = getattr(a, n), getattr(b, n)
        assert torch.equal(p, q), n
        sa, sb = oa.state[p], ob.state[q]
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), n
        assert sa["exp_avg"].abs().max().item() > 0, n


def test_no_grad_forward_and_frozen_geometry():
    sc, cam = _scene_f()[:2]
    feats, G = _features(sc.P, 5), _seed_map(5, 24, 40)
    ref, _, dref, _ = _run(sc, cam, PLAIN, feats, G)
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    with torch.no_grad():
        out = _render(cam.to("cuda"), pc, torch.zeros(3, device="cuda"), features=feats.cuda().requires_grad_(True))
    assert not out["features"].requires_grad and torch.equal(out["features"], ref["features"].detach())
    # frozen geometry (feature distillation): only the features want a gradient — the replay without the geometry share
    f = feats.cuda().requires_grad_(True)
    out = _render(cam.to("cuda"), pc, torch.zeros(3, device="cuda"), features=f)
    (out["features"] * G).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(out["features"].detach(), ref["features"].detach()) and torch.equal(f.grad, dref)
    # a float64 leaf receives its gradient in its own dtype and shape
    f64 = feats.double().cuda().requires_grad_(True)
    out = _render(cam.to("cuda"), pc, torch.zeros(3, device="cuda"), features=f64)
    (out["features"] * G).sum().backward()
    assert f64.grad.dtype == torch.float64 and f64.grad.shape == (sc.P, 5) and torch.equal(f64.grad.float(), dref)


def test_no_gaussians_gives_a_zero_map_and_zero_gradients():
    rs = dgr.GaussianRasterizationSettings(24, 40, 0.5, 0.3, torch.tensor([0.2, 0.4, 0.1]).cuda(), 1.0, torch.eye(4).cuda(),
                                           torch.eye(4).cuda(), 3, torch.zeros(3).cuda(), False, False)
    z = lambda *s: torch.zeros(*s, device="cuda")
    m3, m2, f = z(0, 3).requires_grad_(), z(0, 3).requires_grad_(), z(0, 7).requires_grad_()
    out = dgr.GaussianRasterizer(rs, return_alpha=True).with_features(f)(
        means3D=m3, means2D=m2, opacities=z(0, 1), shs=z(0, 16, 3), scales=z(0, 3), rotations=z(0, 4))
    assert len(out) == 7 and out[5].shape == (24, 40) and out[6].shape == (7, 24, 40) and not out[6].any()
    (out[6].sum() + out[0].sum()).backward()
    assert f.grad.shape == (0, 7) and m3.grad.shape == (0, 3)


# ---------------------------------------------------------------------------------------------------------------------------
# 10. guards
# ---------------------------------------------------------------------------------------------------------------------------
def test_guards_raise_before_any_launch(monkeypatch):
    sc, cam = _scene_f()[:2]
    camd, bg = cam.to("cuda"), torch.zeros(3, device="cuda")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    calls = []
    monkeypatch.setattr(dgr, "_features_probe", calls.append)
    before = dgr.forward_stats["forwards"]
    for fused in (False, True):
        for bad in (torch.zeros(sc.P + 1, 5, device="cuda"), torch.zeros(sc.P - 1, 5, device="cuda"),
                    torch.zeros(sc.P, 5, 1, device="cuda"), torch.zeros(sc.P * 5, device="cuda")):
            with pytest.raises(ValueError, match="features"):
                _render(camd, pc, bg, features=bad, fused=fused)
        with pytest.raises(RuntimeError, match="HIP device"):
            _render(camd, pc, bg, features=torch.zeros(sc.P, 5), fused=fused)
        prev = dgr.set_deterministic(True)
        try:
            with pytest.raises(ValueError, match="verification mode"):
                _render(camd, pc, bg, features=torch.zeros(sc.P, 5, device="cuda"), fused=fused)
        finally:
            dgr.set_deterministic(prev)
    assert dgr.forward_stats["forwards"] == before and calls == []
    # an empty tensor means none: the reference's five outputs, no replay
    for empty in (torch.Tensor([]), torch.zeros(0, 5, device="cuda"), None):
        out = _render(camd, pc, bg, features=empty)
        assert "features" not in out
    assert calls == []


def test_c_entries_check_capacity_and_arguments():
    import ctypes as C
    from gaussian_renderer import render
    sc, cam = _scene_f()[:2]
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    out = render(cam.to("cuda"), pc, PIPE, torch.zeros(3, device="cuda"), **PLAIN)
    ctx = out["render"].grad_fn
    geom, binning, image, D = dgr._resolve(ctx.state)
    lib, P, Cn = dgr._C.lib, sc.P, 5
    f = _features(P, Cn).cuda()
    fmap = torch.full((Cn, 24, 40), 7.0, device="cuda")
    G = _seed_map(Cn, 24, 40)
    dfeat = torch.full((P, Cn), 7.0, device="cuda")
    scratch = torch.empty(lib.msgs_features_scratch_bytes(P, Cn), dtype=torch.uint8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd(P=P, D=D, g=geom, gb=None, feats=f, Cn=Cn, o=fmap):
        return lib.msgs_features_forward(ctx.call.view_ref, P, p(g), g.numel() if gb is None else gb, D, p(binning),
                                         binning.numel(), p(image), image.numel(), p(feats), Cn, p(o), stream)

    def bwd(P=P, D=D, sb=None, feats=f, Cn=Cn, s=scratch, o=dfeat, rec=None, rb=0):
        return lib.msgs_features_backward(ctx.call.view_ref, P, p(geom), geom.numel(), D, p(binning), binning.numel(), p(image),
                                          image.numel(), p(feats), Cn, p(G), p(rec), rb, p(s),
                                          s.numel() if sb is None else sb, p(o), stream)
    assert fwd(P=-1) == -1 and fwd(Cn=0) == -1 and fwd(o=None) == -1 and fwd(feats=None) == -1 and fwd(gb=16) == -2
    assert bwd(P=-1) == -1 and bwd(Cn=0) == -1 and bwd(o=None) == -1 and bwd(feats=None) == -1 and bwd(sb=8) == -2
    rec = torch.zeros(lib.msgs_backward_scratch_bytes(P), dtype=torch.uint8, device="cuda")
    assert bwd(rec=rec, rb=rec.numel() - 1) == -2
    torch.cuda.synchronize()
    assert (fmap == 7.0).all() and (dfeat == 7.0).all() and not rec.any()           # refused calls wrote nothing
    # no instance: the forward zero-fills the map, the backward zero-fills dL/dfeatures, no replay runs
    assert fwd(D=0) == 0 and bwd(D=0) == 0
    torch.cuda.synchronize()
    assert not fmap.any() and not dfeat.any()
    # the real call: the map of the Python layer; the geometry share lands in the records' slots 0..5 only
    assert fwd() == 0 and bwd(rec=rec, rb=rec.numel()) == 0
    torch.cuda.synchronize()
    with torch.no_grad():
        ref = _render(cam.to("cuda"), SyntheticGaussians(sc, "cuda", requires_grad=False), torch.zeros(3, device="cuda"),
                      features=f)["features"]
    assert torch.equal(fmap, ref) and dfeat.abs().max() > 0
    slots = rec[:80 * P].view(torch.float64).view(P, 10)              # ten doubles per record (msgs_internal.h)
    assert not rec[80 * P:].any() and slots[:, :6].abs().max() > 0 and not slots[:, 6:].any()

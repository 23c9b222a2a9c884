"""Antialiasing on the GPU (SPEC M14; include/msgs.h msgs_screen_compensation_*): o_eff = o rho in front of K1,
and the definition "an antialiased render is the plain render of the same model with o_eff in the place of the opacity".

References, none of them the kernels under test:
  1  float64 autograd through oracle/torch_oracle.py's preprocess: tests/antialias_truth.py (pinned by
     tests/test_antialias_cpu.py) — o_eff, every gradient of the op, the view matrix's included;
  2  the plain GaussianRasterizer fed screen_compensation(...): bit-equal outputs, equal gradients;
  3  end to end, torch_oracle.rasterize fed o rho64 in float64, dL/dC zero on the oracle's borderline pixels.
Tolerances are the project's own: FWD_ATOL, BWD_RTOL, CEIL of tests/test_camera_grad_gpu.py, the 2 % cap on masked pixels of
tests/test_distortion_gpu.py.  The measured maxima are printed (pytest -s) and recorded in profiles/antialias_notes.md."""
import functools
import math

import pytest
import torch

import antialias_truth as at
import diff_gaussian_rasterization as dgr
import scenes
from oracle import torch_oracle as to
from parity_utils import BWD_RTOL, FWD_ATOL, PIPE, rel_err, report, small_scene
from route_utils import PLAIN, non_speculative, reset_forward_state
from synthetic_model import SyntheticGaussians
from test_alpha_grad_gpu import _scene as _alpha_scene
from test_camera_grad_gpu import CEIL as CAMERA_CEIL
from test_features_gpu import _features, _seed_map

pytestmark = pytest.mark.gpu

OP_SCENES = ("S1", "S2", "S3", "S1:1", "S1:257")
GEOMETRY = ("means3D", "scales", "rotations", "cov3D_precomp")


@functools.lru_cache(maxsize=None)
def _truth(name, smod, precomp):
    sc, cam = at.scene(name)
    return sc, cam, at.seed(sc.P), at.truth(sc, cam, at.seed(sc.P), smod, precomp, camera=True)


def _settings(cam, smod=1.0, st=PLAIN, bg=None, sh_degree=0):
    """the raster settings of gaussian_renderer._settings for a camera whose tensors are already where they should be"""
    bg = torch.zeros(3, device="cuda") if bg is None else bg
    return dgr.GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(0.5 * cam.FoVx),
        tanfovy=math.tan(0.5 * cam.FoVy), bg=bg, scale_modifier=smod, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=sh_degree, campos=cam.camera_center, prefiltered=False, debug=False, **st)


def _op(name, smod, precomp, camera=True):
    """screen_compensation on fresh leaves + the backward of sum g o_eff: (o_eff, {name: grad}, leaves, truth)"""
    sc, cam, g, t = _truth(name, smod, precomp)
    leaf = lambda x: x.detach().cuda().clone().requires_grad_(True)
    c = cam.to("cuda")
    L = dict(means3D=leaf(sc.means3D), opacities=leaf(sc.opacities))
    if camera:
        c.world_view_transform = L["viewmatrix"] = leaf(cam.world_view_transform)
        c.full_proj_transform = L["projmatrix"] = leaf(cam.full_proj_transform)
        c.camera_center = L["campos"] = leaf(cam.camera_center)
    if precomp:
        L["cov3D_precomp"] = leaf(t["cov3D_input"])
        shape = dict(cov3D_precomp=L["cov3D_precomp"])
    else:
        L["scales"], L["rotations"] = leaf(sc.scales), leaf(sc.rotations)
        shape = dict(scales=L["scales"], rotations=L["rotations"])
    o_eff = dgr.screen_compensation(L["means3D"], L["opacities"], _settings(c, smod), **shape)
    (o_eff * g.cuda()).sum().backward()
    torch.cuda.synchronize()
    return o_eff.detach(), {k: (v.grad.detach().clone() if v.grad is not None else None) for k, v in L.items()}, L, t


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2. the op against float64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smod", [1.0, 0.7])
@pytest.mark.parametrize("precomp", [False, True], ids=["scales+rotations", "cov3D_precomp"])
@pytest.mark.parametrize("name", OP_SCENES)
def test_o_eff_and_gradients_against_float64(name, precomp, smod):
    o_eff, g, L, t = _op(name, smod, precomp)
    sc, _, seed, _ = _truth(name, smod, precomp)
    what = f"antialias op {name} [{'cov3D_precomp' if precomp else 'scales+rotations'}, scale_modifier {smod}]"
    assert o_eff.shape == sc.opacities.shape and o_eff.dtype == torch.float32 and o_eff.is_cuda
    e = (o_eff.cpu().double().reshape(-1) - t["o_eff"]).abs().max().item()
    report(what, "o_eff max abs err", e)
    assert e <= FWD_ATOL
    skipped = ~t["regular"]
    assert torch.equal(o_eff.cpu()[skipped], sc.opacities[skipped])                 # rho = 1 exactly: the opacity's bits
    errs = {"opacities": rel_err(g["opacities"], t["opacities"])}
    for k in GEOMETRY:
        if k in L:
            errs[k] = rel_err(g[k], t[k])
    for k, v in errs.items():
        report(what, f"grad {k} max-norm rel err", v)
    for k, v in errs.items():
        assert v <= BWD_RTOL, (what, k, v)
    # the camera: the view matrix in M8's flat convention (column 3 never enters); nothing else of it enters rho
    ref = t["viewmatrix"]
    ev = (g["viewmatrix"].cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    report(what, "grad viewmatrix max|g - g64| / max|g64|", ev)
    assert ev <= CAMERA_CEIL, (what, ev)
    assert g["viewmatrix"].shape == (4, 4) and torch.all(g["viewmatrix"][:, 3] == 0)
    assert g["projmatrix"] is None and g["campos"] is None
    # rows without a geometry gradient: behind the near plane, and on the floor — exactly zero, and dL/do = rho g
    flat = t["floored"] | skipped
    for k in GEOMETRY:
        if k in L:
            assert not g[k].cpu()[flat].any(), (what, k)
    go = g["opacities"].cpu().reshape(-1)
    assert torch.equal(go[skipped], seed.reshape(-1)[skipped])
    floor32 = torch.sqrt(torch.tensor(at.FLOOR, dtype=torch.float32))
    assert torch.equal(go[t["floored"]], (floor32 * seed.reshape(-1))[t["floored"]])
    if name == "S2":                                                                # (a smaller scale_modifier floors more rows)
        assert int(t["floored"].sum()) == (2 if smod == 1.0 else 6)
    if name == "S1":
        assert int(skipped.sum()) == 3


@pytest.mark.parametrize("precomp", [False, True], ids=["scales+rotations", "cov3D_precomp"])
def test_two_runs_give_equal_bits(precomp):
    a, ga, _, _ = _op("S1", 1.0, precomp)
    b, gb, _, _ = _op("S1", 1.0, precomp)
    assert torch.equal(a, b)
    for k in ga:
        assert (ga[k] is None) == (gb[k] is None) and (ga[k] is None or torch.equal(ga[k], gb[k])), k
    assert ga["viewmatrix"].abs().max() > 0


def test_camera_without_grad_gets_none_and_the_same_gaussian_gradients():
    _, ga, _, _ = _op("S1", 1.0, False, camera=True)
    _, gb, L, _ = _op("S1", 1.0, False, camera=False)
    assert "viewmatrix" not in L
    for k in ("means3D", "opacities", "scales", "rotations"):
        assert torch.equal(ga[k], gb[k]), k


def test_no_gaussians():
    cam = scenes.front_camera(40, 24).to("cuda")
    z = lambda *s: torch.zeros(*s, device="cuda", requires_grad=True)
    m, o, s, q = z(0, 3), z(0, 1), z(0, 3), z(0, 4)
    out = dgr.screen_compensation(m, o, _settings(cam), scales=s, rotations=q)
    assert out.shape == (0, 1)
    out.sum().backward()
    assert m.grad.shape == (0, 3) and o.grad.shape == (0, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the definition: with_antialiasing() == the plain rasterizer fed screen_compensation(...)
# ---------------------------------------------------------------------------------------------------------------------------
LEAVES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


def _render(sc, cam, how, st=PLAIN, extras=False, smod=1.0, pipe=PIPE, loss=True):
    """one render (+ backward) on fresh leaves.  how: "module" = with_antialiasing(), "fed" = the plain module fed
    screen_compensation(...), "plain" = no antialiasing.  extras: alpha, distortion and a C = 5 feature map as well.
    Returns (outputs, {leaf: grad})"""
    from gaussian_renderer import _colour_inputs, _shape_inputs
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    c = cam.to("cuda")
    H, W = c.image_height, c.image_width
    settings = _settings(c, smod, {**PLAIN, **st}, torch.tensor([0.1, 0.2, 0.3], device="cuda"), pc.active_sh_degree)
    feats = _features(sc.P, 5).cuda().requires_grad_(True) if extras else None
    r = dgr.GaussianRasterizer(settings, return_alpha=extras).with_features(feats).with_distortion(extras)
    shape = _shape_inputs(pc, pipe, smod)
    opac = pc.get_opacity
    if how == "module":
        r = r.with_antialiasing()
    elif how == "fed":
        opac = dgr.screen_compensation(pc.get_xyz, opac, settings, **shape)
    vs = torch.zeros_like(pc.get_xyz, requires_grad=True) + 0
    vs.retain_grad()
    outs = r(means3D=pc.get_xyz, means2D=vs, opacities=opac, max_pixel_sizes=pc.get_max_pixel_sizes,
             min_pixel_sizes=pc.get_min_pixel_sizes, occ_multiplier=pc.get_occ_multiplier, dc_delta=pc.get_dc_delta,
             base_mask=pc.get_base_mask, **_colour_inputs(c, pc, pipe, None), **shape)
    assert len(outs) == (8 if extras else 5)
    grads = {}
    if loss:
        total = (outs[0] * scenes.grad_seed(W, H, 78).cuda()).sum() + (outs[2] * scenes.grad_seed(W, H, 77)[0].cuda() * 0.1).sum()
        if extras:
            total = total + (outs[5] * scenes.grad_seed(W, H, 79)[1].cuda()).sum() + \
                (outs[6] * (_seed_map(1, H, W, 131)[0])).sum() + (outs[7] * _seed_map(5, H, W)).sum()
        total.backward()
        grads = {n: getattr(pc, n).grad.detach().clone() for n in LEAVES}
        grads["viewspace"] = vs.grad.detach().clone()
        if extras:
            grads["features"] = feats.grad.detach().clone()
    torch.cuda.synchronize()
    return tuple(o.detach() for o in outs), grads


def _same(a, b, what, plain=None):
    (oa, ga), (ob, gb) = a, b
    for i, (x, y) in enumerate(zip(oa, ob)):
        assert torch.equal(x, y), (what, "output", i)
    worst = 0.0
    for k in ga:
        e = rel_err(ga[k], gb[k])
        worst = max(worst, e)
        assert e <= 1e-6, (what, k, e)
    report(what, "with_antialiasing() vs the plain module fed o_eff: worst leaf gradient rel err", worst)
    if plain is not None:                                                          # ... and it is not the unfiltered render
        assert (oa[0] - plain[0][0]).abs().max() > 1e-3, what


@pytest.mark.parametrize("extras", [False, True], ids=["five outputs", "alpha+distortion+features"])
@pytest.mark.parametrize("name", ["S1", "S2q"])
def test_definition(name, extras):
    sc, cam = at.scene(name)
    _same(_render(sc, cam, "module", extras=extras), _render(sc, cam, "fed", extras=extras), f"definition {name}",
          _render(sc, cam, "plain", extras=extras, loss=False))


def test_definition_with_cov3D_precomp_and_scale_modifier():
    import types
    sc, cam = at.scene("S1")
    pipe = types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=True, debug=False)
    _same(_render(sc, cam, "module", smod=0.7, pipe=pipe), _render(sc, cam, "fed", smod=0.7, pipe=pipe), "definition cov3D")


def test_definition_under_the_multi_scale_filters():
    sc, cam = _alpha_scene("C")[:2]
    st = dict(filter_small=True, filter_large=True, fade_size=1.0)
    a, b, p = _render(sc, cam, "module", st), _render(sc, cam, "fed", st), _render(sc, cam, "plain", st, loss=False)
    _same(a, b, "definition, filters on", p)
    # pixel_sizes (M1) see the compensated opacity
    assert not torch.equal(a[0][4], p[0][4])


def test_definition_on_the_first_call_and_the_speculative_route():
    sc, cam = small_scene(20000, 320, 200, seed=21)
    got = {}
    for how in ("module", "fed"):
        reset_forward_state()
        n0 = non_speculative()
        got[how, "first"] = _render(sc, cam, how)                                   # first call: exact buffers
        assert non_speculative() == n0 + 1
        got[how, "speculative"] = _render(sc, cam, how)                             # the speculative stage 2 that stands
        assert non_speculative() == n0 + 1
    _same(got["module", "first"], got["fed", "first"], "definition, first call")
    _same(got["module", "speculative"], got["fed", "speculative"], "definition, speculative")
    _same(got["module", "first"], got["module", "speculative"], "first call vs speculative")


def test_no_chained_mode_and_no_warning_under_antialiasing(recwarn):
    """the reference's getters are recognised by the plain module (chained mode); with_antialiasing() goes straight to the
    plain route and does not warn"""
    sc, cam = at.scene("S1")
    prev, dgr._warned_chain[0] = dgr._warned_chain[0], False
    try:
        outs, _ = _render(sc, cam, "module")
        assert not dgr._warned_chain[0] and not [w for w in recwarn.list if "not recognised" in str(w.message)]
    finally:
        dgr._warned_chain[0] = prev


# ---------------------------------------------------------------------------------------------------------------------------
# 4. end to end against the float64 oracle fed o rho64
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S1:200", "S2q"])
def test_end_to_end_against_the_float64_oracle(name):
    sc, cam = at.scene(name)
    H, W = cam.image_height, cam.image_width
    bg = torch.tensor([0.1, 0.2, 0.3])
    dt = torch.float64
    # the truth: the oracle's rasterizer fed o rho64
    leaf64 = lambda x: x.detach().to(dt).clone().requires_grad_(True)
    T = dict(means3D=leaf64(sc.means3D), opacities=leaf64(sc.opacities), scales=leaf64(sc.scales), rotations=leaf64(sc.rotations))
    view = to.view_dict(cam, sh_degree=sc.sh_degree)
    rho, _, _ = at.rho(T["means3D"], view, scales=T["scales"], rotations=T["rotations"])
    color, _, _, _, _, aux = to.rasterize(T["means3D"], T["opacities"].reshape(-1) * rho, view, bg, scales=T["scales"],
                                          rotations=T["rotations"], shs=sc.shs.to(dt))
    bl = aux["borderline"]
    what = f"antialias end to end {name}"
    report(what, "borderline pixel fraction (bound 2e-2)", bl.float().mean().item())
    assert bl.float().mean().item() <= 0.02
    dL = scenes.grad_seed(W, H, 78) * (~bl).float()
    (color * dL.to(dt)).sum().backward()
    # the op
    leaf = lambda x: x.detach().cuda().clone().requires_grad_(True)
    G = dict(means3D=leaf(sc.means3D), opacities=leaf(sc.opacities), scales=leaf(sc.scales), rotations=leaf(sc.rotations))
    settings = _settings(cam.to("cuda"), bg=bg.cuda(), sh_degree=sc.sh_degree)
    r = dgr.GaussianRasterizer(settings)
    kw = dict(means2D=torch.zeros(sc.P, 3, device="cuda"), shs=sc.shs.cuda(), scales=G["scales"], rotations=G["rotations"])
    reset_forward_state()
    img = r.with_antialiasing()(means3D=G["means3D"], opacities=G["opacities"], **kw)[0]
    (img * dL.cuda()).sum().backward()
    with torch.no_grad():
        plain = r(means3D=G["means3D"], opacities=G["opacities"], **kw)[0]
    torch.cuda.synchronize()
    e = (img.detach().cpu().double() - color.detach()).abs()[:, ~bl].max().item()
    report(what, "colour max abs err off the borderline pixels", e)
    diff = (img.detach() - plain).abs().max().item()
    report(what, "antialiased vs plain colour, max abs", diff)
    errs = {k: rel_err(G[k].grad, T[k].grad) for k in G}
    for k, v in errs.items():
        report(what, f"grad {k} max-norm rel err", v)
    assert e <= FWD_ATOL
    assert diff > 0.05                                                              # not the unfiltered render
    for k, v in errs.items():
        assert v <= BWD_RTOL, (what, k, v)


# ---------------------------------------------------------------------------------------------------------------------------
# 5, 6. verification mode, contributions(), preprocess_only()
# ---------------------------------------------------------------------------------------------------------------------------
def test_verification_mode():
    sc, cam = at.scene("S1")
    prev = dgr.set_deterministic(True)
    try:
        _same(_render(sc, cam, "module"), _render(sc, cam, "fed"), "definition, verification mode",
              _render(sc, cam, "plain", loss=False))
    finally:
        dgr.set_deterministic(prev)


def test_contributions_and_preprocess_only_use_o_eff():
    sc, cam = at.scene("S2q")
    c = cam.to("cuda")
    settings = _settings(c)
    m, o, s, q = sc.means3D.cuda(), sc.opacities.cuda(), sc.scales.cuda(), sc.rotations.cuda()
    r = dgr.GaussianRasterizer(settings)
    o_eff = dgr.screen_compensation(m, o, settings, scales=s, rotations=q)
    assert not o_eff.requires_grad and (o_eff < o).any()
    for a, b, p in zip(r.with_antialiasing().preprocess_only(m, o, scales=s, rotations=q),
                       r.preprocess_only(m, o_eff, scales=s, rotations=q), r.preprocess_only(m, o, scales=s, rotations=q)):
        assert torch.equal(a, b)
    assert not torch.equal(a, p)                                                    # (pixel_sizes: not the plain call's)
    ca = r.with_antialiasing().contributions(m, o, scales=s, rotations=q)
    cb = r.contributions(m, o_eff, scales=s, rotations=q)
    cp = r.contributions(m, o, scales=s, rotations=q)
    for x, y in zip(ca, cb):
        assert torch.equal(x, y)
    assert ca.weight_sum.abs().max() > 0 and not torch.equal(ca.weight_sum, cp.weight_sum)


def test_host_entry():
    from gaussian_renderer import RESULT_KEYS, render, render_with_antialiasing
    sc, cam = at.scene("S2q")
    c, bg = cam.to("cuda"), torch.tensor([0.1, 0.2, 0.3], device="cuda")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    out = render_with_antialiasing(c, pc, PIPE, bg)
    assert tuple(out) == RESULT_KEYS
    out["render"].sum().backward()
    assert out["viewspace_points"].grad is not None and pc._opacity.grad.abs().max() > 0
    ref = _render(sc, cam, "module", loss=False)[0]
    with torch.no_grad():
        plain = render(c, SyntheticGaussians(sc, "cuda", requires_grad=False), PIPE, bg)
    assert torch.equal(out["render"].detach(), ref[0]) and torch.equal(out["pixel_sizes"], ref[4])
    assert (out["render"].detach() - plain["render"]).abs().max() > 0.05

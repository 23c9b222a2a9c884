"""The 3-D smoothing filter on the GPU (SPEC M16; include/msgs.h msgs_filter3d_sweep, msgs_smoothing_filter_*).

References, none of them the kernels under test:
  1  tests/filter3d_truth.py (float64, written from the definitions; pinned by tests/test_filter3d_cpu.py): the sweep with
     its borderline flags, and the filtered getters through float64 autograd;
  2  the plain GaussianRasterizer fed smoothing_filter(...): the definition of a filtered render, bit for bit;
  3  end to end, oracle/torch_oracle.py fed the float64-filtered scales and opacities, dL/dC zero on its borderline pixels.
Tolerances.  Sweep: max(1e-6, 4 x the error of the float32 restatement of the same formulas on the same inputs).  Getters: 2e-6
relative forward (about a dozen float32 roundings and two library calls of at most 2 ulp), BWD_RTOL per gradient tensor in
max-norm.  Routes: FWD_ATOL / BWD_RTOL and the 2 % cap on masked pixels, as tests/test_antialias_gpu.py.  The measured maxima are
printed (pytest -s) and recorded in profiles/filter3d_notes.md."""
import functools
import math

import pytest
import torch

import diff_gaussian_rasterization as dgr
import filter3d_truth as ft
import scenes
from oracle import torch_oracle as to
from parity_utils import BWD_RTOL, FWD_ATOL, PIPE, rel_err, report, small_scene
from route_utils import PLAIN, reset_forward_state
from synthetic_model import SyntheticGaussians

pytestmark = pytest.mark.gpu

CHUNK = dgr.FILTER3D_CAMERA_CHUNK
SWEEP_P = (1, 63, 257, 4099)
SWEEP_V = (1, 3, CHUNK, CHUNK + 1, 2 * CHUNK + 5)
GETTER_FWD_RTOL = 2e-6


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the sweep
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sweep_truth(P, V, rule):
    m, cams = ft.centres(P), ft.cameras(V)
    return m, cams, ft.sweep(m, cams, rule), ft.restatement_error(m, cams, rule)[0]


def _rel(got, want):
    return ((got.double() - want).abs() / want).max().item() if want.numel() else 0.0


@pytest.mark.parametrize("rule", ft.RULES)
@pytest.mark.parametrize("V", SWEEP_V)
@pytest.mark.parametrize("P", SWEEP_P)
def test_sweep_against_float64(P, V, rule):
    m, cams, t, restated = _sweep_truth(P, V, rule)
    what = f"filter3d sweep P={P} V={V} {rule}"
    filt, valid = dgr.compute_3d_filter(m.cuda(), cams, rule=rule)
    again = dgr.compute_3d_filter(m.cuda(), cams, rule=rule)
    torch.cuda.synchronize()
    assert filt.shape == (P, 1) and filt.dtype == torch.float32 and valid.shape == (P,) and valid.dtype == torch.bool
    assert not filt.requires_grad
    assert torch.equal(filt, again[0]) and torch.equal(valid, again[1])              # two runs: the same bits
    filt, valid = filt.cpu().reshape(-1), valid.cpu()
    ok = ~t["flagged"]
    assert torch.equal(valid[ok], t["valid"][ok])
    if t["fallback"] is None:                                                        # nobody is seen: the identity
        assert not t["flagged"].any() and not valid.any() and torch.equal(filt, torch.zeros(P))
        return
    tol = max(1e-6, 4.0 * restated)
    e = _rel(filt[ok], t["filter"][ok])                # (relative error of filter_3D = that of nu; unseen rows: the fallback's)
    report(what, f"nu max rel err on unflagged Gaussians (restatement {restated:.2e}, bound {tol:.2e})", e)
    assert e <= tol
    unseen = ok & ~t["valid"]
    if unseen.any():                                                                 # they all carry the one fallback value
        assert (filt[unseen] == filt[unseen][0]).all() and filt[unseen][0] == filt[ok & t["valid"]].max()
    fl = t["flagged"]
    if fl.any():
        e_lo = (filt[fl].double() - t["filter_lo"][fl]).abs() / t["filter_lo"][fl]
        e_hi = (filt[fl].double() - t["filter_hi"][fl]).abs() / t["filter_hi"][fl]
        assert (torch.minimum(e_lo, e_hi) <= tol).all(), what
    assert torch.isfinite(filt).all() and (filt > 0).all()


def test_sweep_everything_behind_every_camera_gives_zeros():
    cams = ft.cameras(1)                                                             # at (0, 0, -8), looking along +z
    filt, valid = dgr.compute_3d_filter(torch.tensor([[0.0, 0.0, -14.0]], device="cuda"), cams)
    assert torch.equal(filt.cpu(), torch.zeros(1, 1)) and not valid.any()
    m = ft.centres(300).clone()
    m[:, 2] = -9.0 - m[:, 2].abs()                                                   # 300 of them, all behind it
    for rule in ft.RULES:
        filt, valid = dgr.compute_3d_filter(m.cuda(), cams, rule=rule)
        assert torch.equal(filt.cpu(), torch.zeros(300, 1)) and not valid.any()
    # ... and the getters read that as "no filter"
    s, o, _, _, _ = ft.getter_rows(300, False)
    s_eff, o_eff = dgr.smoothing_filter(s.cuda(), o.cuda(), filt)
    assert torch.equal(s_eff.cpu(), s) and torch.equal(o_eff.cpu(), o)


def test_sweep_nan_centre_is_invalid_and_does_not_poison_the_fallback():
    cams = ft.cameras(CHUNK + 1)
    m = ft.centres(257).clone()
    clean = dgr.compute_3d_filter(m.cuda(), cams)
    for row, col, bad in ((5, 0, float("nan")), (70, 2, float("inf")), (200, 1, float("nan"))):
        m[row, col] = bad
    filt, valid = dgr.compute_3d_filter(m.cuda(), cams)
    t = ft.sweep(m, cams)
    rows = torch.tensor([5, 70, 200])
    assert not valid.cpu()[rows].any() and not t["valid"][rows].any()
    assert torch.isfinite(filt).all()
    keep = torch.ones(257, dtype=torch.bool)
    keep[rows] = False
    fb = filt.cpu()[~t["valid"] & ~t["flagged"]]
    assert (fb == fb[0]).all() and (filt.cpu()[rows] == fb[0]).all()
    # the other rows are what they were, unless one of the three held the fallback minimum
    if clean[0].max() == filt.max():
        assert torch.equal(filt.cpu()[keep], clean[0].cpu()[keep])


def test_sweep_takes_a_non_contiguous_float64_model_and_cameras_anywhere_and_refuses_the_cpu():
    m, cams, t, restated = _sweep_truth(257, 3, "per_camera")
    wide = torch.zeros(257, 6, dtype=torch.float64, device="cuda")
    wide[:, ::2] = m.cuda().double()
    a = dgr.compute_3d_filter(wide[:, ::2].requires_grad_(True), cams)
    b = dgr.compute_3d_filter(m.cuda(), cams)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not a[0].requires_grad
    c = dgr.compute_3d_filter(m.cuda(), [cam.to("cuda") for cam in cams])           # cameras that live on the device
    mixed = dgr.compute_3d_filter(m.cuda(), [cams[0].to("cuda"), cams[1], cams[2]])
    for other in (c, mixed):
        assert torch.equal(other[0], b[0]) and torch.equal(other[1], b[1])
    with pytest.raises(RuntimeError, match="HIP device"):
        dgr.compute_3d_filter(m, cams)
    e = dgr.compute_3d_filter(torch.zeros(0, 3, device="cuda"), cams)
    assert e[0].shape == (0, 1) and e[1].shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the filtered getters
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _getter_truth(P, raw):
    s, o, f, g_s, g_o = ft.getter_rows(P, raw)
    return s, o, f, g_s, g_o, ft.getter_truth(s, o, f, g_s, g_o, raw)


def _elementwise_rel(got, want):
    got, want = got.detach().cpu().double(), want.double()
    zero = want == 0
    assert (got[zero] == 0).all()
    return ((got - want).abs()[~zero] / want.abs()[~zero]).max().item() if (~zero).any() else 0.0


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("P", SWEEP_P)
def test_getters_against_float64(P, raw):
    s, o, f, g_s, g_o, t = _getter_truth(P, raw)
    what = f"filter3d getters P={P} {'raw' if raw else 'activated'}"
    S, O = s.cuda().requires_grad_(True), o.cuda().requires_grad_(True)
    s_eff, o_eff = dgr.smoothing_filter(S, O, f.cuda(), raw=raw)
    assert s_eff.shape == (P, 3) and o_eff.shape == (P, 1) and s_eff.dtype == o_eff.dtype == torch.float32
    ((s_eff * g_s.cuda()).sum() + (o_eff * g_o.cuda()).sum()).backward()
    torch.cuda.synchronize()
    e_s, e_o = _elementwise_rel(s_eff, t["s_eff"]), _elementwise_rel(o_eff, t["o_eff"])
    report(what, "s_eff max elementwise rel err", e_s)
    report(what, "o_eff max elementwise rel err", e_o)
    g_es, g_eo = rel_err(S.grad, t["scales"]), rel_err(O.grad, t["opacities"])
    report(what, "grad scales max-norm rel err", g_es)
    report(what, "grad opacities max-norm rel err", g_eo)
    assert e_s <= GETTER_FWD_RTOL and e_o <= GETTER_FWD_RTOL
    assert g_es <= BWD_RTOL and g_eo <= BWD_RTOL
    for v in (s_eff, o_eff, S.grad, O.grad):
        assert torch.isfinite(v).all()
    off = (f == 0).reshape(-1)
    assert off.any()
    if not raw:                                          # f == 0: the row's own bits, forward and backward
        assert torch.equal(s_eff.detach().cpu()[off], s[off]) and torch.equal(o_eff.detach().cpu()[off], o[off])
        assert torch.equal(S.grad.cpu()[off], g_s[off]) and torch.equal(O.grad.cpu()[off], g_o[off])
    if not raw and P > 5:                                # s_k == 0 under f > 0: s_eff_k = f, o_eff = 0, finite gradients
        assert s_eff[4, 1].item() == f[4, 0].item() and o_eff[4, 0].item() == 0.0 and S.grad[4, 1].item() != 0.0
        assert torch.equal(s_eff.detach().cpu()[5], f[5].expand(3)) and o_eff[5, 0].item() == 0.0
        assert not S.grad[5].any()


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
def test_getters_one_output_used_two_runs_and_empty(raw):
    s, o, f, g_s, g_o, t = _getter_truth(257, raw)
    def run(use_s, use_o):
        S, O = s.cuda().requires_grad_(True), o.cuda().requires_grad_(True)
        s_eff, o_eff = dgr.smoothing_filter(S, O, f.cuda(), raw=raw)
        loss = 0
        if use_s:
            loss = loss + (s_eff * g_s.cuda()).sum()
        if use_o:
            loss = loss + (o_eff * g_o.cuda()).sum()
        loss.backward()
        return S.grad, O.grad
    both, again = run(True, True), run(True, True)
    assert torch.equal(both[0], again[0]) and torch.equal(both[1], again[1])
    only_s, only_o = run(True, False), run(False, True)
    assert not only_s[1].any()                                                       # dL/do comes from o_eff alone
    assert rel_err(only_s[0].double() + only_o[0].double(), t["scales"]) <= BWD_RTOL
    assert rel_err(only_o[1], t["opacities"]) <= BWD_RTOL
    z = lambda *sh: torch.zeros(*sh, device="cuda", requires_grad=True)
    S, O = z(0, 3), z(0, 1)
    s_eff, o_eff = dgr.smoothing_filter(S, O, torch.zeros(0, 1, device="cuda"), raw=raw)
    assert s_eff.shape == (0, 3) and o_eff.shape == (0, 1)
    (s_eff.sum() + o_eff.sum()).backward()
    assert S.grad.shape == (0, 3) and O.grad.shape == (0, 1)


def test_raw_getters_activate_as_the_rasterizer_does():
    """raw=True with f = 0 returns the activated values, expf(x) and 1 / (1 + expf(-x)): within 2 ulp of float64 for the
    exponential (the library call) and 3 ulp for the sigmoid (the call and two roundings), 1 ulp = 2^-23"""
    s, o, _, _, _ = ft.getter_rows(4099, True)
    s_eff, o_eff = dgr.smoothing_filter(s.cuda(), o.cuda(), torch.zeros(4099, 1, device="cuda"), raw=True)
    e_s, e_o = _elementwise_rel(s_eff, torch.exp(s.double())), _elementwise_rel(o_eff, torch.sigmoid(o.double()))
    report("filter3d raw activations", "exp max rel err", e_s)
    report("filter3d raw activations", "sigmoid max rel err", e_o)
    assert e_s <= 2 * 2.0 ** -23 and e_o <= 3 * 2.0 ** -23


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the routes
# ---------------------------------------------------------------------------------------------------------------------------
LEAVES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
ROUTE_VARIANCE = 2.0          # the front camera's pixels are coarse at these sizes: a filter about as large as the Gaussians
BG = (0.1, 0.2, 0.3)


@functools.lru_cache(maxsize=None)
def _route_scene(P=400, W=64, H=40, seed=31):
    sc, cam = small_scene(P, W, H, seed)
    cams = [cam, scenes.front_camera(W // 2, H // 2)]
    filt, valid = dgr.compute_3d_filter(sc.means3D.cuda(), cams, variance=ROUTE_VARIANCE)
    assert valid.any() and (filt > 0).all()
    return sc, cam, filt


def _model(sc, filt, requires_grad=True):
    pc = SyntheticGaussians(sc, "cuda", requires_grad=requires_grad)
    pc.filter_3D = filt
    return pc


def _settings(c, pc, st=PLAIN):
    return dgr.GaussianRasterizationSettings(
        image_height=int(c.image_height), image_width=int(c.image_width), tanfovx=math.tan(0.5 * c.FoVx),
        tanfovy=math.tan(0.5 * c.FoVy), bg=torch.tensor(BG, device="cuda"), scale_modifier=1.0, viewmatrix=c.world_view_transform,
        projmatrix=c.full_proj_transform, sh_degree=pc.active_sh_degree, campos=c.camera_center, prefiltered=False, debug=False,
        **st)


def _backward(pc, image, depth, viewspace, W, H):
    ((image * scenes.grad_seed(W, H, 78).cuda()).sum() + (depth * scenes.grad_seed(W, H, 77)[0].cuda() * 0.1).sum()).backward()
    grads = {n: getattr(pc, n).grad.detach().clone() for n in LEAVES}
    grads["viewspace"] = viewspace.grad.detach().clone()
    torch.cuda.synchronize()
    return grads


def _route(how, raw, antialiasing, st=PLAIN):
    """("host": filter3d.render_with_3d_filter | "fed": the plain module fed smoothing_filter(...)) -> (outputs, gradients)"""
    import filter3d
    from gaussian_renderer import _colour_inputs
    sc, cam, filt = _route_scene()
    pc, c = _model(sc, filt), cam.to("cuda")
    W, H = c.image_width, c.image_height
    reset_forward_state()
    if how == "host":
        out = filter3d.render_with_3d_filter(c, pc, PIPE, torch.tensor(BG, device="cuda"), antialiasing=antialiasing, raw=raw,
                                             **{k: v for k, v in st.items() if k in ("filter_small", "filter_large", "fade_size")})
        outs = (out["render"], out["acc_pixel_size"], out["depth"], out["radii"], out["pixel_sizes"])
        vs = out["viewspace_points"]
    else:
        if raw:
            s_eff, o_eff = dgr.smoothing_filter(pc._scaling, pc._opacity, filt, raw=True)
        else:
            s_eff, o_eff = dgr.smoothing_filter(pc.get_scaling, pc.get_opacity, filt)
        r = dgr.GaussianRasterizer(_settings(c, pc, st))
        if antialiasing:
            r = r.with_antialiasing()
        vs = torch.zeros_like(pc.get_xyz, requires_grad=True) + 0
        vs.retain_grad()
        outs = r(means3D=pc.get_xyz, means2D=vs, opacities=o_eff, max_pixel_sizes=pc.get_max_pixel_sizes,
                 min_pixel_sizes=pc.get_min_pixel_sizes, occ_multiplier=pc.get_occ_multiplier, dc_delta=pc.get_dc_delta,
                 base_mask=pc.get_base_mask, scales=s_eff, rotations=pc.get_rotation, **_colour_inputs(c, pc, PIPE, None))
    grads = _backward(pc, outs[0], outs[2], vs, W, H)
    return tuple(o.detach() for o in outs), grads


@pytest.mark.parametrize("antialiasing", [False, True], ids=["plain", "antialiasing"])
@pytest.mark.parametrize("raw", [True, False], ids=["raw", "activated"])
def test_render_with_3d_filter_is_the_plain_module_fed_the_filtered_getters(raw, antialiasing):
    from gaussian_renderer import render
    (oa, ga), (ob, gb) = _route("host", raw, antialiasing), _route("fed", raw, antialiasing)
    for i, (x, y) in enumerate(zip(oa, ob)):
        assert torch.equal(x, y), ("output", i)
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
        assert torch.isfinite(ga[k]).all()
    assert ga["_scaling"].abs().max() > 0 and ga["_opacity"].abs().max() > 0
    # ... and it is not the unfiltered render
    sc, cam, filt = _route_scene()
    with torch.no_grad():
        plain = render(cam.to("cuda"), SyntheticGaussians(sc, "cuda", requires_grad=False), PIPE, torch.tensor(BG, device="cuda"))
    assert (oa[0] - plain["render"]).abs().max() > 0.01


def test_raw_and_activated_getters_render_the_same_image_under_the_multi_scale_filters():
    st = dict(filter_small=True, filter_large=True, fade_size=1.0)
    (oa, ga), (ob, gb) = _route("host", True, False, st), _route("host", False, False, st)
    assert (oa[0] - ob[0]).abs().max() <= FWD_ATOL
    for k in ga:
        assert rel_err(ga[k], gb[k]) <= BWD_RTOL, k


def test_no_chained_mode_and_no_warning_for_filtered_getters(recwarn):
    prev, dgr._warned_chain[0] = dgr._warned_chain[0], False
    try:
        _route("host", False, False)
        assert not dgr._warned_chain[0] and not [w for w in recwarn.list if "not recognised" in str(w.message)]
    finally:
        dgr._warned_chain[0] = prev


def test_end_to_end_against_the_float64_oracle():
    sc, cam = small_scene(200, 64, 40, seed=33)
    H, W = cam.image_height, cam.image_width
    bg = torch.tensor(BG)
    dt = torch.float64
    filt, _ = dgr.compute_3d_filter(sc.means3D.cuda(), [cam], variance=ROUTE_VARIANCE)
    # the truth: the oracle's rasterizer fed the float64-filtered scales and opacities
    leaf64 = lambda x: x.detach().to(dt).clone().requires_grad_(True)
    T = dict(means3D=leaf64(sc.means3D), opacities=leaf64(sc.opacities), scales=leaf64(sc.scales), rotations=leaf64(sc.rotations))
    s_eff, o_eff = ft.getters(T["scales"], T["opacities"], filt.cpu())
    view = to.view_dict(cam, sh_degree=sc.sh_degree)
    color, _, _, _, _, aux = to.rasterize(T["means3D"], o_eff.reshape(-1), view, bg, scales=s_eff, rotations=T["rotations"],
                                          shs=sc.shs.to(dt))
    bl = aux["borderline"]
    what = "filter3d end to end"
    report(what, "borderline pixel fraction (bound 2e-2)", bl.float().mean().item())
    assert bl.float().mean().item() <= 0.02
    dL = scenes.grad_seed(W, H, 78) * (~bl).float()
    (color * dL.to(dt)).sum().backward()
    # the op
    leaf = lambda x: x.detach().cuda().clone().requires_grad_(True)
    G = dict(means3D=leaf(sc.means3D), opacities=leaf(sc.opacities), scales=leaf(sc.scales), rotations=leaf(sc.rotations))
    c = cam.to("cuda")
    settings = dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=math.tan(0.5 * c.FoVx), tanfovy=math.tan(0.5 * c.FoVy), bg=bg.cuda(),
        scale_modifier=1.0, viewmatrix=c.world_view_transform, projmatrix=c.full_proj_transform, sh_degree=sc.sh_degree,
        campos=c.camera_center, prefiltered=False, debug=False, **PLAIN)
    r = dgr.GaussianRasterizer(settings)
    kw = dict(means3D=G["means3D"], means2D=torch.zeros(sc.P, 3, device="cuda"), shs=sc.shs.cuda(), rotations=G["rotations"])
    reset_forward_state()
    gs, go = dgr.smoothing_filter(G["scales"], G["opacities"], filt)
    img = r(opacities=go, scales=gs, **kw)[0]
    (img * dL.cuda()).sum().backward()
    with torch.no_grad():
        plain = r(opacities=G["opacities"], scales=G["scales"], **kw)[0]
    torch.cuda.synchronize()
    e = (img.detach().cpu().double() - color.detach()).abs()[:, ~bl].max().item()
    report(what, "colour max abs err off the borderline pixels", e)
    diff = (img.detach() - plain).abs().max().item()
    report(what, "filtered vs plain colour, max abs", diff)
    errs = {k: rel_err(G[k].grad, T[k].grad) for k in G}
    for k, v in errs.items():
        report(what, f"grad {k} max-norm rel err", v)
    assert e <= FWD_ATOL
    assert diff > 0.01                                                               # not the unfiltered render
    for k, v in errs.items():
        assert v <= BWD_RTOL, (what, k, v)


def test_bake_then_render_is_the_filtered_render():
    import filter3d
    from gaussian_renderer import render
    sc, cam, filt = _route_scene()
    c, bg = cam.to("cuda"), torch.tensor(BG, device="cuda")
    with torch.no_grad():
        want = filter3d.render_with_3d_filter(c, _model(sc, filt, False), PIPE, bg)
        pc = _model(sc, filt, False)
        before = pc._scaling.detach().clone()
        assert filter3d.bake_3d_filter(pc) is pc and pc.filter_3D is None
        got = render(c, pc, PIPE, bg)
        plain = render(c, SyntheticGaussians(sc, "cuda", requires_grad=False), PIPE, bg)
    e = (got["render"] - want["render"]).abs().max().item()
    report("filter3d bake", "render() of the baked model vs the filtered render, max abs", e)
    assert e <= FWD_ATOL
    assert (pc._scaling.detach() >= before).all() and (got["render"] - plain["render"]).abs().max() > 0.01
    with pytest.raises(ValueError, match="compute_3D_filter"):
        filter3d.render_with_3d_filter(c, pc, PIPE, bg)


def test_a_stale_filter_raises_before_any_launch():
    import filter3d
    sc, cam, filt = _route_scene()
    pc = _model(sc, filt[:-1].contiguous())
    calls = []
    prev, dgr._filter3d_probe = dgr._filter3d_probe, calls.append
    try:
        with pytest.raises(ValueError, match="stale"):
            filter3d.render_with_3d_filter(cam.to("cuda"), pc, PIPE, torch.tensor(BG, device="cuda"))
        with pytest.raises(ValueError, match="stale"):
            dgr.smoothing_filter(pc._scaling, pc._opacity, pc.filter_3D, raw=True)
        assert calls == []
        pc.filter_3D = filt
        filter3d.render_with_3d_filter(cam.to("cuda"), pc, PIPE, torch.tensor(BG, device="cuda"))
        assert calls == ["msgs_smoothing_filter_forward"]
        filter3d.compute_3D_filter(pc, [cam])
        assert calls[-1] == "msgs_filter3d_sweep" and pc.filter_3D.shape == (sc.P, 1)
    finally:
        dgr._filter3d_probe = prev

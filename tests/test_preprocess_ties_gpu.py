"""Exact ties of K1's per-Gaussian decisions in the kernels: the cases and expectations of
tests/preprocess_ties.py (proved, and the oracles held to them, in tests/test_preprocess_ties_cpu.py) through
GaussianRasterizer.preprocess_only, the plain entry (forward and backward), the chained-getter entry and render_fused.
Decisions are compared for exact equality: radii, pixel_sizes (zero or not; bit-identical with and without the filters),
exactly zero gradients of a row that does not exist in the view, bit-equal metamorphic pairs.  The only tolerance is BWD_RTOL
of the clamp rows' gradients against the float64 autograd oracle, each row on its own scale.  profiles/preprocess_ties_notes.md
names the line of preprocess.hip every family pins."""
import functools
import math

import numpy as np
import pytest
import torch

import preprocess_ties as pt
import scenes
from parity_utils import BWD_RTOL, leaf_space, rel_err, report
from test_activation_edges_gpu import BG, ENTRIES, ST, _run, oracles

pytestmark = pytest.mark.gpu

MODEL_LEAVES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
assert ST == pt.OFF


@functools.lru_cache(maxsize=None)
def _case(family):
    return pt.CASES[family]()


def _rs(cam, st):
    import diff_gaussian_rasterization as dgr
    return dgr.GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(0.5 * cam.FoVx),
        tanfovy=math.tan(0.5 * cam.FoVy), bg=BG.cuda(), scale_modifier=1.0, viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=3, campos=cam.camera_center, prefiltered=False, debug=False, **st)


def _inputs(case, filt=None, opacities=None, grad=False):
    """the op's tensors on the device: (means3D, opacities, shs, shape kwargs, filter kwargs)"""
    sc = case.scene
    dev = lambda t: t.detach().to("cuda").contiguous()
    leaf = (lambda t: dev(t.float()).clone().requires_grad_(True)) if grad else (lambda t: dev(t.float()))
    mn, mx, base = filt if filt is not None else (sc.min_pixel_sizes, sc.max_pixel_sizes, sc.base_mask)
    f32 = lambda a: torch.as_tensor(np.asarray(a)).to(torch.float32)
    filt_kw = dict(min_pixel_sizes=dev(f32(mn)), max_pixel_sizes=dev(f32(mx)), base_mask=dev(torch.as_tensor(np.asarray(base)).bool()))
    shape = dict(cov3D_precomp=leaf(case.cov3D)) if case.cov3D is not None else \
        dict(scales=leaf(sc.scales), rotations=leaf(sc.rotations))
    return leaf(sc.means3D), leaf(sc.opacities if opacities is None else opacities), leaf(sc.shs), shape, filt_kw


def _only(case, st=pt.OFF, filt=None, opacities=None):
    """(radii [P] int64, pixel_sizes [P] float32 numpy) of preprocess_only"""
    import diff_gaussian_rasterization as dgr
    m, o, _, shape, fk = _inputs(case, filt, opacities)
    radii, psize = dgr.GaussianRasterizer(_rs(case.cam.to("cuda"), st)).preprocess_only(m, o, **shape, **fk)
    torch.cuda.synchronize()
    return radii.cpu().long(), psize.cpu().numpy()


def _direct(case, st=pt.OFF, filt=None, opacities=None, seed=5):
    """the plain entry on activated leaves, forward and backward: (outputs on the CPU, {input: gradient on the CPU})"""
    import diff_gaussian_rasterization as dgr
    sc, cam = case.scene, case.cam.to("cuda")
    m, o, sh, shape, fk = _inputs(case, filt, opacities, grad=True)
    m2 = torch.zeros_like(m, requires_grad=True)
    outs = dgr.GaussianRasterizer(_rs(cam, st))(means3D=m, means2D=m2, opacities=o, shs=sh, occ_multiplier=sc.occ_multiplier.cuda(),
                                                dc_delta=sc.dc_delta.cuda(), **shape, **fk)
    assert type(outs[0].grad_fn).__name__ == "_RasterizeGaussiansBackward"
    outs[0].backward(scenes.grad_seed(cam.image_width, cam.image_height, seed).cuda())
    torch.cuda.synchronize()
    out = dict(zip(("render", "acc_pixel_size", "depth", "radii", "pixel_sizes"), (t.detach().cpu() for t in outs)))
    grads = dict(means3D=m.grad, opacities=o.grad, shs=sh.grad, means2D=m2.grad, **{k: v.grad for k, v in shape.items()})
    return out, {k: v.detach().cpu() for k, v in grads.items()}


def _pixel_count(case, st=pt.OFF, filt=None):
    import diff_gaussian_rasterization as dgr
    m, o, sh, shape, fk = _inputs(case, filt)
    s = dgr.GaussianRasterizer(_rs(case.cam.to("cuda"), st)).contributions(m, o, shs=sh, **shape, **fk)
    return s.pixel_count.cpu()


def _assert_rows_zero(what, grads, rows):
    for k, g in grads.items():
        assert torch.isfinite(g).all(), (what, k, "non-finite")
        assert not g[rows].any(), (what, k, [i for i in rows if g[i].any()])


def _check_view(what, case, radii, psize, grads, alive_of=None):
    """decisions, and exactly zero gradients on every row that does not exist in the view"""
    pt.check_rows(what, case, radii, psize, alive_of)
    dead = [r["row"] for r in case.rows if (r["alive"] if alive_of is None else alive_of.get(r["row"], r["alive"])) is False]
    assert (radii[dead] == 0).all()
    _assert_rows_zero(what, grads, dead)
    q1 = [r["row"] for r in case.rows if r.get("q1")]
    assert not psize[q1].any()


FAMILIES = ("near", "degenerate", "rect", "rect_ragged", "gate", "clamp")


@pytest.mark.parametrize("family", FAMILIES)
def test_preprocess_only_at_the_ties(family):
    case = _case(family)
    radii, psize = _only(case)
    assert np.isfinite(psize).all()
    pt.check_rows(f"{family} preprocess_only", case, radii, psize)


@pytest.mark.parametrize("family", FAMILIES)
def test_plain_entry_at_the_ties(family):
    case = _case(family)
    out, grads = _direct(case)
    for k, v in out.items():
        assert torch.isfinite(v.float()).all(), (family, k)
    _check_view(f"{family} plain", case, out["radii"].long(), out["pixel_sizes"].numpy(), grads)
    r0, s0 = _only(case)
    assert torch.equal(out["radii"].long(), r0) and np.array_equal(out["pixel_sizes"].numpy(), s0)
    blind = [r["row"] for r in case.rows if r["no_pixels"]]
    if blind:                                                          # alive (radii > 0), and in no pixel
        assert (out["radii"][blind] > 0).all() and not _pixel_count(case)[blind].any(), family


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("family", ["near", "rect", "rect_ragged", "clamp"])
def test_getter_entries_at_the_ties(family, entry):
    """the ties that pass no activation (they sit in means3D), through render() with the chained getters, render() on the
    plain autograd path and render_fused()"""
    case = _case(family)
    W, H = case.cam.image_width, case.cam.image_height
    out, pc = _run(entry, case.scene, case.cam, {}, scenes.grad_seed(W, H, 5))
    grads = {n: getattr(pc, n).grad.detach().cpu() for n in MODEL_LEAVES}
    grads["means2D"] = out["viewspace_points"].grad.detach().cpu()
    radii = out["radii"].detach().cpu().long()
    _check_view(f"{family} {entry}", case, radii, out["pixel_sizes"].detach().cpu().numpy(), grads)
    assert torch.equal(out["visibility_filter"].cpu(), radii > 0)
    # the means enter these entries untouched: the decisions of the plain entry, row for row over the whole scene
    assert torch.equal(radii > 0, _only(case)[0] > 0)


# ---------------------------------------------------------------------------------------------------------------------------
# Q2: the clamp mask, through the gradients
# ---------------------------------------------------------------------------------------------------------------------------
def _rows_on_their_own_scale(what, case, pairs, clean):
    """every tie row's gradient against the float64 truth at BWD_RTOL of the ROW's own magnitude in that tensor (a flipped
    mask moves dL/dmeans3D by >= 100 x that: test_clamp_flip_cannot_hide); the rest of the scene in the max norm"""
    rows = [r["row"] for r in case.rows]
    assert clean[rows].all(), [r["name"] for r in case.rows if not clean[r["row"]]]
    for k, (got, ref) in pairs.items():
        P = ref.shape[0]
        got, ref = got.detach().double().cpu().reshape(P, -1), ref.detach().double().cpu().reshape(P, -1)
        e_all = rel_err(got, ref, clean)
        report(what, f"{k}: clean rows, max norm", e_all)
        d = (got - ref).abs().max(dim=1).values
        own = ref.abs().max(dim=1).values
        worst = max((d[i] / own[i]).item() if own[i] > 0 else float(d[i] > 0) for i in rows)
        report(what, f"{k}: tie rows, worst |d| / own", worst)
        assert e_all <= BWD_RTOL, (what, k, e_all)
        for r in case.rows:
            i = r["row"]
            assert d[i] <= BWD_RTOL * own[i], (what, k, r["name"], d[i].item(), own[i].item())


@functools.lru_cache(maxsize=None)
def _clamp_oracles():
    case = _case("clamp")
    return oracles(case.scene, case.cam, {}, scenes.grad_seed(64, 64, 71))


@pytest.mark.parametrize("entry", ENTRIES)
def test_clamp_rows_against_float64(entry):
    case = _case("clamp")
    dL = scenes.grad_seed(64, 64, 71)
    seen, orc, tg, t_out = _clamp_oracles()
    clean = ~(orc.borderline_gaussians | (t_out["radii"] != orc.radii)).cpu()
    out, pc = _run(entry, case.scene, case.cam, {}, dL)
    assert torch.equal(out["radii"].cpu(), orc.radii)
    _rows_on_their_own_scale(f"clamp {entry}", case, leaf_space(pc, out["viewspace_points"].grad, tg), clean)


def test_clamp_rows_against_float64_plain_entry():
    from oracle import oracle_ctypes as oc
    from oracle import torch_oracle as to
    case = _case("clamp")
    dL = scenes.grad_seed(64, 64, 71)
    orc = oc.rasterize(case.scene, case.cam, pt.OFF, BG)
    t_out, tg = to.forward_backward(case.scene, case.cam, pt.OFF, BG, dL)
    clean = ~(orc.borderline_gaussians | (t_out["radii"] != orc.radii))
    out, grads = _direct(case, seed=71)
    assert torch.equal(out["radii"], orc.radii)
    _rows_on_their_own_scale("clamp direct", case, {k: (grads[k], tg[k]) for k in grads}, clean)


# ---------------------------------------------------------------------------------------------------------------------------
# M1-M4: the gate row under the small filter, the self-calibrated filters, the effective opacity
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fade", [0.0, 1.0])
def test_gate_row_under_the_small_filter(fade):
    case = _case("gate")
    st, mn, mx, base, alive = pt.gate_filters(case, fade)
    radii, psize = _only(case, st, (mn, mx, base))
    pt.check_rows(f"gate fade {fade} preprocess_only", case, radii, psize, alive)
    out, grads = _direct(case, st, (mn, mx, base))
    _check_view(f"gate fade {fade} plain", case, out["radii"].long(), out["pixel_sizes"].numpy(), grads, alive)
    assert np.array_equal(psize, _only(case)[1])


@pytest.mark.parametrize("run", ["fade0", "fade1", "fade05"])
def test_filters_self_calibrated(run):
    """thresholds from the kernel's own pixel_sizes bits: min_ps = s kept / one ulp above dropped, max_ps = s kept / one ulp
    below dropped, <= 0 no filter, base_mask exempt from the small filter only; the fade ramp running out at exactly w = 0"""
    case = _case("filters")
    r0, s = _only(case)
    rows = [r["row"] for r in case.rows]
    assert (r0[rows] > 0).all() and (s[rows] > 0).all()
    st, mn, mx, base, plan = pt.filter_plan(case, run, s)
    want = r0.clone()
    for i, p in plan.items():
        if not p["alive"]:
            want[i] = 0
    r1, s1 = _only(case, st, (mn, mx, base))
    assert torch.equal(r1, want), [(plan[i]["role"], int(r1[i]), int(r0[i])) for i in plan if r1[i] != want[i]]
    assert np.array_equal(s1.view(np.int32), s.view(np.int32))         # M1: written before any filter
    out, grads = _direct(case, st, (mn, mx, base))
    assert torch.equal(out["radii"].long(), want) and np.array_equal(out["pixel_sizes"].numpy().view(np.int32), s.view(np.int32))
    _assert_rows_zero(f"filters {run}", grads, [i for i, p in plan.items() if not p["alive"]])
    blind = [i for i, p in plan.items() if p["alive"] and p.get("no_pixels")]
    if blind:                                                          # w = one ulp: alive, and in no pixel
        assert not _pixel_count(case, st, (mn, mx, base))[blind].any()
    seen = [i for i, p in plan.items() if p["alive"] and not p.get("no_pixels")]
    assert all(grads["opacities"][i].abs().item() > 0 for i in seen)


def test_effective_opacity_is_o_times_w():
    """M4: the scene with w = 0.5 and w = 0.25 rows against the same scene with those rows' filters disabled and their
    opacity multiplied by w: the same render and gradients, bit for bit; dL/dopacity of those rows exactly w times"""
    case = _case("filters")
    _, s = _only(case)
    st, mn, mx, base, plan = pt.filter_plan(case, "fade1", s)
    a, b, ws = pt.metamorphic_pair(case, mn, mx, base, plan)
    assert sorted(ws.values()) == [0.25, 0.5]
    oa, ga = _direct(case, st, (a.min_pixel_sizes, a.max_pixel_sizes, a.base_mask), a.opacities)
    ob, gb = _direct(case, st, (b.min_pixel_sizes, b.max_pixel_sizes, b.base_mask), b.opacities)
    for k in ("render", "depth", "radii"):
        assert torch.equal(oa[k], ob[k]), k
    for k in ga:
        if k != "opacities":
            assert torch.equal(ga[k], gb[k]), k
    other = torch.ones(case.scene.P, dtype=torch.bool)
    other[list(ws)] = False
    assert torch.equal(ga["opacities"][other], gb["opacities"][other])
    for i, w in ws.items():
        assert gb["opacities"][i].abs().item() > 0 and ga["opacities"][i].item() == w * gb["opacities"][i].item(), i


# ---------------------------------------------------------------------------------------------------------------------------
# the same near-plane rule in two other kernels
# ---------------------------------------------------------------------------------------------------------------------------
def test_screen_compensation_near_plane():
    """antialias.hip: a row at t.z = 0.2f is exceptional (rho = 1, o_eff == o bit for bit, no geometry gradient); one ulp
    further out rho < 1"""
    import diff_gaussian_rasterization as dgr
    case = _case("near")
    m, o, _, shape, _ = _inputs(case, grad=True)
    o_eff = dgr.screen_compensation(m, o, _rs(case.cam.to("cuda"), pt.OFF), **shape)
    g = torch.linspace(0.5, 1.5, case.scene.P, device="cuda").view_as(o_eff)
    (o_eff * g).sum().backward()
    torch.cuda.synchronize()
    culled, out = [r["row"] for r in case.rows if r["q1"]], [r["row"] for r in case.rows if not r["q1"]]
    assert len(culled) == 6 and len(out) == 3
    assert torch.equal(o_eff.detach()[culled], o.detach()[culled])
    assert (o_eff.detach()[out] < o.detach()[out]).all()
    for k, t in dict(means3D=m, **shape).items():
        assert not t.grad[culled].any(), k
        # (an isotropic row's rho does not depend on its rotation)
        assert k == "rotations" or t.grad[out].any(dim=1).all(), k
    assert torch.equal(o.grad[culled], g[culled])


def test_filter3d_near_plane():
    """filter3d.hip: valid_points is 0 at t.z = 0.2f and 1 one ulp further out"""
    import diff_gaussian_rasterization as dgr
    case = _case("near")
    _, valid = dgr.compute_3d_filter(case.scene.means3D.cuda(), [case.cam])
    valid = valid.cpu()
    for r in case.rows:
        if r["name"].startswith("centre"):
            assert bool(valid[r["row"]]) == (not r["q1"]), r["name"]

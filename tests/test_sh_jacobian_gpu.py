"""The SH direction term of the per-Gaussian backward comes from the forward.

preprocess_kernel (K1) leaves J[c][j] = sum_k dB_k/dd_j sh[k][c] per rendered Gaussian (GeomLayout::shjac) and
preprocess_backward_kernel (K9) forms dL/dd_j = sum_c J[c][j] dL/drgb_c from it instead of fetching the SH row again.  Here:

(1) every entry that reaches a different K9 path — chained render(), render() with chain_reference_getters = False,
    render_fused(), two views accumulated into one bucket, the factored SH exchange, a depth loss, camera gradients — against the
    float32 CPU oracle at the north star's BWD_RTOL, on scenes laid out so that the staging can go wrong: P = 193 (the last wave
    holds one Gaussian), ranks 0-31 culled next to 32-63 rendered (K9 stages its stores in runs of 32), a wave entirely behind
    the camera next to one entirely rendered, three workgroups with a partial last wave, active SH degree 0 .. 3 with K = 16
    storage, and Gaussians whose colour clamps in one, two and all three channels;
(2) K9 ISOLATED (the pattern of tests/test_k8_isolation_gpu.py): msgs_backward_per_gaussian fed sums of which only the three
    colour sums are non-zero — dL/dmeans3D is then exactly the SH direction term — against float64 autograd through
    gaussian_renderer/sh.py:eval_sh at that test's tolerance.
"""
import copy

import pytest
import torch

import diff_gaussian_rasterization as dgr
import scenes
from parity_utils import BWD_RTOL, PIPE, check_backward, rel_err, report
from synthetic_model import SyntheticGaussians
from test_k8_isolation_gpu import K8_RTOL, _per_gaussian_hip, _plain_call

pytestmark = pytest.mark.gpu

W, H = 96, 64
ST = dict(filter_small=False, filter_large=False, fade_size=1.0)
BG = torch.tensor([0.1, 0.2, 0.3])
# scene name -> (P, active SH degree).  P = 193: one workgroup, its fourth wave holds one Gaussian; P = 700: three workgroups, the
# last wave of the third holds 60
CASES = {"P193_deg0": (193, 0), "P193_deg1": (193, 1), "P193_deg2": (193, 2), "P193_deg3": (193, 3), "P700_deg3": (700, 3)}
ENTRIES = ("chained", "plain", "fused", "accumulate", "factored", "depth", "camera")


@pytest.fixture(autouse=True)
def _restore():
    chain = dgr.chain_reference_getters
    yield
    dgr.chain_reference_getters = chain
    dgr.set_grad_sinks(None)


def _culled(P):
    """ranks 0-31 culled (32-63 rendered); the wave 64-127 entirely behind the camera (128-191 entirely rendered); in the larger
    scene also the first wave of the second workgroup and the upper half-run 480-511"""
    c = torch.zeros(P, dtype=torch.bool)
    c[0:32] = True
    c[64:128] = True
    if P > 256:
        c[256:320] = True
        c[480:512] = True
    return c


def _clamped(P):
    """{Gaussian: channels whose colour clamps at zero} — one, two and all three channels, in a half-culled and in a full run"""
    d = {40: (0,), 41: (0, 1), 42: (0, 1, 2), 130: (2,), 131: (1, 2), 132: (0, 1, 2), 192: (1,)}
    if P > 256:
        d.update({330: (0, 1, 2), 600: (0, 2), 699: (0, 1, 2)})
    return d


def _make(name):
    P, deg = CASES[name]
    seed = 500 + P + deg
    sc = scenes.frustum_scene(P, W, H, seed=seed, sh_degree=deg, scale_k=0.004 * 1920.0 / W * 0.5)
    g = torch.Generator().manual_seed(seed + 1)
    f = 1000.0 * W / 1920.0
    # every centre well inside the image and in front of the near plane: rendered, unless moved behind the camera below
    z = sc.means3D[:, 2].abs().clamp_min(0.6)
    x = (2.0 * torch.rand(P, generator=g) - 1.0) * 0.85 * z * (W / (2.0 * f))
    y = (2.0 * torch.rand(P, generator=g) - 1.0) * 0.85 * z * (H / (2.0 * f))
    culled = _culled(P)
    z = torch.where(culled, torch.full_like(z, -1.0), z)
    sc.means3D = torch.stack([x, y, z], 1).contiguous()
    for i, chans in _clamped(P).items():
        for c in range(3):                         # 0.282 * -5 + 0.5 = -0.91: the rest terms (0.15 sigma) cannot lift it above 0
            sc.shs[i, 0, c] = -5.0 if c in chans else 1.0
    return sc, scenes.front_camera(W, H), culled


def _second_camera():
    """the front camera moved sideways: another direction to every Gaussian (the culled ones stay behind it)"""
    import math
    import numpy as np
    f = 1000.0 * W / 1920.0
    return scenes.make_camera(np.eye(3), np.array([0.35, -0.2, 0.1]), 2.0 * math.atan(W / (2.0 * f)),
                              2.0 * math.atan(H / (2.0 * f)), W, H)


_CACHE = {}


def _case(name):
    """scene, cameras, seeds and the float32 oracle's gradients — computed once per scene, shared by every entry, never changed"""
    if name in _CACHE:
        return _CACHE[name]
    from oracle import oracle_ctypes as oc
    sc, cam, culled = _make(name)
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    with torch.no_grad():                          # what the op receives: the getters evaluated by torch on the GPU
        seen = copy.copy(sc)
        seen.scales = pc.get_scaling.cpu().contiguous()
        seen.rotations = pc.get_rotation.cpu().contiguous()
        seen.opacities = pc.get_opacity.cpu().contiguous()
        seen.shs = pc.get_features.cpu().contiguous()
        seen.means3D = pc.get_xyz.cpu().contiguous()
    seed = CASES[name][0] + CASES[name][1]
    dL = scenes.grad_seed(W, H, seed)
    dL2 = scenes.grad_seed(W, H, seed + 50)
    Gd = scenes.grad_seed(W, H, seed + 70)[0] * 0.1
    cam2 = _second_camera()
    orc = oc.rasterize(seen, cam, ST, BG)
    assert torch.equal(orc.radii > 0, ~culled), "the layout this file is about: exactly the Gaussians not moved away are rendered"
    og = oc.backward(orc, dL)
    for i, chans in _clamped(sc.P).items():        # the oracle agrees that these clamp: no gradient to their rows
        for c in chans:
            assert not og["shs"][i, :, c].any(), (i, c)
    orc2 = oc.rasterize(seen, cam2, ST, BG)
    og2 = oc.backward(orc2, dL2)
    # depth as the oracle's colour channel 0 (tests/test_depth_grad_gpu.py): colour z, no background, dz/dmeans3D added by hand
    V = cam.world_view_transform.to(torch.float32)
    m = seen.means3D
    z32 = ((V[0, 2] * m[:, 0] + V[1, 2] * m[:, 1]) + V[2, 2] * m[:, 2]) + V[3, 2]
    c32 = torch.stack([z32, torch.zeros(sc.P), torch.zeros(sc.P)], 1)
    orcz = oc.rasterize(seen, cam, ST, torch.zeros(3), use_colors_precomp=True, colors_precomp=c32)
    ogz = oc.backward(orcz, torch.stack([Gd, torch.zeros_like(Gd), torch.zeros_like(Gd)], 0))
    ogz["means3D"] = ogz["means3D"] + ogz["colors_precomp"][:, :1] * V[:3, 2][None]
    r = dict(sc=sc, seen=seen, cam=cam, cam2=cam2, culled=culled, dL=dL, dL2=dL2, Gd=Gd, orc=orc, og=og, orc2=orc2, og2=og2,
             orcz=orcz, ogz=ogz)
    _CACHE[name] = r
    return r


def _sum(oga, ogb):
    return {k: oga[k] + ogb[k] for k in ("means3D", "means2D", "opacities", "scales", "rotations")} | \
           {"shs": oga["shs"] + ogb["shs"] if "shs" in ogb else oga["shs"]}


def _clamp_rows_vanish(name, pc, culled):
    """a clamped channel receives no SH gradient, bit for bit; nor does a Gaussian that was not rendered"""
    dc, rest = pc._features_dc.grad, pc._features_rest.grad
    for i, chans in _clamped(pc._xyz.shape[0]).items():
        for c in chans:
            assert not dc[i, :, c].any() and not rest[i, :, c].any(), (name, i, c)
    idx = culled.cuda()
    for t in (pc._xyz.grad, dc, rest, pc._opacity.grad, pc._scaling.grad, pc._rotation.grad):
        assert not t[idx].any(), name
    deg = pc.active_sh_degree
    assert not rest[:, (deg + 1) ** 2 - 1:].any(), name      # coefficients beyond the active degree


def _render_entry(entry, r):
    """one forward + backward of `entry` on fresh leaves -> (pc, means2D gradient, oracle gradients, flagged Gaussians)"""
    from gaussian_renderer import render, render_fused
    sc, cam = r["sc"], r["cam"].to("cuda")
    bg, dL = BG.cuda(), r["dL"].cuda()
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    og, flagged = r["og"], r["orc"].borderline_gaussians
    if entry in ("chained", "plain"):
        dgr.chain_reference_getters = entry == "chained"
        out = render(cam, pc, PIPE, bg, **ST)
        want = "_RasterizeGaussiansChainedBackward" if entry == "chained" else "_RasterizeGaussiansBackward"
        assert type(out["render"].grad_fn).__name__ == want
        out["render"].backward(dL)
        m2 = out["viewspace_points"].grad
    elif entry == "fused":
        out = render_fused(cam, pc, PIPE, bg, **ST)
        out["render"].backward(dL)
        m2 = out["viewspace_points"].grad
    elif entry == "accumulate":
        from multi_view import ViewPipeline
        dgr.chain_reference_getters = True
        dLs = [dL, r["dL2"].cuda()]

        def bwd(i, pkg):
            pkg["render"].backward(dLs[i])
            return pkg["viewspace_points"]
        vs = ViewPipeline("cuda", n_streams=2).train_views([cam, r["cam2"].to("cuda")], pc, PIPE, bg, bwd, share_getters=True,
                                                           accumulate_in_kernel=True, **ST)
        torch.cuda.synchronize()
        m2 = vs[0].grad + vs[1].grad
        og, flagged = _sum(r["og"], r["og2"]), flagged | r["orc2"].borderline_gaussians
    elif entry == "factored":
        P = sc.P
        factor = torch.empty(P, 3, device="cuda")
        dgr.set_grad_sinks({}, sh_factor=factor)
        out = render(cam, pc, PIPE, bg, **ST)
        out["render"].backward(dL)
        dgr.set_grad_sinks(None)
        assert pc._features_dc.grad is None and pc._features_rest.grad is None      # K9 formed no rows
        row = torch.zeros(1, 3 * P + 4, device="cuda")
        row[0, :3 * P] = factor.reshape(-1)
        row[0, 3 * P:3 * P + 3] = cam.camera_center
        g_dc, g_rest = torch.empty(P, 1, 3, device="cuda"), torch.empty(P, 15, 3, device="cuda")
        dgr.sh_grad_from_views(pc._xyz.detach(), row, 1, pc.active_sh_degree, 1.0, g_dc, g_rest)
        pc._features_dc.grad, pc._features_rest.grad = g_dc, g_rest
        m2 = out["viewspace_points"].grad
    elif entry == "depth":
        out = render(cam, pc, PIPE, bg, **ST)
        ((out["render"] * dL).sum() + (out["depth"] * r["Gd"].cuda()).sum()).backward()
        m2 = out["viewspace_points"].grad
        og, flagged = _sum(r["og"], r["ogz"]), flagged | r["orcz"].borderline_gaussians
    else:
        raise KeyError(entry)
    torch.cuda.synchronize()
    return pc, m2, og, flagged


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e != "camera"])
@pytest.mark.parametrize("name", list(CASES))
def test_entries_against_the_float32_oracle(name, entry):
    r = _case(name)
    pc, m2, og, flagged = _render_entry(entry, r)
    check_backward(pc, m2, og, f"sh-jacobian {name} {entry}", rtol=BWD_RTOL, flagged=flagged)
    _clamp_rows_vanish(f"{name} {entry}", pc, r["culled"])


@pytest.mark.parametrize("depth", [False, True], ids=["colour", "colour+depth"])
@pytest.mark.parametrize("name", list(CASES))
def test_camera_entry(name, depth, monkeypatch):
    """the CAMERA variants: the per-Gaussian gradients against the float32 oracle, dL/dcampos (minus the summed direction
    gradient), dL/dviewmatrix and dL/dprojmatrix against float64 autograd at tests/test_camera_grad_gpu.py's ceiling"""
    from oracle import oracle_ctypes as oc
    from test_camera_grad_gpu import CEIL, _compare, _hip, _masked, _oracle
    r = _case(name)
    sc, cam = r["sc"], r["cam"]
    Gd = r["Gd"] if depth else None
    og64, bl = _oracle(sc, cam, ST, 1.0, PIPE, r["dL"], Gd)
    dLm, Gdm = _masked(r["dL"], Gd, bl)
    pc = None

    def keep_pc(scene, dev, requires_grad=True):
        nonlocal pc
        pc = SyntheticGaussians(scene, dev, requires_grad=requires_grad)
        return pc
    import test_camera_grad_gpu as tc
    monkeypatch.setattr(tc, "SyntheticGaussians", keep_pc)        # (_hip returns the gradients; check_backward wants the model)
    out, g, cg = _hip(sc, cam, ST, 1.0, PIPE, dLm, Gdm, entry="chained", bg=BG)
    assert cg["cp"] is not None
    if CASES[name][1] == 0:
        # degree 0: the colour does not depend on the direction — campos receives nothing
        assert not cg["cp"].any(), name
        og64 = {k: v for k, v in og64.items() if k != "cp"}
    _compare(f"sh-jacobian {name} camera/{'depth' if depth else 'colour'}", cg, og64, CEIL)
    og = oc.backward(r["orc"], dLm)
    flagged = r["orc"].borderline_gaussians
    if depth:
        ogz = oc.backward(r["orcz"], torch.stack([Gdm, torch.zeros_like(Gdm), torch.zeros_like(Gdm)], 0))
        V = cam.world_view_transform.to(torch.float32)
        ogz["means3D"] = ogz["means3D"] + ogz["colors_precomp"][:, :1] * V[:3, 2][None]
        og, flagged = _sum(og, ogz), flagged | r["orcz"].borderline_gaussians
    check_backward(pc, out["viewspace_points"].grad, og, f"sh-jacobian {name} camera", rtol=BWD_RTOL, flagged=flagged)
    _clamp_rows_vanish(f"{name} camera", pc, r["culled"])


@pytest.mark.parametrize("name", list(CASES))
def test_direction_term_isolated_against_float64_autograd(name):
    """only the three colour sums non-zero: dL/dmeans3D is the SH direction term alone, dL/dSH the basis x dL/drgb rows"""
    from gaussian_renderer.sh import eval_sh
    r = _case(name)
    seen, cam, culled = r["seen"], r["cam"], r["culled"]
    P, deg = seen.P, seen.sh_degree
    call = _plain_call(seen, cam, ST, BG)
    with torch.no_grad():
        _, _, _, radii, _, (geom, _, _, _) = dgr._forward_impl(call)
    assert torch.equal(radii.cpu() > 0, ~culled)
    gen = torch.Generator().manual_seed(7 + P + deg)
    sums = torch.zeros(P, 9, dtype=torch.float64)
    sums[:, 6:9] = torch.randn(P, 3, generator=gen, dtype=torch.float64).float().double()
    got = _per_gaussian_hip(call, radii, geom, sums)

    dt = torch.float64
    p = seen.means3D.to(dt).clone().requires_grad_(True)
    sh = seen.shs.to(dt).clone().requires_grad_(True)                       # [P, 16, 3]
    d = p - cam.camera_center.to(dt)[None]
    d = d / d.norm(dim=1, keepdim=True)
    col = torch.clamp_min(eval_sh(deg, sh.transpose(1, 2), d) + 0.5, 0.0)   # [P, 3]
    (col * sums[:, 6:9] * (~culled)[:, None].to(dt)).sum().backward()
    for i, chans in _clamped(P).items():
        for c in chans:
            assert col[i, c] == 0, (i, c)
    e_sh = rel_err(got["shs"], sh.grad)
    report(f"sh-jacobian {name} isolated", "shs", e_sh)
    assert e_sh <= K8_RTOL
    for k in ("opacities", "scales", "rotations", "means2D"):
        assert not got[k].any(), k
    if deg == 0:
        assert not got["means3D"].any()          # J = 0: bit for bit nothing
        return
    e = rel_err(got["means3D"], p.grad)
    report(f"sh-jacobian {name} isolated", "means3D (SH direction term)", e)
    assert e <= K8_RTOL, e
    assert not got["means3D"][culled.cuda()].any()
    for i, chans in _clamped(P).items():
        if len(chans) == 3:
            assert not got["means3D"][i].any(), i            # every channel clamped: its share of the direction term vanishes

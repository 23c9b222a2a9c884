"""Antialiasing (SPEC M14) without a GPU: the float64 truth helper of tests/antialias_truth.py is pinned against
closed forms, the test scenes have the properties the GPU tests rely on, and the new surface — three C entries,
screen_compensation(), GaussianRasterizer.with_antialiasing(), render_with_antialiasing() — is what the documents say.

S2's floored rows: the scene (seed 8, scale_k x 0.05) has exactly 2 floored rows among its 296 in front of the near plane
(0.68 %), the next ratio det0 / det1 being 3.0e-5 against the floor's 2.5e-5; the count is asserted as it is, and that the
floor stays rare (<= 5 %)."""
import ctypes as C
import inspect
import math
import os

import pytest
import torch

import antialias_truth as at
import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msgs_screen_compensation_forward", "msgs_screen_compensation_backward", "msgs_screen_compensation_scratch_bytes")


def _on_axis(sigmas_px, W=40, H=24, z=5.0):
    """isotropic Gaussians on the optical axis of front_camera(W, H) whose footprints have the given standard deviations in
    pixels: (rho, floored, regular)"""
    cam = scenes.front_camera(W, H)
    fx = W / (2.0 * math.tan(0.5 * cam.FoVx))
    n = len(sigmas_px)
    s = torch.tensor(sigmas_px, dtype=torch.float64) * z / fx
    means = torch.tensor([[0.0, 0.0, z]], dtype=torch.float64).repeat(n, 1)
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64).repeat(n, 1)
    return at.rho(means, at.view_of(cam), scales=s[:, None].repeat(1, 3), rotations=q)


def test_truth_of_an_isotropic_gaussian_on_the_axis():
    sig = [0.1, 0.5, 1.0, 3.0]
    rho, floored, regular = _on_axis(sig)
    assert regular.all() and not floored.any()
    want = torch.tensor([s * s / (s * s + 0.3) for s in sig], dtype=torch.float64)
    # tan(FoV / 2) is rounded to float32 in the view, as for the op: 1e-7 relative on sigma
    assert torch.allclose(rho, want, rtol=1e-6, atol=0.0), (rho, want)


def test_truth_goes_to_one_for_large_footprints_and_stops_at_the_floor():
    rho, floored, _ = _on_axis([30.0, 300.0, 0.03, 1e-3])
    assert 0.999 < rho[0] < 1.0 and 0.99999 < rho[1] <= 1.0 and not floored[:2].any()
    assert floored[2:].all() and rho[2].item() == rho[3].item() == math.sqrt(at.FLOOR)
    assert abs(math.sqrt(at.FLOOR) - 0.005) < 1e-15


def test_truth_is_one_behind_the_near_plane():
    cam = scenes.front_camera(40, 24)
    means = torch.tensor([[0.0, 0.0, 0.2], [0.0, 0.0, -1.0], [0.0, 0.0, 0.25]], dtype=torch.float64, requires_grad=True)
    s = torch.full((3, 3), 1e-3, dtype=torch.float64, requires_grad=True)
    q = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64).repeat(3, 1)
    rho, floored, regular = at.rho(means, at.view_of(cam), scales=s, rotations=q)
    assert regular.tolist() == [False, False, True] and rho[:2].tolist() == [1.0, 1.0] and 0.005 < rho[2] < 1.0
    rho.sum().backward()
    assert not means.grad[:2].any() and not s.grad[:2].any()
    assert s.grad[2, :2].abs().min() > 0                         # (on the axis the depth-wise scale does not enter)


def test_scene_properties():
    front, lo, hi, floored = {}, {}, {}, {}
    for name in ("S1", "S2", "S3", "S2q"):
        sc, cam = at.scene(name)
        t = at.truth(sc, cam, at.seed(sc.P))
        reg = t["regular"]
        front[name], floored[name] = int(reg.sum()), int(t["floored"].sum())
        lo[name], hi[name] = t["rho"][reg].min().item(), t["rho"][reg].max().item()
        assert torch.equal(t["rho"][~reg], torch.ones(int((~reg).sum()), dtype=torch.float64))
        for k in ("means3D", "scales", "rotations"):
            assert not t[k][~reg].any() and not t[k][t["floored"]].any(), (name, k)
    assert front == {"S1": 297, "S2": 296, "S3": 293, "S2q": 296}
    assert floored == {"S1": 0, "S2": 2, "S3": 0, "S2q": 0}
    assert floored["S2"] <= 0.05 * front["S2"]
    assert 0.64 < lo["S1"] < 0.66 and 0.98 < hi["S1"] < 0.99
    assert lo["S2"] == 0.005 and 0.24 < hi["S2"] < 0.25
    assert lo["S3"] > 0.96
    # the slices: a tail wave, and a second workgroup of one lane
    assert at.scene("S1:1")[0].P == 1 and at.scene("S1:257")[0].P == 257
    assert torch.equal(at.scene("S1:257")[0].means3D, at.scene("S1")[0].means3D[:257])


def test_truth_with_precomputed_covariance_and_scale_modifier_agrees():
    sc, cam = at.scene("S1")
    g = at.seed(sc.P)
    a, b = at.truth(sc, cam, g, 0.7), at.truth(sc, cam, g, 0.7, precomp=True)
    assert (a["o_eff"] - b["o_eff"]).abs().max() < 1e-6           # (the covariance is rounded to float32, as the op is fed it)
    assert (a["means3D"] - b["means3D"]).abs().max() < 1e-5 * a["means3D"].abs().max()
    assert b["cov3D_input"].dtype == torch.float32 and b["cov3D_precomp"].shape == (sc.P, 6)


def test_three_symbols_are_exported_and_declared():
    import diff_gaussian_rasterization as dgr
    lib = dgr._C.lib
    assert lib.msgs_abi_version() == 11
    header = open(os.path.join(ROOT, "include", "msgs.h")).read()
    for n in NAMES:
        assert n in dgr._C.EXPORTS and hasattr(lib, n) and f" {n}(" in header, n
    assert "screen_compensation" in dgr.__all__ and callable(dgr.screen_compensation)
    # twelve doubles per workgroup of 256 Gaussians
    assert [lib.msgs_screen_compensation_scratch_bytes(P) for P in (0, 1, 256, 257, 10**6)] == [96, 96, 96, 192, 96 * 3907]


def _settings():
    import diff_gaussian_rasterization as dgr
    return dgr.GaussianRasterizationSettings(4, 6, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                             False, False)


def test_c_entries_refuse_what_they_do_not_offer_without_a_launch():
    import diff_gaussian_rasterization as dgr
    lib, B = dgr._C.lib, dgr._C
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    view = B.View(4, 6, 1.0, 1.0, 1.0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, None, p, None, None)

    def gaussians(P=3, raw=0, scales=p, rotations=p, cov=None):
        return B.Gaussians(P, raw, p, None, None, p, scales, rotations, cov, None, None, None, None, None, None, None, None)

    fwd = lambda g, v=view: lib.msgs_screen_compensation_forward(C.byref(v), C.byref(g), p, None)
    bwd = lambda g, dV=None, scratch=None, n=0, dsc=None, dcov=None: lib.msgs_screen_compensation_backward(
        C.byref(view), C.byref(g), p, p, p, dsc, None, dcov, dV, scratch, n, None)
    for raw in (1, 2):
        assert fwd(gaussians(raw=raw)) == -1 and bwd(gaussians(raw=raw)) == -1
    assert fwd(gaussians(scales=None)) == -1 and fwd(gaussians(rotations=None)) == -1          # half a pair
    assert fwd(gaussians(scales=None, rotations=None)) == -1 and bwd(gaussians(scales=None, rotations=None)) == -1
    assert fwd(gaussians(cov=p)) == -1                                                            # both
    assert fwd(gaussians(P=-1)) == -1
    no_v = B.View(4, 6, 1.0, 1.0, 1.0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, None, None, None, None)
    assert fwd(gaussians(), no_v) == -1
    assert lib.msgs_screen_compensation_forward(C.byref(view), C.byref(gaussians()), None, None) == -1
    # a gradient for a tensor the inputs do not carry, camera sums without their scratch, too little of it
    assert bwd(gaussians(), dcov=p) == -1 and bwd(gaussians(scales=None, rotations=None, cov=p), dsc=p) == -1
    assert bwd(gaussians(), dV=p) == -1 and bwd(gaussians(P=300), dV=p, scratch=p, n=96) == -2
    # no Gaussian: nothing is launched
    assert fwd(gaussians(P=0, scales=None, rotations=None)) == 0 and bwd(gaussians(P=0)) == 0
    with pytest.raises(ValueError):
        B.check(-1, "msgs_screen_compensation_forward")


def test_with_antialiasing_copies_the_module_it_came_from():
    import diff_gaussian_rasterization as dgr
    r = dgr.GaussianRasterizer(_settings(), return_alpha=True, absgrad=True)
    assert r.antialiasing is False
    f = torch.zeros(3, 5)
    src = r.with_features(f).with_distortion()
    a = src.with_antialiasing()
    assert a is not src and a.antialiasing is True and src.antialiasing is False
    assert a.features is f and a.return_distortion is True and a.return_alpha is True and a.absgrad is True
    assert a.raster_settings is r.raster_settings
    # ... and the other copies carry the flag on
    assert a.with_distortion(False).antialiasing is True and a.with_distortion(False).return_distortion is False
    assert a.with_features(None).antialiasing is True and a.with_features(None).features is None
    assert a.with_antialiasing(False).antialiasing is False and a.with_antialiasing(False).features is f
    # __init__ keeps its pinned parameters and the settings their 15 fields
    assert list(inspect.signature(dgr.GaussianRasterizer.__init__).parameters) == ["self", "raster_settings", "return_alpha",
                                                                                  "absgrad"]
    assert len(dgr.GaussianRasterizationSettings._fields) == 15
    assert list(inspect.signature(dgr.screen_compensation).parameters) == ["means3D", "opacities", "raster_settings", "scales",
                                                                           "rotations", "cov3D_precomp"]


def test_forward_raw_under_antialiasing_raises_before_any_launch():
    import diff_gaussian_rasterization as dgr
    z = lambda *s: torch.zeros(*s)
    r = dgr.GaussianRasterizer(_settings()).with_antialiasing()
    with pytest.raises(ValueError, match="with_antialiasing"):
        r.forward_raw(z(4, 3), z(4, 3), z(4, 1, 3), z(4, 15, 3), z(4, 1), z(4, 3), z(4, 4))


def test_no_cpu_path_and_the_covariance_rule():
    import diff_gaussian_rasterization as dgr
    z = lambda *s: torch.zeros(*s)
    rs = _settings()
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.screen_compensation(z(2, 3), z(2, 1), rs, scales=z(2, 3), rotations=z(2, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.GaussianRasterizer(rs).with_antialiasing()(means3D=z(2, 3), means2D=z(2, 3), opacities=z(2, 1), shs=z(2, 16, 3),
                                                       scales=z(2, 3), rotations=z(2, 4))
    for kw in (dict(), dict(scales=z(2, 3)), dict(scales=z(2, 3), rotations=z(2, 4), cov3D_precomp=z(2, 6))):
        with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
            dgr.screen_compensation(z(2, 3), z(2, 1), rs, **kw)


def test_host_entry_has_the_signature_of_render():
    import gaussian_renderer as gr
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    assert sig(gr.render_with_antialiasing) == sig(gr.render)

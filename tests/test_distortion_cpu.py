"""Depth distortion without a GPU (SPEC M13; 4.13):
  * the committed fixture tests/golden/distortion_truth.npz is what its generator computes;
  * the generator's restated blend loop is the oracle's: its sum w, sum w z, counted pairs and borderline mask against
    torch_oracle.rasterize's 1 - final_T, depth map, n_blended and mask;
  * the signed list-order definition equals the all-ordered-pairs |z_i - z_j| form of Mip-NeRF 360 on these (depth-sorted) lists,
    and the closed forms the kernels walk (forward sum, dDist/dw_i, dDist/dz_i) equal the definition and its autograd in float64;
  * the float32 restatement of the forward formula on the "far" scene: useless unshifted, exact to rounding with z - z_ref —
    the two numbers behind the bound of tests/test_distortion_gpu.py;
  * the Python surface and the guards that need no device."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "distortion_truth.npz")


def _generator():
    spec = importlib.util.spec_from_file_location("make_distortion_golden", os.path.join(ROOT, "tests", "golden",
                                                                                         "make_distortion_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def gen():
    return _generator()


@pytest.fixture(scope="module")
def restated(gen):
    return {k: gen.restated(k) for k in gen.SCENES}


def test_fixture_is_what_the_generator_computes(gen):
    want = gen.compute()
    got = np.load(GOLDEN)
    assert sorted(got.files) == sorted(want)
    for s in gen.SCENES:
        for k in ("borderline", "visible", "G", "count"):
            k = f"{s}_{k}"
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
        for k in ("map", "means3D", "opacities", "scales", "rotations", "means2D"):
            k = f"{s}_{k}"
            assert got[k].dtype == np.float64 and got[k].shape == want[k].shape
            assert np.abs(got[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k


def test_fixture_properties(gen):
    t = np.load(GOLDEN)
    P, H, W = gen.P, gen.H, gen.W
    for s in gen.SCENES:
        g = lambda k: t[f"{s}_{k}"]
        bl, vis = g("borderline"), g("visible")
        assert bl.shape == (H, W) and bl.sum() <= gen.MAX_BORDERLINE * W * H
        assert vis.sum() >= 150
        G = g("G")
        assert G.shape == (H, W) and G.dtype == np.float32 and not G[bl].any() and np.abs(G[~bl]).min() > 0
        assert g("count").min() >= 2                                   # every pixel has a pair to spread
        assert g("map").shape == (H, W) and g("map").min() > 0.5 and g("map").max() < 4.0
        for k, shape in (("means3D", (P, 3)), ("opacities", (P, 1)), ("scales", (P, 3)), ("rotations", (P, 4)), ("means2D", (P, 3))):
            assert g(k).shape == shape and np.isfinite(g(k)).all() and np.abs(g(k)).max() > 0, k
            assert not g(k)[~vis].any(), k
        assert (g("means3D")[:, 2] != 0).sum() >= 150                  # the dL/dz share is everywhere
        assert not g("means2D")[:, 2].any()
    # the same picture from 2000 units away: the same map, a depth gradient that does not care about the offset
    assert np.abs(t["far_map"] - t["F_map"]).max() <= 2e-3 * t["F_map"].max()
    sc = gen.scene("far")[0]
    assert sc.means3D.dtype == torch.float32 and (sc.means3D[:, 2] > 2000).sum() >= 150


@pytest.mark.parametrize("kind", ["F", "far"])
def test_restated_loop_is_the_oracles(gen, restated, kind):
    from oracle import torch_oracle as to
    r = restated[kind]
    sc = r["scene"]
    means3D, opac, scales, rots, _ = r["leaves"]
    with torch.no_grad():
        _, _, depth, _, _, aux = to.rasterize(means3D, opac, r["view"], torch.zeros(3, dtype=torch.float64), scales=scales,
                                              rotations=rots, shs=sc.shs, max_pixel_sizes=sc.max_pixel_sizes,
                                              min_pixel_sizes=sc.min_pixel_sizes, base_mask=sc.base_mask)
    e_w = (r["wsum"] - (1.0 - aux["final_T"])).abs().max().item()
    e_z = ((r["wzsum"] - depth).abs().max() / depth.abs().max()).item()
    print(f"{kind}: sum w {e_w:.2e}  sum w z {e_z:.2e}")
    assert e_w <= 1e-12 and e_z <= 1e-12
    assert torch.equal(r["count"], aux["n_blended"])
    assert torch.equal(r["borderline"], aux["borderline"])


def _closed_forms(w, z):
    """float64, one tile: (Dist by the kernels' forward sum, dDist/dw [n,npix], dDist/dz [n,npix]) from w [n,npix], z [n]:
    T_i = 1 - sum_{j<i} w_j, T_{i+1} = T_i - w_i, T_f = 1 - sum w, R_i = sum_{k>i} w_k z_k, M = sum w z, B_i = 1 + T_f - T_i - T_{i+1}"""
    wz = w * z[:, None]
    Ti = 1.0 - (torch.cumsum(w, 0) - w)
    Tn = Ti - w
    Tf = 1.0 - w.sum(0, keepdim=True)
    M = wz.sum(0, keepdim=True)
    R = M - torch.cumsum(wz, 0)
    B = 1.0 + Tf - Ti - Tn
    dist = 2.0 * (w * (R - z[:, None] * (Tn - Tf))).sum(0)
    dw = 2.0 * (z[:, None] * B - M + 2.0 * R + wz)
    dz = 2.0 * w * B
    return dist, dw, dz


@pytest.mark.parametrize("kind", ["F", "far"])
def test_definition_pairs_form_and_closed_forms(gen, restated, kind):
    worst = dict(pairs=0.0, fwd=0.0, dw=0.0, dz=0.0, shift=0.0)
    for (x0, x1, y0, y1, w, z) in restated[kind]["tiles"]:
        assert bool((z[1:] >= z[:-1]).all())                           # the list is depth-sorted
        d = gen.distortion_of(w, z)
        pairs = (w[:, None, :] * w[None, :, :] * (z[:, None] - z[None, :]).abs()[:, :, None]).sum((0, 1))
        scale = d.abs().max().item()
        worst["pairs"] = max(worst["pairs"], (d - pairs).abs().max().item() / scale)
        wl, zl = w.clone().requires_grad_(True), z.clone().requires_grad_(True)
        gen.distortion_of(wl, zl).sum().backward()
        zs = z - z[0]                                                  # the kernels' shift: nothing may depend on it
        for zz, key in ((z, "fwd"), (zs, "shift")):
            f, dw, dz = _closed_forms(w, zz)
            worst[key] = max(worst[key], (f - d).abs().max().item() / scale)
            worst["dw"] = max(worst["dw"], (dw - wl.grad).abs().max().item() / wl.grad.abs().max().item())
            worst["dz"] = max(worst["dz"], (dz.sum(1) - zl.grad).abs().max().item() / zl.grad.abs().max().item())
    print(kind, worst)
    tol = 1e-12 if kind == "F" else 1e-9                               # (far, unshifted: float64 itself cancels 2000 / spread)
    assert all(v <= tol for v in worst.values()), worst


def forward_f32(w, z, shifted):
    """the kernels' forward sum restated in float32 numpy (back to front, exact weights rounded to float32):
    Dist = 2 sum_i w_i (R_i - z~_i (T_{i+1} - T_f)),  z~ = z - z_ref with z_ref the first entry's depth (shifted) or 0"""
    f = np.float32
    w64 = w.numpy()
    Tn = (1.0 - np.cumsum(w64, 0)).astype(f)                           # T_{i+1}
    Tf = (1.0 - w64.sum(0)).astype(f)
    w32, z32 = w64.astype(f), z.numpy().astype(f)
    assert np.array_equal(z32.astype(np.float64), z.numpy())           # the float32 depths are the truth's, exactly
    zref = z32[0] if shifted else f(0)
    acc, R = np.zeros(w32.shape[1], f), np.zeros(w32.shape[1], f)
    for i in range(w32.shape[0] - 1, -1, -1):
        zt = f(z32[i] - zref)
        acc = acc + w32[i] * (R - zt * (Tn[i] - Tf))
        R = R + w32[i] * zt
    return f(2) * acc


def test_float32_restatement_needs_the_shift(gen, restated):
    err = {False: 0.0, True: 0.0}
    top = max(gen.distortion_of(w, z).max().item() for (*_, w, z) in restated["far"]["tiles"])
    for (x0, x1, y0, y1, w, z) in restated["far"]["tiles"]:
        d = gen.distortion_of(w, z).numpy()
        for shifted in err:
            err[shifted] = max(err[shifted], np.abs(forward_f32(w, z, shifted).astype(np.float64) - d).max() / top)
    print(f"far, float32 restatement: unshifted {err[False]:.3e}  shifted {err[True]:.3e}  (of max Dist)")
    assert err[False] >= 5e-5          # a tenth of which is the GPU test's bound: only a shifted kernel can meet it
    assert err[True] <= 1e-6


# ---------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------------------------------
def _settings():
    import diff_gaussian_rasterization as dgr
    return dgr.GaussianRasterizationSettings(4, 6, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                             False, False)


def test_wrapper_surface():
    import diff_gaussian_rasterization as dgr
    import gaussian_renderer as gr
    r = dgr.GaussianRasterizer(_settings(), return_alpha=True, absgrad=True)
    assert r.return_distortion is False
    r2 = r.with_distortion()
    assert r2 is not r and r2.return_distortion is True and r.return_distortion is False
    assert r2.return_alpha is True and r2.absgrad is True and r2.raster_settings is r.raster_settings
    f = torch.zeros(3, 5)
    assert r2.with_features(f).return_distortion is True and r.with_features(f).with_distortion().features is f
    assert r2.with_distortion(False).return_distortion is False
    for fn in (dgr.rasterize_gaussians, dgr.rasterize_gaussians_raw):
        p = inspect.signature(fn).parameters
        assert p["return_distortion"].default is False and list(p)[-1] == "return_alpha", fn.__name__
    assert inspect.signature(dgr.GaussianRasterizer.forward_raw).parameters["return_distortion"].default is None
    assert "absgrad" in dgr.GaussianRasterizer.with_distortion.__doc__
    # the trailing inputs: nothing unless asked; the marker behind absgrad's and in front of the features
    rs = _settings()
    assert dgr._extra_inputs(rs) == ()
    assert dgr._extra_inputs(rs, return_distortion=True) == (dgr._DISTORTION,)
    assert dgr._extra_inputs(rs, True, return_distortion=True) == (dgr._ALPHA, dgr._DISTORTION)
    m2 = torch.zeros(3, 3)
    extra = dgr._extra_inputs(rs, True, True, m2, return_distortion=True)
    assert len(extra) == 3 and extra[0] is dgr._ALPHA and extra[1].means2D() is m2 and extra[2] is dgr._DISTORTION
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(gr.render_with_distortion) == [
        ("viewpoint_camera", E), ("pc", E), ("pipe", E), ("bg_color", E), ("scaling_modifier", 1.0), ("override_color", None),
        ("filter_small", False), ("filter_large", False), ("fade_size", 1.0), ("fused", False), ("alpha", False)]
    assert gr.RESULT_KEYS == ("render", "acc_pixel_size", "depth", "viewspace_points", "visibility_filter", "radii",
                              "pixel_sizes")


def test_c_abi_has_the_two_entries_and_keeps_its_version():
    import diff_gaussian_rasterization as dgr
    lib = dgr._C.lib
    assert lib.msgs_abi_version() == 11
    for name in ("msgs_distortion_forward", "msgs_distortion_backward"):
        assert name in dgr._C.EXPORTS and hasattr(lib, name)
    header = open(os.path.join(ROOT, "include", "msgs.h")).read()
    assert "int msgs_distortion_forward(" in header and "int msgs_distortion_backward(" in header


def test_verification_mode_is_refused_before_any_launch():
    import diff_gaussian_rasterization as dgr
    z = lambda *s: torch.zeros(*s)
    args = dict(means3D=z(4, 3), means2D=z(4, 3), opacities=z(4, 1), shs=z(4, 16, 3), scales=z(4, 3), rotations=z(4, 4))
    r = dgr.GaussianRasterizer(_settings()).with_distortion()
    prev = dgr.set_deterministic(True)
    try:
        with pytest.raises(ValueError, match="verification mode"):
            r(**args)
    finally:
        dgr.set_deterministic(prev)

"""CPU checks of absgrad, the absolute screen-space gradient for densification (SPEC M10; include/msgs.h
msgs_absgrad):
- the two C entries are declared, exported and listed; ABI and struct sizes unchanged; the scratch query is sane;
- the opt-in surface exists (GaussianRasterizer(..., absgrad=True), rasterize_gaussians*(absgrad=), render_with_absgrad,
  update_training_stats / fused_train_iteration*(absgrad=)) and forward()'s parameters are what they were;
- the float64 fixture of tests/test_absgrad_gpu.py (tests/golden/absgrad_truth.npz) is what its generator computes from
  oracle/torch_oracle.py, and it separates absgrad from |grad| by a wide margin: an implementation that returned |grad|
  could not pass the comparison."""
import ctypes as C
import importlib.util
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("msgs_absgrad_scratch_bytes", "msgs_absgrad")
GOLDEN = os.path.join(ROOT, "tests", "golden", "absgrad_truth.npz")


def test_header_declares_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msgs.h")).read(), flags=re.S)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert re.search(r"size_t\s+msgs_absgrad_scratch_bytes\s*\(\s*int32_t\s+P\s*\)\s*;", src)
    args = norm(re.search(r"int\s+msgs_absgrad\s*\((.*?)\)\s*;", src, flags=re.S).group(1))
    assert args == norm("""const msgs_view_t* view, int32_t P, const void* geom, size_t geom_bytes, int64_t num_instances,
                           const void* binning, size_t binning_bytes, const void* image_state, size_t image_bytes,
                           const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                           void* scratch, size_t scratch_bytes, float* out_absgrad, void* stream""")


def test_library_exports_and_lists_them():
    import diff_gaussian_rasterization as dgr
    for n in NEW:
        assert hasattr(dgr._C.lib, n), n
        assert n in dgr._C.EXPORTS, n
    assert len(dgr._C.lib.msgs_absgrad.argtypes) == 16
    assert dgr._C.lib.msgs_abi_version() == dgr._C.ABI_VERSION == 11
    assert C.sizeof(dgr._C.Grads) == 120


def test_scratch_query():
    import diff_gaussian_rasterization as dgr
    q = dgr._C.lib.msgs_absgrad_scratch_bytes
    prev = 0
    for P in (0, 1, 7, 1000, 10**6, 5 * 10**6):
        n = q(P)
        assert n >= 16 * P and n >= prev and n % 8 == 0, (P, n)
        prev = n
    assert 0 < q(0) <= 4096 and q(-5) == q(0)
    assert q(10**6) <= 32 * 10**6


def test_wrapper_takes_absgrad():
    import torch

    import diff_gaussian_rasterization as dgr
    rs = dgr.GaussianRasterizationSettings(4, 4, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                           False, False)
    p = inspect.signature(dgr.GaussianRasterizer.__init__).parameters
    assert list(p) == ["self", "raster_settings", "return_alpha", "absgrad"] and p["absgrad"].default is False
    assert dgr.GaussianRasterizer(rs).absgrad is False
    assert dgr.GaussianRasterizer(rs, absgrad=True).absgrad is True
    r = dgr.GaussianRasterizer(rs, return_alpha=True, absgrad=True)
    assert r.absgrad is True and r.return_alpha is True
    for fn in (dgr.rasterize_gaussians, dgr.rasterize_gaussians_raw):
        p = inspect.signature(fn).parameters
        assert p["absgrad"].default is False and p["return_alpha"].default is False, fn.__name__
    # forward()'s parameters: the reference's 13, unchanged
    assert list(inspect.signature(dgr.GaussianRasterizer.forward).parameters) == [
        "self", "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp",
        "max_pixel_sizes", "min_pixel_sizes", "occ_multiplier", "dc_delta", "base_mask"]


def test_a_call_without_absgrad_passes_what_it_passed():
    """the trailing inputs of the autograd Functions: nothing is added unless asked, the marker comes last and holds a weak
    reference to the caller's means2D"""
    import torch

    import diff_gaussian_rasterization as dgr
    rs = dgr.GaussianRasterizationSettings(4, 4, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                           False, False)
    assert dgr._extra_inputs(rs) == ()
    assert dgr._extra_inputs(rs, True) == (dgr._ALPHA,)
    m2 = torch.zeros(3, 3)
    extra = dgr._extra_inputs(rs, True, True, m2)
    assert len(extra) == 2 and extra[0] is dgr._ALPHA and extra[1].means2D() is m2
    extra = dgr._extra_inputs(rs, False, True, m2)
    assert len(extra) == 1 and extra[0].means2D() is m2
    del m2
    assert extra[0].means2D() is None


def test_host_layer_signatures():
    import gaussian_renderer as gr
    import train_epilogue
    import train_step
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(gr.render_with_absgrad) == [
        ("viewpoint_camera", E), ("pc", E), ("pipe", E), ("bg_color", E), ("scaling_modifier", 1.0), ("override_color", None),
        ("filter_small", False), ("filter_large", False), ("fade_size", 1.0), ("fused", False), ("alpha", False)]
    assert list(inspect.signature(gr.render).parameters) == [
        "viewpoint_camera", "pc", "pipe", "bg_color", "scaling_modifier", "override_color", "filter_small", "filter_large",
        "fade_size"]
    for f in (train_epilogue.update_training_stats, train_step.fused_train_iteration, train_step.fused_train_iteration_views):
        p = inspect.signature(f).parameters["absgrad"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, f.__name__


def _generator():
    spec = importlib.util.spec_from_file_location("make_absgrad_golden", os.path.join(ROOT, "tests", "golden",
                                                                                      "make_absgrad_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fixture_is_what_the_oracle_computes():
    gen = _generator()
    want = gen.compute()
    got = np.load(GOLDEN)
    assert sorted(got.files) == sorted(want)
    for k in ("borderline", "visible"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("absgrad", "grad"):
        assert got[k].dtype == np.float64 and got[k].shape == (gen.P, 2)
        scale = np.abs(want[k]).max()
        assert np.abs(got[k] - want[k]).max() <= 1e-12 * scale, k


def test_fixture_separates_absgrad_from_the_net_gradient():
    gen = _generator()
    t = np.load(GOLDEN)
    a, g, vis = t["absgrad"], t["grad"], t["visible"]
    assert t["borderline"].shape == (gen.H, gen.W) and t["borderline"].sum() <= gen.MAX_BORDERLINE * gen.W * gen.H
    assert vis.sum() >= 150
    assert (a >= 0).all() and np.isfinite(a).all()
    assert (a >= np.abs(g) * (1 - 1e-12)).all()                   # the triangle inequality, componentwise
    assert (a[~vis] == 0).all() and (g[~vis] == 0).all()
    na, ng = np.linalg.norm(a, axis=1), np.linalg.norm(g, axis=1)
    assert ((na > 1.5 * ng) & vis).sum() >= 0.9 * vis.sum()
    assert np.abs(a).sum() > 4 * np.abs(g).sum()

"""CPU checks of the feature channels (SPEC M12; include/msgs.h msgs_features_*):
- the three C entries are declared, prototyped, exported and listed; ABI and struct sizes unchanged; the scratch query is sane;
  refused calls need no device;
- the opt-in surface exists (GaussianRasterizer.with_features, forward_raw / rasterize_gaussians* by keyword,
  host render_with_features) and the pinned signatures are what they were;
- the guards of the Python layer raise without a device; a model without Gaussians needs none;
- the float64 fixture of tests/test_features_gpu.py (tests/golden/features_truth.npz) is what its generator computes from
  oracle/torch_oracle.py, and it has the properties the GPU comparison leans on."""
import ctypes as C
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("msgs_features_scratch_bytes", "msgs_features_forward", "msgs_features_backward")
GOLDEN = os.path.join(ROOT, "tests", "golden", "features_truth.npz")


# ---------------------------------------------------------------------------------------------------------------------------
# the C boundary
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msgs.h")).read(), flags=re.S)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert re.search(r"size_t\s+msgs_features_scratch_bytes\s*\(\s*int32_t\s+P\s*,\s*int32_t\s+C\s*\)\s*;", src)
    args = norm(re.search(r"int\s+msgs_features_forward\s*\((.*?)\)\s*;", src, flags=re.S).group(1))
    assert args == norm("""const msgs_view_t* view, int32_t P, const void* geom, size_t geom_bytes, int64_t num_instances,
                           const void* binning, size_t binning_bytes, const void* image_state, size_t image_bytes,
                           const float* features, int32_t C, float* out, void* stream""")
    args = norm(re.search(r"int\s+msgs_features_backward\s*\((.*?)\)\s*;", src, flags=re.S).group(1))
    assert args == norm("""const msgs_view_t* view, int32_t P, const void* geom, size_t geom_bytes, int64_t num_instances,
                           const void* binning, size_t binning_bytes, const void* image_state, size_t image_bytes,
                           const float* features, int32_t C, const float* dL_dfeature_map, void* grad_records,
                           size_t grad_records_bytes, void* scratch, size_t scratch_bytes, float* dL_dfeatures, void* stream""")
    assert "MSGS_ABI_VERSION 11" in re.sub(r"\s+", " ", src)


def test_library_exports_prototypes_and_lists_them():
    import diff_gaussian_rasterization as dgr
    lib = dgr._C.lib
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in dgr._C.EXPORTS, n
    vp, sz = C.c_void_p, C.c_size_t
    assert lib.msgs_features_scratch_bytes.argtypes == [C.c_int32, C.c_int32] and lib.msgs_features_scratch_bytes.restype is sz
    assert lib.msgs_features_forward.argtypes == [C.POINTER(dgr._C.View), C.c_int32, vp, sz, C.c_int64, vp, sz, vp, sz, vp,
                                                  C.c_int32, vp, vp]
    assert lib.msgs_features_backward.argtypes == [C.POINTER(dgr._C.View), C.c_int32, vp, sz, C.c_int64, vp, sz, vp, sz, vp,
                                                   C.c_int32, vp, vp, sz, vp, sz, vp, vp]
    assert lib.msgs_features_forward.restype is C.c_int and lib.msgs_features_backward.restype is C.c_int
    assert lib.msgs_abi_version() == dgr._C.ABI_VERSION == 11
    assert C.sizeof(dgr._C.Grads) == 120 and C.sizeof(dgr._C.View) == 96


def test_scratch_query():
    import diff_gaussian_rasterization as dgr
    q = dgr._C.lib.msgs_features_scratch_bytes
    prev = 0
    for P in (0, 1, 7, 1000, 10**6, 5 * 10**6):
        n = q(P, 16)
        assert n >= 8 * P and n >= prev and n % 8 == 0, (P, n)        # at least one double per Gaussian
        assert q(P, 1) == n == q(P, 1000)                             # one block of channels at a time, whatever C is
        prev = n
    assert 0 < q(0, 5) <= 4096 and q(-5, 5) == q(0, 5)
    assert q(10**6, 64) <= 128 * 10**6


def test_refused_calls_need_no_device():
    """argument checks come before any launch: NULL and short buffers are refused on a machine without a GPU too"""
    import diff_gaussian_rasterization as dgr
    lib = dgr._C.lib
    view = dgr._C.View(24, 40, 0.5, 0.3, 1.0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, None, None, None, None)
    buf = (C.c_uint64 * 256)()
    b = C.c_void_p(C.addressof(buf))
    n = lib.msgs_features_scratch_bytes(10, 5)
    fwd = lambda v=C.byref(view), P=10, D=5, g=b, f=b, Cn=5, o=b, gb=1 << 30: lib.msgs_features_forward(
        v, P, g, gb, D, b, 1 << 30, b, 1 << 30, f, Cn, o, None)
    assert fwd(v=None) == -1 and fwd(P=-1) == -1 and fwd(D=-1) == -1 and fwd(Cn=0) == -1 and fwd(o=None) == -1
    assert fwd(g=None) == -1 and fwd(f=None) == -1 and fwd(f=C.c_void_p(C.addressof(buf) + 2)) == -1
    assert fwd(gb=16) == -2
    bwd = lambda v=C.byref(view), P=10, D=5, f=b, Cn=5, G=b, rec=None, rb=0, s=b, sb=n, o=b: lib.msgs_features_backward(
        v, P, b, 1 << 30, D, b, 1 << 30, b, 1 << 30, f, Cn, G, rec, rb, s, sb, o, None)
    assert bwd(v=None) == -1 and bwd(P=-1) == -1 and bwd(D=-1) == -1 and bwd(Cn=0) == -1 and bwd(o=None) == -1
    assert bwd(f=None) == -1 and bwd(G=None) == -1 and bwd(s=None) == -1
    assert bwd(s=C.c_void_p(C.addressof(buf) + 4)) == -1                  # rows of doubles: 8-byte aligned
    assert bwd(rec=C.c_void_p(C.addressof(buf) + 4), rb=1 << 30) == -1
    assert bwd(sb=n - 1) == -2 and bwd(rec=b, rb=8) == -2
    assert bwd(P=0, o=None, s=None) == 0                                  # dL_dfeatures is [0, C]: nothing to write
    prev = lib.msgs_set_deterministic(1)
    try:
        assert fwd() == -1 and bwd() == -1                                # not offered in the verification mode
    finally:
        lib.msgs_set_deterministic(prev)
    assert all(x == 0 for x in buf)


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
    assert r.features is None
    f = torch.zeros(3, 5)
    r2 = r.with_features(f)
    assert r2 is not r and r2.features is f and r.features is None
    assert r2.return_alpha is True and r2.absgrad is True and r2.raster_settings is r.raster_settings
    assert list(inspect.signature(dgr.GaussianRasterizer.with_features).parameters) == ["self", "features"]
    for fn in (dgr.rasterize_gaussians, dgr.rasterize_gaussians_raw, dgr.GaussianRasterizer.forward_raw):
        p = inspect.signature(fn).parameters
        assert p["features"].default is None, fn.__name__
    # the reference's call surface and the pinned opt-in signatures are what they were
    assert list(inspect.signature(dgr.GaussianRasterizer.forward).parameters) == [
        "self", "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp",
        "max_pixel_sizes", "min_pixel_sizes", "occ_multiplier", "dc_delta", "base_mask"]
    assert list(inspect.signature(dgr.GaussianRasterizer.__init__).parameters) == ["self", "raster_settings", "return_alpha",
                                                                                  "absgrad"]
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(gr.render_with_features) == [
        ("viewpoint_camera", E), ("pc", E), ("pipe", E), ("bg_color", E), ("features", E), ("scaling_modifier", 1.0),
        ("override_color", None), ("filter_small", False), ("filter_large", False), ("fade_size", 1.0), ("fused", False)]
    assert list(inspect.signature(gr.render).parameters) == [
        "viewpoint_camera", "pc", "pipe", "bg_color", "scaling_modifier", "override_color", "filter_small", "filter_large",
        "fade_size"]
    assert gr.RESULT_KEYS == ("render", "acc_pixel_size", "depth", "viewspace_points", "visibility_filter", "radii",
                              "pixel_sizes")


def test_guards_need_no_device():
    import diff_gaussian_rasterization as dgr
    z = lambda *s: torch.zeros(*s)
    args = dict(means3D=z(4, 3), means2D=z(4, 3), opacities=z(4, 1), shs=z(4, 16, 3), scales=z(4, 3), rotations=z(4, 4))
    r = dgr.GaussianRasterizer(_settings())
    for bad in (z(5, 3), z(3, 3), z(4, 3, 1), z(12)):
        with pytest.raises((ValueError, RuntimeError), match="features"):
            r.with_features(bad)(**args)
    with pytest.raises(RuntimeError, match="HIP device"):                    # a CPU tensor: there is no CPU path
        r.with_features(z(4, 3))(**args)
    prev = dgr.set_deterministic(True)
    try:
        with pytest.raises(ValueError, match="verification mode"):
            r.with_features(z(4, 3))(**args)
    finally:
        dgr.set_deterministic(prev)


def test_fixture_is_what_the_oracle_computes():
    gen = _generator()
    want = gen.compute()
    got = np.load(GOLDEN)
    assert sorted(got.files) == sorted(want)
    for k in ("borderline", "visible", "features", "G"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    for k in ("map", "dfeatures", "means3D", "opacities", "scales", "rotations", "means2D"):
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape
        assert np.abs(got[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k


def _generator():
    spec = importlib.util.spec_from_file_location("make_features_golden", os.path.join(ROOT, "tests", "golden",
                                                                                       "make_features_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fixture_properties():
    gen = _generator()
    t = np.load(GOLDEN)
    P, Cn, H, W = gen.P, gen.C, gen.H, gen.W
    vis, bl = t["visible"], t["borderline"]
    assert bl.shape == (H, W) and bl.sum() <= gen.MAX_BORDERLINE * W * H
    assert vis.sum() >= 150
    f, G = t["features"], t["G"]
    assert f.shape == (P, Cn) and f.dtype == np.float32 and f.min() >= 0 and f.max() < 1 and Cn % 3 != 0
    assert G.shape == (Cn, H, W) and G.dtype == np.float32 and not G[:, bl].any() and np.abs(G[:, ~bl]).min() > 0
    assert t["map"].shape == (Cn, H, W) and t["dfeatures"].shape == (P, Cn)
    # a convex-like combination of features in [0, 1) with weights that add up to alpha <= 1
    assert t["map"].min() >= 0 and t["map"].max() < 1 and t["map"].max() > 0.5
    assert not t["dfeatures"][~vis].any() and (np.abs(t["dfeatures"][vis]).max(1) > 0).sum() >= 0.9 * vis.sum()
    for k, shape in (("means3D", (P, 3)), ("opacities", (P, 1)), ("scales", (P, 3)), ("rotations", (P, 4)), ("means2D", (P, 3))):
        assert t[k].shape == shape and np.isfinite(t[k]).all() and np.abs(t[k]).max() > 0, k
        assert not t[k][~vis].any(), k
    assert not t["means2D"][:, 2].any()
    # the channels are different quantities: a replay that blended one channel into all could not pass
    assert np.abs(t["map"][0] - t["map"][1]).max() > 0.05 and np.abs(t["dfeatures"][:, 0] - t["dfeatures"][:, 1]).max() > 0.05

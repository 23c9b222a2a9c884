"""Median depth and Gaussian id without a GPU (SPEC M15; 4.15):
  * the committed fixture tests/golden/median_depth_truth.npz is what its generator computes, and has the properties the GPU
    tests rely on (every pixel of F crosses 1/2; thin has empty, crossing and never-crossing pixels; the mask is small);
  * the definition on hand-made lists: strict T_i > 0.5, the last blended entry of a ray that never crosses, -1 for none;
  * the C ABI: the header declares the two entries, the built library exports them, the version is still 11;
  * the Python surface, the refusal in the verification mode, and the order of the trailing-input markers for every combination
    of alpha / absgrad / distortion / median / features / bg / camera, on CPU stand-ins."""
import importlib.util
import inspect
import itertools
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "median_depth_truth.npz")


def _generator():
    spec = importlib.util.spec_from_file_location("make_median_depth_golden", os.path.join(ROOT, "tests", "golden",
                                                                                           "make_median_depth_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def gen():
    return _generator()


def test_fixture_is_what_the_generator_computes(gen):
    want = gen.compute()
    got = np.load(GOLDEN)
    assert sorted(got.files) == sorted(want)
    for s in gen.SCENES:
        for k in ("id", "mask", "borderline", "near", "visible", "G", "count", "crossed", "pos"):
            k = f"{s}_{k}"
            assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
        for k in ("depth", "means3D", "viewmatrix"):
            k = f"{s}_{k}"
            assert got[k].dtype == np.float64 and got[k].shape == want[k].shape
            assert np.abs(got[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k


def test_fixture_properties(gen):
    t = np.load(GOLDEN)
    H, W = gen.H, gen.W
    census = {}
    for s in gen.SCENES:
        g = lambda k: t[f"{s}_{k}"]
        P = gen.scene(s)[0].means3D.shape[0]
        mask, ids, depth, count = g("mask"), g("id"), g("depth"), g("count")
        assert mask.shape == (H, W) and np.array_equal(mask, g("borderline") | g("near"))
        assert mask.sum() <= gen.MAX_MASKED * W * H                                    # the condition of the masking
        G = g("G")
        assert G.shape == (H, W) and G.dtype == np.float32 and not G[mask].any() and np.abs(G[~mask]).min() > 0
        empty = count == 0
        assert ids.dtype == np.int32 and np.array_equal(ids == -1, empty) and ids.max() < P
        assert not depth[empty].any() and (depth[~empty] > 0.2).all()
        assert g("visible")[ids[~empty]].all()
        assert not g("crossed")[empty].any()
        census[s] = (int(empty.sum()), int(g("crossed").sum()), int((~empty & ~g("crossed")).sum()),
                     int(g("borderline").sum()), int((g("near") & ~g("borderline")).sum()))
        # the gradient: sum of G over the pixels of each Gaussian along the view axis (the front camera looks down +z), nothing
        # for a Gaussian that is nobody's median
        m3 = g("means3D")
        assert m3.shape == (P, 3) and np.isfinite(m3).all()
        want = np.zeros(P)
        np.add.at(want, ids[~empty], G[~empty].astype(np.float64))
        assert np.abs(m3 @ gen.scene(s)[1].world_view_transform[:3, 2].double().numpy() - want).max() <= 1e-12 * np.abs(want).max()
        assert not m3[want == 0].any()
        assert g("viewmatrix").shape == (4, 4) and np.abs(g("viewmatrix")).max() > 0
    # (empty, crossing, never crossing, borderline, near and not borderline) as measured by the float64 restatement
    assert census == {"F": (0, 960, 0, 1, 3), "thin": (323, 8, 629, 2, 0)}, census


def test_definition_on_hand_made_lists(gen):
    """three entries, four pixels: alpha 0.5 exactly leaves T = 0.5 — not > 0.5, so the walk stops AT that entry; a transparent
    ray ends on its last blended entry; an unblended entry in between is never selected; no blended entry: -1"""
    a = torch.tensor([[0.5, 0.1, 0.6, 0.0],
                      [0.9, 0.0, 0.9, 0.0],
                      [0.9, 0.2, 0.9, 0.0]], dtype=torch.float64)
    blended = a > 0
    T = torch.cat([torch.ones(1, 4, dtype=torch.float64), torch.cumprod(1 - a, 0)[:-1]], 0)
    m, crossed, near = gen.median_of(a * T, blended)
    assert m.tolist() == [0, 2, 0, -1]
    assert crossed.tolist() == [True, False, True, False]
    assert near.tolist() == [True, False, False, False]
    # T_1 = 1 > 0.5 always: a pixel with a blended entry has a median, and a first entry that crosses is its own median
    b = torch.tensor([[0.3], [0.3], [0.3]], dtype=torch.float64)              # T: 1, 0.7, 0.49 -> entry 1 takes T to 0.49
    Tb = torch.tensor([[1.0], [0.7], [0.49]], dtype=torch.float64)
    assert gen.median_of(b * Tb, b > 0)[0].tolist() == [1]


# ---------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------------
def test_c_abi_has_the_two_entries_and_keeps_its_version():
    import diff_gaussian_rasterization as dgr
    lib = dgr._C.lib
    assert lib.msgs_abi_version() == 11
    for name in ("msgs_median_depth_forward", "msgs_median_depth_backward"):
        assert name in dgr._C.EXPORTS and hasattr(lib, name)
    assert len(lib.msgs_median_depth_forward.argtypes) == 12 and len(lib.msgs_median_depth_backward.argtypes) == 7
    header = open(os.path.join(ROOT, "include", "msgs.h")).read()
    assert "int msgs_median_depth_forward(" in header and "int msgs_median_depth_backward(" in header
    assert "float* out_median_depth, int32_t* out_median_id, void* stream);" in header
    assert "#define MSGS_ABI_VERSION 11" in header
    assert "//" not in header.split("msgs_median_depth_forward:")[1].split("int msgs_median_depth_backward(")[0]     # C99 comments


# ---------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------------------------------
def _settings(**kw):
    import diff_gaussian_rasterization as dgr
    rs = dgr.GaussianRasterizationSettings(4, 6, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                           False, False)
    return rs._replace(**kw) if kw else rs


def test_wrapper_surface():
    import diff_gaussian_rasterization as dgr
    import gaussian_renderer as gr
    r = dgr.GaussianRasterizer(_settings(), return_alpha=True, absgrad=True)
    assert r.return_median_depth is False
    r2 = r.with_median_depth()
    assert r2 is not r and r2.return_median_depth is True and r.return_median_depth is False
    assert r2.return_alpha is True and r2.absgrad is True and r2.raster_settings is r.raster_settings
    assert list(inspect.signature(dgr.GaussianRasterizer.with_median_depth).parameters) == ["self", "on"]
    assert inspect.signature(dgr.GaussianRasterizer.with_median_depth).parameters["on"].default is True
    f = torch.zeros(3, 5)
    # the flag survives every other with_*(), and they survive it
    assert r2.with_features(f).return_median_depth and r2.with_distortion().return_median_depth
    assert r2.with_antialiasing().return_median_depth
    r3 = r.with_features(f).with_distortion().with_antialiasing().with_median_depth()
    assert r3.features is f and r3.return_distortion and r3.antialiasing and r3.return_median_depth
    assert r2.with_median_depth(False).return_median_depth is False
    for fn in (dgr.rasterize_gaussians, dgr.rasterize_gaussians_raw):
        p = inspect.signature(fn).parameters
        assert p["return_median_depth"].default is False, fn.__name__
    assert inspect.signature(dgr.GaussianRasterizer.forward_raw).parameters["return_median_depth"].default is None
    assert "absgrad" in dgr.GaussianRasterizer.with_median_depth.__doc__
    assert dgr._median_probe is None
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    assert sig(gr.render_with_median_depth) == [
        ("viewpoint_camera", E), ("pc", E), ("pipe", E), ("bg_color", E), ("scaling_modifier", 1.0), ("override_color", None),
        ("filter_small", False), ("filter_large", False), ("fade_size", 1.0), ("alpha", False), ("fused", False)]
    assert gr.RESULT_KEYS == ("render", "acc_pixel_size", "depth", "viewspace_points", "visibility_filter", "radii",
                              "pixel_sizes")
    src = inspect.getsource(gr.render_with_median_depth)
    assert 'out["median_depth"]' in src and 'out["median_id"]' in src and 'out["alpha"]' in src
    # not offered in the view pipeline or the view-parallel exchange
    import multi_view
    import view_parallel
    assert "median" not in inspect.getsource(multi_view) and "median" not in inspect.getsource(view_parallel)


def test_verification_mode_is_refused_before_any_device_call(monkeypatch):
    import diff_gaussian_rasterization as dgr
    z = lambda *s: torch.zeros(*s)
    args = dict(means3D=z(4, 3), means2D=z(4, 3), opacities=z(4, 1), shs=z(4, 16, 3), scales=z(4, 3), rotations=z(4, 4))
    calls = []
    monkeypatch.setattr(dgr, "_median_probe", calls.append)
    r = dgr.GaussianRasterizer(_settings()).with_median_depth()
    prev = dgr.set_deterministic(True)
    try:
        with pytest.raises(ValueError, match="verification mode"):
            r(**args)                                                   # CPU tensors: any device call would raise something else
        with pytest.raises(ValueError, match="verification mode"):
            r.forward_raw(z(4, 3), z(4, 3), z(4, 1, 3), z(4, 15, 3), z(4, 1), z(4, 3), z(4, 4))
        with pytest.raises(ValueError, match="return_median_depth"):
            dgr._extra_inputs(_settings(), return_median_depth=True)
        assert dgr._extra_inputs(_settings()) == ()                     # the call without the flag is not refused
    finally:
        dgr.set_deterministic(prev)
    assert calls == []


# ---------------------------------------------------------------------------------------------------------------------------
# the trailing inputs: [camera x3] [bg] [_ALPHA] [absgrad marker] [_DISTORTION] [_MEDIAN] [_FEATURES, features]
# ---------------------------------------------------------------------------------------------------------------------------
FLAGS = ("camera", "bg", "alpha", "absgrad", "distortion", "median", "features")


@pytest.mark.parametrize("combo", list(itertools.product((False, True), repeat=len(FLAGS))),
                         ids=lambda c: "".join(n[0] if on else "-" for n, on in zip(("c", "b", "a", "g", "d", "m", "f"), c)))
def test_marker_order_is_parsed_for_every_combination(combo):
    import diff_gaussian_rasterization as dgr
    on = dict(zip(FLAGS, combo))
    P = 3
    kw = {}
    if on["camera"]:
        kw.update(viewmatrix=torch.eye(4).requires_grad_(True), projmatrix=torch.eye(4).requires_grad_(True),
                  campos=torch.zeros(3).requires_grad_(True))
    if on["bg"]:
        kw.update(bg=torch.zeros(3).requires_grad_(True))
    rs = _settings(**kw)
    m2, model = torch.zeros(P, 3), types.SimpleNamespace(shape=(P, 3), device=torch.device("cpu"))
    feats = torch.zeros(P, 5, requires_grad=True) if on["features"] else None
    if feats is not None:                                               # (the device guard of _check_features is not the subject)
        feats_ok = dgr._check_features
        dgr._check_features = lambda f, P, dev: f
    try:
        extra = dgr._extra_inputs(rs, on["alpha"], on["absgrad"], m2, feats, model, on["distortion"], on["median"])
    finally:
        if feats is not None:
            dgr._check_features = feats_ok
    # what _extra_inputs built, in order
    want = []
    if on["camera"]:
        want += [rs.viewmatrix, rs.projmatrix, rs.campos]
    if on["bg"]:
        want += [rs.bg]
    if on["alpha"]:
        want += [dgr._ALPHA]
    if on["absgrad"]:
        want += ["absgrad"]
    if on["distortion"]:
        want += [dgr._DISTORTION]
    if on["median"]:
        want += [dgr._MEDIAN]
    if on["features"]:
        want += [dgr._FEATURES, feats]
    assert len(extra) == len(want)
    for got, w in zip(extra, want):
        assert (isinstance(got, dgr._AbsgradMarker) and got.means2D() is m2) if isinstance(w, str) else got is w
    # what _note_extra reads back: a stand-in ctx with the needs_input_grad autograd would report (13 leading inputs)
    ctx = types.SimpleNamespace(needs_input_grad=(False,) * 13 + tuple(torch.is_tensor(t) and t.requires_grad for t in extra))
    camera, alpha = dgr._note_extra(ctx, extra)
    assert alpha is on["alpha"] and ctx.return_alpha is on["alpha"]
    assert len(camera) == (3 if on["camera"] else 0) and all(a is b for a, b in zip(camera, want[:3]))
    assert ctx.camera == (tuple(((4, 4), torch.float32, torch.device("cpu")) if k < 2 else ((3,), torch.float32, torch.device("cpu"))
                                for k in range(3)) if on["camera"] else ())
    assert ctx.has_bg is on["bg"] and (ctx.bg is not None) is on["bg"]
    assert (ctx.absgrad is not None) is on["absgrad"]
    assert ctx.distortion is on["distortion"] and ctx.median is on["median"]
    assert (ctx.features is feats) and (ctx.features is not None) is on["features"]
    assert ctx.n_extra_tail == len(extra) - len(camera)
    # the gradients of the trailing inputs line up with them, and the output gradients are split by the same flags
    g_cam = tuple("cam%d" % k for k in range(len(camera)))
    ctx.g_features = torch.zeros(P, 5) if on["features"] else None
    grads = dgr._extra_grads(ctx, g_cam, "bg" if on["bg"] else None)
    assert len(grads) == len(extra)
    assert grads[:len(camera)] == g_cam and (not on["bg"] or grads[len(camera)] == "bg")
    assert all(g is None for g in grads[len(camera) + int(on["bg"]):len(grads) - (1 if on["features"] else 0)])
    assert not on["features"] or torch.is_tensor(grads[-1])
    tail = []
    for name, n in (("alpha", 1), ("distortion", 1), ("median", 2), ("features", 1)):
        if on[name]:
            tail += [name] + (["median_id"] if n == 2 else [])
    ga, gd, gm, gf = dgr._split_grad_tail(ctx, tuple(tail))
    assert (ga, gd, gm, gf) == tuple(n if on[n] else None for n in ("alpha", "distortion", "median", "features"))

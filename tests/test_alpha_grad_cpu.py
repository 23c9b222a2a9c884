"""CPU checks of the alpha map and the background gradient (include/msgs.h msgs_alpha_map,
msgs_backward_with_alpha, msgs_bg_grad):
- the three C entries and the scratch query are declared, exported and listed, ABI unchanged;
- the scratch query is positive and monotone in the pixel count;
- the opt-in surface exists (GaussianRasterizer(..., return_alpha=True), render_with_alpha) and the default surface
  (the 15 settings fields, render, render_fused, RESULT_KEYS) is what it was."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("msgs_alpha_map", "msgs_backward_with_alpha", "msgs_bg_grad_scratch_bytes", "msgs_bg_grad")


def test_header_declares_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msgs.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n
    # msgs_backward_with_alpha: msgs_backward_with_camera's arguments with dL_dalpha behind dL_ddepth
    cam = re.search(r"int\s+msgs_backward_with_camera\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    alp = re.search(r"int\s+msgs_backward_with_alpha\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(alp) == norm(cam).replace("const float* dL_ddepth,", "const float* dL_ddepth, const float* dL_dalpha,")


def test_library_exports_and_lists_them():
    import diff_gaussian_rasterization as dgr
    for n in NEW:
        assert hasattr(dgr._C.lib, n), n
        assert n in dgr._C.EXPORTS, n
    assert dgr._C.lib.msgs_abi_version() == 11


def test_bg_grad_scratch_query_is_positive_and_monotone():
    import diff_gaussian_rasterization as dgr
    q = dgr._C.lib.msgs_bg_grad_scratch_bytes
    shapes = [(1, 1), (3, 1), (16, 16), (149, 91), (150, 90), (160, 96), (640, 360), (1920, 1080), (3840, 2160), (8192, 8192)]
    shapes.sort(key=lambda s: s[0] * s[1])
    sizes = [q(w, h) for w, h in shapes]
    assert all(s > 0 for s in sizes), sizes
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
    assert all(s % 24 == 0 for s in sizes), sizes                 # rows of three doubles
    assert q(1920, 1080) == q(1080, 1920)                         # a function of the pixel count
    assert q(0, 16) == 0 and q(16, -1) == 0


def test_rasterizer_accepts_return_alpha():
    import torch

    import diff_gaussian_rasterization as dgr
    assert len(dgr.GaussianRasterizationSettings._fields) == 15
    rs = dgr.GaussianRasterizationSettings(4, 4, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                           False, False)
    assert dgr.GaussianRasterizer(rs).return_alpha is False
    assert dgr.GaussianRasterizer(raster_settings=rs).return_alpha is False
    assert dgr.GaussianRasterizer(rs, return_alpha=True).return_alpha is True
    for fn in (dgr.rasterize_gaussians, dgr.rasterize_gaussians_raw):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "return_alpha" and p["return_alpha"].default is False, fn.__name__


def test_render_with_alpha_signature_and_unchanged_render():
    import gaussian_renderer as gr
    sig = lambda f: [(n, p.default) for n, p in inspect.signature(f).parameters.items()]
    E = inspect.Parameter.empty
    base = [("viewpoint_camera", E), ("pc", E), ("pipe", E), ("bg_color", E), ("scaling_modifier", 1.0)]
    tail = [("filter_small", False), ("filter_large", False), ("fade_size", 1.0)]
    assert sig(gr.render_with_alpha) == base + [("override_color", None)] + tail + [("fused", False)]
    assert sig(gr.render) == base + [("override_color", None)] + tail
    assert sig(gr.render_fused) == base + tail
    assert gr.RESULT_KEYS == ("render", "acc_pixel_size", "depth", "viewspace_points", "visibility_filter", "radii",
                              "pixel_sizes")

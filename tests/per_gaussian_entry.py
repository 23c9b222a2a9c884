"""The call pattern of msgs_backward_per_gaussian (the K8 + K9 isolation entry), shared by tests/test_k8_isolation_gpu.py,
tests/test_sh_jacobian_gpu.py and tests/test_per_gaussian_backward_gpu.py.  Not collected by pytest."""
import ctypes as C
import math

import torch


def plain_call(seen, cam, st, bg, dev="cuda", cov=None, scale_modifier=1.0, colors=None):
    """reference-API (raw_params = 0) marshalling of the activated tensors the oracle is fed.  cov: cov3D_precomp [P,6] instead
    of scales / rotations; colors: colors_precomp [P,3] instead of the SH rows"""
    import diff_gaussian_rasterization as dgr
    rs = dgr.GaussianRasterizationSettings(
        image_height=cam.image_height, image_width=cam.image_width, tanfovx=math.tan(cam.FoVx * 0.5),
        tanfovy=math.tan(cam.FoVy * 0.5), bg=bg.to(dev), scale_modifier=scale_modifier,
        viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev),
        sh_degree=seen.sh_degree, campos=cam.camera_center.to(dev), prefiltered=False, debug=False, **st)
    t = lambda x: x.to(dev).contiguous()
    return dgr._Call(rs, t(seen.means3D), None if colors is not None else t(seen.shs), t(colors) if colors is not None else None,
                     t(seen.opacities), None if cov is not None else t(seen.scales),
                     None if cov is not None else t(seen.rotations), t(cov) if cov is not None else None,
                     t(seen.max_pixel_sizes), t(seen.min_pixel_sizes), None, None, t(seen.base_mask))


def per_gaussian_hip(call, radii, geom, sums2d, with_cov=False, fill=None):
    """msgs_backward_per_gaussian on the [P,9] float64 sums -> {tensor name: gradient}.  fill: what every output buffer holds
    before the call (NaN: an element the kernel did not write stays visible); default: uninitialised"""
    import diff_gaussian_rasterization as dgr
    P, K, dev = call.P, call.K, call.device
    e = (lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)) if fill is None else \
        (lambda *s: torch.full(s, fill, dtype=torch.float32, device=dev))
    out = dict(means3D=e(P, 3), means2D=e(P, 3), opacities=e(P))
    if call.colors is not None:
        out["colors"] = e(P, 3)
    else:
        out["shs"] = e(P, K, 3)
    if with_cov:
        out["cov3D_precomp"] = e(P, 6)
    else:
        out["scales"], out["rotations"] = e(P, 3), e(P, 4)
    p = lambda k: C.c_void_p(out[k].data_ptr()) if k in out else None
    grads = dgr._C.Grads(p("means3D"), p("means2D"), p("shs"), p("colors"), p("opacities"), p("scales"), p("rotations"),
                         p("cov3D_precomp"), None, None, None, 0)
    s = sums2d.to(dev).contiguous()
    dgr._C.check(dgr._C.lib.msgs_backward_per_gaussian(
        C.byref(call.view), C.byref(call.g), C.c_void_p(radii.data_ptr()), C.c_void_p(geom.data_ptr()), geom.numel(),
        C.c_void_p(s.data_ptr()), C.byref(grads), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
        "msgs_backward_per_gaussian")
    torch.cuda.synchronize()
    return out

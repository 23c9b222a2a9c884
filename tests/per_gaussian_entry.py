"""The call pattern of msgs_backward_per_gaussian (the K8 + K9 isolation entry), shared by tests/test_k8_isolation_gpu.py,
tests/test_sh_jacobian_gpu.py and tests/test_per_gaussian_backward_gpu.py, and the ways to K1's records (the GaussRec section
of a view's geom buffer) through every entry that runs it, for tests/test_per_gaussian_forward_gpu.py.  Not collected by pytest."""
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


def family_call(fam, inp, dev="cuda"):
    """plain_call for the rows `inp` of a per_gaussian_truth family (its camera, settings, modifier, precomputed inputs)"""
    import types
    seen = types.SimpleNamespace(sh_degree=int(fam["view"]["sh_degree"]), shs=inp.get("shs"), scales=inp.get("scales"),
                                 rotations=inp.get("rotations"), **{k: inp[k] for k in (
                                     "means3D", "opacities", "max_pixel_sizes", "min_pixel_sizes", "base_mask")})
    return plain_call(seen, fam["cam"], fam["settings"], torch.zeros(3), dev=dev, cov=inp.get("cov3D_precomp"),
                      scale_modifier=fam["mod"], colors=inp.get("colors_precomp"))


def records_of(geom, P):
    """[P,12] float32 numpy: the GaussRec section of a view's geom buffer, every row as it lies there"""
    return geom[:48 * P].view(torch.float32).view(P, 12).cpu().numpy().copy()


def k1_only(call):
    """msgs_preprocess_only (K1 alone) into buffers of its own, every byte of them NaN / INT_MIN before the launch ->
    (rec12 [P,12], radii [P], pixel_sizes [P]) numpy.  What the kernel did not write stays visible."""
    import diff_gaussian_rasterization as dgr
    P, dev = call.P, call.device
    lib = dgr._C.lib
    n = int(lib.msgs_geom_bytes(P))
    geom = torch.full(((n + 3) // 4,), float("nan"), dtype=torch.float32, device=dev).view(torch.uint8)[:n]
    radii = torch.full((P,), -2 ** 31, dtype=torch.int32, device=dev)
    psz = torch.full((P,), float("nan"), dtype=torch.float32, device=dev)
    dgr._C.check(lib.msgs_preprocess_only(C.byref(call.view), C.byref(call.g), C.c_void_p(radii.data_ptr()),
                                          C.c_void_p(psz.data_ptr()), C.c_void_p(geom.data_ptr()), n,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "msgs_preprocess_only")
    torch.cuda.synchronize()
    return records_of(geom, P), radii.cpu().numpy(), psz.cpu().numpy()


def records_of_render(out, P):
    """(rec12, radii, pixel_sizes) of a render() / render_fused() / GaussianRasterizer result whose image carries the op's
    autograd node: the node is the forward's ctx, ctx.state[0] its geom buffer"""
    image = out["render"] if isinstance(out, dict) else out[0]
    radii, psz = (out["radii"], out["pixel_sizes"]) if isinstance(out, dict) else (out[3], out[4])
    geom = image.grad_fn.state[0]
    torch.cuda.synchronize()
    return records_of(geom, P), radii.cpu().numpy(), psz.detach().cpu().numpy()


class LeafModel:
    """the attributes render() / render_fused() read of a GaussianModel, on given float32 raw leaves (the reference's stored
    layout: features_dc [P,1,3], features_rest [P,15,3], opacity [P,1])"""

    def __init__(self, leaves, inp, sh_degree, dev="cuda"):
        import torch.nn as nn
        mk = lambda t: nn.Parameter(t.detach().to(dev, torch.float32).contiguous().clone())
        self.max_sh_degree, self.active_sh_degree = 3, int(sh_degree)
        self._xyz, self._features_dc, self._features_rest = mk(leaves["xyz"]), mk(leaves["features_dc"]), mk(leaves["features_rest"])
        self._opacity, self._scaling, self._rotation = mk(leaves["opacity"]), mk(leaves["scaling"]), mk(leaves["rotation"])
        P = self._xyz.shape[0]
        self.get_occ_multiplier = torch.ones(P, 4, 1, device=dev)
        self.get_dc_delta = torch.zeros(P, 12, 1, device=dev)
        self.get_max_pixel_sizes = inp["max_pixel_sizes"].to(dev).contiguous()
        self.get_min_pixel_sizes = inp["min_pixel_sizes"].to(dev).contiguous()
        self.get_base_mask = inp["base_mask"].to(dev).contiguous()

    get_xyz = property(lambda self: self._xyz)
    get_scaling = property(lambda self: torch.exp(self._scaling))
    get_rotation = property(lambda self: torch.nn.functional.normalize(self._rotation))
    get_opacity = property(lambda self: torch.sigmoid(self._opacity))
    get_features = property(lambda self: torch.cat((self._features_dc, self._features_rest), dim=1))

    def activated(self, inp):
        """the getters' float32 results as the device evaluates them, as an inputs dict on the CPU"""
        with torch.no_grad():
            out = dict(inp)
            out.update(means3D=self._xyz.detach().cpu(), opacities=self.get_opacity.cpu().reshape(-1), scales=self.get_scaling.cpu(),
                       rotations=self.get_rotation.cpu(), shs=self.get_features.cpu())
        return out


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

"""Mip-Splatting's 3-D smoothing filter on a model with the reference's attribute names (4.17).

    compute_3D_filter(pc, cameras)        pc.filter_3D [P,1] from the training cameras — after every densification and, as
                                          Mip-Splatting does, every 100 iterations
    render_with_3d_filter(cam, pc, ...)   render() of the filtered model: the rasterizer is fed
                                          diff_gaussian_rasterization.smoothing_filter(...) in the place of scales / opacities
    bake_3d_filter(pc)                    the fused export: the filter is written into the leaves and dropped, so that any viewer
                                          shows the filtered model

The filter bounds every Gaussian's size from below by the highest sampling rate at which any training camera sees it, so a model
trained at one scale does not grow needles and dots that erode when the camera zooms in.  It composes with the 2-D screen filter
(antialiasing=True: GaussianRasterizer.with_antialiasing() then sees s_eff and o_eff) and with the multi-scale filters.
"""
import torch
from diff_gaussian_rasterization import GaussianRasterizer, compute_3d_filter, smoothing_filter

from gaussian_renderer import RESULT_KEYS, _colour_inputs, _settings


def compute_3D_filter(pc, cameras, **kw):
    """pc.filter_3D = compute_3d_filter(pc.get_xyz, cameras, **kw)[0]; returns (filter_3D, valid_points).  kw: rule, variance."""
    filter_3D, valid = compute_3d_filter(pc.get_xyz, cameras, **kw)
    pc.filter_3D = filter_3D
    return filter_3D, valid


def _filter_of(pc, who):
    f = getattr(pc, "filter_3D", None)
    if f is None:
        raise ValueError(f"{who}: the model carries no filter_3D — run compute_3D_filter(pc, cameras) first")
    if f.shape[0] != pc.get_xyz.shape[0]:
        raise ValueError(f"{who}: filter_3D has {f.shape[0]} rows, the model {pc.get_xyz.shape[0]} — it is stale after a "
                         "densification: run compute_3D_filter(pc, cameras) again")
    return f


def _filtered_getters(pc, who, raw):
    """(scales_eff, opacities_eff) of the model under its filter_3D; raw reads the leaves pc._scaling / pc._opacity"""
    f = _filter_of(pc, who)
    if raw:
        return smoothing_filter(pc._scaling, pc._opacity, f, raw=True)
    return smoothing_filter(pc.get_scaling, pc.get_opacity, f, raw=False)


def render_with_3d_filter(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None,
                          filter_small=False, filter_large=False, fade_size=1.0, antialiasing=False, raw=True):
    """render() of the model under its 3-D smoothing filter pc.filter_3D (compute_3D_filter): the same seven keys.  By definition
    the plain render fed smoothing_filter(scales, opacities, filter_3D): every Gaussian is at least as large as the finest pixel
    any training camera sees it with, and its opacity is scaled so that it keeps its mass.  raw=True (default) hands the leaves
    pc._scaling / pc._opacity to the getter kernel, which applies exp and sigmoid itself; raw=False feeds it pc.get_scaling /
    pc.get_opacity.  antialiasing=True adds the 2-D screen filter (render_with_antialiasing) on top: full Mip-Splatting.  The
    chained mode of the reference's getters does not apply to filtered values.  Not with pipe.compute_cov3D_python (the
    covariance would be the unfiltered one): ValueError before any launch, like a stale filter_3D."""
    _filter_of(pc, "render_with_3d_filter")
    if pipe.compute_cov3D_python:
        raise ValueError("render_with_3d_filter: pipe.compute_cov3D_python builds the covariance from the unfiltered scales")
    xyz = pc.get_xyz
    viewspace = torch.zeros_like(xyz, requires_grad=True) + 0
    try:
        viewspace.retain_grad()
    except Exception:
        pass
    scales, opacities = _filtered_getters(pc, "render_with_3d_filter", raw)
    rasterizer = GaussianRasterizer(raster_settings=_settings(
        viewpoint_camera, pc, pipe, bg_color, scaling_modifier, filter_small, filter_large, fade_size))
    if antialiasing:
        rasterizer = rasterizer.with_antialiasing()
    image, acc_pixel_size, depth, radii, pixel_sizes = rasterizer(
        means3D=xyz,
        means2D=viewspace,
        opacities=opacities,
        max_pixel_sizes=pc.get_max_pixel_sizes,
        min_pixel_sizes=pc.get_min_pixel_sizes,
        occ_multiplier=pc.get_occ_multiplier,
        dc_delta=pc.get_dc_delta,
        base_mask=pc.get_base_mask,
        **_colour_inputs(viewpoint_camera, pc, pipe, override_color),
        cov3D_precomp=None, scales=scales, rotations=pc.get_rotation)
    values = (image, acc_pixel_size, depth, viewspace, radii > 0, radii, pixel_sizes)
    return dict(zip(RESULT_KEYS, values))


@torch.no_grad()
def bake_3d_filter(pc):
    """Mip-Splatting's fused export: pc._scaling <- log s_eff, pc._opacity <- logit o_eff, and the filter is dropped — render()
    and any viewer that knows nothing of the filter then show the filtered model.  (o_eff is kept inside the logit's domain, as
    the model's own opacity reset does.)  Returns pc."""
    s_eff, o_eff = _filtered_getters(pc, "bake_3d_filter", raw=True)
    tiny = torch.finfo(torch.float32).tiny
    pc._scaling.data.copy_(torch.log(s_eff.clamp_min(tiny)))
    o = o_eff.clamp(1e-12, 1.0 - 1e-7)
    pc._opacity.data.copy_(torch.log(o / (1.0 - o)).view_as(pc._opacity))
    pc.filter_3D = None
    return pc

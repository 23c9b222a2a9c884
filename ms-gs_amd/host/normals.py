"""Normal maps on a model with the reference's attribute names (4.18): both halves of the depth-normal
consistency loss of 2DGS / GOF / RaDe-GS / PGSR.

    render_with_normals(cam, pc, ...)   render() plus "alpha", "normal" (the Gaussians' normals splatted with the blend weights,
                                        2DGS's rend_normal), "surf_depth" and "surf_normal" (the normals of the depth map,
                                        2DGS's surf_normal)
    normal_consistency(out)             2DGS's term on that result: mean_p (1 - normal_p . (alpha_p surf_normal_p))

A render with normals is defined by composition: the plain render with with_features(gaussian_normals(...)),
return_alpha=True and, for depth="median", with_median_depth(); then depth_to_normal() on the surface depth.  The rasterizer's
kernels are the ones of render_with_features / render_with_median_depth.
"""
import torch
from diff_gaussian_rasterization import GaussianRasterizer, _backend, depth_to_normal, gaussian_normals

from gaussian_renderer import RESULT_KEYS, _colour_inputs, _refuse_filter_3d, _settings, _shape_inputs

DEPTHS = ("median", "expected")


def render_with_normals(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None,
                        filter_small=False, filter_large=False, fade_size=1.0, fused=False, depth="median", world=False):
    """render() — or, with fused=True, render_fused() (then without override_color) — plus the maps of a depth-normal
    consistency loss: the seven keys of RESULT_KEYS and
        "alpha"        [H,W]    render_with_alpha's
        "normal"       [3,H,W]  sum_i w_ip n_i with n = gaussian_normals(...) and w the blend weights of this render: the feature
                                map of render_with_features.  Unnormalised, no background term, magnitude about alpha (2DGS's
                                rend_normal)
        "surf_depth"   [H,W]    depth="median": render_with_median_depth's median_depth (then "median_id" is returned too);
                                depth="expected": depth / alpha.clamp_min(1e-8)
        "surf_normal"  [3,H,W]  depth_to_normal(surf_depth): unit normals of the depth map, 0 on the border and around holes
    Both normal maps are in view space, or in world space with world=True.  The plain route feeds gaussian_normals the model's
    getters (get_xyz, get_scaling, get_rotation), fused=True the leaves (_xyz, _scaling, _rotation) as they are.  A model that
    carries a filter_3D is rendered as filter3d.render_with_3d_filter renders it (not with fused=True); its normals are those of
    the unfiltered model, which the filter does not change.  Gradients, the verification mode (ValueError), deferred_forward:
    as for with_features / with_median_depth."""
    if depth not in DEPTHS:
        raise ValueError(f"render_with_normals: depth must be one of {DEPTHS}, not {depth!r}")
    if _backend.lib.msgs_get_deterministic():
        raise ValueError("render_with_normals is not offered in the verification mode (set_deterministic): features and the "
                         "median depth are not part of what that mode checks")
    median = depth == "median"
    settings = _settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, filter_small, filter_large, fade_size)
    if fused:
        _refuse_filter_3d(pc, "fused=True")
        if override_color is not None:
            raise ValueError("render_with_normals: fused=True cannot be combined with override_color")
        xyz = pc._xyz
        normals = gaussian_normals(xyz, pc._scaling, pc._rotation, settings, world=world)
    else:
        xyz = pc.get_xyz
        normals = gaussian_normals(xyz, pc.get_scaling, pc.get_rotation, settings, world=world)
    rasterizer = GaussianRasterizer(raster_settings=settings, return_alpha=True).with_features(normals)
    if median:
        rasterizer = rasterizer.with_median_depth()
    if fused:
        viewspace = torch.empty_like(xyz, requires_grad=True)
        outs = rasterizer.forward_raw(
            xyz, viewspace, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation,
            max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes,
            occ_multiplier=pc.get_occ_multiplier, dc_delta=pc.get_dc_delta, base_mask=pc.get_base_mask)
    else:
        viewspace = torch.zeros_like(xyz, requires_grad=True) + 0
        try:
            viewspace.retain_grad()
        except Exception:
            pass
        if getattr(pc, "filter_3D", None) is not None:
            from filter3d import _filtered_getters
            if pipe.compute_cov3D_python:
                raise ValueError("render_with_normals: pipe.compute_cov3D_python builds the covariance from the unfiltered scales")
            scales, opacities = _filtered_getters(pc, "render_with_normals", True)
            shape = dict(cov3D_precomp=None, scales=scales, rotations=pc.get_rotation)
        else:
            opacities, shape = pc.get_opacity, _shape_inputs(pc, pipe, scaling_modifier)
        outs = rasterizer(
            means3D=xyz,
            means2D=viewspace,
            opacities=opacities,
            max_pixel_sizes=pc.get_max_pixel_sizes,
            min_pixel_sizes=pc.get_min_pixel_sizes,
            occ_multiplier=pc.get_occ_multiplier,
            dc_delta=pc.get_dc_delta,
            base_mask=pc.get_base_mask,
            **_colour_inputs(viewpoint_camera, pc, pipe, override_color),
            **shape)
    image, acc_pixel_size, blended_depth, radii, pixel_sizes, alpha = outs[:6]
    values = (image, acc_pixel_size, blended_depth, viewspace, radii > 0, radii, pixel_sizes)
    out = dict(zip(RESULT_KEYS, values))
    out["alpha"] = alpha
    out["normal"] = outs[-1]
    if median:
        out["surf_depth"], out["median_id"] = outs[6], outs[7]
    else:
        out["surf_depth"] = blended_depth / alpha.clamp_min(1e-8)
    out["surf_normal"] = depth_to_normal(out["surf_depth"], settings, world=world)
    return out


def normal_consistency(out):
    """2DGS's normal-consistency term on a render_with_normals() result: mean over the pixels of
    1 - normal_p . (alpha_p.detach() surf_normal_p) — the splatted normals (magnitude about alpha) against the depth map's unit
    normals weighted likewise.  Plain torch."""
    surf = out["surf_normal"] * out["alpha"].detach()
    return (1.0 - (out["normal"] * surf).sum(dim=0)).mean()

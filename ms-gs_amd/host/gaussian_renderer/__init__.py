"""Host-side counterpart of the reference's `gaussian_renderer.render`
(/root/reference/gaussian_renderer/__init__.py:18-119): same signature, same argument meaning, same
seven-key result dict, so callers written against the reference (train.py:203, render.py:32,
viewer.py:71, render_traj.py:102) read the same.

The reference's own gaussian_renderer module runs unchanged on top of
ms-gs_amd/diff_gaussian_rasterization — THAT is the drop-in.  This module exists so the parity tests,
smoke() and bench.py can drive the operator through the reference's call pattern without importing
the reference, which does not travel to the GPU box.

Duck typing:
  pc    — the GaussianModel getters read at reference :57-64,71-75,82-89
  pipe  — PipelineParams (/root/reference/arguments/__init__.py:64-69)
  viewpoint_camera — Camera / MiniCam attributes (/root/reference/scene/cameras.py:17-76)
"""
import math
import types

import torch
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer

from .sh import eval_sh

# PipelineParams defaults of the reference (/root/reference/arguments/__init__.py:64-69)
PIPE = types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)

RESULT_KEYS = ("render", "acc_pixel_size", "depth", "viewspace_points", "visibility_filter", "radii",
               "pixel_sizes")


def _settings(cam, pc, pipe, bg_color, scaling_modifier, filter_small, filter_large, fade_size):
    """The 15 raster settings (reference :37-53)."""
    return GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width),
        tanfovx=math.tan(0.5 * cam.FoVx), tanfovy=math.tan(0.5 * cam.FoVy),
        bg=bg_color, scale_modifier=scaling_modifier,
        viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform,
        sh_degree=pc.active_sh_degree, campos=cam.camera_center,
        prefiltered=False, debug=pipe.debug,
        filter_small=filter_small, filter_large=filter_large, fade_size=fade_size)


def _shape_inputs(pc, pipe, scaling_modifier):
    """Either the Python-side covariance or (scales, rotations) for the op (reference :66-75)."""
    if pipe.compute_cov3D_python:
        return dict(cov3D_precomp=pc.get_covariance(scaling_modifier), scales=None, rotations=None)
    return dict(cov3D_precomp=None, scales=pc.get_scaling, rotations=pc.get_rotation)


def _colour_inputs(cam, pc, pipe, override_color):
    """Override colour, Python-side SH->RGB, or raw SH coefficients for the op (reference :77-91)."""
    if override_color is not None:
        return dict(shs=None, colors_precomp=override_color)
    if not pipe.convert_SHs_python:
        return dict(shs=pc.get_features, colors_precomp=None)
    n_coeff = (pc.max_sh_degree + 1) ** 2
    per_channel = pc.get_features.transpose(1, 2).view(-1, 3, n_coeff)
    view_dir = pc.get_xyz - cam.camera_center.repeat(pc.get_features.shape[0], 1)
    view_dir = view_dir / view_dir.norm(dim=1, keepdim=True)
    rgb = eval_sh(pc.active_sh_degree, per_channel, view_dir)
    return dict(shs=None, colors_precomp=torch.clamp_min(rgb + 0.5, 0.0))


def _refuse_filter_3d(pc, who):
    """The raw-parameter routes read the model's leaves themselves: on a model that carries a 3-D smoothing filter
    (filter3d.compute_3D_filter) they would render the UNFILTERED model without saying so."""
    if getattr(pc, "filter_3D", None) is not None:
        raise ValueError(f"{who}: the model carries a filter_3D, which this route would ignore; render through "
                         "filter3d.render_with_3d_filter(), or filter3d.bake_3d_filter(pc) first")


def render(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None,
           filter_small=False, filter_large=False, fade_size=1.0):
    """Render `pc` from `viewpoint_camera`.  `bg_color` must already live on the GPU."""
    xyz = pc.get_xyz
    # gradient sink for the screen-space means (reference :27-31): a non-leaf zero tensor whose
    # .grad is retained so densification can read viewspace_points.grad[:, :2]
    # (/root/reference/scene/gaussian_model.py:698-701)
    viewspace = torch.zeros_like(xyz, requires_grad=True) + 0
    try:
        viewspace.retain_grad()
    except Exception:
        pass

    rasterizer = GaussianRasterizer(raster_settings=_settings(
        viewpoint_camera, pc, pipe, bg_color, scaling_modifier, filter_small, filter_large, fade_size))
    image, acc_pixel_size, depth, radii, pixel_sizes = rasterizer(
        means3D=xyz,
        means2D=viewspace,
        opacities=pc.get_opacity,
        max_pixel_sizes=pc.get_max_pixel_sizes,
        min_pixel_sizes=pc.get_min_pixel_sizes,
        occ_multiplier=pc.get_occ_multiplier,
        dc_delta=pc.get_dc_delta,
        base_mask=pc.get_base_mask,
        **_colour_inputs(viewpoint_camera, pc, pipe, override_color),
        **_shape_inputs(pc, pipe, scaling_modifier))
    # radii == 0 <=> frustum-culled, zero-area or filtered out: excluded from densification statistics
    # (reference :110-119)
    values = (image, acc_pixel_size, depth, viewspace, radii > 0, radii, pixel_sizes)
    return dict(zip(RESULT_KEYS, values))


def render_fused(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, filter_small=False,
                 filter_large=False, fade_size=1.0):
    """Opt-in variant of render(): hands the RAW parameters of the model (pc._xyz,
    pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation — the attribute names of the reference's
    GaussianModel, scene/gaussian_model.py:53-58) to the rasterizer, which evaluates the getters' activations
    (:127-153) and the SH concatenation (:144-149) inside its kernels.  Same result dict as render(); gradients land
    on the same leaf Parameters.  Not usable with override_color / convert_SHs_python / compute_cov3D_python."""
    _refuse_filter_3d(pc, "render_fused")
    xyz = pc._xyz
    # gradient sink for the screen-space means: the op never reads its values, so — unlike render(), which keeps the
    # reference's `zeros_like(...) + 0` — a leaf without the fill and add kernels will do (.grad is populated the same)
    viewspace = torch.empty_like(xyz, requires_grad=True)
    rasterizer = GaussianRasterizer(raster_settings=_settings(
        viewpoint_camera, pc, pipe, bg_color, scaling_modifier, filter_small, filter_large, fade_size))
    image, acc_pixel_size, depth, radii, pixel_sizes = rasterizer.forward_raw(
        xyz, viewspace, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation,
        max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes,
        occ_multiplier=pc.get_occ_multiplier, dc_delta=pc.get_dc_delta, base_mask=pc.get_base_mask)
    values = (image, acc_pixel_size, depth, viewspace, radii > 0, radii, pixel_sizes)
    return dict(zip(RESULT_KEYS, values))


def render_with_alpha(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None,
                      filter_small=False, filter_large=False, fade_size=1.0, fused=False):
    """render() — or, with fused=True, render_fused() (then without override_color) — plus the accumulated opacity of every
    pixel: the seven keys of RESULT_KEYS and "alpha" [H,W] = 1 - final transmittance, differentiable like "render" and
    "depth" (DESIGN.md 2, M9).  Mask / silhouette losses, sky and transparent backgrounds, opacity regularisers and
    compositing read it instead of a second render with colour 1 over background 0.  A `bg_color` that requires grad
    receives its gradient here as in render()."""
    settings = _settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, filter_small, filter_large, fade_size)
    rasterizer = GaussianRasterizer(raster_settings=settings, return_alpha=True)
    if fused:
        _refuse_filter_3d(pc, "fused=True")
        if override_color is not None:
            raise ValueError("render_with_alpha: fused=True cannot be combined with override_color")
        xyz = pc._xyz
        viewspace = torch.empty_like(xyz, requires_grad=True)
        image, acc_pixel_size, depth, radii, pixel_sizes, alpha = rasterizer.forward_raw(
            xyz, viewspace, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation,
            max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes,
            occ_multiplier=pc.get_occ_multiplier, dc_delta=pc.get_dc_delta, base_mask=pc.get_base_mask)
    else:
        xyz = pc.get_xyz
        viewspace = torch.zeros_like(xyz, requires_grad=True) + 0
        try:
            viewspace.retain_grad()
        except Exception:
            pass
        image, acc_pixel_size, depth, radii, pixel_sizes, alpha = rasterizer(
            means3D=xyz,
            means2D=viewspace,
            opacities=pc.get_opacity,
            max_pixel_sizes=pc.get_max_pixel_sizes,
            min_pixel_sizes=pc.get_min_pixel_sizes,
            occ_multiplier=pc.get_occ_multiplier,
            dc_delta=pc.get_dc_delta,
            base_mask=pc.get_base_mask,
            **_colour_inputs(viewpoint_camera, pc, pipe, override_color),
            **_shape_inputs(pc, pipe, scaling_modifier))
    values = (image, acc_pixel_size, depth, viewspace, radii > 0, radii, pixel_sizes)
    out = dict(zip(RESULT_KEYS, values))
    out["alpha"] = alpha
    return out


def render_with_absgrad(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None,
                        filter_small=False, filter_large=False, fade_size=1.0, fused=False, alpha=False):
    """render() — or, with fused=True, render_fused() (then without override_color) — whose backward also leaves the absolute
    screen-space gradient of AbsGS beside the signed one: after loss.backward(), out["viewspace_points"].absgrad is [P,3]
    float32 = (sum over pixels of |that pixel's share of dL/dmean2D| in x and y, 0), in the units of
    out["viewspace_points"].grad.  A Gaussian that some pixels pull left and others right — the blurry,
    over-large one — cancels itself out of .grad and not out of .absgrad: train_epilogue.update_training_stats(absgrad=True)
    accumulates its norm in the place of .grad's.  Same keys as render(), plus "alpha" (render_with_alpha) with alpha=True.
    Image, maps and gradients are those of the call without it, bit for bit."""
    settings = _settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, filter_small, filter_large, fade_size)
    rasterizer = GaussianRasterizer(raster_settings=settings, return_alpha=alpha, absgrad=True)
    if fused:
        _refuse_filter_3d(pc, "fused=True")
        if override_color is not None:
            raise ValueError("render_with_absgrad: fused=True cannot be combined with override_color")
        xyz = pc._xyz
        viewspace = torch.empty_like(xyz, requires_grad=True)
        outs = rasterizer.forward_raw(
            xyz, viewspace, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation,
            max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes,
            occ_multiplier=pc.get_occ_multiplier, dc_delta=pc.get_dc_delta, base_mask=pc.get_base_mask)
    else:
        xyz = pc.get_xyz
        viewspace = torch.zeros_like(xyz, requires_grad=True) + 0
        try:
            viewspace.retain_grad()
        except Exception:
            pass
        outs = rasterizer(
            means3D=xyz,
            means2D=viewspace,
            opacities=pc.get_opacity,
            max_pixel_sizes=pc.get_max_pixel_sizes,
            min_pixel_sizes=pc.get_min_pixel_sizes,
            occ_multiplier=pc.get_occ_multiplier,
            dc_delta=pc.get_dc_delta,
            base_mask=pc.get_base_mask,
            **_colour_inputs(viewpoint_camera, pc, pipe, override_color),
            **_shape_inputs(pc, pipe, scaling_modifier))
    image, acc_pixel_size, depth, radii, pixel_sizes = outs[:5]
    values = (image, acc_pixel_size, depth, viewspace, radii > 0, radii, pixel_sizes)
    out = dict(zip(RESULT_KEYS, values))
    if alpha:
        out["alpha"] = outs[5]
    return out


def render_with_features(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, features, scaling_modifier=1.0,
                         override_color=None, filter_small=False, filter_large=False, fade_size=1.0, fused=False):
    """render() — or, with fused=True, render_fused() (then without override_color) — plus per-Gaussian feature channels
    splatted with the same blend weights: the seven keys of RESULT_KEYS and "features" [C,H,W] float32 for `features` [P,C]
    (embeddings, segmentation logits, normals, distilled 2-D features ...), F[c,p] = sum_i f_ic alpha_ip T_ip.  The map has
    NO background term — compose one outside with the alpha map — and is differentiable: a loss on it reaches `features` and,
    as C more colour channels, the geometry and the camera, not SH / colours.  One forward and one
    backward whatever C is, where override_color needs ceil(C / 3) of each.  Image, maps and their gradients are those of
    the call without features, bit for bit."""
    settings = _settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, filter_small, filter_large, fade_size)
    rasterizer = GaussianRasterizer(raster_settings=settings).with_features(features)
    if fused:
        _refuse_filter_3d(pc, "fused=True")
        if override_color is not None:
            raise ValueError("render_with_features: fused=True cannot be combined with override_color")
        xyz = pc._xyz
        viewspace = torch.empty_like(xyz, requires_grad=True)
        outs = rasterizer.forward_raw(
            xyz, viewspace, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation,
            max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes,
            occ_multiplier=pc.get_occ_multiplier, dc_delta=pc.get_dc_delta, base_mask=pc.get_base_mask)
    else:
        xyz = pc.get_xyz
        viewspace = torch.zeros_like(xyz, requires_grad=True) + 0
        try:
            viewspace.retain_grad()
        except Exception:
            pass
        outs = rasterizer(
            means3D=xyz,
            means2D=viewspace,
            opacities=pc.get_opacity,
            max_pixel_sizes=pc.get_max_pixel_sizes,
            min_pixel_sizes=pc.get_min_pixel_sizes,
            occ_multiplier=pc.get_occ_multiplier,
            dc_delta=pc.get_dc_delta,
            base_mask=pc.get_base_mask,
            **_colour_inputs(viewpoint_camera, pc, pipe, override_color),
            **_shape_inputs(pc, pipe, scaling_modifier))
    image, acc_pixel_size, depth, radii, pixel_sizes = outs[:5]
    values = (image, acc_pixel_size, depth, viewspace, radii > 0, radii, pixel_sizes)
    out = dict(zip(RESULT_KEYS, values))
    out["features"] = outs[5] if len(outs) > 5 else None
    return out


def render_with_distortion(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None,
                           filter_small=False, filter_large=False, fade_size=1.0, fused=False, alpha=False):
    """render() — or, with fused=True, render_fused() (then without override_color) — plus the depth distortion of every ray:
    the seven keys of RESULT_KEYS, "alpha" (render_with_alpha) with alpha=True, and "distortion" [H,W] float32,
    Dist_p = 2 sum_{j<i} w_ip w_jp (z_i - z_j) with w = alpha T the blend weights of this render and z the view depth, over the
    pairs the backward counts in front-to-back order: the distortion loss of Mip-NeRF 360 / 2DGS / gsplat's distloss in its
    signed list-order form.  No background term; 0 where fewer than two Gaussians were blended.  Differentiable: its mean times
    a small weight is the usual regulariser that keeps the coarse and fine Gaussians of one surface from separating in depth;
    the gradient reaches the geometry and the camera, not SH / colours.  Image, maps and their gradients
    are those of the call without it, bit for bit."""
    settings = _settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, filter_small, filter_large, fade_size)
    rasterizer = GaussianRasterizer(raster_settings=settings, return_alpha=alpha).with_distortion()
    if fused:
        _refuse_filter_3d(pc, "fused=True")
        if override_color is not None:
            raise ValueError("render_with_distortion: fused=True cannot be combined with override_color")
        xyz = pc._xyz
        viewspace = torch.empty_like(xyz, requires_grad=True)
        outs = rasterizer.forward_raw(
            xyz, viewspace, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation,
            max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes,
            occ_multiplier=pc.get_occ_multiplier, dc_delta=pc.get_dc_delta, base_mask=pc.get_base_mask)
    else:
        xyz = pc.get_xyz
        viewspace = torch.zeros_like(xyz, requires_grad=True) + 0
        try:
            viewspace.retain_grad()
        except Exception:
            pass
        outs = rasterizer(
            means3D=xyz,
            means2D=viewspace,
            opacities=pc.get_opacity,
            max_pixel_sizes=pc.get_max_pixel_sizes,
            min_pixel_sizes=pc.get_min_pixel_sizes,
            occ_multiplier=pc.get_occ_multiplier,
            dc_delta=pc.get_dc_delta,
            base_mask=pc.get_base_mask,
            **_colour_inputs(viewpoint_camera, pc, pipe, override_color),
            **_shape_inputs(pc, pipe, scaling_modifier))
    image, acc_pixel_size, depth, radii, pixel_sizes = outs[:5]
    values = (image, acc_pixel_size, depth, viewspace, radii > 0, radii, pixel_sizes)
    out = dict(zip(RESULT_KEYS, values))
    if alpha:
        out["alpha"] = outs[5]
    out["distortion"] = outs[5 + int(bool(alpha))]
    return out


def render_with_antialiasing(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None,
                             filter_small=False, filter_large=False, fade_size=1.0):
    """render() ANTIALIASED: the opacity of every Gaussian is multiplied by rho = sqrt(max(0.000025, det0 / det1)), the
    compensation of Mip-Splatting's 2-D screen filter (upstream 3DGS's antialiasing=True, gsplat's
    rasterize_mode="antialiased"), so that the +0.3 dilation of the projected covariance no longer brightens Gaussians smaller
    than a pixel.  The same seven keys.  By definition the plain render of the same model with o rho in the place of the
    opacity (diff_gaussian_rasterization.screen_compensation): "pixel_sizes" and the multi-scale filters see the compensated
    opacity, and the gradients reach opacity, means, scales and rotations (or the covariance) through rho as well
    (DESIGN.md 2, M14).  The getters' backward runs in autograd here: the chained mode does not apply to o rho."""
    xyz = pc.get_xyz
    viewspace = torch.zeros_like(xyz, requires_grad=True) + 0
    try:
        viewspace.retain_grad()
    except Exception:
        pass
    rasterizer = GaussianRasterizer(raster_settings=_settings(
        viewpoint_camera, pc, pipe, bg_color, scaling_modifier, filter_small, filter_large, fade_size)).with_antialiasing()
    image, acc_pixel_size, depth, radii, pixel_sizes = rasterizer(
        means3D=xyz,
        means2D=viewspace,
        opacities=pc.get_opacity,
        max_pixel_sizes=pc.get_max_pixel_sizes,
        min_pixel_sizes=pc.get_min_pixel_sizes,
        occ_multiplier=pc.get_occ_multiplier,
        dc_delta=pc.get_dc_delta,
        base_mask=pc.get_base_mask,
        **_colour_inputs(viewpoint_camera, pc, pipe, override_color),
        **_shape_inputs(pc, pipe, scaling_modifier))
    values = (image, acc_pixel_size, depth, viewspace, radii > 0, radii, pixel_sizes)
    return dict(zip(RESULT_KEYS, values))


def render_with_median_depth(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None,
                             filter_small=False, filter_large=False, fade_size=1.0, alpha=False, fused=False):
    """render() — or, with fused=True, render_fused() (then without override_color) — plus the median depth of every ray and
    the Gaussian it belongs to: the seven keys of RESULT_KEYS, "alpha" (render_with_alpha) with alpha=True, and
        "median_depth" [H,W] float32: the view depth of the Gaussian at which the ray's transmittance falls through 1/2 (the
                                      last blended Gaussian with T > 0.5; the last blended one on a ray that never gets there);
                                      0 where nothing was blended
        "median_id"    [H,W] int32:   that Gaussian's row in the model, -1 where nothing was blended
    Unlike "depth" (the blended sum of z alpha T) it is the depth of one Gaussian: the input of TSDF fusion, of depth
    supervision and of depth-normal consistency (2DGS, RaDe-GS), and it stays on the occluding Gaussian when the level of a
    multi-scale model changes.  median_depth is differentiable towards the means and the camera only, with nothing through the
    selection; median_id is an index map (labels[id.clamp_min(0)] masked by id >= 0).  Image, maps and their gradients are
    those of the call without it, bit for bit."""
    settings = _settings(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, filter_small, filter_large, fade_size)
    rasterizer = GaussianRasterizer(raster_settings=settings, return_alpha=alpha).with_median_depth()
    if fused:
        _refuse_filter_3d(pc, "fused=True")
        if override_color is not None:
            raise ValueError("render_with_median_depth: fused=True cannot be combined with override_color")
        xyz = pc._xyz
        viewspace = torch.empty_like(xyz, requires_grad=True)
        outs = rasterizer.forward_raw(
            xyz, viewspace, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation,
            max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes,
            occ_multiplier=pc.get_occ_multiplier, dc_delta=pc.get_dc_delta, base_mask=pc.get_base_mask)
    else:
        xyz = pc.get_xyz
        viewspace = torch.zeros_like(xyz, requires_grad=True) + 0
        try:
            viewspace.retain_grad()
        except Exception:
            pass
        outs = rasterizer(
            means3D=xyz,
            means2D=viewspace,
            opacities=pc.get_opacity,
            max_pixel_sizes=pc.get_max_pixel_sizes,
            min_pixel_sizes=pc.get_min_pixel_sizes,
            occ_multiplier=pc.get_occ_multiplier,
            dc_delta=pc.get_dc_delta,
            base_mask=pc.get_base_mask,
            **_colour_inputs(viewpoint_camera, pc, pipe, override_color),
            **_shape_inputs(pc, pipe, scaling_modifier))
    image, acc_pixel_size, depth, radii, pixel_sizes = outs[:5]
    values = (image, acc_pixel_size, depth, viewspace, radii > 0, radii, pixel_sizes)
    out = dict(zip(RESULT_KEYS, values))
    if alpha:
        out["alpha"] = outs[5]
    k = 5 + int(bool(alpha))
    out["median_depth"], out["median_id"] = outs[k], outs[k + 1]
    return out

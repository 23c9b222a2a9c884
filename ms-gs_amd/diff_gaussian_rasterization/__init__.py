"""MI355X-native drop-in for the `diff_gaussian_rasterization` package the reference imports at
/root/reference/gaussian_renderer/__init__.py:14 (the MS-GS fork of the 3DGS rasterizer, an
un-vendored CUDA submodule: /root/reference/.gitmodules:4-6).

Same public surface:
  * GaussianRasterizationSettings — NamedTuple with the 15 fields constructed at
    gaussian_renderer/__init__.py:37-53 (the 12 upstream fields + filter_small, filter_large,
    fade_size);
  * GaussianRasterizer(raster_settings=...) — nn.Module called by keyword with the 13 kwargs of
    gaussian_renderer/__init__.py:95-107, returning the 5-tuple
    (rendered_image [3,H,W], acc_pixel_size [H,W], depth [H,W], radii [P] int32, pixel_sizes [P]);
  * rasterize_gaussians(...) / GaussianRasterizer.markVisible(positions).

Host code is Python on PyTorch-ROCm; all device work is hand-written HIP for gfx950 behind the C
ABI of include/msgs.h (ms-gs_amd/csrc, loaded with ctypes by _backend.py).  PyTorch only provides
device memory (caching allocator), streams and autograd plumbing.  There is NO fallback: importing
this package without lib/libmsgs_hip.so raises ImportError, and calling it with CPU tensors raises.
"""
import contextlib
import ctypes as C
import os
import threading
import weakref
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _backend as _C

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_gaussians", "rasterize_gaussians_raw",
           "deferred_forward", "GradAccumulator", "set_grad_accumulator", "ContributionScores", "ContributionAccumulator",
           "screen_compensation", "compute_3d_filter", "smoothing_filter", "FILTER3D_CAMERA_CHUNK",
           "gaussian_normals", "depth_to_normal", "DEPTH_NORMAL_TILE_W", "DEPTH_NORMAL_TILE_H",
           "bilateral_slice", "total_variation_loss", "BILAGRID_TILE_W", "BILAGRID_TILE_H", "BILAGRID_WINDOW_CELLS",
           "tsdf_allocate", "tsdf_integrate", "tsdf_extract", "tsdf_mark_steps", "TSDF_CAMERA_CHUNK", "TSDF_MAX_BLOCKS_PER_AXIS",
           "TSDF_MAX_SLOTS", "vq_assign", "vq_update", "VQ_MAX_DIM", "VQ_MAX_CODES", "VQ_CODE_CHUNK", "VQ_UPDATE_CHUNK",
           "graph_components", "mesh_triangle_clusters", "mesh_edge_report"]


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    filter_small: bool = False
    filter_large: bool = False
    fade_size: float = 1.0


def _f32c(t):
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _opt(t):
    """None and empty tensors both mean 'not provided' (upstream passes torch.Tensor([]))."""
    if t is None or t.numel() == 0:
        return None
    return t


_NO_SWITCH = contextlib.nullcontext()


def _on_device(dev):
    """torch.cuda.device(dev) only when a switch is needed: entering and leaving that context costs ~15 us of host time,
    twice per step on the path between the forward's host synchronisation and the backward launches, where the GPU
    has only the forward's second stage queued."""
    return _NO_SWITCH if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


def _stream(dev):
    """dev's current stream as the void* every entry point takes last."""
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _launch(probe, name, dev, *args):
    """One launching entry point outside the step's hot path: the tests' probe first (probe(name) when not None), then
    lib.`name`(*args, stream) on dev's current stream under _on_device(dev), the status through _C.check(rc, name).  A site
    with several launches and torch ops between them keeps one outer `with _on_device(dev):`; the one here then switches
    nothing."""
    if probe is not None:
        probe(name)
    with _on_device(dev):
        _C.check(getattr(_C.lib, name)(*args, _stream(dev)), name)


_ptr = _C.ptr

_HIP_ONLY = "diff_gaussian_rasterization (MI355X build): tensors must live on a HIP device"


def _hip_only(dev):
    if dev.type != "cuda":
        raise RuntimeError(_HIP_ONLY)


def _require_hip(who, anchor=None, **tensors):
    """The last check in front of a launch: the device the tensors share (None entries are skipped); RuntimeError when one is
    not on a HIP device, ValueError when two are on different ones.  anchor: (noun, device) of what the tensors have to sit
    beside, such as ("the volume", its table's device); None: the first tensor given, under its keyword."""
    noun, dev = anchor if anchor is not None else (None, None)
    if dev is not None and dev.type != "cuda":
        raise RuntimeError(f"{who}: {noun} must live on a HIP device ('cuda'); there is no CPU path")
    for name, t in tensors.items():
        if t is None:
            continue
        if t.device.type != "cuda":
            raise RuntimeError(f"{who}: {name} must live on a HIP device ('cuda'); there is no CPU path")
        if dev is None:
            noun, dev = name, t.device
        elif t.device != dev:
            raise ValueError(f"{who}: {name} is on {t.device}, {noun} on {dev}")
    return dev


def _require_plain_f32(who, what, **tensors):
    """every entry is a float32 tensor that does not require grad (None entries are skipped); `what`: the noun of the
    message, the thing that is not differentiable"""
    for name, t in tensors.items():
        if t is None:
            continue
        if not torch.is_tensor(t):
            raise ValueError(f"{who}: {name} must be a tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{who}: {name} must be float32, not {t.dtype}")
        if t.requires_grad:
            raise ValueError(f"{who}: {name} requires grad — {what} is not differentiable: pass {name}.detach()")


def _bytes(n, device):
    """a byte buffer of at least n bytes.  Large requests are rounded up to one of eight sizes per octave (<= 12.5 % more): the
    trainer changes the model size by a few per cent every densification interval (train.py:253-264) and the instance count
    drifts from view to view — with exact sizes every such step asks the caching allocator for blocks it has never seen
    (hipMalloc: ~1 ms in the first iteration after every densification); with size classes the cached blocks fit again"""
    n = max(int(n), 1)
    if n >= (1 << 20):
        q = 1 << (n.bit_length() - 4)
        n = (n + q - 1) & ~(q - 1)
    return torch.empty(n, dtype=torch.uint8, device=device)


# occ_multiplier / dc_delta: this build implements their identity configuration only (ones / zeros, DESIGN SPEC M5 — every
# published MS-GS configuration; the level-selection semantics of --multi_occ / --multi_dc live in the un-vendored CUDA
# kernels).  Anything else is REFUSED instead of rendered wrongly.  A leaf tensor (the reference passes the Parameter
# itself when multi_occ is off, scene/gaussian_model.py:156-164) is checked once per (tensor object, version): one tiny
# reduction + host read on the first call after creation / densification, nothing afterwards.  A computed tensor (e.g.
# sigmoid(_occ_multiplier) under --multi_occ, :158) is checked on every call.
_identity_checked = {}


def _require_identity(t, name, value, flag):
    if t is None:
        return
    leaf = t.grad_fn is None
    if leaf:
        hit = _identity_checked.get(id(t))
        # (object, version, storage address): `param.data = other` keeps the first two
        if hit is not None and hit[0]() is t and hit[1] == t._version and hit[2] == t.data_ptr():
            return
    if not bool((t.detach() == value).all().item()):
        raise NotImplementedError(
            f"diff_gaussian_rasterization (MI355X build): {name} must be all {value:g} — the {flag} semantics of the "
            "MS-GS rasterizer (scene/gaussian_model.py:156-164,203-213) are not implemented; refusing to render "
            "with them silently ignored")
    if leaf:
        if len(_identity_checked) > 64:
            for k in [k for k, v in _identity_checked.items() if v[0]() is None]:
                del _identity_checked[k]
        _identity_checked[id(t)] = (weakref.ref(t), t._version, t.data_ptr())


def _check_rows(name, t, P, tail):
    """per-Gaussian tensor `t` must be [P, *tail] (element count per row checked; a stale tensor after densify / prune
    would otherwise be read out of bounds by preprocess_kernel)"""
    if t is None:
        return
    if tail is None:                       # width not fixed by the ABI (never read: identity-checked): rows only
        if t.dim() == 0 or int(t.shape[0]) != P:
            raise ValueError(f"{name} must have {P} rows, got {tuple(t.shape)}")
        return
    n = 1
    for d in tail:
        n *= d
    if t.dim() == 0 or int(t.shape[0]) != P or t.numel() != P * n:
        raise ValueError(f"{name} must have shape [{P}, {', '.join(str(d) for d in tail)}], got {tuple(t.shape)}")


class _Call:
    """Marshals one (settings, tensors) pair into the C structs; keeps the tensors alive."""

    def __init__(self, rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                 max_pixel_sizes, min_pixel_sizes, occ_multiplier, dc_delta, base_mask, raw_features=None,
                 rotations_raw=None):
        dev = means3D.device
        if dev.type != "cuda":
            raise RuntimeError("diff_gaussian_rasterization (MI355X build): tensors must live on a HIP device "
                               "('cuda'); there is no CPU path")
        self.device = dev
        P = int(means3D.shape[0])
        self.P = P
        _check_rows("means3D", means3D, P, (3,))
        _check_rows("scales", scales, P, (3,))
        _check_rows("rotations", rotations, P, (4,))
        _check_rows("cov3D_precomp", cov3D_precomp, P, (6,))
        _check_rows("colors_precomp", colors_precomp, P, (3,))
        _check_rows("occ_multiplier", occ_multiplier, P, None)
        _check_rows("dc_delta", dc_delta, P, None)
        _check_rows("rotations_raw", rotations_raw, P, (4,))
        if sh is not None and (sh.dim() != 3 or int(sh.shape[0]) != P or int(sh.shape[2]) != 3):
            raise ValueError(f"shs must have shape [{P}, K, 3], got {tuple(sh.shape)}")
        _require_identity(occ_multiplier, "occ_multiplier", 1.0, "--multi_occ")
        _require_identity(dc_delta, "dc_delta", 0.0, "--multi_dc")
        self.means3D = _f32c(means3D)
        self.sh = _f32c(sh) if sh is not None else None
        self.colors = _f32c(colors_precomp) if colors_precomp is not None else None
        self.opac = _f32c(opacities).reshape(-1)
        self.scales = _f32c(scales) if scales is not None else None
        self.rot = _f32c(rotations) if rotations is not None else None
        self.cov = _f32c(cov3D_precomp) if cov3D_precomp is not None else None
        self.maxps = _f32c(max_pixel_sizes).reshape(-1) if max_pixel_sizes is not None else None
        self.minps = _f32c(min_pixel_sizes).reshape(-1) if min_pixel_sizes is not None else None
        self.occ = _f32c(occ_multiplier) if occ_multiplier is not None else None
        self.dcd = _f32c(dc_delta) if dc_delta is not None else None
        if base_mask is None:
            self.base = None
        elif base_mask.dtype == torch.bool and base_mask.is_contiguous():
            self.base = base_mask.view(torch.uint8)            # same bytes, no copy kernel
        else:
            self.base = base_mask.to(torch.uint8).contiguous()
        for name, t, n in (("opacities", self.opac, P), ("max_pixel_sizes", self.maxps, P),
                           ("min_pixel_sizes", self.minps, P), ("base_mask", self.base, P)):
            if t is not None and t.numel() != n:
                raise ValueError(f"{name} must have {n} elements, got {tuple(t.shape)}")
        self.K = int(self.sh.shape[1]) if self.sh is not None else 0
        self.fdc = self.frest = None
        if raw_features is not None:        # raw GaussianModel parameters (msgs_gaussians_t::raw_params = 1)
            fdc, frest = raw_features
            self.fdc, self.frest = _f32c(fdc), _f32c(frest)
            if self.fdc.numel() != 3 * P or self.frest.numel() != 45 * P:
                raise ValueError("raw mode needs features_dc [P,1,3] and features_rest [P,15,3]")
            self.K = 16
        on = lambda t: _f32c(t if t.device == dev else t.to(dev))
        self.bg, self.vm, self.pm, self.cp = on(rs.bg), on(rs.viewmatrix), on(rs.projmatrix), on(rs.campos)
        self.W, self.H = int(rs.image_width), int(rs.image_height)
        self.view = _C.View(self.H, self.W, float(rs.tanfovx), float(rs.tanfovy), float(rs.scale_modifier),
                            float(rs.fade_size), int(rs.sh_degree), self.K,
                            int(bool(rs.filter_small)), int(bool(rs.filter_large)), int(bool(rs.prefiltered)),
                            int(bool(rs.debug)), 0, 0, 0.0, 0, _ptr(self.bg), _ptr(self.vm), _ptr(self.pm), _ptr(self.cp))
        # mode 1: raw parameters everywhere; mode 2: activated inputs + raw quaternions, gradients chained to the raw
        # parameters inside msgs_backward (include/msgs.h, msgs_gaussians_t::raw_params)
        self.rot_raw = _f32c(rotations_raw) if rotations_raw is not None else None
        mode = 0 if raw_features is None else (2 if rotations_raw is not None else 1)
        self.g = _C.Gaussians(P, mode, _ptr(self.means3D), _ptr(self.sh),
                              _ptr(self.colors), _ptr(self.opac), _ptr(self.scales), _ptr(self.rot), _ptr(self.cov),
                              _ptr(self.maxps), _ptr(self.minps), _ptr(self.occ), _ptr(self.dcd), _ptr(self.base),
                              _ptr(self.fdc), _ptr(self.frest), _ptr(self.rot_raw))
        self.view_ref, self.g_ref = C.byref(self.view), C.byref(self.g)


def _backward_scratch(P, D, dev, depth=False):
    lib = _C.lib
    if lib.msgs_get_deterministic():
        if depth:
            return _bytes(lib.msgs_backward_scratch_bytes_deterministic_depth(P, D), dev)
        return _bytes(lib.msgs_backward_scratch_bytes_deterministic(P, D), dev)
    return _bytes(lib.msgs_backward_scratch_bytes(P), dev)


# MSGS_NO_FORWARD_CLEAR=1: allocate the records in backward as before (a trainer that keeps MANY forward graphs alive before
# running their backwards would otherwise hold 80 bytes per Gaussian per graph)
_forward_clear = os.environ.get("MSGS_NO_FORWARD_CLEAR", "0") != "1"


# grad mode of the CALLER, noted right before .apply(): inside autograd.Function.forward grad mode is always off, and
# ctx.needs_input_grad is True under torch.no_grad() whenever the parameters require grad — every eval / viewer render of a
# trained model would otherwise allocate and clear 80 bytes per Gaussian for a backward that never comes
_caller = threading.local()


def _note_grad_mode():
    _caller.grad_enabled = torch.is_grad_enabled()


def _alloc_grad_records(ctx, P, dev):
    """The backward's per-Gaussian gradient records have to start from zero.  When a backward can follow, the buffer is
    allocated HERE and handed to the forward, whose blend kernel clears it on the side (include/msgs.h, grad_records: the
    kernel is instruction-bound, the stores are free) — the backward then skips its fill launch.  Not in the verification
    mode, whose scratch is sized by the instance count."""
    ctx.grad_rec = None
    ctx.det = bool(_C.lib.msgs_get_deterministic())
    # a backward can follow this forward (msgs_forward*: backward_follows — the tile launch order is prepared)
    ctx.backward_follows = bool(P > 0 and getattr(_caller, "grad_enabled", True) and any(ctx.needs_input_grad))
    if _forward_clear and ctx.backward_follows and not _C.lib.msgs_get_deterministic():
        ctx.grad_rec = _bytes(_C.lib.msgs_backward_scratch_bytes(P), dev)
    return ctx.grad_rec


def _take_backward_scratch(ctx, P, D, dev, depth=False):
    """(scratch, is_clear): the buffer the forward cleared, once; any later backward through the same graph
    (retain_graph) gets a fresh one that msgs_backward clears itself"""
    det = bool(_C.lib.msgs_get_deterministic())
    if det != bool(getattr(ctx, "det", False)):
        raise RuntimeError("diff_gaussian_rasterization: set_deterministic() changed between this forward and its backward (the "
                           "verification mode's backward reads what its own forward left behind)")
    rec = getattr(ctx, "grad_rec", None)
    ctx.grad_rec = None
    if rec is not None and not det:
        return rec, 1
    return _backward_scratch(P, D, dev, depth), 0


def _call_backward(lib, call, ctx, geom, binning, image, D, dL, dL_ddepth, scratch, grads, stream, camera=None):
    """msgs_backward, or msgs_backward_with_depth when the loss used the depth map (dL_ddepth: contiguous float32 [H,W]), or
    msgs_backward_with_camera when camera gradients are wanted (camera: _CameraGrads)"""
    args = (call.view_ref, call.g_ref, _ptr(ctx.radii), _ptr(geom), geom.numel(), D, _ptr(binning), binning.numel(),
            _ptr(image), image.numel(), _ptr(dL))
    tail = (_ptr(scratch), scratch.numel(), C.byref(grads), _C.timer_ptr(), stream)
    if camera is not None:
        cs = camera.scratch
        _C.check(lib.msgs_backward_with_camera(*args, _ptr(dL_ddepth), *tail[:3], _ptr(camera.dV), _ptr(camera.dPM),
                                               _ptr(camera.dcp), _ptr(cs), cs.numel(), *tail[3:]),
                 "msgs_backward_with_camera")
    elif dL_ddepth is None:
        _C.check(lib.msgs_backward(*args, *tail), "msgs_backward")
    else:
        _C.check(lib.msgs_backward_with_depth(*args, _ptr(dL_ddepth), *tail), "msgs_backward_with_depth")


def _call_backward_with_alpha(lib, call, ctx, geom, binning, image, D, dL, dL_ddepth, dL_dalpha, scratch, grads, stream,
                              camera=None):
    """msgs_backward_with_alpha: the loss used the alpha map (dL_dalpha: contiguous float32 [H,W]); depth and camera gradients
    as in _call_backward"""
    cs = camera.scratch if camera is not None else None
    cam = (camera.dV, camera.dPM, camera.dcp) if camera is not None else (None, None, None)
    _C.check(lib.msgs_backward_with_alpha(call.view_ref, call.g_ref, _ptr(ctx.radii), _ptr(geom), geom.numel(), D, _ptr(binning),
                                          binning.numel(), _ptr(image), image.numel(), _ptr(dL), _ptr(dL_ddepth), _ptr(dL_dalpha),
                                          _ptr(scratch), scratch.numel(), C.byref(grads), _ptr(cam[0]), _ptr(cam[1]), _ptr(cam[2]),
                                          _ptr(cs), cs.numel() if cs is not None else 0, _C.timer_ptr(), stream),
             "msgs_backward_with_alpha")


def _run_backward(lib, call, ctx, geom, binning, image, D, dL, dLd, dLa, scratch, grads, stream, cam):
    """today's entry (_call_backward) unless the loss used the alpha map"""
    if dLa is None:
        _call_backward(lib, call, ctx, geom, binning, image, D, dL, dLd, scratch, grads, stream, cam)
    else:
        _call_backward_with_alpha(lib, call, ctx, geom, binning, image, D, dL, dLd, dLa, scratch, grads, stream, cam)


# Camera gradients.  autograd does not look inside the settings NamedTuple, so when grad mode is on and
# one of its viewmatrix / projmatrix / campos requires grad, those three tensors also go to the autograd Function as extra
# trailing inputs; the backward then returns their gradients (in each tensor's own shape, dtype and device).  Otherwise
# nothing is added and the call is exactly the one without camera gradients.
def _camera_inputs(rs):
    if not torch.is_grad_enabled():
        return ()
    cam = (rs.viewmatrix, rs.projmatrix, rs.campos)
    return cam if any(torch.is_tensor(t) and t.requires_grad for t in cam) else ()


def _note_camera(ctx, camera, behind=0):
    """forward: which camera inputs want a gradient (ctx.camera: () or three (shape, dtype, device) | None); `behind`: the
    number of trailing inputs that follow the camera's three (_extra_inputs)"""
    if not camera:
        ctx.camera = ()
        return
    n = len(ctx.needs_input_grad) - behind
    want = ctx.needs_input_grad[n - 3:n]
    ctx.camera = tuple((t.shape, t.dtype, t.device) if w else None for t, w in zip(camera, want))


# Alpha map and background gradient.  The trailing inputs of the three autograd Functions are, in this order,
#   [viewmatrix, projmatrix, campos]   _camera_inputs: three tensors or nothing
#   [bg]                               grad mode on and settings.bg requires grad: the background colour, for its gradient
#   [_ALPHA]                           return_alpha=True: a marker (not a tensor) — the Function returns alpha as a sixth output
#   [_AbsgradMarker]                   absgrad=True: a marker holding a weak reference to the caller's means2D
#   [_DISTORTION]                      return_distortion=True: a marker — the Function returns the distortion map [H,W] behind
#                                      alpha and in front of the feature map
#   [_MEDIAN]                          return_median_depth=True: a marker — the Function returns median_depth [H,W] float32 and
#                                      median_id [H,W] int32 behind the distortion map and in front of the feature map (M15)
#   [_FEATURES, features]              features given: a marker and the [P,C] tensor, always LAST — the marker tells the tensor
#                                      from bg; the Function returns the feature map [C,H,W] as its last output
# A call that asks for none of the new things passes exactly what it passed before them.
class _AlphaMarker:
    def __repr__(self):
        return "return_alpha"


_ALPHA = _AlphaMarker()


# Absgrad (AbsGS, gsplat's absgrad=True).  The backward of a call made with absgrad=True also runs msgs_absgrad
# — one more launch chain on the backward's stream, fed the same dL/dcolor, dL/ddepth and dL/dalpha, independent of whatever the
# main backward does with its gradients (sinks, accumulators, the optimizer step) — and ASSIGNS the result [P,3] float32, in
# means2D's shape, to `means2D.absgrad` of the tensor object the caller passed: beside .grad, where densification reads it.
# Assigned on every backward (retain_graph: the latest one), never accumulated.
class _AbsgradMarker:
    def __init__(self, means2D):
        self.means2D = weakref.ref(means2D)

    def __repr__(self):
        return "absgrad"


# Feature channels (4.12).  `features` [P,C] is splatted with the blend weights of the colour render into one
# more output [C,H,W], F[c,p] = sum_i f_ic alpha_ip T_ip over background 0 (msgs_features_forward: a replay of the blend walk
# behind the forward).  A loss on the map sends gradients to the features and — as C more colour channels — to the geometry: the
# backward first runs msgs_features_backward, which adds the features' geometry sums to the gradient records, then today's
# backward with scratch_is_clear = 1 on top of them.  A loss that does not use the map takes today's backward unchanged.
class _FeaturesMarker:
    def __repr__(self):
        return "features"


_FEATURES = _FeaturesMarker()


def _check_features(features, P, dev):
    """the [P,C] feature tensor of a call, or None when none was given (None, or an empty tensor of a model with Gaussians);
    every guard runs here, before any launch"""
    if features is None or (features.numel() == 0 and not (P == 0 and features.dim() == 2 and features.shape[1] > 0)):
        return None
    if _C.lib.msgs_get_deterministic():
        raise ValueError("features are not offered in the verification mode (set_deterministic): that mode checks the "
                         "gradients of the reference's outputs")
    _check_rows("features", features, P, None)
    if features.dim() != 2:
        raise ValueError(f"features must have shape [{P}, C], got {tuple(features.shape)}")
    if features.device.type != "cuda" or features.device != dev:
        raise RuntimeError("diff_gaussian_rasterization (MI355X build): features must live on the HIP device of the model "
                           "('cuda'); there is no CPU path")
    return features


# Depth distortion (4.13).  return_distortion=True adds one output [H,W] behind alpha:
# Dist_p = 2 sum_{j<i} w_ip w_jp (z_i - z_j), the signed list-order form of the Mip-NeRF 360 distortion loss over the pairs the
# backward counts (msgs_distortion_forward: a replay of the blend walk behind the forward).  A loss on the map makes the
# backward first run msgs_distortion_backward, which adds the map's geometry sums and its dL/dz sum to the gradient records,
# then today's depth-variant backward with scratch_is_clear = 1 on top of them.  A loss that does not use the map takes today's
# backward unchanged.
class _DistortionMarker:
    def __repr__(self):
        return "return_distortion"


_DISTORTION = _DistortionMarker()


# Median depth and Gaussian id (4.15).  return_median_depth=True adds two outputs behind the distortion map:
# median_depth [H,W] float32, the view depth of the Gaussian at which the ray's transmittance falls through 1/2 (the last blended
# entry with T_i > 0.5, T by the forward's own recurrence), and median_id [H,W] int32, that Gaussian's row (-1 / 0.0 where nothing
# was blended; never differentiable).  msgs_median_depth_forward: a front-to-back replay of the tile lists behind the forward.
# A loss on median_depth makes the backward first run msgs_median_depth_backward, which adds every pixel's gradient to slot 9
# (dL/dz) of its Gaussian's record, then today's depth-variant backward with scratch_is_clear = 1 on top of them.  A loss that
# does not use the map takes today's backward unchanged.
class _MedianMarker:
    def __repr__(self):
        return "return_median_depth"


_MEDIAN = _MedianMarker()


def _extra_inputs(rs, return_alpha=False, absgrad=False, means2D=None, features=None, model=None, return_distortion=False,
                  return_median_depth=False):
    """model: the call's means3D / xyz (its rows and device check `features`)"""
    if (absgrad or return_distortion or return_median_depth) and _C.lib.msgs_get_deterministic():
        for flag, message in ((absgrad, "absgrad=True is not offered in the verification mode (set_deterministic): that mode "
                                        "checks the gradients, it does not train"),
                              (return_distortion, "return_distortion=True is not offered in the verification mode "
                                                  "(set_deterministic): that mode checks the gradients of the reference's outputs"),
                              (return_median_depth, "return_median_depth=True is not offered in the verification mode "
                                                    "(set_deterministic): that mode checks the gradients of the reference's outputs")):
            if flag:
                raise ValueError(message)
    if features is not None:
        features = _check_features(features, int(model.shape[0]), model.device)
    extra = list(_camera_inputs(rs))
    if torch.is_grad_enabled() and torch.is_tensor(rs.bg) and rs.bg.requires_grad:
        extra.append(rs.bg)
    if return_alpha:
        extra.append(_ALPHA)
    if absgrad:
        extra.append(_AbsgradMarker(means2D))
    if return_distortion:
        extra.append(_DISTORTION)
    if return_median_depth:
        extra.append(_MEDIAN)
    if features is not None:
        extra += (_FEATURES, features)
    return tuple(extra)


def _note_extra(ctx, extra):
    """forward: split the trailing inputs; leaves ctx.camera (_note_camera), ctx.bg ((shape, dtype, device) when the
    background wants a gradient, else None), ctx.n_extra_tail (inputs behind the camera's), ctx.absgrad (the marker or None)
    ctx.features (the caller's tensor or None), ctx.feat (its contiguous float32 form), ctx.distortion (return_distortion),
    ctx.median (return_median_depth) and returns return_alpha"""
    ctx.features = ctx.feat = None
    n_feat = 0
    if len(extra) >= 2 and extra[-2] is _FEATURES:
        ctx.features, n_feat = extra[-1], 2
        ctx.feat = _f32c(extra[-1].detach())
        ctx.features_want = bool(ctx.needs_input_grad[-1])
        extra = extra[:-2]
    ctx.median = bool(extra) and extra[-1] is _MEDIAN
    n_feat += int(ctx.median)
    extra = extra[:-1] if ctx.median else extra
    ctx.distortion = bool(extra) and extra[-1] is _DISTORTION
    n_feat += int(ctx.distortion)                              # (from here on: the inputs behind the absgrad marker)
    extra = extra[:-1] if ctx.distortion else extra
    ctx.absgrad = extra[-1] if extra and isinstance(extra[-1], _AbsgradMarker) else None
    n_abs = int(ctx.absgrad is not None)
    rest = extra[:-1] if n_abs else extra
    alpha = bool(rest) and rest[-1] is _ALPHA
    rest = rest[:-1] if alpha else rest
    bg = rest[-1] if len(rest) in (1, 4) else None
    camera = rest[:3] if len(rest) >= 3 else ()
    ctx.n_extra_tail = len(extra) - len(camera) + n_feat
    ctx.has_bg = bg is not None
    ctx.bg = None
    if bg is not None and ctx.needs_input_grad[len(ctx.needs_input_grad) - 1 - int(alpha) - n_abs - n_feat]:
        ctx.bg = (bg.shape, bg.dtype, bg.device)
    _note_camera(ctx, camera, ctx.n_extra_tail)
    ctx.return_alpha = alpha
    return camera, alpha


def _replay_args(call, P, geom, binning, image, D):
    """the nine leading arguments of every replay of a forward's state (include/msgs.h: msgs_absgrad, msgs_features_*,
    msgs_distortion_*, msgs_median_depth_forward, msgs_contrib_accumulate): the view, P, then geom, binning and image state with
    their byte counts, the instance count D behind geom's"""
    return (call.view_ref, P, _ptr(geom), geom.numel(), D, _ptr(binning), binning.numel() if binning is not None else 0,
            _ptr(image), image.numel())


def _replay_forward(name, probe, call, state, *tail):
    """what the three *_forward replays share: the state resolved (a deferred forward first waits for its instance count: correct,
    at the price of that view's overlap), the tests' probe, then lib.`name`(replay arguments, *tail, stream) on the current
    stream of the call's device, behind the forward that left `state`"""
    geom, binning, image, D = _resolve(state)
    _launch(probe, name, call.device, *_replay_args(call, call.P, geom, binning, image, D), *tail)


def _absgrad(ctx, call, geom, binning, image, D, dL, dLd, dLa, dev, stream):
    """backward of an absgrad=True call: msgs_absgrad on the backward's stream, the result assigned to means2D.absgrad"""
    m2 = ctx.absgrad.means2D()
    if m2 is None:                          # the caller dropped the tensor: nobody can read the attribute
        return
    P = call.P
    out = torch.empty(P, 3, dtype=torch.float32, device=dev)
    scratch = _bytes(_C.lib.msgs_absgrad_scratch_bytes(P), dev)
    _C.check(_C.lib.msgs_absgrad(*_replay_args(call, P, geom, binning, image, D), _ptr(dL), _ptr(dLd), _ptr(dLa), _ptr(scratch),
                                 scratch.numel(), _ptr(out), stream), "msgs_absgrad")
    m2.absgrad = out.view(m2.shape) if out.shape != m2.shape and out.numel() == m2.numel() else out


def _alpha_map(call, image, alpha, stream):
    """alpha = 1 - final_T of the image state, on `stream` behind the forward that wrote it"""
    _C.check(_C.lib.msgs_alpha_map(call.view_ref, _ptr(image), image.numel(), _ptr(alpha), stream), "msgs_alpha_map")


def _bg_grad(ctx, view_ref, image, dL, W, H, dev, stream):
    """dL/dbg in the background tensor's own shape, dtype and device (msgs_bg_grad: two launches, independent of the backward
    call); image None: a view without Gaussians (final_T = 1)"""
    shape, dtype, device = ctx.bg
    out = torch.empty(3, dtype=torch.float32, device=dev)
    scratch = _bytes(_C.lib.msgs_bg_grad_scratch_bytes(W, H), dev)
    _C.check(_C.lib.msgs_bg_grad(view_ref, _ptr(image), image.numel() if image is not None else 0, _ptr(dL), _ptr(out),
                                 _ptr(scratch), scratch.numel(), stream), "msgs_bg_grad")
    return out.view(shape).to(device=device, dtype=dtype)


def _extra_grads(ctx, g_cam, g_bg):
    """gradients of the trailing inputs in their order: camera, bg, the alpha marker, the absgrad marker, the distortion marker,
    the median marker, the features marker and dL/dfeatures (in the tensor's shape and dtype; None when the loss did not use the feature map)"""
    g_feat = ()
    if ctx.features is not None:
        g, ctx.g_features = getattr(ctx, "g_features", None), None
        g_feat = (None, g.view(ctx.features.shape).to(ctx.features.dtype) if g is not None and ctx.features_want else None)
    return tuple(g_cam) + ((g_bg,) if ctx.has_bg else ()) + ((None,) if ctx.return_alpha else ()) + \
        ((None,) if ctx.absgrad is not None else ()) + ((None,) if ctx.distortion else ()) + \
        ((None,) if ctx.median else ()) + g_feat


def _split_grad_tail(ctx, tail):
    """the gradients of the outputs behind the reference's five: (grad_alpha, grad_distortion, grad_median, grad_features);
    grad_median is that of median_depth — median_id, the output behind it, is not differentiable"""
    k_med = int(ctx.return_alpha) + int(ctx.distortion)
    return (tail[0] if ctx.return_alpha else None), (tail[int(ctx.return_alpha)] if ctx.distortion else None), \
        (tail[k_med] if ctx.median else None), (tail[-1] if ctx.features is not None else None)


_features_probe = None             # tests: a callable (name) run in front of every msgs_features_* call


def _features_forward(ctx, call, state):
    """the feature map [C,H,W] of a call with features: msgs_features_forward on the current stream, behind the forward that
    left `state`.  A deferred forward is resolved first (the replay needs the instance count): correct, at the price of that
    view's overlap."""
    Cn = int(ctx.feat.shape[1])
    out = torch.empty(Cn, call.H, call.W, dtype=torch.float32, device=call.device)
    _replay_forward("msgs_features_forward", _features_probe, call, state, _ptr(ctx.feat), Cn, _ptr(out))
    return out


def _features_backward(ctx, call, geom, binning, image, D, grad_features, scratch, is_clear, dev, stream):
    """In front of _run_backward, when the loss used the feature map: dL/dfeatures (left on ctx for _extra_grads) and, when a
    geometry input wants a gradient, the features' geometry sums ADDED to the gradient records in `scratch` — cleared here
    unless it is the buffer the forward cleared.  Returns the scratch_is_clear flag to hand on: 1 once the records hold sums
    that msgs_backward* has to add to."""
    lib = _C.lib
    P, Cn = call.P, int(ctx.feat.shape[1])
    G = _f32c(grad_features)
    out = torch.empty(P, Cn, dtype=torch.float32, device=dev)
    geom_share = bool(ctx.features_geom)
    if geom_share and not is_clear:
        scratch.zero_()
    acc = _bytes(lib.msgs_features_scratch_bytes(P, Cn), dev)
    if _features_probe is not None:
        _features_probe("msgs_features_backward")
    _C.check(lib.msgs_features_backward(*_replay_args(call, P, geom, binning, image, D), _ptr(ctx.feat), Cn, _ptr(G),
                                        _ptr(scratch) if geom_share else None, scratch.numel() if geom_share else 0, _ptr(acc),
                                        acc.numel(), _ptr(out), stream), "msgs_features_backward")
    ctx.g_features = out
    return 1 if geom_share else is_clear


_distortion_probe = None           # tests: a callable (name) run in front of every msgs_distortion_* call


def _distortion_forward(ctx, call, state):
    """the distortion map [H,W] of a return_distortion=True call: msgs_distortion_forward on the current stream, behind the
    forward that left `state`; the moment map the backward needs stays on ctx.  A deferred forward is resolved first (the replay
    needs the instance count): correct, at the price of that view's overlap."""
    out = torch.empty(call.H, call.W, dtype=torch.float32, device=call.device)
    ctx.dist_moment = torch.empty_like(out)
    _replay_forward("msgs_distortion_forward", _distortion_probe, call, state, _ptr(out), _ptr(ctx.dist_moment))
    return out


def _distortion_backward(ctx, call, geom, binning, image, D, grad_distortion, dLd, scratch, is_clear, dev, stream):
    """In front of _run_backward, when the loss used the distortion map: the map's geometry sums (record slots 0..5) and its
    dL/dz sum (slot 9) ADDED to the gradient records in `scratch` — cleared here unless it is the buffer the forward cleared.
    Returns (dL/ddepth to hand on, scratch_is_clear to hand on): the depth variant of the backward consumes slot 9, so a loss
    without a depth term passes a zero map (fmaf(z, 0, g) is exact: the colour sums keep their bits)."""
    if not is_clear:
        scratch.zero_()
    if _distortion_probe is not None:
        _distortion_probe("msgs_distortion_backward")
    _C.check(_C.lib.msgs_distortion_backward(*_replay_args(call, call.P, geom, binning, image, D), _ptr(ctx.dist_moment),
                                             _ptr(_f32c(grad_distortion)), _ptr(scratch), scratch.numel(), stream),
             "msgs_distortion_backward")
    if dLd is None:
        dLd = torch.zeros(call.H, call.W, dtype=torch.float32, device=dev)
    return dLd, 1


_median_probe = None               # tests: a callable (name) run in front of every msgs_median_depth_* call


def _median_depth_forward(ctx, call, state):
    """(median_depth [H,W] float32, median_id [H,W] int32) of a return_median_depth=True call: msgs_median_depth_forward on the
    current stream, behind the forward that left `state`; the id map stays on ctx for the backward.  A deferred forward is
    resolved first (the replay needs the instance count): correct, at the price of that view's overlap."""
    out = torch.empty(call.H, call.W, dtype=torch.float32, device=call.device)
    ctx.median_id = ids = torch.empty(call.H, call.W, dtype=torch.int32, device=call.device)
    _replay_forward("msgs_median_depth_forward", _median_probe, call, state, _ptr(out), _ptr(ids))
    return out, ids


def _median_depth_backward(ctx, call, D, grad_median, dLd, scratch, is_clear, dev, stream):
    """In front of _run_backward, when the loss used median_depth: every pixel's gradient ADDED to slot 9 (dL/dz) of the record
    of its median Gaussian in `scratch` — cleared here unless it is the buffer the forward cleared or already holds the sums of
    the feature / distortion maps.  Returns (dL/ddepth to hand on, scratch_is_clear to hand on): the depth variant of the
    backward consumes slot 9, so a loss without a depth term passes a zero map (fmaf(z, 0, g) is exact: the colour sums keep
    their bits)."""
    if not is_clear:
        scratch.zero_()
    if D > 0:                                                   # (no instance: every id is -1, nothing to add)
        if _median_probe is not None:
            _median_probe("msgs_median_depth_backward")
        _C.check(_C.lib.msgs_median_depth_backward(call.view_ref, call.P, _ptr(ctx.median_id), _ptr(_f32c(grad_median)),
                                                   _ptr(scratch), scratch.numel(), stream), "msgs_median_depth_backward")
    if dLd is None:
        dLd = torch.zeros(call.H, call.W, dtype=torch.float32, device=dev)
    return dLd, 1


def _refuse_camera_with(camera):
    """the optimizer step inside the backward and the view-parallel exchange of the SH factors do not offer camera
    gradients: refused before anything is launched"""
    if not camera:
        return
    if getattr(_step_in_backward, "opt", None) is not None:
        raise ValueError("camera gradients (a viewmatrix / projmatrix / campos that requires grad) cannot be combined with "
                         "set_optimizer_in_backward")
    if _sinks.sh_factor[0] is not None:
        raise ValueError("camera gradients (a viewmatrix / projmatrix / campos that requires grad) cannot be combined with "
                         "the factored SH gradient of the view-parallel exchange")


class _CameraGrads:
    """float32 outputs of msgs_backward_with_camera (None = not wanted) and its scratch"""

    def __init__(self, ctx, P, dev):
        vm, pm, cp = ctx.camera
        self.dV = torch.empty(16, dtype=torch.float32, device=dev) if vm is not None else None
        self.dPM = torch.empty(16, dtype=torch.float32, device=dev) if pm is not None else None
        self.dcp = torch.empty(3, dtype=torch.float32, device=dev) if cp is not None else None
        self.scratch = _bytes(_C.lib.msgs_camera_grad_scratch_bytes(P), dev)

    def grads(self, ctx):
        return tuple(None if m is None else g.view(m[0]).to(device=m[2], dtype=m[1])
                     for g, m in zip((self.dV, self.dPM, self.dcp), ctx.camera))


def set_deterministic(on=True):
    """Process-wide switch: the VERIFICATION mode (ms-gs_amd/csrc/literal.hip).  Forward and backward blend loops
    restate the reference's per-pixel arithmetic literally (float32, no FMA contraction, exp evaluated in double and rounded
    once), the nine per-(pixel, Gaussian) products are summed in double in a fixed order (in-tile tree, per-entry stores, stable
    grouping by Gaussian): bitwise reproducible by construction, and — against the CPU checker of the tests evaluated the same
    way (exp in double) — every gradient tensor within 1e-4, the north star's sentence as written
    (tests/test_literal_gpu.py).  Several times slower than the default path.  Must not change between a forward and its
    backward.  A checker, not a trainer: absgrad=True raises ValueError at the forward while it is on.  Returns the previous
    setting.  Also: MSGS_DETERMINISTIC=1 in the environment."""
    return bool(_C.lib.msgs_set_deterministic(1 if on else 0))


# instance-count guess per (device, P, W, H, filters): the next call sizes its binning buffers from it (+12.5 %), and
# msgs_forward launches stage 2 on them speculatively, with grids sized for that capacity — so the guess has to follow the
# scene DOWN quickly as well (an outlier, e.g. one render of the same model without its multi-scale filters, would otherwise
# leave every following call with stage-2 grids and buffers many times too large): it halves its excess over the last count
# on every call; views whose counts differ by up to ~28 % alternate without outgrowing it.
class _LRU(dict):
    """a dict that forgets its least recently WRITTEN key beyond `cap` entries (the trainer's model changes size every hundred
    iterations — densify / prune, /root/reference/train.py:253-264 — and a wholesale clear() would throw away every other key's state)"""

    def __init__(self, cap=256):
        super().__init__()
        self.cap = cap

    def __setitem__(self, k, v):
        if k in self:
            super().__delitem__(k)                  # re-insert at the end: most recent
        super().__setitem__(k, v)
        while len(self) > self.cap:
            super().__delitem__(next(iter(self)))

    def setdefault(self, k, default=None):
        # (dict.setdefault would insert without the cap)
        if k not in self:
            self[k] = default
        return self[k]


_last_instances = _LRU()
# ... and per (device, W, H, filters) whatever the model size: (instances, P) of the latest forward.  The reference's training loop
# changes P every densification interval (train.py:253-264: clone / split / prune, a few per cent) and the pyramid level with
# every camera stack (:152-194): a key that has never been seen still gets a guess — the last count of the same view shape, scaled
# by P — so that only the very first forward of a view shape takes the non-speculative route (bench.py reference_schedule).
_instances_by_view = _LRU()
forward_stats = {"forwards": 0, "non_speculative": 0}        # since import (bench.py reference_schedule reads the difference)


def _instance_guess(key):
    g = _last_instances.get(key)
    if g is not None:
        return g
    v = _instances_by_view.get((key[0],) + key[2:])
    if v is None:
        return None
    D, P_ref = v
    ratio = key[1] / max(P_ref, 1)
    if not 0.8 <= ratio <= 1.25:        # another model altogether (D does not scale with P across scenes): no guess
        return None
    return int(D * ratio) + 1


def _capacity(guess):
    """instances the speculative stage 2 of a call with this guess has room for at least (+12.5 % and a constant margin; the
    library sizes it from the buffers' bytes, which _bytes may round up); a view with more takes the redo on exact buffers"""
    return guess + (guess >> 3) + 4096


def _note_instances(key, D, guess):
    _last_instances[key] = max(D, (guess + D) // 2) if guess is not None else D
    _instances_by_view[(key[0],) + key[2:]] = (D, key[1])


# Occlusion cut-off pass (include/msgs.h, msgs_set_occlusion): ONE launch between the per-Gaussian stage and the depth sort that a
# view without cover candidates leaves after its first grid barrier (~5 us) — it runs on EVERY forward; the adaptive skip policy
# of round 5 (and its cliff: a closing view among the skipped calls rendered uncut) is gone.  What is left per (device, P, W, H,
# filters) key is a performance HINT for one small launch: the queue that gives every Gaussian with more than 96 tile instances
# a workgroup of its own (msgs_view_t.no_heavy_queue) pays off when covers closed blocks — the nearest ranks are then all
# giants — and is a wasted ~3 us launch otherwise; it is kept on for HEAVY_QUEUE_MEMORY calls after the key last closed a block
# (msgs_forward_info: the answer travels with the instance count) and on the key's first call.  Outputs never depend on it.
HEAVY_QUEUE_MEMORY = 32
_occ_hot = _LRU(1024)        # key -> calls for which the queue stays on: refreshed by every call of the key that closes a block


def _heavy_queue_off(key):
    return _occ_hot.get(key, 1) == 0


# Depth-slab binning (include/msgs.h, msgs_view_t.slab_fraction).  Stage 2 bins and blends the nearest depth ranks
# first and then only the tiles in which a pixel is still blending: bit-identical outputs, and on a view whose pixels terminate
# early (BASELINE C5: 54.9 M instances, 4.35 M traversed) emit / tile sort / ranges shrink to a fraction.  On a view whose
# pixels walk most of their lists (C3: 44 %) it would only add launches, so the wrapper engages it per (device, P, W, H, filters)
# key from what the library publishes about the key's EARLIER frames (msgs_view_t.feedback_tag -> msgs_forward_info: instances D,
# traversed entries D_trav; one frame late, no synchronisation):
#   slab_policy "adaptive" (default)   on while D >= SLAB_MIN_INSTANCES and D >= SLAB_MIN_RATIO * D_trav (else the key asks for a
#                                      publication on every SLAB_RECHECK-th call only), with
#                                      slab_fraction = 2 * D_trav / D clamped to [0.04, 0.30]; off for SLAB_BACKOFF calls of the key
#                                      when a slab frame emitted more than 70 % of D anyway (the view changed)
#   "never" / a float                  never / always with that fraction (tests, A/B runs)
# Either way the result is exact; the worst case of a wrong guess is ~15 % of a binning pass.
slab_policy = os.environ.get("MSGS_SLAB_POLICY", "adaptive")
SLAB_MIN_INSTANCES = 2_000_000
SLAB_MIN_RATIO = 6.0
SLAB_BACKOFF = 64
SLAB_RECHECK = 16
_fb_stats = _LRU(1024)       # key -> {"D", "D_trav", "backoff", ...}: the latest publication of the key
_fb_tag_of = {}              # key -> tag (1 .. 2^31 - 1)
_fb_key_of = {}              # tag -> key
_fb_next_tag = [0]


def _slab_plan(key, guess, tiles):
    """(slab_fraction, feedback_tag) for the next forward of `key`.  The statistics are kept per VIEW SHAPE (device, W, H,
    filters), not per model size: D / D_trav is a property of the scene and the view, and the trainer changes P by a few per cent
    every densification interval"""
    key = (key[0],) + key[2:]
    pol = slab_policy
    if pol == "never":
        return 0.0, 0
    if pol != "adaptive":
        return float(pol), 0
    if tiles < 2048 or guess is None or guess < SLAB_MIN_INSTANCES // 2:
        return 0.0, 0                                   # small frames: no feedback launch either
    tag = _fb_tag_of.get(key)
    if tag is None:
        if len(_fb_tag_of) > 1024:
            _fb_tag_of.clear(); _fb_key_of.clear(); _fb_stats.clear()
        _fb_next_tag[0] = _fb_next_tag[0] % 0x7FFFFFF0 + 1        # never reused while an old publication may still sit in a status block
        tag = _fb_tag_of[key] = _fb_next_tag[0]
        _fb_key_of[tag] = key
    st = _fb_stats.get(key)
    if st is None:
        return 0.0, tag
    if st["D"] < SLAB_MIN_INSTANCES or st["D"] < SLAB_MIN_RATIO * max(st["D_trav"], 1):
        # not a view for slabs (BASELINE C3: D = 2.3 x D_trav): look again every SLAB_RECHECK-th call only — the publication is
        # one small kernel with a system-scope store, ~4 us per forward
        st["idle"] = (st.get("idle", 0) + 1) % SLAB_RECHECK
        return 0.0, (tag if st["idle"] == 0 else 0)
    if st.get("backoff", 0) > 0:
        st["backoff"] -= 1
        return 0.0, tag
    return min(0.30, max(0.04, 2.0 * st["D_trav"] / st["D"])), tag


def _note_info(key):
    """after the instance count of a forward has been collected on this thread: what travelled with it"""
    info = (C.c_int64 * 8)()
    _C.lib.msgs_forward_info(info)
    tag = int(info[2])
    if tag:
        k = _fb_key_of.get(tag)
        if k is not None:
            st = _fb_stats.setdefault(k, {})
            st["D"], st["D_trav"] = int(info[3]), int(info[4])
            if info[5] >= 0:                            # that frame ran in slab mode: did it pay?
                st["n_open"], st["DA"], st["DB"] = int(info[5]), int(info[6]), int(info[7])
                if info[7] < 0:
                    raise RuntimeError(f"diff_gaussian_rasterization: slab B outgrew its buffers (SlabHeader overflow flag) "
                                       f"[view {k}: D {int(info[3])}, D_trav {int(info[4])}, open tiles {int(info[5])}, slab A {int(info[6])}]")
                if int(info[6]) + int(info[7]) > 0.7 * max(int(info[3]), 1):
                    st["backoff"] = SLAB_BACKOFF
    _occ_hot[key] = HEAVY_QUEUE_MEMORY if info[1] else max(_occ_hot.get(key, 1) - 1, 0)


def _note_count(key, D, guess, done):
    """after the instance count D of a forward has been collected on this thread; done: its stage 2 needs no redo"""
    _note_instances(key, D, guess)
    _note_info(key)
    forward_stats["forwards"] += 1
    if not done:
        forward_stats["non_speculative"] += 1


_size_cache = _LRU()


def _sizes(P, W, H):
    """(geom, stage-1 scratch, image) byte counts per (P, W, H): three ctypes calls saved per forward"""
    k = (P, W, H)
    v = _size_cache.get(k)
    if v is None:
        lib = _C.lib
        v = _size_cache[k] = (int(lib.msgs_geom_bytes(P)), int(lib.msgs_stage1_scratch_bytes(P)), int(lib.msgs_image_bytes(W, H)))
    return v


def _a256(n):
    return (int(n) + 255) & ~255


def _stage2_bytes(D, W, H, frac):
    """(binning, stage-2 scratch) byte counts that serve D instances — with room for slab A's ids in front of slab B's when the call
    asks for depth slabs"""
    lib = _C.lib
    if frac > 0.0:
        return int(lib.msgs_binning_bytes_slab(D, W, H, frac)), int(lib.msgs_stage2_scratch_bytes_slab(D, W, H))
    return int(lib.msgs_binning_bytes(D, W, H)), int(lib.msgs_stage2_scratch_bytes(D, W, H))


def _redo_stage2(call, geom, image, D, frac, outs, grad_rec, backward_follows, stream, alpha=None):
    """Stage 2 again, on buffers sized for the instance count D, when the speculative one did not serve it (first frame of this
    shape, or the scene grew past the margin); returns the new binning buffer.  The outputs are overwritten in place.

    This run reads the geom a truncated speculative stage 2 (capacity < D) may have written to.  What that run left there is
    rewritten or no longer read as input (tests/test_stage2_routes_gpu.py): the SlabHeader counts, the open-tile bitmap and
    n_open are reset by slab_split_kernel; the heavy-queue word is cleared before each emit; offs_b / scan_b are recomputed by
    slab B's recount and scan; and the flag that marks offs_b as stage 1's cell ranges (SlabHeader pad[0]) was cleared by the
    first run's slab B scan, so this run recounts without the cell prefilter."""
    color, acc_ps, depth = outs
    nb_, ns_ = _stage2_bytes(D, call.W, call.H, frac)
    binning = _bytes(nb_, call.device)
    scratch2 = _bytes(ns_, call.device)
    _C.check(_C.lib.msgs_forward_stage2(call.view_ref, call.g_ref, _ptr(geom), geom.numel(), D,
                                        _ptr(binning), binning.numel(), _ptr(scratch2), scratch2.numel(),
                                        _ptr(image), image.numel(), _ptr(color), _ptr(acc_ps), _ptr(depth),
                                        _ptr(grad_rec), grad_rec.numel() if grad_rec is not None else 0,
                                        int(backward_follows), _C.timer_ptr(), stream), "msgs_forward_stage2")
    if alpha is not None:                  # final_T was overwritten: the alpha map again, behind it on the same stream
        _alpha_map(call, image, alpha, stream)
    return binning


# ---- deferred forwards: several views in flight from one host thread (include/msgs.h msgs_forward_launch / _finish) ----
# Inside `with deferred_forward() as pending:` every forward of this package only LAUNCHES (stage 1 and, on buffers sized
# from the instance-count guess, stage 2) and returns its output tensors at once — valid in stream order, like any
# asynchronous kernel result — without waiting for the instance count.  The wait happens in _PendingForward.resolve():
# when the view's backward starts, when the caller resolves the entries of `pending`, or at the end of the `with` block,
# whichever comes first.  If a scene outgrew its guess, resolve() redoes stage 2 on exact buffers on the view's stream
# (the outputs are overwritten in place, stream-ordered behind the truncated result).  A consumer that reads an output
# on ANOTHER stream, or on the host, must resolve the view first.  host/multi_view.py builds the two-stream pipelines
# on top of this.
_deferred = threading.local()

_status_pool = []
_status_lock = threading.Lock()


def _take_status():
    with _status_lock:
        if _status_pool:
            return _status_pool.pop()
    h = C.c_void_p()
    _C.check(_C.lib.msgs_status_create(C.byref(h)), "msgs_status_create")
    return h


def _give_status(h):
    with _status_lock:
        _status_pool.append(h)


class deferred_forward:
    """Context manager; yields the list the forwards' _PendingForward objects are appended to (in call order)."""

    def __enter__(self):
        self.prev = getattr(_deferred, "pending", None)
        _deferred.pending = self.list = []
        return self.list

    def __exit__(self, *exc):
        _deferred.pending = self.prev
        first = None
        for p_ in self.list:                  # every launched view is waited for, also behind one that failed
            if exc[0] is None and first is None:
                try:
                    p_.resolve()
                except Exception as e:        # noqa: BLE001 - re-raised below, after the other handles are finished
                    first = e
            else:
                p_.abandon()
        if first is not None:
            raise first
        return False


class _PendingForward:
    """State of one launched forward: resolve() -> (geom, binning, image, D), waiting for the count if nobody has yet."""

    def __init__(self, call, status, stream, key, guess, geom, binning, image, outs, grad_rec, keep, backward_follows=False,
                 scratch1=None, alpha=None):
        self.backward_follows = bool(backward_follows)
        self.alpha = alpha                    # the alpha map of a return_alpha call: rewritten behind a redo of stage 2
        self.scratch1 = scratch1              # holds the device status words msgs_forward_finish may still copy from
        self.call, self.status, self.stream, self.key, self.guess = call, status, stream, key, guess
        self.geom, self.binning, self.image, self.outs, self.grad_rec, self.keep = geom, binning, image, outs, grad_rec, keep
        self.state = self.error = None
        self.lock = threading.Lock()

    def resolve(self):
        with self.lock:
            if self.state is not None:
                return self.state
            if self.status is None:                     # an earlier resolve() failed: the view has no result
                raise RuntimeError("this forward failed when its instance count was collected") from self.error
            call = self.call
            D, done = C.c_int64(0), C.c_int32(0)
            status, self.status = self.status, None
            try:
                _C.check(_C.lib.msgs_forward_finish(status, C.byref(D), C.byref(done)), "msgs_forward_finish")
            except Exception as e:
                self.error = e
                raise
            finally:
                _give_status(status)
                self.scratch1 = None
            D = int(D.value)
            _note_count(self.key, D, self.guess, done.value)
            if not done.value:
                self.error = RuntimeError("stage 2 on exact buffers failed")     # cleared below
                with _on_device(call.device), torch.cuda.stream(self.stream):
                    self.binning = _redo_stage2(call, self.geom, self.image, D, float(call.view.slab_fraction), self.outs,
                                                self.grad_rec, self.backward_follows, C.c_void_p(self.stream.cuda_stream),
                                                self.alpha)
            self.state = (self.geom, self.binning, self.image, D)
            self.outs = self.grad_rec = self.error = self.alpha = None
            return self.state

    def abandon(self):
        """the caller's block raised: finish the wait (the handle must not be reused while a kernel can still write its
        status words) and swallow secondary errors"""
        try:
            self.resolve()
        except Exception:
            pass


def _resolve(state):
    return state.resolve() if isinstance(state, _PendingForward) else state


def _forward_impl(call, grad_rec=None, backward_follows=False, want_alpha=False):
    """-> (color, acc_ps, depth, radii, pixel_sizes, state); with want_alpha the alpha map sits in front of `state`"""
    dev, P, W, H = call.device, call.P, call.W, call.H
    lib = _C.lib
    key = (dev.index, P, W, H, call.view.filter_small, call.view.filter_large)
    pending = getattr(_deferred, "pending", None)
    call.view.no_heavy_queue = int(_heavy_queue_off(key))
    frac, tag = _slab_plan(key, _instance_guess(key), ((W + 15) // 16) * ((H + 15) // 16))
    if frac > 0.0 and lib.msgs_get_deterministic():
        frac = 0.0
    call.view.slab_fraction, call.view.feedback_tag = frac, tag
    with _on_device(dev):
        cur = torch.cuda.current_stream(dev)
        stream = C.c_void_p(cur.cuda_stream)
        radii = torch.empty(P, dtype=torch.int32, device=dev)
        pixel_sizes = torch.empty(P, dtype=torch.float32, device=dev)
        color = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        acc_ps = torch.empty(H, W, dtype=torch.float32, device=dev)
        depth = torch.empty(H, W, dtype=torch.float32, device=dev)
        alpha = torch.empty(H, W, dtype=torch.float32, device=dev) if want_alpha else None
        n_geom, n_s1, n_img = _sizes(P, W, H)
        guess = _instance_guess(key)
        # two allocations instead of five: what the backward needs again (geom | image | binning) and what dies with the
        # forward (stage-1 scratch | stage-2 scratch); every part starts on a 256-byte boundary
        n_bin = n_s2 = 0
        if guess is not None:
            cap = _capacity(guess)
            n_bin, n_s2 = _stage2_bytes(cap, W, H, frac)
        keep = _bytes(_a256(n_geom) + _a256(n_img) + n_bin, dev)
        geom, image = keep[:n_geom], keep[_a256(n_geom):_a256(n_geom) + n_img]
        binning = keep[_a256(n_geom) + _a256(n_img):] if n_bin else None
        if pending is not None:
            # launch only.  The stage-2 temporaries go back to the caching allocator at once, which hands them out again in
            # THIS stream's order only (blocks are bound to the stream they were allocated on).  The stage-1 scratch holds the
            # device copy of the status words that msgs_forward_finish may still READ at resolve time (MSGS_BLOCKING_SYNC=1, a
            # failed pinned allocation, or a flag that never landed: a copy enqueued behind whatever this stream was given
            # since) — it stays referenced by the pending state until resolve()
            scratch1 = _bytes(n_s1, dev)
            scratch2 = _bytes(n_s2, dev) if n_s2 else None
            status = _take_status()
            try:
                _C.check(lib.msgs_forward_launch(call.view_ref, call.g_ref, _ptr(radii), _ptr(pixel_sizes),
                                                 _ptr(geom), n_geom, _ptr(scratch1), n_s1,
                                                 _ptr(binning), n_bin, _ptr(scratch2), n_s2,
                                                 _ptr(image), n_img, _ptr(color), _ptr(acc_ps), _ptr(depth),
                                                 _ptr(grad_rec), grad_rec.numel() if grad_rec is not None else 0,
                                                 int(backward_follows), status, _C.timer_ptr(), stream), "msgs_forward_launch")
            except Exception:
                _give_status(status)
                raise
            state = _PendingForward(call, status, cur, key, guess, geom, binning, image, (color, acc_ps, depth), grad_rec, keep,
                                    backward_follows, scratch1, alpha)
            pending.append(state)
            if want_alpha:                    # valid in stream order like the other outputs (resolve() rewrites it behind a redo)
                _alpha_map(call, image, alpha, stream)
                return color, acc_ps, depth, radii, pixel_sizes, alpha, state
            return color, acc_ps, depth, radii, pixel_sizes, state
        tmp = _bytes(_a256(n_s1) + n_s2, dev)
        scratch1 = tmp[:n_s1]
        scratch2 = tmp[_a256(n_s1):] if n_s2 else None
        D, done = C.c_int64(0), C.c_int32(0)
        _C.check(lib.msgs_forward(call.view_ref, call.g_ref, _ptr(radii), _ptr(pixel_sizes),
                                  _ptr(geom), n_geom, _ptr(scratch1), n_s1,
                                  _ptr(binning), n_bin, _ptr(scratch2), n_s2,
                                  _ptr(image), n_img, _ptr(color), _ptr(acc_ps), _ptr(depth),
                                  _ptr(grad_rec), grad_rec.numel() if grad_rec is not None else 0, int(backward_follows),
                                  C.byref(D), C.byref(done), _C.timer_ptr(), stream), "msgs_forward")
        D = int(D.value)
        del scratch1, scratch2, tmp
        _note_count(key, D, guess, done.value)
        if not done.value:
            binning = _redo_stage2(call, geom, image, D, frac, (color, acc_ps, depth), grad_rec, backward_follows, stream)
        if want_alpha:
            _alpha_map(call, image, alpha, stream)
            return color, acc_ps, depth, radii, pixel_sizes, alpha, (geom, binning, image, D)
    return color, acc_ps, depth, radii, pixel_sizes, (geom, binning, image, D)


def _forward_tail(ctx, call, state, outs, geometry=(0, 1, 4, 5, 6)):
    """the end of every autograd forward: what its backward finds on ctx; returns the five outputs (six with return_alpha, and
    the distortion map, then median_depth and median_id, then the feature map behind them when asked for).  geometry: the positions of the inputs whose gradient the per-
    Gaussian backward forms from the records' geometry slots (the camera's follow from ctx.camera)."""
    color, acc_ps, depth, radii, pixel_sizes = outs[:5]
    ctx.call, ctx.state, ctx.radii = call, state, radii
    if ctx.distortion:
        outs = tuple(outs) + (_distortion_forward(ctx, call, state),)
    non_diff = (acc_ps, radii, pixel_sizes)
    if ctx.median:
        median_depth, median_id = _median_depth_forward(ctx, call, state)
        outs = tuple(outs) + (median_depth, median_id)
        non_diff += (median_id,)
    if ctx.features is not None:
        ctx.features_geom = any(ctx.needs_input_grad[k] for k in geometry) or any(m is not None for m in ctx.camera)
        outs = tuple(outs) + (_features_forward(ctx, call, state),)
    ctx.mark_non_differentiable(*non_diff)                      # depth and alpha are differentiable
    ctx.set_materialize_grads(False)      # grad_depth / grad_alpha are None unless the loss used that map: then today's path
    return tuple(outs)


def _backward_body(ctx, grad_color, grad_depth, grad_tail, destinations, after_main=None):
    """What every backward of the op runs, in the one order its launches take on the stream: the backward scratch, the entry's
    `destinations(ctx, call, scratch_is_clear) -> (_C.Grads, dest)` (where the leaf gradients go: fresh tensors, sinks, the
    accumulator or the Adam step; `dest` is whatever the entry wants back, kept alive across the launches), the camera outputs,
    the pre-passes of the opt-in maps the loss used — features, distortion, median depth, each adding to the gradient records and
    handing dL/ddepth and scratch_is_clear on — the main backward, the entry's `after_main(ctx, dest)`, dL/dbg, absgrad and the
    gradients of the trailing inputs.  Returns (dest, those gradients).  A further opt-in map is added HERE, once.
    (The two callbacks are plain functions, not closures made per call: this runs between the forward's host synchronisation
    and the backward's first launch, where host time shows in the step.)"""
    grad_alpha, grad_distortion, grad_median, grad_features = _split_grad_tail(ctx, grad_tail)
    _check_saved(ctx)
    call = ctx.call
    if grad_color is None:
        grad_color = torch.zeros(3, call.H, call.W, dtype=torch.float32, device=call.device)
    geom, binning, image, D = _resolve(ctx.state)
    dev, P = call.device, call.P
    with _on_device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        dL = _f32c(grad_color)
        dLd = _f32c(grad_depth) if grad_depth is not None else None
        dLa = _f32c(grad_alpha) if grad_alpha is not None else None
        scratch, is_clear = _take_backward_scratch(ctx, P, D, dev, dLd is not None or grad_distortion is not None or
                                                   grad_median is not None)
        grads, dest = destinations(ctx, call, is_clear)
        cam = _CameraGrads(ctx, P, dev) if ctx.camera else None
        dLd_loss = dLd                                          # (what the loss itself sent to the depth map: absgrad's input)
        if grad_features is not None:
            grads.scratch_is_clear = _features_backward(ctx, call, geom, binning, image, D, grad_features, scratch, is_clear,
                                                        dev, stream)
        if grad_distortion is not None:
            dLd, grads.scratch_is_clear = _distortion_backward(ctx, call, geom, binning, image, D, grad_distortion, dLd, scratch,
                                                               grads.scratch_is_clear, dev, stream)
        if grad_median is not None:
            dLd, grads.scratch_is_clear = _median_depth_backward(ctx, call, D, grad_median, dLd, scratch,
                                                                 grads.scratch_is_clear, dev, stream)
        _run_backward(_C.lib, call, ctx, geom, binning, image, D, dL, dLd, dLa, scratch, grads, stream, cam)
        if after_main is not None:
            after_main(ctx, dest)
        g_bg = _bg_grad(ctx, call.view_ref, image, dL, call.W, call.H, dev, stream) if ctx.bg is not None else None
        if ctx.absgrad is not None:
            _absgrad(ctx, call, geom, binning, image, D, dL, dLd_loss, dLa, dev, stream)
    return dest, _extra_grads(ctx, cam.grads(ctx) if cam is not None else (), g_bg)


def _fresh_destinations(ctx, call, is_clear):
    """_RasterizeGaussians.backward: fresh tensors, in the order of msgs_grads_t — means3D, means2D, sh, colours, opacity, scales,
    rotations, cov3D"""
    P, dev, f32 = call.P, call.device, torch.float32
    g = (torch.empty(P, 3, dtype=f32, device=dev), torch.empty(P, 3, dtype=f32, device=dev),
         torch.empty(P, call.K, 3, dtype=f32, device=dev) if call.sh is not None else None,
         torch.empty(P, 3, dtype=f32, device=dev) if call.colors is not None else None,
         torch.empty(P, dtype=f32, device=dev),
         torch.empty(P, 3, dtype=f32, device=dev) if call.scales is not None else None,
         torch.empty(P, 4, dtype=f32, device=dev) if call.rot is not None else None,
         torch.empty(P, 6, dtype=f32, device=dev) if call.cov is not None else None)
    return _C.Grads(*map(_ptr, g), None, None, None, is_clear), g


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                max_pixel_sizes, min_pixel_sizes, occ_multiplier, dc_delta, base_mask, raster_settings, *extra):
        camera, want_alpha = _note_extra(ctx, extra)
        if means3D.shape[0] == 0:
            # nothing to rasterize: background image, no native call (every per-Gaussian tensor is empty,
            # which upstream's convention cannot tell apart from "not provided")
            rs = raster_settings
            dev = means3D.device
            _hip_only(dev)
            H, W = int(rs.image_height), int(rs.image_width)
            color = rs.bg.to(dev, torch.float32).view(3, 1, 1).expand(3, H, W).contiguous()
            ctx.empty = True
            ctx.in_shapes = [t.shape for t in (means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                               cov3Ds_precomp)]
            ctx.dev = dev
            ctx.HW = (H, W, int(bool(rs.debug)))
            outs = (color, torch.zeros(H, W, device=dev), torch.zeros(H, W, device=dev),
                    torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, device=dev))
            non_diff = (outs[1],) + outs[3:]                    # (depth stays differentiable: zero gradients)
            # nothing blended, in the order of _forward_tail: alpha 0, no distortion pair, median depth 0 — [H,W] zeros — then
            # median id -1 and a zero feature map; zero gradients throughout
            extra = [torch.zeros(H, W, device=dev) for _ in range(int(want_alpha) + int(ctx.distortion) + int(ctx.median))]
            if ctx.median:
                extra.append(torch.full((H, W), -1, dtype=torch.int32, device=dev))
                non_diff += (extra[-1],)
            if ctx.features is not None:
                extra.append(torch.zeros(int(ctx.features.shape[1]), H, W, device=dev))
            ctx.mark_non_differentiable(*non_diff)
            ctx.set_materialize_grads(False)
            return outs + tuple(extra)
        ctx.empty = False
        call = _Call(raster_settings, means3D, _opt(sh), _opt(colors_precomp), opacities, _opt(scales),
                     _opt(rotations), _opt(cov3Ds_precomp), _opt(max_pixel_sizes), _opt(min_pixel_sizes),
                     _opt(occ_multiplier), _opt(dc_delta), _opt(base_mask))
        *outs, state = _forward_impl(call, _alloc_grad_records(ctx, call.P, call.device), ctx.backward_follows, want_alpha)
        ctx.shapes = (means2D.shape, opacities.shape)
        _save_inputs(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        return _forward_tail(ctx, call, state, outs, geometry=(0, 1, 4, 5, 6, 7))

    @staticmethod
    def backward(ctx, grad_color, grad_acc_ps, grad_depth, grad_radii, grad_pixel_sizes, *grad_tail):
        if ctx.empty:
            grad_features = _split_grad_tail(ctx, grad_tail)[3]
            cam = tuple(None if m is None else torch.zeros(m[0], dtype=m[1], device=m[2]) for m in ctx.camera)
            g_bg = None
            if ctx.bg is not None:          # the image is the background: dL/dbg_c = sum_p dL/dC_{c,p} (final_T = 1)
                H, W, debug = ctx.HW
                if grad_color is None:
                    grad_color = torch.zeros(3, H, W, dtype=torch.float32, device=ctx.dev)
                view = _C.View(H, W, 1.0, 1.0, 1.0, 1.0, 0, 0, 0, 0, 0, debug, 0, 0, 0.0, 0, None, None, None, None)
                with _on_device(ctx.dev):
                    stream = C.c_void_p(torch.cuda.current_stream(ctx.dev).cuda_stream)
                    g_bg = _bg_grad(ctx, C.byref(view), None, _f32c(grad_color), W, H, ctx.dev, stream)
            m2 = ctx.absgrad.means2D() if ctx.absgrad is not None else None
            if m2 is not None:              # no Gaussian: zeros [0, 3], no launch
                m2.absgrad = torch.zeros(ctx.in_shapes[1], dtype=torch.float32, device=ctx.dev)
            if grad_features is not None:
                ctx.g_features = torch.zeros(ctx.features.shape, dtype=torch.float32, device=ctx.dev)
            return tuple(torch.zeros(s, device=ctx.dev) for s in ctx.in_shapes) + (None,) * 6 + _extra_grads(ctx, cam, g_bg)
        g, g_extra = _backward_body(ctx, grad_color, grad_depth, grad_tail, _fresh_destinations)
        g_means3D, g_means2D, g_sh, g_col, g_opac, g_scales, g_rot, g_cov = g
        m2_shape, op_shape = ctx.shapes
        # occ_multiplier / dc_delta / pixel-size inputs / masks receive no gradient (DESIGN.md SPEC M5)
        return (g_means3D, g_means2D.view(m2_shape) if g_means2D.shape == m2_shape else g_means2D,
                g_sh, g_col, g_opac.view(op_shape), g_scales, g_rot, g_cov,
                None, None, None, None, None, None) + g_extra


# Gradient sinks (view-parallel training): a trainer that exchanges gradients through one flat bucket registers, per leaf
# parameter, the slice of the bucket its gradient belongs in.  The backward of the raw / chained entries then writes the
# gradient THERE and returns a fresh alias of that slice; with param.grad = None autograd adopts the alias as .grad (no
# copy), so neither a zero-fill of the bucket nor an accumulation pass over it is needed.  Keys: id() of the leaf tensor
# OBJECT, validated through a weak reference (an address-based key could match an unrelated tensor after densification
# re-allocates the parameters).
class _SinkRegistry(threading.local):
    """per host thread: set_grad_sinks and the forward that snapshots the sinks run on the training loop's thread; a second
    thread of the process (a viewer, an evaluation loop, another trainer) neither sees nor disturbs them"""

    def __init__(self):
        self.grad = {}
        self.sh_factor = [None, None]   # [destination tensor, optional torch.cuda.Event recorded once the factors are written]


_sinks = _SinkRegistry()


def _save_inputs(ctx, *tensors):
    """Everything the backward re-reads goes through save_for_backward, so that an in-place edit between forward and
    backward (optimizer step, reset_opacity-style edit) raises autograd's version-counter error instead of yielding
    silently wrong gradients.  (The ctypes structs on ctx.call point at the same storage.)"""
    tensors = tensors + (getattr(ctx, "features", None),)
    ctx.save_for_backward(*[t for t in tensors if torch.is_tensor(t) and t.numel() > 0])


def _check_saved(ctx):
    if not getattr(ctx, "empty", False):
        ctx.saved_tensors              # raises "modified by an inplace operation" when a version changed


def set_grad_sinks(mapping, sh_factor=None, factors_ready=None):
    """mapping: {leaf parameter: destination tensor (float32, contiguous, same numel)} or None to clear.
    sh_factor: optional [P,3] float32 destination.  When given, the backward of the raw / chained entries does NOT form
    the 48-float SH gradient rows: it writes this view's clamp-masked dL/drgb there (the SH gradient is the outer product
    basis(direction) x dL/drgb, rebuilt by sh_grad_from_views after the ranks have exchanged the factors) and returns
    None for features_dc / features_rest.  factors_ready: optional torch.cuda.Event (created BEFORE the call so that its
    handle exists); the library records it on the backward's stream right behind the kernel that writes the factors, ahead
    of the per-Gaussian backward — a side stream that waits on it can start exchanging the factors while that kernel runs."""
    _grad_sinks, _sh_factor_sink = _sinks.grad, _sinks.sh_factor
    _grad_sinks.clear()
    _sh_factor_sink[0] = None
    _sh_factor_sink[1] = None
    if sh_factor is not None:
        if sh_factor.dtype != torch.float32 or not sh_factor.is_contiguous() or sh_factor.dim() != 2 or sh_factor.shape[1] != 3:
            raise ValueError("sh_factor sink must be a contiguous float32 [P,3] tensor")
        _sh_factor_sink[0] = sh_factor
        _sh_factor_sink[1] = factors_ready
    if mapping:
        for leaf, dest in mapping.items():
            if dest.dtype != torch.float32 or not dest.is_contiguous() or dest.numel() != leaf.numel():
                raise ValueError("grad sink must be a contiguous float32 tensor with the parameter's numel")
            if dest.data_ptr() % 16:
                raise ValueError("grad sink must be 16-byte aligned (the backward stores float4 rows)")
            _grad_sinks[id(leaf)] = (weakref.ref(leaf), dest)


class GradAccumulator:
    """One gradient bucket for ALL views of an optimizer step (include/msgs.h, msgs_grads_t::accumulate).

    While installed (set_grad_accumulator), the backward of the raw / chained entries writes the leaf gradients straight into
    this object's tensors — the first view of a step stores every row, the later ones ADD their rendered rows inside the
    per-Gaussian kernel — and returns None for the leaves, so autograd runs no `param.grad += g` passes (six kernels and
    3 x 236 bytes per Gaussian and view at SH degree 3) and the kernel writes no zero rows for Gaussians a view did not
    render.  The sums are formed in the order of the backward calls, like autograd's: same bits.  Views may run on
    different streams: each backward waits for the previous one's kernel through an event.  finish() hands the bucket to
    the parameters' .grad (call it on the stream that will consume the gradients)."""

    def __init__(self, leaves, dest=None):
        """dest: optional destination tensors, one per leaf (e.g. the slices of a flat exchange bucket): used for every
        step instead of fresh allocations; float32, contiguous, 16-byte aligned, the leaf's numel."""
        self.leaves = list(leaves)
        for t in self.leaves:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device.type != "cuda":
                raise ValueError("GradAccumulator: leaves must be contiguous float32 tensors on a HIP device")
        self.fixed = None
        if dest is not None:
            dest = list(dest)
            if len(dest) != len(self.leaves):
                raise ValueError("GradAccumulator: one destination per leaf")
            for t, d in zip(self.leaves, dest):
                if d.dtype != torch.float32 or not d.is_contiguous() or d.numel() != t.numel() or d.device != t.device \
                        or d.data_ptr() % 16:
                    raise ValueError("GradAccumulator: a destination must be a contiguous, 16-byte aligned float32 tensor "
                                     "with its leaf's numel on the leaf's device")
            self.fixed = [d.view(t.shape) for t, d in zip(self.leaves, dest)]
        self.dest = None
        self.count = 0
        self.events = [torch.cuda.Event(), torch.cuda.Event()]
        for e in self.events:                       # torch creates the HIP event on the first record()
            e.record(torch.cuda.current_stream(self.leaves[0].device))
        self.last = None
        self.lock = threading.Lock()

    def begin_step(self):
        """fresh (uninitialised) tensors — or the caller's destinations: the first backward of the step writes every row"""
        self.dest = self.fixed if self.fixed is not None else [torch.empty_like(t) for t in self.leaves]
        self.count = 0
        self.last = None

    def _take(self, leaves):
        """(destinations in the order of `leaves`, accumulate flag, event to wait for or None, event to record)"""
        with self.lock:
            if self.dest is None:
                self.begin_step()
            by_id = {id(t): d for t, d in zip(self.leaves, self.dest)}
            try:
                dests = [by_id[id(t)] for t in leaves]
            except KeyError:
                raise ValueError("GradAccumulator: the call's parameters are not the tensors it was built for "
                                 "(densification re-creates them: build a new accumulator)") from None
            acc, wait = self.count > 0, self.last
            rec = self.events[self.count & 1]
            self.count += 1
            self.last = rec
            return dests, acc, wait, rec

    def finish(self):
        """param.grad = bucket (or += when a gradient is already there); the current stream waits for the last view"""
        if self.dest is None or self.count == 0:
            return
        if self.last is not None:
            torch.cuda.current_stream(self.leaves[0].device).wait_event(self.last)
        for t, d in zip(self.leaves, self.dest):
            if t.grad is None or t.grad.data_ptr() == d.data_ptr():
                t.grad = d
            else:
                t.grad += d
        self.dest = None
        self.count = 0
        self.last = None


_accumulator = threading.local()


def set_grad_accumulator(acc):
    """Install (or, with None, remove) the GradAccumulator the following forwards of the raw / chained entries OF THIS THREAD
    snapshot (the forward runs on the caller's thread; the backward finds the accumulator on its ctx).  Returns the previous one."""
    prev = getattr(_accumulator, "acc", None)
    _accumulator.acc = acc
    return prev


_step_in_backward = threading.local()


def set_optimizer_in_backward(optimizer):
    """Install (or, with None, remove) the optimizer whose step the following forwards of the RAW entry OF THIS THREAD hand to
    their backward (include/msgs.h, msgs_adam_in_backward_t): the per-Gaussian backward kernel then applies the Adam update to
    the six leaf tensors and their moments itself, where it forms their gradients — the 236 bytes of gradient per Gaussian are
    neither written nor read back, the leaves receive no .grad — and `optimizer.take_step_in_backward(leaves)` is called once
    per backward to deliver the table, `optimizer.commit_step_in_backward(leaves)` behind the launch to advance the step
    counters (train_epilogue.FusedAdam implements both).  One view per
    optimizer step, as in the reference's loop (/root/reference/train.py:203-216, :416-418); not with a GradAccumulator or the
    factored SH gradient.  Bit-identical parameters and moments to backward + FusedAdam.step() (tests/test_train_step_gpu.py).
    Returns the previous one."""
    prev = getattr(_step_in_backward, "opt", None)
    _step_in_backward.opt = optimizer
    return prev


def _snapshot_sinks(ctx, leaves):
    """Called in forward (the caller's thread): the sinks registered for THIS call travel on its ctx, so that the
    backward — which runs on autograd's worker thread — never reads module state another thread may be changing."""
    ctx.sinks = tuple(_sinks.grad.get(id(t)) for t in leaves)
    ctx.sh_factor = (_sinks.sh_factor[0], _sinks.sh_factor[1])
    ctx.accum = getattr(_accumulator, "acc", None)
    ctx.step_opt = getattr(_step_in_backward, "opt", None)
    ctx.leaves = leaves if (ctx.accum is not None or ctx.step_opt is not None) else None


def _grad_out(hit, shape, dev):
    if hit is not None and hit[0]() is not None and hit[1].device == dev:
        return hit[1].view(shape)                   # a NEW alias: autograd may adopt it as param.grad
    return torch.empty(shape, dtype=torch.float32, device=dev)


def _leaf_destinations(ctx, call, is_clear):
    """_RasterizeGaussiansRaw.backward: where the six leaf gradients go — consumed by the Adam step, into the accumulator, or
    into sinks / fresh tensors.  dest = (dL/dmeans2D, the six gradients autograd is handed (None where they live in the
    accumulator or were consumed by the step), the Adam table or None)"""
    dev, P = call.device, call.P
    dc_shape, rest_shape, op_shape = ctx.shapes[1:]
    g_m2 = torch.empty(P, 3, dtype=torch.float32, device=dev)
    factor, ready = ctx.sh_factor
    if factor is not None and (factor.device != dev or factor.shape[0] != P):
        raise ValueError("sh_factor sink does not match this model (device / number of Gaussians)")
    accum = getattr(ctx, "accum", None)
    step_opt = getattr(ctx, "step_opt", None)
    acc_flag, ev_wait, ev_rec = 0, None, None
    adam = g_xyz = g_dc = g_rest = g_opac = g_scal = g_rot = None
    if step_opt is not None:
        if accum is not None or factor is not None:
            raise ValueError("set_optimizer_in_backward cannot be combined with a GradAccumulator or the factored SH gradient")
        if call.view.sh_coeffs != 16:
            raise ValueError("set_optimizer_in_backward needs 16 SH coefficients per Gaussian")
        adam = step_opt.take_step_in_backward(ctx.leaves)        # (a _C.AdamInBackward; keeps its tensors alive itself)
    elif accum is not None:
        if factor is not None:
            raise ValueError("GradAccumulator and the factored SH gradient cannot be combined")
        (g_xyz, g_dc, g_rest, g_opac, g_scal, g_rot), acc, wait, rec = accum._take(ctx.leaves)
        acc_flag = 1 if acc else 0
        ev_wait = C.c_void_p(wait.cuda_event) if wait is not None else None
        ev_rec = C.c_void_p(rec.cuda_event)
    else:
        kx, kdc, krest, kop, ksc, krot = ctx.sinks
        g_xyz = _grad_out(kx, (P, 3), dev)
        if factor is None:
            g_dc, g_rest = _grad_out(kdc, dc_shape, dev), _grad_out(krest, rest_shape, dev)
        g_opac, g_scal, g_rot = _grad_out(kop, op_shape, dev), _grad_out(ksc, (P, 3), dev), _grad_out(krot, (P, 4), dev)
    grads = _C.Grads(_ptr(g_xyz), _ptr(g_m2), None, _ptr(factor), _ptr(g_opac), _ptr(g_scal), _ptr(g_rot), None,
                     _ptr(g_dc), _ptr(g_rest),
                     C.c_void_p(ready.cuda_event) if (factor is not None and ready is not None) else None,
                     is_clear, acc_flag, ev_wait, ev_rec, C.addressof(adam) if adam is not None else None)
    if accum is not None or adam is not None:
        return grads, (g_m2, (None,) * 6, adam)
    return grads, (g_m2, (g_xyz, g_dc, g_rest, g_opac, g_scal, g_rot), None)


def _commit_step(ctx, dest):
    """behind the main backward of the raw entry: the kernel that takes the Adam step has been launched"""
    if dest[2] is not None:
        ctx.step_opt.commit_step_in_backward(ctx.leaves)


class _RasterizeGaussiansRaw(torch.autograd.Function):
    """Opt-in fused entry: takes the RAW GaussianModel parameters
    (/root/reference/scene/gaussian_model.py:53-58: _xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation);
    exp / sigmoid / normalize (:39-47) and the dc|rest concatenation (:144-149) run inside the HIP kernels and the
    backward returns gradients w.r.t. the raw parameters.  Same five outputs as the reference op."""

    @staticmethod
    def forward(ctx, xyz, means2D, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw,
                max_pixel_sizes, min_pixel_sizes, occ_multiplier, dc_delta, base_mask, raster_settings, *extra):
        if xyz.shape[0] == 0:
            raise ValueError("rasterize_gaussians_raw: empty model")
        camera, want_alpha = _note_extra(ctx, extra)
        _refuse_camera_with(camera)
        call = _Call(raster_settings, xyz, None, None, opacity_raw, scaling_raw, rotation_raw, None,
                     _opt(max_pixel_sizes), _opt(min_pixel_sizes), _opt(occ_multiplier), _opt(dc_delta),
                     _opt(base_mask), raw_features=(features_dc, features_rest))
        *outs, state = _forward_impl(call, _alloc_grad_records(ctx, call.P, call.device), ctx.backward_follows, want_alpha)
        ctx.shapes = (means2D.shape, features_dc.shape, features_rest.shape, opacity_raw.shape)
        _snapshot_sinks(ctx, (xyz, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw))
        _save_inputs(ctx, xyz, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw)
        return _forward_tail(ctx, call, state, outs)

    @staticmethod
    def backward(ctx, grad_color, grad_acc_ps, grad_depth, grad_radii, grad_pixel_sizes, *grad_tail):
        (g_m2, leaf, _), g_extra = _backward_body(ctx, grad_color, grad_depth, grad_tail, _leaf_destinations, _commit_step)
        return (leaf[0], g_m2.view(ctx.shapes[0])) + leaf[1:] + (None, None, None, None, None, None) + g_extra


class _RasterizeGaussiansChained(torch.autograd.Function):
    """The reference-API call whose inputs are recognised as the reference's own getters applied to leaf parameters
    (see _match_reference_getters).  Forward: exactly the reference-API forward on the activated tensors (bit-identical
    outputs).  Backward: msgs_backward applies the chain rule of sigmoid / exp / normalize / cat itself and the gradients
    go straight to the leaf parameters, instead of autograd running the getters' backward kernels afterwards (at 1 M
    Gaussians: two strided 190 MB copies for the cat and ~15 small kernels)."""

    @staticmethod
    def forward(ctx, xyz, means2D, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw,
                shs, opacities, scales, rotations, max_pixel_sizes, min_pixel_sizes, occ_multiplier, dc_delta, base_mask,
                raster_settings, *extra):
        camera, want_alpha = _note_extra(ctx, extra)
        _refuse_camera_with(camera)
        call = _Call(raster_settings, xyz, _opt(shs), None, opacities, scales, rotations, None,
                     _opt(max_pixel_sizes), _opt(min_pixel_sizes), _opt(occ_multiplier), _opt(dc_delta),
                     _opt(base_mask), raw_features=(features_dc, features_rest), rotations_raw=rotation_raw)
        *outs, state = _forward_impl(call, _alloc_grad_records(ctx, call.P, call.device), ctx.backward_follows, want_alpha)
        ctx.shapes = (means2D.shape, features_dc.shape, features_rest.shape, opacity_raw.shape)
        _snapshot_sinks(ctx, (xyz, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw))
        _save_inputs(ctx, xyz, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw, shs, opacities,
                     scales, rotations)
        return _forward_tail(ctx, call, state, outs)

    @staticmethod
    def backward(ctx, grad_color, grad_acc_ps, grad_depth, grad_radii, grad_pixel_sizes, *grad_tail):
        g = _RasterizeGaussiansRaw.backward(ctx, grad_color, grad_acc_ps, grad_depth, grad_radii, grad_pixel_sizes, *grad_tail)
        return g[:7] + (None,) * 10 + g[13:]            # (the trailing inputs' gradients — camera, bg, markers, features — at the end)


# Recognition of the reference's getters (scene/gaussian_model.py:127-153) in the autograd graph of the arguments of
# GaussianRasterizer.forward.  Module-level switch; MSGS_NO_GETTER_CHAIN=1 in the environment turns it off.
chain_reference_getters = os.environ.get("MSGS_NO_GETTER_CHAIN", "0") != "1"
# the chained kernels read the SH rows from the concatenated tensor the reference built (aligned rows, visible ones
# only: K1 111 -> 89 us, K9 141 -> 126 us at C3) at the price of keeping that [P,16,3] tensor alive until backward
_chain_reads_cat = os.environ.get("MSGS_CHAIN_SPLIT_READS", "0") != "1"


_warned_chain = [False]


def _leaf(fn):
    return fn.variable if fn is not None and type(fn).__name__ == "AccumulateGrad" else None


def _match_reference_getters(means3D, sh, opacities, scales, rotations):
    """(features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw) when the four tensors are, provably from
    their grad_fn chains,  cat((dc, rest), dim=1), sigmoid(leaf), exp(leaf) and F.normalize(leaf)  of float32 CUDA leaf
    tensors with the reference's shapes; None otherwise (then autograd handles everything as usual)."""
    try:
        P = means3D.shape[0]
        f = sh.grad_fn
        if type(f).__name__ != "CatBackward0" or f._saved_dim != 1 or len(f.next_functions) != 2:
            return None
        dc, rest = _leaf(f.next_functions[0][0]), _leaf(f.next_functions[1][0])
        f = opacities.grad_fn
        if type(f).__name__ != "SigmoidBackward0":
            return None
        op = _leaf(f.next_functions[0][0])
        f = scales.grad_fn
        if type(f).__name__ != "ExpBackward0":
            return None
        sc = _leaf(f.next_functions[0][0])
        # F.normalize: x / x.norm(2, 1, keepdim=True).clamp_min(1e-12).expand_as(x)
        f = rotations.grad_fn
        if type(f).__name__ != "DivBackward0":
            return None
        rot = _leaf(f.next_functions[0][0])
        e = f.next_functions[1][0]
        if type(e).__name__ != "ExpandBackward0":
            return None
        c = e.next_functions[0][0]
        if type(c).__name__ != "ClampMinBackward0" or float(c._saved_min) != 1e-12:
            return None
        n = c.next_functions[0][0]
        if type(n).__name__ != "LinalgVectorNormBackward0" or float(n._saved_ord) != 2.0 or \
                tuple(n._saved_dim) != (1,) or not n._saved_keepdim or _leaf(n.next_functions[0][0]) is not rot:
            return None
        leaves = (dc, rest, op, sc, rot)
        want = ((P, 1, 3), (P, 15, 3), (P, 1), (P, 3), (P, 4))
        for t, shape in zip(leaves, want):
            if t is None or tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() \
                    or t.device != means3D.device or not t.requires_grad:
                return None
        if tuple(sh.shape) != (P, 16, 3) or tuple(opacities.shape) != (P, 1):
            return None
        return leaves
    except (AttributeError, IndexError, TypeError):
        return None


def sh_grad_from_views(means3D, gathered, n_views, sh_degree, scale, out_dc, out_rest):
    """out_dc [P,1,3], out_rest [P,15,3] = scale * sum_v basis(normalize(means3D - campos_v)) x drgb_v
    (include/msgs.h msgs_sh_grad_from_views): the SH gradient of n_views views rebuilt from their factors.
    `gathered` is the all-gathered exchange buffer [n_views, 3P + 4]: row v = {drgb_v [P,3] | campos_v [3] | pad}."""
    P = int(means3D.shape[0])
    dev = means3D.device
    if dev.type != "cuda":
        raise RuntimeError("sh_grad_from_views: tensors must live on a HIP device (no CPU path)")
    row = 3 * P + 4
    for t, name, numel in ((means3D, "means3D", 3 * P), (gathered, "gathered", n_views * row), (out_dc, "out_dc", 3 * P),
                           (out_rest, "out_rest", 45 * P)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel or t.device != dev:
            raise ValueError(f"sh_grad_from_views: {name} must be a contiguous float32 tensor of {numel} elements on {dev}")
    base = gathered.data_ptr()
    _launch(None, "msgs_sh_grad_from_views", dev, P, int(n_views), int(sh_degree), _ptr(means3D), C.c_void_p(base + 4 * 3 * P), row,
            C.c_void_p(base), row, float(scale), _ptr(out_dc), _ptr(out_rest))
    return out_dc, out_rest


def rasterize_gaussians_raw(xyz, means2D, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw,
                            max_pixel_sizes, min_pixel_sizes, occ_multiplier, dc_delta, base_mask, raster_settings,
                            features=None, return_median_depth=False, return_distortion=False, absgrad=False,
                            return_alpha=False):
    """return_alpha=True: a sixth output, the alpha map [H,W] (1 - final transmittance), differentiable
    absgrad=True: every backward also assigns means2D.absgrad.
    features [P,C]: one more output at the END, the feature map [C,H,W], differentiable.
    return_distortion=True: one more output behind alpha and in front of the feature map, the depth-distortion map [H,W],
    differentiable.
    return_median_depth=True: two more outputs behind the distortion map and in front of the feature map, median_depth [H,W]
    float32 (differentiable w.r.t. the means and the camera) and median_id [H,W] int32.  All five by
    keyword."""
    extra = _extra_inputs(raster_settings, return_alpha, absgrad, means2D, features, xyz, return_distortion,
                          return_median_depth)
    _note_grad_mode()
    return _RasterizeGaussiansRaw.apply(xyz, means2D, features_dc, features_rest, opacity_raw, scaling_raw,
                                        rotation_raw, max_pixel_sizes, min_pixel_sizes, occ_multiplier, dc_delta,
                                        base_mask, raster_settings,
                                        *extra)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        max_pixel_sizes, min_pixel_sizes, occ_multiplier, dc_delta, base_mask, raster_settings,
                        features=None, return_median_depth=False, return_distortion=False, absgrad=False,
                        return_alpha=False):
    extra = _extra_inputs(raster_settings, return_alpha, absgrad, means2D, features, means3D, return_distortion,
                          return_median_depth)
    _note_grad_mode()
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, max_pixel_sizes, min_pixel_sizes, occ_multiplier, dc_delta,
                                     base_mask, raster_settings,
                                     *extra)


rasterize_gaussians.__doc__ = rasterize_gaussians_raw.__doc__         # the same five keywords, the same outputs


# Antialiasing (4.14): the opacity compensation of Mip-Splatting's 2-D screen filter as a pre-pass.  An
# antialiased render is the plain render of the same model with o_eff = o rho in the place of the opacity; the rasterizer, its
# backward and every opt-in output only ever see an opacity tensor.
_compensation_probe = None         # tests: a callable (name) run in front of every msgs_screen_compensation_* call


class _ScreenCompensation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, opacities, scales, rotations, cov3D_precomp, viewmatrix, raster_settings):
        P, dev = int(means3D.shape[0]), means3D.device
        ctx.shapes = tuple(None if t is None else t.shape for t in (means3D, opacities, scales, rotations, cov3D_precomp))
        ctx.vm = None if viewmatrix is None or not ctx.needs_input_grad[5] else (viewmatrix.shape, viewmatrix.dtype,
                                                                                 viewmatrix.device)
        ctx.dev = dev
        ctx.empty = P == 0
        if P == 0:
            _hip_only(dev)
            return torch.zeros(opacities.shape, dtype=torch.float32, device=dev)
        call = _Call(raster_settings, means3D, None, None, opacities, scales, rotations, cov3D_precomp, None, None, None, None,
                     None)
        o_eff = torch.empty(P, dtype=torch.float32, device=dev)
        _launch(_compensation_probe, "msgs_screen_compensation_forward", dev, call.view_ref, call.g_ref, _ptr(o_eff))
        ctx.call = call
        ctx.features = None
        _save_inputs(ctx, means3D, opacities, scales, rotations, cov3D_precomp, viewmatrix)
        return o_eff.view(opacities.shape)

    @staticmethod
    def backward(ctx, grad_o_eff):
        dev = ctx.dev
        zeros = lambda s: None if s is None else torch.zeros(s, dtype=torch.float32, device=dev)
        g_vm = None
        if ctx.empty or grad_o_eff is None:
            if ctx.vm is not None:
                g_vm = torch.zeros(ctx.vm[0], dtype=ctx.vm[1], device=ctx.vm[2])
            return tuple(zeros(s) for s in ctx.shapes) + (g_vm, None)
        _check_saved(ctx)
        call = ctx.call
        P = call.P
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        g_opac, g_means = new(P), new(P, 3)
        g_scales = new(P, 3) if call.scales is not None else None
        g_rot = new(P, 4) if call.rot is not None else None
        g_cov = new(P, 6) if call.cov is not None else None
        dV = new(16) if ctx.vm is not None else None
        scratch = _bytes(_C.lib.msgs_screen_compensation_scratch_bytes(P), dev) if dV is not None else None
        g = _f32c(grad_o_eff).reshape(-1)
        _launch(_compensation_probe, "msgs_screen_compensation_backward", dev, call.view_ref, call.g_ref, _ptr(g), _ptr(g_opac),
                _ptr(g_means), _ptr(g_scales), _ptr(g_rot), _ptr(g_cov), _ptr(dV), _ptr(scratch),
                scratch.numel() if scratch is not None else 0)
        if dV is not None:
            g_vm = dV.view(ctx.vm[0]).to(device=ctx.vm[2], dtype=ctx.vm[1])
        sh = ctx.shapes
        return (g_means.view(sh[0]), g_opac.view(sh[1]), None if g_scales is None else g_scales.view(sh[2]),
                None if g_rot is None else g_rot.view(sh[3]), None if g_cov is None else g_cov.view(sh[4]), g_vm, None)


def screen_compensation(means3D, opacities, raster_settings, scales=None, rotations=None, cov3D_precomp=None):
    """o_eff = opacities * rho, in opacities' shape (float32): the opacity compensation of the antialiasing filter of
    Mip-Splatting (upstream 3DGS's antialiasing=True, gsplat's rasterize_mode="antialiased") for the view of `raster_settings`:
        rho = sqrt(max(0.000025, det0 / det1)),   det0 = a0 c0 - b^2,   det1 = (a0 + 0.3)(c0 + 0.3) - b^2
    with (a0, b, c0) the projected 2-D covariance before the rasterizer's +0.3 dilation, the float32 values the rasterizer forms
    itself.  Rendering the same model with o_eff in the place of its opacities IS the antialiased render
    (GaussianRasterizer.with_antialiasing() does just that); a Gaussian smaller than a pixel is dimmed by the factor the dilation
    spreads it out.  rho is 1 exactly for a Gaussian behind the near plane (view depth <= 0.2) or with non-finite inputs.
    Differentiable in opacities, means3D, scales + rotations or cov3D_precomp (exactly one of the two, the rasterizer's rule)
    and, when it requires grad, raster_settings.viewmatrix; projmatrix, campos and bg do not enter.  Two HIP kernels beside
    the rasterizer's own; activated inputs only."""
    if means3D.shape[0] > 0:        # (no Gaussian: every tensor is empty, which upstream's convention reads as "not provided")
        scales, rotations, cov3D_precomp = _opt(scales), _opt(rotations), _opt(cov3D_precomp)
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
    vm = raster_settings.viewmatrix
    vm = vm if torch.is_grad_enabled() and torch.is_tensor(vm) and vm.requires_grad else None
    return _ScreenCompensation.apply(means3D, opacities, scales, rotations, cov3D_precomp, vm, raster_settings)


# 3-D smoothing filter (4.17): the other half of Mip-Splatting.  Every Gaussian is bounded from below in size
# by the highest sampling rate at which any training camera sees it; a filtered render is the plain render of the same model with
# (s_eff, o_eff) in the place of the scales and the opacity, so the rasterizer and every opt-in output only see two tensors.
FILTER3D_CAMERA_CHUNK = _C.FILTER3D_CAMERA_CHUNK
_filter3d_probe = None             # tests: a callable (name) run in front of every msgs_filter3d_* / msgs_smoothing_filter_* call


def _camera_table(cameras, device=None):
    """[V, 20] float32: world_view_transform (16, the layout the rasterizer's viewmatrix has), fx, fy, W, H.  The matrices are
    stacked where they live and the focal lengths are formed in double on the host: cameras on the host give a host table that
    travels in one transfer, cameras already on `device` only send their [V, 4] intrinsics.  device=None: the host table."""
    import math
    mats, intr = [], []
    for cam in cameras:
        M = cam.world_view_transform
        if not torch.is_tensor(M):
            M = torch.as_tensor(M, dtype=torch.float32)
        if M.shape != (4, 4):
            raise ValueError("compute_3d_filter: world_view_transform must be [4,4]")
        mats.append(M)
        W, H = float(cam.image_width), float(cam.image_height)
        intr.append((W / (2.0 * math.tan(0.5 * float(cam.FoVx))), H / (2.0 * math.tan(0.5 * float(cam.FoVy))), W, H))
    if not mats:
        raise ValueError("compute_3d_filter: at least one camera is needed")
    if len({m.device for m in mats}) > 1:
        mats = [m.cpu() for m in mats]
    M = torch.stack(mats).detach().float().reshape(len(mats), 16)
    intr = torch.tensor(intr, dtype=torch.float64).float()
    if device is None or M.device.type == "cpu":
        table = torch.cat([M.cpu(), intr], dim=1).contiguous()
        return table if device is None else table.to(device)
    return torch.cat([M.to(device), intr.to(device)], dim=1).contiguous()


@torch.no_grad()
def compute_3d_filter(means3D, cameras, rule="per_camera", variance=0.2):
    """(filter_3D [P,1] float32, valid_points [P] bool) of Mip-Splatting's 3-D smoothing filter for the centres `means3D` and the
    camera set `cameras` (any sequence of objects with world_view_transform, FoVx, FoVy, image_width, image_height).  Camera n
    sees a centre iff its view depth t.z exceeds 0.2 and its projection lies within 15 % of the image around it;
        rule="per_camera":     nu = max over the seeing cameras of fx_n / t.z      (the paper; right for mixed focal lengths)
        rule="mip_splatting":  nu = (max fx over ALL cameras) / (min t.z over the seeing cameras)      (the published code)
    and filter_3D = sqrt(variance) / nu.  valid_points tells which centres some camera sees; the others take the largest filter
    of those (the published code's distance[~valid].max()); if none is seen the filter is 0 everywhere, which smoothing_filter()
    reads as the identity.  One sweep kernel over the whole set (the camera table travels in one copy) on the current stream,
    without a host read-back; the same bits on every run.  Carries no gradient.  Recompute it whenever the model's rows change
    (after every densification) and, as Mip-Splatting does, every 100 iterations."""
    if rule not in _C.FILTER3D_RULES:
        raise ValueError(f"compute_3d_filter: rule must be one of {sorted(_C.FILTER3D_RULES)}, not {rule!r}")
    if not float(variance) > 0.0:
        raise ValueError("compute_3d_filter: variance must be positive")
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise ValueError("compute_3d_filter: means3D must be [P,3]")
    cameras = list(cameras)
    if not cameras:
        raise ValueError("compute_3d_filter: at least one camera is needed")
    dev = means3D.device
    _hip_only(dev)
    P, V = int(means3D.shape[0]), len(cameras)
    filt = torch.empty(P, 1, dtype=torch.float32, device=dev)
    valid = torch.empty(P, dtype=torch.bool, device=dev)
    if P == 0:
        return filt, valid
    means = _f32c(means3D.detach())
    cams = _camera_table(cameras, dev)
    scratch = _bytes(_C.lib.msgs_filter3d_scratch_bytes(P, V), dev)
    _launch(_filter3d_probe, "msgs_filter3d_sweep", dev, P, _ptr(means), V, _ptr(cams), _C.FILTER3D_RULES[rule], float(variance),
            _ptr(filt), _ptr(valid), _ptr(scratch), scratch.numel())
    return filt, valid


def _check_filter_rows(scales, opacities, filter_3D):
    P = int(scales.shape[0])
    if scales.dim() != 2 or scales.shape[1] != 3:
        raise ValueError("smoothing_filter: scales must be [P,3]")
    if opacities.numel() != P or filter_3D.numel() != P:
        raise ValueError(f"smoothing_filter: {P} rows of scales, {opacities.numel()} opacities and {filter_3D.numel()} rows of "
                         "filter_3D — a filter computed before a densification is stale: run compute_3d_filter again")
    return P


class _SmoothingFilter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scales, opacities, filter_3D, raw):
        P, dev = int(scales.shape[0]), scales.device
        _hip_only(dev)
        ctx.shapes, ctx.raw, ctx.P, ctx.dev = (scales.shape, opacities.shape), bool(raw), P, dev
        s_eff = torch.empty(P, 3, dtype=torch.float32, device=dev)
        o_eff = torch.empty(opacities.shape, dtype=torch.float32, device=dev)
        if P == 0:
            return s_eff, o_eff
        s, o, f = _f32c(scales.detach()), _f32c(opacities.detach()), _f32c(filter_3D.detach())
        _launch(_filter3d_probe, "msgs_smoothing_filter_forward", dev, P, int(ctx.raw), _ptr(s), _ptr(o), _ptr(f), _ptr(s_eff),
                _ptr(o_eff))
        ctx.save_for_backward(s, o, f)
        return s_eff, o_eff

    @staticmethod
    def backward(ctx, g_s_eff, g_o_eff):
        P, dev = ctx.P, ctx.dev
        new = torch.zeros if P == 0 or (g_s_eff is None and g_o_eff is None) else torch.empty   # (the kernel writes every row)
        g_s = new(ctx.shapes[0], dtype=torch.float32, device=dev)
        g_o = new(ctx.shapes[1], dtype=torch.float32, device=dev)
        if new is torch.zeros:
            return g_s, g_o, None, None
        s, o, f = ctx.saved_tensors
        gs = None if g_s_eff is None else _f32c(g_s_eff)
        go = None if g_o_eff is None else _f32c(g_o_eff)
        _launch(_filter3d_probe, "msgs_smoothing_filter_backward", dev, P, int(ctx.raw), _ptr(s), _ptr(o), _ptr(f), _ptr(gs),
                _ptr(go), _ptr(g_s), _ptr(g_o))
        return g_s, g_o, None, None


def smoothing_filter(scales, opacities, filter_3D, raw=False):
    """(scales_eff [P,3], opacities_eff in opacities' shape), float32: the model's getters under the 3-D smoothing filter
    f = filter_3D [P,1] (compute_3d_filter),
        s_eff_k = sqrt(s_k^2 + f^2),     o_eff = o r_0 r_1 r_2,   r_k = s_k / s_eff_k     (= o sqrt(det S^2 / det(S^2 + f^2 I)))
    Rendering the same model with them in the place of its scales and opacities IS the filtered render.  A row with f == 0 is
    passed through bit for bit; s_k == 0 under f > 0 gives s_eff_k = f, o_eff = 0 and finite gradients.  raw=True takes the
    LEAVES — log-scales and opacity logits — and applies exp and sigmoid inside the kernel, with the rasterizer's own
    expressions; the gradients then land on the leaves and the exp / sigmoid nodes leave autograd.  Differentiable in scales and
    opacities, not in filter_3D.  One streaming HIP kernel forward and one backward.  ValueError when the row counts differ."""
    _check_filter_rows(scales, opacities, filter_3D)
    if filter_3D.requires_grad:
        filter_3D = filter_3D.detach()
    s_eff, o_eff = _SmoothingFilter.apply(scales, opacities, filter_3D, bool(raw))
    # not the reference's getters: the rasterizer skips the chained mode for them without its warning
    s_eff._msgs_filtered = o_eff._msgs_filtered = True
    return s_eff, o_eff


# Normal maps (4.18): the two halves of a depth-normal consistency loss.  gaussian_normals() gives every
# Gaussian the normal that with_features() splats; depth_to_normal() turns a depth map into the normals of the surface it
# describes.  Both are small streaming kernels outside the rasterizer.
DEPTH_NORMAL_TILE_W, DEPTH_NORMAL_TILE_H = _C.DEPTH_NORMAL_TILE_W, _C.DEPTH_NORMAL_TILE_H
_normals_probe = None              # tests: a callable (name) run in front of every msgs_gaussian_normals_* / msgs_depth_normal_* call


def _camera_constant(t, n, dev, name):
    """viewmatrix / campos of the settings as `n` contiguous float32 on `dev`, detached: constants of both functions"""
    t = torch.as_tensor(t).detach()
    if t.numel() != n:
        raise ValueError(f"{name} must have {n} elements, got {tuple(t.shape)}")
    return _f32c(t.to(dev)).reshape(-1)


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, scales, rotations, viewmatrix, campos, world):
        P, dev = int(means3D.shape[0]), means3D.device
        _hip_only(dev)
        ctx.P, ctx.dev, ctx.world, ctx.shape = P, dev, bool(world), rotations.shape
        normals = torch.empty(P, 3, dtype=torch.float32, device=dev)
        if P == 0:
            return normals
        m, s, r = _f32c(means3D.detach()), _f32c(scales.detach()), _f32c(rotations.detach())
        vm, cp = _camera_constant(viewmatrix, 16, dev, "viewmatrix"), _camera_constant(campos, 3, dev, "campos")
        flags = torch.empty(P, dtype=torch.uint8, device=dev)
        _launch(_normals_probe, "msgs_gaussian_normals_forward", dev, P, _ptr(m), _ptr(s), _ptr(r), _ptr(vm), _ptr(cp),
                int(ctx.world), _ptr(normals), _ptr(flags))
        ctx.save_for_backward(r, flags, vm)
        return normals

    @staticmethod
    def backward(ctx, g_normals):
        P, dev = ctx.P, ctx.dev
        if P == 0 or g_normals is None:
            return None, None, torch.zeros(ctx.shape, dtype=torch.float32, device=dev), None, None, None
        r, flags, vm = ctx.saved_tensors
        g = _f32c(g_normals)
        g_rot = torch.empty(P, 4, dtype=torch.float32, device=dev)
        _launch(_normals_probe, "msgs_gaussian_normals_backward", dev, P, _ptr(r), _ptr(flags), _ptr(vm), int(ctx.world), _ptr(g),
                _ptr(g_rot))
        return None, None, g_rot.view(ctx.shape), None, None, None


def gaussian_normals(means3D, scales, rotations, raster_settings, world=False):
    """normals [P,3] float32: the shortest axis of every Gaussian, turned towards the camera of `raster_settings` — what
    2DGS / GOF / PGSR splat as rend_normal (feed it to GaussianRasterizer.with_features()).
        k = 0; if s_1 < s_k: k = 1; if s_2 < s_k: k = 2        (strict: ties go to the lowest index)
        q = r / max(||r||, 1e-12),  n = column k of R(q)       (the R of Sigma = R S^2 R^T)
        sigma = -1 iff n . (campos - p) < 0, else +1
    world=True returns sigma n; by default the vector is rotated into view space with the 3x3 block of viewmatrix, the space
    depth_to_normal() works in.  `scales` only enter the comparison, so log-scales, activated scales and smoothing_filter()ed
    scales select the same axis, and `rotations` are normalised here (harmless on the model's getter): the leaves may be passed
    as they are.  A row with a non-finite input or result is exactly (0, 0, 0) and has no gradient.  Differentiable in
    `rotations` only — through column k of R and the normalisation; the selection, the sign and the camera are constants, and
    means3D / scales receive nothing.  One streaming HIP kernel forward and one backward.  float64 and
    strided inputs are converted; ValueError when the row counts differ."""
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise ValueError("gaussian_normals: means3D must be [P,3]")
    P = int(means3D.shape[0])
    if scales.dim() != 2 or tuple(scales.shape) != (P, 3):
        raise ValueError(f"gaussian_normals: scales must be [{P},3], got {tuple(scales.shape)}")
    if rotations.dim() != 2 or tuple(rotations.shape) != (P, 4):
        raise ValueError(f"gaussian_normals: rotations must be [{P},4], got {tuple(rotations.shape)}")
    return _GaussianNormals.apply(means3D, scales, rotations, raster_settings.viewmatrix, raster_settings.campos, bool(world))


class _DepthToNormal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, viewmatrix, W, H, tanfovx, tanfovy, world):
        dev = depth.device
        _hip_only(dev)
        ctx.dev, ctx.world, ctx.geometry, ctx.shape = dev, bool(world), (W, H, float(tanfovx), float(tanfovy)), depth.shape
        normal = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        if W * H == 0:
            return normal
        z = _f32c(depth.detach())
        vm = _camera_constant(viewmatrix, 16, dev, "viewmatrix") if world else None
        _launch(_normals_probe, "msgs_depth_normal_forward", dev, W, H, ctx.geometry[2], ctx.geometry[3], _ptr(z), _ptr(vm),
                int(ctx.world), _ptr(normal))
        ctx.save_for_backward(z, *(() if vm is None else (vm,)))
        return normal

    @staticmethod
    def backward(ctx, g_normal):
        dev = ctx.dev
        W, H, tx, ty = ctx.geometry
        if W * H == 0 or g_normal is None:
            return (torch.zeros(ctx.shape, dtype=torch.float32, device=dev),) + (None,) * 6
        z = ctx.saved_tensors[0]
        vm = ctx.saved_tensors[1] if ctx.world else None
        g = _f32c(g_normal)
        g_depth = torch.empty(H, W, dtype=torch.float32, device=dev)
        _launch(_normals_probe, "msgs_depth_normal_backward", dev, W, H, tx, ty, _ptr(z), _ptr(vm), int(ctx.world), _ptr(g),
                _ptr(g_depth))
        return (g_depth.view(ctx.shape),) + (None,) * 6


def depth_to_normal(depth, raster_settings, world=False):
    """normal [3,H,W] float32 of the surface a map of view depths `depth` [H,W] describes (median_depth, depth / alpha, a sensor
    map ...) under the camera of `raster_settings` (image_width, image_height, tanfovx, tanfovy): 2DGS's depth_to_normal, the
    surf_normal of a depth-normal consistency loss.  Pixel (x, y) back-projects to P = (a_x z, a_y z, z) with
    a_x = ((2 x + 1) / W - 1) tanfovx, the ray through the pixel centre;
        u = P(x, y+1) - P(x, y-1),   v = P(x+1, y) - P(x-1, y),   n = u x v / ||u x v||
    so a fronto-parallel plane gives (0, 0, -1), facing the camera like gaussian_normals().  The pixel's own depth does not
    enter.  A pixel on the image border, with a stencil depth that is not finite and > 0 (a hole) or with a degenerate cross
    product is exactly 0 and passes no gradient.  world=True rotates the map into world space with the 3x3 block of viewmatrix
    (w_j = sum_k V[4 j + k] n_k).  Differentiable in `depth`; the camera is a constant.  The backward is a gather in a fixed
    order, without atomics: the same bits on every run.  One tiled HIP kernel forward and one backward.
    float64 and strided maps are converted and a [1,H,W] map is taken as [H,W]; ValueError when the shape is not the settings'."""
    H, W = int(raster_settings.image_height), int(raster_settings.image_width)
    if depth.dim() == 3 and depth.shape[0] == 1:
        depth = depth[0]
    if depth.dim() != 2 or tuple(depth.shape) != (H, W):
        raise ValueError(f"depth_to_normal: depth must be [{H},{W}] (image_height, image_width of the settings), got "
                         f"{tuple(depth.shape)}")
    return _DepthToNormal.apply(depth, raster_settings.viewmatrix if world else None, W, H, float(raster_settings.tanfovx),
                                float(raster_settings.tanfovy), bool(world))


# Bilateral-grid colour correction (4.20): the per-image correction a trainer places between render() and the
# photometric loss.  Two functions outside the rasterizer; host/bilagrid.py holds the module that owns a bank of grids.
BILAGRID_TILE_W, BILAGRID_TILE_H, BILAGRID_WINDOW_CELLS = _C.BILAGRID_TILE_W, _C.BILAGRID_TILE_H, _C.BILAGRID_WINDOW_CELLS
_bilagrid_probe = None             # tests: a callable (name) run in front of every msgs_bilagrid_* call


def _bilagrid_sizes(grid, where):
    """(GX, GY, GL) of a grid [12,GL,GY,GX]; the sizes the kernels take, anything else is refused"""
    if grid.dim() != 4 or grid.shape[0] != 12:
        raise ValueError(f"{where}: grid must be [12,GL,GY,GX], got {tuple(grid.shape)}")
    GL, GY, GX = (int(v) for v in grid.shape[1:])
    if not (1 <= GX <= _C.BILAGRID_MAX_XY and 1 <= GY <= _C.BILAGRID_MAX_XY and 1 <= GL <= _C.BILAGRID_MAX_L):
        raise ValueError(f"{where}: grid sizes must satisfy 1 <= GX, GY <= {_C.BILAGRID_MAX_XY} and 1 <= GL <= "
                         f"{_C.BILAGRID_MAX_L}, got GX={GX} GY={GY} GL={GL}")
    return GX, GY, GL


class _BilateralSlice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, grid):
        dev = image.device
        if dev.type != "cuda" or grid.device != dev:
            raise RuntimeError(_HIP_ONLY)
        H, W = int(image.shape[1]), int(image.shape[2])
        GX, GY, GL = _bilagrid_sizes(grid, "bilateral_slice")
        ctx.dev, ctx.geometry, ctx.shapes = dev, (W, H, GX, GY, GL), (image.shape, grid.shape)
        out = torch.empty(3, H, W, dtype=torch.float32, device=dev)
        if W * H == 0:
            return out
        im, gr = _f32c(image.detach()), _f32c(grid.detach())
        _launch(_bilagrid_probe, "msgs_bilagrid_slice_forward", dev, W, H, GX, GY, GL, _ptr(im), _ptr(gr), _ptr(out))
        ctx.save_for_backward(im, gr)
        return out

    @staticmethod
    def backward(ctx, g_out):
        dev = ctx.dev
        W, H, GX, GY, GL = ctx.geometry
        want_image, want_grid = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if W * H == 0 or g_out is None:
            return (torch.zeros(ctx.shapes[0], dtype=torch.float32, device=dev) if want_image else None,
                    torch.zeros(ctx.shapes[1], dtype=torch.float32, device=dev) if want_grid else None)
        im, gr = ctx.saved_tensors
        g = _f32c(g_out)
        g_image = torch.empty(3, H, W, dtype=torch.float32, device=dev) if want_image else None
        g_grid = torch.empty(12, GL, GY, GX, dtype=torch.float32, device=dev) if want_grid else None
        scratch, nbytes = None, 0
        if want_grid:
            nbytes = int(_C.lib.msgs_bilagrid_scratch_bytes(W, H, GX, GY, GL))
            scratch = _bytes(nbytes, dev)
        want = (_C.BILAGRID_GRAD_IMAGE if want_image else 0) | (_C.BILAGRID_GRAD_GRID if want_grid else 0)
        _launch(_bilagrid_probe, "msgs_bilagrid_slice_backward", dev, W, H, GX, GY, GL, _ptr(im), _ptr(gr), _ptr(g), want,
                _ptr(g_image), _ptr(g_grid), _ptr(scratch), nbytes)
        return (g_image.view(ctx.shapes[0]) if want_image else None), (g_grid if want_grid else None)


def bilateral_slice(image, grid):
    """out [3,H,W] float32: `image` [3,H,W] (the layout of render()["render"]) corrected by ONE image's bilateral grid
    `grid` [12,GL,GY,GX] — channel 4 c + j is entry (c, j) of a 3x4 affine colour transform, stored over (x, y, luminance):
        fx = (x + 0.5) / W (GX - 1),  fy = (y + 0.5) / H (GY - 1),  z = 0.299 r + 0.587 g + 0.114 b,  fz = clamp(z, 0, 1) (GL - 1)
        A = trilinear interpolation of the grid at (fx, fy, fz),   out_c = A[c,0] r + A[c,1] g + A[c,2] b + A[c,3]
    which is F.grid_sample(bilinear, border, align_corners=True) followed by the affine product (gsplat's use_bilateral_grid,
    "Bilateral Guided Radiance Field Processing").  The identity grid (eye(4)[:3].flatten() in every cell) returns the image
    bit for bit; a 1x1x1 grid is upstream 3DGS's 3x4 exposure matrix.  Differentiable in both arguments; the guide is computed
    from the image being corrected and its gradient flows (where 0 < z < 1, open at both ends — grid_sample's convention, so a
    black pixel gets the direct term only).  A frozen grid or a detached image skips its half of the backward.  grid.grad is
    summed in one fixed order without float atomics: the same bits on every run.  1 <= GX, GY <= 256 and 1 <= GL <= 32, anything
    else raises ValueError.  A NaN or Inf pixel stays inside the grid; only its own output, its own gradient and the grid nodes
    it touches can carry its NaN.  float64 and strided inputs are converted.  HIP kernels only."""
    if image.dim() != 3 or image.shape[0] != 3:
        raise ValueError(f"bilateral_slice: image must be [3,H,W], got {tuple(image.shape)}")
    _bilagrid_sizes(grid, "bilateral_slice")
    return _BilateralSlice.apply(image, grid)


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        dev = grids.device
        _hip_only(dev)
        N, _, GL, GY, GX = (int(v) for v in grids.shape)
        ctx.dev, ctx.sizes, ctx.shape = dev, (N, GX, GY, GL), grids.shape
        tv = torch.zeros(1, dtype=torch.float32, device=dev)
        if N == 0:
            return tv[0]
        gr = _f32c(grids.detach())
        nbytes = int(_C.lib.msgs_bilagrid_tv_scratch_bytes(gr.numel()))
        scratch = _bytes(nbytes, dev)
        _launch(_bilagrid_probe, "msgs_bilagrid_tv_forward", dev, N, GX, GY, GL, _ptr(gr), _ptr(tv), _ptr(scratch), nbytes)
        ctx.save_for_backward(gr)
        return tv[0]

    @staticmethod
    def backward(ctx, g_tv):
        dev = ctx.dev
        N, GX, GY, GL = ctx.sizes
        g_grids = torch.zeros(ctx.shape, dtype=torch.float32, device=dev)
        if N == 0 or g_tv is None:
            return g_grids
        (gr,) = ctx.saved_tensors
        up = _f32c(g_tv.detach().to(dev)).reshape(1)
        _launch(_bilagrid_probe, "msgs_bilagrid_tv_backward", dev, N, GX, GY, GL, _ptr(gr), _ptr(up), _ptr(g_grids))
        return g_grids


def total_variation_loss(grids):
    """scalar: the total variation of a bank of bilateral grids `grids` [N,12,GL,GY,GX] — the sum over the three spatial axes of
    the mean, over every (n, channel, position), of the squared forward difference along that axis; an axis of size 1 adds 0
    (gsplat's total_variation_loss).  Summed in double in a fixed order (the same bits on every run); differentiable, the
    backward is a gather scaled by the upstream scalar, which is read on the device.  Two HIP kernels forward, one backward."""
    if grids.dim() != 5 or grids.shape[1] != 12:
        raise ValueError(f"total_variation_loss: grids must be [N,12,GL,GY,GX], got {tuple(grids.shape)}")
    _bilagrid_sizes(grids[0] if grids.shape[0] else grids.new_zeros((12,) + tuple(grids.shape[2:])), "total_variation_loss")
    return _TotalVariation.apply(grids)


# TSDF fusion and mesh extraction (4.22): depth maps (median depth, by preference) fused into a block-sparse
# volume of TSDF and weight SUMS, and the zero level set extracted by marching tetrahedra.  `volume` is any object with the
# attributes of host/tsdf.py's TSDFVolume: origin (3 floats), voxel_size, blocks (NBx, NBy, NBz), table int32 [NBz,NBy,NBx],
# slot_block int32 [S], tsdf_sum / weight_sum float32 [S,512], colour_sum float32 [S,3,512] or None.  Nothing here is
# differentiable.
TSDF_CAMERA_CHUNK = _C.TSDF_CAMERA_CHUNK
TSDF_MAX_BLOCKS_PER_AXIS, TSDF_MAX_SLOTS = _C.TSDF_MAX_BLOCKS_PER_AXIS, _C.TSDF_MAX_SLOTS
_tsdf_probe = None                 # tests: a callable (name) run in front of every msgs_tsdf_* call


def tsdf_mark_steps(voxel_size, sdf_trunc, table):
    """steps of the activation walk: the smallest count for which a step of 2 r / steps in view depth, r = sdf_trunc + 2 voxels,
    is at most one voxel along every ray of the host camera table [n,20] — ceil(2 r L / voxel) with L = max over the rows of
    sqrt(1 + tanfovx^2 + tanfovy^2), formed in double from the float32 values the kernels read"""
    import math
    import numpy as np
    v, t = float(np.float32(voxel_size)), float(np.float32(sdf_trunc))
    tab = table.detach().cpu().double()
    L = torch.sqrt(1.0 + (tab[:, 18] / (2.0 * tab[:, 16])) ** 2 + (tab[:, 19] / (2.0 * tab[:, 17])) ** 2).max().item()
    return max(1, int(math.ceil(2.0 * (t + 2.0 * v) * L / v)))


def _tsdf_geometry(volume, who):
    blocks = tuple(int(b) for b in volume.blocks)
    if len(blocks) != 3 or any(b < 1 or b > TSDF_MAX_BLOCKS_PER_AXIS for b in blocks):
        raise ValueError(f"{who}: the volume has {blocks} blocks, 1 .. {TSDF_MAX_BLOCKS_PER_AXIS} per axis are supported")
    if not float(volume.voxel_size) > 0.0:
        raise ValueError(f"{who}: voxel_size must be positive")
    table = volume.table
    if table.dtype != torch.int32 or tuple(table.shape) != blocks[::-1] or not table.is_contiguous():
        raise ValueError(f"{who}: table must be a contiguous int32 tensor {blocks[::-1]}")
    v = _C.TsdfVolume()
    v.origin[:] = [float(o) for o in volume.origin]
    v.voxel_size = float(volume.voxel_size)
    v.nb[:] = blocks
    v.table = table.data_ptr()
    return v


def _tsdf_pool(volume, who):
    v = _tsdf_geometry(volume, who)
    dev = volume.table.device
    S = int(volume.slot_block.shape[0])
    if S > TSDF_MAX_SLOTS:
        raise ValueError(f"{who}: {S} pool slots, at most {TSDF_MAX_SLOTS} are supported")
    want = [("slot_block", volume.slot_block, torch.int32, (S,)), ("tsdf_sum", volume.tsdf_sum, torch.float32, (S, 512)),
            ("weight_sum", volume.weight_sum, torch.float32, (S, 512))]
    if volume.colour_sum is not None:
        want.append(("colour_sum", volume.colour_sum, torch.float32, (S, 3, 512)))
    for name, t, dtype, shape in want:
        if t.device != dev or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous {dtype} tensor {shape} on {dev}")
    v.n_slots = S
    v.slot_block, v.tsdf_sum, v.weight_sum = volume.slot_block.data_ptr(), volume.tsdf_sum.data_ptr(), volume.weight_sum.data_ptr()
    v.colour_sum = None if volume.colour_sum is None else volume.colour_sum.data_ptr()
    return v


def _tsdf_frames(who, dev, depth, cameras, sdf_trunc, depth_trunc, colour=None, weight=None):
    """(msgs_tsdf_frames_t, the host camera table, the tensors it points to) — everything is checked before any launch"""
    _require_plain_f32(who, "TSDF fusion", depth=depth, colour=colour, weight=weight)
    if depth.dim() != 3:
        raise ValueError(f"{who}: depth must be [n,H,W], got {tuple(depth.shape)}")
    n, H, W = (int(x) for x in depth.shape)
    if H < 1 or W < 1 or W * H >= 1 << 29 or n > 65535:
        raise ValueError(f"{who}: depth [n,H,W] = {tuple(depth.shape)} is outside the supported sizes")
    if colour is not None and tuple(colour.shape) != (n, 3, H, W):
        raise ValueError(f"{who}: colour must be [n,3,H,W] = {(n, 3, H, W)}, got {tuple(colour.shape)}")
    if weight is not None and tuple(weight.shape) != (n, H, W):
        raise ValueError(f"{who}: weight must be [n,H,W] = {(n, H, W)}, got {tuple(weight.shape)}")
    if not (float(sdf_trunc) > 0.0 and float(sdf_trunc) < float("inf")):
        raise ValueError(f"{who}: sdf_trunc must be positive and finite")
    if not float(depth_trunc) > 0.0:
        raise ValueError(f"{who}: depth_trunc must be positive")
    if torch.is_tensor(cameras):
        table = cameras.detach().float().cpu().contiguous()
        if table.dim() != 2 or table.shape[1] != _C.FILTER3D_CAMERA_FLOATS:
            raise ValueError(f"{who}: a camera table must be [n,{_C.FILTER3D_CAMERA_FLOATS}]")
    else:
        cameras = list(cameras)
        table = _camera_table(cameras) if cameras else torch.zeros(0, _C.FILTER3D_CAMERA_FLOATS)
    if table.shape[0] != n:
        raise ValueError(f"{who}: {table.shape[0]} cameras for {n} depth maps")
    if n and not bool(((table[:, 18] == W) & (table[:, 19] == H)).all()):
        raise ValueError(f"{who}: every camera of a call must have the size of the depth maps, {W}x{H}")
    _require_hip(who, ("the volume", dev), depth=depth, colour=colour, weight=weight)
    f = _C.TsdfFrames()
    f.n, f.W, f.H = n, W, H
    f.sdf_trunc, f.depth_trunc = float(sdf_trunc), float(depth_trunc)
    return f, table, [t if t is None or t.is_contiguous() else t.contiguous() for t in (depth, colour, weight)]


@torch.no_grad()
def tsdf_allocate(volume, depth, cameras, sdf_trunc, depth_trunc):
    """uint8 [NBz,NBy,NBx]: 1 for every block of the volume's table that holds a sample of the activation walk of SPEC M20 — for
    every pixel with 0 < d <= depth_trunc the points of its ray (through the pixel centre, a_x = ((2x+1)/W - 1) tanfovx) at the
    view depths (d - r) + k 2 r / steps, k = 0 .. steps, r = sdf_trunc + 2 voxels, steps = tsdf_mark_steps(...).  Free space in
    front of the surface is not marked.  One kernel, one lane per pixel; the volume is not changed and nothing is read back."""
    v = _tsdf_geometry(volume, "tsdf_allocate")
    dev = volume.table.device
    f, table, (depth, _, _) = _tsdf_frames("tsdf_allocate", dev, depth, cameras, sdf_trunc, depth_trunc)
    marks = torch.zeros(volume.table.shape, dtype=torch.uint8, device=dev)
    if f.n == 0:
        return marks
    steps = tsdf_mark_steps(volume.voxel_size, sdf_trunc, table)
    cams = table.to(dev)
    f.cameras, f.depth = cams.data_ptr(), depth.data_ptr()
    _launch(_tsdf_probe, "msgs_tsdf_mark_blocks", dev, C.byref(v), C.byref(f), steps, _ptr(marks))
    return marks


@torch.no_grad()
def tsdf_integrate(volume, depth, cameras, sdf_trunc, depth_trunc, colour=None, weight=None):
    """Adds the views (depth [n,H,W], cameras: n camera objects or a [n,20] table, colour [n,3,H,W] iff the volume stores colour,
    weight [n,H,W] or 1) to the sums of every pool slot of `volume`, in place: projective TSDF with nearest-pixel lookup,
    tsdf_sum += w min(1, (d - t.z) / sdf_trunc), weight_sum += w, colour_sum += w c, in camera order (SPEC M20).  One kernel,
    one workgroup per slot; the pool is read and written once whatever n is.  Returns None."""
    v = _tsdf_pool(volume, "tsdf_integrate")
    dev = volume.table.device
    f, table, (depth, colour, weight) = _tsdf_frames("tsdf_integrate", dev, depth, cameras, sdf_trunc, depth_trunc, colour, weight)
    if (colour is None) != (volume.colour_sum is None) and f.n:
        raise ValueError("tsdf_integrate: colour maps are needed exactly when the volume stores colour")
    if v.n_slots == 0 or f.n == 0:
        return
    cams = table.to(dev)
    f.cameras, f.depth = cams.data_ptr(), depth.data_ptr()
    f.colour = None if colour is None else colour.data_ptr()
    f.weight = None if weight is None else weight.data_ptr()
    _launch(_tsdf_probe, "msgs_tsdf_integrate", dev, C.byref(v), C.byref(f))


@torch.no_grad()
def tsdf_extract(volume):
    """(vertices [V,3] float32, colours [V,3] float32 or None, faces [F,3] int32): the zero level set of T = tsdf_sum / weight_sum
    over the observed lattice points by marching tetrahedra (six Kuhn tetrahedra per cube, SPEC M20) — indexed and welded by
    construction, normals towards positive TSDF, in a fixed order.  A count kernel, two torch.cumsum, one host read of the two
    totals, an emit kernel.  Vertices no face uses (on edges without a fully observed cube) are kept; see
    TSDFVolume.extract_mesh(drop_unreferenced=True)."""
    v = _tsdf_pool(volume, "tsdf_extract")
    dev = volume.table.device
    _require_hip("tsdf_extract", ("the volume", dev))
    S = v.n_slots
    has_colour = volume.colour_sum is not None
    empty = (torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev) if has_colour else None,
             torch.zeros(0, 3, dtype=torch.int32, device=dev))
    if S == 0:
        return empty
    with _on_device(dev):
        mask = torch.empty(S * 512, dtype=torch.uint8, device=dev)
        vcount = torch.empty(S * 512, dtype=torch.int32, device=dev)
        tcount = torch.empty(S * 512, dtype=torch.int32, device=dev)
        _launch(_tsdf_probe, "msgs_tsdf_count", dev, C.byref(v), _ptr(mask), _ptr(vcount), _ptr(tcount))
        vend, tend = torch.cumsum(vcount, 0, dtype=torch.int64), torch.cumsum(tcount, 0, dtype=torch.int64)
        V, F = (int(x) for x in torch.stack((vend[-1], tend[-1])).tolist())
        if V >= 1 << 31 or F >= 1 << 31:
            raise ValueError(f"tsdf_extract: {V} vertices and {F} faces do not fit int32 indices")
        if V == 0 and F == 0:
            return empty
        m = _C.TsdfMesh()
        voff, toff = (vend - vcount).to(torch.int32), (tend - tcount).to(torch.int32)
        vertices = torch.empty(V, 3, dtype=torch.float32, device=dev)
        colours = torch.empty(V, 3, dtype=torch.float32, device=dev) if has_colour else None
        faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
        m.edge_mask, m.vertex_offset, m.triangle_offset = mask.data_ptr(), voff.data_ptr(), toff.data_ptr()
        m.n_vertices, m.n_faces = V, F
        m.vertices, m.colours, m.faces = vertices.data_ptr(), None if colours is None else colours.data_ptr(), faces.data_ptr()
        _launch(_tsdf_probe, "msgs_tsdf_emit", dev, C.byref(v), C.byref(m))
    return vertices, colours, faces


# k-means vector quantisation (SPEC M21; 4.23): the two device steps of a k-means iteration on any [P,D] float32
# tensor, D <= VQ_MAX_DIM, K <= VQ_MAX_CODES — the nearest-code search on the f32 MFMA, fused with the argmin so that no [P,K] score
# ever reaches memory, and a centroid update without float atomics whose bits do not depend on the launch.  host/compress.py builds
# k-means and the compressed model file on them.  Not differentiable.
VQ_MAX_DIM, VQ_MAX_CODES = _C.VQ_MAX_DIM, _C.VQ_MAX_CODES
VQ_CODE_CHUNK, VQ_UPDATE_CHUNK = _C.VQ_CODE_CHUNK, _C.VQ_UPDATE_CHUNK
_vq_probe = None                   # tests: a callable (name) run in front of every msgs_vq_* call


def _vq_rows(who, x, codebook, **more):
    """(P, D, K) of x [P,D] and codebook [K,D] — everything is checked before any launch; `more`: further float32 tensors"""
    _require_plain_f32(who, "vector quantisation", x=x, codebook=codebook, **more)
    if x.dim() != 2 or codebook.dim() != 2:
        raise ValueError(f"{who}: x must be [P,D] and codebook [K,D], got {tuple(x.shape)} and {tuple(codebook.shape)}")
    (P, D), (K, Dc) = (int(n) for n in x.shape), (int(n) for n in codebook.shape)
    if D != Dc:
        raise ValueError(f"{who}: x has {D} columns, the codebook {Dc}")
    if not 1 <= D <= VQ_MAX_DIM:
        raise ValueError(f"{who}: D = {D}, 1 .. {VQ_MAX_DIM} columns are supported")
    if not 1 <= K <= VQ_MAX_CODES:
        raise ValueError(f"{who}: K = {K}, 1 .. {VQ_MAX_CODES} codes are supported")
    if P >= 1 << 31:
        raise ValueError(f"{who}: P = {P} rows do not fit int32 indices")
    return P, D, K


@torch.no_grad()
def vq_assign(x, codebook, return_error=True):
    """(idx [P] int32, err [P] float32 or None): for every row of x [P,D] the nearest row of codebook [K,D] under SPEC M21 (a) —
    score s(i,k) = the float32 chain s = n_k; s = fmaf(-x_id, c_kd, s) over ascending d with n_k = float32(1/2 sum_d c_kd^2) taken
    in double, idx the smallest k of minimal score (strict <, from +inf and 0, a NaN never wins), err_i = sum_d (x_id - c_kd)^2 of
    the chosen code as a float32 fmaf chain over the two rows.  One kernel on the f32 MFMA behind a small one that lays the
    codebook out; no [P,K] matrix exists anywhere.  The same bits on every run.  Inputs are assumed finite: a row with a NaN gets
    idx 0 and err NaN; a row with an infinity gets the lowest code whose score came out -inf, or 0 when none did."""
    P, D, K = _vq_rows("vq_assign", x, codebook)
    dev = _require_hip("vq_assign", x=x, codebook=codebook)
    idx = torch.empty(P, dtype=torch.int32, device=dev)
    err = torch.empty(P, dtype=torch.float32, device=dev) if return_error else None
    if P == 0:
        return idx, err
    x, codebook = x.contiguous(), codebook.contiguous()
    scratch = _bytes(_C.lib.msgs_vq_scratch_bytes(0, D, K), dev)
    _launch(_vq_probe, "msgs_vq_assign", dev, P, D, K, _ptr(x), _ptr(codebook), _ptr(idx), _ptr(err), _ptr(scratch),
            scratch.numel())
    return idx, err


@torch.no_grad()
def vq_update(x, idx, codebook, weights=None):
    """(new codebook [K,D] float32, mass [K] float64, count [K] int32): SPEC M21 (b) — c_k = float32(sum w_i x_i / sum w_i) over
    the rows with idx == k, in double, summed in ascending row order within chunks of VQ_UPDATE_CHUNK consecutive members and the
    chunk partials added in chunk order; weights [P] float32 >= 0 or None (1).  A code of mass 0 keeps its row of `codebook`.
    Contract: every idx is in [0, K) — checked here (the member ordering reads the counts anyway), before any launch of the sum.
    The stable sort, the counts and the offsets are torch; the weighted segmented sum is two kernels without atomics: the same
    bits on every run and under every launch geometry.  `codebook` is not changed."""
    P, D, K = _vq_rows("vq_update", x, codebook, weights=weights)
    if not torch.is_tensor(idx) or idx.dtype not in (torch.int32, torch.int64) or tuple(idx.shape) != (P,):
        raise ValueError(f"vq_update: idx must be an int32 or int64 tensor [{P}]")
    if weights is not None and tuple(weights.shape) != (P,):
        raise ValueError(f"vq_update: weights must be [{P}], got {tuple(weights.shape)}")
    dev = _require_hip("vq_update", x=x, idx=idx, codebook=codebook, weights=weights)
    x, codebook = x.contiguous(), codebook.contiguous()
    weights = None if weights is None else weights.contiguous()
    with _on_device(dev):
        if P and (int(idx.min()) < 0 or int(idx.max()) >= K):
            raise ValueError(f"vq_update: idx must lie in [0, {K})")
        order = torch.sort(idx, stable=True).indices if P else torch.zeros(0, dtype=torch.int64, device=dev)
        members = torch.bincount(idx, minlength=K) if P else torch.zeros(K, dtype=torch.int64, device=dev)
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        offsets = torch.cat((zero, torch.cumsum(members, 0))).to(torch.int32)
        chunks = (members + (VQ_UPDATE_CHUNK - 1)) // VQ_UPDATE_CHUNK
        chunk_offsets = torch.cat((zero, torch.cumsum(chunks, 0))).to(torch.int32)
        new = torch.empty_like(codebook)
        mass = torch.empty(K, dtype=torch.float64, device=dev)
        count = torch.empty(K, dtype=torch.int32, device=dev)
        scratch = _bytes(_C.lib.msgs_vq_scratch_bytes(P, D, K), dev)
        _launch(_vq_probe, "msgs_vq_update", dev, P, D, K, _ptr(x), _ptr(weights), _ptr(order), _ptr(offsets), _ptr(chunk_offsets),
                _ptr(codebook), _ptr(new), _ptr(mass), _ptr(count), _ptr(scratch), scratch.numel())
    return new, mass, count


# Connected components and mesh clean-up (SPEC M22; 4.24): the smallest-node label of every node of a graph, the
# connected triangle clusters of a mesh (Open3D's cluster_connected_triangles) and its edge report.  The union-find behind them is
# written by atomicMin only and waits on nobody; its result is defined by the input alone, so it has the same bits on every run.
# host/mesh.py builds post_process_mesh on them.  Not differentiable.
_mesh_probe = None                 # tests: a callable (name) run in front of every msgs_graph_* / msgs_mesh_* call


def _mesh_index_tensor(who, name, t, shape_ok, shape_text):
    if not torch.is_tensor(t) or t.dtype not in (torch.int32, torch.int64) or not shape_ok(t):
        raise ValueError(f"{who}: {name} must be an int32 or int64 tensor {shape_text}")


def _mesh_in_range(who, name, t, n):
    """the last check in front of a launch: 0 <= t < n for every element (one host read); returns t as contiguous int32"""
    if t.numel():
        lo, hi = torch.stack((t.min(), t.max())).tolist()
        if lo < 0 or hi >= n:
            raise ValueError(f"{who}: {name} must lie in [0, {n}), got {lo} .. {hi}")
    return t.to(torch.int32).contiguous()


@torch.no_grad()
def graph_components(n_nodes, a, b):
    """label [n_nodes] int32: label[x] is the smallest node of x's connected component under the undirected edges (a[i], b[i])
    (a, b: [E] int32 or int64 on one HIP device, 0 <= a, b < n_nodes — checked with one host read; self-loops and repeated
    edges are allowed).  SPEC M22 (a): the result is defined by the input alone.  Three launches (identity, link, flatten);
    without edges the labels are torch.arange and nothing is launched."""
    N = int(n_nodes)
    if N < 0 or N >= 1 << 31:
        raise ValueError(f"graph_components: n_nodes = {N} is outside [0, 2^31)")
    for name, t in (("a", a), ("b", b)):
        _mesh_index_tensor("graph_components", name, t, lambda t: t.dim() == 1, "[E]")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("graph_components: a and b must have one shape and one device")
    E, dev = int(a.shape[0]), a.device
    if E >= 1 << 31:
        raise ValueError(f"graph_components: E = {E} edges do not fit int32 indices")
    _require_hip("graph_components", a=a, b=b)
    with _on_device(dev):
        a, b = _mesh_in_range("graph_components", "a", a, N), _mesh_in_range("graph_components", "b", b, N)
        if N == 0 or E == 0:
            return torch.arange(N, dtype=torch.int32, device=dev)
        parent = torch.empty(N, dtype=torch.int32, device=dev)
        label = torch.empty(N, dtype=torch.int32, device=dev)
        _launch(_mesh_probe, "msgs_graph_components", dev, N, E, _ptr(a), _ptr(b), _ptr(parent), _ptr(label))
    return label


def _mesh_faces(who, faces, n_vertices):
    _mesh_index_tensor(who, "faces", faces, lambda t: t.dim() == 2 and t.shape[1] == 3, "[F,3]")
    V, F = int(n_vertices), int(faces.shape[0])
    if V < 0 or V >= 1 << 31:
        raise ValueError(f"{who}: n_vertices = {V} is outside [0, 2^31)")
    if 3 * F >= 1 << 31:
        raise ValueError(f"{who}: {F} faces: 3 F must stay below 2^31")
    _require_hip(who, faces=faces)
    return V, F


def _mesh_sorted_keys(faces, F, mode):
    """(keys_sorted [3F] int64, face_sorted [3F] int32): the corner keys of SPEC M22 (b) in ascending order"""
    dev = faces.device
    keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    face_of_key = torch.empty(3 * F, dtype=torch.int32, device=dev)
    _launch(_mesh_probe, "msgs_mesh_corner_keys", dev, F, _ptr(faces), mode, _ptr(keys), _ptr(face_of_key))
    keys_sorted, order = torch.sort(keys)
    return keys_sorted, face_of_key[order]


@torch.no_grad()
def mesh_triangle_clusters(faces, n_vertices, connectivity="edge"):
    """(triangle_clusters [F] int32, cluster_n_triangles [K] int32) of faces [F,3] (int32 or int64, on a HIP device) over
    n_vertices vertices — SPEC M22 (b).  connectivity "edge" (Open3D's rule): two faces are adjacent when they share an
    undirected edge; "vertex": when they share a vertex.  Cluster ids run 0 .. K-1 in ascending order of each cluster's smallest
    face index (in "edge" mode Open3D's numbering).  Indices outside [0, n_vertices) are refused with ValueError before any
    launch (one host read); reading K is the second.  A key kernel, torch.sort, the union-find (three launches), torch.cumsum
    and torch.bincount.  F == 0 launches nothing."""
    if connectivity not in ("edge", "vertex"):
        raise ValueError(f"mesh_triangle_clusters: connectivity must be 'edge' or 'vertex', not {connectivity!r}")
    V, F = _mesh_faces("mesh_triangle_clusters", faces, n_vertices)
    dev = faces.device
    with _on_device(dev):
        faces = _mesh_in_range("mesh_triangle_clusters", "faces", faces, V)
        if F == 0:
            return torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
        mode = _C.MESH_EDGE if connectivity == "edge" else _C.MESH_VERTEX
        keys_sorted, face_sorted = _mesh_sorted_keys(faces, F, mode)
        parent = torch.empty(F, dtype=torch.int32, device=dev)
        label = torch.empty(F, dtype=torch.int32, device=dev)
        _launch(_mesh_probe, "msgs_mesh_link_sorted", dev, F, 3 * F, _ptr(keys_sorted), _ptr(face_sorted), _ptr(parent), _ptr(label))
        is_root = label == torch.arange(F, dtype=torch.int32, device=dev)
        rank = torch.cumsum(is_root, 0, dtype=torch.int32) - 1             # of a root: its cluster id
        clusters = rank[label.long()]
        counts = torch.bincount(clusters).to(torch.int32)
    return clusters, counts


@torch.no_grad()
def mesh_edge_report(faces, n_vertices):
    """(boundary, manifold, non_manifold): the numbers of undirected edges of faces [F,3] used once, twice and more often, as
    Python ints — SPEC M22 (c), from the sorted "edge" keys of mesh_triangle_clusters.  Every face corner counts as one use, so
    a face with a repeated index uses one of its edges twice.  Indices are checked as there; F == 0 launches nothing."""
    V, F = _mesh_faces("mesh_edge_report", faces, n_vertices)
    dev = faces.device
    with _on_device(dev):
        faces = _mesh_in_range("mesh_edge_report", "faces", faces, V)
        if F == 0:
            return 0, 0, 0
        keys_sorted, _ = _mesh_sorted_keys(faces, F, _C.MESH_EDGE)
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        _launch(_mesh_probe, "msgs_mesh_edge_report", dev, 3 * F, _ptr(keys_sorted), _ptr(counts))
        boundary, manifold, non_manifold = counts.tolist()
    return boundary, manifold, non_manifold


# Contribution scores (4.11): what every Gaussian did to the images of one or many views, the criterion of
# contribution-based pruning (LightGaussian's global significance, RadSplat's max contribution, Mini-Splatting's importance).
# With w_ip = alpha_ip T_ip, the blend weight of Gaussian i in pixel p, and an optional per-pixel weight map m_p >= 0:
#     weight_sum = sum_p m_p w_ip      weight_max = max_p m_p w_ip      pixel_count = #{p : m_p > 0, the pair was blended}
# Across views they combine as sum, max, sum — in ONE accumulator that every view's replay adds to (msgs_contrib_accumulate).
class ContributionScores(NamedTuple):
    weight_sum: torch.Tensor       # [P] float32
    weight_max: torch.Tensor       # [P] float32
    pixel_count: torch.Tensor      # [P] int64


_contrib_probe = None              # tests: a callable (call, state) run behind the forward of every contributions() call


def _refuse_contrib_in_verification_mode():
    if _C.lib.msgs_get_deterministic():
        raise ValueError("contribution scores are not offered in the verification mode (set_deterministic): that mode checks the "
                         "reference's arithmetic, it does not train or prune")


class ContributionAccumulator:
    """The scores of P Gaussians over any number of views: owns the accumulator (24 bytes per Gaussian), GaussianRasterizer.
    contributions(..., into=acc) adds a view to it, scores() reads it, reset() starts over.  All on the current stream of the
    caller: add and read on one stream, or order the streams yourself."""

    def __init__(self, P, device):
        _refuse_contrib_in_verification_mode()
        self.P, self.device = int(P), torch.device(device)
        if self.P < 0:
            raise ValueError("P must be >= 0")
        if self.P > 0 and self.device.type != "cuda":
            raise RuntimeError("diff_gaussian_rasterization (MI355X build): the accumulator must live on a HIP device ('cuda')")
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.nbytes = int(_C.lib.msgs_contrib_scratch_bytes(self.P))
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=self.device) if self.P > 0 else None
        self.views = 0

    def reset(self):
        """forget every view: the next add clears the accumulator (no launch here)"""
        self.views = 0

    def _add(self, call, state, pixel_weights):
        geom, binning, image, D = state
        _launch(None, "msgs_contrib_accumulate", self.device, *_replay_args(call, self.P, geom, binning, image, D),
                _ptr(pixel_weights), _ptr(self.buf), self.nbytes, int(self.views == 0))
        self.views += 1

    def scores(self):
        """ContributionScores of the views added so far (zeros before the first)"""
        dev, P = self.device, self.P
        if P == 0 or self.views == 0:
            return ContributionScores(torch.zeros(P, dtype=torch.float32, device=dev), torch.zeros(P, dtype=torch.float32, device=dev),
                                      torch.zeros(P, dtype=torch.int64, device=dev))
        ws = torch.empty(P, dtype=torch.float32, device=dev)
        wm = torch.empty(P, dtype=torch.float32, device=dev)
        pc = torch.empty(P, dtype=torch.int64, device=dev)
        _launch(None, "msgs_contrib_finish", dev, P, _ptr(self.buf), self.nbytes, _ptr(ws), _ptr(wm), _ptr(pc))
        return ContributionScores(ws, wm, pc)


def _check_pixel_weights(pw, H, W, dev):
    if pw is None:
        return None
    if not isinstance(pw, torch.Tensor) or pw.dtype != torch.float32 or tuple(pw.shape) != (H, W):
        raise ValueError(f"pixel_weights must be a float32 tensor of shape [{H}, {W}], got "
                         f"{getattr(pw, 'dtype', type(pw).__name__)} {tuple(getattr(pw, 'shape', ()))}")
    if pw.device != dev:
        raise ValueError(f"pixel_weights must live on {dev}, got {pw.device}")
    return pw.detach() if pw.is_contiguous() else pw.detach().contiguous()


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings, return_alpha=False, absgrad=False):
        """return_alpha=True: forward / forward_raw return the 6-tuple (color, acc_pixel_size, depth, radii, pixel_sizes, alpha)
        with alpha [H,W] float32 = 1 - final transmittance, differentiable; default: the reference's 5-tuple.
        absgrad=True: every backward through a forward / forward_raw of this module also assigns `means2D.absgrad`, float32
        in means2D's shape: (sum over pixels of |that pixel's share of dL/dmean2D| in x and y, 0) — the densification statistic
        of AbsGS, in the units of means2D.grad.  Outputs and gradients are those of the call without it.
        Not offered in the verification mode (set_deterministic): ValueError at the forward."""
        super().__init__()
        self.raster_settings = raster_settings
        self.return_alpha = bool(return_alpha)
        self.absgrad = bool(absgrad)
        self.features = None
        self.return_distortion = False
        self.return_median_depth = False
        self.antialiasing = False

    def _with(self, **flags):
        """a new module like this one — the settings, return_alpha, absgrad and every flag that travels on the module — with
        `flags` replaced: what the with_*() methods return"""
        r = GaussianRasterizer(self.raster_settings, self.return_alpha, self.absgrad)
        for name in ("features", "return_distortion", "return_median_depth", "antialiasing"):
            setattr(r, name, flags.get(name, getattr(self, name)))
        return r

    def with_antialiasing(self, on=True):
        """A rasterizer like this one whose forward / contributions / preprocess_only render ANTIALIASED: the opacity of every
        Gaussian is first multiplied by rho = sqrt(max(0.000025, det0 / det1)), the compensation of Mip-Splatting's 2-D screen
        filter (upstream 3DGS's antialiasing=True, gsplat's rasterize_mode="antialiased"; screen_compensation()), so that the
        +0.3 dilation of the projected covariance no longer brightens Gaussians smaller than a pixel.  By definition the result
        is the plain render of the same model with o_eff = o rho in the place of the opacity, bit for bit: return_alpha,
        absgrad, with_features, with_distortion, depth and camera gradients and the verification mode work as without it, and
        pixel_sizes and the multi-scale filters see o_eff.  Gradients reach opacities, means3D, scales / rotations / cov3D and
        a viewmatrix that requires grad through rho as well.  forward() of such a module takes the plain route: the chained
        backward of the reference's getters does not apply to o rho, their backward runs in autograd.  forward_raw() raises
        ValueError: the raw entry applies the sigmoid inside its kernels.
        (__init__ keeps its pinned parameters, so the flag travels on the module, as with_distortion() does.)"""
        return self._with(antialiasing=bool(on))

    def _opacities(self, means3D, opacities, scales, rotations, cov3D_precomp):
        """the opacities the rasterizer is fed: o rho under with_antialiasing(), else the caller's"""
        if not self.antialiasing:
            return opacities
        return screen_compensation(means3D, opacities, self.raster_settings, scales, rotations, cov3D_precomp)

    def with_distortion(self, return_distortion=True):
        """A rasterizer like this one whose forward / forward_raw also return the depth-distortion map [H,W] float32,
            Dist_p = 2 sum_{j<i} w_ip w_jp (z_i - z_j),   w_ip = alpha_ip T_ip,   z_i the view depth the depth map blends,
        over exactly the pairs the backward counts, in tile-list order (front to back): the signed list-order form of the
        Mip-NeRF 360 distortion loss sum_i sum_j w_i w_j |z_i - z_j| (2DGS, gsplat's distloss), equal to it on a depth-sorted
        list and without a kink at ties.  No background term; exactly 0 for a pixel with fewer than two blended Gaussians.  The
        map is one more output behind alpha and in front of the feature map.  Differentiable: a loss on it sends gradients to
        means, opacity, scales / rotations / cov3D and the camera; SH and colours receive nothing from it.  A loss that ignores
        the map runs today's backward unchanged.  With absgrad=True the statistic means2D.absgrad does NOT include the
        distortion's share: it is that of the colour, depth and alpha terms, as without the map.  Inside deferred_forward such
        a call resolves its own view before the replay: correct, but that view's overlap is lost.  Not offered in the
        verification mode (set_deterministic): ValueError before any launch.
        (__init__ keeps its pinned parameters, so the flag travels on the module, as with_features() does.)"""
        return self._with(return_distortion=bool(return_distortion))

    def with_median_depth(self, on=True):
        """A rasterizer like this one whose forward / forward_raw also return two maps, behind alpha and the distortion map and
        in front of the feature map:
            median_depth [H,W] float32: the view depth (the z the depth map blends) of the Gaussian at which the ray's
                                        transmittance falls through 1/2; 0.0 where nothing was blended
            median_id    [H,W] int32:   the row of that Gaussian in the model; -1 where nothing was blended
        Over the blended entries i = 1..n of a pixel (the pairs the backward counts, in tile-list order, front to back) with the
        forward's own recurrence T_1 = 1, T_{i+1} = fmaf(-T_i, alpha_i, T_i), the median entry is the LAST one with T_i > 0.5
        (the 2DGS / gsplat rule): the entry whose blending takes T to <= 1/2, or the last blended entry of a ray that never
        gets there.  Unlike the blended depth map it is the depth of one Gaussian — no smear across silhouettes, no drift when
        coarse and fine Gaussians stack on a surface — and median_id says which: picking, labels[median_id] lookups, per-pixel
        level ids.  median_depth is differentiable with d median_depth_p / dz_i = [i = median entry of p] and nothing through
        the selection, as in 2DGS: a loss on it sends gradients to means3D and, when asked, to the camera; opacity, scales,
        rotations, means2D, SH and colours receive exactly nothing.  median_id is never differentiable.  A loss that ignores
        the map runs today's backward unchanged.  With absgrad=True the statistic means2D.absgrad does not include this map's
        share: it has none.  Inside deferred_forward such a call resolves its own view before the replay: correct, but that
        view's overlap is lost.  Not offered in the verification mode (set_deterministic): ValueError before any launch
        (DESIGN.md 2, M15).
        (__init__ keeps its pinned parameters, so the flag travels on the module, as with_distortion() does.)"""
        return self._with(return_median_depth=bool(on))

    def with_features(self, features):
        """A rasterizer like this one whose forward / forward_raw also splat `features` [P,C] (float32 device tensor, C >= 1;
        None or an empty tensor: none): per-Gaussian vectors — embeddings, logits, normals — blended with the weights of this
        render.  The feature map [C,H,W] float32, F[c,p] = sum_i f_ic alpha_ip T_ip, becomes one more output at the END of
        the tuple (behind alpha when both are asked for).  No background term: a pixel nothing was blended into is 0; compose
        a background outside with the alpha map.  Differentiable: a loss on the map sends gradients to `features` and, the
        features acting as C more colour channels, to means, opacity, scales / rotations / cov3D and the camera; SH and colours
        receive nothing from it.  Rows of Gaussians in no tile list are never read.  Inside
        deferred_forward a call with features resolves its own view before the replay: correct, but that view's overlap is
        lost.  Not offered in the verification mode (set_deterministic): ValueError before any launch.
        (forward() keeps the reference's 13 parameters, so the tensor travels on the module.)"""
        return self._with(features=features)

    def markVisible(self, positions):
        """Boolean mask of points in front of the near plane (upstream markVisible; unused by the
        reference's Python)."""
        rs = self.raster_settings
        with torch.no_grad():
            pos = _f32c(positions)
            dev = pos.device
            if dev.type != "cuda":
                raise RuntimeError("markVisible: positions must live on a HIP device")
            vm, pm = _f32c(rs.viewmatrix.to(dev)), _f32c(rs.projmatrix.to(dev))
            out = torch.empty(pos.shape[0], dtype=torch.uint8, device=dev)
            _launch(None, "msgs_mark_visible", dev, int(pos.shape[0]), _ptr(pos), _ptr(vm), _ptr(pm), _ptr(out))
        return out.bool()

    def preprocess_only(self, means3D, opacities, scales=None, rotations=None, cov3D_precomp=None,
                        max_pixel_sizes=None, min_pixel_sizes=None, base_mask=None):
        """(radii, pixel_sizes) of this view exactly as forward() returns them, from the per-Gaussian kernel alone —
        no sort / binning / blend, no colour.  For camera sweeps that only read visibility_filter and pixel_sizes
        (/root/reference/train.py:283-300,334-338).  Same argument meaning as forward(); no gradients."""
        rs = self.raster_settings
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        with torch.no_grad():
            P = int(means3D.shape[0])
            dev = means3D.device
            opacities = self._opacities(means3D, opacities, scales, rotations, cov3D_precomp)
            call = _Call(rs, means3D, None, torch.zeros(P, 3, device=dev), opacities, scales, rotations,
                         cov3D_precomp, max_pixel_sizes, min_pixel_sizes, None, None, base_mask)
            radii = torch.zeros(P, dtype=torch.int32, device=dev)
            pixel_sizes = torch.zeros(P, dtype=torch.float32, device=dev)
            if P == 0:
                return radii, pixel_sizes
            geom = torch.empty(int(_C.lib.msgs_geom_bytes(P)), dtype=torch.uint8, device=dev)
            _launch(None, "msgs_preprocess_only", dev, call.view_ref, call.g_ref, _ptr(radii), _ptr(pixel_sizes), _ptr(geom),
                    geom.numel())
        return radii, pixel_sizes

    def contributions(self, means3D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None,
                      max_pixel_sizes=None, min_pixel_sizes=None, base_mask=None, *, pixel_weights=None, into=None):
        """Contribution scores of this view: ContributionScores(weight_sum, weight_max, pixel_count), each
        [P], with w = alpha T the blend weight of a Gaussian in a pixel — its sum and maximum over the pixels and the number of
        pixels it was blended into.  pixel_weights [H,W] float32 (a mask, a per-pixel error ...) multiplies w per pixel and a
        pixel with weight <= 0 (or NaN) does not count.  One ordinary forward of the view (culling, lists and termination are
        the render's) and one replay of the blend walk; no gradients, and nothing of a surrounding render / backward changes.
        Colours do not enter: with neither shs nor colors_precomp, zeros stand in.
        into: a ContributionAccumulator for [P] on this device — the view is ADDED to it (sum, max, sum across views) and
        nothing is returned; read into.scores() after the last view.  Without it: the scores of this one view.
        Not offered in the verification mode (set_deterministic): ValueError before any launch."""
        rs = self.raster_settings
        if shs is not None and colors_precomp is not None:
            raise Exception('Please provide at most one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        _refuse_contrib_in_verification_mode()
        with torch.no_grad():
            P, dev = int(means3D.shape[0]), means3D.device
            if P > 0 and dev.type != "cuda":
                raise RuntimeError("diff_gaussian_rasterization (MI355X build): tensors must live on a HIP device "
                                   "('cuda'); there is no CPU path")
            pw = _check_pixel_weights(pixel_weights, int(rs.image_height), int(rs.image_width), dev)
            if into is not None and (not isinstance(into, ContributionAccumulator) or into.P != P or into.device != dev):
                raise ValueError(f"into must be a ContributionAccumulator for {P} Gaussians on {dev}")
            acc = into if into is not None else ContributionAccumulator(P, dev)
            if P > 0:
                if shs is None and colors_precomp is None:
                    colors_precomp = torch.zeros(P, 3, dtype=torch.float32, device=dev)
                opacities = self._opacities(means3D, opacities, scales, rotations, cov3D_precomp)
                call = _Call(rs, means3D, _opt(shs), _opt(colors_precomp), opacities, _opt(scales), _opt(rotations),
                             _opt(cov3D_precomp), _opt(max_pixel_sizes), _opt(min_pixel_sizes), None, None, _opt(base_mask))
                pending, _deferred.pending = getattr(_deferred, "pending", None), None      # not deferred: the replay reads D
                try:
                    state = _forward_impl(call)[-1]
                finally:
                    _deferred.pending = pending
                if _contrib_probe is not None:
                    _contrib_probe(call, state)
                acc._add(call, state, pw)
            else:
                acc.views += 1
            return None if into is not None else acc.scores()

    def forward_raw(self, xyz, means2D, features_dc, features_rest, opacity_raw, scaling_raw, rotation_raw,
                    max_pixel_sizes=None, min_pixel_sizes=None, occ_multiplier=None, dc_delta=None, base_mask=None, features=None,
                    return_distortion=None, return_median_depth=None):
        """Opt-in fused path on raw GaussianModel parameters (not part of the reference API).  features [P,C]: as in
        with_features(); None: the module's own (with_features), if any.  return_distortion: as in with_distortion(); None:
        the module's own.  return_median_depth: as in with_median_depth(); None: the module's own.  Not offered under with_antialiasing(): ValueError before any launch."""
        if self.antialiasing:
            raise ValueError("with_antialiasing() is not offered on the raw-parameter entry (forward_raw / render_fused): the "
                             "sigmoid is applied inside its kernels; render through forward() instead")
        features = features if features is not None else self.features
        return_distortion = self.return_distortion if return_distortion is None else bool(return_distortion)
        return_median_depth = self.return_median_depth if return_median_depth is None else bool(return_median_depth)
        empty = torch.Tensor([])
        o = lambda t: t if t is not None else empty
        return rasterize_gaussians_raw(xyz, means2D, features_dc, features_rest, opacity_raw, scaling_raw,
                                       rotation_raw, o(max_pixel_sizes), o(min_pixel_sizes), o(occ_multiplier),
                                       o(dc_delta), o(base_mask), self.raster_settings, absgrad=self.absgrad,
                                       return_alpha=self.return_alpha, features=features,
                                       return_distortion=return_distortion, return_median_depth=return_median_depth)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, max_pixel_sizes=None, min_pixel_sizes=None, occ_multiplier=None,
                dc_delta=None, base_mask=None):
        """The reference's 13 parameters.  Feature channels, the distortion map and the median-depth maps travel on the module:
        with_features(features)(...), with_distortion()(...), with_median_depth()(...)."""
        rs = self.raster_settings
        features = self.features
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        empty = torch.Tensor([])
        if self.antialiasing:
            # o rho is not the sigmoid getter: straight to the plain route (no chained mode, none of its warning)
            opacities = self._opacities(means3D, opacities, scales, rotations, cov3D_precomp)
        elif chain_reference_getters and torch.is_grad_enabled() and shs is not None and cov3D_precomp is None \
                and means3D.shape[0] > 0 and means3D.device.type == "cuda" \
                and not (getattr(scales, "_msgs_filtered", False) or getattr(opacities, "_msgs_filtered", False)):
            leaves = _match_reference_getters(means3D, shs, opacities, scales, rotations)
            if leaves is None and not _warned_chain[0] and all(
                    t is not None and t.grad_fn is not None for t in (shs, opacities, scales, rotations)):
                # all four inputs carry an autograd history but it is not the reference's getters (or PyTorch renamed
                # its autograd nodes): correct results through the plain path, but say so once — the chained backward
                # is ~15 % of the step at 1 M Gaussians
                _warned_chain[0] = True
                import warnings
                warnings.warn("diff_gaussian_rasterization: inputs were not recognised as the reference's getters "
                              "(cat / sigmoid / exp / normalize of leaf parameters); their backward runs in autograd")
            if leaves is not None:
                o = lambda t: t if t is not None else empty
                _note_grad_mode()
                return _RasterizeGaussiansChained.apply(
                    means3D, means2D, *leaves, shs.detach() if _chain_reads_cat else empty, opacities.detach(), scales.detach(),
                    rotations.detach(),
                    o(max_pixel_sizes), o(min_pixel_sizes), o(occ_multiplier), o(dc_delta), o(base_mask), rs,
                    *_extra_inputs(rs, self.return_alpha, self.absgrad, means2D, features, means3D, self.return_distortion,
                                   self.return_median_depth))
        return rasterize_gaussians(
            means3D, means2D,
            shs if shs is not None else empty,
            colors_precomp if colors_precomp is not None else empty,
            opacities,
            scales if scales is not None else empty,
            rotations if rotations is not None else empty,
            cov3D_precomp if cov3D_precomp is not None else empty,
            max_pixel_sizes if max_pixel_sizes is not None else empty,
            min_pixel_sizes if min_pixel_sizes is not None else empty,
            occ_multiplier if occ_multiplier is not None else empty,
            dc_delta if dc_delta is not None else empty,
            base_mask if base_mask is not None else empty,
            rs, absgrad=self.absgrad, return_alpha=self.return_alpha, features=features,
            return_distortion=self.return_distortion, return_median_depth=self.return_median_depth)

"""Torch restatement of the reference's four model-surgery methods (GaussianModel.densify_and_prune, grow_large_gaussians,
prune_points, densification_postfix; DESIGN.md SPEC D1) on any device — the checker of ms-gs_amd/host/densify.py at scale.

Same signatures as host/densify.py: (model, <the reference's arguments>, *, optimizer=None[, draws=None]).  Same sequence of
torch operations as the reference (clone postfix, split postfix, prune of the split parents, prune), so on the CPU it reproduces
the reference bit for bit (tests/test_densify_cpu.py against tests/golden/densify_*.npz), and on the GPU it computes what the
reference computes there.  Two deliberate extensions, shared with host/densify.py: tensors that no optimizer group holds are
remapped too (without moments, keeping type and requires_grad), and the appended target_reso_lvl column stays int64.
No empty_cache().
"""
import torch
import torch.nn as nn

GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
          ("occ_multiplier", "_occ_multiplier"), ("dc_delta", "_dc_delta"), ("scaling", "_scaling"), ("rotation", "_rotation"))


def _opt(model, optimizer):
    return optimizer if optimizer is not None else model.optimizer


def _remap(model, opt, fn):
    """every parameter tensor t of the model becomes fn(name, t); moments likewise (fn(name, m, moment=True))"""
    held = {}
    for group in opt.param_groups:
        held[group["name"]] = group
    for name, attr in GROUPS:
        group = held.get(name)
        if group is None:
            old = getattr(model, attr)
            new = fn(name, old.detach())
            new = nn.Parameter(new, requires_grad=old.requires_grad) if isinstance(old, nn.Parameter) else \
                new.requires_grad_(old.requires_grad)
            setattr(model, attr, new)
            continue
        old = group["params"][0]
        st = opt.state.get(old, None)
        if st is not None and len(st) == 0:
            st = None
        new = nn.Parameter(fn(name, old).detach().requires_grad_(True))
        if st is not None:
            st["exp_avg"] = fn(name, st["exp_avg"], moment=True)
            st["exp_avg_sq"] = fn(name, st["exp_avg_sq"], moment=True)
            del opt.state[old]
            group["params"][0] = new
            opt.state[new] = st
        else:
            if old in opt.state:
                del opt.state[old]
            group["params"][0] = new
        setattr(model, attr, new)


def prune_points(model, mask, *, optimizer=None):
    valid = ~mask
    with torch.no_grad():
        _remap(model, _opt(model, optimizer), lambda name, t, moment=False: t[valid])
    for k in ("xyz_gradient_accum", "denom", "max_radii2D", "max_pixel_sizes", "min_pixel_sizes", "base_gaussian_mask",
              "target_reso_lvl"):
        setattr(model, k, getattr(model, k)[valid])


def densification_postfix(model, new_xyz, new_features_dc, new_features_rest, new_opacities, new_occ_multiplier, new_dc_delta,
                          new_scaling, new_rotation, new_target_reso_lvl, new_max_pixel_sizes, new_min_pixel_sizes, reso_lvl=0,
                          *, optimizer=None):
    new = {"xyz": new_xyz, "f_dc": new_features_dc, "f_rest": new_features_rest, "opacity": new_opacities,
           "occ_multiplier": new_occ_multiplier, "dc_delta": new_dc_delta, "scaling": new_scaling, "rotation": new_rotation}

    def grow(name, t, moment=False):
        ext = new[name].to(t.device, t.dtype)
        return torch.cat((t, torch.zeros_like(ext) if moment else ext), dim=0)
    with torch.no_grad():
        _remap(model, _opt(model, optimizer), grow)
    dev, n, L = model._xyz.device, len(new_xyz), model.reso_lvls
    model.xyz_gradient_accum[:, reso_lvl, :] = 0
    model.xyz_gradient_accum = torch.cat([model.xyz_gradient_accum, torch.zeros((n, L, 1), device=dev)], dim=0)
    model.denom[:, reso_lvl, :] = 0
    model.denom = torch.cat([model.denom, torch.zeros((n, L, 1), device=dev)], dim=0)
    model.max_radii2D = torch.zeros((model._xyz.shape[0]), device=dev)
    model.max_pixel_sizes = torch.cat((model.max_pixel_sizes, new_max_pixel_sizes.to(dev)), dim=0)
    model.min_pixel_sizes = torch.cat((model.min_pixel_sizes, new_min_pixel_sizes.to(dev)), dim=0)
    model.base_gaussian_mask = torch.cat((model.base_gaussian_mask, torch.zeros((n,), device=dev, dtype=torch.bool)), dim=0)
    model.target_reso_lvl = torch.cat((model.target_reso_lvl, new_target_reso_lvl.to(dev, torch.int64)), dim=0)


def build_rotation(r):
    """utils/general_utils.py:78-99, op for op"""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _rows(model, mask):
    return dict(xyz=model._xyz[mask], f_dc=model._features_dc[mask], f_rest=model._features_rest[mask],
                opacity=model._opacity[mask], occ=model._occ_multiplier[mask], dc=model._dc_delta[mask],
                scaling=model._scaling[mask], rotation=model._rotation[mask], target=model.target_reso_lvl[mask],
                maxps=model.max_pixel_sizes[mask], minps=model.min_pixel_sizes[mask])


def densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size, *, optimizer=None, draws=None):
    opt = _opt(model, optimizer)
    dev = model._xyz.device
    with torch.no_grad():
        grads = model.xyz_gradient_accum[:, 0] / model.denom[:, 0]
        grads[grads.isnan()] = 0.0
        grads[model.target_reso_lvl != 0] = 0.0
        # clone
        sel = torch.where(torch.norm(grads, dim=-1) >= max_grad, True, False)
        sel = torch.logical_and(sel, torch.max(torch.exp(model._scaling), dim=1).values <= model.percent_dense * extent)
        r = _rows(model, sel)
        densification_postfix(model, r["xyz"], r["f_dc"], r["f_rest"], r["opacity"], r["occ"], r["dc"], r["scaling"],
                              r["rotation"], r["target"], r["maxps"], r["minps"], optimizer=opt)
        # split
        n = model._xyz.shape[0]
        padded = torch.zeros((n), device=dev)
        padded[:grads.shape[0]] = grads.squeeze()
        sel = torch.where(padded >= max_grad, True, False)
        sel = torch.logical_and(sel, torch.max(torch.exp(model._scaling), dim=1).values > model.percent_dense * extent)
        stds = torch.exp(model._scaling)[sel].repeat(2, 1)
        means = torch.zeros((stds.size(0), 3), device=dev)
        z = torch.randn((stds.size(0), 3), device=dev) if draws is None else draws.to(dev)
        samples = z * stds + means                                  # torch.normal(mean, std): normal_(0, 1).mul_(std).add_(mean)
        rots = build_rotation(model._rotation[sel]).repeat(2, 1, 1)
        r = _rows(model, sel)
        new_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + model._xyz[sel].repeat(2, 1)
        new_scaling = torch.log(torch.exp(model._scaling)[sel].repeat(2, 1) / (0.8 * 2))
        densification_postfix(model, new_xyz, r["f_dc"].repeat(2, 1, 1), r["f_rest"].repeat(2, 1, 1), r["opacity"].repeat(2, 1),
                              r["occ"].repeat(2, 1, 1), r["dc"].repeat(2, 1, 1), new_scaling, r["rotation"].repeat(2, 1),
                              r["target"].repeat(2), r["maxps"].repeat(2) / (0.8 * 2), r["minps"].repeat(2) / (0.8 * 2),
                              optimizer=opt)
        prune_points(model, torch.cat((sel, torch.zeros(2 * int(sel.sum()), device=dev, dtype=bool))), optimizer=opt)
        # prune
        pm = (torch.sigmoid(model._opacity) < min_opacity).squeeze()
        if max_screen_size:
            big_vs = model.max_radii2D > max_screen_size
            big_ws = torch.exp(model._scaling).max(dim=1).values > 0.1 * extent
            pm = torch.logical_or(torch.logical_and(torch.logical_or(big_vs, big_ws), model.target_reso_lvl == 0), pm)
        pm = torch.logical_and(pm, model.target_reso_lvl == 0)
        prune_points(model, pm, optimizer=opt)
    return z


def grow_large_gaussians(model, grad_threshold, reso_lvl, *, optimizer=None):
    with torch.no_grad():
        grads = model.xyz_gradient_accum[:, reso_lvl] / model.denom[:, reso_lvl]
        grads[grads.isnan()] = 0.0
        sel = torch.where(torch.norm(grads, dim=-1) >= grad_threshold, True, False)
        r = _rows(model, sel)
        x = torch.sigmoid(model._opacity[sel]) / 2
        new_opacity = torch.log(x / (1 - x))
        new_scaling = torch.log(torch.exp(model._scaling[sel]) * 2)
        densification_postfix(model, r["xyz"], r["f_dc"], r["f_rest"], new_opacity, r["occ"], r["dc"], new_scaling, r["rotation"],
                              torch.ones_like(r["target"]) * reso_lvl, r["maxps"] * 2, r["minps"] * 2, reso_lvl=reso_lvl,
                              optimizer=optimizer)

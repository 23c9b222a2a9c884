"""Float64 truth of the antialiasing compensation (SPEC M14) and the scenes its tests share.

oracle/torch_oracle.py's preprocess returns the differentiable 2-D covariance (a, b, c) WITH the 0.3 of Q3 added, so
    det1 = a c - b^2,   det0 = (a - 0.3)(c - 0.3) - b^2,   rho = sqrt(clamp_min(det0 / det1, 0.000025))
is the whole definition; rows behind the near plane (float32 view depth <= 0.2, Q1) or with det1 == 0 have rho = 1.  Autograd
through it gives every gradient, the view matrix's included."""
import torch

import scenes
from oracle import torch_oracle as to
from parity_utils import small_scene

FLOOR = 0.000025           # rho >= 0.005
DILATION = 0.3

# name: (P, W, H, seed, factor on small_scene's scale_k)
SCENES = {"S1": (300, 40, 24, 7, 1.0), "S2": (300, 40, 24, 8, 0.05), "S3": (300, 64, 48, 9, 4.0), "S2q": (300, 40, 24, 8, 0.25)}


def scene(name):
    """(scene, camera) by name; "S1[:n]" is the slice of S1's first n Gaussians"""
    n = None
    if ":" in name:
        name, n = name.split(":")
        n = int(n)
    P, W, H, seed, k = SCENES[name]
    sc, cam = small_scene(P, W, H, seed, scale_k=0.004 * 1920.0 / W * 0.5 * k)
    if n is not None:
        sc = sc.subset(torch.arange(n))
    return sc, cam


def view_of(cam, scale_modifier=1.0, viewmatrix=None):
    v = to.view_dict(cam, sh_degree=0, scale_modifier=scale_modifier)
    if viewmatrix is not None:
        v["viewmatrix"] = viewmatrix
    return v


def rho(means3D, view, scales=None, rotations=None, cov3D_precomp=None):
    """(rho [P] float64, differentiable; floored [P] bool; regular [P] bool — False where rho is 1 by definition)"""
    P = means3D.shape[0]
    pre = to.preprocess(means3D, torch.ones(P, 1, dtype=torch.float64), view, scales=scales, rotations=rotations,
                        cov3D_precomp=cov3D_precomp, colors_precomp=torch.zeros(P, 3, dtype=torch.float64))
    a, b, c = pre["cov2"]
    det1 = a * c - b * b
    det0 = (a - DILATION) * (c - DILATION) - b * b
    regular = (pre["depth32"] > 0.2) & (det1.detach() != 0)
    r = det0 / torch.where(regular, det1, torch.ones_like(det1))
    value = torch.sqrt(torch.clamp_min(r, FLOOR))
    floored = regular & (r.detach() <= FLOOR)
    return torch.where(regular, value, torch.ones_like(value)), floored, regular


def truth(sc, cam, g, scale_modifier=1.0, precomp=False, camera=False):
    """o_eff and the gradients of sum_i g_i o_eff_i in float64: dict(o_eff, rho, floored, regular, and the gradients opacities,
    means3D, scales + rotations | cov3D_precomp, viewmatrix when `camera`)"""
    dt = torch.float64
    leaf = lambda t: t.detach().to(dt).clone().requires_grad_(True)
    means, opac = leaf(sc.means3D), leaf(sc.opacities)
    V = leaf(cam.world_view_transform) if camera else None
    view = view_of(cam, scale_modifier, V)
    leaves = dict(means3D=means, opacities=opac)
    if precomp:
        cov = leaf(to.cov3d_from_scale_rot(sc.scales.to(dt), sc.rotations.to(dt), scale_modifier).float())   # what the op is fed
        leaves["cov3D_precomp"] = cov
        r, floored, regular = rho(means, view, cov3D_precomp=cov)
    else:
        s, q = leaf(sc.scales), leaf(sc.rotations)
        leaves["scales"], leaves["rotations"] = s, q
        r, floored, regular = rho(means, view, scales=s, rotations=q)
    if camera:
        leaves["viewmatrix"] = V
    o_eff = opac.reshape(-1) * r
    (o_eff * g.to(dt).reshape(-1)).sum().backward()
    out = dict(o_eff=o_eff.detach(), rho=r.detach(), floored=floored, regular=regular)
    if precomp:
        out["cov3D_input"] = cov.detach().float()
    out.update({k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()})
    return out


def seed(P, s=41):
    """g = dL/do_eff [P,1] float32, seeded, N(0,1)"""
    return torch.randn(P, 1, generator=torch.Generator().manual_seed(s))

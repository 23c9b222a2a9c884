"""Float64 truth of the normal maps (SPEC M17; 4.18), written from the definitions, and the inputs its tests
share.  Nothing here touches the library.

(a) Gaussian normals.  k = 0; s_1 < s_k: k = 1; s_2 < s_k: k = 2.  q = r / max(||r||, 1e-12).  n = column k of R(q), R the
rotation of Sigma = R S^2 R^T.  sigma = -1 iff n . (campos - p) < 0.  Output sigma n (world) or its rotation into view space,
out_c = sigma sum_j n_j V[j, c] with V = world_view_transform (a point maps to [p, 1] V).  A row with a non-finite input or
result is (0, 0, 0).  The sign is a discrete decision: a row with |n . d| / ||d|| <= FLAG_COS is FLAGGED, two float32
evaluations may orient it differently.

(b) Depth to normal.  P(x, y) = (a_x z, a_y z, z), a_x = ((2 x + 1) / W - 1) tanfovx; u = P(x, y+1) - P(x, y-1),
v = P(x+1, y) - P(x-1, y), n = u x v / ||u x v||; valid iff the pixel is not on the border, the four depths are finite and > 0
and ||u x v||^2 is finite and > 0, else 0.  World: w_j = sum_k V[j, k] n_k.

Both functions take dtype=torch.float32 as the float32 RESTATEMENT of the same formulas; gradients come from autograd."""
import math

import torch

import scenes

FLAG_COS = 1e-5
GAUSSIAN_P = (1, 63, 64, 257, 4099)
TANFOV = (0.7, 0.45)                       # fx != fy
AXIS_TEST_FILTER = 0.01                    # the 3-D filter of the "same axis" test: small enough to keep the two smallest s_eff of a row apart


# ---------------------------------------------------------------------------------------------------------------------------
# (a) Gaussian normals
# ---------------------------------------------------------------------------------------------------------------------------
def rotation_matrix(q):
    """R(q) [P,3,3] for q = (r, x, y, z), not assumed to be of unit length: I - 2 |v|^2 I + 2 v v^T + 2 r [v]x — the entries of
    the reference's build_rotation in vector form"""
    r, v = q[:, 0], q[:, 1:]
    eye = torch.eye(3, dtype=q.dtype).expand(q.shape[0], 3, 3)
    zero = torch.zeros_like(r)
    cross = torch.stack([zero, -v[:, 2], v[:, 1], v[:, 2], zero, -v[:, 0], -v[:, 1], v[:, 0], zero], dim=1).view(-1, 3, 3)
    vv = v[:, :, None] * v[:, None, :]
    return eye * (1.0 - 2.0 * (v * v).sum(dim=1))[:, None, None] + 2.0 * vv + 2.0 * r[:, None, None] * cross


def shortest_axis(scales):
    s = scales
    rows = torch.arange(s.shape[0])
    k = torch.zeros(s.shape[0], dtype=torch.long)
    k = torch.where(s[:, 1] < s[rows, k], torch.ones_like(k), k)
    k = torch.where(s[:, 2] < s[rows, k], torch.full_like(k, 2), k)
    return k


def normalise(r):
    return r / r.norm(dim=1, keepdim=True).clamp_min(1e-12)


def gaussian_normals(means3D, scales, rotations, viewmatrix, campos, world=False, dtype=torch.float64):
    """dict(normal [P,3], k, sigma, valid, flagged) in `dtype`; differentiable in `rotations` when it is a `dtype` leaf"""
    p, s = means3D.detach().to(dtype), scales.detach().to(dtype)
    r = rotations if rotations.dtype == dtype else rotations.detach().to(dtype)
    V, c = viewmatrix.detach().cpu().to(dtype), campos.detach().cpu().to(dtype)
    P = p.shape[0]
    finite_in = torch.isfinite(p).all(dim=1) & torch.isfinite(s).all(dim=1) & torch.isfinite(r.detach()).all(dim=1)
    unit = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=dtype).expand(P, 4)
    r_safe = torch.where(finite_in[:, None], r, unit)
    p_safe = torch.where(finite_in[:, None], p, torch.zeros_like(p))
    k = shortest_axis(s)
    n = rotation_matrix(normalise(r_safe))[torch.arange(P), :, k]
    d = c[None, :] - p_safe
    facing = (n.detach() * d).sum(dim=1)
    sigma = torch.where(facing < 0, -torch.ones_like(facing), torch.ones_like(facing))
    out = sigma[:, None] * n
    if not world:
        out = out @ V[:3, :3]
    valid = finite_in & torch.isfinite(out.detach()).all(dim=1)
    out = torch.where(valid[:, None], out, torch.zeros_like(out))
    cos = facing / (d.norm(dim=1) * n.detach().norm(dim=1)).clamp_min(1e-300 if dtype == torch.float64 else 1e-30)
    return dict(normal=out, k=k, sigma=sigma, valid=valid, flagged=valid & (cos.abs() <= FLAG_COS))


def camera():
    """a ring camera off every axis: a full 3x3 rotation and a camera centre away from the origin"""
    return scenes.ring_camera(1, 7, 1920, 1080)


def gaussian_rows(P, raw, seed=5):
    """(means3D [P,3], scales [P,3], rotations [P,4], g [P,3]) float32: centres in a ball of radius 4 around the origin (the
    camera sits at radius 8); raw: log-scales in [-6, 1] and quaternions of length 0.1 .. 10; activated: their exp (float32) and
    the float32-normalised quaternions"""
    g = torch.Generator().manual_seed(seed + 31 * P)                # (the same leaves for raw and activated)
    d = torch.randn(P, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    means = (4.0 * d * torch.rand(P, 1, generator=g, dtype=torch.float64) ** (1.0 / 3.0)).float()
    logs = (-6.0 + 7.0 * torch.rand(P, 3, generator=g, dtype=torch.float64)).float()
    rot = torch.randn(P, 4, generator=g, dtype=torch.float64)
    rot = rot / rot.norm(dim=1, keepdim=True) * torch.exp(math.log(0.1) + math.log(100.0) * torch.rand(P, 1, generator=g,
                                                                                                      dtype=torch.float64))
    rot = rot.float()
    grad = torch.randn(P, 3, generator=g)
    if raw:
        return means.contiguous(), logs.contiguous(), rot.contiguous(), grad
    return means.contiguous(), torch.exp(logs).contiguous(), normalise(rot).contiguous(), grad


def gaussian_truth(means3D, scales, rotations, g, cam, world):
    """float64 forward, dL/drotations of sum g . normal by autograd, and the float32 restatement's own forward error on the
    unflagged rows"""
    r = rotations.detach().double().clone().requires_grad_(True)
    t = gaussian_normals(means3D, scales, r, cam.world_view_transform, cam.camera_center, world)
    (t["normal"] * g.double()).sum().backward()
    t32 = gaussian_normals(means3D, scales, rotations.float(), cam.world_view_transform, cam.camera_center, world, torch.float32)
    ok = ~t["flagged"]
    restated = (t32["normal"].double() - t["normal"].detach()).abs()[ok].max().item() if bool(ok.any()) else 0.0
    return dict(normal=t["normal"].detach(), grad=r.grad, flagged=t["flagged"], valid=t["valid"], k=t["k"], sigma=t["sigma"],
                restated=restated)


# ---------------------------------------------------------------------------------------------------------------------------
# (b) depth to normal
# ---------------------------------------------------------------------------------------------------------------------------
def rays(W, H, tanfovx, tanfovy, dtype=torch.float64):
    """(a_x [W], a_y [H])"""
    c = lambda v: torch.tensor(v, dtype=dtype)
    ax = ((c(2.0) * torch.arange(W, dtype=dtype) + c(1.0)) / c(float(W)) - c(1.0)) * c(tanfovx)
    ay = ((c(2.0) * torch.arange(H, dtype=dtype) + c(1.0)) / c(float(H)) - c(1.0)) * c(tanfovy)
    return ax, ay


def depth_to_normal(depth, tanfovx, tanfovy, viewmatrix=None, dtype=torch.float64):
    """(normal [3,H,W], valid [H,W]) in `dtype`; differentiable in `depth` when it is a `dtype` leaf.  viewmatrix: the world map"""
    z = depth if depth.dtype == dtype else depth.detach().to(dtype)
    H, W = z.shape
    out = torch.zeros(3, H, W, dtype=dtype)
    valid = torch.zeros(H, W, dtype=torch.bool)
    if H < 3 or W < 3:
        return out + 0.0 * torch.nan_to_num(z).sum(), valid           # (still a function of z: its gradient is 0)
    good = torch.isfinite(z.detach()) & (z.detach() > 0)
    zs = torch.where(good, z, torch.ones_like(z))                 # holes carry no gradient and no NaN into the others
    ax, ay = rays(W, H, tanfovx, tanfovy, dtype)
    pts = torch.stack([ax[None, :] * zs, ay[:, None] * zs, zs])
    u = pts[:, 2:, 1:-1] - pts[:, :-2, 1:-1]
    v = pts[:, 1:-1, 2:] - pts[:, 1:-1, :-2]
    c = torch.linalg.cross(u, v, dim=0)
    cc = (c * c).sum(dim=0)
    ok = good[2:, 1:-1] & good[:-2, 1:-1] & good[1:-1, 2:] & good[1:-1, :-2] & torch.isfinite(cc.detach()) & (cc.detach() > 0)
    n = torch.where(ok[None], c / torch.sqrt(torch.where(ok, cc, torch.ones_like(cc)))[None], torch.zeros_like(c))
    if viewmatrix is not None:
        R = viewmatrix.detach().cpu().to(dtype)[:3, :3]
        n = torch.einsum("jk,khw->jhw", R, n)
    out = torch.nn.functional.pad(n, (1, 1, 1, 1))
    valid[1:-1, 1:-1] = ok
    return out, valid


def plane_depth(W, H, tanfovx, tanfovy, n, d):
    """float64 depth map [H,W] of the plane n . P = d seen through the pixel centres: z = d / (n_x a_x + n_y a_y + n_z)"""
    ax, ay = rays(W, H, tanfovx, tanfovy)
    return d / (n[0] * ax[None, :] + n[1] * ay[:, None] + n[2])


PLANE = (torch.tensor([0.28, -0.19, -0.94], dtype=torch.float64) / torch.tensor([0.28, -0.19, -0.94],
                                                                                 dtype=torch.float64).norm(), -5.0)


def depth_map(H, W, seed=3):
    """float32 [H,W]: a tilted plane facing the camera at depth about 5 plus a smooth relief of amplitude 0.3 (depths > 0)"""
    g = torch.Generator().manual_seed(seed)
    ph = 2.0 * math.pi * torch.rand(4, generator=g, dtype=torch.float64)
    z = plane_depth(W, H, TANFOV[0], TANFOV[1], *PLANE)
    x, y = torch.arange(W, dtype=torch.float64)[None, :], torch.arange(H, dtype=torch.float64)[:, None]
    relief = 0.2 * torch.sin(0.37 * x + ph[0]) * torch.cos(0.29 * y + ph[1]) + 0.1 * torch.sin(0.11 * x + 0.17 * y + ph[2])
    return (z + relief).float().contiguous()


def depth_shapes(tile_w, tile_h):
    return ((1, 1), (2, 5), (3, 3), (3, tile_w + 1), (tile_h + 1, 3), (2 * tile_h + 3, 2 * tile_w + 5))


def depth_truth(depth, g, viewmatrix=None):
    """float64 forward, dL/ddepth of sum g . normal by autograd, and the float32 restatement's own errors: forward (max abs on
    the valid pixels) and backward (max-norm relative)"""
    z = depth.detach().double().clone().requires_grad_(True)
    n, valid = depth_to_normal(z, TANFOV[0], TANFOV[1], viewmatrix)
    (n * g.double()).sum().backward()
    grad = z.grad if z.grad is not None else torch.zeros_like(z)
    z32 = depth.detach().float().clone().requires_grad_(True)
    n32, valid32 = depth_to_normal(z32, TANFOV[0], TANFOV[1], viewmatrix, torch.float32)
    (n32 * g.float()).sum().backward()
    grad32 = z32.grad if z32.grad is not None else torch.zeros_like(z32)
    both = valid & valid32
    fwd = (n32.detach().double() - n.detach()).abs()[:, both].max().item() if bool(both.any()) else 0.0
    scale = max(grad.abs().max().item(), 1e-20)
    bwd = (grad32.double() - grad).abs().max().item() / scale if grad.numel() else 0.0
    return dict(normal=n.detach(), valid=valid, grad=grad, restated=fwd, restated_bwd=bwd, same_valid=bool((valid == valid32).all()))

"""CPU checks of the camera gradients (include/msgs.h msgs_backward_with_camera):
- the C entry and its scratch query are declared, exported and listed, ABI unchanged;
- host/camera_pose.posed_camera reproduces the camera at a zero twist and its Jacobian matches central differences;
- the float64 torch oracle's camera gradients (autograd through float64 viewmatrix / projmatrix / campos leaves), which the
  GPU tests hold the kernels to, match central finite differences on a tiny scene."""
import math
import os
import re

import numpy as np
import torch

import scenes
from oracle import torch_oracle as to

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("msgs_backward_with_camera", "msgs_camera_grad_scratch_bytes")


def test_header_declares_camera_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msgs.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), n


def test_library_exports_and_lists_them():
    import diff_gaussian_rasterization as dgr
    for n in NEW:
        assert hasattr(dgr._C.lib, n), n
        assert n in dgr._C.EXPORTS, n
    assert dgr._C.lib.msgs_abi_version() == 11


def test_camera_scratch_query_is_monotone():
    import diff_gaussian_rasterization as dgr
    q = dgr._C.lib.msgs_camera_grad_scratch_bytes
    sizes = [q(P) for P in (0, 1, 255, 256, 257, 1000, 100_000, 1_000_000, 5_000_000)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), sizes
    assert q(1_000_000) >= 8 * 27 * (1_000_000 // 256)          # one row of 27 doubles per workgroup of 256 Gaussians
    assert all(s % 256 == 0 and s > 0 for s in sizes)


def _cam64(cam):
    out = scenes.Camera(cam.image_width, cam.image_height, cam.FoVx, cam.FoVy, cam.world_view_transform.double(),
                        cam.full_proj_transform.double(), cam.camera_center.double(), cam.znear, cam.zfar)
    return out


def _tilted_camera(W=64, H=48):
    a = 0.3
    R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    return scenes.make_camera(R, np.array([0.2, -0.1, 0.5]), 1.0, 0.8, W, H)


def test_posed_camera_zero_twist_and_jacobian():
    from camera_pose import posed_camera
    cam = _tilted_camera()
    same = posed_camera(cam, torch.zeros(6, dtype=torch.float64))
    for n in ("world_view_transform", "full_proj_transform", "camera_center"):
        a, b = getattr(same, n), getattr(cam, n)
        assert a.dtype == b.dtype and a.shape == b.shape, n
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-6), (n, (a - b).abs().max().item())
    c64 = _cam64(cam)
    tw = torch.tensor([0.01, -0.02, 0.015, 0.05, -0.03, 0.02], dtype=torch.float64)

    def f(t):
        c = posed_camera(c64, t)
        return torch.cat([c.world_view_transform.reshape(-1), c.full_proj_transform.reshape(-1), c.camera_center])
    J = torch.autograd.functional.jacobian(f, tw)
    eps = 1e-6
    for i in range(6):
        e = torch.zeros(6, dtype=torch.float64)
        e[i] = eps
        fd = (f(tw + e) - f(tw - e)) / (2 * eps)
        assert torch.allclose(J[:, i], fd, rtol=1e-6, atol=1e-8), (i, (J[:, i] - fd).abs().max().item())
    # the twist moves the camera centre as the pose says: a pure translation v in camera axes moves it by -R^T v
    c = posed_camera(c64, torch.tensor([0.0, 0.0, 0.0, 0.1, 0.0, 0.0], dtype=torch.float64))
    R = c64.world_view_transform[:3, :3]             # = W2C rotation transposed
    assert torch.allclose(c.camera_center - c64.camera_center, -(R @ torch.tensor([0.1, 0.0, 0.0], dtype=torch.float64)),
                          atol=1e-12)


def _tiny_scene(cam):
    """Gaussians well inside the view (the Q2 clamp of the EWA Jacobian, a reference convention that drops d tx_c / d t,
    is inactive) and in front of it"""
    sc = scenes.frustum_scene(200, 64, 48, seed=5, scale_k=0.004 * 1920.0 / 64 * 2.0)
    V = cam.world_view_transform.to(torch.float64)
    t = torch.cat([sc.means3D.to(torch.float64), torch.ones(sc.P, 1, dtype=torch.float64)], 1) @ V
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    keep = (t[:, 2] > 1.0) & ((t[:, 0] / t[:, 2]).abs() < 0.8 * tx) & ((t[:, 1] / t[:, 2]).abs() < 0.8 * ty)
    idx = torch.nonzero(keep).view(-1)[:24]
    return sc.subset(idx)


def _oracle_loss(sc, cam, V, PM, cp, dL):
    view = to.view_dict(cam, sh_degree=sc.sh_degree)
    view["viewmatrix"], view["projmatrix"], view["campos"] = V, PM, cp
    dt = torch.float64
    color, _, _, _, _, aux = to.rasterize(sc.means3D.to(dt), sc.opacities.to(dt), view, torch.tensor([0.1, 0.2, 0.3]),
                                            scales=sc.scales.to(dt), rotations=sc.rotations.to(dt), shs=sc.shs.to(dt))
    return (color * dL).sum(), aux          # (the oracle's depth map is not differentiable: depth is checked on the GPU)


def test_oracle_camera_gradients_match_finite_differences():
    """the truth of the GPU tests: autograd through float64 camera leaves = central differences (all 35 entries)"""
    cam = _tilted_camera()
    sc = _tiny_scene(cam)
    dt = torch.float64
    dL = scenes.grad_seed(64, 48, 3).to(dt)
    base = [cam.world_view_transform.to(dt), cam.full_proj_transform.to(dt), cam.camera_center.to(dt)]
    with torch.no_grad():
        aux = _oracle_loss(sc, cam, *base, dL)[1]
    assert (aux["pre"]["radii"] > 0).sum() >= 10                 # enough rendered Gaussians to mean something
    dL = dL * (~aux["borderline"]).to(dt)                         # no weight on pixels with an alpha decision near a flip
    leaves = [b.clone().requires_grad_(True) for b in base]
    loss, aux = _oracle_loss(sc, cam, *leaves, dL)
    loss.backward()
    eps = 1e-6
    for t, (b, leaf) in enumerate(zip(base, leaves)):
        g = leaf.grad.reshape(-1)
        fd = torch.zeros_like(g)
        for k in range(g.numel()):
            args_p = [x.clone() for x in base]
            args_m = [x.clone() for x in base]
            args_p[t].view(-1)[k] += eps
            args_m[t].view(-1)[k] -= eps
            with torch.no_grad():
                fd[k] = (_oracle_loss(sc, cam, *args_p, dL)[0] - _oracle_loss(sc, cam, *args_m, dL)[0]) / (2 * eps)
        scale = g.abs().max().item()
        assert scale > 0, t
        err = (g - fd).abs().max().item()
        assert err <= 1e-5 * scale, (t, err, scale)
        if t == 0:
            assert torch.all(g.view(4, 4)[:, 3] == 0)                # column 3 of V never enters
        if t == 1:
            assert torch.all(g.view(4, 4)[:, 2] == 0)                # column 2 of PM never enters

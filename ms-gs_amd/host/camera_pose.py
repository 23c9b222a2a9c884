"""Differentiable camera pose for pose refinement.

posed_camera(cam, twist) returns a copy of a reference-style camera (world_view_transform, full_proj_transform,
camera_center; row-vector convention, world_view_transform = W2C^T) whose world-to-camera transform is

    W2C' = exp(hat(twist)) W2C,      twist = (omega, v): rotation vector omega [3], translation v [3] (camera frame),

and whose three tensors are differentiable functions of the twist.  The projection matrix is recovered once from the
original camera (full = world_view_transform @ proj) and kept.  render() and render_fused() forward the three tensors
into the rasterizer settings, where the camera gradients reach them (msgs_backward_with_camera)::

    twist = torch.zeros(6, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([twist], lr=1e-3)
    loss = l1(render(posed_camera(cam, twist), pc, pipe, bg)["render"], gt)
    loss.backward(); opt.step()
"""
import copy

import torch


def _hat(twist):
    w, v = twist[:3], twist[3:]
    z = torch.zeros((), dtype=twist.dtype, device=twist.device)
    return torch.stack([torch.stack([z, -w[2], w[1], v[0]]),
                        torch.stack([w[2], z, -w[0], v[1]]),
                        torch.stack([-w[1], w[0], z, v[2]]),
                        torch.stack([z, z, z, z])])


def projection_of(cam):
    """proj with full_proj_transform = world_view_transform @ proj (float64, no gradient)"""
    wvt = cam.world_view_transform.detach().to(torch.float64)
    return torch.linalg.solve(wvt, cam.full_proj_transform.detach().to(torch.float64))


def posed_camera(cam, twist, proj=None):
    """A copy of `cam` moved by the se(3) twist (6-vector, any float dtype, on the camera's device).  proj: the
    projection matrix (projection_of(cam)) when the caller has it already."""
    if twist.shape != (6,):
        raise ValueError(f"twist must have shape (6,), got {tuple(twist.shape)}")
    dt, dev = cam.world_view_transform.dtype, cam.world_view_transform.device
    if proj is None:
        proj = projection_of(cam)
    w2c = cam.world_view_transform.detach().to(twist.device, twist.dtype).transpose(0, 1)
    w2c_new = torch.linalg.matrix_exp(_hat(twist)) @ w2c
    wvt = w2c_new.transpose(0, 1)
    full = wvt @ proj.to(twist.device, twist.dtype)
    # camera centre: -R^T t of the new W2C (= inverse(wvt)[3, :3])
    center = -(w2c_new[:3, :3].transpose(0, 1) @ w2c_new[:3, 3])
    out = copy.copy(cam)
    out.world_view_transform = wvt.to(dev, dt)
    out.full_proj_transform = full.to(dev, dt)
    out.camera_center = center.to(dev, dt)
    return out

"""The float64 reference of the getter backward itself (parity_utils.leaf_space), pinned against the closed forms of
torch's F.normalize = x / x.norm().clamp_min(eps): below the clamp the norm passes no gradient (dL/draw = g / eps), at and
above it the gradient is the projection (g - q (q.g)) / ||raw||.  tests/test_activation_edges_gpu.py measures the kernels
against this reference; if torch's normalize semantics change, this test shows it."""
import types

import numpy as np
import torch

from parity_utils import NORMALIZE_EPS_F32, leaf_space


def test_normalize_eps_is_the_float32_clamp():
    assert NORMALIZE_EPS_F32 == float(np.float32(1e-12)) and NORMALIZE_EPS_F32 < 1e-12


def test_leaf_space_rotation_gradient_at_the_normalize_clamp():
    eps = NORMALIZE_EPS_F32
    below = float(np.nextafter(np.float32(eps), np.float32(0)))
    raw = torch.tensor([[3e-13, 4e-13, 0.0, 0.0], [below, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0],
                        [eps, 0.0, 0.0, 0.0], [0.0, -eps, 0.0, 0.0], [1e-9, 2e-9, -2e-9, 4e-9], [0.5, -1.5, 2.0, 1.0],
                        [1e9, 0.0, 3e9, 0.0]], dtype=torch.float32)
    P = raw.shape[0]
    g = torch.tensor([[1.0, 2.0, 3.0, 4.0]] * P, dtype=torch.float64) * torch.arange(1, P + 1, dtype=torch.float64)[:, None]
    pc = types.SimpleNamespace(_xyz=types.SimpleNamespace(grad=None), _opacity=torch.zeros(P, 1),
                               _scaling=torch.zeros(P, 3), _rotation=raw)
    og = dict(means3D=torch.zeros(P, 3), opacities=torch.zeros(P, 1), scales=torch.zeros(P, 3), rotations=g,
              means2D=torch.zeros(P, 3))
    ref = leaf_space(pc, None, og)["rotation"][1]
    x = raw.double()
    n = x.norm(dim=1, keepdim=True)
    clamped = (n < eps).flatten()
    assert clamped.tolist() == [True, True, True, False, False, False, False, False]
    assert torch.equal(ref[clamped], g[clamped] / eps)                 # no projection below the clamp
    q = x / n
    proj = (g - q * (q * g).sum(dim=1, keepdim=True)) / n
    d = (ref - proj).abs().max(dim=1).values[~clamped]
    assert (d <= 1e-12 * proj.abs().max(dim=1).values[~clamped]).all(), d      # the projection, to rounding of its own size
    # the issue's worked example: raw (3e-13, 4e-13, 0, 0), g (1, 2, 3, 4) -> (1, 2, 3, 4) / eps, not (0.64, 1.52, 3, 4) / eps
    assert torch.allclose(ref[0] * eps, torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64), rtol=1e-15)
    assert abs(proj[0, 0].item() * eps - 1.0) > 0.3

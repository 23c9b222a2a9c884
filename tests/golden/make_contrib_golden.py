"""Generates tests/golden/contrib_truth.npz: the float64 truth of the per-Gaussian contribution scores (DESIGN.md SPEC M11) on
scene F, independent of the op:
    python tests/golden/make_contrib_golden.py        (CPU only, a few seconds)

oracle/torch_oracle.rasterize takes a `colors_precomp` leaf; with zero colours and a zero background the red channel of pixel p
is sum_i w_ip c_i0, so ONE batched autograd.grad of the red channel over the pixels is the whole matrix w[p, i] = alpha_ip T_ip
of the blended pairs (and exactly 0 elsewhere: the smallest positive weight of scene F is 8.1e-7, so w > 0 marks the blended
pairs).  From it, per Gaussian: sum, max and count over the pixels, once with the weight map `m_plain` (1 everywhere) and once
with the seeded non-negative `m_weighted`.  Both maps are ZERO on the pixels the oracle flags as borderline (an alpha or a
transmittance within rounding of a threshold): the test hands the same maps to the op, so those pixels count on neither side.

tests/test_contrib_cpu.py imports compute() and pins the committed file to it."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

W, H, P, SCENE_SEED, MAP_SEED = 40, 24, 200, 1, 81
PLAIN = dict(filter_small=False, filter_large=False, fade_size=1.0)
MAX_BORDERLINE = 0.02          # of the image's pixels (the cap of make_absgrad_golden.py)
PATH = os.path.join(HERE, "contrib_truth.npz")


def scene_f():
    """(scene, camera) of scene F (make_absgrad_golden.py)"""
    from parity_utils import small_scene
    return small_scene(P, W, H, seed=SCENE_SEED)


def weight_map():
    """[H,W] float32, seeded: a quarter of the pixels 0, the others uniform in (0.25, 2.25)"""
    g = torch.Generator().manual_seed(MAP_SEED)
    m = 0.25 + 2.0 * torch.rand(H, W, generator=g)
    return torch.where(torch.rand(H, W, generator=g) < 0.25, torch.zeros(H, W), m)


def compute():
    """dict: sum_* / max_* [P] float64 and count_* [P] int64 for * in (plain, weighted); m_plain, m_weighted [H,W] float32 (zero
    on borderline pixels); borderline [H,W] bool; visible [P] bool; alpha [H,W] float64 = 1 - final_T"""
    from oracle import torch_oracle as to
    sc, cam = scene_f()
    dt = torch.float64
    view = to.view_dict(cam, sh_degree=sc.sh_degree, **PLAIN)
    col = torch.zeros(P, 3, dtype=dt, requires_grad=True)
    kw = dict(max_pixel_sizes=sc.max_pixel_sizes, min_pixel_sizes=sc.min_pixel_sizes, base_mask=sc.base_mask,
              scales=sc.scales.to(dt), rotations=sc.rotations.to(dt), colors_precomp=col)
    color, _, _, radii, _, aux = to.rasterize(sc.means3D.to(dt), sc.opacities.to(dt), view, torch.zeros(3), **kw)
    N = W * H
    g, = torch.autograd.grad(color[0].reshape(-1), col, grad_outputs=torch.eye(N, dtype=dt), is_grads_batched=True)
    w = g[:, :, 0]                                                          # [N, P]
    borderline = aux["borderline"]
    assert borderline.sum().item() <= MAX_BORDERLINE * N, "too many borderline pixels for this fixture"
    alpha = 1.0 - aux["final_T"].to(dt)
    assert (w.sum(1) - alpha.reshape(-1)).abs().max().item() <= 1e-12      # the weights of a pixel add up to its alpha
    assert int((w > 0).sum()) == int(aux["n_blended"].sum())                # and w > 0 marks exactly the blended pairs
    keep = (~borderline).to(torch.float32)
    out = dict(borderline=borderline.numpy(), visible=(radii > 0).numpy(), alpha=alpha.numpy())
    for name, m in (("plain", keep), ("weighted", weight_map() * keep)):
        md = m.to(dt).reshape(-1, 1)
        t = w * md
        out["m_" + name] = m.numpy()
        out["sum_" + name] = t.sum(0).numpy()
        out["max_" + name] = t.max(0).values.numpy()
        out["count_" + name] = ((w > 0) & (md > 0)).sum(0).numpy().astype(np.int64)
    return out


if __name__ == "__main__":
    out = compute()
    np.savez(PATH, **out)
    for name in ("plain", "weighted"):
        c = out["count_" + name]
        print(f"{name}: visible {int(out['visible'].sum())}  counted > 0: {int((c > 0).sum())}  pairs {int(c.sum())}  "
              f"sum of sums {out['sum_' + name].sum():.6g}  largest max {out['max_' + name].max():.6g}  "
              f"pixels with weight 0: {int((out['m_' + name] == 0).sum())}")
    print(f"borderline pixels {int(out['borderline'].sum())} of {W * H}")

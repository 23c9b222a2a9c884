"""Generates tests/golden/contrib_truth.npz: the float64 truth of the per-Gaussian contribution scores (DESIGN.md SPEC M11) on
scene F, independent of the op:
    python tests/golden/make_contrib_golden.py        (CPU only, a few seconds)

tests/replay_truth.render restates the blend loop of oracle/torch_oracle.rasterize and keeps, per tile, the matrix w[i, p] =
alpha_ip T_ip of the blended pairs (exactly 0 elsewhere) with the mask of the blended pairs.  From it (replay_truth.contributions),
per Gaussian: sum, max and count over the pixels, once with the weight map `m_plain` (1 everywhere) and once
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
import replay_truth as rt                        # noqa: E402  (tests/ is on the path now)
from replay_truth import MAX_BORDERLINE          # noqa: E402  (of the image's pixels)

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
    sc, cam = scene_f()
    r = rt.render(sc, cam, PLAIN)
    N = W * H
    borderline = r.borderline
    assert borderline.sum().item() <= MAX_BORDERLINE * N, "too many borderline pixels for this fixture"
    keep = (~borderline).to(torch.float32)
    out = dict(borderline=borderline.numpy(), visible=(r.radii > 0).numpy(), alpha=r.alpha.detach().numpy())
    for name, m in (("plain", keep), ("weighted", weight_map() * keep)):
        s, mx, cnt = rt.contributions(r, m)
        out["m_" + name] = m.numpy()
        out["sum_" + name] = s.numpy()
        out["max_" + name] = mx.numpy()
        out["count_" + name] = cnt.numpy().astype(np.int64)
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

"""Both routes of tests/test_alpha_grad_gpu.py::test_alpha_gradient_equals_colour_route — the alpha loss (sum G alpha) and the
colour route (override_color = [1, 0, 0], bg = 0, sum G render[0]) — against float64, per gradient tensor (max-norm relative
error on the Gaussians neither oracle build flags), next to the float32 oracle's own distance and the alpha-vs-colour difference
the test asserts.  Scene A against oracle/torch_oracle.py (float64 autograd), the slab and occlusion scenes on all four backward
routes against the float64 build of the C++ oracle.  The figures behind ROUTE_CEILINGS of that test and profiles/alpha_notes.md
(not a test; needs a GPU).

    python tools/alpha_route_truth.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ms-gs_amd"), os.path.join(ROOT, "ms-gs_amd", "host"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import test_alpha_grad_gpu as T
from parity_utils import leaf_space, rel_err
from oracle import oracle_ctypes as oc, torch_oracle as to

def measure(kind, route, use_torch):
    sc, cam, st, smod, pipe, env = T._scene(kind)
    w, h = cam.image_width, cam.image_height
    Ga = T._seeds(w, h)[2]
    bg = torch.zeros(3)
    T._set_route(route)
    with T._env(env):
        outA, gA = T._run(sc, cam, st, smod, pipe, bg, Ga=Ga, env=env); pcA = T._run.last_pc
        outB, gB = T._run(sc, cam, st, smod, pipe, bg, Ga=Ga, colour_one=True, env=env); pcB = T._run.last_pc
    T._set_route("default")
    seen = T._seen(sc, pcA)
    Gc = Ga.cpu()
    o32, o64, _, _ = T._oracles_colour_one(seen, cam, st)
    flagged = o32.borderline_gaussians | o64.borderline_gaussians | (o32.radii != o64.radii)
    dl = torch.stack([Gc, torch.zeros_like(Gc), torch.zeros_like(Gc)], 0)
    if use_torch:
        dt = torch.float64
        leaf = lambda t: t.detach().to(dt).clone().requires_grad_(True)
        m3, op, s_, r_ = leaf(seen.means3D), leaf(seen.opacities), leaf(seen.scales), leaf(seen.rotations)
        view = to.view_dict(cam, sh_degree=seen.sh_degree, scale_modifier=smod, **st)
        color, _, _, _, _, aux = to.rasterize(m3, op, view, torch.zeros(3, dtype=dt), scales=s_, rotations=r_,
                                              colors_precomp=torch.ones(seen.P, 3, dtype=dt), max_pixel_sizes=seen.max_pixel_sizes,
                                              min_pixel_sizes=seen.min_pixel_sizes, base_mask=seen.base_mask)
        (color[0] * Gc.to(dt)).sum().backward()
        g2 = aux["means2D"].grad
        m2t = torch.zeros(seen.P, 3, dtype=dt); m2t[:, 0], m2t[:, 1] = g2[:, 0] * 0.5 * w, g2[:, 1] * 0.5 * h
        truth = dict(means3D=m3.grad, opacities=op.grad, scales=s_.grad, rotations=r_.grad, means2D=m2t)
    else:
        truth = dict(oc.backward(o64, dl)); truth.pop("colors_precomp", None)
    o32g = dict(oc.backward(o32, dl)); o32g.pop("colors_precomp", None)
    la = leaf_space(pcA, outA["viewspace_points"].grad, truth)
    lb = leaf_space(pcB, outB["viewspace_points"].grad, truth)
    lo = leaf_space(pcA, outA["viewspace_points"].grad, o32g)
    print(f"== {kind}/{route} truth={'torch64' if use_torch else 'oracle64'} flagged {flagged.float().mean().item():.4f} P {seen.P}", flush=True)
    names = {"means3D": "xyz", "opacity": "opacity", "scaling": "scaling", "rotation": "rotation", "means2D": "viewspace"}
    for k in la:
        da, db = rel_err(la[k][0], la[k][1], ~flagged), rel_err(lb[k][0], lb[k][1], ~flagged)
        do = rel_err(lo[k][1], la[k][1], ~flagged)
        ab = T._rel(gA[names[k]], gB[names[k]])
        print(f"   {k:9s} alpha-route vs truth {da:.3e}   colour-route vs truth {db:.3e}   oracle32 vs truth {do:.3e}   alpha vs colour (all rows) {ab:.3e}   ok(<=1.25x) {da <= 1.25 * db}", flush=True)

measure("A", "default", True)
for kind in ("slab", "occlusion"):
    for route in T.ROUTES:
        measure(kind, route, False)

"""Where the dL/dscaling / dL/drotation residual of the full-size parity tests comes from — by test, not by prose.

(1) K8 + K9 ISOLATED: the HIP per-Gaussian backward (msgs_backward_per_gaussian: 2-D covariance backward, projection, SH,
    scale / quaternion chain) is fed the ORACLE's nine per-Gaussian 2-D sums — bit-identical inputs — and compared with the
    oracle's own K8 + K9 on every output tensor at C2 and C3.  If that agrees to ~1e-6, everything the full-size tests
    see on dL/dscaling and dL/drotation is the blend backward's per-pixel float32 rounding, multiplied by the conditioning
    of the conic -> covariance chain; K8/K9 themselves add nothing.
(2) dL/dcov3D through the precomputed-covariance entry at C2 and C3 (the same blend backward, the chain cut after the
    2-D -> 3-D covariance step): asserted at the north star's 1e-4 together with the other tensors of that entry.
(3) The amplification itself: the per-Gaussian map sums -> dL/dscaling is linear, so its sensitivity is measured directly by
    perturbing the oracle's sums by one float32 ulp-sized relative amount (1e-7) and reading the relative movement of the
    outputs: the printed factor is the condition number the floor document talks about.
"""
import math

import pytest
import torch

import scenes
from parity_utils import hip_render, rel_err, report
from per_gaussian_entry import per_gaussian_hip as _per_gaussian_hip, plain_call as _plain_call

pytestmark = pytest.mark.gpu

K8_RTOL = 1e-6            # measured 2e-8 on dL/dmeans3D, 0.0 (bit-equal) on the other five tensors at C2 and C3
COV_RTOL = 1e-4           # north star


@pytest.mark.parametrize("name", ["C2", "C3"])
def test_per_gaussian_backward_on_the_oracles_sums(name):
    import diff_gaussian_rasterization as dgr
    from oracle import oracle_ctypes as oc
    sc, cam, st = scenes.config(name)
    bg = torch.zeros(3)
    dL = scenes.grad_seed(cam.image_width, cam.image_height, 1 if name == "C2" else 2)
    _, pc, _ = hip_render(sc, cam, st, bg)                 # builds pc.seen: the activated tensors as the GPU evaluates them
    seen = pc.seen
    call = _plain_call(seen, cam, st, bg)
    with torch.no_grad():
        _, _, _, radii, _, (geom, _, _, _) = dgr._forward_impl(call)
    orc = oc.rasterize(seen, cam, st, bg)
    og = oc.backward(orc, dL, want_sums2d=True)
    assert torch.equal(radii.cpu(), orc.radii)
    got = _per_gaussian_hip(call, radii, geom, og["sums2d"])
    worst = {}
    for k in ("means3D", "means2D", "shs", "opacities", "scales", "rotations"):
        worst[k] = rel_err(got[k], og[k].reshape(got[k].shape))
        report(f"{name} K8+K9 isolated", k, worst[k])
    assert max(worst.values()) <= K8_RTOL, worst

    # (3) the conditioning of sums -> outputs: relative movement of each output per relative perturbation of the sums
    g = torch.Generator().manual_seed(5)
    eps = 1e-7
    pert = og["sums2d"] * (1.0 + eps * (2.0 * torch.rand(og["sums2d"].shape, generator=g, dtype=torch.float64) - 1.0))
    moved = _per_gaussian_hip(call, radii, geom, pert)
    for k in ("means3D", "opacities", "scales", "rotations"):
        report(f"{name} amplification (output rel movement / 1e-7 input rel perturbation)", k,
               rel_err(moved[k], got[k]) / eps)


@pytest.mark.parametrize("name", ["C2", "C3"])
def test_precomputed_covariance_entry_full_size(name):
    """render() with pipe.compute_cov3D_python (gaussian_renderer/__init__.py:68-72): the op receives cov3D_precomp and
    returns dL/dcov3D — the blend backward and the 2-D -> 3-D covariance step without the scale / quaternion tail."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from oracle import oracle_ctypes as oc
    from parity_utils import check_forward
    sc, cam, st = scenes.config(name)
    W, H = cam.image_width, cam.image_height
    bg = torch.zeros(3)
    dL = scenes.grad_seed(W, H, 1 if name == "C2" else 2)
    _, pc, _ = hip_render(sc, cam, st, bg)
    seen = pc.seen
    dev = "cuda"
    with torch.no_grad():
        cov = pc.get_covariance(1.0).detach()               # torch on the GPU, gaussian_model.py:33-37
    camd = cam.to(dev)
    rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5),
                                       tanfovy=math.tan(cam.FoVy * 0.5), bg=bg.to(dev), scale_modifier=1.0,
                                       viewmatrix=camd.world_view_transform, projmatrix=camd.full_proj_transform,
                                       sh_degree=seen.sh_degree, campos=camd.camera_center, prefiltered=False,
                                       debug=False, **st)
    t = lambda x: x.to(dev).contiguous().requires_grad_(True)
    means, opac, covd, shs = t(seen.means3D), t(seen.opacities), cov.clone().requires_grad_(True), t(seen.shs)
    m2 = torch.zeros(seen.P, 3, device=dev, requires_grad=True)
    img, aps, dep, radii, psz = GaussianRasterizer(rs)(
        means3D=means, means2D=m2, opacities=opac, shs=shs, cov3D_precomp=covd,
        max_pixel_sizes=seen.max_pixel_sizes.to(dev), min_pixel_sizes=seen.min_pixel_sizes.to(dev),
        base_mask=seen.base_mask.to(dev))
    (img * dL.to(dev)).sum().backward()
    orc = oc.rasterize(seen, cam, st, bg, use_cov_precomp=True, cov3D_precomp=cov.cpu())
    og = oc.backward(orc, dL)
    out = dict(render=img, acc_pixel_size=aps, depth=dep, radii=radii, visibility_filter=radii > 0, pixel_sizes=psz)
    check_forward(out, orc, f"{name} cov-precomp")
    clean = ~orc.borderline_gaussians
    for k, g, ref in (("means3D", means.grad, og["means3D"]), ("opacities", opac.grad, og["opacities"]),
                      ("shs", shs.grad, og["shs"]), ("cov3D", covd.grad, og["cov3D_precomp"]),
                      ("means2D", m2.grad, og["means2D"])):
        e = rel_err(g, ref.reshape(g.shape), clean)
        report(f"{name} cov-precomp", k, e)
        assert e <= COV_RTOL, (k, e)

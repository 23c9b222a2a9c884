"""The composed GPU training iteration (render_fused -> l1_ssim_loss -> backward -> statistics -> FusedAdam) against
the same iteration composed the reference's way (render + torch loss formulation, evaluated in float64 + torch.optim.Adam +
masked-index statistics), and a short optimisation run as the train-step harness of SURVEY §8(d)."""
import pytest
import torch
import torch.nn.functional as F

import scenes
from oracle import loss_oracle as lo
from parity_utils import PIPE, small_scene

pytestmark = pytest.mark.gpu


def _torch_loss(x, gt, lam):
    w = torch.from_numpy(lo.window_2d()).to(x.device, x.dtype).expand(3, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t, w, padding=5, groups=3)
    m1, m2 = conv(x), conv(gt)
    s1, s2, s12 = conv(x * x) - m1 * m1, conv(gt * gt) - m2 * m2, conv(x * gt) - m1 * m2
    S = ((2 * m1 * m2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((m1 * m1 + m2 * m2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return (1 - lam) * (x - gt).abs().mean() + lam * (1 - S.mean())


def _reference_style_iteration(model, opt, cam, gt, bg, lvl, st):
    from gaussian_renderer import render
    pkg = render(cam, model, PIPE, bg, **st)
    # the loss formula in float64.  On _scaling / _rotation the distance below is that of ONE Gaussian of this scene (index 1080,
    # radius 39 px), whose gradient responds to the pixel gradient in steps, as float32 accumulation of cancelling terms does: it moves
    # in steps of ~3e-5 of the largest entry and not at all in between (two pixel gradients 7e-7 apart give the same bits, 1000 x
    # their difference fed alone moves it by 1.6e-7).  Fed the float64 oracle's pixel gradient, it lands 2.0e-5 / 4.1e-5 from
    # where the float32 formulation puts it, as much as the tolerance; every other Gaussian agrees to 2.5e-6 either way
    # (profiles/loss_notes.md).  The truth is the reference that does not add a step of its own.
    loss = _torch_loss(pkg["render"].double(), gt.double(), 0.2)
    loss.backward()
    with torch.no_grad():
        vis, radii, ps = pkg["visibility_filter"], pkg["radii"], pkg["pixel_sizes"]
        mask = vis & (model.target_reso_lvl == lvl)
        if lvl > 0:
            model.max_pixel_sizes[mask] = torch.max(model.max_pixel_sizes[mask] * 0.95, ps[mask])
        if lvl < model.reso_lvls - 1:
            mn = torch.clip(model.min_pixel_sizes[mask] * 1.05, -1)
            model.min_pixel_sizes[mask] = torch.where(ps[mask] > 0, torch.where(mn < 0, ps[mask], torch.min(mn, ps[mask])), mn)
        model.max_radii2D[vis] = torch.max(model.max_radii2D[vis], radii[vis])
        model.xyz_gradient_accum[:, lvl][vis] += torch.norm(pkg["viewspace_points"].grad[vis, :2], dim=-1, keepdim=True)
        model.denom[:, lvl][vis] += 1
        opt.step()
        opt.zero_grad(set_to_none=True)
    return loss.detach(), pkg


def test_first_iteration_matches_the_reference_composition():
    from synthetic_model import SyntheticGaussians
    from train_epilogue import FusedAdam
    from train_step import fused_train_iteration
    W, H = 160, 128
    sc, cam = small_scene(6000, W, H, 21, multiscale=True, scale_k=0.004 * 1920.0 / W * 0.2)
    st = dict(filter_small=True, filter_large=True, fade_size=0.0)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    bg = torch.zeros(3).cuda()
    camd = cam.to("cuda")
    a, b = SyntheticGaussians(sc, "cuda"), SyntheticGaussians(sc, "cuda")
    ga = a.training_setup(7, sc.target_reso_lvl)
    gb = b.training_setup(7, sc.target_reso_lvl)
    oa, ob = FusedAdam(ga, lr=0.0, eps=1e-15), torch.optim.Adam(gb, lr=0.0, eps=1e-15)
    before = {n: getattr(a, n).detach().clone() for n in a.LEAVES}
    la, _, pa = fused_train_iteration(a, oa, camd, gt, PIPE, bg, **st)
    lb, pb = _reference_style_iteration(b, ob, camd, gt, bg, 0, st)
    assert abs(la.item() - lb.item()) <= 1e-5
    assert torch.equal(pa["radii"], pb["radii"])
    for k in ("denom", "max_radii2D"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for k in ("max_pixel_sizes", "min_pixel_sizes"):       # pixel sizes: in-kernel expf vs torch.exp, 1 ulp apart
        assert torch.allclose(getattr(a, k), getattr(b, k), rtol=1e-5, atol=0), k
    ref = b.xyz_gradient_accum
    e = (a.xyz_gradient_accum - ref).abs().max().item() / ref.abs().max().item()
    print(f"[parity] train step xyz_gradient_accum: {e:.3e}")
    assert e <= 5e-6                 # measured 4.1e-7
    # first Adam step = -lr * g / (|g| + eps): +-lr wherever the gradient is not ~0.  Compare the moments (linear in
    # the gradient) for every Gaussian, and the parameters where the gradient is well above the float-atomic noise.
    for (n, ga_, gb_) in zip(a.LEAVES, ga, gb):
        p, q = ga_["params"][0], gb_["params"][0]
        ma, mb = oa.state[p]["exp_avg"], ob.state[q]["exp_avg"]
        e = (ma - mb).abs().max().item() / mb.abs().max().item()
        print(f"[parity] train step exp_avg {n}: {e:.3e}")
        assert e <= (5e-5 if n in ("_scaling", "_rotation") else 5e-6), n      # measured 1.8e-5 / 2.7e-5 / <= 4.0e-7
        sure = mb.abs() > 1e-3 * mb.abs().max()
        assert sure.any()
        step_a, step_b = (p - before[n])[sure], (q - before[n])[sure]
        assert (step_a - step_b).abs().max().item() <= 1e-3 * step_b.abs().max().item(), n


def test_short_run_reduces_the_loss():
    """Fit a fixed target (a render of a perturbed copy of the scene) for 30 iterations."""
    from gaussian_renderer import render
    from synthetic_model import SyntheticGaussians
    from train_epilogue import FusedAdam
    from train_step import fused_train_iteration
    W, H = 192, 128
    sc, cam = small_scene(8000, W, H, 33)
    bg = torch.zeros(3).cuda()
    camd = cam.to("cuda")
    with torch.no_grad():
        target = render(camd, SyntheticGaussians(sc, "cuda", requires_grad=False), PIPE, bg)["render"].clone()
    g = torch.Generator().manual_seed(4)
    sc.shs = sc.shs + 0.3 * torch.randn(sc.shs.shape, generator=g)
    sc.means3D = sc.means3D + 0.01 * torch.randn(sc.means3D.shape, generator=g)
    model = SyntheticGaussians(sc, "cuda")
    opt = FusedAdam(model.training_setup(1), lr=0.0, eps=1e-15)
    losses = []
    for it in range(30):
        loss, l1, pkg = fused_train_iteration(model, opt, camd, target, PIPE, bg)
        losses.append(loss.item())
    assert all(torch.isfinite(p).all() for p in model.parameters())
    assert losses[-1] < 0.6 * losses[0], losses
    assert model.denom.sum().item() > 0 and model.max_radii2D.max().item() > 0


def test_multi_view_iteration_equals_the_serial_composition():
    """train_step.fused_train_iteration_views (two views in flight, gradients summed in the kernel, statistics in view order, one
    Adam step) against the same iteration composed serially from the same pieces: parameters, optimizer moments and every
    statistic bit for bit, over three optimizer steps of four views"""
    from gaussian_renderer import render_fused
    from loss_utils import l1_ssim_loss
    from multi_view import ViewPipeline
    from synthetic_model import SyntheticGaussians
    from train_epilogue import FusedAdam, update_training_stats
    from train_step import fused_train_iteration_views
    W, H, V = 200, 128, 4
    sc = scenes.ball_scene(30000, seed=12, log_s=-3.2)
    cams = [scenes.ring_camera(v, 8, W, H).to("cuda") for v in range(V)]
    gts = [torch.rand(3, H, W, generator=torch.Generator().manual_seed(50 + v)).cuda() for v in range(V)]
    bg = torch.zeros(3).cuda()
    st = dict(filter_small=False, filter_large=False, fade_size=1.0)
    a, b = SyntheticGaussians(sc, "cuda"), SyntheticGaussians(sc, "cuda")
    oa = FusedAdam(a.training_setup(1), lr=0.0, eps=1e-15)
    ob = FusedAdam(b.training_setup(1), lr=0.0, eps=1e-15)
    pipe2 = ViewPipeline("cuda")
    for it in range(3):
        la, _ = fused_train_iteration_views(a, oa, pipe2, cams, gts, PIPE, bg, **st)
        lb = []
        for c, g in zip(cams, gts):                   # the serial composition
            pkg = render_fused(c, b, PIPE, bg, **st)
            loss, _ = l1_ssim_loss(pkg["render"], g, 0.2)
            loss.backward()
            lb.append(loss.detach())
            with torch.no_grad():
                update_training_stats(b, pkg["viewspace_points"], pkg["radii"], pkg["pixel_sizes"], 0)
        with torch.no_grad():
            ob.step()
            ob.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        assert torch.equal(la, torch.stack(lb)), it
        for n in a.LEAVES:
            assert torch.equal(getattr(a, n), getattr(b, n)), (it, n)
        for k in ("xyz_gradient_accum", "denom", "max_radii2D", "max_pixel_sizes", "min_pixel_sizes"):
            assert torch.equal(getattr(a, k), getattr(b, k)), (it, k)
    for (ga_, gb_) in zip(oa.param_groups, ob.param_groups):
        pa, pb = ga_["params"][0], gb_["params"][0]
        assert torch.equal(oa.state[pa]["exp_avg"], ob.state[pb]["exp_avg"])
        assert torch.equal(oa.state[pa]["exp_avg_sq"], ob.state[pb]["exp_avg_sq"])


@pytest.mark.parametrize("deg", [3, 1])
def test_the_step_inside_the_backward_gives_the_same_bits_as_backward_plus_optimizer(deg):
    """fused_train_iteration(step_in_backward=True): the per-Gaussian backward kernel applies the Adam update itself
    (include/msgs.h, msgs_adam_in_backward_t) — parameters, both moments, the statistics and the losses of a 12-iteration run
    are BIT-identical to the default composition (gradient tensors written by the backward, read by FusedAdam.step), with a
    model whose size is not a multiple of the kernel's 32-row runs, filters on, an active SH degree below the stored one."""
    from synthetic_model import SyntheticGaussians
    from train_epilogue import FusedAdam
    from train_step import fused_train_iteration
    W, H = 160, 128
    sc, cam = small_scene(6007, W, H, 23, multiscale=True, scale_k=0.004 * 1920.0 / W * 0.2, sh_degree=deg)
    st = dict(filter_small=True, filter_large=True, fade_size=0.0)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(2)).cuda()
    bg = torch.zeros(3).cuda()
    camd = cam.to("cuda")
    a, b = SyntheticGaussians(sc, "cuda"), SyntheticGaussians(sc, "cuda")
    oa = FusedAdam(a.training_setup(7, sc.target_reso_lvl), lr=0.0, eps=1e-15)
    ob = FusedAdam(b.training_setup(7, sc.target_reso_lvl), lr=0.0, eps=1e-15)
    for it in range(12):
        la, _, pa = fused_train_iteration(a, oa, camd, gt, PIPE, bg, step_in_backward=True, **st)
        lb, _, pb = fused_train_iteration(b, ob, camd, gt, PIPE, bg, **st)
        assert all(getattr(a, n).grad is None for n in a.LEAVES)           # no gradient tensors were formed
        assert torch.equal(la, lb), it
        assert torch.equal(pa["render"], pb["render"]) and torch.equal(pa["radii"], pb["radii"])
    assert (pa["radii"] == 0).any() and (pa["radii"] > 0).any()            # rendered and unrendered rows both took the step
    for n in a.LEAVES:
        p, q = getattr(a, n), getattr(b, n)
        assert torch.equal(p, q), n
        sa, sb = oa.state[p], ob.state[q]
        assert sa["step"].item() == sb["step"].item() == 12
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), n
        assert sa["exp_avg"].abs().max().item() > 0
    for k in ("denom", "max_radii2D", "max_pixel_sizes", "min_pixel_sizes", "xyz_gradient_accum"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_the_step_inside_the_backward_refuses_what_it_cannot_serve():
    import diff_gaussian_rasterization as dgr
    from gaussian_renderer import render_fused
    from synthetic_model import SyntheticGaussians
    from train_epilogue import FusedAdam
    W, H = 96, 64
    sc, cam = small_scene(500, W, H, 5)
    camd, bg = cam.to("cuda"), torch.zeros(3).cuda()
    model = SyntheticGaussians(sc, "cuda")
    opt = FusedAdam(model.training_setup(1), lr=0.0, eps=1e-15)
    other = FusedAdam([{"params": [torch.nn.Parameter(torch.zeros(4, device="cuda"))], "lr": 0.1, "name": "x"}], lr=0.0, eps=1e-15)
    prev = dgr.set_optimizer_in_backward(other)            # an optimizer that does not own the model's tensors
    try:
        out = render_fused(camd, model, PIPE, bg)["render"].sum()
    finally:
        assert dgr.set_optimizer_in_backward(prev) is other
    with pytest.raises(ValueError, match="not a parameter of this optimizer"):
        out.backward()
    model._xyz.grad = torch.zeros_like(model._xyz)         # a pending .grad would be ignored by the step: refused
    dgr.set_optimizer_in_backward(opt)
    try:
        out = render_fused(camd, model, PIPE, bg)["render"].sum()
    finally:
        dgr.set_optimizer_in_backward(None)
    with pytest.raises(RuntimeError, match="already holds a .grad"):
        out.backward()
    assert getattr(opt, "steps_in_backward", 0) == 0 and len(opt.state) == 0

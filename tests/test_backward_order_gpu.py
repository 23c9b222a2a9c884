"""The order of the Python op's launch sequence with EVERY opt-in on at once (M9 alpha and background gradient, M10
absgrad, M12 features, M13 distortion, M15 median depth), through each of the three entries: plain forward() with the getter
chain switched off, chained forward(), forward_raw().  The suites of the single opt-ins check the numbers against their own
truths; this one pins what they do not name — the order of the shared sequence:
  forward   distortion, median, features replays (_forward_tail)
  backward  msgs_features_backward, msgs_distortion_backward, msgs_median_depth_backward, the main backward, msgs_bg_grad,
            msgs_absgrad
The main backward is recorded by pass-through wrappers on BOTH module globals _run_backward chooses between: a loss that uses the
alpha map leaves through _call_backward_with_alpha, any other through _call_backward.  No numerical closeness is asserted."""
import pytest
import torch

import diff_gaussian_rasterization as dgr
import scenes
from parity_utils import PIPE, small_scene
from route_utils import PLAIN
from synthetic_model import SyntheticGaussians

pytestmark = pytest.mark.gpu

W, H, P, CH = 48, 32, 200, 5         # 3 x 2 tiles of 16 x 16 pixels; C = 5 is no multiple of 4
ENTRIES = {"plain": "_RasterizeGaussiansBackward", "chained": "_RasterizeGaussiansChainedBackward",
           "raw": "_RasterizeGaussiansRawBackward"}
FORWARD = ["msgs_distortion_forward", "msgs_median_depth_forward", "msgs_features_forward"]
BACKWARD = ["msgs_features_backward", "msgs_distortion_backward", "msgs_median_depth_backward", "main backward", "msgs_bg_grad",
            "msgs_absgrad"]


def _seed(seed, *shape):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) - 0.5).cuda()


@pytest.fixture(scope="module")
def case():
    sc, cam = small_scene(P, W, H, seed=211)
    seeds = (scenes.grad_seed(W, H, 212).cuda(), _seed(213, H, W), _seed(214, H, W), _seed(215, H, W), _seed(216, H, W),
             _seed(217, CH, H, W))
    return sc, cam.to("cuda"), torch.rand(P, CH, generator=torch.Generator().manual_seed(218)), seeds


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_everything_on_runs_in_the_pinned_order(entry, case, monkeypatch):
    from gaussian_renderer import _colour_inputs, _settings, _shape_inputs
    sc, cam, feats, seeds = case
    calls = []
    for probe in ("_features_probe", "_distortion_probe", "_median_probe"):
        monkeypatch.setattr(dgr, probe, calls.append)
    for name in ("_call_backward", "_call_backward_with_alpha"):
        fn = getattr(dgr, name)
        monkeypatch.setattr(dgr, name, lambda *a, _fn=fn, **kw: (calls.append("main backward"), _fn(*a, **kw))[1])
    for name in ("msgs_bg_grad", "msgs_absgrad"):
        fn = getattr(dgr._C.lib, name)
        monkeypatch.setattr(dgr._C.lib, name, lambda *a, _fn=fn, _n=name: (calls.append(_n), _fn(*a))[1])
    monkeypatch.setattr(dgr, "chain_reference_getters", entry == "chained")

    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    f = feats.cuda().requires_grad_(True)
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda", requires_grad=True)
    settings = _settings(cam, pc, PIPE, bg, 1.0, PLAIN["filter_small"], PLAIN["filter_large"], PLAIN["fade_size"])
    r = dgr.GaussianRasterizer(settings, return_alpha=True, absgrad=True).with_features(f).with_distortion().with_median_depth()
    vs = torch.zeros_like(pc._xyz, requires_grad=True)
    kw = dict(max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes,
              occ_multiplier=pc.get_occ_multiplier, dc_delta=pc.get_dc_delta, base_mask=pc.get_base_mask)
    if entry == "raw":
        outs = r.forward_raw(pc._xyz, vs, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation, **kw)
    else:
        outs = r(means3D=pc.get_xyz, means2D=vs, opacities=pc.get_opacity, **kw, **_colour_inputs(cam, pc, PIPE, None),
                 **_shape_inputs(pc, PIPE, 1.0))
    assert len(outs) == 10 and type(outs[0].grad_fn).__name__ == ENTRIES[entry]
    assert calls == FORWARD, calls
    assert (outs[3] > 0).any()                                    # something was rendered: no pre-pass is skipped
    image, _, depth, _, _, alpha, distortion, median_depth, median_id, fmap = outs
    assert fmap.shape == (CH, H, W) and not median_id.requires_grad
    del calls[:]
    # every differentiable map: colour, depth, alpha, distortion, median depth, features
    loss = sum((m * g).sum() for m, g in zip((image, depth, alpha, distortion, median_depth, fmap), seeds))
    loss.backward()
    torch.cuda.synchronize()
    assert calls == BACKWARD, calls

    assert torch.is_tensor(vs.absgrad) and vs.absgrad.shape == vs.shape and torch.isfinite(vs.absgrad).all()
    leaves = {"bg": bg, "features": f, "means2D": vs, "xyz": pc._xyz, "features_dc": pc._features_dc,
              "features_rest": pc._features_rest, "opacity": pc._opacity, "scaling": pc._scaling, "rotation": pc._rotation}
    for name, t in leaves.items():
        assert t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad).all(), name

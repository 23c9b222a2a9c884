"""The opt-in blend replays (alpha map, absgrad, contribution scores, feature channels, depth distortion, median depth / id:
DESIGN.md 4.9-4.13, 4.15) swept against a float64 truth that is not made of this library: tests/replay_truth.py (oracle/
torch_oracle.preprocess + the restated blend loop + the definitions + autograd) on the seeded cases of tests/replay_cases.py —
tile lists of two and three 256-entry batches, early termination inside lists of 1400, the multi-scale filters with a fade, rigid
poses, focal lengths 0.6 / 1.7, the scaling modifier, precomputed covariances, models of 1 / 7 / 63 / 64 / 65 rows, feature widths
1 / 8 / 9 / 17, a median crossing behind skipped entries.  tests/test_replay_sweep_cpu.py pins the truth to the committed fixtures
and to the oracle on every case and asserts the conditions of every masking used here.

  (a) all opt-ins of one call together, on the four backward routes, through the plain entry and forward_raw: every map, median_id
      exactly, every leaf gradient, dL/dfeatures and means2D.absgrad for ONE backward of the sum of the seeded maps;
  (b) each opt-in output alone on the haze, opaque and filter cases (the median also on the skipped-entry case), so that a failure
      of (a) names its replay;
  (c) GaussianRasterizer.contributions with a mask and with a seeded weight map: sums, maxima, exact counts.
Seeds are zero on the truth's borderline pixels (the median's also where a blended T is within 1e-4 of 1/2), which are left out of
the map comparisons too.  Tolerances are those of the truth tests on scene F (FWD_ATOL, BWD_RTOL of tests/parity_utils.py).  For
dL/dscaling, dL/drotation and dL/dmeans3D — the tensors behind K8's conic -> covariance map — a route that misses BWD_RTOL may
instead meet the project's three-way rule (parity_utils.check_against_truth): no farther from the truth than TRUTH_FACTOR x the
float32 evaluation of replay_truth on that case and tensor, + 1e-6; the allowance is measured on the reference, never on the
kernels, and its uses are counted.  The measured maxima are printed by the last test (pytest -s) and recorded in
profiles/replay_sweep_notes.md.  The precomputed-covariance case has no forward_raw form (that entry takes raw scales and rotations)."""
import collections
import types

import pytest
import torch

import diff_gaussian_rasterization as dgr
import replay_cases as rc
from parity_utils import BWD_RTOL, FWD_ATOL, PIPE, TRUTH_FACTOR, check_backward, leaf_space, rel_err
from synthetic_model import SyntheticGaussians
from test_depth_grad_gpu import ROUTES

pytestmark = pytest.mark.gpu

PIPE_COV = types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=True, debug=False)
K8_TENSORS = ("scaling", "rotation", "means3D")      # dL/dmeans3D takes a term through the same K8 map
ALL = rc.OUTPUTS
MAXIMA = collections.defaultdict(float)               # quantity -> the largest measured error of the session
ALLOWANCE = []                                         # (test, tensor, HIP distance, float32 distance) that needed the three-way rule
ENTRIES = [(n, fused) for n in rc.CASES for fused in (False, True) if not (fused and rc.CASES[n]().cov3D_precomp)]


@pytest.fixture(autouse=True)
def _reset_routes():
    yield
    dgr._C.lib.msgs_set_backward_generation(0)
    dgr._C.lib.msgs_set_blend_granularity(0)


def _set_route(route):
    gen, gran = ROUTES[route]
    dgr._C.lib.msgs_set_backward_generation(gen)
    dgr._C.lib.msgs_set_blend_granularity(gran)


def _note(what, value):
    MAXIMA[what] = max(MAXIMA[what], value)
    return value


def _rasterizer(c, cam, pc, outputs=(), absgrad=False, features=None):
    from gaussian_renderer import _settings
    pipe = PIPE_COV if c.cov3D_precomp else PIPE
    st = c.settings
    settings = _settings(cam, pc, pipe, c.bg.cuda(), c.smod, st["filter_small"], st["filter_large"], st["fade_size"])
    r = dgr.GaussianRasterizer(settings, return_alpha="alpha" in outputs, absgrad=absgrad)
    return r.with_features(features).with_distortion("distortion" in outputs).with_median_depth("median_depth" in outputs), pipe


def _run(name, outputs, fused, absgrad):
    """one forward with the opt-in outputs of `outputs` (colour and depth are always returned) and one backward of the sum of the
    masked seeds of `outputs` times their maps, on fresh leaves.  Returns (out dict, model, means2D leaf, feature leaf or None)"""
    from gaussian_renderer import _colour_inputs, _shape_inputs
    c, _, _ = rc.truth(name)
    seeds = rc.masked_seeds(name)
    cam = c.cam.to("cuda")
    pc = SyntheticGaussians(c.scene, "cuda", requires_grad=True)
    f = c.features.cuda().clone().requires_grad_(True) if "features" in outputs else None
    r, pipe = _rasterizer(c, cam, pc, outputs, absgrad, f)
    kw = dict(max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes,
              occ_multiplier=pc.get_occ_multiplier, dc_delta=pc.get_dc_delta, base_mask=pc.get_base_mask)
    if fused:
        vs = torch.empty_like(pc._xyz, requires_grad=True)
        outs = r.forward_raw(pc._xyz, vs, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation, **kw)
    else:
        vs = torch.zeros_like(pc.get_xyz, requires_grad=True)
        outs = r(means3D=pc.get_xyz, means2D=vs, opacities=pc.get_opacity, **kw, **_colour_inputs(cam, pc, pipe, None),
                 **_shape_inputs(pc, pipe, c.smod))
    out = dict(color=outs[0], depth=outs[2], radii=outs[3])
    rest = list(outs[5:])
    if "alpha" in outputs:
        out["alpha"] = rest.pop(0)
    if "distortion" in outputs:
        out["distortion"] = rest.pop(0)
    if "median_depth" in outputs:
        out["median_depth"], out["median_id"] = rest.pop(0), rest.pop(0)
    if f is not None:
        out["features"] = rest.pop(0)
    assert not rest
    sum((out[k] * seeds[k].cuda()).sum() for k in outputs).backward()
    torch.cuda.synchronize()
    return out, pc, vs, f


def _check(name, label, outputs, out, pc, vs, f, absgrad):
    c, t, _ = rc.truth(name)
    g = rc.truth_gradients(name, tuple(outputs))
    keep, keep_m = ~t.borderline, ~(t.borderline | t.near)
    assert torch.equal((out["radii"] > 0).cpu(), t.radii > 0), f"{label}: another set of rendered Gaussians"
    cpu = lambda k: out[k].detach().cpu().double()
    # --- the maps ---
    e = _note("colour map, abs", ((cpu("color") - t.color.detach()).abs() * keep).max().item())
    assert e <= FWD_ATOL, f"{label}: colour {e:.3e}"
    scale = max(t.depth.abs().max().item(), 1.0)
    e = _note("depth map, abs / max(1, max depth)", ((cpu("depth") - t.depth.detach()).abs() * keep).max().item() / scale)
    assert e <= FWD_ATOL, f"{label}: depth {e:.3e}"
    if "alpha" in outputs:
        e = _note("alpha map, abs", ((cpu("alpha") - t.alpha.detach()).abs() * keep).max().item())
        assert e <= FWD_ATOL, f"{label}: alpha {e:.3e}"
    if "distortion" in outputs:
        e = _note("distortion map, rel", rel_err(cpu("distortion") * keep, t.distortion.detach() * keep))
        assert e <= BWD_RTOL, f"{label}: distortion map {e:.3e}"
    if "features" in outputs:
        assert out["features"].shape == (c.features.shape[1], t.H, t.W)
        e = _note("feature map, rel", rel_err(cpu("features") * keep[None], t.features.detach() * keep[None]))
        assert e <= BWD_RTOL, f"{label}: feature map {e:.3e}"
    if "median_depth" in outputs:
        I = out["median_id"].cpu()
        assert I.dtype == torch.int32
        wrong = (I != t.median_id) & keep_m
        assert not wrong.any(), f"{label}: {int(wrong.sum())} pixels off the mask with another median id"
        e = _note("median depth map, rel", rel_err(cpu("median_depth") * keep_m, t.median_depth.detach() * keep_m))
        assert e <= BWD_RTOL, f"{label}: median depth map {e:.3e}"
        empty = (t.n_blended == 0) & keep_m
        assert (I[empty] == -1).all() and not cpu("median_depth")[empty].any()
    # --- the gradients ---
    for leaf in (pc._xyz, pc._opacity, pc._scaling, pc._rotation, pc._features_dc, pc._features_rest):
        if leaf.grad is None:                       # (None stands for zeros in check_backward's pairs)
            leaf.grad = torch.zeros_like(leaf)
    m2 = vs.grad if vs.grad is not None else torch.zeros_like(vs)
    pairs = leaf_space(pc, m2, g)
    by_key = {}
    over = [k for k in K8_TENSORS if rel_err(*pairs[k]) > BWD_RTOL]
    if over:
        ref32 = leaf_space(pc, m2, rc.truth_gradients(name, tuple(outputs), torch.float32))
        for k in over:
            d_hip, d_f32 = rel_err(*pairs[k]), rel_err(ref32[k][1], pairs[k][1])
            by_key[k] = max(BWD_RTOL, TRUTH_FACTOR * d_f32 + 1e-6)
            ALLOWANCE.append((label, k, d_hip, d_f32))
            print(f"{label}: grad {k}: HIP {d_hip:.3e} from the truth, the float32 evaluation {d_f32:.3e}")
    worst = check_backward(pc, m2, g, label, rtol=BWD_RTOL, rtol_by_key=by_key)
    for k, v in worst.items():
        _note(f"grad {k}, rel", v)
    if f is not None:
        e = _note("dL/dfeatures, rel", rel_err(f.grad, g["features"]))
        assert e <= BWD_RTOL, f"{label}: dL/dfeatures {e:.3e}"
        assert not f.grad[(t.radii == 0).cuda()].any()
    if absgrad:
        a = vs.absgrad
        assert a.shape == (t.P, 3) and a.dtype == torch.float32 and not a[:, 2].any()
        e = _note("absgrad, rel", rel_err(a[:, :2], g["absgrad"]))
        assert e <= BWD_RTOL, f"{label}: absgrad {e:.3e}"
    else:
        assert not hasattr(vs, "absgrad")


# ---------------------------------------------------------------------------------------------------------------------------
# (a) all opt-ins together
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name,fused", ENTRIES)
def test_all_opt_in_outputs_together_against_float64_truth(name, fused, route):
    _set_route(route)
    out, pc, vs, f = _run(name, ALL, fused, absgrad=True)
    _check(name, f"replay sweep {name} [{route}{', fused' if fused else ''}]", ALL, out, pc, vs, f, absgrad=True)


# ---------------------------------------------------------------------------------------------------------------------------
# (b) each output alone
# ---------------------------------------------------------------------------------------------------------------------------
ALONE = {"alpha": ("alpha",), "absgrad": ("color",), "features": ("features",), "distortion": ("distortion",),
         "median": ("median_depth",)}


# the median replay of the haze cases ends inside the first batch (alpha ~ 0.01: T reaches 1/2 after about 70 entries), so the case
# built for a late crossing runs the median alone too
ALONE_RUNS = [(n, w) for n in rc.ALONE for w in ALONE] + [(n, "median") for n in rc.MEDIAN_ALONE]


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name,which", ALONE_RUNS)
def test_each_opt_in_output_alone_against_float64_truth(name, which, fused, route):
    _set_route(route)
    outputs = ALONE[which]
    out, pc, vs, f = _run(name, outputs, fused, absgrad=which == "absgrad")
    _check(name, f"replay sweep {name}, {which} alone [{route}{', fused' if fused else ''}]", outputs, out, pc, vs, f,
           absgrad=which == "absgrad")


# ---------------------------------------------------------------------------------------------------------------------------
# (c) contribution scores
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", list(rc.CASES))
def test_contribution_scores_against_float64_truth(name, route):
    from gaussian_renderer import _shape_inputs
    import replay_truth as rt
    c, t, _ = rc.truth(name)
    seeds = rc.masked_seeds(name)
    _set_route(route)
    pc = SyntheticGaussians(c.scene, "cuda", requires_grad=False)
    r, pipe = _rasterizer(c, c.cam.to("cuda"), pc)
    shape = {k: v for k, v in _shape_inputs(pc, pipe, c.smod).items() if v is not None}
    for kind in ("ones", "weights"):
        m = seeds[kind]
        assert not m[t.borderline].any() and (m >= 0).all()
        s = r.contributions(pc.get_xyz, pc.get_opacity, max_pixel_sizes=pc.get_max_pixel_sizes,
                            min_pixel_sizes=pc.get_min_pixel_sizes, base_mask=pc.get_base_mask, pixel_weights=m.cuda(), **shape)
        torch.cuda.synchronize()
        want_sum, want_max, want_count = rt.contributions(t, m)
        label = f"replay sweep {name}, contributions [{route}, {kind}]"
        assert torch.equal(s.pixel_count.cpu(), want_count), f"{label}: counts differ on " \
            f"{int((s.pixel_count.cpu() != want_count).sum())} Gaussians"
        for key, got, want in (("sum", s.weight_sum, want_sum), ("max", s.weight_max, want_max)):
            e = _note(f"contribution {key}, rel", rel_err(got, want))
            assert e <= BWD_RTOL, f"{label}: weight_{key} {e:.3e}"


def test_zz_report_the_measured_maxima():
    """printed for profiles/replay_sweep_notes.md (pytest -s); runs last in this file"""
    for k in sorted(MAXIMA):
        print(f"[replay sweep] max {k} = {MAXIMA[k]:.3e}")
    print(f"[replay sweep] (test, tensor) pairs that needed the float32 allowance: {len(ALLOWANCE)}")
    for row in ALLOWANCE:
        print(f"[replay sweep]   {row[0]}: {row[1]}: HIP {row[2]:.3e}, float32 evaluation {row[3]:.3e}")

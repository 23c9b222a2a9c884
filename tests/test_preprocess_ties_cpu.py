"""Exact ties of K1's per-Gaussian decisions, on the CPU: every case of tests/preprocess_ties.py
is what it claims to be (the camera identities, the compared operands bit-equal at T and strictly ordered at T- / T+), and
both oracles — oracle/torch_oracle.py in float64 and in float32, oracle/msgs_oracle.cpp in float32 — take the SPEC's side
at every tie.  The kernels are held to the same expectations in tests/test_preprocess_ties_gpu.py."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import preprocess_ties as pt
import scenes
from oracle import oracle_ctypes as oc
from oracle import torch_oracle as to
from parity_utils import BWD_RTOL

F = np.float32
BG = torch.tensor([0.2, 0.1, 0.3])
ORACLES = ("torch64", "torch32", "cpp32")
REL = {"<": np.less, "==": np.equal, ">": np.greater}


@functools.lru_cache(maxsize=None)
def _case(family):
    return pt.CASES[family]()


def _decide(which, case, st=pt.OFF, filt=None, opacities=None):
    """(radii int64 [P], pixel_sizes numpy [P] in the oracle's own format) of one oracle; filt = (min_ps, max_ps, base_mask)"""
    sc = case.scene
    mn, mx, base = filt if filt is not None else (sc.min_pixel_sizes.numpy(), sc.max_pixel_sizes.numpy(), sc.base_mask.numpy())
    if which == "cpp32":
        s2 = pt.with_filters(case, mn, mx, base, opacities)
        r = oc.rasterize(s2, case.cam, st, BG, use_cov_precomp=case.cov3D is not None, cov3D_precomp=case.cov3D)
        return r.radii.long(), r.pixel_sizes.numpy()
    dt = torch.float64 if which == "torch64" else torch.float32
    view = to.view_dict(case.cam, sh_degree=sc.sh_degree, **st)
    shape = dict(cov3D_precomp=case.cov3D) if case.cov3D is not None else dict(scales=sc.scales, rotations=sc.rotations)
    with torch.no_grad():
        pre = to.preprocess(sc.means3D, sc.opacities if opacities is None else opacities, view, shs=sc.shs,
                            min_pixel_sizes=torch.as_tensor(np.asarray(mn)).to(dt), max_pixel_sizes=torch.as_tensor(np.asarray(mx)).to(dt),
                            base_mask=torch.as_tensor(np.asarray(base)), dtype=dt, **shape)
    assert pre["pixel_sizes"].dtype == dt
    return pre["radii"].long(), pre["pixel_sizes"].numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# the construction
# ---------------------------------------------------------------------------------------------------------------------------
def test_float32_facts():
    assert F(1.3) * F(0.5) == F(0.65) == pt.LIMIT
    assert F(2.0) + F(0.0000001) == F(2.0) and F(1.0) / (F(2.0) + F(0.0000001)) == F(0.5)
    assert F(255.0) * pt.O_GATE == F(1.0) and F(255.0) * pt.up(pt.O_GATE) > F(1.0) and F(255.0) * pt.down(pt.O_GATE) < F(1.0)
    assert F(2.0 ** 25) + F(0.3) == F(2.0 ** 25)
    assert pt.NEAR <= F(0.2) and not pt.up(pt.NEAR) <= F(0.2)
    s = F(1.2345678)
    assert F(1) - (F(2) * s / s - F(1)) / F(1) == 0 and 0 < F(1) - (pt.toward0(F(2) * s) / s - F(1)) / F(1) < 3e-7


@pytest.mark.parametrize("W,H", [(64, 64), (70, 50)])
def test_camera_identities(W, H):
    cam = pt.tie_camera(W, H)
    assert F(math.tan(0.5 * cam.FoVx)) == F(0.5) == F(math.tan(0.5 * cam.FoVy))
    assert torch.equal(cam.world_view_transform, torch.eye(4)) and not cam.camera_center.any()
    pm = cam.full_proj_transform.reshape(-1)
    want = torch.zeros(16)
    want[0] = want[5] = 2.0
    want[11] = 1.0
    want[10] = cam.zfar / (cam.zfar - cam.znear)
    want[14] = -(cam.zfar * cam.znear) / (cam.zfar - cam.znear)
    assert torch.equal(pm, want)
    for family in pt.CASES:
        case = _case(family)
        if (case.cam.image_width, case.cam.image_height) != (W, H):
            continue
        k1 = pt.k1_f32(case)
        p = case.scene.means3D.numpy()
        for k, key in enumerate(("tx", "ty", "tz")):                  # t = p, bit for bit
            assert np.array_equal(k1[key].view(np.int32), p[:, k].view(np.int32)), (family, key)
        assert np.array_equal(k1["hw"].view(np.int32), p[:, 2].view(np.int32))
        assert k1["fx"] == F(W) and k1["fy"] == F(H) and k1["limx"] == pt.LIMIT == k1["limy"]
        at2 = p[:, 2] == 2.0
        assert (k1["pw"][at2] == F(0.5)).all()
        assert np.array_equal(k1["ndc_x"][at2], p[at2, 0]) and np.array_equal(k1["ndc_y"][at2], p[at2, 1])
        for r in case.rows:                                           # the pixel centre is exact where x, y are dyadic
            i = r["row"]
            if p[i, 2] != 2.0 or r["role"] not in ("T", "cal"):
                continue
            for key, v, n in (("px", p[i, 0], W), ("py", p[i, 1], H)):
                assert Fraction(float(k1[key][i])) == ((Fraction(float(v)) + 1) * n - 1) / 2, (family, r["name"], key)


@pytest.mark.parametrize("family", ["near", "degenerate", "rect", "gate", "clamp"])
def test_operands_tie_exactly(family):
    case = _case(family)
    k1 = pt.k1_f32(case)
    roles = set()
    for r in case.rows:
        lhs, rhs = k1[r["lhs"]][r["row"]], r["rhs"]
        assert lhs.dtype == np.float32 and np.asarray(rhs).dtype == np.float32
        assert REL[r["rel"]](lhs, rhs), (r["name"], float(lhs), float(rhs))
        assert REL[r["rel"]](np.float64(lhs), np.float64(rhs))
        if r["rel"] == "==":
            assert lhs.view(np.int32) == np.asarray(rhs).view(np.int32) or (lhs == 0 and rhs == 0)
        elif family != "degenerate":
            # one float32 step of the operand from the tie.  The rect's operand moves by the least its coordinate allows:
            # one ulp of x = -1.2 is 3.8e-6 px, four ulps of 16; det jumps from 0 to 2^27
            steps = abs(int(np.abs(F(lhs)).view(np.int32)) - int(np.abs(F(rhs)).view(np.int32)))
            assert steps <= (4 if family == "rect" else 1), (r["name"], steps)
        roles.add(r["role"])
    assert {"T", "T-"} <= roles
    if family == "rect":
        for r in case.rows:
            i = r["row"]
            assert k1["radius"][i] == 8 and 7.2 < k1["three_sigma"][i] < 7.8, (r["name"], float(k1["three_sigma"][i]))
            # the neighbours are the nearest coordinates at which the operand moves: at most two float32 steps of x / y
            v = case.scene.means3D[i, 0 if r["axis"] == "x" else 1].numpy()
            tie = pt.X_LEFT if r["lhs"].startswith("hi") else pt.X_RIGHT
            assert abs(int(np.abs(v).view(np.int32)) - int(np.abs(tie).view(np.int32))) == (0 if r["role"] == "T" else
                                                                                            1 if r["lhs"].startswith("hi") else 2)
    if family == "degenerate":
        for r in case.rows:
            i = r["row"]
            assert k1["a0"][i] == k1["c0"][i] == F(2.0 ** 25) == k1["a"][i] == k1["c"][i]
            assert abs(k1["b"][i]) == (F(2.0 ** 25) if r["role"] == "T" else F(2.0 ** 25 - 2))
            if r["role"] == "T-":
                assert k1["det"][i] == F(2.0 ** 27) and k1["radius"][i] == 24576
    if family == "clamp":
        assert np.isclose(k1["px"][case.named("x+ T")["row"]], 1.15 * 64, atol=1.0)


def test_rows_straddle_the_seams():
    for family in pt.CASES:
        rows = sorted(r["row"] for r in _case(family).rows)
        assert len(set(rows)) == len(rows) and max(rows) < pt.P
    rows = sorted(r["row"] for r in _case("rect").rows)
    assert {63, 64} <= set(rows) and {255, 256} <= set(rows) and pt.P > 256
    assert _case("rect").scene.P == pt.P


def test_ragged_rect_rows():
    case = _case("rect_ragged")
    k1 = pt.k1_f32(case)
    assert (case.cam.image_width, case.cam.image_height) == (70, 50)
    for r in case.rows:
        i = r["row"]
        lo, hi = r["span"]
        assert lo <= k1[r["lhs"]][i] < hi, (r["name"], float(k1[r["lhs"]][i]))
        centre = k1["px" if r["lhs"] == "lo_x" else "py"][i]
        assert centre > (70 if r["lhs"] == "lo_x" else 50) + 5               # beyond the last pixel, by more than 4 sigma


# ---------------------------------------------------------------------------------------------------------------------------
# the oracles at the ties
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ORACLES)
@pytest.mark.parametrize("family", ["near", "degenerate", "rect", "rect_ragged", "gate", "clamp"])
def test_oracle_decisions(family, which):
    case = _case(family)
    radii, psize = _decide(which, case)
    assert np.isfinite(psize).all()
    pt.check_rows(f"{family} {which}", case, radii, psize)


@pytest.mark.parametrize("which", ORACLES)
@pytest.mark.parametrize("fade", [0.0, 1.0])
def test_oracle_gate_row_under_the_small_filter(which, fade):
    case = _case("gate")
    st, mn, mx, base, alive = pt.gate_filters(case, fade)
    radii, psize = _decide(which, case, st, (mn.numpy(), mx.numpy(), base.numpy()))
    assert sorted(alive.values()) == [False] + [True] * 5
    pt.check_rows(f"gate filtered {which}", case, radii, psize, alive)


@pytest.mark.parametrize("which", ORACLES)
@pytest.mark.parametrize("run", ["fade0", "fade1", "fade05"])
def test_oracle_filters_self_calibrated(run, which):
    case = _case("filters")
    r0, s = _decide(which, case)
    rows = [r["row"] for r in case.rows]
    assert (r0[rows] > 0).all() and (s[rows] > 0).all()
    st, mn, mx, base, plan = pt.filter_plan(case, run, s)
    r1, s1 = _decide(which, case, st, (mn, mx, base))
    assert np.array_equal(s1, s)                                       # M1: written before any filter
    assert len(plan) >= 5
    for i, p in plan.items():
        assert int(r1[i]) == (int(r0[i]) if p["alive"] else 0), (run, which, p["role"], int(r1[i]), int(r0[i]))
    others = [i for i in range(case.scene.P) if i not in plan]
    assert torch.equal(r1[others], r0[others])
    # the thresholds are what the plan says, in the oracle's own format
    for i, p in plan.items():
        if p["role"] == "min_1.5s":
            assert Fraction(float(mn[i])) == Fraction(float(s[i])) * Fraction(3, 2) and mn[i] / s[i] == 1.5
        if p["role"] == "both_1.5":
            assert mn[i] / s[i] == 1.5 and s[i] / mx[i] == 1.5 and s[i] > mx[i]
        if p["role"] == "min_2s":
            assert 1.0 - (mn[i] / s[i] - 1.0) == 0.0
        if p["role"] == "min_2s_down":
            assert 0.0 < 1.0 - (mn[i] / s[i] - 1.0) < 3e-7
        if p["role"] in ("min_up", "base_min_up"):
            assert mn[i] > s[i] and pt.down(mn[i]) == s[i]
        if p["role"] in ("max_down", "base_max_down"):
            assert mx[i] < s[i] and pt.up(mx[i]) == s[i]


@pytest.mark.parametrize("which", ["torch64", "cpp32"])
def test_oracle_effective_opacity_is_o_times_w(which):
    """M4 in the oracles: the render of the scene with 0 < w < 1 rows equals the render with those rows' filters disabled and
    their opacity multiplied by w"""
    case = _case("filters")
    _, s = _decide("cpp32", case)
    st, mn, mx, base, plan = pt.filter_plan(case, "fade1", s)
    a, b, ws = pt.metamorphic_pair(case, mn, mx, base, plan)
    assert sorted(ws.values()) == [0.25, 0.5]
    if which == "cpp32":
        ra, rb = oc.rasterize(a, case.cam, st, BG), oc.rasterize(b, case.cam, st, BG)
        assert torch.equal(ra.color, rb.color) and torch.equal(ra.radii, rb.radii)
        dL = scenes.grad_seed(64, 64, 5)
        ga, gb = oc.backward(ra, dL), oc.backward(rb, dL)
        for k in ("means3D", "scales", "rotations", "shs", "means2D"):
            assert torch.equal(ga[k], gb[k]), k
        for i, w in ws.items():
            assert gb["opacities"][i].abs().item() > 0 and ga["opacities"][i].item() == w * gb["opacities"][i].item()
    else:
        # float64: the float32 oracle's sizes are not the float64 oracle's, so w is close to, not exactly, the plan's
        dL = scenes.grad_seed(64, 64, 5)
        (oa, ga), (ob, gb) = to.forward_backward(a, case.cam, st, BG, dL), to.forward_backward(b, case.cam, st, BG, dL)
        assert (oa["color"] - ob["color"]).abs().max().item() < 1e-5
        for i, w in ws.items():
            assert abs(ga["opacities"][i].item() / gb["opacities"][i].item() - w) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------------
# Q2: the clamp mask, seen through gradients
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_torch_oracle_clamp_mask_at_the_limit(dtype):
    """the conic's gradient towards the clamped coordinate: T- and T carry the Jacobian's term, T+ does not"""
    sc, cam, rows = pt.clamp_probe()
    view = to.view_dict(cam, sh_degree=sc.sh_degree, **pt.OFF)
    m = sc.means3D.to(dtype).clone().requires_grad_(True)
    pre = to.preprocess(m, sc.opacities, view, scales=sc.scales, rotations=sc.rotations, shs=sc.shs, dtype=dtype)
    pre["conic"].sum().backward()
    for j in range(0, len(rows), 3):
        ax = 0 if rows[j]["axis"] == "x" else 1
        g_in, g_tie, g_out = (m.grad[j + k, ax].item() for k in range(3))
        assert [rows[j + k]["role"] for k in range(3)] == ["T-", "T", "T+"]
        assert abs(g_tie - g_in) <= 1e-4 * abs(g_in), (rows[j]["name"], g_in, g_tie)
        assert abs(g_out - g_tie) >= 0.1 * abs(g_tie), (rows[j]["name"], g_tie, g_out)


@functools.lru_cache(maxsize=None)
def _clamp_truth(name=None, role=None):
    case = _case("clamp")
    sc = case.scene if name is None else pt.clamp_variant(case, name, role)
    return to.forward_backward(sc, case.cam, pt.OFF, BG, scenes.grad_seed(64, 64, 71))


def test_clamp_flip_cannot_hide():
    """in the float64 oracle dL/dmeans3D towards the clamped coordinate of T and of T+ (the same row moved one ulp out) differ by
    at least 100 x BWD_RTOL x the row's own gradient scale; T and T- (one ulp in) do not differ"""
    case = _case("clamp")
    _, g = _clamp_truth()
    for r in case.rows:
        if r["role"] != "T":
            continue
        i, ax = r["row"], 0 if r["axis"] == "x" else 1
        own = g["means3D"][i].abs().max().item()
        g_out = _clamp_truth(r["name"], "T+")[1]["means3D"][i, ax].item()
        g_in = _clamp_truth(r["name"], "T-")[1]["means3D"][i, ax].item()
        g_tie = g["means3D"][i, ax].item()
        assert own > 0
        assert abs(g_tie - g_out) >= 100 * BWD_RTOL * own, (r["name"], g_tie, g_out, own)
        assert abs(g_tie - g_in) <= BWD_RTOL * own, (r["name"], g_tie, g_in, own)


def test_cpp_oracle_clamp_rows_against_float64():
    """the float32 C++ oracle's hand-derived backward carries the same mask: every clamp row against the float64 autograd
    gradient on the row's own scale"""
    case = _case("clamp")
    dL = scenes.grad_seed(64, 64, 71)
    orc = oc.rasterize(case.scene, case.cam, pt.OFF, BG)
    og = oc.backward(orc, dL)
    t_out, tg = _clamp_truth()
    assert torch.equal(orc.radii, t_out["radii"])
    for r in case.rows:
        i = r["row"]
        assert not orc.borderline_gaussians[i], r["name"]              # no undecided alpha on a tie row: nothing to exclude
        for k in ("means3D", "scales", "rotations", "opacities"):
            own = tg[k][i].abs().max().item()
            d = (og[k][i].double() - tg[k][i]).abs().max().item()
            assert d <= BWD_RTOL * own, (r["name"], k, d, own)

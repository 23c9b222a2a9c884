"""tests/per_gaussian_truth.py is what it claims to be: the float64 statement of K8 + K9, row by row.

(1) against the float64 build of the CPU oracle on its own sums, every row to 1e-11 of the row's own scale;
(2) against float64 autograd through torch_oracle.preprocess (regularised=False), every row to 1e-10; with the regulariser the
    difference is what 1e-7 / (denom^2 + 1e-7) explains, row by row;
(3) columns is the Jacobian: backward(sums) == sum_j sums_j columns_j;
(4) the family table keeps its promises, decided on the float32 forward;
(5) the float32 restatement's own distance from the truth — the yardstick of tests/test_per_gaussian_backward_gpu.py — is
    measured, is what that file records, and stays within the north star's 1e-4 on every row of every family but `needle`;
(6) a deliberately broken restatement is seen by the per-row criterion on the one-hot pattern of its family; what the tensor-wide
    norm (parity_utils.rel_err) makes of the same mistake on the dense pattern is printed beside it.

Measured figures: profiles/per_gaussian_backward_notes.md (pytest -s tests/test_per_gaussian_truth_cpu.py prints them)."""
import types

import numpy as np
import pytest
import torch

import per_gaussian_truth as pt
import preprocess_ties as ties
import scenes
from oracle import torch_oracle as to
from parity_utils import BWD_RTOL, rel_err, small_scene
from test_per_gaussian_backward_gpu import MARGIN_OF_ORDER, YARDSTICK

ORACLE_RTOL = 1e-11
AUTOGRAD_RTOL = 1e-10
# denom >= 0.3^2 (the +0.3 of Q3 on both diagonals of a positive semi-definite matrix), so 1e-7 / (denom^2 + 1e-7) <= this
REGULARISER_MAX = 1e-7 / (0.09 ** 2 + 1e-7)


def _inputs_of(sc, cov=None):
    inp = dict(means3D=sc.means3D, opacities=sc.opacities.reshape(-1), shs=sc.shs, min_pixel_sizes=sc.min_pixel_sizes,
               max_pixel_sizes=sc.max_pixel_sizes, base_mask=sc.base_mask)
    if cov is not None:
        inp["cov3D_precomp"] = cov
    else:
        inp["scales"], inp["rotations"] = sc.scales, sc.rotations
    return inp


def _assert_rows(what, got, truth, scale, keys, rtol):
    """every row of every tensor: |got - truth| <= rtol * scale; exactly equal where the scale is 0"""
    for k in keys:
        e, s = pt.row_error(got[k], truth, k), scale[k]
        bad = np.nonzero(~(e <= rtol * s))[0]
        worst = float((e[s > 0] / s[s > 0]).max()) if (s > 0).any() else 0.0
        print(f"[per-gaussian] {what}: {k}: worst row {worst:.3e} of its own scale (bound {rtol:g})")
        assert bad.size == 0, (what, k, bad[:5], e[bad[:5]], s[bad[:5]])


# ---- (1) ----------------------------------------------------------------------------------------------------------------
ORACLE_CASES = {
    "plain_deg3": dict(deg=3, filters=False, cov=False),
    "plain_deg0": dict(deg=0, filters=False, cov=False),
    "filters_deg3": dict(deg=3, filters=True, cov=False),
    "cov_precomp": dict(deg=3, filters=False, cov=True),
}


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_against_the_float64_oracle_build(name):
    from oracle import oracle_ctypes as oc
    cfg = ORACLE_CASES[name]
    W, H = 96, 64
    sc, cam = small_scene(400, W, H, seed=31 + len(name), sh_degree=cfg["deg"], multiscale=cfg["filters"])
    st = dict(filter_small=cfg["filters"], filter_large=cfg["filters"], fade_size=1.0)
    bg = torch.tensor([0.1, 0.2, 0.3])
    view = to.view_dict(cam, sh_degree=cfg["deg"], **st)
    if cfg["filters"]:
        # the scene's own thresholds give weights 0 and 1 only: fractional ones from the forward's sizes on every seventh row
        size = pt.forward_f32(view, _inputs_of(sc))["pixel_sizes"]
        sc.min_pixel_sizes, sc.max_pixel_sizes = sc.min_pixel_sizes.clone(), sc.max_pixel_sizes.clone()
        sc.min_pixel_sizes[0::7] = 1.3 * size[0::7]
        sc.max_pixel_sizes[3::7] = size[3::7] / 1.25
        sc.max_pixel_sizes[0::21] = size[0::21] / 1.5
    cov = to.cov3d_from_scale_rot(sc.scales, sc.rotations, 1.0).to(torch.float32).contiguous() if cfg["cov"] else None
    orc = oc.rasterize(sc, cam, st, bg, f64=True, use_cov_precomp=cfg["cov"], cov3D_precomp=cov)
    og = oc.backward(orc, scenes.grad_seed(W, H, 3), want_sums2d=True)
    inp = _inputs_of(sc, cov)
    dec = pt.forward_decisions(view, inp, pixel_sizes=orc.pixel_sizes.numpy())       # the weight a float64 forward applies
    assert np.array_equal(dec["rendered"], (orc.radii > 0).numpy())
    assert dec["rendered"].sum() > 200 and (not cfg["filters"] or ((dec["weight"] > 0) & (dec["weight"] < 1)).sum() >= 3)
    truth = pt.backward(view, inp, og["sums2d"], decisions=dec)
    scale = pt.error_scale(truth)
    got = dict(means3D=og["means3D"], means2D=og["means2D"], opacities=og["opacities"].reshape(-1), shs=og["shs"])
    if cfg["cov"]:
        got["cov3D"] = og["cov3D_precomp"]
    else:
        got["scales"], got["rotations"] = og["scales"], og["rotations"]
    _assert_rows(f"oracle64 {name}", got, truth, scale, pt.tensor_names(inp), ORACLE_RTOL)
    assert np.abs(og["sums2d"].numpy()[dec["rendered"]]).max(axis=0).min() > 0        # all nine sums are exercised


# ---- (2) ----------------------------------------------------------------------------------------------------------------
AUTOGRAD_FAMILIES = ("round", "round_front", "clamp", "modifier_0.7", "modifier_1.6", "quaternion", "filter_fade0.5",
                     "filter_fade1")


def _autograd(view, inp, sums, rendered):
    """float64 autograd of L = <sums, (ndc x, ndc y, conic A, 2 conic B, conic C, o_eff, rgb)> through torch_oracle.preprocess.
    ndc = pixel / (0.5 W): the NDC-ish unit of dL_dmeans2D; 2 conic B: sums[:, 3] is the reference's dL_dconic.y, the gradient
    by ONE of the two symmetric off-diagonal entries (its blend backward adds -0.5 dx dy, and dL_db carries the 2)"""
    dt = torch.float64
    leaf = lambda k: inp[k].detach().to(dt).clone().requires_grad_(True)
    lv = {k: leaf(k) for k in ("means3D", "opacities", "scales", "rotations", "shs")}
    pre = to.preprocess(lv["means3D"], lv["opacities"], view, scales=lv["scales"], rotations=lv["rotations"], shs=lv["shs"],
                        max_pixel_sizes=inp["max_pixel_sizes"], min_pixel_sizes=inp["min_pixel_sizes"],
                        base_mask=inp["base_mask"])
    W, H = view["image_width"], view["image_height"]
    s = torch.from_numpy(np.where(rendered[:, None], sums, 0.0))
    con = pre["conic"]
    L = (s[:, 0] * pre["px"] / (0.5 * W) + s[:, 1] * pre["py"] / (0.5 * H) + s[:, 2] * con[:, 0] + 2.0 * s[:, 3] * con[:, 1]
         + s[:, 4] * con[:, 2] + s[:, 5] * pre["opacity"] + (s[:, 6:9] * pre["rgb"]).sum(dim=1)).sum()
    L.backward()
    g = {k: v.grad.numpy() for k, v in lv.items()}
    g["means2D"] = np.concatenate([s[:, :2].numpy(), np.zeros((len(sums), 1))], axis=1)
    return g, pre


@pytest.mark.parametrize("pattern", ["onehot", "dense"])
@pytest.mark.parametrize("name", AUTOGRAD_FAMILIES)
def test_against_float64_autograd(name, pattern):
    view, inp, sums, _ = pt.case(name, pattern, pt.P_MAX)
    pre64 = pt.forward_f32(view, inp, dtype=torch.float64)
    dec = pt.forward_decisions(view, inp, pixel_sizes=pre64["pixel_sizes"].numpy())
    plain = pt.backward(view, inp, sums, decisions=dec, regularised=False)
    auto, pre = _autograd(view, inp, sums, dec["rendered"])
    assert np.array_equal(pre["visible"].numpy(), dec["rendered"])
    scale = pt.error_scale(plain)
    keys = pt.tensor_names(inp)
    _assert_rows(f"autograd {name} {pattern}", auto, plain, scale, keys, AUTOGRAD_RTOL)
    # with the regulariser: the conic sums' share of every covariance-borne tensor shrinks by denom^2 / (denom^2 + 1e-7), and
    # nothing else changes — per row |reg - plain| <= 1e-7 / (denom^2 + 1e-7) x the scale of that share, at most REGULARISER_MAX
    reg = pt.backward(view, inp, sums, decisions=dec)
    conic_only = dict(plain, sums=plain["sums"] * np.array([0, 0, 1, 1, 1, 0, 0, 0, 0.0])[None])
    share = pt.error_scale(conic_only)
    denom = plain["geometry"]["denom"]
    factor = np.where(dec["rendered"], 1e-7 / (denom * denom + 1e-7), 0.0)
    assert factor.max() <= REGULARISER_MAX
    for k in keys:
        d = pt.row_error(reg[k], plain, k)
        if k in ("means3D", "scales", "rotations", "cov3D"):
            assert (d <= factor * share[k] * (1 + 1e-9) + 1e-13 * scale[k]).all(), k     # (+ the float64 rounding of both)
        else:
            assert not d.any(), k


# ---- (3) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pt.FAMILIES))
def test_columns_are_the_jacobian(name):
    view, inp, sums, _ = pt.case(name, "decades", pt.P_MAX)
    res = pt.backward(view, inp, sums)
    scale = pt.error_scale(res)
    P = len(sums)
    for k in pt.tensor_names(inp):
        acc = np.zeros_like(res[k])
        for j in range(9):
            acc = acc + res["sums"][:, j].reshape((P,) + (1,) * (acc.ndim - 1)) * res["columns"][j][k]
        e = np.abs(acc - res[k]).reshape(P, -1).max(axis=1)
        # the same expressions in float64: the restatement's own rounding, in units of 2^-53 scale, is what YARDSTICK holds
        # in units of 2^-24 scale; twice, for both sides, and the nine terms added in another order
        assert (e <= (4 * YARDSTICK[name][k] + 16) * 2.0 ** -53 * scale[k]).all(), (name, k)
        assert not res[k][~res["rendered"]].any()


# ---- (4) ----------------------------------------------------------------------------------------------------------------
def _operands(fam):
    """the float32 operands of K1's comparators (tests/preprocess_ties.k1_f32; the modifier folded into the scales: K1 forms
    S = mod * s before anything else)"""
    inp = fam["inputs"]
    sc = types.SimpleNamespace(means3D=inp["means3D"], opacities=inp["opacities"],
                               scales=None if "scales" not in inp else
                               torch.from_numpy(np.float32(fam["mod"]) * inp["scales"].numpy()),
                               rotations=inp.get("rotations"))
    with np.errstate(all="ignore"):
        return ties.k1_f32(types.SimpleNamespace(scene=sc, cam=fam["cam"], cov3D=inp.get("cov3D_precomp")))


def test_the_camera_is_general():
    cam = pt.general_camera()
    assert (cam.world_view_transform[:3, :3] != 0).all() and (cam.world_view_transform[3, :3] != 0).all()
    view = pt.family("round")["view"]
    assert abs(pt.W / (2 * view["tanfovx"]) - pt.H / (2 * view["tanfovy"])) > 1.0
    assert torch.equal(pt.family("round_front")["cam"].world_view_transform, torch.eye(4))
    assert (pt.W, pt.H) == (160, 96)


@pytest.mark.parametrize("name", list(pt.FAMILIES))
def test_family_keeps_its_promises(name):
    fam = pt.family(name)
    exp, inp, n = fam["expect"], fam["inputs"], fam["n"]
    assert n <= 300 and 9 * n <= pt.P_MAX or name == "dead", "every geometry carries every one-hot sum within P_MAX rows"
    dec = pt.forward_decisions(fam["view"], inp)
    k1 = _operands(fam)
    m = pt.MARGIN
    want = np.asarray(exp["rendered"])
    assert np.array_equal(dec["rendered"], want)
    kind = np.asarray(exp.get("kind", np.array(["live"] * n)))
    front = k1["tz"] > 0.2
    # ---- the margins: every comparator of K1 that decides something about the row, 1 % from its tie ----
    assert (np.abs(k1["tz"] - 0.2) >= m * 0.2).all()
    for q, lim in (("txtz", "limx"), ("tytz", "limy")):
        assert (np.abs(np.abs(k1[q][front]) - k1[lim]) >= m * k1[lim]).all(), q
    assert (k1["det"][front] >= 0.08).all()                      # the tie is det == 0; the +0.3 floor is 0.09
    assert (k1["v255"] >= 1.0 + m).all()
    gx, gy = float(pt.W), float(pt.H)                            # 10 x 6 whole tiles
    on = (k1["hi_x"] >= 16 * (1 + m)) & (k1["hi_y"] >= 16 * (1 + m)) & (k1["lo_x"] <= gx * (1 - m)) & (k1["lo_y"] <= gy * (1 - m))
    off = (k1["hi_x"] <= 16 * (1 - m)) | (k1["hi_y"] <= 16 * (1 - m)) | (k1["lo_x"] >= gx * (1 + m)) | (k1["lo_y"] >= gy * (1 + m))
    assert on[want].all()
    assert off[kind == "offscreen"].all() and on[front & (kind != "offscreen")].all()
    assert not front[kind == "behind"].any() and front[kind != "behind"].all()
    size = dec["pixel_sizes"].astype(np.float64)
    mn, mx = inp["min_pixel_sizes"].numpy().astype(np.float64), inp["max_pixel_sizes"].numpy().astype(np.float64)
    if fam["settings"]["filter_small"]:
        fade = fam["settings"]["fade_size"]
        size = np.where(size > 0, size, np.nan)
        for thr, rel in ((mn, mn / size), (mx, size / mx)):
            act = front & (thr > 0)
            assert (np.abs(rel[act] - 1.0) >= m).all()                               # size against the threshold
            raw = 1.0 - (rel[act] - 1.0) / fade
            assert ((np.abs(raw) >= m) | (rel[act] < 1)).all()                       # ... and the weight against 0
    # ---- what the family is for ----
    if "clamped_x" in exp:
        assert np.array_equal(dec["clamped_x"], exp["clamped_x"]) and np.array_equal(dec["clamped_y"], exp["clamped_y"])
        cx, cy = dec["clamped_x"], dec["clamped_y"]
        for sel in (cx & ~cy, cy & ~cx, cx & cy):
            assert sel.sum() >= 4
        assert {(np.sign(a), np.sign(b)) for a, b in zip(k1["txtz"][cx & cy], k1["tytz"][cx & cy])} == \
            {(1, 1), (1, -1), (-1, 1), (-1, -1)}
        assert {np.sign(v) for v in k1["txtz"][cx & ~cy]} == {1, -1} and {np.sign(v) for v in k1["tytz"][cy & ~cx]} == {1, -1}
        assert not (cx | cy)[1::2].any() and (cx | cy)[0::2].all()                   # every clamped row has its twin inside
        inside = np.maximum(np.abs(k1["txtz"]) / k1["limx"], np.abs(k1["tytz"]) / k1["limy"])[1::2]
        assert (inside > 0.95).all() and (inside < 1 - m).all()
    else:
        assert not dec["clamped_x"][want].any() and not dec["clamped_y"][want].any() or name == "dead"
    if "cut" in exp:
        assert np.array_equal(dec["cut"], exp["cut"]) and exp["cut"].sum() >= 10 and (~exp["cut"]).sum() >= 10
        denom = k1["det"].astype(np.float64)
        assert (denom[exp["cut"]] >= 10 * pt.GIANT_OVERFLOW).all()
        assert (denom[~exp["cut"]] <= pt.GIANT_OVERFLOW / 10).all() and (denom[~exp["cut"]] >= 3e16).all()
    else:
        assert not dec["cut"].any()
    if "weight" in exp:
        assert np.allclose(dec["weight"], exp["weight"], rtol=0, atol=2e-6)
        for role in pt.FILTER_ROLES:
            assert (exp["role"] == role).sum() >= 4, role
        assert set(np.round(exp["weight"][exp["role"] == "both"], 6)) < {0.3, 0.6} | set()
    if "sh_clamped" in exp:
        assert np.array_equal(dec["sh_clamped"], exp["sh_clamped"])
        per_row = dec["sh_clamped"].sum(axis=1)
        assert (per_row == 0).sum() >= 4 and (per_row == 3).sum() >= 4
        for c in range(3):
            assert ((per_row == 1) & dec["sh_clamped"][:, c]).sum() >= 4, c
    elif "shs" in inp:
        assert not dec["sh_clamped"][want].any()
    if "scales" in inp:
        s = inp["scales"].numpy().astype(np.float64)
        aspect = s.max(axis=1) / s.min(axis=1)
        if "max_aspect" in exp:
            assert (aspect <= exp["max_aspect"]).all()
        if "min_aspect" in exp:
            assert (aspect >= exp["min_aspect"]).all() and aspect.max() >= 500 and aspect.max() <= 2000
    if exp.get("lowpass"):
        assert (k1["a0"] <= 0.03 * 0.3).all() and (k1["c0"] <= 0.03 * 0.3).all()       # the +0.3 is > 97 % of both diagonals
    if name == "quaternion":
        q = inp["rotations"].numpy().astype(np.float64)
        norm = np.linalg.norm(q, axis=1)
        k = exp["kind"]
        assert (np.abs(norm[k != "nonunit"] - 1) < 1e-6).all() and (np.abs(norm[k == "nonunit"] - 1) > 0.02).sum() >= 6
        assert ((q[k == "basis"] != 0).sum(axis=1) == 1).all() and {int(np.argmax(np.abs(r))) for r in q[k == "basis"]} == {0, 1, 2, 3}
        assert (q[:, 0] < 0).sum() >= 8 and ((q[k == "pair"] != 0).sum(axis=1) >= 2).all()
    if name == "dead":
        first_wave = kind[:64]
        for what in ("live", "behind", "offscreen", "filtered"):
            assert (first_wave == what).sum() >= 8, what
        assert (kind[32:64] != "live").all() and (kind[:32] == "live").sum() >= 10 and (kind[64:] == "live").sum() >= 10
        assert (dec["weight"][kind == "filtered"] == 0).all()
    if "cov3D_precomp" in inp:
        cov = inp["cov3D_precomp"].numpy()
        assert (np.abs(cov[:, [1, 2, 4]]) > 1e-3 * np.abs(cov[:, [0, 3, 5]]).max(axis=1, keepdims=True)).all(axis=1).sum() >= n - 4


def test_row_counts_leave_partial_waves_runs_and_workgroups():
    assert pt.ROW_COUNTS == (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300)
    for name in pt.FAMILIES:
        s300, geo = pt._sums(pt.family(name), "onehot")
        view, inp, s, g = pt.case(name, "onehot", 65)
        assert np.array_equal(s, s300[:65], equal_nan=True) and np.array_equal(g, geo[:65])     # a prefix: truncation
        n = pt.family(name)["n"]
        live = np.asarray(pt.family(name)["expect"]["rendered"])[geo]
        assert ((s300[live] != 0).sum(axis=1) == 1).all()
        if 9 * n <= pt.P_MAX:
            seen = {(a, int(np.nonzero(r)[0][0])) for a, r, l in zip(geo, s300, live) if l}
            assert len(seen) == 9 * live[:n].sum()                                   # every geometry with every sum


# ---- (5) ----------------------------------------------------------------------------------------------------------------
NORTH_STAR_IN_ULPS = BWD_RTOL / pt.EPS32


@pytest.mark.parametrize("name", list(pt.FAMILIES))
def test_yardstick_is_recorded(name):
    """the float32 restatement's distance from the truth per tensor, in units of 2^-24 x the row's scale: what the GPU test's
    bounds are twice of.  Fails if a recorded constant is below what is measured now."""
    measured = pt.yardstick(name)
    rec = YARDSTICK[name]
    print(f"[per-gaussian] yardstick {name}: " + ", ".join(f"{k} {v:.2f} (recorded {rec[k]:g})" for k, v in measured.items()))
    assert set(rec) == set(measured)
    for k, v in measured.items():
        assert v <= rec[k], (name, k, v, rec[k])
        assert rec[k] <= 1.25 * v + 1.0, (name, k, "recorded far above what is measured: measure again", v, rec[k])
    if not pt.family(name)["needle"]:
        # a condition, not a measurement: a legal float32 evaluation is inside the north star on EVERY row
        assert max(measured.values()) <= NORTH_STAR_IN_ULPS, (name, measured)
        assert MARGIN_OF_ORDER * max(rec.values()) <= NORTH_STAR_IN_ULPS


# ---- (6) ----------------------------------------------------------------------------------------------------------------
MUTANTS = {           # mutation -> (family, tensor it must show in)
    "dq2_sign": ("quaternion", "rotations"),
    "x_mul_ignored": ("clamp", "means3D"),
    "gm_half_dropped": ("round", "scales"),
    "modifier_once": ("modifier_1.6", "scales"),
}


@pytest.mark.parametrize("mutation", list(MUTANTS))
def test_per_row_criterion_sees_a_broken_restatement(mutation):
    name, key = MUTANTS[mutation]
    out = {}
    for pattern in ("onehot", "dense"):
        view, inp, sums, _ = pt.case(name, pattern, pt.P_MAX)
        dec = pt.forward_decisions(view, inp)
        truth = pt.backward(view, inp, sums, decisions=dec)
        broken = pt.backward(view, inp, sums, decisions=dec, dtype=np.float32, mutate=mutation)
        scale = pt.error_scale(truth)
        ratio = pt.worst_ratio(broken[key], truth, scale, key)
        bound = MARGIN_OF_ORDER * YARDSTICK[name][key]
        rows = int(((pt.row_error(broken[key], truth, key) > bound * pt.EPS32 * scale[key])).sum())
        out[pattern] = (ratio, bound, rows, rel_err(torch.from_numpy(broken[key].astype(np.float64)), torch.from_numpy(truth[key])))
    # the same mistake on the kind of scene the tensor-wide comparisons run on (scale_modifier 1, every centre within 1.15 of
    # the frustum, dense sums): what the old norm on the old scenes makes of it
    sc = scenes.frustum_scene(2000, pt.W, pt.H, seed=3)
    view = to.view_dict(scenes.front_camera(pt.W, pt.H), sh_degree=3, **pt.OFF)
    inp = _inputs_of(sc)
    sums = np.random.default_rng(3).normal(size=(sc.P, 9)).astype(np.float32).astype(np.float64)
    dec = pt.forward_decisions(view, inp)
    truth = pt.backward(view, inp, sums, decisions=dec)
    broken = pt.backward(view, inp, sums, decisions=dec, dtype=np.float32, mutate=mutation)
    scene = rel_err(torch.from_numpy(broken[key].astype(np.float64)), torch.from_numpy(truth[key]))
    for pattern, (ratio, bound, rows, glob) in out.items():
        print(f"[per-gaussian] mutant {mutation} on {name}/{pattern}: {key} worst row {ratio:.3e} x 2^-24 scale (bound {bound:g}), "
              f"{rows} rows over; tensor-wide rel_err {glob:.3e} (north star {BWD_RTOL:g})")
    print(f"[per-gaussian] mutant {mutation} on frustum_scene(2000, seed 3), dense: tensor-wide rel_err {scene:.3e}, "
          f"{int(dec['clamped_x'][dec['rendered']].sum())} of {int(dec['rendered'].sum())} rendered rows clamped in x")
    assert out["onehot"][0] > out["onehot"][1] and out["onehot"][2] > 0

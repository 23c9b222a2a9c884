"""preprocess_backward_kernel (K8 + K9) one Gaussian at a time: msgs_backward_per_gaussian on planted sums against the float64
restatement of tests/per_gaussian_truth.py, every row relative to ITS OWN scale

    |got - truth| <= k * 2^-24 * scale[i, t],   scale[i, t] = sum_j |sums[i, j]| ||columns[j][t][i]||_inf

over the row families of that module (round, clamp, lowpass, needle, modifier, quaternion, giant, filter, dead, precomputed,
sh), three sum patterns (one-hot: the kernel's Jacobian column by column; dense; sign-mixed over six decades) and row counts
that leave the last wave, the last 32-row SH run and the last workgroup partly filled.  The entry runs the TEXTBOOK branch of
the kernel, which shares everything behind the sums with the production branches; there is no blend, no borderline pixel and
no atomic, so two runs must give the same bits.

k = MARGIN_OF_ORDER x YARDSTICK[family][tensor].  YARDSTICK is the float32 restatement's own worst distance from the truth in
the same unit — the same expressions in the kernel's order, one rounding per operation — measured on the CPU by
tests/test_per_gaussian_truth_cpu.py::test_yardstick_is_recorded, which fails if a constant here is below what it measures.
The margin of 2 covers FMA contraction and another order of the same products (the convention of test_position_noise); it does
not cover a different formula.  A tensor whose yardstick is 0 (dL_dmeans2D, dL_dcolors, dL_dopacities at weight 1: copies of
float32-representable sums) must be exact.  Achieved ratios: profiles/per_gaussian_backward_notes.md."""
import numpy as np
import pytest
import torch

import per_gaussian_truth as pt

pytestmark = pytest.mark.gpu

MARGIN_OF_ORDER = 2.0
YARDSTICK = {
    "round": dict(means3D=24, means2D=0, opacities=0, scales=36, rotations=27, shs=4.6),
    "round_front": dict(means3D=21, means2D=0, opacities=0, scales=17, rotations=33, shs=4.6),
    "clamp": dict(means3D=27, means2D=0, opacities=0, scales=20, rotations=37, shs=4),
    "lowpass": dict(means3D=30, means2D=0, opacities=0, scales=59, rotations=35, shs=4.5),
    "needle": dict(means3D=870000, means2D=0, opacities=0, scales=330000, rotations=680000, shs=4.3),
    "modifier_0.7": dict(means3D=52, means2D=0, opacities=0, scales=22, rotations=28, shs=4.8),
    "modifier_1.6": dict(means3D=52, means2D=0, opacities=0, scales=16, rotations=21, shs=4.8),
    "quaternion": dict(means3D=30, means2D=0, opacities=0, scales=41, rotations=36, shs=4.4),
    "giant": dict(means3D=31, means2D=0, opacities=0, scales=18, rotations=45, shs=4.1),
    "filter_fade0.5": dict(means3D=18, means2D=0, opacities=1, scales=26, rotations=24, shs=3.7),
    "filter_fade1": dict(means3D=36, means2D=0, opacities=1, scales=17, rotations=28, shs=4.1),
    "dead": dict(means3D=16, means2D=0, opacities=0, scales=17, rotations=20, shs=3.5),
    "precomputed": dict(means3D=130, means2D=0, opacities=0, cov3D=110, colors=0),
    "precomputed_cov": dict(means3D=120, means2D=0, opacities=0, cov3D=110, shs=6.2),
    "precomputed_colour": dict(means3D=30, means2D=0, opacities=0, scales=19, rotations=26, colors=0),
    "sh0_K16_padded": dict(means3D=13, means2D=0, opacities=0, scales=23, rotations=36, shs=1.9),
    "sh1_K16_padded": dict(means3D=26, means2D=0, opacities=0, scales=27, rotations=34, shs=2.7),
    "sh2_K16_padded": dict(means3D=18, means2D=0, opacities=0, scales=35, rotations=65, shs=4.3),
    "sh3_K16": dict(means3D=20, means2D=0, opacities=0, scales=15, rotations=37, shs=6),
    "sh0_K1": dict(means3D=16, means2D=0, opacities=0, scales=21, rotations=41, shs=2),
    "sh1_K4": dict(means3D=17, means2D=0, opacities=0, scales=340, rotations=25, shs=2.2),
    "sh2_K9": dict(means3D=17, means2D=0, opacities=0, scales=17, rotations=26, shs=3.1),
}
# (opacities of the filter families: dL/dopacity = w * sum is ONE rounded product, at most half an ulp = 2^-24 of itself, whatever the
#  weight; measured 0.82 and 0.93)
ACHIEVED = {}        # (family, tensor) -> worst ratio over everything run so far


def _run(name, pattern, P):
    import diff_gaussian_rasterization as dgr
    from per_gaussian_entry import family_call, per_gaussian_hip
    fam = pt.family(name)
    view, inp, sums, _ = pt.case(name, pattern, P)
    cov = inp.get("cov3D_precomp")
    call = family_call(fam, inp)
    with torch.no_grad():
        _, _, _, radii, psz, (geom, _, _, _) = dgr._forward_impl(call)
    torch.cuda.synchronize()
    s = torch.from_numpy(sums)
    runs = [per_gaussian_hip(call, radii, geom, s, with_cov=cov is not None, fill=float("nan")) for _ in range(2)]
    got = {("cov3D" if k == "cov3D_precomp" else k): v.cpu().numpy() for k, v in runs[0].items()}
    again = {("cov3D" if k == "cov3D_precomp" else k): v.cpu().numpy() for k, v in runs[1].items()}
    # the weight the kernel stored is a function of the pixel size it returned: the truth multiplies by exactly that
    dec = pt.forward_decisions(view, inp, pixel_sizes=psz.cpu().numpy())
    return view, inp, sums, dec, radii.cpu().numpy(), got, again


@pytest.mark.parametrize("P", pt.ROW_COUNTS)
@pytest.mark.parametrize("pattern", pt.PATTERNS)
@pytest.mark.parametrize("name", list(pt.FAMILIES))
def test_every_row_against_its_own_scale(name, pattern, P):
    view, inp, sums, dec, radii, got, again = _run(name, pattern, P)
    rendered = dec["rendered"]
    assert np.array_equal(radii > 0, rendered), np.nonzero((radii > 0) != rendered)[0]
    truth = pt.backward(view, inp, sums, decisions=dec)
    scale = pt.error_scale(truth)
    keys = pt.tensor_names(inp)
    assert set(got) == set(keys)
    f32 = sums.astype(np.float32)
    for k in keys:
        g = got[k]
        assert np.isfinite(g).all(), (k, "an element was not written, or a dead row's NaN / Inf leaked")
        assert not g[~rendered].any(), (k, "a row that was not rendered is not zero")
        assert np.array_equal(g.view(np.uint32), again[k].view(np.uint32)), (k, "two runs differ")
        e, sc = pt.row_error(g, truth, k), scale[k]
        bound = MARGIN_OF_ORDER * YARDSTICK[name][k]
        ratio = pt.worst_ratio(g, truth, scale, k)
        ACHIEVED[(name, k)] = max(ACHIEVED.get((name, k), 0.0), ratio)
        print(f"[per-gaussian] {name} {pattern} P={P}: {k} worst row {ratio:.2f} x 2^-24 scale (bound {bound:g}; "
              f"worst so far {ACHIEVED[(name, k)]:.2f})")
        bad = np.nonzero(~(e <= bound * pt.EPS32 * sc))[0]
        assert bad.size == 0, (name, pattern, P, k, "rows", bad[:8], "ratio", (e[bad[:8]] / (pt.EPS32 * sc[bad[:8]] + 1e-300)),
                               "sums", [[pt.SUM_NAMES[j] for j in np.nonzero(sums[i])[0]] for i in bad[:8]])
        zero = sc == 0
        assert not g.reshape(len(g), -1)[zero].any(), (k, "a row whose scale is exactly 0 must be +-0")
    # ---- the exact parts ----
    live = rendered
    m2 = got["means2D"]
    assert np.array_equal(m2[live, 0].view(np.uint32), f32[live, 0].view(np.uint32))
    assert np.array_equal(m2[live, 1].view(np.uint32), f32[live, 1].view(np.uint32)) and not m2[:, 2].any()
    one = live & (dec["weight"] == 1)
    assert np.array_equal(got["opacities"][one].view(np.uint32), f32[one, 5].view(np.uint32))
    if "colors" in got:
        assert np.array_equal(got["colors"][live].view(np.uint32), f32[live, 6:9].view(np.uint32))
    else:
        cl = dec["sh_clamped"] & live[:, None]
        assert not (got["shs"] * cl[:, None, :]).any(), "a clamped channel passes no SH gradient"
        ncoef = (int(view["sh_degree"]) + 1) ** 2
        assert not got["shs"][:, ncoef:].any(), "coefficients beyond the active degree"
        # only colour sums planted, all of them on clamped channels: nothing reaches dL/dmeans3D (its scale is 0 there, so the
        # +-0 assertion above has covered it; this names the property)
        only_clamped = live & ~(sums[:, :6] != 0).any(axis=1) & ~((sums[:, 6:9] != 0) & ~dec["sh_clamped"]).any(axis=1)
        assert not got["means3D"][only_clamped].any()
    if "cut" in pt.family(name)["expect"]:
        cut = dec["cut"] & live
        for k in ("scales", "rotations"):
            assert not got[k][cut].any(), (k, "denom2inv == 0: the covariance chain is cut")
            planted = live & ~dec["cut"] & (sums[:, 2:5] != 0).any(axis=1)
            assert got[k][planted].any(axis=1).all(), (k, "the neighbours at denom ~ 1e17 are not cut")
        proj = cut & (sums[:, :2] != 0).any(axis=1)
        assert got["means3D"][proj].any(axis=1).all(), "the projection part of a cut row is present"
        conic_only = cut & ~(sums[:, :2] != 0).any(axis=1) & ~(sums[:, 5:] != 0).any(axis=1)
        assert not got["means3D"][conic_only].any(), "the covariance part of a cut row is exactly zero"

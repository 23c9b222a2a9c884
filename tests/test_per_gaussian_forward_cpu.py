"""The per-Gaussian forward's truth, yardstick, arrangements and checker (tests/per_gaussian_forward_truth.py) on the CPU; no kernel.

 (1) the truth against the float64 build of oracle/msgs_oracle.cpp on every per-Gaussian value that build exposes
 (2) the float32 yardstick's worst ratio per arrangement and field (printed: profiles/per_gaussian_forward_notes.md holds the
     table), the bounds derived from it, and that the float32 oracle passes the checker under them
 (3) the conditions of the arrangements, from the truth alone: margins from every tie, survivor sets per wave, distinct
     colours, the side of the gate of each twin, how many rows are unbounded
 (4) every mutation is caught per row — and whether today's tensor-wide assertions (parity_utils.check_forward: 1e-5 abs on the
     image, 1e-4 on pixel_sizes, radii) see it on a render of the same rows"""
import numpy as np
import pytest
import torch

import culling_truth as ct
import per_gaussian_forward_truth as ft
from oracle import torch_oracle as to
from parity_utils import FWD_ATOL, small_scene

ORACLE_RTOL = 1e-11


# ---- (1) ----------------------------------------------------------------------------------------------------------------
ORACLE_CASES = {
    "plain_deg3": dict(deg=3, filters=False, cov=False),
    "plain_deg0": dict(deg=0, filters=False, cov=False),
    "filters_deg3": dict(deg=3, filters=True, cov=False),
    "cov_precomp": dict(deg=3, filters=False, cov=True),
}


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_truth_against_the_float64_oracle_build(name):
    from oracle import oracle_ctypes as oc
    cfg = ORACLE_CASES[name]
    Wd, Hd = 96, 64
    sc, cam = small_scene(400, Wd, Hd, seed=41 + len(name), sh_degree=cfg["deg"], multiscale=cfg["filters"])
    st = dict(filter_small=cfg["filters"], filter_large=cfg["filters"], fade_size=1.0)
    view = to.view_dict(cam, sh_degree=cfg["deg"], **st)
    inp = dict(means3D=sc.means3D, opacities=sc.opacities.reshape(-1), shs=sc.shs, min_pixel_sizes=sc.min_pixel_sizes,
               max_pixel_sizes=sc.max_pixel_sizes, base_mask=sc.base_mask, scales=sc.scales, rotations=sc.rotations)
    cov = None
    if cfg["filters"]:                    # fractional weights from the forward's own sizes on every seventh row
        size = torch.from_numpy(ft.yardstick(view, inp)["pixel_sizes"])
        sc.min_pixel_sizes, sc.max_pixel_sizes = sc.min_pixel_sizes.clone(), sc.max_pixel_sizes.clone()
        sc.min_pixel_sizes[0::7] = 1.3 * size[0::7]
        sc.max_pixel_sizes[3::7] = size[3::7] / 1.25
        inp.update(min_pixel_sizes=sc.min_pixel_sizes, max_pixel_sizes=sc.max_pixel_sizes)
    if cfg["cov"]:
        cov = to.cov3d_from_scale_rot(sc.scales, sc.rotations, 1.0).to(torch.float32).contiguous()
        inp.update(cov3D_precomp=cov, scales=None, rotations=None)
    orc = oc.rasterize(sc, cam, st, torch.tensor([0.1, 0.2, 0.3]), f64=True, use_cov_precomp=cfg["cov"], cov3D_precomp=cov)
    tr = ft.truth(view, inp)
    P = sc.P
    f64 = torch.float64
    m2, co = orc._arr("means2D", (P, 2), f64).numpy(), orc._arr("conic_opacity", (P, 4), f64).numpy()
    rgb, dep = orc._arr("rgb", (P, 3), f64).numpy(), orc._arr("depths", (P,), f64).numpy()
    live = orc.radii.numpy() > 0
    assert np.array_equal(tr["radii"], orc.radii.numpy()) and live.sum() > 200
    assert not cfg["filters"] or ((tr["weight"] > 0) & (tr["weight"] < 1) & live).sum() >= 3
    got = dict(px=m2[:, 0], py=m2[:, 1], A=ft.KLOG * co[:, 0], Bh=ft.KLOG * co[:, 1], C=ft.KLOG * co[:, 2],
               lo=np.log2(np.where(live, co[:, 3], 1.0)), r=rgb[:, 0], g=rgb[:, 1], b=rgb[:, 2], depth=dep)
    for f, g in got.items():
        e = np.abs(g[live] - tr[f][live]) / np.maximum(np.abs(tr[f][live]), 1.0 if f in ("px", "py", "lo", "r", "g", "b") else 1e-300)
        print(f"[k1-rows] oracle64 {name}: {f}: worst row {e.max():.3e} of its own size (bound {ORACLE_RTOL:g})")
        assert e.max() <= ORACLE_RTOL, (name, f, int(e.argmax()))
    ps = orc.pixel_sizes.numpy()
    e = np.abs(ps - tr["pixel_sizes"]) / np.maximum(tr["pixel_sizes"], 1e-300)
    print(f"[k1-rows] oracle64 {name}: pixel_sizes: worst row {e[tr['ok'] & (ps > 0)].max():.3e} (bound {ORACLE_RTOL:g}), "
          f"{int((tr['ok'] & ~live).sum())} of them not rendered")
    assert (e[tr["ok"] & (tr["pixel_sizes"] > 0)] <= ORACLE_RTOL).all() and not ps[~tr["ok"]].any()
    assert np.array_equal(ps == 0, tr["pixel_sizes"] == 0)


# ---- (2) ----------------------------------------------------------------------------------------------------------------
def test_yardstick_and_bounds():
    """prints the table of profiles/per_gaussian_forward_notes.md; the conditions: the float32 oracle is within a few tens of
    ulps of every row's own scale on the ordinary arrangements, and every bound is what bounds() says it is: 2 x a yardstick"""
    fields = ft.VALUE_FIELDS
    print("[k1-rows] yardstick | " + " | ".join(fields))
    for name in ft.ARRANGEMENTS:
        r = ft.yardstick_ratios(name)
        print(f"[k1-rows] yardstick {name} | " + " | ".join(f"{r[f]:.1f}" for f in fields))
    b = ft.bounds()
    print("[k1-rows] bound ordinary | " + " | ".join(f"{b['ordinary'][f]:.1f}" for f in fields))
    for n, d in b["needle"].items():
        print(f"[k1-rows] bound {n} | " + " | ".join(f"{d[f]:.1f}" for f in fields))
    print("[k1-rows] bound lo under a fractional weight | " + ", ".join(f"{n} {v:.1f}" for n, v in b["lo"].items()))
    assert set(b["needle"]) == {"needle"} and set(b["lo"]) == {"filter_fade0.5", "filter_fade1", "faded_below_gate"}
    for f in fields:
        own = max(ft.yardstick_ratios(n)[f] for n in ft.ARRANGEMENTS if n != "needle" and not (f == "lo" and n in b["lo"]))
        assert b["ordinary"][f] == ft.MARGIN_OF_ORDER * own
        # a legal float32 evaluation is a few ulps of the row's scale (measured: at most 18.9, on two machines whose BLAS round
        # differently), so every bound stays below 80 x 2^-24 = 4.8e-6: twenty times under the 1e-4 that held pixel_sizes so far
        assert own <= 40.0, (f, own)
    # the tensor-wide 1e-4 on pixel_sizes, in the same unit: what the row-wise bound is tighter than
    print(f"[k1-rows] parity_utils' 1e-4 on pixel_sizes = {1e-4 / ft.EPS32:.0f} x 2^-24; the row-wise bound {b['ordinary']['psize']:.1f} x kappa")


@pytest.mark.parametrize("name", list(ft.ARRANGEMENTS))
def test_the_float32_oracle_passes_the_checker(name):
    """the checker on the yardstick itself, at every row count (a prefix of the rows): no violation under bounds twice its own
    worst ratio — and the checker's worst ratios are the yardstick's"""
    fam = ft.arrangement(name)
    for raw in ((False, True) if ft.has_raw(fam) else (False,)):
        y = ft.yardstick_of(name, raw=raw)
        rec = ft.rec12_of(y)
        for P in ft.ROW_COUNTS:
            tr, sc = ft.truth_of(name, P, raw=raw)
            bad, worst = ft.check(rec[:P], y["radii"][:P], y["pixel_sizes"][:P], tr, sc, ft.bound_of(name))
            assert not bad, (name, raw, P, bad[:4])
        for f in ft.VALUE_FIELDS:
            assert worst[f] <= ft.yardstick_ratios(name)[f] + 1e-9
    # a record that was never written does not pass
    tr, sc = ft.truth_of(name)
    y = ft.yardstick_of(name)
    rec = ft.rec12_of(y)
    live = np.nonzero(tr["radii"] > 0)[0]
    rec[live[0], 6] = np.nan
    bad, _ = ft.check(rec, y["radii"], y["pixel_sizes"], tr, sc, ft.bound_of(name))
    assert [b for b in bad if b[0] == "r" and b[1] == live[0]]


# ---- (3) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ft.ARRANGEMENTS))
def test_arrangement_keeps_its_promises(name):
    fam = ft.arrangement(name)
    n = fam["n"]
    assert n <= ft.P_MAX
    variants = [fam["inputs"]]
    if ft.has_raw(fam):
        a = ft.activate(ft.raw_leaves(fam["inputs"]), fam["inputs"], torch.float64)
        variants.append({k: (v.to(torch.float32) if torch.is_tensor(v) and v.dtype == torch.float64 else v) for k, v in a.items()})
    for inp in variants:
        for what, good in ft.tie_margins(fam, inp).items():
            assert good.all(), (name, what, np.nonzero(~good)[0][:8])
    tr, _ = ft.truth_of(name, n)
    live = tr["radii"] > 0
    assert np.array_equal(live, np.asarray(fam["expect"]["rendered"]))
    exact = tr["radius_lo"] == tr["radius_hi"]
    print(f"[k1-rows] {name}: {int(live.sum())} of {n} rows rendered, {int((tr['unbounded'] & live).sum())} unbounded, "
          f"radii held exactly on {int((exact & live).sum())}, least |negative-definite test| {np.abs(tr['nd_rel'][live]).min():.2e} of sA sC")
    assert (exact | ~live).all() or name == "giant"
    assert (tr["radius_hi"] - tr["radius_lo"] <= 2e-3 * tr["radius_hi"]).all()
    for raw in ((False, True) if ft.has_raw(fam) else (False,)):
        t2, _ = ft.truth_of(name, raw=raw)
        assert not (t2["unbounded"] & (t2["radii"] > 0)).any()           # no arrangement has an unbounded row today
    if name.startswith("sparse_"):
        full, _ = ft.truth_of(name)
        alive = full["radii"] > 0
        layout = fam["expect"]["layout"]
        for w, planted in enumerate(layout):
            want = ft.SURVIVORS[planted]()[:min(64, ft.P_MAX - 64 * w)]
            assert np.array_equal(alive[64 * w:64 * w + 64], want), (name, w, planted)
            rows = 64 * w + np.nonzero(want)[0]
            rgb = np.stack([full[c][rows] for c in "rgb"], axis=1)
            d = np.abs(rgb[:, None, :] - rgb[None, :, :]).max(axis=2) + np.eye(len(rows))
            assert len(rows) < 2 or d.min() > ft.DISTINCT, (name, w, d.min())
            assert not full["sh_clamped"][rows].any()
        kinds = fam["expect"]["kind"]
        for k in ("behind", "offscreen", "filtered"):
            assert (kinds == k).sum() >= 20, k
        assert (full["weight"][kinds == "filtered"] == 0).all() and (full["pixel_sizes"][kinds == "filtered"] > 0).all()
        assert (full["pixel_sizes"][kinds == "offscreen"] > 0).all()     # culled later: the size is still formed
    if name == "faded_below_gate":
        below = fam["expect"]["below"]
        v_eff = 255.0 * tr["o_eff"]
        assert (255.0 * fam["inputs"]["opacities"].numpy() > 1 + ft.MARGIN).all()
        assert (v_eff[below] < 1 - ft.MARGIN).all() and (v_eff[~below] > 1 + ft.MARGIN).all() and below.sum() == 16
        assert np.array_equal(tr["gate_eff"], ~below)
        assert live.all() and (tr["pixel_sizes"] > 0).all() and (tr["tau2"][below] == 1.0).all() and (tr["tau2"][~below] < 0).all()
        assert np.allclose(tr["weight"], fam["expect"]["weight"], rtol=0, atol=2e-6)
        twins = lambda v: np.array_equal(np.asarray(v)[0::2], np.asarray(v)[1::2])
        assert twins(fam["inputs"]["means3D"]) and twins(fam["inputs"]["opacities"]) and twins(fam["inputs"]["scales"])


def test_sparse_arrangements_cover_the_layouts():
    planted = {s for n in ft.SPARSE_NAMES for s in ft.arrangement(n)["expect"]["layout"]}
    assert planted == set(ft.SURVIVORS)
    assert ("all", "none", "all") == ft.SPARSE_LAYOUTS["b"][:3]           # a wave with none between two full waves
    combos = {(ft.arrangement(n)["view"]["sh_degree"], ft.arrangement(n)["inputs"]["shs"].shape[1]) for n in ft.SPARSE_NAMES}
    assert combos == {(0, 16), (1, 16), (2, 16), (3, 16), (0, 1), (1, 4), (2, 9)}
    for n in ft.SPARSE_NAMES:                                             # the staged rows: both layouts
        if ft.arrangement(n)["inputs"]["shs"].shape[1] == 16:
            assert n.replace("sparse_a", "sparse_b") in ft.ARRANGEMENTS and n.replace("sparse_b", "sparse_a") in ft.ARRANGEMENTS


# ---- (4) ----------------------------------------------------------------------------------------------------------------
def _todays_assertions(name, rec, radii, psz):
    """(image max abs difference, worst pixel_sizes error in check_forward's unit, radii equal) of the mutant's records against
    the clean yardstick's: the float64 blend of the records (culling_truth.evaluate) at the arrangement's own W x H"""
    y = ft.yardstick_of(name)
    img = []
    for r12, rad in ((ft.rec12_of(y), y["radii"]), (rec, radii)):
        r = ct.make_records(torch.from_numpy(np.nan_to_num(r12)), torch.from_numpy(np.asarray(rad)))
        img.append(ct.evaluate(r, ft.W, ft.H).image)
    d_img = float((img[0] - img[1]).abs().max())
    d_ps = float((np.abs(psz.astype(np.float64) - y["pixel_sizes"]) / np.maximum(np.abs(y["pixel_sizes"]), 1.0)).max())
    return d_img, d_ps, bool(np.array_equal(radii, y["radii"]))


@pytest.mark.parametrize("mutation", ft.MUTATIONS)
def test_checker_sees_the_mutation(mutation):
    name = ft.MUTANT_ON[mutation]
    rec, radii, psz = ft.mutant(mutation, name)
    tr, sc = ft.truth_of(name)
    bound = ft.bound_of(name)
    bad, worst = ft.check(rec, radii, psz, tr, sc, bound)
    assert bad, (mutation, "not caught")
    rules = sorted({b[0] for b in bad})
    over = {f: worst[f] / bound[f] for f in ft.VALUE_FIELDS if worst[f] > bound[f]}
    d_img, d_ps, same_radii = _todays_assertions(name, rec, radii, psz)
    seen = d_img > FWD_ATOL or d_ps > 1e-4 or not same_radii
    print(f"[k1-rows] mutant {mutation} on {name}: caught by {rules}; margin over the bound "
          + (", ".join(f"{f} x{v:.3g}" for f, v in over.items()) or "(a tau2 rule, absolute)")
          + f"; today's assertions: image {d_img:.2e} (bound {FWD_ATOL:g}), pixel_sizes {d_ps:.2e} (bound 1e-4), radii "
          + ("equal" if same_radii else "differ") + (" -> SEEN" if seen else " -> MISSED"))
    want = {"colours_swapped": "r", "second_half_from_neighbour": "r", "lo_without_weight": "lo", "conB_sign": "Bh",
            "lowpass_one_diagonal": "C", "px_centre_dropped": "px", "modifier_once": "A",
            "tau2_without_margin": "tau2 off its documented value", "conic_1e-5_off": "A"}[mutation]
    assert want in rules, (mutation, rules)
    if mutation == "colours_swapped":                                     # the explicit check names the two rows
        pairs = ft.colour_swaps(rec, tr)
        assert len(pairs) == 2 and pairs[0][:2] == pairs[1][:2][::-1], pairs
        return
    # the same mistake on ONE row, the faintest one it changes (least blend weight summed over the image): the row-wise
    # criterion does not care how much of the image a row carries
    y = ft.yardstick_of(name)
    clean = ft.rec12_of(y)
    changed = np.nonzero((tr["radii"] > 0) & (y["radii"] > 0) & (clean.view(np.uint32) != rec.view(np.uint32)).any(axis=1))[0]
    r = ct.make_records(torch.from_numpy(clean), torch.from_numpy(y["radii"]))
    wsum = np.full(len(clean), np.inf)
    wsum[r.ids.numpy()] = ct.evaluate(r, ft.W, ft.H).wsum.numpy()
    i = changed[np.argmin(wsum[changed])]
    one, one_ps = clean.copy(), y["pixel_sizes"].copy()
    one[i], one_ps[i] = rec[i], psz[i]
    bad1, _ = ft.check(one, y["radii"], one_ps, tr, sc, bound)
    d_img, d_ps, _ = _todays_assertions(name, one, y["radii"], one_ps)
    seen = d_img > FWD_ATOL or d_ps > 1e-4
    print(f"[k1-rows] mutant {mutation} on row {i} of {name} alone (blend weight sum {wsum[i]:.3g}): caught by "
          f"{sorted({b[0] for b in bad1})}; today's assertions: image {d_img:.2e}, pixel_sizes {d_ps:.2e}" + (" -> SEEN" if seen else " -> MISSED"))
    assert bad1 and {b[1] for b in bad1} == {i}, (mutation, i, bad1[:4])

"""preprocess_kernel (K1) one Gaussian at a time: the twelve floats of every record, `radii` and `pixel_sizes` against the
float64 truth of tests/per_gaussian_forward_truth.py, every row relative to ITS OWN scale

    |got - truth| <= bound[field] x 2^-24 x scale[row, field]

over the 22 row families of per_gaussian_truth, the sparse_* arrangements (planted survivor sets per 64-row wave, pairwise
distinct colours: the SH staging) and faded_below_gate, at row counts that leave the last wave and the last workgroup partly
filled, through every entry that runs K1:

    only            msgs_preprocess_only by ctypes into NaN-filled buffers of its own, twice
    plain           GaussianRasterizer.forward on the activated inputs (the autograd node's ctx.state[0])
    chained         render() on raw leaves with the reference's getters recognised: the concatenated SH rows ...
    chained_split   ... and the split features_dc / features_rest rows
    getters_plain   render() on the same leaves with the recognition off
    fused           render_fused(): the activations inside K1, twice

The families with precomputed covariance / colour take the first two with those inputs; the raw-leaf entries take the
arrangements in the stored layout (scales, rotations, K = 16).  The truth of an entry is formed from the numbers that entry
reads: the family's float32 inputs; the getters' float32 results as the device evaluated them; for `fused` the float64 getters
on the float32 leaves.  Entries that receive bit-equal activated inputs must produce bit-identical records, and so must two
runs of one entry.

bound = 2 x the float32 oracle's own worst ratio (per_gaussian_forward_truth.bounds(): computed there from the oracle's float32
evaluation, never from a kernel's output).  Achieved ratios: profiles/per_gaussian_forward_notes.md."""
import functools
import math

import numpy as np
import pytest
import torch

import per_gaussian_forward_truth as ft

pytestmark = pytest.mark.gpu

ACHIEVED = {}        # (arrangement, entry group, field) -> worst ratio over everything run so far
BG = torch.tensor([0.2, 0.1, 0.3])


def _settings(fam):
    import diff_gaussian_rasterization as dgr
    cam = fam["cam"].to("cuda")
    return dgr.GaussianRasterizationSettings(
        image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=math.tan(0.5 * cam.FoVx),
        tanfovy=math.tan(0.5 * cam.FoVy), bg=BG.cuda(), scale_modifier=fam["mod"], viewmatrix=cam.world_view_transform,
        projmatrix=cam.full_proj_transform, sh_degree=int(fam["view"]["sh_degree"]), campos=cam.camera_center, prefiltered=False,
        debug=False, **fam["settings"])


def _plain(fam, inp):
    """the plain autograd entry on activated inputs"""
    import diff_gaussian_rasterization as dgr
    from per_gaussian_entry import records_of_render
    d = lambda k: None if inp.get(k) is None else inp[k].to("cuda").contiguous()
    m = d("means3D").requires_grad_(True)
    outs = dgr.GaussianRasterizer(_settings(fam))(
        means3D=m, means2D=torch.zeros_like(m, requires_grad=True), opacities=d("opacities"), shs=d("shs"),
        colors_precomp=d("colors_precomp"), scales=d("scales"), rotations=d("rotations"), cov3D_precomp=d("cov3D_precomp"),
        max_pixel_sizes=d("max_pixel_sizes"), min_pixel_sizes=d("min_pixel_sizes"), base_mask=d("base_mask"))
    assert type(outs[0].grad_fn).__name__ == "_RasterizeGaussiansBackward"
    return records_of_render(outs, m.shape[0])


def _render(entry, fam, pc):
    import diff_gaussian_rasterization as dgr
    from gaussian_renderer import PIPE, render, render_fused
    from per_gaussian_entry import records_of_render
    prev = dgr.chain_reference_getters, dgr._chain_reads_cat
    dgr.chain_reference_getters, dgr._chain_reads_cat = entry.startswith("chained"), entry != "chained_split"
    try:
        fn = render_fused if entry == "fused" else render
        out = fn(fam["cam"].to("cuda"), pc, PIPE, BG.cuda(), scaling_modifier=fam["mod"], **fam["settings"])
    finally:
        dgr.chain_reference_getters, dgr._chain_reads_cat = prev
    want = {"fused": "_RasterizeGaussiansRawBackward", "getters_plain": "_RasterizeGaussiansBackward"}.get(
        entry, "_RasterizeGaussiansChainedBackward")
    assert type(out["render"].grad_fn).__name__ == want, (entry, type(out["render"].grad_fn).__name__)
    return records_of_render(out, pc._xyz.shape[0])


@functools.lru_cache(maxsize=None)
def _getters_on_device(name):
    """(the getters' float32 results on the device at P_MAX rows, their truth, its scale)"""
    from per_gaussian_entry import LeafModel
    view, inp = ft.case(name)
    act = LeafModel(ft.raw_leaves(inp), inp, view["sh_degree"]).activated(inp)
    tr = ft.truth(view, act)
    return act, tr, ft.scale(tr)


def _same_bits(what, a, b):
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        same = x.view(np.uint32) == y.view(np.uint32) if x.dtype == np.float32 else x == y
        if k == 0:                                     # records: the rows that exist (the others hold whatever the buffer held)
            same = same | (a[1] <= 0)[:, None]
        assert same.all(), (what, ("records", "radii", "pixel_sizes")[k], np.nonzero(~same)[0][:8])


def _hold(name, P, group, entry, got, tr, sc):
    rec, radii, psz = got
    bad, worst = ft.check(rec, radii, psz, tr, sc, ft.bound_of(name))
    for f, v in worst.items():
        ACHIEVED[(name, group, f)] = max(ACHIEVED.get((name, group, f), 0.0), v)
    print(f"[k1-rows] {name} P={P} {entry}: " + " ".join(f"{f}={v:.2f}" for f, v in worst.items()))
    assert not bad, (name, P, entry, bad[:6])
    if name.startswith("sparse_"):
        swaps = ft.colour_swaps(rec, tr)
        assert not swaps, (name, P, entry, "a row carries the colour of another row of its wave: (row, whose, own distance, "
                           "distance to that one)", swaps[:4])
    live = tr["radius_hi"] > 0
    assert np.isfinite(rec[live]).all(), (name, P, entry, "a field of a live row was not written")


@pytest.mark.parametrize("P", ft.ROW_COUNTS)
@pytest.mark.parametrize("name", list(ft.ARRANGEMENTS))
def test_every_record_against_its_own_scale(name, P):
    from per_gaussian_entry import LeafModel, family_call, k1_only
    fam = ft.arrangement(name)
    view, inp = ft.case(name, P)
    tr, sc = ft.truth_of(name, P)
    # ---- the family's own activated inputs ----
    call = family_call(fam, inp)
    first, again = k1_only(call), k1_only(call)
    assert (first[1] >= 0).all() and np.isfinite(first[2]).all(), "radii / pixel_sizes of every row are written"
    _hold(name, P, "activated", "only", first, tr, sc)
    _same_bits(f"{name} P={P}: two runs of msgs_preprocess_only", first, again)
    plain = _plain(fam, inp)
    _same_bits(f"{name} P={P}: plain entry vs msgs_preprocess_only", first, plain)
    # ---- the exact parts: the sort key's depth (Q10: SPEC words its float32 order) and a precomputed colour (a copy) ----
    from oracle import torch_oracle as to
    live = first[1] > 0
    depth32 = to.depth_key_f32(inp["means3D"], view["viewmatrix"]).numpy()
    assert np.array_equal(first[0][live, 9].view(np.uint32), depth32[live].view(np.uint32)), "record depth != Q10's float32 depth"
    if inp.get("colors_precomp") is not None:
        want = inp["colors_precomp"].numpy()
        assert np.array_equal(first[0][live, 6:9].view(np.uint32), np.ascontiguousarray(want[live]).view(np.uint32))
    if not ft.has_raw(fam):
        return
    # ---- raw leaves: the getters on the device, then K1 on their results ----
    leaves = ft.raw_leaves(inp)
    pc = LeafModel(leaves, inp, view["sh_degree"])
    act_max, tr_g, sc_g = _getters_on_device(name)
    act = pc.activated(inp)
    for k in ("opacities", "scales", "rotations", "shs"):
        assert torch.equal(act[k], act_max[k][:P]), (k, "the getters' results depend on the row count")
    tr_g, sc_g = ft.cut(tr_g, P), ft.cut(sc_g, P)
    runs = {e: _render(e, fam, pc) for e in ("chained", "chained_split", "getters_plain")}
    _hold(name, P, "getters", "chained", runs["chained"], tr_g, sc_g)
    _same_bits(f"{name} P={P}: chained, split SH rows vs concatenated", runs["chained"], runs["chained_split"])
    _same_bits(f"{name} P={P}: chained vs plain on the getters' results", runs["chained"], runs["getters_plain"])
    # ---- the activations inside K1 ----
    tr_f, sc_f = ft.truth_of(name, P, raw=True)
    fused, fused2 = _render("fused", fam, pc), _render("fused", fam, pc)
    _hold(name, P, "fused", "fused", fused, tr_f, sc_f)
    _same_bits(f"{name} P={P}: two runs of render_fused", fused, fused2)


def test_faded_rows_below_the_gate():
    """255 o > 1 and 255 o w < 1: alive with a pixel size, tau2 exactly 1.0f; the twin on the other side has a level set"""
    from per_gaussian_entry import family_call, k1_only
    fam = ft.arrangement("faded_below_gate")
    view, inp = ft.case("faded_below_gate", fam["n"])
    rec, radii, psz = k1_only(family_call(fam, inp))
    below = fam["expect"]["below"]
    assert (radii > 0).all() and (psz > 0).all()
    assert (rec[below, 11] == np.float32(1.0)).all() and (rec[~below, 11] < 0).all() and (rec[~below, 11] > ft.UNBOUNDED).all()
    assert np.array_equal(psz[0::2].view(np.uint32), psz[1::2].view(np.uint32)), "the pixel size is gated on o, not on o w"


def test_zz_report_achieved():
    """prints the worst achieved ratio per arrangement, entry group and field (profiles/per_gaussian_forward_notes.md); runs last"""
    fields = ft.VALUE_FIELDS + ("pixel_sizes", "tau2")
    b = ft.bounds()
    print("[k1-rows] bound ordinary | " + " | ".join(f"{b['ordinary'][f]:.1f}" for f in ft.VALUE_FIELDS))
    for n, d in b["needle"].items():
        print(f"[k1-rows] bound {n} | " + " | ".join(f"{d[f]:.1f}" for f in ft.VALUE_FIELDS))
    print("[k1-rows] bound lo under a fractional weight | " + ", ".join(f"{n} {v:.1f}" for n, v in b["lo"].items()))
    for name in ft.ARRANGEMENTS:
        for group in ("activated", "getters", "fused"):
            if (name, group, "px") in ACHIEVED:
                print(f"[k1-rows] achieved {name} {group} | " + " | ".join(f"{ACHIEVED[(name, group, f)]:.2f}" for f in fields))
    for f in ft.VALUE_FIELDS:
        rows = [(v, n, g) for (n, g, ff), v in ACHIEVED.items() if ff == f and n != "needle"]
        if rows:
            v, n, g = max(rows)
            print(f"[k1-rows] worst {f}: {v:.2f} x 2^-24 scale on {n} ({g}); bound {ft.bound_of(n)[f]:.1f}")

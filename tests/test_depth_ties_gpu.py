"""SPEC Q10's tie rule on the GPU: Gaussians whose float32 view depths are equal BIT FOR BIT blend in Gaussian-index order.

The scenes (tests/tie_scenes.py) put every Gaussian on one, two or four depth planes — two of the four differ in the lowest key
bit — with a share of culled rows interleaved (key 0xFFFFFFFF: the depth sort's DROP pass) and densify-style clones (SPEC D1:
bit-identical xyz) whose partners sit in different blocks of the sort.  Reversing the index order of such a scene moves every
pixel by far more than the forward tolerance (tests/test_depth_ties_cpu.py asserts that on the CPU), so a kernel that reorders
equal keys anywhere — match-any ranking inside a wave, the per-wave counters inside a block, the histogram and group-sum bases
across blocks, the compaction's device-side count, or a route that re-walks the depth order from a rank in the middle of a tie
group — cannot hide inside the tolerances below.

  * default mode against the float32 oracle at the project's tolerances, every blend kernel, both entries;
  * the verification mode, bit for bit over all pixels (its own stable sort, on tied tile lists);
  * every chunk shape of the compacting depth sort (4, 8 and 16 keys per thread; survivor counts on the chunk edges of the
    passes behind the DROP pass) by bit-identity with the render of the compacted scene;
  * the routes that cut the depth order — the speculative stage 2 and its redo, depth slabs whose split rank lies inside the
    single tie group, the occlusion cut-off with its covers tied to what they hide — by bit-identity with the plain route.

Every test asserts that the depths the op received still hold no more distinct values than the scene has planes (+ the culled
z): the ties survive the model class."""
import ctypes as C

import pytest
import torch

import scenes
import tie_scenes
from parity_utils import PIPE, check_backward, check_forward, hip_render, leaf_space, rel_err, report
from route_utils import (LEAVES, PLAIN, assert_identical, guesses_around, non_speculative, reset_forward_state, result, run)
from test_literal_gpu import GUARD_BWD, GUARD_FWD, TOL_BWD, TOL_FWD

pytestmark = pytest.mark.gpu

# name: (P, W, H, seed, levels, clones); px = 3.0 and a culled share of 0.1 everywhere.  The oracle's own exclusions on these
# inputs (a property of the scenes, counted on the CPU): see the table in _oracle_of's docstring
SCENES = {"one_plane": (1500, 96, 64, 1, tie_scenes.ONE_PLANE, 0.0),
          "four_planes": (3000, 128, 96, 2, tie_scenes.FOUR_PLANES, 0.0),
          "four_planes_clones": (4000, 160, 112, 3, tie_scenes.FOUR_PLANES, 0.5)}
BG = (0.2, 0.5, 0.1)


def _scene(name):
    P, W, H, seed, levels, clones = SCENES[name]
    sc = tie_scenes.tied_scene(P, W, H, seed, levels, culled=0.1, px=3.0, clones=clones)
    return sc, scenes.front_camera(W, H), torch.tensor(BG), scenes.grad_seed(W, H, seed), levels


_ORACLE = {}


def _oracle_of(name, seen, cam, bg, dL, literal=False):
    """the float32 oracle's forward and backward on what the op received, computed once per scene and shared (the activated
    tensors torch hands the op are the same bits in every test of a scene: asserted).

    Fractions the oracle excludes on these inputs, counted on the CPU (budgets: 0.0045 of the pixels, 0.03 of the Gaussians):
      one_plane 0.00049 / 0.0013, four_planes 0.00073 / 0.0030, four_planes_clones 0.00106 / 0.0040"""
    from oracle import oracle_ctypes as oc
    key = (name, literal)
    if key not in _ORACLE:
        if literal:
            with oc.exp_double():
                orc = oc.rasterize(seen, cam, PLAIN, bg)
                og = oc.backward(orc, dL)
        else:
            orc = oc.rasterize(seen, cam, PLAIN, bg)
            og = oc.backward(orc, dL)
        _ORACLE[key] = (orc, og, seen)
    orc, og, first = _ORACLE[key]
    for f in ("means3D", "scales", "rotations", "opacities", "shs"):
        assert torch.equal(getattr(first, f), getattr(seen, f)), (name, f)
    return orc, og


@pytest.fixture()
def blend_kernels(request):
    import diff_gaussian_rasterization as dgr
    gran, gen = request.param
    lib = dgr._C.lib
    pg, pb = lib.msgs_set_blend_granularity(gran), lib.msgs_set_backward_generation(gen)
    yield request.param
    lib.msgs_set_blend_granularity(pg)
    lib.msgs_set_backward_generation(pb)


@pytest.fixture()
def literal():
    import diff_gaussian_rasterization as dgr
    prev = dgr.set_deterministic(True)
    yield
    dgr.set_deterministic(prev)


def _seen(pc, sc):
    """the activated tensors the op receives, as torch evaluates them on the GPU (parity_utils.hip_render): the oracle's inputs"""
    import copy
    with torch.no_grad():
        seen = copy.copy(sc)
        seen.scales, seen.rotations = pc.get_scaling.cpu().contiguous(), pc.get_rotation.cpu().contiguous()
        seen.opacities, seen.shs = pc.get_opacity.cpu().contiguous(), pc.get_features.cpu().contiguous()
        seen.means3D = pc.get_xyz.detach().cpu().contiguous()
    return seen


def _fused_render(sc, cam, bg, dL):
    """what parity_utils.hip_render does, through the raw-parameter entry (render_fused): (outputs, model with .seen, means2D
    gradient)"""
    from gaussian_renderer import render_fused
    from synthetic_model import SyntheticGaussians
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    pc.seen = _seen(pc, sc)
    out = render_fused(cam.to("cuda"), pc, PIPE, bg.cuda(), **PLAIN)
    out["render"].backward(dL.cuda())
    torch.cuda.synchronize()
    return out, pc, out["viewspace_points"].grad


def _render_model(pc, cam, bg, dL):
    """one first-call render (exact buffers, no slabs) of a model that exists already; route_utils.result()"""
    import diff_gaussian_rasterization as dgr
    from gaussian_renderer import render
    prev, dgr.slab_policy = dgr.slab_policy, "never"
    try:
        reset_forward_state()
        out = render(cam, pc, PIPE, bg, **PLAIN)
        out["render"].backward(dL)
        torch.cuda.synchronize()
        return result(out, pc, out["render"].grad_fn, cam.image_width, cam.image_height)
    finally:
        dgr.slab_policy = prev


# ------------------------------------------------------------------------------------------------ default mode vs the oracle ---
@pytest.mark.parametrize("fused", [False, True], ids=["render", "fused"])
@pytest.mark.parametrize("blend_kernels", [(0, 0), (1, 1), (1, 2), (2, 0)], indirect=True,
                         ids=["auto", "quadrant-bwd1", "quadrant-bwd2", "fine"])
@pytest.mark.parametrize("name", list(SCENES))
def test_tied_depths_against_the_oracle(name, blend_kernels, fused):
    """forward <= 1e-5 off the flagged pixels, every gradient tensor <= 1e-4 (max-norm relative) off the flagged Gaussians, the
    default budgets on what is flagged"""
    sc, cam, bg, dL, levels = _scene(name)
    reset_forward_state()
    out, pc, m2 = _fused_render(sc, cam, bg, dL) if fused else hip_render(sc, cam, PLAIN, bg, dL)
    tie_scenes.assert_tied(pc.seen.means3D[:, 2], levels)
    orc, og = _oracle_of(name, pc.seen, cam, bg, dL)
    what = f"ties {name} {'fused' if fused else 'render'} {blend_kernels}"
    check_forward(out, orc, what)
    check_backward(pc, m2, og, what, flagged=orc.borderline_gaussians)


# --------------------------------------------------------------------------------------------------------- verification mode ---
@pytest.mark.parametrize("name", list(SCENES))
def test_tied_depths_in_the_verification_mode(literal, name):
    """set_deterministic(True) against the oracle evaluated the same way (exp in double): tests/test_literal_gpu.py's tolerances
    and regression guards over ALL pixels and ALL Gaussians, no exclusions — the forward is expected bit-identical, which a
    single swapped pair of a tie group breaks wherever the pair overlaps.  literal.hip's own stable sort sees tied tile lists."""
    sc, cam, bg, dL, levels = _scene(name)
    reset_forward_state()
    out, pc, m2 = hip_render(sc, cam, PLAIN, bg, dL)
    tie_scenes.assert_tied(pc.seen.means3D[:, 2], levels)
    orc, og = _oracle_of(name, pc.seen, cam, bg, dL, literal=True)
    what = f"ties {name} literal"
    col = out["render"].detach().cpu()
    d = (col - orc.color).abs().max().item()
    report(what, "forward: max |HIP - oracle| over ALL pixels", d)
    report(what, "forward: pixel channels that differ at all (fraction)", (col != orc.color).float().mean().item())
    assert d <= TOL_FWD, (what, d)
    assert d <= GUARD_FWD, (what, d)
    for key, ref in (("acc_pixel_size", orc.acc_pixel_size), ("depth", orc.depth)):
        dd = (out[key].detach().cpu() - ref).abs().max().item()
        assert dd <= TOL_FWD * max(ref.abs().max().item(), 1.0), (what, key, dd)
    assert torch.equal(out["radii"].cpu(), orc.radii), what
    worst = {k: rel_err(got, ref) for k, (got, ref) in leaf_space(pc, m2, og).items()}
    for k, v in worst.items():
        report(what, f"grad {k}: max-norm rel err over ALL Gaussians", v)
    for k, v in worst.items():
        assert v <= TOL_BWD, f"{what}: grad {k} rel err {v:.3e} > {TOL_BWD} ({worst})"
        assert v <= GUARD_BWD, f"{what}: grad {k} rel err {v:.3e} above its regression guard {GUARD_BWD} ({worst})"


# ------------------------------------------------------------------------------------ every shape of the compacting depth sort ---
def _large(P, W, H, culled, seed):
    return lambda: tie_scenes.tied_scene(P, W, H, seed, tie_scenes.TWO_PLANES, culled=culled, px=2.0, sh_degree=0, n_coeffs=1)


def _edge(P, W, H, V, seed):
    return lambda: tie_scenes.exact_survivors_scene(P, W, H, seed, V)


# name: (builder, W, H, seed of dL/dcolor, survivors or None, levels).  Keys per thread of the depth sort (SortGeom): 4 below
# 400 000 Gaussians, 8 below 2 000 000, 16 from there on; a chunk of the passes behind the DROP pass is 256 x that many survivors.
SORT_CASES = {
    "8_keys_per_thread": (_large(450_000, 256, 192, 0.95, 4), 256, 192, 4, None, tie_scenes.TWO_PLANES),
    "16_keys_per_thread": (_large(2_100_000, 320, 240, 0.987, 5), 320, 240, 5, None, tie_scenes.TWO_PLANES),
    "4_keys_V1023": (_edge(5000, 96, 64, 1023, 6), 96, 64, 6, 1023, tie_scenes.ONE_PLANE),
    "4_keys_V1024": (_edge(5000, 96, 64, 1024, 7), 96, 64, 7, 1024, tie_scenes.ONE_PLANE),
    "4_keys_V1025": (_edge(5000, 96, 64, 1025, 8), 96, 64, 8, 1025, tie_scenes.ONE_PLANE),
    "16_keys_V4095": (_edge(2_100_000, 160, 112, 4095, 9), 160, 112, 9, 4095, tie_scenes.ONE_PLANE),
    "16_keys_V4097": (_edge(2_100_000, 160, 112, 4097, 10), 160, 112, 10, 4097, tie_scenes.ONE_PLANE),
}


@pytest.mark.parametrize("case", list(SORT_CASES))
def test_every_sort_shape_is_bit_identical_to_the_compacted_scene(case):
    """The compacted scene sc.subset(keep), keep = the rows that are not culled, holds the same Gaussians in the same index order
    — the same tie order — and goes through the 4-keys-per-thread shape without anything to drop.  It is held to the oracle at
    the project's tolerances; the full scene then has to give the SAME BITS: image, depth, acc_pixel_size, final_T, n_contrib,
    the instance count, and on the rows `keep` radii, pixel sizes and every gradient, with exact zeros on every other row.  An
    equal-key pair swapped by the DROP pass, by a pass that reads its count from the device word, by the 8- or 16-key ranking or
    by the bases across blocks and groups changes pixels and gradients of the full render only.  (The reference entry: the
    sort is the same code behind both.)  The oracle's own exclusions on the compacted scenes, counted on the CPU: <= 0.00065
    of the pixels, <= 0.0030 of the Gaussians.
    Inputs from 16.8 M pairs up (SortGeom::scanned: no compaction, the group-scan kernel) are out of scope here; only
    tests/test_max_size_gpu.py reaches them."""
    from oracle import oracle_ctypes as oc
    from synthetic_model import SyntheticGaussians
    build, W, H, seed, V, levels = SORT_CASES[case]
    sc = build()
    keep = tie_scenes.survivors(sc)
    comp = sc.subset(keep)
    assert comp.P < 400_000 and (V is None or comp.P == V)
    cam = scenes.front_camera(W, H)
    bg, dL = torch.tensor(BG), scenes.grad_seed(W, H, seed)
    # the compacted MODEL is the full model's rows `keep`: the leaves are copied, not derived again from the compacted scene, and
    # what torch's getters hand the op for a row must not depend on where the row sits (a condition of the input)
    full, small = SyntheticGaussians(sc, "cuda"), SyntheticGaussians(comp, "cuda")
    keep_d = keep.cuda()
    with torch.no_grad():
        for n in LEAVES:
            getattr(small, n).copy_(getattr(full, n)[keep_d])
        for n in ("get_xyz", "get_scaling", "get_rotation", "get_opacity", "get_features"):
            assert torch.equal(getattr(full, n)[keep_d], getattr(small, n)), (case, n)
    tie_scenes.assert_tied(full.get_xyz[:, 2], levels)
    # (1) the compacted model against the oracle
    a = _render_model(small, cam.to("cuda"), bg.cuda(), dL.cuda())
    oa, pa, Da, _, ppa = a
    if V is not None:
        assert int((oa["radii"] > 0).sum()) == V            # a condition of the input: every survivor owns a tile
    seen = _seen(small, comp)
    tie_scenes.assert_tied(seen.means3D[:, 2], levels)
    orc = oc.rasterize(seen, cam, PLAIN, bg)
    og = oc.backward(orc, dL)
    what = f"ties sort {case} compacted"
    check_forward(oa, orc, what)
    check_backward(small, oa["viewspace_points"].grad, og, what, flagged=orc.borderline_gaussians)
    # (2) the full model: the same bits
    ob, pb, Db, _, ppb = _render_model(full, cam.to("cuda"), bg.cuda(), dL.cuda())
    print(f"[ties] sort {case}: P {sc.P}, survivors {comp.P}, rendered {int((oa['radii'] > 0).sum())}, D {Da}")
    assert Da == Db, (Da, Db)
    for k in ("render", "depth", "acc_pixel_size"):
        assert torch.equal(oa[k], ob[k]), (case, k)
    assert torch.equal(ppa[0], ppb[0]), (case, "final_T")
    assert torch.equal(ppa[1], ppb[1]), (case, "n_contrib")
    gone = torch.ones(sc.P, dtype=torch.bool, device="cuda")
    gone[keep_d] = False

    def rows(what, full, compacted):
        assert torch.equal(full[keep_d], compacted), (case, what)
        assert not bool(full[gone].any()), (case, what, "rows that are not rendered")          # (any() is false for -0.0 too)
    rows("radii", ob["radii"], oa["radii"])
    rows("pixel_sizes", ob["pixel_sizes"], oa["pixel_sizes"])
    rows("means2D grad", ob["viewspace_points"].grad, oa["viewspace_points"].grad)
    for n in LEAVES:
        rows(n, getattr(pb, n).grad, getattr(pa, n).grad)


# ------------------------------------------------------------------------------------------- routes that cut the depth order ---
@pytest.mark.parametrize("fused", [False, True], ids=["render", "fused"])
def test_speculative_stage2_and_its_redo_on_tied_depths(fused):
    """the four-plane clone scene three times: exact buffers (first call), the speculative stage 2 on buffers sized from that
    count, and a forced redo (a guess whose capacity is below D): identical bits, and each call took the route it claims"""
    import diff_gaussian_rasterization as dgr
    sc, cam, bg, dL, levels = _scene("four_planes_clones")
    cam, bg, dL = cam.to("cuda"), bg.cuda(), dL.cuda()
    n0 = non_speculative()
    first = run(sc, cam, PLAIN, bg, dL, "never", fused=fused)
    assert non_speculative() - n0 == 1
    tie_scenes.assert_tied(first[1].get_xyz[:, 2], levels)
    D = first[2]
    key, = list(dgr._last_instances)
    n0 = non_speculative()
    spec = run(sc, cam, PLAIN, bg, dL, "never", fused=fused, reset=False)
    assert non_speculative() - n0 == 0
    assert_identical(spec, first, ("ties", "speculative", fused))
    # the largest guess whose capacity is below D, halved: the allocator's size classes round the buffers up by less than that
    guess = guesses_around(D)[0] // 2
    dgr._last_instances[key] = guess
    n0 = non_speculative()
    redo = run(sc, cam, PLAIN, bg, dL, "never", fused=fused, reset=False)
    assert non_speculative() - n0 == 1, (guess, D)
    assert_identical(redo, first, ("ties", "redo", fused))
    print(f"[ties] speculative / redo, fused={fused}: D {D}, guess of the redo {guess}")


def test_depth_slabs_split_inside_a_single_tie_group():
    """one plane, 60 000 Gaussians, 3200 tiles: EVERY rendered Gaussian has the same key, so the rank r_A at which slab A ends
    (0 < DA < D) lies strictly inside the one tie group, and slab B's rebuild behind it has to continue in index order"""
    W, H = 1024, 800
    sc = tie_scenes.tied_scene(60_000, W, H, 11, tie_scenes.SLAB_PLANE, culled=0.1, px=4.0, opac=(0.6, 0.99))
    cam = scenes.front_camera(W, H).to("cuda")
    bg, dL = torch.tensor(BG).cuda(), scenes.grad_seed(W, H, 11).cuda()
    one = run(sc, cam, PLAIN, bg, dL, "never")
    tie_scenes.assert_tied(one[1].get_xyz[:, 2], tie_scenes.SLAB_PLANE)
    D = one[2]
    assert one[3]["active"] == 0
    for policy in ("0.1", "0.3"):
        slab = run(sc, cam, PLAIN, bg, dL, policy)
        s = slab[3]
        print(f"[ties] slabs {policy}: D {D}, {s}")
        assert s["active"] == 1 and s["overflow"] == 0 and 0 < s["DA"] < D, (policy, D, s)
        assert_identical(slab, one, ("ties", "slabs", policy))


def _occlusion_stats(ctx):
    import diff_gaussian_rasterization as dgr
    geom = dgr._resolve(ctx.state)[0]
    o = (C.c_int64 * 8)()
    dgr._C.check(dgr._C.lib.msgs_occlusion_stats(C.c_void_p(geom.data_ptr()), geom.numel(), ctx.call.P, o,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "msgs_occlusion_stats")
    return dict(ran=int(o[0]), heavy=int(o[1]), candidates=int(o[2]), closed_blocks=int(o[3]), blocks=int(o[4]))


def test_occlusion_cutoff_with_covers_tied_to_what_they_hide():
    """two planes; 40 screen-filling, nearly opaque giants at z = 2.0 EXACTLY: they tie with each other and with the small
    Gaussians of the near plane, at lower and at higher indices — the cut-off's depth buckets must neither drop a small Gaussian
    that precedes the closing cover in index order nor keep the order of the covers from being the index order"""
    import diff_gaussian_rasterization as dgr
    W, H = 640, 400
    sc = tie_scenes.tied_scene(4000, W, H, 12, tie_scenes.TWO_PLANES, culled=0.1, px=3.0)
    sc = tie_scenes.with_giants(sc, W, H, 12, 40, giant_scale=1.2, giant_opacity=0.9, z=2.0)
    giants = sc.meta["giants"]
    near = torch.nonzero(sc.means3D[:, 2] == 2.0).squeeze(1)
    small = near[~torch.isin(near, giants)]
    assert (small < giants.min()).any() and (small > giants.max()).any() and small.numel() > 1000
    cam = scenes.front_camera(W, H).to("cuda")
    bg, dL = torch.tensor(BG).cuda(), scenes.grad_seed(W, H, 12).cuda()
    res = {}
    for on in (1, 0):
        prev = dgr._C.lib.msgs_set_occlusion(on)
        try:
            res[on] = run(sc, cam, PLAIN, bg, dL, "never")
            stats = _occlusion_stats(res[on][0]["render"].grad_fn)
        finally:
            dgr._C.lib.msgs_set_occlusion(prev)
        if on:
            print(f"[ties] occlusion: D with the cut-off {res[on][2]}, {stats}")
            assert stats["ran"] == 1 and stats["closed_blocks"] > 0, stats
        else:
            print(f"[ties] occlusion: D without {res[on][2]}")
            assert stats["ran"] == 0, stats
    tie_scenes.assert_tied(res[1][1].get_xyz[:, 2], tie_scenes.TWO_PLANES)
    assert res[1][2] <= res[0][2]
    # (the instance counts differ by what the cut removed: everything a pixel walks is the same)
    (oa, pa, _, _, ppa), (ob, pb, _, _, ppb) = res[1], res[0]
    assert_identical((oa, pa, 0, None, ppa), (ob, pb, 0, None, ppb), ("ties", "occlusion"))

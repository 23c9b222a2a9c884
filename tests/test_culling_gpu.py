"""Exact level-set culling on needle footprints, against the op's OWN float32 records evaluated in float64 (tests/culling_truth.py).

Four pieces of code decide which (Gaussian, pixel) pairs exist at all: the per-Gaussian tile count of preprocess_kernel, the
three emit paths of binning.hip (one thread per Gaussian; one wave per Gaussian above 96 instances; emit_heavy_kernel for the
queued Gaussians of blocks that do not fit the LDS stage), the quadrant masks of the 8x8-per-wave blend kernels and the 4x4
sub-block test of the fine kernels.  A pair lost at a needle's tip costs a pixel or two of weight ~1/255 and hides inside every
image tolerance; the culling degrading to "keep the whole rect" changes no output bit at all.  Here both directions are pinned:

  pair counts     must_i <= pixel_count_i <= may_i per Gaussian (contribution scores); weight_sum_i against sum_p w_ip
  forward image   every pixel within FWD_ATOL + the pixel's band-pair weights of sum_i c_i w_ip
  backward walk   dL/dC = 1 on channel 0: the gradient of override_color[:, 0] is sum_p w_ip (the backward kernels' own masks)
  instance count  sum lower_i <= D <= sum upper_i, the per-Gaussian counts (GeomLayout::tiles) and the emitted tile sets (the
                  tile ranges of the binning buffer) tile by tile; sum upper_i <= 0.6 sum rect tiles where the bound must bite
  conditions      band <= 1e-3 of the must pairs and min T >= 1e-2 in the truth (termination never decides membership), the
                  layout guard of the records read, and every family property of the scene — asserted first, from the truth of
                  the records actually produced: a scene that misses its family fails loudly

Scenes (tests/culling_families.py), the smallest at which each path exists, every one under the three blend routes:
  L  thread path, small stage       W  wave path, wide stage       Q  unstaged blocks: emit_heavy_kernel on the key's first call,
  the wave path straight to HBM on the second       T  more than 64 tile rows, staged and (x 4 copies) unstaged
  O  opaque blobs whose level set reaches past the 3-sigma rect
Measured values: profiles/culling_notes.md (printed here with pytest -s, prefix [culling])."""
import pytest
import torch

import culling_families as cf
import culling_truth as ct
import scenes
from parity_utils import BWD_RTOL, FWD_ATOL, PIPE
from route_utils import LEAVES, PLAIN, assert_identical, non_speculative, reset_forward_state, result

pytestmark = pytest.mark.gpu

ROUTES = {"quadrant-bwd1": (1, 1), "quadrant-bwd2": (1, 2), "fine": (2, 0)}
SCENES = {"L": cf.scene_L, "W": cf.scene_W, "Q": cf.scene_Q, "T": cf.scene_T, "T_unstaged": lambda: cf.scene_T(4), "O": cf.scene_O}
TWICE = ("Q", "T_unstaged")              # rendered twice: heavy queue on (first call of the key), then off
SMALL_STAGE, WIDE_STAGE, HEAVY = 3072, 12288, 96


@pytest.fixture(autouse=True)
def _reset_routes():
    import diff_gaussian_rasterization as dgr
    yield
    dgr._C.lib.msgs_set_backward_generation(0)
    dgr._C.lib.msgs_set_blend_granularity(0)


def _a256(n):
    return (n + 255) & ~255


def _render(sc, cam, colour):
    """one forward + backward with dL/dC = 1 on channel 0 -> (route_utils.result(), gradient of the colours)"""
    from gaussian_renderer import render
    from synthetic_model import SyntheticGaussians
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    col = colour.clone().requires_grad_(True)
    out = render(cam, pc, PIPE, torch.zeros(3, device="cuda"), override_color=col, **PLAIN)
    seed = torch.zeros_like(out["render"])
    seed[0] = 1.0
    out["render"].backward(seed)
    torch.cuda.synchronize()
    for n in LEAVES:                                     # (the colours are given: the SH leaves are not part of the graph)
        if getattr(pc, n).grad is None:
            getattr(pc, n).grad = torch.zeros_like(getattr(pc, n))
    return result(out, pc, out["render"].grad_fn, cam.image_width, cam.image_height), col.grad.detach()


def _contributions(sc, cam):
    import diff_gaussian_rasterization as dgr
    from gaussian_renderer import _settings
    from synthetic_model import SyntheticGaussians
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    rs = _settings(cam, pc, PIPE, torch.zeros(3, device="cuda"), 1.0, False, False, 1.0)
    s = dgr.GaussianRasterizer(rs).contributions(pc.get_xyz, pc.get_opacity, scales=pc.get_scaling, rotations=pc.get_rotation,
                                                 max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes,
                                                 base_mask=pc.get_base_mask)
    torch.cuda.synchronize()
    return s


_TRUTH = {}


def _truth_of(name, geom, P, radii, W, H):
    """the truth of a scene's records, computed once and shared by the routes (the records are the same bits on every route:
    asserted)"""
    rec = ct.decode_records(geom, P, radii)
    raw = geom[:48 * P].clone()
    if name not in _TRUTH:
        _TRUTH[name] = (raw, rec, ct.evaluate(rec, W, H))
    assert torch.equal(_TRUTH[name][0], raw), (name, "the records differ between routes")
    return _TRUTH[name][1:]


def _layout_guard(name, rec):
    """reading a private layout needs a guard: tau2 is -log2(255 o) less its documented margin wherever the Gaussian can reach
    1/255, the form is negative definite or tau2 says it is not, colours and depths are what went in"""
    lo = rec.lo.double()
    t = -(ct.LOG2_255 + lo)                                         # -log2(255 o)
    want = t - (1e-5 * t.abs() + 2e-3)
    reach = t < 0                                                   # 255 o > 1: the Gaussian can reach alpha 1/255
    edge = t.abs() < 2e-4                                           # 255 o within rounding of 1: either side is right
    unb = rec.tau2 <= ct.UNBOUNDED
    nd = ct.negative_definite(rec)
    ok_tau = torch.where(unb, reach & ~nd, torch.where(reach, (rec.tau2.double() - want).abs() <= 1e-4, rec.tau2 == 1.0)) | edge
    assert bool(ok_tau.all()), (name, "GaussRec layout: tau2 is not where it was", rec.ids[~ok_tau][:8].tolist())
    assert bool((nd | unb | ~reach).all()), (name, "GaussRec layout: a bounded form that is not negative definite")
    assert bool((rec.lo <= 0).all()) and bool((rec.depth > 0.2).all()), (name, "GaussRec layout: log2 o / depth")


def _tile_sets(binning, D, n_tiles, P, truth):
    """([n, tiles] bool: the tiles each truth row was emitted into, instances in tile ranges) from the binning buffer: uint2
    {start, end} per tile at offset 0, the sorted Gaussian ids behind the ranges and the 64 eight-byte D_trav words"""
    ranges = binning[:8 * n_tiles].view(torch.int32).view(n_tiles, 2).to(torch.int64)
    ids = binning[_a256(8 * n_tiles) + 512:][:4 * max(D, 1)].view(torch.int32).to(torch.int64)
    start, end = ranges[:, 0], ranges[:, 1]
    length = end - start
    assert bool((length >= 0).all()) and bool((end <= D).all()) and int(length.sum()) <= D, "BinningLayout: the tile ranges"
    row_of = torch.full((P,), -1, dtype=torch.int64, device=binning.device)
    row_of[truth.ids] = torch.arange(truth.ids.numel(), device=binning.device)
    sets = torch.zeros(truth.ids.numel(), n_tiles, dtype=torch.bool, device=binning.device)
    tile_of = torch.repeat_interleave(torch.arange(n_tiles, device=binning.device), length)
    pos = torch.cat([torch.arange(int(s), int(e), device=binning.device) for s, e in zip(start.tolist(), end.tolist()) if e > s]) \
        if int(length.sum()) else torch.zeros(0, dtype=torch.int64, device=binning.device)
    g = ids[pos]
    assert bool((g >= 0).all()) and bool((g < P).all()) and bool((row_of[g] >= 0).all()), "BinningLayout: the sorted ids"
    sets[row_of[g], tile_of] = True
    assert int(sets.sum()) == int(length.sum()), "a Gaussian twice in one tile's list"
    return sets, int(length.sum())


def _family_conditions(name, P, truth, rec):
    """what makes the scene the scene it claims to be, from the truth of the records the op produced; returns the notes"""
    lower, upper, rect = truth.lower, truth.upper, truth.rect_tiles
    s_lower, s_upper, s_rect = int(lower.sum()), int(upper.sum()), int(rect.sum())
    heavy = lower > HEAVY
    light = (upper >= 1) & (upper <= HEAVY)
    note = ""
    if name == "L":
        assert rec.n == P == 256
        assert int(upper.max()) <= HEAVY and s_upper <= min(SMALL_STAGE, 8 * P), (int(upper.max()), s_upper)
        note = "thread path (every upper_i <= 96), small stage (sum upper <= 8 P), staged (sum upper <= 3072)"
    if name == "W":
        assert rec.n == P == 256
        assert int(heavy.sum()) >= 16 and s_lower > 8 * P and s_upper <= WIDE_STAGE, (int(heavy.sum()), s_lower, s_upper)
        note = f"wave path ({int(heavy.sum())} with lower_i > 96), wide stage (sum lower > 8 P), staged (sum upper <= 12288)"
    if name in ("Q", "T_unstaged"):
        assert rec.n == P == 512
        blocks = ct.rank_blocks(truth)
        assert len(blocks) == 2
        for b in blocks:
            assert int(lower[b].sum()) > WIDE_STAGE, int(lower[b].sum())
            if name == "Q":
                assert int(heavy[b].sum()) >= 32 and int(light[b].sum()) >= 32, (int(heavy[b].sum()), int(light[b].sum()))
        note = "two rank blocks, each unstaged (sum lower > 12288): " + ", ".join(
            f"{int(lower[b].sum())} instances / {int(heavy[b].sum())} heavy / {int(light[b].sum())} light" for b in blocks)
    if name in ("T", "T_unstaged"):
        rows = (truth.must_tile.reshape(rec.n, truth.gy, truth.gx) > 0).any(2)
        span = torch.where(rows.any(1), rows.shape[1] - rows.int().flip(1).argmax(1) - rows.int().argmax(1), torch.zeros_like(lower))
        tall = heavy & (span > 64)
        assert truth.gy == 69 and int(tall.sum()) >= 16, int(tall.sum())
        note += f"; {int(tall.sum())} with lower_i > 96 over more than 64 tile rows"
    if name == "T":
        assert rec.n == P == 128 and s_lower > 8 * P and s_upper <= WIDE_STAGE, (s_lower, s_upper)
        note = "one rank block, wide stage, staged (sum upper <= 12288)" + note
    if name == "O":
        assert rec.n == P == 24 and bool((rec.lo >= -0.16).all())                  # opacities 0.9 .. 1
        assert int(truth.may_outside.sum()) > 0
        note = f"{int(truth.may_outside.sum())} may pixels outside their rect, {int((truth.may_outside > 0).sum())} Gaussians"
    if name in ("W", "Q", "T", "T_unstaged"):
        assert s_upper <= 0.6 * s_rect, (s_upper, s_rect)
    return note


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", list(SCENES))
def test_culling_against_the_records(name, route):
    _verify(*_run(name, route))


def _run(name, route):
    """the scene under the route, rendered (twice where the second call takes another emit path) and scored -> what _verify reads"""
    import diff_gaussian_rasterization as dgr
    W, H, fam = SCENES[name]()
    P = fam["px"].shape[0]
    sc, cam = cf.scene_of(fam, W, H), scenes.front_camera(W, H).to("cuda")
    colour = (0.2 + 0.8 * torch.rand(P, 3, generator=torch.Generator().manual_seed(7))).cuda()
    gran, gen = ROUTES[route]
    dgr._C.lib.msgs_set_blend_granularity(gran)
    dgr._C.lib.msgs_set_backward_generation(gen)
    prev_slab, dgr.slab_policy = dgr.slab_policy, "never"           # (out of scope here; fewer than 2048 tiles anyway)
    try:
        reset_forward_state()
        assert len(dgr._occ_hot) == 0                                # the key's first call: exact buffers, heavy queue on
        n0 = non_speculative()
        first, grad = _render(sc, cam, colour)
        assert non_speculative() - n0 == 1
        key, = list(dgr._last_instances)
        if name in TWICE:
            assert dgr._heavy_queue_off(key)                         # no block was closed: the queue is off from now on
            n0 = non_speculative()
            second, grad2 = _render(sc, cam, colour)
            assert non_speculative() - n0 == 0                       # ... and the second call took the speculative stage 2
            assert_identical(second, first, ("culling", name, route, "heavy queue off"))
            assert torch.equal(grad, grad2)
        scores = _contributions(sc, cam)
    finally:
        dgr.slab_policy = prev_slab
    out, _, D, _, _ = first
    geom, binning = dgr._resolve(out["render"].grad_fn.state)[:2]
    return (name, route, W, H, P, colour, out["render"].detach(), out["radii"], geom, binning, D, scores.pixel_count,
            scores.weight_sum, grad)


def _verify(name, route, W, H, P, colour, image, radii, geom, binning, D, pixel_count, weight_sum, grad):
    """every check, on what one render left behind (tensors on any device)"""
    rec, truth = _truth_of(name, geom, P, radii, W, H)
    what = f"[culling] {name} {route}:"

    # ---- conditions of the test, first ----
    _layout_guard(name, rec)
    assert torch.equal(torch.stack([rec.r, rec.g, rec.b], 1), colour[rec.ids]), "GaussRec layout: the colours"
    s_must, s_band = int(truth.must.sum()), int(truth.band.sum())
    print(f"{what} band {s_band} of {s_must} must pairs = {s_band / s_must:.2e}; min T {truth.min_T:.4f}")
    assert s_band <= 1e-3 * s_must, (s_band, s_must)
    assert truth.min_T >= 1e-2, truth.min_T
    note = _family_conditions(name, P, truth, rec)
    s_lower, s_upper, s_rect = int(truth.lower.sum()), int(truth.upper.sum()), int(truth.rect_tiles.sum())

    # ---- instance count, per-Gaussian counts, emitted tile sets ----
    n_tiles = truth.gx * truth.gy
    counts = (geom[_a256(48 * P) + _a256(32 * P):][:4 * P].view(torch.int32).to(torch.int64) & 0xFFFFF)
    assert int(counts.sum()) == D and int(counts[radii == 0].sum()) == 0, "GeomLayout: the tile counts"
    sets, emitted = _tile_sets(binning, D, n_tiles, P, truth)
    print(f"{what} D {D} (in tile ranges {emitted}, parked on the sentinel {D - emitted}); sum lower {s_lower}, sum upper "
          f"{s_upper}, sum rect {s_rect}; upper / rect {s_upper / s_rect:.3f}; {note}")
    assert bool((sets.sum(1) <= counts[rec.ids]).all()), "emitted more tiles than counted"
    bad = ct.check(truth, tile_count=counts[rec.ids], tile_set=sets)
    assert bad == [], (len(bad), bad[:6])
    assert s_lower <= D <= s_upper, (s_lower, D, s_upper)
    if name in TWICE:
        assert D > 2 * WIDE_STAGE
    elif name != "O":
        assert (D > 8 * P) == (name != "L")                          # the stage the emit chose

    # ---- pair counts and weight sums (contribution scores) ----
    pix = pixel_count[rec.ids]
    bad = ct.check(truth, pixel_count=pix)
    assert bad == [], (len(bad), bad[:6])
    assert not bool(pixel_count[radii == 0].any())
    tol = BWD_RTOL * float(truth.wsum.max()) + truth.wband
    e_sum = (weight_sum[rec.ids].double() - truth.wsum).abs()
    e_grad = (grad[rec.ids, 0].double() - truth.wsum).abs()
    print(f"{what} pixel counts: sum must {s_must}, counted {int(pix.sum())}, sum may {int(truth.may.sum())}; weight_sum: largest "
          f"error {float(e_sum.max()):.3e}, colour gradient: {float(e_grad.max()):.3e} (allowed {BWD_RTOL * float(truth.wsum.max()):.3e} "
          f"+ band weights; largest sum {float(truth.wsum.max()):.3f})")
    assert bool((e_sum <= tol).all()), (float(e_sum.max()), rec.ids[e_sum > tol][:8].tolist())

    # ---- backward walk ----
    assert bool((e_grad <= tol).all()), (float(e_grad.max()), rec.ids[e_grad > tol][:8].tolist())
    assert not bool(grad[radii == 0].any())

    # ---- forward image ----
    e_img = (image.double() - truth.image).abs()
    over = e_img - truth.band_pix[None]
    print(f"{what} forward: largest |image - truth| {float(e_img.max()):.3e}, beyond the band weights {float(over.max()):.3e} "
          f"(allowed {FWD_ATOL:.0e}); pixels beyond {int((over > FWD_ATOL).any(0).sum())} of {W * H}; first-order worst case of the "
          f"float32 exponents {float(truth.round_pix.max()):.3e}")
    assert bool((over <= FWD_ATOL).all()), float(over.max())

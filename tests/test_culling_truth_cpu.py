"""The float64 culling truth (tests/culling_truth.py) tested on its own, without a GPU: synthetic float32 records of the needle
families (tests/culling_families.py: sigma_major 3 .. 10^4 px, aspect 1 .. 10^3.5, every angle incl. 0/45/90/135 -+ 1e-3 degrees,
centres on tile borders and up to 20 000 px off-screen, opacities 0.0045 .. 1), built directly in 2-D, seeded.

The GPU tests (tests/test_culling_gpu.py) hold the op to this reference; here the reference is held to brute force, to its own
definitions and to the faults it has to catch."""
import numpy as np
import pytest
import torch

import culling_families as cf
import culling_truth as ct

W, H = 256, 192


def _records(fam):
    rec12, radii = cf.synthetic_records(fam)
    return ct.make_records(rec12, radii)


@pytest.fixture(scope="module")
def wide():
    """the prototype's families at full range: 320 footprints on 256 x 192"""
    fam = cf.concat(cf.needles(200, W, H, 1, opacity=(0.0045, 1.0), off=0.25),
                    cf.needles(120, W, H, 2, s_major=(3.0, 60.0), s_minor=(0.6, 60.0), opacity=(0.0045, 1.0), off=0.0))
    # eight of them along the axes -+ 1e-3 degrees from 8 000 .. 20 000 px off-screen, opaque enough to reach the image
    far = np.arange(8)
    fam["s1"][far], fam["s2"][far], fam["opacity"][far] = 1e4, np.linspace(0.6, 20.0, 8), 0.7
    fam["theta"][far] = np.asarray([0.0, 0.001, 179.999, 0.0, 90.0, 90.001, 89.999, 90.0])
    d = np.linspace(8000.0, 20000.0, 8) * np.asarray([1, -1, 1, -1, 1, -1, 1, -1])
    fam["px"][far] = np.where(far < 4, W / 2 + d, np.linspace(20.0, 230.0, 8))
    fam["py"][far] = np.where(far < 4, np.linspace(20.0, 170.0, 8), H / 2 + d)
    rec = _records(fam)
    return fam, rec, ct.evaluate(rec, W, H)


@pytest.fixture(scope="module", params=["L", "W", "O"])
def scene(request):
    """three of the GPU tests' scenes, on synthetic records"""
    w, h, fam = getattr(cf, "scene_" + request.param)()
    rec = _records(fam)
    return request.param, w, h, rec, ct.evaluate(rec, w, h)


def test_families_cover_what_they_claim(wide):
    fam, rec, tr = wide
    asp = fam["s1"] / fam["s2"]
    assert fam["s1"].min() < 4 and fam["s1"].max() > 5000 and asp.min() < 1.5 and asp.max() > 1000
    assert fam["opacity"].min() < 0.006 and fam["opacity"].max() > 0.8
    for a in cf.SPECIAL_ANGLES:
        assert (np.abs((fam["theta"] - a + 90.0) % 180.0 - 90.0) <= 1.001e-3).any(), a
    off = np.maximum(np.maximum(-fam["px"], fam["px"] - W), np.maximum(-fam["py"], fam["py"] - H))
    assert off.max() > 19000 and int((tr.must[:8] > 0).sum()) >= 6 and ((fam["px"] % 16 == 0) | (fam["py"] % 16 == 0)).sum() > 10
    assert rec.n >= 300 and int((tr.must > 0).sum()) > 200
    assert int(((rec.tau2 > ct.UNBOUNDED) & (rec.tau2 <= 0)).sum()) > 250              # bounded forms: the culling has work to do


def test_rect_maximum_against_brute_force(wide):
    """on a 1/8 px lattice that contains the rectangle's edges and corners: never below the lattice maximum, and above it by no
    more than one lattice step accounts for — the optimum is either a corner (a lattice point), a point of an edge where the
    derivative along the edge vanishes (within 1/16 px of a lattice point: <= |C| or |A| times (1/16)^2), or the centre (gradient
    zero: <= (|A| + 2 |Bh| + |C|) (1/16)^2)"""
    _, rec, _ = wide
    ok = ct.negative_definite(rec)
    g = torch.Generator().manual_seed(3)
    pick = torch.nonzero(ok).squeeze(1)
    pick = pick[torch.randperm(pick.numel(), generator=g)[:120]]
    A, Bh, C = rec.A[pick].double(), rec.Bh[pick].double(), rec.C[pick].double()
    px, py = rec.px[pick].double(), rec.py[pick].double()
    h = 1.0 / 8
    lat = torch.arange(0, 15 + h / 2, h, dtype=torch.float64)
    n_checked = n_inside = 0
    for k in range(8):
        # rectangles of 15 x 15 px (a tile's pixel centres) near the centre, near the major axis far out, and anywhere
        if k < 2:
            x0, y0 = (px - 7).round() + float(8 * k), (py - 7).round() - float(8 * k)
        else:
            x0 = torch.randint(0, W - 15, (pick.numel(),), generator=g).double()
            y0 = torch.randint(0, H - 15, (pick.numel(),), generator=g).double()
        got = ct.rect_form_max(A, Bh, C, px, py, x0, x0 + 15, y0, y0 + 15)
        dx = (px[:, None, None] - (x0[:, None, None] + lat[None, None, :]))
        dy = (py[:, None, None] - (y0[:, None, None] + lat[None, :, None]))
        f = A[:, None, None] * dx * dx + 2 * Bh[:, None, None] * dx * dy + C[:, None, None] * dy * dy
        brute = f.reshape(pick.numel(), -1).max(1).values
        step = (A.abs() + 2 * Bh.abs() + C.abs()) * (h / 2) ** 2
        slack = 1e-12 * (1.0 + brute.abs())
        assert bool((got >= brute - slack).all()), float((brute - got).max())
        assert bool((got <= brute + step + slack).all()), float((got - brute - step).max())
        assert bool((got <= 0).all())
        n_checked += pick.numel()
        n_inside += int((got == 0).sum())
    assert n_checked >= 900 and 0 < n_inside < n_checked


def test_pair_eps_bounds_the_float32_chain(wide):
    """eval_pair's FMA chain, restated in float32 (each fma = the exact product and sum rounded once), against p64 on pairs
    of every record: the allowance holds, and it is not idle (a fifth of it is reached somewhere)"""
    _, rec, _ = wide
    g = np.random.default_rng(4)
    f32, f64 = np.float32, np.float64
    worst = 0.0
    for _ in range(40):
        x = g.integers(0, W, rec.n).astype(f32)
        y = g.integers(0, H, rec.n).astype(f32)
        px, py, A, Bh, C, lo = (getattr(rec, k).numpy() for k in ("px", "py", "A", "Bh", "C", "lo"))
        dx, dy = px - x, py - y                                                   # float32
        dxx, dxy, dyy = dx * dx, dx * dy, dy * dy
        fma = lambda a, b, c: (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)
        p32 = fma(A, dxx, fma(Bh + Bh, dxy, fma(C, dyy, lo))).astype(f64)
        ddx, ddy = px.astype(f64) - x, py.astype(f64) - y
        tA, tB, tC = A.astype(f64) * ddx * ddx, 2.0 * Bh.astype(f64) * ddx * ddy, C.astype(f64) * ddy * ddy
        p64 = tA + tB + tC + lo
        eps = ct.pair_eps(*(torch.from_numpy(v) for v in (tA, tB, tC, lo.astype(f64)))).numpy()
        fin = np.isfinite(p32) & np.isfinite(p64)
        assert fin.sum() > 0.9 * rec.n
        assert (np.abs(p32 - p64)[fin] <= (eps - ct.EPS_ABS)[fin]).all()
        worst = max(worst, float((np.abs(p32 - p64)[fin] / eps[fin]).max()))
    assert 0.05 <= worst <= 1.0, worst


def test_lower_is_at_most_upper(wide, scene):
    for tr in (wide[2], scene[4]):
        assert bool((tr.lower <= tr.upper).all())
        assert bool((tr.upper <= tr.rect_tiles).all()) and bool((tr.must <= tr.may).all())
        assert bool(((tr.must_tile > 0) <= tr.upper_tile).all())                    # tile by tile, not only in number


def test_restated_row_extents_stay_inside_the_bounds(wide, scene):
    """the op's per-row extents restated in float32 (count margin 0.03, emit margin 0.02): lower_i <= emit <= count <= upper_i
    for every footprint, and far fewer tiles than the rects hold"""
    for rec, tr, w, h in ((wide[1], wide[2], W, H), (scene[3], scene[4], scene[1], scene[2])):
        count, emit = ct.row_extent_count(rec, w, h, 0.03), ct.row_extent_count(rec, w, h, 0.02)
        assert ct.check(tr, tile_count=count) == [] and ct.check(tr, tile_count=emit) == []
        assert bool((emit <= count).all())


def test_band_share(wide, scene):
    """at most 1e-3 of the must pairs are undecided: in each scene of the GPU tests, and in the full-range families among the
    footprints whose exponent does not cancel — aspect up to 30, or any aspect within 1e-3 degrees of an axis.  Far from the centre
    of a long OBLIQUE needle the three monomials of the exponent are ~(d / sigma_minor)^2 each and cancel to a few units: float32
    cannot decide those pairs (nor the sign test on the ridge, within ~1e-3 d of it), the band says so — 3 % of their must pairs
    here, reported — and the band condition limits how many such needles a scene may hold (scene L: four)."""
    fam, rec, full = wide
    dev = np.abs((fam["theta"] + 45.0) % 90.0 - 45.0)                                # degrees from the nearest axis
    plain = torch.from_numpy((fam["s1"] / fam["s2"] <= 30.0) | (dev <= 1.001e-3))[rec.ids]
    share = lambda t, m: t.band[m].sum().item() / t.must[m].sum().item()
    assert int(plain.sum()) >= 150 and full.must[plain].sum().item() > 100000 and share(full, plain) <= 1e-3
    name, _, _, _, tr = scene
    everything = torch.ones_like(tr.must, dtype=torch.bool)
    print(f"[culling truth] scene {name}: must {int(tr.must.sum())}, band {int(tr.band.sum())}, share {share(tr, everything):.2e}; "
          f"full-range families: {share(full, plain):.2e} without the long oblique needles, {share(full, ~plain):.2e} on them")
    assert tr.must.sum().item() > 10000 and share(tr, everything) <= 1e-3


def test_transmittance_and_weights_in_list_order():
    """four records on a 32 x 16 image, two of them at the same depth (ties by index), one nearly opaque: final T, min T, the
    weights and the image against a per-pixel loop written out here"""
    fam = cf._pack(px=[9.3, 14.0, 20.5, 12.2], py=[7.1, 8.0, 6.4, 9.9], s1=[6.0, 9.0, 5.0, 7.0], s2=[3.0, 2.0, 5.0, 1.5],
                   theta=[20.0, 95.0, 0.0, 140.0], opacity=[0.6, 0.999, 0.3, 0.05], depth=[3.0, 2.0, 3.0, 1.5])
    rec12, radii = cf.synthetic_records(fam)
    perm = torch.tensor([2, 0, 3, 1])                    # rows out of depth order; ids 0 and 1 (rows 2 / 0 of fam) tie at depth 3
    rec = ct.make_records(rec12[perm], radii[perm])
    w, h = 32, 16
    tr = ct.evaluate(rec, w, h, chunk=3)                 # (a chunk boundary inside the list)
    assert [int(rec.ids[i]) for i in tr.order] == [2, 3, 0, 1]
    minx, miny, maxx, maxy = ct.tile_rect(rec, w, h)
    T_ref = np.ones((h, w))
    wsum = np.zeros(4)
    img = np.zeros((3, h, w))
    for yy in range(h):
        for xx in range(w):
            T = 1.0
            for i in tr.order.tolist():
                if not (minx[i] <= xx // 16 < maxx[i] and miny[i] <= yy // 16 < maxy[i]):
                    continue
                dx, dy = float(rec.px[i]) - xx, float(rec.py[i]) - yy
                q = float(rec.A[i]) * dx * dx + 2 * float(rec.Bh[i]) * dx * dy + float(rec.C[i]) * dy * dy
                p = q + float(rec.lo[i])
                if q > 0 or 2.0 ** p < 1 / 255:
                    continue
                a = min(0.99, 2.0 ** p)
                wsum[i] += a * T
                for c, f in enumerate("rgb"):
                    img[c, yy, xx] += float(getattr(rec, f)[i]) * a * T
                T *= 1 - a
            T_ref[yy, xx] = T
    assert np.allclose(tr.final_T.numpy(), T_ref, rtol=1e-12, atol=0)
    assert tr.min_T == pytest.approx(T_ref.min(), rel=1e-12) and tr.min_T < 0.05      # the opaque record's core: 1 - 0.99, and more
    assert np.allclose(tr.wsum.numpy(), wsum, rtol=1e-12) and np.allclose(tr.image.numpy(), img, rtol=1e-12, atol=1e-300)
    assert (wsum > 0).all()


def test_rect_is_the_float32_one():
    """truncation towards zero of the float32 quotient, clamped: centres left of / above the image, a radius ending exactly on a
    tile border, a footprint beyond the grid"""
    rec12 = torch.zeros(4, 12)
    rec12[:, 0] = torch.tensor([-20.0, 40.0, 300.0, 16.0])
    rec12[:, 1] = torch.tensor([8.0, 40.0, 100.0, 16.0])
    rec = ct.make_records(rec12, torch.tensor([12, 8, 20, 16]))
    got = [tuple(int(v[i]) for v in ct.tile_rect(rec, 256, 192)) for i in range(4)]
    # -32/16 = -2 -> 0, (-8+15)/16 -> 0: empty in x.  32/16 = 2 .. (48+15)/16 = 3.  280/16 = 17 -> 16 (clamped), empty.  0 .. 47/16 = 2
    assert got == [(0, 0, 0, 2), (2, 2, 3, 3), (16, 5, 16, 8), (0, 0, 2, 2)]


def test_checker_names_the_dropped_tile(wide):
    """from a tile set that satisfies every bound (the upper tiles), drop ONE tile: the one with the fewest must pixels of all —
    the checker reports exactly that Gaussian and tile, with the number of must pixels, and nothing else"""
    _, _, tr = wide
    tiles = tr.upper_tile.clone()
    assert ct.check(tr, tile_set=tiles, tile_count=tiles.sum(1)) == []
    cand = torch.where(tr.must_tile > 0, tr.must_tile, torch.full_like(tr.must_tile, 1 << 40))
    flat = int(cand.argmin())
    i, t = flat // cand.shape[1], flat % cand.shape[1]
    assert 1 <= int(tr.must_tile[i, t]) <= 3                                        # a tip: a handful of pixels
    tiles[i, t] = False
    got = ct.check(tr, tile_set=tiles)
    assert got == [dict(id=int(tr.ids[i]), kind="lost_tile", tile=(t % tr.gx, t // tr.gx), must_pixels=int(tr.must_tile[i, t]))]
    # the same fault seen through the counts only: that Gaussian's count falls below lower_i
    got = ct.check(tr, tile_count=tiles.sum(1))
    assert [(v["id"], v["kind"]) for v in got] == [(int(tr.ids[i]), "count_below_lower")]
    # ... and through the pixel counts: one must pixel less than must_i
    pix = tr.must.clone()
    pix[i] -= 1
    got = ct.check(tr, pixel_count=pix)
    assert [(v["id"], v["kind"]) for v in got] == [(int(tr.ids[i]), "pixels_below_must")]
    assert ct.check(tr, pixel_count=tr.may) == [] and ct.check(tr, pixel_count=tr.may + 1) != []


def test_checker_rejects_whole_rect_counts(wide, scene):
    """the silent loss of the culling — every Gaussian counted with its whole rect — fails the upper bound on the needles, and
    the sums show it: the upper bounds of the scenes hold well under 0.6 of the rect tiles"""
    for tr in (wide[2], scene[4]):
        got = ct.check(tr, tile_count=tr.rect_tiles)
        assert got and all(v["kind"] == "count_above_upper" for v in got)
        assert len(got) == int((tr.rect_tiles > tr.upper).sum()) and len(got) >= 0.3 * tr.upper.numel()
    name, _, _, _, tr = scene
    if name != "O":                                      # (O: two dozen round blobs, whose level set fills their rect)
        assert tr.upper.sum().item() <= 0.6 * tr.rect_tiles.sum().item()


def test_scene_families_on_synthetic_records(scene):
    """what the GPU tests assert from the op's records, on the synthetic ones: the construction aims where it should"""
    name, w, h, rec, tr = scene
    assert tr.min_T >= 1e-2
    if name == "L":
        assert int(tr.upper.max()) <= 96 and int(tr.upper.sum()) <= min(3072, 8 * rec.n)
    if name == "W":
        assert int((tr.lower > 96).sum()) >= 16 and int(tr.lower.sum()) > 8 * rec.n and int(tr.upper.sum()) <= 12288
    if name == "O":
        assert int(tr.may_outside.sum()) > 0

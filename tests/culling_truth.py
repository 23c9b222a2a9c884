"""A float64 truth for the exact level-set culling, built from the op's OWN float32 records (tests/test_culling_gpu.py) or from
synthetic ones (tests/test_culling_truth_cpu.py).  Plain torch float64, no kernel code; it runs on the device of its inputs.

Culling is a promise about the form the blend kernels evaluate, not about the 3-D scene: a needle's float32 covariance, determinant
and conic differ from their float64 values by per cent, so a truth built from the scene disagrees with the op about where the
footprint IS before any culling happens.  Here the twelve float32 values of a record (GaussRec, the first section of a view's
`geom` buffer)

    px, py, A', Bh', C', log2(o_eff), r, g, b, view depth, pixel size, tau2

are taken as exact inputs.  For pixel (x, y), dx = px - x, dy = py - y (exact in float64):

    q64 = A' dx^2 + 2 Bh' dx dy + C' dy^2          p64 = q64 + log2 o

and the kernels blend the pair iff exp2(p) >= 1/255 and the exponent is not positive (blend.hip eval_pair / forward_walk), inside
the Gaussian's tile rect only (preprocess.hip: floor-divisions of px -+ radius in float32, restated in tile_rect()).

Every pair is classified with the rounding allowance pair_eps():

    must  p64 >= -log2 255 + eps  and  q64 <= -eps       the op has to blend it, whatever its roundings
    may   p64 >= -log2 255 - eps                          the op is allowed to
    band  may and not must                                undecided by float32: a condition of the test, never a tolerance

Per Gaussian: must_i / may_i (pixel counts), lower_i = rect tiles that hold a must pixel, upper_i = rect tiles whose continuous
pixel rectangle, grown by 0.06 px on every side, is reached by the level set with the documented margins doubled (rect_form_max(),
upper_tau()).  The blend weights w_ip = alpha_ip T_ip are formed in list order (record depth ascending, ties by index) in float64."""
import math
from types import SimpleNamespace

import torch

TILE = 16
U = 2.0 ** -24
LOG2_255 = math.log2(255.0)
EPS_REL = 7.0 * U                  # pair_eps()
EPS_ABS = 2.0 ** -20
GROW = 0.06                        # px: twice the count's margin (LEVELSET_MARGIN_COUNT = 0.03)
UNBOUNDED = -1.0e38                # tau2 at or below: "cannot be bounded, keep the whole rect" (the op stores -3e38)
FIELDS = ("px", "py", "A", "Bh", "C", "lo", "r", "g", "b", "depth", "psize", "tau2")


# ----------------------------------------------------------------------------------------------------------------- records ---
def make_records(rec12, radii, ids=None):
    """rec12 [n, 12] float32 in the record's order, radii [n] integer -> the rows with radii > 0 as a namespace of float32
    columns (+ .radii int64, .ids int64: the row numbers in the input, .n)"""
    rec12 = rec12.reshape(-1, 12)
    assert rec12.dtype == torch.float32 and rec12.shape[0] == radii.shape[0]
    keep = torch.nonzero(radii > 0).squeeze(1)
    r = SimpleNamespace(**{f: rec12[keep, k].contiguous() for k, f in enumerate(FIELDS)})
    r.radii = radii[keep].to(torch.int64)
    r.ids = keep if ids is None else ids[keep]
    r.n = int(keep.numel())
    return r


def decode_records(geom, P, radii):
    """the GaussRec array of a view's geom buffer (uint8; GeomLayout::rec == 0, 48 bytes per Gaussian); rows with radii == 0 hold
    nothing meaningful and are left out"""
    assert geom.dtype == torch.uint8 and geom.numel() >= 48 * P
    return make_records(geom[:48 * P].view(torch.float32).view(P, 12).clone(), radii)


def tile_rect(rec, W, H):
    """(minx, miny, maxx, maxy) int64, max exclusive: preprocess.hip's rect in ITS float32 arithmetic — (int) of a float32 quotient
    (truncation), clamped to the grid"""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    rad = rec.radii.to(torch.float32)
    f = lambda v, g: (v / TILE).trunc().to(torch.int64).clamp(0, g)
    return (f(rec.px - rad, gx), f(rec.py - rad, gy), f((rec.px + rad) + float(TILE - 1), gx), f((rec.py + rad) + float(TILE - 1), gy))


def depth_order(rec):
    """positions of the records in list order: depth bits ascending (positive floats: value order), ties by Gaussian index"""
    by_id = torch.argsort(rec.ids, stable=True)
    return by_id[torch.argsort(rec.depth[by_id], stable=True)]


# ------------------------------------------------------------------------------------------------------- rounding allowance ---
def pair_eps(tA, tB, tC, lo):
    """|p_float32 - p64| of one pair, bounded from eval_pair's FMA chain; tA, tB, tC = A' dx^2, 2 Bh' dx dy, C' dy^2 (float64).

    With u = 2^-24 and |d_k| <= u for every rounding (first order; the u^2 terms are 2e-14 relative):
      dx^ = (px - x)(1 + d)            the subtraction that forms dx (x is an integer-valued float32): u; likewise dy
      dxx^ = dx^ dx^ (1 + d)           -> 3u on dx^2; likewise dxy^ and dyy^ (2 Bh' is exact)
      t1 = fma(C', dyy^, lo)           one rounding of the sum: u (|C' dy^2| + |lo|)
      t2 = fma(B2', dxy^, t1)          u (|2 Bh' dx dy| + |C' dy^2| + |lo|)
      p^ = fma(A', dxx^, t2)           u (all four)
    so |p^ - p64| <= 4u |A' dx^2| + 5u |2 Bh' dx dy| + 6u |C' dy^2| + 3u |lo| <= 6u S,  S = the sum of the four magnitudes.
    EPS_REL = 7u leaves one unit for the second-order terms.  The comparison itself adds a constant: v_exp_f32 is good to 1 ulp
    (2^-23 relative in alpha = 1.72e-7 in p), the float32 constant 1/255 is off by at most 2^-24 relative (8.6e-8 in p):
    2.6e-7 together, below EPS_ABS = 2^-20.  The sign test (p^ <= log2 o + 2.4e-7 |log2 o|, rounded: never below log2 o) is
    covered by the same eps on q64: q64 <= -eps implies p^ <= log2 o."""
    return EPS_REL * (tA.abs() + tB.abs() + tC.abs() + lo.abs()) + EPS_ABS


# ------------------------------------------------------------------------------------------------- rectangle maximum, upper ---
def rect_form_max(A, Bh, C, px, py, x0, x1, y0, y1):
    """max of f(d) = A dx^2 + 2 Bh dx dy + C dy^2, d = (px - x, py - y), over x in [x0, x1], y in [y0, y1], for a NEGATIVE
    DEFINITE form (float64, broadcasting): 0 when the centre is inside; otherwise the maximum lies on one of the at most two
    edges facing the centre, where f is a concave parabola whose optimum is clamped to the edge."""
    dxlo, dxhi, dylo, dyhi = px - x1, px - x0, py - y1, py - y0
    zero = torch.zeros_like(dxlo + dylo)
    cx = torch.minimum(torch.maximum(zero, dxlo), dxhi) + zero
    cy = torch.minimum(torch.maximum(zero, dylo), dyhi) + zero
    f = lambda dx, dy: A * dx * dx + 2.0 * Bh * dx * dy + C * dy * dy
    dy_e = torch.minimum(torch.maximum(-Bh * cx / C, dylo), dyhi)                 # on the vertical edge dx = cx
    dx_e = torch.minimum(torch.maximum(-Bh * cy / A, dxlo), dxhi)                 # on the horizontal edge dy = cy
    ninf = torch.full_like(zero, -math.inf)
    fv = torch.where(cx != 0, f(cx, dy_e), ninf)
    fh = torch.where(cy != 0, f(dx_e, cy), ninf)
    return torch.where((cx == 0) & (cy == 0), zero, torch.maximum(fv, fh))


def upper_tau(lo):
    """the level a tile's rectangle maximum has to reach to count for upper_i: -log2(255 o) less the header's documented safety
    margin of tau2 (1e-5 |.| + 2e-3), doubled"""
    t = -(LOG2_255 + lo)
    return t - 2.0 * (1e-5 * t.abs() + 2e-3)


def negative_definite(rec):
    A, Bh, C = rec.A.double(), rec.Bh.double(), rec.C.double()
    return (A < 0) & (C < 0) & (A * C - Bh * Bh > 0)


def upper_tiles(rec, W, H, rect=None):
    """[n, tiles] bool: the tiles that count for upper_i.  A record whose form cannot be bounded (not negative definite, or
    tau2 == -3e38: the op keeps its whole rect by design) counts its whole rect."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    minx, miny, maxx, maxy = rect if rect is not None else tile_rect(rec, W, H)
    dev = rec.px.device
    tx = torch.arange(gx, device=dev)[None, None, :]
    ty = torch.arange(gy, device=dev)[None, :, None]
    inrect = (tx >= minx[:, None, None]) & (tx < maxx[:, None, None]) & (ty >= miny[:, None, None]) & (ty < maxy[:, None, None])
    c = lambda v: v.double()[:, None, None]
    bounded = negative_definite(rec) & (rec.tau2 > UNBOUNDED)
    # (an unbounded record goes through the formula with a harmless stand-in form: its row is replaced below)
    A = torch.where(bounded, rec.A.double(), torch.full_like(rec.A.double(), -1.0))
    Bh = torch.where(bounded, rec.Bh.double(), torch.zeros_like(A))
    C = torch.where(bounded, rec.C.double(), torch.full_like(A, -1.0))
    x0, y0 = (TILE * tx).double(), (TILE * ty).double()
    fmax = rect_form_max(A[:, None, None], Bh[:, None, None], C[:, None, None], c(rec.px), c(rec.py),
                         x0 - GROW, x0 + (TILE - 1) + GROW, y0 - GROW, y0 + (TILE - 1) + GROW)
    hit = fmax >= upper_tau(rec.lo.double())[:, None, None]
    hit = torch.where(bounded[:, None, None], hit, torch.ones_like(hit))
    return (hit & inrect).reshape(rec.n, gy * gx), inrect.reshape(rec.n, gy * gx)


# ------------------------------------------------------------------------------------------------------------------ the truth ---
def evaluate(rec, W, H, chunk=32):
    """Everything the tests compare against, from the records alone.  Returns a namespace; per Gaussian (rows = records, see
    rec.ids): must, may, band (pixel counts, int64), lower, upper, rect_tiles (tile counts), wsum (sum_p w_ip, float64), wband (the
    weights of its band pairs), may_outside (may pixels of the image outside its rect), must_tile [n, tiles] (must pixels per
    tile); per pixel: image [3, H, W] = sum_i c_i w_ip, band_pix [H, W] (weights of the pixel's band pairs), round_pix [H, W] (sum_i w_ip
    ln 2 eps_ip: what the float32 exponents can move the pixel by at worst, to first order — information, no tolerance), final_T; and
    min_T, order (list order)."""
    dev = rec.px.device
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    Wp, Hp = gx * TILE, gy * TILE
    n = rec.n
    rect = tile_rect(rec, W, H)
    up, inrect_t = upper_tiles(rec, W, H, rect)
    x = torch.arange(Wp, device=dev, dtype=torch.float64)[None, None, :]
    y = torch.arange(Hp, device=dev, dtype=torch.float64)[None, :, None]
    inimg = ((x < W) & (y < H))
    must = torch.zeros(n, dtype=torch.int64, device=dev)
    may, band, may_outside = must.clone(), must.clone(), must.clone()
    must_tile = torch.zeros(n, gy * gx, dtype=torch.int64, device=dev)
    wsum = torch.zeros(n, dtype=torch.float64, device=dev)
    wband = wsum.clone()
    image = torch.zeros(3, Hp, Wp, dtype=torch.float64, device=dev)
    band_pix = torch.zeros(Hp, Wp, dtype=torch.float64, device=dev)
    round_pix = band_pix.clone()
    T = torch.ones(Hp, Wp, dtype=torch.float64, device=dev)
    order = depth_order(rec)
    thr = -LOG2_255
    for s in range(0, n, chunk):
        k = order[s:s + chunk]
        c = lambda v: v[k].double()[:, None, None]
        dx, dy = c(rec.px) - x, c(rec.py) - y
        tA, tB, tC, lo = c(rec.A) * dx * dx, 2.0 * c(rec.Bh) * dx * dy, c(rec.C) * dy * dy, c(rec.lo)
        q = tA + tB + tC
        p = q + lo
        eps = pair_eps(tA, tB, tC, lo)
        del tA, tB, tC, dx, dy
        inrect = inrect_t[k].reshape(-1, gy, gx).repeat_interleave(TILE, 1).repeat_interleave(TILE, 2) & inimg
        m_may_all = (p >= thr - eps) & inimg
        m_must = inrect & (p >= thr + eps) & (q <= -eps)
        m_may = inrect & m_may_all
        m_band = m_may & ~m_must
        blend = inrect & (p >= thr) & (q <= 0)
        a_raw = torch.exp2(p).clamp(max=0.99)
        alpha = torch.where(blend, a_raw, torch.zeros_like(a_raw))
        keepT = torch.cumprod(1.0 - alpha, 0)
        T_before = torch.cat([T[None], T[None] * keepT[:-1]], 0)
        w = alpha * T_before
        wb = torch.where(m_band, a_raw * T_before, torch.zeros_like(w))
        T = T * keepT[-1]
        must[k], may[k], band[k] = m_must.sum((1, 2)), m_may.sum((1, 2)), m_band.sum((1, 2))
        may_outside[k] = (m_may_all & ~inrect).sum((1, 2))
        must_tile[k] = m_must.reshape(-1, gy, TILE, gx, TILE).sum((2, 4)).reshape(-1, gy * gx)
        wsum[k], wband[k] = w.sum((1, 2)), wb.sum((1, 2))
        for ch, f in enumerate(("r", "g", "b")):
            image[ch] += (getattr(rec, f)[k].double()[:, None, None] * w).sum(0)
        band_pix += wb.sum(0)
        round_pix += (w * eps).sum(0) * math.log(2.0)
    t = SimpleNamespace(must=must, may=may, band=band, may_outside=may_outside, must_tile=must_tile, wsum=wsum, wband=wband,
                        image=image[:, :H, :W], band_pix=band_pix[:H, :W], round_pix=round_pix[:H, :W], final_T=T[:H, :W], order=order, rect=rect,
                        upper_tile=up, lower=(must_tile > 0).sum(1), upper=up.sum(1), rect_tiles=inrect_t.sum(1), gx=gx, gy=gy,
                        ids=rec.ids)
    t.min_T = float(T[:H, :W].min())
    return t


def rank_blocks(truth, block=256):
    """the records of every block of `block` consecutive depth ranks (the emit's unit of work), as lists of positions: valid
    when every record is in the depth sort, i.e. when every lower_i >= 1 (asserted)"""
    assert bool((truth.lower >= 1).all()), "a record without a must tile may not be in the depth sort"
    return [truth.order[s:s + block] for s in range(0, truth.order.numel(), block)]


# ---------------------------------------------------------------------------------------------------------------- the checker ---
def check(truth, tile_count=None, tile_set=None, pixel_count=None):
    """Violations of the bounds, one dict each ({"id", "kind", ...}); [] = none.
      tile_set    [n, tiles] bool, the tiles each Gaussian was emitted into: a rect tile with a must pixel that is missing ->
                  kind "lost_tile" with the tile (tx, ty) and its number of must pixels; a tile outside upper -> "extra_tile"
      tile_count  [n] tile instances per Gaussian: below lower_i -> "count_below_lower", above upper_i -> "count_above_upper"
      pixel_count [n] blended pixels per Gaussian: below must_i -> "pixels_below_must" (with the tile holding the most must
                  pixels, where to start looking), above may_i -> "pixels_above_may" """
    out = []
    ids = truth.ids.tolist()
    if tile_set is not None:
        lost = (truth.must_tile > 0) & ~tile_set
        for i, t in torch.nonzero(lost).tolist():
            out.append(dict(id=ids[i], kind="lost_tile", tile=(t % truth.gx, t // truth.gx), must_pixels=int(truth.must_tile[i, t])))
        for i, t in torch.nonzero(tile_set & ~truth.upper_tile).tolist():
            out.append(dict(id=ids[i], kind="extra_tile", tile=(t % truth.gx, t // truth.gx), must_pixels=int(truth.must_tile[i, t])))
    if tile_count is not None:
        for i in torch.nonzero(tile_count < truth.lower).squeeze(1).tolist():
            out.append(dict(id=ids[i], kind="count_below_lower", count=int(tile_count[i]), lower=int(truth.lower[i])))
        for i in torch.nonzero(tile_count > truth.upper).squeeze(1).tolist():
            out.append(dict(id=ids[i], kind="count_above_upper", count=int(tile_count[i]), upper=int(truth.upper[i]),
                            rect_tiles=int(truth.rect_tiles[i])))
    if pixel_count is not None:
        for i in torch.nonzero(pixel_count < truth.must).squeeze(1).tolist():
            t = int(truth.must_tile[i].argmax())
            out.append(dict(id=ids[i], kind="pixels_below_must", count=int(pixel_count[i]), must=int(truth.must[i]),
                            tile=(t % truth.gx, t // truth.gx), must_pixels=int(truth.must_tile[i, t])))
        for i in torch.nonzero(pixel_count > truth.may).squeeze(1).tolist():
            out.append(dict(id=ids[i], kind="pixels_above_may", count=int(pixel_count[i]), may=int(truth.may[i])))
    return out


# ------------------------------------------------------------------------------------- the op's row extents, restated (CPU) ---
def row_extent_count(rec, W, H, margin):
    """[n] tile instances by the per-tile-row extents of msgs_internal.h (levelset_rows_setup / levelset_row_interval) restated
    in float32 with the same order of operations, for bounded records (others: the whole rect; a record that can never reach
    1/255, tau2 > 0: 0) — what the count (margin 0.03) and the emit (0.02) evaluate.  Not a truth: a tool to localise a failure
    and to aim scenes without a GPU."""
    f32 = torch.float32
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    minx, miny, maxx, maxy = tile_rect(rec, W, H)
    A, Bh, C, tau2, px, py = (v.to(f32) for v in (rec.A, rec.Bh, rec.C, rec.tau2, rec.px, rec.py))
    det = A * C - Bh * Bh
    Atau = A * tau2
    invA = 1.0 / A
    dymax = torch.sqrt(Atau / det)
    dx_ext = torch.sqrt((C * tau2) / det)
    dyR = -(Bh * dx_ext) / C
    ty = torch.arange(gy, device=px.device)[None, :]
    y0 = (ty * TILE).to(f32)
    col = lambda v: v[:, None]
    m = torch.tensor(margin, dtype=f32)
    dym = col(dymax) + m
    lo = torch.maximum(col(py) - (y0 + float(TILE - 1)), -dym)
    hi = torch.minimum(col(py) - y0, dym)
    dyr = torch.minimum(torch.maximum(col(dyR).expand_as(lo), lo), hi)
    dyl = torch.minimum(torch.maximum(col(-dyR).expand_as(lo), lo), hi)
    fma = lambda a, b, c: (a.double() * b.double() + c.double()).to(f32)          # one rounding (the products are exact in double)
    sr = torch.sqrt(torch.clamp(fma(-col(det), dyr * dyr, col(Atau)), min=0.0))
    sl = torch.sqrt(torch.clamp(fma(-col(det), dyl * dyl, col(Atau)), min=0.0))
    dx_max = (-(col(Bh) * dyr) - sr) * col(invA)
    dx_min = (-(col(Bh) * dyl) + sl) * col(invA)
    xl = (col(px) - dx_max) - m
    xr = (col(px) - dx_min) + m
    tlo = torch.maximum(col(minx), torch.ceil((xl - float(TILE - 1)) * (1.0 / TILE)).clamp(-2 ** 30, 2 ** 30).to(torch.int64))
    thi = torch.minimum(col(maxx) - 1, torch.floor(xr * (1.0 / TILE)).clamp(-2 ** 30, 2 ** 30).to(torch.int64))
    rows = (ty >= col(miny)) & (ty < col(maxy)) & (lo <= hi) & (tlo <= thi)
    cnt = torch.where(rows, thi - tlo + 1, torch.zeros_like(tlo)).sum(1)
    whole = (maxx - minx) * (maxy - miny)
    bounded = (rec.tau2 > UNBOUNDED) & (rec.tau2 <= 0)
    return torch.where(bounded, cnt, torch.where(rec.tau2 > 0, torch.zeros_like(whole), whole))

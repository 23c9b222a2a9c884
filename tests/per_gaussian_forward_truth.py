"""The per-Gaussian forward (K1, preprocess_kernel) one record at a time: the float64 truth of everything K1 writes per Gaussian,
the error scale of every field of every row, the row arrangements K1 is tested on, and the row-wise checker.  Not collected by
pytest: tests/test_per_gaussian_forward_cpu.py holds the truth to the float64 oracle build, measures the float32 yardstick and
shows what the checker sees; tests/test_per_gaussian_forward_gpu.py holds the kernel's records to the truth.

The twelve floats of a record (GaussRec, culling_truth.FIELDS), in the units preprocess.hip writes them:

    px, py        pixel centre convention: ((ndc + 1) W - 1) / 2
    A, Bh, C      -1/2 log2(e) x (conic a, b, c)
    lo            log2(o w), w the multi-scale filter weight
    r, g, b       SH colour + 0.5 clamped at 0, or colors_precomp
    depth         view-space z
    psize         SPEC M1 pixel size, before any filter (gated on 255 o > 1)
    tau2          -log2(255 o w) less (1e-5 |.| + 2e-3) where 255 o w > 1, else exactly 1.0f; -3e38 where the form cannot be bounded

truth() is oracle/torch_oracle.py:preprocess in float64 with its decisions taken from its float32 pass, as everywhere else;
yardstick() is the same in float32: what another float32 evaluation of the same formulas achieves.  Every comparison is

    |got - truth| <= bound[field] x 2^-24 x scale[row, field]

with scale the size of the terms that are added up (not of what is left after they cancel), and bound = 2 x the yardstick's own
worst ratio — bounds() computes it from the yardstick; nothing here is computed from a kernel's output.  `radii` is a ceiling:
it is held to the integers the row's own float32 allowance on 3 sigma leaves (radius_lo .. radius_hi: one integer, i.e. exact
equality, on every rendered row but the giants'); `tau2` has rules of its own (check())."""
import functools
import math
import types

import numpy as np
import torch

import per_gaussian_truth as pt
import preprocess_ties as ties
from culling_truth import FIELDS
from oracle import torch_oracle as to

F32 = np.float32
EPS32 = 2.0 ** -24
KLOG = -0.5 * math.log2(math.e)
LOG2E = math.log2(math.e)
MARGIN = pt.MARGIN
MARGIN_OF_ORDER = 2.0              # another order of the same products, FMA contraction, the 1-ulp __log2f and reciprocal
TAU2_ATOL = 1e-4                   # tests/test_culling_gpu.py:_layout_guard
UNBOUNDED = -1.0e38                # tau2 at or below: the op stores -3e38
RADIUS_ULPS = 16.0                 # radii = ceil(3 sigma) is held to [ceil(3 sigma (1 - t)), ceil(3 sigma (1 + t))], t the row's own
                                   # float32 allowance (_records): one integer — exact — on all but a few rows of the ordinary
                                   # arrangements; the giants' 3 sigma ~ 1e5 .. 1e6 px does not resolve an integer in float32
ND_MARGIN = 1e-5                   # no row's negative-definite test (float32, relative to sA sC) sits nearer to its tie
VALUE_FIELDS = FIELDS[:11]         # tau2 has its own rules
ROW_COUNTS = pt.ROW_COUNTS
P_MAX = pt.P_MAX
W, H = pt.W, pt.H
MUTATIONS = ("colours_swapped", "second_half_from_neighbour", "lo_without_weight", "conB_sign", "lowpass_one_diagonal",
             "px_centre_dropped", "modifier_once", "tau2_without_margin", "conic_1e-5_off")


# ---------------------------------------------------------------------------------------------------------------------------
# truth and yardstick
# ---------------------------------------------------------------------------------------------------------------------------
def _t(v):
    return None if v is None else torch.as_tensor(v)


def _oracle(view, inp, dtype, decisions=None):
    with torch.no_grad():
        return to.preprocess(_t(inp["means3D"]), _t(inp["opacities"]), view, scales=_t(inp.get("scales")),
                             rotations=_t(inp.get("rotations")), cov3D_precomp=_t(inp.get("cov3D_precomp")),
                             shs=_t(inp.get("shs")), colors_precomp=_t(inp.get("colors_precomp")),
                             max_pixel_sizes=_t(inp.get("max_pixel_sizes")), min_pixel_sizes=_t(inp.get("min_pixel_sizes")),
                             base_mask=_t(inp.get("base_mask")), dtype=dtype, _decisions=decisions)


def _filter_terms(view, size, inp):
    """(w, cond) in float64 from pixel sizes `size`: the weight of SPEC M2-M4 and the conditioning of log(w) on the size,
    sum over the binding filters of rel / (fade w_f) — w_f = 1 - (rel - 1) / fade, so d ln w_f = -(rel / (fade w_f)) d ln size"""
    P = size.shape[0]
    w, cond = np.ones(P), np.zeros(P)
    fade = float(view.get("fade_size", 1.0))
    base = np.zeros(P, dtype=bool) if inp.get("base_mask") is None else np.asarray(_t(inp["base_mask"])).astype(bool)
    f64 = lambda k: np.asarray(_t(inp[k]).to(torch.float32)).astype(np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        for on, key, small in ((view.get("filter_small", False), "min_pixel_sizes", True),
                               (view.get("filter_large", False), "max_pixel_sizes", False)):
            if not on or inp.get(key) is None:
                continue
            thr = f64(key)
            act = ((~base) & (thr > 0) & (size < thr)) if small else ((thr > 0) & (size > thr))
            rel = thr / np.maximum(size, 1e-30) if small else size / np.maximum(thr, 1e-30)
            wf = np.clip(1.0 - (rel - 1.0) / fade, 0.0, 1.0) if fade > 0 else np.zeros(P)
            w = np.where(act, w * wf, w)
            cond = cond + np.where(act & (wf > 0) & (wf < 1), rel / (max(fade, 1e-30) * np.maximum(wf, 1e-300)), 0.0)
    return w, cond


def _records(view, inp, dtype):
    pre32 = _oracle(view, inp, torch.float32)
    pre = pre32 if dtype == torch.float32 else _oracle(view, inp, dtype, decisions=pre32)
    npdt = F32 if dtype == torch.float32 else np.float64
    n = lambda t: t.detach().numpy().astype(npdt)
    k = npdt(F32(KLOG)) if npdt is F32 else KLOG
    con, o_eff = n(pre["conic"]), n(pre["opacity"])
    # ---- the decisions K1 takes on o w, from the float32 pass ----
    o32 = pre32["opacity"].numpy().astype(F32)
    c32 = pre32["conic"].numpy().astype(F32)
    with np.errstate(all="ignore"):
        gate_eff = F32(255.0) * o32 > F32(1.0)
        sA, sBh, sC = F32(KLOG) * c32[:, 0], F32(KLOG) * c32[:, 1], F32(KLOG) * c32[:, 2]
        nd_val = sA * sC - sBh * sBh
        nd32 = (sA < 0) & (sC < 0) & (nd_val > 0)
        nd_rel = nd_val.astype(np.float64) / np.maximum(np.abs(sA.astype(np.float64) * sC.astype(np.float64)), 1e-300)
        lo = np.log2(o_eff)
        t_plain = -np.log2(npdt(255.0) * o_eff)
        tau2 = t_plain - (npdt(F32(1e-5)) * np.abs(t_plain) + npdt(F32(2e-3))) if npdt is F32 else \
            t_plain - (1e-5 * np.abs(t_plain) + 2e-3)
        tau2 = np.where(gate_eff, tau2, npdt(1.0)).astype(npdt)
    unbounded = gate_eff & ~nd32
    if npdt is F32:
        tau2 = np.where(unbounded, F32(-3.0e38), tau2)
    rgb = n(pre["rgb"])
    depth32 = pre32["depth32"].numpy()
    ok = (depth32 > 0.2) & pre32["det_nonzero"].numpy()
    a, b, c = (t.detach().numpy().astype(np.float64) for t in pre["cov2"])
    with np.errstate(all="ignore"):
        kappa = (a * c + b * b) / np.abs(a * c - b * b)
        mid = 0.5 * (a + c)
        disc = mid * mid - (a * c - b * b)
        root = np.sqrt(np.maximum(disc, 0.1))
        lam = mid + root
        three_sigma = 3.0 * np.sqrt(lam)                                                                    # Q4
        # what float32 can move lam by: RADIUS_ULPS roundings of mid (and of a, c in it), and the cancellation mid^2 - det under
        # the root — RADIUS_ULPS roundings of mid^2 over 2 root, and never more than the root of that error itself (a round
        # footprint: root ~ 0); nothing where the 0.1 floor of Q4 stands in for the difference
        d_disc = RADIUS_ULPS * EPS32 * mid * mid
        d_root = np.where(disc + d_disc < 0.1, 0.0, np.minimum(d_disc / (2.0 * root), np.sqrt(d_disc)))
        radius_rtol = (RADIUS_ULPS * EPS32 * lam + d_root) / (2.0 * lam)
    size = n(pre["pixel_sizes"])
    w, cond = _filter_terms(view, size.astype(np.float64), inp)
    out = dict(px=n(pre["px"]), py=n(pre["py"]), A=k * con[:, 0], Bh=k * con[:, 1], C=k * con[:, 2], lo=lo.astype(npdt),
               r=rgb[:, 0], g=rgb[:, 1], b=rgb[:, 2], depth=n(pre["depth"]), psize=size, tau2=tau2)
    vis = pre["visible"].numpy()
    with np.errstate(all="ignore"):
        r_lo = np.where(vis, np.ceil(three_sigma * (1.0 - radius_rtol)), 0.0).astype(np.int64)
        r_hi = np.where(vis, np.ceil(three_sigma * (1.0 + radius_rtol)), 0.0).astype(np.int64)
    out.update(radii=pre["radii"].numpy().astype(np.int64), radius_lo=r_lo, radius_hi=r_hi, pixel_sizes=size, ok=ok, visible=pre["visible"].numpy().copy(),
               gate_eff=gate_eff, unbounded=unbounded, nd_rel=nd_rel, t_plain=t_plain.astype(npdt), o_eff=o_eff, weight=w,
               cond_lo=cond, kappa=kappa, cov2=(a, b, c), sh_clamped=pre["clamped"].numpy().copy())
    return out


def truth(view, inputs):
    """The twelve record fields (culling_truth.FIELDS), `radii` and `pixel_sizes` of every row in float64, and what the checks
    need beside them: ok (in front, det != 0: pixel_sizes is formed), visible, gate_eff (255 o w > 1), unbounded (gate_eff and
    the float32 scaled form fails the negative-definite test), nd_rel (that test's value relative to sA sC), t_plain
    (-log2(255 o w)), weight, kappa, cond_lo.  Rows with radii == 0 carry values nobody compares."""
    return _records(view, inputs, torch.float64)


def yardstick(view, inputs):
    """the same in float32 (tau2 = -3e38 where unbounded, as the op stores it)"""
    return _records(view, inputs, torch.float32)


def scale(tr):
    """{field: [P] float64}: what a float32 evaluation of the field can be expected to be right relative to.
      px, py   max(|.|, 1): (ndc + 1) W - 1 adds terms of size W/2 and 1
      A, C     |value| kappa, kappa = (a c + b^2) / |a c - b^2| of the float64 2-D covariance: the determinant's cancellation
      Bh       sqrt(|A C|) kappa
      lo       max(|lo|, 1), and under a binding filter + log2(e) kappa sum_f rel / (fade w_f): w_f = 1 - (rel - 1) / fade is formed
               from the pixel size, whose own relative scale is kappa
      r, g, b  1
      depth    |depth|
      psize    value x kappa (0 where the size is gated off: then it must be exactly 0)"""
    kap = tr["kappa"]
    ab = lambda v: np.abs(np.asarray(v, dtype=np.float64))
    return dict(px=np.maximum(ab(tr["px"]), 1.0), py=np.maximum(ab(tr["py"]), 1.0), A=ab(tr["A"]) * kap,
                Bh=np.sqrt(ab(tr["A"]) * ab(tr["C"])) * kap, C=ab(tr["C"]) * kap,
                lo=np.maximum(ab(tr["lo"]), 1.0) + LOG2E * kap * tr["cond_lo"],
                r=np.ones_like(kap), g=np.ones_like(kap), b=np.ones_like(kap), depth=ab(tr["depth"]), psize=ab(tr["psize"]) * kap)


def rec12_of(y):
    """[P,12] float32 in the record's order from a truth() / yardstick() dict"""
    return np.stack([np.asarray(y[f], dtype=np.float64) for f in FIELDS], axis=1).astype(F32)


def _rows_of(tr, field):
    return tr["ok"] if field == "psize" else tr["radii"] > 0


def ratios(rec12, tr, sc):
    """{field: worst |got - truth| / (2^-24 scale)} over the rows the field is held on (radii > 0; psize: ok)"""
    out = {}
    for k, f in enumerate(VALUE_FIELDS):
        rows = _rows_of(tr, f) & (sc[f] > 0)
        e = np.abs(rec12[rows, k].astype(np.float64) - tr[f][rows])
        out[f] = float((e / (EPS32 * sc[f][rows])).max()) if rows.any() else 0.0
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the checker (the GPU test runs it on the kernel's records, the CPU test on the yardstick and on its mutants)
# ---------------------------------------------------------------------------------------------------------------------------
def check(rec12, radii, pixel_sizes, tr, sc, bound, first=0):
    """(violations, worst ratios).  rec12 [P,12] float32 (rows that were never written: NaN), radii [P], pixel_sizes [P] as an
    entry returned them, tr / sc: truth() / scale() of the same rows, bound: {field: units of 2^-24 scale}.  A violation is
    (field or rule, row + first, ratio or value)."""
    rec12 = np.asarray(rec12, dtype=F32).reshape(-1, 12)
    radii = np.asarray(radii).astype(np.int64).reshape(-1)
    psz = np.asarray(pixel_sizes, dtype=F32).reshape(-1)
    bad = []
    add = lambda what, rows, vals: bad.extend((what, int(i) + first, float(v)) for i, v in zip(rows[:8], np.asarray(vals)[:8]))
    rows = np.nonzero((radii < tr["radius_lo"]) | (radii > tr["radius_hi"]))[0]
    add("radii", rows, radii[rows])
    live = tr["radius_hi"] > 0
    worst = {}
    for k, f in enumerate(VALUE_FIELDS):
        got = rec12[:, k].astype(np.float64)
        held = live                                                 # (psize here is the RECORD's: rows with a record)
        with np.errstate(all="ignore"):
            e = np.abs(got - tr[f])
        lim = bound[f] * EPS32 * sc[f]
        rows = np.nonzero(held & ~(e <= lim))[0]                    # (a NaN — never written — fails)
        with np.errstate(all="ignore"):
            r = e / (EPS32 * sc[f])
        add(f, rows, r[rows])
        sel = held & (sc[f] > 0)
        worst[f] = float(np.nanmax(r[sel])) if sel.any() else 0.0
        if np.isnan(got[held]).any():
            worst[f] = float("inf")
    # ---- pixel_sizes, the output: every row, rendered or not ----
    e = np.abs(psz.astype(np.float64) - tr["pixel_sizes"])
    rows = np.nonzero(tr["ok"] & ~(e <= bound["psize"] * EPS32 * sc["psize"]))[0]
    with np.errstate(all="ignore"):
        r = e / (EPS32 * sc["psize"])
    add("pixel_sizes", rows, r[rows])
    sel = tr["ok"] & (sc["psize"] > 0)
    worst["pixel_sizes"] = float(np.nanmax(r[sel])) if sel.any() else 0.0
    rows = np.nonzero(~tr["ok"] & ~(psz == 0))[0]
    add("pixel_sizes of a row that does not exist", rows, psz[rows])
    rows = np.nonzero(live & (rec12[:, 10].view(np.uint32) != psz.view(np.uint32)))[0]
    add("record psize != pixel_sizes", rows, rec12[rows, 10])
    # ---- tau2, against the truth's o w ----
    tau = rec12[:, 11].astype(np.float64)
    below = live & ~tr["gate_eff"]
    rows = np.nonzero(below & ~(rec12[:, 11] == F32(1.0)))[0]
    add("tau2 below the gate is not 1.0f", rows, tau[rows])
    above = live & tr["gate_eff"]
    unb = tau <= UNBOUNDED
    rows = np.nonzero(above & unb & ~tr["unbounded"])[0]
    add("tau2 unbounded on a negative definite form", rows, tr["nd_rel"][rows])
    fin = above & ~unb
    rows = np.nonzero(fin & ~(tau <= tr["t_plain"]))[0]
    add("tau2 above -log2(255 o w)", rows, tau[rows] - tr["t_plain"][rows])
    rows = np.nonzero(fin & ~(np.abs(tau - tr["tau2"]) <= TAU2_ATOL))[0]
    add("tau2 off its documented value", rows, tau[rows] - tr["tau2"][rows])
    worst["tau2"] = float(np.abs(tau - tr["tau2"])[fin].max()) if fin.any() else 0.0       # (absolute, not a ratio)
    return bad, worst


def colour_swaps(rec12, tr):
    """[(row, the row of its wave whose TRUE colour its colour is nearest to, distance to its own truth, distance to that one)]
    of the live rows whose colour is nearer to another live row of their 64-row wave than to their own: on the sparse
    arrangements (colours of a wave pairwise > DISTINCT apart) this names a staged row that reached the wrong lane"""
    rec12 = np.asarray(rec12, dtype=F32).reshape(-1, 12)
    live = tr["radius_hi"] > 0
    out = []
    for w0 in range(0, rec12.shape[0], 64):
        rows = w0 + np.nonzero(live[w0:w0 + 64])[0]
        if len(rows) < 2:
            continue
        want = np.stack([tr[c][rows] for c in "rgb"], axis=1)
        got = rec12[rows, 6:9].astype(np.float64)
        d = np.abs(got[:, None, :] - want[None, :, :]).max(axis=2)
        near = np.nanargmin(np.where(np.isnan(d), np.inf, d), axis=1)
        for k in np.nonzero(near != np.arange(len(rows)))[0]:
            out.append((int(rows[k]), int(rows[near[k]]), float(d[k, k]), float(d[k, near[k]])))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# arrangements: the 22 families of per_gaussian_truth and the new ones built from their generators
# ---------------------------------------------------------------------------------------------------------------------------
SURVIVORS = {
    "lane0": lambda: np.arange(64) == 0,
    "lane63": lambda: np.arange(64) == 63,
    "even": lambda: np.arange(64) % 2 == 0,
    "allbut31": lambda: np.arange(64) != 31,
    "none": lambda: np.zeros(64, dtype=bool),
    "all": lambda: np.ones(64, dtype=bool),
}
# five waves each (the last one 44 rows at P_MAX = 300): every planted set in a whole wave of one layout or the other, and in
# "b" the wave with none between two full ones
SPARSE_LAYOUTS = {"a": ("lane0", "lane63", "even", "allbut31", "all"), "b": ("all", "none", "all", "lane63", "even")}
COLOUR_STEP = 0.3                  # the planted colours of a wave's lanes: a 4 x 4 x 4 lattice with this step
DISTINCT = 1e-2


def _sparse(deg, K, layout):
    """SH staging: live rows with pairwise distinct colours, dead rows (behind, off screen, filtered to w = 0 in turn) planted so
    that each 64-row wave has the survivor set SPARSE_LAYOUTS[layout] names"""
    name = f"sparse_{layout}_sh{deg}_K{K}"
    rng = np.random.default_rng(40 + 10 * deg + K + (100 if layout == "b" else 0))
    n = P_MAX
    live = np.concatenate([SURVIVORS[s]() for s in SPARSE_LAYOUTS[layout]])[:n]
    tv = pt._view_points(rng, n)
    s, o, q = pt._scales_px(rng, tv, 2.0, 6.0), rng.uniform(0.3, 0.9, n), pt._unit_quats(rng, n)
    kind = np.array(["live"] * n, dtype=object)
    dead = np.nonzero(~live)[0]
    kind[dead] = np.array(["behind", "offscreen", "filtered"], dtype=object)[np.arange(len(dead)) % 3]
    for i in dead:                                                  # (the dead rows of per_gaussian_truth._dead)
        if kind[i] == "behind":
            tv[i, 2] = -rng.uniform(0.5, 3.0) if i % 2 else rng.uniform(0.05, 0.15)
        elif kind[i] == "offscreen":
            tv[i, 0] = (2.2 if i % 2 else -2.2) * pt.TANX * tv[i, 2]
    means = pt._world(tv)
    sh = pt._shs(rng, n, K=K, deg=deg)
    lane = np.arange(n) % 64
    target = 0.6 + COLOUR_STEP * np.stack([lane % 4, (lane // 4) % 4, lane // 16], axis=1) + 0.02 * (np.arange(n) // 64)[:, None]
    sh[:, 0, :] = (target - 0.5) / to.SH_C0
    probe = pt._family(name + "_probe", means, s, q, opac=o, shs=sh, deg=deg)
    size = pt.forward_f32(probe["view"], probe["inputs"])["pixel_sizes"].numpy().astype(np.float64)
    mn = np.where(kind == "filtered", 2.5 * size, -1.0)
    return pt._family(name, means, s, q, opac=o, shs=sh, deg=deg, min_ps=mn,
                      settings=dict(filter_small=True, filter_large=True, fade_size=1.0),
                      expect=dict(rendered=live, kind=kind, layout=SPARSE_LAYOUTS[layout]))


def _faded_below_gate():
    """rows 2k: 255 o = 1.5 .. 4 passes the gate of the pixel size, the filter weight takes 255 o w to 0.55 .. 0.9: alive
    (radii > 0, pixel_sizes > 0), tau2 = 1.0f, in no tile.  rows 2k + 1: the twin — same Gaussian, a threshold that leaves
    255 o w = 1.15 .. 0.9 x 255 o.  k even through the small filter, k odd through the large one (fade 1)."""
    rng = np.random.default_rng(31)
    n = 32
    tv = pt._view_points(rng, n)
    twin = lambda a: np.repeat(a[0::2], 2, axis=0)
    means, s, q = twin(pt._world(tv)), twin(pt._scales_px(rng, tv, 2.0, 6.0)), twin(pt._unit_quats(rng, n))
    v = twin(rng.uniform(1.5, 4.0, n))
    o = v / 255.0
    probe = pt._family("faded_probe", means, s, q, opac=o)
    size = pt.forward_f32(probe["view"], probe["inputs"])["pixel_sizes"].numpy().astype(np.float64)
    below = np.arange(n) % 2 == 0
    v_eff = np.where(below, rng.uniform(0.55, 0.9, n), rng.uniform(1.15, 0.9 * v))
    w = v_eff / v
    small = (np.arange(n) // 2) % 2 == 0
    rel = 2.0 - w                                                    # w = 1 - (rel - 1) / 1
    mn = np.where(small, size * rel, -1.0)
    mx = np.where(small, -1.0, size / rel)
    return pt._family("faded_below_gate", means, s, q, opac=o, min_ps=mn, max_ps=mx,
                      settings=dict(filter_small=True, filter_large=True, fade_size=1.0),
                      expect=dict(rendered=np.ones(n, dtype=bool), below=below, weight=w, v255=v))


SPARSE = [(deg, 16, lay) for deg in (0, 1, 2, 3) for lay in ("a", "b")] + [(deg, (deg + 1) ** 2, "a") for deg in (0, 1, 2)]
ARRANGEMENTS = {name: functools.partial(pt.family, name) for name in pt.FAMILIES}
ARRANGEMENTS.update({f"sparse_{lay}_sh{deg}_K{K}": functools.partial(_sparse, deg, K, lay) for deg, K, lay in SPARSE})
ARRANGEMENTS["faded_below_gate"] = _faded_below_gate
SPARSE_NAMES = tuple(n for n in ARRANGEMENTS if n.startswith("sparse_"))


@functools.lru_cache(maxsize=None)
def arrangement(name):
    fam = ARRANGEMENTS[name]()
    assert fam["name"] == name, (fam["name"], name)
    return fam


def rows_of(fam, P):
    """geometry index of the P rows: the arrangement's rows tiled to P_MAX exactly as per_gaussian_truth.case tiles them"""
    return (np.arange(P_MAX) % fam["n"])[:P]


def take(inp, geo):
    idx = torch.from_numpy(np.asarray(geo))
    return {k: (v[idx].contiguous() if v is not None else None) for k, v in inp.items()}


def case(name, P=P_MAX):
    """(view, inputs [P rows])"""
    fam = arrangement(name)
    return fam["view"], take(fam["inputs"], rows_of(fam, P))


# ---- raw leaves: the entries that evaluate the getters' activations themselves ----
def has_raw(fam):
    """the raw-parameter entries read the reference's stored layout: scales / rotations and K = 16 SH rows"""
    inp = fam["inputs"]
    return "scales" in inp and inp.get("shs") is not None and inp["shs"].shape[1] == 16


def raw_leaves(inp):
    """the float64 inverse activations of the inputs, rounded to float32: log scale, logit opacity, the quaternion itself (a
    unit quaternion is a fixed point of F.normalize up to rounding; any other is normalised: another Gaussian, the same
    check), the SH rows split into dc and rest"""
    f64 = lambda k: inp[k].to(torch.float64)
    o = f64("opacities").reshape(-1)
    leaves = dict(xyz=inp["means3D"].clone(), features_dc=inp["shs"][:, :1].contiguous(), features_rest=inp["shs"][:, 1:].contiguous(),
                  opacity=torch.log(o / (1.0 - o)).to(torch.float32).reshape(-1, 1), scaling=torch.log(f64("scales")).to(torch.float32),
                  rotation=inp["rotations"].clone())
    return leaves


def activate(leaves, inp, dtype):
    """the getters (sigmoid, exp, F.normalize, cat) on the float32 leaves in `dtype` -> an inputs dict"""
    c = lambda k: leaves[k].to(dtype)
    rot = c("rotation")
    rot = rot / rot.norm(dim=1, keepdim=True).clamp_min(1e-12)
    out = dict(inp)
    out.update(means3D=leaves["xyz"], opacities=torch.sigmoid(c("opacity")).reshape(-1), scales=torch.exp(c("scaling")), rotations=rot,
               shs=torch.cat([leaves["features_dc"], leaves["features_rest"]], dim=1))
    return out


@functools.lru_cache(maxsize=None)
def _truth_at_max(name, raw):
    view, inp = case(name)
    if raw:
        inp = activate(raw_leaves(inp), inp, torch.float64)
    tr = truth(view, inp)
    return tr, scale(tr)


def cut(d, P):
    """the first P rows of a truth() / scale() dict"""
    return {k: (tuple(x[:P] for x in v) if isinstance(v, tuple) else v[:P]) for k, v in d.items()}


def truth_of(name, P=P_MAX, raw=False):
    """(truth, scale) of the first P rows; raw: of the float64 getters on the float32 raw leaves.  Computed once at P_MAX:
    every row is a function of its own inputs alone, and every smaller count is a prefix."""
    tr, sc = _truth_at_max(name, bool(raw))
    return cut(tr, P), cut(sc, P)


def yardstick_of(name, raw=False):
    view, inp = case(name)
    if raw:
        inp = activate(raw_leaves(inp), inp, torch.float32)
    return yardstick(view, inp)


# ---------------------------------------------------------------------------------------------------------------------------
# the yardstick's ratios and the bounds derived from them
# ---------------------------------------------------------------------------------------------------------------------------
def has_fractional_weight(name):
    tr, _ = truth_of(name)
    return bool(((tr["weight"] > 0) & (tr["weight"] < 1) & (tr["radii"] > 0)).any())


@functools.lru_cache(maxsize=None)
def yardstick_ratios(name):
    """{field: worst ratio} of the float32 oracle on arrangement `name` at P_MAX rows, the worse of the activated inputs and
    (where the arrangement has them) the float32 getters on the raw leaves; pixel_sizes is held on every ok row"""
    out = {}
    for raw in ((False, True) if has_raw(arrangement(name)) else (False,)):
        tr, sc = truth_of(name, raw=raw)
        y = yardstick_of(name, raw=raw)
        assert ((y["radii"] >= tr["radius_lo"]) & (y["radii"] <= tr["radius_hi"])).all() and np.array_equal(y["visible"], tr["visible"]), name
        r = ratios(rec12_of(y), tr, sc)
        for f, v in r.items():
            out[f] = max(out.get(f, 0.0), v)
    return out


@functools.lru_cache(maxsize=None)
def bounds():
    """{"ordinary": {field: bound}, "needle": {...}, "lo": {arrangement: bound}}:
      ordinary   2 x the yardstick's worst ratio over every arrangement but `needle` (lo: also without the arrangements with a
                 fractional filter weight)
      needle     2 x its own ratios
      lo         of an arrangement with a fractional filter weight: 2 x its own ratio"""
    ordinary, lo = {}, {}
    for name in ARRANGEMENTS:
        if arrangement(name)["needle"]:
            continue
        r = yardstick_ratios(name)
        frac = has_fractional_weight(name)
        for f, v in r.items():
            if f == "lo" and frac:
                lo[name] = MARGIN_OF_ORDER * v
            else:
                ordinary[f] = max(ordinary.get(f, 0.0), MARGIN_OF_ORDER * v)
    needle = {n: {f: MARGIN_OF_ORDER * v for f, v in yardstick_ratios(n).items()} for n in ARRANGEMENTS if arrangement(n)["needle"]}
    return dict(ordinary=ordinary, needle=needle, lo=lo)


def bound_of(name):
    """{field: bound} of arrangement `name`"""
    b = bounds()
    if name in b["needle"]:
        return dict(b["needle"][name])
    out = dict(b["ordinary"])
    if name in b["lo"]:
        out["lo"] = b["lo"][name]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the margins from every forward tie
# ---------------------------------------------------------------------------------------------------------------------------
def tie_margins(fam, inp=None):
    """{comparator: [P] bool — the row keeps MARGIN from that tie (or the comparator does not decide anything about it)} of an
    arrangement's own rows (inp: other activated inputs of the same rows), from the float32 operands of K1's comparators
    (preprocess_ties.k1_f32)"""
    inp = fam["inputs"] if inp is None else inp
    f32 = lambda k: None if inp.get(k) is None else inp[k].to(torch.float32)
    sc = types.SimpleNamespace(means3D=f32("means3D"), opacities=f32("opacities"),
                               scales=None if inp.get("scales") is None else torch.from_numpy(F32(fam["mod"]) * f32("scales").numpy()),
                               rotations=f32("rotations"))
    with np.errstate(all="ignore"):
        k1 = ties.k1_f32(types.SimpleNamespace(scene=sc, cam=fam["cam"], cov3D=f32("cov3D_precomp")))
        m = MARGIN
        front = k1["tz"] > 0.2
        out = dict(near=np.abs(k1["tz"] - 0.2) >= m * 0.2)
        for q, lim in (("txtz", "limx"), ("tytz", "limy")):
            out[q] = ~front | (np.abs(np.abs(k1[q]) - k1[lim]) >= m * k1[lim])
        out["det"] = ~front | (k1["det"] >= 0.08)
        gx, gy = float(W), float(H)
        on = (k1["hi_x"] >= 16 * (1 + m)) & (k1["hi_y"] >= 16 * (1 + m)) & (k1["lo_x"] <= gx * (1 - m)) & (k1["lo_y"] <= gy * (1 - m))
        off = (k1["hi_x"] <= 16 * (1 - m)) | (k1["hi_y"] <= 16 * (1 - m)) | (k1["lo_x"] >= gx * (1 + m)) | (k1["lo_y"] >= gy * (1 + m))
        out["rect"] = ~front | on | off
        v255 = k1["v255"].astype(np.float64)
        out["gate"] = ~front | (np.abs(v255 - 1.0) >= m)
        y = yardstick(fam["view"], inp)
        size = np.where(y["pixel_sizes"] > 0, y["pixel_sizes"].astype(np.float64), np.nan)
        fade = float(fam["settings"]["fade_size"])
        out["filter"] = np.ones_like(front)
        if fam["settings"]["filter_small"] or fam["settings"]["filter_large"]:
            mn, mx = (inp[k].numpy().astype(np.float64) for k in ("min_pixel_sizes", "max_pixel_sizes"))
            for thr, rel in ((mn, mn / size), (mx, size / mx)):
                act = front & (thr > 0)
                raw = 1.0 - (rel - 1.0) / fade
                good = (np.abs(rel - 1.0) >= m) & ((np.abs(raw) >= m) | (rel < 1))
                out["filter"] &= ~act | good
        w = y["weight"]
        out["gate_eff"] = ~front | ~(w > 0) | (np.abs(v255 * w - 1.0) >= m)
        out["nd"] = ~(y["radii"] > 0) | ~y["gate_eff"] | (np.abs(y["nd_rel"]) >= ND_MARGIN)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# deliberate mistakes, applied to the float32 yardstick on the CPU only — never to a kernel
# ---------------------------------------------------------------------------------------------------------------------------
MUTANT_ON = {          # mutation -> the arrangement it is shown on
    "colours_swapped": "sparse_a_sh3_K16",
    "second_half_from_neighbour": "sparse_a_sh3_K16",
    "lo_without_weight": "filter_fade1",
    "conB_sign": "round",
    "lowpass_one_diagonal": "round",
    "px_centre_dropped": "round",
    "modifier_once": "modifier_1.6",
    "tau2_without_margin": "round",
    "conic_1e-5_off": "round",
}


def mutant(mutation, name):
    """(rec12 [P,12] float32, radii, pixel_sizes) of the float32 yardstick of arrangement `name` with one mistake"""
    assert mutation in MUTATIONS
    view, inp = case(name)
    y = yardstick(view, inp)
    rec = rec12_of(y)
    col = {f: k for k, f in enumerate(FIELDS)}
    live = y["radii"] > 0
    with np.errstate(all="ignore"):
        if mutation == "colours_swapped":                          # two live lanes of the one wave that has two neighbours alive
            wave = next(w for w in range(P_MAX // 64) if live[64 * w:64 * w + 64].sum() >= 2)
            i, j = (64 * wave + np.nonzero(live[64 * wave:64 * wave + 64])[0][:2])
            rec[[i, j], col["r"]:col["b"] + 1] = rec[[j, i], col["r"]:col["b"] + 1]
        elif mutation == "second_half_from_neighbour":             # coefficients 8 .. 15 of row i read from row i + 1
            sh = inp["shs"].clone()
            sh[:, 8:] = torch.roll(inp["shs"][:, 8:], -1, dims=0)
            y2 = yardstick(view, dict(inp, shs=sh))
            for f in ("r", "g", "b"):
                rec[:, col[f]] = y2[f]
        elif mutation == "lo_without_weight":
            rec[:, col["lo"]] = np.log2(inp["opacities"].numpy().astype(F32))
        elif mutation == "conB_sign":
            rec[:, col["Bh"]] = -rec[:, col["Bh"]]
        elif mutation == "lowpass_one_diagonal":                   # the +0.3 of Q3 on a alone
            a, b, c = (v.astype(F32) for v in y["cov2"])
            c = c - F32(0.3)
            det = a * c - b * b
            k = F32(KLOG)
            rec[:, col["A"]], rec[:, col["Bh"]], rec[:, col["C"]] = k * (c / det), k * (-b / det), k * (a / det)
        elif mutation == "px_centre_dropped":                      # (ndc + 1) W / 2 without the -1
            rec[:, col["px"]] = rec[:, col["px"]] + F32(0.5)
        elif mutation == "modifier_once":                          # cov = mod s^2 R ...: the modifier's square root in its place
            y2 = yardstick(dict(view, scale_modifier=math.sqrt(float(view["scale_modifier"]))), inp)
            rec = rec12_of(y2)
            rec[:, col["r"]:col["b"] + 1] = rec12_of(y)[:, col["r"]:col["b"] + 1]
            return rec, y2["radii"], y2["pixel_sizes"]
        elif mutation == "conic_1e-5_off":                         # not a formula: the size of mistake the issue is about
            for f in ("A", "Bh", "C"):
                rec[:, col[f]] = rec[:, col[f]] * F32(1.0 + 1e-5)
        elif mutation == "tau2_without_margin":
            rec[:, col["tau2"]] = np.where(y["gate_eff"] & ~y["unbounded"], y["t_plain"], rec[:, col["tau2"]])
    return rec, y["radii"], y["pixel_sizes"]

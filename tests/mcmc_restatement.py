"""The MCMC densification (DESIGN.md SPEC M18) restated in float64 numpy, op by op as the SPEC writes it: the reference the GPU
tests compare ms-gs_amd/host/mcmc.py with.  Model states are the dictionaries of densify_fixtures.make_inputs / snapshot."""
import math

import numpy as np

N_MAX = 51
O_MIN, O_MAX = 0.005, 1.0 - 2.0 ** -24
X_MIN = math.log(O_MIN) - math.log1p(-O_MIN)
X_MAX = math.log(O_MAX) - math.log(2.0 ** -24)
PARAMS = ("xyz", "f_dc", "f_rest", "opacity", "occ_multiplier", "dc_delta", "scaling", "rotation")
COPIED = ("xyz", "f_dc", "f_rest", "occ_multiplier", "dc_delta", "rotation", "target_reso_lvl")


def weights(opacity, dead=None):
    x = np.asarray(opacity, np.float64).reshape(-1)
    with np.errstate(over="ignore"):
        w = 1.0 / (1.0 + np.exp(-x))
    w = np.where(w > 0.0, w, 0.0)
    if dead is not None:
        w = np.where(np.asarray(dead, bool).reshape(-1), 0.0, w)
    return w


def sample(opacity, u, dead=None):
    """(source, count, cdf): draw j takes the first row whose inclusive CDF exceeds u_j * total, the last row of positive weight
    when the product rounds up to the total"""
    w = weights(opacity, dead)
    cdf = np.cumsum(w)
    total = cdf[-1]
    v = np.asarray(u, np.float64) * total
    src = np.searchsorted(cdf, v, side="right")
    src = np.where(src >= w.size, np.flatnonzero(w > 0)[-1], src)
    return src.astype(np.int64), np.bincount(src, minlength=w.size).astype(np.int64), cdf


def relocation(x, s, N):
    """SPEC M18 (b) for logits x [n], log-scales s [n,3] and N [n] (already clamped to N_MAX by the caller or not: clamped here):
    (x_new [n], s_new [n,3], c [n]) in float64"""
    x = np.asarray(x, np.float64).reshape(-1)
    s = np.asarray(s, np.float64).reshape(-1, 3)
    N = np.minimum(np.asarray(N, np.int64).reshape(-1), N_MAX)
    log1mo = -(np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x))))
    o = 1.0 / (1.0 + np.exp(-x))
    l = log1mo / N
    on = -np.expm1(l)
    D = np.zeros_like(x)
    for n in np.unique(N):
        sel = N == n
        acc = np.zeros(int(sel.sum()))
        for i in range(1, int(n) + 1):
            for k in range(i):
                acc += math.comb(i - 1, k) * (-1.0) ** k / math.sqrt(k + 1) * on[sel] ** (k + 1)
        D[sel] = acc
    c = o / D
    x_new = np.where(on < O_MIN, X_MIN, np.where(on > O_MAX, X_MAX, np.log(on) - l))
    return x_new, s + np.log(c)[:, None], c


def _moments(d):
    return [k for k in d if k.startswith("m_") and not k.endswith("_step")]


def _drawn(d, count):
    """the drawn rows and their new float32 values from the OLD state: rows, x_new, s_new, max/min pixel sizes"""
    rows = np.flatnonzero(count > 0)
    xn, sn, c = relocation(d["opacity"][rows, 0], d["scaling"][rows], count[rows] + 1)
    cf = c.astype(np.float32)
    return rows, xn.astype(np.float32), sn.astype(np.float32), d["max_pixel_sizes"][rows] * cf, d["min_pixel_sizes"][rows] * cf


def _update_sources(out, rows, xn, sn, pmax, pmin):
    out["opacity"][rows, 0], out["scaling"][rows] = xn, sn
    out["max_pixel_sizes"][rows], out["min_pixel_sizes"][rows] = pmax, pmin
    for k in _moments(out):
        out[k][rows] = 0


def relocate(d, dead, u):
    """relocate_gs on a state dictionary: (new state, source of every draw, count)"""
    dead = np.asarray(dead, bool).reshape(-1)
    out = {k: np.array(v, copy=True) for k, v in d.items()}
    dead_rows = np.flatnonzero(dead)
    if dead_rows.size == 0 or not (weights(d["opacity"], dead) > 0).any():
        return out, np.zeros(0, np.int64), np.zeros(dead.size, np.int64)
    src, count, _ = sample(d["opacity"], u, dead)
    rows, xn, sn, pmax, pmin = _drawn(d, count)
    at = np.searchsorted(rows, src)
    for k in COPIED:
        out[k][dead_rows] = d[k][src]
    out["opacity"][dead_rows, 0], out["scaling"][dead_rows] = xn[at], sn[at]
    out["max_pixel_sizes"][dead_rows], out["min_pixel_sizes"][dead_rows] = pmax[at], pmin[at]
    out["xyz_gradient_accum"][dead_rows], out["denom"][dead_rows], out["max_radii2D"][dead_rows] = 0, 0, 0
    out["base_gaussian_mask"][dead_rows] = False
    _update_sources(out, rows, xn, sn, pmax, pmin)
    return out, src, count


def add_new(d, cap_max, u, reso_lvl=0):
    """add_new_gs on a state dictionary (u: as many uniforms as rows are added): the new state"""
    P = d["xyz"].shape[0]
    n_new = max(0, min(int(cap_max), int(1.05 * P)) - P)
    out = {k: np.array(v, copy=True) for k, v in d.items()}
    if n_new == 0:
        return out
    src, count, _ = sample(d["opacity"], u)
    rows, xn, sn, pmax, pmin = _drawn(d, count)
    at = np.searchsorted(rows, src)
    _update_sources(out, rows, xn, sn, pmax, pmin)
    new = {k: d[k][src] for k in COPIED}
    new["opacity"], new["scaling"] = xn[at][:, None], sn[at]
    new["max_pixel_sizes"], new["min_pixel_sizes"] = pmax[at], pmin[at]
    # densification_postfix (SPEC D1): moments and statistics of the new rows are zero, column reso_lvl of the old rows' accum /
    # denom is cleared, max_radii2D is zero everywhere, the base mask of new rows is False
    out["xyz_gradient_accum"][:, reso_lvl], out["denom"][:, reso_lvl] = 0, 0
    zeros = lambda k: np.zeros((n_new,) + out[k].shape[1:], out[k].dtype)
    for k in list(out):
        if np.ndim(out[k]) == 0:
            continue
        out[k] = np.concatenate([out[k], new[k].astype(out[k].dtype) if k in new else zeros(k)])
    out["max_radii2D"][:] = 0
    return out


NOISE_SIZES = (1, 65, 4097)
NOISE_GAIN = 5e5 * 0.00016


def noise_inputs(seed, P):
    """float32 inputs of the noise tests: scales over six decades, unnormalised quaternions, a third of the rows each with the
    gate open (o < 0.004), around its threshold, and closed (o >= 0.9)"""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    kind = np.arange(P) % 3 if P > 1 else np.zeros(1, np.int64)
    o = np.where(kind == 0, rng.uniform(5e-4, 4e-3, P), np.where(kind == 1, rng.uniform(4e-3, 0.02, P), rng.uniform(0.9, 0.999, P)))
    return dict(xyz=f32(rng.normal(0, 2, (P, 3))), scaling=f32(np.log(10.0 ** rng.uniform(-4, 2, (P, 3)))),
                rotation=f32(rng.normal(0, 1, (P, 4)) * 10.0 ** rng.uniform(-1, 1, (P, 1))),
                opacity=f32(np.log(o / (1 - o)))[:, None], draws=f32(rng.normal(0, 1, (P, 3))), closed=kind == 2)


def noise(xyz, scaling, rotation, opacity, draws, gain, dtype=np.float64):
    """add_position_noise, every operation in `dtype`, in the order the kernel takes them: (new xyz, error scale per component
    |xyz| + (|R| S^2 |R^T| |xi|) g)"""
    f = lambda a: np.asarray(a, dtype)
    p, l, q, xi, ox = f(xyz), f(scaling), f(rotation), f(draws), f(opacity).reshape(-1)
    one, two = dtype(1), dtype(2)
    nrm = np.maximum(np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]), dtype(1e-12))
    r, x, y, z = (q[:, k] / nrm for k in range(4))
    R = np.empty((p.shape[0], 3, 3), dtype)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)
    s = np.exp(l)
    t = np.stack([((R[:, 0, k] * xi[:, 0] + R[:, 1, k] * xi[:, 1]) + R[:, 2, k] * xi[:, 2]) * (s[:, k] * s[:, k]) for k in range(3)], 1)
    dd = np.stack([(R[:, k, 0] * t[:, 0] + R[:, k, 1] * t[:, 1]) + R[:, k, 2] * t[:, 2] for k in range(3)], 1)
    o = one / (one + np.exp(-ox))
    with np.errstate(over="ignore"):
        g = dtype(gain) / (one + np.exp(dtype(-100) * (dtype(0.005) - o)))
    ta = np.stack([(np.abs(R[:, :, k]) * np.abs(xi)).sum(1) * (s[:, k] * s[:, k]) for k in range(3)], 1)
    scale = np.abs(p) + np.einsum("nkj,nj->nk", np.abs(R), ta) * g[:, None]
    return p + dd * g[:, None], scale

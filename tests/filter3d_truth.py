"""Float64 truth of Mip-Splatting's 3-D smoothing filter (SPEC M16; 4.17), written from the definitions, and the
scene its tests share.  Nothing here touches the library.

Camera n of V has M_n = world_view_transform (a centre p maps to t = [p, 1] M_n), W_n, H_n, fx_n = W_n / (2 tan(FoVx_n / 2)),
fy_n likewise.  With zc = max(t.z, 0.001), x = t.x / zc fx + W / 2, y = t.y / zc fy + H / 2, camera n SEES p iff
    t.z > 0.2   and   -0.15 W <= x <= 1.15 W   and   -0.15 H <= y <= 1.15 H
    rule "per_camera":     nu = max over the seeing cameras of fx_n / t.z
    rule "mip_splatting":  nu = (max over ALL cameras of fx_n) / (min over the seeing cameras of t.z)
valid_points = some camera sees p; a Gaussian no camera sees takes the smallest nu of those that are seen; nobody seen: the
filter is 0.  filter_3D = sqrt(variance) / nu.

The five comparisons are discrete decisions: two float32 evaluations may take one differently when a quantity lies on its
threshold.  sweep() therefore also returns the result with every decision within SLACK x W (x H; x 0.2 for the depth test) of its
threshold taken as passed ("hi") and as failed ("lo"); a Gaussian whose nu changes under either is FLAGGED.

Scene: centres uniform in a ball of radius 14, cameras on a ring of radius 8 in the plane y = 0 looking at the origin, 1920x1080
at f = 1000 px halved (v mod 3) times for camera v — mixed focal lengths, as on MS-GS's image pyramid."""
import math

import torch

import scenes

SLACK = 1e-5
VARIANCE = 0.2
RULES = ("per_camera", "mip_splatting")
BALL_RADIUS = 14.0
RING_RADIUS = 8.0


def centres(P, seed=7, radius=BALL_RADIUS):
    """[P,3] float32, uniform in the ball.  (The default seed is one for which every shape of the GPU tests meets the two
    conditions tests/test_filter3d_cpu.py states on the truth alone: few flagged Gaussians, and none of them near the fallback
    minimum.  Seed 5 misses the second at P = 4099, V = 133.)"""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(P, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    r = radius * torch.rand(P, 1, generator=g, dtype=torch.float64) ** (1.0 / 3.0)
    return (d * r).float().contiguous()


def cameras(V, equal_focals=False):
    """camera v of the ring at 1920x1080 / 2^(v mod 3) (equal_focals: all at full size)"""
    out = []
    for v in range(V):
        k = 0 if equal_focals else v % 3
        out.append(scenes.ring_camera(v, V, 1920 >> k, 1080 >> k, radius=RING_RADIUS))
    return out


def table(cams, dtype=torch.float64):
    """(M [V,4,4], fx, fy, W, H [V]) — the focal lengths are formed in double and rounded once, as the op's host side does"""
    M = torch.stack([c.world_view_transform.detach().cpu().float() for c in cams]).to(dtype)
    W = torch.tensor([float(c.image_width) for c in cams], dtype=torch.float64)
    H = torch.tensor([float(c.image_height) for c in cams], dtype=torch.float64)
    fx = torch.tensor([c.image_width / (2.0 * math.tan(0.5 * c.FoVx)) for c in cams], dtype=torch.float64)
    fy = torch.tensor([c.image_height / (2.0 * math.tan(0.5 * c.FoVy)) for c in cams], dtype=torch.float64)
    f32 = lambda t: t.float().to(dtype)                           # the table the op reads is float32
    return M, f32(fx), f32(fy), f32(W), f32(H)


def _nu(seen, rate, z, fx, rule):
    """nu [P] (0 where no camera sees the Gaussian) from seen [P,V], rate = fx / t.z [P,V], z [P,V]"""
    any_seen = seen.any(dim=1)
    if rule == "per_camera":
        nu = torch.where(seen, rate, torch.zeros_like(rate)).max(dim=1).values
    elif rule == "mip_splatting":
        zmin = torch.where(seen, z, torch.full_like(z, float("inf"))).min(dim=1).values
        nu = fx.max() / zmin
    else:
        raise ValueError(rule)
    return torch.where(any_seen, nu, torch.zeros_like(nu)), any_seen


def _finish(nu, any_seen, sd):
    """(filter_3D [P], fallback nu or None)"""
    if not bool(any_seen.any()):
        return torch.zeros_like(nu), None
    fb = nu[any_seen].min()
    return sd / torch.where(any_seen, nu, fb.expand_as(nu)), fb


def sweep(means3D, cams, rule="per_camera", variance=VARIANCE, dtype=torch.float64, slack=SLACK):
    """dict(nu, valid, filter, fallback; nu_hi / nu_lo, valid_hi / valid_lo, filter_hi / filter_lo, flagged) in `dtype`.
    dtype=torch.float32 is the float32 RESTATEMENT: the same formulas, operation for operation, in float32."""
    M, fx, fy, W, H = table(cams, dtype)
    p = means3D.detach().cpu().float().to(dtype)
    P = p.shape[0]
    x0, x1, x2 = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    t = [((M[:, 0, k] * x0 + M[:, 1, k] * x1) + M[:, 2, k] * x2) + M[:, 3, k] for k in range(3)]        # [P,V] each
    c = lambda v: torch.tensor(v, dtype=dtype)
    zc = torch.maximum(t[2], c(0.001))
    x = (t[0] / zc) * fx + W / c(2.0)
    y = (t[1] / zc) * fy + H / c(2.0)
    lo_x, hi_x, lo_y, hi_y = c(-0.15) * W, c(1.15) * W, c(-0.15) * H, c(1.15) * H
    near = c(0.2)

    def seen_with(e):
        """e = +1: decisions within the slack pass; -1: they fail; 0: as they fall (NaN / Inf: every comparison is false)"""
        ex, ey, ez = e * slack * W, e * slack * H, e * slack * near
        return (t[2] > near - ez) & (x >= lo_x - ex) & (x <= hi_x + ex) & (y >= lo_y - ey) & (y <= hi_y + ey)

    rate = fx / t[2]
    sd = torch.sqrt(c(variance))
    out = {}
    for tag, e in (("", 0.0), ("_hi", 1.0), ("_lo", -1.0)):
        nu, any_seen = _nu(seen_with(e), rate, t[2], fx, rule)
        filt, fb = _finish(nu, any_seen, sd)
        out["nu" + tag], out["valid" + tag], out["filter" + tag], out["fallback" + tag] = nu, any_seen, filt, fb
    out["flagged"] = (out["nu_hi"] != out["nu"]) | (out["nu_lo"] != out["nu"]) if P else torch.zeros(0, dtype=torch.bool)
    return out


def restatement_error(means3D, cams, rule, variance=VARIANCE):
    """max over the unflagged Gaussians of |filter32 - filter64| / filter64: the float32 restatement's own error (the relative
    error of nu, with the two roundings of sqrt(variance) / nu on top); 0 when nobody is seen.  Also: does the restatement take
    every validity decision of an unflagged Gaussian as float64 does?"""
    t64 = sweep(means3D, cams, rule, variance)
    t32 = sweep(means3D, cams, rule, variance, dtype=torch.float32)
    ok = ~t64["flagged"]
    same = bool((t32["valid"][ok] == t64["valid"][ok]).all())
    if t64["fallback"] is None or not bool(ok.any()):
        return 0.0, same
    e = ((t32["filter"].double() - t64["filter"]).abs() / t64["filter"])[ok]
    return float(e.max()), same


# ---- the filtered getters ----
def activate(scales, opacities, raw, dtype=torch.float64):
    s, o = scales.to(dtype), opacities.to(dtype)
    return (torch.exp(s), torch.sigmoid(o)) if raw else (s, o)


def getters(scales, opacities, filter_3D, raw=False):
    """(s_eff [P,3], o_eff [P,1]) in float64, differentiable in float64 leaves `scales` / `opacities` (the raw ones under raw):
    s_eff_k = sqrt(s_k^2 + f^2), o_eff = o prod_k s_k / s_eff_k; a row with f == 0 is the row itself"""
    s, o = activate(scales, opacities, raw)
    f = filter_3D.detach().to(torch.float64).reshape(-1, 1)
    off = (f == 0).expand_as(s)
    inner = torch.where(off, torch.ones_like(s), s * s + f * f)
    root = torch.sqrt(inner)
    s_eff = torch.where(off, s, root)
    r = torch.where(off, torch.ones_like(s), s / root)
    return s_eff, o.reshape(-1, 1) * r.prod(dim=1, keepdim=True)


def getters_determinant_form(s, o, f):
    """o sqrt(det S^2 / det(S^2 + f^2 I)) — the same o_eff, written as Mip-Splatting writes it (generic rows only)"""
    f = f.reshape(-1, 1)
    return o.reshape(-1, 1) * torch.sqrt((s * s).prod(dim=1, keepdim=True) / (s * s + f * f).prod(dim=1, keepdim=True))


def closed_form_gradients(s, o, f, g_s, g_o):
    """(dL/ds [P,3], dL/do [P,1]) of sum g_s s_eff + sum g_o o_eff from the closed forms of DESIGN.md 4.17 (f > 0, s > 0):
    d s_eff_k / d s_k = r_k,  d o_eff / d s_k = o_eff f^2 / (s_k s_eff_k^2),  d o_eff / d o = r_0 r_1 r_2"""
    f = f.reshape(-1, 1)
    s_eff = torch.sqrt(s * s + f * f)
    r = s / s_eff
    rp = r.prod(dim=1, keepdim=True)
    o_eff = o.reshape(-1, 1) * rp
    return r * g_s + (o_eff * f * f / (s * s_eff * s_eff)) * g_o.reshape(-1, 1), rp * g_o.reshape(-1, 1)


def getter_truth(scales, opacities, filter_3D, g_s, g_o, raw=False):
    """dict(s_eff, o_eff, scales, opacities): forward and the gradients of sum g_s s_eff + sum g_o o_eff by float64 autograd"""
    dt = torch.float64
    s = scales.detach().cpu().to(dt).clone().requires_grad_(True)
    o = opacities.detach().cpu().to(dt).clone().requires_grad_(True)
    s_eff, o_eff = getters(s, o, filter_3D.detach().cpu(), raw)
    ((s_eff * g_s.to(dt)).sum() + (o_eff * g_o.to(dt).reshape(-1, 1)).sum()).backward()
    return dict(s_eff=s_eff.detach(), o_eff=o_eff.detach(), scales=s.grad, opacities=o.grad)


def getter_rows(P, raw, seed=3):
    """(scales [P,3], opacities [P,1], filter_3D [P,1], g_s, g_o) float32 with the edge rows of SPEC M16 in front (as many as fit):
    f = 0;  s = 1e-6 under f = 1e-2;  s = 10 under f = 1e-4;  one s_k = 0 under f > 0;  all s_k = 0 under f > 0.
    raw: log-scales in [-20, 5], logits in [-12, 12] (the s_k = 0 rows do not exist in the raw parametrisation)"""
    g = torch.Generator().manual_seed(seed + 17 * P + int(raw))
    u = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)
    if raw:
        s = -20.0 + 25.0 * u(P, 3)
        o = -12.0 + 24.0 * u(P, 1)
    else:
        s = torch.exp(math.log(1e-3) + (math.log(2.0) - math.log(1e-3)) * u(P, 3))
        o = 0.01 + 0.98 * u(P, 1)
    f = torch.exp(math.log(1e-3) + (math.log(0.3) - math.log(1e-3)) * u(P, 1))
    act = (lambda v: math.log(v)) if raw else (lambda v: v)
    edges = [(None, 0.0), (act(1e-6), 1e-2), (act(10.0), 1e-4)]
    if not raw:
        edges += [("one", 0.05), (0.0, 0.05)]
    for i, (sv, fv) in enumerate(edges):
        row = (i + 1) % P if P > 1 else 0                         # P = 1: the last edge row that is written wins
        if P == 1 and i > 0:
            break
        if sv == "one":
            s[row, 1] = 0.0
        elif sv is not None:
            s[row] = sv
        f[row] = fv
    g_s = torch.randn(P, 3, generator=g)
    g_o = torch.randn(P, 1, generator=g)
    return s.float().contiguous(), o.float().contiguous(), f.float().contiguous(), g_s, g_o

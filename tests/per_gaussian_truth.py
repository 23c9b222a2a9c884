"""The per-Gaussian backward (K8 + K9, preprocess_backward_kernel) restated row by row, and the row families it is tested on.
Not collected by pytest: tests/test_per_gaussian_truth_cpu.py holds the restatement to the float64 oracle build and to autograd,
tests/test_per_gaussian_backward_gpu.py holds msgs_backward_per_gaussian to the restatement.

backward() is NOT autograd: it is the hand-derived map  nine 2-D sums -> gradients  as DESIGN.md SPEC words it (the conic ->
2-D covariance -> 3-D covariance -> scale / quaternion chain, the projection, the SH colour), every expression written in the
order preprocess.hip evaluates it, in the dtype asked for: float64 is the truth, float32 (numpy, one rounding per operation,
no contraction) is the yardstick a float32 implementation is measured with.  The map is linear in the sums, so
`columns` — the same tensors for each of the nine one-hot sums — is its Jacobian, and

    scale[i, t] = sum_j |sums[i, j]| * ||columns[j][t][i]||_inf

is what row i of tensor t can be expected to be right relative to: for a one-hot row the row's own infinity norm, for a dense
row the size of the terms that are added up (not of what is left after they cancel).

Units are those of include/msgs.h: sums[:, 0:2] = dL/dmean2D in the NDC-ish units of dL_dmeans2D (pixel gradient x 0.5 W,
0.5 H), sums[:, 2:5] = dL/dconic A, B, C, sums[:, 5] = dL/dopacity_eff (dL/dopacity = weight x sums[:, 5]),
sums[:, 6:9] = dL/drgb.

The two regularisers of the reference formula: 1 / (denom^2 + 1e-7) in the conic backward is NOT the derivative of the
forward's 1 / denom (regularised=False drops it: that is what autograd gives); 1 / (h_w + 1e-7) in the projection IS the exact
derivative of the forward's p_w = 1 / (h_w + 1e-7) (Q9) and is therefore the same in both.

Discrete decisions (the Q2 clamp masks, the denom2inv == 0 cut, the Q8 clamp flags, the filter weight, rendered or not) are
inputs of the backward: forward_decisions() takes them from the float32 forward, exactly as torch_oracle.preprocess does for
its `_decisions`."""
import math

import numpy as np
import torch

import scenes
from oracle import torch_oracle as to

F32 = np.float32
EPS32 = 2.0 ** -24
SUM_NAMES = ("mean2D x", "mean2D y", "conic A", "conic B", "conic C", "opacity", "rgb r", "rgb g", "rgb b")
MUTATIONS = ("dq2_sign", "x_mul_ignored", "gm_half_dropped", "modifier_once")


def _np(t, dt):
    if t is None:
        return None
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.astype(dt)


def _torch(t):
    return None if t is None else torch.as_tensor(t)


def tensor_names(inp):
    """the gradient tensors an entry with these inputs returns"""
    return (("means3D", "means2D", "opacities")
            + (("cov3D",) if inp.get("cov3D_precomp") is not None else ("scales", "rotations"))
            + (("colors",) if inp.get("colors_precomp") is not None else ("shs",)))


# ---------------------------------------------------------------------------------------------------------------------------
# decisions
# ---------------------------------------------------------------------------------------------------------------------------
def filter_weight(view, size, min_ps, max_ps, base_mask):
    """SPEC M2-M4 in size's own dtype, the operations of preprocess.hip:filter_weight in their order (float32 sizes of the
    kernel give the kernel's weight bit for bit: divisions, subtractions and min / max only)"""
    dt = size.dtype.type
    P = size.shape[0]
    w = np.ones(P, dtype=dt)
    fade = dt(view.get("fade_size", 1.0))
    base = np.zeros(P, dtype=bool) if base_mask is None else _np(base_mask, bool)
    with np.errstate(all="ignore"):
        if view.get("filter_small", False) and min_ps is not None:
            mn = _np(min_ps, F32).astype(dt)
            act = (~base) & (mn > 0) & (size < mn)
            ws = np.minimum(dt(1), np.maximum(dt(0), dt(1) - (mn / np.maximum(size, dt(F32(1e-30))) - dt(1)) / fade)) \
                if fade > 0 else np.zeros(P, dtype=dt)
            w = np.where(act, w * ws, w)
        if view.get("filter_large", False) and max_ps is not None:
            mx = _np(max_ps, F32).astype(dt)
            act = (mx > 0) & (size > mx)
            wl = np.minimum(dt(1), np.maximum(dt(0), dt(1) - (size / mx - dt(1)) / fade)) if fade > 0 else np.zeros(P, dtype=dt)
            w = np.where(act, w * wl, w)
    return w


def forward_f32(view, inp, dtype=torch.float32):
    """torch_oracle.preprocess on these inputs (float32: the forward the decisions are read from)"""
    with torch.no_grad():
        return to.preprocess(_torch(inp["means3D"]), _torch(inp["opacities"]), view, scales=_torch(inp.get("scales")),
                             rotations=_torch(inp.get("rotations")), cov3D_precomp=_torch(inp.get("cov3D_precomp")),
                             shs=_torch(inp.get("shs")), colors_precomp=_torch(inp.get("colors_precomp")),
                             max_pixel_sizes=_torch(inp.get("max_pixel_sizes")), min_pixel_sizes=_torch(inp.get("min_pixel_sizes")),
                             base_mask=_torch(inp.get("base_mask")), dtype=dtype)


def forward_decisions(view, inp, pixel_sizes=None):
    """The discrete inputs of the backward, from the float32 forward: clamped_x, clamped_y, cut (denom2inv == 0: denom^2 + 1e-7
    overflows float32), sh_clamped [P,3], rendered, and the filter weight — a function of the forward's pixel size
    (filter_weight above).  pixel_sizes: the sizes to form the weight from, in their own dtype (the kernel's float32
    pixel_sizes give the weight the kernel stored; float64 sizes the weight a float64 forward applies); default: the float32
    forward's."""
    pre = forward_f32(view, inp)
    a, b, c = pre["cov2"]
    denom = a * c - b * b
    cut = (1.0 / ((denom * denom) + 1e-7)) == 0
    rendered = pre["visible"].numpy().copy()
    size = pre["pixel_sizes"].numpy() if pixel_sizes is None else np.asarray(pixel_sizes)
    w = filter_weight(view, size, inp.get("min_pixel_sizes"), inp.get("max_pixel_sizes"), inp.get("base_mask"))
    return dict(clamped_x=pre["clamped_x"].numpy().copy(), clamped_y=pre["clamped_y"].numpy().copy(), cut=cut.numpy().copy(),
                sh_clamped=pre["clamped"].numpy().copy(), rendered=rendered, weight=w, pixel_sizes=size,
                radii=pre["radii"].numpy().copy(), forward=pre)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _sh_table(deg, x, y, z, dt):
    """preprocess.hip:sh_coef_table — (basis, d/dx, d/dy, d/dz) of the coefficients of the active degree, k ascending; float32
    carries the kernel's float constants, float64 the exact ones"""
    k = (lambda v: dt(F32(v))) if dt is F32 else dt
    C0, C1 = k(to.SH_C0), k(to.SH_C1)
    C2, C3 = [k(v) for v in to.SH_C2], [k(v) for v in to.SH_C3]
    z0 = np.zeros_like(x)
    full = lambda v: z0 + v
    rows = [(full(C0), z0, z0, z0)]
    if deg > 0:
        rows += [(-C1 * y, z0, full(-C1), z0), (C1 * z, z0, z0, full(C1)), (-C1 * x, full(-C1), z0, z0)]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        two, four = dt(2), dt(4)
        rows += [(C2[0] * xy, C2[0] * y, C2[0] * x, z0),
                 (C2[1] * yz, z0, C2[1] * z, C2[1] * y),
                 (C2[2] * (two * zz - xx - yy), C2[2] * -two * x, C2[2] * -two * y, C2[2] * four * z),
                 (C2[3] * xz, C2[3] * z, z0, C2[3] * x),
                 (C2[4] * (xx - yy), C2[4] * two * x, C2[4] * -two * y, z0)]
    if deg > 2:
        three, six, eight = dt(3), dt(6), dt(8)
        rows += [(C3[0] * y * (three * xx - yy), C3[0] * six * xy, C3[0] * (three * xx - three * yy), z0),
                 (C3[1] * xy * z, C3[1] * yz, C3[1] * xz, C3[1] * xy),
                 (C3[2] * y * (four * zz - xx - yy), C3[2] * -two * xy, C3[2] * (four * zz - xx - three * yy), C3[2] * eight * yz),
                 (C3[3] * z * (two * zz - three * xx - three * yy), C3[3] * -six * xz, C3[3] * -six * yz,
                  C3[3] * (six * zz - three * xx - three * yy)),
                 (C3[4] * x * (four * zz - xx - yy), C3[4] * (four * zz - three * xx - yy), C3[4] * -two * xy, C3[4] * eight * xz),
                 (C3[5] * z * (xx - yy), C3[5] * two * xz, C3[5] * -two * yz, C3[5] * (xx - yy)),
                 (C3[6] * x * (xx - three * yy), C3[6] * (three * xx - three * yy), C3[6] * -six * xy, z0)]
    return rows


def _prepare(view, inp, dt, dec, regularised, mutate):
    """everything of a row that does not depend on the sums"""
    f = lambda key: _np(inp.get(key), F32).astype(dt) if inp.get(key) is not None else None
    V = _np(view["viewmatrix"], F32).astype(dt).reshape(-1)
    M = _np(view["projmatrix"], F32).astype(dt).reshape(-1)
    cam = _np(view["campos"], F32).astype(dt).reshape(-1)
    Wd, Hd = dt(int(view["image_width"])), dt(int(view["image_height"]))
    tanx, tany = dt(F32(view["tanfovx"])), dt(F32(view["tanfovy"]))
    fx, fy = Wd / (dt(2) * tanx), Hd / (dt(2) * tany)
    mod = dt(F32(view.get("scale_modifier", 1.0)))
    one, two = dt(1), dt(2)
    p = f("means3D")
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    g = dict(dt=dt, P=p.shape[0], V=V, M=M, mod=mod, fx=fx, fy=fy, mutate=mutate)
    t = [((V[k] * x + V[4 + k] * y) + V[8 + k] * z) + V[12 + k] for k in range(3)]
    if inp.get("cov3D_precomp") is not None:
        cv = f("cov3D_precomp")
        cov = [cv[:, k] for k in range(6)]
        g["precomp_cov"] = True
    else:
        s, q = f("scales"), f("rotations")
        r, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = [[one - two * (qy * qy + qz * qz), two * (qx * qy - r * qz), two * (qx * qz + r * qy)],
             [two * (qx * qy + r * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - r * qx)],
             [two * (qx * qz - r * qy), two * (qy * qz + r * qx), one - two * (qx * qx + qy * qy)]]
        S = [mod * s[:, k] for k in range(3)]
        Mm = [[R[i][j] * S[j] for j in range(3)] for i in range(3)]
        dot = lambda a, b: Mm[a][0] * Mm[b][0] + Mm[a][1] * Mm[b][1] + Mm[a][2] * Mm[b][2]
        cov = [dot(0, 0), dot(0, 1), dot(0, 2), dot(1, 1), dot(1, 2), dot(2, 2)]
        g.update(precomp_cov=False, R=R, S=S, q=(r, qx, qy, qz))
    # ---- compute_cov2d ----
    lim13 = dt(F32(1.3)) if dt is F32 else dt(1.3)
    limx, limy = lim13 * tanx, lim13 * tany
    txtz, tytz = t[0] / t[2], t[1] / t[2]
    x_mul = np.where(dec["clamped_x"], dt(0), one)
    y_mul = np.where(dec["clamped_y"], dt(0), one)
    if mutate == "x_mul_ignored":
        x_mul = np.ones_like(x_mul)
    tx_c = np.minimum(limx, np.maximum(-limx, txtz)) * t[2]
    ty_c = np.minimum(limy, np.maximum(-limy, tytz)) * t[2]
    J00, J02 = fx / t[2], -(fx * tx_c) / (t[2] * t[2])
    J11, J12 = fy / t[2], -(fy * ty_c) / (t[2] * t[2])
    T = [[J00 * V[4 * c] + J02 * V[4 * c + 2] for c in range(3)], [J11 * V[4 * c + 1] + J12 * V[4 * c + 2] for c in range(3)]]
    Sg = [[cov[0], cov[1], cov[2]], [cov[1], cov[3], cov[4]], [cov[2], cov[4], cov[5]]]
    ST = [[Sg[i][0] * T[r_][0] + Sg[i][1] * T[r_][1] + Sg[i][2] * T[r_][2] for i in range(3)] for r_ in range(2)]
    c03 = dt(F32(0.3)) if dt is F32 else dt(0.3)
    ca = (T[0][0] * ST[0][0] + T[0][1] * ST[0][1] + T[0][2] * ST[0][2]) + c03
    cb = T[0][0] * ST[1][0] + T[0][1] * ST[1][1] + T[0][2] * ST[1][2]
    cc = (T[1][0] * ST[1][0] + T[1][1] * ST[1][1] + T[1][2] * ST[1][2]) + c03
    denom = ca * cc - cb * cb
    e7 = dt(F32(0.0000001)) if dt is F32 else dt(1e-7)
    d2i = one / ((denom * denom) + e7) if regularised else one / (denom * denom)
    d2i = np.where(dec["cut"], dt(0), d2i)
    g.update(t=t, T=T, ST=ST, ca=ca, cb=cb, cc=cc, denom=denom, d2i=d2i, x_mul=x_mul, y_mul=y_mul, tx_c=tx_c, ty_c=ty_c,
             txtz=txtz, tytz=tytz)
    # ---- projection ----
    h = [((M[k] * x + M[4 + k] * y) + M[8 + k] * z) + M[12 + k] for k in range(4)]
    m_w = one / (h[3] + e7)
    g.update(h=h, m_w=m_w, mul1=h[0] * m_w * m_w, mul2=h[1] * m_w * m_w)
    # ---- colour ----
    if inp.get("colors_precomp") is not None:
        g["precomp_colour"] = True
    else:
        sh = f("shs")
        deg = int(view["sh_degree"])
        dox, doy, doz = x - cam[0], y - cam[1], z - cam[2]
        ln = np.sqrt(dox * dox + doy * doy + doz * doz)
        d = (dox / ln, doy / ln, doz / ln)
        g.update(precomp_colour=False, sh=sh, K=sh.shape[1], d=d, dlen=ln, table=_sh_table(deg, d[0], d[1], d[2], dt),
                 keep=np.where(dec["sh_clamped"], dt(0), one))
    g.update(weight=dec["weight"].astype(dt), rendered=dec["rendered"].astype(bool))
    return g


def _apply(g, sums):
    """the linear map sums [P,9] -> gradients, in the kernel's order"""
    dt = g["dt"]
    P, V, M = g["P"], g["V"], g["M"]
    two, half = dt(2), dt(0.5)
    s = [sums[:, j].astype(dt) for j in range(9)]
    g2x, g2y, gA, gBh, gC = s[0], s[1], s[2], s[3], s[4]
    ca, cb, cc, denom, d2i = g["ca"], g["cb"], g["cc"], g["denom"], g["d2i"]
    live = d2i != 0
    z = lambda v: np.where(live, v, dt(0))
    dL_da = z(d2i * (-cc * cc * gA + two * cb * cc * gBh + (denom - ca * cc) * gC))
    dL_dc = z(d2i * (-ca * ca * gC + two * ca * cb * gBh + (denom - ca * cc) * gA))
    dL_db = z(d2i * two * (cb * cc * gA - (denom + two * cb * cb) * gBh + ca * cb * gC))
    T, ST = g["T"], g["ST"]
    dcov = [None] * 6
    dcov[0] = T[0][0] * T[0][0] * dL_da + T[0][0] * T[1][0] * dL_db + T[1][0] * T[1][0] * dL_dc
    dcov[3] = T[0][1] * T[0][1] * dL_da + T[0][1] * T[1][1] * dL_db + T[1][1] * T[1][1] * dL_dc
    dcov[5] = T[0][2] * T[0][2] * dL_da + T[0][2] * T[1][2] * dL_db + T[1][2] * T[1][2] * dL_dc
    dcov[1] = two * T[0][0] * T[0][1] * dL_da + (T[0][0] * T[1][1] + T[0][1] * T[1][0]) * dL_db + two * T[1][0] * T[1][1] * dL_dc
    dcov[2] = two * T[0][0] * T[0][2] * dL_da + (T[0][0] * T[1][2] + T[0][2] * T[1][0]) * dL_db + two * T[1][0] * T[1][2] * dL_dc
    dcov[4] = two * T[0][2] * T[0][1] * dL_da + (T[0][1] * T[1][2] + T[0][2] * T[1][1]) * dL_db + two * T[1][1] * T[1][2] * dL_dc
    dcov = [z(v) for v in dcov]
    dT0 = [two * ST[0][k] * dL_da + ST[1][k] * dL_db for k in range(3)]
    dT1 = [two * ST[1][k] * dL_dc + ST[0][k] * dL_db for k in range(3)]
    dJ00 = V[0] * dT0[0] + V[4] * dT0[1] + V[8] * dT0[2]
    dJ02 = V[2] * dT0[0] + V[6] * dT0[1] + V[10] * dT0[2]
    dJ11 = V[1] * dT1[0] + V[5] * dT1[1] + V[9] * dT1[2]
    dJ12 = V[2] * dT1[0] + V[6] * dT1[1] + V[10] * dT1[2]
    fx, fy = g["fx"], g["fy"]
    tz = dt(1) / g["t"][2]
    tz2 = tz * tz
    tz3 = tz2 * tz
    dtx = g["x_mul"] * -fx * tz2 * dJ02
    dty = g["y_mul"] * -fy * tz2 * dJ12
    dtz = -fx * tz2 * dJ00 - fy * tz2 * dJ11 + (two * fx * g["tx_c"]) * tz3 * dJ02 + (two * fy * g["ty_c"]) * tz3 * dJ12
    dmean = [V[4 * j + 0] * dtx + V[4 * j + 1] * dty + V[4 * j + 2] * dtz for j in range(3)]
    m_w, mul1, mul2 = g["m_w"], g["mul1"], g["mul2"]
    dmean = [dmean[j] + ((M[4 * j + 0] * m_w - M[4 * j + 3] * mul1) * g2x + (M[4 * j + 1] * m_w - M[4 * j + 3] * mul2) * g2y)
             for j in range(3)]
    out = {}
    # ---- colour ----
    if g["precomp_colour"]:
        out["colors"] = np.stack([s[6], s[7], s[8]], axis=1)
    else:
        dcol = [s[6 + c] * g["keep"][:, c] for c in range(3)]
        sh, K, d = g["sh"], g["K"], g["d"]
        dsh = np.zeros((P, K, 3), dtype=dt)
        ddir = [np.zeros(P, dtype=dt) for _ in range(3)]
        for k, (basis, bx, by, bz) in enumerate(g["table"]):
            acc = np.zeros(P, dtype=dt)
            for c in range(3):
                dsh[:, k, c] = basis * dcol[c]
                acc = acc + sh[:, k, c] * dcol[c]
            ddir = [ddir[0] + bx * acc, ddir[1] + by * acc, ddir[2] + bz * acc]
        dotv = d[0] * ddir[0] + d[1] * ddir[1] + d[2] * ddir[2]
        dmean = [dmean[j] + (ddir[j] - d[j] * dotv) / g["dlen"] for j in range(3)]
        out["shs"] = dsh
    out["means3D"] = np.stack(dmean, axis=1)
    out["means2D"] = np.stack([g2x, g2y, np.zeros(P, dtype=dt)], axis=1)
    out["opacities"] = g["weight"] * s[5]
    # ---- 3-D covariance ----
    if g["precomp_cov"]:
        out["cov3D"] = np.stack(dcov, axis=1)
    else:
        R, S, (r, x, y, zq), mod = g["R"], g["S"], g["q"], g["mod"]
        hf = dt(1) if g["mutate"] == "gm_half_dropped" else half
        Gm = [[dcov[0], hf * dcov[1], hf * dcov[2]], [hf * dcov[1], dcov[3], hf * dcov[4]], [hf * dcov[2], hf * dcov[4], dcov[5]]]
        dM = [[None] * 3 for _ in range(3)]
        for a in range(3):
            for b in range(3):
                acc = np.zeros(P, dtype=dt)
                for k in range(3):
                    acc = acc + Gm[a][k] * (R[k][b] * S[b])
                dM[a][b] = two * acc
        dscale, dR = [], [[None] * 3 for _ in range(3)]
        for j in range(3):
            ds = dM[0][j] * R[0][j] + dM[1][j] * R[1][j] + dM[2][j] * R[2][j]
            dscale.append(ds if g["mutate"] == "modifier_once" else mod * ds)
            for a in range(3):
                dR[a][j] = dM[a][j] * S[j]
        sg = dt(-1) if g["mutate"] == "dq2_sign" else dt(1)
        dq = [two * (-zq * dR[0][1] + y * dR[0][2] + zq * dR[1][0] - x * dR[1][2] - y * dR[2][0] + x * dR[2][1]),
              two * (y * dR[0][1] + zq * dR[0][2] + y * dR[1][0] - two * x * dR[1][1] - r * dR[1][2] + zq * dR[2][0]
                     + r * dR[2][1] - two * x * dR[2][2]),
              two * (-two * y * dR[0][0] + x * dR[0][1] + sg * r * dR[0][2] + x * dR[1][0] + zq * dR[1][2] - r * dR[2][0]
                     + zq * dR[2][1] - two * y * dR[2][2]),
              two * (-two * zq * dR[0][0] - r * dR[0][1] + x * dR[0][2] + r * dR[1][0] - two * zq * dR[1][1] + y * dR[1][2]
                     + x * dR[2][0] + y * dR[2][1])]
        out["scales"] = np.stack(dscale, axis=1)
        out["rotations"] = np.stack(dq, axis=1)
    rend = g["rendered"]
    for k, v in out.items():
        out[k] = np.where(rend.reshape((P,) + (1,) * (v.ndim - 1)), v, dt(0))
    return out


def backward(view, inputs, sums, *, dtype=np.float64, regularised=True, decisions=None, mutate=None):
    """K8 + K9 on the nine per-Gaussian sums [P,9] (float64 array or tensor).  Returns a dict of numpy arrays in `dtype`:
    means3D [P,3], means2D [P,3] (third column 0), opacities [P], scales [P,3] and rotations [P,4] — or cov3D [P,6] with
    cov3D_precomp —, shs [P,K,3] — or colors [P,3] with colors_precomp —, and
      columns   the same tensors for each of the nine one-hot sums (the Jacobian), a list of nine dicts
      rendered  [P] bool; rows that were not rendered are zero in every tensor whatever their sums hold
    `inputs`: dict of float32 tensors (means3D, opacities, scales + rotations | cov3D_precomp, shs | colors_precomp,
    min_pixel_sizes, max_pixel_sizes, base_mask); `view`: torch_oracle.view_dict().  dtype=np.float32 evaluates the same
    expressions in the kernel's order, every operation rounded to float32.  mutate: one of MUTATIONS — a deliberately wrong
    restatement, for showing what a criterion can see (tests/test_per_gaussian_truth_cpu.py); never set otherwise."""
    dt = np.dtype(dtype).type
    assert mutate is None or mutate in MUTATIONS
    dec = forward_decisions(view, inputs) if decisions is None else decisions
    sums = _np(sums, np.float64).reshape(-1, 9)
    rend = dec["rendered"].astype(bool)
    sums = np.where(rend[:, None], sums, 0.0)              # whatever a row that was not rendered carries is never read
    with np.errstate(all="ignore"):
        g = _prepare(view, inputs, dt, dec, regularised, mutate)
        out = _apply(g, sums)
        cols = []
        for j in range(9):
            e = np.zeros_like(sums)
            e[:, j] = 1.0
            cols.append(_apply(g, e))
    out["columns"] = cols
    out["rendered"] = rend
    out["sums"] = sums
    out["geometry"] = g
    return out


def error_scale(res):
    """{tensor: [P]}: scale[i, t] = sum_j |sums[i, j]| ||columns[j][t][i]||_inf of a backward() result"""
    s = np.abs(res["sums"])
    P = s.shape[0]
    out = {}
    for k in res["columns"][0]:
        norms = np.stack([np.abs(col[k].astype(np.float64)).reshape(P, -1).max(axis=1) for col in res["columns"]], axis=1)
        out[k] = (s * norms).sum(axis=1)
    return out


def row_error(got, truth, key):
    """[P]: ||got_i - truth_i||_inf of tensor `key` (got: array or tensor of any float dtype)"""
    a = _np(got, np.float64).reshape(truth[key].shape)
    return np.abs(a - truth[key].astype(np.float64)).reshape(a.shape[0], -1).max(axis=1)


def worst_ratio(got, truth, scale, key, rows=None):
    """max over rows with scale > 0 of row_error / (2^-24 scale); 0.0 where there is none"""
    e, s = row_error(got, truth, key), scale[key]
    ok = s > 0 if rows is None else (s > 0) & rows
    return float((e[ok] / (EPS32 * s[ok])).max()) if ok.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# families: 160 x 96, a general rigid pose (every entry of the rotation non-zero, fx = 100 != fy = 96 / 0.9)
# ---------------------------------------------------------------------------------------------------------------------------
W, H = 160, 96
TANX, TANY = 0.8, 0.45
ROW_COUNTS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300)
P_MAX = 300
PATTERNS = ("onehot", "dense", "decades")
OFF = dict(filter_small=False, filter_large=False, fade_size=1.0)
MARGIN = 0.01                                   # every row sits this far (relative) from each forward tie


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


POSE_R = _rot(0.4, -0.7, 0.3)                   # camera-to-world rotation
POSE_T = np.array([0.3, -0.2, 0.5])             # world-to-camera translation


def general_camera():
    return scenes.make_camera(POSE_R, POSE_T, 2.0 * math.atan(TANX), 2.0 * math.atan(TANY), W, H)


def front_camera():
    return scenes.make_camera(np.eye(3), np.zeros(3), 2.0 * math.atan(TANX), 2.0 * math.atan(TANY), W, H)


def _world(tv, front=False):
    """view-space points [n,3] -> world (t = R^T p + T)"""
    return tv if front else (tv - POSE_T[None]) @ POSE_R.T


def _view_points(rng, n, zlo=2.0, zhi=6.0, ndc=0.8):
    z = rng.uniform(zlo, zhi, n)
    return np.stack([rng.uniform(-ndc, ndc, n) * TANX * z, rng.uniform(-ndc, ndc, n) * TANY * z, z], axis=1)


def _unit_quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _scales_px(rng, tv, lo, hi, aspect=4.0):
    """scales whose footprint is lo .. hi pixels (geometric mean) with per-axis spread up to `aspect`"""
    base = rng.uniform(lo, hi, len(tv)) * tv[:, 2] / 100.0
    u = np.exp(rng.uniform(-0.5 * math.log(aspect), 0.5 * math.log(aspect), (len(tv), 3)))
    return base[:, None] * u


def _shs(rng, n, K=16, deg=2, clamp=None):
    """dc planted so that every channel is far from the Q8 clamp: +1.5 -> colour 0.92 (clamp[i] lists the channels of row i
    planted at -5 -> -0.91); the rest coefficients (sigma 0.1) cannot move either across 0"""
    sh = np.zeros((n, K, 3))
    sh[:, 0, :] = 1.5 + 0.2 * rng.uniform(-1, 1, (n, 3))
    ncoef = (deg + 1) ** 2
    if ncoef > 1:
        sh[:, 1:ncoef, :] = 0.1 * rng.normal(size=(n, ncoef - 1, 3)).clip(-2.5, 2.5)
    if K > ncoef:
        sh[:, ncoef:, :] = 0.1 * rng.normal(size=(n, K - ncoef, 3))       # beyond the active degree: must not matter
    for i, chans in (clamp or {}).items():
        for c in chans:
            sh[i, 0, c] = -5.0
    return sh


def _family(name, means, scales, quats, *, opac=None, shs=None, deg=2, settings=None, mod=1.0, front=False, cov=None,
            colors=None, min_ps=None, max_ps=None, base=None, expect=None, needle=False):
    n = len(means)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=F32)))
    rng = np.random.default_rng(sum(map(ord, name)))
    inp = dict(means3D=t32(means), opacities=t32(np.full(n, 0.7) if opac is None else opac),
               min_pixel_sizes=t32(-np.ones(n) if min_ps is None else min_ps),
               max_pixel_sizes=t32(-np.ones(n) if max_ps is None else max_ps),
               base_mask=torch.from_numpy(np.zeros(n, dtype=bool) if base is None else np.asarray(base, dtype=bool)))
    if cov is not None:
        inp["cov3D_precomp"] = t32(cov)
    else:
        inp["scales"], inp["rotations"] = t32(scales), t32(quats)
    if colors is not None:
        inp["colors_precomp"] = t32(colors)
    else:
        inp["shs"] = t32(_shs(rng, n, deg=deg) if shs is None else shs)
    cam = front_camera() if front else general_camera()
    st = dict(OFF if settings is None else settings)
    view = to.view_dict(cam, sh_degree=deg, scale_modifier=float(F32(mod)), **st)
    return dict(name=name, inputs=inp, cam=cam, settings=st, view=view, mod=float(F32(mod)), n=n, expect=expect or {},
                needle=needle)


def _round(name, seed, front=False, mod=1.0):
    rng = np.random.default_rng(seed)
    n = 32
    tv = _view_points(rng, n)
    return _family(name, _world(tv, front), _scales_px(rng, tv, 2.0, 6.0), _unit_quats(rng, n), front=front, mod=mod,
                   opac=rng.uniform(0.2, 0.95, n), expect=dict(rendered=np.ones(n, dtype=bool), max_aspect=4.0))


def _clamp():
    """rows 2k: centre outside 1.3 tan(fov) (x only, y only, both, each sign), rows 2k + 1: the twin just inside the limit"""
    rng = np.random.default_rng(11)
    sides = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, 1), (-1, -1)]
    tv, want = [], []
    for k in range(16):
        sx, sy = sides[k % 8]
        z = rng.uniform(2.5, 5.0)
        out = rng.uniform(1.36, 1.5)
        free = rng.uniform(-0.6, 0.6)
        for f_ in (out, 1.3 * 0.97):
            tv.append(((sx * f_ if sx else free) * TANX * z, (sy * f_ if sy else free) * TANY * z, z))
            want.append((bool(sx) and f_ == out, bool(sy) and f_ == out))
    tv = np.array(tv)
    n = len(tv)
    want = np.array(want)
    twin = lambda a: np.repeat(a[0::2], 2, axis=0)          # a row and its twin differ in the clamped coordinate alone
    # 25 .. 40 px: the footprint reaches the image from 40 pixels outside
    return _family("clamp", _world(tv), twin(_scales_px(rng, tv, 25.0, 40.0, aspect=2.0)), twin(_unit_quats(rng, n)),
                   opac=twin(rng.uniform(0.3, 0.9, n)),
                   expect=dict(rendered=np.ones(n, dtype=bool), clamped_x=want[:, 0], clamped_y=want[:, 1]))


def _lowpass():
    rng = np.random.default_rng(12)
    n = 32
    tv = _view_points(rng, n)
    return _family("lowpass", _world(tv), _scales_px(rng, tv, 0.01, 0.05), _unit_quats(rng, n), opac=rng.uniform(0.3, 0.9, n),
                   expect=dict(rendered=np.ones(n, dtype=bool), lowpass=True))


def _needle():
    rng = np.random.default_rng(13)
    n = 32
    tv = _view_points(rng, n, ndc=0.6)
    thin = rng.uniform(0.3, 1.0, n) * tv[:, 2] / 100.0
    aspect = np.exp(rng.uniform(math.log(50.0), math.log(1000.0), n))
    s = np.stack([thin, thin * rng.uniform(1.0, 2.0, n), thin * aspect], axis=1)
    s = np.take_along_axis(s, np.argsort(rng.uniform(size=(n, 3)), axis=1), axis=1)
    return _family("needle", _world(tv), s, _unit_quats(rng, n), opac=rng.uniform(0.3, 0.9, n), needle=True,
                   expect=dict(rendered=np.ones(n, dtype=bool), min_aspect=50.0))


def _quaternion():
    rng = np.random.default_rng(14)
    r2 = math.sqrt(0.5)
    q = [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (-1, 0, 0, 0), (0, 0, 0, -1)]
    q += [(r2, r2, 0, 0), (-r2, r2, 0, 0), (r2, 0, -r2, 0), (0, r2, 0, r2), (0, 0, -r2, -r2), (-r2, 0, 0, r2), (0, -r2, r2, 0),
          (0.5, 0.5, 0.5, 0.5), (-0.5, 0.5, -0.5, 0.5), (-0.5, -0.5, -0.5, -0.5)]
    gen = _unit_quats(rng, 8)
    gen[:4, 0] = -np.abs(gen[:4, 0])                                  # negative r
    non = _unit_quats(rng, 8) * rng.uniform(0.5, 1.6, 8)[:, None]     # not unit: the formula is the un-normalised one
    non[:3, 0] = -np.abs(non[:3, 0])
    q = np.concatenate([np.array(q, dtype=np.float64), gen, non])
    n = len(q)
    tv = _view_points(rng, n)
    kind = np.array(["basis"] * 6 + ["pair"] * 10 + ["unit"] * 8 + ["nonunit"] * 8)
    return _family("quaternion", _world(tv), _scales_px(rng, tv, 2.0, 5.0), q, opac=rng.uniform(0.3, 0.9, n),
                   expect=dict(rendered=np.ones(n, dtype=bool), kind=kind))


GIANT_OVERFLOW = math.sqrt(3.4028234663852886e38)     # denom beyond this: denom^2 + 1e-7 overflows float32


def _giant():
    """even rows: denom = 10 .. 1000 x the overflow point (cut); odd rows: the neighbours at denom ~ 1e17 .. 1e18"""
    rng = np.random.default_rng(15)
    n = 32
    tv = _view_points(rng, n, ndc=0.5)
    cut = np.arange(n) % 2 == 0
    target = np.where(cut, GIANT_OVERFLOW * np.exp(rng.uniform(math.log(12.0), math.log(1000.0), n)),
                      np.exp(rng.uniform(math.log(1e17), math.log(1e18), n)))
    sigma_px = target ** 0.25                                # denom ~ sigma^4 for a round footprint
    s = (sigma_px * tv[:, 2] / 100.0)[:, None] * np.exp(rng.uniform(-0.1, 0.1, (n, 3)))
    return _family("giant", _world(tv), s, _unit_quats(rng, n), opac=rng.uniform(0.3, 0.9, n),
                   expect=dict(rendered=np.ones(n, dtype=bool), cut=cut))


FILTER_ROLES = ("one", "small", "large", "both", "base", "zero_small", "zero_large", "off")


def _filter(fade):
    """thresholds set from the float32 forward's own pixel sizes: min = 1.25 size -> w = 1 - 0.25 / fade, max = size / 1.2 ->
    w = 1 - 0.2 / fade, both -> the product; a base_mask row with min = 1.25 size keeps w = 1; min = 2.3 size or
    max = size / 2.3 -> w = 0, not rendered; "one": thresholds that do not bind (min = size / 2, max = 2 size); "off": -1"""
    rng = np.random.default_rng(16)
    n = 32
    tv = _view_points(rng, n)
    means, s, q, o = _world(tv), _scales_px(rng, tv, 2.0, 6.0), _unit_quats(rng, n), rng.uniform(0.3, 0.9, n)
    probe = _family("filter_probe", means, s, q, opac=o)
    size = forward_f32(probe["view"], probe["inputs"])["pixel_sizes"].numpy().astype(np.float64)
    role = np.array([FILTER_ROLES[i % len(FILTER_ROLES)] for i in range(n)])
    mn, mx, base = -np.ones(n), -np.ones(n), np.zeros(n, dtype=bool)
    w = np.ones(n)
    for i in range(n):
        if role[i] == "one":
            mn[i], mx[i] = size[i] / 2.0, size[i] * 2.0
        if role[i] in ("small", "both", "base"):
            mn[i] = 1.25 * size[i]
        if role[i] in ("large", "both"):
            mx[i] = size[i] / 1.2
        if role[i] == "base":
            base[i] = True
        if role[i] == "zero_small":
            mn[i] = 2.3 * size[i]
        if role[i] == "zero_large":
            mx[i] = size[i] / 2.3
        w[i] = dict(one=1.0, off=1.0, base=1.0, small=1 - 0.25 / fade, large=1 - 0.2 / fade,
                    both=(1 - 0.25 / fade) * (1 - 0.2 / fade), zero_small=0.0, zero_large=0.0)[role[i]]
    return _family(f"filter_fade{fade:g}", means, s, q, opac=o, min_ps=mn, max_ps=mx, base=base,
                   settings=dict(filter_small=True, filter_large=True, fade_size=fade),
                   expect=dict(rendered=w > 0, weight=w, role=role))


def _dead():
    """live rows interleaved with rows behind the camera, off screen and filtered out, inside one wave: two of every three
    rows of the first 32-row run are dead, then one whole dead run of 32, then alternating"""
    rng = np.random.default_rng(17)
    n = 96
    tv = _view_points(rng, n)
    s, o = _scales_px(rng, tv, 2.0, 6.0), rng.uniform(0.3, 0.9, n)
    kind = np.array(["live"] * n, dtype=object)
    dead_no = 0
    for i in range(n):
        if (i % 3 != 0) if i < 32 else (i < 64 or i % 2 == 1):
            kind[i] = ("behind", "offscreen", "filtered")[dead_no % 3]
            dead_no += 1
    for i in range(n):
        if kind[i] == "behind":
            tv[i, 2] = -rng.uniform(0.5, 3.0) if i % 2 else rng.uniform(0.05, 0.15)
        elif kind[i] == "offscreen":
            z = tv[i, 2]
            tv[i, 0] = (2.2 if i % 2 else -2.2) * TANX * z                 # 96 pixels beyond the edge, radius < 20
    means, q = _world(tv), _unit_quats(rng, n)
    probe = _family("dead_probe", means, s, q, opac=o)
    size = forward_f32(probe["view"], probe["inputs"])["pixel_sizes"].numpy().astype(np.float64)
    mn = np.where(kind == "filtered", 2.5 * size, -1.0)
    return _family("dead", means, s, q, opac=o, min_ps=mn, settings=dict(filter_small=True, filter_large=True, fade_size=1.0),
                   expect=dict(rendered=kind == "live", kind=kind))


def _precomputed(cov=True, colour=True):
    """cov: general symmetric positive definite matrices through cov3D_precomp (dL_dcov3D, no scale / quaternion tail);
    colour: colors_precomp (dL_dcolors, no clamp mask); either alone keeps the other half on its usual path"""
    rng = np.random.default_rng(18)
    n = 32
    tv = _view_points(rng, n)
    sig = rng.uniform(2.0, 6.0, n) * tv[:, 2] / 100.0
    A = rng.normal(size=(n, 3, 3)) * sig[:, None, None] * 0.6
    S = A @ A.transpose(0, 2, 1)
    packed = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], axis=1)
    name = "precomputed" + ("" if cov and colour else "_cov" if cov else "_colour")
    return _family(name, _world(tv), _scales_px(rng, tv, 2.0, 6.0), _unit_quats(rng, n), cov=packed if cov else None,
                   colors=rng.uniform(0.0, 1.0, (n, 3)) if colour else None, opac=rng.uniform(0.3, 0.9, n),
                   expect=dict(rendered=np.ones(n, dtype=bool)))


SH_CLAMPS = ((), (0,), (1,), (2,), (0, 1, 2), (0, 2))


def _sh(deg, full):
    """full: K = 16 storage (the Jacobian path with staged rows); else K = (deg + 1)^2 (the per-thread path).  Row i clamps the
    channels SH_CLAMPS[i % 6]"""
    rng = np.random.default_rng(20 + deg + (10 if full else 0))
    n = 30
    K = 16 if full else (deg + 1) ** 2
    tv = _view_points(rng, n)
    clamp = {i: SH_CLAMPS[i % len(SH_CLAMPS)] for i in range(n)}
    want = np.zeros((n, 3), dtype=bool)
    for i, ch in clamp.items():
        want[i, list(ch)] = True
    return _family(f"sh{deg}_K{K}" + ("" if not full or deg == 3 else "_padded"), _world(tv), _scales_px(rng, tv, 2.0, 6.0),
                   _unit_quats(rng, n), opac=rng.uniform(0.3, 0.9, n), shs=_shs(rng, n, K=K, deg=deg, clamp=clamp), deg=deg,
                   expect=dict(rendered=np.ones(n, dtype=bool), sh_clamped=want))


FAMILIES = {
    "round": lambda: _round("round", 10),
    "round_front": lambda: _round("round_front", 10, front=True),
    "clamp": _clamp,
    "lowpass": _lowpass,
    "needle": _needle,
    "modifier_0.7": lambda: _round("modifier_0.7", 19, mod=0.7),
    "modifier_1.6": lambda: _round("modifier_1.6", 19, mod=1.6),
    "quaternion": _quaternion,
    "giant": _giant,
    "filter_fade0.5": lambda: _filter(0.5),
    "filter_fade1": lambda: _filter(1.0),
    "dead": _dead,
    "precomputed": _precomputed,
    "precomputed_cov": lambda: _precomputed(colour=False),
    "precomputed_colour": lambda: _precomputed(cov=False),
    "sh0_K16_padded": lambda: _sh(0, True), "sh1_K16_padded": lambda: _sh(1, True), "sh2_K16_padded": lambda: _sh(2, True),
    "sh3_K16": lambda: _sh(3, True),
    "sh0_K1": lambda: _sh(0, False), "sh1_K4": lambda: _sh(1, False), "sh2_K9": lambda: _sh(2, False),
}       # (K = (3 + 1)^2 IS 16: degree 3 has one layout, and it takes the staged path)

_CACHE = {}


def family(name):
    if name not in _CACHE:
        fam = FAMILIES[name]()
        assert fam["name"] == name, (fam["name"], name)
        _CACHE[name] = fam
    return _CACHE[name]


def _sums(fam, pattern):
    """[P_MAX, 9] float64 (float32-representable, so that the truth and the kernel read the same numbers) and the geometry
    index of every row.  onehot: geometry g = i % n carries sum j = (i // n) % 9, value +-1 .. 2; dense: N(0, 1) in all nine;
    decades: random signs, magnitudes log-uniform over six decades.  Rows the family expects dead carry NaN / Inf."""
    n = fam["n"]
    rng = np.random.default_rng(1000 + sum(map(ord, fam["name"])) + PATTERNS.index(pattern))
    i = np.arange(P_MAX)
    geo = i % n
    if pattern == "onehot":
        s = np.zeros((P_MAX, 9))
        s[i, (i // n) % 9] = rng.choice([-1.0, 1.0], P_MAX) * rng.uniform(1.0, 2.0, P_MAX)
    elif pattern == "dense":
        s = rng.normal(size=(P_MAX, 9))
    else:
        s = rng.choice([-1.0, 1.0], (P_MAX, 9)) * 10.0 ** rng.uniform(-3.0, 3.0, (P_MAX, 9))
    s = s.astype(F32).astype(np.float64)
    dead = ~np.asarray(fam["expect"]["rendered"])[geo]
    junk = np.array([np.nan, np.inf, -np.inf])
    s[dead] = junk[(np.arange(P_MAX)[:, None] + np.arange(9)[None, :]) % 3][dead]
    return s, geo


def case(name, pattern, P):
    """(view, inputs [P rows], sums [P,9] float64, geometry index [P]) of family `name`: its rows tiled to P_MAX, then truncated"""
    fam = family(name)
    s, geo = _sums(fam, pattern)
    idx = torch.from_numpy(geo[:P])
    inp = {k: (v[idx].contiguous() if v is not None else None) for k, v in fam["inputs"].items()}
    return fam["view"], inp, s[:P].copy(), geo[:P]


def yardstick(name):
    """{tensor: worst |float32 restatement - float64| / (2^-24 scale)} of family `name` over its three sum patterns at P_MAX rows
    (every smaller row count is a prefix of these rows)"""
    worst = {}
    for pattern in PATTERNS:
        view, inp, sums, _ = case(name, pattern, P_MAX)
        dec = forward_decisions(view, inp)
        t64 = backward(view, inp, sums, decisions=dec)
        t32 = backward(view, inp, sums, decisions=dec, dtype=np.float32)
        scale = error_scale(t64)
        for k in tensor_names(inp):
            worst[k] = max(worst.get(k, 0.0), worst_ratio(t32[k], t64, scale, k))
    return worst

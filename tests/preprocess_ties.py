"""Exact ties of the per-Gaussian decisions of K1 (preprocess_kernel): case builders and the
expected decisions.  Not collected by pytest; tests/test_preprocess_ties_cpu.py proves every case is what it claims to be and
holds both oracles to it, tests/test_preprocess_ties_gpu.py holds the kernels to the same expectations.

Every decision of K1 is one comparator.  A tie row T makes its two operands bit-equal in float32; its neighbours T- and T+
are the same row with the compared operand one float32 ulp to either side.  The camera makes the arithmetic exact:
viewmatrix = I (t = p bit for bit), tanfov = 0.5 (fx = W, limit = 1.3f * 0.5f = 0.65f), projmatrix with PM[0] = PM[5] = 2,
PM[11] = 1 (h.x = 2x, h.w = z; at z = 2 the reference's p_w = 1 / (2 + 1e-7f) is 0.5f, so ndc = (x, y) and the pixel centre is
exact for dyadic x).  preprocess.hip is compiled with contraction off, so a tie of exactly representable operands is a tie in
the kernel as well.

The tie rows sit inside an ordinary small scene, at scattered rows of one wave and across the 64- and 256-row seams
(SLOTS), so that culled and alive lanes share ballots, the staged-SH row compaction and the workgroup counters.

Roles: "T" the tie, "T-" / "T+" the operand one ulp below / above (for a right / bottom / negative edge: in the direction of
the comparison, see each family).  Expectation fields of a row (None: not pinned):
  alive      radii > 0
  radius     the exact radius ("restated": the float32 restatement k1_f32 decides)
  psize      "zero" / "pos": pixel_sizes == 0 / > 0
  no_pixels  contributions().pixel_count == 0 although radii > 0
  lhs, rhs, rel   the compared operands (a key of k1_f32's result, a float32 constant) and their relation at this row"""
import copy
import math
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Optional

import numpy as np
import torch

import scenes
from parity_utils import small_scene

F = np.float32
P = 300
ZNEAR, ZFAR = 0.01, 100.0
OFF = dict(filter_small=False, filter_large=False, fade_size=1.0)
# triples first over the wave seam and the block seam, then scattered inside waves
SLOTS = (62, 63, 64, 254, 255, 256, 3, 17, 18, 126, 127, 128, 190, 191, 192, 40, 65, 99, 257, 258, 277, 129, 130, 189,
         193, 221, 253, 61, 66, 299)
NEAR = F(0.2)
LIMIT = F(1.3) * F(0.5)                  # the Q2 limit as K1 forms it: 1.3f * tanfov
O_GATE = F(1.0) / F(255.0)               # 255f * o == 1.0f


def up(x):
    return np.nextafter(x, np.asarray(np.inf, dtype=np.asarray(x).dtype))


def down(x):
    return np.nextafter(x, np.asarray(-np.inf, dtype=np.asarray(x).dtype))


def toward0(x):
    return np.nextafter(x, np.asarray(0, dtype=np.asarray(x).dtype))


def tie_camera(W=64, H=64):
    """viewmatrix = I, tanfovx = tanfovy = 0.5, campos = 0, the projection written out in the kernels' flat row-vector
    convention h_k = sum_j ph_j PM[4j + k]"""
    PM = torch.zeros(4, 4)
    PM[0, 0] = 2.0                                      # PM[0]
    PM[1, 1] = 2.0                                      # PM[5]
    PM[2, 3] = 1.0                                      # PM[11]
    PM[2, 2] = ZFAR / (ZFAR - ZNEAR)                    # PM[10]
    PM[3, 2] = -(ZFAR * ZNEAR) / (ZFAR - ZNEAR)         # PM[14]
    fov = 2.0 * math.atan(0.5)
    return scenes.Camera(int(W), int(H), fov, fov, torch.eye(4), PM, torch.zeros(3), ZNEAR, ZFAR)


@dataclass
class Case:
    family: str
    scene: scenes.Scene
    cam: scenes.Camera
    rows: list = field(default_factory=list)
    cov3D: Optional[torch.Tensor] = None                # [P,6] float32: the case enters through cov3D_precomp

    def idx(self, **want):
        return [r["row"] for r in self.rows if all(r.get(k) == v for k, v in want.items())]

    def named(self, name):
        (r,) = [r for r in self.rows if r["name"] == name]
        return r


def _base(seed, W=64, H=64):
    sc, _ = small_scene(P, W, H, seed)
    sc = copy.copy(sc)
    for k in ("means3D", "scales", "rotations", "opacities", "max_pixel_sizes", "min_pixel_sizes", "base_mask"):
        setattr(sc, k, getattr(sc, k).clone())
    return sc, tie_camera(W, H)


def _put(case, slot, name, role, mean, scale, opacity=0.8, **expect):
    sc, i = case.scene, SLOTS[slot]
    sc.means3D[i] = torch.from_numpy(np.asarray(mean, dtype=F))
    sc.scales[i] = torch.from_numpy(np.broadcast_to(np.asarray(scale, dtype=F), (3,)).copy())
    sc.rotations[i] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    sc.opacities[i] = torch.from_numpy(np.asarray([opacity], dtype=F))
    row = dict(row=i, name=name, role=role, alive=None, radius=None, psize=None, no_pixels=False, lhs=None, rhs=None, rel=None)
    row.update(expect)
    case.rows.append(row)
    return row


# ---------------------------------------------------------------------------------------------------------------------------
# float32 restatement of K1's phase A (preprocess.hip, one rounding per operation, the kernel's operation order)
# ---------------------------------------------------------------------------------------------------------------------------
def _cov3d_f32(s, q, mod):
    r, x, y, z = (q[:, k] for k in range(4))
    one, two = F(1), F(2)
    R = [[one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)],
         [two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)],
         [two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)]]
    S = [F(mod) * s[:, k] for k in range(3)]
    M = [[R[i][j] * S[j] for j in range(3)] for i in range(3)]
    dot = lambda a, b: (M[a][0] * M[b][0] + M[a][1] * M[b][1]) + M[a][2] * M[b][2]
    return np.stack([dot(0, 0), dot(0, 1), dot(0, 2), dot(1, 1), dot(1, 2), dot(2, 2)], axis=1)


def k1_f32(case, opacities=None):
    """the operands of K1's comparators for every row of the case, float32 arrays [P]"""
    sc, cam = case.scene, case.cam
    W, H = F(cam.image_width), F(cam.image_height)
    V = cam.world_view_transform.numpy().astype(F).reshape(-1)
    PM = cam.full_proj_transform.numpy().astype(F).reshape(-1)
    p = sc.means3D.numpy().astype(F)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    o = (sc.opacities if opacities is None else opacities).numpy().astype(F).reshape(-1)
    tanx, tany = F(math.tan(cam.FoVx * 0.5)), F(math.tan(cam.FoVy * 0.5))
    with np.errstate(all="ignore"):
        t = [((V[k] * x + V[4 + k] * y) + V[8 + k] * z) + V[12 + k] for k in range(3)]
        h = [((PM[k] * x + PM[4 + k] * y) + PM[8 + k] * z) + PM[12 + k] for k in range(4)]
        pw = F(1) / (h[3] + F(0.0000001))
        ndc_x, ndc_y = h[0] * pw, h[1] * pw
        fx, fy = W / (F(2) * tanx), H / (F(2) * tany)
        limx, limy = F(1.3) * tanx, F(1.3) * tany
        txtz, tytz = t[0] / t[2], t[1] / t[2]
        tx_c = np.minimum(limx, np.maximum(-limx, txtz)) * t[2]
        ty_c = np.minimum(limy, np.maximum(-limy, tytz)) * t[2]
        zero = np.zeros_like(x)
        J = [[fx / t[2], zero, -(fx * tx_c) / (t[2] * t[2])], [zero, fy / t[2], -(fy * ty_c) / (t[2] * t[2])]]
        T = [[(J[r][0] * V[4 * c + 0] + J[r][1] * V[4 * c + 1]) + J[r][2] * V[4 * c + 2] for c in range(3)] for r in range(2)]
        cov = case.cov3D.numpy().astype(F) if case.cov3D is not None else \
            _cov3d_f32(sc.scales.numpy().astype(F), sc.rotations.numpy().astype(F), 1.0)
        S = [[cov[:, 0], cov[:, 1], cov[:, 2]], [cov[:, 1], cov[:, 3], cov[:, 4]], [cov[:, 2], cov[:, 4], cov[:, 5]]]
        ST = [[(S[i][0] * T[r][0] + S[i][1] * T[r][1]) + S[i][2] * T[r][2] for i in range(3)] for r in range(2)]
        a0 = (T[0][0] * ST[0][0] + T[0][1] * ST[0][1]) + T[0][2] * ST[0][2]
        b = (T[0][0] * ST[1][0] + T[0][1] * ST[1][1]) + T[0][2] * ST[1][2]
        c0 = (T[1][0] * ST[1][0] + T[1][1] * ST[1][1]) + T[1][2] * ST[1][2]
        a, c = a0 + F(0.3), c0 + F(0.3)
        det = a * c - b * b
        mid = F(0.5) * (a + c)
        root = np.sqrt(np.maximum(F(0.1), mid * mid - det))
        three_sigma = F(3) * np.sqrt(np.maximum(mid + root, mid - root))
        radius = np.ceil(three_sigma)
        px = ((ndc_x + F(1)) * W - F(1)) * F(0.5)
        py = ((ndc_y + F(1)) * H - F(1)) * F(0.5)
        lo_x, lo_y = px - radius, py - radius
        hi_x, hi_y = ((px + radius) + F(16)) - F(1), ((py + radius) + F(16)) - F(1)
        v255 = F(255) * o
    return dict(tx=t[0], ty=t[1], tz=t[2], hw=h[3], pw=pw, ndc_x=ndc_x, ndc_y=ndc_y, txtz=txtz, tytz=tytz, limx=limx, limy=limy,
                a0=a0, b=b, c0=c0, a=a, c=c, det=det, three_sigma=three_sigma, radius=radius, px=px, py=py, lo_x=lo_x,
                lo_y=lo_y, hi_x=hi_x, hi_y=hi_y, v255=v255, fx=fx, fy=fy)


# ---------------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------------
def case_near():
    """Q1: t.z <= 0.2f culls.  T- and T are culled (radii 0, pixel_sizes 0, every gradient exactly 0), T+ is alive; with large
    x, y the decision still reads z alone (T+ then fails the rect, which leaves pixel_sizes > 0: still told apart from Q1)"""
    sc, cam = _base(7101)
    case = Case("near", sc, cam)
    s = 0.012                                                        # 3.8 px at z = 0.2
    k = 0
    for tag, (x, y) in (("centre", (0.0, 0.0)), ("far_a", (5.0, -3.0)), ("far_b", (-2.0, 4.0))):
        onscreen = tag == "centre"
        for role, zz in (("T-", down(NEAR)), ("T", NEAR), ("T+", up(NEAR))):
            culled = role != "T+"
            _put(case, k, f"{tag} {role}", role, (x, y, zz), s, lhs="tz", rhs=NEAR, rel={"T-": "<", "T": "==", "T+": ">"}[role],
                 alive=False if culled else onscreen, psize="zero" if culled else "pos", q1=culled)
            k += 1
    return case


def case_degenerate():
    """Q3: det == 0.0f culls.  cov3D_precomp, mean on the axis at z = 1 (fx / z = 64): Sxx = Syy = |Sxy| = 2^13 gives
    a0 = |b| = c0 = 2^25, the +0.3 is absorbed and det == 0; with |Sxy| one ulp smaller det = 2^27 > 0 and the row is alive
    with the radius of Q4's float32 restatement.  (A negative determinant is out of scope.)"""
    from oracle import torch_oracle as to
    sc, cam = _base(7102)
    case = Case("degenerate", sc, cam)
    k = 0
    S = F(2.0 ** 13)
    for sign in (1.0, -1.0):
        for rep in range(2):
            for role, sxy in (("T", S), ("T-", toward0(S))):
                dead = role == "T"
                _put(case, k, f"{'pos' if sign > 0 else 'neg'}{rep} {role}", role, (0.0, 0.0, 1.0), 1.0, lhs="det", rhs=F(0),
                     rel="==" if dead else ">", alive=not dead, psize="zero" if dead else "pos",
                     radius=None if dead else "restated", sxy=F(sign) * sxy)
                k += 1
    cov = to.cov3d_from_scale_rot(sc.scales, sc.rotations, 1.0).to(torch.float32).contiguous()
    for r in case.rows:
        cov[r["row"]] = torch.from_numpy(np.asarray([S, r["sxy"], 0.0, S, 0.0, S], dtype=F))
    case.cov3D = cov
    return case


RECT_SCALE = 0.065                        # 3 sqrt(lambda) ~ 7.4 .. 7.6 at the four edges: radius 8, far from ceil's own tie
X_LEFT, X_RIGHT = F(-1.203125), F(1.265625)      # px = -7 (px + 8 + 15 == 16) and px = 72 (px - 8 == 64) on a 64-pixel axis


def _rect_operand(v, edge):
    """the compared operand of an isotropic radius-8 row at z = 2 on a 64-pixel axis, as K1 forms it from the coordinate v"""
    px = ((F(v) + F(1)) * F(64) - F(1)) * F(0.5)
    return ((px + F(8)) + F(16)) - F(1) if edge == "low" else px - F(8)


def _rect_neighbour(v, edge, step):
    """the nearest float32 coordinate beyond v (step = up / down) at which the operand leaves the tie: one ulp of the
    coordinate on the low edge; on the high edge x + 1 has the coarser ulp and swallows the first step"""
    tie, w = _rect_operand(v, edge), v
    for _ in range(4):
        w = step(w)
        if _rect_operand(w, edge) != tie:
            return w
    raise AssertionError((v, edge))


def case_rect():
    """Q5: (maxx - minx) * (maxy - miny) == 0 culls.  Isotropic, z = 2, identity rotation, radius 8.
    low edge:  px + r + 15 == 16.0 -> max = 1, alive; one ulp less -> max = 0, culled (T- culled, T and T+ alive)
    high edge: px - r == 64.0 -> min = 4 = grid, culled; one ulp less -> min = 3, alive (T- alive, T and T+ culled)"""
    sc, cam = _base(7103)
    case = Case("rect", sc, cam)
    k = 0
    for axis in ("x", "y"):
        for edge, v in (("low", X_LEFT), ("high", X_RIGHT)):
            for role, vv in (("T-", _rect_neighbour(v, edge, down)), ("T", v), ("T+", _rect_neighbour(v, edge, up))):
                alive = (role != "T-") if edge == "low" else (role == "T-")
                mean = (vv, 0.0, 2.0) if axis == "x" else (0.0, vv, 2.0)
                _put(case, k, f"{axis} {edge} {role}", role, mean, RECT_SCALE, lhs=("hi_" if edge == "low" else "lo_") + axis,
                     rhs=F(16) if edge == "low" else F(64), rel={"T-": "<", "T": "==", "T+": ">"}[role], alive=alive,
                     radius=8 if alive else None, psize="pos", axis=axis)
                k += 1
    return case


def case_rect_ragged():
    """70 x 50 (5 x 4 tiles, the last column 6 and the last row 2 pixels wide): a centre beyond the last pixel column / row
    whose rect still starts inside the last tile's nominal 16-pixel span is alive (radii > 0: the reference's
    visibility_filter) although no pixel can see it; one whose rect starts beyond the span is culled"""
    sc, cam = _base(7104, 70, 50)
    case = Case("rect_ragged", sc, cam)
    # px = ((x + 1) 70 - 1) / 2, py = ((y + 1) 50 - 1) / 2 at z = 2
    _put(case, 0, "x inside span", "in", (169.0 / 70.0 - 1.0, 0.0, 2.0), RECT_SCALE, alive=True, psize="pos", no_pixels=True,
         lhs="lo_x", span=(64.0, 80.0))
    _put(case, 1, "x beyond span", "out", (185.0 / 70.0 - 1.0, 0.0, 2.0), RECT_SCALE, alive=False, psize="pos", lhs="lo_x",
         span=(80.0, 1e9))
    _put(case, 2, "y inside span", "in", (0.0, 117.0 / 50.0 - 1.0, 2.0), RECT_SCALE, alive=True, psize="pos", no_pixels=True,
         lhs="lo_y", span=(48.0, 64.0))
    _put(case, 3, "y beyond span", "out", (0.0, 149.0 / 50.0 - 1.0, 2.0), RECT_SCALE, alive=False, psize="pos", lhs="lo_y",
         span=(64.0, 1e9))
    return case


def case_gate():
    """M1: 255f * o > 1.0f gates the pixel size (and the tile count).  o = float32(1) / float32(255) gives exactly 1.0f:
    pixel_sizes = 0, radii > 0, no pixel (T- the same, T+ has a size).  Three more rows at the tie carry a min_pixel_size
    (1.0, 0, -1): with filter_small on, M2 applied to size 0 drops the first and only the first (gate_filters)."""
    sc, cam = _base(7105)
    case = Case("gate", sc, cam)
    for k, (role, o) in enumerate((("T-", down(O_GATE)), ("T", O_GATE), ("T+", up(O_GATE)))):
        _put(case, k, f"gate {role}", role, (0.125 * (k - 1), 0.0, 2.0), RECT_SCALE, opacity=o, lhs="v255", rhs=F(1),
             rel={"T-": "<", "T": "==", "T+": ">"}[role], alive=True, psize="pos" if role == "T+" else "zero",
             no_pixels=role != "T+")
    for k, mn in enumerate((1.0, 0.0, -1.0)):
        _put(case, 3 + k, f"min {mn:g}", "T", (0.125 * (k - 1), 0.25, 2.0), RECT_SCALE, opacity=O_GATE, lhs="v255", rhs=F(1),
             rel="==", alive=True, psize="zero", no_pixels=True, min_ps=mn)
    return case


def gate_filters(case, fade):
    """(settings, min_ps, max_ps, base_mask, {row: alive}) of the gate case with the small filter on"""
    sc = case.scene
    mn = sc.min_pixel_sizes.clone()
    alive = {}
    for r in case.rows:
        if "min_ps" in r:
            mn[r["row"]] = r["min_ps"]
            alive[r["row"]] = not r["min_ps"] > 0
        else:
            alive[r["row"]] = True
    return dict(filter_small=True, filter_large=True, fade_size=fade), mn, sc.max_pixel_sizes.clone(), sc.base_mask.clone(), alive


N_CAL = 30


def case_filters():
    """M2-M4: thirty rows inside the image whose thresholds are set from a first, unfiltered pass (the implementation's own
    pixel_sizes bits, so that nothing depends on logf): filter_plan()"""
    sc, cam = _base(7106)
    case = Case("filters", sc, cam)
    for k in range(N_CAL):
        x, y = -0.75 + 0.25 * (k % 7), -0.5 + 0.25 * (k // 7)              # half-pixel centres 7.5 + 8 j
        _put(case, k, f"cal {k}", "cal", (x, y, 2.0), 0.05 + 0.002 * k, opacity=0.3 + 0.02 * k, alive=True, psize="pos")
    return case


def _exact(prod, a, b):
    """prod == a * b in exact rational arithmetic"""
    return Fraction(float(prod)) == Fraction(float(a)) * Fraction(b)


FADE0_ROLES = ("min_eq", "min_up", "min_zero", "min_neg", "max_eq", "max_down", "max_zero", "max_neg", "base_min_up",
               "base_max_down")


def filter_plan(case, run, s):
    """(settings, min_ps, max_ps, base_mask, {row: dict(role, alive, w)}) for run in "fade0" / "fade1" / "fade05", from the
    calibrated sizes s [P] (float32 or float64 numpy: the thresholds are built in s's own format)
      fade0 (fade_size 0):  min_ps = s kept, one ulp above dropped, 0 and -1 no filter; max_ps = s kept, one ulp below dropped,
                            0 and -1 no filter; base_mask with min_ps one ulp above kept, with max_ps one ulp below dropped
      fade1 (fade_size 1):  min_ps = 2 s: w = 0, dropped; one ulp below 2 s: w ~ 1 ulp, alive, no pixel; max_ps = s / 2 dropped;
                            min_ps = 1.5 s (a row where that product is exact): w = 0.5; the same with max_ps = m, s / m == 1.5
                            as well: w = 0.25
      fade05 (fade_size 0.5): the rows of fade1; min_ps = 1.5 s now gives w = 0"""
    dt = s.dtype
    rows = [r["row"] for r in case.rows]
    Pn = case.scene.P
    mn, mx = np.full(Pn, -1.0, dtype=dt), np.full(Pn, -1.0, dtype=dt)
    base = np.zeros(Pn, dtype=bool)
    plan = {}
    one5 = dt.type(1.5)
    if run == "fade0":
        for role, i in zip(FADE0_ROLES, rows):
            si = s[i]
            alive = True
            if role == "min_eq":
                mn[i] = si
            elif role in ("min_up", "base_min_up"):
                mn[i] = up(si)
                base[i] = role.startswith("base")
                alive = bool(base[i])
            elif role == "min_zero":
                mn[i] = 0
            elif role == "max_eq":
                mx[i] = si
            elif role in ("max_down", "base_max_down"):
                mx[i] = toward0(si)
                base[i] = role.startswith("base")
                alive = False
            elif role == "max_zero":
                mx[i] = 0
            plan[i] = dict(role=role, alive=alive, w=1.0 if alive else 0.0)
        return dict(filter_small=True, filter_large=True, fade_size=0.0), mn, mx, base, plan
    fixed = rows[len(FADE0_ROLES):len(FADE0_ROLES) + 3]
    pool = rows[len(FADE0_ROLES) + 3:]
    i = fixed[0]
    mn[i] = dt.type(2) * s[i]
    plan[i] = dict(role="min_2s", alive=False, w=0.0)
    i = fixed[1]
    mn[i] = toward0(dt.type(2) * s[i])
    plan[i] = dict(role="min_2s_down", alive=run == "fade1", w=None if run == "fade1" else 0.0, no_pixels=True)
    i = fixed[2]
    mx[i] = s[i] / dt.type(2)
    plan[i] = dict(role="max_half", alive=False, w=0.0)
    exact15 = [i for i in pool if _exact(one5 * s[i], s[i], Fraction(3, 2))]
    both = None
    for i in exact15:
        m = s[i] / one5
        for cand in (m, up(m), down(m)):
            if s[i] / cand == one5 and s[i] > cand:
                both = (i, cand)
                break
        if both:
            break
    assert both is not None and len(exact15) >= 2, "no calibrated row has an exact 1.5 s (and s / m == 1.5)"
    half = [i for i in exact15 if i != both[0]][0]
    w15 = 0.5 if run == "fade1" else 0.0
    mn[half] = one5 * s[half]
    plan[half] = dict(role="min_1.5s", alive=w15 > 0, w=w15)
    mn[both[0]] = one5 * s[both[0]]
    mx[both[0]] = both[1]
    plan[both[0]] = dict(role="both_1.5", alive=w15 > 0, w=w15 * w15)
    return dict(filter_small=True, filter_large=True, fade_size=1.0 if run == "fade1" else 0.5), mn, mx, base, plan


def with_filters(case, mn, mx, base, opacities=None):
    """a copy of the case's scene carrying these thresholds (float32 tensors: what the op and the float32 oracles take)"""
    sc = copy.copy(case.scene)
    sc.min_pixel_sizes = torch.as_tensor(np.asarray(mn)).to(torch.float32).contiguous()
    sc.max_pixel_sizes = torch.as_tensor(np.asarray(mx)).to(torch.float32).contiguous()
    sc.base_mask = torch.as_tensor(np.asarray(base)).to(torch.bool).contiguous()
    if opacities is not None:
        sc.opacities = opacities
    return sc


def metamorphic_pair(case, mn, mx, base, plan):
    """M4: (scene A, scene B, {row: w}).  A carries the fade1 plan; B is A with the filters of the 0 < w < 1 rows disabled and
    their opacity multiplied by w (a power of two: exact).  Renders and gradients must be equal, dL/dopacity of those rows in A
    exactly w times B's.  (pixel_sizes of those rows, and with them acc_pixel_size, legitimately differ: M1 reads the input
    opacity.)"""
    ws = {i: p["w"] for i, p in plan.items() if p["w"] is not None and 0.0 < p["w"] < 1.0}
    mn2, mx2 = np.array(mn, copy=True), np.array(mx, copy=True)
    o2 = case.scene.opacities.clone()
    for i, w in ws.items():
        mn2[i] = mx2[i] = -1.0
        o2[i] = o2[i] * w
    return with_filters(case, mn, mx, base), with_filters(case, mn2, mx2, base, o2), ws


CLAMP_SIDES = (("x", 1.0), ("x", -1.0), ("y", 1.0), ("y", -1.0))


def case_clamp(sz=0.3):
    """Q2: t.x / t.z < -lim or > lim masks the Jacobian's x-term (strict: a coordinate ON the limit keeps its gradient).
    z = 1, |x| = 0.65f = 1.3f * 0.5f.  T- (one ulp inside) and T are not clamped, T+ (one ulp outside) is.  The centre is
    off-screen at px ~ 1.15 W; the footprint (sigma ~ 14 px towards the image, `sz` along the view axis feeding the masked
    term) reaches it with weight.  Same on the negative side and in y."""
    sc, cam = _base(7107)
    case = Case("clamp", sc, cam)
    k = 0
    for axis, sign in CLAMP_SIDES:
        for role, v, off in (("T-", toward0(LIMIT), -0.25), ("T", LIMIT, 0.0), ("T+", up(LIMIT), 0.25)):
            v = F(sign) * v
            mean = (v, off, 1.0) if axis == "x" else (off, v, 1.0)
            scale = (0.1, 0.08, sz) if axis == "x" else (0.08, 0.1, sz)
            rel = {"T-": "<", "T": "==", "T+": ">"}[role]
            if sign < 0:
                rel = {"<": ">", "==": "==", ">": "<"}[rel]
            _put(case, k, f"{axis}{'+' if sign > 0 else '-'} {role}", role, mean, scale, opacity=0.5, lhs="t" + axis + "tz",
                 rhs=F(sign) * LIMIT, rel=rel, alive=True, psize="pos", axis=axis, sign=sign, clamped=role == "T+")
            k += 1
    return case


def clamp_variant(case, name, role):
    """the case's scene with the row `name` moved onto its neighbour `role` ("T-" / "T+") along the clamped axis, all else equal"""
    r = case.named(name)
    sc = copy.copy(case.scene)
    sc.means3D = sc.means3D.clone()
    lim = LIMIT if role == "T" else (toward0(LIMIT) if role == "T-" else up(LIMIT))
    sc.means3D[r["row"], 0 if r["axis"] == "x" else 1] = float(F(r["sign"]) * lim)
    return sc


def clamp_probe():
    """twelve rows (the four sides x T-, T, T+) alone, all with the other image coordinate 0: the preprocess-level probe of the
    mask (the conic's gradient towards the clamped coordinate)"""
    case = case_clamp()
    idx = torch.tensor([r["row"] for r in case.rows])
    sc = case.scene.subset(idx)
    for j, r in enumerate(case.rows):
        sc.means3D[j, 1 if r["axis"] == "x" else 0] = 0.0
    return sc, case.cam, case.rows


def check_rows(what, case, radii, psize, alive_of=None):
    """the expectations of the case's rows against (radii, pixel_sizes) [P] of an oracle or of the kernels; alive_of {row: alive}
    overrides the rows' own (a filtered run)"""
    k1 = k1_f32(case)
    for r in case.rows:
        i = r["row"]
        alive = r["alive"] if alive_of is None else alive_of.get(i, r["alive"])
        if alive is not None:
            assert (radii[i] > 0) == alive, (what, r["name"], int(radii[i]))
        want = r["radius"]
        if alive and want is not None:
            want = int(k1["radius"][i]) if want == "restated" else want
            assert int(radii[i]) == want, (what, r["name"], int(radii[i]), want)
        if r["psize"] is not None:
            assert (psize[i] == 0) if r["psize"] == "zero" else (psize[i] > 0), (what, r["name"], float(psize[i]))


CASES = dict(near=case_near, degenerate=case_degenerate, rect=case_rect, rect_ragged=case_rect_ragged, gate=case_gate,
             filters=case_filters, clamp=case_clamp)

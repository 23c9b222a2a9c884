"""Footprint families for the culling tests, drawn in 2-D: centre (px, py), sigma along and across the major axis in pixels,
angle, opacity, view depth.  Two ways from there:

  synthetic_records()  float32 records built directly from the 2-D parameters, with the float32 steps preprocess.hip takes from
                       the 2-D covariance on (determinant, conic, radius, log2 scaling, tau2): the CPU tests' inputs
  scene_of()           a scenes.Scene for scenes.front_camera whose Gaussians AIM at those footprints: flat discs / needles with
                       scales (s1, s2, tiny) rotated about the view axis at the depth drawn (cov2D = (f / z)^2 R diag(s1^2, s2^2) R^T
                       + 0.3 I whatever the centre, because the disc has no extent along the view axis).  What the op makes of them is
                       read back from its records; every family property is asserted from those (tests/test_culling_gpu.py).

Seeded with numpy's PCG64: the same bits on every machine."""
import math

import numpy as np
import torch

KLOG = np.float32(-0.72134752044448170368)         # -1/2 log2(e)
SPECIAL_ANGLES = (0.0, 45.0, 90.0, 135.0)
TINY = 1e-3                                        # world-space scale along the view axis


def _loguniform(g, lo, hi, n):
    return np.exp(g.uniform(math.log(lo), math.log(hi), n))


def _angles(g, n, special=0.3, about=None, spread=None):
    """degrees: uniform in [0, 180), a share `special` of them at 0/45/90/135 -+ 1e-3; or, with `about`, within `spread` of it"""
    if about is not None:
        return (about + g.uniform(-spread, spread, n)) % 180.0
    th = g.uniform(0.0, 180.0, n)
    sp = g.random(n) < special
    th_sp = np.asarray(SPECIAL_ANGLES)[g.integers(0, 4, n)] + g.choice([-1e-3, 0.0, 1e-3], n)
    return np.where(sp, th_sp, th) % 180.0


def _centres(g, n, W, H, border=0.25, off=0.0):
    """a share `border` on tile borders (x or y a multiple of 16, or half a pixel / a pixel below one), the rest uniform on the
    image; also returns the share `off` of rows the caller moves off-screen"""
    px, py = g.uniform(-0.5, W - 0.5, n), g.uniform(-0.5, H - 0.5, n)
    kind = g.random(n)
    on_b = kind < border
    bx = 16.0 * g.integers(0, W // 16 + 1, n) - g.choice([0.0, 0.5, 1.0], n)
    by = 16.0 * g.integers(0, H // 16 + 1, n) - g.choice([0.0, 0.5, 1.0], n)
    which = g.random(n) < 0.5
    px = np.where(on_b & which, bx, px)
    py = np.where(on_b & ~which, by, py)
    is_off = (kind >= border) & (kind < border + off)
    return px, py, is_off


def _pack(px, py, s1, s2, theta, opacity, depth):
    return dict(px=np.asarray(px, np.float64), py=np.asarray(py, np.float64), s1=np.asarray(s1, np.float64),
                s2=np.asarray(s2, np.float64), theta=np.asarray(theta, np.float64), opacity=np.asarray(opacity, np.float64),
                depth=np.asarray(depth, np.float64))


def concat(*fams):
    return {k: np.concatenate([f[k] for f in fams]) for k in fams[0]}


def repeat(fam, times):
    return {k: np.tile(v, times) for k, v in fam.items()}


def needles(n, W, H, seed, s_major=(3.0, 1e4), s_minor=(0.6, 4.0), max_aspect=10 ** 3.5, opacity=(0.0045, 0.3), off=0.2,
            depth=(2.0, 10.0), angle=None, spread=None, border=0.25):
    """the prototype's families: sigma_major log-uniform, aspect up to max_aspect, every angle incl. 0/45/90/135 -+ 1e-3, centres
    on tile borders and off-screen (an off-screen needle points at the image, within a few degrees), opacities log-uniform"""
    g = np.random.default_rng(seed)
    s1 = _loguniform(g, s_major[0], s_major[1], n)
    s2 = np.minimum(_loguniform(g, s_minor[0], s_minor[1], n), s1)
    s2 = np.maximum(s2, s1 / max_aspect)
    th = _angles(g, n, about=angle, spread=spread)
    px, py, is_off = _centres(g, n, W, H, border=border, off=off)
    # off-screen: along the needle's own axis (within two degrees), up to 20 000 px but no further than 1.5 sigma_major, from
    # where its level set can still reach back
    d = g.uniform(0.2, 1.0, n) * np.minimum(20000.0, 1.5 * s1) * g.choice([-1.0, 1.0], n)
    aim = np.radians(th + g.uniform(-2.0, 2.0, n))
    px = np.where(is_off, (W - 1) / 2 + g.uniform(-0.4, 0.4, n) * W + d * np.cos(aim), px)
    py = np.where(is_off, (H - 1) / 2 + g.uniform(-0.4, 0.4, n) * H + d * np.sin(aim), py)
    return _pack(px, py, s1, s2, th, _loguniform(g, opacity[0], opacity[1], n), g.uniform(depth[0], depth[1], n))


def covariance(fam):
    """(a, b, c) of the 2-D covariance in float64; the sigmas include the 0.3 px^2 screen-space dilation"""
    th = np.radians(fam["theta"])
    co, si = np.cos(th), np.sin(th)
    v1, v2 = fam["s1"] ** 2, fam["s2"] ** 2
    return v1 * co * co + v2 * si * si, (v1 - v2) * co * si, v1 * si * si + v2 * co * co


def synthetic_records(fam, seed=0):
    """(rec12 [n, 12] float32, radii [n] int64): the covariance rounded to float32, then preprocess.hip's float32 steps"""
    f32 = np.float32
    a, b, c = (v.astype(f32) for v in covariance(fam))
    n = a.shape[0]
    with np.errstate(all="ignore"):
        det = a * c - b * b
        inv = f32(1.0) / det
        conA, conB, conC = c * inv, -b * inv, a * inv
        mid = f32(0.5) * (a + c)
        root = np.sqrt(np.maximum(f32(0.1), mid * mid - det))
        radius = np.ceil(f32(3.0) * np.sqrt(np.maximum(mid + root, mid - root)))
        sA, sBh, sC = KLOG * conA, KLOG * conB, KLOG * conC
        o = fam["opacity"].astype(f32)
        v255 = f32(255.0) * o
        tau2 = -np.log2(v255).astype(f32)
        tau2 = tau2 - (f32(1e-5) * np.abs(tau2) + f32(2e-3))
        nd = (sA < 0) & (sC < 0) & (sA * sC - sBh * sBh > 0)
        tau2 = np.where(v255 > 1, np.where(nd, tau2, f32(-3.0e38)), f32(1.0)).astype(f32)
    rgb = np.random.default_rng(seed + 77).uniform(0.2, 1.0, (n, 3)).astype(f32)
    rec = np.stack([fam["px"].astype(f32), fam["py"].astype(f32), sA, sBh, sC, np.log2(o).astype(f32), rgb[:, 0], rgb[:, 1],
                    rgb[:, 2], fam["depth"].astype(f32), np.zeros(n, f32), tau2], 1).astype(f32)
    ok = (det != 0) & np.isfinite(rec).all(1)
    radii = np.where(ok, np.minimum(radius, 2.0e9), 0).astype(np.int64)
    return torch.from_numpy(rec), torch.from_numpy(radii)


def scene_of(fam, W, H):
    """the scenes.Scene that aims at the family under scenes.front_camera(W, H)"""
    import scenes
    n = fam["px"].shape[0]
    f = 1000.0 * W / 1920.0
    z = fam["depth"]
    x, y = (fam["px"] - (W - 1) / 2) * z / f, (fam["py"] - (H - 1) / 2) * z / f
    s1 = np.sqrt(np.maximum(fam["s1"] ** 2 - 0.3, 1e-4)) * z / f
    s2 = np.sqrt(np.maximum(fam["s2"] ** 2 - 0.3, 1e-4)) * z / f
    half = np.radians(fam["theta"]) / 2
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).float()
    return scenes.Scene(means3D=t(np.stack([x, y, z], 1)), scales=t(np.stack([s1, s2, np.full(n, TINY)], 1)),
                        rotations=t(np.stack([np.cos(half), np.zeros(n), np.zeros(n), np.sin(half)], 1)),
                        opacities=t(fam["opacity"][:, None]), shs=torch.zeros(n, 16, 3), max_pixel_sizes=-torch.ones(n),
                        min_pixel_sizes=-torch.ones(n), occ_multiplier=torch.ones(n, 4, 1), dc_delta=torch.zeros(n, 12, 1),
                        base_mask=torch.zeros(n, dtype=torch.bool), sh_degree=3, target_reso_lvl=torch.zeros(n, dtype=torch.long),
                        meta=dict(kind="culling"))


# ------------------------------------------------------------------------------------------- the scenes of the GPU tests ---
LOW = (0.005, 0.012)            # opacities of W / Q / T: hundreds of overlapping footprints must leave min T >= 1e-2


def scene_L():
    """thread path, small stage: 256 x 192, P = 256, the prototype's families; every footprint at most 96 tiles.  Four groups:
    blobs and short needles (aspect up to 30, any angle); long needles along the axes -+ 1e-3 degrees with every aspect up to
    10^3.5 and centres up to 20 000 px off-screen; four long oblique needles (45 / 135 -+ 1e-3 and two free angles) on the screen.
    (Far from the centre of a long OBLIQUE needle the three monomials of the exponent are ~(d / sigma_minor)^2 each and cancel:
    float32 cannot decide those pairs, the band says so, and the band condition limits how many of them a scene may hold.)"""
    W, H = 256, 192
    g = np.random.default_rng(13)
    axis = needles(44, W, H, 12, s_major=(40.0, 1e4), s_minor=(0.6, 1.5), opacity=(0.0045, 0.05), off=0.5)
    axis["theta"] = (np.asarray([0.0, 90.0])[g.integers(0, 2, 44)] + g.choice([-1e-3, 0.0, 1e-3], 44)) % 180.0
    # (the off-screen centres were placed along the angle drawn first: put them along the new one, pointing at the image)
    far = (axis["px"] < 0) | (axis["px"] > W - 1) | (axis["py"] < 0) | (axis["py"] > H - 1)
    d = np.hypot(axis["px"] - W / 2, axis["py"] - H / 2) * g.choice([-1.0, 1.0], 44)
    horiz = np.round(axis["theta"] / 90.0) % 2 == 0
    axis["px"] = np.where(far, np.where(horiz, W / 2 + d, g.uniform(8.0, W - 8.0, 44)), axis["px"])
    axis["py"] = np.where(far, np.where(horiz, g.uniform(8.0, H - 8.0, 44), H / 2 + d), axis["py"])
    oblique = needles(4, W, H, 15, s_major=(300.0, 5000.0), s_minor=(1.5, 3.0), opacity=(0.008, 0.03), off=0.0)
    oblique["theta"] = np.asarray([45.001, 134.999, 27.0, 118.0])
    return W, H, concat(needles(138, W, H, 11, s_major=(3.0, 10.0), s_minor=(2.0, 10.0), opacity=(0.0045, 0.3), off=0.0),
                        needles(70, W, H, 14, s_major=(3.0, 50.0), s_minor=(0.6, 3.0), max_aspect=30.0, opacity=(0.0045, 0.3), off=0.0),
                        axis, oblique)


def _giants(n, W, H, seed, opacity=LOW, s_major=(300.0, 3000.0), s_minor=(40.0, 70.0)):
    return needles(n, W, H, seed, s_major=s_major, s_minor=s_minor, opacity=opacity, off=0.0, border=0.5)


def scene_W():
    """wave path, wide stage: 256 x 192, P = 256; 32 wide bands across the image among thin needles.  (The thin ones of W and Q
    keep to aspect 150 and low opacities: the float32 exponent of a long oblique needle is off by ~1e-7 (d / sigma_minor)^2 far
    from its centre, and a needle of aspect 300 and opacity 0.05 alone moved a pixel by the whole forward tolerance, 1.0e-5.)"""
    W, H = 256, 192
    return W, H, concat(_giants(32, W, H, 21, opacity=(0.008, 0.03)),
                        needles(224, W, H, 22, s_major=(20.0, 300.0), s_minor=(2.0, 4.0), opacity=(0.006, 0.03), off=0.0))


def scene_Q():
    """unstaged blocks: 256 x 192, P = 512, two rank blocks; in each more than 12288 instances, heavy and light footprints"""
    W, H = 256, 192
    return W, H, concat(_giants(280, W, H, 31), needles(232, W, H, 32, s_major=(20.0, 300.0), s_minor=(2.0, 4.0), opacity=LOW,
                                                        off=0.0))


def scene_T(copies=1):
    """more than 64 tile rows: 64 x 1104 (4 x 69 tiles), P = 128 x copies; near-vertical and slightly tilted needles"""
    W, H = 64, 1104
    base = concat(needles(36, W, H, 41, s_major=(1400.0, 2000.0), s_minor=(14.0, 30.0), opacity=(0.008, 0.012), off=0.0, angle=90.0,
                          spread=2.0, border=0.5),
                  needles(92, W, H, 42, s_major=(50.0, 2000.0), s_minor=(1.5, 4.0), opacity=LOW, off=0.0, angle=90.0, spread=8.0))
    return W, H, repeat(base, copies)


def scene_O():
    """level set beyond the rect: 256 x 192, P = 24, opacities 0.9 .. 0.98 (the 1/255 level set reaches 3.3 sigma, the rect
    3 sigma); on a 6 x 4 grid 40 px apart so that no footprint reaches another's core, every second centre placed so that
    centre + radius ends half a pixel short of a tile border in x, the others in y"""
    W, H = 256, 192
    g = np.random.default_rng(51)
    n = 24
    s1 = g.uniform(7.0, 11.0, n)
    s2 = s1 / g.uniform(1.0, 1.6, n)
    th = np.where(np.arange(n) % 2 == 0, 0.0, 90.0) + g.choice([-1e-3, 0.0, 1e-3], n)
    r = np.ceil(3.0 * s1)                                           # the radius the op will find, to the rounding of s1
    cx, cy = 28.0 + 40.0 * (np.arange(n) % 6), 30.0 + 40.0 * (np.arange(n) // 6)
    # along the major axis: the smallest shift that puts centre + radius at 16 k - 0.5
    snap = lambda c: c + ((-0.5 - (c + r)) % 16.0)
    px = np.where(np.arange(n) % 2 == 0, snap(cx), cx)
    py = np.where(np.arange(n) % 2 == 1, snap(cy), cy)
    return W, H, _pack(px, py, s1, s2, th, g.uniform(0.9, 0.98, n), g.uniform(2.0, 10.0, n))

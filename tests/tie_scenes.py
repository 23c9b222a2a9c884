"""Scenes in which many Gaussians share their float32 view depth BIT FOR BIT, so that the second half of SPEC Q10 (DESIGN.md 2:
order inside a tile = depth bits ascending, THEN Gaussian index) decides what a pixel blends.  scenes.frustum_scene and
ball_scene draw continuous depths; two Gaussians with the same depth bits essentially never meet on screen there.

Everything is for scenes.front_camera(W, H): m2 = m6 = 0, m10 = 1, m14 = 0, so the view depth of Q1 — ((m2 x + m6 y) + m10 z)
+ m14 — IS means3D[:, 2], and a depth level is one sort key.  Shared by tests/test_depth_ties_cpu.py and
tests/test_depth_ties_gpu.py; every tensor is drawn from a CPU torch.Generator (the same bits on every machine)."""
import torch

import scenes

ONE_PLANE = (2.0,)
# the adjacent pair differs in the lowest key bit only: a higher index at the smaller depth must still come first
FOUR_PLANES = (1.5, 3.0, float(torch.nextafter(torch.tensor(3.0), torch.tensor(4.0))), 6.0)
TWO_PLANES = (2.0, 4.0)           # the large-P scenes and the occlusion scene
SLAB_PLANE = (3.0,)               # the depth-slab scene


def _tans(W, H):
    f = 1000.0 * W / 1920.0
    return f, W / (2.0 * f), H / (2.0 * f)


def _scene(means, scales, rot, opac, shs, sh_degree, meta):
    P = means.shape[0]
    return scenes.Scene(means3D=means.contiguous(), scales=scales.contiguous(), rotations=rot.contiguous(),
                        opacities=opac.contiguous(), shs=shs.contiguous(),
                        max_pixel_sizes=-torch.ones(P), min_pixel_sizes=-torch.ones(P),           # no multi-scale fields
                        occ_multiplier=torch.ones(P, 4, 1), dc_delta=torch.zeros(P, 12, 1),
                        base_mask=torch.zeros(P, dtype=torch.bool), sh_degree=sh_degree,
                        target_reso_lvl=torch.zeros(P, dtype=torch.long), meta=meta)


def tied_scene(P, W, H, seed, levels, culled, px, opac=(0.05, 0.6), clones=0.0, sh_degree=3, n_coeffs=16):
    """P Gaussians on the depth planes `levels` (z = levels[randint]), x and y uniform in +-1.05 z tan(fov / 2), footprints of
    about `px` pixels, opacity uniform in `opac`.  A `culled` share of the rows, interleaved with the others, sits at z = -1:
    not rendered (Q1), key 0xFFFFFFFF in the depth sort, which drops them in its first pass.  `clones` = c copies means, scales
    and rotations of c P / 2 random rows of the first half onto row + P / 2 — what densify_and_prune's clone leaves behind
    (SPEC D1: bit-identical xyz), with the partners P / 2 rows apart, i.e. in different blocks of the sort; opacity and SH stay
    different, so the order of a pair shows in every pixel it covers."""
    g = torch.Generator().manual_seed(seed)
    f, tanx, tany = _tans(W, H)
    lv = torch.tensor(levels, dtype=torch.float32)
    z = lv[torch.randint(0, lv.numel(), (P,), generator=g)]
    x = (2.0 * torch.rand(P, generator=g) - 1.0) * 1.05 * z * tanx
    y = (2.0 * torch.rand(P, generator=g) - 1.0) * 1.05 * z * tany
    gone = torch.rand(P, generator=g) < culled
    scales = torch.exp(torch.log(px / f * z)[:, None] + 0.4 * torch.randn(P, 3, generator=g))
    rot, _, shs = scenes._common_attrs(g, P, sh_degree, n_coeffs)
    opacities = opac[0] + (opac[1] - opac[0]) * torch.rand(P, 1, generator=g)
    means = torch.stack([x, y, torch.where(gone, -torch.ones(P), z)], dim=1)
    n_clones = int(clones * P / 2)
    if n_clones:
        half = P // 2
        src = torch.randperm(half, generator=g)[:n_clones]
        means[src + half] = means[src]
        scales[src + half] = scales[src]
        rot[src + half] = rot[src]
    return _scene(means, scales, rot, opacities, shs, sh_degree,
                  dict(kind="tied", seed=seed, width=W, height=H, levels=tuple(float(v) for v in lv), culled=culled, px=px,
                       clones=n_clones))


def exact_survivors_scene(P, W, H, seed, V, z=2.0, px=2.0, opac=(0.05, 0.6), sh_degree=0, n_coeffs=1):
    """P rows of which EXACTLY V are rendered: V random rows on the plane `z`, centred inside +-0.9 z tan(fov / 2) (on screen,
    so each owns at least the tile of its centre), the other P - V at z = -1.  For survivor counts on the chunk edges of the
    sort passes that run behind the compaction."""
    g = torch.Generator().manual_seed(seed)
    f, tanx, tany = _tans(W, H)
    keep = torch.zeros(P, dtype=torch.bool)
    keep[torch.randperm(P, generator=g)[:V]] = True
    x = (2.0 * torch.rand(P, generator=g) - 1.0) * 0.9 * z * tanx
    y = (2.0 * torch.rand(P, generator=g) - 1.0) * 0.9 * z * tany
    scales = torch.exp(torch.log(torch.tensor(px / f * z)) + 0.4 * torch.randn(P, 3, generator=g))
    rot, _, shs = scenes._common_attrs(g, P, sh_degree, n_coeffs)
    opacities = opac[0] + (opac[1] - opac[0]) * torch.rand(P, 1, generator=g)
    means = torch.stack([x, y, torch.where(keep, torch.full((P,), float(z)), -torch.ones(P))], dim=1)
    return _scene(means, scales, rot, opacities, shs, sh_degree,
                  dict(kind="exact_survivors", seed=seed, width=W, height=H, levels=(float(z),), V=V, px=px))


def with_giants(sc, W, H, seed, n_giants, giant_scale, giant_opacity, z):
    """`n_giants` random rows become screen-filling, nearly opaque Gaussians at depth `z` EXACTLY: cover candidates of the
    occlusion cut-off that tie with each other and with every small Gaussian of that plane, some at lower and some at higher
    indices (sizes and opacity as the giants of tests/test_occlusion_gpu.py)"""
    g = torch.Generator().manual_seed(seed + 1)
    idx = torch.randperm(sc.P, generator=g)[:n_giants]
    sc.means3D[idx, 2] = float(z)
    sc.means3D[idx, 0] *= 0.3
    sc.means3D[idx, 1] *= 0.3
    sc.scales[idx] = giant_scale * float(z) * (0.7 + 0.6 * torch.rand(n_giants, 3, generator=g))
    sc.opacities[idx, 0] = float(giant_opacity)
    sc.meta = dict(sc.meta, giants=idx)
    return sc


def reversed_rows(sc):
    """the same Gaussians in the opposite index order: every tie group is blended back to front instead"""
    return sc.subset(torch.arange(sc.P - 1, -1, -1))


def survivors(sc):
    """indices of the rows that are not culled by depth (Q1), in index order: sc.subset(survivors(sc)) keeps every tie order"""
    return torch.nonzero(sc.means3D[:, 2] > 0.2).squeeze(1)


def assert_tied(depths, levels):
    """the depths the op sees still carry the ties: at most len(levels) + 1 distinct values (the planes and the culled z)"""
    n = torch.unique(depths.detach().cpu()).numel()
    assert n <= len(levels) + 1, (n, levels)

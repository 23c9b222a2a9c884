"""Float64 truth of TSDF fusion and marching-tetrahedra extraction (SPEC M20; 4.22), written from the definitions,
the float32 restatements of both, and the cases their tests share.  Nothing here touches the library.

A volume is a dict with the layout of TSDFVolume.state_dict(): voxel_size, sdf_trunc, depth_trunc, origin, blocks (NBx, NBy, NBz),
block_coords [S,3] (bx, by, bz), tsdf_sum / weight_sum [S,512] (index i + 8 j + 64 k), colour_sum [S,3,512] or None.  Frames are
a dict: cams (camera objects), depth [n,H,W] float32, colour [n,3,H,W] or None, weight [n,H,W] or None.

Discrete decisions of the integration (which pixel, in front of the camera, inside the truncation band) can fall differently in
two float32 evaluations when a quantity lies on its threshold; integrate(..., dtype=float64) FLAGS such (lattice point, camera)
pairs, and a flagged lattice point is left out of value comparisons (at most MAX_BORDERLINE of them).  activate() returns the
block set twice: with every sample within BLOCK_SLACK of a block face counted on one side only where that is certain ("lo") and
on both sides ("hi").  Classification in extract() is on the sign of the stored sums: it has no borderline."""
import math

import numpy as np
import torch

import scenes

MAX_BORDERLINE = 0.02          # the cap on flagged lattice points per case (the figure of profiles/replay_sweep_notes.md)
BLOCK_SLACK = 1e-5             # in blocks: 4e-5 voxels, two orders above the float32 rounding of a block coordinate here
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))    # the six Kuhn tetrahedra: 0, e_a, e_a + e_b, 7


# ---- volumes ----
def empty_volume(voxel_size, sdf_trunc, depth_trunc, bounds, colour=True):
    voxel = float(np.float32(voxel_size))
    lo, hi = (np.asarray(b, dtype=np.float64) for b in bounds)
    origin = tuple(float(np.float32(x)) for x in lo)
    blocks = tuple(max(1, int(math.ceil((h - o) / (8 * voxel) - 1e-9))) for h, o in zip(hi, origin))
    return {"voxel_size": voxel, "sdf_trunc": float(np.float32(sdf_trunc)), "depth_trunc": float(depth_trunc), "origin": origin,
            "blocks": blocks, "block_coords": torch.zeros(0, 3, dtype=torch.int32), "tsdf_sum": torch.zeros(0, 512),
            "weight_sum": torch.zeros(0, 512), "colour_sum": torch.zeros(0, 3, 512) if colour else None}


def with_blocks(vol, marks):
    """a copy of `vol` with zeroed slots appended for the marked blocks [NBz,NBy,NBx] that have none, in ascending linear order"""
    nx, ny, nz = vol["blocks"]
    have = np.zeros(nx * ny * nz, dtype=bool)
    c = vol["block_coords"].long().numpy()
    have[(c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]] = True
    new = np.nonzero(np.asarray(marks).reshape(-1).astype(bool) & ~have)[0]
    coords = torch.tensor(np.stack([new % nx, (new // nx) % ny, new // (nx * ny)], axis=1), dtype=torch.int32).reshape(-1, 3)
    out = dict(vol)
    grow = lambda t: torch.cat([t, t.new_zeros((len(new),) + tuple(t.shape[1:]))])
    out["block_coords"] = torch.cat([vol["block_coords"], coords])
    out["tsdf_sum"], out["weight_sum"] = grow(vol["tsdf_sum"]), grow(vol["weight_sum"])
    out["colour_sum"] = None if vol["colour_sum"] is None else grow(vol["colour_sum"])
    return out


def lattice_index(vol):
    """[S,512,3] int64: (i, j, k) of every stored lattice point"""
    l = torch.arange(512)
    local = torch.stack([l % 8, (l // 8) % 8, l // 64], dim=1)
    return vol["block_coords"].long()[:, None, :] * 8 + local[None]


def lattice_points(vol, dtype=torch.float64):
    """[S,512,3]: origin + voxel (i, j, k), each operation in `dtype`"""
    origin = torch.tensor(vol["origin"], dtype=torch.float32).to(dtype)
    voxel = torch.tensor(vol["voxel_size"], dtype=torch.float32).to(dtype)
    return origin + voxel * lattice_index(vol).to(dtype)


def planted(vol_geometry, block_coords, field, colour_field=None, weight=1.0):
    """a volume whose blocks `block_coords` carry weight_sum = weight and tsdf_sum = weight * float32(field(p)) at every lattice
    point p [.,3] (float64); colour_field(p) -> [.,3] likewise"""
    vol = dict(vol_geometry)
    vol["block_coords"] = torch.as_tensor(block_coords, dtype=torch.int32).reshape(-1, 3)
    p = lattice_points(vol)
    S = p.shape[0]
    vol["weight_sum"] = torch.full((S, 512), float(weight))
    vol["tsdf_sum"] = (field(p.reshape(-1, 3)).float().reshape(S, 512) * float(weight)).contiguous()
    vol["colour_sum"] = None
    if colour_field is not None:
        c = colour_field(p.reshape(-1, 3)).float().reshape(S, 512, 3) * float(weight)
        vol["colour_sum"] = c.permute(0, 2, 1).contiguous()
    return vol


# ---- cameras and frames ----
def look_at_camera(position, target, W, H, tanfov=0.5):
    C, t = np.asarray(position, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (t - C) / np.linalg.norm(t - C)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([0.0, 0.0, 1.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=1)                               # columns: the camera axes in the world
    fovx = 2.0 * math.atan(tanfov)
    fovy = 2.0 * math.atan(tanfov * H / W)
    return scenes.make_camera(R, -R.T @ C, fovx, fovy, W, H)


def table(cams, dtype=torch.float64):
    """(M [n,4,4], fx, fy [n]): the float32 values the kernels read, in `dtype`; t = [p, 1] M"""
    M = torch.stack([c.world_view_transform.detach().cpu().float() for c in cams]).to(dtype)
    fx = torch.tensor([c.image_width / (2.0 * math.tan(0.5 * c.FoVx)) for c in cams], dtype=torch.float64).float().to(dtype)
    fy = torch.tensor([c.image_height / (2.0 * math.tan(0.5 * c.FoVy)) for c in cams], dtype=torch.float64).float().to(dtype)
    return M, fx, fy


def pixel_rays(cam):
    """(centre [3], directions [H,W,3]) in the world, float64: the ray of pixel (x, y) is centre + z direction, z its view depth"""
    M, fx, fy = table([cam])
    M, W, H = M[0], cam.image_width, cam.image_height
    ax = ((2.0 * torch.arange(W, dtype=torch.float64) + 1.0) / W - 1.0) * (W / (2.0 * fx[0]))
    ay = ((2.0 * torch.arange(H, dtype=torch.float64) + 1.0) / H - 1.0) * (H / (2.0 * fy[0]))
    q = torch.stack([ax[None, :].expand(H, W), ay[:, None].expand(H, W), torch.ones(H, W, dtype=torch.float64)], dim=-1)
    R, T = M[:3, :3], M[3, :3]
    return -T @ R.T, q @ R.T


def sphere_frames(cams, centre, radius, colour=True):
    """analytic z-depth of the sphere at the pixel centres, rounded to float32, 0 on the background; colour 0.5 + 0.5 sin(3 hit)"""
    depth, colours = [], []
    s = torch.tensor(centre, dtype=torch.float64)
    for cam in cams:
        c, v = pixel_rays(cam)
        oc = c - s
        a, b, cc = (v * v).sum(-1), (v * oc).sum(-1), (oc * oc).sum() - radius * radius
        disc = b * b - a * cc
        z = (-b - torch.sqrt(disc.clamp_min(0.0))) / a
        hit = (disc > 0) & (z > 0)
        depth.append(torch.where(hit, z, torch.zeros_like(z)).float())
        p = c + z[..., None] * v
        colours.append(torch.where(hit[..., None], 0.5 + 0.5 * torch.sin(3.0 * p), torch.zeros_like(p)).permute(2, 0, 1).float())
    return {"cams": list(cams), "depth": torch.stack(depth), "colour": torch.stack(colours) if colour else None, "weight": None}


SPHERE_CENTRE = (0.031, 0.017, -0.023)        # off the lattice and off its symmetry planes: see sphere_case()
SPHERE_TARGET = (0.013, -0.021, 0.008)
SPHERE_RADIUS = 0.8


def sphere_cameras(W=64, H=64, corners=True, distance=3.0):
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    if corners:
        dirs += [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    out = []
    for d in dirs:
        d = np.asarray(d, dtype=np.float64)
        out.append(look_at_camera(distance * d / np.linalg.norm(d), SPHERE_TARGET, W, H))
    return out


_SPHERE = {}


def sphere_case(corners=True):
    """(empty volume over [-4,4]^3 at voxel 1/16 with sdf_trunc = 4 voxels, frames of the 14 cameras at 64x64).  Everything is
    placed off the origin: centred, the lattice points on the diagonal symmetry planes project exactly onto the middle column
    boundary of the eight corner cameras and 10 % of the points are borderline; so placed, 0.65 %."""
    if corners not in _SPHERE:
        vol = empty_volume(1.0 / 16, 4.0 / 16, 10.0, ((-4, -4, -4), (4, 4, 4)))
        _SPHERE[corners] = (vol, sphere_frames(sphere_cameras(corners=corners), SPHERE_CENTRE, SPHERE_RADIUS))
    return _SPHERE[corners]


def small_case(n, W=32, H=32, colour=True, radius=0.5, distance=2.0, inside_camera=False):
    """(empty volume over [-1,1]^3 at voxel 1/16, sdf_trunc 4 voxels, depth_trunc 10; frames of n cameras on a spiral at
    `distance` around a sphere of `radius`) for the seam tests; inside_camera: the first camera stands inside the box at
    (-0.93, 0.05, 0.02), with lattice points of an active block behind it"""
    centre, target = (0.031, 0.017, -0.023), (0.013, -0.021, 0.008)
    cams = []
    for v in range(n):
        zc = 1.0 - 2.0 * (v + 0.5) / n
        az = 2.399963229728653 * v                                 # the golden angle
        rad = math.sqrt(max(0.0, 1.0 - zc * zc))
        cams.append(look_at_camera((distance * rad * math.cos(az), distance * rad * math.sin(az), distance * zc), target, W, H))
    if inside_camera:
        cams[0] = look_at_camera((-0.93, 0.05, 0.02), target, W, H)
    vol = empty_volume(1.0 / 16, 4.0 / 16, 10.0, ((-1, -1, -1), (1, 1, 1)), colour=colour)
    return vol, sphere_frames(cams, centre, radius, colour=colour)


def restatement_errors(active, frames, flagged, truth):
    """(float32 restatement of the integration on `active`, its largest errors against the float64 `truth` off the flagged points
    for tsdf_sum and colour_sum)"""
    r32, _ = integrate(as_float32(active), frames, dtype=torch.float32)
    ok = ~flagged
    e_t = (r32["tsdf_sum"].double() - truth["tsdf_sum"]).abs()[ok].max().item() if ok.any() else 0.0
    e_c = 0.0
    if truth["colour_sum"] is not None and ok.any():
        e_c = (r32["colour_sum"].double() - truth["colour_sum"]).abs()[ok[:, None, :].expand(-1, 3, -1)].max().item()
    return r32, e_t, e_c


# ---- activation ----
def mark_steps(vol, cams):
    """= diff_gaussian_rasterization.tsdf_mark_steps, restated"""
    _, fx, fy = table(cams)
    W = torch.tensor([float(c.image_width) for c in cams], dtype=torch.float64)
    H = torch.tensor([float(c.image_height) for c in cams], dtype=torch.float64)
    L = torch.sqrt(1.0 + (W / (2.0 * fx)) ** 2 + (H / (2.0 * fy)) ** 2).max().item()
    v, t = vol["voxel_size"], vol["sdf_trunc"]
    return max(1, int(math.ceil(2.0 * (t + 2.0 * v) * L / v)))


def activate(vol, frames):
    """(lo, hi) bool [NBz,NBy,NBx]: the blocks holding a sample of the activation walk, float64"""
    nx, ny, nz = vol["blocks"]
    lo, hi = np.zeros(nx * ny * nz, dtype=bool), np.zeros(nx * ny * nz, dtype=bool)
    cams = frames["cams"]
    if not cams:
        return lo.reshape(nz, ny, nx), hi.reshape(nz, ny, nx)
    steps = mark_steps(vol, cams)
    M, fx, fy = table(cams)
    v, r = vol["voxel_size"], vol["sdf_trunc"] + 2.0 * vol["voxel_size"]
    origin = torch.tensor(vol["origin"], dtype=torch.float64)
    nb = torch.tensor([nx, ny, nz])
    for n, cam in enumerate(cams):
        W, H = cam.image_width, cam.image_height
        d = frames["depth"][n].double()
        ok = (d > 0) & (d <= vol["depth_trunc"]) & torch.isfinite(d)
        ys, xs = torch.nonzero(ok, as_tuple=True)
        if not len(xs):
            continue
        ax = ((2.0 * xs.double() + 1.0) / W - 1.0) * (W / (2.0 * fx[n]))
        ay = ((2.0 * ys.double() + 1.0) / H - 1.0) * (H / (2.0 * fy[n]))
        z = (d[ys, xs] - r)[:, None] + torch.arange(steps + 1, dtype=torch.float64)[None, :] * (2.0 * r / steps)
        q = torch.stack([ax[:, None] * z, ay[:, None] * z, z], dim=-1) - M[n, 3, :3]
        g = ((q @ M[n, :3, :3].T - origin) / (8.0 * v)).reshape(-1, 3)[(z > 0).reshape(-1)]
        sure = ((g - torch.round(g)).abs() >= BLOCK_SLACK).all(dim=1)
        for shift in [(0, 0, 0)] + [(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]:
            b = torch.floor(g + BLOCK_SLACK * torch.tensor(shift, dtype=torch.float64)).long()
            inside = ((b >= 0) & (b < nb)).all(dim=1)
            lin = ((b[:, 2] * ny + b[:, 1]) * nx + b[:, 0])
            hi[lin[inside].numpy()] = True
            if shift == (0, 0, 0):
                lo[lin[inside & sure].numpy()] = True
    return lo.reshape(nz, ny, nx), hi.reshape(nz, ny, nx)


# ---- integration ----
def integrate(vol, frames, dtype=torch.float64):
    """(volume with the frames added to its sums, flagged [S,512] bool).  dtype=torch.float32 is the float32 RESTATEMENT: the
    operations of SPEC M20 one by one, in camera order from the stored values; the flags are only meaningful in float64."""
    cams = frames["cams"]
    M, fx, fy = table(cams, dtype)
    p = lattice_points(vol, dtype)
    S = p.shape[0]
    c = lambda x: torch.tensor(x, dtype=torch.float32).to(dtype)
    trunc, dtrunc = c(vol["sdf_trunc"]), c(vol["depth_trunc"])
    ts, ws = vol["tsdf_sum"].to(dtype).clone(), vol["weight_sum"].to(dtype).clone()
    cs = None if vol["colour_sum"] is None else vol["colour_sum"].to(dtype).clone()
    flagged = torch.zeros(S, 512, dtype=torch.bool)
    p0, p1, p2 = p[..., 0], p[..., 1], p[..., 2]
    for n, cam in enumerate(cams):
        W, H = cam.image_width, cam.image_height
        t = [((M[n, 0, k] * p0 + M[n, 1, k] * p1) + M[n, 2, k] * p2) + M[n, 3, k] for k in range(3)]
        front = t[2] > 0
        tz = torch.where(front, t[2], torch.ones_like(t[2]))
        x = (t[0] / tz) * fx[n] + c(float(W)) / c(2.0)
        y = (t[1] / tz) * fy[n] + c(float(H)) / c(2.0)
        inside = front & (x >= 0) & (x < W) & (y >= 0) & (y < H)
        px = torch.where(inside, torch.floor(x), torch.zeros_like(x)).long().clamp(0, W - 1)
        py = torch.where(inside, torch.floor(y), torch.zeros_like(y)).long().clamp(0, H - 1)
        d = frames["depth"][n].to(dtype)[py, px]
        w = torch.ones_like(d) if frames.get("weight") is None else frames["weight"][n].to(dtype)[py, px]
        sample = inside & (d > 0) & (d <= dtrunc) & torch.isfinite(d) & (w > 0) & torch.isfinite(w)
        d, w = torch.where(sample, d, torch.ones_like(d)), torch.where(sample, w, torch.zeros_like(w))
        sdf = d - t[2]
        ok = sample & ~(sdf < -trunc)
        val = torch.minimum(torch.ones_like(sdf), sdf / trunc)
        ts = torch.where(ok, ts + w * val, ts)
        ws = torch.where(ok, ws + w, ws)
        if cs is not None:
            col = frames["colour"][n].to(dtype)[:, py, px]                        # [3,S,512]
            cs = torch.where(ok[:, None, :], cs + w[:, None, :] * col.permute(1, 0, 2), cs)
        if dtype == torch.float64:
            B = 16.0 * 2.0 ** -23 * max(W, H)
            near = ((x - torch.round(x)).abs() < B) | ((y - torch.round(y)).abs() < B)
            flagged |= (t[2].abs() < 1e-5) | (front & near) | (sample & ((sdf + trunc).abs() < 1e-5 * trunc))
    out = dict(vol)
    out["tsdf_sum"], out["weight_sum"], out["colour_sum"] = ts, ws, cs
    return out, flagged


def as_float32(vol):
    out = dict(vol)
    for k in ("tsdf_sum", "weight_sum", "colour_sum"):
        out[k] = None if vol[k] is None else vol[k].float()
    return out


# ---- extraction ----
def tet_table():
    """n [16], owner / direction codes [6][16][6]: the rule of SPEC M20.  Case m (bit u: chain corner u inside) of a POSITIVE
    tetrahedron: one inside corner i, the others (j, k, l) with (i, j, k, l) even: (e_ij, e_ik, e_il); one outside corner: the
    reverse; two inside i < j, two outside (k, l) with (i, j, k, l) even: the quad (e_ik, e_il, e_jl, e_jk) split along q0 q2."""
    def parity(seq):
        return sum(1 for a in range(4) for b in range(a + 1, 4) if seq[a] > seq[b]) % 2

    n = np.zeros(16, dtype=np.int64)
    owner, direction = np.zeros((6, 16, 6), dtype=np.int64), np.zeros((6, 16, 6), dtype=np.int64)
    for q, (a, b, _) in enumerate(PERMS):
        code = (0, 1 << a, (1 << a) | (1 << b), 7)
        positive = parity(PERMS[q] + (3,)) == 0
        for m in range(16):
            ins = [u for u in range(4) if (m >> u) & 1]
            outs = [u for u in range(4) if not (m >> u) & 1]
            tris = []
            if len(ins) in (1, 3):
                i, rest = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
                j, k, l = rest
                if parity((i, j, k, l)):
                    k, l = l, k
                tris = [[(i, j), (i, k), (i, l)]] if len(ins) == 1 else [[(i, j), (i, l), (i, k)]]
            elif len(ins) == 2:
                (i, j), (k, l) = ins, outs
                if parity((i, j, k, l)):
                    k, l = l, k
                quad = [(i, k), (i, l), (j, l), (j, k)]
                tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
            n[m] = len(tris)
            for tr, tri in enumerate(tris):
                if not positive:
                    tri = [tri[0], tri[2], tri[1]]
                for v, (u0, u1) in enumerate(tri):
                    u0, u1 = min(u0, u1), max(u0, u1)
                    owner[q, m, 3 * tr + v], direction[q, m, 3 * tr + v] = code[u0], code[u1] ^ code[u0]
    return n, owner, direction


def _popcount(a):
    a = a.astype(np.int64)
    return sum((a >> b) & 1 for b in range(8))


def extract(vol, dtype=np.float64):
    """(vertices [V,3], colours [V,3] or None, faces [F,3] int64) of SPEC M20 from the stored sums, every operation in `dtype`
    (np.float32: the float32 RESTATEMENT on the identical volume).  Order: vertices by owner (slot, lattice index) and direction
    code; faces by cube (slot, lattice index), tetrahedron, triangle."""
    nx, ny, nz = vol["blocks"]
    X, Y, Z = 8 * nx + 1, 8 * ny + 1, 8 * nz + 1                  # one layer of padding at the upper ends
    coords = vol["block_coords"].long().numpy().reshape(-1, 3)
    S = len(coords)
    l = np.arange(512)
    li = np.stack([l % 8, (l // 8) % 8, l // 64], axis=1)
    idx = coords[:, None, :] * 8 + li[None]                        # [S,512,3], in key order
    pos = ((idx[..., 2] * Y + idx[..., 1]) * X + idx[..., 0]).reshape(-1)
    N = X * Y * Z
    ts, ws = np.zeros(N, dtype=dtype), np.zeros(N, dtype=dtype)
    ts[pos], ws[pos] = vol["tsdf_sum"].numpy().reshape(-1).astype(dtype), vol["weight_sum"].numpy().reshape(-1).astype(dtype)
    obs = ws > 0
    inside = obs & (ts < 0)
    T = np.where(obs, ts / np.where(obs, ws, 1), 0).astype(dtype)
    off = lambda code: (code & 1) + X * ((code >> 1) & 1) + X * Y * ((code >> 2) & 1)
    origin, voxel = np.asarray(vol["origin"], dtype=np.float32).astype(dtype), dtype(np.float32(vol["voxel_size"]))
    colour = None
    if vol["colour_sum"] is not None:
        colour = np.zeros((N, 3), dtype=dtype)
        colour[pos] = vol["colour_sum"].numpy().astype(dtype).transpose(0, 2, 1).reshape(-1, 3)
        colour = colour / np.where(obs, ws, 1)[:, None]
    # crossing masks, vertex offsets
    mask = np.zeros(N, dtype=np.int64)
    for d in range(1, 8):
        mask[pos] |= (obs[pos] & obs[pos + off(d)] & (inside[pos] != inside[pos + off(d)])).astype(np.int64) << (d - 1)
    voff = np.zeros(N, dtype=np.int64)
    counts = _popcount(mask[pos])
    voff[pos] = np.cumsum(counts) - counts
    V = int(counts.sum())
    vertices = np.zeros((V, 3), dtype=dtype)
    colours = None if colour is None else np.zeros((V, 3), dtype=dtype)
    flat_idx = idx.reshape(-1, 3)
    for d in range(1, 8):
        sel = ((mask[pos] >> (d - 1)) & 1).astype(bool)
        a, b = pos[sel], pos[sel] + off(d)
        vid = voff[a] + _popcount(mask[a] & ((1 << (d - 1)) - 1))
        t = T[a] / (T[a] - T[b])
        step = np.array([(d >> k) & 1 for k in range(3)])
        pa = origin + voxel * flat_idx[sel].astype(dtype)
        pb = origin + voxel * (flat_idx[sel] + step).astype(dtype)
        vertices[vid] = pa + t[:, None] * (pb - pa)
        if colours is not None:
            colours[vid] = colour[a] + t[:, None] * (colour[b] - colour[a])
    # faces
    n_tri, owner, direction = tet_table()
    whole = np.ones(len(pos), dtype=bool)
    cube = np.zeros(len(pos), dtype=np.int64)
    for d in range(8):
        whole &= obs[pos + off(d)]
        cube |= inside[pos + off(d)].astype(np.int64) << d
    rows, keys = [], []
    for q, (a, b, _) in enumerate(PERMS):
        c1, c2 = 1 << a, (1 << a) | (1 << b)
        m = (cube & 1) | (((cube >> c1) & 1) << 1) | (((cube >> c2) & 1) << 2) | (((cube >> 7) & 1) << 3)
        for case in range(1, 15):
            sel = np.nonzero(whole & (m == case))[0]
            if not len(sel):
                continue
            for tr in range(n_tri[case]):
                tri = []
                for v in range(3):
                    o = pos[sel] + off(owner[q, case, 3 * tr + v])
                    tri.append(voff[o] + _popcount(mask[o] & ((1 << (direction[q, case, 3 * tr + v] - 1)) - 1)))
                rows.append(np.stack(tri, axis=1))
                keys.append(np.stack([sel, np.full(len(sel), q), np.full(len(sel), tr)], axis=1))
    if not rows:
        return vertices, colours, np.zeros((0, 3), dtype=np.int64)
    rows, keys = np.concatenate(rows), np.concatenate(keys)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    return vertices, colours, rows[order]


# ---- mesh properties ----
def drop_unreferenced(vertices, faces):
    used = np.zeros(len(vertices), dtype=bool)
    used[faces.reshape(-1)] = True
    renumber = np.cumsum(used) - 1
    return vertices[used], renumber[faces]


def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def boundary_edges(faces):
    """the directed edges whose reverse is no edge of the mesh, and whether any directed edge occurs twice"""
    e = directed_edges(faces)
    base = int(e.max()) + 1 if len(e) else 1
    fwd, rev = e[:, 0] * base + e[:, 1], e[:, 1] * base + e[:, 0]
    return e[~np.isin(fwd, rev)], len(np.unique(fwd)) != len(fwd)


def euler_characteristic(faces):
    f = np.asarray(faces, dtype=np.int64)
    e = np.sort(directed_edges(f), axis=1)
    return len(np.unique(f)) - len(np.unique(e, axis=0)) + len(f)


def face_normals(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return np.cross(b - a, c - a), (a + b + c) / 3.0

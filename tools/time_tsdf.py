"""Times TSDF fusion and mesh extraction (not a test): a sphere shell of about 20 000 active blocks (voxel 1/128, radius 1.6,
sdf_trunc 4 voxels) under 64 cameras at 1920x1080, with colour.

In ONE process after a warm-up, event-timed medians of
  allocate    tsdf_allocate: msgs_tsdf_mark_blocks over the 64 depth maps
  integrate   tsdf_integrate: msgs_tsdf_integrate, all 64 cameras in one call — against the traffic floor, one read and one write
              of the pool plus the maps once, at the achievable HBM rate (the depth and colour GATHERS of a wave fall into a small
              image patch, so the maps are fetched about once; whether the kernel is bound by them or by the pool is what the
              kernel trace's FETCH_SIZE shows)
  count, emit msgs_tsdf_count and msgs_tsdf_emit alone, and tsdf_extract as a whole (two cumsum and one host read between them)
  torch       the same definition composed from torch ops on the same [S,512] lattice points, per camera (`--torch-cameras` of
              them are timed; the sum over 64 is extrapolated and said to be so)
    python tools/time_tsdf.py [--steps 10] [--warmup 3] [--cameras 64] [--width 1920] [--height 1080] [--json out.json]
For the kernels' own times and bytes trace by themselves:
    rocprofv3 --kernel-trace --stats -- python tools/time_tsdf.py --steps 3 --torch-cameras 0"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ms-gs_amd"), os.path.join(ROOT, "ms-gs_amd", "host")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import diff_gaussian_rasterization as dgr  # noqa: E402
import tsdf  # noqa: E402

HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12          # bytes/s (MI355X: measured streaming rate, specification)
CENTRE, RADIUS = (0.031, 0.017, -0.023), 1.6


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def median_ms(fn, warmup, steps):
    ts = [timed(fn)[0] for _ in range(warmup + steps)][warmup:]
    return {"ms": round(float(np.median(ts)), 4), "p10_p90": [round(float(np.percentile(ts, q)), 4) for q in (10, 90)]}


def camera(position, target, W, H, tanfovx=0.5):
    C_, t = np.asarray(position, dtype=np.float64), np.asarray(target, dtype=np.float64)
    z = (t - C_) / np.linalg.norm(t - C_)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([0.0, 0.0, 1.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=1)
    M = np.eye(4)
    M[:3, :3], M[3, :3] = R, -R.T @ C_                             # t = [p, 1] M
    return types.SimpleNamespace(world_view_transform=torch.tensor(M, dtype=torch.float32), image_width=W, image_height=H,
                                 FoVx=2.0 * math.atan(tanfovx), FoVy=2.0 * math.atan(tanfovx * H / W))


def cameras(n, W, H, distance=6.5):
    out = []
    for v in range(n):
        zc = 1.0 - 2.0 * (v + 0.5) / n
        az, rad = 2.399963229728653 * v, math.sqrt(max(0.0, 1.0 - zc * zc))
        out.append(camera((distance * rad * math.cos(az), distance * rad * math.sin(az), distance * zc), CENTRE, W, H))
    return out


def sphere_maps(cams, dev):
    """(depth [n,H,W], colour [n,3,H,W]) of the sphere, analytic, formed on the device in float64 and rounded once"""
    depth, colour = [], []
    s = torch.tensor(CENTRE, dtype=torch.float64, device=dev)
    for cam in cams:
        M = cam.world_view_transform.double().to(dev)
        W, H = cam.image_width, cam.image_height
        ax = ((2.0 * torch.arange(W, dtype=torch.float64, device=dev) + 1.0) / W - 1.0) * math.tan(0.5 * cam.FoVx)
        ay = ((2.0 * torch.arange(H, dtype=torch.float64, device=dev) + 1.0) / H - 1.0) * math.tan(0.5 * cam.FoVy)
        q = torch.stack([ax[None, :].expand(H, W), ay[:, None].expand(H, W), torch.ones(H, W, dtype=torch.float64, device=dev)], -1)
        R, T = M[:3, :3], M[3, :3]
        c, v = -T @ R.T, q @ R.T
        oc = c - s
        a, b, cc = (v * v).sum(-1), (v * oc).sum(-1), (oc * oc).sum() - RADIUS * RADIUS
        disc = b * b - a * cc
        z = (-b - torch.sqrt(disc.clamp_min(0.0))) / a
        hit = (disc > 0) & (z > 0)
        depth.append(torch.where(hit, z, torch.zeros_like(z)).float())
        p = c + z[..., None] * v
        colour.append(torch.where(hit[..., None], 0.5 + 0.5 * torch.sin(3.0 * p), torch.zeros_like(p)).permute(2, 0, 1).float())
    return torch.stack(depth), torch.stack(colour)


def torch_integrate_one(vol, points, row, depth, colour, sdf_trunc, depth_trunc):
    """one camera of SPEC M20's integration composed from torch ops on the pool's lattice points [S,512,3] (in place)"""
    M, fx, fy = row[:16].view(4, 4), row[16], row[17]
    H, W = depth.shape
    t = points @ M[:3, :3] + M[3, :3]
    tz = t[..., 2]
    front = tz > 0
    zs = torch.where(front, tz, torch.ones_like(tz))
    x, y = t[..., 0] / zs * fx + W / 2.0, t[..., 1] / zs * fy + H / 2.0
    inside = front & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    px, py = x.floor().long().clamp(0, W - 1), y.floor().long().clamp(0, H - 1)
    d = depth[py, px]
    sdf = d - tz
    ok = inside & (d > 0) & (d <= depth_trunc) & torch.isfinite(d) & ~(sdf < -sdf_trunc)
    w = ok.float()
    vol.tsdf_sum += w * torch.clamp(sdf / sdf_trunc, max=1.0).nan_to_num(0.0)
    vol.weight_sum += w
    vol.colour_sum += w[:, None, :] * colour[:, py, px].permute(1, 0, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cameras", type=int, default=64)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--voxel", type=float, default=1.0 / 128)
    ap.add_argument("--torch-cameras", type=int, default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_tsdf.py needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    cams = cameras(a.cameras, a.width, a.height)
    depth, colour = sphere_maps(cams, dev)
    vol = tsdf.TSDFVolume(a.voxel, 4 * a.voxel, depth_trunc=20.0, bounds=((-2, -2, -2), (2, 2, 2)), device=dev)
    table_host = dgr._camera_table(cams)                           # the wrappers upload it: 5 KB per call
    table = table_host.to(dev)
    out = {"cameras": a.cameras, "image": [a.width, a.height], "voxel": a.voxel, "blocks_per_axis": list(vol.blocks)}
    out["allocate"] = median_ms(lambda: dgr.tsdf_allocate(vol, depth, table_host, vol.sdf_trunc, vol.depth_trunc), a.warmup, a.steps)
    vol.integrate(depth, table_host, colour=colour)
    S = vol.num_blocks
    out["active_blocks"] = S
    out["integrate"] = median_ms(lambda: dgr.tsdf_integrate(vol, depth, table_host, vol.sdf_trunc, vol.depth_trunc, colour=colour),
                                 a.warmup, a.steps)
    pool_bytes = S * 512 * 5 * 4
    map_bytes = depth.numel() * 4 + colour.numel() * 4
    floor_bytes = 2 * pool_bytes + map_bytes
    out["integrate"].update(pool_bytes=pool_bytes, map_bytes=map_bytes, floor_bytes=floor_bytes,
                            floor_ms_at_6p3TBs=round(floor_bytes / HBM_ACHIEVABLE * 1e3, 4),
                            share_of_floor=round(floor_bytes / HBM_ACHIEVABLE * 1e3 / out["integrate"]["ms"], 4),
                            pool_only_floor_ms=round(2 * pool_bytes / HBM_ACHIEVABLE * 1e3, 4),
                            lattice_camera_pairs_per_s=round(S * 512 * a.cameras / (out["integrate"]["ms"] * 1e-3), 1))
    # count and emit alone, through the library's entry points
    v = dgr._tsdf_pool(vol, "time_tsdf")
    mask = torch.empty(S * 512, dtype=torch.uint8, device=dev)
    vcount, tcount = (torch.empty(S * 512, dtype=torch.int32, device=dev) for _ in range(2))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    count = lambda: dgr._C.check(dgr._C.lib.msgs_tsdf_count(C.byref(v), ptr(mask), ptr(vcount), ptr(tcount), stream), "count")
    out["count"] = median_ms(count, a.warmup, a.steps)
    vend, tend = torch.cumsum(vcount, 0, dtype=torch.int64), torch.cumsum(tcount, 0, dtype=torch.int64)
    V, F = int(vend[-1]), int(tend[-1])
    voff, toff = (vend - vcount).to(torch.int32), (tend - tcount).to(torch.int32)
    m = dgr._C.TsdfMesh()
    vertices, colours = torch.empty(V, 3, device=dev), torch.empty(V, 3, device=dev)
    faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    m.edge_mask, m.vertex_offset, m.triangle_offset = mask.data_ptr(), voff.data_ptr(), toff.data_ptr()
    m.n_vertices, m.n_faces = V, F
    m.vertices, m.colours, m.faces = vertices.data_ptr(), colours.data_ptr(), faces.data_ptr()
    out["emit"] = median_ms(lambda: dgr._C.check(dgr._C.lib.msgs_tsdf_emit(C.byref(v), C.byref(m), stream), "emit"), a.warmup, a.steps)
    out["extract"] = median_ms(lambda: dgr.tsdf_extract(vol), a.warmup, a.steps)
    out["extract"].update(vertices=V, faces=F)
    out["count"].update(floor_bytes=S * 512 * 17, share_of_floor=round(S * 512 * 17 / HBM_ACHIEVABLE * 1e3 / out["count"]["ms"], 4))
    emit_bytes = S * 512 * 17 + V * 24 + F * 12
    out["emit"].update(floor_bytes=emit_bytes, share_of_floor=round(emit_bytes / HBM_ACHIEVABLE * 1e3 / out["emit"]["ms"], 4))
    if a.torch_cameras > 0:
        l = torch.arange(512, device=dev)
        local = torch.stack([l % 8, (l // 8) % 8, l // 64], dim=1)
        b = vol.slot_block.long()
        nx, ny = vol.blocks[0], vol.blocks[1]
        coords = torch.stack([b % nx, (b // nx) % ny, b // (nx * ny)], dim=1)
        points = torch.tensor(vol.origin, device=dev) + vol.voxel_size * (coords[:, None, :] * 8 + local[None]).float()
        k = min(a.torch_cameras, a.cameras)

        def torch_cameras():
            for n in range(k):
                torch_integrate_one(vol, points, table[n], depth[n], colour[n], vol.sdf_trunc, vol.depth_trunc)
        t = median_ms(torch_cameras, 1, max(3, a.steps // 2))
        out["torch"] = {"cameras_timed": k, "ms_per_camera": round(t["ms"] / k, 4),
                        "ms_for_all_cameras_extrapolated": round(t["ms"] / k * a.cameras, 3),
                        "kernel_is_faster_by": round(t["ms"] / k * a.cameras / out["integrate"]["ms"], 2)}
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

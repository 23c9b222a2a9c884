"""Times mesh clean-up (not a test) on the shell of tools/time_tsdf.py — the sphere of radius 1.6 at voxel 1/128 fused from 64 views
and extracted: about 2.37 M vertices and 4.74 M faces — with `--floaters` small closed spheres of 80 faces each planted around it.

In ONE process after a warm-up, event-timed medians of
  clusters      mesh_triangle_clusters: key kernel, torch.sort, gather, union-find (identity, link, flatten), cumsum, bincount
  post_process  post_process_mesh with 2DGS's defaults (50 clusters, 50 triangles), which drops most floaters
  parts         msgs_mesh_corner_keys, torch.sort of the keys, the gather of the face ids, msgs_mesh_link_sorted (its three
                launches), msgs_mesh_edge_report, each alone; and a device copy of the keys' size as the session's streaming rate
  host          what a user does today: faces to the host, numpy edge keys, scipy.sparse.csgraph.connected_components, mask and
                renumber in numpy — wall clock, on the same mesh; the two results are compared
    python tools/time_mesh.py [--steps 10] [--warmup 3] [--floaters 300] [--json out.json]
For the kernels' own times trace by themselves:
    rocprofv3 --kernel-trace --stats -- python tools/time_mesh.py --steps 3 --warmup 1 --no-host"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ms-gs_amd"), os.path.join(ROOT, "ms-gs_amd", "host"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import diff_gaussian_rasterization as dgr  # noqa: E402
import mesh  # noqa: E402
import tsdf  # noqa: E402
from time_tsdf import HBM_ACHIEVABLE, cameras, median_ms, sphere_maps  # noqa: E402


def uv_sphere(rings=6, segments=8):
    """(vertices [2 + (rings-1) segments, 3], faces [2 segments (rings-1), 3]) of a closed unit sphere"""
    th = np.pi * np.arange(1, rings) / rings
    ph = 2.0 * np.pi * np.arange(segments) / segments
    ring = np.stack([np.sin(th)[:, None] * np.cos(ph), np.sin(th)[:, None] * np.sin(ph), np.cos(th)[:, None] * np.ones(segments)], -1)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring.reshape(-1, 3), [[0.0, 0.0, -1.0]]])
    at = lambda r, s: 1 + r * segments + s % segments
    f = []
    for s in range(segments):
        f.append((0, at(0, s), at(0, s + 1)))
        f.append((len(v) - 1, at(rings - 2, s + 1), at(rings - 2, s)))
        for r in range(rings - 2):
            f += [(at(r, s), at(r + 1, s), at(r + 1, s + 1)), (at(r, s), at(r + 1, s + 1), at(r, s + 1))]
    return v, np.array(f)


def with_floaters(v, c, f, n, seed=7):
    """n closed spheres of 36, 80 or 140 faces (a third each) around the shell: under 2DGS's defaults the 36s fall under the floor
    of 50 triangles and the 80s under the 50th largest count"""
    g = np.random.default_rng(seed)
    kinds = [uv_sphere(4, 6), uv_sphere(6, 8), uv_sphere(8, 10)]
    centres = g.standard_normal((n, 3))
    centres = centres / np.linalg.norm(centres, axis=1, keepdims=True) * g.uniform(1.75, 1.95, (n, 1))
    fv, ff, base = [], [], len(v)
    for i in range(n):
        sv, sf = kinds[i % 3]
        fv.append(centres[i] + 0.01 * sv)
        ff.append(sf + base)
        base += len(sv)
    fv, ff = np.concatenate(fv) if n else np.zeros((0, 3)), np.concatenate(ff) if n else np.zeros((0, 3), dtype=np.int64)
    dev = v.device
    v = torch.cat([v, torch.tensor(fv, dtype=torch.float32, device=dev)])
    c = torch.cat([c, torch.full((len(fv), 3), 0.5, device=dev)])
    f = torch.cat([f, torch.tensor(ff, dtype=torch.int32, device=dev)])
    return v, c, f[torch.randperm(len(f), generator=torch.Generator().manual_seed(seed)).to(dev)]       # no order to lean on


def host_clean_up(v, c, f, cluster_to_keep=50, min_triangles=50):
    """today's way: everything on the host"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    t0 = time.perf_counter()
    vn, cn, fn = v.cpu().numpy(), c.cpu().numpy(), f.cpu().numpy().astype(np.int64)
    t1 = time.perf_counter()
    F = len(fn)
    lo, hi = np.minimum(fn, np.roll(fn, -1, 1)), np.maximum(fn, np.roll(fn, -1, 1))
    keys = ((lo << 32) | hi).reshape(-1)
    order = np.argsort(keys, kind="stable")
    ks, face = keys[order], order // 3
    same = ks[1:] == ks[:-1]
    a, b = face[:-1][same], face[1:][same]
    k, comp = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(F, F)), directed=False)
    counts = np.bincount(comp, minlength=k)
    t2 = time.perf_counter()
    threshold = max(min_triangles, np.sort(counts)[-cluster_to_keep] if k > cluster_to_keep else 0)
    keep = (counts >= threshold)[comp] & (fn[:, 0] != fn[:, 1]) & (fn[:, 1] != fn[:, 2]) & (fn[:, 2] != fn[:, 0])
    fk = fn[keep]
    used = np.zeros(len(vn), dtype=bool)
    used[fk.reshape(-1)] = True
    out = vn[used], cn[used], (np.cumsum(used) - 1)[fk]
    t3 = time.perf_counter()
    ms = lambda x: round(1e3 * x, 1)
    return out, np.sort(counts), {"copy_ms": ms(t1 - t0), "components_ms": ms(t2 - t1), "mask_renumber_ms": ms(t3 - t2),
                                  "total_ms": ms(t3 - t0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--floaters", type=int, default=300)
    ap.add_argument("--voxel", type=float, default=1.0 / 128)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_mesh.py needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    cams = cameras(64, 1920, 1080)
    depth, colour = sphere_maps(cams, dev)
    vol = tsdf.TSDFVolume(a.voxel, 4 * a.voxel, depth_trunc=20.0, bounds=((-2, -2, -2), (2, 2, 2)), device=dev)
    vol.integrate(depth, dgr._camera_table(cams), colour=colour)
    v, c, f = vol.extract_mesh()
    del depth, colour, vol
    out = {"shell": {"vertices": len(v), "faces": len(f)}, "floaters": a.floaters}
    v, c, f = with_floaters(v, c, f, a.floaters)
    V, F = len(v), len(f)
    out["mesh"] = {"vertices": V, "faces": F}
    out["clusters"] = median_ms(lambda: dgr.mesh_triangle_clusters(f, V), a.warmup, a.steps)
    out["post_process"] = median_ms(lambda: mesh.post_process_mesh(v, c, f), a.warmup, a.steps)
    clusters, counts = dgr.mesh_triangle_clusters(f, V)
    v2, c2, f2 = mesh.post_process_mesh(v, c, f)
    out["clusters"].update(K=len(counts), largest=int(counts.max()))
    out["post_process"].update(vertices=len(v2), faces=len(f2), edge_report=list(mesh.edge_report(f2, len(v2))))
    # the parts, through the library's entry points
    lib, ptr = dgr._C.lib, lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    keys = torch.empty(3 * F, dtype=torch.int64, device=dev)
    face_of_key = torch.empty(3 * F, dtype=torch.int32, device=dev)
    parent, label = (torch.empty(F, dtype=torch.int32, device=dev) for _ in range(2))
    counts3 = torch.empty(3, dtype=torch.int64, device=dev)
    check = dgr._C.check
    parts = {}
    parts["corner_keys"] = median_ms(lambda: check(lib.msgs_mesh_corner_keys(F, ptr(f), 0, ptr(keys), ptr(face_of_key), stream),
                                                   "keys"), a.warmup, a.steps)
    parts["torch_sort"] = median_ms(lambda: torch.sort(keys), a.warmup, a.steps)
    ks, order = torch.sort(keys)
    parts["gather"] = median_ms(lambda: face_of_key[order], a.warmup, a.steps)
    fs = face_of_key[order]
    parts["link_sorted"] = median_ms(lambda: check(lib.msgs_mesh_link_sorted(F, 3 * F, ptr(ks), ptr(fs), ptr(parent), ptr(label),
                                                                            stream), "link"), a.warmup, a.steps)
    parts["rank_and_count"] = median_ms(lambda: torch.bincount((torch.cumsum(label == torch.arange(F, dtype=torch.int32, device=dev),
                                                                             0, dtype=torch.int32) - 1)[label.long()]),
                                        a.warmup, a.steps)
    parts["edge_report"] = median_ms(lambda: check(lib.msgs_mesh_edge_report(3 * F, ptr(ks), ptr(counts3), stream), "report"),
                                     a.warmup, a.steps)
    copy_to = torch.empty_like(keys)
    parts["copy_of_the_keys"] = median_ms(lambda: copy_to.copy_(keys), a.warmup, a.steps)
    parts["copy_of_the_keys"].update(bytes=2 * keys.numel() * 8,
                                     TB_per_s=round(2 * keys.numel() * 8 / (parts["copy_of_the_keys"]["ms"] * 1e-3) / 1e12, 3))
    key_bytes = 3 * F * (4 + 8 + 4)                               # one index read, one key and one face id written per corner
    parts["corner_keys"].update(bytes=key_bytes, TB_per_s=round(key_bytes / (parts["corner_keys"]["ms"] * 1e-3) / 1e12, 3),
                                share_of_6p3TBs=round(key_bytes / HBM_ACHIEVABLE * 1e3 / parts["corner_keys"]["ms"], 4))
    for k in ("torch_sort", "link_sorted"):
        parts[k]["share_of_clusters"] = round(parts[k]["ms"] / out["clusters"]["ms"], 4)
    out["parts"] = parts
    if not a.no_host:
        (hv, hc, hf), host_counts, out["host"] = host_clean_up(v, c, f)
        out["host"]["same_result"] = bool(np.array_equal(np.sort(counts.cpu().numpy()), host_counts) and
                                          np.array_equal(hf, f2.cpu().numpy()) and np.array_equal(hv, v2.cpu().numpy()) and
                                          np.array_equal(hc, c2.cpu().numpy()))
        out["host"]["post_process_is_faster_by"] = round(out["host"]["total_ms"] / out["post_process"]["ms"], 1)
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

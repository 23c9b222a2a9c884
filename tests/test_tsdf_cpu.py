"""TSDF fusion and mesh extraction without a GPU (SPEC M20; 4.22): the float64 truth of tests/tsdf_truth.py against
analysis (planted plane and sphere fields, the fused sphere case of the GPU tests), the float32 restatement's incremental
property, the wrappers' validation and the mesh PLY writer.  Nothing in this file reaches a kernel."""
import math
import os

import numpy as np
import pytest
import torch

import tsdf                        # host/tsdf.py: the feature under test (with it, diff_gaussian_rasterization's tsdf_* wrappers)
import tsdf_truth as tt
from model_io import read_ply, write_mesh_ply

VOXEL = 1.0 / 16


def _all_blocks(blocks):
    nx, ny, nz = blocks
    return [(x, y, z) for z in range(nz) for y in range(ny) for x in range(nx)]


def _box(half):
    return tt.empty_volume(VOXEL, 4 * VOXEL, 10.0, ((-half,) * 3, (half,) * 3))


def _sphere_field(centre, radius=tt.SPHERE_RADIUS):
    c = torch.tensor(centre, dtype=torch.float64)
    return lambda p: (p - c).norm(dim=1) - radius


def _closed_sphere_checks(vertices, faces, centre):
    v, f = tt.drop_unreferenced(vertices, faces)
    assert len(v) == len(vertices)                                 # every crossing edge of a fully observed field is used
    open_edges, doubled = tt.boundary_edges(f)
    assert len(open_edges) == 0 and not doubled                   # every undirected edge: two faces, once in each direction
    assert tt.euler_characteristic(f) == 2
    normal, centroid = tt.face_normals(v, f)
    assert ((normal * (centroid - np.asarray(centre))).sum(axis=1) > 0).all()
    return v, f


def test_tet_table_is_the_rule():
    n, owner, direction = tt.tet_table()
    assert n.tolist() == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
    for q in range(6):
        for m in range(16):
            for v in range(3 * n[m]):
                o, d = owner[q, m, v], direction[q, m, v]
                assert 1 <= d <= 7 and o & d == 0                 # the owner is the lower end
                chain = (0, 1 << tt.PERMS[q][0], (1 << tt.PERMS[q][0]) | (1 << tt.PERMS[q][1]), 7)
                u0, u1 = chain.index(o), chain.index(o | d)
                assert ((m >> u0) & 1) != ((m >> u1) & 1)         # a crossing edge of this case


def test_plane_field_gives_vertices_on_the_plane():
    # n . p - c with dyadic n and c: every lattice value is exact in float32 and none is 0
    normal, c = torch.tensor([0.5, 0.25, 1.0], dtype=torch.float64), 0.1015625 + 1.0 / 256
    geometry = _box(0.5)
    assert geometry["blocks"] == (2, 2, 2)
    colour = lambda p: torch.stack([0.5 + 0.25 * p[:, 0], 0.5 - 0.25 * p[:, 1], 0.5 + 0.125 * p[:, 2]], dim=1)
    vol = tt.planted(geometry, _all_blocks(geometry["blocks"]), lambda p: p @ normal - c, colour)
    assert (vol["tsdf_sum"] != 0).all()
    v, col, f = tt.extract(vol)
    assert len(f) > 100
    assert np.abs(v @ normal.numpy() - c).max() < 1e-12
    assert np.abs(col - colour(torch.tensor(v)).numpy()).max() < 1e-12           # a linear colour is interpolated exactly
    nrm, _ = tt.face_normals(v, f)
    assert (nrm @ normal.numpy() > 0).all()                       # towards positive TSDF
    # a weight other than 1 changes the sums, not the mesh
    v2, _, f2 = tt.extract(tt.planted(geometry, _all_blocks(geometry["blocks"]), lambda p: p @ normal - c, colour, weight=4.0))
    assert np.array_equal(f, f2) and np.abs(v - v2).max() < 1e-12


@pytest.mark.parametrize("centre", [tt.SPHERE_CENTRE, "corner"])
def test_sphere_field_is_closed_oriented_and_a_sphere(centre):
    geometry = _box(1.0)
    assert geometry["blocks"] == (4, 4, 4)
    if centre == "corner":
        # the surface passes through the cube whose highest corner is the block corner (0.5, 0.5, 0.5): it reads eight blocks
        centre = tuple(0.5 - 0.5 * VOXEL - tt.SPHERE_RADIUS / math.sqrt(3.0) + e for e in (0.004, -0.003, 0.002))
        field = _sphere_field(centre)
        k = 8 * 3 - 1                                              # the lattice index of the cube's lowest corner on every axis
        corners = torch.tensor([[-1.0 + VOXEL * (k + dx), -1.0 + VOXEL * (k + dy), -1.0 + VOXEL * (k + dz)]
                                for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)], dtype=torch.float64)
        signs = field(corners) < 0
        assert signs.any() and not signs.all()
    vol = tt.planted(geometry, _all_blocks(geometry["blocks"]), _sphere_field(centre))
    vertices, _, faces = tt.extract(vol)
    v, f = _closed_sphere_checks(vertices, faces, centre)
    r = np.linalg.norm(v - np.asarray(centre), axis=1)
    assert np.abs(r - tt.SPHERE_RADIUS).max() < 0.5 * VOXEL * VOXEL / tt.SPHERE_RADIUS + 1e-6    # linear interpolation of a distance


def test_a_missing_block_opens_the_mesh_along_its_rim_only():
    geometry = _box(1.0)
    blocks = _all_blocks(geometry["blocks"])
    gone = (3, 2, 1)                                               # the sphere crosses it: |(0.5..0.75, 0.25..0.5, -0.5..-0.25)|
    full = tt.planted(geometry, blocks, _sphere_field(tt.SPHERE_CENTRE))
    part = tt.planted(geometry, [b for b in blocks if b != gone], _sphere_field(tt.SPHERE_CENTRE))
    vf, _, ff = tt.extract(full)
    vp, _, fp = tt.extract(part)
    open_edges, doubled = tt.boundary_edges(fp)
    assert len(open_edges) > 0 and not doubled
    # the cubes that read the block span the lattice indices 8 b - 1 .. 8 b + 8 on every axis
    lo = np.array([-1.0 + VOXEL * (8 * b - 1) for b in gone])
    hi = np.array([-1.0 + VOXEL * (8 * b + 8) for b in gone])
    rim = vp[np.unique(open_edges)]
    assert ((rim >= lo - 1e-12) & (rim <= hi + 1e-12)).all()
    assert (np.minimum(np.abs(rim - lo), np.abs(rim - hi)).min(axis=1) < 1e-12).all()
    # ... and the rest is the full mesh without the faces inside that box
    centroid = lambda v, f: v[f].mean(axis=1)
    cf = centroid(vf, ff)
    outside = ~((cf > lo) & (cf < hi)).all(axis=1)
    assert len(fp) == int(outside.sum()) < len(ff)
    assert np.abs(np.sort(centroid(vp, fp), axis=0) - np.sort(cf[outside], axis=0)).max() < 1e-12


# ---- the fused sphere case of the GPU tests ----
@pytest.fixture(scope="module")
def fused():
    vol, frames = tt.sphere_case()
    lo, hi = tt.activate(vol, frames)
    active = tt.with_blocks(vol, lo)
    truth, flagged = tt.integrate(active, frames)
    return dict(vol=vol, frames=frames, lo=lo, hi=hi, active=active, truth=truth, flagged=flagged)


def _crossing_cubes(vol, centre):
    """(lowest corners [C,3] of the cubes the analytic sphere crosses, the stored observed flag as a dense array)"""
    nx, ny, nz = vol["blocks"]
    g = [np.arange(8 * n) for n in (nx, ny, nz)]
    P = np.stack(np.meshgrid(*g, indexing="ij"), axis=-1).astype(np.float64) * vol["voxel_size"] + np.asarray(vol["origin"])
    inside = np.linalg.norm(P - np.asarray(centre), axis=-1) < tt.SPHERE_RADIUS
    sh = lambda a, d: a[d[0]:a.shape[0] - 1 + d[0], d[1]:a.shape[1] - 1 + d[1], d[2]:a.shape[2] - 1 + d[2]]
    corners = [(dx, dy, dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]
    n_in = sum(sh(inside, d).astype(int) for d in corners)
    observed = np.zeros(inside.shape, dtype=bool)
    idx = tt.lattice_index(vol).numpy().reshape(-1, 3)
    observed[idx[:, 0], idx[:, 1], idx[:, 2]] = (vol["weight_sum"].numpy() > 0).reshape(-1)
    whole = np.all([sh(observed, d) for d in corners], axis=0)
    crossing = (n_in > 0) & (n_in < 8)
    return int(crossing.sum()), int((crossing & ~whole).sum())


def test_sphere_case_activation_has_no_borderline_block(fused):
    assert np.array_equal(fused["lo"], fused["hi"])
    n = int(fused["lo"].sum())
    print(f"[tsdf] sphere case: {n} active blocks of {fused['lo'].size}")
    assert n == 88                                                 # measured here; profiles/tsdf_notes.md


def test_sphere_case_truth(fused):
    truth, flagged = fused["truth"], fused["flagged"]
    share = flagged.float().mean().item()
    print(f"[tsdf] sphere case: borderline share {share:.4%} of {flagged.numel()} lattice points")
    assert share < tt.MAX_BORDERLINE
    # unit weights: the weight sums are whole numbers
    assert torch.equal(truth["weight_sum"], truth["weight_sum"].round()) and truth["weight_sum"].max() <= 14
    crossing, incomplete = _crossing_cubes(truth, tt.SPHERE_CENTRE)
    print(f"[tsdf] sphere case: {crossing} crossing cubes, {incomplete} incomplete")
    # measured here (the case was proposed with 3276 under other camera rolls; the property is the second figure);
    # observed implies stored, so every corner of these cubes lies in an active block
    assert crossing == 3094 and incomplete == 0
    # the six axis cameras alone leave crossing cubes with an unobserved corner: that is why the case has fourteen
    vol6, frames6 = tt.sphere_case(corners=False)
    truth6, _ = tt.integrate(tt.with_blocks(vol6, tt.activate(vol6, frames6)[0]), frames6)
    crossing6, incomplete6 = _crossing_cubes(truth6, tt.SPHERE_CENTRE)
    print(f"[tsdf] six axis cameras: {crossing6} crossing cubes, {incomplete6} incomplete")
    assert crossing6 == crossing and incomplete6 > 0


# the largest radial deviation of the float64 truth mesh of the sphere case from the sphere, measured here (profiles/tsdf_notes.md):
# the bias of a projective TSDF (d - t.z is measured along the view axis, not along the normal), not kernel error
SPHERE_CASE_RADIAL_DEVIATION = 4.399735e-02   # 0.704 voxels, at the silhouettes of the corner cameras


def test_sphere_case_truth_mesh(fused):
    vertices, colours, faces = tt.extract(fused["truth"])
    v, f = tt.drop_unreferenced(vertices, faces)
    open_edges, doubled = tt.boundary_edges(f)
    assert len(open_edges) == 0 and not doubled and tt.euler_characteristic(f) == 2
    normal, centroid = tt.face_normals(v, f)
    assert ((normal * (centroid - np.asarray(tt.SPHERE_CENTRE))).sum(axis=1) > 0).all()
    dev = np.abs(np.linalg.norm(v - np.asarray(tt.SPHERE_CENTRE), axis=1) - tt.SPHERE_RADIUS).max()
    print(f"[tsdf] sphere case: {len(v)} vertices, {len(f)} faces, max radial deviation {dev:.6e} = {dev / VOXEL:.4f} voxels")
    assert dev <= SPHERE_CASE_RADIAL_DEVIATION * (1 + 1e-6)
    assert np.isfinite(colours).all() and colours.min() >= 0 and colours.max() <= 1


def test_restatement_error_is_recorded(fused):
    """the float32 restatement's own error against float64 on the sphere case, off the flagged points: the scale of the GPU
    test's tolerances (tests/test_tsdf_gpu.py carries the figures measured here)"""
    r32, _ = tt.integrate(tt.as_float32(fused["active"]), fused["frames"], dtype=torch.float32)
    ok = ~fused["flagged"]
    assert torch.equal(r32["weight_sum"][ok].double(), fused["truth"]["weight_sum"][ok])
    e_t = (r32["tsdf_sum"].double() - fused["truth"]["tsdf_sum"]).abs()[ok].max().item()
    e_c = (r32["colour_sum"].double() - fused["truth"]["colour_sum"]).abs()[ok[:, None, :].expand(-1, 3, -1)].max().item()
    v64, c64, f64 = tt.extract(tt.as_float32(r32))
    v32, c32, f32 = tt.extract(tt.as_float32(r32), dtype=np.float32)
    assert np.array_equal(f64, f32)
    e_v, e_col = np.abs(v32.astype(np.float64) - v64).max(), np.abs(c32.astype(np.float64) - c64).max()
    print(f"[tsdf] restatement errors: tsdf_sum {e_t:.3e} colour_sum {e_c:.3e} vertices {e_v:.3e} colours {e_col:.3e}")
    assert 0 < e_t < 1e-4 and 0 < e_c < 1e-4 and 0 < e_v < 1e-5 and 0 < e_col < 1e-4


def test_incremental_integration_leaves_the_same_bits(fused):
    frames, active = fused["frames"], tt.as_float32(fused["active"])
    part = lambda a, b: {"cams": frames["cams"][a:b], "depth": frames["depth"][a:b], "colour": frames["colour"][a:b],
                         "weight": None}
    whole, _ = tt.integrate(active, frames, dtype=torch.float32)
    step, _ = tt.integrate(active, part(0, 5), dtype=torch.float32)
    step, _ = tt.integrate(step, part(5, 14), dtype=torch.float32)
    for k in ("tsdf_sum", "weight_sum", "colour_sum"):
        assert whole[k].dtype == torch.float32 and torch.equal(whole[k].view(torch.int32), step[k].view(torch.int32)), k


# ---- the wrappers refuse before any library call ----
class _Volume:
    def __init__(self, blocks=(2, 2, 2), S=3, colour=True):
        self.origin, self.voxel_size, self.blocks = (0.0, 0.0, 0.0), VOXEL, blocks
        self.table = torch.full(blocks[::-1], -1, dtype=torch.int32)
        self.slot_block = torch.zeros(S, dtype=torch.int32)
        self.tsdf_sum, self.weight_sum = torch.zeros(S, 512), torch.zeros(S, 512)
        self.colour_sum = torch.zeros(S, 3, 512) if colour else None


def test_wrappers_validate_before_any_call(monkeypatch):
    import diff_gaussian_rasterization as dgr
    calls = []
    monkeypatch.setattr(dgr, "_tsdf_probe", calls.append)
    cams = tt.sphere_cameras(W=8, H=6)[:2]
    depth, colour = torch.ones(2, 6, 8), torch.ones(2, 3, 6, 8)
    vol = _Volume()
    args = lambda **kw: dict(dict(volume=vol, depth=depth, cameras=cams, sdf_trunc=0.25, depth_trunc=5.0, colour=colour), **kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.tsdf_integrate(**args())
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.tsdf_allocate(vol, depth, cams, 0.25, 5.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.tsdf_extract(vol)
    with pytest.raises(ValueError, match="float32"):
        dgr.tsdf_integrate(**args(depth=depth.double()))
    with pytest.raises(ValueError, match="float32"):
        dgr.tsdf_integrate(**args(colour=colour.half()))
    with pytest.raises(ValueError, match="not differentiable"):
        dgr.tsdf_integrate(**args(depth=depth.clone().requires_grad_(True)))
    with pytest.raises(ValueError, match="not differentiable"):
        dgr.tsdf_integrate(**args(weight=torch.ones(2, 6, 8, requires_grad=True)))
    with pytest.raises(ValueError, match="size of the depth maps"):
        dgr.tsdf_integrate(**args(depth=torch.ones(2, 6, 9), colour=torch.ones(2, 3, 6, 9)))
    with pytest.raises(ValueError, match="size of the depth maps"):
        dgr.tsdf_integrate(**args(cameras=[cams[0], tt.sphere_cameras(W=8, H=7)[0]]))
    with pytest.raises(ValueError, match="cameras for"):
        dgr.tsdf_integrate(**args(cameras=cams[:1]))
    with pytest.raises(ValueError, match=r"\[n,H,W\]"):
        dgr.tsdf_integrate(**args(depth=depth[0]))
    with pytest.raises(ValueError, match="colour must be"):
        dgr.tsdf_integrate(**args(colour=colour[:, :2]))
    with pytest.raises(ValueError, match="weight must be"):
        dgr.tsdf_integrate(**args(weight=torch.ones(2, 6, 7)))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sdf_trunc"):
            dgr.tsdf_integrate(**args(sdf_trunc=bad))
    with pytest.raises(ValueError, match="depth_trunc"):
        dgr.tsdf_integrate(**args(depth_trunc=0.0))
    with pytest.raises(ValueError, match="per axis"):
        dgr.tsdf_integrate(**args(volume=_Volume(blocks=(2, 257, 2))))
    with pytest.raises(ValueError, match="table"):
        v = _Volume()
        v.table = v.table.long()
        dgr.tsdf_integrate(**args(volume=v))
    with pytest.raises(ValueError, match="weight_sum"):
        v = _Volume()
        v.weight_sum = torch.zeros(2, 512)
        dgr.tsdf_extract(v)
    assert calls == []


def test_constants_mirror_the_header():
    import re
    import diff_gaussian_rasterization as dgr
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msgs.h")).read()
    value = lambda name: eval(re.search(rf"#define {name} (\(?[0-9 <]+\)?)", src).group(1))
    assert dgr.TSDF_CAMERA_CHUNK == value("MSGS_TSDF_CAMERA_CHUNK") == 64
    assert dgr.TSDF_MAX_BLOCKS_PER_AXIS == value("MSGS_TSDF_MAX_BLOCKS_PER_AXIS") == 256
    assert dgr.TSDF_MAX_SLOTS == value("MSGS_TSDF_MAX_SLOTS") == 1 << 22
    import ctypes as C
    assert C.sizeof(dgr._C.TsdfVolume) == 72 and C.sizeof(dgr._C.TsdfFrames) == 56 and C.sizeof(dgr._C.TsdfMesh) == 56
    assert dgr._C.TsdfVolume.table.offset == 32 and dgr._C.TsdfFrames.cameras.offset == 16 and dgr._C.TsdfMesh.vertices.offset == 32
    # the table limit is what the volume refuses at
    with pytest.raises(ValueError, match="pool slots"):
        dgr.tsdf_extract(_big_pool())


def _big_pool():
    v = _Volume(S=0)
    v.slot_block = torch.zeros((1 << 22) + 1, dtype=torch.int32)
    return v


def test_volume_refuses_bad_geometry():
    with pytest.raises(ValueError, match="at most 256 per axis"):
        tsdf.TSDFVolume(VOXEL, depth_trunc=5.0, bounds=((-64.1, -1, -1), (64.1, 1, 1)), device="cpu")
    tsdf.volume_geometry(VOXEL, ((-64, -1, -1), (64, 1, 1)))       # exactly 256 blocks
    for kw in (dict(voxel_size=0.0), dict(voxel_size=VOXEL, sdf_trunc=0.0), dict(voxel_size=VOXEL, sdf_trunc=-1.0),
               dict(voxel_size=VOXEL, depth_trunc=0.0), dict(voxel_size=VOXEL, bounds=((0, 0, 0), (1, 0, 1)))):
        full = dict(dict(depth_trunc=5.0, bounds=((-1, -1, -1), (1, 1, 1)), device="cpu"), **kw)
        with pytest.raises(ValueError):
            tsdf.TSDFVolume(**full)
    vol = tsdf.TSDFVolume(VOXEL, depth_trunc=5.0, bounds=((-1, -1, -1), (1, 1, 1)), device="cpu")
    assert vol.sdf_trunc == float(np.float32(5 * np.float32(VOXEL))) and vol.blocks == (4, 4, 4) and vol.num_blocks == 0
    with pytest.raises(RuntimeError, match="no CPU path"):
        vol.integrate(torch.ones(1, 6, 8), tt.sphere_cameras(W=8, H=6)[:1], colour=torch.ones(1, 3, 6, 8))
    # state_dict round trip of a planted field, on the host
    planted = tt.planted(_box(1.0), [(3, 2, 1), (0, 0, 0)], _sphere_field(tt.SPHERE_CENTRE))
    state = vol.load_state_dict(planted).state_dict()
    assert torch.equal(state["block_coords"], planted["block_coords"]) and torch.equal(state["tsdf_sum"], planted["tsdf_sum"])
    assert state["colour_sum"] is None and state["blocks"] == (4, 4, 4)
    assert vol.table[1, 2, 3] == 0 and vol.table[0, 0, 0] == 1 and int((vol.table >= 0).sum()) == 2
    with pytest.raises(ValueError, match="twice"):
        vol.load_state_dict(dict(planted, block_coords=torch.tensor([[1, 1, 1], [1, 1, 1]])))


def test_write_mesh_ply_byte_for_byte(tmp_path):
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.5], [0.0, 1.0, -0.25], [1.5, 1.0, 2.0]])
    f = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    c = torch.tensor([[0.0, 0.5, 1.0], [1.2, -0.1, 0.25], [0.1, 0.2, 0.3], [1.0, 1.0, 0.0]])
    path = os.path.join(tmp_path, "mesh.ply")
    write_mesh_ply(path, v, f, c)
    raw = open(path, "rb").read()
    header = (b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
              b"property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 2\n"
              b"property list uchar int vertex_indices\nend_header\n")
    assert raw.startswith(header) and len(raw) == len(header) + 4 * 15 + 2 * 13
    vt = np.dtype([("xyz", "<f4", (3,)), ("rgb", "u1", (3,))])
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert vt.itemsize == 15 and ft.itemsize == 13
    vr = np.frombuffer(raw, dtype=vt, count=4, offset=len(header))
    fr = np.frombuffer(raw, dtype=ft, count=2, offset=len(header) + 60)
    assert np.array_equal(vr["xyz"], v.numpy()) and (fr["n"] == 3).all() and np.array_equal(fr["v"], f.numpy())
    assert vr["rgb"][0].tolist() == [0, 128, 255] and vr["rgb"][1].tolist() == [255, 0, 64] and vr["rgb"][3].tolist() == [255, 255, 0]
    assert fr["v"][-1].tolist() == [2, 1, 3]
    back = read_ply(path)                                          # the vertex element reads back
    assert len(back) == 4 and back["x"][3] == 1.5 and back["blue"][0] == 255
    # without colours: x y z only
    write_mesh_ply(path, v.numpy(), f.numpy())
    raw = open(path, "rb").read()
    assert b"red" not in raw[:200] and raw.endswith(np.array([3], "u1").tobytes() + np.array([2, 1, 3], "<i4").tobytes())
    assert len(raw) == raw.index(b"end_header\n") + 11 + 4 * 12 + 2 * 13

"""TSDF fusion and mesh extraction on the GPU (SPEC M20; 4.22) against tests/tsdf_truth.py.

Integration is compared with the float64 truth off the lattice points the truth flags as borderline (at most MAX_BORDERLINE of
them): the active block set lies between the truth's certain and possible sets (equal on the sphere case, where they are the
same set: tests/test_tsdf_cpu.py), weight_sum has the bits of the float32 restatement, and tsdf_sum / colour_sum lie within
TOLERANCE_FACTOR x the float32 restatement's own largest error against float64 — the factor covers FMA contraction and another
order of the three products, not a different algorithm.  Extraction is compared with the numpy restatement on the IDENTICAL
float32 volume read back through state_dict: faces as integers (classification is on the sign of a stored sum, there is no
borderline), vertices and colours within the same factor of the restatement's error against float64 arithmetic on that volume.

Restatement errors of the sphere case, measured on the CPU by tests/test_tsdf_cpu.py::test_restatement_error_is_recorded
(x86-64, torch float32 against float64, recorded in profiles/tsdf_notes.md):
    tsdf_sum 2.395e-06   colour_sum 7.153e-07   vertices 3.405e-08   colours 5.812e-08
The seam cases measure theirs when they run."""
import numpy as np
import pytest
import torch

import tsdf                        # host/tsdf.py: the feature under test
import tsdf_truth as tt

pytestmark = pytest.mark.gpu

TOLERANCE_FACTOR = 4.0
SPHERE_E_TSDF, SPHERE_E_COLOUR, SPHERE_E_VERTEX, SPHERE_E_VCOLOUR = 2.395e-06, 7.153e-07, 3.405e-08, 5.812e-08


def _volume(geometry, colour=True):
    nx, ny, nz = geometry["blocks"]
    v, o = geometry["voxel_size"], geometry["origin"]
    vol = tsdf.TSDFVolume(v, geometry["sdf_trunc"], depth_trunc=geometry["depth_trunc"],
                          bounds=(o, tuple(x + 8 * v * n for x, n in zip(o, (nx, ny, nz)))), colour=colour, device="cuda")
    assert vol.blocks == (nx, ny, nz) and vol.origin == tuple(o)
    return vol


def _fuse(geometry, frames, parts=None, start=None):
    """a TSDFVolume on the GPU (empty, or loaded from the state `start`) with the frames integrated, in one call or in the
    camera ranges `parts`"""
    vol = _volume(geometry, colour=frames["colour"] is not None)
    if start is not None:
        vol.load_state_dict(start)
    n = len(frames["cams"])
    for a, b in parts or [(0, n)]:
        dev = lambda t: None if t is None else t[a:b].cuda()
        vol.integrate(dev(frames["depth"]), frames["cams"][a:b], colour=dev(frames["colour"]), weight=dev(frames.get("weight")))
    return vol


def _marks_of(state):
    nx, ny, nz = state["blocks"]
    m = np.zeros((nz, ny, nx), dtype=bool)
    c = state["block_coords"].long().numpy()
    m[c[:, 2], c[:, 1], c[:, 0]] = True
    return m


def _check_fused(name, geometry, frames, state, errors=None):
    """the GPU volume `state` against the truth of integrating `frames` into the empty volume; returns (truth, flagged)"""
    lo, hi = tt.activate(geometry, frames)
    got = _marks_of(state)
    assert not (lo & ~got).any(), f"{name}: {int((lo & ~got).sum())} blocks of the truth's certain set are not active"
    assert not (got & ~hi).any(), f"{name}: {int((got & ~hi).sum())} active blocks outside the truth's possible set"
    active = tt.with_blocks(geometry, got)
    assert torch.equal(active["block_coords"], state["block_coords"]), f"{name}: slots are not in ascending block order"
    truth, flagged = tt.integrate(active, frames)
    share = flagged.float().mean().item()
    r32, e_t, e_c = tt.restatement_errors(active, frames, flagged, truth)
    if errors is not None:
        e_t, e_c = errors
    ok = ~flagged
    for k in ("tsdf_sum", "weight_sum", "colour_sum"):
        assert state[k] is None or bool(torch.isfinite(state[k]).all()), f"{name}: {k} is not finite"
    d_t = (state["tsdf_sum"].double() - truth["tsdf_sum"]).abs()[ok].max().item()
    d_c = 0.0
    if truth["colour_sum"] is not None:
        d_c = (state["colour_sum"].double() - truth["colour_sum"]).abs()[ok[:, None, :].expand(-1, 3, -1)].max().item()
    print(f"[tsdf] {name}: {len(state['block_coords'])} blocks, borderline {share:.4%}, tsdf_sum {d_t:.3e} (restatement {e_t:.3e}), "
          f"colour_sum {d_c:.3e} (restatement {e_c:.3e})")
    assert share < tt.MAX_BORDERLINE, f"{name}: {share:.4%} borderline lattice points"
    assert torch.equal(state["weight_sum"][ok].view(torch.int32), r32["weight_sum"][ok].view(torch.int32)), f"{name}: weight_sum"
    assert d_t <= TOLERANCE_FACTOR * e_t, f"{name}: tsdf_sum {d_t:.3e} from the truth, the restatement {e_t:.3e}"
    assert d_c <= TOLERANCE_FACTOR * e_c, f"{name}: colour_sum {d_c:.3e} from the truth, the restatement {e_c:.3e}"
    return truth, flagged


def _check_extraction(name, vol, errors=None):
    """tsdf_extract on the volume against the numpy restatement on the identical float32 sums"""
    import diff_gaussian_rasterization as dgr
    state = vol.state_dict()
    v, c, f = dgr.tsdf_extract(vol)
    v64, c64, f64 = tt.extract(state)
    v32, c32, f32 = tt.extract(state, dtype=np.float32)
    assert np.array_equal(f64, f32)
    assert f.dtype == torch.int32 and np.array_equal(f.cpu().numpy().astype(np.int64), f64), f"{name}: faces"
    e_v = np.abs(v32.astype(np.float64) - v64).max() if len(v64) else 0.0
    e_c = np.abs(c32.astype(np.float64) - c64).max() if c64 is not None and len(c64) else 0.0
    if errors is not None:
        e_v, e_c = errors
    d_v = np.abs(v.cpu().numpy().astype(np.float64) - v64).max() if len(v64) else 0.0
    d_c = np.abs(c.cpu().numpy().astype(np.float64) - c64).max() if c64 is not None and len(c64) else 0.0
    print(f"[tsdf] {name}: {len(v64)} vertices, {len(f64)} faces, vertices {d_v:.3e} (restatement {e_v:.3e}), "
          f"colours {d_c:.3e} (restatement {e_c:.3e})")
    assert tuple(v.shape) == v64.shape and (c is None) == (c64 is None)
    assert d_v <= TOLERANCE_FACTOR * e_v, f"{name}: vertices {d_v:.3e} from float64, the restatement {e_v:.3e}"
    assert d_c <= TOLERANCE_FACTOR * e_c, f"{name}: colours {d_c:.3e} from float64, the restatement {e_c:.3e}"
    return v, c, f


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _by_block(state):
    """the sums keyed by block, for volumes whose slots were created in different orders"""
    nx, ny, _ = state["blocks"]
    c = state["block_coords"].long()
    order = torch.argsort((c[:, 2] * ny + c[:, 1]) * nx + c[:, 0])
    return [c[order]] + [state[k][order] for k in ("tsdf_sum", "weight_sum", "colour_sum") if state[k] is not None]


# ---- the sphere case ----
@pytest.fixture(scope="module")
def sphere():
    geometry, frames = tt.sphere_case()
    vol = _fuse(geometry, frames)
    return dict(geometry=geometry, frames=frames, vol=vol, state=vol.state_dict())


def test_sphere_case_against_float64(sphere):
    lo, hi = tt.activate(sphere["geometry"], sphere["frames"])
    assert np.array_equal(lo, hi) and np.array_equal(_marks_of(sphere["state"]), lo)          # the active block set is EQUAL
    _check_fused("sphere", sphere["geometry"], sphere["frames"], sphere["state"], errors=(SPHERE_E_TSDF, SPHERE_E_COLOUR))
    w = sphere["state"]["weight_sum"]
    assert torch.equal(w, w.round()) and 0 < w.max() <= 14                                   # unit weights: whole numbers


def test_sphere_case_mesh(sphere):
    _check_extraction("sphere", sphere["vol"], errors=(SPHERE_E_VERTEX, SPHERE_E_VCOLOUR))
    v, c, f = sphere["vol"].extract_mesh()
    v, f = v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(np.int64)
    assert len(np.unique(f)) == len(v) and c.shape == (len(v), 3)
    open_edges, doubled = tt.boundary_edges(f)
    assert len(open_edges) == 0 and not doubled and tt.euler_characteristic(f) == 2
    normal, centroid = tt.face_normals(v, f)
    assert ((normal * (centroid - np.asarray(tt.SPHERE_CENTRE))).sum(axis=1) > 0).all()


def test_two_runs_and_incremental_integration_leave_the_same_bits(sphere):
    import diff_gaussian_rasterization as dgr
    again = _fuse(sphere["geometry"], sphere["frames"])
    a, b = sphere["state"], again.state_dict()
    assert torch.equal(a["block_coords"], b["block_coords"])
    assert all(_same_bits(a[k], b[k]) for k in ("tsdf_sum", "weight_sum", "colour_sum"))
    for x, y in zip(dgr.tsdf_extract(sphere["vol"]), dgr.tsdf_extract(again)):
        assert _same_bits(x, y)
    # on one set of blocks, views 0..4 and then 5..13 leave the bits of all fourteen at once (a block that a later batch
    # activates has not seen the earlier views: that is the sparse volume, not the integration)
    zeroed = tt.with_blocks(sphere["geometry"], _marks_of(a))
    once = _fuse(sphere["geometry"], sphere["frames"], start=zeroed).state_dict()
    steps = _fuse(sphere["geometry"], sphere["frames"], parts=[(0, 5), (5, 14)], start=zeroed).state_dict()
    for x, y, z in zip(_by_block(steps), _by_block(once), _by_block(a)):
        assert (_same_bits(x, y) and _same_bits(x, z)) if x.dtype == torch.float32 else (torch.equal(x, y) and torch.equal(x, z))


# ---- seams and edges ----
def _chunk():
    import diff_gaussian_rasterization as dgr
    assert dgr.TSDF_CAMERA_CHUNK == 64
    return dgr.TSDF_CAMERA_CHUNK


def _special_depth(frames):
    """holes, depths past depth_trunc, NaN and Inf pixels in every map; returns the number of pixels changed"""
    g = torch.Generator().manual_seed(11)
    d = frames["depth"]
    kind = torch.randint(0, 12, d.shape, generator=g)
    for k, value in ((0, 0.0), (1, 25.0), (2, float("nan")), (3, float("inf")), (4, -1.0), (5, float("-inf"))):
        d[kind == k] = value
    return int((kind < 6).sum())


def _seam_case(name):
    if name == "chunk_plus_one":
        return tt.small_case(_chunk() + 1, 24, 24)
    if name == "one_camera":
        return tt.small_case(1)
    if name == "odd_image":
        return tt.small_case(5, 67, 45)
    if name == "camera_inside":
        geometry, frames = tt.small_case(4, inside_camera=True)
        M, _, _ = tt.table(frames["cams"][:1])
        p = tt.lattice_points(tt.with_blocks(geometry, tt.activate(geometry, frames)[0])).reshape(-1, 3)
        assert int(((p @ M[0, :3, 2] + M[0, 3, 2]) < 0).sum()) > 100       # stored lattice points behind the first camera
        return geometry, frames
    if name == "special_depth":
        geometry, frames = tt.small_case(6)
        assert _special_depth(frames) > 1000
        return geometry, frames
    if name == "weights":
        geometry, frames = tt.small_case(6)
        g = torch.Generator().manual_seed(5)
        choice = torch.randint(0, 5, frames["depth"].shape, generator=g)
        frames["weight"] = torch.tensor([0.0, 0.0, 0.5, 1.0, 2.0])[choice]          # dyadic: the weight sums are exact
        return geometry, frames
    if name == "no_colour":
        return tt.small_case(5, colour=False)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["chunk_plus_one", "one_camera", "odd_image", "camera_inside", "special_depth", "weights",
                                  "no_colour"])
def test_seams(name):
    geometry, frames = _seam_case(name)
    vol = _fuse(geometry, frames)
    state = vol.state_dict()
    assert (state["colour_sum"] is None) == (name == "no_colour") and len(state["block_coords"]) > 0
    _check_fused(name, geometry, frames, state)
    v, c, f = _check_extraction(name, vol)
    assert len(f) > 0 and bool(torch.isfinite(v).all()) and (c is None or bool(torch.isfinite(c).all()))
    if name == "weights":
        assert bool((state["weight_sum"] * 2 == (state["weight_sum"] * 2).round()).all())


def test_zero_cameras_and_an_empty_volume_launch_nothing(monkeypatch):
    import diff_gaussian_rasterization as dgr
    calls = []
    monkeypatch.setattr(dgr, "_tsdf_probe", calls.append)
    geometry, _ = tt.small_case(1)
    vol = _volume(geometry)
    vol.integrate(torch.zeros(0, 8, 8, device="cuda"), [], colour=torch.zeros(0, 3, 8, 8, device="cuda"))
    v, c, f = vol.extract_mesh()
    assert calls == [] and vol.num_blocks == 0 and v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3)
    # background only: nothing is activated, the integration has no slot to run on
    vol.integrate(torch.zeros(2, 8, 8, device="cuda"), tt.sphere_cameras(W=8, H=8)[:2], colour=torch.zeros(2, 3, 8, 8, device="cuda"))
    assert calls == ["msgs_tsdf_mark_blocks"] and vol.num_blocks == 0


# ---- planted fields ----
def _planted_volume(geometry, blocks, field, colour=None):
    planted = tt.planted(geometry, blocks, field, colour)
    return _volume(geometry, colour=colour is not None).load_state_dict(planted)


def _box(half):
    return tt.empty_volume(1.0 / 16, 4.0 / 16, 10.0, ((-half,) * 3, (half,) * 3))


def _all_blocks(blocks):
    nx, ny, nz = blocks
    return [(x, y, z) for z in range(nz) for y in range(ny) for x in range(nx)]


def _sphere_field(centre, radius):
    c = torch.tensor(centre, dtype=torch.float64)
    return lambda p: (p - c).norm(dim=1) - radius


COLOUR_FIELD = lambda p: 0.5 + 0.5 * torch.sin(3.0 * p)


def test_planted_plane():
    normal, c = torch.tensor([0.5, 0.25, 1.0], dtype=torch.float64), 0.1015625 + 1.0 / 256
    geometry = _box(0.5)
    vol = _planted_volume(geometry, _all_blocks(geometry["blocks"]), lambda p: p @ normal - c, COLOUR_FIELD)
    v, _, f = _check_extraction("plane", vol)
    assert len(f) > 100 and (v.double().cpu() @ normal - c).abs().max() < 1e-6


def test_planted_sphere_reads_table_index_0_and_the_last_of_each_axis():
    # every block of the table is active, the first and the last included: the neighbour lookup of the last blocks leaves the table
    geometry = _box(1.0)
    blocks = _all_blocks(geometry["blocks"])
    assert (0, 0, 0) in blocks and (3, 3, 3) in blocks
    vol = _planted_volume(geometry, blocks, _sphere_field(tt.SPHERE_CENTRE, 0.85), COLOUR_FIELD)
    assert int(vol.table[0, 0, 0]) == 0 and int(vol.table[3, 3, 3]) == 63
    v, c, f = _check_extraction("planted sphere", vol)
    f = f.cpu().numpy().astype(np.int64)
    assert len(tt.boundary_edges(f)[0]) == 0 and tt.euler_characteristic(f) == 2
    # blocks in the table's corners whose upper neighbours are outside the table or not active: the mesh ends inside them
    corner = _planted_volume(geometry, [(0, 0, 0), (3, 3, 3), (3, 0, 0), (0, 3, 0), (0, 0, 3)],
                             lambda p: p.abs().max(dim=1).values - 0.77, COLOUR_FIELD)
    _check_extraction("table corners", corner)


def test_a_block_without_upper_neighbours():
    geometry = _box(1.0)
    vol = _planted_volume(geometry, [(1, 2, 1)], _sphere_field((-0.26, 0.27, -0.24), 0.17), COLOUR_FIELD)
    assert int((vol.table >= 0).sum()) == 1
    v, c, f = _check_extraction("lone block", vol)
    # only the 7^3 cubes inside the block are meshed; crossings on its upper faces have no second end and are no vertices
    lo, hi = np.array([-0.5, 0.0, -0.5]), np.array([-0.5, 0.0, -0.5]) + 7.0 / 16
    assert len(f) > 0 and bool(((v.cpu().numpy() >= lo - 1e-6) & (v.cpu().numpy() <= hi + 1e-6)).all())


# ---- rendered views ----
def test_integrate_views_is_integrate_on_the_rendered_maps():
    import scenes
    from gaussian_renderer import render_with_median_depth
    from parity_utils import PIPE, small_scene
    from synthetic_model import SyntheticGaussians
    W, H = 160, 96
    sc, cam = small_scene(4000, W, H, seed=123)
    rot = lambda a: np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    cams = [cam] + [scenes.make_camera(rot(a), np.array([t, 0.0, 0.0]), cam.FoVx, cam.FoVy, W, H) for a, t in ((0.12, 0.4), (-0.1, -0.3))]
    cams = [c.to("cuda") for c in cams]
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    bg = torch.zeros(3, device="cuda")
    kw = dict(depth_trunc=30.0, bounds=((-14, -9, -3), (14, 9, 13)), device="cuda")
    by_views = tsdf.TSDFVolume(0.2, **kw)
    by_views.integrate_views(cams, pc, PIPE, bg)
    with torch.no_grad():
        outs = [render_with_median_depth(c, pc, PIPE, bg) for c in cams]
    depth = torch.stack([o["median_depth"] for o in outs])
    assert bool((depth > 0).any())
    by_maps = tsdf.TSDFVolume(0.2, **kw)
    by_maps.integrate(depth, cams, colour=torch.stack([o["render"] for o in outs]))
    a, b = by_views.state_dict(), by_maps.state_dict()
    assert len(a["block_coords"]) > 10 and torch.equal(a["block_coords"], b["block_coords"])
    assert all(_same_bits(a[k], b[k]) for k in ("tsdf_sum", "weight_sum", "colour_sum")) and a["weight_sum"].max() >= 2
    # the expected depth: blended depth over alpha, weighted by alpha
    expected = tsdf.TSDFVolume(0.2, **kw)
    expected.integrate_views(cams, pc, PIPE, bg, depth="expected")
    w = expected.state_dict()["weight_sum"]
    assert expected.num_blocks > 10 and bool(torch.isfinite(w).all()) and not torch.equal(w, w.round())
    v, c, f = by_views.extract_mesh()
    assert len(f) > 0 and int(f.max()) == len(v) - 1 and bool(torch.isfinite(v).all()) and bool(torch.isfinite(c).all())

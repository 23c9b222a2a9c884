"""Connected components and mesh clean-up on the GPU (SPEC M22; 4.24; include/msgs.h msgs_graph_components,
msgs_mesh_*) against the host truth of tests/mesh_truth.py.  The labels are defined by the input alone (the smallest node of the
component), so every comparison here is exact integer equality, or bit equality for gathered vertices and colours, on every run:
no tolerance, no left-out cases."""
import numpy as np
import pytest
import torch

import diff_gaussian_rasterization as dgr
import mesh                        # host/mesh.py: the feature under test
import mesh_truth as mt
import tsdf                        # host/tsdf.py
import tsdf_truth as tt

pytestmark = pytest.mark.gpu


def _dev(x, dtype=torch.int32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda()


def _np(t):
    return t.cpu().numpy().astype(np.int64)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


# ---- (a) graph components ----
@pytest.mark.parametrize("name", mt.GRAPH_NAMES)
def test_graph_components(name):
    N, a, b, want = mt.graph_case(name)
    ad, bd = _dev(a), _dev(b)
    first, second = dgr.graph_components(N, ad, bd), dgr.graph_components(N, ad, bd)
    assert first.dtype == torch.int32 and first.shape == (N,) and first.is_cuda
    assert np.array_equal(_np(first), want), name
    assert _same(first, second)                                            # the same bits on every run
    # the edge list the other way round and with int64 indices: the same graph
    assert _same(dgr.graph_components(N, bd.long(), ad.long()), first)


def test_graph_components_without_nodes_or_edges_launches_nothing(monkeypatch):
    calls = []
    monkeypatch.setattr(dgr, "_mesh_probe", calls.append)
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    out = dgr.graph_components(0, none, none)
    assert out.shape == (0,) and out.dtype == torch.int32
    assert dgr.graph_components(5, none, none).tolist() == [0, 1, 2, 3, 4]
    assert calls == []
    dgr.graph_components(2, none.new_tensor([0]), none.new_tensor([1]))
    assert calls == ["msgs_graph_components"]


def test_graph_components_refuses_nodes_outside_the_graph(monkeypatch):
    calls = []
    monkeypatch.setattr(dgr, "_mesh_probe", calls.append)
    ok = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    for bad in ([0, 1, 4], [0, -1, 2]):
        bad = torch.tensor(bad, dtype=torch.int32, device="cuda")
        with pytest.raises(ValueError, match=r"must lie in \[0, 4\)"):
            dgr.graph_components(4, ok, bad)
        with pytest.raises(ValueError, match=r"must lie in \[0, 4\)"):
            dgr.graph_components(4, bad, ok)
    assert calls == []


# ---- (b), (c) hand meshes ----
HAND = mt.hand_meshes()


def _clusters(faces, V, connectivity):
    fd = _dev(faces)
    first, second = dgr.mesh_triangle_clusters(fd, V, connectivity), dgr.mesh_triangle_clusters(fd, V, connectivity)
    for x, y in zip(first, second):
        assert x.dtype == torch.int32 and _same(x, y)
    assert first[0].shape == (len(faces),)
    return _np(first[0]), _np(first[1])


@pytest.mark.parametrize("connectivity", ["edge", "vertex"])
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_meshes(name, connectivity):
    faces, V = HAND[name]
    clusters, counts = _clusters(faces, V, connectivity)
    want = mt.triangle_clusters(faces, connectivity)
    assert np.array_equal(clusters, want[0]) and np.array_equal(counts, want[1])
    assert dgr.mesh_edge_report(_dev(faces), V) == mt.edge_report(faces)
    assert mesh.edge_report(_dev(faces, torch.int64), V) == mt.edge_report(faces)
    # any permutation of the faces renumbers the clusters by their new smallest face index, exactly as the rule says
    perm = np.random.default_rng(len(faces)).permutation(len(faces))
    clusters, counts = _clusters(faces[perm], V, connectivity)
    want = mt.triangle_clusters(faces[perm], connectivity)
    assert np.array_equal(clusters, want[0]) and np.array_equal(counts, want[1])
    # ... and rotating every face's corners changes nothing
    assert np.array_equal(_clusters(np.roll(faces, 1, axis=1), V, connectivity)[0], mt.triangle_clusters(faces, connectivity)[0])


def test_hand_meshes_say_what_the_issue_says():
    count = lambda name, c: _clusters(*HAND[name], c)[1].tolist()
    report = lambda name: dgr.mesh_edge_report(_dev(HAND[name][0]), HAND[name][1])
    assert count("two tetrahedra", "edge") == count("two tetrahedra", "vertex") == [4, 4]
    assert count("shared vertex", "edge") == [4, 4] and count("shared vertex", "vertex") == [8]
    assert count("shared edge", "edge") == count("shared edge", "vertex") == [8] and report("shared edge")[2] == 1
    assert report("one triangle") == (3, 0, 0) and report("tetrahedron") == (0, 6, 0)
    assert count("repeated index", "edge") == [4, 1, 4] and count("repeated index", "vertex") == [5, 4]
    assert count("unused vertices", "edge") == [4, 4]
    # post_process_mesh drops the face that repeats an index and the vertex only it used; remove_degenerate=False keeps it
    faces, V = HAND["repeated index"]
    v = torch.arange(3 * V, dtype=torch.float32, device="cuda").reshape(V, 3)
    v2, c2, f2 = mesh.post_process_mesh(v, None, _dev(faces), cluster_to_keep=5, min_triangles=1)
    assert c2 is None and f2.dtype == torch.int32 and len(f2) == 8 and torch.equal(v2, v[[0, 1, 2, 3, 5, 6, 7, 8]])
    v3, _, f3 = mesh.post_process_mesh(v, None, _dev(faces), cluster_to_keep=5, min_triangles=1, remove_degenerate=False)
    assert torch.equal(v3, v) and torch.equal(f3, _dev(faces))
    for kw in (dict(), dict(remove_degenerate=False), dict(connectivity="vertex")):
        want = mt.post_process_mesh(v.cpu().numpy(), None, faces, cluster_to_keep=2, min_triangles=2, **kw)
        got = mesh.post_process_mesh(v, None, _dev(faces), cluster_to_keep=2, min_triangles=2, **kw)
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(_np(got[2]), want[2])


def test_a_mesh_of_many_workgroups_and_a_ragged_end():
    """a strip of 1237 quads (lower triangle i, upper triangle n + i) without the quads 300 and 900 and without the upper
    triangle of quad 763, whose neighbours then share one vertex only: 4 pieces by edges, 3 by vertices; shuffled, so that runs of
    equal keys join faces across wave and workgroup seams; 3 F is no multiple of 64"""
    n = 1237
    i = np.arange(n)
    faces = np.concatenate([np.stack([i, i + 1, i + n + 1], 1), np.stack([i + 1, i + n + 2, i + n + 1], 1)])
    cut = np.ones(len(faces), dtype=bool)
    cut[[300, n + 300, 900, n + 900, n + 763]] = False
    faces = faces[cut][np.random.default_rng(4).permutation(int(cut.sum()))]
    V = 2 * n + 2
    assert (3 * len(faces)) % 64 != 0
    for connectivity, pieces in (("edge", 4), ("vertex", 3)):
        clusters, counts = _clusters(faces, V, connectivity)
        want = mt.triangle_clusters(faces, connectivity)
        assert len(want[1]) == pieces and np.array_equal(clusters, want[0]) and np.array_equal(counts, want[1])
    assert dgr.mesh_edge_report(_dev(faces), V) == mt.edge_report(faces)


def test_more_keys_than_one_pass_of_the_edge_report_grid():
    """the edge report walks the sorted keys with a fixed grid of 2048 workgroups of 256 lanes: 3 F = 539 940 keys need a second
    trip, with a ragged end; the strip has holes (boundary edges), a fin on one edge and 15 faces twice (non-manifold edges)"""
    n = 90007
    i = np.arange(n)
    faces = np.concatenate([np.stack([i, i + 1, i + n + 1], 1), np.stack([i + 1, i + n + 2, i + n + 1], 1)])
    cut = np.ones(len(faces), dtype=bool)
    cut[np.random.default_rng(8).integers(0, len(faces), 50)] = False
    faces = np.concatenate([faces[cut], [[5, 6, 2 * n + 2]], faces[:15]])      # a fin on the edge {5, 6}; 15 faces twice
    assert 3 * len(faces) > 2048 * 256 and (3 * len(faces)) % 64 != 0
    V = 2 * n + 3
    want = mt.edge_report(faces)
    assert min(want) > 0
    fd = _dev(faces)
    assert dgr.mesh_edge_report(fd, V) == want == dgr.mesh_edge_report(fd, V)
    clusters, counts = dgr.mesh_triangle_clusters(fd, V)
    want = mt.triangle_clusters(faces)
    assert len(want[1]) > 1 and np.array_equal(_np(clusters), want[0]) and np.array_equal(_np(counts), want[1])


# ---- the planted three-body volume ----
_PLANTED = {}


def _planted():
    """(vertices, colours, faces) of extract_mesh on the planted volume, the truth's clusters on those faces; computed once"""
    if not _PLANTED:
        state = mt.planted_volume(colour=True)
        vol = tsdf.TSDFVolume(state["voxel_size"], state["sdf_trunc"], depth_trunc=10.0,
                              bounds=((-1,) * 3, (1,) * 3)).load_state_dict(state)
        v, c, f = vol.extract_mesh()
        _PLANTED["mesh"] = (v, c, f)
        _PLANTED["truth"] = mt.triangle_clusters(_np(f))
    return _PLANTED["mesh"] + _PLANTED["truth"]


def test_planted_volume_clusters_equal_the_truth():
    v, c, f, want_clusters, want_counts = _planted()
    assert np.array_equal(_np(f), mt.planted_mesh()[1])                   # the GPU extraction has the truth's faces
    for connectivity in ("edge", "vertex"):
        clusters, counts = mesh.cluster_connected_triangles(f, len(v), connectivity)
        again = dgr.mesh_triangle_clusters(f, len(v), connectivity)
        assert _same(clusters, again[0]) and _same(counts, again[1])
        assert np.array_equal(_np(clusters), want_clusters) and np.array_equal(_np(counts), want_counts)
    assert len(want_counts) == 3
    report = mesh.edge_report(f, len(v))
    assert report == mt.edge_report(_np(f)) and report.boundary == 0 and report.non_manifold == 0
    assert 2 * report.manifold == 3 * len(f)


def test_planted_volume_post_process_equals_the_restatement():
    v, c, f, want_clusters, want_counts = _planted()
    vn, cn, fn = v.cpu().numpy(), c.cpu().numpy(), _np(f)
    v2, c2, f2 = mesh.post_process_mesh(v, c, f, cluster_to_keep=2, min_triangles=1)
    w2, d2, g2 = mt.post_process_mesh(vn, cn, fn, cluster_to_keep=2, min_triangles=1)
    assert f2.dtype == torch.int32 and np.array_equal(_np(f2), g2)
    assert v2.dtype == c2.dtype == torch.float32
    assert np.array_equal(v2.cpu().numpy().view(np.uint32), w2.view(np.uint32))
    assert np.array_equal(c2.cpu().numpy().view(np.uint32), d2.view(np.uint32))
    # order kept: the surviving faces are the input's, in the input's order, over the same points
    floater = int(want_counts.argmin())
    assert torch.equal(v2[f2.long()], v[f[torch.as_tensor(want_clusters != floater).cuda()].long()])
    assert len(f2) == len(f) - want_counts[floater] and len(v2) < len(v)
    # two clusters, closed, two spheres
    clusters, counts = dgr.mesh_triangle_clusters(f2, len(v2))
    assert _np(counts).tolist() == [int(n) for k, n in enumerate(want_counts) if k != floater]
    assert mesh.edge_report(f2, len(v2))[::2] == (0, 0) and tt.euler_characteristic(g2) == 4
    # a second run has the same bits
    for x, y in zip((v2, c2, f2), mesh.post_process_mesh(v, c, f, cluster_to_keep=2, min_triangles=1)):
        assert _same(x, y)
    # the defaults (50 clusters, 50 triangles) lose nothing here: the floater has more than 50 faces
    v3, c3, f3 = mesh.post_process_mesh(v, c, f)
    assert want_counts.min() >= 50 and _same(v3, v) and _same(c3, c) and _same(f3, f)
    # a floor above the floater drops it whatever cluster_to_keep says
    _, _, f4 = mesh.post_process_mesh(v, c, f, min_triangles=int(want_counts.min()) + 1)
    assert _same(f4, f2)
    # without colours
    v5, c5, f5 = mesh.post_process_mesh(v, None, f, cluster_to_keep=2, min_triangles=1)
    assert c5 is None and _same(v5, v2) and _same(f5, f2)
    # in one line behind the extraction, as the README has it
    assert _same(mesh.post_process_mesh(*_PLANTED["mesh"], cluster_to_keep=2, min_triangles=1)[2], f2)


# ---- zero launches and refusals ----
def test_no_faces_launch_nothing(monkeypatch):
    calls = []
    monkeypatch.setattr(dgr, "_mesh_probe", calls.append)
    none = torch.zeros(0, 3, dtype=torch.int32, device="cuda")
    for connectivity in ("edge", "vertex"):
        clusters, counts = dgr.mesh_triangle_clusters(none, 7, connectivity)
        assert clusters.shape == (0,) and counts.shape == (0,) and clusters.dtype == counts.dtype == torch.int32
        assert clusters.is_cuda and counts.is_cuda
    assert dgr.mesh_edge_report(none, 7) == (0, 0, 0) and dgr.mesh_edge_report(none, 0) == (0, 0, 0)
    v = torch.rand(7, 3, device="cuda")
    v2, c2, f2 = mesh.post_process_mesh(v, v.clone(), none)
    assert v2.shape == (0, 3) and c2.shape == (0, 3) and f2.shape == (0, 3) and f2.dtype == torch.int32
    v2, c2, f2 = mesh.post_process_mesh(v[:0], None, none)
    assert v2.shape == (0, 3) and c2 is None and f2.shape == (0, 3)
    assert calls == []
    dgr.mesh_triangle_clusters(none.new_tensor([[0, 1, 2]]), 7)
    assert calls == ["msgs_mesh_corner_keys", "msgs_mesh_link_sorted"]


def test_indices_outside_the_vertices_are_refused_before_any_launch(monkeypatch):
    calls = []
    monkeypatch.setattr(dgr, "_mesh_probe", calls.append)
    v = torch.rand(4, 3, device="cuda")
    for bad in ([[0, 1, 2], [1, 2, 4]], [[0, 1, 2], [1, -1, 3]]):
        for dtype in (torch.int32, torch.int64):
            faces = torch.tensor(bad, dtype=dtype, device="cuda")
            with pytest.raises(ValueError, match=r"must lie in \[0, 4\)"):
                dgr.mesh_triangle_clusters(faces, 4)
            with pytest.raises(ValueError, match=r"must lie in \[0, 4\)"):
                dgr.mesh_edge_report(faces, 4)
            with pytest.raises(ValueError, match=r"must lie in \[0, 4\)"):
                mesh.post_process_mesh(v, None, faces)
    assert calls == []

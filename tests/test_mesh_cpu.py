"""Connected components and mesh clean-up without a GPU (SPEC M22; 4.24): the truth of tests/mesh_truth.py against
its second statement through scipy on every graph the GPU tests use, the selection rule, the key packing, the truth on a planted
three-body volume, and the surface with its refusals.  Nothing in this file reaches a kernel; every comparison is exact."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import diff_gaussian_rasterization as dgr
import mesh                        # host/mesh.py: the feature under test
import mesh_truth as mt
import tsdf_truth as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msgs_graph_components", "msgs_mesh_corner_keys", "msgs_mesh_link_sorted", "msgs_mesh_edge_report")


@pytest.mark.parametrize("name", mt.GRAPH_NAMES)
def test_the_two_truths_agree(name):
    N, a, b, label = mt.graph_case(name)
    assert label.shape == (N,) and np.array_equal(label, mt.components_scipy(N, a, b))
    # the definition itself: a label is a node of its own component and the smallest one
    assert (label <= np.arange(N)).all() and np.array_equal(label[label], label)
    if len(a):
        assert np.array_equal(label[a], label[b])


def test_the_two_truths_agree_on_the_face_graphs():
    v, f = mt.planted_mesh()
    for faces in [f] + [m for m, _ in mt.hand_meshes().values()]:
        for connectivity in ("edge", "vertex"):
            keys, face = mt.corner_keys(faces, connectivity)
            order = np.argsort(keys, kind="stable")
            same = keys[order][1:] == keys[order][:-1]
            a, b = face[order][:-1][same], face[order][1:][same]           # the sorted-neighbour form the kernel links
            assert np.array_equal(mt.face_labels(faces, connectivity), mt.components_scipy(len(faces), a, b))


def test_select_clusters():
    pick = lambda counts, **kw: mesh.select_clusters(torch.tensor(counts, dtype=torch.int32), **kw).tolist()
    # ties at the threshold are all kept
    assert pick([100, 50, 50, 10], cluster_to_keep=2, min_triangles=1) == [True, True, True, False]
    # more clusters asked for than there are: the floor alone decides
    assert pick([100, 50, 50, 10], cluster_to_keep=10, min_triangles=20) == [True, True, True, False]
    assert pick([100, 50, 50, 10], cluster_to_keep=4, min_triangles=1) == [True] * 4
    # the floor wins over a smaller k-th count
    assert pick([100, 50, 50, 10], cluster_to_keep=3, min_triangles=60) == [True, False, False, False]
    assert pick([3, 9, 5], cluster_to_keep=1, min_triangles=0) == [False, True, False]
    # defaults: 2DGS's 50 and 50
    assert pick([49, 50, 51]) == [False, True, True]
    empty = mesh.select_clusters(torch.zeros(0, dtype=torch.int32))
    assert empty.shape == (0,) and empty.dtype == torch.bool
    for counts, kw in (([100, 50, 50, 10], dict(cluster_to_keep=2, min_triangles=1)), ([4, 4, 4], dict(cluster_to_keep=1)),
                       ([], {}), ([7], dict(min_triangles=7)), (list(range(200)), {})):
        assert pick(counts, **kw) == mt.select_clusters(counts, **kw).tolist()
    assert mesh.select_clusters(torch.tensor([5, 6], dtype=torch.int64), 1, 1).tolist() == [False, True]
    with pytest.raises(ValueError):
        mesh.select_clusters(torch.tensor([5, 6]), cluster_to_keep=0)
    with pytest.raises(ValueError):
        mesh.select_clusters(torch.tensor([5.0, 6.0]))


def test_key_packing_at_the_ends_of_the_index_range():
    top = 2 ** 31 - 2
    assert int(mt.pack_edge_key(0, top)) == int(mt.pack_edge_key(top, 0)) == top
    assert int(mt.pack_edge_key(top, top)) == (top << 32) | top < 2 ** 63
    assert int(mt.pack_edge_key(1, 0)) == 1 and int(mt.pack_edge_key(1, top)) == (1 << 32) | top
    # distinct pairs, distinct keys; ascending in (min, max)
    pairs = [(0, 0), (0, 1), (0, top), (1, 1), (1, top), (top - 1, top), (top, top)]
    keys = [int(mt.pack_edge_key(v, u)) for u, v in pairs]
    assert keys == sorted(set(keys))
    keys, face = mt.corner_keys(np.array([[0, top, 5], [7, 7, 0]]))
    assert keys.tolist() == [top, (5 << 32) | top, 5, (7 << 32) | 7, 7, 7] and face.tolist() == [0, 0, 0, 1, 1, 1]
    assert mt.corner_keys(np.array([[0, top, 5]]), "vertex")[0].tolist() == [0, top, 5]


def test_truth_on_the_hand_meshes():
    m = mt.hand_meshes()
    cl = lambda name, c: mt.triangle_clusters(m[name][0], c)
    assert cl("two tetrahedra", "edge")[1].tolist() == cl("two tetrahedra", "vertex")[1].tolist() == [4, 4]
    assert cl("shared vertex", "edge")[1].tolist() == [4, 4] and cl("shared vertex", "vertex")[1].tolist() == [8]
    assert cl("shared edge", "edge")[1].tolist() == cl("shared edge", "vertex")[1].tolist() == [8]
    assert mt.edge_report(m["shared edge"][0]) == (0, 10, 1)
    assert mt.edge_report(m["one triangle"][0]) == (3, 0, 0) and mt.edge_report(m["tetrahedron"][0]) == (0, 6, 0)
    assert cl("repeated index", "edge")[0].tolist() == [0] * 4 + [1] + [2] * 4
    assert cl("repeated index", "vertex")[0].tolist() == [0] * 5 + [1] * 4
    # numbering follows the smallest face index: reversing the faces reverses the ids
    faces = m["repeated index"][0]
    assert mt.triangle_clusters(faces[::-1])[0].tolist() == [0] * 4 + [1] + [2] * 4
    assert mt.triangle_clusters(faces[[8, 4, 0, 1, 2, 3, 5, 6, 7]])[0].tolist() == [0, 1, 2, 2, 2, 2, 0, 0, 0]


def test_truth_on_the_planted_volume_finds_three_closed_clusters():
    v, f = mt.planted_mesh()
    assert len(f) > 5000 and f.max() == len(v) - 1
    clusters, counts = mt.triangle_clusters(f)
    assert len(counts) == 3 and counts.sum() == len(f) and counts.min() >= 50
    assert np.array_equal(mt.triangle_clusters(f, "vertex")[0], clusters)
    centres = np.array([c for c, _ in mt.SPHERES])
    seen = set()
    for k in range(3):
        part = f[clusters == k]
        assert len(tt.boundary_edges(part)[0]) == 0 and tt.euler_characteristic(part) == 2
        b, m, n = mt.edge_report(part)
        assert (b, n) == (0, 0) and 2 * m == 3 * len(part)
        body = int(np.argmin(np.linalg.norm(v[part.reshape(-1)].mean(0) - centres, axis=1)))
        r = np.linalg.norm(v[np.unique(part)] - centres[body], axis=1)
        assert np.abs(r - mt.SPHERES[body][1]).max() < 0.02
        seen.add(body)
    assert seen == {0, 1, 2}
    # the clean-up that keeps two: the floater goes, order and rows stay
    v2, _, f2 = mt.post_process_mesh(v, None, f, cluster_to_keep=2, min_triangles=1)
    floater = int(counts.argmin())
    assert len(f2) == len(f) - counts[floater] and tt.euler_characteristic(f2) == 4 and len(tt.boundary_edges(f2)[0]) == 0
    assert np.array_equal(v2[f2], v[f[clusters != floater]])
    v3, _, f3 = mt.post_process_mesh(v, None, f)
    assert np.array_equal(f3, f) and np.array_equal(v3, v)


def test_symbols_are_declared_exported_and_bound():
    B = dgr._C
    header = open(os.path.join(ROOT, "include", "msgs.h")).read()
    nargs = {}
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, header), n
        assert n in B.EXPORTS and callable(getattr(B.lib, n)) and getattr(B.lib, n).restype is C.c_int
        nargs[n] = len(re.search(r"\bint %s\(([^;]*)\);" % n, header).group(1).split(","))
        assert len(getattr(B.lib, n).argtypes) == nargs[n], n
    assert nargs == {NAMES[0]: 7, NAMES[1]: 6, NAMES[2]: 7, NAMES[3]: 4}
    assert B.ABI_VERSION == 11 and B.lib.msgs_abi_version() == 11
    value = lambda name: int(re.search(rf"#define {name} ([0-9]+)", header).group(1))
    assert value("MSGS_MESH_EDGE") == B.MESH_EDGE == 0 and value("MSGS_MESH_VERTEX") == B.MESH_VERTEX == 1
    for n in ("graph_components", "mesh_triangle_clusters", "mesh_edge_report"):
        assert n in dgr.__all__ and callable(getattr(dgr, n))
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(dgr.graph_components) == ["n_nodes", "a", "b"]
    assert sig(dgr.mesh_triangle_clusters) == ["faces", "n_vertices", "connectivity"]
    assert sig(dgr.mesh_edge_report) == ["faces", "n_vertices"]
    assert sig(mesh.post_process_mesh) == ["vertices", "colours", "faces", "cluster_to_keep", "min_triangles", "connectivity",
                                           "remove_degenerate"]
    assert inspect.signature(mesh.post_process_mesh).parameters["connectivity"].default == "edge"
    assert sig(mesh.select_clusters) == ["cluster_n_triangles", "cluster_to_keep", "min_triangles"]
    for n in ("cluster_connected_triangles", "remove_unreferenced_vertices", "edge_report"):
        assert callable(getattr(mesh, n))
    assert "csrc/mesh.hip" in open(os.path.join(ROOT, "ms-gs_amd", "Makefile")).read()


def test_argument_checks_of_the_c_entries():
    """negative and oversized counts, an unknown mode and NULL pointers are refused before anything is launched; empty inputs
    return at once (no GPU is touched: every call below ends in the argument checks)"""
    lib = dgr._C.lib
    p = C.c_void_p(256)                                                    # never dereferenced
    bad, big = -1, 1 << 31
    assert lib.msgs_graph_components(bad, 0, p, p, p, p, None) == bad
    assert lib.msgs_graph_components(4, bad, p, p, p, p, None) == bad
    assert lib.msgs_graph_components(big, 0, p, p, p, p, None) == bad
    assert lib.msgs_graph_components(4, 2, None, p, p, p, None) == bad
    assert lib.msgs_graph_components(4, 2, p, None, p, p, None) == bad
    assert lib.msgs_graph_components(4, 0, None, None, None, p, None) == bad
    assert lib.msgs_graph_components(4, 0, None, None, p, None, None) == bad
    assert lib.msgs_graph_components(0, 1, p, p, p, p, None) == bad
    assert lib.msgs_graph_components(0, 0, None, None, None, None, None) == 0
    assert lib.msgs_mesh_corner_keys(bad, p, 0, p, p, None) == bad
    assert lib.msgs_mesh_corner_keys((big + 2) // 3, p, 0, p, p, None) == bad          # 3 F >= 2^31
    assert lib.msgs_mesh_corner_keys(4, p, 2, p, p, None) == bad
    assert lib.msgs_mesh_corner_keys(4, None, 0, p, p, None) == bad
    assert lib.msgs_mesh_corner_keys(4, p, 1, None, p, None) == bad
    assert lib.msgs_mesh_corner_keys(4, p, 1, p, None, None) == bad
    assert lib.msgs_mesh_corner_keys(0, None, 0, None, None, None) == 0
    assert lib.msgs_mesh_link_sorted(bad, 0, p, p, p, p, None) == bad
    assert lib.msgs_mesh_link_sorted(4, bad, p, p, p, p, None) == bad
    assert lib.msgs_mesh_link_sorted((big + 2) // 3, 12, p, p, p, p, None) == bad
    assert lib.msgs_mesh_link_sorted(4, 12, None, p, p, p, None) == bad
    assert lib.msgs_mesh_link_sorted(4, 12, p, None, p, p, None) == bad
    assert lib.msgs_mesh_link_sorted(4, 12, p, p, None, p, None) == bad
    assert lib.msgs_mesh_link_sorted(4, 12, p, p, p, None, None) == bad
    assert lib.msgs_mesh_link_sorted(0, 3, p, p, p, p, None) == bad
    assert lib.msgs_mesh_link_sorted(0, 0, None, None, None, None, None) == 0
    assert lib.msgs_mesh_edge_report(bad, p, p, None) == bad
    assert lib.msgs_mesh_edge_report(big, p, p, None) == bad
    assert lib.msgs_mesh_edge_report(12, None, p, None) == bad
    assert lib.msgs_mesh_edge_report(12, p, None, None) == bad
    assert lib.msgs_mesh_edge_report(0, None, None, None) == bad


def test_refusals_come_before_any_launch(monkeypatch):
    calls = []
    monkeypatch.setattr(dgr, "_mesh_probe", calls.append)
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32)
    v = torch.zeros(4, 3)
    for bad in (faces.float(), faces[:, :2], faces.reshape(-1), [[0, 1, 2]], None):
        with pytest.raises(ValueError):
            dgr.mesh_triangle_clusters(bad, 4)
        with pytest.raises(ValueError):
            dgr.mesh_edge_report(bad, 4)
    with pytest.raises(ValueError, match="connectivity"):
        dgr.mesh_triangle_clusters(faces, 4, "face")
    with pytest.raises(ValueError, match="n_vertices"):
        dgr.mesh_triangle_clusters(faces, -1)
    e = torch.tensor([0, 1], dtype=torch.int32)
    for a, b in ((e.float(), e), (e, e[:1]), (e[None], e[None]), (e, None)):
        with pytest.raises(ValueError):
            dgr.graph_components(4, a, b)
    with pytest.raises(ValueError, match="n_nodes"):
        dgr.graph_components(-1, e, e)
    with pytest.raises(ValueError, match="vertices"):
        mesh.post_process_mesh(torch.zeros(4), None, faces)
    with pytest.raises(ValueError, match="colours"):
        mesh.post_process_mesh(v, torch.zeros(3, 3), faces)
    # host tensors: the package's error, still before any launch
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.graph_components(4, e, e)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.mesh_triangle_clusters(faces, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.mesh_edge_report(faces, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mesh.post_process_mesh(v, None, faces)
    assert calls == []


def test_remove_unreferenced_vertices_keeps_order_and_bits():
    g = torch.Generator().manual_seed(2)
    v, c = torch.randn(9, 3, generator=g), torch.rand(9, 3, generator=g)
    f = torch.tensor([[7, 2, 5], [5, 2, 8]], dtype=torch.int32)
    v2, c2, f2 = mesh.remove_unreferenced_vertices(v, c, f)
    assert torch.equal(v2, v[[2, 5, 7, 8]]) and torch.equal(c2, c[[2, 5, 7, 8]])
    assert f2.dtype == torch.int32 and f2.tolist() == [[2, 0, 1], [1, 0, 3]]
    v3, c3, f3 = mesh.remove_unreferenced_vertices(v, None, f[:0])
    assert v3.shape == (0, 3) and c3 is None and f3.shape == (0, 3)
    w, _, h = mt.post_process_mesh(v.numpy(), None, f.numpy(), cluster_to_keep=5, min_triangles=1)
    assert np.array_equal(w, v2.numpy()) and np.array_equal(h, f2.numpy())

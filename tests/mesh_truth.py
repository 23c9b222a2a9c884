"""Host truth of connected components and mesh clean-up (SPEC M22; 4.24), written from the definitions in plain
numpy / Python, a second, independent statement of (a) through scipy.sparse.csgraph.connected_components, and the cases the
CPU and GPU tests share.  Nothing here touches the library.  Every result is an integer array (or a gather of the input's
rows), so every comparison against it is exact."""
import numpy as np

import tsdf_truth as tt


# ---- (a) graph components ----
def components(n, a, b):
    """label [n] int64: label[x] = the smallest node of x's connected component.  A sequential union-find with union by
    smaller index (so a root is its tree's minimum) and path halving."""
    parent = list(range(int(n)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(x) for x in range(int(n))], dtype=np.int64).reshape(-1)


def components_scipy(n, a, b):
    """the same through scipy: its arbitrary component numbers mapped to each component's smallest node"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = int(n)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    g = coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(n, n))
    k, comp = connected_components(g, directed=False)
    smallest = np.full(k, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    return smallest[comp]


# ---- (b) triangle clusters ----
def pack_edge_key(u, v):
    """(min << 32) | max as int64, for int arrays or scalars of vertex indices in [0, 2^31)"""
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    return (np.minimum(u, v) << 32) | np.maximum(u, v)


def corner_keys(faces, connectivity="edge"):
    """(keys [3F] int64, face_of_key [3F]) in corner order c = 3 f + k"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    face_of_key = np.repeat(np.arange(len(f)), 3)
    if connectivity == "vertex":
        return f.reshape(-1), face_of_key
    assert connectivity == "edge"
    return pack_edge_key(f, np.roll(f, -1, axis=1)).reshape(-1), face_of_key


def face_labels(faces, connectivity="edge"):
    """label [F]: the smallest face index of each face's cluster — two faces are adjacent iff they hold one key in common"""
    keys, face = corner_keys(faces, connectivity)
    first = {}
    a, b = [], []
    for k, f in zip(keys.tolist(), face.tolist()):
        if k in first:
            a.append(first[k])
            b.append(f)
        else:
            first[k] = f
    return components(len(np.asarray(faces).reshape(-1, 3)), a, b)


def triangle_clusters(faces, connectivity="edge"):
    """(triangle_clusters [F], cluster_n_triangles [K]) int64: ids 0 .. K-1 in ascending order of the cluster's smallest face"""
    label = face_labels(faces, connectivity)
    roots = np.nonzero(label == np.arange(len(label)))[0]          # ascending
    cluster_of_root = np.full(len(label), -1, dtype=np.int64)
    cluster_of_root[roots] = np.arange(len(roots))
    clusters = cluster_of_root[label]
    return clusters, np.bincount(clusters, minlength=len(roots)).astype(np.int64)


# ---- (c) edge report ----
def edge_report(faces):
    """(boundary, manifold, non_manifold): distinct undirected edge keys with 1, 2 and more corner uses"""
    keys, _ = corner_keys(faces, "edge")
    _, uses = np.unique(keys, return_counts=True)
    return int((uses == 1).sum()), int((uses == 2).sum()), int((uses > 2).sum())


# ---- (d) selection ----
def select_clusters(counts, cluster_to_keep=50, min_triangles=50):
    counts = [int(c) for c in counts]
    threshold = int(min_triangles)
    if len(counts) > cluster_to_keep:
        threshold = max(threshold, sorted(counts, reverse=True)[cluster_to_keep - 1])
    return np.array([c >= threshold for c in counts], dtype=bool)


# ---- (e) post_process_mesh ----
def post_process_mesh(vertices, colours, faces, cluster_to_keep=50, min_triangles=50, connectivity="edge", remove_degenerate=True):
    """numpy restatement: (vertices, colours, faces) — rows of the inputs gathered, never recomputed"""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    clusters, counts = triangle_clusters(f, connectivity)
    keep = select_clusters(counts, cluster_to_keep, min_triangles)[clusters] if len(f) else np.zeros(0, dtype=bool)
    if remove_degenerate:
        keep = keep & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    f = f[keep]
    used = np.zeros(len(vertices), dtype=bool)
    used[f.reshape(-1)] = True
    renumber = np.cumsum(used) - 1
    return vertices[used], None if colours is None else colours[used], renumber[f]


# ---- shared cases ----
def path_graph(n, order, seed=0):
    """the n - 1 edges (i, i + 1) in ascending, descending or seeded shuffled order"""
    i = np.arange(n - 1)
    if order == "descending":
        i = i[::-1].copy()
    elif order == "shuffled":
        np.random.default_rng(seed).shuffle(i)
    else:
        assert order == "ascending"
    return n, i, i + 1


def star_graph(leaves, hub_last):
    n = leaves + 1
    hub = n - 1 if hub_last else 0
    leaf = np.arange(leaves) + (0 if hub_last else 1)
    return n, leaf, np.full(leaves, hub)


def random_graph(n, e, seed):
    g = np.random.default_rng(seed)
    return n, g.integers(0, n, e), g.integers(0, n, e)


GRAPH_NAMES = ("one node", "no edges", "self-loops", "duplicated", "path ascending", "path descending", "path shuffled",
               "star hub last", "star hub 0", "sparse 1", "sparse 2", "sparse 3", "giant 1", "giant 2", "giant 3", "ragged")
_GRAPHS = {}


def graph_case(name):
    """(N, a, b, label): a graph of graph_cases() with its truth, computed once"""
    if not _GRAPHS:
        _GRAPHS.update(graph_cases())
    if len(_GRAPHS[name]) == 3:
        _GRAPHS[name] = _GRAPHS[name] + (components(*_GRAPHS[name]),)
    return _GRAPHS[name]


def graph_cases():
    """{name: (N, a, b)}: every graph the GPU tests run — the CPU tests hold the two truths against each other on all of them"""
    cases = {"one node": (1, np.zeros(0, int), np.zeros(0, int)), "no edges": (5, np.zeros(0, int), np.zeros(0, int)),
             "self-loops": (7, np.arange(7), np.arange(7))}
    n, a, b = random_graph(300, 200, 5)
    cases["duplicated"] = (n, np.concatenate([a, b, a]), np.concatenate([b, a, b]))
    for order in ("ascending", "descending", "shuffled"):
        cases[f"path {order}"] = path_graph(100003, order, seed=11)
    cases["star hub last"] = star_graph(50000, True)
    cases["star hub 0"] = star_graph(50000, False)
    for seed in (1, 2, 3):
        cases[f"sparse {seed}"] = random_graph(20000, 8000, seed)
        cases[f"giant {seed}"] = random_graph(20000, 40000, 100 + seed)
    cases["ragged"] = random_graph(5000, 3 * 256 + 64 + 37, 9)       # E = 869: no multiple of 64 or 256
    return cases


TET = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]])        # a closed tetrahedron on vertices 0..3, outward


def hand_meshes():
    """{name: (faces [F,3], n_vertices)}"""
    shared_vertex = np.concatenate([TET, np.where(TET == 0, 3, TET + 3)])              # vertices 3..6: 3 is shared
    # two tetrahedra on the edge {0, 1}, (0,1,2,3) and (0,1,4,5): the edge is used by four faces
    second = np.array([[0, 4, 1], [0, 1, 5], [1, 4, 5], [4, 0, 5]])
    return {"two tetrahedra": (np.concatenate([TET, TET + 4]), 8),
            "shared vertex": (shared_vertex, 7),
            "shared edge": (np.concatenate([TET, second]), 6),
            "one triangle": (np.array([[0, 1, 2]]), 3),
            "tetrahedron": (TET.copy(), 4),
            "repeated index": (np.concatenate([TET, [[3, 3, 4]], TET + 5]), 9),
            "unused vertices": (np.concatenate([TET + 2, TET + 9]), 20)}


# the planted volume of the tests: the minimum of three sphere distances — two bodies well apart and a floater off the symmetry
# planes, in tt.empty_volume(1/16, 4/16, 10, ((-1,)*3, (1,)*3))
SPHERES = (((-0.45, 0.05, 0.02), 0.35), ((0.47, -0.04, -0.03), 0.36), ((0.03, 0.63, 0.41), 0.12))


def planted_volume(colour=True):
    import torch
    geometry = tt.empty_volume(1.0 / 16, 4.0 / 16, 10.0, ((-1,) * 3, (1,) * 3), colour=colour)

    def field(p):
        d = [(p - torch.tensor(c, dtype=torch.float64)).norm(dim=1) - r for c, r in SPHERES]
        return torch.stack(d).min(dim=0).values

    blocks = [(x, y, z) for z in range(geometry["blocks"][2]) for y in range(geometry["blocks"][1])
              for x in range(geometry["blocks"][0])]
    colour_field = (lambda p: 0.5 + 0.25 * torch.sin(3.0 * p)) if colour else None
    return tt.planted(geometry, blocks, field, colour_field)


_PLANTED = {}


def planted_mesh():
    """(vertices [V,3] float64, faces [F,3] int64) of tsdf_truth.extract on the planted volume, unreferenced vertices dropped;
    computed once"""
    if "mesh" not in _PLANTED:
        v, _, f = tt.extract(planted_volume(colour=False))
        _PLANTED["mesh"] = tt.drop_unreferenced(v, f)
    return _PLANTED["mesh"]

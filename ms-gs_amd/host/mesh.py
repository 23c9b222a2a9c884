"""Mesh clean-up behind TSDF extraction (4.24): what 2DGS's post_process_mesh does with Open3D's
cluster_connected_triangles(), remove_degenerate_triangles() and remove_unreferenced_vertices(), on the GPU and without Open3D.

    vertices, colours, faces = post_process_mesh(*vol.extract_mesh())          keeps the 50 largest clusters of >= 50 triangles
    clusters, counts = cluster_connected_triangles(faces, len(vertices))
    report = edge_report(faces, len(vertices))                                 boundary / manifold / non-manifold edge counts

A cluster is a connected component of the faces under shared undirected edges (Open3D's rule, the default) or shared vertices.
The components come from a union-find that is written by atomicMin only: every face's label is the smallest face index of its
cluster, which the input alone defines, so clusters, counts and the cleaned mesh have the same bits on every run.  Cluster area,
smoothing, decimation, vertex normals and merging of duplicate vertices (the TSDF mesh is welded already) are not here.
Nothing here is differentiable.
"""
from typing import NamedTuple

import torch
from diff_gaussian_rasterization import mesh_edge_report, mesh_triangle_clusters


class EdgeReport(NamedTuple):
    boundary: int                  # undirected edges used by exactly one face
    manifold: int                  # ... by exactly two
    non_manifold: int              # ... by more than two


def cluster_connected_triangles(faces, n_vertices, connectivity="edge"):
    """(triangle_clusters [F] int32, cluster_n_triangles [K] int32): Open3D's cluster_connected_triangles() without the areas.
    Clusters are numbered in ascending order of their smallest face index, as Open3D numbers them in "edge" mode."""
    return mesh_triangle_clusters(faces, n_vertices, connectivity)


def edge_report(faces, n_vertices):
    """EdgeReport of faces [F,3]: a mesh is closed iff boundary == 0 and a manifold iff non_manifold == 0 as well"""
    return EdgeReport(*mesh_edge_report(faces, n_vertices))


def select_clusters(cluster_n_triangles, cluster_to_keep=50, min_triangles=50):
    """bool [K]: the clusters 2DGS's post_process_mesh keeps — those of at least threshold = max(min_triangles, the
    cluster_to_keep-th largest count) triangles; ties at the threshold are all kept.  With K <= cluster_to_keep the threshold is
    min_triangles (2DGS raises an IndexError for K < cluster_to_keep).  Pure torch on the tensor's device, no host read."""
    counts = cluster_n_triangles
    if not torch.is_tensor(counts) or counts.dim() != 1 or counts.dtype not in (torch.int32, torch.int64):
        raise ValueError("select_clusters: cluster_n_triangles must be an int32 or int64 tensor [K]")
    k = int(cluster_to_keep)
    if k < 1:
        raise ValueError(f"select_clusters: cluster_to_keep = {cluster_to_keep} must be at least 1")
    threshold = torch.full((), int(min_triangles), dtype=torch.int64, device=counts.device)
    if counts.shape[0] > k:
        threshold = torch.maximum(threshold, torch.topk(counts.long(), k).values[k - 1])
    return counts >= threshold


def remove_unreferenced_vertices(vertices, colours, faces):
    """(vertices, colours, faces) without the vertices no face uses, the faces renumbered, both in their order — the rule of
    TSDFVolume.extract_mesh(drop_unreferenced=True).  colours may be None.  One host read: the number of vertices left."""
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=vertices.device)
    used[faces.reshape(-1).long()] = True
    renumber = (torch.cumsum(used, 0) - 1).to(torch.int32)
    return vertices[used], None if colours is None else colours[used], renumber[faces.long()].reshape(-1, 3)


@torch.no_grad()
def post_process_mesh(vertices, colours, faces, cluster_to_keep=50, min_triangles=50, connectivity="edge", remove_degenerate=True):
    """(vertices [V',3], colours [V',3] or None, faces [F',3] int32): the mesh without the faces of the clusters that
    select_clusters() drops, without the faces that repeat an index (remove_degenerate) and then without the vertices no face
    uses any more; the survivors keep their order and their bits.  The host reads the cluster count and the two surviving
    sizes (and, once, the index range of `faces`)."""
    if not torch.is_tensor(vertices) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("post_process_mesh: vertices must be a tensor [V,3]")
    if colours is not None and (not torch.is_tensor(colours) or colours.shape[0] != vertices.shape[0]):
        raise ValueError("post_process_mesh: colours must be None or a tensor with one row per vertex")
    clusters, counts = mesh_triangle_clusters(faces, vertices.shape[0], connectivity)
    keep = select_clusters(counts, cluster_to_keep, min_triangles)[clusters.long()]
    if remove_degenerate:
        a, b, c = faces[:, 0], faces[:, 1], faces[:, 2]
        keep = keep & (a != b) & (b != c) & (c != a)
    return remove_unreferenced_vertices(vertices, colours, faces[keep].to(torch.int32))

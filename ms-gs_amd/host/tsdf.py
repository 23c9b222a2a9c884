"""TSDF fusion of rendered depth maps into a triangle mesh (4.22): what 2DGS and RaDe-GS do with Open3D's
ScalableTSDFVolume.integrate() and extract_triangle_mesh(), on the GPU and without Open3D.

    vol = TSDFVolume(voxel_size, depth_trunc=..., bounds=((x0, y0, z0), (x1, y1, z1)))
    vol.integrate_views(cameras, pc, pipe, bg)            renders median depth and colour of every view and fuses them
    vol.integrate(depth, cameras, colour, weight)         ... or fuses maps that exist already
    vertices, colours, faces = vol.extract_mesh()
    vertices, colours, faces = post_process_mesh(*vol.extract_mesh())     ... without floaters (host/mesh.py, M22)
    model_io.write_mesh_ply(path, vertices, faces, colours)

The volume is a table of 8x8x8 blocks over `bounds` (at most 256 per axis) with a pool of the blocks near a surface.  It stores
the SUMS of w tsdf, w and w colour, so fusing views one by one, in batches or all at once leaves the same bits, and extraction
reads the sign of the TSDF from the sign of the stored sum.  Extraction is marching tetrahedra (six Kuhn tetrahedra per cube):
the mesh is indexed, welded and closed wherever the field is observed, with normals towards free space, and has the same bits
on every run.  Nothing here is differentiable.
"""
import math

import numpy as np
import torch
from diff_gaussian_rasterization import (TSDF_CAMERA_CHUNK, TSDF_MAX_BLOCKS_PER_AXIS, TSDF_MAX_SLOTS, tsdf_allocate, tsdf_extract,
                                         tsdf_integrate)

BLOCK = 8
BLOCK_POINTS = BLOCK ** 3


def volume_geometry(voxel_size, bounds):
    """(voxel_size rounded to float32, origin (3 float32 values), blocks (NBx, NBy, NBz)) of a volume over `bounds`; refuses an
    empty box and more than TSDF_MAX_BLOCKS_PER_AXIS blocks along an axis"""
    voxel = float(np.float32(voxel_size))
    if not (voxel > 0.0 and math.isfinite(voxel)):
        raise ValueError("TSDFVolume: voxel_size must be positive and finite")
    lo, hi = (np.asarray(b, dtype=np.float64).reshape(3) for b in bounds)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError(f"TSDFVolume: bounds must be a finite box (lo, hi) with hi > lo, got {bounds}")
    origin = tuple(float(np.float32(x)) for x in lo)
    blocks = tuple(int(math.ceil((h - o) / (BLOCK * voxel) - 1e-9)) for h, o in zip(hi, origin))
    if max(blocks) > TSDF_MAX_BLOCKS_PER_AXIS:
        raise ValueError(f"TSDFVolume: bounds {bounds} at voxel_size {voxel:g} need {blocks} blocks of {BLOCK} voxels; at most "
                         f"{TSDF_MAX_BLOCKS_PER_AXIS} per axis are supported — use a larger voxel or a smaller box")
    return voxel, origin, tuple(max(b, 1) for b in blocks)


class TSDFVolume:
    def __init__(self, voxel_size, sdf_trunc=None, *, depth_trunc, bounds, colour=True, device="cuda"):
        """voxel_size: lattice spacing; sdf_trunc: truncation distance (default 5 voxel_size); depth_trunc: depth pixels beyond
        it are no surface samples; bounds: (lo, hi) of the box the table covers; colour: also fuse colour maps."""
        self.voxel_size, self.origin, self.blocks = volume_geometry(voxel_size, bounds)
        self.sdf_trunc = float(np.float32(5.0 * self.voxel_size if sdf_trunc is None else sdf_trunc))
        if not (self.sdf_trunc > 0.0 and math.isfinite(self.sdf_trunc)):
            raise ValueError("TSDFVolume: sdf_trunc must be positive and finite")
        self.depth_trunc = float(depth_trunc)
        if not self.depth_trunc > 0.0:
            raise ValueError("TSDFVolume: depth_trunc must be positive")
        self.device = torch.device(device)
        self.has_colour = bool(colour)
        self._reset(0)

    def _reset(self, S):
        dev, f32 = self.device, torch.float32
        self.table = torch.full(self.blocks[::-1], -1, dtype=torch.int32, device=dev)
        self.slot_block = torch.zeros(S, dtype=torch.int32, device=dev)
        self.tsdf_sum = torch.zeros(S, BLOCK_POINTS, dtype=f32, device=dev)
        self.weight_sum = torch.zeros(S, BLOCK_POINTS, dtype=f32, device=dev)
        self.colour_sum = torch.zeros(S, 3, BLOCK_POINTS, dtype=f32, device=dev) if self.has_colour else None

    @property
    def num_blocks(self):
        return int(self.slot_block.shape[0])

    def _append(self, new_blocks):
        """new pool slots, zeroed, for the ascending linear block indices `new_blocks` (int64, on the device)"""
        n, S = int(new_blocks.shape[0]), self.num_blocks
        if n == 0:
            return
        if S + n > TSDF_MAX_SLOTS:
            raise ValueError(f"TSDFVolume: {S + n} active blocks, at most {TSDF_MAX_SLOTS} are supported — use a larger voxel")
        self.table.view(-1)[new_blocks] = torch.arange(S, S + n, dtype=torch.int32, device=self.device)
        grow = lambda t: torch.cat([t, t.new_zeros((n,) + tuple(t.shape[1:]))])
        self.slot_block = torch.cat([self.slot_block, new_blocks.to(torch.int32)])
        self.tsdf_sum, self.weight_sum = grow(self.tsdf_sum), grow(self.weight_sum)
        if self.has_colour:
            self.colour_sum = grow(self.colour_sum)

    @torch.no_grad()
    def integrate(self, depth, cameras, colour=None, weight=None):
        """Fuses depth [n,H,W] seen by `cameras` (n objects with world_view_transform, FoVx, FoVy, image_width, image_height,
        all of one size) with colour [n,3,H,W] (needed iff the volume stores colour) and weight [n,H,W] (default 1).  Blocks
        near the new surface samples are activated first; taking their list (torch.nonzero) is the call's one host read."""
        cameras = cameras if torch.is_tensor(cameras) else list(cameras)
        marks = tsdf_allocate(self, depth, cameras, self.sdf_trunc, self.depth_trunc)
        self._append(torch.nonzero(marks.view(-1).bool() & (self.table.view(-1) < 0)).view(-1))
        tsdf_integrate(self, depth, cameras, self.sdf_trunc, self.depth_trunc, colour=colour, weight=weight)

    @torch.no_grad()
    def integrate_views(self, cameras, pc, pipe, bg, depth="median"):
        """Renders every camera and fuses the maps, TSDF_CAMERA_CHUNK views per integrate() call (consecutive cameras of one
        image size share a call).  depth="median": render_with_median_depth's map with weight 1 — the depth of one Gaussian
        per ray, which does not smear across silhouettes; depth="expected": render_with_alpha's blended depth over
        alpha.clamp_min(1e-8) with weight alpha."""
        from gaussian_renderer import render_with_alpha, render_with_median_depth
        if depth not in ("median", "expected"):
            raise ValueError(f"integrate_views: depth must be 'median' or 'expected', not {depth!r}")
        batch, maps = [], []

        def flush():
            if batch:
                d, c, w = (None if m[0] is None else torch.stack(m) for m in zip(*maps))
                self.integrate(d, batch, colour=c if self.has_colour else None, weight=w)
            batch.clear()
            maps.clear()

        for cam in cameras:
            if batch and (len(batch) == TSDF_CAMERA_CHUNK or (cam.image_width, cam.image_height) !=
                          (batch[0].image_width, batch[0].image_height)):
                flush()
            if depth == "median":
                out = render_with_median_depth(cam, pc, pipe, bg)
                d, w = out["median_depth"], None
            else:
                out = render_with_alpha(cam, pc, pipe, bg)
                w = out["alpha"]
                d = out["depth"].reshape(w.shape) / w.clamp_min(1e-8)
            batch.append(cam)
            maps.append((d.detach(), out["render"].detach() if self.has_colour else None, None if w is None else w.detach()))
        flush()

    @torch.no_grad()
    def extract_mesh(self, drop_unreferenced=True):
        """(vertices [V,3] float32, colours [V,3] float32 or None, faces [F,3] int32).  drop_unreferenced removes the vertices
        no face uses (crossings next to unobserved lattice points) and renumbers the faces; the order is kept."""
        vertices, colours, faces = tsdf_extract(self)
        if drop_unreferenced and vertices.shape[0]:
            used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=vertices.device)
            used[faces.reshape(-1).long()] = True
            renumber = (torch.cumsum(used, 0) - 1).to(torch.int32)
            vertices, faces = vertices[used], renumber[faces.long()]
            colours = None if colours is None else colours[used]
        return vertices, colours, faces

    def state_dict(self):
        """geometry, the active blocks' coordinates [S,3] (bx, by, bz) in slot order, and their sums — on the host"""
        b = self.slot_block.long().cpu()
        nx, ny = self.blocks[0], self.blocks[1]
        coords = torch.stack([b % nx, (b // nx) % ny, b // (nx * ny)], dim=1).to(torch.int32)
        cpu = lambda t: None if t is None else t.detach().cpu().clone()
        return {"voxel_size": self.voxel_size, "sdf_trunc": self.sdf_trunc, "depth_trunc": self.depth_trunc,
                "origin": tuple(self.origin), "blocks": tuple(self.blocks), "block_coords": coords,
                "tsdf_sum": cpu(self.tsdf_sum), "weight_sum": cpu(self.weight_sum), "colour_sum": cpu(self.colour_sum)}

    def load_state_dict(self, state):
        """replaces geometry, blocks and sums by those of `state` (state_dict(), or a synthetic field of the same layout)"""
        blocks = tuple(int(b) for b in state["blocks"])
        if len(blocks) != 3 or min(blocks) < 1 or max(blocks) > TSDF_MAX_BLOCKS_PER_AXIS:
            raise ValueError(f"TSDFVolume: {blocks} blocks, 1 .. {TSDF_MAX_BLOCKS_PER_AXIS} per axis are supported")
        coords = torch.as_tensor(state["block_coords"]).long().reshape(-1, 3)
        S = int(coords.shape[0])
        if S > TSDF_MAX_SLOTS:
            raise ValueError(f"TSDFVolume: {S} active blocks, at most {TSDF_MAX_SLOTS} are supported")
        if S and (bool((coords < 0).any()) or bool((coords >= torch.tensor(blocks)).any())):
            raise ValueError("TSDFVolume: block_coords outside the table")
        linear = (coords[:, 2] * blocks[1] + coords[:, 1]) * blocks[0] + coords[:, 0]
        if torch.unique(linear).numel() != S:
            raise ValueError("TSDFVolume: block_coords holds a block twice")
        for k, shape in (("tsdf_sum", (S, BLOCK_POINTS)), ("weight_sum", (S, BLOCK_POINTS))):
            if tuple(state[k].shape) != shape:
                raise ValueError(f"TSDFVolume: {k} must be {shape}")
        self.voxel_size = float(np.float32(state["voxel_size"]))
        self.sdf_trunc, self.depth_trunc = float(np.float32(state["sdf_trunc"])), float(state["depth_trunc"])
        self.origin, self.blocks = tuple(float(np.float32(x)) for x in state["origin"]), blocks
        self.has_colour = state.get("colour_sum") is not None
        self._reset(S)
        dev = self.device
        self.slot_block = linear.to(torch.int32).to(dev)
        self.table.view(-1)[linear.to(dev)] = torch.arange(S, dtype=torch.int32, device=dev)
        self.tsdf_sum = state["tsdf_sum"].float().contiguous().to(dev).clone()
        self.weight_sum = state["weight_sum"].float().contiguous().to(dev).clone()
        if self.has_colour:
            if tuple(state["colour_sum"].shape) != (S, 3, BLOCK_POINTS):
                raise ValueError(f"TSDFVolume: colour_sum must be {(S, 3, BLOCK_POINTS)}")
            self.colour_sum = state["colour_sum"].float().contiguous().to(dev).clone()
        return self

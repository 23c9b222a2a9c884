"""Normal maps (SPEC M17) without a GPU: the float64 truth of tests/normals_truth.py against independent
statements of its definitions and against the conditions the GPU tests rely on, and the surface — the C ABI's symbols and
argument checks, the Python entries' refusals, the host route's signature."""
import ctypes as C
import inspect
import math
import os
import re
import types

import pytest
import torch

import normals_truth as nt
import scenes
from oracle import torch_oracle as to
from parity_utils import small_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msgs_gaussian_normals_forward", "msgs_gaussian_normals_backward", "msgs_depth_normal_forward",
         "msgs_depth_normal_backward")
TILE_W, TILE_H = 64, 8
FLAGGED_CAP = 0.01
E2E_SCENE = dict(P=300, W=64, H=48, seed=41)          # = tests/test_normals_gpu.py


def _settings(W=5, H=4, cam=None):
    import diff_gaussian_rasterization as dgr
    cam = cam or scenes.front_camera(W, H)
    return dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=nt.TANFOV[0], tanfovy=nt.TANFOV[1], bg=torch.zeros(3), scale_modifier=1.0,
        viewmatrix=cam.world_view_transform, projmatrix=cam.full_proj_transform, sh_degree=0, campos=cam.camera_center,
        prefiltered=False, debug=False)


# ---------------------------------------------------------------------------------------------------------------------------
# the definitions
# ---------------------------------------------------------------------------------------------------------------------------
def test_rotation_matrix_is_the_oracles():
    g = torch.Generator().manual_seed(1)
    q = torch.randn(500, 4, generator=g, dtype=torch.float64)
    for qq in (q, nt.normalise(q)):                          # the entries agree for any q, of unit length or not
        assert torch.allclose(nt.rotation_matrix(qq), to.quat_to_rot(qq), rtol=0, atol=1e-14 * float(qq.abs().max()) ** 2)
    R = nt.rotation_matrix(nt.normalise(q))
    assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(500, 3, 3), atol=1e-13)


def test_the_normal_is_the_eigenvector_of_the_smallest_eigenvalue_of_sigma():
    """pins column-versus-row: Sigma = R S^2 R^T of the oracle has the eigenvector R[:, k] for s_k^2"""
    m, s, r, _ = nt.gaussian_rows(257, raw=False)
    cam = nt.camera()
    t = nt.gaussian_normals(m, s, r, cam.world_view_transform, cam.camera_center, world=True)
    packed = to.cov3d_from_scale_rot(s.double(), nt.normalise(r.double()), 1.0)
    S = torch.stack([packed[:, 0], packed[:, 1], packed[:, 2], packed[:, 1], packed[:, 3], packed[:, 4], packed[:, 2],
                     packed[:, 4], packed[:, 5]], dim=1).view(-1, 3, 3)
    w, vec = torch.linalg.eigh(S)                            # ascending
    smallest = vec[:, :, 0]
    assert torch.allclose(w[:, 0], s.double().min(dim=1).values ** 2, rtol=1e-6)
    n = t["normal"]
    assert ((n * smallest).sum(dim=1).abs() >= 1 - 1e-7).all()
    assert torch.allclose(n.norm(dim=1), torch.ones(257, dtype=torch.float64), atol=1e-12)
    # ... turned towards the camera, and the view-space vector is the same one rotated
    d = cam.camera_center.double()[None] - m.double()
    assert ((n * d).sum(dim=1) >= 0).all() and (t["sigma"] < 0).any() and (t["sigma"] > 0).any()
    view = nt.gaussian_normals(m, s, r, cam.world_view_transform, cam.camera_center)["normal"]
    assert torch.allclose(view, n @ cam.world_view_transform.double()[:3, :3], atol=1e-14)


def test_axis_selection_ties_and_exceptional_rows():
    s = torch.tensor([[2.0, 1.0, 1.0], [1.0, 1.0, 1.0], [3.0, 2.0, 1.0], [1.0, 2.0, 1.0], [2.0, 1.0, 3.0]])
    assert nt.shortest_axis(s).tolist() == [1, 0, 2, 0, 1]
    assert torch.equal(nt.shortest_axis(torch.log(s)), nt.shortest_axis(s))
    cam = nt.camera()
    m = torch.zeros(4, 3)
    r = torch.tensor([[1.0, 0, 0, 0], [0.0, 0, 0, 0], [float("nan"), 0, 0, 0], [3e-13, 4e-13, 0, 0]])
    t = nt.gaussian_normals(m, s[:4], r, cam.world_view_transform, cam.camera_center, world=True)
    assert torch.isfinite(t["normal"]).all() and t["valid"].tolist() == [True, True, False, True]
    assert torch.equal(t["normal"][2], torch.zeros(3, dtype=torch.float64))
    assert torch.equal(t["normal"][0].abs(), torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64))


@pytest.mark.parametrize("shape", [(3, 3), (7, 11), (19, 133)])
@pytest.mark.parametrize("plane", [(0.0, 0.0, -1.0), (0.28, -0.19, -0.94), (-0.5, 0.4, -0.7)])
def test_depth_to_normal_of_an_analytic_plane(shape, plane):
    """every stencil of a plane lies in it: the normal is the plane's own, facing the camera; fx != fy"""
    H, W = shape
    n = torch.tensor(plane, dtype=torch.float64)
    n = n / n.norm()
    z = nt.plane_depth(W, H, nt.TANFOV[0], nt.TANFOV[1], n, -5.0)
    assert (z > 0).all()
    got, valid = nt.depth_to_normal(z, *nt.TANFOV)
    assert valid[1:-1, 1:-1].all() and not valid[0].any() and not valid[-1].any() and not valid[:, 0].any() and not valid[:, -1].any()
    assert (got[:, valid] - n[:, None]).abs().max() <= 1e-9
    assert torch.equal(got[:, ~valid], torch.zeros(3, int((~valid).sum()), dtype=torch.float64))
    if plane[0] == 0.0:
        assert (got[2, valid] == -1.0).all()
    cam = nt.camera()
    world, _ = nt.depth_to_normal(z, *nt.TANFOV, viewmatrix=cam.world_view_transform)
    R = cam.world_view_transform.double()[:3, :3]
    assert (world[:, valid] - (R @ n)[:, None]).abs().max() <= 1e-9
    # the world normal rotated back into view space by gaussian_normals' map is the view normal (the camera's matrix is
    # float32: orthonormal to a few 2^-24)
    assert ((R.T @ world[:, valid]) - got[:, valid]).abs().max() <= 1e-6


def test_depth_to_normal_holes_invalidate_their_four_neighbours_only():
    z = nt.depth_map(9, 11).double()
    base, base_valid = nt.depth_to_normal(z, *nt.TANFOV)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        zz = z.clone().requires_grad_(True)
        with torch.no_grad():
            zz[4, 5] = bad
        n, valid = nt.depth_to_normal(zz, *nt.TANFOV)
        want = base_valid.clone()
        for y, x in ((3, 5), (5, 5), (4, 4), (4, 6)):
            want[y, x] = False
        assert torch.equal(valid, want) and valid[4, 5]                  # the centre's own depth does not enter
        assert torch.equal(n[:, want], base[:, want])
        n.sum().backward()
        assert torch.isfinite(zz.grad).all() and zz.grad[4, 5] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# the conditions the GPU tests rely on, met by the truth alone
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("P", nt.GAUSSIAN_P)
def test_gpu_scenes_have_few_flagged_rows(P, raw):
    m, s, r, _ = nt.gaussian_rows(P, raw)
    cam = nt.camera()
    t = nt.gaussian_normals(m, s, r, cam.world_view_transform, cam.camera_center)
    assert t["valid"].all() and t["flagged"].float().mean().item() <= FLAGGED_CAP
    assert len(set(t["k"].tolist())) == min(P, 3) or P < 20             # every axis is selected somewhere


def test_the_same_axis_test_has_no_near_ties():
    """log-scales, their exp and the filtered scales of the GPU test's 4099 rows keep their two smallest entries at least
    5e-6 apart (relative; 40 float32 ulp): no rounding of exp or sqrt can reorder them"""
    _, logs, _, _ = nt.gaussian_rows(4099, raw=True)
    s = torch.exp(logs.double())
    for v in (logs.double(), s, torch.sqrt(s * s + nt.AXIS_TEST_FILTER ** 2)):
        srt = v.sort(dim=1).values
        assert ((srt[:, 1] - srt[:, 0]) / srt[:, 1].abs()).min().item() >= 5e-6
        assert torch.equal(nt.shortest_axis(v), nt.shortest_axis(logs.double()))


def test_end_to_end_scene_has_few_flagged_rows():
    sc, cam = small_scene(E2E_SCENE["P"], E2E_SCENE["W"], E2E_SCENE["H"], E2E_SCENE["seed"])
    t = nt.gaussian_normals(sc.means3D, sc.scales, sc.rotations, cam.world_view_transform, cam.camera_center)
    assert t["flagged"].float().mean().item() <= FLAGGED_CAP


@pytest.mark.parametrize("shape", nt.depth_shapes(TILE_W, TILE_H))
def test_float32_restatement_of_depth_to_normal(shape):
    """the relief is rough enough: float32 differences of neighbouring depths keep the normal within 1e-4 of float64"""
    H, W = shape
    z = nt.depth_map(H, W)
    assert (z > 0).all()
    t = nt.depth_truth(z, scenes.grad_seed(W, H, 5) * (W * H))
    print(f"[normals] {H}x{W}: restatement forward {t['restated']:.3e} backward {t['restated_bwd']:.3e}")
    assert t["same_valid"] and t["restated"] <= 1e-4
    assert t["valid"].sum().item() == max(H - 2, 0) * max(W - 2, 0)


# ---------------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _backend as B
    header = open(os.path.join(ROOT, "include", "msgs.h")).read()
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, header), n
        assert n in B.EXPORTS and callable(getattr(B.lib, n)) and getattr(B.lib, n).restype is C.c_int
    nargs = {n: len(re.search(r"\bint %s\(([^;]*)\);" % n, header).group(1).split(",")) for n in NAMES}
    assert nargs == {NAMES[0]: 10, NAMES[1]: 8, NAMES[2]: 9, NAMES[3]: 10}
    for n in NAMES:
        assert len(getattr(B.lib, n).argtypes) == nargs[n], n
    assert B.ABI_VERSION == 11 and B.lib.msgs_abi_version() == 11
    assert int(re.search(r"#define MSGS_DEPTH_NORMAL_TILE_W (\d+)", header).group(1)) == dgr.DEPTH_NORMAL_TILE_W == TILE_W
    assert int(re.search(r"#define MSGS_DEPTH_NORMAL_TILE_H (\d+)", header).group(1)) == dgr.DEPTH_NORMAL_TILE_H == TILE_H
    for n in ("gaussian_normals", "depth_to_normal", "DEPTH_NORMAL_TILE_W", "DEPTH_NORMAL_TILE_H"):
        assert n in dgr.__all__
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(dgr.gaussian_normals) == ["means3D", "scales", "rotations", "raster_settings", "world"]
    assert sig(dgr.depth_to_normal) == ["depth", "raster_settings", "world"]
    assert "csrc/normals.hip" in open(os.path.join(ROOT, "ms-gs_amd", "Makefile")).read()


def test_argument_checks_of_the_c_entries():
    """NULL or misaligned pointers and negative sizes are refused before anything is launched (no GPU is touched)"""
    from diff_gaussian_rasterization import _backend as B
    lib = B.lib
    p, odd = C.c_void_p(256), C.c_void_p(260)                              # never dereferenced: every call below is refused
    fwd = lambda P=10, m=p, s=p, r=p, vm=p, cp=p, n=p, f=p: lib.msgs_gaussian_normals_forward(P, m, s, r, vm, cp, 0, n, f, None)
    assert fwd(P=-1) == -1 and fwd(r=odd) == -1
    assert fwd(P=0, m=None, s=None, r=None, vm=None, cp=None, n=None, f=None) == 0
    for k in ("m", "s", "r", "vm", "cp", "n", "f"):
        assert fwd(**{k: None}) == -1, k
    bwd = lambda P=10, r=p, f=p, vm=p, world=0, g=p, d=p: lib.msgs_gaussian_normals_backward(P, r, f, vm, world, g, d, None)
    assert bwd(P=-1) == -1 and bwd(P=0, r=None, f=None, g=None, d=None) == 0 and bwd(r=odd) == -1 and bwd(d=odd) == -1
    for k in ("r", "f", "vm", "g", "d"):
        assert bwd(**{k: None}) == -1, k
    dn = lambda W=8, H=6, z=p, vm=p, world=1, n=p: lib.msgs_depth_normal_forward(W, H, 0.5, 0.5, z, vm, world, n, None)
    assert dn(W=-1) == -1 and dn(H=-1) == -1 and dn(W=0, z=None, n=None) == 0 and dn(H=0, z=None, n=None) == 0
    assert dn(W=1 << 20, H=1 << 20) == -1
    for k in ("z", "vm", "n"):
        assert dn(**{k: None}) == -1, k
    db = lambda W=8, H=6, z=p, vm=p, world=1, g=p, d=p: lib.msgs_depth_normal_backward(W, H, 0.5, 0.5, z, vm, world, g, d, None)
    assert db(W=-1) == -1 and db(H=0, z=None, g=None, d=None) == 0 and db(W=1 << 20, H=1 << 20) == -1
    for k in ("z", "vm", "g", "d"):
        assert db(**{k: None}) == -1, k


def test_python_entries_refuse_bad_input_before_any_launch():
    import diff_gaussian_rasterization as dgr
    calls = []
    prev, dgr._normals_probe = dgr._normals_probe, calls.append
    try:
        z = lambda *s: torch.zeros(*s)
        rs = _settings(5, 4)
        for m, s, r in ((z(5, 3), z(4, 3), z(5, 4)), (z(5, 3), z(5, 3), z(4, 4)), (z(5, 3), z(5, 3), z(5, 3)), (z(5, 2), z(5, 3), z(5, 4)),
                        (z(5, 3), z(5), z(5, 4))):
            with pytest.raises(ValueError):
                dgr.gaussian_normals(m, s, r, rs)
        for d in (z(5, 4), z(4), z(2, 4, 5), z(3, 5)):
            with pytest.raises(ValueError):
                dgr.depth_to_normal(d, rs)
        with pytest.raises(RuntimeError, match="HIP device"):
            dgr.gaussian_normals(z(5, 3), z(5, 3), z(5, 4), rs)
        with pytest.raises(RuntimeError, match="HIP device"):
            dgr.depth_to_normal(z(4, 5), rs)
        assert calls == []
    finally:
        dgr._normals_probe = prev


def test_host_route_surface():
    import gaussian_renderer as gr
    import normals
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(normals.render_with_normals) == sig(gr.render) + ["fused", "depth", "world"]
    d = inspect.signature(normals.render_with_normals).parameters
    assert d["depth"].default == "median" and d["world"].default is False and d["fused"].default is False
    pc = types.SimpleNamespace(filter_3D=torch.zeros(3, 1), get_xyz=torch.zeros(3, 3), active_sh_degree=0)
    pipe = types.SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False)
    cam = scenes.front_camera(40, 24)
    with pytest.raises(ValueError, match="depth"):
        normals.render_with_normals(cam, pc, pipe, torch.zeros(3), depth="mean")
    with pytest.raises(ValueError, match="filter_3D"):
        normals.render_with_normals(cam, pc, pipe, torch.zeros(3), fused=True)
    # 2DGS's term in plain torch: 0 where the two maps agree, 2 alpha where they are opposite
    g = torch.Generator().manual_seed(2)
    n = torch.nn.functional.normalize(torch.randn(3, 6, 7, generator=g), dim=0)
    alpha = torch.rand(6, 7, generator=g)
    out = dict(normal=(alpha * n).requires_grad_(True), surf_normal=n.clone().requires_grad_(True), alpha=alpha.clone().requires_grad_(True))
    loss = normals.normal_consistency(out)
    assert abs(loss.item() - (1.0 - alpha * alpha).mean().item()) < 1e-6
    loss.backward()
    assert out["alpha"].grad is None and out["normal"].grad is not None and out["surf_normal"].grad is not None
    out["surf_normal"] = -n
    assert abs(normals.normal_consistency(out).item() - (1.0 + alpha * alpha).mean().item()) < 1e-6

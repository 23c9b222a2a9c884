"""Bilateral-grid colour correction on the GPU (SPEC M19; include/msgs.h msgs_bilagrid_*).

References, none of them the kernels under test:
  1  tests/bilagrid_truth.py (float64, written from the definition; pinned to F.grid_sample by tests/test_bilagrid_cpu.py),
     gradients by float64 autograd;
  2  render() — bit for bit — for the composition.
Tolerances.  Forward: max(1e-6, 4 x the error of the float32 restatement of the same formulas on the same inputs), the rule of
tests/test_filter3d_gpu.py.  Both gradients: BWD_RTOL in max-norm; dL/dimage on unflagged pixels only (a pixel whose guide lies
within 1e-5 of a plane of the grid, at most 0.5 % of a scene: float32 may land in the neighbouring cell), the forward and dL/dgrid
everywhere.  Total variation: 1e-6 relative.  Every case runs twice and must repeat bit for bit.  The measured maxima are printed
(pytest -s) and recorded in profiles/bilagrid_notes.md.

The cases (tests/bilagrid_truth.py CASES), with T the tile of the slice kernels and 16 xy nodes in a tile's LDS window: 1x1 and
the exposure grid (one node), 64x64 under 2x2x2 and 200x130 under 4x3x5 (windows of 2-4 nodes per axis, odd sizes, scalar rows),
37x23 and 300x17 under 16x16x8 (a tile spans up to 16x16 / 5x16 nodes: the path that reads the grid from global memory),
(2 T_W + 1) x (T_H + 1) under 3x2x8 (tiles of one column and one row, a row length that is no multiple of 4) and 1920x16 under
16x16x8 (the training geometry along x: 128-pixel cells, 16-byte rows; its 16 rows cross all 16 planes in y, so it reads global
memory too — the LDS window with 16-byte rows is the 64x64 case)."""
import functools

import pytest
import torch

import bilagrid_truth as bt
import diff_gaussian_rasterization as dgr
import scenes
from parity_utils import BWD_RTOL, PIPE, rel_err, report, small_scene
from route_utils import reset_forward_state
from synthetic_model import SyntheticGaussians

pytestmark = pytest.mark.gpu

assert (dgr.BILAGRID_TILE_W, dgr.BILAGRID_TILE_H) == (bt.TILE_W, bt.TILE_H)


def _run(image, grid, dL, image_grad=True, grid_grad=True):
    im = image.cuda().requires_grad_(image_grad)
    gr = grid.cuda().requires_grad_(grid_grad)
    out = dgr.bilateral_slice(im, gr)
    if image_grad or grid_grad:
        (out * dL.cuda()).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), im.grad, gr.grad


@functools.lru_cache(maxsize=None)
def _gpu(name):
    """two runs of a case"""
    return _run(*bt.scene(name)), _run(*bt.scene(name))


def _window_nodes(W, H, GX, GY):
    """the largest number of xy nodes a tile touches (float64 statement of the geometry)"""
    def axis(n, G, T):
        if G == 1:
            return 1
        best = 0
        for x0 in range(0, n, T):
            x1 = min(x0 + T, n) - 1
            a, b = (min(int((x + 0.5) / n * (G - 1)), G - 2) for x in (x0, x1))
            best = max(best, b - a + 2)
        return best
    return axis(W, GX, bt.TILE_W) * axis(H, GY, bt.TILE_H)


def test_cases_reach_both_grid_paths():
    """a condition on the inputs: the LDS window and the global-memory path are both exercised"""
    nodes = {name: _window_nodes(*bt.CASES[name][:4]) for name in bt.CASES}
    assert nodes["37x23"] > dgr.BILAGRID_WINDOW_CELLS and nodes["300x17"] > dgr.BILAGRID_WINDOW_CELLS
    assert nodes["strip"] > dgr.BILAGRID_WINDOW_CELLS            # 16 rows under 16 planes in y: 128-pixel cells in x only
    for name in ("1x1", "exposure", "64x64", "200x130", "tile_edges"):
        assert nodes[name] <= dgr.BILAGRID_WINDOW_CELLS, name
    # 16-byte rows and scalar rows on either path
    assert bt.CASES["64x64"][0] % 4 == 0 and bt.CASES["tile_edges"][0] % 4 != 0
    assert bt.CASES["strip"][0] % 4 == 0 and bt.CASES["37x23"][0] % 4 != 0


@pytest.mark.parametrize("name", list(bt.CASES))
def test_slice_against_float64(name):
    t = bt.truth(name)
    (out, g_image, g_grid), again = _gpu(name)
    W, H, GX, GY, GL, _ = bt.CASES[name]
    assert out.shape == (3, H, W) and out.dtype == torch.float32
    assert g_image.shape == (3, H, W) and g_grid.shape == (12, GL, GY, GX)
    tol = max(1e-6, 4.0 * t["restated_out"])
    e = (out.double().cpu() - t["out"]).abs().max().item()
    report(f"bilagrid {name}", f"forward max abs err (restatement {t['restated_out']:.2e}, bound {tol:.2e})", e)
    ok = (~t["flags"]).unsqueeze(0).expand(3, H, W)
    e_i = rel_err(g_image, t["g_image"], ok)
    e_g = rel_err(g_grid, t["g_grid"])
    report(f"bilagrid {name}", f"dL/dimage max rel err on unflagged pixels (restatement {t['restated_g_image']:.2e})", e_i)
    report(f"bilagrid {name}", f"dL/dgrid max rel err (restatement {t['restated_g_grid']:.2e})", e_g)
    report(f"bilagrid {name}", "flagged share", t["flags"].float().mean().item())
    assert e <= tol
    assert e_i <= BWD_RTOL
    assert e_g <= BWD_RTOL
    for a, b in zip((out, g_image, g_grid), again):                          # two runs: the same bits
        assert torch.equal(a, b)


def test_hand_made_pixels():
    """black, z > 1 and z < 0 get the direct term A[:, :3]^T dL/dout only.  Against the truth within BWD_RTOL, and exactly: with
    GL = 2 a clamped guide reads ONE plane (black and z < 0: plane 0, weight 1 - 0), so pulling the other plane away changes the
    guide term of any pixel that has one and nothing else — these pixels must keep their bits.  For z > 1 the kernel forms
    A = B0 + 1 (B1 - B0), which depends on plane 0 by a rounding, so there the comparison grid copies plane 1 into plane 0 (no
    guide term for anybody) and the bound is that rounding, 1e-6; a guide term would be of order 1."""
    image, grid, dL = bt.scene("64x64")
    t = bt.truth("64x64")
    (_, g_image, _), _ = _gpu("64x64")
    scale = t["g_image"].abs().max().item()
    apart = grid.clone()
    apart[:, 1] += 5.0
    _, g_apart, _ = _run(image, apart, dL, grid_grad=False)
    flat = grid.clone()
    flat[:, 0] = grid[:, 1]
    _, g_flat, _ = _run(image, flat, dL, grid_grad=False)
    assert not torch.equal(g_apart, g_image)                                # (the other pixels do have a guide term)
    for key in ("black", "above", "below"):
        (y, x), _ = bt.HAND_MADE["64x64"][key]
        assert not t["flags"][y, x]
        got = g_image[:, y, x].double().cpu()
        assert (got - t["g_image"][:, y, x]).abs().max().item() <= BWD_RTOL * scale, key
        if key == "above":
            assert (g_flat[:, y, x] - g_image[:, y, x]).abs().max().item() <= 1e-6 * scale
        else:
            assert torch.equal(g_apart[:, y, x], g_image[:, y, x]), key


@pytest.mark.parametrize("name", ["64x64", "200x130"])
def test_pixel_on_a_plane_of_the_grid_takes_either_adjacent_cell(name):
    """fz within 1e-7 of an integer: dL/dimage is the truth's for the cell on either side"""
    image, grid, dL = bt.scene(name)
    t = bt.truth(name)
    (y, x), rgb = bt.HAND_MADE[name]["integer"]
    assert t["flags"][y, x]
    (_, g_image, _), _ = _gpu(name)
    got = g_image[:, y, x].double().cpu()
    scale = t["g_image"].abs().max().item()
    errs = []
    for nudge in (-2e-6, 2e-6):                          # the same pixel clearly on either side (the direct term moves by ~1e-6)
        im = image.clone()
        im[:, y, x] = torch.tensor(rgb, dtype=torch.float64).add(nudge).float()
        _, want, _ = bt.slice_gradients(im, grid, dL)
        errs.append((got - want[:, y, x]).abs().max().item() / scale)
    report(f"bilagrid {name}", "dL/dimage of the pixel on a plane: rel err against the cell below / above", min(errs))
    assert min(errs) <= BWD_RTOL, errs
    assert max(errs) > 10 * BWD_RTOL, errs               # (the two sides do differ: the test can tell them apart)


@pytest.mark.parametrize("name", ["64x64", "200x130", "37x23", "strip"])
def test_identity_grid_returns_the_image_bit_for_bit(name):
    image, _, dL = bt.scene(name)
    W, H, GX, GY, GL, _ = bt.CASES[name]
    out, g_image, g_grid = _run(image, bt.identity_grid(GX, GY, GL), dL)
    assert torch.equal(out.cpu(), image)
    assert torch.equal(g_image.cpu(), dL)
    assert g_grid.abs().max() > 0


def test_exposure_is_the_one_cell_grid():
    import bilagrid
    image, grid, dL = bt.scene("exposure")
    E = grid.reshape(3, 4)
    im = image.cuda().requires_grad_(True)
    Eg = E.cuda().requires_grad_(True)
    out = bilagrid.apply_exposure(im, Eg)
    (out * dL.cuda()).sum().backward()
    E64 = E.double().clone().requires_grad_(True)
    im64 = image.double().clone().requires_grad_(True)
    want = torch.einsum("cj,jhw->chw", E64[:, :3], im64) + E64[:, 3].view(3, 1, 1)
    (want * dL.double()).sum().backward()
    tol = max(1e-6, 4.0 * bt.truth("exposure")["restated_out"])
    assert (out.double().cpu() - want.detach()).abs().max().item() <= tol
    e_E, e_i = rel_err(Eg.grad, E64.grad), rel_err(im.grad, im64.grad)
    report("bilagrid exposure", "dL/dE max rel err against the float64 matmul", e_E)
    assert e_E <= BWD_RTOL and e_i <= BWD_RTOL
    assert Eg.grad.shape == (3, 4)


def test_non_finite_pixels_stay_in_the_grid_and_touch_nobody_else():
    image, grid, dL = bt.scene("200x130")
    (clean, g_clean, _), _ = _gpu("200x130")
    bad = image.clone()
    planted = ((40, 77), (99, 150))
    bad[0, 40, 77] = float("nan")
    bad[:, 99, 150] = torch.tensor([float("inf"), 0.3, float("-inf")])
    out, g_image, g_grid = _run(bad, grid, dL)
    others = torch.ones(130, 200, dtype=torch.bool, device="cuda")
    for y, x in planted:
        others[y, x] = False
        assert not torch.isfinite(out[:, y, x]).all()
    assert torch.equal(out[:, others], clean[:, others])
    assert torch.equal(g_image[:, others], g_clean[:, others])
    assert g_grid.shape == (12, 5, 3, 4)
    again = _run(*bt.scene("200x130"))                                       # the device is healthy: a clean call matches
    for a, b in zip(again, _gpu("200x130")[0]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["200x130", "37x23"])
def test_flags_skip_a_half_and_leave_the_other_unchanged(name):
    image, grid, dL = bt.scene(name)
    (_, g_image, g_grid), _ = _gpu(name)
    _, gi, gg = _run(image, grid, dL, grid_grad=False)                       # a frozen grid
    assert gg is None and torch.equal(gi, g_image)
    _, gi, gg = _run(image, grid, dL, image_grad=False)                      # a detached image
    assert gi is None and torch.equal(gg, g_grid)


def test_probe_sees_one_call_per_half(monkeypatch):
    image, grid, dL = bt.scene("64x64")
    calls = []
    monkeypatch.setattr(dgr, "_bilagrid_probe", calls.append)
    _run(image, grid, dL)
    assert calls == ["msgs_bilagrid_slice_forward", "msgs_bilagrid_slice_backward"]


def test_refusals():
    image = torch.zeros(3, 8, 8, device="cuda")
    for shape in ((12, 33, 2, 2), (12, 2, 2, 257), (11, 2, 2, 2)):
        with pytest.raises(ValueError):
            dgr.bilateral_slice(image, torch.zeros(shape, device="cuda"))
    with pytest.raises(RuntimeError, match="HIP device"):
        dgr.bilateral_slice(image, torch.zeros(12, 2, 2, 2))


def test_converted_inputs():
    """float64 and strided inputs are converted; the result is that of the float32 contiguous copies"""
    image, grid, dL = bt.scene("200x130")
    (out, g_image, g_grid), _ = _gpu("200x130")
    im = image.permute(1, 2, 0).contiguous().permute(2, 0, 1).double().cuda().requires_grad_(True)
    gr = grid.double().cuda().requires_grad_(True)
    o = dgr.bilateral_slice(im, gr)
    (o * dL.cuda()).sum().backward()
    assert torch.equal(o, out) and torch.equal(im.grad.float(), g_image) and torch.equal(gr.grad.float(), g_grid)


@pytest.mark.parametrize("name", list(bt.TV_BANKS))
def test_total_variation(name):
    bank = bt.tv_bank(name)
    want, want_grad = bt.tv_truth(name)
    runs = []
    for _ in range(2):
        g = bank.cuda().requires_grad_(True)
        tv = dgr.total_variation_loss(g)
        (tv * 1.7).backward()
        torch.cuda.synchronize()
        runs.append((tv.detach(), g.grad))
    tv, grad = runs[0]
    assert tv.dim() == 0 and grad.shape == bank.shape
    assert torch.equal(tv, runs[1][0]) and torch.equal(grad, runs[1][1])
    if name == "1x1x1":
        assert tv.item() == 0.0 and not grad.any()
        return
    e = abs(tv.item() - want.item()) / want.item()
    e_g = rel_err(grad, want_grad * 1.7)
    report(f"bilagrid tv {name}", "value rel err", e)
    report(f"bilagrid tv {name}", "gradient max rel err", e_g)
    assert e <= 1e-6 and e_g <= 1e-6


def test_module_slices_its_own_grid_and_regularises_the_bank():
    import bilagrid
    image, _, dL = bt.scene("64x64")
    m = bilagrid.BilateralGrid(3, grid_X=4, grid_Y=3, grid_W=5).cuda()
    with torch.no_grad():
        m.grids.add_(0.1 * torch.randn(m.grids.shape, generator=torch.Generator().manual_seed(5)).cuda())
    out = m(image.cuda(), 1)
    assert torch.equal(out, dgr.bilateral_slice(image.cuda(), m.grids[1].detach()))
    (out * dL.cuda()).sum().backward()
    assert m.grids.grad[1].abs().max() > 0 and not m.grids.grad[0].any() and not m.grids.grad[2].any()
    assert torch.equal(m.tv_loss(), dgr.total_variation_loss(m.grids.detach()))


# ---------------------------------------------------------------------------------------------------------------------------
# composition with render()
# ---------------------------------------------------------------------------------------------------------------------------
E2E = dict(P=300, W=64, H=48, seed=41)
LEAVES = SyntheticGaussians.LEAVES
BG = (0.1, 0.2, 0.3)


@functools.lru_cache(maxsize=None)
def _scene():
    return small_scene(E2E["P"], E2E["W"], E2E["H"], E2E["seed"])


def _fresh():
    sc, cam = _scene()
    reset_forward_state()
    return SyntheticGaussians(sc, "cuda", requires_grad=True), cam.to("cuda"), torch.tensor(BG, device="cuda")


def _grads(pc, out):
    torch.cuda.synchronize()
    g = {n: getattr(pc, n).grad.detach().clone() for n in LEAVES if getattr(pc, n).grad is not None}
    if out["viewspace_points"].grad is not None:
        g["viewspace"] = out["viewspace_points"].grad.detach().clone()
    return g


def test_render_with_bilateral_grid_composes_with_render():
    import bilagrid
    from gaussian_renderer import render
    seed = scenes.grad_seed(E2E["W"], E2E["H"], 78).cuda()
    pc, cam, bg = _fresh()
    plain = render(cam, pc, PIPE, bg)
    (plain["render"] * seed).sum().backward()
    want = _grads(pc, plain)
    assert len(want) >= 5

    grids = bilagrid.BilateralGrid(2, grid_X=4, grid_Y=4, grid_W=4).cuda()
    pc2, cam, bg = _fresh()
    out = bilagrid.render_with_bilateral_grid(cam, pc2, PIPE, bg, grids, 1)
    assert set(out) == set(plain) | {"render_raw"}
    assert torch.equal(out["render"], plain["render"]) and torch.equal(out["render_raw"], plain["render"])
    (out["render"] * seed).sum().backward()
    got = _grads(pc2, out)
    assert set(got) == set(want)
    for n in want:
        assert torch.equal(got[n], want[n]), n
    assert grids.grids.grad is not None and grids.grids.grad[1].abs().max() > 0

    with torch.no_grad():
        grids.grids.add_(0.2 * torch.randn(grids.grids.shape, generator=torch.Generator().manual_seed(6)).cuda())
    pc3, cam, bg = _fresh()
    out = bilagrid.render_with_bilateral_grid(cam, pc3, PIPE, bg, grids, 0)
    assert torch.equal(out["render_raw"], plain["render"])
    assert (out["render"] - plain["render"]).abs().max() > 1e-3

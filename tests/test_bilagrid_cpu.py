"""Bilateral-grid colour correction (SPEC M19) without a GPU: the float64 truth of tests/bilagrid_truth.py against
torch's grid_sample and against the definition of the total variation, the conditions the GPU tests rely on (the share of
flagged pixels), and the surface — the C ABI's symbols, constants and argument checks, the Python entries' refusals."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import bilagrid_truth as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("msgs_bilagrid_scratch_bytes", "msgs_bilagrid_slice_forward", "msgs_bilagrid_slice_backward",
         "msgs_bilagrid_tv_scratch_bytes", "msgs_bilagrid_tv_forward", "msgs_bilagrid_tv_backward")
FLAGGED_CAP = 0.005


def _grid_sample_matrix(image, grid):
    """F.grid_sample (float64, bilinear, border, align_corners=True) on ((x_n, y_n, z) - 0.5) * 2: A [3,4,H,W]"""
    _, H, W = image.shape
    x = ((torch.arange(W, dtype=torch.float64) + 0.5) / W).view(1, W).expand(H, W)
    y = ((torch.arange(H, dtype=torch.float64) + 0.5) / H).view(H, 1).expand(H, W)
    z = bt.guide(image)
    coords = (torch.stack([x, y, z], dim=-1) - 0.5) * 2.0
    A = F.grid_sample(grid.unsqueeze(0), coords.view(1, 1, H, W, 3), mode="bilinear", padding_mode="border", align_corners=True)
    return A.view(3, 4, H, W)


def _grid_sample_slice(image, grid):
    A = _grid_sample_matrix(image, grid)
    return A[:, 0] * image[0] + A[:, 1] * image[1] + A[:, 2] * image[2] + A[:, 3]


@pytest.mark.parametrize("name", list(bt.CASES))
def test_truth_equals_grid_sample_and_affine_product(name):
    image, grid, dL = bt.scene(name)
    t = bt.truth(name)
    im = image.double().clone().requires_grad_(True)
    gr = grid.double().clone().requires_grad_(True)
    out = _grid_sample_slice(im, gr)
    (out * dL.double()).sum().backward()
    assert (out.detach() - t["out"]).abs().max().item() <= 1e-12
    for got, want in ((im.grad, t["g_image"]), (gr.grad, t["g_grid"])):
        assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


def test_hand_made_pixels_take_the_direct_term_only():
    """black, z > 1 and z < 0: the truth's dL/dimage is A[:, :3]^T dL/dout alone, A being grid_sample's matrix of the pixel"""
    image, grid, dL = bt.scene("64x64")
    t = bt.truth("64x64")
    A = _grid_sample_matrix(image.double(), grid.double())
    for key in ("black", "above", "below"):
        (y, x), _ = bt.HAND_MADE["64x64"][key]
        z = bt.guide(image.double())[y, x].item()
        assert not 0 < z < 1, key
        direct = A[:, :3, y, x].t() @ dL[:, y, x].double()
        assert (t["g_image"][:, y, x] - direct).abs().max().item() <= 1e-13, key
    (y, x), _ = bt.HAND_MADE["64x64"]["integer"]                     # just inside the interval: the guide term is there
    assert 0 < bt.guide(image.double())[y, x].item() < 1
    assert (t["g_image"][:, y, x] - A[:, :3, y, x].t() @ dL[:, y, x].double()).abs().max().item() > 1e-3


@pytest.mark.parametrize("name", list(bt.CASES))
def test_flagged_share_is_small(name):
    fl = bt.truth(name)["flags"]
    assert fl.float().mean().item() <= FLAGGED_CAP
    for key, ((y, x), _) in bt.HAND_MADE.get(name, {}).items():
        assert bool(fl[y, x]) == (key == "integer"), key


@pytest.mark.parametrize("name", list(bt.TV_BANKS))
def test_tv_truth_equals_the_definition(name):
    g = bt.tv_bank(name).double()
    want = torch.zeros((), dtype=torch.float64)
    if g.shape[4] > 1:
        want = want + (g[:, :, :, :, 1:] - g[:, :, :, :, :-1]).pow(2).mean()
    if g.shape[3] > 1:
        want = want + (g[:, :, :, 1:] - g[:, :, :, :-1]).pow(2).mean()
    if g.shape[2] > 1:
        want = want + (g[:, :, 1:] - g[:, :, :-1]).pow(2).mean()
    tv, grad = bt.tv_truth(name)
    assert abs(tv.item() - want.item()) <= 1e-13 * max(1.0, want.item())
    assert grad.shape == g.shape
    if name == "1x1x1":
        assert tv.item() == 0.0 and not grad.any()


def test_identity_grid_is_the_identity_in_the_truth():
    image, _, _ = bt.scene("200x130")
    out = bt.slice_forward(image, bt.identity_grid(4, 3, 5))
    assert (out - image.double()).abs().max().item() <= 1e-15


# ---------------------------------------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_mirrors_agree():
    import diff_gaussian_rasterization as dgr
    hdr = open(os.path.join(ROOT, "include", "msgs.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in dgr._C.EXPORTS and hasattr(dgr._C.lib, n)

    def const(name):
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1))
    assert (dgr.BILAGRID_TILE_W, dgr.BILAGRID_TILE_H) == (const("MSGS_BILAGRID_TILE_W"), const("MSGS_BILAGRID_TILE_H"))
    assert (dgr.BILAGRID_TILE_W, dgr.BILAGRID_TILE_H) == (bt.TILE_W, bt.TILE_H)
    assert dgr.BILAGRID_WINDOW_CELLS == const("MSGS_BILAGRID_WINDOW_CELLS")
    assert (dgr._C.BILAGRID_MAX_XY, dgr._C.BILAGRID_MAX_L) == (const("MSGS_BILAGRID_MAX_XY"), const("MSGS_BILAGRID_MAX_L")) == (256, 32)
    assert (dgr._C.BILAGRID_GRAD_IMAGE, dgr._C.BILAGRID_GRAD_GRID) == (const("MSGS_BILAGRID_GRAD_IMAGE"),
                                                                       const("MSGS_BILAGRID_GRAD_GRID"))
    assert const("MSGS_ABI_VERSION") == 11 == dgr._C.lib.msgs_abi_version()


def test_c_entries_refuse_bad_sizes_and_null_pointers_before_any_launch():
    """host-only: every call below must return an error code without touching a device"""
    import diff_gaussian_rasterization as dgr
    lib = dgr._C.lib
    p = C.c_void_p(256)                       # never dereferenced: the argument checks come first
    bad_sizes = [(64, 64, 257, 2, 2), (64, 64, 2, 257, 2), (64, 64, 2, 2, 33), (64, 64, 0, 2, 2), (64, 64, 2, 2, 0), (0, 64, 2, 2, 2),
                 (64, -1, 2, 2, 2)]
    for s in bad_sizes:
        assert lib.msgs_bilagrid_slice_forward(*s, p, p, p, None) == -1, s
        assert lib.msgs_bilagrid_slice_backward(*s, p, p, p, 3, p, p, p, 1 << 40, None) == -1, s
        assert lib.msgs_bilagrid_scratch_bytes(*s) == 0
    ok = (64, 64, 2, 2, 2)
    assert lib.msgs_bilagrid_slice_forward(*ok, None, p, p, None) == -1
    assert lib.msgs_bilagrid_slice_forward(*ok, p, None, p, None) == -1
    assert lib.msgs_bilagrid_slice_forward(*ok, p, p, None, None) == -1
    need = lib.msgs_bilagrid_scratch_bytes(*ok)
    assert need > 0 and need % 256 == 0
    assert lib.msgs_bilagrid_slice_backward(*ok, p, p, None, 3, p, p, p, need, None) == -1
    assert lib.msgs_bilagrid_slice_backward(*ok, p, p, p, 1, None, None, None, 0, None) == -1      # image half without its pointer
    assert lib.msgs_bilagrid_slice_backward(*ok, p, p, p, 2, None, None, p, need, None) == -1      # grid half without its pointer
    assert lib.msgs_bilagrid_slice_backward(*ok, p, p, p, 2, None, p, None, need, None) == -1      # ... without scratch
    assert lib.msgs_bilagrid_slice_backward(*ok, p, p, p, 4, p, p, p, need, None) == -1            # unknown bit
    assert lib.msgs_bilagrid_slice_backward(*ok, p, p, p, 2, None, p, p, need - 1, None) == -2     # MSGS_ERR_CAPACITY
    assert lib.msgs_bilagrid_slice_backward(*ok, p, p, p, 0, None, None, None, 0, None) == 0       # nothing wanted: nothing done
    tv_need = lib.msgs_bilagrid_tv_scratch_bytes(3 * 12 * 8 * 16 * 16)
    assert tv_need > 0 and tv_need % 256 == 0
    assert lib.msgs_bilagrid_tv_forward(3, 16, 16, 33, p, p, p, tv_need, None) == -1
    assert lib.msgs_bilagrid_tv_forward(3, 16, 16, 8, None, p, p, tv_need, None) == -1
    assert lib.msgs_bilagrid_tv_forward(3, 16, 16, 8, p, None, p, tv_need, None) == -1
    assert lib.msgs_bilagrid_tv_forward(3, 16, 16, 8, p, p, p, 8, None) == -2
    assert lib.msgs_bilagrid_tv_backward(3, 257, 16, 8, p, p, p, None) == -1
    assert lib.msgs_bilagrid_tv_backward(3, 16, 16, 8, None, p, p, None) == -1
    assert lib.msgs_bilagrid_tv_backward(0, 16, 16, 8, None, None, None, None) == 0


def test_scratch_grows_with_the_image_and_covers_every_wave_window():
    import diff_gaussian_rasterization as dgr
    lib = dgr._C.lib
    small, large = lib.msgs_bilagrid_scratch_bytes(64, 16, 16, 16, 8), lib.msgs_bilagrid_scratch_bytes(1920, 1080, 16, 16, 8)
    assert 0 < small < large
    # the training geometry: 30 x 270 strips of 64 x 4 pixels, each a window of at most 2 x 2 nodes x 8 planes x 12 floats
    assert large == 30 * 270 * 2 * 2 * 8 * 12 * 4


def test_cpu_tensors_and_bad_shapes_are_refused():
    import diff_gaussian_rasterization as dgr
    image, grid, _ = bt.scene("64x64")
    with pytest.raises(RuntimeError, match="HIP device"):
        dgr.bilateral_slice(image, grid)
    with pytest.raises(RuntimeError, match="HIP device"):
        dgr.total_variation_loss(bt.tv_bank("4x3x5"))
    for bad in (torch.zeros(12, 33, 2, 2), torch.zeros(12, 2, 2, 257), torch.zeros(12, 2, 257, 2), torch.zeros(11, 2, 2, 2),
                torch.zeros(12, 2, 2)):
        with pytest.raises(ValueError):
            dgr.bilateral_slice(image, bad)
    with pytest.raises(ValueError):
        dgr.bilateral_slice(torch.zeros(4, 8, 8), grid)
    with pytest.raises(ValueError):
        dgr.total_variation_loss(torch.zeros(2, 11, 2, 2, 2))


def test_host_module_surface():
    import inspect

    import bilagrid
    m = bilagrid.BilateralGrid(5)
    assert tuple(m.grids.shape) == (5, 12, 8, 16, 16) and m.grids.requires_grad
    assert torch.equal(m.grids[3], bt.identity_grid(16, 16, 8))
    assert list(inspect.signature(bilagrid.BilateralGrid.__init__).parameters)[1:] == ["num_images", "grid_X", "grid_Y", "grid_W"]
    sig = list(inspect.signature(bilagrid.render_with_bilateral_grid).parameters)
    assert sig == ["viewpoint_camera", "pc", "pipe", "bg_color", "bil_grids", "image_index", "render_kwargs"]
    with pytest.raises(ValueError):
        bilagrid.apply_exposure(torch.zeros(3, 4, 4), torch.zeros(4, 3))

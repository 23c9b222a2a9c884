"""Per-image colour correction with bilateral grids (4.20): what a trainer places between render() and the
photometric loss, so that exposure and white-balance differences between the captures are explained by a per-image transform
and not by floaters.

    BilateralGrid(num_images)              a bank of learned grids [N,12,GL,GY,GX], identity-initialised (gsplat's
                                           use_bilateral_grid, "Bilateral Guided Radiance Field Processing")
    apply_exposure(image, exposure_3x4)    upstream 3DGS's learned per-image 3x4 exposure matrix: the grid of size 1x1x1
    render_with_bilateral_grid(cam, ...)   render() with "render" corrected and "render_raw" added

All three go through diff_gaussian_rasterization.bilateral_slice / total_variation_loss (HIP); the rasterizer is untouched, so
every other opt-in composes by construction.
"""
import torch
from torch import nn

from diff_gaussian_rasterization import bilateral_slice, total_variation_loss


def identity_grids(num_images, grid_X=16, grid_Y=16, grid_W=8, device=None):
    """[N,12,GL,GY,GX]: eye(4)[:3].flatten() in every cell"""
    eye = torch.eye(4, dtype=torch.float32, device=device)[:3].reshape(12)
    return eye.view(1, 12, 1, 1, 1).repeat(int(num_images), 1, int(grid_W), int(grid_Y), int(grid_X)).contiguous()


class BilateralGrid(nn.Module):
    """A bank of bilateral grids, one per training image (gsplat's names and defaults: grid_X x grid_Y cells over the image,
    grid_W planes over the luminance).  `grids` is a Parameter [N,12,grid_W,grid_Y,grid_X], identity-initialised: at the start
    forward() returns its input bit for bit.  Give the parameter its own Adam group and add tv_loss() times a weight of the
    caller's choice to the loss."""

    def __init__(self, num_images, grid_X=16, grid_Y=16, grid_W=8):
        super().__init__()
        self.grid_width, self.grid_height, self.grid_guidance = int(grid_X), int(grid_Y), int(grid_W)
        self.grids = nn.Parameter(identity_grids(num_images, grid_X, grid_Y, grid_W))

    def forward(self, image, image_index):
        """`image` [3,H,W] corrected by the grid of image `image_index` (an int)"""
        return bilateral_slice(image, self.grids[int(image_index)])

    def tv_loss(self):
        return total_variation_loss(self.grids)


def apply_exposure(image, exposure_3x4):
    """Upstream 3DGS's per-image exposure: out = E[:, :3] @ rgb + E[:, 3] per pixel of `image` [3,H,W], with `exposure_3x4`
    [3,4] that image's learned matrix.  It is exactly the bilateral grid of size 1x1x1 and runs as one: no coordinates, no
    guide term, gradients to both arguments."""
    if tuple(exposure_3x4.shape) != (3, 4):
        raise ValueError(f"apply_exposure: exposure must be [3,4], got {tuple(exposure_3x4.shape)}")
    return bilateral_slice(image, exposure_3x4.reshape(12, 1, 1, 1))


def render_with_bilateral_grid(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, bil_grids, image_index, **render_kwargs):
    """render()'s dict with "render" = bil_grids(render, image_index) and the uncorrected image under "render_raw".
    `bil_grids` is a BilateralGrid (any callable (image, index) -> image works); `render_kwargs` go to render() as they are.
    With an identity grid "render" and every Gaussian gradient equal render()'s bit for bit."""
    from gaussian_renderer import render
    out = render(viewpoint_camera, pc, pipe, bg_color, **render_kwargs)
    out["render_raw"] = out["render"]
    out["render"] = bil_grids(out["render_raw"], image_index)
    return out

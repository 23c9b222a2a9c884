"""Contribution scores over a camera set, and pruning by them (SPEC M11; 4.11).

The reference prunes by opacity alone (/root/reference/scene/gaussian_model.py:683-694).  What a Gaussian actually did to the
images is its blend weight w = alpha T over the pixels it was blended into: LightGaussian's global significance, RadSplat's
max-contribution pruning and Mini-Splatting's importance rank by it, and so do error-weighted densification scores.  After
insert_large_gaussians / grow_large_gaussians stacks of coarse and fine Gaussians cover the same surface at different levels,
and many of them never win a pixel.

  contribution_scores(cams, pc, pipe, bg_color, pixel_weights=None, **filters)  -> ContributionScores over all cameras
  contribution_prune_mask(scores, fraction= | threshold=, key="weight_sum")     -> bool [P], True = remove (pure torch)
  prune_by_contribution(model, scores, optimizer=None, **mask_kw)               -> the mask; rows and Adam moments removed
"""
import torch

from diff_gaussian_rasterization import ContributionAccumulator, ContributionScores, GaussianRasterizer
from gaussian_renderer import _settings

KEYS = ContributionScores._fields


@torch.no_grad()
def contribution_scores(cams, pc, pipe, bg_color, *, pixel_weights=None, scaling_modifier=1.0, **filters):
    """Scores of every Gaussian of `pc` over `cams`: weight_sum and pixel_count added, weight_max maximised across the views —
    one accumulator, one forward and one replay per camera, no per-view [P] tensors.  Each camera is rendered as render() renders
    it (same culling, lists and termination; **filters: filter_small / filter_large / fade_size); colours do not enter.
    pixel_weights: None, or a callable (cam_index, cam) -> [H,W] float32 tensor or None — a mask, or a per-pixel error for
    error-weighted scores; a pixel with weight <= 0 does not count."""
    xyz = pc.get_xyz
    act = dict(opacities=pc.get_opacity, scales=pc.get_scaling, rotations=pc.get_rotation,        # evaluated once
               max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes, base_mask=pc.get_base_mask)
    acc = ContributionAccumulator(int(xyz.shape[0]), xyz.device)
    for i, cam in enumerate(cams):
        rasterizer = GaussianRasterizer(raster_settings=_settings(
            cam, pc, pipe, bg_color, scaling_modifier, filters.get("filter_small", False), filters.get("filter_large", False),
            filters.get("fade_size", 1.0)))
        rasterizer.contributions(xyz, pixel_weights=pixel_weights(i, cam) if pixel_weights is not None else None, into=acc, **act)
    return acc.scores()


def contribution_prune_mask(scores, *, fraction=None, threshold=None, key="weight_sum"):
    """bool [P], True = remove.  Exactly one of:
      threshold  remove the rows with score < threshold;
      fraction   remove the floor(fraction P) rows that are lowest by (score, index) — a stable order, so ties and never-seen
                 rows (score 0) leave in index order.
    key: "weight_sum" | "weight_max" | "pixel_count", or a [P] tensor of your own (e.g. weight_sum * volume ** beta)."""
    if (fraction is None) == (threshold is None):
        raise ValueError("give exactly one of fraction= and threshold=")
    if isinstance(key, str):
        if key not in KEYS:
            raise ValueError(f"key must be one of {KEYS} or a tensor, got {key!r}")
        score = getattr(scores, key)
    else:
        score = key
    score = score.reshape(-1)
    P = int(score.shape[0])
    if threshold is not None:
        return score < threshold
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError(f"fraction must lie in [0, 1], got {fraction}")
    n = min(P, int(float(fraction) * P))
    mask = torch.zeros(P, dtype=torch.bool, device=score.device)
    if n > 0:
        mask[torch.sort(score, stable=True).indices[:n]] = True
    return mask


def prune_by_contribution(model, scores, *, optimizer=None, **mask_kw):
    """contribution_prune_mask(scores, **mask_kw), then densify.prune_points: the rows leave every tensor of the model and the
    optimizer's moments.  Returns the mask (in the row order before the prune)."""
    from densify import prune_points
    mask = contribution_prune_mask(scores, **mask_kw)
    prune_points(model, mask, optimizer=optimizer)
    return mask

"""The seeded image pairs of the loss sweep (tests/test_loss_cases_cpu.py, tests/test_loss_gpu.py): what uniform noise never
reaches.  On noise the windowed variance E[x^2] - mu^2 is about 0.08 and nothing cancels; a render close to its target, smooth
shading, white or black backgrounds and saturated regions have variances far below C2 = 9e-4, and there the float32 rounding of
E[x^2] and mu^2 lands directly in sigma1^2 + sigma2^2 + C2.

Every case is a small function of fixed seeds that returns (img, gt), float32 [C,H,W], numpy only; none is larger than
3 x 135 x 240.  What makes a case what its name says is asserted from the float64 truth alone in tests/test_loss_cases_cpu.py."""
import functools

import numpy as np

from oracle import loss_oracle as lo

LAMBDAS = (0.0, 0.2, 1.0)
SHAPE = (3, 70, 90)                 # 3 x 3 tiles of 32, ragged on both axes


def _u(seed, shape=SHAPE):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def _f32(*a):
    return tuple(np.ascontiguousarray(v, dtype=np.float32) for v in a)


def _texture(C, H, W):
    """the smooth low-frequency target of tests/golden/make_loss_golden.py case f"""
    yy, xx = np.meshgrid(np.linspace(0, 3, H), np.linspace(0, 3, W), indexing="ij")
    return np.stack([0.5 + 0.5 * np.sin(xx * (c + 1) + yy) for c in range(C)])


def white_background():
    """x = 1 - 1e-3 U, y = 1"""
    return _f32(1.0 - 1e-3 * _u(101), np.ones(SHAPE))


def flat_offset():
    """x = 0.98, y = 1 everywhere"""
    return _f32(np.full(SHAPE, 0.98), np.ones(SHAPE))


def flat_grey():
    """y = 0.7, x = y + 1e-3 U"""
    y = np.full(SHAPE, 0.7, dtype=np.float32)
    return _f32(y + 1e-3 * _u(102), y)


def converged_ramp():
    """y ramps 0.6 .. 1.0 across W, x = y + 1e-2 (U - 1/2): a converged render (not clamped: x passes 1 at the right edge)"""
    y = np.broadcast_to(np.linspace(0.6, 1.0, SHAPE[2], dtype=np.float32), SHAPE)
    return _f32(y + 1e-2 * (_u(103) - 0.5), y)


def half_white():
    """left half exactly 1 in both images, right half independent noise; the seam (column 45) is inside a tile"""
    x, y = _u(104), _u(105)
    x[:, :, :45] = 1.0
    y[:, :, :45] = 1.0
    return _f32(x, y)


def near_black():
    """x = 1e-3 U, y = 0"""
    return _f32(1e-3 * _u(106), np.zeros(SHAPE))


def _converged_texture(H, W, seed):
    gt = _texture(3, H, W)
    n = np.random.default_rng(seed).standard_normal((3, H, W))
    return _f32(np.clip(gt + 1e-3 * n, 0.0, 1.0), gt)


def converged_texture_small():
    return _converged_texture(33, 65, 107)


def converged_texture_large():
    return _converged_texture(135, 240, 108)


def saturated_mix():
    """blocks of exact 0 and exact 1 shared by both images (61 % of the pixels: sign(0) applies there), the remainder a texture
    with a 2e-2 perturbation; no block edge is a multiple of 32"""
    gt = _texture(*SHAPE)
    x = np.clip(gt + 2e-2 * np.random.default_rng(109).standard_normal(SHAPE), 0.0, 1.0)
    for a in (x, gt):
        a[:, :41, :37] = 0.0
        a[:, 29:, 45:] = 1.0
        a[:, 47:, :21] = 1.0
    return _f32(x, gt)


def bright_hdr_flat():
    """unclamped values above 1: x = 8.0, y = 7.9; the cancellation grows with the value squared"""
    return _f32(np.full(SHAPE, 8.0), np.full(SHAPE, 7.9))


def bright_hdr_noisy():
    """x = 8.0 + 1e-2 (U - 1/2), y = 7.9 + 1e-2 (U' - 1/2)"""
    return _f32(8.0 + 1e-2 * (_u(110) - 0.5), 7.9 + 1e-2 * (_u(111) - 0.5))


def one_channel():
    """C = 1: y = 0.5, x = y + 1e-3 U"""
    y = np.full((1, 40, 40), 0.5, dtype=np.float32)
    return _f32(y + 1e-3 * _u(112, (1, 40, 40)), y)


def tiny_flat_5x3():
    """the window is mostly zero padding, which must stay a true 0"""
    return _f32(np.full((3, 5, 3), 0.98), np.ones((3, 5, 3)))


def tiny_flat_1x1():
    return _f32(np.full((3, 1, 1), 0.98), np.ones((3, 1, 1)))


CASES = {f.__name__: f for f in (white_background, flat_offset, flat_grey, converged_ramp, half_white, near_black,
                                 converged_texture_small, converged_texture_large, saturated_mix, bright_hdr_flat,
                                 bright_hdr_noisy, one_channel, tiny_flat_5x3, tiny_flat_1x1)}
# the pairs on which the reference formulation evaluated in float32 is itself outside GRAD_RTOL of the float64 truth
FLAT_OR_CONVERGED = ("white_background", "flat_offset", "flat_grey", "converged_ramp")
# upstream: None = loss.backward(), 0.1 = (loss * 0.1).backward() (the loss multiplier of the train step)
RUNS = [(name, lam, up) for name in CASES for lam in LAMBDAS for up in (None, 0.1)]


@functools.lru_cache(maxsize=None)
def pair(name):
    img, gt = CASES[name]()
    img.setflags(write=False)
    gt.setflags(write=False)
    return img, gt


@functools.lru_cache(maxsize=None)
def truth(name, lam):
    """float64 oracle of one case at one lambda: dict(loss, l1, ssim, grad); computed once and shared, never modified"""
    r = lo.l1_ssim(*pair(name), lam, dtype=np.float64)
    r["grad"].setflags(write=False)
    return r

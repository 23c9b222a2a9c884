"""Float64 truth of the bilateral-grid slice and of the total variation (DESIGN.md SPEC M19), written from the definition corner
by corner, with gradients by float64 autograd; the same formulas restated in float32 for the error scale; the borderline flags;
and the scenes of tests/test_bilagrid_cpu.py and tests/test_bilagrid_gpu.py (fixed seeds, built once and cached).

SPEC M19.  image [3,H,W], grid [12,GL,GY,GX] (channel 4 c + j = entry (c, j) of a 3x4 matrix).
    fx = (x + 0.5) / W (GX - 1),  fy = (y + 0.5) / H (GY - 1),  z = 0.299 r + 0.587 g + 0.114 b,  fz = clamp(z, 0, 1) (GL - 1)
    axis of size G > 1: cell k = min(floor(f), G - 2), weights 1 - t and t with t = f - k; size 1: coordinate 0, weight 1
    A = sum over the 8 corners of w grid[:, kz, ky, kx];  out_c = A[c,0] r + A[c,1] g + A[c,2] b + A[c,3]
The guide's gradient flows where 0 < z < 1 (open at both ends) and nowhere else.

Flags.  A pixel is borderline when z (GL - 1) lies within 1e-5 (GL - 1) of an integer in [0, GL - 1], unless it is exactly
black: there float32 may land in the neighbouring cell or on the other side of the open interval.  The flags exempt a pixel from
the dL/dimage check ONLY: the forward and dL/dgrid are continuous across a cell boundary.
"""
import functools

import torch

GUIDE = (0.299, 0.587, 0.114)
FLAG_WINDOW = 1e-5
TILE_W, TILE_H = 64, 16            # the kernels' tile; tests/test_bilagrid_cpu.py checks it against the package's constants

# name: (W, H, GX, GY, GL, seed)
CASES = {
    "1x1": (1, 1, 1, 1, 1, 11),
    "exposure": (129, 65, 1, 1, 1, 12),
    "64x64": (64, 64, 2, 2, 2, 13),
    "200x130": (200, 130, 4, 3, 5, 14),
    "37x23": (37, 23, 16, 16, 8, 15),
    "300x17": (300, 17, 16, 16, 8, 16),
    "tile_edges": (2 * TILE_W + 1, TILE_H + 1, 3, 2, 8, 17),
    "strip": (1920, 16, 16, 16, 8, 18),
}
# hand-made pixels (y, x): rgb, planted into the random image of a case
NEAR_ONE = 1.0 - 2.0 ** -24                  # float32 neighbours of 1 and of 1/4 from below: fz is within 1e-7 of an integer,
NEAR_QUARTER = 0.25 - 2.0 ** -26             # and float64 still tells the side
HAND_MADE = {
    "64x64": {"black": ((3, 5), (0.0, 0.0, 0.0)), "above": ((3, 6), (1.2, 1.1, 1.15)), "below": ((3, 7), (-0.1, -0.05, -0.02)),
              "integer": ((3, 8), (NEAR_ONE, NEAR_ONE, NEAR_ONE))},
    "200x130": {"integer": ((10, 20), (NEAR_QUARTER, NEAR_QUARTER, NEAR_QUARTER))},
}
TV_BANKS = {"1x1x1": (1, 1, 1, 1, 21), "16x16x8": (3, 16, 16, 8, 22), "4x3x5": (2, 4, 3, 5, 23)}     # N, GX, GY, GL, seed


def identity_grid(GX, GY, GL, dtype=torch.float32):
    return torch.eye(4, dtype=dtype)[:3].reshape(12, 1, 1, 1).repeat(1, GL, GY, GX).contiguous()


def random_scene(W, H, GX, GY, GL, seed):
    """image uniform in [-0.1, 1.2] (both clamps of the guide occur), grid = identity + 0.3 normal, dL/dout normal; float32"""
    g = torch.Generator().manual_seed(seed)
    image = (torch.rand(3, H, W, generator=g, dtype=torch.float64) * 1.3 - 0.1).float()
    grid = (identity_grid(GX, GY, GL, torch.float64) + 0.3 * torch.randn(12, GL, GY, GX, generator=g, dtype=torch.float64)).float()
    dL = torch.randn(3, H, W, generator=g, dtype=torch.float64).float()
    return image, grid, dL


@functools.lru_cache(maxsize=None)
def scene(name):
    image, grid, dL = random_scene(*CASES[name])
    for (y, x), rgb in HAND_MADE.get(name, {}).values():
        image[:, y, x] = torch.tensor(rgb, dtype=torch.float64).float()
    return image, grid, dL


def _axis(f, G):
    """[(offset, weight)] of the corners along an axis whose continuous coordinate is f"""
    if G == 1:
        return torch.zeros_like(f, dtype=torch.long), [(0, torch.ones_like(f))]
    k = torch.floor(f.detach()).clamp(0, G - 2)
    t = f - k
    return k.long(), [(0, 1.0 - t), (1, t)]


def guide(image):
    return GUIDE[0] * image[0] + GUIDE[1] * image[1] + GUIDE[2] * image[2]


def slice_forward(image, grid, dtype=torch.float64):
    """the SPEC in `dtype`, corner by corner; differentiable in both arguments (float64: the truth; float32: the restatement)"""
    image, grid = image.to(dtype), grid.to(dtype)
    _, H, W = image.shape
    _, GL, GY, GX = grid.shape
    fx = ((torch.arange(W, dtype=dtype) + 0.5) / W * (GX - 1)).view(1, W).expand(H, W)
    fy = ((torch.arange(H, dtype=dtype) + 0.5) / H * (GY - 1)).view(H, 1).expand(H, W)
    z = guide(image)
    inside = (z > 0) & (z < 1)                                   # the open interval: the only place the guide's gradient flows
    zc = torch.where(inside, z, z.detach().clamp(0, 1))
    zc = torch.where(torch.isfinite(z), zc, torch.where(z > 0, torch.ones_like(z), torch.zeros_like(z)))
    fz = zc * (GL - 1)
    kx, cx = _axis(fx, GX)
    ky, cy = _axis(fy, GY)
    kz, cz = _axis(fz, GL)
    A = torch.zeros(12, H, W, dtype=dtype)
    for oz, wz in cz:
        for oy, wy in cy:
            for ox, wx in cx:
                A = A + (wz * wy * wx) * grid[:, kz + oz, ky + oy, kx + ox]
    A = A.view(3, 4, H, W)
    return A[:, 0] * image[0] + A[:, 1] * image[1] + A[:, 2] * image[2] + A[:, 3]


def slice_gradients(image, grid, dL, dtype=torch.float64):
    """(out, dL/dimage, dL/dgrid) in `dtype` under the loss sum(out * dL)"""
    im = image.to(dtype).clone().requires_grad_(True)
    gr = grid.to(dtype).clone().requires_grad_(True)
    out = slice_forward(im, gr, dtype)
    (out * dL.to(dtype)).sum().backward()
    return out.detach(), im.grad, gr.grad


def flags(image, GL):
    """[H,W] bool: the pixels exempt from the dL/dimage check"""
    z = guide(image.double())
    if GL == 1:
        return torch.zeros_like(z, dtype=torch.bool)
    fz = z * (GL - 1)
    j = torch.round(fz)
    near = ((fz - j).abs() <= FLAG_WINDOW * (GL - 1)) & (j >= 0) & (j <= GL - 1)
    black = (image == 0).all(dim=0)
    return near & ~black


@functools.lru_cache(maxsize=None)
def truth(name):
    """dict of the float64 truth of a case, the float32 restatement's errors against it and the flags"""
    image, grid, dL = scene(name)
    out, g_image, g_grid = slice_gradients(image, grid, dL)
    out32, gi32, gg32 = slice_gradients(image, grid, dL, torch.float32)
    fl = flags(image, grid.shape[1])
    ok = ~fl
    scale_i, scale_g = max(g_image.abs().max().item(), 1e-20), max(g_grid.abs().max().item(), 1e-20)
    return dict(out=out, g_image=g_image, g_grid=g_grid, flags=fl,
                restated_out=(out32.double() - out).abs().max().item(),
                restated_g_image=((gi32.double() - g_image).abs() * ok).max().item() / scale_i,
                restated_g_grid=(gg32.double() - g_grid).abs().max().item() / scale_g)


def tv_forward(grids, dtype=torch.float64):
    """sum over the three spatial axes of the mean squared forward difference along that axis; an axis of size 1 adds 0"""
    g = grids.to(dtype)
    N, C, GL, GY, GX = g.shape
    total = torch.zeros((), dtype=dtype)
    count = N * C * GL * GY * GX
    for axis, G in ((4, GX), (3, GY), (2, GL)):
        if G > 1:
            d = g.narrow(axis, 1, G - 1) - g.narrow(axis, 0, G - 1)
            total = total + (d * d).sum() / (count // G * (G - 1))
    return total


@functools.lru_cache(maxsize=None)
def tv_bank(name):
    N, GX, GY, GL, seed = TV_BANKS[name]
    g = torch.Generator().manual_seed(seed)
    return (identity_grid(GX, GY, GL, torch.float64).unsqueeze(0)
            + 0.3 * torch.randn(N, 12, GL, GY, GX, generator=g, dtype=torch.float64)).float()


@functools.lru_cache(maxsize=None)
def tv_truth(name):
    g = tv_bank(name).double().requires_grad_(True)
    tv = tv_forward(g)
    if tv.requires_grad:
        tv.backward()
    grad = g.grad if g.grad is not None else torch.zeros_like(g)
    return tv.detach(), grad

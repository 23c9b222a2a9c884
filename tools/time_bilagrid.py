"""Times the bilateral-grid colour correction (not a test): a 1920x1080 image under a 16x16x8 grid of a bank of 200.

Two parts, in ONE process after a warm-up, alternating call by call and event-timed:
  entries  msgs_bilagrid_slice_forward, msgs_bilagrid_slice_backward (both halves, the image half alone, the grid half alone),
           msgs_bilagrid_tv_forward / _backward, `--batch` calls per timing, with the derived bytes they move and the TB/s that
           makes; beside them msgs_loss_forward / msgs_loss_backward on the same image, the yardstick: they stream the same planes.
  steps    one slice forward + backward through autograd (both gradients) against the torch composition (5-D grid_sample + the
           affine product), and one total variation forward + backward against slices + mean.
The image is `--image smooth` (low-frequency colour over a black border, what a render looks like: a wave's 256 pixels touch two
or three planes of the grid) or `--image noise` (uniform noise: every wave touches all planes, the worst case of the per-wave sums).
    python tools/time_bilagrid.py [--steps 20] [--warmup 4] [--image smooth] [--json out.json]
For the kernels' own times trace by themselves:
    rocprofv3 --kernel-trace --stats -- python tools/time_bilagrid.py --only entries --steps 10"""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ms-gs_amd"), os.path.join(ROOT, "ms-gs_amd", "host"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import diff_gaussian_rasterization as dgr  # noqa: E402

# bytes per pixel: image 12 in + out 12; image 12 + dL/dout 12 in + dL/dimage 12 out (the slab and the grid come on top)
SLICE_FWD_BYTES, SLICE_BWD_BYTES = 24, 36
# msgs_loss_forward / _backward per pixel-channel (csrc/loss.hip): 8 read + 12 written, 20 read + 4 written
LOSS_FWD_BYTES, LOSS_BWD_BYTES = 3 * 20, 3 * 24


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def alternate(fns, warmup, steps):
    ms = {v: [] for v in fns}
    for it in range(warmup + steps):
        for v, fn in fns.items():
            t, _ = timed(fn)
            if it >= warmup:
                ms[v].append(t)
    row = {v: round(float(np.median(t)), 5) for v, t in ms.items()}
    row.update({f"{v}_p10_p90": [round(float(np.percentile(t, q)), 5) for q in (10, 90)] for v, t in ms.items()})
    return row


def make_image(kind, W, H, g):
    if kind == "noise":
        return (torch.rand(3, H, W, generator=g) * 1.3 - 0.1).cuda()
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32) / H, torch.arange(W, dtype=torch.float32) / W, indexing="ij")
    img = torch.stack([0.5 + 0.45 * torch.sin(2 * math.pi * (1.3 * x + 0.4 * y)), 0.5 + 0.45 * torch.cos(2 * math.pi * (0.7 * x - 1.1 * y)),
                       0.5 + 0.45 * torch.sin(2 * math.pi * (0.5 * x + 1.7 * y) + 1.0)])
    img = img + 0.01 * torch.randn(3, H, W, generator=g)
    border = ((x - 0.5).abs() > 0.45) | ((y - 0.5).abs() > 0.45)             # a black background: the guide term is off there
    img[:, border] = 0.0
    return img.cuda()


def torch_slice(image, grid):
    _, H, W = image.shape
    x = ((torch.arange(W, device=image.device, dtype=torch.float32) + 0.5) / W).view(1, W).expand(H, W)
    y = ((torch.arange(H, device=image.device, dtype=torch.float32) + 0.5) / H).view(H, 1).expand(H, W)
    z = 0.299 * image[0] + 0.587 * image[1] + 0.114 * image[2]
    coords = (torch.stack([x, y, z], dim=-1) - 0.5) * 2.0
    A = F.grid_sample(grid.unsqueeze(0), coords.view(1, 1, H, W, 3), mode="bilinear", padding_mode="border",
                      align_corners=True).view(3, 4, H, W)
    return torch.einsum("cjhw,jhw->chw", A[:, :3], image) + A[:, 3]


def torch_tv(g):
    return ((g[:, :, :, :, 1:] - g[:, :, :, :, :-1]).pow(2).mean() + (g[:, :, :, 1:] - g[:, :, :, :-1]).pow(2).mean()
            + (g[:, :, 1:] - g[:, :, :-1]).pow(2).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--grid", type=int, nargs=3, default=(16, 16, 8), metavar=("GX", "GY", "GL"))
    ap.add_argument("--bank", type=int, default=200)
    ap.add_argument("--image", choices=("smooth", "noise"), default="smooth")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=("entries", "steps"), default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    W, H, (GX, GY, GL), NB = a.width, a.height, a.grid, a.bank
    N = W * H
    g = torch.Generator().manual_seed(3)
    image = make_image(a.image, W, H, g)
    eye = torch.eye(4)[:3].reshape(12, 1, 1, 1)
    bank = (eye.view(1, 12, 1, 1, 1) + 0.05 * torch.randn(NB, 12, GL, GY, GX, generator=g)).cuda()
    grid = bank[7 % NB].contiguous()
    dL = (torch.rand(3, H, W, generator=g) - 0.5).cuda()
    row = dict(W=W, H=H, grid=[GX, GY, GL], bank=NB, image=a.image, steps=a.steps, warmup=a.warmup)

    if a.only in (None, "entries"):
        lib = dgr._C.lib
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check = dgr._C.check
        out, g_image, g_grid = torch.empty_like(image), torch.empty_like(image), torch.empty_like(grid)
        nb = int(lib.msgs_bilagrid_scratch_bytes(W, H, GX, GY, GL))
        slab = torch.empty(nb, dtype=torch.uint8, device="cuda")
        tvb = int(lib.msgs_bilagrid_tv_scratch_bytes(bank.numel()))
        tv_scratch, tv, up, g_bank = (torch.empty(tvb, dtype=torch.uint8, device="cuda"), torch.empty(1, device="cuda"),
                                      torch.ones(1, device="cuda"), torch.empty_like(bank))
        gt = (image + 0.05 * torch.randn(3, H, W, generator=g).cuda()).contiguous()
        lb = int(lib.msgs_loss_scratch_bytes(3, H, W))
        loss_scratch, out3, g_loss = torch.empty(lb, dtype=torch.uint8, device="cuda"), torch.empty(3, device="cuda"), torch.empty_like(image)

        def batch(fn):
            def run():
                for _ in range(a.batch):
                    check(fn(), "entry")
            return run

        def backward(want):
            return batch(lambda: lib.msgs_bilagrid_slice_backward(W, H, GX, GY, GL, p(image), p(grid), p(dL), want, p(g_image),
                                                                  p(g_grid), p(slab), nb, stream))
        fns = dict(
            slice_forward=batch(lambda: lib.msgs_bilagrid_slice_forward(W, H, GX, GY, GL, p(image), p(grid), p(out), stream)),
            slice_backward=backward(3), slice_backward_image_only=backward(1), slice_backward_grid_only=backward(2),
            tv_forward=batch(lambda: lib.msgs_bilagrid_tv_forward(NB, GX, GY, GL, p(bank), p(tv), p(tv_scratch), tvb, stream)),
            tv_backward=batch(lambda: lib.msgs_bilagrid_tv_backward(NB, GX, GY, GL, p(bank), p(up), p(g_bank), stream)),
            loss_forward=batch(lambda: lib.msgs_loss_forward(p(image), p(gt), 3, H, W, C.c_float(0.2), p(out3), p(loss_scratch), lb, 1,
                                                             stream)),
            loss_backward=batch(lambda: lib.msgs_loss_backward(p(image), p(gt), 3, H, W, C.c_float(0.2), p(up), p(loss_scratch), lb,
                                                               p(g_loss), stream)))
        per_call = alternate(fns, a.warmup, a.steps)
        for k, v in per_call.items():
            row[k] = [round(x / a.batch, 5) for x in v] if isinstance(v, list) else round(v / a.batch, 5)
        bank_bytes = bank.numel() * 4
        nbytes = dict(slice_forward=SLICE_FWD_BYTES * N, slice_backward=SLICE_BWD_BYTES * N + 2 * nb,
                      slice_backward_image_only=SLICE_BWD_BYTES * N, slice_backward_grid_only=24 * N + 2 * nb,
                      tv_forward=bank_bytes, tv_backward=2 * bank_bytes, loss_forward=LOSS_FWD_BYTES * N,
                      loss_backward=LOSS_BWD_BYTES * N)
        for k, b in nbytes.items():
            row[k + "_TBps"] = round(b / (row[k] * 1e-3) / 1e12, 3)
        row["slab_MB"] = round(nb / 1e6, 2)

    if a.only in (None, "steps"):
        def slice_step(fn):
            def run():
                im, gr = image.clone().requires_grad_(True), grid.clone().requires_grad_(True)
                (fn(im, gr) * dL).sum().backward()
                return im.grad, gr.grad
            return run

        def tv_step(fn):
            def run():
                b = bank.clone().requires_grad_(True)
                fn(b).backward()
                return b.grad
            return run

        row.update(alternate(dict(slice_step_hip=slice_step(dgr.bilateral_slice), slice_step_torch=slice_step(torch_slice),
                                  tv_step_hip=tv_step(dgr.total_variation_loss), tv_step_torch=tv_step(torch_tv)),
                             a.warmup, a.steps))
        row["slice_step_torch_over_hip"] = round(row["slice_step_torch"] / row["slice_step_hip"], 2)
        row["tv_step_torch_over_hip"] = round(row["tv_step_torch"] / row["tv_step_hip"], 2)
        gi, gg = slice_step(dgr.bilateral_slice)()
        ti, tg = slice_step(torch_slice)()
        row["slice_grad_image_vs_torch"] = float((gi - ti).abs().max() / ti.abs().max())
        row["slice_grad_grid_vs_torch"] = float((gg - tg).abs().max() / tg.abs().max())
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()

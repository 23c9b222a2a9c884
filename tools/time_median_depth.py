"""Times the median-depth and Gaussian-id maps (not a test): config C3 (1 M Gaussians, 1920x1080, multi-scale filters), one view.

Two parts, in ONE process after a warm-up, alternating call by call and event-timed:
  steps    forward only: render() beside render_with_median_depth() under no_grad (the forward replay alone).
           forward + backward: a render() step with a colour loss, beside render_with_median_depth() with the same colour loss
           plus a loss on median_depth (the forward replay, the slot-9 scatter and the depth variant of the backward), and
           beside render_with_median_depth() whose loss ignores the map.  Leaf gradients are dropped between iterations.
  entries  on the state ONE forward left behind: msgs_median_depth_forward and msgs_median_depth_backward, beside the yardsticks
           of the same view: msgs_distortion_forward and msgs_distortion_backward (the same staging, a back-to-front walk over
           the whole traversed list).  Also reports how the median ids are spread: distinct ids per 8x8 block (the atomics one
           wave of the backward issues) and the fraction of pixels with a median.
    python tools/time_median_depth.py [--steps 20] [--warmup 4] [--json out.json]
For the kernels' own times, trace the entries by themselves:
    rocprofv3 --kernel-trace --stats -- python tools/time_median_depth.py --only entries --steps 10
(compare blend_median_depth_forward_kernel / median_depth_backward_kernel with blend_distortion_forward_kernel /
blend_distortion_backward_kernel in the statistics)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ms-gs_amd"), os.path.join(ROOT, "ms-gs_amd", "host"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import diff_gaussian_rasterization as dgr  # noqa: E402
import scenes  # noqa: E402
from gaussian_renderer import PIPE, render, render_with_median_depth  # noqa: E402
from synthetic_model import SyntheticGaussians  # noqa: E402

ENTRIES = ("median_depth_forward", "median_depth_backward", "distortion_forward", "distortion_backward")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


def summary(ms):
    row = {v: round(float(np.median(t)), 4) for v, t in ms.items()}
    row.update({f"{v}_p10_p90": [round(float(np.percentile(t, q)), 4) for q in (10, 90)] for v, t in ms.items()})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--only", choices=("steps", "entries"), default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sc, cam, st = scenes.config(a.config)
    W, H = cam.image_width, cam.image_height
    cam, bg = cam.to("cuda"), torch.zeros(3, device="cuda")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    P = int(pc.get_xyz.shape[0])
    g = torch.Generator().manual_seed(3)
    dL = (torch.rand(3, H, W, generator=g) - 0.5).cuda()
    Gm = (torch.rand(H, W, generator=g) - 0.5).cuda()
    row = dict(config=a.config, steps=a.steps, warmup=a.warmup, P=P)

    def drop_grads():
        for n in pc.LEAVES:
            getattr(pc, n).grad = None

    def plain_forward():
        with torch.no_grad():
            render(cam, pc, PIPE, bg, **st)

    def median_forward():
        with torch.no_grad():
            render_with_median_depth(cam, pc, PIPE, bg, **st)

    def plain_step():
        out = render(cam, pc, PIPE, bg, **st)
        (out["render"] * dL).sum().backward()
        drop_grads()

    def median_step(use):
        out = render_with_median_depth(cam, pc, PIPE, bg, **st)
        loss = (out["render"] * dL).sum()
        if use:
            loss = loss + (out["median_depth"] * Gm).sum()
        loss.backward()
        drop_grads()

    if a.only != "entries":
        fns = dict(render_forward=plain_forward, median_forward=median_forward, render_step=plain_step,
                   median_step=lambda: median_step(True), median_step_map_unused=lambda: median_step(False))
        ms = {v: [] for v in fns}
        for it in range(a.warmup + a.steps):
            for v, fn in fns.items():
                t, _ = timed(fn)
                if it >= a.warmup:
                    ms[v].append(t)
        row.update(summary(ms))
        row["median_forward_plus_ms"] = round(row["median_forward"] - row["render_forward"], 4)
        row["median_step_plus_ms"] = round(row["median_step"] - row["render_step"], 4)

    if a.only in (None, "entries"):
        from gaussian_renderer import _settings
        with torch.no_grad():
            frozen = SyntheticGaussians(sc, "cuda", requires_grad=False)
        rast = dgr.GaussianRasterizer(_settings(cam, frozen, PIPE, bg, 1.0, st["filter_small"], st["filter_large"],
                                                st["fade_size"]))
        acc = dgr.ContributionAccumulator(P, "cuda")
        seen = []
        prev, dgr._contrib_probe = dgr._contrib_probe, lambda call, state: seen.append((call, state))
        try:
            with torch.no_grad():
                rast.contributions(frozen.get_xyz, frozen.get_opacity, scales=frozen.get_scaling, rotations=frozen.get_rotation,
                                   max_pixel_sizes=frozen.get_max_pixel_sizes, min_pixel_sizes=frozen.get_min_pixel_sizes,
                                   base_mask=frozen.get_base_mask, into=acc)
        finally:
            dgr._contrib_probe = prev
        call, (geom, binning, image, D) = seen[0]
        lib = dgr._C.lib
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        dmap, moment = torch.empty(H, W, device="cuda"), torch.empty(H, W, device="cuda")
        zmap, imap = torch.empty(H, W, device="cuda"), torch.empty(H, W, dtype=torch.int32, device="cuda")
        rec = torch.zeros(lib.msgs_backward_scratch_bytes(P), dtype=torch.uint8, device="cuda")
        common = (call.view_ref, P, p(geom), geom.numel(), D, p(binning), binning.numel(), p(image), image.numel())

        def med_forward():
            dgr._C.check(lib.msgs_median_depth_forward(*common, p(zmap), p(imap), stream), "msgs_median_depth_forward")

        def med_backward():
            dgr._C.check(lib.msgs_median_depth_backward(call.view_ref, P, p(imap), p(Gm), p(rec), rec.numel(), stream),
                         "msgs_median_depth_backward")

        def dist_forward():
            dgr._C.check(lib.msgs_distortion_forward(*common, p(dmap), p(moment), stream), "msgs_distortion_forward")

        def dist_backward():
            dgr._C.check(lib.msgs_distortion_backward(*common, p(moment), p(Gm), p(rec), rec.numel(), stream),
                         "msgs_distortion_backward")
        med_forward()                           # the backwards read this view's id map / moment map
        dist_forward()
        fns = dict(median_depth_forward=med_forward, median_depth_backward=med_backward, distortion_forward=dist_forward,
                   distortion_backward=dist_backward)
        ms = {v: [] for v in ENTRIES}
        for it in range(a.warmup + a.steps):
            for v in ENTRIES:
                t, _ = timed(fns[v])
                if it >= a.warmup:
                    ms[v].append(t)
        row.update(summary(ms))
        row["instances"] = int(D)
        # how the ids are spread: the backward issues one atomic per distinct id of an 8x8 block
        h8, w8 = H // 8 * 8, W // 8 * 8
        blocks = imap[:h8, :w8].view(h8 // 8, 8, w8 // 8, 8).permute(0, 2, 1, 3).reshape(-1, 64).long()
        srt = blocks.sort(dim=1).values
        distinct = 1 + (srt[:, 1:] != srt[:, :-1]).sum(1) - (srt[:, 0] < 0).long()
        row["pixels_with_a_median"] = round(float((imap >= 0).float().mean()), 4)
        row["distinct_ids_per_8x8_block_mean_max"] = [round(float(distinct.float().mean()), 2), int(distinct.max())]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()

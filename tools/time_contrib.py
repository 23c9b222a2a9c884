"""Times the contribution scores (not a test): config C3 (1 M Gaussians, 1920x1080, multi-scale filters), one view.

Two parts, in ONE process after a warm-up, alternating call by call and event-timed:
  calls    a plain no_grad forward (render) beside the whole GaussianRasterizer.contributions() call into an accumulator
           (forward + replay), without and with a weight map; reported: the medians and the added time per view;
  entries  on the state ONE forward left behind: msgs_contrib_accumulate alone (clear_first = 0: the replay kernel and nothing
           else), with and without a weight map, beside msgs_absgrad of the same view (its zero fill, replay and finish), the
           yardstick of the replay.
    python tools/time_contrib.py [--steps 40] [--warmup 8] [--json out.json]
For the kernels' own times, trace the entries by themselves:
    rocprofv3 --kernel-trace --stats -- python tools/time_contrib.py --only entries --steps 10
(compare blend_contrib_kernel with blend_absgrad_kernel in the statistics)."""
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
from gaussian_renderer import PIPE, _settings, render  # noqa: E402
from synthetic_model import SyntheticGaussians  # noqa: E402

CALLS = ("forward", "contrib", "contrib_weighted")
ENTRIES = ("replay", "replay_weighted", "absgrad_entry")


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
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--only", choices=("calls", "entries"), default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sc, cam, st = scenes.config(a.config)
    W, H = cam.image_width, cam.image_height
    cam, bg = cam.to("cuda"), torch.zeros(3, device="cuda")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    P = int(pc.get_xyz.shape[0])
    g = torch.Generator().manual_seed(3)
    wmap = torch.where(torch.rand(H, W, generator=g) < 0.25, torch.zeros(H, W), 0.25 + 2.0 * torch.rand(H, W, generator=g)).cuda()
    rast = dgr.GaussianRasterizer(_settings(cam, pc, PIPE, bg, 1.0, st["filter_small"], st["filter_large"], st["fade_size"]))
    acc = dgr.ContributionAccumulator(P, "cuda")
    row = dict(config=a.config, steps=a.steps, warmup=a.warmup, P=P)

    def contrib(pw):
        with torch.no_grad():
            rast.contributions(pc.get_xyz, pc.get_opacity, scales=pc.get_scaling, rotations=pc.get_rotation,
                               max_pixel_sizes=pc.get_max_pixel_sizes, min_pixel_sizes=pc.get_min_pixel_sizes,
                               base_mask=pc.get_base_mask, pixel_weights=pw, into=acc)

    def forward():
        with torch.no_grad():
            return render(cam, pc, PIPE, bg, **st)

    if a.only != "entries":
        fns = dict(forward=forward, contrib=lambda: contrib(None), contrib_weighted=lambda: contrib(wmap))
        ms = {v: [] for v in CALLS}
        for it in range(a.warmup + a.steps):
            for v in CALLS:
                t, _ = timed(fns[v])
                if it >= a.warmup:
                    ms[v].append(t)
        row.update(summary(ms))
        row["added_ms"] = round(row["contrib"] - row["forward"], 4)
        row["added_weighted_ms"] = round(row["contrib_weighted"] - row["forward"], 4)
        s = acc.scores()
        row["views_added"], row["seen"] = acc.views, int((s.pixel_count > 0).sum().item())

    if a.only != "calls":
        seen = []
        prev, dgr._contrib_probe = dgr._contrib_probe, lambda call, state: seen.append((call, state))
        try:
            acc.reset()
            contrib(None)
        finally:
            dgr._contrib_probe = prev
        call, (geom, binning, image, D) = seen[0]
        lib = dgr._C.lib
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        dL = scenes.grad_seed(W, H, 78).cuda().contiguous()
        scratch = torch.empty(lib.msgs_absgrad_scratch_bytes(P), dtype=torch.uint8, device="cuda")
        out = torch.empty(P, 3, device="cuda")

        def replay(pw):
            dgr._C.check(lib.msgs_contrib_accumulate(call.view_ref, P, p(geom), geom.numel(), D, p(binning), binning.numel(),
                                                     p(image), image.numel(), p(pw), p(acc.buf), acc.nbytes, 0, stream),
                         "msgs_contrib_accumulate")

        def absgrad():
            dgr._C.check(lib.msgs_absgrad(call.view_ref, P, p(geom), geom.numel(), D, p(binning), binning.numel(), p(image),
                                          image.numel(), p(dL), None, None, p(scratch), scratch.numel(), p(out), stream),
                         "msgs_absgrad")
        fns = dict(replay=lambda: replay(None), replay_weighted=lambda: replay(wmap), absgrad_entry=absgrad)
        ms = {v: [] for v in ENTRIES}
        for it in range(a.warmup + a.steps):
            for v in ENTRIES:
                t, _ = timed(fns[v])
                if it >= a.warmup:
                    ms[v].append(t)
        row.update(summary(ms))
        row["instances"] = int(D)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()

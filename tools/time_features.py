"""Times the feature channels (not a test): config C3 (1 M Gaussians, 1920x1080, multi-scale filters), one view.

Two parts, in ONE process after a warm-up, alternating call by call and event-timed:
  routes   for C = 3, 8 and 16: the FEATURE route — one render_with_features forward and the backward of a loss on the feature
           map — beside the COLOUR route doing the same job: ceil(C / 3) calls of render(..., override_color=triple) over
           background 0 with their backwards.  Leaf gradients are dropped between iterations on both sides.
           (--only colour runs the colour route alone: it needs nothing of this commit, so the parent commit can run it too.)
  entries  on the state ONE forward left behind, for one block of 8 channels: msgs_features_forward alone,
           msgs_features_backward with and without the geometry share (its zero fill, replay and finish), beside
           msgs_contrib_accumulate of the same view (clear_first = 0: the replay kernel and nothing else), the yardstick.
    python tools/time_features.py [--steps 20] [--warmup 4] [--json out.json]
For the kernels' own times, trace the entries by themselves:
    rocprofv3 --kernel-trace --stats -- python tools/time_features.py --only entries --steps 10
(compare blend_features_forward_kernel / blend_features_backward_kernel with blend_contrib_kernel in the statistics)."""
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
from gaussian_renderer import PIPE, render  # noqa: E402
from synthetic_model import SyntheticGaussians  # noqa: E402

CHANNELS = (3, 8, 16)
ENTRIES = ("features_forward", "features_backward", "features_backward_frozen", "contrib_replay")


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
    ap.add_argument("--only", choices=("routes", "colour", "entries"), default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sc, cam, st = scenes.config(a.config)
    W, H = cam.image_width, cam.image_height
    cam, bg = cam.to("cuda"), torch.zeros(3, device="cuda")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    P = int(pc.get_xyz.shape[0])
    g = torch.Generator().manual_seed(3)
    feats = torch.rand(P, max(CHANNELS), generator=g).cuda()
    G = (torch.rand(max(CHANNELS), H, W, generator=g) - 0.5).cuda()
    row = dict(config=a.config, steps=a.steps, warmup=a.warmup, P=P)

    def drop_grads():
        for n in pc.LEAVES:
            getattr(pc, n).grad = None

    def feature_route(Cn):
        from gaussian_renderer import render_with_features
        f = feats[:, :Cn].contiguous().requires_grad_(True)
        out = render_with_features(cam, pc, PIPE, bg, f, **st)
        (out["features"] * G[:Cn]).sum().backward()
        drop_grads()

    def colour_route(Cn):
        for c0 in range(0, Cn, 3):
            n = min(3, Cn - c0)
            col = torch.zeros(P, 3, device="cuda")
            col[:, :n] = feats[:, c0:c0 + n]
            col.requires_grad_(True)
            out = render(cam, pc, PIPE, bg, override_color=col, **st)
            (out["render"][:n] * G[c0:c0 + n]).sum().backward()
        drop_grads()

    if a.only != "entries":
        fns = {}
        for Cn in CHANNELS:
            if a.only != "colour":
                fns[f"features_C{Cn}"] = lambda Cn=Cn: feature_route(Cn)
            fns[f"colour_C{Cn}"] = lambda Cn=Cn: colour_route(Cn)
        ms = {v: [] for v in fns}
        for it in range(a.warmup + a.steps):
            for v, fn in fns.items():
                t, _ = timed(fn)
                if it >= a.warmup:
                    ms[v].append(t)
        row.update(summary(ms))

    if a.only in (None, "entries"):
        from gaussian_renderer import _settings
        Cn = 8
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
        f8, G8 = feats[:, :Cn].contiguous(), G[:Cn].contiguous()
        fmap = torch.empty(Cn, H, W, device="cuda")
        dfeat = torch.empty(P, Cn, device="cuda")
        scratch = torch.empty(lib.msgs_features_scratch_bytes(P, Cn), dtype=torch.uint8, device="cuda")
        rec = torch.zeros(lib.msgs_backward_scratch_bytes(P), dtype=torch.uint8, device="cuda")

        def forward():
            dgr._C.check(lib.msgs_features_forward(call.view_ref, P, p(geom), geom.numel(), D, p(binning), binning.numel(),
                                                   p(image), image.numel(), p(f8), Cn, p(fmap), stream), "msgs_features_forward")

        def backward(records):
            dgr._C.check(lib.msgs_features_backward(call.view_ref, P, p(geom), geom.numel(), D, p(binning), binning.numel(),
                                                    p(image), image.numel(), p(f8), Cn, p(G8), p(records),
                                                    records.numel() if records is not None else 0, p(scratch), scratch.numel(),
                                                    p(dfeat), stream), "msgs_features_backward")

        def replay():
            dgr._C.check(lib.msgs_contrib_accumulate(call.view_ref, P, p(geom), geom.numel(), D, p(binning), binning.numel(),
                                                     p(image), image.numel(), None, p(acc.buf), acc.nbytes, 0, stream),
                         "msgs_contrib_accumulate")
        fns = dict(features_forward=forward, features_backward=lambda: backward(rec),
                   features_backward_frozen=lambda: backward(None), contrib_replay=replay)
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

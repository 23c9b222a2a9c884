"""Times the depth-distortion map (not a test): config C3 (1 M Gaussians, 1920x1080, multi-scale filters), one view.

Two parts, in ONE process after a warm-up, alternating call by call and event-timed:
  steps    a render() forward + backward of a colour loss, beside render_with_distortion() with the same colour loss plus a
           loss on the distortion map (the forward replay, the backward replay and the depth variant of the backward), and
           beside render_with_distortion() whose loss ignores the map (the forward replay alone).  Leaf gradients are dropped
           between iterations.
  entries  on the state ONE forward left behind: msgs_distortion_forward and msgs_distortion_backward, beside the yardsticks of
           the same view: msgs_features_forward and msgs_features_backward with the geometry share for one block of 8 channels,
           and msgs_contrib_accumulate (clear_first = 0: the replay kernel and nothing else).
    python tools/time_distortion.py [--steps 20] [--warmup 4] [--json out.json]
For the kernels' own times, trace the entries by themselves:
    rocprofv3 --kernel-trace --stats -- python tools/time_distortion.py --only entries --steps 10
(compare blend_distortion_forward_kernel / blend_distortion_backward_kernel with blend_features_forward_kernel<8> /
blend_features_backward_kernel<8, true> in the statistics)."""
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
from gaussian_renderer import PIPE, render, render_with_distortion  # noqa: E402
from synthetic_model import SyntheticGaussians  # noqa: E402

ENTRIES = ("distortion_forward", "distortion_backward", "features_forward_C8", "features_backward_C8", "contrib_replay")


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
    Gx = (torch.rand(H, W, generator=g) - 0.5).cuda()
    row = dict(config=a.config, steps=a.steps, warmup=a.warmup, P=P)

    def drop_grads():
        for n in pc.LEAVES:
            getattr(pc, n).grad = None

    def plain_step():
        out = render(cam, pc, PIPE, bg, **st)
        (out["render"] * dL).sum().backward()
        drop_grads()

    def distortion_step(use):
        out = render_with_distortion(cam, pc, PIPE, bg, **st)
        loss = (out["render"] * dL).sum()
        if use:
            loss = loss + (out["distortion"] * Gx).sum()
        loss.backward()
        drop_grads()

    if a.only != "entries":
        fns = dict(render_step=plain_step, distortion_step=lambda: distortion_step(True),
                   distortion_step_map_unused=lambda: distortion_step(False))
        ms = {v: [] for v in fns}
        for it in range(a.warmup + a.steps):
            for v, fn in fns.items():
                t, _ = timed(fn)
                if it >= a.warmup:
                    ms[v].append(t)
        row.update(summary(ms))
        row["distortion_step_plus_ms"] = round(row["distortion_step"] - row["render_step"], 4)

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
        f8 = torch.rand(P, Cn, generator=g).cuda()
        G8 = (torch.rand(Cn, H, W, generator=g) - 0.5).cuda()
        fmap = torch.empty(Cn, H, W, device="cuda")
        dfeat = torch.empty(P, Cn, device="cuda")
        dmap, moment = torch.empty(H, W, device="cuda"), torch.empty(H, W, device="cuda")
        scratch = torch.empty(lib.msgs_features_scratch_bytes(P, Cn), dtype=torch.uint8, device="cuda")
        rec = torch.zeros(lib.msgs_backward_scratch_bytes(P), dtype=torch.uint8, device="cuda")
        common = (call.view_ref, P, p(geom), geom.numel(), D, p(binning), binning.numel(), p(image), image.numel())

        def dist_forward():
            dgr._C.check(lib.msgs_distortion_forward(*common, p(dmap), p(moment), stream), "msgs_distortion_forward")

        def dist_backward():
            dgr._C.check(lib.msgs_distortion_backward(*common, p(moment), p(Gx), p(rec), rec.numel(), stream),
                         "msgs_distortion_backward")

        def feat_forward():
            dgr._C.check(lib.msgs_features_forward(*common, p(f8), Cn, p(fmap), stream), "msgs_features_forward")

        def feat_backward():
            dgr._C.check(lib.msgs_features_backward(*common, p(f8), Cn, p(G8), p(rec), rec.numel(), p(scratch), scratch.numel(),
                                                    p(dfeat), stream), "msgs_features_backward")

        def replay():
            dgr._C.check(lib.msgs_contrib_accumulate(*common, None, p(acc.buf), acc.nbytes, 0, stream), "msgs_contrib_accumulate")
        dist_forward()                          # the backward reads this view's moment map
        fns = dict(distortion_forward=dist_forward, distortion_backward=dist_backward, features_forward_C8=feat_forward,
                   features_backward_C8=feat_backward, contrib_replay=replay)
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

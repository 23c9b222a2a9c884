"""Times what absgrad=True adds to a training step (not a test): config C3 (1 M Gaussians, 1920x1080, multi-scale filters), one
view per step, forward + backward on a fixed dL/dcolor, absgrad off against on — through the reference API (render /
render_with_absgrad) and through the raw-parameter entry (render_fused / render_with_absgrad(fused=True)).

The four variants alternate step by step in ONE process after a warm-up, every step is event-timed from the forward's first
launch to the backward's last (the optimizer is not part of it: the flag does not reach it); reported: the median per variant
and the added time per step.  For the kernel's own time, trace one variant by itself:
    python tools/time_absgrad.py [--steps 40] [--warmup 8] [--json out.json]
    rocprofv3 --kernel-trace --stats -- python tools/time_absgrad.py --only ref_on --steps 10
(compare blend_absgrad_kernel with the blend backward kernel of the same view in the statistics)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ms-gs_amd"), os.path.join(ROOT, "ms-gs_amd", "host"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import scenes  # noqa: E402
from gaussian_renderer import PIPE, render, render_fused, render_with_absgrad  # noqa: E402
from synthetic_model import SyntheticGaussians  # noqa: E402

VARIANTS = ("ref_off", "ref_on", "fused_off", "fused_on")


def step(variant, cam, pc, bg, dL, st):
    if variant == "ref_off":
        out = render(cam, pc, PIPE, bg, **st)
    elif variant == "fused_off":
        out = render_fused(cam, pc, PIPE, bg, **st)
    else:
        out = render_with_absgrad(cam, pc, PIPE, bg, fused=variant == "fused_on", **st)
    out["render"].backward(dL)
    for p in pc.parameters():
        p.grad = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--only", choices=VARIANTS, default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    sc, cam, st = scenes.config(a.config)
    W, H = cam.image_width, cam.image_height
    cam, bg, dL = cam.to("cuda"), torch.zeros(3, device="cuda"), scenes.grad_seed(W, H, 78).cuda()
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    variants = (a.only,) if a.only else VARIANTS
    ms = {v: [] for v in variants}
    for it in range(a.warmup + a.steps):
        for v in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = step(v, cam, pc, bg, dL, st)
            e1.record()
            torch.cuda.synchronize()
            assert hasattr(out["viewspace_points"], "absgrad") == v.endswith("_on")
            if it >= a.warmup:
                ms[v].append(e0.elapsed_time(e1))
    row = {v: round(float(np.median(t)), 4) for v, t in ms.items()}
    row.update({f"{v}_p10_p90": [round(float(np.percentile(t, q)), 4) for q in (10, 90)] for v, t in ms.items()})
    if not a.only:
        row["added_ref_ms"] = round(row["ref_on"] - row["ref_off"], 4)
        row["added_fused_ms"] = round(row["fused_on"] - row["fused_off"], 4)
    row.update(config=a.config, steps=a.steps, warmup=a.warmup)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()

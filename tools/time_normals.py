"""Times the normal maps (not a test): config C3 (1 M Gaussians, 1920x1080, multi-scale filters).

Two parts, in ONE process after a warm-up, alternating call by call and event-timed:
  entries  msgs_gaussian_normals_forward / _backward and msgs_depth_normal_forward / _backward, view and world space, `--batch`
           calls per timing, with the bytes they move and the GB/s that makes; beside them msgs_smoothing_filter_forward /
           _backward of the same model (M16), the project's streaming yardstick: one lane per Gaussian.
  steps    forward + backward through render(), render_with_features() at C = 3 (a loss on the map), render_with_median_depth()
           (a loss on the map) and render_with_normals() with normal_consistency() for depth="median" and "expected".
    python tools/time_normals.py [--steps 20] [--warmup 4] [--json out.json]
For the kernels' own times — and alpha_map_kernel's, which every render_with_normals() step launches — trace by themselves:
    rocprofv3 --kernel-trace --stats -- python tools/time_normals.py --steps 10"""
import argparse
import ctypes as C
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ms-gs_amd"), os.path.join(ROOT, "ms-gs_amd", "host"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import diff_gaussian_rasterization as dgr  # noqa: E402
import scenes  # noqa: E402
from gaussian_renderer import PIPE, _settings, render, render_with_features, render_with_median_depth  # noqa: E402
from normals import normal_consistency, render_with_normals  # noqa: E402
from synthetic_model import SyntheticGaussians  # noqa: E402

# bytes per Gaussian: means 12 + scales 12 + rotation 16 in, normal 12 + flag 1 out; rotation 16 + flag 1 + gradient 12 in, 16 out
GN_FWD_BYTES, GN_BWD_BYTES = 40 + 13, 29 + 16
# bytes per pixel: depth 4 in, normal 12 out; depth 4 + gradient 12 in, 4 out
DN_FWD_BYTES, DN_BWD_BYTES = 4 + 12, 16 + 4
# msgs_smoothing_filter_* (tools/time_filter3d.py)
SF_FWD_BYTES, SF_BWD_BYTES = 20 + 16, 36 + 16


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


def alternate(fns, warmup, steps):
    ms = {v: [] for v in fns}
    for it in range(warmup + steps):
        for v, fn in fns.items():
            t, _ = timed(fn)
            if it >= warmup:
                ms[v].append(t)
    return summary(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=("entries", "steps"), default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    warnings.filterwarnings("ignore", message=".*not recognised.*")
    sc, cam, st = scenes.config(a.config)
    W, H = cam.image_width, cam.image_height
    cam, bg = cam.to("cuda"), torch.zeros(3, device="cuda")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    P, N = int(pc.get_xyz.shape[0]), W * H
    g = torch.Generator().manual_seed(3)
    settings = _settings(cam, pc, PIPE, bg, 1.0, st["filter_small"], st["filter_large"], st["fade_size"])
    row = dict(config=a.config, steps=a.steps, warmup=a.warmup, P=P, W=W, H=H)

    if a.only in (None, "entries"):
        lib = dgr._C.lib
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        with torch.no_grad():
            m, s, r = pc._xyz.detach().contiguous(), pc._scaling.detach().contiguous(), pc._rotation.detach().contiguous()
            o = pc._opacity.detach().contiguous()
            depth = render_with_median_depth(cam, pc, PIPE, bg, **st)["median_depth"].contiguous()
        vm, cp = cam.world_view_transform.contiguous().reshape(-1), cam.camera_center.contiguous()
        nrm, flags = torch.empty(P, 3, device="cuda"), torch.empty(P, dtype=torch.uint8, device="cuda")
        g_n, g_r = torch.rand(P, 3, generator=g).cuda(), torch.empty(P, 4, device="cuda")
        nmap, g_map, g_z = torch.empty(3, H, W, device="cuda"), torch.rand(3, H, W, generator=g).cuda(), torch.empty(H, W, device="cuda")
        tx, ty = float(settings.tanfovx), float(settings.tanfovy)
        f3d = torch.full((P, 1), 0.01, device="cuda")
        s_eff, o_eff, gs, go = (torch.empty(P, n, device="cuda") for n in (3, 1, 3, 1))
        gs.uniform_(), go.uniform_()
        ds, do = torch.empty(P, 3, device="cuda"), torch.empty(P, 1, device="cuda")
        check = dgr._C.check

        def batch(fn):
            def run():
                for _ in range(a.batch):
                    check(fn(), "entry")
            return run

        fns = {}
        for world in (0, 1):
            tag = "_world" if world else ""
            fns["gaussian_normals_forward" + tag] = batch(lambda w=world: lib.msgs_gaussian_normals_forward(
                P, p(m), p(s), p(r), p(vm), p(cp), w, p(nrm), p(flags), stream))
            fns["gaussian_normals_backward" + tag] = batch(lambda w=world: lib.msgs_gaussian_normals_backward(
                P, p(r), p(flags), p(vm), w, p(g_n), p(g_r), stream))
            fns["depth_normal_forward" + tag] = batch(lambda w=world: lib.msgs_depth_normal_forward(
                W, H, tx, ty, p(depth), p(vm), w, p(nmap), stream))
            fns["depth_normal_backward" + tag] = batch(lambda w=world: lib.msgs_depth_normal_backward(
                W, H, tx, ty, p(depth), p(vm), w, p(g_map), p(g_z), stream))
        fns["smoothing_filter_forward_raw"] = batch(lambda: lib.msgs_smoothing_filter_forward(
            P, 1, p(s), p(o), p(f3d), p(s_eff), p(o_eff), stream))
        fns["smoothing_filter_backward_raw"] = batch(lambda: lib.msgs_smoothing_filter_backward(
            P, 1, p(s), p(o), p(f3d), p(gs), p(go), p(ds), p(do), stream))
        fns["gaussian_normals_forward"]()                              # (flags for the backward)
        per_call = alternate(fns, a.warmup, a.steps)
        for k, v in per_call.items():
            row[k] = [round(x / a.batch, 5) for x in v] if isinstance(v, list) else round(v / a.batch, 5)
        for k in fns:
            n, b = ((P, GN_FWD_BYTES if "forward" in k else GN_BWD_BYTES) if k.startswith("gaussian") else
                    (N, DN_FWD_BYTES if "forward" in k else DN_BWD_BYTES) if k.startswith("depth") else
                    (P, SF_FWD_BYTES if "forward" in k else SF_BWD_BYTES))
            row[k + "_GBps"] = round(b * n / (row[k] * 1e-3) / 1e9, 1)
        row["depth_valid_fraction"] = round(float((depth > 0).float().mean()), 4)

    if a.only in (None, "steps"):
        dL = (torch.rand(3, H, W, generator=g) - 0.5).cuda()
        feats = torch.rand(P, 3, generator=g).cuda().requires_grad_(True)

        def clear():
            for n in pc.LEAVES:
                getattr(pc, n).grad = None
            feats.grad = None

        def render_step():
            (render(cam, pc, PIPE, bg, **st)["render"] * dL).sum().backward()
            clear()

        def features_step():
            out = render_with_features(cam, pc, PIPE, bg, feats, **st)
            ((out["render"] * dL).sum() + (out["features"] * dL).sum()).backward()
            clear()

        def median_step():
            out = render_with_median_depth(cam, pc, PIPE, bg, **st)
            ((out["render"] * dL).sum() + (out["median_depth"] * dL[0]).sum()).backward()
            clear()

        def normals_step(depth):
            out = render_with_normals(cam, pc, PIPE, bg, depth=depth, **st)
            ((out["render"] * dL).sum() + 0.05 * normal_consistency(out)).backward()
            clear()

        row.update(alternate(dict(render_step=render_step, features3_step=features_step, median_depth_step=median_step,
                                  normals_step_median=lambda: normals_step("median"),
                                  normals_step_expected=lambda: normals_step("expected")), a.warmup, a.steps))
        # what the composition predicts: both opt-in routes on top of one plain render
        row["features3_plus_median_minus_render"] = round(row["features3_step"] + row["median_depth_step"] - row["render_step"], 4)
        row["normals_step_median_minus_that"] = round(row["normals_step_median"] - row["features3_plus_median_minus_render"], 4)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()

"""Times the antialiasing pre-pass (not a test): config C3 (1 M Gaussians, 1920x1080, multi-scale filters), one view.

Two parts, in ONE process after a warm-up, alternating call by call and event-timed:
  steps    forward + backward of a colour loss through render(), through render() with the chained getters switched off
           (their backward in autograd: the part of the antialiased step's extra time that is not the new kernels'), and
           through render_with_antialiasing(); then the same three forward-only.  Leaf gradients are dropped between
           iterations.
  entries  msgs_screen_compensation_forward and msgs_screen_compensation_backward (without and with the camera sums) on the
           model's activated tensors, `--batch` calls per timing, with the bytes they move and the GB/s that makes; beside them
           preprocess_kernel and preprocess_backward_kernel of the same view from the library's own event pairs (KernelTimer),
           the yardstick streaming kernels.
    python tools/time_antialias.py [--steps 20] [--warmup 4] [--json out.json]
For the kernels' own times, trace the entries by themselves:
    rocprofv3 --kernel-trace --stats -- python tools/time_antialias.py --only entries --steps 10"""
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
from gaussian_renderer import PIPE, _settings, render, render_with_antialiasing  # noqa: E402
from synthetic_model import SyntheticGaussians  # noqa: E402

# bytes per Gaussian with scales + rotations: means 12, opacity 4, scales 12, rotations 16 in (+ dL/do_eff 4); o_eff 4 out,
# dL/dopacity 4 + dL/dmeans3D 12 + dL/dscales 12 + dL/drotations 16 out
FWD_BYTES, BWD_BYTES = 44 + 4, 48 + 44


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
    row = dict(config=a.config, steps=a.steps, warmup=a.warmup, P=P)

    def drop_grads():
        for n in pc.LEAVES:
            getattr(pc, n).grad = None

    def step(fn, chained=True, backward=True):
        prev, dgr.chain_reference_getters = dgr.chain_reference_getters, chained
        try:
            if backward:
                (fn(cam, pc, PIPE, bg, **st)["render"] * dL).sum().backward()
                drop_grads()
            else:
                with torch.no_grad():
                    fn(cam, pc, PIPE, bg, **st)
        finally:
            dgr.chain_reference_getters = prev

    if a.only != "entries":
        row.update(alternate(dict(render_step=lambda: step(render),
                                  render_step_getters_in_autograd=lambda: step(render, chained=False),
                                  antialiasing_step=lambda: step(render_with_antialiasing)), a.warmup, a.steps))
        row.update(alternate(dict(render_forward=lambda: step(render, backward=False),
                                  antialiasing_forward=lambda: step(render_with_antialiasing, backward=False)),
                             a.warmup, a.steps))
        row["antialiasing_step_plus_ms"] = round(row["antialiasing_step"] - row["render_step"], 4)
        row["of_which_getters_in_autograd_ms"] = round(row["render_step_getters_in_autograd"] - row["render_step"], 4)
        row["antialiasing_forward_plus_ms"] = round(row["antialiasing_forward"] - row["render_forward"], 4)

    if a.only in (None, "entries"):
        with torch.no_grad():
            frozen = SyntheticGaussians(sc, "cuda", requires_grad=False)
            m, o = frozen.get_xyz.contiguous(), frozen.get_opacity.contiguous()
            s, q = frozen.get_scaling.contiguous(), frozen.get_rotation.contiguous()
        settings = _settings(cam, frozen, PIPE, bg, 1.0, st["filter_small"], st["filter_large"], st["fade_size"])
        call = dgr._Call(settings, m, None, None, o, s, q, None, None, None, None, None, None)
        lib = dgr._C.lib
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        o_eff, go = torch.empty(P, device="cuda"), torch.rand(P, generator=g).cuda()
        d_o, d_m, d_s, d_q = (torch.empty(P, n, device="cuda") for n in (1, 3, 3, 4))
        dV = torch.empty(16, device="cuda")
        scratch = torch.empty(lib.msgs_screen_compensation_scratch_bytes(P), dtype=torch.uint8, device="cuda")

        def forward():
            for _ in range(a.batch):
                dgr._C.check(lib.msgs_screen_compensation_forward(call.view_ref, call.g_ref, p(o_eff), stream), "forward")

        def backward(camera):
            for _ in range(a.batch):
                dgr._C.check(lib.msgs_screen_compensation_backward(
                    call.view_ref, call.g_ref, p(go), p(d_o), p(d_m), p(d_s), p(d_q), None, p(dV) if camera else None,
                    p(scratch) if camera else None, scratch.numel() if camera else 0, stream), "backward")

        per_call = alternate(dict(compensation_forward=forward, compensation_backward=lambda: backward(False),
                                  compensation_backward_with_camera=lambda: backward(True)), a.warmup, a.steps)
        for k, v in per_call.items():
            row[k] = [round(x / a.batch, 5) for x in v] if isinstance(v, list) else round(v / a.batch, 5)
        row["compensation_forward_GBps"] = round(FWD_BYTES * P / (row["compensation_forward"] * 1e-3) / 1e9, 1)
        row["compensation_backward_GBps"] = round(BWD_BYTES * P / (row["compensation_backward"] * 1e-3) / 1e9, 1)
        # the yardsticks: K1 and K8 + K9 of a plain step of the same view, from the library's event pairs
        timer = dgr._C.KernelTimer(only=("preprocess", "preprocess_bwd"))
        k1, k9 = [], []
        dgr._C.set_timer(timer)
        try:
            for it in range(a.warmup + a.steps):
                step(render)
                torch.cuda.synchronize()
                t = timer.read_ms()
                if it >= a.warmup:
                    k1.append(t["preprocess"])
                    k9.append(t["preprocess_bwd"])
        finally:
            dgr._C.set_timer(None)
        row["preprocess_kernel"] = round(float(np.median(k1)), 4)
        row["preprocess_backward_kernel"] = round(float(np.median(k9)), 4)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()

"""Times the 3-D smoothing filter (not a test): config C3 (1 M Gaussians, 1920x1080, multi-scale filters).

Three parts, in ONE process after a warm-up, alternating call by call and event-timed:
  sweep    compute_3d_filter over `--cameras` ring cameras (1920x1080 at f = 1000 px, halved v mod 3 times) — and
           msgs_filter3d_sweep alone on a table that is already on the device — against the torch loop that states the
           definition camera by camera — about ten launches per camera over all P, the only way to the result without the sweep
           kernel; both rules; and how far the two results are apart.
  entries  msgs_smoothing_filter_forward / _backward in both raw modes, `--batch` calls per timing, with the bytes they move
           and the GB/s that makes; beside them msgs_screen_compensation_forward / _backward of the same model (M14), the same
           class of kernel: one lane per Gaussian.
  steps    forward + backward of a colour loss through render(), through render_with_3d_filter() with raw=True and raw=False,
           and through render() fed filtered getters composed in torch (a dozen elementwise autograd nodes).
    python tools/time_filter3d.py [--steps 20] [--warmup 4] [--json out.json]
For the kernels' own times, trace by themselves:
    rocprofv3 --kernel-trace --stats -- python tools/time_filter3d.py --only entries --steps 10"""
import argparse
import ctypes as C
import json
import math
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
from filter3d import compute_3D_filter, render_with_3d_filter  # noqa: E402
from gaussian_renderer import PIPE, _settings, render  # noqa: E402
from synthetic_model import SyntheticGaussians  # noqa: E402

# bytes per Gaussian: scales 12 + opacity 4 + filter 4 in, s_eff 12 + o_eff 4 out; the backward reads the two gradients as well
FWD_BYTES, BWD_BYTES = 20 + 16, 36 + 16
# msgs_screen_compensation_* (tools/time_antialias.py)
AA_FWD_BYTES, AA_BWD_BYTES = 44 + 4, 48 + 44


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


def torch_sweep(means3D, cams, rule, variance=0.2):
    """the definition, camera by camera, as the published recipe loops (tensors on the device, one camera at a time)"""
    P, dev = means3D.shape[0], means3D.device
    valid = torch.zeros(P, dtype=torch.bool, device=dev)
    rate = torch.zeros(P, device=dev)
    zmin = torch.full((P,), float("inf"), device=dev)
    fmax = 0.0
    for cam in cams:
        M = cam.world_view_transform
        W, H = float(cam.image_width), float(cam.image_height)
        fx, fy = W / (2.0 * math.tan(0.5 * cam.FoVx)), H / (2.0 * math.tan(0.5 * cam.FoVy))
        fmax = max(fmax, fx)
        t = means3D @ M[:3, :3] + M[3, :3]
        z = t[:, 2]
        zc = z.clamp_min(0.001)
        x, y = t[:, 0] / zc * fx + W / 2.0, t[:, 1] / zc * fy + H / 2.0
        ok = (z > 0.2) & (x >= -0.15 * W) & (x <= 1.15 * W) & (y >= -0.15 * H) & (y <= 1.15 * H)
        rate = torch.where(ok, torch.maximum(rate, fx / z), rate)
        zmin = torch.where(ok, torch.minimum(zmin, z), zmin)
        valid |= ok
    nu = rate if rule == "per_camera" else fmax / zmin
    nu = torch.where(valid, nu, torch.where(valid, nu, torch.full_like(nu, float("inf"))).min())
    return (variance ** 0.5 / nu)[:, None], valid


class TorchFiltered:
    """the model with its filtered getters composed in torch: what a trainer writes without smoothing_filter()"""

    def __init__(self, pc):
        self._pc = pc

    def __getattr__(self, name):
        return getattr(self._pc, name)

    def _parts(self):
        s = self._pc.get_scaling
        s2 = torch.square(s) + torch.square(self._pc.filter_3D)
        return s, s2

    @property
    def get_scaling(self):
        return torch.sqrt(self._parts()[1])

    @property
    def get_opacity(self):
        s, s2 = self._parts()
        return self._pc.get_opacity * torch.sqrt(torch.prod(torch.square(s), dim=1) / torch.prod(s2, dim=1))[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C3")
    ap.add_argument("--cameras", type=int, default=300)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--only", choices=("sweep", "entries", "steps"), default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    warnings.filterwarnings("ignore", message=".*not recognised.*")
    sc, cam, st = scenes.config(a.config)
    W, H = cam.image_width, cam.image_height
    cam, bg = cam.to("cuda"), torch.zeros(3, device="cuda")
    pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
    P = int(pc.get_xyz.shape[0])
    g = torch.Generator().manual_seed(3)
    ring = [scenes.ring_camera(v, a.cameras, 1920 >> (v % 3), 1080 >> (v % 3)) for v in range(a.cameras)]
    row = dict(config=a.config, steps=a.steps, warmup=a.warmup, P=P, cameras=a.cameras)

    if a.only in (None, "sweep"):
        means = pc.get_xyz.detach()
        ring_dev = [c.to("cuda") for c in ring]
        few = max(2, a.steps // 5)                                     # the torch loop takes a while: fewer repetitions
        lib = dgr._C.lib
        ptr = lambda t: C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        table = dgr._camera_table(ring, means.device)
        filt, valid = torch.empty(P, 1, device="cuda"), torch.empty(P, dtype=torch.bool, device="cuda")
        scratch = torch.empty(lib.msgs_filter3d_scratch_bytes(P, a.cameras), dtype=torch.uint8, device="cuda")

        def entry(rule):                                               # the launches alone: memset, sweep kernel, finish kernel
            dgr._C.check(lib.msgs_filter3d_sweep(P, ptr(means), a.cameras, ptr(table), dgr._C.FILTER3D_RULES[rule], 0.2, ptr(filt),
                                                 ptr(valid), ptr(scratch), scratch.numel(), stream), "msgs_filter3d_sweep")

        for rule in ("per_camera", "mip_splatting"):
            row.update(alternate({f"sweep_{rule}": lambda: dgr.compute_3d_filter(means, ring, rule=rule),
                                  f"sweep_entry_{rule}": lambda: entry(rule)}, a.warmup, a.steps))
            row.update(alternate({f"torch_loop_{rule}": lambda: torch_sweep(means, ring_dev, rule)}, 1, few))
            f0, v0 = dgr.compute_3d_filter(means, ring, rule=rule)
            f1, v1 = torch_sweep(means, ring_dev, rule)
            same = v0 == v1
            rel = ((f0 - f1).abs() / f1)[same]
            row[f"sweep_vs_torch_{rule}"] = dict(
                valid_differs=int((~same).sum()), unseen=int((~v0).sum()), max_rel=float(rel.max()),
                rows_beyond_1e_5=int((rel > 1e-5).sum()))
            row[f"sweep_speedup_{rule}"] = round(row[f"torch_loop_{rule}"] / row[f"sweep_{rule}"], 1)

    compute_3D_filter(pc, ring)
    if a.only in (None, "entries"):
        lib = dgr._C.lib
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        f = pc.filter_3D
        s_eff, o_eff = torch.empty(P, 3, device="cuda"), torch.empty(P, 1, device="cuda")
        gs, go = torch.rand(P, 3, generator=g).cuda(), torch.rand(P, 1, generator=g).cuda()
        ds, do = torch.empty(P, 3, device="cuda"), torch.empty(P, 1, device="cuda")
        with torch.no_grad():
            inputs = {True: (pc._scaling.detach().contiguous(), pc._opacity.detach().contiguous()),
                      False: (pc.get_scaling.contiguous(), pc.get_opacity.contiguous())}

        def forward(raw):
            s, o = inputs[raw]
            for _ in range(a.batch):
                dgr._C.check(lib.msgs_smoothing_filter_forward(P, int(raw), p(s), p(o), p(f), p(s_eff), p(o_eff), stream), "forward")

        def backward(raw):
            s, o = inputs[raw]
            for _ in range(a.batch):
                dgr._C.check(lib.msgs_smoothing_filter_backward(P, int(raw), p(s), p(o), p(f), p(gs), p(go), p(ds), p(do), stream),
                             "backward")

        # M14's kernels on the same model, in the same session
        with torch.no_grad():
            m, o_act = pc.get_xyz.detach().contiguous(), pc.get_opacity.contiguous()
            s_act, q_act = pc.get_scaling.contiguous(), pc.get_rotation.contiguous()
        settings = _settings(cam, pc, PIPE, bg, 1.0, st["filter_small"], st["filter_large"], st["fade_size"])
        call = dgr._Call(settings, m, None, None, o_act, s_act, q_act, None, None, None, None, None, None)
        aa_o, aa_go = torch.empty(P, device="cuda"), torch.rand(P, generator=g).cuda()
        d_o, d_m, d_s, d_q = (torch.empty(P, n, device="cuda") for n in (1, 3, 3, 4))

        def aa_forward():
            for _ in range(a.batch):
                dgr._C.check(lib.msgs_screen_compensation_forward(call.view_ref, call.g_ref, p(aa_o), stream), "aa forward")

        def aa_backward():
            for _ in range(a.batch):
                dgr._C.check(lib.msgs_screen_compensation_backward(call.view_ref, call.g_ref, p(aa_go), p(d_o), p(d_m), p(d_s),
                                                                   p(d_q), None, None, None, 0, stream), "aa backward")

        per_call = alternate(dict(getters_forward=lambda: forward(False), getters_forward_raw=lambda: forward(True),
                                  getters_backward=lambda: backward(False), getters_backward_raw=lambda: backward(True),
                                  compensation_forward=aa_forward, compensation_backward=aa_backward), a.warmup, a.steps)
        for k, v in per_call.items():
            row[k] = [round(x / a.batch, 5) for x in v] if isinstance(v, list) else round(v / a.batch, 5)
        for k, b in (("getters_forward", FWD_BYTES), ("getters_forward_raw", FWD_BYTES), ("getters_backward", BWD_BYTES),
                     ("getters_backward_raw", BWD_BYTES), ("compensation_forward", AA_FWD_BYTES),
                     ("compensation_backward", AA_BWD_BYTES)):
            row[k + "_GBps"] = round(b * P / (row[k] * 1e-3) / 1e9, 1)

    if a.only in (None, "steps"):
        dL = (torch.rand(3, H, W, generator=g) - 0.5).cuda()
        composed = TorchFiltered(pc)

        def step(fn, model, **kw):
            (fn(cam, model, PIPE, bg, **st, **kw)["render"] * dL).sum().backward()
            for n in pc.LEAVES:
                getattr(pc, n).grad = None

        def plain_step():                                              # (render() refuses a filtered model on no route: it
            keep, pc.filter_3D = pc.filter_3D, None                    #  reads the getters; the filter is lifted to be sure)
            try:
                step(render, pc)
            finally:
                pc.filter_3D = keep

        row.update(alternate(dict(render_step=plain_step,
                                  filter3d_step_raw=lambda: step(render_with_3d_filter, pc, raw=True),
                                  filter3d_step_activated=lambda: step(render_with_3d_filter, pc, raw=False),
                                  filter3d_step_torch_getters=lambda: step(render, composed)), a.warmup, a.steps))
        for k in ("raw", "activated", "torch_getters"):
            row[f"filter3d_step_{k}_plus_ms"] = round(row[f"filter3d_step_{k}"] - row["render_step"], 4)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)
    print(json.dumps(row))


if __name__ == "__main__":
    main()

"""Backward time without and with camera gradients (msgs_backward vs msgs_backward_with_camera: viewmatrix, projmatrix and
campos requiring grad), at a BASELINE config (default C3): event-timed median over N backward calls per case, the two cases
alternated in one process (not a test).

    python tools/time_camera_backward.py [config] [N]
"""
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ms-gs_amd"), os.path.join(ROOT, "ms-gs_amd", "host"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch

import scenes
from gaussian_renderer import render
from parity_utils import PIPE
from synthetic_model import SyntheticGaussians

torch.autograd.set_multithreading_enabled(False)          # as bench.py: backward on the calling thread
cfg = sys.argv[1] if len(sys.argv) > 1 else "C3"
N = max(50, int(sys.argv[2]) if len(sys.argv) > 2 else 50)
sc, cam, st = scenes.config(cfg)
pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
camd, bg = cam.to("cuda"), torch.zeros(3, device="cuda")
dL = scenes.grad_seed(cam.image_width, cam.image_height, 5).to("cuda")
camg = copy.copy(camd)
camg.world_view_transform = camd.world_view_transform.clone().requires_grad_(True)
camg.full_proj_transform = camd.full_proj_transform.clone().requires_grad_(True)
camg.camera_center = camd.camera_center.clone().requires_grad_(True)


def backward_ms(camera):
    for p_ in pc.parameters():
        p_.grad = None
    out = render(camg if camera else camd, pc, PIPE, bg, **st)
    loss = (out["render"] * dL).sum()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    loss.backward()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


for _ in range(3):
    backward_ms(False), backward_ms(True)
t = {False: [], True: []}
for _ in range(N):
    for d in (False, True):
        t[d].append(backward_ms(d))
c, d = statistics.median(t[False]), statistics.median(t[True])
print(f"{cfg}: backward median over {N} calls: without camera gradients {c:.3f} ms, with {d:.3f} ms ({(d / c - 1) * 100:+.1f} %)")

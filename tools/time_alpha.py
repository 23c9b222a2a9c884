"""Step time (forward + loss + backward) of the alpha map and the background gradient against the plain call, at a BASELINE
config (default C3): event-timed medians, the four variants alternated in one process (not a test).

  (i)   colour loss, return_alpha off                 render()
  (ii)  return_alpha on, colour loss                  render_with_alpha(), alpha unused: one more streaming kernel in the forward
  (iii) colour + alpha loss                           ... and msgs_backward_with_alpha
  (iv)  (iii) with a bg leaf                          ... and msgs_bg_grad

    python tools/time_alpha.py [config] [timed steps] [warm-up steps]
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ms-gs_amd"), os.path.join(ROOT, "ms-gs_amd", "host"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch

import scenes
from gaussian_renderer import render, render_with_alpha
from parity_utils import PIPE
from synthetic_model import SyntheticGaussians

torch.autograd.set_multithreading_enabled(False)          # as bench.py: backward on the calling thread
cfg = sys.argv[1] if len(sys.argv) > 1 else "C3"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 50
WARM = int(sys.argv[3]) if len(sys.argv) > 3 else 30
sc, cam, st = scenes.config(cfg)
pc = SyntheticGaussians(sc, "cuda", requires_grad=True)
camd = cam.to("cuda")
bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
bg_leaf = bg.clone().requires_grad_(True)
dL = scenes.grad_seed(cam.image_width, cam.image_height, 5).to("cuda")
Ga = scenes.grad_seed(cam.image_width, cam.image_height, 6)[0].to("cuda")
VARIANTS = ("i", "ii", "iii", "iv")


def step_ms(v):
    for p_ in pc.parameters():
        p_.grad = None
    bg_leaf.grad = None
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    if v == "i":
        out = render(camd, pc, PIPE, bg, **st)
    else:
        out = render_with_alpha(camd, pc, PIPE, bg_leaf if v == "iv" else bg, **st)
    loss = (out["render"] * dL).sum()
    if v in ("iii", "iv"):
        loss = loss + (out["alpha"] * Ga).sum()
    loss.backward()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


for _ in range(WARM):
    for v in VARIANTS:
        step_ms(v)
t = {v: [] for v in VARIANTS}
for _ in range(N):
    for v in VARIANTS:
        t[v].append(step_ms(v))
base = statistics.median(t["i"])
for v in VARIANTS:
    m = statistics.median(t[v])
    print(f"{cfg} ({v}): step median over {N} (after {WARM} warm-up, alternated): {m:.4f} ms, min {min(t[v]):.4f} "
          f"({(m - base) * 1000:+.1f} us, {(m / base - 1) * 100:+.2f} % against (i))")

"""Times one densify_and_prune call (not a test): the GPU model surgery (ms-gs_amd/host/densify.py: msgs_densify_select +
msgs_densify_apply, one host read) against the torch restatement of the reference's sequence (tests/densify_restatement.py:
two torch.cat postfixes, two boolean-mask prunes, ~90 host synchronisations), at C3 (1 M Gaussians) and C5 (5 M).

Selection fractions close to training: ~5 % cloned, ~5 % split, ~2 % pruned.  Every timed call gets a fresh copy of the model
(the copy is not timed); event-timed medians include the host read of the segment sizes.  GB/s counts the bytes each call
must move at least: every source tensor read once, every output tensor written once.
    python tools/time_densify.py [--sizes 1000000 5000000] [--reps 7] [--json out.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ms-gs_amd"), os.path.join(ROOT, "ms-gs_amd", "host"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import densify  # noqa: E402
import densify_restatement as rs  # noqa: E402
from train_epilogue import FusedAdam  # noqa: E402

HBM_TBPS = 6.3
NAMES = (("xyz", "_xyz", (3,)), ("f_dc", "_features_dc", (1, 3)), ("f_rest", "_features_rest", (15, 3)), ("opacity", "_opacity", (1,)),
         ("occ_multiplier", "_occ_multiplier", (4, 1)), ("dc_delta", "_dc_delta", (12, 1)), ("scaling", "_scaling", (3,)),
         ("rotation", "_rotation", (4,)))
TRAINED = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
MAX_GRAD, MIN_OPACITY, EXTENT, PD = 0.0002, 0.005, 4.0, 0.01


def base_model(P, L, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    u = lambda *s: torch.rand(*s, device="cuda", generator=g)
    b = {}
    for name, attr, shp in NAMES:
        b[name] = torch.randn((P,) + shp, device="cuda", generator=g) * 0.1
    b["occ_multiplier"].fill_(1.0)
    b["dc_delta"].zero_()
    sel = u(P)
    big = u(P) < 0.5
    # max scale below / above percent_dense * extent = 0.04 for half the rows each
    m = torch.where(big, 0.05 + 0.2 * u(P), 0.005 + 0.03 * u(P))
    b["scaling"] = torch.log(m[:, None] * (0.5 + 0.5 * u(P, 3)))
    b["scaling"][:, 0] = torch.log(m)
    op = torch.where(u(P) < 0.02, torch.full((P,), 0.002, device="cuda"), 0.01 + 0.9 * u(P))
    b["opacity"] = torch.log(op / (1 - op))[:, None]
    accum = u(P, L, 1) * 1e-3
    denom = torch.ones(P, L, 1, device="cuda")
    accum[:, 0, 0] = torch.where(sel < 0.10, 4e-4, 1e-4)               # 10 % over max_grad: half clone, half split
    b["xyz_gradient_accum"], b["denom"] = accum, denom
    b["max_radii2D"] = (u(P) * 30).floor()
    b["max_pixel_sizes"] = u(P) * 4
    b["min_pixel_sizes"] = u(P) * 4
    b["base_gaussian_mask"] = u(P) < 0.3
    b["target_reso_lvl"] = torch.zeros(P, dtype=torch.int64, device="cuda")
    for n in TRAINED:
        b[f"{n}_m"] = torch.randn_like(b[n]) * 1e-3
        b[f"{n}_v"] = torch.rand_like(b[n]) * 1e-6
    return b


def fresh(b, L):
    from types import SimpleNamespace
    m = SimpleNamespace(reso_lvls=L, percent_dense=PD)
    groups = []
    for name, attr, _ in NAMES:
        p = nn.Parameter(b[name].clone(), requires_grad=name in TRAINED)
        setattr(m, attr, p)
        groups.append({"params": [p], "lr": 1e-3 if name in TRAINED else 0.0, "name": name})
    for k in ("xyz_gradient_accum", "denom", "max_radii2D", "max_pixel_sizes", "min_pixel_sizes", "base_gaussian_mask",
              "target_reso_lvl"):
        setattr(m, k, b[k].clone())
    opt = FusedAdam(groups, lr=0.0, eps=1e-15)
    for name, attr, _ in NAMES:
        if name in TRAINED:
            opt.state[getattr(m, attr)] = {"step": torch.tensor(100.0), "exp_avg": b[f"{name}_m"].clone(),
                                           "exp_avg_sq": b[f"{name}_v"].clone()}
    m.optimizer = opt
    return m


def bytes_of(m):
    n = 0
    for name, attr, _ in NAMES:
        t = getattr(m, attr)
        n += t.numel() * 4
        st = m.optimizer.state.get(t)
        if st:
            n += 2 * t.numel() * 4
    for k in ("xyz_gradient_accum", "denom", "max_radii2D", "max_pixel_sizes", "min_pixel_sizes", "base_gaussian_mask",
              "target_reso_lvl"):
        t = getattr(m, k)
        n += t.numel() * t.element_size()
    return n


def time_call(b, L, fn, reps):
    ms = []
    info = None
    for r in range(reps + 1):
        m = fresh(b, L)
        src = bytes_of(m)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.manual_seed(r)
        e0.record()
        out = fn(m)
        e1.record()
        torch.cuda.synchronize()
        if r > 0:                                   # the first call warms the allocator and the kernels
            ms.append(e0.elapsed_time(e1))
        info = (src, bytes_of(m), m._xyz.shape[0], out)
        del m
    return float(np.median(ms)), info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 5_000_000])
    ap.add_argument("--L", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rows = []
    for P in a.sizes:
        b = base_model(P, a.L)
        hip_ms, (src, dst, P_out, c) = time_call(b, a.L, lambda m: densify.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, None),
                                                 a.reps)
        ref_ms, (_, _, P_ref, _) = time_call(b, a.L, lambda m: rs.densify_and_prune(m, MAX_GRAD, MIN_OPACITY, EXTENT, None),
                                             a.reps)
        assert P_ref == P_out, (P_ref, P_out)
        moved = src + dst
        row = dict(P=P, P_out=P_out, cloned=c.clones / P, split=c.split / P, pruned=(P + c.clones + c.split - P_out) / P,
                   hip_ms=round(hip_ms, 3), torch_ms=round(ref_ms, 3), speedup=round(ref_ms / hip_ms, 1), bytes=moved,
                   hip_GBps=round(moved / hip_ms / 1e6, 0), floor_ms=round(moved / (HBM_TBPS * 1e9), 3),
                   frac_of_copy_rate=round(moved / hip_ms / 1e6 / (HBM_TBPS * 1e3), 2))
        rows.append(row)
        print(f"P={P:>9}  cloned {row['cloned']:.1%} split {row['split']:.1%} pruned {row['pruned']:.1%}  "
              f"HIP {hip_ms:.3f} ms ({row['hip_GBps']:.0f} GB/s = {row['frac_of_copy_rate']:.0%} of {HBM_TBPS} TB/s; "
              f"floor {row['floor_ms']:.3f} ms)   torch {ref_ms:.2f} ms   x{row['speedup']}", flush=True)
        del b
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()

"""Times the MCMC densification (not a test): ms-gs_amd/host/mcmc.py (msgs_mcmc_*, DESIGN.md SPEC M18) against a torch composition
of the same definitions, written here the way a trainer would write them today — the opacity-weighted draw as cumsum +
searchsorted, the relocation rule as a loop over a binomial table, index assignments for the surgery, build_scaling_rotation and
two bmm for the noise.  At 1 M Gaussians by default:

  add_position_noise                      one call on the model
  relocate_gs with 2 % dead rows          a fresh copy of the model per call (the copy is not timed)
  add_new_gs with +5 %                    likewise; the torch side appends with tests/densify_restatement.densification_postfix

HIP and torch calls alternate; event-timed medians, host reads included.
    python tools/time_mcmc.py [--P 1000000] [--reps 7] [--json out.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_mcmc.py --only kernels
runs the noise kernel and smoothing_filter_forward_kernel<true> (the streaming kernel of M16, its bandwidth yardstick) 120 times each
on the same model for the kernel trace; --stats DIR/..._results.db (or the kernel_stats.csv of --output-format csv) then prints
both kernels' rows with their GB/s."""
import argparse
import csv
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ms-gs_amd"), os.path.join(ROOT, "ms-gs_amd", "host"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import densify_restatement as drs  # noqa: E402
import mcmc  # noqa: E402
from diff_gaussian_rasterization import _backend as _C  # noqa: E402
from time_densify import NAMES, base_model, fresh  # noqa: E402

N_MAX = 51
NOISE_BYTES, FILTER_BYTES = 68, 36            # per Gaussian: 14 floats in + 3 out; 5 in + 4 out


# ---- the torch compositions ------------------------------------------------------------------------------------------------------
def noise_torch(m, gain, draws):
    with torch.no_grad():
        R = drs.build_rotation(m._rotation)
        L = R * torch.exp(m._scaling)[:, None, :]
        cov = torch.bmm(L, L.transpose(1, 2))
        o = torch.sigmoid(m._opacity)
        g = gain / (1 + torch.exp(-100 * (0.005 - o)))
        m._xyz.add_(torch.bmm(cov, draws[:, :, None]).squeeze(-1) * g)


_BINOM = None


def _binom(device):
    global _BINOM
    if _BINOM is None:
        _BINOM = torch.tensor([[math.comb(n, k) if k <= n else 0 for k in range(N_MAX)] for n in range(N_MAX)],
                              dtype=torch.float64, device=device)
    return _BINOM


def _sample_torch(opacity, u, dead=None):
    w = torch.sigmoid(opacity.double().reshape(-1))
    if dead is not None:
        w = torch.where(dead, torch.zeros_like(w), w)
    cdf = torch.cumsum(w, 0)
    src = torch.searchsorted(cdf, u * cdf[-1], right=True).clamp_(max=w.numel() - 1)
    return src, torch.bincount(src, minlength=w.numel())


def _relocation_torch(x, s, N):
    """SPEC M18 (b) in float64 for the drawn rows: x_new, s_new, c"""
    x, s = x.double(), s.double()
    log1mo = -torch.nn.functional.softplus(x)
    o = torch.sigmoid(x)
    l = log1mo / N
    on = -torch.expm1(l)
    B = _binom(x.device)
    k = torch.arange(N_MAX, device=x.device, dtype=torch.float64)
    coef = (-1.0) ** k / torch.sqrt(k + 1)
    powers = on[:, None] ** (k + 1)[None, :]
    D = torch.zeros_like(x)
    for i in range(1, N_MAX + 1):
        D += torch.where(N >= i, (B[i - 1][None, :] * coef[None, :] * powers).sum(1), torch.zeros_like(x))
    c = o / D
    x_new = torch.where(on < 0.005, torch.full_like(x, math.log(0.005 / 0.995)), torch.log(on) - l)
    return x_new.float(), (s + torch.log(c)[:, None]).float(), c.float()


def _drawn_torch(m, count):
    rows = torch.nonzero(count > 0).squeeze(1)
    N = (count[rows] + 1).clamp(max=N_MAX)
    xn, sn, c = _relocation_torch(m._opacity.detach()[rows, 0], m._scaling.detach()[rows], N)
    return rows, xn, sn, c


def _update_sources_torch(m, rows, xn, sn, c):
    m._opacity.data[rows, 0], m._scaling.data[rows] = xn, sn
    m.max_pixel_sizes[rows] *= c
    m.min_pixel_sizes[rows] *= c
    for st in m.optimizer.state.values():
        st["exp_avg"][rows] = 0
        st["exp_avg_sq"][rows] = 0


def relocate_torch(m, dead, u):
    with torch.no_grad():
        dead_rows = torch.nonzero(dead).squeeze(1)
        src, count = _sample_torch(m._opacity.detach(), u, dead)
        rows, xn, sn, c = _drawn_torch(m, count)
        at = torch.searchsorted(rows, src)
        for _, attr, _ in NAMES:
            if attr not in ("_opacity", "_scaling"):
                getattr(m, attr).data[dead_rows] = getattr(m, attr).data[src]
        m._opacity.data[dead_rows, 0], m._scaling.data[dead_rows] = xn[at], sn[at]
        m.max_pixel_sizes[dead_rows] = m.max_pixel_sizes[src] * c[at]
        m.min_pixel_sizes[dead_rows] = m.min_pixel_sizes[src] * c[at]
        m.target_reso_lvl[dead_rows] = m.target_reso_lvl[src]
        m.xyz_gradient_accum[dead_rows], m.denom[dead_rows], m.max_radii2D[dead_rows] = 0, 0, 0
        m.base_gaussian_mask[dead_rows] = False
        _update_sources_torch(m, rows, xn, sn, c)
    return int(dead_rows.numel())


def add_new_torch(m, cap_max, u):
    with torch.no_grad():
        src, count = _sample_torch(m._opacity.detach(), u)
        rows, xn, sn, c = _drawn_torch(m, count)
        at = torch.searchsorted(rows, src)
        new = {attr: getattr(m, attr).detach()[src] for _, attr, _ in NAMES}
        new["_opacity"], new["_scaling"] = xn[at][:, None], sn[at]
        pmax, pmin, tgt = m.max_pixel_sizes[src] * c[at], m.min_pixel_sizes[src] * c[at], m.target_reso_lvl[src]
        _update_sources_torch(m, rows, xn, sn, c)
    drs.densification_postfix(m, *(new[attr] for _, attr, _ in NAMES), tgt, pmax, pmin, reso_lvl=0)
    return int(u.numel())


# ---- timing ------------------------------------------------------------------------------------------------------------------------
def _events(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def alternate(b, L, hip, ref, reps):
    """medians of `reps` alternated calls, each on a fresh copy of the model; the first pair warms up.  Also the largest difference
    between the two sides' last results (xyz, opacity, scaling, max_pixel_sizes): the compositions compute the same thing"""
    ms, last = {"hip": [], "torch": []}, {}
    for r in range(reps + 1):
        for name, fn in (("hip", hip), ("torch", ref)):
            m = fresh(b, L)
            t, _ = _events(lambda: fn(m))
            if r > 0:
                ms[name].append(t)
            last[name] = [getattr(m, attr).detach() for attr in ("_xyz", "_opacity", "_scaling")] + [m.max_pixel_sizes]
            del m
    diff = max(float((x - y).abs().max()) if x.shape == y.shape else float("inf") for x, y in zip(last["hip"], last["torch"]))
    return float(np.median(ms["hip"])), float(np.median(ms["torch"])), diff


def run_kernels(b, P, L, n=120):
    """what the kernel trace looks at: n dispatches each of the noise kernel and of M16's raw getter kernel on the same model"""
    m = fresh(b, L)
    draws = torch.randn(P, 3, device="cuda")
    filt = torch.full((P,), 1e-3, device="cuda")
    s_eff, o_eff = torch.empty(P, 3, device="cuda"), torch.empty(P, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for _ in range(n):
        mcmc.add_position_noise(m, 0.00016, noise_lr=1.0, draws=draws)
        _C.check(_C.lib.msgs_smoothing_filter_forward(P, 1, ptr(m._scaling), ptr(m._opacity), ptr(filt), ptr(s_eff), ptr(o_eff),
                                                      stream), "msgs_smoothing_filter_forward")
    torch.cuda.synchronize()


def print_stats(path, P):
    """the two kernels' rows of a rocprofv3 --kernel-trace --stats run: its results database (the default output) or, with
    --output-format csv, its kernel_stats.csv"""
    per_row = lambda name: NOISE_BYTES if "mcmc_noise_kernel" in name else FILTER_BYTES if "smoothing_filter_forward_kernel" in name else 0
    found = []                               # (name, calls, mean ns)
    if path.endswith(".db"):
        import sqlite3
        db = sqlite3.connect(path)
        for name, calls, mean in db.execute("select name, count(*), avg(duration) from kernels group by name"):
            found.append((name, int(calls), float(mean)))
    else:
        with open(path) as f:
            for r in csv.DictReader(f):
                found.append((r["Name"], int(r["Calls"]), float(r["AverageNs"])))
    rows = [dict(kernel=name.split("(")[-2].split("::")[-1] if "(" in name else name, calls=calls, mean_us=round(mean / 1e3, 2),
                 GBps=round(per_row(name) * P / mean, 0)) for name, calls, mean in found if per_row(name)]
    print(json.dumps(rows))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--L", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=("calls", "kernels"), default="calls")
    ap.add_argument("--stats", default=None, help="results .db or kernel_stats.csv of a rocprofv3 run")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    P = a.P
    if a.stats is not None:
        print_stats(a.stats, P)
        return
    assert torch.cuda.is_available(), "time_mcmc.py needs a GPU"
    b = base_model(P, a.L)
    if a.only == "kernels":
        run_kernels(b, P, a.L)
        return
    rows = []
    g = torch.Generator(device="cuda").manual_seed(1)
    draws = torch.randn(P, 3, device="cuda", generator=g)
    gain = 5e5 * 0.00016
    hip, ref, diff = alternate(b, a.L, lambda m: mcmc.add_position_noise(m, 0.00016, draws=draws), lambda m: noise_torch(m, gain, draws),
                         a.reps)
    rows.append(dict(call="add_position_noise", P=P, hip_ms=round(hip, 4), torch_ms=round(ref, 3), speedup=round(ref / hip, 1),
                     hip_GBps=round(NOISE_BYTES * P / hip / 1e6, 0), max_abs_diff=diff))
    dead = torch.rand(P, device="cuda", generator=g) < 0.02
    n_dead = int(dead.sum())
    u = torch.rand(n_dead, dtype=torch.float64, device="cuda", generator=g)
    hip, ref, diff = alternate(b, a.L, lambda m: mcmc.relocate_gs(m, dead, uniforms=u), lambda m: relocate_torch(m, dead, u), a.reps)
    rows.append(dict(call="relocate_gs", P=P, dead=n_dead, hip_ms=round(hip, 3), torch_ms=round(ref, 3), speedup=round(ref / hip, 1),
                     max_abs_diff=diff))
    n_new = int(1.05 * P) - P
    u = torch.rand(n_new, dtype=torch.float64, device="cuda", generator=g)
    hip, ref, diff = alternate(b, a.L, lambda m: mcmc.add_new_gs(m, 10 * P, uniforms=u), lambda m: add_new_torch(m, 10 * P, u), a.reps)
    rows.append(dict(call="add_new_gs", P=P, added=n_new, hip_ms=round(hip, 3), torch_ms=round(ref, 3), speedup=round(ref / hip, 1),
                     max_abs_diff=diff))
    for r in rows:
        print(r, flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()

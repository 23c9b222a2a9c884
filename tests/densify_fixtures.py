"""Seeded model states for the model-surgery tests (tests/golden/make_densify_golden.py, test_densify_cpu.py,
test_densify_gpu.py): a namespace with the reference GaussianModel's attribute names plus a torch.optim.Adam / FusedAdam whose
param groups are those of gaussian_model.py:235-246, and snapshots of everything a surgery call changes.

Every value that a selection rule compares is kept at least 1e-3 relative away from its threshold, so that the roundings of the
CPU and the GPU (exp, sigmoid, a/b) cannot flip a selection; the tie tests build their exact rows themselves."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

NAMES = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
         ("occ_multiplier", "_occ_multiplier"), ("dc_delta", "_dc_delta"), ("scaling", "_scaling"), ("rotation", "_rotation"))
TRAINED = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
STATS = ("xyz_gradient_accum", "denom", "max_radii2D", "max_pixel_sizes", "min_pixel_sizes", "base_gaussian_mask",
         "target_reso_lvl")
PERCENT_DENSE, EXTENT, MAX_GRAD, MIN_OPACITY = 0.01, 4.0, 0.0002, 0.005


def _away(rng, n, thr, below=0.5):
    """n positive values, each at least 1e-3 relative away from thr: below it with probability `below`"""
    lo = thr * rng.uniform(0.2, 0.999, n)
    hi = thr * rng.uniform(1.001, 4.0, n)
    return np.where(rng.random(n) < below, lo, hi)


def make_inputs(seed, P, L, *, lvl=0, mixed_targets=True, frac_grad=0.12, frac_big=0.5, frac_low_opacity=0.05):
    """numpy arrays of one model state; column `lvl` of accum / denom carries the selection signal"""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    d = {}
    d["xyz"] = f32(rng.normal(0, 2, (P, 3)))
    d["f_dc"] = f32(rng.normal(0, 1, (P, 1, 3)))
    d["f_rest"] = f32(rng.normal(0, 0.1, (P, 15, 3)))
    # sigmoid(o) away from MIN_OPACITY
    op = np.where(rng.random(P) < frac_low_opacity, MIN_OPACITY * rng.uniform(0.2, 0.95, P), rng.uniform(0.006, 0.95, P))
    d["opacity"] = f32(np.log(op / (1 - op)))[:, None]
    d["occ_multiplier"] = np.ones((P, 4, 1), np.float32)
    d["dc_delta"] = np.zeros((P, 12, 1), np.float32)
    # max activated scale: away from percent_dense*extent, 0.1*extent and 1.6 * 0.1*extent (children of split rows)
    lim = PERCENT_DENSE * EXTENT
    m = np.where(rng.random(P) < frac_big, rng.choice([0.05, 0.2, 0.3, 0.5, 0.7, 1.2], P) * rng.uniform(0.95, 1.05, P),
                 _away(rng, P, lim, below=1.0))
    sc = m[:, None] * rng.uniform(0.3, 1.0, (P, 3))
    sc[np.arange(P), rng.integers(0, 3, P)] = m
    d["scaling"] = f32(np.log(sc))
    d["rotation"] = f32(rng.normal(0, 1, (P, 4)))
    accum = rng.uniform(0, 1e-3, (P, L, 1))
    denom = rng.integers(0, 6, (P, L, 1)).astype(np.float64)
    g = np.where(rng.random(P) < frac_grad, _away(rng, P, MAX_GRAD, below=0.0), _away(rng, P, MAX_GRAD, below=1.0))
    dn = rng.integers(1, 8, P).astype(np.float64)
    z = rng.random(P)
    dn[z < 0.04] = 0.0                                                  # denom == 0: NaN (accum 0) or inf (accum > 0)
    acc = g * dn
    acc[(z < 0.02)] = 0.0
    acc[(z >= 0.02) & (z < 0.04)] = 3e-4
    accum[:, lvl, 0], denom[:, lvl, 0] = acc, dn
    d["xyz_gradient_accum"], d["denom"] = f32(accum), f32(denom)
    d["max_radii2D"] = f32(rng.integers(0, 40, P))
    d["max_pixel_sizes"] = f32(np.where(rng.random(P) < 0.3, -1.0, rng.uniform(0.1, 8, P)))
    d["min_pixel_sizes"] = f32(np.where(rng.random(P) < 0.3, -1.0, rng.uniform(0.1, 8, P)))
    d["base_gaussian_mask"] = rng.random(P) < 0.3
    d["target_reso_lvl"] = (np.where(rng.random(P) < 0.3, rng.integers(0, L, P), 0) if mixed_targets and L > 1
                            else np.zeros(P)).astype(np.int64)
    for n in TRAINED:
        d[f"m_{n}_exp_avg"] = f32(rng.normal(0, 1e-3, d[n].shape))
        d[f"m_{n}_exp_avg_sq"] = f32(rng.uniform(0, 1e-6, d[n].shape))
        d[f"m_{n}_step"] = np.float32(7.0)
    return d


def build_model(d, device, L, *, cls=None, optimizer="adam", lr0_groups=True):
    """a model (the reference's GaussianModel when cls is given, else a namespace with its attribute names) + optimizer"""
    dev = torch.device(device)
    m = cls.__new__(cls) if cls is not None else SimpleNamespace()
    if cls is not None:
        m.setup_functions()
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    for name, attr in NAMES:
        trained = name in TRAINED
        setattr(m, attr, nn.Parameter(t(d[name]), requires_grad=trained))
    for k in STATS:
        setattr(m, k, t(d[k]))
    m.reso_lvls, m.percent_dense = L, PERCENT_DENSE
    lrs = dict(xyz=0.00016, f_dc=0.0025, f_rest=0.0025 / 20.0, opacity=0.05, occ_multiplier=0.0, dc_delta=0.0, scaling=0.005,
               rotation=0.001)
    groups = [{"params": [getattr(m, attr)], "lr": lrs[name], "name": name} for name, attr in NAMES
              if lr0_groups or name in TRAINED]
    if optimizer == "adam":
        opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    else:
        from train_epilogue import FusedAdam
        opt = FusedAdam(groups, lr=0.0, eps=1e-15)
    for name, attr in NAMES:
        if name in TRAINED:
            p = getattr(m, attr)
            opt.state[p] = {"step": torch.tensor(float(d[f"m_{name}_step"])), "exp_avg": t(d[f"m_{name}_exp_avg"]),
                            "exp_avg_sq": t(d[f"m_{name}_exp_avg_sq"])}
    m.optimizer = opt
    return m, opt


def snapshot(m, opt):
    """numpy copies of everything a surgery call produces (keys as in make_inputs)"""
    out = {}
    group_of = {g["name"]: g for g in opt.param_groups}
    for name, attr in NAMES:
        p = getattr(m, attr)
        out[name] = p.detach().cpu().numpy().copy()
        g = group_of.get(name)
        if g is not None:
            assert g["params"][0] is p, name
            st = opt.state.get(p, None)
            if st:
                out[f"m_{name}_exp_avg"] = st["exp_avg"].detach().cpu().numpy().copy()
                out[f"m_{name}_exp_avg_sq"] = st["exp_avg_sq"].detach().cpu().numpy().copy()
                out[f"m_{name}_step"] = np.float32(float(st["step"]))
    for k in STATS:
        out[k] = getattr(m, k).detach().cpu().numpy().copy()
    return out


def bits_equal(a, b):
    """same dtype, shape and bytes (NaN payloads and signed zeros included)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return np.array_equal(np.ascontiguousarray(np.atleast_1d(a)).view(np.uint8), np.ascontiguousarray(np.atleast_1d(b)).view(np.uint8))

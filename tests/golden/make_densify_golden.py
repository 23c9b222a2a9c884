"""Generates tests/golden/densify_*.npz by running the REFERENCE's own model-surgery methods on CPU tensors:
    python tests/golden/make_densify_golden.py      (needs the reference tree; build container only, never on the GPU box)

What runs is the reference's unmodified GaussianModel.densify_and_prune / grow_large_gaussians / prune_points /
densification_postfix (scene/gaussian_model.py:419-662), loaded through ref_model_loader.py, with two shims around each call:
  - torch.zeros(..., device="cuda") makes a CPU tensor (the methods allocate their zero rows on "cuda");
  - torch.normal(mean=, std=) is restated as randn(shape) * std + mean (what ATen's normal(Tensor, Tensor) does: normal_(0, 1),
    then mul_(std).add_(mean)) with the draws recorded, so the GPU tests can feed the same z.
Stored per case: the inputs (in_*), the call's arguments (arg_*), the draws (z) and every output (out_*), keys of
tests/densify_fixtures.py."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import densify_fixtures as fx  # noqa: E402
from ref_model_loader import load_gaussian_model  # noqa: E402

# name: (op, P, L, seed, extra)
CASES = {
    "densify_prune_l1": ("densify_and_prune", 200, 1, 11, dict(max_screen_size=None)),
    "densify_prune_l4": ("densify_and_prune", 200, 4, 12, dict(max_screen_size=20)),
    "densify_prune_l7": ("densify_and_prune", 160, 7, 13, dict(max_screen_size=None)),
    "densify_grow_l4": ("grow_large_gaussians", 200, 4, 14, dict(reso_lvl=2, grad_threshold=0.0002)),
    "densify_grow_l7": ("grow_large_gaussians", 160, 7, 15, dict(reso_lvl=6, grad_threshold=0.0003)),
    "densify_points_l4": ("prune_points", 200, 4, 16, {}),
    "densify_postfix_l4": ("densification_postfix", 200, 4, 17, dict(reso_lvl=3, n_new=40)),
}


class _Shims:
    def __enter__(self):
        self.zeros, self.normal = torch.zeros, torch.normal
        self.draws = []
        zeros, draws = self.zeros, self.draws

        def cpu_zeros(*a, **k):
            if str(k.get("device", "cpu")).startswith("cuda"):
                k["device"] = "cpu"
            return zeros(*a, **k)

        def normal(mean, std, *a, **k):
            assert not a and not k and mean.shape == std.shape
            z = torch.randn(mean.shape)
            draws.append(z.clone())
            return z * std + mean
        torch.zeros, torch.normal = cpu_zeros, normal
        return self

    def __exit__(self, *exc):
        torch.zeros, torch.normal = self.zeros, self.normal


def run_reference(op, d, L, extra, seed):
    GaussianModel = load_gaussian_model()
    m, opt = fx.build_model(d, "cpu", L, cls=GaussianModel)
    args = {}
    torch.manual_seed(seed)
    with _Shims() as sh:
        if op == "densify_and_prune":
            args = dict(max_grad=fx.MAX_GRAD, min_opacity=fx.MIN_OPACITY, extent=fx.EXTENT, **extra)
            m.densify_and_prune(args["max_grad"], args["min_opacity"], args["extent"], args["max_screen_size"])
        elif op == "grow_large_gaussians":
            args = dict(extra)
            m.grow_large_gaussians(args["grad_threshold"], args["reso_lvl"])
        elif op == "prune_points":
            mask = np.random.default_rng(seed).random(d["xyz"].shape[0]) < 0.3
            args = dict(mask=mask)
            m.prune_points(torch.from_numpy(mask))
        else:
            n = extra["n_new"]
            new = new_rows(seed, n, L, extra["reso_lvl"])
            args = dict(reso_lvl=extra["reso_lvl"], **{f"new_{k}": v for k, v in new.items()})
            t = {k: torch.from_numpy(v) for k, v in new.items()}
            m.densification_postfix(t["xyz"], t["f_dc"], t["f_rest"], t["opacity"], t["occ_multiplier"], t["dc_delta"],
                                    t["scaling"], t["rotation"], t["target_reso_lvl"], t["max_pixel_sizes"],
                                    t["min_pixel_sizes"], reso_lvl=extra["reso_lvl"])
        z = torch.cat(sh.draws).numpy() if sh.draws else np.zeros((0, 3), np.float32)
    return args, z, fx.snapshot(m, opt)


def new_rows(seed, n, L, lvl):
    """rows as pool_large_gaussians hands them over (target as int64 here: the reference's float column is what SPEC D1 fixes)"""
    rng = np.random.default_rng(seed + 1000)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return dict(xyz=f32(rng.normal(0, 2, (n, 3))), f_dc=f32(rng.normal(0, 1, (n, 1, 3))), f_rest=f32(rng.normal(0, .1, (n, 15, 3))),
                opacity=f32(rng.normal(0, 1, (n, 1))), occ_multiplier=np.ones((n, 4, 1), np.float32),
                dc_delta=np.zeros((n, 12, 1), np.float32), scaling=f32(rng.normal(-3, 1, (n, 3))),
                rotation=f32(rng.normal(0, 1, (n, 4))), target_reso_lvl=np.full(n, lvl, np.int64),
                max_pixel_sizes=-np.ones(n, np.float32), min_pixel_sizes=-np.ones(n, np.float32))


def main():
    for name, (op, P, L, seed, extra) in CASES.items():
        lvl = extra.get("reso_lvl", 0) if op == "grow_large_gaussians" else 0
        d = fx.make_inputs(seed, P, L, lvl=lvl)
        args, z, out = run_reference(op, d, L, extra, seed)
        rec = {"op": np.array(op), "L": np.int64(L)}
        rec.update({f"in_{k}": v for k, v in d.items()})
        for k, v in args.items():
            rec[f"arg_{k}"] = np.array(np.nan if v is None else v)
        rec["z"] = z
        rec.update({f"out_{k}": v for k, v in out.items()})
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **rec)
        print(name, op, "P", P, "->", out["xyz"].shape[0], "z", z.shape, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

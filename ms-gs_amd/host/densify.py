"""GPU model surgery for MS-GS: the densification MECHANISM of the reference's GaussianModel — what one call does to the
model's tensors and the optimizer state — as two calls of libmsgs_hip.so (msgs_densify_select + msgs_densify_apply, one host
read of the segment sizes in between) instead of ~90 host synchronisations, ~400 launches and four copies of the model:

  densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size)    gaussian_model.py:599-625 (clone, split, prune)
  grow_large_gaussians(model, grad_threshold, reso_lvl)                       gaussian_model.py:627-662
  prune_points(model, mask)                                                   gaussian_model.py:452-472
  densification_postfix(model, new_xyz, ..., new_min_pixel_sizes, reso_lvl=0)  gaussian_model.py:496-537

Each takes the reference's argument list after `model`, so `GaussianModel.densify_and_prune = densify.densify_and_prune` is a
drop-in.  Semantics, quirks included: DESIGN.md SPEC D1.  The POLICY (when to call, with which thresholds)
stays with the caller.

Model fields read: _xyz, _features_dc, _features_rest, _opacity, _occ_multiplier, _dc_delta, _scaling, _rotation,
xyz_gradient_accum / denom [P, L, 1], max_radii2D, max_pixel_sizes, min_pixel_sizes [P], base_gaussian_mask [P] bool,
target_reso_lvl [P] int64, percent_dense, reso_lvls.  The optimizer is `model.optimizer` or the `optimizer=` keyword
(torch.optim.Adam or train_epilogue.FusedAdam): its state is re-keyed as _prune_optimizer / cat_tensors_to_optimizer do — each
group keeps its state dict object and its `step`, the new nn.Parameter takes the old one's place.  Tensors of the model that no
optimizer group holds (the lr-0 groups left out, as in SyntheticGaussians.training_setup) are remapped without moments and keep
their type and requires_grad.  No torch.cuda.empty_cache(): that is allocator policy and costs the next iteration.

There is no CPU or torch fallback: CPU tensors raise.
"""
import ctypes as C
from types import SimpleNamespace

import torch
import torch.nn as nn

from diff_gaussian_rasterization import _backend as _C
from diff_gaussian_rasterization._backend import ptr as _ptr

# optimizer group name -> model attribute (gaussian_model.py:235-246)
GROUPS = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
          ("occ_multiplier", "_occ_multiplier"), ("dc_delta", "_dc_delta"), ("scaling", "_scaling"), ("rotation", "_rotation"))
STATS = ("xyz_gradient_accum", "denom", "max_radii2D", "max_pixel_sizes", "min_pixel_sizes", "base_gaussian_mask",
         "target_reso_lvl")

# row kinds of the output (include/msgs.h): kept, clone, first child, second child, grown, appended
KEEP, CLONE, CHILD1, CHILD2, GROW, APPEND = range(6)
_ESZ = {torch.float32: 4, torch.int64: 8, torch.bool: 1}


def _rules(**by_kind):
    r = [_C.DR_ZERO] * 8
    for k, v in by_kind.items():
        r[dict(keep=KEEP, clone=CLONE, child1=CHILD1, child2=CHILD2, grow=GROW, append=APPEND)[k]] = v
    return r


def _src(t, what, dtype=torch.float32):
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: tensor lives on {t.device}; the densification kernels are GPU-only (no CPU path)")
    if t.dtype != dtype:
        raise ValueError(f"{what}: need {dtype}, got {t.dtype}")
    return t.detach().contiguous()


def _width(t, P):
    w = 1
    for d in t.shape[1:]:
        w *= int(d)
    return w


class _Surgery:
    """One call: gathers the model's tensors and the optimizer's view of them, runs select + apply, installs the results."""

    def __init__(self, model, optimizer):
        self.model = model
        self.opt = optimizer if optimizer is not None else getattr(model, "optimizer", None)
        if self.opt is None:
            raise ValueError("densify: the model has no optimizer (pass optimizer=)")
        self.params = []            # (name, attr, group or None, old tensor, state dict or None)
        by_name = {}
        for group in self.opt.param_groups:
            if len(group["params"]) != 1:
                raise ValueError("densify: every optimizer group must hold exactly one tensor (gaussian_model.py:235-246)")
            by_name[group.get("name")] = group
        for name, attr in GROUPS:
            g = by_name.get(name)
            old = g["params"][0] if g is not None else getattr(model, attr)
            st = self.opt.state.get(old, None) if g is not None else None
            if st is not None and len(st) == 0:
                st = None                               # a group that has not stepped yet: no moments to carry
            if st is not None and ("exp_avg" not in st or "exp_avg_sq" not in st):
                raise ValueError(f"densify: optimizer state of '{name}' lacks exp_avg / exp_avg_sq")
            self.params.append((name, attr, g, old, st))
        self.P = int(self.params[0][3].shape[0])
        self.device = self.params[0][3].device
        if self.device.type != "cuda":
            raise RuntimeError(f"densify: the model lives on {self.device}; the densification kernels are GPU-only (no CPU path)")
        self.L = int(model.reso_lvls)
        for name, attr, g, old, st in self.params:
            if old.shape[0] != self.P:
                raise ValueError(f"densify: '{name}' has {old.shape[0]} rows, xyz has {self.P}")
        for k in STATS:
            t = getattr(model, k)
            if t.shape[0] != self.P:
                raise ValueError(f"densify: {k} has {t.shape[0]} rows, xyz has {self.P}")
        self.stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def p(self, attr):
        for name, a, g, old, st in self.params:
            if a == attr:
                return _src(old, attr)

    def select(self, mode, reso_lvl=0, n_append=0, prune_mask=None, **f):
        m = self.model
        s = _C.DensifySelect()
        s.mode, s.reso_lvl, s.reso_lvls, s.P, s.n_append = mode, int(reso_lvl), self.L, self.P, int(n_append)
        for k, v in f.items():         # thresholds land in c_float fields: rounded to float32 as torch rounds a Python float
            setattr(s, k, v)           # it compares with a float32 tensor
        keep = []
        if mode != _C.DENSIFY_PRUNE_MASK:
            for k in ("xyz_gradient_accum", "denom"):
                t = getattr(m, k)
                if t.device.type != "cuda":
                    raise RuntimeError(f"{k}: tensor lives on {t.device} (no CPU path)")
                if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != self.P * self.L:
                    raise ValueError(f"{k} must be a contiguous float32 [P, reso_lvls, 1] tensor")
            s.xyz_gradient_accum, s.denom = _ptr(m.xyz_gradient_accum), _ptr(m.denom)
        if mode == _C.DENSIFY_PRUNE:
            op, sc, tg = self.p("_opacity"), self.p("_scaling"), _src(m.target_reso_lvl, "target_reso_lvl", torch.int64)
            keep += [op, sc, tg]
            s.opacity, s.scaling, s.target_reso_lvl = _ptr(op), _ptr(sc), _ptr(tg)
        if mode == _C.DENSIFY_PRUNE_MASK:
            pm = _src(prune_mask, "mask", torch.bool)
            if pm.numel() != self.P:
                raise ValueError(f"prune_points: mask has {pm.numel()} entries, the model {self.P} rows")
            keep.append(pm)
            s.prune_mask = _ptr(pm)
        self.scratch_bytes = int(_C.lib.msgs_densify_scratch_bytes(self.P, int(n_append)))
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=self.device)
        counts = (C.c_int64 * 8)()
        with torch.cuda.device(self.device):
            _C.check(_C.lib.msgs_densify_select(C.byref(s), _ptr(self.scratch), self.scratch_bytes, counts, self.stream),
                     "msgs_densify_select")
        self.sel = s
        self.counts = SimpleNamespace(kept=counts[0], clones=counts[1], children=counts[2], split=counts[3], grown=counts[4],
                                      appended=counts[5], P_out=counts[6])
        return self.counts

    def apply(self, param_rules, moment_rules, stats_rules, *, reso_lvl=0, draws=None, append=None, constant=0):
        """param_rules(attr) / moment_rules / stats_rules(name) -> rule list; append: dict attr|stat -> tensor [n_append, ...]"""
        m, P_out = self.model, int(self.counts.P_out)
        table, outs, keep = [], {}, []

        def add(key, src, like, dtype, rules, app=None, const=0):
            w = _width(like, self.P)
            out = torch.empty((P_out,) + tuple(like.shape[1:]), dtype=dtype, device=self.device)
            outs[key] = out
            t = _C.DensifyTensor()
            t.dst, t.src, t.constant, t.width, t.elem_bytes = _ptr(out), _ptr(src), int(const), w, _ESZ[dtype]
            if app is not None:
                a = app.detach().to(self.device, dtype).contiguous()
                if a.numel() != self.counts.appended * w:
                    raise ValueError(f"densification_postfix: {key} has {a.numel()} elements, expected "
                                     f"{self.counts.appended} rows of {w}")
                keep.append(a)
                t.append_src = _ptr(a)
            for k, r in enumerate(rules):
                t.rule[k] = r
            keep.append(src)
            table.append(t)

        for name, attr, g, old, st in self.params:
            src = _src(old, attr)
            add(attr, src, old, torch.float32, param_rules(attr), append.get(attr) if append else None)
            if st is not None:
                for mk in ("exp_avg", "exp_avg_sq"):
                    ms = _src(st[mk], f"{name} {mk}")
                    if ms.numel() != src.numel():
                        raise ValueError(f"densify: optimizer state {mk} of '{name}' and the parameter differ in size")
                    add((attr, mk), ms, old, torch.float32, moment_rules())
        for k in STATS:
            t = getattr(m, k)
            dtype = {"base_gaussian_mask": torch.bool, "target_reso_lvl": torch.int64}.get(k, torch.float32)
            src = _src(t, k, dtype)
            add(k, src, t, dtype, stats_rules(k), append.get(k) if append else None,
                const=constant if k == "target_reso_lvl" else 0)
        if len(table) > _C.DENSIFY_MAX_TENSORS:
            raise ValueError("densify: too many tensors for one launch")
        a = _C.DensifyApply()
        a.P, a.n_append, a.P_out, a.n_split = self.P, int(self.counts.appended), P_out, int(self.counts.split)
        a.n_tensors, a.reso_lvl = len(table), int(reso_lvl)
        if draws is not None:
            keep.append(draws)
            a.xyz, a.scaling, a.rotation, a.draws = (_ptr(self.p("_xyz")), _ptr(self.p("_scaling")), _ptr(self.p("_rotation")),
                                                     _ptr(draws))
            keep += [self.p("_xyz"), self.p("_scaling"), self.p("_rotation")]
        arr = (_C.DensifyTensor * max(len(table), 1))(*table)
        a.tensors = arr
        with torch.cuda.device(self.device):
            _C.check(_C.lib.msgs_densify_apply(C.byref(a), _ptr(self.scratch), self.scratch_bytes, self.stream),
                     "msgs_densify_apply")
        self._install(outs)
        return outs

    def _install(self, outs):
        m, opt = self.model, self.opt
        for name, attr, g, old, st in self.params:
            new = outs[attr]
            if g is not None:           # _prune_optimizer / cat_tensors_to_optimizer: a fresh leaf in the old one's place
                param = nn.Parameter(new.requires_grad_(True))
                if st is not None:
                    st["exp_avg"], st["exp_avg_sq"] = outs[(attr, "exp_avg")], outs[(attr, "exp_avg_sq")]
                    del opt.state[old]
                    g["params"][0] = param
                    opt.state[param] = st
                else:
                    if old in opt.state:
                        del opt.state[old]
                    g["params"][0] = param
            elif isinstance(old, nn.Parameter):
                param = nn.Parameter(new, requires_grad=old.requires_grad)
            else:
                param = new.requires_grad_(old.requires_grad)
            setattr(m, attr, param)
        for k in STATS:
            setattr(m, k, outs[k])


def densify_and_prune(model, max_grad, min_opacity, extent, max_screen_size, *, optimizer=None, draws=None):
    """gaussian_model.py:599-625 in one select + apply.  draws: optional [2*n_split, 3] standard-normal tensor used in place of
    torch.randn((2*n_split, 3)) on the model's device (what torch.normal(mean=0, std) draws from the default generator)."""
    s = _Surgery(model, optimizer)
    c = s.select(_C.DENSIFY_PRUNE, 0, grad_threshold=float(max_grad), min_opacity=float(min_opacity),
                 scale_limit=float(model.percent_dense * extent), big_world_limit=float(0.1 * extent),
                 has_max_screen_size=1 if max_screen_size else 0,
                 max_screen_size=float(max_screen_size) if max_screen_size else 0.0)
    ns = int(c.split)
    if draws is None:
        draws = torch.randn((2 * ns, 3), device=s.device)
    else:
        if tuple(draws.shape) != (2 * ns, 3):
            raise ValueError(f"densify_and_prune: draws must be [{2 * ns}, 3] ({ns} rows split), got {tuple(draws.shape)}")
        draws = _src(draws.to(s.device), "draws")

    def prules(attr):
        child = {"_xyz": _C.DR_SPLIT_XYZ, "_scaling": _C.DR_SPLIT_SCALE}.get(attr, _C.DR_COPY)
        return _rules(keep=_C.DR_COPY, clone=_C.DR_COPY, child1=child, child2=child)

    def srules(k):
        if k in ("xyz_gradient_accum", "denom"):
            return _rules(keep=_C.DR_COPY_CLEAR_COL)
        if k == "max_radii2D":
            return _rules()
        if k in ("max_pixel_sizes", "min_pixel_sizes"):
            return _rules(keep=_C.DR_COPY, clone=_C.DR_COPY, child1=_C.DR_SPLIT_DIV, child2=_C.DR_SPLIT_DIV)
        if k == "base_gaussian_mask":
            return _rules(keep=_C.DR_COPY)
        return _rules(keep=_C.DR_COPY, clone=_C.DR_COPY, child1=_C.DR_COPY, child2=_C.DR_COPY)     # target_reso_lvl

    s.apply(prules, lambda: _rules(keep=_C.DR_COPY), srules, reso_lvl=0, draws=draws)
    return c


def grow_large_gaussians(model, grad_threshold, reso_lvl, *, optimizer=None):
    """gaussian_model.py:627-662: rows with |g| >= grad_threshold at level reso_lvl are appended with half the opacity, twice the
    scale and the pixel sizes, target_reso_lvl = reso_lvl; column reso_lvl of the statistics is cleared; nothing is pruned."""
    s = _Surgery(model, optimizer)
    lvl = int(reso_lvl)
    c = s.select(_C.DENSIFY_GROW, lvl, grad_threshold=float(grad_threshold))

    def prules(attr):
        return _rules(keep=_C.DR_COPY, grow={"_opacity": _C.DR_GROW_OPACITY, "_scaling": _C.DR_GROW_SCALE}.get(attr, _C.DR_COPY))

    def srules(k):
        if k in ("xyz_gradient_accum", "denom"):
            return _rules(keep=_C.DR_COPY_CLEAR_COL)
        if k == "max_radii2D":
            return _rules()
        if k in ("max_pixel_sizes", "min_pixel_sizes"):
            return _rules(keep=_C.DR_COPY, grow=_C.DR_GROW_MUL)
        if k == "base_gaussian_mask":
            return _rules(keep=_C.DR_COPY)
        return _rules(keep=_C.DR_COPY, grow=_C.DR_CONST)

    s.apply(prules, lambda: _rules(keep=_C.DR_COPY), srules, reso_lvl=lvl, constant=lvl)
    return c


def prune_points(model, mask, *, optimizer=None):
    """gaussian_model.py:452-472: remove the rows where `mask` is True from every tensor and the optimizer's moments."""
    s = _Surgery(model, optimizer)
    mask = torch.as_tensor(mask, device=s.device)
    c = s.select(_C.DENSIFY_PRUNE_MASK, 0, prune_mask=mask)
    copy = lambda *a: _rules(keep=_C.DR_COPY)
    s.apply(copy, copy, copy)
    return c


def densification_postfix(model, new_xyz, new_features_dc, new_features_rest, new_opacities, new_occ_multiplier, new_dc_delta,
                          new_scaling, new_rotation, new_target_reso_lvl, new_max_pixel_sizes, new_min_pixel_sizes, reso_lvl=0,
                          *, optimizer=None):
    """gaussian_model.py:496-537: append rows (zero moments, zero statistics, base mask False), clear column reso_lvl of the
    statistics, max_radii2D all zeros.  new_target_reso_lvl is stored as int64 whatever its dtype (the reference's torch.cat of a
    float column — what pool_large_gaussians returns — would turn the column into float32)."""
    s = _Surgery(model, optimizer)
    M = int(new_xyz.shape[0])
    lvl = int(reso_lvl)
    c = s.select(_C.DENSIFY_APPEND, lvl, n_append=M)
    append = {"_xyz": new_xyz, "_features_dc": new_features_dc, "_features_rest": new_features_rest, "_opacity": new_opacities,
              "_occ_multiplier": new_occ_multiplier, "_dc_delta": new_dc_delta, "_scaling": new_scaling, "_rotation": new_rotation,
              "target_reso_lvl": new_target_reso_lvl.to(torch.int64) if torch.is_tensor(new_target_reso_lvl) else
              torch.as_tensor(new_target_reso_lvl, dtype=torch.int64),
              "max_pixel_sizes": new_max_pixel_sizes, "min_pixel_sizes": new_min_pixel_sizes}

    def srules(k):
        if k in ("xyz_gradient_accum", "denom"):
            return _rules(keep=_C.DR_COPY_CLEAR_COL)
        if k == "max_radii2D":
            return _rules()
        if k == "base_gaussian_mask":
            return _rules(keep=_C.DR_COPY)
        return _rules(keep=_C.DR_COPY, append=_C.DR_APPEND)

    s.apply(lambda attr: _rules(keep=_C.DR_COPY, append=_C.DR_APPEND), lambda: _rules(keep=_C.DR_COPY), srules,
            reso_lvl=lvl, append=append)
    return c

"""MCMC densification for MS-GS models ("3D Gaussian Splatting as Markov Chain Monte Carlo"): the MECHANISM a trainer with a fixed
budget of Gaussians needs besides the renderer, on libmsgs_hip.so's msgs_mcmc_* (csrc/mcmc.hip).  Semantics: DESIGN.md SPEC M18.

  relocate_gs(model, dead_mask)                 dead rows become copies of opacity-sampled live rows, in place
  add_new_gs(model, cap_max)                    grow by 5 % up to cap_max with opacity-sampled rows (densification_postfix)
  relocate_and_grow(model, cap_max)             the two in upstream's order, dead = opacity <= min_opacity
  add_position_noise(model, xyz_lr)             xyz += Sigma xi * noise_lr * xyz_lr * gate(opacity), one streaming kernel
  mcmc_regularizer(model)                       opacity_reg * mean(opacity) + scale_reg * mean(scale)
  sample_by_opacity(opacity, uniforms)          the multinomial draw on its own: (source, count)

The POLICY (when to call, which rates) stays with the caller, as in densify.py.  The model and the optimizer are those of
densify.py (same fields, torch.optim.Adam or train_epilogue.FusedAdam, groups that have not stepped or are absent).  Random numbers
are tensors: `uniforms` float64 in [0, 1) for the draws (float32 uniforms are 2^-24 apart, coarser than one row's probability at a
few million Gaussians), `draws` standard normal [P, 3] for the noise; both default to torch's generator on the model's device.

There is no CPU or torch fallback: CPU tensors raise.
"""
import ctypes as C
import warnings
from types import SimpleNamespace

import torch

import densify
from densify import _Surgery, _ptr, _src, _width
from diff_gaussian_rasterization import _backend as _C

_PARAM_RULES = {"_opacity": _C.MR_OPACITY, "_scaling": _C.MR_SCALE}
_STAT_RULES = {"xyz_gradient_accum": _C.MR_ZERO, "denom": _C.MR_ZERO, "max_radii2D": _C.MR_ZERO, "max_pixel_sizes": _C.MR_PIX_MAX,
               "min_pixel_sizes": _C.MR_PIX_MIN, "base_gaussian_mask": _C.MR_ZERO, "target_reso_lvl": _C.MR_COPY}
_STAT_DTYPES = {"base_gaussian_mask": torch.bool, "target_reso_lvl": torch.int64}
# what densification_postfix takes for the new rows, in its argument order
_NEW_ROWS = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_occ_multiplier", "_dc_delta", "_scaling", "_rotation",
             "target_reso_lvl", "max_pixel_sizes", "min_pixel_sizes")


def _in_place(t, what, dtype=torch.float32):
    """the tensor itself (written through its pointer): on the GPU, of the right type, contiguous"""
    if not t.is_contiguous():
        raise ValueError(f"{what}: must be contiguous (it is written in place)")
    return _src(t, what, dtype)         # .contiguous() of a contiguous tensor is the tensor


def _uniforms(u, n, device, what):
    if u is None:
        return torch.rand(n, dtype=torch.float64, device=device)
    if u.device.type != "cuda":
        raise RuntimeError(f"{what}: uniforms live on {u.device}; the MCMC kernels are GPU-only (no CPU path)")
    if u.dtype != torch.float64:
        raise ValueError(f"{what}: uniforms must be float64 (float32 is too coarse for a draw among millions), got {u.dtype}")
    if u.numel() != n:
        raise ValueError(f"{what}: need {n} uniforms, got {u.numel()}")
    return u.detach().reshape(-1).contiguous()


class _Mcmc:
    """One call: the model's tensors as _Surgery gathers them, the CDF in scratch, then draw + relocation."""

    def __init__(self, model, optimizer, dead, what):
        s = self.s = _Surgery(model, optimizer)
        self.what = what
        self.opacity = _in_place(next(old for _, attr, _, old, _ in s.params if attr == "_opacity"), "_opacity")
        if self.opacity.numel() != s.P:
            raise ValueError(f"{what}: _opacity must be [P, 1]")
        self.dead = None
        if dead is not None:
            self.dead = _src(dead, "dead_mask", torch.bool).reshape(-1)
            if self.dead.numel() != s.P:
                raise ValueError(f"{what}: dead_mask has {self.dead.numel()} entries, the model {s.P} rows")
        self.scratch_bytes = int(_C.lib.msgs_mcmc_scratch_bytes(s.P))
        self.scratch = torch.empty(self.scratch_bytes, dtype=torch.uint8, device=s.device)
        counts = (C.c_int64 * 4)()
        with torch.cuda.device(s.device):
            _C.check(_C.lib.msgs_mcmc_prepare(s.P, _ptr(self.opacity), _ptr(self.dead), _ptr(self.scratch), self.scratch_bytes,
                                              counts, s.stream), "msgs_mcmc_prepare")
        self.n_dead, self.n_positive = int(counts[0]), int(counts[1])

    def relocate(self, u, fresh=None):
        """draw len(u) sources; write the dead rows (fresh is None) or the rows of the `fresh` blocks; update the sources"""
        s, m = self.s, self.s.model
        table, keep = [], [u]

        def add(t, rule, dtype, key, st=None):
            t = _in_place(t, key, dtype)
            e = _C.McmcTensor()
            e.data, e.width, e.elem_bytes, e.rule = _ptr(t), _width(t, s.P), densify._ESZ[dtype], rule
            if fresh is not None and key in fresh:
                e.fresh = _ptr(fresh[key])
            if st is not None:
                for mk in ("exp_avg", "exp_avg_sq"):
                    ms = _in_place(st[mk], f"{key} {mk}")
                    if ms.numel() != t.numel():
                        raise ValueError(f"{self.what}: optimizer state {mk} of '{key}' and the parameter differ in size")
                    setattr(e, mk, _ptr(ms))
                    keep.append(ms)
            keep.append(t)
            table.append(e)

        for name, attr, g, old, st in s.params:
            add(old, _PARAM_RULES.get(attr, _C.MR_COPY), torch.float32, attr, st)
        for k in densify.STATS:
            add(getattr(m, k), _STAT_RULES[k], _STAT_DTYPES.get(k, torch.float32), k)
        r = _C.McmcRelocate()
        r.P, r.n, r.in_place, r.n_tensors = s.P, int(u.numel()), 1 if fresh is None else 0, len(table)
        r.u = _ptr(u)
        arr = (_C.McmcTensor * len(table))(*table)
        r.tensors = arr
        with torch.cuda.device(s.device):
            _C.check(_C.lib.msgs_mcmc_relocate(C.byref(r), _ptr(self.scratch), self.scratch_bytes, s.stream), "msgs_mcmc_relocate")


def sample_by_opacity(opacity, uniforms, dead=None):
    """n = len(uniforms) draws with replacement, row i with probability sigmoid(opacity_i) / sum (0 where dead).  Returns
    (source [n] int32, count [P] int32), or None with a warning when no row has positive weight."""
    op = _src(opacity, "opacity").reshape(-1)
    P = op.numel()
    if dead is not None:
        dead = _src(dead, "dead", torch.bool).reshape(-1)
        if dead.numel() != P:
            raise ValueError(f"sample_by_opacity: dead has {dead.numel()} entries, opacity {P}")
    u = _uniforms(uniforms, uniforms.numel(), op.device, "sample_by_opacity")
    n = u.numel()
    source = torch.empty(n, dtype=torch.int32, device=op.device)
    count = torch.zeros(P, dtype=torch.int32, device=op.device)
    nbytes = int(_C.lib.msgs_mcmc_scratch_bytes(P))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=op.device)
    with torch.cuda.device(op.device):
        rc = _C.lib.msgs_mcmc_sample(P, _ptr(op), _ptr(dead), n, _ptr(u), _ptr(source), _ptr(count), _ptr(scratch), nbytes,
                                     C.c_void_p(torch.cuda.current_stream(op.device).cuda_stream))
    if rc == _C.ERR_NO_WEIGHT:
        warnings.warn("sample_by_opacity: no row of positive weight, nothing drawn")
        return None
    _C.check(rc, "msgs_mcmc_sample")
    return source, count


def relocate_gs(model, dead_mask, *, optimizer=None, uniforms=None):
    """Every dead row (row order) becomes a copy of a live row drawn by opacity; the drawn rows and their copies share the
    source's opacity and scale by SPEC M18 (b).  In place: P, the parameter objects and the optimizer's keys stay; drawn rows
    have their moments zeroed, dead rows keep theirs (upstream).  uniforms: float64 [n_dead].  One host read (the dead count)."""
    k = _Mcmc(model, optimizer, dead_mask, "relocate_gs")
    out = SimpleNamespace(dead=k.n_dead, relocated=0)
    if k.n_dead == 0:
        return out
    if k.n_positive == 0:
        warnings.warn("relocate_gs: no live row of positive weight to relocate to, the model is unchanged")
        return out
    k.relocate(_uniforms(uniforms, k.n_dead, k.s.device, "relocate_gs"))
    out.relocated = k.n_dead
    return out


def add_new_gs(model, cap_max, *, optimizer=None, uniforms=None, reso_lvl=0):
    """n_new = max(0, min(cap_max, int(1.05 P)) - P) rows drawn from all rows by opacity, built like relocated rows and appended
    through densify.densification_postfix (statistics: SPEC D1); the drawn rows are updated as in relocate_gs."""
    P = int(model._xyz.shape[0])
    n_new = max(0, min(int(cap_max), int(1.05 * P)) - P)
    out = SimpleNamespace(added=0, P_out=P)
    if n_new == 0:
        if model._xyz.device.type != "cuda":
            raise RuntimeError(f"add_new_gs: the model lives on {model._xyz.device}; the MCMC kernels are GPU-only (no CPU path)")
        return out
    k = _Mcmc(model, optimizer, None, "add_new_gs")
    if k.n_positive == 0:
        warnings.warn("add_new_gs: no row of positive weight to draw from, the model is unchanged")
        return out
    s, m = k.s, model
    fresh = {}
    for key in _NEW_ROWS:
        t = getattr(m, key) if key in densify.STATS else next(old for _, attr, _, old, _ in s.params if attr == key)
        fresh[key] = torch.empty((n_new,) + tuple(t.shape[1:]), dtype=t.dtype, device=s.device)
    k.relocate(_uniforms(uniforms, n_new, s.device, "add_new_gs"), fresh)
    c = densify.densification_postfix(model, *(fresh[key] for key in _NEW_ROWS), reso_lvl=reso_lvl, optimizer=s.opt)
    out.added, out.P_out = n_new, int(c.P_out)
    return out


def relocate_and_grow(model, cap_max, min_opacity=0.005, *, optimizer=None, reso_lvl=0, relocate_uniforms=None,
                      grow_uniforms=None):
    """upstream's densification step: dead = opacity <= min_opacity, relocate_gs, then add_new_gs"""
    with torch.no_grad():
        dead = (torch.sigmoid(model._opacity) <= min_opacity).reshape(-1)
    r = relocate_gs(model, dead, optimizer=optimizer, uniforms=relocate_uniforms)
    a = add_new_gs(model, cap_max, optimizer=optimizer, uniforms=grow_uniforms, reso_lvl=reso_lvl)
    return SimpleNamespace(dead=r.dead, relocated=r.relocated, added=a.added, P_out=a.P_out)


def add_position_noise(model, xyz_lr, noise_lr=5e5, *, draws=None):
    """xyz += R S^2 R^T xi * noise_lr * xyz_lr / (1 + exp(-100 (0.005 - opacity))), in place on model._xyz, after the optimizer
    step.  draws: [P, 3] standard normal (default torch.randn).  Touches no moments and needs no optimizer."""
    xyz = _in_place(model._xyz, "_xyz")
    P = int(xyz.shape[0])
    sc, rot, op = _src(model._scaling, "_scaling"), _src(model._rotation, "_rotation"), _src(model._opacity, "_opacity")
    if sc.numel() != 3 * P or rot.numel() != 4 * P or op.numel() != P or xyz.numel() != 3 * P:
        raise ValueError("add_position_noise: need _xyz [P,3], _scaling [P,3], _rotation [P,4], _opacity [P,1]")
    if draws is None:
        draws = torch.randn((P, 3), device=xyz.device)
    else:
        draws = _src(draws, "draws")
        if tuple(draws.shape) != (P, 3):
            raise ValueError(f"add_position_noise: draws must be [{P}, 3], got {tuple(draws.shape)}")
    with torch.cuda.device(xyz.device):
        _C.check(_C.lib.msgs_mcmc_noise(P, _ptr(xyz), _ptr(sc), _ptr(rot), _ptr(op), _ptr(draws), float(noise_lr) * float(xyz_lr),
                                        C.c_void_p(torch.cuda.current_stream(xyz.device).cuda_stream)), "msgs_mcmc_noise")


def mcmc_regularizer(model, opacity_reg=0.01, scale_reg=0.01):
    """the two L1 terms 3DGS-MCMC adds to the loss: opacity_reg * mean(opacity) + scale_reg * mean(scale)"""
    return opacity_reg * torch.sigmoid(model._opacity).mean() + scale_reg * torch.exp(model._scaling).mean()

"""The GPU model surgery (ms-gs_amd/host/densify.py -> msgs_densify_select / msgs_densify_apply, DESIGN.md SPEC D1) against the
reference's outputs (tests/golden/densify_*.npz) and against the torch restatement (tests/densify_restatement.py) run on the same
GPU: row count and order, dtypes and every copied value bit for bit; the transformed values of new rows within 2 ulp, the split
children's positions within the rounding bound of torch.bmm."""
import glob
import os

import numpy as np
import pytest
import torch

import densify_fixtures as fx
import densify_restatement as rs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "densify_*.npz")))
EPS = 2.0 ** -24


def _densify():
    import densify
    return densify


def call(mod, m, opt, op, args, draws=None):
    if op == "densify_and_prune":
        return mod.densify_and_prune(m, args["max_grad"], args["min_opacity"], args["extent"], args["max_screen_size"],
                                     optimizer=opt, draws=draws)
    if op == "grow_large_gaussians":
        return mod.grow_large_gaussians(m, args["grad_threshold"], args["reso_lvl"], optimizer=opt)
    if op == "prune_points":
        return mod.prune_points(m, args["mask"], optimizer=opt)
    n = args["new"]
    return mod.densification_postfix(m, n["xyz"], n["f_dc"], n["f_rest"], n["opacity"], n["occ_multiplier"], n["dc_delta"],
                                      n["scaling"], n["rotation"], n["target_reso_lvl"], n["max_pixel_sizes"],
                                      n["min_pixel_sizes"], reso_lvl=args["reso_lvl"], optimizer=opt)


def golden_args(g, dev):
    op = str(g["op"])
    if op == "densify_and_prune":
        mss = float(g["arg_max_screen_size"])
        return op, dict(max_grad=float(g["arg_max_grad"]), min_opacity=float(g["arg_min_opacity"]), extent=float(g["arg_extent"]),
                        max_screen_size=None if np.isnan(mss) else mss)
    if op == "grow_large_gaussians":
        return op, dict(grad_threshold=float(g["arg_grad_threshold"]), reso_lvl=int(g["arg_reso_lvl"]))
    if op == "prune_points":
        return op, dict(mask=torch.from_numpy(g["arg_mask"]).to(dev))
    new = {k[len("arg_new_"):]: torch.from_numpy(g[k]).to(dev) for k in g.files if k.startswith("arg_new_")}
    return op, dict(new=new, reso_lvl=int(g["arg_reso_lvl"]))


def transformed_rows(op, c, P_out):
    """rows whose values are computed rather than copied: the split children (densify) or the grown rows"""
    if op == "densify_and_prune":
        return slice(c.kept + c.clones, P_out)
    if op == "grow_large_gaussians":
        return slice(c.kept, P_out)
    return slice(P_out, P_out)


def ulp(x):
    x = np.abs(np.asarray(x, np.float32))
    return np.spacing(np.maximum(x, np.float32(np.finfo(np.float32).tiny)))


def compare(got, want, op, c, *, zmax=0.0, where=""):
    """exact except in the transformed rows: log / scale fields within 2 ulp (+ 8 ulp of 1 for logs near 0), xyz of the children
    within the rounding bound of R·s (three products and two sums, any order, FMA or not) plus the final addition, with
    |s_j| = |z_j| exp(s_parent_j) <= zmax * 1.6 * exp(s_child_j) and |R| <= 1 entrywise"""
    assert set(got) == set(want), (where, set(got) ^ set(want))
    P_out = want["xyz"].shape[0]
    tr = transformed_rows(op, c, P_out)
    for k in want:
        a, b = got[k], want[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (where, k, a.shape, b.shape)
        if tr.start == tr.stop or a.ndim == 0 or k not in ("xyz", "scaling", "opacity", "max_pixel_sizes", "min_pixel_sizes"):
            assert fx.bits_equal(a, b), (where, k, np.argwhere(a != b)[:5])
            continue
        keep = np.ones(a.shape[0], bool)
        keep[tr] = False
        assert fx.bits_equal(a[keep], b[keep]), (where, k)
        at, bt = a[tr].astype(np.float64), b[tr].astype(np.float64)
        if k == "xyz" and op == "densify_and_prune":
            continue                                      # checked below against the bound
        tol = 2 * ulp(b[tr]) + (8 * EPS if k in ("scaling", "opacity") else 0.0)
        bad = np.abs(at - bt) > tol
        assert not bad.any(), (where, k, at[bad][:4], bt[bad][:4])
    if op == "densify_and_prune" and tr.stop > tr.start:
        a, b = got["xyz"][tr].astype(np.float64), want["xyz"][tr].astype(np.float64)
        sabs = (zmax * 1.6 * np.exp(want["scaling"][tr].astype(np.float64))).sum(axis=1, keepdims=True)
        tol = 8 * EPS * sabs + 2 * ulp(want["xyz"][tr])
        bad = np.abs(a - b) > tol
        assert not bad.any(), (where, a[bad][:4], b[bad][:4])


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
@pytest.mark.parametrize("optimizer,lr0_groups", [("adam", True), ("fused", True), ("fused", False)])
def test_matches_the_reference_goldens(path, optimizer, lr0_groups):
    g = np.load(path)
    L = int(g["L"])
    d = {k[3:]: g[k] for k in g.files if k.startswith("in_")}
    m, opt = fx.build_model(d, "cuda", L, optimizer=optimizer, lr0_groups=lr0_groups)
    op, args = golden_args(g, "cuda")
    z = torch.from_numpy(g["z"]).cuda() if op == "densify_and_prune" else None
    c = call(_densify(), m, opt, op, args, draws=z)
    torch.cuda.synchronize()
    got = fx.snapshot(m, opt)
    want = {k[4:]: g[k] for k in g.files if k.startswith("out_")}
    if not lr0_groups:
        assert not m._occ_multiplier.requires_grad and not m._dc_delta.requires_grad
    assert c.P_out == want["xyz"].shape[0]
    zmax = float(np.abs(g["z"]).max()) if g["z"].size else 0.0
    compare(got, want, op, c, zmax=zmax, where=os.path.basename(path))


def _model(seed, P, L, lvl=0, optimizer="fused", **kw):
    return fx.build_model(fx.make_inputs(seed, P, L, lvl=lvl, **kw), "cuda", L, optimizer=optimizer)


def _vs_restatement(seed, P, L, op, args, *, lvl=0, check_inputs=False):
    ma, oa = _model(seed, P, L, lvl=lvl)
    mb, ob = _model(seed, P, L, lvl=lvl)
    if check_inputs:
        before = fx.snapshot(ma, oa)
        olds = {attr: getattr(ma, attr) for _, attr in fx.NAMES}
        old_stats = {k: getattr(ma, k) for k in fx.STATS}
    z = None
    if op == "densify_and_prune":
        torch.manual_seed(seed)
        c = call(_densify(), ma, oa, op, args)
        torch.manual_seed(seed)
        z = rs.densify_and_prune(mb, args["max_grad"], args["min_opacity"], args["extent"], args["max_screen_size"], optimizer=ob)
    else:
        c = call(_densify(), ma, oa, op, args)
        call(rs, mb, ob, op, args)
    torch.cuda.synchronize()
    got, want = fx.snapshot(ma, oa), fx.snapshot(mb, ob)
    assert c.P_out == want["xyz"].shape[0]
    zmax = float(z.abs().max()) if z is not None and z.numel() else 0.0
    compare(got, want, op, c, zmax=zmax, where=f"{op} P={P}")
    if check_inputs:
        lvl = args.get("reso_lvl", 0)
        for name, attr in fx.NAMES:
            assert fx.bits_equal(olds[attr].detach().cpu().numpy(), before[name]), attr
        for k in fx.STATS:
            now, was = old_stats[k].cpu().numpy(), before[k].copy()
            if k in ("xyz_gradient_accum", "denom") and op != "prune_points":
                was[:, lvl] = 0                       # the reference's own in-place clear of the tensor it replaces
            assert fx.bits_equal(now, was), k
    return c, z


def _prune_args(mss=20):
    return dict(max_grad=fx.MAX_GRAD, min_opacity=fx.MIN_OPACITY, extent=fx.EXTENT, max_screen_size=mss)


@pytest.mark.parametrize("P,L", [(200_000, 4), (1_000_000, 1), (5_000_000, 3)])
def test_densify_and_prune_matches_the_restatement_at_scale(P, L):
    c, z = _vs_restatement(P % 97, P, L, "densify_and_prune", _prune_args(), check_inputs=(P == 200_000))
    assert c.clones > 0 and c.split > 0 and c.children > 0 and c.kept + c.clones + 2 * c.children < P + c.clones + 2 * c.split


@pytest.mark.parametrize("P,L,lvl", [(300_000, 4, 2), (1_000_000, 7, 6)])
def test_grow_matches_the_restatement_at_scale(P, L, lvl):
    c, _ = _vs_restatement(7, P, L, "grow_large_gaussians", dict(grad_threshold=fx.MAX_GRAD, reso_lvl=lvl), lvl=lvl,
                           check_inputs=(P == 300_000))
    assert c.grown > 0


def test_prune_points_and_postfix_match_the_restatement():
    P, L = 250_000, 4
    rng = np.random.default_rng(3)
    mask = torch.from_numpy(rng.random(P) < 0.2).cuda()
    _vs_restatement(3, P, L, "prune_points", dict(mask=mask), check_inputs=True)
    _vs_restatement(4, P, L, "densification_postfix", dict(new=_new_rows(12345, L, 2), reso_lvl=2), check_inputs=True)


def _new_rows(n, L, lvl):
    g = torch.Generator(device="cuda").manual_seed(9)
    r = lambda *s: torch.randn(*s, generator=g, device="cuda")
    return dict(xyz=r(n, 3), f_dc=r(n, 1, 3), f_rest=r(n, 15, 3), opacity=r(n, 1), occ_multiplier=torch.ones(n, 4, 1, device="cuda"),
                dc_delta=torch.zeros(n, 12, 1, device="cuda"), scaling=r(n, 3) - 3, rotation=r(n, 4),
                target_reso_lvl=torch.full((n,), float(lvl), device="cuda"),          # float, as pool_large_gaussians returns it
                max_pixel_sizes=-torch.ones(n, device="cuda"), min_pixel_sizes=-torch.ones(n, device="cuda"))


def test_ties_pin_greater_equal_against_greater():
    """rows with g == max_grad exactly and max(exp(s)) == percent_dense * extent exactly (float32): clone (>=, <=), not split"""
    P, L = 4096, 1
    d = fx.make_inputs(21, P, L)
    thr = np.float32(fx.MAX_GRAD)
    lim = torch.tensor(fx.PERCENT_DENSE * fx.EXTENT, dtype=torch.float32)
    s = torch.log(lim).cuda()
    for _ in range(64):                                   # the float32 s whose exp on this GPU is exactly the limit
        e = torch.exp(s)
        if e.item() == lim.item():
            break
        s = torch.nextafter(s, torch.tensor(-np.inf if e.item() > lim.item() else np.inf, device="cuda"))
    assert torch.exp(s).item() == lim.item()
    tie = np.arange(0, P, 7)
    d["xyz_gradient_accum"][tie, 0, 0] = thr
    d["denom"][tie, 0, 0] = 1.0
    d["target_reso_lvl"][tie] = 0
    d["scaling"][tie] = s.item() - 1.0
    d["scaling"][tie, 1] = s.item()
    d["opacity"][tie] = 2.0
    ma, oa = fx.build_model(d, "cuda", L, optimizer="fused")
    mb, ob = fx.build_model(d, "cuda", L, optimizer="fused")
    torch.manual_seed(1)
    c = _densify().densify_and_prune(ma, fx.MAX_GRAD, fx.MIN_OPACITY, fx.EXTENT, None)
    torch.manual_seed(1)
    z = rs.densify_and_prune(mb, fx.MAX_GRAD, fx.MIN_OPACITY, fx.EXTENT, None, optimizer=ob)
    got, want = fx.snapshot(ma, oa), fx.snapshot(mb, ob)
    compare(got, want, "densify_and_prune", c, zmax=float(z.abs().max()) if z.numel() else 0.0, where="ties")
    # every tie row is cloned: its clone (same rotation bits) sits in the clone segment
    clones = got["rotation"][c.kept:c.kept + c.clones]
    for i in tie[:50]:
        assert (clones == d["rotation"][i]).all(axis=1).any(), i


def test_edge_cases():
    D = _densify()
    # nothing selected, nothing pruned
    m, o = _model(31, 5000, 2, frac_low_opacity=0.0)
    m.xyz_gradient_accum.zero_()                          # no inf rows (denom 0, accum > 0) either
    c = D.densify_and_prune(m, 1e9, 0.0, fx.EXTENT, None)
    assert (c.clones, c.split, c.P_out) == (0, 0, 5000)
    # everything pruned
    m, o = _model(32, 5000, 2, mixed_targets=False)
    c = D.densify_and_prune(m, fx.MAX_GRAD, 2.0, fx.EXTENT, None)
    assert c.P_out == 0 and m._xyz.shape == (0, 3) and m._features_rest.shape == (0, 15, 3)
    assert o.state[m._xyz]["exp_avg"].shape == (0, 3) and m.target_reso_lvl.dtype == torch.int64
    # P = 0 through every call
    c = D.densify_and_prune(m, fx.MAX_GRAD, 0.005, fx.EXTENT, 20)
    assert c.P_out == 0
    c = D.grow_large_gaussians(m, fx.MAX_GRAD, 1)
    assert c.P_out == 0
    c = D.prune_points(m, torch.zeros(0, dtype=torch.bool, device="cuda"))
    assert c.P_out == 0
    new = _new_rows(17, 2, 1)
    D.densification_postfix(m, *[new[k] for k in ("xyz", "f_dc", "f_rest", "opacity", "occ_multiplier", "dc_delta", "scaling",
                                                  "rotation", "target_reso_lvl", "max_pixel_sizes", "min_pixel_sizes")], 1)
    assert m._xyz.shape == (17, 3) and torch.equal(m._xyz.detach(), new["xyz"]) and m.target_reso_lvl.dtype == torch.int64
    assert (m.target_reso_lvl == 1).all() and not m.base_gaussian_mask.any() and o.state[m._xyz]["step"].item() == 7.0


def test_random_stream_is_torch_normal_on_the_gpu():
    """torch.normal(mean=0, std) on the GPU draws randn(2n, 3) * std + 0 — and densify_and_prune with the same seed gives the
    restatement's children (which use torch.normal's own formulation)"""
    std = torch.rand(2 * 777, 3, device="cuda") + 0.1
    torch.manual_seed(11)
    a = torch.normal(mean=torch.zeros(2 * 777, 3, device="cuda"), std=std)
    torch.manual_seed(11)
    b = torch.randn((2 * 777, 3), device="cuda") * std + torch.zeros(2 * 777, 3, device="cuda")
    assert torch.equal(a, b)
    _vs_restatement(12, 100_000, 2, "densify_and_prune", _prune_args(None), check_inputs=True)


def test_large_f_rest_past_2_31_bytes():
    """12 M rows: f_rest is 2.16 GB; grown rows and kept rows near the end against torch indexing"""
    D = _densify()
    P, L = 12_000_000, 2
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(5)
    from types import SimpleNamespace
    import torch.nn as nn
    m = SimpleNamespace(reso_lvls=L, percent_dense=fx.PERCENT_DENSE)
    m._xyz = nn.Parameter(torch.randn(P, 3, device=dev, generator=g))
    m._features_dc = nn.Parameter(torch.randn(P, 1, 3, device=dev, generator=g))
    m._features_rest = nn.Parameter(torch.randn(P, 15, 3, device=dev, generator=g))
    m._opacity = nn.Parameter(torch.randn(P, 1, device=dev, generator=g))
    m._occ_multiplier = torch.ones(P, 4, 1, device=dev)
    m._dc_delta = torch.zeros(P, 12, 1, device=dev)
    m._scaling = nn.Parameter(torch.randn(P, 3, device=dev, generator=g) - 4)
    m._rotation = nn.Parameter(torch.randn(P, 4, device=dev, generator=g))
    m.xyz_gradient_accum = torch.rand(P, L, 1, device=dev, generator=g) * 1e-3
    m.denom = torch.ones(P, L, 1, device=dev)
    m.max_radii2D = torch.zeros(P, device=dev)
    m.max_pixel_sizes = torch.rand(P, device=dev, generator=g)
    m.min_pixel_sizes = torch.rand(P, device=dev, generator=g)
    m.base_gaussian_mask = torch.zeros(P, dtype=torch.bool, device=dev)
    m.target_reso_lvl = torch.zeros(P, dtype=torch.int64, device=dev)
    from train_epilogue import FusedAdam
    opt = FusedAdam([{"params": [m._features_rest], "lr": 1e-3, "name": "f_rest"}], lr=0.0, eps=1e-15)
    opt.state[m._features_rest] = {"step": torch.tensor(3.0), "exp_avg": torch.randn(P, 15, 3, device=dev, generator=g),
                                   "exp_avg_sq": torch.rand(P, 15, 3, device=dev, generator=g)}
    m.optimizer = opt
    assert m._features_rest.numel() * 4 > 2 ** 31
    fr = m._features_rest.detach()
    mom = opt.state[m._features_rest]["exp_avg"]
    sel = torch.sqrt((m.xyz_gradient_accum[:, 1, 0] / m.denom[:, 1, 0]) ** 2) >= 9e-4
    idx = torch.nonzero(sel).squeeze(1)
    tail_src = fr[idx[-2000:]].clone()
    kept_tail = fr[-3000:].clone()
    mom_tail = mom[-3000:].clone()
    c = D.grow_large_gaussians(m, 9e-4, 1)
    assert c.grown == idx.numel() and c.P_out == P + idx.numel()
    out = m._features_rest.detach()
    assert torch.equal(out[-2000:], tail_src)
    assert torch.equal(out[P - 3000:P], kept_tail)
    st = opt.state[m._features_rest]
    assert torch.equal(st["exp_avg"][P - 3000:P], mom_tail) and not st["exp_avg"][P:].any()
    del fr, mom, out, st
    # prune everything but the last rows: the far end lands at the front
    mask = torch.ones(m._xyz.shape[0], dtype=torch.bool, device=dev)
    mask[-5:] = False
    last = m._features_rest.detach()[-5:].clone()
    D.prune_points(m, mask)
    assert torch.equal(m._features_rest.detach(), last)


def test_fused_train_iteration_after_densify_step_in_backward_is_bit_identical():
    """densify both copies of a trained model the same way, then train one with the separate FusedAdam step and one with the step
    inside the backward (the optimizer is installed again by fused_train_iteration on every call): bit-identical parameters"""
    from parity_utils import PIPE, small_scene
    from synthetic_model import SyntheticGaussians
    from train_epilogue import FusedAdam
    from train_step import fused_train_iteration
    D = _densify()
    W, H = 160, 128
    sc, cam = small_scene(6000, W, H, 21, multiscale=True, scale_k=0.004 * 1920.0 / W * 0.2)
    st = dict(filter_small=True, filter_large=True, fade_size=0.0)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    bg = torch.zeros(3).cuda()
    camd = cam.to("cuda")
    a, b = SyntheticGaussians(sc, "cuda"), SyntheticGaussians(sc, "cuda")
    oa = FusedAdam(a.training_setup(4, sc.target_reso_lvl), lr=0.0, eps=1e-15)
    ob = FusedAdam(b.training_setup(4, sc.target_reso_lvl), lr=0.0, eps=1e-15)
    for mod, opt in ((a, oa), (b, ob)):
        mod.percent_dense = 0.01
        for _ in range(3):
            fused_train_iteration(mod, opt, camd, gt, PIPE, bg, **st)
    g = (a.xyz_gradient_accum[:, 0] / a.denom[:, 0]).nan_to_num(0)
    thr = float(torch.quantile(g[g > 0], 0.8))
    ext = float(torch.exp(a._scaling.detach()).max(dim=1).values.median()) / 0.01
    P0 = a._xyz.shape[0]
    torch.manual_seed(3)
    ca = D.densify_and_prune(a, thr, 0.005, ext, None, optimizer=oa)
    torch.manual_seed(3)
    cb = D.densify_and_prune(b, thr, 0.005, ext, None, optimizer=ob)
    assert ca.P_out == cb.P_out and ca.clones > 0 and ca.split > 0 and a._xyz.shape[0] != P0
    for n in a.LEAVES:
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    for it in range(4):
        la, _, _ = fused_train_iteration(a, oa, camd, gt, PIPE, bg, **st)
        lb, _, _ = fused_train_iteration(b, ob, camd, gt, PIPE, bg, step_in_backward=True, **st)
        assert torch.equal(la, lb), it
    for n in a.LEAVES:
        p, q = getattr(a, n), getattr(b, n)
        assert torch.equal(p, q), n
        assert torch.equal(oa.state[p]["exp_avg"], ob.state[q]["exp_avg"]), n
        assert oa.state[p]["step"].item() == ob.state[q]["step"].item() == 7
    for k in ("xyz_gradient_accum", "denom", "max_radii2D", "max_pixel_sizes", "min_pixel_sizes"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_update_training_stats_accepts_the_model_after_an_insertion():
    """pool_large_gaussians rows (float target column) through the GPU densification_postfix: target_reso_lvl stays int64 and
    update_training_stats takes the model (the reference's postfix would have made the column float32)"""
    from parity_utils import PIPE, small_scene
    from synthetic_model import SyntheticGaussians
    from train_epilogue import FusedAdam, update_training_stats
    from train_step import fused_train_iteration
    from voxel_pool import pool_large_gaussians
    D = _densify()
    W, H = 160, 128
    sc, cam = small_scene(5000, W, H, 22, multiscale=True, scale_k=0.004 * 1920.0 / W * 0.2)
    m = SyntheticGaussians(sc, "cuda")
    opt = FusedAdam(m.training_setup(4, sc.target_reso_lvl), lr=0.0, eps=1e-15)
    P = m._xyz.shape[0]
    mask = torch.rand(P, generator=torch.Generator().manual_seed(2)).cuda() < 0.3
    new = pool_large_gaussians(m._xyz.detach(), m._features_dc.detach(), m._features_rest.detach(), m._opacity.detach(),
                               m._occ_multiplier, m._dc_delta, m._rotation.detach(), m._scaling.detach(), m.max_pixel_sizes,
                               m.min_pixel_sizes, mask, torch.rand(P, device="cuda") + 0.5, 2, 4.0)
    assert new["target_reso_lvl"].dtype == torch.float32
    D.densification_postfix(m, new["xyz"], new["features_dc"], new["features_rest"], new["opacity"], new["occ_multiplier"],
                            new["dc_delta"], new["scaling"], new["rotation"], new["target_reso_lvl"], new["max_pixel_sizes"],
                            new["min_pixel_sizes"], reso_lvl=2, optimizer=opt)
    M = new["xyz"].shape[0]
    assert m._xyz.shape[0] == P + M and m.target_reso_lvl.dtype == torch.int64 and (m.target_reso_lvl[P:] == 2).all()
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    loss, _, pkg = fused_train_iteration(m, opt, cam.to("cuda"), gt, PIPE, torch.zeros(3).cuda(), reso_lvl=2)
    assert torch.isfinite(loss)
    update_training_stats(m, pkg["viewspace_points"], pkg["radii"], pkg["pixel_sizes"], 2)
    assert m.denom[:, 2].sum().item() > 0

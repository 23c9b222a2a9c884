"""CPU checks of the model-surgery restatement (tests/densify_restatement.py) and of the drop-in surface of
ms-gs_amd/host/densify.py (DESIGN.md SPEC D1): the restatement against the reference's own outputs (tests/golden/densify_*.npz,
tests/golden/make_densify_golden.py) bit for bit, against the live reference on further seeds when its tree is present, and the
signatures / C ABI of the GPU calls."""
import glob
import inspect
import os
import subprocess

import numpy as np
import pytest
import torch

import densify_fixtures as fx
import densify_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "densify_*.npz")))


def run_restatement(fn, m, opt, g, *, draws=None):
    op = str(g["op"])
    if op == "densify_and_prune":
        mss = float(g["arg_max_screen_size"])
        rs.densify_and_prune(m, float(g["arg_max_grad"]), float(g["arg_min_opacity"]), float(g["arg_extent"]),
                             None if np.isnan(mss) else mss, optimizer=opt, draws=draws)
    elif op == "grow_large_gaussians":
        rs.grow_large_gaussians(m, float(g["arg_grad_threshold"]), int(g["arg_reso_lvl"]), optimizer=opt)
    elif op == "prune_points":
        rs.prune_points(m, torch.from_numpy(g["arg_mask"]).to(m._xyz.device), optimizer=opt)
    else:
        new = {k[len("arg_new_"):]: torch.from_numpy(g[k]).to(m._xyz.device) for k in g.files if k.startswith("arg_new_")}
        rs.densification_postfix(m, new["xyz"], new["f_dc"], new["f_rest"], new["opacity"], new["occ_multiplier"],
                                 new["dc_delta"], new["scaling"], new["rotation"], new["target_reso_lvl"],
                                 new["max_pixel_sizes"], new["min_pixel_sizes"], reso_lvl=int(g["arg_reso_lvl"]), optimizer=opt)


def inputs_of(g):
    return {k[3:]: g[k] for k in g.files if k.startswith("in_")}


def test_goldens_exist_and_are_small():
    assert len(GOLDEN) == 7
    ops = set()
    for p in GOLDEN:
        assert os.path.getsize(p) <= 512 * 1024, p
        ops.add(str(np.load(p)["op"]))
    assert ops == {"densify_and_prune", "grow_large_gaussians", "prune_points", "densification_postfix"}


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-4] for p in GOLDEN])
@pytest.mark.parametrize("lr0_groups", [True, False])
def test_restatement_matches_the_reference_bit_for_bit(path, lr0_groups):
    g = np.load(path)
    L = int(g["L"])
    m, opt = fx.build_model(inputs_of(g), "cpu", L, lr0_groups=lr0_groups)
    run_restatement(None, m, opt, g, draws=torch.from_numpy(g["z"]))
    got = fx.snapshot(m, opt)
    want = {k[4:]: g[k] for k in g.files if k.startswith("out_")}
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape, k
        assert fx.bits_equal(got[k], v), k
    # the lr-0 groups without an optimizer group keep their type and requires_grad
    if not lr0_groups:
        assert not m._occ_multiplier.requires_grad and not m._dc_delta.requires_grad
    for group in opt.param_groups:
        assert opt.state[group["params"][0]] if group["name"] in fx.TRAINED else True


def test_restatement_draws_what_torch_normal_draws():
    """torch.normal(mean=0, std) == randn(shape) * std + 0 from the default generator (the draws densify_and_prune takes)"""
    std = torch.rand(64, 3) + 0.1
    torch.manual_seed(5)
    a = torch.normal(mean=torch.zeros(64, 3), std=std)
    torch.manual_seed(5)
    b = torch.randn((64, 3)) * std + torch.zeros(64, 3)
    assert torch.equal(a, b)


@pytest.mark.parametrize("seed", [101, 102])
def test_restatement_matches_the_live_reference(seed):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from ref_model_loader import available
    if not available():
        pytest.skip("the reference tree is not on this machine (the goldens above pin it)")
    import make_densify_golden as mk
    for op, P, L, extra in (("densify_and_prune", 300, 3, dict(max_screen_size=20)),
                            ("densify_and_prune", 300, 1, dict(max_screen_size=None)),
                            ("grow_large_gaussians", 300, 5, dict(reso_lvl=3, grad_threshold=0.0002))):
        lvl = extra.get("reso_lvl", 0) if op == "grow_large_gaussians" else 0
        d = fx.make_inputs(seed, P, L, lvl=lvl)
        args, z, want = mk.run_reference(op, d, L, extra, seed)
        m, opt = fx.build_model(d, "cpu", L)
        g = {"op": np.array(op), **{f"arg_{k}": np.array(np.nan if v is None else v) for k, v in args.items()}}

        class G(dict):
            files = property(lambda self: list(self.keys()))
        run_restatement(None, m, opt, G(g), draws=torch.from_numpy(z))
        got = fx.snapshot(m, opt)
        for k, v in want.items():
            assert fx.bits_equal(got[k], v), (op, k)


REF_ARGS = {"densify_and_prune": ["max_grad", "min_opacity", "extent", "max_screen_size"],
            "grow_large_gaussians": ["grad_threshold", "reso_lvl"],
            "prune_points": ["mask"],
            "densification_postfix": ["new_xyz", "new_features_dc", "new_features_rest", "new_opacities", "new_occ_multiplier",
                                      "new_dc_delta", "new_scaling", "new_rotation", "new_target_reso_lvl", "new_max_pixel_sizes",
                                      "new_min_pixel_sizes", "reso_lvl"]}


@pytest.mark.parametrize("name", sorted(REF_ARGS))
def test_drop_in_signatures(name):
    """(model, <the reference's parameters>): assigning the function to GaussianModel replaces the method"""
    import densify
    for mod in (densify, rs):
        params = list(inspect.signature(getattr(mod, name)).parameters.values())
        positional = [p.name for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
        assert positional == ["model"] + REF_ARGS[name], (mod.__name__, name)
        assert all(p.kind == p.KEYWORD_ONLY for p in params if p.name not in positional)
    from ref_model_loader import available
    if available():
        ref = getattr(__import__("ref_model_loader").load_gaussian_model(), name)
        assert list(inspect.signature(ref).parameters)[1:] == REF_ARGS[name]
    assert inspect.signature(densify.densification_postfix).parameters["reso_lvl"].default == 0


def test_cpu_models_raise():
    import densify
    d = fx.make_inputs(1, 16, 2)
    m, opt = fx.build_model(d, "cpu", 2)
    with pytest.raises(RuntimeError, match="GPU-only"):
        densify.densify_and_prune(m, 0.0002, 0.005, 4.0, None)
    with pytest.raises(RuntimeError, match="GPU-only"):
        densify.prune_points(m, torch.zeros(16, dtype=torch.bool))
    assert m._xyz.shape[0] == 16


def test_abi_structs_match_the_header(tmp_path):
    """ctypes mirrors of msgs_densify_select_t / msgs_densify_tensor_t / msgs_densify_apply_t against the C compiler's layout"""
    import ctypes as C
    from diff_gaussian_rasterization import _backend as B
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "msgs.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(msgs_densify_select_t), offsetof(msgs_densify_select_t, opacity), offsetof(msgs_densify_select_t, prune_mask),'
                   'sizeof(msgs_densify_tensor_t), offsetof(msgs_densify_tensor_t, rule), sizeof(msgs_densify_apply_t),'
                   'offsetof(msgs_densify_apply_t, tensors));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(B.DensifySelect), B.DensifySelect.opacity.offset, B.DensifySelect.prune_mask.offset,
                   C.sizeof(B.DensifyTensor), B.DensifyTensor.rule.offset, C.sizeof(B.DensifyApply), B.DensifyApply.tensors.offset]
    lib = B.lib
    assert lib.msgs_densify_scratch_bytes(0, 0) > 0
    assert lib.msgs_densify_scratch_bytes(10**6, 0) >= 9 * 10**6
    counts = (C.c_int64 * 8)()
    s = B.DensifySelect()
    s.mode, s.P = 9, 10
    assert lib.msgs_densify_select(C.byref(s), C.c_void_p(1), 1 << 20, counts, None) == -1     # unknown mode: refused
    s.mode, s.P = B.DENSIFY_PRUNE, 1 << 29
    assert lib.msgs_densify_select(C.byref(s), C.c_void_p(1), 1 << 20, counts, None) == -3     # beyond 2^29 rows

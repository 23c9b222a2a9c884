"""CPU checks of the MCMC densification (DESIGN.md SPEC M18): the float64 restatement's own properties (tests/mcmc_restatement.py),
the ctypes mirrors against include/msgs.h, and the refusal of CPU tensors (no kernel runs here)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import densify_fixtures as fx
import mcmc_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XS = np.array([-5.3, -5.29, -1.0, 0.0, 3.0, 6.0, 16.0, 30.0])
NS = (1, 2, 3, 7, 51)


def _grid():
    s = np.tile(np.array([[-3.0, -1.0, 0.5]]), (XS.size, 1))
    return {N: rs.relocation(XS, s, np.full(XS.size, N)) + (s,) for N in NS}


def test_one_copy_is_the_identity():
    xn, sn, c, s = _grid()[1]
    assert np.abs(c - 1.0).max() < 1e-12
    assert np.abs(sn - s).max() < 1e-12
    assert np.abs(xn - np.clip(XS, rs.X_MIN, rs.X_MAX)).max() < 1e-9     # up to the clamps (x = -5.3 is below, x = 30 above)


def test_scale_ratio_decreases_in_N_and_never_exceeds_one():
    g = _grid()
    cs = np.stack([g[N][2] for N in NS])
    assert (cs <= 1.0 + 1e-12).all()
    assert (np.diff(cs, axis=0) < 0).all()
    for N in NS:
        assert np.abs(g[N][1] - g[N][3] - np.log(g[N][2])[:, None]).max() < 1e-12


def test_new_opacity_never_falls_below_its_floor():
    x = np.concatenate([XS, np.linspace(-20, 40, 121)])
    s = np.zeros((x.size, 3))
    for N in (1, 2, 7, 51, 52, 300):
        xn, _, _ = rs.relocation(x, s, np.full(x.size, N))
        assert (xn >= rs.X_MIN).all() and np.isfinite(xn).all()
        assert (xn <= rs.X_MAX).all()
    a, b = rs.relocation(x, s, np.full(x.size, 51)), rs.relocation(x, s, np.full(x.size, 300))
    assert all(np.array_equal(p, q) for p, q in zip(a, b))              # N is capped at 51


def test_unclamped_new_opacity_composes_to_the_old_one():
    """N copies of opacity o_new leave the transmittance of one copy of o: (1 - o_new)^N = 1 - o"""
    x = np.array([-1.0, 0.0, 3.0, 6.0])
    for N in (2, 7, 51):
        xn, _, _ = rs.relocation(x, np.zeros((4, 3)), np.full(4, N))
        lhs = N * -(np.maximum(xn, 0) + np.log1p(np.exp(-np.abs(xn))))
        assert np.abs(lhs - -(np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x))))).max() < 1e-12


def test_sampling_restatement_edges():
    x = np.array([0.0, 1.0, -2.0, 3.0, 0.5])
    dead = np.array([True, False, True, False, True])
    u = np.array([0.0, np.nextafter(1.0, 0.0), 0.5, 0.999999])
    src, count, cdf = rs.sample(x, u, dead)
    assert src[0] == 1 and src[1] == 3 and not dead[src].any()
    assert np.array_equal(count, np.bincount(src, minlength=5)) and cdf[0] == 0.0 and cdf[2] == cdf[1] and cdf[4] == cdf[3]
    src, _, _ = rs.sample(x, np.array([1.0]), dead)                     # a product equal to the total: last positive row
    assert src[0] == 3


def _header_struct(name):
    src = open(os.path.join(ROOT, "include", "msgs.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (name, name), src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, field = decl.rsplit(None, 1) if "*" not in decl else (decl[:decl.rindex("*") + 1], decl[decl.rindex("*") + 1:])
            fields.append((typ.strip(), field.strip()))
    return fields


def _lp64_size(fields):
    size = {"int32_t": 4, "int64_t": 8, "float": 4, "double": 8}
    off, align = 0, 1
    for typ, _ in fields:
        n = 8 if typ.endswith("*") else size[typ]
        off = (off + n - 1) // n * n + n
        align = max(align, n)
    return (off + align - 1) // align * align


def test_ctypes_mirrors_match_the_header():
    import diff_gaussian_rasterization as dgr
    B = dgr._C
    for cname, mirror, want in (("msgs_mcmc_tensor", B.McmcTensor, 48), ("msgs_mcmc_relocate", B.McmcRelocate, 40)):
        fields = _header_struct(cname)
        assert [f for _, f in fields] == [f[0] for f in mirror._fields_]
        assert C.sizeof(mirror) == _lp64_size(fields) == want
    assert B.McmcTensor.width.offset == 32 and B.McmcRelocate.u.offset == 24 and B.McmcRelocate.tensors.offset == 32
    src = open(os.path.join(ROOT, "include", "msgs.h")).read()
    defs = dict(re.findall(r"#define (MSGS_M[CR]_[A-Z_]+|MSGS_MCMC_[A-Z_]+|MSGS_ERR_NO_WEIGHT) \(?(-?\d+)\)?", src))
    assert int(defs["MSGS_MCMC_N_MAX"]) == B.MCMC_N_MAX == rs.N_MAX
    assert int(defs["MSGS_MCMC_MAX_TENSORS"]) == B.MCMC_MAX_TENSORS and int(defs["MSGS_ERR_NO_WEIGHT"]) == B.ERR_NO_WEIGHT
    for k in ("COPY", "ZERO", "OPACITY", "SCALE", "PIX_MAX", "PIX_MIN"):
        assert int(defs["MSGS_MR_" + k]) == getattr(B, "MR_" + k)
    assert b"positive weight" in B.lib.msgs_error_string(B.ERR_NO_WEIGHT)
    prev = 0
    for P in (0, 1, 256, 257, 10 ** 6):
        n = B.lib.msgs_mcmc_scratch_bytes(P)
        assert n >= prev and n % 256 == 0 and n >= 44 * P
        prev = n


def test_cpu_tensors_raise():
    import mcmc
    d = fx.make_inputs(3, 40, 2)
    m, opt = fx.build_model(d, "cpu", 2)
    dead = torch.zeros(40, dtype=torch.bool)
    dead[::7] = True
    with pytest.raises(RuntimeError, match="no CPU path"):
        mcmc.relocate_gs(m, dead, optimizer=opt)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mcmc.add_new_gs(m, 100, optimizer=opt)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mcmc.add_new_gs(m, 10, optimizer=opt)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mcmc.relocate_and_grow(m, 100, optimizer=opt)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mcmc.add_position_noise(m, 0.00016)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mcmc.sample_by_opacity(m._opacity, torch.rand(8, dtype=torch.float64))
    assert fx.bits_equal(fx.snapshot(m, opt)["xyz"], d["xyz"])


def test_regularizer_is_the_two_means():
    import mcmc
    d = fx.make_inputs(5, 30, 1)
    m, _ = fx.build_model(d, "cpu", 1)
    got = mcmc.mcmc_regularizer(m, opacity_reg=0.02, scale_reg=0.03)
    want = 0.02 * rs.weights(d["opacity"]).mean() + 0.03 * np.exp(d["scaling"].astype(np.float64)).mean()
    assert abs(float(got.detach()) - want) < 1e-6 * want and got.requires_grad


def test_noise_restatement_in_float32_stays_inside_the_gpu_tolerance():
    """the float32 restatement the GPU test's k was measured on (tests/test_mcmc_gpu.py::test_position_noise) passes that test's
    bound, 2 x the measured ratio (the factor leaves room for another libm's exp)"""
    from test_mcmc_gpu import NOISE_K_MEASURED, NOISE_SEED
    for P in rs.NOISE_SIZES:
        d = rs.noise_inputs(NOISE_SEED, P)
        a = {k: d[k] for k in ("xyz", "scaling", "rotation", "opacity", "draws")}
        w64, scale = rs.noise(**a, gain=rs.NOISE_GAIN)
        w32, _ = rs.noise(**a, gain=rs.NOISE_GAIN, dtype=np.float32)
        ratio = (np.abs(w32.astype(np.float64) - w64) / (2.0 ** -24 * scale)).max()
        assert ratio <= 2 * NOISE_K_MEASURED[P], (P, ratio)

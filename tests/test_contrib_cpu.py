"""CPU checks of the contribution scores (SPEC M11; include/msgs.h msgs_contrib_*):
- the three C entries are declared, prototyped, exported and listed; ABI and struct sizes unchanged; the scratch query is sane;
- the opt-in surface exists (GaussianRasterizer.contributions, ContributionAccumulator, ContributionScores, host/contribution.py)
  and forward()'s parameters are what they were;
- contribution_prune_mask: fraction, threshold, ties by index, the exactly-one-argument errors, fraction = 0 and 1;
- the float64 fixture of tests/test_contrib_gpu.py (tests/golden/contrib_truth.npz) is what its generator computes from
  oracle/torch_oracle.py, and it has the properties the GPU comparison leans on."""
import ctypes as C
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("msgs_contrib_scratch_bytes", "msgs_contrib_accumulate", "msgs_contrib_finish")
GOLDEN = os.path.join(ROOT, "tests", "golden", "contrib_truth.npz")


# ---------------------------------------------------------------------------------------------------------------------------
# the C boundary
# ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msgs.h")).read(), flags=re.S)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert re.search(r"size_t\s+msgs_contrib_scratch_bytes\s*\(\s*int32_t\s+P\s*\)\s*;", src)
    args = norm(re.search(r"int\s+msgs_contrib_accumulate\s*\((.*?)\)\s*;", src, flags=re.S).group(1))
    assert args == norm("""const msgs_view_t* view, int32_t P, const void* geom, size_t geom_bytes, int64_t num_instances,
                           const void* binning, size_t binning_bytes, const void* image_state, size_t image_bytes,
                           const float* pixel_weights, void* acc, size_t acc_bytes, int32_t clear_first, void* stream""")
    args = norm(re.search(r"int\s+msgs_contrib_finish\s*\((.*?)\)\s*;", src, flags=re.S).group(1))
    assert args == norm("""int32_t P, const void* acc, size_t acc_bytes, float* weight_sum, float* weight_max,
                           int64_t* pixel_count, void* stream""")


def test_library_exports_prototypes_and_lists_them():
    import diff_gaussian_rasterization as dgr
    lib = dgr._C.lib
    for n in NEW:
        assert hasattr(lib, n), n
        assert n in dgr._C.EXPORTS, n
    vp, sz = C.c_void_p, C.c_size_t
    assert lib.msgs_contrib_scratch_bytes.argtypes == [C.c_int32] and lib.msgs_contrib_scratch_bytes.restype is sz
    assert lib.msgs_contrib_accumulate.argtypes == [C.POINTER(dgr._C.View), C.c_int32, vp, sz, C.c_int64, vp, sz, vp, sz, vp, vp, sz,
                                                    C.c_int32, vp]
    assert lib.msgs_contrib_finish.argtypes == [C.c_int32, vp, sz, vp, vp, vp, vp]
    assert lib.msgs_contrib_accumulate.restype is C.c_int and lib.msgs_contrib_finish.restype is C.c_int
    assert lib.msgs_abi_version() == dgr._C.ABI_VERSION == 11
    assert C.sizeof(dgr._C.Grads) == 120 and C.sizeof(dgr._C.View) == 96


def test_scratch_query():
    import diff_gaussian_rasterization as dgr
    q = dgr._C.lib.msgs_contrib_scratch_bytes
    prev = 0
    for P in (0, 1, 7, 1000, 10**6, 5 * 10**6):
        n = q(P)
        assert n >= 20 * P and n >= prev and n % 8 == 0, (P, n)       # a double, a 64-bit count and a float per Gaussian
        prev = n
    assert 0 < q(0) <= 4096 and q(-5) == q(0)
    assert q(10**6) <= 32 * 10**6


def test_refused_calls_need_no_device():
    """argument checks come before any launch: NULL and short buffers are refused on a machine without a GPU too"""
    import diff_gaussian_rasterization as dgr
    lib = dgr._C.lib
    view = dgr._C.View(24, 40, 0.5, 0.3, 1.0, 1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, None, None, None, None)
    buf = (C.c_uint64 * 64)()
    acc, n = C.c_void_p(C.addressof(buf)), lib.msgs_contrib_scratch_bytes(10)
    call = lambda v=C.byref(view), P=10, a=acc, nb=n, D=5, g=acc: lib.msgs_contrib_accumulate(
        v, P, g, 1 << 30, D, acc, 1 << 30, acc, 1 << 30, None, a, nb, 1, None)
    assert call(v=None) == -1 and call(P=-1) == -1 and call(a=None) == -1 and call(D=-1) == -1 and call(g=None) == -1
    assert call(a=C.c_void_p(C.addressof(buf) + 4)) == -1                   # rows of doubles: 8-byte aligned
    assert call(nb=n - 1) == -2
    fin = lambda P=10, a=acc, nb=n, o=acc: lib.msgs_contrib_finish(P, a, nb, o, acc, acc, None)
    assert fin(P=-1) == -1 and fin(a=None) == -1 and fin(o=None) == -1 and fin(nb=n - 1) == -2
    assert fin(P=0, a=None, o=None) == 0                                    # nothing to convert
    assert all(x == 0 for x in buf)


# ---------------------------------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------------------------------
def test_wrapper_surface():
    import diff_gaussian_rasterization as dgr
    p = inspect.signature(dgr.GaussianRasterizer.contributions).parameters
    assert list(p) == ["self", "means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp",
                       "max_pixel_sizes", "min_pixel_sizes", "base_mask", "pixel_weights", "into"]
    for n in ("pixel_weights", "into"):
        assert p[n].kind is inspect.Parameter.KEYWORD_ONLY and p[n].default is None
    assert dgr.ContributionScores._fields == ("weight_sum", "weight_max", "pixel_count")
    assert "ContributionScores" in dgr.__all__ and "ContributionAccumulator" in dgr.__all__
    # forward()'s parameters: the reference's 13, unchanged
    assert list(inspect.signature(dgr.GaussianRasterizer.forward).parameters) == [
        "self", "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp",
        "max_pixel_sizes", "min_pixel_sizes", "occ_multiplier", "dc_delta", "base_mask"]
    assert list(inspect.signature(dgr.GaussianRasterizer.__init__).parameters) == ["self", "raster_settings", "return_alpha",
                                                                                  "absgrad"]


def test_no_gaussians_needs_no_device():
    import diff_gaussian_rasterization as dgr
    rs = dgr.GaussianRasterizationSettings(4, 6, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3),
                                           False, False)
    z = lambda *s: torch.zeros(*s)
    r = dgr.GaussianRasterizer(rs)
    s = r.contributions(z(0, 3), z(0, 1), scales=z(0, 3), rotations=z(0, 4))
    assert isinstance(s, dgr.ContributionScores)
    assert s.weight_sum.shape == s.weight_max.shape == s.pixel_count.shape == (0,)
    assert s.weight_sum.dtype == s.weight_max.dtype == torch.float32 and s.pixel_count.dtype == torch.int64
    acc = dgr.ContributionAccumulator(0, "cpu")
    assert r.contributions(z(0, 3), z(0, 1), scales=z(0, 3), rotations=z(0, 4), into=acc) is None and acc.views == 1
    for bad in (z(4, 6).double(), z(6, 4), z(4, 6, 1), [[0.0] * 6] * 4):
        with pytest.raises(ValueError, match="pixel_weights"):
            r.contributions(z(0, 3), z(0, 1), scales=z(0, 3), rotations=z(0, 4), pixel_weights=bad)
    with pytest.raises(ValueError, match="ContributionAccumulator"):
        r.contributions(z(0, 3), z(0, 1), scales=z(0, 3), rotations=z(0, 4), into=dgr.ContributionAccumulator(0, "cpu").scores())
    with pytest.raises(RuntimeError, match="HIP device"):
        dgr.ContributionAccumulator(3, "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):                  # no silent CPU fallback
        r.contributions(z(2, 3), z(2, 1), scales=z(2, 3), rotations=z(2, 4))


def test_host_layer_signatures():
    import contribution
    sig = lambda f: [(n, p.default, p.kind) for n, p in inspect.signature(f).parameters.items()]
    E, KW, PK = inspect.Parameter.empty, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert sig(contribution.contribution_scores)[:5] == [("cams", E, PK), ("pc", E, PK), ("pipe", E, PK), ("bg_color", E, PK),
                                                         ("pixel_weights", None, KW)]
    assert sig(contribution.contribution_prune_mask) == [("scores", E, PK), ("fraction", None, KW), ("threshold", None, KW),
                                                         ("key", "weight_sum", KW)]
    assert sig(contribution.prune_by_contribution)[:2] == [("model", E, PK), ("scores", E, PK)]
    assert inspect.signature(contribution.prune_by_contribution).parameters["optimizer"].kind is KW


# ---------------------------------------------------------------------------------------------------------------------------
# contribution_prune_mask
# ---------------------------------------------------------------------------------------------------------------------------
def _scores(ws, wm=None, pc=None):
    from diff_gaussian_rasterization import ContributionScores
    ws = torch.tensor(ws, dtype=torch.float32)
    wm = ws * 0.5 if wm is None else torch.tensor(wm, dtype=torch.float32)
    pc = (ws > 0).long() * 3 if pc is None else torch.tensor(pc, dtype=torch.int64)
    return ContributionScores(ws, wm, pc)


def test_prune_mask_by_fraction_is_stable():
    from contribution import contribution_prune_mask as M
    s = _scores([0.5, 0.0, 2.0, 0.0, 0.5, 0.0, 1.0, 0.5])
    idx = lambda m: m.nonzero().flatten().tolist()
    assert M(s, fraction=0.0).dtype == torch.bool and idx(M(s, fraction=0.0)) == []
    assert idx(M(s, fraction=1.0)) == list(range(8))
    assert idx(M(s, fraction=0.125)) == [1]                       # never-seen rows leave first, in index order
    assert idx(M(s, fraction=0.25)) == [1, 3]
    assert idx(M(s, fraction=0.375)) == [1, 3, 5]
    assert idx(M(s, fraction=0.5)) == [0, 1, 3, 5]                # ties at 0.5: the lowest index goes first
    assert idx(M(s, fraction=0.625)) == [0, 1, 3, 4, 5]
    assert idx(M(s, fraction=0.3)) == [1, 3]                      # floor(0.3 * 8) = 2
    assert idx(M(s, fraction=0.99)) == [0, 1, 3, 4, 5, 6, 7]      # floor(7.92) = 7: the largest stays
    # against numpy's stable argsort on a larger random case with many ties
    g = torch.Generator().manual_seed(4)
    ws = torch.randint(0, 6, (1001,), generator=g).float()
    for f in (0.1, 0.25, 0.5, 0.77):
        want = np.zeros(1001, bool)
        want[np.argsort(ws.numpy(), kind="stable")[:int(np.floor(f * 1001))]] = True
        assert np.array_equal(M(_scores(ws.tolist()), fraction=f).numpy(), want), f


def test_prune_mask_by_threshold_and_key():
    from contribution import contribution_prune_mask as M
    s = _scores([0.5, 0.0, 2.0, 0.25], wm=[0.4, 0.0, 0.1, 0.2], pc=[9, 0, 40, 1])
    idx = lambda m: m.nonzero().flatten().tolist()
    assert idx(M(s, threshold=0.5)) == [1, 3]                     # strictly below
    assert idx(M(s, threshold=0.0)) == []
    assert idx(M(s, threshold=0.2, key="weight_max")) == [1, 2]
    assert idx(M(s, threshold=2, key="pixel_count")) == [1, 3]
    assert idx(M(s, fraction=0.5, key="weight_max")) == [1, 2]
    assert idx(M(s, fraction=0.5, key=s.weight_sum * s.pixel_count)) == [1, 3]        # a score of the caller's own
    assert idx(M(_scores([]), fraction=0.5)) == [] and M(_scores([]), threshold=1.0).shape == (0,)


def test_prune_mask_argument_errors():
    from contribution import contribution_prune_mask as M
    s = _scores([1.0, 2.0])
    with pytest.raises(ValueError, match="exactly one"):
        M(s)
    with pytest.raises(ValueError, match="exactly one"):
        M(s, fraction=0.5, threshold=0.1)
    with pytest.raises(ValueError, match="fraction"):
        M(s, fraction=1.5)
    with pytest.raises(ValueError, match="fraction"):
        M(s, fraction=-0.1)
    with pytest.raises(ValueError, match="key"):
        M(s, fraction=0.5, key="opacity")


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 fixture
# ---------------------------------------------------------------------------------------------------------------------------
def _generator():
    spec = importlib.util.spec_from_file_location("make_contrib_golden", os.path.join(ROOT, "tests", "golden",
                                                                                      "make_contrib_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_fixture_is_what_the_oracle_computes():
    gen = _generator()
    want = gen.compute()
    got = np.load(GOLDEN)
    assert sorted(got.files) == sorted(want)
    for k in ("borderline", "visible", "count_plain", "count_weighted", "m_plain", "m_weighted"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    for k in ("sum_plain", "max_plain", "sum_weighted", "max_weighted", "alpha"):
        assert got[k].dtype == np.float64 and got[k].shape == want[k].shape
        assert np.abs(got[k] - want[k]).max() <= 1e-12 * np.abs(want[k]).max(), k


def test_fixture_properties():
    gen = _generator()
    t = np.load(GOLDEN)
    vis, bl = t["visible"], t["borderline"]
    assert bl.shape == (gen.H, gen.W) and bl.sum() <= gen.MAX_BORDERLINE * gen.W * gen.H
    assert vis.sum() >= 150
    assert np.array_equal(t["m_plain"], (~bl).astype(np.float32))
    mw = t["m_weighted"]
    assert mw.dtype == np.float32 and (mw >= 0).all() and (mw[bl] == 0).all()
    assert 0.15 * mw.size <= (mw == 0).sum() <= 0.35 * mw.size and mw.max() > 2.0        # a real mask and real weights
    for name in ("plain", "weighted"):
        s, m, c = t["sum_" + name], t["max_" + name], t["count_" + name]
        assert c.dtype == np.int64 and s.shape == m.shape == c.shape == (gen.P,)
        assert np.array_equal(c == 0, s == 0) and np.array_equal(c == 0, m == 0)          # zero together
        assert (c[~vis] == 0).all() and (c[vis] > 0).sum() >= 0.9 * vis.sum()
        assert (m <= s * (1 + 1e-12)).all() and (s <= c * m * (1 + 1e-12)).all()
    assert (t["max_plain"] <= 0.99).all() and t["max_plain"].max() > 0.5
    assert (t["count_weighted"] <= t["count_plain"]).all() and t["count_weighted"].sum() < 0.9 * t["count_plain"].sum()
    # a pixel's weights add up to its alpha: sum_i weight_sum_i = sum_p alpha_p over the counted pixels
    assert abs(t["sum_plain"].sum() - (t["alpha"] * t["m_plain"]).sum()) <= 1e-9 * t["alpha"].sum()
    # the weighted scores are another quantity: a replay that ignored the map could not pass
    assert np.abs(t["sum_weighted"] - t["sum_plain"]).max() > 0.05 * t["sum_plain"].max()

"""Vector quantisation and the compressed model file without a GPU (SPEC M21; 4.23): the truth of tests/vq_truth.py
against brute force and against its own second statement, the wrappers' validation, and the container on a model built by hand.
Nothing in this file reaches a kernel."""
import os
import re
import types

import numpy as np
import pytest
import torch

import compress                    # host/compress.py: the feature under test
import diff_gaussian_rasterization as dgr
import vq_truth as vt


def _data(P, D, K, seed):
    g = np.random.default_rng(seed)
    return g.standard_normal((P, D)).astype(np.float32), g.standard_normal((K, D)).astype(np.float32)


def _no_launch(monkeypatch):
    calls = []
    monkeypatch.setattr(dgr, "_vq_probe", calls.append)
    return calls


def test_symbols_abi_and_constants():
    for name in ("msgs_vq_scratch_bytes", "msgs_vq_assign", "msgs_vq_update"):
        assert name in dgr._C.EXPORTS and hasattr(dgr._C.lib, name)
    assert dgr._C.lib.msgs_abi_version() == 11
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "msgs.h")).read()
    value = lambda name: int(re.search(rf"#define {name} ([0-9]+)", src).group(1))
    assert dgr.VQ_MAX_DIM == value("MSGS_VQ_MAX_DIM") == 64
    assert dgr.VQ_MAX_CODES == value("MSGS_VQ_MAX_CODES") == 65536
    assert dgr.VQ_CODE_CHUNK == value("MSGS_VQ_CODE_CHUNK")
    assert dgr.VQ_UPDATE_CHUNK == value("MSGS_VQ_UPDATE_CHUNK") == vt.UPDATE_CHUNK
    for name in ("vq_assign", "vq_update", "VQ_MAX_DIM", "VQ_MAX_CODES", "VQ_CODE_CHUNK", "VQ_UPDATE_CHUNK"):
        assert name in dgr.__all__
    # the size query: 0 for what is refused, and room for either call otherwise
    q = dgr._C.lib.msgs_vq_scratch_bytes
    assert q(10, 65, 4) == 0 and q(10, 4, 65537) == 0 and q(-1, 4, 4) == 0 and q(10, 0, 4) == 0
    assert q(1000, 45, 300) >= max(5 * 64 * (48 + 1) * 4, (1000 // 256 + 300) * 46 * 8)


def test_refusals_come_before_any_launch(monkeypatch):
    calls = _no_launch(monkeypatch)
    x, c = torch.zeros(10, 4), torch.zeros(3, 4)
    idx = torch.zeros(10, dtype=torch.int32)
    for bad in (dict(x=torch.zeros(10)), dict(codebook=torch.zeros(3, 5)), dict(x=torch.zeros(10, 4, 1)),
                dict(x=torch.zeros(10, 65), codebook=torch.zeros(3, 65)), dict(codebook=torch.zeros(65537, 4)),
                dict(x=torch.zeros(10, 0), codebook=torch.zeros(3, 0)), dict(codebook=torch.zeros(0, 4)),
                dict(x=x.double()), dict(codebook=c.half()), dict(x=[1.0])):
        with pytest.raises(ValueError):
            dgr.vq_assign(**dict(dict(x=x, codebook=c), **bad))
    with pytest.raises(ValueError, match="D = 65"):
        dgr.vq_assign(torch.zeros(10, 65), torch.zeros(3, 65))
    with pytest.raises(ValueError, match="K = 65537"):
        dgr.vq_assign(x, torch.zeros(65537, 4))
    for who, args in (("x", (x.clone().requires_grad_(True), c)), ("codebook", (x, c.clone().requires_grad_(True)))):
        with pytest.raises(ValueError, match=rf"not differentiable: pass {who}\.detach\(\)"):
            dgr.vq_assign(*args)
        with pytest.raises(ValueError, match=rf"not differentiable: pass {who}\.detach\(\)"):
            dgr.vq_update(args[0], idx, args[1])
    with pytest.raises(ValueError, match=r"not differentiable: pass weights\.detach\(\)"):
        dgr.vq_update(x, idx, c, torch.ones(10, requires_grad=True))
    for bad in (dict(idx=idx.float()), dict(idx=idx[:9]), dict(idx=idx[:, None]), dict(weights=torch.ones(9)),
                dict(weights=torch.ones(10, dtype=torch.float64)), dict(idx=None)):
        with pytest.raises(ValueError):
            dgr.vq_update(**dict(dict(x=x, idx=idx, codebook=c), **bad))
    # host tensors: the package's error, still before any launch
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.vq_assign(x, c)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.vq_assign(torch.zeros(0, 4), c)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.vq_update(x, idx, c, torch.ones(10))
    assert calls == []


def test_kmeans_refusals(monkeypatch):
    calls = _no_launch(monkeypatch)
    with pytest.raises(ValueError, match="K = 11 codes for P = 10 rows"):
        compress.kmeans(torch.zeros(10, 4), 11)
    with pytest.raises(ValueError, match="D = 65"):
        compress.kmeans(torch.zeros(100, 65), 4)
    with pytest.raises(ValueError, match="K = 65537"):
        compress.kmeans(torch.zeros(70000, 2), 65537)
    with pytest.raises(ValueError):
        compress.kmeans(torch.zeros(10), 2)
    with pytest.raises(ValueError, match="weights"):
        compress.kmeans(torch.zeros(10, 4), 2, weights=torch.ones(9))
    with pytest.raises(ValueError, match="init"):
        compress.kmeans(torch.zeros(10, 4), 2, init=torch.zeros(3, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        compress.kmeans(torch.zeros(10, 4), 2)
    assert calls == []


@pytest.mark.parametrize("P,D,K", [(200, 45, 30), (64, 3, 17), (50, 1, 1), (33, 64, 5)])
def test_truth_against_brute_force(P, D, K):
    x, c = _data(P, D, K, seed=P)
    idx, err, s = vt.assign(x, c)
    assert np.array_equal(idx, vt.assign_brute(x, c))
    # the score is the squared distance up to a term that does not depend on the code
    d2 = ((x[:, None, :].astype(np.float64) - c[None].astype(np.float64)) ** 2).sum(2)
    assert np.abs(2 * s + (x.astype(np.float64) ** 2).sum(1)[:, None] - d2).max() < 1e-11
    assert np.abs(err - d2[np.arange(P), idx]).max() < 1e-12
    # the float32 chain stays inside the bound the margins are built on, and the float32 error inside float32's reach
    gap, flagged, b = vt.margins(x, c)
    assert (np.abs(vt.scores_float32(x, c).astype(np.float64) - s).max(1) <= b).all()
    assert np.abs(vt.err_float32(x, c, idx) - err).max() <= (D + 2) * vt.U * err.max()
    assert gap.shape == (P,) and (gap >= 0).all() and (K > 1 or np.isinf(gap).all())


def test_truth_breaks_ties_towards_the_lower_code():
    x, c = _data(40, 5, 6, seed=3)
    c[4] = c[1]
    c[5] = c[1]
    idx, _, _ = vt.assign(x, c)
    assert (idx < 4).all() and (idx == 1).any()
    gap, flagged, _ = vt.margins(x, c)
    assert flagged[idx == 1].all() and (gap[idx == 1] == 0).all()


def test_truth_update_chunked_is_the_mean():
    C = vt.UPDATE_CHUNK
    g = np.random.default_rng(5)
    idx = np.concatenate([np.full(3 * C + 7, 2), np.full(C, 0), [4]])              # codes 1 and 3 stay empty
    g.shuffle(idx)
    x = g.standard_normal((len(idx), 6)).astype(np.float32)
    c = g.standard_normal((5, 6)).astype(np.float32)
    for w in (None, g.random(len(idx)).astype(np.float32) * (g.random(len(idx)) > 0.2)):
        new, mass, count = vt.update_chunked(x, idx, c, w)
        ref, mass2, count2 = vt.update(x, idx, c, w)
        assert count.tolist() == count2.tolist() == [C, 0, 3 * C + 7, 0, 1]
        assert np.abs(mass - mass2).max() <= 1e-12 * mass.max()
        ulp = np.spacing(np.abs(ref))
        assert (np.abs(new.astype(np.float64) - ref.astype(np.float64)) <= ulp).all()
        assert np.array_equal(new[[1, 3]], c[[1, 3]])                              # an empty code keeps its row
        ww = np.ones(len(idx)) if w is None else w.astype(np.float64)
        assert np.abs(new[4] - x[idx == 4][0]).max() == 0 or ww[idx == 4][0] == 0  # one member: itself
    # all weights of a code zero: mass 0, the row stays although it has members
    w = np.ones(len(idx), np.float32)
    w[idx == 0] = 0
    new, mass, count = vt.update_chunked(x, idx, c, w)
    assert mass[0] == 0 and count[0] == C and np.array_equal(new[0], c[0])


def test_truth_kmeans_distortion_does_not_increase():
    g = np.random.default_rng(11)
    centres = 3.0 * g.standard_normal((12, 8))
    x = (centres[g.integers(0, 12, 600)] + 0.3 * g.standard_normal((600, 8))).astype(np.float32)
    w = g.random(600).astype(np.float32)
    for weights in (None, w):
        c, idx, history, _ = vt.kmeans(x, x[:12], 6, weights)
        assert len(history) == 7
        assert all(b <= a * (1 + 1e-12) for a, b in zip(history, history[1:]))
        assert history[-1] < 0.5 * history[0]
        assert np.array_equal(idx, vt.assign(x, c)[0])
    # the chunk-ordered statement walks the same path
    c2, idx2, history2, _ = vt.kmeans(x, x[:12], 6, w, chunked=True)
    assert np.array_equal(idx, idx2) and np.abs(c - c2).max() <= 1e-6 * np.abs(c).max()


def test_truth_reseeds_empty_codes_in_the_stated_order():
    x = np.zeros((6, 2), np.float32)
    x[:, 0] = [0.0, 0.1, 5.0, 0.2, 9.0, 5.0]
    c = np.array([[0.0, 0.0], [100.0, 100.0], [0.1, 0.0], [200.0, 0.0]], np.float32)
    idx, err, _ = vt.assign(x, c)
    assert set(idx.tolist()) == {0, 2}                                             # codes 1 and 3 are empty
    new, _, count = vt.update(x, idx, c)
    out = vt.reseed(x, new, count, None, err)
    assert np.array_equal(out[1], x[4]) and np.array_equal(out[3], x[2])          # the worst row, then the lower of the tied two
    assert np.array_equal(out[[0, 2]], new[[0, 2]])


def _model(P, seed=0, filter_3d=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    m = types.SimpleNamespace(active_sh_degree=2, max_sh_degree=3)
    m._xyz, m._features_dc, m._features_rest = r(P, 3), r(P, 1, 3), r(P, 15, 3)
    m._opacity, m._scaling, m._rotation = r(P, 1), r(P, 3), r(P, 4)
    m._occ_multiplier, m._dc_delta = torch.ones(P, 4, 1), torch.zeros(P, 12, 1)
    m.base_gaussian_mask = torch.rand(P, generator=g) < 0.3
    m.max_pixel_sizes, m.min_pixel_sizes = r(P).abs() * 4, -torch.ones(P)
    if filter_3d:
        m.filter_3D = r(P, 1).abs()
    return m


LOSSLESS = ("_xyz", "_features_dc", "_opacity", "_occ_multiplier", "_dc_delta", "_scaling", "_rotation", "base_gaussian_mask",
            "max_pixel_sizes", "min_pixel_sizes")


@pytest.mark.parametrize("filter_3d", [False, True])
def test_container_round_trip(tmp_path, filter_3d):
    P, K = 300, 16
    m = _model(P, seed=4, filter_3d=filter_3d)
    rows = compress.sh_rows(m)
    assert rows.shape == (P, 45) and torch.equal(rows[:, 16], m._features_rest[:, 1, 1])   # the PLY's f_rest_16
    c, idx, _, _ = vt.kmeans(rows.numpy(), rows.numpy()[:K], 2)
    path = str(tmp_path / "deep" / "model.npz")
    compress.save_compressed(m, path, quantised=(torch.from_numpy(c), torch.from_numpy(idx)))
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    back = compress.load_compressed(types.SimpleNamespace(), path, device="cpu")
    for k in LOSSLESS + (("filter_3D",) if filter_3d else ()):
        a, b = getattr(back, k).detach(), getattr(m, k)
        assert a.dtype == b.dtype and torch.equal(a, b), k
    assert hasattr(back, "filter_3D") == filter_3d
    want = torch.from_numpy(c[idx]).reshape(P, 3, 15).transpose(1, 2)
    assert torch.equal(back._features_rest.detach(), want) and back._features_rest.is_contiguous()
    assert torch.equal(compress.sh_rows(back), torch.from_numpy(c[idx]))
    assert back._xyz.requires_grad and back._features_rest.requires_grad and not back._occ_multiplier.requires_grad
    assert back.active_sh_degree == back.max_sh_degree == 3
    # the file is what SPEC M21 (d) says
    with np.load(path) as z:
        assert z["sh_codebook"].dtype == np.float32 and z["sh_codebook"].shape == (K, 45)
        assert z["sh_index"].dtype == np.uint16 and np.array_equal(z["sh_index"], idx)
        assert int(z["sh_degree"]) == 3 and z["opacity"].dtype == np.float32
    # a codebook of the model's own rows is lossless
    compress.save_compressed(m, path, quantised=(rows, torch.arange(P)))
    assert torch.equal(compress.load_compressed(types.SimpleNamespace(), path, device="cpu")._features_rest.detach(), m._features_rest)
    # k-means itself needs the GPU, and bad indices are refused
    with pytest.raises(RuntimeError, match="no CPU path"):
        compress.save_compressed(m, path, sh_codes=8)
    with pytest.raises(ValueError, match="indices"):
        compress.save_compressed(m, path, quantised=(rows[:4], torch.full((P,), 4)))


def test_index_width_follows_the_codebook(tmp_path):
    P = 65537
    m = _model(P, seed=1)
    m._features_rest = m._features_rest[:, :1, :].contiguous()                     # D = 3 keeps the two files small
    rows = compress.sh_rows(m)
    small, large = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    compress.save_compressed(m, small, quantised=(rows[:65536], torch.arange(P) % 65536))
    compress.save_compressed(m, large, quantised=(rows, torch.arange(P)))
    with np.load(small) as a, np.load(large) as b:
        assert a["sh_index"].dtype == np.uint16 and a["sh_index"][-1] == 0 and a["sh_index"][65535] == 65535
        assert b["sh_index"].dtype == np.int32 and b["sh_index"][-1] == 65536
    assert torch.equal(compress.load_compressed(types.SimpleNamespace(), large, device="cpu")._features_rest.detach(), m._features_rest)


def test_size_report_adds_up(tmp_path):
    m = _model(2000, seed=2)
    rows = compress.sh_rows(m)
    path = str(tmp_path / "m.npz")
    compress.save_compressed(m, path, quantised=(rows[:64], torch.arange(2000) % 64))
    report = compress.compressed_size_report(path)
    assert report["total"] == os.path.getsize(path)
    assert sum(v for k, v in report.items() if k != "total") == report["total"]
    for k in ("sh_codebook", "sh_index", "xyz", "f_dc", "opacity", "scaling", "rotation", "occ_multiplier", "dc_delta",
              "base_gaussian_mask", "max_pixel_sizes", "min_pixel_sizes", "sh_degree"):
        assert report[k] > 0, k
    # constant fields cost almost nothing under deflate; random floats do not shrink
    assert report["occ_multiplier"] < 400 and report["dc_delta"] < 400 and report["xyz"] > 0.8 * 2000 * 12
    assert report["sh_codebook"] > 0.8 * 64 * 45 * 4 and report["sh_index"] < 2000 * 2 + 400

"""Vector quantisation on the GPU (SPEC M21; 4.23) against tests/vq_truth.py.

Assignment is compared with the float64 argmin off the rows the truth flags (gap between the best and the second-best float64
score under 2 max_k B(i,k), B the float32 chain's error bound; at most MAX_FLAGGED of the rows, a condition on the inputs); on
every row the chosen code scores within 2 max_k B of the minimum.  err: max(1e-6 x scale, 4 x the error of a float32
restatement), the rule of tests/test_filter3d_gpu.py.  The update owes the BITS of the truth's chunk-ordered statement, and
1 float32 ulp to the plain float64 mean.  Every case runs twice and must repeat bit for bit.  Measured maxima are printed
(pytest -s) and recorded in profiles/vq_notes.md."""
import copy
import functools

import numpy as np
import pytest
import torch

import compress                    # host/compress.py: the feature under test
import diff_gaussian_rasterization as dgr
import vq_truth as vt
from parity_utils import PIPE, report, small_scene

pytestmark = pytest.mark.gpu

MAX_FLAGGED = 0.005
CHUNK = dgr.VQ_CODE_CHUNK
SHAPES = [(1000, 45, 300), (777, 3, 65), (515, 7, 33), (300, 64, 257), (1, 1, 1), (31, 2, 31)]


def _twice(fn):
    a, b = fn(), fn()
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(u, v), "two runs differ"
    return a


def _assign(x, c, return_error=True):
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
    idx, err = _twice(lambda: dgr.vq_assign(xd, cd, return_error=return_error))
    assert idx.dtype == torch.int32 and idx.shape == (len(x),) and (err is None) == (not return_error)
    return idx.cpu().numpy().astype(np.int64), None if err is None else err.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(P, D, K):
    g = torch.Generator().manual_seed(1000 * P + K)
    x, c = torch.randn(P, D, generator=g).numpy(), torch.randn(K, D, generator=g).numpy()
    idx, err, s = vt.assign(x, c)
    gap, flagged, b = vt.margins(x, c)
    e32 = float(np.abs(vt.err_float32(x, c, idx) - err).max())
    return x, c, idx, err, s, flagged, b, e32


@pytest.mark.parametrize("P,D,K", SHAPES)
def test_assignment_against_float64(P, D, K):
    x, c, idx, err, s, flagged, b, e32 = _case(P, D, K)
    what = f"vq_assign P={P} D={D} K={K}"
    assert flagged.mean() <= MAX_FLAGGED, f"{what}: {flagged.mean():.3%} of the rows are flagged (a condition on the inputs)"
    got, gerr = _assign(x, c)
    assert got.min() >= 0 and got.max() < K
    ok = ~flagged
    assert np.array_equal(got[ok], idx[ok]), f"{what}: {int((got[ok] != idx[ok]).sum())} unflagged rows chose another code"
    excess = s[np.arange(P), got] - s.min(1)
    report(what, "largest score excess over the minimum / (2 max_k B)", float((excess / (2 * b)).max()))
    assert (excess <= 2 * b).all()
    same = got == idx
    scale = float(err.max())
    tol = max(1e-6 * scale, 4.0 * e32)
    e = float(np.abs(gerr[same] - err[same]).max())
    report(what, f"err max abs error (restatement {e32:.2e}, bound {tol:.2e})", e)
    assert e <= tol
    # without the error: the same indices
    assert np.array_equal(_assign(x, c, return_error=False)[0], got)


def test_empty_input_returns_empty_outputs_without_a_launch(monkeypatch):
    calls = []
    monkeypatch.setattr(dgr, "_vq_probe", calls.append)
    idx, err = dgr.vq_assign(torch.zeros(0, 5, device="cuda"), torch.zeros(3, 5, device="cuda"))
    assert idx.shape == (0,) and idx.dtype == torch.int32 and err.shape == (0,) and err.dtype == torch.float32 and idx.is_cuda
    assert calls == []
    with pytest.raises(ValueError, match=r"idx must lie in \[0, 3\)"):
        dgr.vq_update(torch.zeros(4, 5, device="cuda"), torch.tensor([0, 1, 3, 2], device="cuda"), torch.zeros(3, 5, device="cuda"))
    with pytest.raises(ValueError, match=r"idx must lie in \[0, 3\)"):
        dgr.vq_update(torch.zeros(4, 5, device="cuda"), torch.tensor([0, -1, 1, 2], device="cuda"), torch.zeros(3, 5, device="cuda"))
    assert calls == []


@pytest.mark.parametrize("D", [45, 64])
def test_planted_winners_across_every_edge(D):
    K = 2 * CHUNK + 33
    P = 3 * K + 5
    g = torch.Generator().manual_seed(D)
    c = torch.randn(K, D, generator=g).numpy()
    x = (c[np.arange(P) % K] + np.float32(1e-3) * torch.randn(P, D, generator=g).numpy()).astype(np.float32)
    idx, _, _ = vt.assign(x, c)
    gap, flagged, b = vt.margins(x, c)
    assert np.array_equal(idx, np.arange(P) % K) and not flagged.any(), "the planted margins do not exceed the bound"
    got, gerr = _assign(x, c)
    assert np.array_equal(got, np.arange(P) % K)
    assert gerr.max() < D * 2.5e-5                                 # (1e-3 x a normal deviate)^2 per column


def test_ties_go_to_the_lower_index():
    # twins: {the higher copy: the code it copies}
    D, K, P = 9, 3 * CHUNK, 400
    g = torch.Generator().manual_seed(7)
    base = torch.randn(K, D, generator=g).numpy()
    x = torch.randn(P, D, generator=g).numpy()
    twins = {17: 5,                                                # inside one 32-code tile
             40: 20,                                               # across tiles of a chunk: 40 copies 20
             CHUNK + 3: 2,                                         # across chunks
             2 * CHUNK + 50: CHUNK + 31,
             K - 1: 0}
    c = base.copy()
    for hi, lo in twins.items():
        c[hi] = c[lo]
    # rows that sit on a twinned code, so that the twins do win
    for j, lo in enumerate(twins.values()):
        x[10 * j:10 * j + 10] = c[lo] + np.float32(1e-3) * x[10 * j:10 * j + 10]
    got, _ = _assign(x, c)
    assert not np.isin(got, list(twins)).any(), "a higher copy of an identical row was selected"
    for j, lo in enumerate(twins.values()):
        assert (got[10 * j:10 * j + 10] == lo).all()
    keep = np.array([k for k in range(K) if k not in twins])
    idx, _, _ = vt.assign(x, c[keep])
    _, flagged, _ = vt.margins(x, c[keep])
    assert np.array_equal(got[~flagged], keep[idx][~flagged])
    # K identical rows: 0 everywhere
    same = np.repeat(base[:1], K, axis=0)
    got, gerr = _assign(x, same)
    assert (got == 0).all()
    assert np.abs(gerr - ((x.astype(np.float64) - same[0]) ** 2).sum(1)).max() <= 1e-5 * gerr.max()


def _update_case(weights):
    C = dgr.VQ_UPDATE_CHUNK
    g = np.random.default_rng(21)
    idx = np.concatenate([np.full(3 * C + 7, 3), np.full(C, 0), [5]])              # codes 1, 2 and 4 have no members
    g.shuffle(idx)
    D, K = 45, 6
    x = g.standard_normal((len(idx), D)).astype(np.float32)
    c = g.standard_normal((K, D)).astype(np.float32)
    w = None
    if weights == "random":
        w = g.random(len(idx)).astype(np.float32)
    elif weights == "some zero":
        w = (g.random(len(idx)) * (g.random(len(idx)) > 0.3)).astype(np.float32)
    elif weights == "a code of zeros":
        w = np.ones(len(idx), np.float32)
        w[idx == 0] = 0
    return x, idx, c, w


@pytest.mark.parametrize("weights", [None, "random", "some zero", "a code of zeros"])
@pytest.mark.parametrize("index_type", [torch.int32, torch.int64])
def test_update_has_the_bits_of_the_chunk_ordered_statement(weights, index_type):
    C = dgr.VQ_UPDATE_CHUNK
    x, idx, c, w = _update_case(weights)
    want, wmass, wcount = vt.update_chunked(x, idx, c, w)
    plain, _, _ = vt.update(x, idx, c, w)
    cd = torch.from_numpy(c).cuda()
    args = (torch.from_numpy(x).cuda(), torch.from_numpy(idx).cuda().to(index_type), cd,
            None if w is None else torch.from_numpy(w).cuda())
    new, mass, count = _twice(lambda: dgr.vq_update(*args))
    assert torch.equal(cd.cpu(), torch.from_numpy(c)), "the input codebook was changed"
    assert new.dtype == torch.float32 and mass.dtype == torch.float64 and count.dtype == torch.int32
    assert count.cpu().tolist() == wcount.tolist() == [C, 0, 0, 3 * C + 7, 0, 1]
    assert np.array_equal(mass.cpu().numpy(), wmass), "mass is not exact"
    new = new.cpu().numpy()
    assert np.array_equal(new.view(np.int32), want.view(np.int32)), "not the bits of the chunk-ordered statement"
    assert (np.abs(new.astype(np.float64) - plain.astype(np.float64)) <= np.spacing(np.abs(plain))).all()
    assert np.array_equal(new[[1, 2, 4]], c[[1, 2, 4]])                            # a code without members keeps its row
    if weights == "a code of zeros":
        assert mass[0].item() == 0.0 and np.array_equal(new[0], c[0])


def test_kmeans_follows_the_truth():
    P, D, K, iters = 1000, 45, 40, 3
    g = torch.Generator().manual_seed(4)           # chosen on the CPU truth alone: no margin of any iteration under the bound
    centres = 2.0 * torch.randn(K, D, generator=g)
    x = (centres[torch.randint(0, K, (P,), generator=g)] + 0.25 * torch.randn(P, D, generator=g)).contiguous()
    w = torch.rand(P, generator=g) + 0.1
    init = x[torch.randperm(P, generator=torch.Generator().manual_seed(0))[:K]]
    for weights in (None, w):
        wn = None if weights is None else weights.numpy()
        tc, tidx, thist, slack = vt.kmeans(x.numpy(), init.numpy(), iters, wn, chunked=True)
        assert slack > 0, "a margin of some iteration falls under the bound (a condition on the inputs)"
        run = lambda: compress.kmeans(x.cuda(), K, iters=iters, weights=None if weights is None else weights.cuda(), seed=0)
        (c1, i1, h1), (c2, i2, h2) = run(), run()
        assert torch.equal(c1, c2) and torch.equal(i1, i2) and h1 == h2, "two runs differ"
        assert torch.equal(c1, compress.kmeans(x.cuda(), K, iters=iters, seed=5, init=init.cuda(),
                                               weights=None if weights is None else weights.cuda())[0])     # seed 0 drew `init`
        assert np.array_equal(i1.cpu().numpy(), tidx)
        assert np.abs(c1.cpu().numpy() - tc).max() <= 1e-6 * np.abs(tc).max()
        assert len(h1) == iters + 1 and all(b <= a * (1 + 1e-6) for a, b in zip(h1, h1[1:]))
        assert np.allclose(h1, thist, rtol=1e-5, atol=0)
    # tol stops early, K == P is every row its own code, iters == 0 is the initial assignment
    c, i, h = compress.kmeans(x.cuda(), K, iters=50, tol=0.5, seed=0)
    assert len(h) < 10
    c, i, h = compress.kmeans(x[:50].cuda(), 50, iters=1, seed=1)
    assert sorted(i.cpu().tolist()) == list(range(50)) and h[-1] == 0.0
    c, i, h = compress.kmeans(x.cuda(), K, iters=0, seed=0)
    assert torch.equal(c.cpu(), init) and len(h) == 1


def test_kmeans_reseeds_empty_codes_in_the_stated_order():
    x = torch.zeros(6, 2)
    x[:, 0] = torch.tensor([0.0, 0.1, 5.0, 0.2, 9.0, 5.0])
    init = torch.tensor([[0.0, 0.0], [100.0, 100.0], [0.1, 0.0], [200.0, 0.0]])
    idx, err, _ = vt.assign(x.numpy(), init.numpy())
    new, _, count = vt.update_chunked(x.numpy(), idx, init.numpy())
    want = vt.reseed(x.numpy(), new, count, None, err)
    assert np.array_equal(want[1], x[4].numpy()) and np.array_equal(want[3], x[2].numpy())
    # after one iteration the final assignment sends the two reseeded rows to their own codes
    c, i, h = compress.kmeans(x.cuda(), 4, iters=1, init=init.cuda())
    assert np.array_equal(c.cpu().numpy().view(np.int32), want.view(np.int32))
    assert i.cpu().tolist() == vt.assign(x.numpy(), want)[0].tolist() and i[4].item() == 1 and i[2].item() == 3


def test_compressed_model_renders(tmp_path):
    W, H, P = 96, 64, 1500
    sc, cam = small_scene(P, W, H, seed=5, multiscale=True)
    from gaussian_renderer import render
    from synthetic_model import SyntheticGaussians
    pc = SyntheticGaussians(sc, "cuda", requires_grad=False)
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    st = dict(filter_small=True, filter_large=True, fade_size=0.0)
    draw = lambda m: render(cam.to("cuda"), m, PIPE, bg, **st)
    with torch.no_grad():
        ref = draw(pc)
    rows = compress.sh_rows(pc)
    assert rows.shape == (P, 45) and len(torch.unique(rows, dim=0)) == P
    idx, err = dgr.vq_assign(rows, rows)
    assert torch.equal(idx.cpu(), torch.arange(P, dtype=torch.int32)) and (err == 0).all()
    path = str(tmp_path / "own.npz")
    compress.save_compressed(pc, path, quantised=(rows, idx))
    back = compress.load_compressed(copy.copy(pc), path)
    assert back._features_rest.is_cuda and torch.equal(back._features_rest.detach(), pc._features_rest.detach())
    with torch.no_grad():
        out = draw(back)
    for k in ("render", "depth", "radii"):
        assert torch.equal(out[k], ref[k]), f"{k} differs after a lossless round trip"
    # K = 8 through k-means: lossy, but a model like any other — and the same arrays twice
    small, again = str(tmp_path / "k8.npz"), str(tmp_path / "k8b.npz")
    w = torch.rand(P, generator=torch.Generator().manual_seed(1)).cuda()
    cb, ix = compress.save_compressed(pc, small, sh_codes=8, iters=3, weights=w)
    compress.save_compressed(pc, again, sh_codes=8, iters=3, weights=w)
    with np.load(small) as a, np.load(again) as b:                 # (the zip records carry the time of writing)
        assert a.files == b.files and all(np.array_equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a.files)
    assert cb.shape == (8, 45) and ix.shape == (P,) and int(ix.max()) < 8
    lossy = compress.load_compressed(copy.copy(pc), small)
    assert torch.equal(compress.sh_rows(lossy), cb[ix.long()])
    assert torch.equal(lossy._opacity.detach(), pc._opacity.detach()) and torch.equal(lossy._scaling.detach(), pc._scaling.detach())
    with torch.no_grad():
        out = draw(lossy)
    assert out["render"].shape == ref["render"].shape and torch.isfinite(out["render"]).all()
    assert out["depth"].shape == ref["depth"].shape and torch.equal(out["radii"], ref["radii"])
    report("compressed K=8", "max abs colour difference from the original", float((out["render"] - ref["render"]).abs().max()))
    sizes = compress.compressed_size_report(small)
    assert sizes["total"] < compress.compressed_size_report(path)["total"]

"""The opt-in replay sweep without a GPU: pins and conditions from the reference alone (oracle/torch_oracle.py, tests/).

  1  tests/replay_truth.py IS the truths the project already trusts: on scene F (and `far`, `thin`) it reproduces every array of the
     five committed fixtures tests/golden/{absgrad,contrib,features,distortion,median_depth}_truth.npz, to the tolerance of the
     fixture's own CPU pin (integers and masks exactly, float64 arrays to 1e-12 of their max-norm).
  2  its restated blend loop is the oracle's: on EVERY case of tests/replay_cases.py — filters, fade, rigid poses, focal lengths,
     the scaling modifier, precomputed covariances — colour, depth, 1 - final_T, n_blended, radii and the borderline mask equal
     torch_oracle.rasterize in float64 (floats to 1e-12 of the max-norm, the rest exactly).
  3  the conditions that keep tests/test_replay_sweep_gpu.py from hiding a failure, per case, from the truth alone: borderline
     pixels <= 2 %; the haze cases blend > 256 resp. > 512 pairs at every pixel; half of the opaque case's pixels terminate; the
     filter cases have unrendered rows and empty pixels; the skipped-entry case has median entries at list positions above the
     pixel's blended count.
  4  the float32 evaluation of the same code takes the float64 decisions off the flagged pixels on every case, and is within
     BWD_RTOL of float64 on dL/dscaling and dL/drotation on >= 90 % of the cases: the list is not needle-heavy, so the float32
     allowance of the GPU sweep is an exception there and not the rule."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import replay_cases as rc
import replay_truth as rt
from parity_utils import BWD_RTOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = list(rc.CASES)


def _generator(kind):
    spec = importlib.util.spec_from_file_location(f"make_{kind}_golden", os.path.join(GOLDEN, f"make_{kind}_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m, np.load(os.path.join(GOLDEN, f"{kind}_truth.npz"))


def _same(got, want, key):
    """the rule of the fixtures' own CPU pins"""
    got = got.detach().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape, key
    if want.dtype == np.float64:
        assert np.abs(got.astype(np.float64) - want).max() <= 1e-12 * np.abs(want).max(), key
    else:
        assert np.array_equal(got.astype(want.dtype), want), key


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the module is the committed truths
# ---------------------------------------------------------------------------------------------------------------------------
def test_module_reproduces_the_absgrad_fixture():
    gen, t = _generator("absgrad")
    sc, cam, bg, dL = gen.scene_f()
    r = rt.render(sc, cam, bg=bg, per_pixel=True)
    g = rt.gradients(r, dict(color=dL.double() * (~r.borderline)[None]), absgrad=True)
    assert sorted(t.files) == ["absgrad", "borderline", "grad", "visible"]
    for k, got in (("absgrad", g["absgrad"]), ("grad", g["absgrad_net"]), ("borderline", r.borderline), ("visible", r.radii > 0)):
        _same(got, t[k], k)
    _same(g["means2D"][:, :2], t["grad"], "the per-pixel shares add up to dL/dmeans2D")


def test_module_reproduces_the_contrib_fixture():
    gen, t = _generator("contrib")
    r = rt.render(*gen.scene_f())
    seen = {"borderline", "visible", "alpha"}
    for k, got in (("borderline", r.borderline), ("visible", r.radii > 0), ("alpha", r.alpha)):
        _same(got, t[k], k)
    for name in ("plain", "weighted"):
        m = torch.from_numpy(t["m_" + name])
        assert not m[r.borderline].any()
        for k, got in zip(("sum_", "max_", "count_"), rt.contributions(r, m)):
            _same(got, t[k + name], k + name)
            seen |= {k + name, "m_" + name}
    assert seen == set(t.files)


def test_module_reproduces_the_features_fixture():
    gen, t = _generator("features")
    r = rt.render(*gen.scene_f(), features=torch.from_numpy(t["features"]))
    g = rt.gradients(r, dict(features=torch.from_numpy(t["G"])))
    got = dict(g, map=r.features, dfeatures=g["features"], borderline=r.borderline, visible=r.radii > 0)
    assert not t["G"][:, t["borderline"]].any()
    for k in t.files:
        if k not in ("features", "G"):
            _same(got[k], t[k], k)


@pytest.mark.parametrize("kind", ["F", "far"])
def test_module_reproduces_the_distortion_fixture(kind):
    gen, t = _generator("distortion")
    g_ = lambda k: t[f"{kind}_{k}"]
    r = rt.render(*gen.scene(kind))
    g = rt.gradients(r, dict(distortion=torch.from_numpy(g_("G"))))
    got = dict(g, map=r.distortion, borderline=r.borderline, visible=r.radii > 0, count=r.n_blended)
    assert not g_("G")[g_("borderline")].any()
    for k in t.files:
        if k.startswith(kind + "_") and k != kind + "_G":
            _same(got[k[len(kind) + 1:]], t[k], k)


@pytest.mark.parametrize("kind", ["F", "thin"])
def test_module_reproduces_the_median_depth_fixture(kind):
    gen, t = _generator("median_depth")
    g_ = lambda k: t[f"{kind}_{k}"]
    leaves = {}

    def edit(view):
        leaves["viewmatrix"] = view["viewmatrix"].to(torch.float64).clone().requires_grad_(True)
        view["viewmatrix"] = leaves["viewmatrix"]
    r = rt.render(*gen.scene(kind), view_edit=edit)
    g = rt.gradients(r, dict(median_depth=torch.from_numpy(g_("G"))), extra_leaves=leaves)
    got = dict(depth=r.median_depth, id=r.median_id, means3D=g["means3D"], viewmatrix=g["viewmatrix"], mask=r.borderline | r.near,
               borderline=r.borderline, near=r.near, visible=r.radii > 0, count=r.n_blended, crossed=r.crossed, pos=r.median_pos)
    assert not g_("G")[g_("mask")].any()
    for k in t.files:
        if k.startswith(kind + "_") and k != kind + "_G":
            _same(got[k[len(kind) + 1:]], t[k], k)
    for k in ("opacities", "scales", "rotations", "means2D"):                      # the map moves with the depths alone
        assert not g[k].any(), k


def test_scene_f_of_the_sweep_is_the_fixtures_scene():
    gen, _ = _generator("features")
    sc, _ = gen.scene_f()
    c = rc.CASES["F"]()
    for k in ("means3D", "opacities", "scales", "rotations", "shs"):
        assert torch.equal(getattr(c.scene, k), getattr(sc, k)), k
    assert (c.cam.image_width, c.cam.image_height, c.settings, c.smod) == (40, 24, rt.PLAIN, 1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the restated loop is the oracle's, on every case
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_restated_loop_is_the_oracles(name):
    from oracle import torch_oracle as to
    c, r, _ = rc.truth(name)
    L = r.leaves
    kw = dict(shs=L["shs"], max_pixel_sizes=c.scene.max_pixel_sizes, min_pixel_sizes=c.scene.min_pixel_sizes,
              base_mask=c.scene.base_mask)
    if c.cov3D_precomp:
        kw["cov3D_precomp"] = to.cov3d_from_scale_rot(L["scales"], L["rotations"], c.smod)
    else:
        kw["scales"], kw["rotations"] = L["scales"], L["rotations"]
    view = to.view_dict(c.cam, sh_degree=c.scene.sh_degree, scale_modifier=c.smod, **c.settings)
    with torch.no_grad():
        color, _, depth, radii, _, aux = to.rasterize(L["means3D"], L["opacities"], view, c.bg, **kw)
    worst = {}
    for k, got, want in (("color", r.color, color), ("depth", r.depth, depth), ("alpha", r.alpha, 1.0 - aux["final_T"])):
        worst[k] = ((got.detach() - want).abs().max() / want.abs().max().clamp_min(1e-300)).item()
    print(f"{name}: restated loop vs rasterize {worst}")
    assert all(v <= 1e-12 for v in worst.values()), worst
    assert torch.equal(r.n_blended, aux["n_blended"]) and torch.equal(r.borderline, aux["borderline"])
    assert torch.equal(r.radii, radii) and r.radii.dtype == torch.int32
    assert torch.equal(r.final_T, 1.0 - r.alpha.detach())


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the conditions of the GPU sweep
# ---------------------------------------------------------------------------------------------------------------------------
def test_case_list_covers_what_it_must():
    cases = {n: fn() for n, fn in rc.CASES.items()}
    assert 20 <= len(cases) <= 28
    assert all(c.cam.image_width <= 130 and c.cam.image_height <= 90 for c in cases.values())
    sizes = {(c.scene.means3D.shape[0], c.cam.image_width, c.cam.image_height) for c in cases.values()}
    assert {(1, 1, 1), (7, 17, 1), (63, 33, 17), (64, 33, 17), (65, 33, 17)} <= sizes
    assert any(w % 16 == 0 and h % 16 == 0 for _, w, h in sizes)
    assert {1, 8, 9, 17} <= {c.features.shape[1] for c in cases.values()}
    assert {0.7, 1.6} <= {c.smod for c in cases.values()}
    assert sum(c.cov3D_precomp for c in cases.values()) >= 1
    front = torch.eye(4)
    rigid = [c for c in cases.values() if (c.cam.world_view_transform.float() - front).abs().max() > 1e-3]
    assert len(rigid) >= 4
    tans = {round(float(np.tan(c.cam.FoVx / 2)), 3) for c in rigid}    # tan(FoVx / 2) = 0.96 / focal at every width
    assert {0.96, 1.6, round(0.96 / 1.7, 3)} <= tans                  # focal 1.0, 0.6 and 1.7 among the rigid poses
    assert {(True, 0.0), (True, 0.5)} <= {(c.settings["filter_small"] and c.settings["filter_large"], c.settings["fade_size"])
                                          for c in cases.values()}


@pytest.mark.parametrize("name", NAMES)
def test_borderline_pixels_stay_under_the_cap(name):
    _, r, seconds = rc.truth(name)
    share, near = r.borderline.float().mean().item(), (r.near & ~r.borderline).float().mean().item()
    lists = max((t[4].numel() for t in r.tiles), default=0)
    print(f"{name}: {r.W} x {r.H}, P {r.P}, rendered {int((r.radii > 0).sum())}, borderline {int(r.borderline.sum())} of {r.W * r.H} "
          f"({100 * share:.2f} %), near-median {100 * near:.2f} %, blended pairs per pixel {int(r.n_blended.min())} .. "
          f"{int(r.n_blended.max())}, longest list {lists}, truth {seconds:.2f} s")
    assert r.borderline.sum().item() <= rt.MAX_BORDERLINE * r.W * r.H


def test_haze_cases_blend_past_one_and_two_batches():
    for name, batches in (("haze2", 1), ("haze3", 2)):
        _, r, _ = rc.truth(name)
        assert r.n_blended.min().item() > 256 * batches, name
        assert (r.final_T > 1e-3).all(), name                          # ... without terminating
    c = rc.CASES["haze2"]()
    assert c.cam.image_width % 16 and c.cam.image_height % 16         # partial tiles in x and y


def test_opaque_case_terminates_inside_long_lists():
    _, r, _ = rc.truth("opaque")
    assert max(t[4].numel() for t in r.tiles) > 1024
    assert r.terminated.float().mean().item() >= 0.5                  # (an entry's T (1 - alpha) < 1e-4 ended the pixel: Q7)
    assert (r.final_T[r.terminated] < 1e-2).all()
    assert r.n_blended.max().item() < 256                             # ... within the first batch of lists five batches long


@pytest.mark.parametrize("name", rc.FILTERED)
def test_filter_cases_have_unrendered_rows_and_empty_pixels(name):
    c, r, _ = rc.truth(name)
    assert c.settings["filter_small"] and c.settings["filter_large"]
    assert 0 < (r.radii == 0).sum().item() < r.P
    assert (r.n_blended == 0).any() and (r.median_id[r.n_blended == 0] == -1).all()


def test_filter_fade_changes_the_opacities_the_replays_use():
    _, r0, _ = rc.truth("ms_fade0")
    _, r5, _ = rc.truth("ms_fade05")
    faded = (r5.radii > 0) & (r0.radii == 0)                          # the fade keeps Gaussians the hard filter drops ...
    assert faded.any() and not ((r0.radii > 0) & (r5.radii == 0)).any()
    o, o_eff = r5.leaves["opacities"].detach().reshape(-1), r5.pre["opacity"].detach()
    assert (o_eff[faded] < o[faded]).all() and (o_eff[faded] > 0).all()       # ... with their opacity weighed down
    both = (r5.radii > 0) & ~faded
    assert torch.equal(o_eff[both], o[both])
    hit = torch.zeros(r5.P, dtype=torch.bool)
    for t in r5.tiles:
        hit[t[4][t[6].any(1)]] = True
    assert (hit & faded).any()                                        # ... and some pixel blends one of them


def test_skipped_entry_case_has_medians_behind_skipped_entries():
    _, r, _ = rc.truth("median_behind_skipped")
    has = r.median_id >= 0
    behind = has & (r.median_pos > r.n_blended)
    print(f"median_behind_skipped: {int(behind.sum())} pixels with the median entry above the blended count, "
          f"{int((r.median_pos >= 256).sum())} in the second batch, position up to {int(r.median_pos.max())}")
    assert behind.any()
    assert (r.median_pos >= 256).any() and r.n_blended.max().item() < 177


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the float32 evaluation of the same code
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_float32_evaluation_takes_the_same_decisions(name):
    _, r, _ = rc.truth(name)
    _, s, _ = rc.truth(name, torch.float32)
    assert s.color.dtype == torch.float32 and s.pre["conic"].dtype == torch.float32
    keep = ~r.borderline
    assert torch.equal(s.radii, r.radii)
    assert torch.equal(s.n_blended[keep], r.n_blended[keep])
    for a, b in zip(r.tiles, s.tiles):
        assert torch.equal(a[4], b[4])                                # the same lists ...
        k = keep[a[2]:a[3], a[0]:a[1]].reshape(-1)
        assert torch.equal(a[6][:, k], b[6][:, k])                    # ... and the same blended pairs
    km = keep & ~r.near
    assert torch.equal(s.median_id[km], r.median_id[km])


def test_float32_evaluation_meets_the_tolerance_on_most_cases():
    """a condition on the case list: where the reference's own float32 arithmetic misses BWD_RTOL on dL/dscaling / dL/drotation,
    a float32 kernel cannot be asked to meet it"""
    within = 0
    for name in NAMES:
        g, s = rc.truth_gradients(name), rc.truth_gradients(name, dtype=torch.float32)
        e = {k: ((s[k].double() - g[k]).abs().max() / g[k].abs().max().clamp_min(1e-300)).item() for k in ("scales", "rotations")}
        print(f"{name}: float32 evaluation vs float64 {e}")
        within += max(e.values()) <= BWD_RTOL
    assert within >= 0.9 * len(NAMES), (within, len(NAMES))

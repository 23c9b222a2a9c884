"""The seeded case list of the opt-in replay sweep (tests/test_replay_sweep_cpu.py, tests/test_replay_sweep_gpu.py): what the
committed float64 truths of the opt-in outputs (scene F, 40 x 24, front camera, filters off) never reach — tile lists of two and
three 256-entry batches that never terminate, early termination inside lists of hundreds, the multi-scale filters with and without
a fade, general view matrices, other focal lengths, the scaling modifier, the precomputed-covariance entry, models of 1 / 7 / 63 /
64 / 65 rows, feature widths around FEAT_CB = 8, and a median crossing that lies behind entries the pixel skips.

Every case is a small function of fixed seeds that returns a Case; scenes come from parity_utils.small_scene and fuzz_cases.posed,
nothing here builds a scene of its own.  The conditions that make a case what its name says are asserted from the float64 truth
alone in tests/test_replay_sweep_cpu.py.  Not here: the `deep` scene of tests/test_absgrad_gpu.py (3000 Gaussians, opacities 0.02 ..
0.06): 82 of its 480 pixels are borderline, and masking them would hide a sixth of the image."""
import collections
import functools
import time

import torch

import replay_truth as rt
import scenes
from fuzz_cases import posed
from parity_utils import small_scene

PLAIN = dict(filter_small=False, filter_large=False, fade_size=1.0)
Case = collections.namedtuple("Case", "name scene cam settings smod seeds features bg cov3D_precomp")


def _uniform(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) - 0.5


def weight_map(W, H, seed=81):
    """[H,W] float32: a quarter of the pixels 0, the others uniform in (0.25, 2.25) (tests/golden/make_contrib_golden.py)"""
    g = torch.Generator().manual_seed(seed)
    m = 0.25 + 2.0 * torch.rand(H, W, generator=g)
    return torch.where(torch.rand(H, W, generator=g) < 0.25, torch.zeros(H, W), m)


def _case(name, sc, cam, C, st=PLAIN, smod=1.0, cov=False, bg=(0.2, 0.4, 0.1)):
    """the seeds of the fixtures of scene F at this image size: colour 78, depth 77 (x 0.1), alpha 79, distortion 131, median
    depth 151, features 91 / 92, contribution weights 81"""
    W, H = cam.image_width, cam.image_height
    assert W <= 130 and H <= 90
    seeds = dict(color=scenes.grad_seed(W, H, 78), depth=scenes.grad_seed(W, H, 77)[0] * 0.1, alpha=scenes.grad_seed(W, H, 79)[1],
                 distortion=_uniform((H, W), 131), median_depth=_uniform((H, W), 151), features=_uniform((C, H, W), 92),
                 weights=weight_map(W, H))
    feats = torch.rand(sc.means3D.shape[0], C, generator=torch.Generator().manual_seed(91))
    return Case(name, sc, cam, dict(st), float(smod), seeds, feats, torch.tensor(bg), cov)


def _haze(P, W, H, seed, lo):
    sc, cam = small_scene(P, W, H, seed=seed, scale_k=6.0)
    sc.opacities = lo + lo * torch.rand(sc.opacities.shape, generator=torch.Generator().manual_seed(seed))
    return sc, cam


def _multiscale(fade):
    sc, cam = small_scene(777, 100, 70, seed=12, multiscale=True, scale_k=0.004 * 1920 / 100 * 0.25)
    return sc, cam, dict(filter_small=True, filter_large=True, fade_size=fade)


def _rigid(P, W, H, seed, focal, **kw):
    sc, cam = small_scene(P, W, H, seed=seed, **kw)
    return posed(sc, cam, "rigid", focal, seed)


def case_f():
    return _case("F", *small_scene(200, 40, 24, seed=1), C=5)


def case_haze_two_batches():
    return _case("haze2", *_haze(500, 24, 20, 3, 0.008), C=8)


def case_haze_three_batches():
    return _case("haze3", *_haze(700, 40, 24, 5, 0.006), C=1)


def case_opaque():
    return _case("opaque", *small_scene(1500, 40, 24, seed=1, scale_k=0.192), C=9)


def case_multiscale_fade0():
    sc, cam, st = _multiscale(0.0)
    return _case("ms_fade0", sc, cam, C=17, st=st)


def case_multiscale_fade05():
    sc, cam, st = _multiscale(0.5)
    return _case("ms_fade05", sc, cam, C=8, st=st)


def case_p1():
    return _case("p1_1x1", *small_scene(1, 1, 1, seed=2), C=1)


def case_p7():
    return _case("p7_17x1", *small_scene(7, 17, 1, seed=4), C=9)


def case_p63():
    return _case("p63_33x17", *small_scene(63, 33, 17, seed=63), C=17)


def case_p64():
    return _case("p64_33x17", *small_scene(64, 33, 17, seed=64), C=8)


def case_p65():
    return _case("p65_33x17", *small_scene(65, 33, 17, seed=65), C=9)


def case_whole_tiles():
    return _case("whole_tiles_48x32", *small_scene(150, 48, 32, seed=8), C=5)


def case_rigid_a():
    return _case("rigid_a", *_rigid(300, 56, 40, 21, 1.0), C=5)


def case_rigid_b():
    return _case("rigid_b", *_rigid(260, 41, 23, 22, 1.0), C=1)


def case_rigid_wide():
    return _case("rigid_focal06", *_rigid(300, 56, 40, 23, 0.6), C=9)


def case_rigid_narrow():
    return _case("rigid_focal17", *_rigid(300, 56, 40, 24, 1.7), C=8)


def case_rigid_multiscale():
    sc, cam = _rigid(500, 72, 50, 25, 1.0, multiscale=True, scale_k=0.004 * 1920 / 72 * 0.25)
    return _case("rigid_ms_fade05", sc, cam, C=5, st=dict(filter_small=True, filter_large=True, fade_size=0.5))


def case_front_wide():
    sc, cam = small_scene(250, 40, 24, seed=26)
    return _case("front_focal06", *posed(sc, cam, "front", 0.6, 26), C=5)


def case_smod07():
    return _case("smod07", *small_scene(250, 40, 24, seed=31), C=5, smod=0.7)


def case_smod16():
    return _case("smod16", *small_scene(250, 40, 24, seed=32), C=17, smod=1.6)


def case_cov3d_precomp():
    return _case("cov3D_precomp", *small_scene(220, 40, 24, seed=41), C=5, cov=True)


def case_median_behind_skipped():
    """small footprints and low opacities: a pixel skips most of its tile's list (alpha < 1/255 there) and needs many blends to
    cross 1/2, so the median entry sits at a list position far above the pixel's blended count (41 .. 108 blended pairs per pixel;
    the median entry at list positions up to 371, on 96 pixels in the second 256-entry batch)"""
    sc, cam = small_scene(1000, 40, 24, seed=29, scale_k=0.004 * 1920 / 40 * 0.45)
    sc.opacities = sc.opacities * torch.tensor(0.2, dtype=torch.float32)
    return _case("median_behind_skipped", sc, cam, C=1)


def case_thin():
    """the `thin` scene of tests/golden/make_median_depth_golden.py: empty, crossing and never-crossing pixels"""
    sc, cam = small_scene(20, 40, 24, seed=3)
    sc.opacities = sc.opacities * torch.tensor(0.35, dtype=torch.float32)
    return _case("thin", sc, cam, C=8)


def case_sparse():
    """the `sparse` scene of tests/test_absgrad_gpu.py: whole tiles empty, odd sizes"""
    return _case("sparse_41x23", *small_scene(8, 41, 23, seed=5), C=9)


CASES = collections.OrderedDict((fn().name, fn) for fn in (
    case_f, case_haze_two_batches, case_haze_three_batches, case_opaque, case_multiscale_fade0, case_multiscale_fade05, case_p1,
    case_p7, case_p63, case_p64, case_p65, case_whole_tiles, case_rigid_a, case_rigid_b, case_rigid_wide, case_rigid_narrow,
    case_rigid_multiscale, case_front_wide, case_smod07, case_smod16, case_cov3d_precomp, case_median_behind_skipped, case_thin,
    case_sparse))
OUTPUTS = ("color", "depth", "alpha", "distortion", "median_depth", "features")      # replay_truth.MAPS: the seeded maps


@functools.lru_cache(maxsize=None)
def truth(name, dtype=torch.float64):
    """(case, replay_truth.render of it in `dtype`, CPU seconds), computed once per process"""
    c = CASES[name]()
    t0 = time.perf_counter()
    r = rt.render(c.scene, c.cam, c.settings, c.smod, bg=c.bg, features=c.features, cov3D_precomp=c.cov3D_precomp, dtype=dtype,
                  per_pixel=dtype == torch.float64)
    return c, r, time.perf_counter() - t0


def masked_seeds(name):
    """the case's seeds, zero where the float64 truth flags the pixel: every map on its borderline pixels, the median depth also
    on the pixels with a blended T within replay_truth.NEAR of 1/2; "ones" / "weights": the two contribution weight maps"""
    c, r, _ = truth(name)
    keep, keep_m = (~r.borderline).to(torch.float32), (~(r.borderline | r.near)).to(torch.float32)
    out = {k: c.seeds[k] * (keep_m if k == "median_depth" else keep) for k in OUTPUTS}
    out["ones"], out["weights"] = keep.clone(), c.seeds["weights"] * keep
    return out


@functools.lru_cache(maxsize=None)
def truth_gradients(name, outputs=OUTPUTS, dtype=torch.float64):
    """replay_truth.gradients of the case for the masked seeds of `outputs` (absgrad with the float64 evaluation)"""
    _, r, _ = truth(name, dtype)
    seeds = masked_seeds(name)
    return rt.gradients(r, {k: seeds[k] for k in outputs}, absgrad=dtype == torch.float64)


HAZE = ("haze2", "haze3")
FILTERED = ("ms_fade0", "ms_fade05")
ALONE = HAZE + ("opaque",) + FILTERED          # the cases that also run each opt-in output alone
MEDIAN_ALONE = ("median_behind_skipped",)      # ... and the one whose median replay goes past the first batch: the median alone

"""Every route stage 2 of the forward can take, against an exact-buffer single-pass render of the same inputs.

Stage 2 (emit, tile sort, ranges, blend) normally goes out speculatively on buffers sized from a guess of the instance count D
(capacity = guess + guess / 8 + 4096, diff_gaussian_rasterization._capacity); a view that outgrew that capacity has its
stage 2 redone on exact buffers, on the same geom (msgs_forward_stage2: _forward_impl immediately, _PendingForward.resolve for a
deferred view).  With depth slabs on that redo must not read anything the truncated run left behind as its own:
in particular the coarse cell ranges stage 1's scan leaves in geom.offs_b, which slab B's recount consumes (and overwrites with
its counts, which slab B's scan then turns into offsets): a redo that decodes those offsets as ranges drops instances from open
tiles — with a handful of tiles open (the cell prefilter) and with most of them open alike.

The matrix: three views of >= 2048 tiles (a dense opaque scene in which slab A leaves a PARTIAL set of tiles open — the recount's
cell prefilter — a multi-scale one with its filters on, a hazy one in which most tiles stay open), the guess states around
the capacity boundary, slabs off / forced / adaptive, the reference and the raw-parameter entries, immediate and deferred
(ViewPipeline: the redo happens in resolve()), with a backward and forward-only.  Every cell is BIT-IDENTICAL to the single
pass: outputs, D, final_T / n_contrib, the means2D gradient and the six leaf gradients; every cell asserts the route it took
(forward_stats["non_speculative"]) and the slab header.  Plus: stage 2 run twice on one geom through the C ABI gives the same
bits (the invariant the redo relies on), and one redo cell against the float32 CPU oracle."""
import ctypes as C

import pytest
import torch

import scenes
from parity_utils import PIPE, check_backward, check_forward, hip_render
from route_utils import (PLAIN, assert_identical, capacity, guesses_around, non_speculative, per_pixel, reset_forward_state,
                         result, slab_stats)

pytestmark = pytest.mark.gpu
FILTERS = dict(filter_small=True, filter_large=True, fade_size=0.0)
RANGED_MAX_OPEN = 1024          # binning.hip slab_recount_kernel: up to this many open tiles the coarse-cell prefilter is used


def _scene(name):
    """(scene, camera, settings, background, dL/dcolor) of the three views; 10^5 Gaussians each"""
    if name == "partial":       # dense and opaque: pixels terminate inside slab A, at fraction 0.12 a few hundred tiles stay open
        W, H, seed = 1280, 720, 31
        sc = scenes.frustum_scene(100_000, W, H, seed=seed, scale_k=0.004 * 1920.0 / W * 3.0)
        opac, st = (0.6, 0.99), PLAIN
    elif name == "multiscale":  # multi-scale levels and their filters
        W, H, seed = 1024, 800, 32
        sc = scenes.frustum_scene(100_000, W, H, seed=seed, multiscale=True, scale_k=0.004 * 1920.0 / W * 2.0)
        opac, st = (0.6, 0.99), FILTERS
    else:                       # hazy: nothing terminates, most tiles stay open (the recount without cell ranges)
        W, H, seed = 1280, 720, 33
        sc = scenes.frustum_scene(100_000, W, H, seed=seed, scale_k=0.004 * 1920.0 / W * 1.3)
        opac, st = (0.004, 0.02), PLAIN
    g = torch.Generator().manual_seed(seed + 7)
    sc.opacities[:, 0] = opac[0] + (opac[1] - opac[0]) * torch.rand(sc.P, generator=g)
    cam = scenes.front_camera(W, H).to("cuda")
    bg = torch.tensor([0.3, 0.1, 0.2], device="cuda")
    dL = scenes.grad_seed(W, H, seed).cuda()
    return sc, cam, st, bg, dL


def _render(entry, sc, cam, st, bg, dL, mod=1.0):
    """one render through `entry` = (fused, deferred, backward); returns route_utils.result()"""
    from gaussian_renderer import render, render_fused
    from multi_view import ViewPipeline
    from synthetic_model import SyntheticGaussians
    fused, deferred, backward = entry
    fn = render_fused if fused else render
    pc = SyntheticGaussians(sc, "cuda", requires_grad=backward)
    if backward:
        if deferred:
            kept = []

            def bwd(i, pkg):
                pkg["render"].backward(dL)
                kept.append(pkg)
                return pkg["viewspace_points"]
            ViewPipeline("cuda", n_streams=2).train_views([cam], pc, PIPE, bg, bwd, render_fn=fn, scaling_modifier=mod, **st)
            out = kept[0]
        else:
            out = fn(cam, pc, PIPE, bg, scaling_modifier=mod, **st)
            out["render"].backward(dL)
    else:
        with torch.no_grad():
            if deferred:
                out = ViewPipeline("cuda", n_streams=2).render_views([cam], pc, PIPE, bg, render_fn=fn, scaling_modifier=mod,
                                                                     **st)[0]
            else:
                out = fn(cam, pc, PIPE, bg, scaling_modifier=mod, **st)
    torch.cuda.synchronize()
    return result(out, pc, out["render"].grad_fn if backward else None, cam.image_width, cam.image_height)


def _single_pass(entry, sc, cam, st, bg, dL, mod=1.0):
    """the yardstick: wrapper state reset (exact buffers), no slabs"""
    import diff_gaussian_rasterization as dgr
    prev, dgr.slab_policy = dgr.slab_policy, "never"
    try:
        reset_forward_state()
        n0 = non_speculative()
        r = _render(entry, sc, cam, st, bg, dL, mod)
        assert non_speculative() - n0 == 1             # the first-call route
        return r
    finally:
        dgr.slab_policy = prev


def _speculative_fits(entry, key, guess, sc, cam, st, bg, dL):
    """does a forward-only render through `entry`'s route (immediate / deferred) with this guess keep its speculative stage 2?"""
    import diff_gaussian_rasterization as dgr
    reset_forward_state()
    dgr._last_instances[key] = guess
    n0 = non_speculative()
    _render((entry[0], entry[1], False), sc, cam, st, bg, dL)
    return non_speculative() == n0


def _boundary(entry, key, D, sc, cam, st, bg, dL):
    """(largest guess that takes the redo, smallest guess whose speculative stage 2 stands) for this route and slab setting.
    The library sizes the speculative stage 2 from the BYTES of the buffers the wrapper hands it, which the caching allocator's
    size classes round up; in slab mode it derives the capacity from the slab layout's byte counts, which can come out a few
    instances below the formula's — so the real boundary lies near the formula's (route_utils.guesses_around), not on it"""
    lo, hi = D // 2, guesses_around(D)[1]
    assert not _speculative_fits(entry, key, lo, sc, cam, st, bg, dL)
    while not _speculative_fits(entry, key, hi, sc, cam, st, bg, dL):
        lo, hi = hi, hi + 64
        assert hi <= D, (hi, D)              # a guess of D itself must fit
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _speculative_fits(entry, key, mid, sc, cam, st, bg, dL):
            hi = mid
        else:
            lo = mid
    return lo, hi


ENTRIES = {"render": (False, False, True), "fused": (True, False, True), "deferred": (False, True, True),
           "no_grad": (False, False, False), "fused_deferred_no_grad": (True, True, False)}
# guess state -> route it claims (1: the redo / first-call route, 0: the speculative stage 2 stands, None: either)
GUESSES = {"none": 1, "exact": 0, "half": 1, "just_below": 1, "just_fits": 0, "tenfold": 0, "growth": 1, "by_view_P+3%": None}


def _cell(entry, guess_state, sc, cam, st, bg, dL, D, key, D_grown, priming, bounds):
    """set up the guess state (after `priming` frames of the view, which the adaptive policy needs) and render one cell;
    returns (result, routes taken, scaling modifier)"""
    import diff_gaussian_rasterization as dgr
    reset_forward_state()
    mod = 1.0
    if guess_state == "growth":             # the same key rendered with larger footprints after frames at 1.0
        for _ in range(priming):
            _render(ENTRIES["no_grad"], sc, cam, st, bg, dL, 1.0)
        mod, D = 1.5, D_grown
        assert capacity(dgr._instance_guess(key)) < D, (D, dgr._instance_guess(key))
    elif guess_state == "by_view_P+3%":     # a key never seen, guessed from the view shape's last count scaled by P
        small = sc.subset(torch.arange(int(round(sc.P / 1.03))))
        for _ in range(priming):
            _render(ENTRIES["no_grad"], small, cam, st, bg, dL)
        assert key not in dgr._last_instances and dgr._instance_guess(key) is not None
    elif guess_state != "none":
        for _ in range(priming):
            _render(ENTRIES["no_grad"], sc, cam, st, bg, dL)
        g = {"exact": D, "half": D // 2, "tenfold": 10 * D}.get(guess_state)
        if g is None:
            g = bounds[entry[1]][0 if guess_state == "just_below" else 1]
        dgr._last_instances.clear()
        dgr._last_instances[key] = g
    guess = dgr._instance_guess(key)
    expect = GUESSES[guess_state]
    assert (guess is None) == (guess_state == "none")
    if guess is not None and capacity(guess) >= D + 4096 and guess_state != "just_below":
        assert expect in (0, None), (guess_state, guess, D)
        expect = 0
    n0 = non_speculative()
    r = _render(entry, sc, cam, st, bg, dL, mod)
    redo = non_speculative() - n0
    assert expect is None or redo == expect, (guess_state, "route", redo, guess, D)
    return r, redo, mod


@pytest.mark.parametrize("policy", ["never", "0.04", "0.12", "adaptive"])
@pytest.mark.parametrize("name", ["partial", "multiscale", "hazy"])
def test_capacity_routes_match_the_single_pass(name, policy):
    import diff_gaussian_rasterization as dgr
    sc, cam, st, bg, dL = _scene(name)
    refs = {}
    for e in ENTRIES.values():
        for mod in (1.0, 1.5):
            if (e[0], e[2], mod) not in refs:
                refs[(e[0], e[2], mod)] = _single_pass(e, sc, cam, st, bg, dL, mod)
    D, D_grown = refs[(False, True, 1.0)][2], refs[(False, True, 1.5)][2]
    key, = list(dgr._last_instances)            # (every single pass rendered this key)
    assert D > 8 * 4096 and D_grown > capacity(D), (D, D_grown)
    prev = dgr.slab_policy, dgr.SLAB_MIN_INSTANCES, dgr.SLAB_MIN_RATIO
    seen = []
    try:
        if policy == "adaptive":
            # three frames of the key publish D and D_trav, the fourth plans slabs.  The thresholds are lowered to these views
            # (10^5 Gaussians; the hazy one walks its lists): which views SHOULD engage is test_slab_gpu's subject, not this one's
            dgr.SLAB_MIN_INSTANCES, dgr.SLAB_MIN_RATIO = D // 4, 1.0
        dgr.slab_policy = policy
        priming = 3 if policy == "adaptive" else 1
        # the largest guess that redoes and the smallest that fits, immediate and deferred (the buffers are allocated differently)
        bounds = None
        if policy != "adaptive":
            bounds = {dfr: _boundary((False, dfr, False), key, D, sc, cam, st, bg, dL) for dfr in (False, True)}
        for guess_state in GUESSES:
            if policy == "adaptive" and guess_state in ("none", "just_below", "just_fits"):
                continue        # no guess: no plan (the single pass itself); the boundary searches would need priming per probe
            entries = ENTRIES if guess_state in ("half", "just_below", "just_fits", "growth") else {"render": ENTRIES["render"]}
            for ename, e in entries.items():
                r, redo, mod = _cell(e, guess_state, sc, cam, st, bg, dL, D, key, D_grown, priming, bounds)
                what = (name, policy, guess_state, ename)
                assert_identical(r, refs[(e[0], e[2], mod)], what, backward=e[2])
                s = r[3]
                seen.append((guess_state, ename, redo, None if s is None else s["n_open"]))
                if s is None:
                    continue
                assert s["overflow"] == 0, (what, s)
                assert s["active"] == (policy != "never"), (what, s)
                if s["active"] and name == "partial" and mod == 1.0:
                    assert s["n_open"] > 0, (what, s)
                    if policy != "0.04":        # (at 0.04 most tiles stay open: the ranged recount without the cell mask)
                        assert s["n_open"] <= RANGED_MAX_OPEN, (what, "the cell prefilter of the recount was not reached", s)
                if s["active"] and name == "hazy":
                    assert s["n_open"] > RANGED_MAX_OPEN, (what, s)
    finally:
        dgr.slab_policy, dgr.SLAB_MIN_INSTANCES, dgr.SLAB_MIN_RATIO = prev
    print(f"[routes] {name} {policy}: D {D} (x1.5: {D_grown}), boundary {bounds}; (guess, entry, redo, n_open): {seen}")
    assert any(redo for _, _, redo, _ in seen) and any(not redo for _, _, redo, _ in seen)


@pytest.mark.parametrize("name", ["partial", "multiscale"])
def test_capacity_routes_in_the_verification_mode(name):
    """set_deterministic(True): slabs are off whatever the policy; the speculative and redo routes against its own single pass"""
    import diff_gaussian_rasterization as dgr
    sc, cam, st, bg, dL = _scene(name)
    prev = dgr.set_deterministic(True)
    prev_pol = dgr.slab_policy
    try:
        refs = {e: _single_pass(ENTRIES[e], sc, cam, st, bg, dL) for e in ("render", "deferred")}
        D = refs["render"][2]
        key, = list(dgr._last_instances)
        dgr.slab_policy = "0.12"
        bounds = {dfr: _boundary((False, dfr, False), key, D, sc, cam, st, bg, dL) for dfr in (False, True)}
        for guess_state in ("half", "just_below", "just_fits", "tenfold"):
            for ename in ("render", "deferred"):
                r, redo, _ = _cell(ENTRIES[ename], guess_state, sc, cam, st, bg, dL, D, key, None, 1, bounds)
                assert_identical(r, refs[ename], (name, "deterministic", guess_state, ename))
                assert r[3]["active"] == 0 and r[3]["overflow"] == 0
    finally:
        dgr.slab_policy = prev_pol
        dgr.set_deterministic(prev)


def test_stage2_twice_on_one_geom_is_bit_identical():
    """msgs_forward_stage2 a second time on the geom of a finished forward (fresh binning and scratch, as resolve() does),
    slab mode on with a partial set of tiles open: image, final_T and n_contrib are the same bits, and so is the slab header.
    This is what the redo of a truncated speculative stage 2 relies on: nothing stage 2 writes into geom is read back as input."""
    import diff_gaussian_rasterization as dgr
    from gaussian_renderer import render
    from synthetic_model import SyntheticGaussians
    sc, cam, st, bg, dL = _scene("partial")
    W, H = cam.image_width, cam.image_height
    prev = dgr.slab_policy
    try:
        dgr.slab_policy = "0.12"
        reset_forward_state()
        pc = SyntheticGaussians(sc, "cuda")
        out = render(cam, pc, PIPE, bg, **st)          # first call: exact buffers
        torch.cuda.synchronize()
    finally:
        dgr.slab_policy = prev
    ctx = out["render"].grad_fn
    call = ctx.call
    geom, _, image, D = dgr._resolve(ctx.state)
    s1 = slab_stats(ctx)
    assert s1["active"] == 1 and s1["overflow"] == 0 and 0 < s1["n_open"] <= RANGED_MAX_OPEN, s1
    first = [out[k].clone() for k in ("render", "acc_pixel_size", "depth")] + list(per_pixel(image, W, H))
    frac = float(call.view.slab_fraction)
    assert frac > 0.0
    lib = dgr._C.lib
    nb, ns = dgr._stage2_bytes(D, W, H, frac)
    binning, scratch2 = dgr._bytes(nb, call.device), dgr._bytes(ns, call.device)
    color = torch.full_like(out["render"], float("nan"))
    acc_ps, depth = torch.full_like(out["acc_pixel_size"], float("nan")), torch.full_like(out["depth"], float("nan"))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dgr._C.check(lib.msgs_forward_stage2(call.view_ref, call.g_ref, dgr._ptr(geom), geom.numel(), D,
                                         dgr._ptr(binning), binning.numel(), dgr._ptr(scratch2), scratch2.numel(),
                                         dgr._ptr(image), image.numel(), dgr._ptr(color), dgr._ptr(acc_ps), dgr._ptr(depth),
                                         None, 0, 0, None, stream), "msgs_forward_stage2")
    torch.cuda.synchronize()
    second = [color, acc_ps, depth] + list(per_pixel(image, W, H))
    for what, a, b in zip(("render", "acc_pixel_size", "depth", "final_T", "n_contrib"), first, second):
        assert torch.equal(a, b), what
    s2 = slab_stats(ctx)
    assert s2 == s1, (s1, s2)


def test_slab_redo_against_the_oracle():
    """the partial view, slab mode, a guess of D / 2 (the redo on exact buffers) against the float32 CPU oracle: what identity
    with the single pass cannot see (a bug both routes share)"""
    import diff_gaussian_rasterization as dgr
    from oracle import oracle_ctypes as oc
    sc, cam, st, bg, dL = _scene("partial")
    prev = dgr.slab_policy
    try:
        dgr.slab_policy = "0.12"
        reset_forward_state()
        hip_render(sc, cam, st, bg, dL)                 # first call: learns D and the key
        key, = [k for k in dgr._last_instances]
        D = dgr._last_instances[key]
        dgr._last_instances[key] = D // 2
        n0 = non_speculative()
        out, pc, m2 = hip_render(sc, cam, st, bg, dL)
        assert non_speculative() - n0 == 1
    finally:
        dgr.slab_policy = prev
    s = slab_stats(out["render"].grad_fn)
    assert s["active"] == 1 and s["overflow"] == 0 and 0 < s["n_open"] <= RANGED_MAX_OPEN, s
    cpu_cam, cpu_bg, cpu_dL = cam.to("cpu"), bg.cpu(), dL.cpu()
    orc = oc.rasterize(pc.seen, cpu_cam, st, cpu_bg)
    og = oc.backward(orc, cpu_dL)
    check_forward(out, orc, "slab redo")
    check_backward(pc, m2, og, "slab redo", flagged=orc.borderline_gaussians)

"""Shared helpers of the tests that steer the forward's routes (speculative stage 2, the redo on exact buffers, depth slabs):
the wrapper state that decides a route, reset in one place, and bit-identity of two renders — outputs, instance count, the
per-pixel state the backward reads and every gradient."""
import ctypes as C

import torch

from parity_utils import PIPE

LEAVES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
OUT_KEYS = ("render", "acc_pixel_size", "depth", "radii", "pixel_sizes")
PLAIN = dict(filter_small=False, filter_large=False, fade_size=1.0)


def reset_forward_state():
    """forget everything the wrapper remembers about earlier forwards: the instance-count guesses (per key and per view shape,
    diff_gaussian_rasterization._instance_guess), the slab policy's publications and tags, and the heavy-queue hint.  After it
    the next forward of any key takes the first-call route (exact buffers)."""
    import diff_gaussian_rasterization as dgr
    dgr._last_instances.clear()
    dgr._instances_by_view.clear()
    dgr._fb_stats.clear()
    dgr._fb_tag_of.clear()
    dgr._fb_key_of.clear()
    dgr._occ_hot.clear()


def capacity(guess):
    """the instance capacity of the stage-2 buffers a guess buys"""
    import diff_gaussian_rasterization as dgr
    return dgr._capacity(guess)


def guesses_around(D):
    """(largest guess whose capacity is below D, smallest guess whose capacity is >= D): g + g // 8 skips values, so search"""
    lo, hi = 0, D
    assert capacity(lo) < D <= capacity(hi), D            # (D > 4096)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if capacity(mid) < D:
            lo = mid
        else:
            hi = mid
    return lo, hi


def non_speculative():
    import diff_gaussian_rasterization as dgr
    return dgr.forward_stats["non_speculative"]


def slab_stats(ctx):
    """the SlabHeader of the view's geom (msgs_slab_stats)"""
    import diff_gaussian_rasterization as dgr
    geom = dgr._resolve(ctx.state)[0]
    o = (C.c_int64 * 6)()
    dgr._C.check(dgr._C.lib.msgs_slab_stats(C.c_void_p(geom.data_ptr()), geom.numel(), ctx.call.P, o,
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "msgs_slab_stats")
    return dict(active=int(o[0]), rA=int(o[1]), DA=int(o[2]), n_open=int(o[3]), DB=int(o[4]), overflow=int(o[5]))


def per_pixel(image, W, H):
    """(final_T [N] f32, n_contrib [N] u32) of an image buffer: final_T at offset 0, n_contrib at the next 256-byte boundary
    (ImageLayout)"""
    n4 = 4 * W * H
    a = (n4 + 255) & ~255
    return image[:n4].clone(), image[a:a + n4].clone()


def result(out, pc, ctx, W, H):
    """(outputs, model, D, slab stats, per-pixel state) of a render; the last three are None without a backward graph"""
    import diff_gaussian_rasterization as dgr
    if ctx is None:
        return out, pc, None, None, None
    geom, binning, image, D = dgr._resolve(ctx.state)
    return out, pc, D, slab_stats(ctx), per_pixel(image, W, H)


def run(sc, cam, st, bg, dL, policy, backward=True, fused=False, calls=1, reset=True):
    """`calls` renders of the same view (after `reset`, the first sizes its stage-2 buffers exactly, the later ones take the
    speculative route on buffers sized from the previous count); returns result() of the LAST"""
    import diff_gaussian_rasterization as dgr
    from gaussian_renderer import render, render_fused
    from synthetic_model import SyntheticGaussians
    prev_slab, dgr.slab_policy = dgr.slab_policy, policy
    try:
        if reset:
            reset_forward_state()
        fn = render_fused if fused else render
        for _ in range(calls):
            pc = SyntheticGaussians(sc, "cuda", requires_grad=backward)
            if backward:
                out = fn(cam, pc, PIPE, bg, **st)
                out["render"].backward(dL)
            else:
                with torch.no_grad():
                    out = fn(cam, pc, PIPE, bg, **st)
        torch.cuda.synchronize()
        return result(out, pc, out["render"].grad_fn if backward else None, cam.image_width, cam.image_height)
    finally:
        dgr.slab_policy = prev_slab


def assert_identical(a, b, what, backward=True):
    (oa, pa, Da, _, ppa), (ob, pb, Db, _, ppb) = a, b
    for k in OUT_KEYS:
        assert torch.equal(oa[k], ob[k]), (what, k)
    if backward:
        assert Da == Db, (what, "instance count", Da, Db)
        assert torch.equal(ppa[0], ppb[0]), (what, "final_T")
        assert torch.equal(ppa[1], ppb[1]), (what, "n_contrib")
        assert torch.equal(oa["viewspace_points"].grad, ob["viewspace_points"].grad), (what, "means2D grad")
        for n in LEAVES:
            assert torch.equal(getattr(pa, n).grad, getattr(pb, n).grad), (what, n)

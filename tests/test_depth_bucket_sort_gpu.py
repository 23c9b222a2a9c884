"""The forward's depth sort on the bucket path (ms-gs_amd/csrc/sort.hip, depth_sort_buckets: fine histogram of the keys' depth
bins -> splitter -> one compacting bucket pass -> one workgroup per bucket in LDS) against the LSD passes it replaces.

Part 1 drives both through the test-only shim (tests/native/depth_sort_harness.hip) on the same raw inputs: keys, values and the
survivor count of the bucket path must EQUAL those of the LSD path and those of numpy's stable argsort of the surviving keys —
integers, no tolerance.  The sizes and contents are the smallest that reach each branch: one wave and its edges, one and several
rounds per thread of the LDS kernel, a size above its cap, all keys equal (no LDS pass at all), a bucket of exactly the cap, one
fine bin of cap + 1 keys (the chunked fall-back, flagged), the clamped end bins, dropped keys at the edges / everywhere / nowhere.
Every output has guard words, the scratch is dirty (0xA5) except in the pre-zeroed case.

Part 2 renders small scenes forward + backward with the process-wide switch on either side (msgs_set_depth_sort) and demands
bit-identical outputs, per-pixel state and gradients: reference and fused entry, occlusion cut-off off, depth slabs forced."""
import ctypes as C

import numpy as np
import pytest
import torch

import depth_sort_harness as D
import scenes
from route_utils import assert_identical, run as route_run
from sort_reference import DROPPED, compacted_reference

pytestmark = pytest.mark.gpu

GUARD = 64                      # words in front of and behind every output
SENT32, SENT8 = 0x5EEDBEEF, 0xA5
CONST = D.constants()
CAP = CONST.LDS_CAP
ONE_BIN = 0x40000000            # depth 2.0: the keys ONE_BIN + [0, 2^BIN_SHIFT) share one fine bin


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


class Out:
    def __init__(self, n):
        self.n = n
        self.t = torch.full((GUARD + max(n, 1) + GUARD,), SENT32, dtype=torch.int32, device="cuda")

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + 4 * GUARD)

    def data(self, count):
        return self.t[GUARD:GUARD + count].cpu().numpy().view(np.uint32)

    def guards_intact(self):
        s = SENT32
        return bool((self.t[:GUARD] == s).all()) and bool((self.t[GUARD + max(self.n, 1):] == s).all())


def sort(keys, buckets, pre_zeroed=False):
    """(rc, V, keys_out[:V], vals_out[:V], info words) of one path over the host array `keys`"""
    n = len(keys)
    kin = _i32(keys) if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    before = kin.clone()
    kout, vout, nv, info = Out(n), Out(n), Out(1), Out(2)
    scratch = torch.full((D.scratch(n).total,), SENT8, dtype=torch.uint8, device="cuda")
    if pre_zeroed:
        off, words = D.zero_region(n, scratch.data_ptr())
        scratch[off:off + 4 * words] = 0
    rc = D.lib().msgsd_sort(int(buckets), C.c_void_p(kin.data_ptr()), kout.ptr, vout.ptr, n, C.c_void_p(scratch.data_ptr()),
                            scratch.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream), int(pre_zeroed), nv.ptr,
                            info.ptr if buckets else None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    for o in (kout, vout, nv, info):
        assert o.guards_intact()
    assert torch.equal(kin, before), "the input keys were written"
    V = int(nv.data(1)[0])
    assert 0 <= V <= n
    return V, kout.data(V), vout.data(V), info.data(2)


def check(keys, pre_zeroed=False):
    """bucket path == LSD path == numpy; returns the bucket path's info words"""
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    eV, ek, ev = compacted_reference(keys, None, 0, 32) if len(keys) else (0, keys, keys)
    bV, bk, bv, info = sort(keys, True, pre_zeroed)
    lV, lk, lv, _ = sort(keys, False, pre_zeroed)
    largest_bin = int(np.bincount(D.depth_bin(keys[keys != DROPPED])).max()) if eV else 0
    print(f"[depth sort] n {len(keys)} V {eV} largest bin {largest_bin} info {info.tolist()}")
    assert bV == eV and lV == eV, (bV, lV, eV)
    for name, got, want in (("keys", bk, ek), ("values", bv, ev)):
        assert np.array_equal(got, want), f"bucket path vs numpy: {name} differ first at {int(np.argmax(got != want))}"
    assert np.array_equal(bk, lk) and np.array_equal(bv, lv), "bucket path vs LSD path"
    if len(keys):
        assert int(info[0]) == 1
        # the flag counts exactly the buckets the splitter makes larger than the cap
        hist = np.bincount(D.depth_bin(keys[keys != DROPPED]), minlength=CONST.BINS) if eV else np.zeros(CONST.BINS, np.int64)
        _, bases = D.splitter(hist)
        assert int(info[1]) == int((np.diff(bases) > CAP).sum()), (info, np.diff(bases).max())
    return info


def depths(n, rng, lo=0.25, hi=60.0):
    """positive-float keys: depths log-uniform in [lo, hi)"""
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n)).astype(np.float32).view(np.uint32)


@pytest.mark.parametrize("n", [1, 63, 65, 2049, 5000, CAP + 37])
def test_sizes(n):
    """random depths with 30 % of the keys dropped (at n = 1: the one key kept)"""
    rng = np.random.default_rng(n)
    keys = depths(n, rng)
    if n > 1:
        keys[rng.random(n) < 0.3] = DROPPED
    check(keys)


def test_empty_input():
    V, k, v, _ = sort(np.zeros(0, np.uint32), True)
    assert V == 0


@pytest.mark.parametrize("pre_zeroed", [False, True])
def test_random_keys_with_drops(pre_zeroed):
    """20 000 positive floats, 30 % dropped: many buckets of several rounds each; once on a scratch of which only the words of
    depth_sort_zero_region are clear"""
    rng = np.random.default_rng(7)
    keys = depths(20_000, rng)
    keys[rng.random(len(keys)) < 0.3] = DROPPED
    info = check(keys, pre_zeroed)
    assert int(info[1]) == 0


CONTENT = {
    "all-equal": lambda rng: np.full(5000, 0x40490FDB, np.uint32),
    "all-equal-above-cap": lambda rng: np.full(CAP + 1, 0x40490FDB, np.uint32),          # chunked, one identity pass
    "two-keys": lambda rng: np.where(rng.random(5000) < 0.5, 0x3F800000, 0x41200000).astype(np.uint32),
    "two-keys-lowest-bit": lambda rng: (0x40000000 + (rng.random(5000) < 0.5)).astype(np.uint32),
    "all-dropped": lambda rng: np.full(5000, DROPPED, np.uint32),
    "none-dropped": lambda rng: depths(5000, rng),
    "drops-at-both-ends": lambda rng: np.concatenate([[DROPPED], depths(4998, rng), [DROPPED]]).astype(np.uint32),
    "only-the-ends-kept": lambda rng: np.concatenate([[0x40000001], np.full(4998, DROPPED), [0x40000000]]).astype(np.uint32),
    # the clamped ends of the bin function: below depth 0.1875 (zero, denormals, small depths), the largest finite float, and
    # the keys above it up to the largest key that is kept
    "clamped-ends": lambda rng: rng.choice(np.array([0, 1, 0x00800000, 0x3E3FFFFF, 0x3E400000, 0x3E4CCCCD, 0x7F7FFFFE, 0x7F7FFFFF,
                                                     0x7F800000, 0x80000000, 0xFFFFFFFE, DROPPED], np.uint32), 5000),
    "bottom-bin-all-bits": lambda rng: rng.integers(0, 0x3E400000, 5000, dtype=np.uint64).astype(np.uint32),
    "top-bin-above-cap": lambda rng: rng.integers(0x7F7FFFFF, 0xFFFFFFFF, CAP + 808, dtype=np.uint64).astype(np.uint32),
    # one fine bin: its keys differ in the low BIN_SHIFT bits only and all land in one bucket
    "one-bin-exactly-cap": lambda rng: (ONE_BIN + rng.integers(0, 1 << CONST.BIN_SHIFT, CAP)).astype(np.uint32),
    "one-bin-cap-plus-1": lambda rng: (ONE_BIN + rng.integers(0, 1 << CONST.BIN_SHIFT, CAP + 1)).astype(np.uint32),
    "one-bin-three-chunks-with-drops": lambda rng: np.where(rng.random(3 * CAP + 5) < 0.2, DROPPED,
                                                            ONE_BIN + rng.integers(0, 1 << CONST.BIN_SHIFT, 3 * CAP + 5)).astype(np.uint32),
    "lowest-bit-only": lambda rng: (0x3FC00000 + 2 * (np.arange(5000) // 50) + (rng.random(5000) < 0.5)).astype(np.uint32),
}
ABOVE_CAP = {"all-equal-above-cap": 1, "top-bin-above-cap": 1, "one-bin-cap-plus-1": 1, "one-bin-three-chunks-with-drops": 1}


@pytest.mark.parametrize("name", list(CONTENT))
def test_contents(name):
    keys = CONTENT[name](np.random.default_rng(len(name)))
    info = check(keys)
    # the chunked fall-back ran exactly where a bucket outgrew the cap, and its flag says so
    assert int(info[1]) == ABOVE_CAP.get(name, 0), (name, info)


def test_a_large_bin_among_spread_keys():
    """one fine bin of nearly the cap among 10 000 spread keys: its bucket also takes the neighbouring bins' keys, so it ends at
    or above the cap as the splitter decides — check() asserts the flag against the numpy restatement of the splitter"""
    rng = np.random.default_rng(11)
    keys = np.concatenate([depths(10_000, rng), (ONE_BIN + rng.integers(0, 1 << CONST.BIN_SHIFT, CAP - 40)).astype(np.uint32)])
    rng.shuffle(keys)
    check(keys)


# ------------------------------------------------------------------------------------------------------------- end to end ---
def _render(sc, cam, st, bg, dL, mode, policy="never", fused=False, occlusion=True, calls=1):
    import diff_gaussian_rasterization as dgr
    lib = dgr._C.lib
    prev, prev_occ = lib.msgs_set_depth_sort(mode), lib.msgs_set_occlusion(1 if occlusion else 0)
    try:
        r = route_run(sc, cam, st, bg, dL, policy, fused=fused, calls=calls)
        ctx = r[0]["render"].grad_fn
        geom = dgr._resolve(ctx.state)[0]
        o = (C.c_int64 * 3)()
        dgr._C.check(lib.msgs_depth_sort_stats(C.c_void_p(geom.data_ptr()), geom.numel(), ctx.call.P, o,
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), "msgs_depth_sort_stats")
        return r, [int(v) for v in o]
    finally:
        lib.msgs_set_depth_sort(prev)
        lib.msgs_set_occlusion(prev_occ)


FILTERS = dict(filter_small=True, filter_large=True, fade_size=0.0)
E2E = {
    "128x128": dict(W=128, H=128, P=6000),
    "16x16-one-tile": dict(W=16, H=16, P=3000),
    "128x128-fused": dict(W=128, H=128, P=6000, fused=True),
    "128x128-occlusion-off": dict(W=128, H=128, P=6000, occlusion=False),
    "768x768-slabs-forced": dict(W=768, H=768, P=20_000, policy="0.15", calls=2, opaque=True),
}


@pytest.mark.parametrize("name", list(E2E))
def test_render_and_backward_are_bit_identical_across_the_switch(name):
    c = dict(E2E[name])
    W, H, P, opaque = c.pop("W"), c.pop("H"), c.pop("P"), c.pop("opaque", False)
    sc = scenes.frustum_scene(P, W, H, seed=31, multiscale=True, scale_k=0.004 * 1920.0 / W * 0.5)
    if opaque:
        sc.opacities[:, 0] = 0.55 + 0.44 * torch.rand(P, generator=torch.Generator().manual_seed(3))
    cam = scenes.front_camera(W, H).to("cuda")
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    dL = scenes.grad_seed(W, H, 31).cuda()
    lsd, s_lsd = _render(sc, cam, FILTERS, bg, dL, D.MODE_LSD, **c)
    bkt, s_bkt = _render(sc, cam, FILTERS, bg, dL, D.MODE_BUCKETS, **c)
    auto, s_auto = _render(sc, cam, FILTERS, bg, dL, D.MODE_AUTO, **c)
    print(f"[depth sort] {name}: D {lsd[2]} stats lsd {s_lsd} buckets {s_bkt} auto {s_auto} slab {bkt[3]}")
    assert s_lsd[0] == 0 and s_bkt[0] == 1 and s_bkt[1] == 0 and s_lsd[2] == s_bkt[2] > 0
    assert s_auto[0] == int(D.uses_buckets(P, D.MODE_AUTO))
    assert_identical(bkt, lsd, name)
    assert_identical(auto, lsd, name)
    assert bkt[3] == lsd[3]
    if "policy" in c:
        assert bkt[3]["active"] == 1, bkt[3]

"""adam_multi_kernel (ms-gs_amd/csrc/epilogue.hip) through msgs_adam_step: both kernel paths, chunk edges, neighbours.

A workgroup owns ADAM_CHUNK = 4096 consecutive floats of one tensor.  It streams them as float4 when the chunk is full
AND all four pointers of the tensor are 16-byte aligned, and walks them one float at a time otherwise.  torch
allocations are always aligned, so tensors of an optimizer never reach the second case on a full chunk; here the eight
tensors of one call (the ABI's maximum) are carved from one flat buffer at chosen float offsets, with canaries between.
Moments bit for bit against oracle.epilogue_oracle.adam_step, parameters to the rtol = atol = 2e-7 of
tests/test_epilogue_gpu.py (sqrt / divide roundings of ATen's CPU kernels, one ulp per step)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import epilogue_oracle as eo

pytestmark = pytest.mark.gpu

CHUNK = 4096
ROLES = ("param", "grad", "exp_avg", "exp_avg_sq")
# (length, role that is misaligned or None, by how many floats): every role is the odd one out once, every misalignment
# 1..3 occurs; aligned tensors have a lone ragged chunk (1), one full chunk (4096), a full chunk and a tail (4097), three
# full chunks (12 288); misaligned ones have full chunks only (8192), full chunks and a tail (8193), a ragged chunk (4095, 5)
LAYOUT = ((1, None, 0), (4095, "grad", 2), (4096, None, 0), (4097, None, 0), (8192, "exp_avg", 1), (8193, "param", 3),
          (12288, None, 0), (5, "exp_avg_sq", 1))
LRS = (1.6e-4, 2.5e-3, 2.5e-3 / 20, 0.05, 5e-3, 1e-3, 2e-2, 7e-4)           # all different: a slot mix-up shows
CANARY = 4                                                                   # floats between neighbours and at both ends


def _carve(layout):
    """float offsets {(k, role): start} inside one buffer and its length; every region is followed by >= CANARY floats"""
    at, cursor = {}, CANARY
    for k, (n, odd, mis) in enumerate(layout):
        for role in ROLES:
            start = (cursor + 3) // 4 * 4 + (mis if role == odd else 0)
            at[(k, role)] = start
            cursor = start + n + CANARY
    return at, (cursor + 3) // 4 * 4 + CANARY


def _run(layout, lrs, steps, seed, null_empty=()):
    from diff_gaussian_rasterization import _backend as _C
    gen = torch.Generator().manual_seed(seed)
    at, total = _carve(layout)
    host = -(torch.arange(total, dtype=torch.float32) + 1000.0)             # canary pattern: every float distinct
    owned = torch.zeros(total, dtype=torch.bool)
    state = []
    for k, (n, _, _) in enumerate(layout):
        p = torch.randn(n, generator=gen)
        state.append(dict(p=p.numpy().copy(), m=np.zeros(n, np.float32), v=np.zeros(n, np.float32)))
        for role, init in (("param", p), ("grad", torch.zeros(n)), ("exp_avg", torch.zeros(n)), ("exp_avg_sq", torch.zeros(n))):
            o = at[(k, role)]
            assert not owned[max(o - CANARY, 0): o + n + CANARY].any()      # regions and their canaries do not overlap
            host[o: o + n] = init
        for role in ROLES:
            owned[at[(k, role)]: at[(k, role)] + n] = True
    flat = host.cuda()
    assert flat.data_ptr() % 16 == 0
    arr = (_C.AdamTensor * len(layout))()
    for k, (n, odd, mis) in enumerate(layout):
        ptr = {role: flat.data_ptr() + 4 * at[(k, role)] for role in ROLES}
        for role in ROLES:
            assert ptr[role] % 16 == (4 * mis if role == odd else 0)
        if k in null_empty:
            assert n == 0
            ptr = dict.fromkeys(ROLES, None)
        arr[k] = _C.AdamTensor(ptr["param"], ptr["grad"], ptr["exp_avg"], ptr["exp_avg_sq"], n, lrs[k])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    grads = None
    for step in range(1, steps + 1):
        grads = [torch.randn(n, generator=gen) * (10.0 ** float(torch.randint(-7, 1, (1,), generator=gen)))
                 for n, _, _ in layout]
        for k, (n, _, _) in enumerate(layout):
            o = at[(k, "grad")]
            flat[o: o + n] = grads[k].cuda()
            s = state[k]
            eo.adam_step(s["p"], grads[k].numpy(), s["m"], s["v"], step, lrs[k])
        assert _C.lib.msgs_adam_step(arr, len(layout), step, 0.9, 0.999, 1e-15, stream) == 0
    torch.cuda.synchronize()
    got = flat.cpu()
    # the canaries, bit for bit: nothing outside the 4 x n floats of a tensor was written
    assert torch.equal(got[~owned].view(torch.int32), host[~owned].view(torch.int32))
    for k, (n, odd, mis) in enumerate(layout):
        tag = f"tensor {k}: n={n}, {odd} off by {mis}"
        cut = lambda role: got[at[(k, role)]: at[(k, role)] + n].numpy()
        np.testing.assert_array_equal(cut("grad"), grads[k].numpy(), err_msg=tag)          # read, never written
        np.testing.assert_array_equal(cut("exp_avg"), state[k]["m"], err_msg=tag)
        np.testing.assert_array_equal(cut("exp_avg_sq"), state[k]["v"], err_msg=tag)
        np.testing.assert_allclose(cut("param"), state[k]["p"], rtol=2e-7, atol=2e-7, err_msg=tag)
        if n:
            assert (cut("param") != host[at[(k, "param")]: at[(k, "param")] + n].numpy()).any(), tag   # it did step


def test_layout_reaches_both_paths_on_full_and_ragged_chunks():
    """what the kernel's branch `vec_ok && base + CHUNK <= n` sees for LAYOUT, restated (needs no GPU work)"""
    seen = set()
    for n, odd, _ in LAYOUT:
        for c in range((n + CHUNK - 1) // CHUNK):
            full = (c + 1) * CHUNK <= n
            seen.add(("aligned" if odd is None else "misaligned", "full" if full else "ragged"))
    assert seen == {("aligned", "full"), ("aligned", "ragged"), ("misaligned", "full"), ("misaligned", "ragged")}
    assert len(LAYOUT) == 8 and sorted(n for n, _, _ in LAYOUT) == [1, 5, 4095, 4096, 4097, 8192, 8193, 12288]
    assert {odd for _, odd, _ in LAYOUT} == {None, *ROLES} and {m for _, odd, m in LAYOUT if odd} == {1, 2, 3}
    at, total = _carve(LAYOUT)
    starts = sorted((o, LAYOUT[k][0]) for (k, _), o in at.items())
    assert starts[0][0] >= CANARY and total - (starts[-1][0] + starts[-1][1]) >= CANARY
    assert all(b[0] - (a[0] + a[1]) >= CANARY for a, b in zip(starts, starts[1:]))


def test_eight_carved_tensors_three_steps():
    _run(LAYOUT, LRS, steps=3, seed=2024)


def test_zero_length_tensors_among_others_are_a_no_op():
    """msgs_adam_step ACCEPTS n = 0 (with or without pointers): such a tensor owns no workgroup, and the tensors around
    it — first, in the middle, last — step exactly as they do without it."""
    layout = ((0, None, 0), (5, None, 0), (0, "param", 1), (4096, None, 0), (0, None, 0), (4097, "grad", 3), (1, None, 0),
              (0, None, 0))
    _run(layout, LRS, steps=3, seed=7, null_empty=(2, 7))

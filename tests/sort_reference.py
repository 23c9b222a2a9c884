"""Exact host references (numpy, integers only) for ms-gs_amd/csrc/sort.hip: the stable radix sort of (u32 key, u32 value)
pairs on a bit range, an O(n) checker of a sorted result for the sizes at which an argsort is too slow, and the exclusive scan
with its gather / mask / side-value variants."""
import numpy as np

DROPPED = 0xFFFFFFFF      # the key a compacting sort drops


def key_field(keys, begin_bit, end_bit):
    """the bits [begin_bit, end_bit) the sort orders by"""
    k = np.asarray(keys).astype(np.uint64)
    return ((k >> np.uint64(begin_bit)) & np.uint64((1 << (end_bit - begin_bit)) - 1)).astype(np.uint32)


def sort_reference(keys, vals, begin_bit, end_bit):
    """(keys_out, vals_out) of a stable sort by the key field; whole keys travel; vals None = the element index"""
    keys = np.asarray(keys)
    n = keys.shape[0]
    vals = np.arange(n, dtype=np.uint32) if vals is None else np.asarray(vals)
    perm = np.argsort(key_field(keys, begin_bit, end_bit), kind="stable")
    return keys[perm], vals[perm]


def compacted_reference(keys, vals, begin_bit, end_bit):
    """a compacting sort: the stable sort of the pairs whose key is not DROPPED -> (V, keys_out[:V], vals_out[:V])"""
    keys = np.asarray(keys)
    n = keys.shape[0]
    vals = np.arange(n, dtype=np.uint32) if vals is None else np.asarray(vals)
    keep = keys != np.asarray(DROPPED, dtype=keys.dtype)
    k, v = sort_reference(keys[keep], vals[keep], begin_bit, end_bit)
    return int(keep.sum()), k, v


def check_sorted(keys_in, vals_in, keys_out, vals_out, begin_bit, end_bit):
    """O(n) check that (keys_out, vals_out) is THE stable sort of (keys_in, vals_in) by the key field.  vals_in: None (the
    element index) or a permutation of 0 .. n-1 (distinct values: each names its source position).  Returns None when the
    result is right, else a string saying which property fails.  The four properties together admit exactly one result:
      1. the key field is non-decreasing;
      2. vals_out is a permutation of the input values;
      3. every key still sits beside its value: keys_in[source of vals_out[i]] == keys_out[i];
      4. inside every run of equal key field the source positions increase (stability)."""
    keys_in, keys_out, vals_out = np.asarray(keys_in), np.asarray(keys_out), np.asarray(vals_out)
    n = keys_in.shape[0]
    if keys_out.shape[0] != n or vals_out.shape[0] != n:
        return f"length: {keys_out.shape[0]} keys and {vals_out.shape[0]} values for {n} pairs"
    if n == 0:
        return None
    f = key_field(keys_out, begin_bit, end_bit)
    up = f[1:] >= f[:-1]
    if not up.all():
        i = int(np.argmin(up))
        return f"order: key field {int(f[i])} at {i} is followed by {int(f[i + 1])}"
    if int(vals_out.max()) >= n:
        return f"values: {int(vals_out.max())} is not an input value"
    counts = np.bincount(vals_out, minlength=n)
    if not (counts == 1).all():
        v = int(np.argmax(counts != 1))
        return f"values: {v} occurs {int(counts[v])} times"
    if vals_in is None:
        src = vals_out
    else:
        vals_in = np.asarray(vals_in)
        inv = np.empty(n, dtype=np.int64)
        inv[vals_in] = np.arange(n, dtype=np.int64)
        src = inv[vals_out]
    together = keys_in[src] == keys_out
    if not together.all():
        i = int(np.argmin(together))
        return f"pairing: output {i} holds key {int(keys_out[i])} beside the value of key {int(keys_in[src[i]])}"
    src = src.astype(np.int64)
    stable = (src[1:] > src[:-1]) | (f[1:] != f[:-1])
    if not stable.all():
        i = int(np.argmin(stable))
        return f"stability: equal key fields at {i} and {i + 1} come from positions {int(src[i])} and {int(src[i + 1])}"
    return None


def scan_reference(inp, n, gather=None, in_mask=0xFFFFFFFF, side_shift=None):
    """exclusive scan of x[i] = inp[gather[i] if gather is given else i] & in_mask over i < n.
    -> (out: u32 prefixes mod 2^32, total: exact python int, side: u32 inp[gather[i]] >> side_shift, or None)"""
    inp = np.asarray(inp).astype(np.uint64)
    raw = inp[np.asarray(gather)[:n].astype(np.int64)] if gather is not None else inp[:n]
    x = raw & np.uint64(in_mask)
    inc = np.cumsum(x, dtype=np.uint64)             # exact: n < 2^32 values below 2^32
    out = np.zeros(n, dtype=np.uint64)
    out[1:] = inc[:-1]
    total = int(inc[-1]) if n > 0 else 0
    side = (raw >> np.uint64(side_shift)).astype(np.uint32) if side_shift is not None else None
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32), total, side

"""ms-gs_amd/csrc/sort.hip called directly — radix_sort_pairs, exclusive_scan_u32, launch_zero — through the test-only harness
library (tests/native/sort_harness.hip, tests/sort_harness.py), every result compared EXACTLY with the numpy references of
tests/sort_reference.py.  Integer work throughout: no tolerances.

The code paths of the sort are chosen by size (4 / 8 / 16 keys per thread, the scanned route with group_scan_kernel from
SORT_SCANNED_MIN_BLOCKS blocks) and by argument (compaction, a device-side count, 16-bit keys, pre-zeroed scratch, the bit
range and with it the number of passes and the ping-pong parity).  The sizes at which the paths change are DERIVED from the
library's geometry query (sort_harness.thresholds), never written down here; tests/test_sort_reference_cpu.py asserts that the
derived sizes cover all four regimes.  The regime of every parametrised size is part of its test id (pytest -v lists them), and
every test prints its geometry (items, scanned, blocks, groups: shown with -s or -rP).

Every output buffer has guard words in front and behind that must keep their sentinel; the sort's scratch is filled with 0xA5
bytes before every call (production scratch is never clean); inputs stay on the host (a multi-pass sort clobbers its inputs).
Results of up to ARGSORT_MAX pairs are compared with the stable argsort, larger ones go through the O(n) checker, which admits
exactly the same single result.  The shim refuses a device-side count above n before launching, so no case can write out of
range."""
import ctypes as C

import numpy as np
import pytest
import torch

import sort_harness as H
from sort_reference import DROPPED, check_sorted, compacted_reference, scan_reference, sort_reference

pytestmark = pytest.mark.gpu

GUARD_BYTES = 256               # in front of and behind every output: the data keeps the 256-byte alignment of production buffers
SENT32, SENT16, SENT8 = 0x5EEDBEEF, 0x5EED, 0xA5
SENT64 = 0x5EEDBEEF5EEDBEEF
FILLER = 0x77777777             # input words behind a device-side count: never read
ARGSORT_MAX = 300_000
FULL = 0xFFFFFFFF

CONST = H.constants()
THRESHOLDS = H.thresholds()
REGIME_N = H.regime_sizes()                     # one ragged size per regime
REGIMES = list(H.REGIMES)
_SENT = {torch.int32: SENT32, torch.int16: SENT16, torch.uint8: SENT8, torch.int64: SENT64}
_NP = {torch.int32: np.uint32, torch.int16: np.uint16, torch.uint8: np.uint8, torch.int64: np.uint64}
_NPS = {torch.int32: np.int32, torch.int16: np.int16, torch.uint8: np.uint8, torch.int64: np.int64}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype):
    """a numpy array of unsigned words as a device tensor of the signed torch type of the same width"""
    return torch.from_numpy(np.ascontiguousarray(a).view(_NPS[dtype])).cuda()


class Guarded:
    """n elements on the device between two guard regions, everything filled with a sentinel; `offset` elements of extra
    distance from the front guard move the data off its 256-byte alignment"""

    def __init__(self, n, dtype=torch.int32, offset=0):
        self.n, self.dtype, self.size = int(n), dtype, torch.empty((), dtype=dtype).element_size()
        self.g = GUARD_BYTES // self.size + offset
        self.t = torch.full((self.g + self.n + GUARD_BYTES // self.size,), _SENT[dtype], dtype=dtype, device="cuda")
        assert self.t.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + self.g * self.size)

    def load(self, a):
        self.t[self.g:self.g + len(a)] = _dev(a, self.dtype)
        return self

    def data(self, count=None):
        count = self.n if count is None else count
        return self.t[self.g:self.g + count].cpu().numpy().view(_NP[self.dtype])

    def guards_intact(self):
        s = _SENT[self.dtype]
        return bool((self.t[:self.g] == s).all()) and bool((self.t[self.g + self.n:] == s).all())

    def untouched(self, start=0):
        return bool((self.t[self.g + start:self.g + self.n] == _SENT[self.dtype]).all())


def _log(what, n):
    g = H.geom(n)
    print(f"[sort] {what}: n {n} -> {H.regime(n)} (items {g.items}, scanned {g.scanned}, nb {g.nb}, gsize {g.gsize}, "
          f"ngroups {g.ngroups})")
    return g


# ======================================================================================================================= sort ===
class SortRun:
    def __init__(self, rc, kout, vout, n_valid):
        self.rc, self.kout, self.vout, self.n_valid = rc, kout, vout, n_valid

    def assert_guards(self):
        assert self.kout.guards_intact(), "keys_out: a guard word was written"
        assert self.vout.guards_intact(), "vals_out: a guard word was written"
        assert self.n_valid is None or self.n_valid.guards_intact(), "n_valid_dev: a guard word was written"

    def valid(self):
        return int(self.n_valid.data()[0])


def new_scratch(n):
    return torch.full((H.geom(n).scratch_bytes,), SENT8, dtype=torch.uint8, device="cuda")


def run_sort(keys, vals, bits, *, cap=None, n_dev=None, compact=False, keys16=False, pre_zeroed=False, scratch=None):
    """radix_sort_pairs over the host arrays `keys` (uint32, or uint16 with keys16) and `vals` (uint32 or None).  cap: the n the
    sort is called with when it is more than len(keys) (device-side count); the rest of the inputs is FILLER."""
    n = len(keys) if cap is None else cap
    kdt = torch.int16 if keys16 else torch.int32
    assert keys.dtype == (np.uint16 if keys16 else np.uint32) and len(keys) <= n
    kin = torch.full((max(n, 1),), FILLER & (0xFFFF if keys16 else FULL), dtype=kdt, device="cuda")
    kin[:len(keys)] = _dev(keys, kdt)
    vin = None
    if vals is not None:
        assert vals.dtype == np.uint32 and len(vals) == len(keys)
        vin = torch.full((max(n, 1),), FILLER, dtype=torch.int32, device="cuda")
        vin[:len(vals)] = _dev(vals, torch.int32)
    assert kin.data_ptr() % 256 == 0
    kout, vout = Guarded(n, kdt), Guarded(n, torch.int32)
    if scratch is None:
        scratch = new_scratch(n)
    if pre_zeroed:      # only the words radix_sort_zero_region names are cleared; everything else stays dirty
        off, words = H.zero_region(n, *bits, scratch_ptr=scratch.data_ptr())
        scratch[off:off + 4 * words] = 0
    nv = Guarded(1) if compact else None
    nd = torch.tensor([n_dev], dtype=torch.int32, device="cuda") if n_dev is not None else None
    rc = H.lib().msgst_sort_pairs(C.c_void_p(kin.data_ptr()), C.c_void_p(vin.data_ptr()) if vin is not None else None,
                                  kout.ptr, vout.ptr, n, bits[0], bits[1], C.c_void_p(scratch.data_ptr()), scratch.numel(),
                                  _stream(), int(pre_zeroed), nv.ptr if nv else None,
                                  C.c_void_p(nd.data_ptr()) if nd is not None else None, int(keys16))
    torch.cuda.synchronize()
    return SortRun(rc, kout, vout, nv)


def verify_sorted(keys, vals, bits, run, count=None, argsort=False):
    """the first `count` outputs (all of them by default) are the stable sort of (keys, vals); the guards are intact"""
    count = len(keys) if count is None else count
    assert run.rc == 0, run.rc
    ko, vo = run.kout.data(count), run.vout.data(count)
    if argsort or count <= ARGSORT_MAX:
        ek, ev = sort_reference(keys, vals, *bits)
        assert np.array_equal(ko, ek), f"keys differ first at {int(np.argmax(ko != ek))}"
        assert np.array_equal(vo, ev), f"values differ first at {int(np.argmax(vo != ev))}"
    else:
        why = check_sorted(keys, vals, ko, vo, *bits)
        assert why is None, why
    run.assert_guards()


def uniform(n, rng, below=1 << 32):
    return rng.integers(0, below, n, dtype=np.uint64).astype(np.uint32)


def perm(n, rng):
    return rng.permutation(n).astype(np.uint32)


# --------------------------------------------------------------------------------------------------------------------- sizes ---
SIZES = [(n, "fixed") for n in (1, 63, 64, 65, 255, 256, 257)] + \
        [(H.chunk(1) + d, f"chunk{d:+d}") for d in (-1, 0, 1)] + H.group_sizes() + H.boundary_sizes()


@pytest.mark.parametrize("n,what", SIZES, ids=[f"{n}-{w}-{H.regime(n)}" for n, w in SIZES])
def test_sizes(n, what):
    """every size at which the launch geometry changes, on keys with about four copies of every value spread over all 32 bits
    (ties in every pass), identity values on even sizes and a permutation on odd ones"""
    _log(f"sizes {what}", n)
    rng = np.random.default_rng(n)
    keys = (rng.integers(0, max(2, n // 4), n, dtype=np.uint64) * 2654435761 & FULL).astype(np.uint32)
    vals = perm(n, rng) if n % 2 else None
    verify_sorted(keys, vals, (0, 32), run_sort(keys, vals, (0, 32)))


# ------------------------------------------------------------------------------------------------------------------ patterns ---
def _steps(n, copies):
    """non-decreasing keys over the whole 32-bit range, `copies` of each"""
    distinct = n // copies + 1
    return (np.arange(n, dtype=np.uint64) // copies * (FULL // distinct)).astype(np.uint32)


def _single(n, at, other):
    keys = np.full(n, 0x40302010, dtype=np.uint32)
    keys[at] = other
    return keys


PATTERNS = {
    "uniform": lambda n, rng: (uniform(n, rng), (0, 32)),
    "all_equal": lambda n, rng: (np.full(n, 0x9E3779B9, dtype=np.uint32), (0, 32)),
    "two_values_top_digit": lambda n, rng: ((uniform(n, rng, 2) << np.uint32(31)) | np.uint32(0x00ABCDEF), (0, 32)),
    "two_values_bottom_digit": lambda n, rng: (uniform(n, rng, 2) | np.uint32(0xABCDEF00), (0, 32)),
    "sorted": lambda n, rng: (_steps(n, 3), (0, 32)),
    "reversed": lambda n, rng: (_steps(n, 3)[::-1].copy(), (0, 32)),
    # the 64 keys a wave ranks together are identical (every lane a peer of every other, lane 63 the last), waves differ
    "wave_constant": lambda n, rng: ((np.arange(n, dtype=np.uint64) // 64 * 2654435761 & FULL).astype(np.uint32), (0, 32)),
    # a block's keys fall into ONE digit in every pass, and neighbouring blocks into different ones
    "block_digit": lambda n, rng: ((np.arange(n, dtype=np.uint64) // H.chunk(n) % 256 * 0x01010101).astype(np.uint32), (0, 32)),
    "tile_ids_13bit": lambda n, rng: (uniform(n, rng, 1 << 13), (0, 13)),
    "single_larger_at_0": lambda n, rng: (_single(n, 0, 0xF0302010), (0, 32)),
    "single_smaller_at_end": lambda n, rng: (_single(n, n - 1, 0x40302000), (0, 32)),
}


@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("regime", REGIMES)
def test_key_patterns(regime, pattern):
    n = REGIME_N[regime]
    _log(f"pattern {pattern}", n)
    keys, bits = PATTERNS[pattern](n, np.random.default_rng(len(pattern)))
    assert keys.dtype == np.uint32 and len(keys) == n
    verify_sorted(keys, None, bits, run_sort(keys, None, bits))


# ---------------------------------------------------------------------------------------------------------------- bit ranges ---
BIT_RANGES = [(0, 32), (0, 31), (0, 8), (0, 1), (0, 9), (0, 13), (0, 16), (0, 17), (3, 16), (5, 32), (24, 32)]


# every range in the three unscanned regimes; on the scanned route the 3-pass range (the other ping-pong parity together with
# gsum_is_base), its 1-, 2- and 4-pass sorts being those of test_pre_zeroed_scratch
RANGE_CASES = [(r, b) for r in REGIMES[:3] for b in BIT_RANGES] + [("items16-scanned", (0, 17))]


@pytest.mark.parametrize("regime,bits", RANGE_CASES, ids=[f"{r}-bits{b[0]}-{b[1]}" for r, b in RANGE_CASES])
def test_bit_ranges(regime, bits):
    """1 to 4 passes, both ping-pong parities, digit masks under 8 bits, a non-zero begin_bit; all 32 key bits are random, so
    the bits outside the range must travel with the pair and must not influence the order"""
    n = REGIME_N[regime]
    _log(f"bits {bits}", n)
    rng = np.random.default_rng(bits[0] * 40 + bits[1])
    keys, vals = uniform(n, rng), perm(n, rng)
    verify_sorted(keys, vals, bits, run_sort(keys, vals, bits))


# -------------------------------------------------------------------------------------------------------------------- values ---
@pytest.mark.parametrize("bits", [(0, 32), (0, 13)], ids=lambda b: f"bits{b[0]}-{b[1]}")
@pytest.mark.parametrize("regime", REGIMES[:3])
def test_values_with_repeats(regime, bits):
    """values need not be distinct: compared with the argsort result at every size (the checker needs distinct values)"""
    n = REGIME_N[regime]
    _log(f"repeated values {bits}", n)
    rng = np.random.default_rng(n + bits[1])
    keys, vals = uniform(n, rng), uniform(n, rng, 1000)
    verify_sorted(keys, vals, bits, run_sort(keys, vals, bits), argsort=True)


# ---------------------------------------------------------------------------------------------------------------- compaction ---
def _drop_mask(n, fraction, placement, rng):
    chunk = H.chunk(n)
    if fraction == "none":
        return np.zeros(n, dtype=bool)
    if fraction == "all":
        return np.ones(n, dtype=bool)
    if fraction == "all_but_one":
        m = np.ones(n, dtype=bool)
        m[{"scattered": n // 3, "front": n - 1, "back": 0}[placement]] = False
        return m
    share = {"1%": 0.01, "50%": 0.5}[fraction]
    if placement == "scattered":
        return rng.random(n) < share
    whole = max(1, int(n * share) // chunk) * chunk             # whole blocks of dropped keys
    m = np.zeros(n, dtype=bool)
    if placement == "front":
        m[:whole] = True
    else:
        m[(n - whole) // chunk * chunk:] = True                 # from a block edge to the end
    return m


COMPACTION = [(r, f, "scattered") for r in REGIMES[:3] for f in ("none", "1%", "50%", "all_but_one", "all")] + \
             [(r, f, p) for r in REGIMES[:3] for f in ("1%", "50%") for p in ("front", "back")] + \
             [("items16-scanned", "50%", "scattered"), ("items16-scanned", "50%", "front"), ("items16-scanned", "all", "scattered")]


@pytest.mark.parametrize("regime,fraction,placement", COMPACTION, ids=["-".join(c) for c in COMPACTION])
def test_compaction(regime, fraction, placement):
    """n_valid_dev: keys equal to 0xFFFFFFFF leave the sort in the first pass and the later passes take their count from the
    device word.  Below the scanned threshold *n_valid_dev == V and the first V outputs are the stable sort of the survivors
    (the tail is unspecified); on the scanned route *n_valid_dev == n and all n pairs are sorted, the dropped keys last."""
    n = REGIME_N[regime]
    g = _log(f"compaction {fraction} {placement}", n)
    rng = np.random.default_rng(n % 1000 + len(fraction) + len(placement))
    keys = uniform(n, rng, FULL)                                # (below 0xFFFFFFFF)
    keys[_drop_mask(n, fraction, placement, rng)] = DROPPED
    run = run_sort(keys, None, (0, 32), compact=True)
    assert run.rc == 0
    if g.scanned:
        assert run.valid() == n
        verify_sorted(keys, None, (0, 32), run)
        V = int((keys != DROPPED).sum())
        assert (run.kout.data()[V:] == DROPPED).all()
    else:
        V, ek, ev = compacted_reference(keys, None, 0, 32)
        assert run.valid() == V, (run.valid(), V)
        assert np.array_equal(run.kout.data(V), ek) and np.array_equal(run.vout.data(V), ev)
        run.assert_guards()


# --------------------------------------------------------------------------------------------------------- device-side count ---
def _counts(cap):
    chunk = H.chunk(cap)
    third = cap // 3
    if third % chunk == 0:
        third += 7
    return {"0": 0, "1": 1, "chunk-1": chunk - 1, "chunk": chunk, "chunk+1": chunk + 1, "third": third, "cap-1": cap - 1, "cap": cap}


@pytest.mark.parametrize("count", ["0", "1", "chunk-1", "chunk", "chunk+1", "third", "cap-1", "cap"])
@pytest.mark.parametrize("regime", REGIMES)
def test_device_side_count(regime, count):
    """n_dev: the grids and the group geometry are those of the capacity, surplus blocks leave at once, group_scan_kernel
    recomputes its block and group counts from the device word.  Only the first n_dev outputs are specified; with a count of
    0 nothing is written."""
    cap = REGIME_N[regime]
    c = _counts(cap)[count]
    _log(f"device count {count} = {c} of capacity", cap)
    assert H.supports_device_count(cap, 0, 32)
    rng = np.random.default_rng(c % 1009)
    keys = uniform(c, rng)
    vals = perm(c, rng) if c % 2 else None
    run = run_sort(keys, vals, (0, 32), cap=cap, n_dev=c)
    verify_sorted(keys, vals, (0, 32), run, count=c)
    if c == 0:
        assert run.kout.untouched() and run.vout.untouched()


# -------------------------------------------------------------------------------------------------------------- 16-bit keys ---
def _keys16_sizes():
    """per regime a size of full chunks only and a ragged one"""
    out = {}
    for r in REGIMES:
        n = REGIME_N[r]
        full = -(-n // H.chunk(n)) * H.chunk(n)
        if H.regime(full) != r:
            full = n // H.chunk(n) * H.chunk(n)
        assert H.regime(full) == r and full % H.chunk(full) == 0 and n % H.chunk(n) != 0, (r, n, full)
        out[r] = {"full": full, "ragged": n}
    return out


KEYS16_N = _keys16_sizes()
KEYS16 = [(r, s, b, d) for r in REGIMES[:3] for s in ("full", "ragged") for b in ((0, 13), (0, 16)) for d in (False, True)] + \
         [("items16-scanned", "ragged", (0, 13), False), ("items16-scanned", "full", (0, 16), True)]


@pytest.mark.parametrize("regime,shape,bits,device_count", KEYS16,
                         ids=[f"{r}-{s}-bits{b[1]}-{'ndev' if d else 'n'}" for r, s, b, d in KEYS16])
def test_keys16(regime, shape, bits, device_count):
    """uint16 key arrays (the tile sort): the vectorised histogram needs full chunks and 8 | ITEMS, so 4 keys per thread and
    every ragged last chunk take the scalar path.  Tile ids with the sentinel 0xFFFF among them."""
    n = KEYS16_N[regime][shape]
    _log(f"keys16 {shape} {bits} device_count={device_count}", n)
    assert H.keys16_ok(n, *bits)
    rng = np.random.default_rng(n % 1013 + bits[1])
    keys = rng.integers(0, 1 << 13 if bits[1] == 13 else 1 << 16, n, dtype=np.uint64).astype(np.uint16)
    keys[rng.random(n) < 0.02] = 0xFFFF
    keys[n - 1] = 0xFFFF
    vals = perm(n, rng)
    if device_count:        # a count that ends inside a chunk, on a grid sized for n
        c = n - H.chunk(n) - 5 if n > 2 * H.chunk(n) else n - 5
        keys, vals = keys[:c], perm(c, rng)
        run = run_sort(keys, vals, bits, cap=n, n_dev=c, keys16=True)
        verify_sorted(keys, vals, bits, run, count=c)
    else:
        verify_sorted(keys, vals, bits, run_sort(keys, vals, bits, keys16=True))


def test_keys16_needs_an_end_bit_of_at_most_16():
    for n in REGIME_N.values():
        assert H.keys16_ok(n, 0, 16) and H.keys16_ok(n, 3, 16) and not H.keys16_ok(n, 0, 17) and not H.keys16_ok(n, 16, 32)
    keys = np.arange(100, dtype=np.uint16)
    run = run_sort(keys, None, (0, 17), keys16=True)
    assert run.rc == H.REFUSED_KEYS16 and run.kout.untouched() and run.vout.untouched()


# ---------------------------------------------------------------------------------------------------------- pre-zeroed scratch ---
@pytest.mark.parametrize("bits", [(0, 8), (0, 13), (0, 32)], ids=["1pass", "2passes", "4passes"])
@pytest.mark.parametrize("regime", REGIMES)
def test_pre_zeroed_scratch(regime, bits):
    """pre_zeroed = true on a scratch of 0xA5 bytes in which ONLY the region radix_sort_zero_region names was cleared: a word the
    sort needs zero and the query does not name, or names in the wrong place, stays dirty"""
    n = REGIME_N[regime]
    _log(f"pre-zeroed {bits}", n)
    rng = np.random.default_rng(bits[1])
    keys = uniform(n, rng)
    verify_sorted(keys, None, bits, run_sort(keys, None, bits, pre_zeroed=True))


def test_two_sorts_back_to_back_on_one_scratch():
    """pre_zeroed = false clears what the sort needs itself, whatever the previous sort of another size and pass count left"""
    big, small = REGIME_N["items16"], REGIME_N["items4"]
    scratch = new_scratch(big)
    rng = np.random.default_rng(3)
    for n, bits in ((big, (0, 32)), (small, (0, 13)), (big, (0, 13)), (small, (0, 32)), (REGIME_N["items8"], (0, 17))):
        _log(f"back to back {bits}", n)
        keys = uniform(n, rng)
        verify_sorted(keys, None, bits, run_sort(keys, None, bits, scratch=scratch))


# ------------------------------------------------------------------------------------------------------------ argument edges ---
def test_n_zero_and_refused_arguments():
    none = np.zeros(0, dtype=np.uint32)
    run = run_sort(none, None, (0, 32), compact=True)
    assert run.rc == 0 and run.valid() == 0
    assert run.kout.guards_intact() and run.vout.guards_intact() and run.n_valid.guards_intact()
    # (more than four passes cannot be asked for with 32 key bits)
    assert H.supports_device_count(1000, 0, 32)
    keys = np.arange(2000, dtype=np.uint32)
    run = run_sort(keys[:1000], None, (0, 32), cap=1000, n_dev=1001)
    assert run.rc == H.REFUSED_COUNT and run.kout.untouched() and run.vout.untouched()
    run = run_sort(keys, None, (0, 32), n_dev=5, compact=True)
    assert run.rc == H.REFUSED_BOTH_COUNTS and run.kout.untouched() and run.vout.untouched() and run.valid() == SENT32
    run = run_sort(keys, None, (0, 32), scratch=new_scratch(1000))
    assert run.rc == H.REFUSED_SCRATCH and run.kout.untouched()


# ======================================================================================================================= scan ===
TICKET = 0x0123456789AB
EXTRA = (0xCAFE0001, 0x8BADF00D)
SCAN_BIG = CONST.SCAN_THREADS * CONST.SCAN_CHUNK + 2 * CONST.SCAN_CHUNK + 7     # > SCAN_THREADS blocks, not a multiple of 16
SCAN_LENGTHS = [0, 1, 15, 16, 17, CONST.SCAN_CHUNK - 1, CONST.SCAN_CHUNK, CONST.SCAN_CHUNK + 1, SCAN_BIG]
assert H.scan_blocks(SCAN_BIG) > CONST.SCAN_THREADS and SCAN_BIG % 16


def scan_values(kind, m, rng):
    if kind == "small":
        return uniform(m, rng, 1000)
    if kind == "near_2^31":         # a handful of values pass 2^32 already
        return (np.uint32(0x7FFFFF00) + uniform(m, rng, 0x200)).astype(np.uint32)
    if kind == "zero_blocks":       # whole chunks of zeros between chunks of values: per-block sums that are exactly 0
        v = uniform(m, rng, 50)
        v[(np.arange(m) // CONST.SCAN_CHUNK) % 2 == 0] = 0
        return v
    raise ValueError(kind)


def run_scan(inp, n, *, gather=None, in_mask=FULL, side=False, side_flag=True, n_ptr=None, in_off=0, out_off=0, in_place=False,
             clamp=0, alias_gather_out=False):
    """exclusive_scan_u32 with every optional output given -> dict of what came back (numpy / ints) and the buffers"""
    bin_ = Guarded(len(inp), offset=in_off).load(inp)
    bout = bin_ if in_place or alias_gather_out else Guarded(n, offset=out_off)
    bg = _dev(gather, torch.int32) if gather is not None else None
    bside = Guarded(n) if side else None
    partials = Guarded(H.scan_blocks(max(n, 1)) + 2, torch.int64)
    total, status = Guarded(1, torch.int64), Guarded(3, torch.int64)
    clamped, zero_word, overflow, flag = Guarded(1), Guarded(1), Guarded(1), Guarded(1)
    extra = _dev(np.array(EXTRA, dtype=np.uint32), torch.int32)
    nptr = torch.tensor([n_ptr], dtype=torch.int32, device="cuda") if n_ptr is not None else None
    host = (C.c_uint64 * 4)()
    rc = H.lib().msgst_scan(bin_.ptr, C.c_void_p(bg.data_ptr()) if bg is not None else None, bout.ptr, n, partials.ptr, total.ptr,
                            _stream(), status.ptr, 1, TICKET, SENT64, host, C.c_void_p(nptr.data_ptr()) if nptr is not None else None,
                            clamped.ptr, clamp, C.c_void_p(extra.data_ptr()), zero_word.ptr, overflow.ptr, in_mask,
                            bside.ptr if side else None, flag.ptr if side_flag else None)
    torch.cuda.synchronize()
    bufs = [bin_, bout, partials, total, status, clamped, zero_word, overflow, flag] + ([bside] if side else [])
    return dict(rc=rc, inp=bin_, out=bout, side=bside, total=int(total.data()[0]), status=[int(x) for x in status.data()],
                host=[int(x) for x in host], clamped=int(clamped.data()[0]), zero_word=int(zero_word.data()[0]),
                overflow=int(overflow.data()[0]), flag=int(flag.data()[0]), bufs=bufs)


def verify_scan(r, inp, n, *, gather=None, in_mask=FULL, side=False, side_flag=True, n_ptr=None, clamp=0):
    m = n if n_ptr is None else n_ptr
    m = max(m, 0)
    eo, esum, eside = scan_reference(inp, m, gather, in_mask, CONST.TILE_COUNT_BITS if side else None)
    info = EXTRA[0] | EXTRA[1] << 32
    assert r["rc"] == 0, r["rc"]
    got = r["out"].data(m)
    assert np.array_equal(got, eo), f"prefixes differ first at {int(np.argmax(got != eo))} of {m}"
    if r["out"] is not r["inp"]:
        assert r["out"].untouched(m), "an output at or behind the element count was written"
    assert r["total"] == esum, (r["total"], esum)
    assert r["status"] == [esum, 0, info], r["status"]
    assert r["host"] == [esum, 0, TICKET, info], r["host"]
    assert r["zero_word"] == 0
    assert r["clamped"] == min(esum, clamp), (r["clamped"], esum, clamp)
    assert r["overflow"] == (1 if esum > clamp else SENT32), (r["overflow"], esum, clamp)
    if side:
        assert np.array_equal(r["side"].data(m), eside) and r["side"].untouched(m)
    if side_flag and n > 0:
        assert r["flag"] == (1 if side else 0)
    else:
        assert r["flag"] == SENT32                  # (the n <= 0 launch has no reduce pass: the flag is not part of it)
    for b in r["bufs"]:
        assert b.guards_intact()
    return esum


@pytest.mark.parametrize("clamp_kind", ["above", "equal", "below"])
@pytest.mark.parametrize("kind", ["small", "near_2^31", "zero_blocks"])
@pytest.mark.parametrize("n", SCAN_LENGTHS)
def test_scan(n, kind, clamp_kind):
    """out, the exact u64 total beside prefixes that wrap mod 2^32, the status and host words, zero_word, the clamped total and
    the overflow flag (set above the clamp, left alone otherwise).  With values near 2^31 ONE block's sum passes 2^32 from 15
    values on: the block totals scan_reduce_kernel leaves have to be 64-bit for the grand total to be exact."""
    rng = np.random.default_rng(n % 1000 + len(kind))
    inp = scan_values(kind, n, rng)
    esum = scan_reference(inp, n)[1]
    if kind == "near_2^31" and n >= 15:
        assert esum > 1 << 32
    clamp = {"above": min(esum + 10, FULL), "equal": min(esum, FULL), "below": min(esum // 2, FULL)}[clamp_kind]
    verify_scan(run_scan(inp, n, clamp=clamp), inp, n, clamp=clamp)


@pytest.mark.parametrize("where", ["in", "out", "both"])
@pytest.mark.parametrize("n", [17, CONST.SCAN_CHUNK + 1, SCAN_BIG])
def test_scan_off_the_16_byte_alignment(n, where):
    """`in` / `out` 4 bytes behind a 16-byte boundary: scan_load_items / scan_store_items take their scalar paths"""
    inp = scan_values("near_2^31", n, np.random.default_rng(n))
    r = run_scan(inp, n, in_off=int(where != "out"), out_off=int(where != "in"), clamp=5)
    assert (r["inp"].ptr.value % 16 == 4) == (where != "out") and (r["out"].ptr.value % 16 == 4) == (where != "in")
    verify_scan(r, inp, n, clamp=5)


@pytest.mark.parametrize("n", [17, CONST.SCAN_CHUNK + 1, SCAN_BIG])
def test_scan_in_place(n):
    inp = scan_values("small", n, np.random.default_rng(n))
    r = run_scan(inp, n, in_place=True, clamp=FULL)
    assert r["out"] is r["inp"]
    verify_scan(r, inp, n, clamp=FULL)


@pytest.mark.parametrize("which", ["0", "1", "17", "n-1", "n"])
@pytest.mark.parametrize("gathered", [False, True], ids=["plain", "gathered"])
def test_scan_device_side_length(which, gathered):
    """n_ptr on a grid sized for n: blocks behind the data leave, block 0 still publishes; nothing at or behind n_ptr is written"""
    n = 3 * CONST.SCAN_CHUNK + 5
    m = {"0": 0, "1": 1, "17": 17, "n-1": n - 1, "n": n}[which]
    rng = np.random.default_rng(m)
    inp = scan_values("near_2^31", n + 13, rng)
    gather = perm(n + 13, rng)[:n] if gathered else None
    r = run_scan(inp, n, gather=gather, n_ptr=m, clamp=1000)
    verify_scan(r, inp, n, gather=gather, n_ptr=m, clamp=1000)


@pytest.mark.parametrize("side", [False, True], ids=["no_side", "side_out"])
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("n", [17, CONST.SCAN_CHUNK + 1, SCAN_BIG])
def test_scan_gathered(n, masked, side):
    """in[gather[i]] & in_mask is scanned, in[gather[i]] >> TILE_COUNT_BITS goes to side_out, and side_flag says which"""
    rng = np.random.default_rng(n + masked + 2 * side)
    inp = uniform(n + 13, rng)                      # a count in the low TILE_COUNT_BITS bits, a side value above them
    gather = perm(n + 13, rng)[:n]
    mask = (1 << CONST.TILE_COUNT_BITS) - 1 if masked else FULL
    r = run_scan(inp, n, gather=gather, in_mask=mask, side=side, clamp=1 << 20)
    verify_scan(r, inp, n, gather=gather, in_mask=mask, side=side, clamp=1 << 20)
    assert np.array_equal(r["inp"].data(), inp)     # the table itself is only read


def test_scan_side_flag_is_optional_and_zero_without_side_out():
    n = 100
    inp = scan_values("small", n, np.random.default_rng(1))
    verify_scan(run_scan(inp, n, side_flag=False, clamp=7), inp, n, side_flag=False, clamp=7)
    r = run_scan(inp, n, side_flag=True, clamp=7)
    assert r["flag"] == 0
    verify_scan(r, inp, n, clamp=7)


def test_scan_refuses_what_it_cannot_do():
    """a gather staged through `out` cannot have out == in, a mask or side values need a gather, and the shim refuses an n_ptr
    above n: an error, and nothing was launched (every output still holds its sentinel)"""
    n = 100
    rng = np.random.default_rng(2)
    inp = scan_values("small", n, rng)
    for kw, rc in ((dict(gather=perm(n, rng), alias_gather_out=True), H.HIP_INVALID_VALUE),
                   (dict(in_mask=0xFFFFF), H.HIP_INVALID_VALUE), (dict(side=True), H.HIP_INVALID_VALUE),
                   (dict(n_ptr=n + 1), H.REFUSED_COUNT)):
        r = run_scan(inp, n, **kw)
        assert r["rc"] == rc, (kw.keys(), r["rc"])
        assert np.array_equal(r["inp"].data(), inp)
        assert r["out"] is r["inp"] or r["out"].untouched()
        assert r["total"] == SENT64 and r["status"] == [SENT64] * 3 and r["zero_word"] == SENT32 and r["clamped"] == SENT32
        assert r["overflow"] == SENT32 and r["flag"] == SENT32
        if rc != H.REFUSED_COUNT:
            assert r["host"] == [SENT64] * 4


# ================================================================================================================ launch_zero ===
@pytest.mark.parametrize("offset", [0, 4], ids=["aligned", "offset4"])
@pytest.mark.parametrize("nbytes", [0, 4, 12, 16, 20, 4096 + 4, (2 << 20) + 8, 1027])
def test_launch_zero(nbytes, offset):
    """exactly the requested bytes become zero — through the kernel (16-byte aligned, whole words) and through the fallback
    (an unaligned pointer or a byte count that is no multiple of 4) — and the bytes on both sides stay"""
    buf = Guarded(nbytes, torch.uint8, offset=offset)
    assert buf.ptr.value % 16 == offset
    rc = H.lib().msgst_launch_zero(buf.ptr, nbytes, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert not buf.data().any()
    assert buf.guards_intact()

"""ctypes loader of the TEST-ONLY library ms-gs_amd/build/libmsgs_sort_harness.so (tests/native/sort_harness.hip + sort.o): the
radix sort, the exclusive scan and launch_zero of ms-gs_amd/csrc/sort.hip behind a C shim with raw device pointers, and the host
queries that describe the sort's geometry.  Loading it and the host queries need no GPU.  Not part of the product ABI."""
import ctypes as C
import os
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# MSGS_SORT_HARNESS_LIB: another build of the library (a mutated sort.hip, to see the tests fail)
LIB_PATH = os.environ.get("MSGS_SORT_HARNESS_LIB") or os.path.join(ROOT, "ms-gs_amd", "build", "libmsgs_sort_harness.so")

# shim refusals (negative; nothing was launched) and the one HIP error the entry points themselves return
REFUSED_COUNT, REFUSED_BOTH_COUNTS, REFUSED_KEYS16, REFUSED_SCRATCH = -1, -2, -3, -4
HIP_INVALID_VALUE = 1

Geom = namedtuple("Geom", "items mid big scanned gsize ngroups nb scratch_bytes")
Constants = namedtuple("Constants", "SCAN_CHUNK SCAN_THREADS TILE_COUNT_BITS SORT_THREADS SORT_MID_N SORT_BIG_N "
                                    "SORT_SCANNED_MIN_BLOCKS SORT_MAX_GROUPS SORT_SCANNED_GSIZE SCAN_ITEMS")

_lib = None


def lib():
    """the library; a missing file is an error (make -C ms-gs_amd, or __graft_entry__.build(), produces it)"""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH}: build it with `make -C ms-gs_amd`")
        L = C.CDLL(LIB_PATH)
        i64, p, i, u64, u32 = C.c_int64, C.c_void_p, C.c_int, C.c_uint64, C.c_uint32
        L.msgst_sort_geom.argtypes, L.msgst_sort_geom.restype = [i64, C.POINTER(i64)], None
        L.msgst_constants.argtypes, L.msgst_constants.restype = [C.POINTER(i64)], None
        L.msgst_scan_blocks.argtypes, L.msgst_scan_blocks.restype = [i64], i64
        L.msgst_sort_zero_region.argtypes = [i64, i, i, p, C.POINTER(i64), C.POINTER(i64)]
        L.msgst_sort_zero_region.restype = i
        L.msgst_sort_keys16_ok.argtypes, L.msgst_sort_keys16_ok.restype = [i64, i, i], i
        L.msgst_sort_supports_device_count.argtypes, L.msgst_sort_supports_device_count.restype = [i64, i, i], i
        L.msgst_sort_pairs.argtypes = [p, p, p, p, i64, i, i, p, i64, p, i, p, p, i]
        L.msgst_sort_pairs.restype = i
        L.msgst_scan.argtypes = [p, p, p, i64, p, p, p, p, i, u64, u64, C.POINTER(u64), p, p, u64, p, p, p, u32, p, p]
        L.msgst_scan.restype = i
        L.msgst_launch_zero.argtypes, L.msgst_launch_zero.restype = [p, u64, p], i
        _lib = L
    return _lib


def geom(n):
    out = (C.c_int64 * 8)()
    lib().msgst_sort_geom(int(n), out)
    return Geom(int(out[0]), bool(out[1]), bool(out[2]), bool(out[3]), int(out[4]), int(out[5]), int(out[6]), int(out[7]))


def constants():
    out = (C.c_int64 * 10)()
    lib().msgst_constants(out)
    return Constants(*[int(v) for v in out])


def scan_blocks(n):
    return int(lib().msgst_scan_blocks(int(n)))


def zero_region(n, begin_bit, end_bit, scratch_ptr=None):
    """(byte offset into the scratch, words) of the region a pre_zeroed sort needs clear, or None.  scratch_ptr: the address of
    a scratch buffer of geom(n).scratch_bytes (only offsets into it are formed); a host buffer stands in when it is not given"""
    off, words = C.c_int64(0), C.c_int64(0)
    stand_in = None
    if scratch_ptr is None:
        stand_in = (C.c_char * geom(n).scratch_bytes)()
        scratch_ptr = C.addressof(stand_in)
    if not lib().msgst_sort_zero_region(int(n), begin_bit, end_bit, C.c_void_p(scratch_ptr), C.byref(off), C.byref(words)):
        return None
    return int(off.value), int(words.value)


def keys16_ok(n, begin_bit, end_bit):
    return bool(lib().msgst_sort_keys16_ok(int(n), begin_bit, end_bit))


def supports_device_count(n, begin_bit, end_bit):
    return bool(lib().msgst_sort_supports_device_count(int(n), begin_bit, end_bit))


def regime(n):
    """the name of the code path a sort of n pairs takes: keys per thread, and whether the group-scan kernel runs"""
    g = geom(n)
    return f"items{g.items}" + ("-scanned" if g.scanned else "")


REGIMES = ("items4", "items8", "items16", "items16-scanned")


def _first(pred, lo, hi):
    """smallest n in [lo, hi] with pred(n), pred monotone (false ... false true ... true); None when pred(hi) is false"""
    if not pred(hi):
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if pred(mid):
            hi = mid
        else:
            lo = mid + 1
    return lo


def thresholds():
    """the smallest n with 8 keys per thread, with 16, and on the scanned route, found by bisection on the geometry query"""
    top = 1 << 32
    mid = _first(lambda n: geom(n).items >= 8, 1, top)
    big = _first(lambda n: geom(n).items >= 16, 1, top)
    scanned = _first(lambda n: geom(n).scanned, 1, top)
    assert mid and big and scanned and mid < big < scanned, (mid, big, scanned)
    return dict(mid=mid, big=big, scanned=scanned)


def chunk(n):
    """pairs per block of a sort of n pairs"""
    return constants().SORT_THREADS * geom(n).items


def boundary_sizes():
    """each threshold, the size below it, and one chunk + 1 above it: [(n, what)]"""
    out = []
    for name, t in thresholds().items():
        out += [(t - 1, f"{name}-1"), (t, name), (t + chunk(t) + 1, f"{name}+chunk+1")]
    return out


def group_sizes():
    """one full group of 8 blocks +-1 pair, and the first size at which a group grows past 8 blocks +-1 pair (4 keys per thread)"""
    g1 = geom(1)
    one_group = g1.gsize * chunk(1)
    grows = _first(lambda n: geom(n).gsize > g1.gsize, 1, thresholds()["mid"] - 1)
    assert grows is not None
    return [(one_group - 1, "group-1"), (one_group, "group"), (one_group + 1, "group+1"),
            (grows - 1, "gsize-grows-1"), (grows, "gsize-grows"), (grows + 1, "gsize-grows+1")]


def regime_sizes():
    """one ragged size per regime, derived from the thresholds: {regime name: n}"""
    t = thresholds()
    sizes = {"items4": 69 * chunk(1) + 369, "items8": t["mid"] + chunk(t["mid"]) + 1, "items16": t["big"],
             "items16-scanned": t["scanned"]}
    for name, n in sizes.items():
        assert regime(n) == name, (name, n, regime(n))
    return sizes

"""ctypes loader of the TEST-ONLY library ms-gs_amd/build/libmsgs_depth_sort_harness.so (tests/native/depth_sort_harness.hip +
sort.o): the forward's depth sort — bucket path and LSD passes — behind one C shim with raw device pointers, the host rule that
chooses between them, and a numpy restatement of the splitter.  Loading it and the host queries need no GPU.  Not part of the
product ABI."""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("MSGS_DEPTH_SORT_HARNESS_LIB") or os.path.join(ROOT, "ms-gs_amd", "build",
                                                                         "libmsgs_depth_sort_harness.so")

REFUSED_SCRATCH, REFUSED_SIZE = -4, -6
MODE_AUTO, MODE_LSD, MODE_BUCKETS = 0, 1, 2

Constants = namedtuple("Constants", "BIN_SHIFT BIN_LO BINS COARSE BUCKETS LDS_CAP BUCKET_MAX_P HARD_MAX_N LDS_THREADS LDS_ITEMS")
Scratch = namedtuple("Scratch", "sort coarse map bases slices total zero_end")

_lib = None


def lib():
    """the library; a missing file is an error (make -C ms-gs_amd, or __graft_entry__.build(), produces it)"""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH}: build it with `make -C ms-gs_amd`")
        L = C.CDLL(LIB_PATH)
        i64, p, i, u32 = C.c_int64, C.c_void_p, C.c_int, C.c_uint32
        L.msgsd_constants.argtypes, L.msgsd_constants.restype = [C.POINTER(i64)], None
        L.msgsd_depth_bin.argtypes, L.msgsd_depth_bin.restype = [u32], u32
        L.msgsd_scratch.argtypes, L.msgsd_scratch.restype = [i64, C.POINTER(i64)], None
        L.msgsd_zero_region.argtypes, L.msgsd_zero_region.restype = [i64, p, C.POINTER(i64), C.POINTER(i64)], i
        L.msgsd_uses_buckets.argtypes, L.msgsd_uses_buckets.restype = [i64], i
        L.msgsd_set_mode.argtypes, L.msgsd_set_mode.restype = [i], i
        L.msgsd_get_mode.argtypes, L.msgsd_get_mode.restype = [], i
        L.msgsd_sort.argtypes, L.msgsd_sort.restype = [i, p, p, p, i64, p, i64, p, i, p, p], i
        _lib = L
    return _lib


def constants():
    out = (C.c_int64 * 10)()
    lib().msgsd_constants(out)
    return Constants(*[int(v) for v in out])


def scratch(n):
    out = (C.c_int64 * 7)()
    lib().msgsd_scratch(int(n), out)
    return Scratch(*[int(v) for v in out])


def zero_region(n, scratch_ptr=None):
    """(byte offset into the scratch, words) of what a pre_zeroed bucket sort needs clear"""
    off, words = C.c_int64(0), C.c_int64(0)
    stand_in = None
    if scratch_ptr is None:
        stand_in = (C.c_char * scratch(n).total)()
        scratch_ptr = C.addressof(stand_in)
    if not lib().msgsd_zero_region(int(n), C.c_void_p(scratch_ptr), C.byref(off), C.byref(words)):
        return None
    return int(off.value), int(words.value)


def uses_buckets(n, mode=None):
    """the host rule for n Gaussians; with `mode` under that value of the switch (restored afterwards)"""
    if mode is None:
        return bool(lib().msgsd_uses_buckets(int(n)))
    prev = lib().msgsd_set_mode(mode)
    try:
        return bool(lib().msgsd_uses_buckets(int(n)))
    finally:
        lib().msgsd_set_mode(prev)


def depth_bin(keys):
    """numpy restatement of depth_bin (msgs_internal.h) over an array of uint32 keys"""
    c = constants()
    b = (np.asarray(keys, dtype=np.uint32) >> np.uint32(c.BIN_SHIFT)).astype(np.int64)
    return np.clip(b, c.BIN_LO, c.BIN_LO + c.BINS - 1) - c.BIN_LO


def splitter(hist, buckets=None):
    """numpy restatement of depth_split_kernel: (bucket of every bin, bases[0 .. buckets + 1]) from the bins' counts.
    bucket[b] = floor(exclusive_prefix[b] * buckets / V); bases[k] = keys in buckets below k."""
    buckets = constants().BUCKETS if buckets is None else buckets
    hist = np.asarray(hist, dtype=np.int64)
    excl = np.cumsum(hist) - hist
    V = int(hist.sum())
    bucket = excl * buckets // V if V else np.zeros_like(excl)
    size = np.bincount(bucket, weights=hist, minlength=buckets + 1).astype(np.int64)
    bases = np.concatenate([[0], np.cumsum(size)])
    return bucket, bases

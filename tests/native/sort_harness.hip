// sort_harness.hip — TEST-ONLY C shim over the internal sort / scan entry points of ms-gs_amd/csrc/sort.hip
// (msgs_internal.h).  Linked with build/sort.o alone into ms-gs_amd/build/libmsgs_sort_harness.so; not part of the product
// ABI (include/msgs.h), never shipped by setup.py.  tests/sort_harness.py loads it, tests/test_sort_gpu.py drives it.
//
// Return codes: 0 = success, > 0 = the hipError_t of the call, < 0 = the shim refused the arguments BEFORE launching
// anything (a test must never be able to produce an out-of-range write):
//   -1 a device-side count above n        -2 n_valid_dev together with n_dev     -3 keys16 without radix_sort_keys16_ok
//   -4 the scratch is smaller than SortScratch(n)                                -5 the mapped host words are unavailable
#include "../../ms-gs_amd/csrc/msgs_internal.h"

using namespace msgs;

namespace {
// the value of a device word the launch is going to trust, read on the stream the launch goes to
int read_count(const void* dev_word, hipStream_t s, uint32_t* v) {
    hipError_t e = hipMemcpyAsync(v, dev_word, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return (int)e;
}
}  // namespace

extern "C" {

// out[0..7] = items, mid, big, scanned, gsize, ngroups, nb, SortScratch(n).total
void msgst_sort_geom(int64_t n, int64_t* out) {
    const SortGeom G(n);
    out[0] = G.items; out[1] = G.mid; out[2] = G.big; out[3] = G.scanned;
    out[4] = G.gsize; out[5] = G.ngroups; out[6] = G.nb;
    out[7] = (int64_t)SortScratch(n).total;
}

// out[0..9] = SCAN_CHUNK, SCAN_THREADS, TILE_COUNT_BITS, SORT_THREADS, SORT_MID_N, SORT_BIG_N, SORT_SCANNED_MIN_BLOCKS,
//             SORT_MAX_GROUPS, SORT_SCANNED_GSIZE, SCAN_ITEMS
void msgst_constants(int64_t* out) {
    out[0] = SCAN_CHUNK; out[1] = SCAN_THREADS; out[2] = TILE_COUNT_BITS; out[3] = SORT_THREADS; out[4] = SORT_MID_N;
    out[5] = SORT_BIG_N; out[6] = SORT_SCANNED_MIN_BLOCKS; out[7] = SORT_MAX_GROUPS; out[8] = SORT_SCANNED_GSIZE;
    out[9] = SCAN_ITEMS;
}

int64_t msgst_scan_blocks(int64_t n) { return scan_blocks(n); }

// radix_sort_zero_region as (byte offset into the scratch, words); returns 1 when there is such a region.  `scratch`: the
// start of a buffer of SortScratch(n).total bytes, host or device (never dereferenced)
int msgst_sort_zero_region(int64_t n, int begin_bit, int end_bit, void* scratch, int64_t* byte_offset, int64_t* words) {
    char* const base = (char*)scratch;
    uint32_t* p = nullptr;
    size_t w = 0;
    if (!radix_sort_zero_region(n, begin_bit, end_bit, base, &p, &w)) return 0;
    *byte_offset = (int64_t)(reinterpret_cast<char*>(p) - base);
    *words = (int64_t)w;
    return 1;
}

int msgst_sort_keys16_ok(int64_t n, int begin_bit, int end_bit) { return radix_sort_keys16_ok(n, begin_bit, end_bit) ? 1 : 0; }

int msgst_sort_supports_device_count(int64_t n, int begin_bit, int end_bit) {
    return radix_sort_supports_device_count(n, begin_bit, end_bit) ? 1 : 0;
}

int msgst_sort_pairs(void* keys_in, void* vals_in, void* keys_out, void* vals_out, int64_t n, int begin_bit, int end_bit,
                     void* scratch, int64_t scratch_bytes, void* stream, int pre_zeroed, void* n_valid_dev, const void* n_dev,
                     int keys16) {
    hipStream_t s = (hipStream_t)stream;
    if (n_valid_dev && n_dev) return -2;
    if (keys16 && !radix_sort_keys16_ok(n, begin_bit, end_bit)) return -3;
    if (n > 0 && scratch_bytes < (int64_t)SortScratch(n).total) return -4;
    if (n_dev) {
        uint32_t v = 0;
        if (int e = read_count(n_dev, s, &v)) return e;
        if ((int64_t)v > (n > 0 ? n : 0)) return -1;
    }
    return (int)radix_sort_pairs((uint32_t*)keys_in, (uint32_t*)vals_in, (uint32_t*)keys_out, (uint32_t*)vals_out, n, begin_bit,
                                 end_bit, (char*)scratch, s, pre_zeroed != 0, (uint32_t*)n_valid_dev, (const uint32_t*)n_dev,
                                 keys16 != 0);
}

// use_host: the polled host words are allocated here (mapped, 4 x u64, filled with host_fill), handed to the scan, and
// copied to host_out[0..3] after a stream synchronise
int msgst_scan(const void* in, const void* gather, void* out, int64_t n, void* partials, void* total, void* stream,
               void* status, int use_host, uint64_t ticket, uint64_t host_fill, uint64_t* host_out, const void* n_ptr,
               void* clamped_total, uint64_t clamp, const void* extra, void* zero_word, void* overflow_flag, uint32_t in_mask,
               void* side_out, void* side_flag) {
    hipStream_t s = (hipStream_t)stream;
    if (n_ptr) {
        uint32_t v = 0;
        if (int e = read_count(n_ptr, s, &v)) return e;
        if ((int64_t)v > (n > 0 ? n : 0)) return -1;
    }
    uint64_t* host = nullptr;
    uint64_t* host_dev = nullptr;
    if (use_host) {
        void *h = nullptr, *d = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return -5; }
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { (void)hipHostFree(h); (void)hipGetLastError(); return -5; }
        host = (uint64_t*)h;
        host_dev = (uint64_t*)d;
        for (int k = 0; k < 8; ++k) host[k] = host_fill;
    }
    hipError_t e = exclusive_scan_u32((const uint32_t*)in, (const uint32_t*)gather, (uint32_t*)out, n, (uint64_t*)partials,
                                      (uint64_t*)total, s, (uint64_t*)status, host_dev, ticket, (const uint32_t*)n_ptr,
                                      (uint32_t*)clamped_total, clamp, (const uint32_t*)extra, (uint32_t*)zero_word,
                                      (uint32_t*)overflow_flag, in_mask, (uint32_t*)side_out, (uint32_t*)side_flag);
    if (use_host) {
        const hipError_t es = hipStreamSynchronize(s);
        for (int k = 0; k < 4; ++k) host_out[k] = host[k];
        (void)hipHostFree(host);
        if (e == hipSuccess) e = es;
    }
    return (int)e;
}

int msgst_launch_zero(void* ptr, uint64_t bytes, void* stream) { return (int)launch_zero(ptr, (size_t)bytes, (hipStream_t)stream); }

}  // extern "C"

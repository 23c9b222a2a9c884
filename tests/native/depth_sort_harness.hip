// depth_sort_harness.hip — TEST-ONLY C shim over the forward's depth sort in ms-gs_amd/csrc/sort.hip (msgs_internal.h): the bucket
// path (depth_sort_buckets) and the LSD passes (radix_sort_pairs with a survivor count) on the same raw device pointers, and the
// host queries of the bucket path.  Linked with build/sort.o alone into ms-gs_amd/build/libmsgs_depth_sort_harness.so; not part
// of the product ABI (include/msgs.h), never shipped by setup.py.  tests/depth_sort_harness.py loads it.
//
// Return codes: 0 = success, > 0 = the hipError_t of the call, < 0 = the shim refused the arguments BEFORE launching anything:
//   -4 the scratch is smaller than DepthSortScratch(n)        -6 n is outside what the bucket path sorts
#include "../../ms-gs_amd/csrc/msgs_internal.h"

using namespace msgs;

extern "C" {

// out[0..9] = DEPTH_BIN_SHIFT, DEPTH_BIN_LO, DEPTH_BINS, DEPTH_COARSE, DEPTH_BUCKETS, DEPTH_LDS_CAP, DEPTH_BUCKET_MAX_P,
//             DEPTH_BUCKET_HARD_MAX (the largest n the bucket path sorts), DEPTH_LDS_THREADS, DEPTH_LDS_ITEMS
void msgsd_constants(int64_t* out) {
    out[0] = DEPTH_BIN_SHIFT; out[1] = DEPTH_BIN_LO; out[2] = DEPTH_BINS; out[3] = DEPTH_COARSE; out[4] = DEPTH_BUCKETS;
    out[5] = DEPTH_LDS_CAP; out[6] = DEPTH_BUCKET_MAX_P; out[7] = DEPTH_BUCKET_HARD_MAX;
    out[8] = DEPTH_LDS_THREADS; out[9] = DEPTH_LDS_ITEMS;
}

uint32_t msgsd_depth_bin(uint32_t key) { return depth_bin(key); }

// out[0..6] = DepthSortScratch(n): sort, coarse, map, bases, slices, total, zero_end
void msgsd_scratch(int64_t n, int64_t* out) {
    const DepthSortScratch L(n);
    out[0] = (int64_t)L.sort; out[1] = (int64_t)L.coarse; out[2] = (int64_t)L.map; out[3] = (int64_t)L.bases;
    out[4] = (int64_t)L.slices; out[5] = (int64_t)L.total; out[6] = (int64_t)L.zero_end();
}

// depth_sort_zero_region as (byte offset into the scratch, words); `scratch` is never dereferenced
int msgsd_zero_region(int64_t n, void* scratch, int64_t* byte_offset, int64_t* words) {
    char* const base = (char*)scratch;
    uint32_t* p = nullptr;
    size_t w = 0;
    if (!depth_sort_zero_region(n, base, &p, &w)) return 0;
    *byte_offset = (int64_t)(reinterpret_cast<char*>(p) - base);
    *words = (int64_t)w;
    return 1;
}

int msgsd_uses_buckets(int64_t n) { return depth_sort_uses_buckets(n) ? 1 : 0; }
int msgsd_set_mode(int mode) { return set_depth_sort(mode); }
int msgsd_get_mode(void) { return get_depth_sort(); }

// buckets != 0: depth_sort_buckets; else radix_sort_pairs(keys_in, nullptr, ..., 0, 32, ..., n_valid_dev) on the same scratch.
// info: two device words (may be NULL)
int msgsd_sort(int buckets, void* keys_in, void* keys_out, void* vals_out, int64_t n, void* scratch, int64_t scratch_bytes,
               void* stream, int pre_zeroed, void* n_valid_dev, void* info) {
    hipStream_t s = (hipStream_t)stream;
    if (n > 0 && scratch_bytes < (int64_t)DepthSortScratch(n).total) return -4;
    if (buckets) {
        if (n > DEPTH_BUCKET_HARD_MAX) return -6;
        return (int)depth_sort_buckets((const uint32_t*)keys_in, (uint32_t*)keys_out, (uint32_t*)vals_out, n, (char*)scratch, s,
                                       pre_zeroed != 0, (uint32_t*)n_valid_dev, (uint32_t*)info);
    }
    return (int)radix_sort_pairs((uint32_t*)keys_in, nullptr, (uint32_t*)keys_out, (uint32_t*)vals_out, n, 0, 32,
                                 (char*)scratch + DepthSortScratch(n).sort, s, pre_zeroed != 0, (uint32_t*)n_valid_dev);
}

}  // extern "C"

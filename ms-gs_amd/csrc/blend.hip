// blend.hip — per-tile front-to-back alpha-composite forward (K6) and back-to-front gradient
// backward (K7) for gfx950.  Replaces renderCUDA forward/backward of the
// reference's un-vendored CUDA module (call site gaussian_renderer/__init__.py:94-108).
//
// Structure (both kernels): one 256-thread workgroup per 16x16 tile; the four wave64s each own one
// 8x8 pixel QUADRANT (lane l -> pixel (l & 7, l >> 3) of the quadrant).  The tile's depth-sorted
// Gaussian list is staged through LDS in batches of 256 records (coalesced 4-B id loads, then three
// 16-B gathers per record).  The loading thread also classifies its record against the four
// quadrants with the exact alpha >= 1/255 level-set test, and every wave compacts the batch to the
// entries that can touch ITS quadrant (64-bit ballot + popcount prefix), so the per-pixel loop only
// visits records that matter for that wave.  Skipping a record whose alpha is < 1/255 on every
// pixel of the quadrant is exactly what the per-pixel `continue` of the reference does, so results
// are unchanged.
//
// Both kernels are INSTRUCTION-ISSUE bound (a SIMD issues about one instruction of any kind per 2 cycles; compares, selects
// and DPP at half rate, v_exp / v_rcp at a quarter: tools/valu_calib.hip), so the per-(pixel, Gaussian)
// math is kept minimal: the record carries the conic pre-scaled into the log2 domain and log2(opacity), so
//     alpha_raw = exp2( A' dx^2 + 2B' dx dy + C' dy^2 + log2 o )
// is six FMA-class ops and one v_exp_f32; the three monomials double as the weights of the conic sums in
// the backward, the mean gradient is accumulated as (sum q dx, sum q dy), the colour recurrence is one
// scalar (see blend_backward_kernel), and every per-Gaussian constant factor (0.5 W, -1/2, 1/o, 2 ln 2,
// the conic in front of the mean sums) is applied once per Gaussian in preprocess_backward_kernel
// instead of once per pixel here.
//
// Backward reduction: per (wave, record) the nine partial sums are reduced across the 64 lanes with a
// hand-scheduled DPP reduce-scatter inside each 16-lane row (row_reduce_scatter: 8 -> 4 -> 2 -> 1 values per
// lane, the ninth riding on the duplicate lanes), one cross-row all-reduce of the single remaining value, and ONE
// global_atomic_add_f64 instruction from nine lanes into the 80-byte per-Gaussian gradient record of double accumulators
// (the tiles' float32 sums add up exactly, so the default backward is reproducible whatever order the atomics arrive in:
// DESIGN.md 4.2) — one atomic per (quadrant or tile, Gaussian, component) instead of the reference's one per (pixel,
// Gaussian, component).
// (An LDS accumulator committed once per batch was measured slower and removed, profiles/r1_notes.md.)
//
// Roofline: HBM-bound by contract (BASELINE.json); algorithmic bytes K6 = 48*D_trav + 28*N + 8*tiles,
// K7 = 48*D_trav + 20*N + 36*V.
#include "msgs_internal.h"

#include <atomic>
#include <type_traits>

#include <algorithm>

namespace msgs {

namespace {

constexpr int BATCH = 256;
constexpr float ALPHA_MIN = 1.0f / 255.0f;
constexpr float T_MIN = 0.0001f;

// Shared by forward and backward so both take bit-identical skip decisions: explicit FMA order.
//   p = A' dx^2 + B2' dx dy + C' dy^2 + lo     (log2 of the unclamped alpha; B2' = 2 Bh', doubled when the record is
// staged into LDS).  The three monomials double as the weights of the backward's conic sums, and the mean gradient is
// accumulated as (sum q dx, sum q dy) — preprocess_backward_kernel applies the per-Gaussian (A', Bh', C') to them —
// so the backward needs no product beyond these.
struct PairEval { float dxx, dxy, dyy, p; };
__device__ __forceinline__ PairEval eval_pair(float A, float B2, float C, float lo, float dx, float dy) {
#pragma clang fp contract(off)   // only the explicit FMAs below; nothing else may be fused differently per kernel
    PairEval e;
    e.dxx = __fmul_rn(dx, dx);
    e.dxy = __fmul_rn(dx, dy);
    e.dyy = __fmul_rn(dy, dy);
    e.p = __fmaf_rn(A, e.dxx, __fmaf_rn(B2, e.dxy, __fmaf_rn(C, e.dyy, lo)));
    return e;
}
__device__ __forceinline__ float4 doubled_w(const float4& r) { return make_float4(r.x, r.y, r.z, r.w + r.w); }
// Bound of the sign test of the exponent (SPEC Q11: an entry whose exponent comes out positive is skipped — a rounding guard, the
// conic being positive definite).  e.p is log2(alpha) = q + log2(opacity) from ONE FMA chain, and q > 0 is tested as p > bound.
// With bound = log2(opacity) itself (rounds 1-5) the sign of q was resolved to one ulp of log2(opacity) only: a cross term of
// +0.6 ulp rounds the chain up and two negative terms of 0.4 ulp each are lost — an entry with q = -1e-8 was skipped a hair from
// the centre of a giant Gaussian (found by the 60 000-configuration sweep, profiles/r5_parity.md 2.3).  The bound sits two to
// four ulps above log2(opacity): roundings of the chain never skip; a genuinely positive exponent (an indefinite conic from a
// degenerate covariance) still does.  One value per staged record, in a slot the walks read anyway.
__device__ __forceinline__ float sign_test_bound(float lo) { return __fmaf_rn(fabsf(lo), 2.4e-7f, lo); }
__device__ __forceinline__ float4 with_bound(const float4& r2, float lo) { return make_float4(r2.x, r2.y, r2.z, sign_test_bound(lo)); }

// quadrant hit mask of one record (bit q: quadrant q = qx + 2*qy of the tile at (tx0, ty0))
__device__ __forceinline__ uint32_t quadrant_mask(const float4& r0, float C, float tau2, float tx0, float ty0) {
    if (!(tau2 > -1.0e38f)) return 0xFu;
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float x0 = tx0 + (float)((q & 1) * 8), y0 = ty0 + (float)((q >> 1) * 8);
        if (levelset_hits_rect(r0.x, r0.y, r0.z, r0.w, C, tau2, x0, x0 + 7.0f, y0, y0 + 7.0f)) m |= 1u << q;
    }
    return m;
}

// XCD-aware tile order: the dispatcher places workgroup b on XCD b % 8 (MI355X_MICROARCH.md).  Give
// every XCD a contiguous run of tiles so neighbouring tiles (which share Gaussians) share an L2.
__device__ __forceinline__ int swizzled_tile(int bid, int num_tiles) {
    const int per = num_tiles >> 3;            // tiles per XCD in the divisible part
    const int main = per << 3;
    if (bid >= main) return bid;               // ragged tail: identity
    return (bid & 7) * per + (bid >> 3);
}

// Side job of the forward blend kernels: clear the backward's per-Gaussian gradient records (msgs.h, grad_records).  They
// have to start from zero; done here the 80 bytes per Gaussian cost nothing — the kernels are instruction-issue bound with
// the memory pipe mostly idle, the stores are fire-and-forget and nothing in this kernel reads them — and the backward saves a
// fill launch.  Workgroup b clears slice b of the buffer (n16 sixteen-byte words in total).
constexpr int CLEAR_INLINE_MIN_TILES = 2048;
__device__ __forceinline__ void clear_slice(uint4* __restrict__ p, size_t n16) {
    if (p == nullptr) return;
    const size_t per = (n16 + gridDim.x - 1) / gridDim.x;
    const size_t lo = per * blockIdx.x;
    const size_t hi = lo + per < n16 ? lo + per : n16;
    for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// Per-tile traversal length for the backward's launch order (ImageLayout::tile_last): the position behind the last entry any
// pixel of the tile blended = the number of list entries the backward will walk for this tile — its work, to first order.
// Also invalidates the previous frame's launch order (launch_tile_order re-validates it after this kernel).
// The stored key estimates the backward's instruction count for the tile (/ 16): ~52 per traversed entry (record fetch, loop
// control, the 64-lane reduction, the atomics) + ~36 per (quadrant, entry) evaluation, the latter counted as the entries the
// forward's waves walked (`walked`, wave-uniform).
__device__ __forceinline__ void note_tile_last(uint32_t* s_wlast, int nwaves, uint32_t last, uint32_t walked, int tile, int w,
                                               int lane, uint32_t* __restrict__ tile_last,
                                               uint32_t* __restrict__ order_flag, unsigned long long* __restrict__ dtrav = nullptr) {
    if (tile_last == nullptr) return;
    const uint32_t wl = wave_max_u32(last);
    if (lane == 0) { s_wlast[w] = wl; s_wlast[nwaves + w] = walked; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t m = 0, q = 0;
        for (int k = 0; k < nwaves; ++k) { m = max(m, s_wlast[k]); q += s_wlast[nwaves + k]; }
        tile_last[tile] = (52u * m + 36u * q) >> 4;
        // entries of this tile's list that are traversed (sum over the tiles = D_trav), into one of DTRAV_SLOTS accumulators
        if (dtrav) atomicAdd(&dtrav[tile & (DTRAV_SLOTS - 1)], (unsigned long long)m);
        if (blockIdx.x == 0 && order_flag) *order_flag = 0u;
    }
}

// Per-pixel forward state and the walk over one wave's compacted entry list — shared by the quadrant-per-wave kernel
// and the fine-grained (4x4 sub-block per wave) kernel, so that both evaluate every pixel with the same instructions in
// the same order (bit-identical images, test_blend_granularities_agree).
struct FwdPix {
    float T, C0, C1, C2, aps, adp;
};
// depth-slab binning (msgs_view_t.slab_fraction) and feedback: what blend_forward_kernel does besides blending
struct FwdSlab {
    uint32_t* open_bits;          // slab A: publish the tiles that are still open here (bitmap) ...
    uint32_t* open_list;          // ... and here (list, any order)
    uint32_t* n_open;             // ... counted here
    const uint32_t* tile_list;    // slab B: blend only these tiles
    const uint32_t* n_tiles;      // ... this many
    unsigned long long* dtrav;    // D_trav accumulators (feedback; nullable)
};
// lp[0..cnt): BYTE offsets of the batch's 16-byte records this wave has to evaluate, in list order.  `alive` = lanes still
// blending, as a SCALAR mask: every predicate is the ballot of one direct comparison combined with scalar logic (a ballot
// of a derived bool costs two VALU instructions per use), and per-lane selects take their condition from the mask.
// Returns the byte offset of the last entry blended in this batch (0xFFFFFFFF: none).
// COUNT (diagnostic replica, msgs_blend_lane_stats): also counts, per wave, the entry evaluations (x 64 = evaluated lanes), the
// lanes still blending at each of them and the lanes that blended — scalar popcounts, no effect on the arithmetic.
struct LaneStats { uint32_t steps, alive, blended; };
// Entry lists of the forward kernels: BYTE offsets of the 16-byte records, four bytes each so that ONE 16-byte LDS read
// fetches four of them, and padded to a multiple of four with the offset of a SENTINEL record (slot BATCH of the record
// arrays: zero conic, log2-opacity -1e30 -> alpha = exp2(-1e30) = 0 < 1/255, never valid, every product with it is an exact
// zero).  The walk then takes four entries per trip with one list read, one "any pixel left?" test and one counter update for
// the four — 36 instead of 45 instructions per entry; a padded or post-termination evaluation changes no pixel.
// Measured at C3 (blend_forward_kernel incl. the clearing of the gradient records): two entries per trip 187 us; four per trip
// 216 us when the compiler is free to hoist all thirteen LDS reads of a trip (97 VGPRs -> 4 waves per SIMD) and 182 us
// when it is held to 64 VGPRs / 8 waves per SIMD (amdgpu_waves_per_eu below): issue-bound code wants the waves, not the
// hoisting.  (Folding the two selects of the update into one — alpha_b = blend ? alpha : 0, T = fma(-T, alpha_b, T) —
// measured the same time and was not kept; eight entries per trip: 184 us, no gain.)
constexpr int LIST_PAD = 4;
constexpr uint32_t SENTINEL_OFF = (uint32_t)BATCH << 4;

__device__ __forceinline__ void write_sentinel_record(float4* s_r0, float4* s_r1, float4* s_r2) {
    s_r0[BATCH] = make_float4(0.f, 0.f, 0.f, 0.f);
    s_r1[BATCH] = make_float4(0.f, -1.0e30f, 0.f, 0.f);
    s_r2[BATCH] = make_float4(0.f, 0.f, 0.f, 0.f);
}
// after the compaction: lanes 0..2 of the wave pad its list (cnt entries) up to the next multiple of four
__device__ __forceinline__ void pad_list(uint32_t* lp, int cnt, int lane) {
    if (lane < LIST_PAD - 1) lp[cnt + lane] = SENTINEL_OFF;
}

template <bool COUNT = false>
__device__ __forceinline__ uint32_t forward_walk(const uint32_t* lp, int cnt, const float4* s_r0, const float4* s_r1,
                                                 const float4* s_r2, float pxf, float pyf, FwdPix& st, uint64_t& alive_io,
                                                 uint32_t& walked, LaneStats* stats = nullptr) {
    // the state lives in LOCAL scalars while the list is walked (through the struct reference the compiler turned the
    // two selects of the update into EXEC-masked moves with duplicated loop-carried copies: +14 % VALU instructions)
    float T = st.T, C0 = st.C0, C1 = st.C1, C2 = st.C2, aps = st.aps, adp = st.adp;
    uint64_t alive = alive_io;
    uint32_t last_off = 0xFFFFFFFFu;
    // (a scalar entry index via readfirstlane was measured: 221 -> 257 us — the VALU->SALU->VALU hop in front of
    //  the LDS reads costs more than the two address instructions it saves)
    auto blend_entry = [&](uint32_t off) {
        const float4 r0 = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_r0) + off);
        const float4 r1 = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_r1) + off);
        const float4 r2 = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_r2) + off);
        const float dx = r0.x - pxf, dy = r0.y - pyf;
        const PairEval ev = eval_pair(r0.z, r0.w, r1.x, r1.y, dx, dy);
        const float alpha = fminf(0.99f, __builtin_amdgcn_exp2f(ev.p));
        const float test_T = __fmaf_rn(-T, alpha, T);
        const uint64_t m_pow = __builtin_amdgcn_ballot_w64(ev.p <= r2.w);          // power <= 0 (r2.w: sign_test_bound)
        const uint64_t m_alpha = __builtin_amdgcn_ballot_w64(alpha >= ALPHA_MIN);   // alpha >= 1/255
        const uint64_t m_stop = __builtin_amdgcn_ballot_w64(test_T < T_MIN);
        const uint64_t validm = alive & m_pow & m_alpha;
        const uint64_t stopm = validm & m_stop;
        if (COUNT) {
            // (a trip on padding evaluates the sentinel record and can never blend: not counted)
            if (off != SENTINEL_OFF) {
                stats->steps += 1u; stats->alive += (uint32_t)__popcll(alive); stats->blended += (uint32_t)__popcll(validm & ~stopm);
            }
        }
        alive &= ~stopm;                                                            // terminated: NOT blended (Q7)
        const bool blend = __builtin_amdgcn_inverse_ballot_w64(validm & ~stopm);
        const float wgt = blend ? alpha * T : 0.0f;
        C0 = fmaf(r1.z, wgt, C0); C1 = fmaf(r1.w, wgt, C1); C2 = fmaf(r2.x, wgt, C2);
        adp = fmaf(r2.y, wgt, adp); aps = fmaf(r2.z, wgt, aps);
        T = blend ? test_T : T;
        last_off = blend ? off : last_off;
    };
    int j = 0;
    for (; j < cnt; j += LIST_PAD) {                       // the list is padded to a multiple of four
        if (alive == 0) break;
        const uint4 o = *reinterpret_cast<const uint4*>(lp + j);
        blend_entry(o.x); blend_entry(o.y); blend_entry(o.z); blend_entry(o.w);
    }
    walked += (uint32_t)min(j, cnt);                       // wave-uniform: entries this wave evaluated (backward work estimate)
    st.T = T; st.C0 = C0; st.C1 = C1; st.C2 = C2; st.aps = aps; st.adp = adp;
    alive_io = alive;
    return last_off;
}

__device__ __forceinline__ void forward_store(const FwdPix& st, uint32_t last, bool inside, int px, int py,
                                              const ViewParams& vp, float* out_color, float* out_ps, float* out_depth,
                                              float* final_T, uint32_t* n_contrib) {
    if (inside) {
        const size_t N = (size_t)vp.W * vp.H;
        const size_t pix = (size_t)py * vp.W + px;
        out_color[pix] = st.C0 + st.T * vp.bg[0];
        out_color[N + pix] = st.C1 + st.T * vp.bg[1];
        out_color[2 * N + pix] = st.C2 + st.T * vp.bg[2];
        out_ps[pix] = st.aps;
        out_depth[pix] = st.adp;
        final_T[pix] = st.T;
        n_contrib[pix] = last;
    }
}

// ---------------------------------------------------------------------------------------------
// K6
// ---------------------------------------------------------------------------------------------
// (the kernel: blend_forward_kernel below — one call per workgroup, or, for slab B, one call per listed tile)
template <bool COUNT>
__device__ __forceinline__ void blend_forward_tile(int tile, const ViewParams& vp, const GaussRec* __restrict__ rec,
                                                            const uint32_t* __restrict__ ids,
                                                            const uint2* __restrict__ ranges,
                                                            float* __restrict__ out_color,
                                                            float* __restrict__ out_ps,
                                                            float* __restrict__ out_depth,
                                                            float* __restrict__ final_T,
                                                            uint32_t* __restrict__ n_contrib,
                                                            unsigned long long* __restrict__ lane_stats,
                                                            uint32_t* __restrict__ tile_last,
                                                            uint32_t* __restrict__ order_flag, const FwdSlab& sb,
                                                            float4* s_r0, float4* s_r1, float4* s_r2, uint32_t* s_mask,
                                                            uint32_t* s_wlast, uint32_t (*s_list)[BATCH + LIST_PAD]) {
    const int tx = tile % vp.gx, ty = tile / vp.gx;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int px = tx * TILE + (w & 1) * 8 + (lane & 7);
    const int py = ty * TILE + (w >> 1) * 8 + (lane >> 3);
    const bool inside = px < vp.W && py < vp.H;
    const float pxf = (float)px, pyf = (float)py;
    const float tx0 = (float)(tx * TILE), ty0 = (float)(ty * TILE);
    const uint2 range = ranges[tile];
    const int len = (int)(range.y - range.x);
    const uint64_t lt_mask = (1ull << lane) - 1ull;

    FwdPix st = {1.0f, 0.f, 0.f, 0.f, 0.f, 0.f};
    LaneStats ls = {0u, 0u, 0u};
    uint32_t last = 0, walked = 0;
    // lanes still blending, as a SCALAR mask: every predicate below is the ballot of one direct comparison combined with
    // scalar logic (a ballot of a derived bool costs two VALU instructions per use; these kernels' time is their VALU
    // instruction count), and per-lane selects take their condition from the mask for free
    uint64_t alive = __builtin_amdgcn_ballot_w64(inside);

    for (int base = 0; base < len; base += BATCH) {
        if (__syncthreads_and(alive == 0)) break;    // barrier also protects the LDS batch
        const int n = min(BATCH, len - base);
        if (tid < n) {
            const uint32_t id = ids[range.x + base + tid];
            const float4 r0 = rec[id].r0, r1 = rec[id].r1, r2 = rec[id].r2;
            s_r0[tid] = doubled_w(r0); s_r1[tid] = r1; s_r2[tid] = with_bound(r2, r1.y);
            s_mask[tid] = quadrant_mask(r0, r1.x, r2.w, tx0, ty0);
        }
        __syncthreads();
        // per-wave compaction of the batch to this wave's quadrant; the list holds BYTE offsets of the 16-byte records
        // (one shift less per pair evaluation)
        int cnt = 0;
#pragma unroll
        for (int c = 0; c < BATCH / 64; ++c) {
            const int e = c * 64 + lane;
            const bool hit = e < n && ((s_mask[e] >> w) & 1u);
            const uint64_t b = __ballot(hit);
            if (hit) s_list[w][cnt + __popcll(b & lt_mask)] = (uint32_t)(e << 4);
            cnt += __popcll(b);
        }
        pad_list(s_list[w], cnt, lane);
        const uint32_t last_off = forward_walk<COUNT>(s_list[w], cnt, s_r0, s_r1, s_r2, pxf, pyf, st, alive, walked, &ls);
        if (last_off != 0xFFFFFFFFu) last = (uint32_t)base + (last_off >> 4) + 1u;   // once per batch, not per pair
    }
    if (COUNT) {
        if (lane == 0) {
            atomicAdd(&lane_stats[0], (unsigned long long)ls.steps);
            atomicAdd(&lane_stats[1], (unsigned long long)ls.alive);
            atomicAdd(&lane_stats[2], (unsigned long long)ls.blended);
        }
    } else {
        forward_store(st, last, inside, px, py, vp, out_color, out_ps, out_depth, final_T, n_contrib);
        // slab A: a pixel that is still blending at the end of this list may blend entries of slab B — the tile stays OPEN and
        // is blended again over its complete list (which then also counts its traversed entries).  Where every pixel has
        // terminated (Q7) nothing behind the list is ever evaluated: the tile is done, bit for bit.
        const bool open = sb.open_bits != nullptr && __syncthreads_or(alive != 0);
        note_tile_last(s_wlast, 4, inside ? last : 0u, walked, tile, w, lane, tile_last, order_flag, open ? nullptr : sb.dtrav);
        if (open && threadIdx.x == 0) {
            atomicOr(&sb.open_bits[tile >> 5], 1u << (tile & 31));
            sb.open_list[atomicAdd(sb.n_open, 1u)] = (uint32_t)tile;
        }
    }
}

template <bool COUNT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void blend_forward_kernel(ViewParams vp, const GaussRec* __restrict__ rec,
                                                            const uint32_t* __restrict__ ids,
                                                            const uint2* __restrict__ ranges,
                                                            float* __restrict__ out_color,
                                                            float* __restrict__ out_ps,
                                                            float* __restrict__ out_depth,
                                                            float* __restrict__ final_T,
                                                            uint32_t* __restrict__ n_contrib,
                                                            unsigned long long* __restrict__ lane_stats,
                                                            uint4* __restrict__ clear_ptr, size_t clear_n16,
                                                            uint32_t* __restrict__ tile_last,
                                                            uint32_t* __restrict__ order_flag, FwdSlab sb) {
    __shared__ float4 s_r0[BATCH + 1], s_r1[BATCH + 1], s_r2[BATCH + 1];     // slot BATCH: the sentinel record
    __shared__ uint32_t s_mask[BATCH];
    __shared__ uint32_t s_wlast[8];
    __shared__ __attribute__((aligned(16))) uint32_t s_list[4][BATCH + LIST_PAD];
    clear_slice(clear_ptr, clear_n16);
    if (threadIdx.x == 0) write_sentinel_record(s_r0, s_r1, s_r2);          // ordered by the first barrier of the batch loop
    if (sb.tile_list == nullptr) {
        blend_forward_tile<COUNT>(swizzled_tile(blockIdx.x, vp.gx * vp.gy), vp, rec, ids, ranges, out_color, out_ps, out_depth, final_T,
                                  n_contrib, lane_stats, tile_last, order_flag, sb, s_r0, s_r1, s_r2, s_mask, s_wlast, s_list);
        return;
    }
    // slab B: the tiles slab A left open, in the order they were listed; a small grid walks the list (normally a handful of
    // tiles: a grid of one workgroup per tile of the image would spend 25 us at 4K on workgroups that only learn that)
    const uint32_t n = *sb.n_tiles;
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        blend_forward_tile<COUNT>((int)sb.tile_list[k], vp, rec, ids, ranges, out_color, out_ps, out_depth, final_T, n_contrib,
                                  lane_stats, tile_last, order_flag, sb, s_r0, s_r1, s_r2, s_mask, s_wlast, s_list);
        __syncthreads();            // the staged batch and the per-wave slots are reused by the next tile
    }
}

// Feedback publication (msgs_view_t.feedback_tag): one wave sums the D_trav accumulators and writes
// {D_trav, tag | n_open, DA | DB, D | ticket} into words 4..7 of the forward's pinned status block (the last word last).
__global__ __launch_bounds__(64) void forward_feedback_kernel(const unsigned long long* __restrict__ dtrav,
                                                              const SlabHeader* __restrict__ hdr, int slab_mode,
                                                              int64_t D_host, const uint32_t* __restrict__ D_dev, uint32_t tag,
                                                              uint64_t ticket, volatile uint64_t* __restrict__ host) {
    static_assert(DTRAV_SLOTS == 64, "one accumulator per lane");
    unsigned long long acc = dtrav[threadIdx.x];
    for (int off = 32; off > 0; off >>= 1)
        acc += ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(acc >> 32), off) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)acc, off);
    if (threadIdx.x == 0) {
        const uint64_t D = D_dev ? (uint64_t)*D_dev : (uint64_t)D_host;
        const bool overflow = slab_mode && hdr->pad0 != 0u;
        host[4] = (uint64_t)acc | (overflow ? (1ull << 63) : 0ull);
        host[5] = (uint64_t)tag | ((uint64_t)(slab_mode ? hdr->n_open : 0xFFFFFFFFu) << 32);
        host[6] = slab_mode ? ((uint64_t)hdr->DA | ((uint64_t)hdr->DB << 32)) : 0ull;
        __threadfence_system();
        host[7] = (D & 0xFFFFFFFFFFull) | ((ticket & 0xFFFFFFull) << 40);
    }
}

// Can record e of the staged batch reach the SB x SB sub-block whose first pixel is (bx0, by0)?  The exact alpha >= 1/255
// level-set test of the fine-grained kernels, forward and backward alike (s_r0 holds the cross term doubled).
template <int SB>
__device__ __forceinline__ bool fine_hit(const float4* s_r0, const float4* s_r1, const float* s_tau, int e, float bx0, float by0) {
    const float4 r0 = s_r0[e];
    const float C = s_r1[e].x, tau2 = s_tau[e];
    return !(tau2 > -1.0e38f) ||
           levelset_hits_rect(r0.x, r0.y, r0.z, 0.5f * r0.w, C, tau2, bx0, bx0 + (float)(SB - 1), by0, by0 + (float)(SB - 1));
}
// Fine-grained variant for FEW tiles (low pyramid levels): one wave64 per 4x4 pixel sub-block (lanes 0..15) — sixteen per tile —
// in workgroups of WAVES waves, G = 16 / WAVES workgroups per tile.  With fewer than ~300 tiles the quadrant kernel is latency-bound
// — one wave per SIMD at best, and a pixel's list is inherently sequential — so its time is the length of the longest per-wave entry
// chain; a 4x4 block with its own exact hit list shortens that chain (an entry reaches it far less often than an 8x8 quadrant) at
// the price of idle lanes, which are free in that regime.  Round 3: (i) the sixteen waves of a tile used to share ONE workgroup,
// i.e. one CU did a whole tile's work while at 135 / 40 / 12 / 2 tiles most CUs had none; the launch now splits a tile over G
// workgroups (every one stages the tile's list for itself: redundant reads of a few MB against idle CUs) so that tiles x G fills
// the chip; (ii) every wave classifies the batch against its OWN block and compacts in the same pass (lanes = records) — no mask
// array, one barrier less per batch; (iii) the next batch's records travel in registers while the current one is walked.
// Same arithmetic per pixel in the same order: results are bit-identical to blend_forward_kernel.
// SB = side of the sub-block a wave owns: 4 (lanes 0..15, sixteen sub-blocks per tile) or 2 (lanes 0..3, sixty-four per tile — the
// entry chain of a wave is what bounds this regime, and a 2x2 block is reached by fewer entries still; the list is staged and
// classified per workgroup as before, so the waves per workgroup grow with the sub-block count).
template <int WAVES, int SB = 4>
__global__ __launch_bounds__(64 * WAVES) void blend_forward_fine_kernel(ViewParams vp, const GaussRec* __restrict__ rec,
                                                            const uint32_t* __restrict__ ids,
                                                            const uint2* __restrict__ ranges,
                                                            float* __restrict__ out_color,
                                                            float* __restrict__ out_ps,
                                                            float* __restrict__ out_depth,
                                                            float* __restrict__ final_T,
                                                            uint32_t* __restrict__ n_contrib,
                                                            uint4* __restrict__ clear_ptr, size_t clear_n16,
                                                            uint32_t* __restrict__ order_flag) {
    constexpr int PER_ROW = TILE / SB, NSB = PER_ROW * PER_ROW, LANES = SB * SB;
    constexpr int T = 64 * WAVES, G = NSB / WAVES;
    constexpr int R = (BATCH + T - 1) / T;               // records a thread stages per batch
    __shared__ float4 s_r0[BATCH + 1], s_r1[BATCH + 1], s_r2[BATCH + 1];     // slot BATCH: the sentinel record
    __shared__ float s_tau[BATCH];                                           // (s_r2.w carries the sign-test bound)
    __shared__ __attribute__((aligned(16))) uint32_t s_list[WAVES][BATCH + LIST_PAD];
    clear_slice(clear_ptr, clear_n16);
    if (threadIdx.x == 0) {
        write_sentinel_record(s_r0, s_r1, s_r2);          // ordered by the first barrier of the batch loop
        if (blockIdx.x == 0 && order_flag) *order_flag = 0u;      // (no backward launch order in this regime)
    }
    const int tile = blockIdx.x / G, grp = blockIdx.x % G;
    const int tx = tile % vp.gx, ty = tile / vp.gx;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int sb = grp * WAVES + w;                       // this wave's SB x SB sub-block of the tile
    const int px = tx * TILE + (sb % PER_ROW) * SB + (lane % SB);
    const int py = ty * TILE + (sb / PER_ROW) * SB + ((lane / SB) % SB);
    const bool inside = lane < LANES && px < vp.W && py < vp.H;  // the other lanes idle: this variant buys latency, not throughput
    const float pxf = (float)px, pyf = (float)py;
    const float bx0 = (float)(tx * TILE + (sb % PER_ROW) * SB), by0 = (float)(ty * TILE + (sb / PER_ROW) * SB);
    const uint2 range = ranges[tile];
    const int len = (int)(range.y - range.x);
    const uint64_t lt_mask = (1ull << lane) - 1ull;

    FwdPix st = {1.0f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t last = 0, walked = 0;
    uint64_t alive = __builtin_amdgcn_ballot_w64(inside);

    float4 p0[R], p1[R], p2[R];
    auto fetch = [&](int base) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int e = tid + k * T;
            if (e < BATCH && base + e < len) {
                const uint32_t id = ids[range.x + base + e];
                p0[k] = rec[id].r0; p1[k] = rec[id].r1; p2[k] = rec[id].r2;
            }
        }
    };
    fetch(0);
    for (int base = 0; base < len; base += BATCH) {
        if (__syncthreads_and(alive == 0)) break;    // barrier also protects the LDS batch
        const int n = min(BATCH, len - base);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int e = tid + k * T;
            if (e < n) { s_r0[e] = doubled_w(p0[k]); s_r1[e] = p1[k]; s_r2[e] = with_bound(p2[k], p1[k].y); s_tau[e] = p2[k].w; }
        }
        fetch(base + BATCH);
        __syncthreads();
        // classification against this wave's block and compaction in one pass; the list holds BYTE offsets of the records
        int cnt = 0;
#pragma unroll
        for (int c = 0; c < BATCH / 64; ++c) {
            const int e = c * 64 + lane;
            const bool hit = e < n && fine_hit<SB>(s_r0, s_r1, s_tau, e, bx0, by0);
            const uint64_t b = __ballot(hit);
            if (hit) s_list[w][cnt + __popcll(b & lt_mask)] = (uint32_t)(e << 4);
            cnt += __popcll(b);
        }
        pad_list(s_list[w], cnt, lane);
        const uint32_t last_off = forward_walk(s_list[w], cnt, s_r0, s_r1, s_r2, pxf, pyf, st, alive, walked);
        if (last_off != 0xFFFFFFFFu) last = (uint32_t)base + (last_off >> 4) + 1u;   // once per batch, not per pair
    }
    forward_store(st, last, inside, px, py, vp, out_color, out_ps, out_depth, final_T, n_contrib);
}

// ---------------------------------------------------------------------------------------------
// K7
// ---------------------------------------------------------------------------------------------
// 64 lanes x 9 partial sums -> ONE value per lane holding a 16-lane-row total, hand-scheduled DPP (the backward's
// time is its VALU instruction count; this is 21 instructions against 34 for selects + quad_perm exchanges):
//   * v0..v7 are reduce-scattered 8 -> 4 -> 2 -> 1 values per lane: across the half rows (row_ror:8) and across
//     neighbouring quads (row_half_mirror) the "keep mine / add the partner's" choice is the DPP bank mask — a bank is
//     a quad of lanes, so a second, bank-masked add overwrites the half of the lanes that keep the other operand and no
//     select is needed; only the last level (lane parity inside a quad) takes the two selects.
//   * v8 is all-reduced inside the row (4 adds) and rides on the lanes whose bit 1 is set, which would otherwise hold a
//     duplicate of their lane ^ 2 neighbour.
// Result: lane l holds the row total of component comp(l) = 4*((l>>3)&1) + 2*((l>>2)&1) + (l&1) when (l & 2) == 0, and
// the row total of component 8 when (l & 2) != 0.  The caller adds the four rows.
// All hazards (VALU write -> DPP read needs two wait states) are resolved by the instruction order inside the block;
// the leading s_nop covers whatever the compiler scheduled right before it.
template <class A> struct BwdSumsT { A v0, v1, v2, v3, v4, v5, v6, v7, v8; };
using BwdSums = BwdSumsT<float>;
// Depth variant (ten sums, the tenth = sum alpha T dL/dD): v0..v7 as above; v8 and v9 share the lanes whose bit 1 is set —
// the first exchange (lane parity) sends v9 from even lanes and v8 from odd ones, so the even lanes all-reduce v8 and the odd
// lanes v9 with the same three row steps that follow.  Two selects more than the nine-sum block, still one value per lane:
// lane l holds component comp(l) for (l & 2) == 0, component 8 + (l & 1) otherwise.
// The two blocks differ in the leading selects and the first t8 step only; the rest of the text is shared.
#define ROW_SCATTER_HALF_ROWS                                                             \
    "v_add_f32_dpp %[a0], %[v0], %[v0] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"          \
    "v_add_f32_dpp %[a1], %[v1], %[v1] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"          \
    "v_add_f32_dpp %[a2], %[v2], %[v2] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"          \
    "v_add_f32_dpp %[a3], %[v3], %[v3] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"          \
    "v_add_f32_dpp %[a0], %[v4], %[v4] row_ror:8 row_mask:0xf bank_mask:0xc\n\t"          \
    "v_add_f32_dpp %[a1], %[v5], %[v5] row_ror:8 row_mask:0xf bank_mask:0xc\n\t"          \
    "v_add_f32_dpp %[a2], %[v6], %[v6] row_ror:8 row_mask:0xf bank_mask:0xc\n\t"          \
    "v_add_f32_dpp %[a3], %[v7], %[v7] row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
#define ROW_SCATTER_QUADS_AND_LANES                                                       \
    "v_add_f32_dpp %[b0], %[a0], %[a0] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"    \
    "v_add_f32_dpp %[b1], %[a1], %[a1] row_half_mirror row_mask:0xf bank_mask:0xf\n\t"    \
    "v_add_f32_dpp %[b0], %[a2], %[a2] row_half_mirror row_mask:0xf bank_mask:0xa\n\t"    \
    "v_add_f32_dpp %[b1], %[a3], %[a3] row_half_mirror row_mask:0xf bank_mask:0xa\n\t"    \
    "v_add_f32_dpp %[t8], %[t8], %[t8] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t" \
    "v_cndmask_b32_e64 %[send], %[b1], %[b0], %[odd]\n\t"                                 \
    "v_cndmask_b32_e64 %[keep], %[b0], %[b1], %[odd]\n\t"                                 \
    "v_add_f32_dpp %[t8], %[t8], %[t8] row_ror:4 row_mask:0xf bank_mask:0xf\n\t"          \
    "v_add_f32_dpp %[c], %[send], %[keep] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t" \
    "s_nop 0\n\t"                                                                         \
    "v_add_f32_dpp %[t8], %[t8], %[t8] row_ror:8 row_mask:0xf bank_mask:0xf\n\t"          \
    "v_add_f32_dpp %[c], %[c], %[c] quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"   \
    "v_cndmask_b32_e64 %[c], %[c], %[t8], %[bit1]"
#define ROW_SCATTER_OUTS                                                                                      \
    [a0] "=&v"(a0), [a1] "=&v"(a1), [a2] "=&v"(a2), [a3] "=&v"(a3), [b0] "=&v"(b0), [b1] "=&v"(b1),           \
    [t8] "=&v"(t8), [keep] "=&v"(keep), [send] "=&v"(send), [c] "=&v"(c)
#define ROW_SCATTER_INS                                                                                       \
    [v0] "v"(v.v0), [v1] "v"(v.v1), [v2] "v"(v.v2), [v3] "v"(v.v3), [v4] "v"(v.v4), [v5] "v"(v.v5),           \
    [v6] "v"(v.v6), [v7] "v"(v.v7), [v8] "v"(v.v8)
template <bool DEPTH>
__device__ __forceinline__ float row_reduce_scatter(const BwdSums& v, float v9) {
    float a0, a1, a2, a3, b0, b1, t8, keep, send, c;
    const uint64_t odd = 0xAAAAAAAAAAAAAAAAull, bit1 = 0xCCCCCCCCCCCCCCCCull;
    if constexpr (DEPTH) {
        float k89, s89;
        asm volatile(
            "s_nop 1\n\t"
            "v_cndmask_b32_e64 %[s89], %[v9], %[v8], %[odd]\n\t"
            "v_cndmask_b32_e64 %[k89], %[v8], %[v9], %[odd]\n\t"
            ROW_SCATTER_HALF_ROWS
            "v_add_f32_dpp %[t8], %[s89], %[k89] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
            ROW_SCATTER_QUADS_AND_LANES
            : ROW_SCATTER_OUTS, [k89] "=&v"(k89), [s89] "=&v"(s89)
            : ROW_SCATTER_INS, [v9] "v"(v9), [odd] "s"(odd), [bit1] "s"(bit1));
    } else {
        asm volatile(
            "s_nop 1\n\t"
            ROW_SCATTER_HALF_ROWS
            "v_add_f32_dpp %[t8], %[v8], %[v8] quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
            ROW_SCATTER_QUADS_AND_LANES
            : ROW_SCATTER_OUTS
            : ROW_SCATTER_INS, [odd] "s"(odd), [bit1] "s"(bit1));
    }
    return c;
}
#undef ROW_SCATTER_HALF_ROWS
#undef ROW_SCATTER_QUADS_AND_LANES
#undef ROW_SCATTER_OUTS
#undef ROW_SCATTER_INS
// component (0..8; depth: 0..9) that lane l of a row delivers after row_reduce_scatter
template <bool DEPTH>
__device__ __forceinline__ uint32_t row_reduce_component(int l) {
    return (l & 2) ? (DEPTH ? 8u + (uint32_t)(l & 1) : 8u) : (uint32_t)(4 * ((l >> 3) & 1) + 2 * ((l >> 2) & 1) + (l & 1));
}
// the nine lanes that issue the per-entry atomics (depth: ten, lane 3 delivers component 9); lane l adds to record slot
// row_reduce_component<DEPTH>(l).  (A macro: as a function the predicate is simplified on its own before it is inlined, and the
// operands of one s_or_b64 then come out in another order in some of the kernels.)
#define IS_ATOMIC_LANE(DEPTH, lane) \
    ((DEPTH) ? (lane) < 16 && (!((lane) & 2) || (lane) == 2 || (lane) == 3) : (lane) < 16 && (!((lane) & 2) || (lane) == 2))
// One reduction per (wave, entry): rows by DPP, the four rows by `cross_row` (v_permlane16/32_swap in the latency-bound
// four-waves kernel, where they beat ds_bpermute — profiles/r1_notes.md; ds_bpermute in the one-wave-per-tile kernel; nothing in
// the fine-grained kernel, whose pixels live in row 0), scalar record address from the wave-uniform id (`id()`: read from LDS
// here, behind the reduction), ONE atomic instruction from the nine (depth: ten) lanes.
template <bool DEPTH, class CrossRow, class Id>
__device__ __forceinline__ void reduce_and_add(const BwdSums& v, float v9, CrossRow cross_row, Id id,
                                               grad_acc_t* __restrict__ grad_rec, bool alane, uint32_t aoff) {
    const float outv = cross_row(row_reduce_scatter<DEPTH>(v, v9));
    const uint32_t gid = __builtin_amdgcn_readfirstlane(id());
    grad_acc_t* gdst = grad_rec + (size_t)gid * GRAD_REC_FLOATS;
    if (alane) unsafeAtomicAdd(gdst + aoff, (grad_acc_t)outv);
}
// Per-pixel backward state and the per-(pixel, Gaussian) step — shared by the three backward kernels.  Same arithmetic per
// pixel in the same order in all of them.
// DEPTH (the depth variants, msgs_backward_with_depth): the depth map is a fourth channel with colour z and no background —
// its share z dL/dD enters g_i (so S and dL/dalpha), and a tenth sum alpha T dL/dD = dL/dz goes to record slot 9.
struct BwdPix {
    float T, S, dL0, dL1, dL2, dLd;  // S: see bwd_pix_start_S; dLd: dL/dD (depth variant)
    uint32_t last;
};
// S = sum_c dL/dC_c * (colour composited BEHIND the current entry, background included, normalised by the
// transmittance in front of it).  dL/dalpha_i = T_i (g_i - S_i) with g_i = sum_c dL/dC_c colour_i,c, and
// S_{i-1} = S_i + alpha_i (g_i - S_i): the three per-channel recurrences of the textbook form collapse into one
// scalar, and starting it at bg . dL/dC absorbs the separate background term (-T_final bg.dL / (1 - alpha_i)).
template <bool ALPHA>
__device__ __forceinline__ void bwd_pix_start_S(BwdPix& st, const ViewParams& vp, bool inside, size_t pix,
                                                const float* dL_dalpha) {
    st.S = vp.bg[0] * st.dL0 + vp.bg[1] * st.dL1 + vp.bg[2] * st.dL2;
    if constexpr (ALPHA) { if (inside) st.S -= dL_dalpha[pix]; }     // the alpha map's share (lanes outside the image do not read)
}
// First part of the step: the pair's monomials and its unclamped alpha.
struct PairAlpha { PairEval ev; float a_raw; };
__device__ __forceinline__ PairAlpha pair_alpha(const float4& r0, const float4& r1, float dx, float dy) {
    PairAlpha a;
    a.ev = eval_pair(r0.z, r0.w, r1.x, r1.y, dx, dy);
    a.a_raw = __builtin_amdgcn_exp2f(a.ev.p);
    return a;
}
// The lanes the pair counts for, as a SCALAR mask: three ballots of direct comparisons and scalar ANDs (a ballot of a derived
// bool costs two VALU instructions).  pos = the entry's 0-based position in the tile list; `last` = the position behind the
// last entry the pixel blended; bound: sign_test_bound.
__device__ __forceinline__ uint64_t pair_valid(const PairAlpha& a, uint32_t pos, uint32_t last, float bound) {
    return __builtin_amdgcn_ballot_w64(pos < last) & __builtin_amdgcn_ballot_w64(a.ev.p <= bound) &
           __builtin_amdgcn_ballot_w64(a.a_raw >= ALPHA_MIN);   // alpha = min(0.99, a_raw) >= 1/255  <=>  a_raw >= 1/255
}
// Last part: the T and S recurrences of the pixel; returns q = alpha_raw dL/dalpha and dch = alpha T (the weight of dL/dC in
// the colour sums).  z(): the entry's view depth (DEPTH only), read where g_i is formed.
struct PairGrad { float q, dch; };
template <bool DEPTH, class Z>
__device__ __forceinline__ PairGrad pair_grad(BwdPix& s, const PairAlpha& a, uint64_t validm, const float4& r1, float cb, Z z) {
    const bool valid = __builtin_amdgcn_inverse_ballot_w64(validm);
    // ONE select masks the lane: with a_m = 0 everything downstream is the identity (alpha 0, 1/(1-0) = 1 exactly,
    // T unchanged, zero contributions), so neither alpha nor T needs a select of its own
    const float a_m = valid ? a.a_raw : 0.0f;
    const float alpha_m = fminf(0.99f, a_m);
    const float inv = __builtin_amdgcn_rcpf(1.0f - alpha_m);
    const float Tn = s.T * inv;
    s.T = Tn;
    PairGrad g;
    g.dch = alpha_m * Tn;
    float gi = fmaf(cb, s.dL2, fmaf(r1.w, s.dL1, r1.z * s.dL0));
    if constexpr (DEPTH) gi = fmaf(z(), s.dLd, gi);
    const float sm = gi - s.S;
    const float dL_dalpha = sm * Tn;
    s.S = fmaf(alpha_m, sm, s.S);
    g.q = a_m * dL_dalpha;                                    // Q6: gradient passes the 0.99 clamp
    return g;
}
// The walk over one wave's compacted entry list (back to front) — shared by the four-waves-per-tile kernel (CROSS_ROW: the
// pixels of an 8x8 quadrant fill the wave, the four 16-lane rows are added with v_permlane16/32_swap) and the fine-grained
// kernel (the sixteen pixels of a 4x4 sub-block live in row 0: the row reduction is the whole reduction).
template <bool CROSS_ROW, bool DEPTH = false>
__device__ __forceinline__ void backward_walk(const uint16_t* lp, int cnt, int base, const float4* s_r0, const float4* s_r1,
                                              const float2* s_b, const uint32_t* s_id, float pxf, float pyf, BwdPix& st,
                                              bool alane, uint32_t aoff, grad_acc_t* __restrict__ grad_rec,
                                              const float* s_z = nullptr) {
    for (int j = cnt - 1; j >= 0; --j) {
        const int e = lp[j];
        const float4 r0 = s_r0[e], r1 = s_r1[e];
        const float2 bl = s_b[e];                              // {blue, sign_test_bound}
        const float dx = r0.x - pxf, dy = r0.y - pyf;
        const PairAlpha a = pair_alpha(r0, r1, dx, dy);
        const uint64_t validm = pair_valid(a, (uint32_t)(base + e), st.last, bl.y);
        if (validm == 0) continue;
        const PairGrad g = pair_grad<DEPTH>(st, a, validm, r1, bl.x, [=] { return s_z[e]; });
        const float q = g.q, dch = g.dch;
        const BwdSums v = {q * dx, q * dy, q * a.ev.dxx, q * a.ev.dxy, q * a.ev.dyy, q, dch * st.dL0, dch * st.dL1, dch * st.dL2};
        reduce_and_add<DEPTH>(v, DEPTH ? dch * st.dLd : 0.f, [](float x) { return CROSS_ROW ? cross_row_allreduce(x) : x; },
                              [=] { return s_id[e]; }, grad_rec, alane, aoff);
    }
}

// Gradient record components accumulated here (scaled to dL/d{mean2D, conic, opacity} per Gaussian
// in preprocess_backward_kernel):
//   [0] sum q dx  [1] sum q dy  [2] sum q dx dx   [3] sum q dx dy   [4] sum q dy dy   [5] sum q
//   [6..8] sum alpha T dL/dC_c                     with q = alpha_raw * dL/dalpha
//   [9]    sum alpha T dL/dD  (= dL/dz; depth variant only)
// CH = 3: the colour backward (the default); CH = 4: colour + depth (msgs_backward_with_depth), dL_ddepth [H,W] read
// ALPHA (msgs_backward_with_alpha): a gradient G = dL/dA of the alpha map A = 1 - T_final arrives in dL_dalpha [H,W]; it adds
// G T_final / (1 - alpha_i) to dL/dalpha_i, which is the background term with -G in the place of bg . dL/dC: an inside pixel
// starts S at bg . dL/dC - G.  Nothing else changes (no new sum, no new record slot); ALPHA = false never reads the pointer.
template <int CH, bool ALPHA = false>
__global__ __launch_bounds__(256) void blend_backward_kernel(ViewParams vp, const GaussRec* __restrict__ rec,
                                                             const uint32_t* __restrict__ ids,
                                                             const uint2* __restrict__ ranges,
                                                             const float* __restrict__ final_T,
                                                             const uint32_t* __restrict__ n_contrib,
                                                             const float* __restrict__ dL_dcolor,
                                                             grad_acc_t* __restrict__ grad_rec,
                                                             const float* __restrict__ dL_ddepth,
                                                             const float* __restrict__ dL_dalpha) {
    constexpr bool DEPTH = CH == 4;
    __shared__ float4 s_r0[BATCH], s_r1[BATCH];
    __shared__ float2 s_b[BATCH];                          // {blue, sign_test_bound}
    __shared__ float s_z[DEPTH ? BATCH : 1];               // view depth (depth variant)
    __shared__ uint32_t s_id[BATCH];
    __shared__ uint32_t s_mask[BATCH];
    __shared__ uint16_t s_list[4][BATCH];
    __shared__ uint32_t s_wmax[4];

    const int num_tiles = vp.gx * vp.gy;
    const int tile = swizzled_tile(blockIdx.x, num_tiles);
    const int tx = tile % vp.gx, ty = tile / vp.gx;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int px = tx * TILE + (w & 1) * 8 + (lane & 7);
    const int py = ty * TILE + (w >> 1) * 8 + (lane >> 3);
    const bool inside = px < vp.W && py < vp.H;
    const float pxf = (float)px, pyf = (float)py;
    const float tx0 = (float)(tx * TILE), ty0 = (float)(ty * TILE);
    const uint2 range = ranges[tile];
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    const size_t N = (size_t)vp.W * vp.H;
    const size_t pix = (size_t)py * vp.W + px;

    BwdPix st;
    st.T = inside ? final_T[pix] : 1.0f;
    st.last = inside ? n_contrib[pix] : 0u;
    st.dL0 = st.dL1 = st.dL2 = 0.f;
    if (inside) { st.dL0 = dL_dcolor[pix]; st.dL1 = dL_dcolor[N + pix]; st.dL2 = dL_dcolor[2 * N + pix]; }
    st.dLd = (DEPTH && inside) ? dL_ddepth[pix] : 0.f;

    const uint32_t wave_last = wave_max_u32(st.last);
    if (lane == 0) s_wmax[w] = wave_last;
    __syncthreads();
    const uint32_t tile_last = max(max(s_wmax[0], s_wmax[1]), max(s_wmax[2], s_wmax[3]));

    bwd_pix_start_S<ALPHA>(st, vp, inside, pix, dL_dalpha);
    const bool alane = IS_ATOMIC_LANE(DEPTH, lane);
    const uint32_t aoff = row_reduce_component<DEPTH>(lane);

    const int nb = ((int)tile_last + BATCH - 1) / BATCH;
    for (int b = nb - 1; b >= 0; --b) {
        __syncthreads();                              // previous batch fully consumed (and flushed)
        const int base = b * BATCH;
        const int n = min(BATCH, (int)tile_last - base);
        if (tid < n) {
            const uint32_t id = ids[range.x + base + tid];
            const float4 r0 = rec[id].r0, r1 = rec[id].r1;
            const float4 r2 = rec[id].r2;
            s_r0[tid] = doubled_w(r0); s_r1[tid] = r1; s_b[tid] = make_float2(r2.x, sign_test_bound(r1.y)); s_id[tid] = id;
            if constexpr (DEPTH) s_z[tid] = r2.y;
            s_mask[tid] = quadrant_mask(r0, r1.x, r2.w, tx0, ty0);
        }
        __syncthreads();
        int cnt = 0;
#pragma unroll
        for (int c = 0; c < BATCH / 64; ++c) {
            const int e = c * 64 + lane;
            const bool hit = e < n && (uint32_t)(base + e) < wave_last && ((s_mask[e] >> w) & 1u);
            const uint64_t bal = __ballot(hit);
            if (hit) s_list[w][cnt + __popcll(bal & lt_mask)] = (uint16_t)e;
            cnt += __popcll(bal);
        }
        backward_walk<true, DEPTH>(s_list[w], cnt, base, s_r0, s_r1, s_b, s_id, pxf, pyf, st, alane, aoff, grad_rec, s_z);
    }
}

// Fine-grained variant for FEW tiles (low pyramid levels), the counterpart of blend_forward_fine_kernel: one wave64 per 4x4 pixel
// sub-block (lanes 0..15), WAVES per workgroup, 16 / WAVES workgroups per tile; same per-pixel arithmetic in the same order as
// blend_backward_kernel; one atomic per (sub-block, Gaussian, component).  A workgroup walks the tile's list back from the last
// entry ITS pixels blended.
template <int WAVES, int SB = 4, int CH = 3, bool ALPHA = false>
__global__ __launch_bounds__(64 * WAVES) void blend_backward_fine_kernel(ViewParams vp, const GaussRec* __restrict__ rec,
                                                             const uint32_t* __restrict__ ids,
                                                             const uint2* __restrict__ ranges,
                                                             const float* __restrict__ final_T,
                                                             const uint32_t* __restrict__ n_contrib,
                                                             const float* __restrict__ dL_dcolor,
                                                             grad_acc_t* __restrict__ grad_rec,
                                                             const float* __restrict__ dL_ddepth,
                                                             const float* __restrict__ dL_dalpha) {
    constexpr bool DEPTH = CH == 4;
    constexpr int PER_ROW = TILE / SB, NSB = PER_ROW * PER_ROW, LANES = SB * SB;
    constexpr int T = 64 * WAVES, G = NSB / WAVES;
    constexpr int R = (BATCH + T - 1) / T;               // records a thread stages per batch
    __shared__ float4 s_r0[BATCH], s_r1[BATCH];
    __shared__ float2 s_b[BATCH];                          // {blue, sign_test_bound}
    __shared__ float s_z[DEPTH ? BATCH : 1];               // view depth (depth variant)
    __shared__ float s_tau[BATCH];
    __shared__ uint32_t s_id[BATCH];
    __shared__ uint16_t s_list[WAVES][BATCH];
    __shared__ uint32_t s_wmax[WAVES];

    const int tile = blockIdx.x / G, grp = blockIdx.x % G;
    const int tx = tile % vp.gx, ty = tile / vp.gx;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int sb = grp * WAVES + w;                       // this wave's SB x SB sub-block of the tile
    const int px = tx * TILE + (sb % PER_ROW) * SB + (lane % SB);
    const int py = ty * TILE + (sb / PER_ROW) * SB + ((lane / SB) % SB);
    const bool inside = lane < LANES && px < vp.W && py < vp.H;  // the other lanes idle (see blend_forward_fine_kernel)
    const float pxf = (float)px, pyf = (float)py;
    const float bx0 = (float)(tx * TILE + (sb % PER_ROW) * SB), by0 = (float)(ty * TILE + (sb / PER_ROW) * SB);
    const uint2 range = ranges[tile];
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    const size_t N = (size_t)vp.W * vp.H;
    const size_t pix = (size_t)py * vp.W + px;

    BwdPix st;
    st.T = inside ? final_T[pix] : 1.0f;
    st.last = inside ? n_contrib[pix] : 0u;
    st.dL0 = st.dL1 = st.dL2 = 0.f;
    if (inside) { st.dL0 = dL_dcolor[pix]; st.dL1 = dL_dcolor[N + pix]; st.dL2 = dL_dcolor[2 * N + pix]; }
    st.dLd = (DEPTH && inside) ? dL_ddepth[pix] : 0.f;

    const uint32_t wave_last = wave_max_u32(st.last);
    if (lane == 0) s_wmax[w] = wave_last;
    __syncthreads();
    uint32_t grp_last = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) grp_last = max(grp_last, s_wmax[k]);

    bwd_pix_start_S<ALPHA>(st, vp, inside, pix, dL_dalpha);
    const bool alane = IS_ATOMIC_LANE(DEPTH, lane);
    const uint32_t aoff = row_reduce_component<DEPTH>(lane);

    const int nb = ((int)grp_last + BATCH - 1) / BATCH;
    // register prefetch of the next (nearer) batch, as in blend_forward_fine_kernel
    float4 p0[R], p1[R], p2[R];
    uint32_t pid[R];
    auto fetch = [&](int base) {
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int e = tid + k * T;
            if (e < BATCH && base + e < (int)grp_last) {
                pid[k] = ids[range.x + base + e];
                p0[k] = rec[pid[k]].r0; p1[k] = rec[pid[k]].r1; p2[k] = rec[pid[k]].r2;
            }
        }
    };
    if (nb > 0) fetch((nb - 1) * BATCH);
    for (int b = nb - 1; b >= 0; --b) {
        __syncthreads();                              // previous batch fully consumed (and flushed)
        const int base = b * BATCH;
        const int n = min(BATCH, (int)grp_last - base);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int e = tid + k * T;
            if (e < n) {
                s_r0[e] = doubled_w(p0[k]); s_r1[e] = p1[k]; s_b[e] = make_float2(p2[k].x, sign_test_bound(p1[k].y)); s_id[e] = pid[k];
                s_tau[e] = p2[k].w;
                if constexpr (DEPTH) s_z[e] = p2[k].y;
            }
        }
        if (b > 0) fetch(base - BATCH);
        __syncthreads();
        // classification against this wave's block and compaction in one pass
        int cnt = 0;
#pragma unroll
        for (int c = 0; c < BATCH / 64; ++c) {
            const int e = c * 64 + lane;
            const bool hit = e < n && (uint32_t)(base + e) < wave_last && fine_hit<SB>(s_r0, s_r1, s_tau, e, bx0, by0);
            const uint64_t bal = __ballot(hit);
            if (hit) s_list[w][cnt + __popcll(bal & lt_mask)] = (uint16_t)e;
            cnt += __popcll(bal);
        }
        backward_walk<false, DEPTH>(s_list[w], cnt, base, s_r0, s_r1, s_b, s_id, pxf, pyf, st, alane, aoff, grad_rec, s_z);
    }
}

// ---------------------------------------------------------------------------------------------
// one-wave-per-tile backward: ONE wave64 per tile, four pixels per lane (lane l owns pixel (l & 7, l >> 3) of each of the
// four 8x8 quadrants).  Everything that is uniform over the tile — record fetch from LDS, loop control,
// the 64-lane reduction and the atomics — is paid once per (tile, Gaussian) instead of
// once per (quadrant, Gaussian); the quadrant hit mask becomes a wave-uniform branch per quadrant; there is
// no workgroup barrier (a single wave owns the tile) and the next batch of 64 records is prefetched into
// registers while the current one is consumed.  The four per-quadrant evaluations are independent, which
// gives the scheduler four-way ILP.
// ---------------------------------------------------------------------------------------------
constexpr int WB = 64;   // records per batch (one per lane)

__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one (pixel, Gaussian) backward step accumulated into the per-lane partial sums; returns the lanes that contributed as a
// scalar mask (the caller only needs "any lane?")
// (no wave-level early-out here: every ballot-driven branch is a VALU -> SALU -> branch round trip, and the
// quadrant hit masks already removed the quadrants the record cannot touch)
// (DEPTH: z is the entry's view depth and v9 the tenth sum, see BwdPix)
template <bool DEPTH>
__device__ __forceinline__ uint64_t bwd_quad_step(BwdPix& s, BwdSums& v, float* v9, const float4& r0, const float4& r1, float cb,
                                                  float bound, float dx, float dy, uint32_t pos0, float z) {
    const PairAlpha a = pair_alpha(r0, r1, dx, dy);
    const uint64_t validm = pair_valid(a, pos0, s.last, bound);
    const PairGrad g = pair_grad<DEPTH>(s, a, validm, r1, cb, [=] { return z; });
    v.v0 = fmaf(g.q, dx, v.v0); v.v1 = fmaf(g.q, dy, v.v1);
    v.v2 = fmaf(g.q, a.ev.dxx, v.v2); v.v3 = fmaf(g.q, a.ev.dxy, v.v3); v.v4 = fmaf(g.q, a.ev.dyy, v.v4);
    v.v5 += g.q;
    v.v6 = fmaf(g.dch, s.dL0, v.v6); v.v7 = fmaf(g.dch, s.dL1, v.v7); v.v8 = fmaf(g.dch, s.dL2, v.v8);
    if constexpr (DEPTH) *v9 = fmaf(g.dch, s.dLd, *v9);
    return validm;
}

#if defined(MSGS_TRACE_TILES)
// tool build (tools/trace_tiles.sh): per-tile {start, end (s_memrealtime, 100 MHz), HW_ID, XCC_ID, tile, traversal length} of the
// one-wave-per-tile backward, for the occupancy timeline in profiles/; never part of the product library
__device__ unsigned long long* g_tile_trace = nullptr;
__global__ void trace_set_kernel(unsigned long long* p) { g_tile_trace = p; }
#endif

// COUNT = true (diagnostic replica, msgs_blend_lane_stats): nothing is reduced or written; grad_out receives four counters —
// (tile, entry) visits, (quadrant, entry) evaluations (each 64 lanes), lanes that contributed, visits with a contribution.
// (The verification mode — msgs_set_deterministic — does not run this kernel: literal.hip restates the reference's loop.)
// CH = 4 (colour + depth): the depth channel of backward_walk, with z in the free slot of s_bi.  (tools/isa_mix.py finds the
// <false, 3, false> instantiation by the mangled-name fragment `blend_backward_tile_kernelILb0ELi3ELb0E`.)
// ALPHA: see blend_backward_kernel.
template <bool COUNT = false, int CH = 3, bool ALPHA = false>
__global__ __launch_bounds__(64) void blend_backward_tile_kernel(ViewParams vp, const GaussRec* __restrict__ rec,
                                                                 const uint32_t* __restrict__ ids,
                                                                 const uint2* __restrict__ ranges,
                                                                 const float* __restrict__ final_T,
                                                                 const uint32_t* __restrict__ n_contrib,
                                                                 const float* __restrict__ dL_dcolor,
                                                                 void* __restrict__ grad_out,
                                                                 const uint32_t* __restrict__ tile_order,
                                                                 const float* __restrict__ dL_ddepth,
                                                                 const float* __restrict__ dL_dalpha) {
    constexpr bool DEPTH = CH == 4;
    __shared__ float4 s_r0[WB], s_r1[WB];
    __shared__ float4 s_bi[WB];                            // {blue, sign_test_bound, id bits, - | depth}: 16-byte stride like s_r0 /
                                                           // s_r1, so one address register serves every LDS read of an entry
    const int num_tiles = vp.gx * vp.gy;
    const int lane = threadIdx.x;
    // launch order: heaviest tiles first inside every XCD's contiguous run (launch_tile_order) when the forward left a valid
    // order behind, the plain XCD swizzle otherwise
    int tile = swizzled_tile(blockIdx.x, num_tiles);
    if (tile_order != nullptr) {
        const uint32_t flag = tile_order[num_tiles];
        if (flag == TILE_ORDER_MAGIC) tile = (int)tile_order[tile];                       // per XCD run
    }
    const int tx = tile % vp.gx, ty = tile / vp.gx;
    const int bx = tx * TILE + (lane & 7), by = ty * TILE + (lane >> 3);
    const float bxf = (float)bx, byf = (float)by;
    const float tx0 = (float)(tx * TILE), ty0 = (float)(ty * TILE);
    const uint2 range = ranges[tile];
    const size_t N = (size_t)vp.W * vp.H;

#if defined(MSGS_TRACE_TILES)
    const unsigned long long trace_t0 = __builtin_amdgcn_s_memrealtime();
#endif
    uint32_t cnt_visits = 0, cnt_steps = 0, cnt_lanes = 0, cnt_hits = 0;       // COUNT only
    BwdPix q0, q1, q2, q3;
    uint32_t ql0, ql1, ql2, ql3;                           // wave-uniform: last blended position per quadrant
    {
        auto init = [&](BwdPix& s, int qi) -> uint32_t {
            const int px = bx + (qi & 1) * 8, py = by + (qi >> 1) * 8;
            const bool inside = px < vp.W && py < vp.H;
            const size_t pix = (size_t)py * vp.W + px;
            const float Tf = inside ? final_T[pix] : 1.0f;
            s.last = inside ? n_contrib[pix] : 0u;
            // (the counting replica does not read dL/dcolor: it only enters the sums, not the validity of a lane)
            s.dL0 = (inside && !COUNT) ? dL_dcolor[pix] : 0.f;
            s.dL1 = (inside && !COUNT) ? dL_dcolor[N + pix] : 0.f;
            s.dL2 = (inside && !COUNT) ? dL_dcolor[2 * N + pix] : 0.f;
            s.dLd = (DEPTH && inside) ? dL_ddepth[pix] : 0.f;
            s.S = vp.bg[0] * s.dL0 + vp.bg[1] * s.dL1 + vp.bg[2] * s.dL2;
            if constexpr (ALPHA) { if (inside) s.S -= dL_dalpha[pix]; }
            s.T = Tf;
            return __builtin_amdgcn_readfirstlane(wave_max_u32(s.last));
        };
        ql0 = init(q0, 0); ql1 = init(q1, 1); ql2 = init(q2, 2); ql3 = init(q3, 3);
    }
    const uint32_t tile_last = max(max(ql0, ql1), max(ql2, ql3));
    const bool alane = IS_ATOMIC_LANE(DEPTH, lane);
    const uint32_t aoff = row_reduce_component<DEPTH>(lane);
    const int xrow16 = (lane ^ 16) << 2, xrow32 = (lane ^ 32) << 2;     // ds_bpermute byte addresses of the partner lanes

    const int nb = ((int)tile_last + WB - 1) / WB;
    float4 n0 = make_float4(0, 0, 0, 0), n1 = n0, n2 = n0;
    uint32_t nid = 0;
    if (nb > 0) {
        const int i0 = (nb - 1) * WB + lane;
        if (i0 < (int)tile_last) { nid = ids[range.x + i0]; n0 = rec[nid].r0; n1 = rec[nid].r1; n2 = rec[nid].r2; }
    }
    for (int b = nb - 1; b >= 0; --b) {
        const int base = b * WB;
        const int n = min(WB, (int)tile_last - base);
        wave_fence();
        s_r0[lane] = doubled_w(n0); s_r1[lane] = n1; s_bi[lane] = make_float4(n2.x, sign_test_bound(n1.y), __uint_as_float(nid), DEPTH ? n2.y : 0.f);
        // quadrant hit masks of the batch as four 64-bit ballots; a record beyond the last blended entry of a
        // quadrant cannot matter to that quadrant
        const uint32_t mymask = lane < n ? quadrant_mask(n0, n1.x, n2.w, tx0, ty0) : 0u;
        const uint32_t mypos = (uint32_t)(base + lane);
        const uint64_t h0 = __ballot((mymask & 1u) && mypos < ql0), h1 = __ballot((mymask & 2u) && mypos < ql1),
                       h2 = __ballot((mymask & 4u) && mypos < ql2), h3 = __ballot((mymask & 8u) && mypos < ql3);
        wave_fence();
        if (b > 0) {                                      // prefetch the next (nearer) batch: always full
            nid = ids[range.x + base - WB + lane];
            n0 = rec[nid].r0; n1 = rec[nid].r1; n2 = rec[nid].r2;
        }
        uint64_t todo = h0 | h1 | h2 | h3;
        while (todo) {
            const int e = 63 - __builtin_clzll(todo);     // back to front
            const uint64_t bit = 1ull << e;
            todo &= ~bit;
            const uint32_t pos0 = (uint32_t)(base + e);   // 0-based position in the tile list
            const float4 r0 = s_r0[e], r1 = s_r1[e];
            const float2 bl = *reinterpret_cast<const float2*>(&s_bi[e]);      // {blue, sign_test_bound}: one 8-byte read
            const float dx = r0.x - bxf, dy = r0.y - byf;
            BwdSums v = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            float v9 = 0.f;                                // depth variant: the tenth sum
            float* const pv9 = DEPTH ? &v9 : nullptr;
            const float z = DEPTH ? s_bi[e].w : 0.f;       // depth variant: the entry's view depth
            uint64_t any = 0;
            if constexpr (COUNT) cnt_visits += 1u;
            // the four quadrants, one list for every variant: DEPTH hands z and the tenth sum to the step, COUNT tallies its result
            if (h0 & bit) {
                const uint64_t m = bwd_quad_step<DEPTH>(q0, v, pv9, r0, r1, bl.x, bl.y, dx, dy, pos0, z);
                any |= m;
                if constexpr (COUNT) { cnt_steps += 1u; cnt_lanes += (uint32_t)__popcll(m); }
            }
            if (h1 & bit) {
                const uint64_t m = bwd_quad_step<DEPTH>(q1, v, pv9, r0, r1, bl.x, bl.y, dx - 8.0f, dy, pos0, z);
                any |= m;
                if constexpr (COUNT) { cnt_steps += 1u; cnt_lanes += (uint32_t)__popcll(m); }
            }
            if (h2 & bit) {
                const uint64_t m = bwd_quad_step<DEPTH>(q2, v, pv9, r0, r1, bl.x, bl.y, dx, dy - 8.0f, pos0, z);
                any |= m;
                if constexpr (COUNT) { cnt_steps += 1u; cnt_lanes += (uint32_t)__popcll(m); }
            }
            if (h3 & bit) {
                const uint64_t m = bwd_quad_step<DEPTH>(q3, v, pv9, r0, r1, bl.x, bl.y, dx - 8.0f, dy - 8.0f, pos0, z);
                any |= m;
                if constexpr (COUNT) { cnt_steps += 1u; cnt_lanes += (uint32_t)__popcll(m); }
            }
            if constexpr (COUNT) {
                if (any) cnt_hits += 1u;
                continue;
            }
            if (any == 0) continue;                        // no lane contributed: nothing to reduce
            // one 64-lane reduction per (tile, Gaussian), the four rows through the LDS crossbar (ds_bpermute lane ^ 16,
            // lane ^ 32: two adds on the VALU; v_permlane16/32_swap are multi-cycle there).  Lanes 0,1,4,5,8,9,12,13 then hold
            // components 0..7 and lane 2 component 8 (depth: lane 3 component 9).
            // (record id through v_readlane of a register copy and a scalar-base atomic — no 64-bit VALU multiply-add —
            //  were measured: no difference, 357..382 us for all four combinations)
            reduce_and_add<DEPTH>(v, v9, [=](float x) { return cross_row_allreduce_bperm(x, xrow16, xrow32); },
                                  [=] { return __float_as_uint(s_bi[e].z); }, (grad_acc_t*)grad_out, alane, aoff);
        }
    }
    if constexpr (COUNT) {
        if (lane == 0) {
            unsigned long long* o = (unsigned long long*)grad_out;
            atomicAdd(&o[0], (unsigned long long)cnt_visits); atomicAdd(&o[1], (unsigned long long)cnt_steps);
            atomicAdd(&o[2], (unsigned long long)cnt_lanes); atomicAdd(&o[3], (unsigned long long)cnt_hits);
        }
    }
#if defined(MSGS_TRACE_TILES)
    if (!COUNT && !DEPTH && g_tile_trace && lane == 0) {
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned long long* o = g_tile_trace + 4ull * blockIdx.x;
        o[0] = trace_t0; o[1] = __builtin_amdgcn_s_memrealtime();
        o[2] = ((unsigned long long)xcc << 32) | hw; o[3] = ((unsigned long long)tile << 32) | tile_last;
    }
#endif
}

// ---------------------------------------------------------------------------------------------
// The skeleton of the opt-in tile-list replays below.  All of them run in the four-waves-per-tile shape of blend_backward_kernel
// (one 256-thread workgroup per tile, one 8x8 quadrant per wave, whatever the tile count) and share its pixel mapping, its
// per-batch staging of the tile's records into LDS and its per-wave compacted list of the staged entries that touch the wave's
// quadrant.  A replay adds its per-pixel state, one more store per staged entry, and the walk over the compacted list.
// (blend_backward_kernel itself spells the same steps out: folded onto these helpers its registers come out in another order.)
// ---------------------------------------------------------------------------------------------
// The pixel of a lane: wave w owns quadrant (w & 1, w >> 1) of the (XCD-swizzled) tile, lane l its pixel (l & 7, l >> 3).
struct ReplayPixel {
    int tile, tx, ty, tid, w, lane, px, py;
    bool inside;
    size_t pix;                                              // py * W + px (an index only where inside)
};
__device__ __forceinline__ ReplayPixel replay_pixel(const ViewParams& vp) {
    ReplayPixel p;
    const int num_tiles = vp.gx * vp.gy;
    p.tile = swizzled_tile(blockIdx.x, num_tiles);
    p.tx = p.tile % vp.gx; p.ty = p.tile / vp.gx;
    p.tid = threadIdx.x; p.w = p.tid >> 6; p.lane = p.tid & 63;
    p.px = p.tx * TILE + (p.w & 1) * 8 + (p.lane & 7);
    p.py = p.ty * TILE + (p.w >> 1) * 8 + (p.lane >> 3);
    p.inside = p.px < vp.W && p.py < vp.H;
    p.pix = (size_t)p.py * vp.W + p.px;
    return p;
}
// ... and what the staging and the walks take beside it.  (Inlined, the members are plain values of the kernel: one that is not
// read behind the prologue holds no register during the walk.  A kernel that fills a BwdPix reads `inside` and `pix` once, into
// locals: its loads of final_T and n_contrib then stay under ONE branch on `inside`; read through the struct between the stores
// to the BwdPix, each load gets a branch and a kernel-argument fetch of its own.)
struct ReplayTile : ReplayPixel {
    float pxf, pyf, tx0, ty0;                                // the pixel and the tile's corner, as the pair arithmetic takes them
    uint2 range;                                             // the tile's entries in `ids`
    uint64_t lt_mask;                                        // the lanes below this one
    size_t N;                                                // W * H: the plane stride of a [C,H,W] map
};
__device__ __forceinline__ ReplayTile replay_tile(const ViewParams& vp, const uint2* __restrict__ ranges) {
    ReplayTile t;
    static_cast<ReplayPixel&>(t) = replay_pixel(vp);
    t.pxf = (float)t.px; t.pyf = (float)t.py;
    t.tx0 = (float)(t.tx * TILE); t.ty0 = (float)(t.ty * TILE);
    t.range = ranges[t.tile];
    t.lt_mask = (1ull << t.lane) - 1ull;
    t.N = (size_t)vp.W * vp.H;
    return t;
}
// How far the tile's list is replayed, from `last` = the position behind the last entry the lane's pixel blended: a wave lists
// entries below wave_last, the workgroup stages entries below tile_last.  Contains a barrier.
struct ReplayEnds { uint32_t wave_last, tile_last; };
__device__ __forceinline__ ReplayEnds replay_ends(uint32_t last, uint32_t (&s_wmax)[4], int w, int lane) {
    ReplayEnds e;
    e.wave_last = wave_max_u32(last);
    if (lane == 0) s_wmax[w] = e.wave_last;
    __syncthreads();
    e.tile_last = max(max(s_wmax[0], s_wmax[1]), max(s_wmax[2], s_wmax[3]));
    return e;
}
// This wave's list of the n staged entries (positions base .. base + n - 1 of the tile's list): the LDS slots, ascending, of those
// below wave_last whose quadrant mask — mask_of(slot) — has the wave's bit.  Compacted by ballot; returns their number.
template <class MaskOf>
__device__ __forceinline__ int compact_quadrant_list(const ReplayTile& t, int base, int n, uint32_t wave_last, uint16_t* s_listw,
                                                     MaskOf mask_of) {
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < BATCH / 64; ++c) {
        const int e = c * 64 + t.lane;
        const bool hit = e < n && (uint32_t)(base + e) < wave_last && ((mask_of(e) >> t.w) & 1u);
        const uint64_t bal = __ballot(hit);
        if (hit) s_listw[cnt + __popcll(bal & t.lt_mask)] = (uint16_t)e;
        cnt += __popcll(bal);
    }
    return cnt;
}
// One batch of a replay, called behind the barrier that ends the previous batch: thread k stages entry base + k of the tile's
// list into slot k (BATCH entries, fewer in the batch that reaches tile_last), a barrier, then every wave compacts its list into
// s_listw; returns the list's length.  extra(k, id, r0, r1, r2) stores what else the kernel's walk reads of the entry, from its
// id and its record as loaded.  Two LDS layouts:
// colour — s_r0 = r0 with the doubled cross term, s_r1 = r1 whole (red and green in z, w), the quadrant masks in s_mask;
template <class Extra>
__device__ __forceinline__ int stage_and_list_colour(const ReplayTile& t, const GaussRec* rec, const uint32_t* ids, int base,
                                                     const ReplayEnds& ends, float4* s_r0, float4* s_r1, uint32_t* s_mask,
                                                     uint16_t* s_listw, Extra extra) {
    const int n = min(BATCH, (int)ends.tile_last - base);
    if (t.tid < n) {
        const uint32_t id = ids[t.range.x + base + t.tid];
        const float4 r0 = rec[id].r0, r1 = rec[id].r1;
        const float4 r2 = rec[id].r2;
        s_r0[t.tid] = doubled_w(r0); s_r1[t.tid] = r1;
        extra(t.tid, id, r0, r1, r2);
        s_mask[t.tid] = quadrant_mask(r0, r1.x, r2.w, t.tx0, t.ty0);
    }
    __syncthreads();
    return compact_quadrant_list(t, base, n, ends.wave_last, s_listw, [=](int e) { return s_mask[e]; });
}
// packed, for the walks that read no colour — s_r1 = {C', p0', sign_test_bound, quadrant mask bits}: the bound and the mask ride
// in the two colour slots instead of arrays of their own (2 KB of LDS less).  (extra goes first: the id is stored and dead
// before the quadrant mask is worked out.)
template <class Extra>
__device__ __forceinline__ int stage_and_list_packed(const ReplayTile& t, const GaussRec* rec, const uint32_t* ids, int base,
                                                     const ReplayEnds& ends, float4* s_r0, float4* s_r1, uint16_t* s_listw,
                                                     Extra extra) {
    const int n = min(BATCH, (int)ends.tile_last - base);
    if (t.tid < n) {
        const uint32_t id = ids[t.range.x + base + t.tid];
        const float4 r0 = rec[id].r0, r1 = rec[id].r1;
        const float4 r2 = rec[id].r2;
        s_r0[t.tid] = doubled_w(r0);
        extra(t.tid, id, r0, r1, r2);
        s_r1[t.tid] = make_float4(r1.x, r1.y, sign_test_bound(r1.y), __uint_as_float(quadrant_mask(r0, r1.x, r2.w, t.tx0, t.ty0)));
    }
    __syncthreads();
    return compact_quadrant_list(t, base, n, ends.wave_last, s_listw, [=](int e) { return __float_as_uint(s_r1[e].w); });
}

// ---------------------------------------------------------------------------------------------
// Absgrad (DESIGN.md SPEC M10, 4.10; msgs_absgrad): sum_p |dL/dmean2D contribution of pixel p| per Gaussian, the densification
// statistic of AbsGS.  The per-pixel terms exist only here, in front of the cross-pixel reduction, so this is ONE more replay of
// the back-to-front walk of blend_backward_kernel (stage_and_list_colour with its extras: the same staging and quadrant lists;
// the same pair_alpha / pair_valid / pair_grad, hence the same pairs and the same q as the gradient itself) with a two-sum tail
// in the place of the nine-sum scatter:
//     u = A' dx + Bh' dy,  w = C' dy + Bh' dx   (the log2-scaled conic of the staged record; r0.w holds 2 Bh')
//     acc[id] += { sum_lanes |q u|, sum_lanes |q w| }
// The factors ln2 W and ln2 H of dL/dmean2D (preprocess_backward_kernel) are applied once per Gaussian by absgrad_finish_kernel.
// Opt-in: nothing of the default path calls or shares a kernel with it.
// ---------------------------------------------------------------------------------------------
// Two partial sums per lane -> their wave totals in lanes 0 (a) and 1 (b), a fixed tree: the lane-parity exchange leaves a on
// the even and b on the odd lanes, three row steps and the cross-row all-reduce then serve both at once (4 DPP adds, 2 selects).
__device__ __forceinline__ float wave_reduce_pair(float a, float b, int lane) {
    const bool odd = lane & 1;
    const float keep = odd ? b : a, send = odd ? a : b;
    float c = keep + dpp_mov<0xB1>(send);     // quad_perm [1,0,3,2]
    c += dpp_mov<0x4E>(c);                    // quad_perm [2,3,0,1]
    c += dpp_mov<0x124>(c);                   // row_ror:4
    c += dpp_mov<0x128>(c);                   // row_ror:8: every lane = the row total of its parity's sum
    return cross_row_allreduce(c);
}

// The walk of backward_walk<true> with the absgrad tail: float32 totals per (quadrant, entry), ONE global_atomic_add_f64 from
// two lanes into the [P, 2] double accumulator (the float32 totals add up exactly there: reproducible).
template <bool DEPTH>
__device__ __forceinline__ void absgrad_walk(const uint16_t* lp, int cnt, int base, const float4* s_r0, const float4* s_r1,
                                             const float2* s_b, const uint32_t* s_id, float pxf, float pyf, BwdPix& st,
                                             int lane, double* __restrict__ acc, const float* s_z) {
    for (int j = cnt - 1; j >= 0; --j) {
        const int e = lp[j];
        const float4 r0 = s_r0[e], r1 = s_r1[e];
        const float2 bl = s_b[e];                              // {blue, sign_test_bound}
        const float dx = r0.x - pxf, dy = r0.y - pyf;
        const PairAlpha a = pair_alpha(r0, r1, dx, dy);
        const uint64_t validm = pair_valid(a, (uint32_t)(base + e), st.last, bl.y);
        if (validm == 0) continue;
        const PairGrad g = pair_grad<DEPTH>(st, a, validm, r1, bl.x, [=] { return s_z[e]; });   // q = 0 on the masked lanes
        const float bh = 0.5f * r0.w;
        const float u = fmaf(r0.z, dx, bh * dy), w = fmaf(r1.x, dy, bh * dx);
        const float tot = wave_reduce_pair(fabsf(g.q * u), fabsf(g.q * w), lane);
        const uint32_t gid = __builtin_amdgcn_readfirstlane(s_id[e]);
        if (lane < 2) unsafeAtomicAdd(acc + (size_t)gid * 2 + lane, (double)tot);
    }
}

// The replay skeleton (replay_tile, replay_ends, stage_and_list_colour) around BwdPix and absgrad_walk.
template <bool DEPTH, bool ALPHA>
__global__ __launch_bounds__(256) void blend_absgrad_kernel(ViewParams vp, const GaussRec* __restrict__ rec,
                                                            const uint32_t* __restrict__ ids,
                                                            const uint2* __restrict__ ranges,
                                                            const float* __restrict__ final_T,
                                                            const uint32_t* __restrict__ n_contrib,
                                                            const float* __restrict__ dL_dcolor,
                                                            double* __restrict__ acc,
                                                            const float* __restrict__ dL_ddepth,
                                                            const float* __restrict__ dL_dalpha) {
    __shared__ float4 s_r0[BATCH], s_r1[BATCH];
    __shared__ float2 s_b[BATCH];                          // {blue, sign_test_bound}
    __shared__ float s_z[DEPTH ? BATCH : 1];               // view depth (depth variant)
    __shared__ uint32_t s_id[BATCH];
    __shared__ uint32_t s_mask[BATCH];
    __shared__ uint16_t s_list[4][BATCH];
    __shared__ uint32_t s_wmax[4];

    const ReplayTile t = replay_tile(vp, ranges);
    const bool inside = t.inside;
    const size_t pix = t.pix;
    BwdPix st;
    st.T = inside ? final_T[pix] : 1.0f;
    st.last = inside ? n_contrib[pix] : 0u;
    st.dL0 = st.dL1 = st.dL2 = 0.f;
    if (inside) { st.dL0 = dL_dcolor[pix]; st.dL1 = dL_dcolor[t.N + pix]; st.dL2 = dL_dcolor[2 * t.N + pix]; }
    st.dLd = (DEPTH && inside) ? dL_ddepth[pix] : 0.f;
    const ReplayEnds ends = replay_ends(st.last, s_wmax, t.w, t.lane);

    bwd_pix_start_S<ALPHA>(st, vp, inside, pix, dL_dalpha);

    const int nb = ((int)ends.tile_last + BATCH - 1) / BATCH;
    for (int b = nb - 1; b >= 0; --b) {
        __syncthreads();                              // previous batch fully consumed
        const int base = b * BATCH;
        const int cnt = stage_and_list_colour(t, rec, ids, base, ends, s_r0, s_r1, s_mask, s_list[t.w],
                                              [&](int k, uint32_t id, const float4&, const float4& r1, const float4& r2) {
            s_b[k] = make_float2(r2.x, sign_test_bound(r1.y)); s_id[k] = id;
            if constexpr (DEPTH) s_z[k] = r2.y;
        });
        absgrad_walk<DEPTH>(s_list[t.w], cnt, base, s_r0, s_r1, s_b, s_id, t.pxf, t.pyf, st, t.lane, acc, s_z);
    }
}

// out [P, 3] float32 = { ln2 W acc.x, ln2 H acc.y, 0 }: the units of dL/dmean2D (preprocess_backward_kernel)
__global__ __launch_bounds__(256) void absgrad_finish_kernel(int P, float sx, float sy, const double* __restrict__ acc,
                                                             float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    out[3 * (size_t)i + 0] = (float)acc[2 * (size_t)i + 0] * sx;
    out[3 * (size_t)i + 1] = (float)acc[2 * (size_t)i + 1] * sy;
    out[3 * (size_t)i + 2] = 0.f;
}

// ---------------------------------------------------------------------------------------------
// Contribution scores (DESIGN.md SPEC M11, 4.11; msgs_contrib_accumulate): per Gaussian, over the pixels p of a view with an
// optional weight map m_p >= 0,
//     weight_sum = sum_p m_p w_ip,   weight_max = max_p m_p w_ip,   pixel_count = #{p : m_p > 0, pair (i, p) blended}
// with w_ip = alpha_ip T_ip = PairGrad::dch, the weight of dL/dC in the colour gradient.  Like absgrad, w_ip exists only in front
// of the cross-pixel reduction: one more replay of the back-to-front walk of blend_backward_kernel (stage_and_list_colour without
// blue and depth; pair_alpha / pair_valid, and pair_grad on a zero dL/dC — only its T recurrence and dch stay alive), with a
// three-value tail.  No dL inputs, no gradients.  Opt-in: nothing of the default path calls or shares a kernel with it.
// ---------------------------------------------------------------------------------------------
// One accumulator row per Gaussian (CONTRIB_ACC_BYTES): the caller owns it across views.
struct ContribAcc {
    double sum;                     // +0: float32 wave totals, added exactly
    unsigned long long count;       // +8: 64 bits — a 4K view adds at most 8.3e6 per Gaussian
    uint32_t max_bits;              // +16: bit pattern of a non-negative float: orders like the float
    uint32_t pad;
};
static_assert(sizeof(ContribAcc) == CONTRIB_ACC_BYTES, "msgs_contrib_scratch_bytes");

// every lane receives the wave maximum (the tree of wave_allreduce_sum); unsigned, for bit patterns of non-negative floats
__device__ __forceinline__ uint32_t wave_allreduce_max_u32(uint32_t v) {
    typedef unsigned u2 __attribute__((ext_vector_type(2)));
    v = max(v, dpp_mov_u<0xB1>(v));           // quad_perm [1,0,3,2]
    v = max(v, dpp_mov_u<0x4E>(v));           // quad_perm [2,3,0,1]
    v = max(v, dpp_mov_u<0x124>(v));          // row_ror:4
    v = max(v, dpp_mov_u<0x128>(v));          // row_ror:8: every lane = its row's maximum
    const u2 a = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    v = max(a.x, a.y);
    const u2 b = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return max(b.x, b.y);
}

// wave_allreduce_sum whose adds stay adds: without this the first one is contracted with the multiply that produced the lane's
// term (an FMA on the unrounded product), and the total is no longer the sum of the float32 terms the maximum sees — a weight
// map of ones would then give other bits than no map.
__device__ __forceinline__ float wave_allreduce_sum_of_terms(float v) {
#pragma clang fp contract(off)
    v = v + dpp_mov<0xB1>(v);                 // quad_perm [1,0,3,2]
    v = v + dpp_mov<0x4E>(v);                 // quad_perm [2,3,0,1]
    v = v + dpp_mov<0x124>(v);                // row_ror:4
    v = v + dpp_mov<0x128>(v);                // row_ror:8: every lane = its row's total
    return cross_row_allreduce(v);
}

// The walk of backward_walk<true> with the contribution tail.  m: the lane's pixel weight (0 outside the image); wmask: the lanes
// with m > 0.  Per (quadrant, entry) with a counted pair: the wave total and the wave maximum of t = m dch (two fixed trees),
// the count as a scalar popcount, and three atomics from three lanes — every one independent of the order of arrival.
template <bool WEIGHTED>
__device__ __forceinline__ void contrib_walk(const uint16_t* lp, int cnt, int base, const float4* s_r0, const float4* s_r1,
                                             const float* s_bound, const uint32_t* s_id, float pxf, float pyf, BwdPix& st,
                                             float m, uint64_t wmask, uint32_t aoff, ContribAcc* __restrict__ acc) {
    for (int j = cnt - 1; j >= 0; --j) {
        const int e = lp[j];
        const float4 r0 = s_r0[e], r1 = s_r1[e];
        const float dx = r0.x - pxf, dy = r0.y - pyf;
        const PairAlpha a = pair_alpha(r0, r1, dx, dy);
        const uint64_t validm = pair_valid(a, (uint32_t)(base + e), st.last, s_bound[e]);
        if (validm == 0) continue;
        const PairGrad g = pair_grad<false>(st, a, validm, r1, 0.f, [] { return 0.f; });   // dch = 0 on the masked lanes
        const uint64_t counted = validm & wmask;
        if (counted == 0) continue;                            // (T has moved on; nothing to add)
        const float t = WEIGHTED ? m * g.dch : g.dch;
        const float tot = wave_allreduce_sum_of_terms(t);
        const uint32_t mx = wave_allreduce_max_u32(__float_as_uint(t));
        const uint32_t gid = __builtin_amdgcn_readfirstlane(s_id[e]);
        // lane k < 3 owns the 8-byte slot k of the row (sum, count, max): the address is the lane's own, as in reduce_and_add
        char* slot = reinterpret_cast<char*>(acc + gid) + aoff;
        if (aoff == 0) unsafeAtomicAdd(reinterpret_cast<double*>(slot), (double)tot);
        else if (aoff == 8) atomicAdd(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)__popcll(counted));
        else if (aoff == 16) atomicMax(reinterpret_cast<uint32_t*>(slot), mx);
    }
}

// The replay skeleton around a BwdPix with zero dL/dC and contrib_walk.
// pixel_weights [H,W] (WEIGHTED): a negative or NaN weight counts as 0; finite weights only reach the products.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void blend_contrib_kernel(ViewParams vp, const GaussRec* __restrict__ rec,
                                                            const uint32_t* __restrict__ ids,
                                                            const uint2* __restrict__ ranges,
                                                            const float* __restrict__ final_T,
                                                            const uint32_t* __restrict__ n_contrib,
                                                            const float* __restrict__ pixel_weights,
                                                            ContribAcc* __restrict__ acc) {
    __shared__ float4 s_r0[BATCH], s_r1[BATCH];
    __shared__ float s_bound[BATCH];                       // sign_test_bound
    __shared__ uint32_t s_id[BATCH];
    __shared__ uint32_t s_mask[BATCH];
    __shared__ uint16_t s_list[4][BATCH];
    __shared__ uint32_t s_wmax[4];

    const ReplayTile t = replay_tile(vp, ranges);
    const bool inside = t.inside;
    const size_t pix = t.pix;
    BwdPix st;
    st.T = inside ? final_T[pix] : 1.0f;
    st.last = inside ? n_contrib[pix] : 0u;
    st.dL0 = st.dL1 = st.dL2 = st.dLd = 0.f;
    st.S = 0.f;
    float m = inside ? 1.0f : 0.0f;
    if constexpr (WEIGHTED) {
        const float pw = inside ? pixel_weights[pix] : 0.0f;
        m = pw > 0.0f ? fminf(pw, 3.4028234664e38f) : 0.0f;    // NaN and negatives fail the comparison
    }
    const uint64_t wmask = __builtin_amdgcn_ballot_w64(m > 0.0f);
    const uint32_t aoff = t.lane < 3 ? 8u * (uint32_t)t.lane : 0xFFFFFFFFu;  // byte offset of the lane's slot; none: no atomic
    const ReplayEnds ends = replay_ends(st.last, s_wmax, t.w, t.lane);

    const int nb = ((int)ends.tile_last + BATCH - 1) / BATCH;
    for (int b = nb - 1; b >= 0; --b) {
        __syncthreads();                              // previous batch fully consumed
        const int base = b * BATCH;
        const int cnt = stage_and_list_colour(t, rec, ids, base, ends, s_r0, s_r1, s_mask, s_list[t.w],
                                              [&](int k, uint32_t id, const float4&, const float4& r1, const float4&) {
            s_bound[k] = sign_test_bound(r1.y); s_id[k] = id;
        });
        contrib_walk<WEIGHTED>(s_list[t.w], cnt, base, s_r0, s_r1, s_bound, s_id, t.pxf, t.pyf, st, m, wmask, aoff, acc);
    }
}

__global__ __launch_bounds__(256) void contrib_finish_kernel(int P, const ContribAcc* __restrict__ acc,
                                                             float* __restrict__ weight_sum, float* __restrict__ weight_max,
                                                             long long* __restrict__ pixel_count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const ContribAcc a = acc[i];
    weight_sum[i] = (float)a.sum;
    weight_max[i] = __uint_as_float(a.max_bits);
    pixel_count[i] = (long long)a.count;
}

// ---------------------------------------------------------------------------------------------
// Feature channels (DESIGN.md SPEC M12, 4.12; msgs_features_forward / msgs_features_backward): per-Gaussian vectors f_i [C]
// splatted with the blend weights w_ip = alpha_ip T_ip = PairGrad::dch, over background 0:
//     F[c,p] = sum_i f_ic w_ip          dL/df_ic = sum_p G_cp w_ip          (G = dL/dF)
// and, as C more colour channels, a share of dL/dalpha: q_f from e_ip = sum_c G_cp f_ic in the place of g_i with a recurrence S_f
// of its own that starts at 0; its six geometry sums are ADDED to record slots 0..5 in front of the ordinary blend backward.
// Two more replays of the back-to-front walk of blend_backward_kernel (pair_alpha / pair_valid / pair_grad as in
// blend_contrib_kernel: the same pairs, the same weights).  No colour is read here, so the staging is stage_and_list_packed: the
// 2 KB of LDS it saves keep eight waves per SIMD beside the feature block, which its `extra` fills (stage_feature_row).
// Channels go in blocks of CB, one launch per block — every block is linear and independent, the geometry sums included.  A
// block's CB features of each staged entry lie in LDS and are read at a wave-uniform address.  Opt-in: nothing of the default
// path calls or shares a kernel with them.
// ---------------------------------------------------------------------------------------------
constexpr int FEAT_CB = 8;          // channels per launch (the resource table behind the choice)

// Channels c0 .. c0 + CB - 1 of row `id` of features [P, C] -> dst[0 .. CB/4); channels at or behind C are staged as zeros.
// vec: C % 4 == 0 and a 16-byte aligned base (c0 is a multiple of CB): 16-byte loads; the same values either way.
template <int CB>
__device__ __forceinline__ void stage_feature_row(float4* dst, const float* __restrict__ features, uint32_t id, int C, int c0,
                                                  bool vec) {
    const float* row = features + (size_t)id * C + c0;
#pragma unroll
    for (int k = 0; k < CB / 4; ++k) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const int c = c0 + 4 * k;
        if (vec) {
            if (c < C) v = *reinterpret_cast<const float4*>(row + 4 * k);
        } else {
            if (c + 0 < C) v.x = row[4 * k + 0];
            if (c + 1 < C) v.y = row[4 * k + 1];
            if (c + 2 < C) v.z = row[4 * k + 2];
            if (c + 3 < C) v.w = row[4 * k + 3];
        }
        dst[k] = v;
    }
}

// The walk of contrib_walk with CB accumulators per lane: one FMA per (pair, channel), back to front.  pair_grad on a zero dL/dC
// (only its T recurrence and dch stay alive); dch = 0 on the masked lanes.
template <int CB>
__device__ __forceinline__ void features_forward_walk(const uint16_t* lp, int cnt, int base, const float4* s_r0, const float4* s_r1,
                                                      const float4* s_f, float pxf, float pyf, BwdPix& st,
                                                      float (&acc)[CB]) {
    for (int j = cnt - 1; j >= 0; --j) {
        const int e = lp[j];
        const float4 r0 = s_r0[e], r1 = s_r1[e];
        const float dx = r0.x - pxf, dy = r0.y - pyf;
        const PairAlpha a = pair_alpha(r0, r1, dx, dy);
        const uint64_t validm = pair_valid(a, (uint32_t)(base + e), st.last, r1.z);
        if (validm == 0) continue;
        const PairGrad g = pair_grad<false>(st, a, validm, make_float4(r1.x, r1.y, 0.f, 0.f), 0.f, [] { return 0.f; });
#pragma unroll
        for (int k = 0; k < CB / 4; ++k) {
            const float4 f = s_f[e * (CB / 4) + k];
            acc[4 * k + 0] = fmaf(f.x, g.dch, acc[4 * k + 0]); acc[4 * k + 1] = fmaf(f.y, g.dch, acc[4 * k + 1]);
            acc[4 * k + 2] = fmaf(f.z, g.dch, acc[4 * k + 2]); acc[4 * k + 3] = fmaf(f.w, g.dch, acc[4 * k + 3]);
        }
    }
}

// out [C,H,W]: channels c0 .. c0 + CB - 1 (the real ones) of every inside pixel, plain stores; a pixel with no counted pair
// stores 0.  The replay skeleton around CB accumulators and features_forward_walk.
template <int CB>
__global__ __launch_bounds__(256) void blend_features_forward_kernel(ViewParams vp, const GaussRec* __restrict__ rec,
                                                                     const uint32_t* __restrict__ ids,
                                                                     const uint2* __restrict__ ranges,
                                                                     const float* __restrict__ final_T,
                                                                     const uint32_t* __restrict__ n_contrib,
                                                                     const float* __restrict__ features, int C, int c0, int vec,
                                                                     float* __restrict__ out) {
    static_assert(CB % 4 == 0, "rows are staged as float4");
    __shared__ float4 s_r0[BATCH], s_r1[BATCH];           // s_r1: {C', p0', sign_test_bound, quadrant mask bits}: no colour here
    __shared__ float4 s_f[BATCH * (CB / 4)];               // the block's CB features of every staged entry
    __shared__ uint16_t s_list[4][BATCH];
    __shared__ uint32_t s_wmax[4];

    const ReplayTile t = replay_tile(vp, ranges);
    const bool inside = t.inside;
    const size_t pix = t.pix;
    BwdPix st;
    st.T = inside ? final_T[pix] : 1.0f;
    st.last = inside ? n_contrib[pix] : 0u;
    st.dL0 = st.dL1 = st.dL2 = st.dLd = 0.f;
    st.S = 0.f;
    float acc[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[c] = 0.f;
    const ReplayEnds ends = replay_ends(st.last, s_wmax, t.w, t.lane);

    const int nb = ((int)ends.tile_last + BATCH - 1) / BATCH;
    for (int b = nb - 1; b >= 0; --b) {
        __syncthreads();                              // previous batch fully consumed
        const int base = b * BATCH;
        const int cnt = stage_and_list_packed(t, rec, ids, base, ends, s_r0, s_r1, s_list[t.w],
                                              [&](int k, uint32_t id, const float4&, const float4&, const float4&) {
            stage_feature_row<CB>(s_f + k * (CB / 4), features, id, C, c0, vec != 0);
        });
        features_forward_walk<CB>(s_list[t.w], cnt, base, s_r0, s_r1, s_f, t.pxf, t.pyf, st, acc);
    }
    if (inside) {
#pragma unroll
        for (int c = 0; c < CB; ++c)
            if (c0 + c < C) out[(size_t)(c0 + c) * t.N + pix] = acc[c];
    }
}

// The backward walk.  G: the lane's CB values of dL/dF (0 outside the image and for the channels behind C).
// GEOM: e = sum_c G_c f_c enters pair_grad as the only colour (red = e under dL/dC = (1, 0, 0), so g_i = e), st.S is S_f; the
// six sums of q_f go to record slots 0..5 with the ordinary reduce_and_add (zeros to 6..8: still one atomic instruction).
// Always: the CB products G_c dch are reduce-scattered by row_reduce_scatter (components 0..7 of its nine) so that the eight
// lanes 0, 1, 4, 5, 8, 9, 12, 13 each own one wave total, and ONE atomic instruction adds them at the lanes' own addresses into
// the entry's row of the [P, CB] double accumulator (float32 totals add up exactly there: the same bits on every run).
template <int CB, bool GEOM>
__device__ __forceinline__ void features_backward_walk(const uint16_t* lp, int cnt, int base, const float4* s_r0,
                                                       const float4* s_r1, const uint32_t* s_id,
                                                       const float4* s_f, float pxf, float pyf, BwdPix& st, const float (&G)[CB],
                                                       bool alane, uint32_t aoff, grad_acc_t* __restrict__ grad_rec, bool flane,
                                                       uint32_t foff, double* __restrict__ acc) {
    static_assert(CB == 8, "the reduce-scatter of row_reduce_scatter delivers eight components");
    for (int j = cnt - 1; j >= 0; --j) {
        const int e = lp[j];
        const float4 r0 = s_r0[e], r1 = s_r1[e];
        const float dx = r0.x - pxf, dy = r0.y - pyf;
        const PairAlpha a = pair_alpha(r0, r1, dx, dy);
        const uint64_t validm = pair_valid(a, (uint32_t)(base + e), st.last, r1.z);
        if (validm == 0) continue;
        PairGrad g;
        if constexpr (GEOM) {
            const float4 f0 = s_f[e * 2], f1 = s_f[e * 2 + 1];
            float ef = G[0] * f0.x;
            ef = fmaf(G[1], f0.y, ef); ef = fmaf(G[2], f0.z, ef); ef = fmaf(G[3], f0.w, ef);
            ef = fmaf(G[4], f1.x, ef); ef = fmaf(G[5], f1.y, ef); ef = fmaf(G[6], f1.z, ef); ef = fmaf(G[7], f1.w, ef);
            g = pair_grad<false>(st, a, validm, make_float4(r1.x, r1.y, ef, 0.f), 0.f, [] { return 0.f; });
            const BwdSums v = {g.q * dx, g.q * dy, g.q * a.ev.dxx, g.q * a.ev.dxy, g.q * a.ev.dyy, g.q, 0.f, 0.f, 0.f};
            reduce_and_add<false>(v, 0.f, [](float x) { return cross_row_allreduce(x); }, [=] { return s_id[e]; }, grad_rec,
                                  alane, aoff);
        } else {
            g = pair_grad<false>(st, a, validm, make_float4(r1.x, r1.y, 0.f, 0.f), 0.f, [] { return 0.f; });
        }
        const BwdSums u = {G[0] * g.dch, G[1] * g.dch, G[2] * g.dch, G[3] * g.dch, G[4] * g.dch, G[5] * g.dch, G[6] * g.dch,
                           G[7] * g.dch, 0.f};
        const float tot = cross_row_allreduce(row_reduce_scatter<false>(u, 0.f));
        const uint32_t gid = __builtin_amdgcn_readfirstlane(s_id[e]);
        if (flane) unsafeAtomicAdd(acc + (size_t)gid * CB + foff, (double)tot);
    }
}

// dL_dF [C,H,W]; acc [P, CB] doubles (this block's channels; cleared by the caller).  GEOM = false (no geometry input requires
// grad): no feature is staged or read, no S_f, no q_f, no record atomic.
template <int CB, bool GEOM>
__global__ __launch_bounds__(256) void blend_features_backward_kernel(ViewParams vp, const GaussRec* __restrict__ rec,
                                                                      const uint32_t* __restrict__ ids,
                                                                      const uint2* __restrict__ ranges,
                                                                      const float* __restrict__ final_T,
                                                                      const uint32_t* __restrict__ n_contrib,
                                                                      const float* __restrict__ features, int C, int c0, int vec,
                                                                      const float* __restrict__ dL_dF,
                                                                      grad_acc_t* __restrict__ grad_rec,
                                                                      double* __restrict__ acc) {
    static_assert(CB % 4 == 0, "rows are staged as float4");
    __shared__ float4 s_r0[BATCH], s_r1[BATCH];           // s_r1: {C', p0', sign_test_bound, quadrant mask bits}: no colour here
    __shared__ float4 s_f[GEOM ? BATCH * (CB / 4) : 1];    // the block's CB features of every staged entry
    __shared__ uint32_t s_id[BATCH];
    __shared__ uint16_t s_list[4][BATCH];
    __shared__ uint32_t s_wmax[4];

    const ReplayTile t = replay_tile(vp, ranges);
    const bool inside = t.inside;
    const size_t pix = t.pix;
    BwdPix st;
    st.T = inside ? final_T[pix] : 1.0f;
    st.last = inside ? n_contrib[pix] : 0u;
    st.dL0 = GEOM ? 1.f : 0.f;                             // g_i = red = e (features_backward_walk)
    st.dL1 = st.dL2 = st.dLd = 0.f;
    st.S = 0.f;                                            // S_f: no background term
    float G[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) G[c] = (inside && c0 + c < C) ? dL_dF[(size_t)(c0 + c) * t.N + pix] : 0.f;
    const ReplayEnds ends = replay_ends(st.last, s_wmax, t.w, t.lane);

    const bool alane = IS_ATOMIC_LANE(false, t.lane);
    const uint32_t aoff = row_reduce_component<false>(t.lane);
    const bool flane = t.lane < 16 && !(t.lane & 2);       // the eight lanes that own components 0..7
    const uint32_t foff = aoff;

    const int nb = ((int)ends.tile_last + BATCH - 1) / BATCH;
    for (int b = nb - 1; b >= 0; --b) {
        __syncthreads();                              // previous batch fully consumed
        const int base = b * BATCH;
        const int cnt = stage_and_list_packed(t, rec, ids, base, ends, s_r0, s_r1, s_list[t.w],
                                              [&](int k, uint32_t id, const float4&, const float4&, const float4&) {
            s_id[k] = id;
            if constexpr (GEOM) stage_feature_row<CB>(s_f + k * (CB / 4), features, id, C, c0, vec != 0);
        });
        features_backward_walk<CB, GEOM>(s_list[t.w], cnt, base, s_r0, s_r1, s_id, s_f, t.pxf, t.pyf, st, G, alane, aoff,
                                         grad_rec, flane, foff, acc);
    }
}

// columns c0 .. c0 + CB - 1 (the real ones) of dL_dfeatures [P, C] from the accumulator block, which is cleared for the next one
template <int CB>
__global__ __launch_bounds__(256) void features_finish_kernel(int P, int C, int c0, double* __restrict__ acc,
                                                              float* __restrict__ dL_dfeatures) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (size_t)P * CB) return;
    const size_t i = k / CB;
    const int c = c0 + (int)(k % CB);
    if (c < C) dL_dfeatures[i * (size_t)C + c] = (float)acc[k];
    acc[k] = 0.0;
}

// ---------------------------------------------------------------------------------------------
// Depth distortion (DESIGN.md SPEC M13, 4.13; msgs_distortion_forward / msgs_distortion_backward): the Mip-NeRF 360 distortion
// of a ray's blended mass, in the signed list-order form, over exactly the pairs the backward counts (i = 1..n front to back,
// w_i = alpha_i T_i, z_i the view depth the depth map blends):
//     Dist = 2 sum_{j<i} w_i w_j (z_i - z_j) = 2 sum_i w_i (R_i - z_i (T_{i+1} - T_f)),     R_i = sum_{k>i} w_k z_k
// Quadratic in the weights, so it exists only inside the walk: two more replays of blend_backward_kernel's back-to-front walk
// (stage_and_list_packed, with s_z — and s_id in the backward — as the extra).  Back to front the suffix moment R_i and the
// suffix weight T_{i+1} - T_f are what the walk has in hand; the backward needs the prefix too and takes it from
// M = sum_i w_i z_i, which the forward stores:  sum_{j<i} w_j z_j = M - R_i - w_i z_i,  sum_{j<i} w_j = 1 - T_i.
// With B_i = 1 + T_f - T_i - T_{i+1}
//     dDist/dw_i = 2 (z_i B_i - (M - R_i - w_i z_i) + R_i)          dDist/dz_i = 2 w_i B_i
// G dDist/dw_i enters the S recurrence as the pair's only colour (S starts at 0: no background term), exactly as e does in
// features_backward_walk; the six sums of q go to record slots 0..5 and sum G dDist/dz_i to slot 9 through reduce_and_add<true>.
// Every z is taken relative to z_ref, the view depth of the tile's first list entry: Dist and both derivatives depend on depth
// differences only, and in float32 the moments of a scene far from the camera would otherwise cancel.
// R accumulates by the same fmaf of the same operands in both kernels, so M - R_i - w_i z_i closes on zero at the front entry.
// Opt-in: nothing of the default path calls or shares a kernel with them.
// ---------------------------------------------------------------------------------------------
// The T recurrence of pair_grad alone (the same operations: w has the bits of PairGrad::dch); a masked lane gets w = 0, T unchanged.
struct DistStep { float a_m, alpha_m, Tn, w; };
__device__ __forceinline__ DistStep dist_step(float& T, const PairAlpha& a, uint64_t validm) {
    const bool valid = __builtin_amdgcn_inverse_ballot_w64(validm);
    DistStep d;
    d.a_m = valid ? a.a_raw : 0.0f;
    d.alpha_m = fminf(0.99f, d.a_m);
    const float inv = __builtin_amdgcn_rcpf(1.0f - d.alpha_m);
    d.Tn = T * inv;
    T = d.Tn;
    d.w = d.alpha_m * d.Tn;
    return d;
}
// R += w z~: ONE expression for both kernels (explicit fmaf: no contraction choice left to the compiler)
__device__ __forceinline__ float dist_moment_add(float R, float w, float zt) { return fmaf(w, zt, R); }

// out_distortion [H,W] = Dist, out_moment [H,W] = M = sum_i w_i (z_i - z_ref): plain stores for the inside pixels; a pixel with
// fewer than two counted pairs stores Dist = 0.  One 256-thread workgroup per tile, one 8x8 quadrant per wave.
__global__ __launch_bounds__(256) void blend_distortion_forward_kernel(ViewParams vp, const GaussRec* __restrict__ rec,
                                                                       const uint32_t* __restrict__ ids,
                                                                       const uint2* __restrict__ ranges,
                                                                       const float* __restrict__ final_T,
                                                                       const uint32_t* __restrict__ n_contrib,
                                                                       float* __restrict__ out_distortion,
                                                                       float* __restrict__ out_moment) {
    __shared__ float4 s_r0[BATCH], s_r1[BATCH];
    __shared__ float s_z[BATCH];
    __shared__ uint16_t s_list[4][BATCH];
    __shared__ uint32_t s_wmax[4];

    const ReplayTile t = replay_tile(vp, ranges);
    const float Tf = t.inside ? final_T[t.pix] : 1.0f;
    const uint32_t last = t.inside ? n_contrib[t.pix] : 0u;
    float T = Tf, R = 0.f, acc = 0.f;
    const ReplayEnds ends = replay_ends(last, s_wmax, t.w, t.lane);
    const float zref = ends.tile_last > 0u ? rec[ids[t.range.x]].r2.y : 0.f;      // (a tile that blended has a first entry)

    const int nb = ((int)ends.tile_last + BATCH - 1) / BATCH;
    for (int b = nb - 1; b >= 0; --b) {
        __syncthreads();                              // previous batch fully consumed
        const int base = b * BATCH;
        const int cnt = stage_and_list_packed(t, rec, ids, base, ends, s_r0, s_r1, s_list[t.w],
                                              [&](int k, uint32_t, const float4&, const float4&, const float4& r2) {
            s_z[k] = r2.y;
        });
        const uint16_t* lp = s_list[t.w];
        for (int j = cnt - 1; j >= 0; --j) {
            const int e = lp[j];
            const float4 r0 = s_r0[e], r1 = s_r1[e];
            const float dx = r0.x - t.pxf, dy = r0.y - t.pyf;
            const PairAlpha a = pair_alpha(r0, r1, dx, dy);
            const uint64_t validm = pair_valid(a, (uint32_t)(base + e), last, r1.z);
            if (validm == 0) continue;
            const float Tp = T;                                           // T_{i+1}
            const DistStep d = dist_step(T, a, validm);
            const float zt = s_z[e] - zref;
            acc = fmaf(d.w, fmaf(-zt, Tp - Tf, R), acc);                  // w_i (R_i - z_i (T_{i+1} - T_f)); w = 0 on the masked lanes
            R = dist_moment_add(R, d.w, zt);
        }
    }
    if (t.inside) { out_distortion[t.pix] = 2.0f * acc; out_moment[t.pix] = R; }
}

// dL_ddist [H,W] = G, moment [H,W] = the forward's out_moment.  ADDS the six sums of q to record slots 0..5 and
// sum_p G dDist/dz_i to slot 9 (zeros to 6..8): one atomic instruction per (quadrant, entry), every lane at its own slot.
__global__ __launch_bounds__(256) void blend_distortion_backward_kernel(ViewParams vp, const GaussRec* __restrict__ rec,
                                                                        const uint32_t* __restrict__ ids,
                                                                        const uint2* __restrict__ ranges,
                                                                        const float* __restrict__ final_T,
                                                                        const uint32_t* __restrict__ n_contrib,
                                                                        const float* __restrict__ moment,
                                                                        const float* __restrict__ dL_ddist,
                                                                        grad_acc_t* __restrict__ grad_rec) {
    __shared__ float4 s_r0[BATCH], s_r1[BATCH];
    __shared__ float s_z[BATCH];
    __shared__ uint32_t s_id[BATCH];
    __shared__ uint16_t s_list[4][BATCH];
    __shared__ uint32_t s_wmax[4];

    const ReplayTile t = replay_tile(vp, ranges);
    const float Tf = t.inside ? final_T[t.pix] : 1.0f;
    const uint32_t last = t.inside ? n_contrib[t.pix] : 0u;
    const float G2 = t.inside ? 2.0f * dL_ddist[t.pix] : 0.f;
    const float M = t.inside ? moment[t.pix] : 0.f;
    const float oneTf = 1.0f + Tf;
    float T = Tf, R = 0.f, S = 0.f;
    const ReplayEnds ends = replay_ends(last, s_wmax, t.w, t.lane);
    const float zref = ends.tile_last > 0u ? rec[ids[t.range.x]].r2.y : 0.f;      // the forward's

    const bool alane = IS_ATOMIC_LANE(true, t.lane);
    const uint32_t aoff = row_reduce_component<true>(t.lane);

    const int nb = ((int)ends.tile_last + BATCH - 1) / BATCH;
    for (int b = nb - 1; b >= 0; --b) {
        __syncthreads();                              // previous batch fully consumed
        const int base = b * BATCH;
        const int cnt = stage_and_list_packed(t, rec, ids, base, ends, s_r0, s_r1, s_list[t.w],
                                              [&](int k, uint32_t id, const float4&, const float4&, const float4& r2) {
            s_z[k] = r2.y; s_id[k] = id;
        });
        const uint16_t* lp = s_list[t.w];
        for (int j = cnt - 1; j >= 0; --j) {
            const int e = lp[j];
            const float4 r0 = s_r0[e], r1 = s_r1[e];
            const float dx = r0.x - t.pxf, dy = r0.y - t.pyf;
            const PairAlpha a = pair_alpha(r0, r1, dx, dy);
            const uint64_t validm = pair_valid(a, (uint32_t)(base + e), last, r1.z);
            if (validm == 0) continue;
            const float Tp = T;                                           // T_{i+1}
            const DistStep d = dist_step(T, a, validm);                   // T = T_i
            const float zt = s_z[e] - zref;
            const float B = (oneTf - d.Tn) - Tp;
            const float front = (M - R) - d.w * zt;                       // sum_{j<i} w_j z_j: closes on 0 at the front entry
            const float ei = G2 * (fmaf(zt, B, R) - front);               // G dDist/dw_i
            const float dz = G2 * (d.w * B);                              // G dDist/dz_i  (0 on the masked lanes)
            const float sm = ei - S;
            const float q = d.a_m * (sm * d.Tn);                          // as pair_grad: the gradient passes the 0.99 clamp
            S = fmaf(d.alpha_m, sm, S);
            R = dist_moment_add(R, d.w, zt);
            const BwdSums v = {q * dx, q * dy, q * a.ev.dxx, q * a.ev.dxy, q * a.ev.dyy, q, 0.f, 0.f, 0.f};
            reduce_and_add<true>(v, dz, [](float x) { return cross_row_allreduce(x); }, [=] { return s_id[e]; }, grad_rec, alane,
                                 aoff);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Median depth and Gaussian id (DESIGN.md SPEC M15, 4.15; msgs_median_depth_forward / msgs_median_depth_backward).  Over the
// blended entries i = 1..n of a pixel (the pairs the backward counts, in tile-list order) with the FORWARD's transmittance
// recurrence T_1 = 1, T_{i+1} = fmaf(-T_i, alpha_i, T_i), the median entry m is the last one with T_i > 0.5 (the 2DGS / gsplat
// rule): the entry whose blending takes T to <= 0.5, or the last blended entry of a ray that never gets there.
//     median_depth = z_m (GaussRec.r2.y, the depth the depth map blends; 0.0f where nothing was blended)
//     median_id    = its row in the model (-1 where nothing was blended)
// T_i exists only inside the walk, hence one more replay of the tile lists (stage_and_list_packed with s_z and s_id as the
// extra) — but FRONT TO BACK, unlike the other replays: the selection compares T_i itself with 0.5, and only the forward's own
// recurrence from T_1 = 1 reproduces the bits the render blended with (T_f divided back up differs in the last places, which
// flips the entry on a ray that crosses near 0.5).  Front to back also ends early: a lane is finished once T <= 0.5 after a blend
// or at n_contrib, a wave leaves its list and the workgroup its batch loop when all their lanes are.  While T_i > 0.5 and
// alpha <= 0.99, T_{i+1} >= 0.005: the forward's T < 1e-4 stop rule cannot fire on an entry this walk looks at, so pair_valid
// (position below n_contrib, sign test, alpha >= 1/255) is exactly "blended" here.
// Gradient: d median_depth / dz_i = [i = m], nothing through the selection.  median_depth_backward_kernel adds G_p to slot 9
// (dL/dz) of record median_id[p]; the depth variant of the per-Gaussian backward carries it to the means and the camera.
// Opt-in: nothing of the default path calls or shares a kernel with them.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void blend_median_depth_forward_kernel(ViewParams vp, const GaussRec* __restrict__ rec,
                                                                         const uint32_t* __restrict__ ids,
                                                                         const uint2* __restrict__ ranges,
                                                                         const uint32_t* __restrict__ n_contrib,
                                                                         float* __restrict__ out_depth,
                                                                         int32_t* __restrict__ out_id) {
    __shared__ float4 s_r0[BATCH], s_r1[BATCH];
    __shared__ float s_z[BATCH];
    __shared__ uint32_t s_id[BATCH];
    __shared__ uint16_t s_list[4][BATCH];
    __shared__ uint32_t s_wmax[4];

    const ReplayTile t = replay_tile(vp, ranges);
    const uint32_t last = t.inside ? n_contrib[t.pix] : 0u;
    float T = 1.0f, zm = 0.0f;
    int32_t idm = -1;
    const ReplayEnds ends = replay_ends(last, s_wmax, t.w, t.lane);

    uint64_t open = __builtin_amdgcn_ballot_w64(last > 0u);          // lanes that have not reached their median entry yet

    for (int base = 0; base < (int)ends.tile_last; base += BATCH) {
        if (__syncthreads_and(open == 0)) break;      // every lane of the tile is finished; the barrier also protects the batch
        // (a finished wave stages its share of the batch and compacts nothing)
        const uint32_t list_last = open ? ends.wave_last : 0u;
        const int cnt = stage_and_list_packed(t, rec, ids, base, ReplayEnds{list_last, ends.tile_last}, s_r0, s_r1, s_list[t.w],
                                              [&](int k, uint32_t id, const float4&, const float4&, const float4& r2) {
            s_z[k] = r2.y; s_id[k] = id;
        });
        const uint16_t* lp = s_list[t.w];
        for (int j = 0; j < cnt; ++j) {
            if (open == 0) break;
            const int e = lp[j];
            const float4 r0 = s_r0[e], r1 = s_r1[e];
            const float dx = r0.x - t.pxf, dy = r0.y - t.pyf;
            const PairAlpha a = pair_alpha(r0, r1, dx, dy);
            const uint32_t pos = (uint32_t)(base + e);
            const uint64_t validm = pair_valid(a, pos, last, r1.z) & open;
            const uint64_t at_end = __builtin_amdgcn_ballot_w64(pos + 1u >= last);      // nothing of this lane's behind this entry
            if (validm != 0) {
                const bool valid = __builtin_amdgcn_inverse_ballot_w64(validm);
                const float alpha = fminf(0.99f, a.a_raw);
                const float Tn = __fmaf_rn(-T, alpha, T);                               // forward_walk's test_T
                const uint64_t crossed = __builtin_amdgcn_ballot_w64(Tn <= 0.5f);
                zm = valid ? s_z[e] : zm;                                               // T_i > 0.5 on every open lane
                idm = valid ? (int32_t)s_id[e] : idm;
                T = valid ? Tn : T;
                open &= ~(validm & crossed);
            }
            open &= ~at_end;
        }
    }
    if (t.inside) { out_depth[t.pix] = zm; out_id[t.pix] = idm; }
}

// median_id [H,W], dL_dmedian [H,W] = G: ADDS sum_{p: median_id[p] = i} G_p to slot 9 of record i.  The pixel mapping of the
// replays (replay_pixel), so that a wave holds one 8x8 block: neighbouring pixels mostly share their median Gaussian, and one
// lane per 80-byte record is the worst shape for an atomic wave-instruction.  The lanes of a wave that hold the same id are
// combined first (leader's id broadcast, ballot of the equal lanes, wave total of their G) and the leader issues ONE add per
// distinct id.
__global__ __launch_bounds__(256) void median_depth_backward_kernel(ViewParams vp, int P, const int32_t* __restrict__ median_id,
                                                                    const float* __restrict__ dL_dmedian,
                                                                    grad_acc_t* __restrict__ grad_rec) {
    const ReplayPixel p = replay_pixel(vp);
    const int32_t id = p.inside ? median_id[p.pix] : -1;
    const float g = p.inside ? dL_dmedian[p.pix] : 0.f;
    uint64_t rem = __builtin_amdgcn_ballot_w64(id >= 0 && id < P);   // (an id outside the model adds nothing)
    while (rem != 0) {
        const int leader = __builtin_ctzll(rem);
        const int32_t cur = lane_bcast(id, leader);
        const bool mine = id == cur;
        const uint64_t same = __builtin_amdgcn_ballot_w64(mine);
        const float tot = wave_allreduce_sum(mine ? g : 0.f);
        if (p.lane == leader) unsafeAtomicAdd(grad_rec + (size_t)cur * GRAD_REC_FLOATS + 9, (grad_acc_t)tot);
        rem &= ~same;
    }
}

// ---------------------------------------------------------------------------------------------
// statistics for the algorithmic-bytes formula: D_trav = sum_tiles max_pixels n_contrib, V = #radii>0
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tile_stats_kernel(ViewParams vp, const uint32_t* __restrict__ n_contrib,
                                                         unsigned long long* __restrict__ out) {
    __shared__ uint32_t s_wmax[4];
    const int tile = blockIdx.x;
    const int tx = tile % vp.gx, ty = tile / vp.gx;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int px = tx * TILE + (tid & 15), py = ty * TILE + (tid >> 4);
    const uint32_t v = (px < vp.W && py < vp.H) ? n_contrib[(size_t)py * vp.W + px] : 0u;
    const uint32_t m = wave_max_u32(v);
    if (lane == 0) s_wmax[w] = m;
    __syncthreads();
    if (tid == 0) atomicAdd(&out[0], (unsigned long long)max(max(s_wmax[0], s_wmax[1]), max(s_wmax[2], s_wmax[3])));
}

__global__ __launch_bounds__(256) void visible_count_kernel(int P, const int32_t* __restrict__ radii,
                                                            unsigned long long* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool vis = i < P && radii[i] > 0;
    const uint64_t b = __ballot(vis);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&out[1], (unsigned long long)__popcll(b));
}

}  // namespace

// Forward: one 256-thread workgroup per tile, one 8x8 quadrant per wave (229 us at C3 in round 1 against 405 us for one wave per
// tile; the strip / 4x4-block list variants of rounds 3-4 measured slower as well — profiles/design_history_r1_r4.md, git history).
// Backward: one wave64 per tile, four pixels per lane, one reduction per (tile, Gaussian) from 4096 tiles up; four waves per tile
// below.  (A packed-fp32 forward with two pixels per lane was also built and measured: correct but 17 % slower — v_pk_*_f32 is
// not full rate on gfx950 — and removed; for the same reason this library is compiled with -fno-slp-vectorize, which alone took
// the backward from 558 to 495 us.)
// backward generation: MSGS_BWD_GEN = 1 | 2 forces one; default (0) picks by tile count — one wave per tile (gen 2) needs
// >= ~4000 tiles to occupy 1024 SIMDs, below that four waves per tile (gen 1) win (C3 scene, profiles/r1_notes.md:
// 8160 tiles 437 vs 667 us; 2040 tiles 334 vs 297; 510 tiles 481 vs 205; 135 tiles 834 vs 303; 2 tiles 1378 vs 431)
constexpr int BWD_GEN2_MIN_TILES = 4096;
// below these tile counts: the sixteen-waves-per-tile kernels (latency-bound regime).  C3 scene, profiles/r1_notes.md:
// forward 510 tiles 109 -> 100 us, 135 tiles 184 -> 112, 40 tiles 285 -> 161; backward 510 tiles 167 -> 184 (worse),
// 135 tiles 262 -> 185, 40 tiles 372 -> 236
constexpr int FINE_MAX_TILES_FWD = 300, FINE_MAX_TILES_BWD = 300;     // (round 3 sweep: 510 tiles forward 102 us coarse vs 127 fine;
                                                                       //  135 tiles 155 vs 104; backward 510 tiles 168 vs 229, 135 tiles 263 vs 182)
static std::atomic<int> g_bwd_gen{[] { const char* e = getenv("MSGS_BWD_GEN"); return (e && (e[0] == '1' || e[0] == '2')) ? e[0] - '0' : 0; }()};
int set_backward_generation(int gen) { return g_bwd_gen.exchange(gen == 1 || gen == 2 ? gen : 0); }
// blend granularity: 0 = by tile count, 1 = coarse (quadrant / tile per wave), 2 = fine (4x4 sub-block per wave)
static std::atomic<int> g_granularity{[] { const char* e = getenv("MSGS_BLEND_GRANULARITY"); return (e && (e[0] == '1' || e[0] == '2')) ? e[0] - '0' : 0; }()};
int set_blend_granularity(int mode) { return g_granularity.exchange(mode == 1 || mode == 2 ? mode : 0); }
// Shape of the fine-grained kernels: the sub-block side SB a wave owns (4 | 2 | 1 -> 16 | 64 | 256 waves per tile) and the
// number G of workgroups a tile's waves are split over (every workgroup stages and classifies the tile's whole list).
// Measured on the pyramid of the C3 scene, forward / backward us at 135, 40, 12, 2 tiles (profiles/r3_notes.md):
//   SB 4: G = 1: 105/184, 139/228, 146/241, 132/224;  G = 2: 87/152, 114/192, 115/194, 100/175;  G = 4: 87/140, 111/180, 108/182,
//         98/166;  G = 8: 112/151, 133/190, 138/188, 117/166;  G = 16: 152/164, 158/198, 149/176, 130/162
//   SB 2: G = 4: 156/251, 104/140, 100/133, 95/129;  G = 8: 128/181, 85/122, 83/117, 75/107;  G = 16: 122/168, 82/111, 82/107,
//         74/98;  G = 32: 167/207, 115/130, 104/108, 91/97
//   SB 1: G = 16: 329/368, 139/152, 82/94, 76/89;  G = 32: 277/330, 120/130, 73/86, 65/81;  G = 64: 246/304, 112/131, 71/84, 62/74
// i.e. the best shape keeps 2000-3000 waves in flight: 4x4 blocks down to ~64 tiles, 2x2 blocks down to ~16, single pixels below.
// Only the four shapes chosen below are built; the others of the table were measured and are no longer instantiated.
// A shape names what is launched: workgroups of WAVES waves, a wave per SB x SB sub-block, G = groups workgroups per tile.
template <int WAVES, int SB>
struct FineShape { static constexpr int waves = WAVES, sb = SB, groups = (TILE / SB) * (TILE / SB) / WAVES; };
// f(FineShape<WAVES, SB>{}) for the shape of a `tiles`-tile image (forward and backward alike)
template <class F>
static void with_fine_shape(int tiles, F&& f) {
    if (tiles <= 16) f(FineShape<4, 1>{});            // single pixels, G = 64
    else if (tiles <= 64) f(FineShape<4, 2>{});       // 2x2 sub-blocks, G = 16
    else if (tiles < 768) f(FineShape<4, 4>{});       // 4x4 sub-blocks, G = 4
    else f(FineShape<16, 4>{});                       // (>= 768 tiles — forced granularity only — one workgroup per tile fills the chip)
}

// Which kernel a `tiles`-tile image runs, decided once per launch from one load of each process-wide flag:
//   forward   granularity 2, or granularity 0 and tiles < FINE_MAX_TILES_FWD     Fine
//             otherwise                                                          Quadrant (the quadrant-list kernel)
//   backward  granularity 2 (whatever the generation)                            Fine
//             granularity 0, generation 0 and tiles < FINE_MAX_TILES_BWD         Fine
//             otherwise generation 1, or generation 0 and tiles < BWD_GEN2_MIN_TILES   Quadrant (four waves per tile)
//             otherwise (generation 2, or generation 0 from BWD_GEN2_MIN_TILES on)     Tile (one wave per tile)
// (a forced generation switches the by-tile-count Fine choice off in the backward only)
enum class FwdRoute { Quadrant, Fine };
enum class BwdRoute { Fine, Quadrant, Tile };
struct Routes { FwdRoute fwd; BwdRoute bwd; };
static Routes routes(int tiles) {
    const int gran = g_granularity.load(), gen = g_bwd_gen.load();
    Routes r;
    r.fwd = gran == 2 || (gran == 0 && tiles < FINE_MAX_TILES_FWD) ? FwdRoute::Fine : FwdRoute::Quadrant;
    if (gran == 2 || (gran == 0 && gen == 0 && tiles < FINE_MAX_TILES_BWD)) r.bwd = BwdRoute::Fine;
    else r.bwd = (gen ? gen == 1 : tiles < BWD_GEN2_MIN_TILES) ? BwdRoute::Quadrant : BwdRoute::Tile;
    return r;
}

// ---------------------------------------------------------------------------------------------
// Launch order of the one-wave-per-tile backward.  A tile is ONE sequential wave there and a SIMD holds six of them, about eight
// tiles per SIMD in total at 1080p: with tiles dispatched in image order the SIMDs run dry at very different times (measured:
// the number of running waves falls linearly over the second half of the kernel).  Dispatching the heaviest tiles first
// leaves only light tiles for the end.  Key = the forward's per-tile traversal length (tile_last), NOT the list length: with
// early termination the two differ by 2.3x on average and by much more per tile.  One 256-thread block per XCD run of the
// swizzled order (the tiles of a run stay on their XCD): counting sort into 2048 bins of 8 entries, heaviest first.
// ---------------------------------------------------------------------------------------------
namespace {
constexpr int ORDER_BINS = 2048, ORDER_SHIFT = 3;
// (One global heaviest-first sequence dealt to the XCDs round-robin was measured too: no better, and it gives up the L2 locality
//  of the contiguous runs.)
// (256 threads per block since round 4: a 1024-thread block needs sixteen free wave slots on ONE CU, and with a second view in
//  flight — host/multi_view.py — it waited 30-45 us for them behind the other view's blend workgroups; four slots are found at once)
constexpr int ORDER_THREADS = 256, ORDER_PER_THREAD = ORDER_BINS / ORDER_THREADS;
__global__ __launch_bounds__(ORDER_THREADS) void tile_order_kernel(int num_tiles, const uint32_t* __restrict__ tile_last,
                                                                   uint32_t* __restrict__ order) {
    __shared__ uint32_t s_bin[ORDER_BINS];
    __shared__ uint32_t s_wave[ORDER_THREADS / 64];
    const int per = num_tiles >> 3, main = per << 3;
    const int x = blockIdx.x;                           // XCD run x: swizzled positions = tiles [x * per, (x + 1) * per)
    const int tid = threadIdx.x;
    for (int b = tid; b < ORDER_BINS; b += ORDER_THREADS) s_bin[b] = 0;
    __syncthreads();
    for (int j = tid; j < per; j += ORDER_THREADS) {
        const uint32_t key = min(tile_last[x * per + j] >> ORDER_SHIFT, (uint32_t)(ORDER_BINS - 1));
        atomicAdd(&s_bin[ORDER_BINS - 1 - key], 1u);    // bin 0 = heaviest
    }
    __syncthreads();
    // exclusive scan of the 2048 bins: ORDER_PER_THREAD consecutive bins per thread
    uint32_t c[ORDER_PER_THREAD], v = 0;
#pragma unroll
    for (int k = 0; k < ORDER_PER_THREAD; ++k) { c[k] = s_bin[ORDER_PER_THREAD * tid + k]; v += c[k]; }
    const int lane = tid & 63, w = tid >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t n = (uint32_t)__shfl_up((int)inc, off);
        if (lane >= off) inc += n;
    }
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int k = 0; k < w; ++k) base += s_wave[k];
    uint32_t run = base + inc - v;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < ORDER_PER_THREAD; ++k) { s_bin[ORDER_PER_THREAD * tid + k] = run; run += c[k]; }
    __syncthreads();
    for (int j = tid; j < per; j += ORDER_THREADS) {
        const uint32_t t = (uint32_t)(x * per + j);
        const uint32_t key = min(tile_last[t] >> ORDER_SHIFT, (uint32_t)(ORDER_BINS - 1));
        const uint32_t pos = atomicAdd(&s_bin[ORDER_BINS - 1 - key], 1u);
        order[x * per + pos] = t;
    }
    if (x == 0) {
        for (int t = main + tid; t < num_tiles; t += ORDER_THREADS) order[t] = (uint32_t)t;      // ragged tail: identity
        if (tid == 0) order[num_tiles] = TILE_ORDER_MAGIC;     // visible to the backward through the stream order
    }
}
}  // namespace

hipError_t launch_tile_order(const ViewParams& vp, const uint32_t* tile_last, uint32_t* tile_order, hipStream_t s) {
    const int tiles = vp.gx * vp.gy;
    const Routes r = routes(tiles);
    // the fine-grained forward kernels do not write tile_last (and clear the order's validity word): no order from garbage
    if (tiles < 8 || r.bwd != BwdRoute::Tile || r.fwd == FwdRoute::Fine) return hipSuccess;
    hipLaunchKernelGGL(tile_order_kernel, dim3(8), dim3(ORDER_THREADS), 0, s, tiles, tile_last, tile_order);
    return hipGetLastError();
}

hipError_t launch_blend_forward(const ViewParams& vp, const char* geom, const uint32_t* ids, const uint2* ranges,
                                float* out_color, float* out_ps, float* out_depth, float* final_T,
                                uint32_t* n_contrib, uint32_t* tile_last, void* clear_ptr, size_t clear_bytes, hipStream_t s,
                                const FwdSlabArgs* slab) {
    const int tiles = vp.gx * vp.gy;
    if (tiles == 0) return clear_ptr && clear_bytes ? launch_zero(clear_ptr, clear_bytes, s) : hipSuccess;
    const GaussRec* rec = reinterpret_cast<const GaussRec*>(geom);   // GeomLayout::rec == 0
    // the gradient records are cleared by the blend kernel itself when it has enough workgroups to spread the stores over the
    // chip; with few tiles (low pyramid levels: 2 .. 500 workgroups, measured 150 -> 410 us at 2 tiles for 80 MB) a fill
    // kernel in front of it is faster
    static_assert(GRAD_REC_BYTES % 16 == 0, "the forward clears the gradient records in 16-byte words");
    const bool inline_clear = clear_ptr && clear_bytes && tiles >= CLEAR_INLINE_MIN_TILES;
    if (clear_ptr && clear_bytes && !inline_clear) {
        hipError_t e = launch_zero(clear_ptr, clear_bytes, s);
        if (e != hipSuccess) return e;
    }
    uint4* const cp = inline_clear ? reinterpret_cast<uint4*>(clear_ptr) : nullptr;
    const size_t cn = inline_clear ? clear_bytes / 16 : 0;
    // tile_last sits in front of tile_order in the image state (ImageLayout): the order's validity word
    uint32_t* order_flag = tile_last ? reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(tile_last) +
                                                                   align256(4 * (size_t)tiles)) + tiles : nullptr;
    FwdSlab sb{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (slab) {
        sb.dtrav = slab->dtrav;
        if (slab->pass == 1) { sb.open_bits = slab->open_bits; sb.open_list = slab->open_list; sb.n_open = slab->n_open; }
        if (slab->pass == 2) { sb.tile_list = slab->open_list; sb.n_tiles = slab->n_open; }
    }
    if (routes(tiles).fwd == FwdRoute::Fine) {   // few tiles (low pyramid levels): one wave per sub-block, the tile split over G workgroups
        if (slab && slab->pass != 0) return hipErrorInvalidValue;        // (the caller engages slabs from SLAB_MIN_TILES tiles on)
        with_fine_shape(tiles, [&](auto shape) {
            using S = decltype(shape);
            hipLaunchKernelGGL((blend_forward_fine_kernel<S::waves, S::sb>), dim3(tiles * S::groups), dim3(64 * S::waves), 0, s, vp, rec,
                               ids, ranges, out_color, out_ps, out_depth, final_T, n_contrib, cp, cn, order_flag);
        });
    } else {
        // slab B walks the list of open tiles with a grid that fills the chip once (normally a handful of tiles)
        const int grid = sb.tile_list ? std::min(tiles, 2048) : tiles;
        hipLaunchKernelGGL(blend_forward_kernel<false>, dim3(grid), dim3(256), 0, s, vp, rec, ids, ranges, out_color, out_ps,
                           out_depth, final_T, n_contrib, (unsigned long long*)nullptr, cp, cn, tile_last, order_flag, sb);
    }
    return hipGetLastError();
}

hipError_t launch_forward_feedback(const unsigned long long* dtrav, const SlabHeader* hdr, int slab_mode, int64_t D,
                                   const uint32_t* D_dev, uint32_t tag, uint64_t ticket, uint64_t* host_mapped, hipStream_t s) {
    if (!host_mapped || !dtrav) return hipSuccess;
    hipLaunchKernelGGL(forward_feedback_kernel, dim3(1), dim3(64), 0, s, dtrav, hdr, slab_mode, D, D_dev, tag, ticket,
                       (volatile uint64_t*)host_mapped);
    return hipGetLastError();
}

// does the forward of a `tiles`-tile image run the quadrant-list kernel (the one that can publish open tiles / tile lengths)?
bool forward_uses_quadrant_kernel(int tiles) { return tiles > 0 && routes(tiles).fwd == FwdRoute::Quadrant; }

hipError_t launch_blend_backward(const ViewParams& vp, const char* geom, const uint32_t* ids, const uint2* ranges,
                                 const float* final_T, const uint32_t* n_contrib, const float* dL_dcolor,
                                 grad_acc_t* grad_rec, hipStream_t s, const uint32_t* tile_order, const float* dL_ddepth,
                                 const float* dL_dalpha) {
    const int tiles = vp.gx * vp.gy;
    if (tiles == 0) return hipSuccess;
    const GaussRec* rec = reinterpret_cast<const GaussRec*>(geom);
    const BwdRoute route = routes(tiles).bwd;
    // dL_ddepth != nullptr: the depth variants of the same three kernels (same route choice, record slot 9 = dL/dz)
    // dL_dalpha != nullptr: the alpha variants (msgs_backward_with_alpha), again the same three kernels and the same route
    with_bool(dL_ddepth != nullptr, [&](auto DEPTH) { with_bool(dL_dalpha != nullptr, [&](auto ALPHA) {
        constexpr int CH = decltype(DEPTH)::value ? 4 : 3;
        constexpr bool AL = decltype(ALPHA)::value;
        if (route == BwdRoute::Fine)
            with_fine_shape(tiles, [&](auto shape) {
                using S = decltype(shape);
                hipLaunchKernelGGL((blend_backward_fine_kernel<S::waves, S::sb, CH, AL>), dim3(tiles * S::groups), dim3(64 * S::waves), 0, s,
                                   vp, rec, ids, ranges, final_T, n_contrib, dL_dcolor, grad_rec, dL_ddepth, dL_dalpha);
            });
        else if (route == BwdRoute::Tile)
            hipLaunchKernelGGL((blend_backward_tile_kernel<false, CH, AL>), dim3(tiles), dim3(64), 0, s, vp, rec, ids, ranges, final_T,
                               n_contrib, dL_dcolor, (void*)grad_rec, tile_order, dL_ddepth, dL_dalpha);
        else
            hipLaunchKernelGGL((blend_backward_kernel<CH, AL>), dim3(tiles), dim3(256), 0, s, vp, rec, ids, ranges, final_T, n_contrib,
                               dL_dcolor, grad_rec, dL_ddepth, dL_dalpha);
    }); });
    return hipGetLastError();
}

// msgs_absgrad: zero fill of the [P, 2] double accumulator, the replay (one of four <DEPTH, ALPHA> instantiations, the four-waves-
// per-tile shape whatever the tile count and whatever route the main backward takes), the finish.  P == 0 is the caller's.
hipError_t launch_blend_absgrad(const ReplayInputs& in, int P, const float* dL_dcolor, const float* dL_ddepth,
                                const float* dL_dalpha, double* acc, float* out, hipStream_t s) {
    const int tiles = in.vp.gx * in.vp.gy;
    hipError_t e = launch_zero(acc, 2 * sizeof(double) * (size_t)P, s);
    if (e != hipSuccess) return e;
    if (tiles > 0)
        with_bool(dL_ddepth != nullptr, [&](auto DEPTH) { with_bool(dL_dalpha != nullptr, [&](auto ALPHA) {
            hipLaunchKernelGGL((blend_absgrad_kernel<decltype(DEPTH)::value, decltype(ALPHA)::value>), dim3(tiles), dim3(256), 0, s,
                               in.vp, in.rec, in.ids, in.ranges, in.final_T, in.n_contrib, dL_dcolor, acc, dL_ddepth, dL_dalpha);
        }); });
    constexpr float LN2 = 0.69314718055994530942f;
    hipLaunchKernelGGL(absgrad_finish_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, LN2 * in.vp.W, LN2 * in.vp.H,
                       (const double*)acc, out);
    return hipGetLastError();
}

// msgs_contrib_accumulate: the replay (the four-waves-per-tile shape whatever the tile count) adds one view to `acc`, which the
// caller cleared or carries over from earlier views; msgs_contrib_finish: the accumulator as three [P] arrays.
hipError_t launch_blend_contrib(const ReplayInputs& in, const float* pixel_weights, void* acc, hipStream_t s) {
    const int tiles = in.vp.gx * in.vp.gy;
    if (tiles <= 0) return hipSuccess;
    with_bool(pixel_weights != nullptr, [&](auto WEIGHTED) {
        hipLaunchKernelGGL((blend_contrib_kernel<decltype(WEIGHTED)::value>), dim3(tiles), dim3(256), 0, s, in.vp, in.rec, in.ids,
                           in.ranges, in.final_T, in.n_contrib, pixel_weights, (ContribAcc*)acc);
    });
    return hipGetLastError();
}

hipError_t launch_contrib_finish(int P, const void* acc, float* weight_sum, float* weight_max, int64_t* pixel_count, hipStream_t s) {
    hipLaunchKernelGGL(contrib_finish_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, (const ContribAcc*)acc, weight_sum,
                       weight_max, (long long*)pixel_count);
    return hipGetLastError();
}

// msgs_features_forward / _backward: one launch per block of FEAT_CB channels (the four-waves-per-tile shape whatever the tile
// count).  16-byte row loads where every row of the block starts on a 16-byte boundary.
static bool feature_rows_vectorise(const float* features, int C) { return C % 4 == 0 && ((uintptr_t)features & 15) == 0; }

hipError_t launch_blend_features_forward(const ReplayInputs& in, const float* features, int C, float* out, hipStream_t s) {
    const int tiles = in.vp.gx * in.vp.gy;
    if (tiles <= 0) return hipSuccess;
    const int vec = feature_rows_vectorise(features, C);
    for (int c0 = 0; c0 < C; c0 += FEAT_CB)
        hipLaunchKernelGGL((blend_features_forward_kernel<FEAT_CB>), dim3(tiles), dim3(256), 0, s, in.vp, in.rec, in.ids, in.ranges,
                           in.final_T, in.n_contrib, features, C, c0, vec, out);
    return hipGetLastError();
}

// acc: [P, FEAT_CB] doubles, cleared here and again by every finish; grad_rec: NULL = no geometry share
hipError_t launch_blend_features_backward(const ReplayInputs& in, int P, const float* features, int C, const float* dL_dF,
                                          grad_acc_t* grad_rec, double* acc, float* dL_dfeatures, hipStream_t s) {
    const int tiles = in.vp.gx * in.vp.gy;
    if (tiles <= 0 || P <= 0) return hipSuccess;
    const int vec = feature_rows_vectorise(features, C);
    hipError_t e = launch_zero(acc, sizeof(double) * FEAT_CB * (size_t)P, s);
    if (e != hipSuccess) return e;
    const unsigned finish_blocks = (unsigned)(((size_t)P * FEAT_CB + 255) / 256);
    for (int c0 = 0; c0 < C; c0 += FEAT_CB) {
        with_bool(grad_rec != nullptr, [&](auto GEOM) {
            hipLaunchKernelGGL((blend_features_backward_kernel<FEAT_CB, decltype(GEOM)::value>), dim3(tiles), dim3(256), 0, s, in.vp,
                               in.rec, in.ids, in.ranges, in.final_T, in.n_contrib, features, C, c0, vec, dL_dF, grad_rec, acc);
        });
        hipLaunchKernelGGL((features_finish_kernel<FEAT_CB>), dim3(finish_blocks), dim3(256), 0, s, P, C, c0, acc, dL_dfeatures);
    }
    return hipGetLastError();
}
size_t features_scratch_bytes(int P) { return sizeof(double) * FEAT_CB * (size_t)(P > 0 ? P : 1); }

// msgs_distortion_forward / _backward (SPEC M13): one launch each, the four-waves-per-tile shape whatever the tile count
hipError_t launch_blend_distortion_forward(const ReplayInputs& in, float* out_distortion, float* out_moment, hipStream_t s) {
    const int tiles = in.vp.gx * in.vp.gy;
    if (tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(blend_distortion_forward_kernel, dim3(tiles), dim3(256), 0, s, in.vp, in.rec, in.ids, in.ranges, in.final_T,
                       in.n_contrib, out_distortion, out_moment);
    return hipGetLastError();
}
hipError_t launch_blend_distortion_backward(const ReplayInputs& in, const float* moment, const float* dL_ddist,
                                            grad_acc_t* grad_rec, hipStream_t s) {
    const int tiles = in.vp.gx * in.vp.gy;
    if (tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(blend_distortion_backward_kernel, dim3(tiles), dim3(256), 0, s, in.vp, in.rec, in.ids, in.ranges, in.final_T,
                       in.n_contrib, moment, dL_ddist, grad_rec);
    return hipGetLastError();
}

// msgs_median_depth_forward / _backward (SPEC M15): one launch each, one workgroup per tile
hipError_t launch_blend_median_depth_forward(const ReplayInputs& in, float* out_depth, int32_t* out_id, hipStream_t s) {
    const int tiles = in.vp.gx * in.vp.gy;
    if (tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(blend_median_depth_forward_kernel, dim3(tiles), dim3(256), 0, s, in.vp, in.rec, in.ids, in.ranges,
                       in.n_contrib, out_depth, out_id);
    return hipGetLastError();
}
hipError_t launch_median_depth_backward(const ViewParams& vp, int P, const int32_t* median_id, const float* dL_dmedian,
                                        grad_acc_t* grad_rec, hipStream_t s) {
    const int tiles = vp.gx * vp.gy;
    if (tiles <= 0 || P <= 0) return hipSuccess;
    hipLaunchKernelGGL(median_depth_backward_kernel, dim3(tiles), dim3(256), 0, s, vp, P, median_id, dL_dmedian, grad_rec);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Deterministic backward (msgs_set_deterministic): no float atomics.  K7 stores the nine sums of every tile entry;
// the entries are then grouped by Gaussian with a STABLE sort of (Gaussian id, entry position) and each Gaussian's
// entries are added in ascending entry position (= ascending tile id) by one thread.  Bitwise reproducible run to run.
// ---------------------------------------------------------------------------------------------
namespace {
// NF sums per entry and per Gaussian: DET_INST_FLOATS, or DET_INST_FLOATS_DEPTH with a depth gradient (the tenth: dL/dz)
template <int NF>
__global__ __launch_bounds__(256) void det_reduce_kernel(const uint32_t* __restrict__ gid_sorted,
                                                         const uint32_t* __restrict__ entry_of, int64_t D,
                                                         const double* __restrict__ inst_grad,
                                                         grad_acc_t* __restrict__ grad_rec, int rec_stride) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= D) return;
    const uint32_t g = gid_sorted[q];
    if (q > 0 && gid_sorted[q - 1] == g) return;               // not the head of its segment
    // the per-tile sums of one Gaussian are added in DOUBLE (exact for any realistic tile count): the deterministic mode
    // is the verification mode, and a Gaussian that covers hundreds of tiles otherwise loses ~1e-6 of its sums to float32
    // accumulation, which the conic -> covariance chain of K8 amplifies by the squared aspect ratio
    double acc[NF];
#pragma unroll
    for (int c = 0; c < NF; ++c) acc[c] = 0.0;
    for (int64_t k = q; k < D && gid_sorted[k] == g; ++k) {
        const double* src = inst_grad + (size_t)entry_of[k] * NF;
#pragma unroll
        for (int c = 0; c < NF; ++c) acc[c] += src[c];
    }
    grad_acc_t* dst = grad_rec + (size_t)g * rec_stride;
#pragma unroll
    for (int c = 0; c < NF; ++c) dst[c] = (grad_acc_t)acc[c];
}
}  // namespace

DetScratch::DetScratch(int64_t P, int64_t D, int nf) {
    const int64_t n = D > 0 ? D : 1;
    size_t o = 0;
    grad_rec = o;  o = align256(o + GRAD_REC_BYTES * (size_t)(P > 0 ? P : 1));
    inst_grad = o; o = align256(o + sizeof(double) * nf * (size_t)n);
    keys = o;      o = align256(o + 4 * (size_t)n);
    keys_s = o;    o = align256(o + 4 * (size_t)n);
    entry = o;     o = align256(o + 4 * (size_t)n);
    sort = o;      o = align256(o + SortScratch(n).total);
    total = o;
}

hipError_t launch_blend_backward_det(const ViewParams& vp, int P, const char* geom, const uint32_t* ids, int64_t D,
                                     const uint2* ranges, const float* final_T, const uint32_t* n_contrib,
                                     const float* dL_dcolor, char* scratch, hipStream_t s, const float* dL_ddepth,
                                     const float* dL_dalpha) {
    const int tiles = vp.gx * vp.gy;
    if (tiles == 0 || D <= 0) return hipSuccess;
    const int nf = dL_ddepth ? DET_INST_FLOATS_DEPTH : DET_INST_FLOATS;
    const DetScratch L(P, D, nf);
    grad_acc_t* grad_rec = (grad_acc_t*)(scratch + L.grad_rec);
    double* inst = (double*)(scratch + L.inst_grad);
    uint32_t* keys = (uint32_t*)(scratch + L.keys);
    uint32_t* keys_s = (uint32_t*)(scratch + L.keys_s);
    uint32_t* entry = (uint32_t*)(scratch + L.entry);
    hipError_t e = launch_zero(inst, sizeof(double) * nf * (size_t)D, s);
    if (e != hipSuccess) return e;
    // the reference's per-pixel backward restated literally (literal.hip): nine (ten) double sums per tile entry
    e = launch_blend_backward_literal(vp, geom, P, ids, ranges, final_T, n_contrib, dL_dcolor, inst, s, dL_ddepth, dL_dalpha);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(keys, ids, 4 * (size_t)D, hipMemcpyDeviceToDevice, s);      // the sort clobbers its input
    if (e != hipSuccess) return e;
    int bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < P) ++bits;
    e = radix_sort_pairs(keys, nullptr, keys_s, entry, D, 0, bits, scratch + L.sort, s);   // stable: entries ascending
    if (e != hipSuccess) return e;
    // ... added per Gaussian in ascending tile order: [P, 9] ([P, 10]) packed doubles, the textbook sums the per-Gaussian
    // backward takes (GRAD_REC_BYTES per Gaussian holds ten)
    static_assert(sizeof(grad_acc_t) == 8, "the verification mode's sums are doubles");
    static_assert(DET_INST_FLOATS_DEPTH <= GRAD_REC_FLOATS, "the [P, 10] sums fit the grad_rec region");
    with_bool(dL_ddepth != nullptr, [&](auto DEPTH) {
        constexpr int NF = decltype(DEPTH)::value ? DET_INST_FLOATS_DEPTH : DET_INST_FLOATS;
        hipLaunchKernelGGL(det_reduce_kernel<NF>, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, s, keys_s, entry, D, inst, grad_rec, NF);
    });
    return hipGetLastError();
}

// diagnostic: the quadrant-per-wave forward replayed with lane counters (no outputs written)
hipError_t launch_blend_backward_lane_stats(const ViewParams& vp, const char* geom, const uint32_t* ids, const uint2* ranges,
                                            const float* final_T, const uint32_t* n_contrib, unsigned long long* out4,
                                            hipStream_t s) {
    hipError_t e = hipMemsetAsync(out4, 0, 32, s);
    if (e != hipSuccess) return e;
    const int tiles = vp.gx * vp.gy;
    if (tiles)
        hipLaunchKernelGGL(blend_backward_tile_kernel<true>, dim3(tiles), dim3(64), 0, s, vp,
                           reinterpret_cast<const GaussRec*>(geom), ids, ranges, final_T, n_contrib, (const float*)nullptr, (void*)out4,
                           (const uint32_t*)nullptr, (const float*)nullptr, (const float*)nullptr);
    return hipGetLastError();
}

hipError_t launch_blend_lane_stats(const ViewParams& vp, const char* geom, const uint32_t* ids, const uint2* ranges,
                                   unsigned long long* out3, hipStream_t s) {
    hipError_t e = hipMemsetAsync(out3, 0, 24, s);
    if (e != hipSuccess) return e;
    const int tiles = vp.gx * vp.gy;
    if (tiles)
        hipLaunchKernelGGL(blend_forward_kernel<true>, dim3(tiles), dim3(256), 0, s, vp, reinterpret_cast<const GaussRec*>(geom),
                           ids, ranges, (float*)nullptr, (float*)nullptr, (float*)nullptr, (float*)nullptr,
                           (uint32_t*)nullptr, out3, (uint4*)nullptr, (size_t)0, (uint32_t*)nullptr, (uint32_t*)nullptr,
                           FwdSlab{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr});
    return hipGetLastError();
}

hipError_t launch_binning_stats(const ViewParams& vp, int P, const int32_t* radii, const uint32_t* n_contrib,
                                unsigned long long* out2, hipStream_t s) {
    hipError_t e = hipMemsetAsync(out2, 0, 16, s);
    if (e != hipSuccess) return e;
    const int tiles = vp.gx * vp.gy;
    if (tiles) hipLaunchKernelGGL(tile_stats_kernel, dim3(tiles), dim3(256), 0, s, vp, n_contrib, out2);
    if (P) hipLaunchKernelGGL(visible_count_kernel, dim3((P + 255) / 256), dim3(256), 0, s, P, radii, out2);
    return hipGetLastError();
}

}  // namespace msgs

#if defined(MSGS_TRACE_TILES)
extern "C" int msgs_debug_set_tile_trace(void* p) {
    hipLaunchKernelGGL(msgs::trace_set_kernel, dim3(1), dim3(1), 0, 0, (unsigned long long*)p);
    return (int)hipDeviceSynchronize();
}
#endif

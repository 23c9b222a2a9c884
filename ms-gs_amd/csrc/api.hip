// api.hip — the extern "C" entry points of libmsgs_hip.so declared in include/msgs.h.
// Host-side orchestration only: argument checks, workspace carving, kernel launches on the caller's
// stream.  No allocation, no global mutable state, one stream synchronisation (stage 1's instance
// count) outside debug mode.
#include "msgs_internal.h"

#include <atomic>
#include <new>

#include <cstring>

using namespace msgs;

namespace {

struct Timer {
    const msgs_timing_t* t;
    hipStream_t s;
    void begin(int k) const { if (t && t->ev[2 * k]) (void)hipEventRecord((hipEvent_t)t->ev[2 * k], s); }
    void end(int k) const { if (t && t->ev[2 * k + 1]) (void)hipEventRecord((hipEvent_t)t->ev[2 * k + 1], s); }
};

inline int check_inputs(const msgs_view_t* v, const msgs_gaussians_t* g) {
    if (!v || !g) return MSGS_ERR_INVALID_ARG;
    if (g->P < 0 || v->image_width <= 0 || v->image_height <= 0) return MSGS_ERR_INVALID_ARG;
    if (!v->bg || !v->viewmatrix || !v->projmatrix || !v->campos) return MSGS_ERR_INVALID_ARG;
    if (g->P > 0 && (!g->means3D || !g->opacities)) return MSGS_ERR_INVALID_ARG;
    if (g->raw_params) {      // 1: raw GaussianModel parameters; 2: activated inputs + chained gradients (msgs.h)
        if (g->raw_params != 1 && g->raw_params != 2) return MSGS_ERR_INVALID_ARG;
        if (!g->features_dc || !g->features_rest || !g->scales || !g->rotations) return MSGS_ERR_INVALID_ARG;
        if (g->raw_params == 2 && !g->rotations_raw) return MSGS_ERR_INVALID_ARG;
        if ((g->shs && g->raw_params != 2) || g->colors_precomp || g->cov3D_precomp) return MSGS_ERR_INVALID_ARG;
        if (v->sh_degree < 0 || v->sh_degree > 3 || v->sh_coeffs != 16) return MSGS_ERR_SH_DEGREE;
        if ((v->image_width + TILE - 1) / TILE > 65535 || (v->image_height + TILE - 1) / TILE > 65535)
            return MSGS_ERR_INVALID_ARG;
        return MSGS_OK;
    }
    // exactly one of shs / colors_precomp, exactly one of (scales, rotations) / cov3D_precomp
    // (upstream raises on both-or-neither)
    if ((g->shs != nullptr) == (g->colors_precomp != nullptr)) return MSGS_ERR_INVALID_ARG;
    const bool sr = g->scales != nullptr && g->rotations != nullptr;
    if ((g->scales != nullptr) != (g->rotations != nullptr)) return MSGS_ERR_INVALID_ARG;
    if (sr == (g->cov3D_precomp != nullptr)) return MSGS_ERR_INVALID_ARG;
    if (g->shs) {
        if (v->sh_degree < 0 || v->sh_degree > 3) return MSGS_ERR_SH_DEGREE;
        if ((v->sh_degree + 1) * (v->sh_degree + 1) > v->sh_coeffs) return MSGS_ERR_SH_DEGREE;
    }
    if ((v->image_width + TILE - 1) / TILE > 65535 || (v->image_height + TILE - 1) / TILE > 65535)
        return MSGS_ERR_INVALID_ARG;
    return MSGS_OK;
}

inline int debug_sync(const msgs_view_t* v, hipStream_t s) {
    if (!v->debug) return MSGS_OK;
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return (int)e;
    e = hipGetLastError();
    return e == hipSuccess ? MSGS_OK : (int)e;
}

inline int tile_bits(int num_tiles) {   // bits needed for tile ids 0..num_tiles (sentinel included)
    int b = 1;
    while ((1ll << b) <= (long long)num_tiles) ++b;
    return b;
}

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) return (int)_e;           \
    } while (0)

}  // namespace

extern "C" {

int msgs_abi_version(void) { return MSGS_ABI_VERSION; }

const char* msgs_error_string(int code) {
    switch (code) {
        case MSGS_OK: return "ok";
        case MSGS_ERR_INVALID_ARG: return "invalid argument (NULL or inconsistent pointers: provide exactly one of shs/colors_precomp and exactly one of scales+rotations/cov3D_precomp)";
        case MSGS_ERR_CAPACITY: return "a caller-supplied buffer is smaller than its size query";
        case MSGS_ERR_TOO_MANY: return "more than 2^32-1 tile instances";
        case MSGS_ERR_SH_DEGREE: return "sh_degree must be 0..3 and (sh_degree+1)^2 <= sh_coeffs";
        case MSGS_ERR_INTERNAL: return "internal error: a look-back wait in the sort/scan kernels timed out";
        case MSGS_ERR_NO_WEIGHT: return "no row of positive weight to sample from";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

size_t msgs_geom_bytes(int32_t P) { return GeomLayout(P > 0 ? P : 1).total; }
size_t msgs_stage1_scratch_bytes(int32_t P) { return Stage1Scratch(P > 0 ? P : 1).total; }
size_t msgs_binning_bytes(int64_t D, int32_t W, int32_t H) {
    return BinningLayout(D, (int64_t)((W + TILE - 1) / TILE) * ((H + TILE - 1) / TILE)).total;
}
size_t msgs_stage2_scratch_bytes(int64_t D, int32_t W, int32_t H) {
    (void)W; (void)H;
    const Stage2Scratch L(D);
    return L.total + align256(4 * (size_t)(D > 0 ? D : 1));   // + sorted key buffer
}
static int64_t tiles_of(int32_t W, int32_t H) { return (int64_t)((W + TILE - 1) / TILE) * ((H + TILE - 1) / TILE); }
size_t msgs_binning_bytes_slab(int64_t D, int32_t W, int32_t H, float fraction) {
    if (!(fraction > 0.f)) return msgs_binning_bytes(D, W, H);
    return msgs_binning_bytes(SlabGeom::ids_needed(D > 0 ? D : 1, (double)fraction, tiles_of(W, H)), W, H);
}
size_t msgs_stage2_scratch_bytes_slab(int64_t D, int32_t W, int32_t H) {
    return msgs_stage2_scratch_bytes((D > 0 ? D : 1) + SLAB_SLACK + 256, W, H);
}
size_t msgs_image_bytes(int32_t W, int32_t H) { return ImageLayout(W, H).total; }
size_t msgs_backward_scratch_bytes(int32_t P) {
    return align256(GRAD_REC_BYTES * (size_t)(P > 0 ? P : 1));
}
size_t msgs_backward_scratch_bytes_deterministic(int32_t P, int64_t D) { return DetScratch(P, D).total; }
size_t msgs_backward_scratch_bytes_deterministic_depth(int32_t P, int64_t D) { return DetScratch(P, D, DET_INST_FLOATS_DEPTH).total; }

static std::atomic<int> g_deterministic{[] { const char* e = getenv("MSGS_DETERMINISTIC"); return (e && e[0] == '1') ? 1 : 0; }()};
int msgs_set_deterministic(int32_t on) { return g_deterministic.exchange(on ? 1 : 0); }
int msgs_get_deterministic(void) { return g_deterministic.load(); }
int msgs_set_backward_generation(int32_t gen) { return set_backward_generation(gen); }
int msgs_set_blend_granularity(int32_t mode) { return set_blend_granularity(mode); }
int msgs_set_occlusion(int32_t on) { return set_occlusion(on); }
int msgs_set_depth_sort(int32_t mode) { return set_depth_sort(mode); }

}  // extern "C"

namespace {
// The caller's stage-2 buffers and outputs: the arguments of msgs_forward_stage2 behind D, as every forward entry point takes them
struct Stage2Buffers {
    void* binning; size_t binning_bytes;
    void* scratch2; size_t scratch2_bytes;
    void* image; size_t image_bytes;
    float* out_color; float* out_acc_ps; float* out_depth;
    void* grad_records; size_t grad_records_bytes;
    int backward_follows;
};

// Speculative stage 2 (msgs_forward): everything stage 2 needs, handed to stage 1 so that it can launch stage 2 on the caller's
// capacity-sized buffers right behind its own last kernel — BEFORE the host waits for the instance count.  The stage-2 kernels then
// read min(D, capacity) from a device word the scan writes; the host checks D <= capacity afterwards (and the caller redoes
// stage 2 on exact buffers when the scene outgrew the guess).  Without it the GPU idled ~14 us per step between the scan and
// the emit while the host learned D and launched (profiles/r3_idle.txt).
struct SpecStage2 {
    int64_t capacity;
    Stage2Buffers buf;
    int launched_rc;           // out: status of the speculative launch
};
int forward_stage2_impl(const msgs_view_t* view, const msgs_gaussians_t* g, const void* geom_v, size_t geom_bytes, int64_t D,
                        const Stage2Buffers& b, const msgs_timing_t* timing, void* stream, const uint32_t* D_dev,
                        uint64_t* fb_dev, uint64_t fb_ticket);

// The instance count D comes back through three pinned, device-mapped host words {D, flags, ticket} that a kernel writes
// itself and the host polls: no copy command, no interrupt-driven wait (a blocking hipStreamSynchronize wakes up tens of
// microseconds after the data landed, and until stage 2 is launched the GPU idles).  Block 0 of the scan's second kernel —
// which sums every block total — writes them first thing, so the host learns D while the last stage-1 kernel still runs.  MSGS_BLOCKING_SYNC=1, or a failed pinned allocation, falls back to a 16-byte copy +
// hipStreamSynchronize.  msgs_forward / msgs_forward_stage1 use one block per calling host thread (they wait before they
// return); msgs_forward_launch takes the block of the caller's msgs_status_t, so that any number of forwards can be in
// flight from one thread, one per handle.
struct StatusBlock {
    uint64_t* host = nullptr;
    uint64_t* dev = nullptr;
    uint64_t ticket = 0;
    bool tried = false;
    void ensure() {
        if (tried) return;
        tried = true;
        void* h = nullptr;
        if (hipHostMalloc(&h, 64, hipHostMallocPortable | hipHostMallocMapped) == hipSuccess) {
            void* d = nullptr;
            if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess) {
                host = (uint64_t*)h;
                dev = (uint64_t*)d;
                for (int k = 0; k < 8; ++k) host[k] = 0;
            } else {
                (void)hipHostFree(h);
            }
        }
        (void)hipGetLastError();
    }
    void release() {
        if (host) (void)hipHostFree(host);
        host = dev = nullptr;
        tried = false;
    }
};

// a stage 1 whose instance count has not been read back yet
struct PendingCount {
    bool active = false;
    bool polled = false;
    hipStream_t stream = nullptr;
    uint64_t ticket = 0;
    volatile uint64_t* host = nullptr;
    const uint64_t* status_dev = nullptr;   // device copy of {D, flags, info}: the fallback when the flag never lands
};

// {cover candidates, any block closed} of the last forward whose count this host thread collected (msgs_forward_info)
thread_local uint64_t t_last_info = 0;
// words 4..7 of the status block as they stood when that count was collected: the feedback publication of an earlier forward
thread_local uint64_t t_last_feedback[4] = {0, 0, 0, 0};

static bool blocking_sync() {
    static const bool blocking = [] { const char* e = getenv("MSGS_BLOCKING_SYNC"); return e && e[0] == '1'; }();
    return blocking;
}

// Depth-slab binning for this call?  (msgs_view_t.slab_fraction; include/msgs.h)  Independent of the buffers, which
// SlabGeom checks.
static bool slab_wanted(const msgs_view_t* view, const msgs_gaussians_t* g) {
    const float f = view->slab_fraction;
    if (!(f > 0.f) || !(f <= 0.5f) || g->P <= 0 || g_deterministic.load() != 0) return false;
    const int64_t tiles = (int64_t)((view->image_width + TILE - 1) / TILE) * ((view->image_height + TILE - 1) / TILE);
    return tiles >= SLAB_MIN_TILES && tiles < 65535 * 16 && forward_uses_quadrant_kernel((int)tiles);
}

// Launches K1, the depth sort and the scan — and, with `spec`, stage 2 right behind them — WITHOUT waiting for D.
int forward_stage1_launch(const msgs_view_t* view, const msgs_gaussians_t* g, int32_t* radii, float* pixel_sizes,
                          void* geom_v, size_t geom_bytes, void* scratch_v, size_t scratch_bytes,
                          const msgs_timing_t* timing, void* stream, SpecStage2* spec, StatusBlock& sb,
                          PendingCount& pend) {
    pend.active = false;
    int rc = check_inputs(view, g);
    if (rc) return rc;
    const int P = g->P;
    if (P == 0) return MSGS_OK;
    if (!radii || !pixel_sizes || !geom_v || !scratch_v) return MSGS_ERR_INVALID_ARG;
    if (geom_bytes < msgs_geom_bytes(P) || scratch_bytes < msgs_stage1_scratch_bytes(P)) return MSGS_ERR_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    char* geom = (char*)geom_v;
    char* scratch = (char*)scratch_v;
    const GeomLayout GL(P);
    const Stage1Scratch SL(P);
    const ViewParams vp = make_view_params(view);
    const Timer tm{timing, s};

    // K1 also clears the depth sort's group-sum table (saves a fill launch) and the header of the occlusion cut-off
    // (enabled = 0, no candidates: what the emit reads when the pass does not run)
    ZeroJob zj1{nullptr, 0, (uint32_t*)(geom + GL.slab_hdr), (GL.occ_hdr - GL.slab_hdr) / 4 + sizeof(OccHeader) / 4 + 2 * (size_t)OCC_BUCKETS};
    // depth sort: the bucket path or the LSD passes, from P and the process-wide switch alone (sort.hip, depth_sort_uses_buckets)
    const bool sort1_buckets = depth_sort_uses_buckets(P);
    const bool sort1_prezeroed = sort1_buckets ? depth_sort_zero_region(P, scratch + SL.sort, &zj1.p0, &zj1.n0)
                                               : radix_sort_zero_region(P, 0, 32, scratch + SL.sort, &zj1.p0, &zj1.n0);
    // exact per-tile occlusion cut-off (occlusion.hip): on unless switched off
    const bool occlusion = get_occlusion() != 0;
    uint32_t* heavy_list = occlusion ? (uint32_t*)(scratch + SL.heavy_list) : nullptr;
    uint32_t* heavy_count = occlusion ? (uint32_t*)(scratch + SL.heavy_count) : nullptr;
    uint32_t* heavy_blk = occlusion ? (uint32_t*)(scratch + SL.heavy_blk) : nullptr;
    tm.begin(MSGS_K_PREPROCESS);
    // (verification mode: the kernel also leaves the raw conic and the effective opacity for the literal blend loops)
    HIP_TRY(launch_preprocess(vp, *g, radii, pixel_sizes, geom, s, zj1, heavy_list, heavy_count, heavy_blk, g_deterministic.load() != 0));
    if (occlusion)      // (timed with K1: two launches that leave at once when the view has no cover candidates)
        HIP_TRY(launch_occlusion(vp, P, geom, heavy_list, heavy_count, heavy_blk, (OccCand*)(scratch + SL.occ_cand), s));
    tm.end(MSGS_K_PREPROCESS);
    if ((rc = debug_sync(view, s))) return rc;

    // depth order of the Gaussians (not rendered -> key 0xFFFFFFFF -> sorted last, zero tiles); the sorted keys stay in geom:
    // the emit compares them with the tiles' cut-off keys
    if (!blocking_sync()) sb.ensure();
    const bool polled = !blocking_sync() && sb.host != nullptr;
    const uint64_t ticket = ++sb.ticket;
    uint64_t* total_dev = (uint64_t*)(scratch + SL.total_out);
    uint64_t* status_dev = total_dev + 2;
    uint32_t* clamped_dev = (uint32_t*)(total_dev + 5);       // min(D, capacity) for a speculative stage 2
    // the speculative stage 2's queue of heavy Gaussians starts empty (binning.hip): cleared by whoever publishes the count
    uint32_t* heavy_q_word = spec ? (uint32_t*)((char*)spec->buf.scratch2 + Stage2Scratch(spec->capacity).heavy_q) : nullptr;

    tm.begin(MSGS_K_DEPTH_SORT);
    if (sort1_buckets)   // (its two info words sit behind the SlabHeader, in the range K1 cleared: zero on the LSD path)
        HIP_TRY(depth_sort_buckets((const uint32_t*)(geom + GL.key), (uint32_t*)(geom + GL.skey), (uint32_t*)(geom + GL.order), P,
                                   scratch + SL.sort, s, sort1_prezeroed, (uint32_t*)(geom + GL.nvalid),
                                   (uint32_t*)(geom + GL.slab_hdr + DEPTH_SORT_INFO_OFFSET)));
    else
        HIP_TRY(radix_sort_pairs((uint32_t*)(geom + GL.key), nullptr, (uint32_t*)(geom + GL.skey),
                                 (uint32_t*)(geom + GL.order), P, 0, 32, scratch + SL.sort, s, sort1_prezeroed,
                                 (uint32_t*)(geom + GL.nvalid)));
    tm.end(MSGS_K_DEPTH_SORT);
    if ((rc = debug_sync(view, s))) return rc;
    tm.begin(MSGS_K_SCAN);
    HIP_TRY(exclusive_scan_u32((const uint32_t*)(geom + GL.tiles), (const uint32_t*)(geom + GL.order),
                               (uint32_t*)(geom + GL.offs), P, (uint64_t*)(scratch + SL.scan_partials), total_dev, s,
                               status_dev, polled ? sb.dev : nullptr, ticket,
                               (const uint32_t*)(geom + GL.nvalid), spec ? clamped_dev : nullptr,
                               spec ? (uint64_t)spec->capacity : 0, (const uint32_t*)(geom + GL.occ_hdr), heavy_q_word, nullptr,
                               // the counts sit below the Gaussians' coarse cell ranges; a view that may run in depth slabs gets the
                               // ranges in depth order (in offs_b: slab B's recount reads them and leaves its counts there)
                               vp.cell_sx >= 0 ? TILE_COUNT_MASK : 0xFFFFFFFFu,
                               vp.cell_sx >= 0 && slab_wanted(view, g) ? (uint32_t*)(geom + GL.offs_b) : nullptr,
                               &reinterpret_cast<SlabHeader*>(geom + GL.slab_hdr)->pad[0]));
    tm.end(MSGS_K_SCAN);
    pend.active = true;
    pend.polled = polled;
    pend.stream = s;
    pend.ticket = ticket;
    pend.host = sb.host;
    pend.status_dev = status_dev;
    if (spec)       // stage 2 goes out NOW, sized for the capacity; the GPU runs it while the host waits for D
        spec->launched_rc = forward_stage2_impl(view, g, geom_v, geom_bytes, spec->capacity, spec->buf, timing, stream,
                                                clamped_dev, polled ? sb.dev : nullptr, ticket);
    return MSGS_OK;
}

// Waits until the count of `pend` has landed (polls the pinned words; falls back to a device copy + synchronise).
int forward_stage1_wait(PendingCount& pend, int64_t* num_instances_host) {
    *num_instances_host = 0;
    if (!pend.active) { t_last_info = 0; for (int k = 0; k < 4; ++k) t_last_feedback[k] = 0; return MSGS_OK; }      // P == 0
    pend.active = false;
    hipStream_t s = pend.stream;
    uint64_t host_status[3] = {0, 0, 0};
    if (pend.polled) {
        volatile uint64_t* hv = pend.host;
        const uint64_t ticket = pend.ticket;
        uint64_t spins = 0;
        while (hv[2] != ticket) {
            if ((++spins & 0xFFFF) == 0) {                 // every 65536 polls: has the stream failed or finished?
                const hipError_t q = hipStreamQuery(s);
                if (q != hipErrorNotReady && q != hipSuccess) return (int)q;
                if (q == hipSuccess && hv[2] != ticket) {  // finished without the flag: fall back to the device copy
                    HIP_TRY(hipMemcpyAsync(host_status, pend.status_dev, sizeof(host_status), hipMemcpyDeviceToHost, s));
                    HIP_TRY(hipStreamSynchronize(s));
                    break;
                }
            }
        }
        if (hv[2] == ticket) { host_status[0] = hv[0]; host_status[1] = hv[1]; host_status[2] = hv[3]; }
        // feedback words (written by forward_feedback_kernel of an EARLIER forward on this block, the last word last): a
        // consistent snapshot or nothing
        for (int k = 0; k < 4; ++k) t_last_feedback[k] = 0;
        for (int attempt = 0; attempt < 4; ++attempt) {
            const uint64_t w7 = hv[7], w4 = hv[4], w5 = hv[5], w6 = hv[6];
            if (hv[7] == w7) { t_last_feedback[0] = w4; t_last_feedback[1] = w5; t_last_feedback[2] = w6; t_last_feedback[3] = w7; break; }
        }
    } else {
        for (int k = 0; k < 4; ++k) t_last_feedback[k] = 0;
        HIP_TRY(hipMemcpyAsync(host_status, pend.status_dev, sizeof(host_status), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    const uint64_t total = host_status[0];
    t_last_info = host_status[2];
    if (host_status[1] != 0) return MSGS_ERR_INTERNAL;
    if (total > 0xFFFFFFFFull) return MSGS_ERR_TOO_MANY;
    *num_instances_host = (int64_t)total;
    return MSGS_OK;
}

StatusBlock& thread_status_block() {
    static thread_local StatusBlock sb;           // (never freed: 64 bytes of pinned memory per calling host thread)
    return sb;
}

// largest D with bytes_of(D) <= bytes (bytes_of monotone); 0 if none
template <class F>
static int64_t max_instances_for(size_t bytes, F bytes_of) {
    if (bytes_of(1) > bytes) return 0;
    int64_t lo = 1, hi = 0xFFFFFFFFll;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (bytes_of(mid) <= bytes) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// instance capacities of the caller's stage-2 buffers: ids of `binning`, and what the scratch serves
void stage2_capacities(const msgs_view_t* view, size_t binning_bytes, size_t scratch2_bytes, int64_t& cb, int64_t& cs) {
    const int W0 = view->image_width, H0 = view->image_height;
    cb = max_instances_for(binning_bytes, [&](int64_t d) { return msgs_binning_bytes(d, W0, H0); });
    cs = max_instances_for(scratch2_bytes, [&](int64_t d) { return msgs_stage2_scratch_bytes(d, W0, H0); });
}

// speculative stage 2 on the caller's buffers: possible when they hold at least 4096 instances, the view is not in debug
// mode and the sort geometry can take its count from a device word
bool prepare_spec(const msgs_view_t* view, const msgs_gaussians_t* g, const Stage2Buffers& b, SpecStage2& spec) {
    if (view->debug || g->P <= 0 || !b.binning || !b.scratch2 || !b.image || !b.out_color || !b.out_acc_ps || !b.out_depth ||
        view->image_width <= 0 || view->image_height <= 0)
        return false;
    const int W0 = view->image_width, H0 = view->image_height;
    int64_t cb, cs;
    stage2_capacities(view, b.binning_bytes, b.scratch2_bytes, cb, cs);
    int64_t cap = cb < cs ? cb : cs;
    const int tiles0 = ((W0 + TILE - 1) / TILE) * ((H0 + TILE - 1) / TILE);
    if (slab_wanted(view, g)) {          // in slab mode the buffers serve fewer instances: slab A's ids sit in front of slab B's
        const SlabGeom SG(cb, cs, (double)view->slab_fraction, tiles0, (int64_t)1 << 40);
        if (SG.ok && SG.cap_d >= 4096) cap = SG.cap_d;      // (else: single pass on the whole capacity)
    }
    if (cap < 4096 || !radix_sort_supports_device_count(cap, 0, tile_bits(tiles0))) return false;
    spec.capacity = cap;
    spec.buf = b;
    spec.launched_rc = MSGS_OK;
    return true;
}

// A forward whose stage 1 is enqueued (with stage 2 behind it, if the buffers allowed) and whose count is not collected yet
struct ForwardLaunch {
    PendingCount pend;
    bool spec = false;           // stage 2 went out speculatively ...
    int64_t capacity = 0;        // ... for at most this many instances ...
    int launched_rc = MSGS_OK;   // ... and its launch returned this
};

// The launch step of msgs_forward, msgs_forward_stage1 and msgs_forward_launch: stage 1, and stage 2 speculatively behind it
// when `b` (nullable) allows.  Nothing is waited for.
int forward_launch(const msgs_view_t* view, const msgs_gaussians_t* g, int32_t* radii, float* pixel_sizes, void* geom,
                   size_t geom_bytes, void* scratch1, size_t scratch1_bytes, const Stage2Buffers* b,
                   const msgs_timing_t* timing, void* stream, StatusBlock& sb, ForwardLaunch& fl) {
    SpecStage2 spec{};
    fl.spec = b && prepare_spec(view, g, *b, spec);
    const int rc = forward_stage1_launch(view, g, radii, pixel_sizes, geom, geom_bytes, scratch1, scratch1_bytes, timing,
                                         stream, fl.spec ? &spec : nullptr, sb, fl.pend);
    if (rc) return rc;
    fl.capacity = spec.capacity;
    fl.launched_rc = spec.launched_rc;
    return MSGS_OK;
}

// The finish step: waits for the count; *stage2_done = 1 when the speculative stage 2 served it (D <= its capacity)
int forward_finish(ForwardLaunch& fl, int64_t* num_instances_host, int32_t* stage2_done) {
    *stage2_done = 0;
    const int rc = forward_stage1_wait(fl.pend, num_instances_host);
    if (rc) return rc;
    if (fl.spec && fl.launched_rc != MSGS_OK) return fl.launched_rc;
    *stage2_done = fl.spec && *num_instances_host <= fl.capacity;
    return MSGS_OK;
}

// stage 2 on buffers that serve D: msgs_forward_stage2, and msgs_forward's sequential route
int forward_stage2_exact(const msgs_view_t* view, const msgs_gaussians_t* g, const void* geom, size_t geom_bytes, int64_t D,
                         const Stage2Buffers& b, const msgs_timing_t* timing, void* stream) {
    uint64_t* fb_dev = nullptr;
    uint64_t fb_ticket = 0;
    if (view && view->feedback_tag != 0 && !blocking_sync()) {        // feedback goes to the calling thread's status block
        StatusBlock& sb = thread_status_block();
        sb.ensure();
        fb_dev = sb.dev;
        fb_ticket = sb.ticket;
    }
    return forward_stage2_impl(view, g, geom, geom_bytes, D, b, timing, stream, nullptr, fb_dev, fb_ticket);
}

}  // namespace

// the handle of msgs_forward_launch / msgs_forward_finish: its own pinned status block + the launch it is waiting for
struct msgs_status {
    StatusBlock sb;
    ForwardLaunch fl;
    bool launched = false;       // a msgs_forward_launch has not been finished yet
};

extern "C" {

int msgs_forward_stage1(const msgs_view_t* view, const msgs_gaussians_t* g, int32_t* radii, float* pixel_sizes,
                        void* geom_v, size_t geom_bytes, void* scratch_v, size_t scratch_bytes,
                        int64_t* num_instances_host, const msgs_timing_t* timing, void* stream) {
    if (!num_instances_host) return MSGS_ERR_INVALID_ARG;
    *num_instances_host = 0;
    ForwardLaunch fl;
    int32_t stage2_done;
    const int rc = forward_launch(view, g, radii, pixel_sizes, geom_v, geom_bytes, scratch_v, scratch_bytes, nullptr, timing,
                                  stream, thread_status_block(), fl);
    return rc ? rc : forward_finish(fl, num_instances_host, &stage2_done);
}

int msgs_status_create(msgs_status_t** out) {
    if (!out) return MSGS_ERR_INVALID_ARG;
    *out = new (std::nothrow) msgs_status();
    if (!*out) return (int)hipErrorOutOfMemory;
    if (!blocking_sync()) (*out)->sb.ensure();
    return MSGS_OK;
}

int msgs_status_destroy(msgs_status_t* st) {
    if (!st) return MSGS_OK;
    if (st->launched && st->fl.pend.active) (void)hipStreamSynchronize(st->fl.pend.stream);   // a kernel may still write the block
    st->sb.release();
    delete st;
    return MSGS_OK;
}

int msgs_forward_launch(const msgs_view_t* view, const msgs_gaussians_t* g, int32_t* radii, float* pixel_sizes, void* geom,
                        size_t geom_bytes, void* scratch1, size_t scratch1_bytes, void* binning, size_t binning_bytes,
                        void* scratch2, size_t scratch2_bytes, void* image, size_t image_bytes, float* out_color,
                        float* out_acc_ps, float* out_depth, void* grad_records, size_t grad_records_bytes,
                        int32_t backward_follows, msgs_status_t* status, const msgs_timing_t* timing, void* stream) {
    if (!view || !g || !status) return MSGS_ERR_INVALID_ARG;
    if (status->launched) return MSGS_ERR_INVALID_ARG;          // one launch per handle at a time
    const Stage2Buffers b{binning, binning_bytes, scratch2, scratch2_bytes, image, image_bytes, out_color, out_acc_ps, out_depth,
                          grad_records, grad_records_bytes, backward_follows};
    const int rc = forward_launch(view, g, radii, pixel_sizes, geom, geom_bytes, scratch1, scratch1_bytes, &b, timing, stream,
                                  status->sb, status->fl);
    if (rc) return rc;
    status->launched = true;
    return MSGS_OK;
}

int msgs_forward_finish(msgs_status_t* status, int64_t* num_instances_host, int32_t* stage2_done) {
    if (!status || !num_instances_host || !stage2_done) return MSGS_ERR_INVALID_ARG;
    *stage2_done = 0;
    *num_instances_host = 0;
    if (!status->launched) return MSGS_ERR_INVALID_ARG;
    status->launched = false;
    return forward_finish(status->fl, num_instances_host, stage2_done);
}

int msgs_forward(const msgs_view_t* view, const msgs_gaussians_t* g, int32_t* radii, float* pixel_sizes, void* geom,
                 size_t geom_bytes, void* scratch1, size_t scratch1_bytes, void* binning, size_t binning_bytes,
                 void* scratch2, size_t scratch2_bytes, void* image, size_t image_bytes, float* out_color,
                 float* out_acc_ps, float* out_depth, void* grad_records, size_t grad_records_bytes,
                 int32_t backward_follows, int64_t* num_instances_host, int32_t* stage2_done, const msgs_timing_t* timing,
                 void* stream) {
    if (!stage2_done) return MSGS_ERR_INVALID_ARG;
    *stage2_done = 0;
    if (!view || !g || !num_instances_host) return MSGS_ERR_INVALID_ARG;
    *num_instances_host = 0;
    const Stage2Buffers b{binning, binning_bytes, scratch2, scratch2_bytes, image, image_bytes, out_color, out_acc_ps, out_depth,
                          grad_records, grad_records_bytes, backward_follows};
    ForwardLaunch fl;
    int rc = forward_launch(view, g, radii, pixel_sizes, geom, geom_bytes, scratch1, scratch1_bytes, &b, timing, stream,
                            thread_status_block(), fl);
    if (!rc) rc = forward_finish(fl, num_instances_host, stage2_done);
    // a speculative stage 2 ran (is running) on these buffers, or ran truncated: then the caller redoes it on exact buffers
    if (rc || fl.spec) return rc;
    // the sequential route (no speculative launch: debug mode, no P, buffers below 4096 instances): stage 2 now, if the
    // buffers serve D
    const int64_t D = *num_instances_host;
    const int W = view->image_width, H = view->image_height;
    if (!binning || binning_bytes < msgs_binning_bytes(D, W, H)) return MSGS_OK;
    if (D > 0 && (!scratch2 || scratch2_bytes < msgs_stage2_scratch_bytes(D, W, H))) return MSGS_OK;
    if ((rc = forward_stage2_exact(view, g, geom, geom_bytes, D, b, timing, stream))) return rc;
    *stage2_done = 1;
    return MSGS_OK;
}

int msgs_preprocess_only(const msgs_view_t* view, const msgs_gaussians_t* g, int32_t* radii, float* pixel_sizes,
                         void* geom_v, size_t geom_bytes, void* stream) {
    int rc = check_inputs(view, g);
    if (rc) return rc;
    const int P = g->P;
    if (P == 0) return MSGS_OK;
    if (!radii || !pixel_sizes || !geom_v) return MSGS_ERR_INVALID_ARG;
    if (geom_bytes < msgs_geom_bytes(P)) return MSGS_ERR_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_preprocess(make_view_params(view), *g, radii, pixel_sizes, (char*)geom_v, s));
    return debug_sync(view, s);
}

int msgs_forward_stage2(const msgs_view_t* view, const msgs_gaussians_t* g, const void* geom_v, size_t geom_bytes,
                        int64_t D, void* binning_v, size_t binning_bytes, void* scratch_v, size_t scratch_bytes,
                        void* image_v, size_t image_bytes, float* out_color, float* out_acc_ps, float* out_depth,
                        void* grad_records, size_t grad_records_bytes, int32_t backward_follows, const msgs_timing_t* timing,
                        void* stream) {
    const Stage2Buffers b{binning_v, binning_bytes, scratch_v, scratch_bytes, image_v, image_bytes, out_color, out_acc_ps,
                          out_depth, grad_records, grad_records_bytes, backward_follows};
    return forward_stage2_exact(view, g, geom_v, geom_bytes, D, b, timing, stream);
}

}  // extern "C"

namespace {
// D_dev != nullptr: speculative launch — D is the CAPACITY (layouts, grids, sort geometry), the kernels read the instance count
// min(D_true, capacity) from *D_dev.
// fb_dev / fb_ticket: pinned status block (device address) for the feedback publication, msgs_view_t.feedback_tag.
int forward_stage2_impl(const msgs_view_t* view, const msgs_gaussians_t* g, const void* geom_v, size_t geom_bytes, int64_t D,
                        const Stage2Buffers& b, const msgs_timing_t* timing, void* stream, const uint32_t* D_dev,
                        uint64_t* fb_dev, uint64_t fb_ticket) {
    int rc = check_inputs(view, g);
    if (rc) return rc;
    if (D < 0 || D > 0xFFFFFFFFll) return MSGS_ERR_TOO_MANY;
    const int P = g->P, W = view->image_width, H = view->image_height;
    if (!b.binning || !b.image || !b.out_color || !b.out_acc_ps || !b.out_depth) return MSGS_ERR_INVALID_ARG;
    if (P > 0 && (!geom_v || geom_bytes < msgs_geom_bytes(P))) return MSGS_ERR_CAPACITY;
    if (b.binning_bytes < msgs_binning_bytes(D, W, H) || b.image_bytes < msgs_image_bytes(W, H)) return MSGS_ERR_CAPACITY;
    if (D > 0 && (!b.scratch2 || b.scratch2_bytes < msgs_stage2_scratch_bytes(D, W, H))) return MSGS_ERR_CAPACITY;
    if (b.grad_records && b.grad_records_bytes < msgs_backward_scratch_bytes(P)) return MSGS_ERR_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    char* geom = const_cast<char*>((const char*)geom_v);        // (slab mode writes its header and second scan into geom)
    char* binning = (char*)b.binning;
    char* scratch = (char*)b.scratch2;
    char* image = (char*)b.image;
    const ViewParams vp = make_view_params(view);
    const int num_tiles = vp.gx * vp.gy;
    const ImageLayout IL(W, H);
    const Timer tm{timing, s};
    const int tbits = tile_bits(num_tiles);
    // (ranges first, then ids: BinningLayout's positions do not depend on the instance count)
    const BinningLayout BL(D, num_tiles);
    uint32_t* ids = (uint32_t*)(binning + BL.ids);
    uint2* ranges = (uint2*)(binning + BL.ranges);
    float* final_T = (float*)(image + IL.final_T);
    uint32_t* n_contrib = (uint32_t*)(image + IL.n_contrib);
    uint32_t* tile_last = (uint32_t*)(image + IL.tile_last);
    const bool literal = g_deterministic.load() != 0;
    const bool feedback = view->feedback_tag != 0 && fb_dev != nullptr && P > 0 && forward_uses_quadrant_kernel(num_tiles) && !literal;
    unsigned long long* dtrav = feedback ? (unsigned long long*)(binning + BL.dtrav) : nullptr;
    const size_t clear_bytes = b.grad_records ? GRAD_REC_BYTES * (size_t)P : 0;

    // ---- depth slabs?  The buffers must serve this D in slab mode (SlabGeom); the speculative caller sized `D` accordingly
    bool slab = D > 0 && slab_wanted(view, g) && radix_sort_supports_device_count(D, 0, tbits);
    int64_t n_a_max = 0, cap_b = 0;
    if (slab) {
        int64_t cb, cs;
        stage2_capacities(view, b.binning_bytes, b.scratch2_bytes, cb, cs);
        const SlabGeom SG(cb, cs, (double)view->slab_fraction, num_tiles, D);
        slab = SG.ok && SG.cap_d == D && SortScratch(SG.n_a_max).total <= SortScratch(SG.cap_b).total;
        n_a_max = SG.n_a_max;
        cap_b = SG.cap_b;
    }

    // the scratch is laid out for the single pass's D, or for slab B's capacity (slab A uses its head)
    const Stage2Scratch SL(slab ? cap_b : D);
    uint32_t *keys_a = nullptr, *ids_a = nullptr, *keys_sorted = nullptr, *heavy_q = nullptr;
    bool keys16 = false;
    if (D > 0) {
        keys_a = (uint32_t*)(scratch + SL.keys_a);
        ids_a = (uint32_t*)(scratch + SL.ids_a);
        keys_sorted = (uint32_t*)(scratch + SL.total);
        // the queue of heavy Gaussians (binning.hip: one more launch) — not on a view the caller marked as ordinary
        // (msgs_view_t.no_heavy_queue: no covers closed anything lately, hence no crowd of giants in the first ranks either;
        // the few Gaussians with many instances are then emitted by their wave inside emit_kernel, as before round 5)
        heavy_q = view->no_heavy_queue ? nullptr : (uint32_t*)(scratch + SL.heavy_q);
        // tile ids (and the sentinel id = number of tiles) below 65536: the emit writes, the tile sort moves and the range
        // search reads 16-bit keys — 6 instead of 8 bytes per pair and pass
        keys16 = num_tiles < 65535 && radix_sort_keys16_ok(slab ? cap_b : D, 0, tbits) &&
                 (!slab || radix_sort_keys16_ok(n_a_max, 0, tbits));
    }

    // One binning pass: emit -> tile sort -> ranges of at most `cap` instances, their number read from *count (nullptr: exactly
    // `cap`); the sorted ids go to ids + base.  The emit also clears the tile sort's group-sum table and, with clear_ranges,
    // the tile-range array (fill launches less).  `t` closes the emit's span, which the caller opens, and times the tile sort
    // and the ranges.  cap == 0: no emit, no sort, only the ranges.
    auto bin_pass = [&](const uint32_t* count, int64_t cap, uint32_t base, int slab_pass, const uint32_t* open,
                        bool clear_ranges, bool ranges_prezeroed, int64_t density_D, const Timer& t) -> int {
        if (cap > 0) {
            ZeroJob zj{nullptr, 0, clear_ranges ? (uint32_t*)ranges : nullptr, clear_ranges ? BL.ranges_and_dtrav_words() : 0};
            const bool sort_prezeroed = radix_sort_zero_region(cap, 0, tbits, scratch + SL.sort, &zj.p0, &zj.n0);
            HIP_TRY(launch_emit(vp, P, geom, keys_a, ids_a, cap, s, zj, count, keys16, heavy_q, slab_pass, open, density_D));
            t.end(MSGS_K_EMIT);
            if ((rc = debug_sync(view, s))) return rc;
            t.begin(MSGS_K_TILE_SORT);
            HIP_TRY(radix_sort_pairs(keys_a, ids_a, keys_sorted, ids + base, cap, 0, tbits, scratch + SL.sort, s, sort_prezeroed,
                                     nullptr, count, keys16));
            t.end(MSGS_K_TILE_SORT);
            if ((rc = debug_sync(view, s))) return rc;
        }
        t.begin(MSGS_K_RANGES);
        HIP_TRY(launch_ranges(keys_sorted, cap, ranges, num_tiles, s, ranges_prezeroed, count, keys16, base));
        t.end(MSGS_K_RANGES);
        return MSGS_OK;
    };

    if (!slab) {
        if (D > 0) {
            if (heavy_q && !D_dev) HIP_TRY(launch_zero(heavy_q, 4, s));     // (a speculative launch had it cleared by stage 1's scan)
            tm.begin(MSGS_K_EMIT);
        }
        if ((rc = bin_pass(D_dev, D, 0, 0, nullptr, /*clear_ranges*/ true, /*ranges_prezeroed*/ D > 0, 0, tm))) return rc;
        if ((rc = debug_sync(view, s))) return rc;

        tm.begin(MSGS_K_BLEND_FWD);
        if (literal) {          // verification mode: the reference's per-pixel loop restated literally (literal.hip)
            if (b.grad_records && clear_bytes) HIP_TRY(launch_zero(b.grad_records, clear_bytes, s));
            HIP_TRY(launch_blend_forward_literal(vp, geom, P, ids, ranges, b.out_color, b.out_acc_ps, b.out_depth, final_T,
                                                 n_contrib, (uint32_t*)(image + IL.tile_order) + num_tiles, s));
        } else {
            if (D == 0 && dtrav) HIP_TRY(launch_zero(dtrav, 8 * (size_t)DTRAV_SLOTS, s));      // (no emit ran: nobody cleared them)
            const FwdSlabArgs fa{0, nullptr, nullptr, nullptr, dtrav};
            HIP_TRY(launch_blend_forward(vp, geom, ids, ranges, b.out_color, b.out_acc_ps, b.out_depth, final_T, n_contrib,
                                         tile_last, b.grad_records, clear_bytes, s, dtrav ? &fa : nullptr));
        }
    } else {
        // ---------------- slab A: the nearest ranks, up to slab_fraction * D instances ----------------
        const GeomLayout GL(P);
        SlabHeader* hdr = reinterpret_cast<SlabHeader*>(geom + GL.slab_hdr);
        uint32_t* open_bits = (uint32_t*)(image + IL.open_bits);
        uint32_t* open_list = (uint32_t*)(image + IL.open_list);
        tm.begin(MSGS_K_EMIT);
        HIP_TRY(launch_slab_split(P, geom, D, D_dev, view->slab_fraction, open_bits, num_tiles, s));
        if (heavy_q) HIP_TRY(launch_zero(heavy_q, 4, s));
        if ((rc = bin_pass(&hdr->DA, n_a_max, 0, 1, nullptr, /*clear_ranges*/ true, /*ranges_prezeroed*/ true, D, tm))) return rc;
        if ((rc = debug_sync(view, s))) return rc;
        tm.begin(MSGS_K_BLEND_FWD);
        const FwdSlabArgs fa{1, open_bits, open_list, &hdr->n_open, dtrav};
        HIP_TRY(launch_blend_forward(vp, geom, ids, ranges, b.out_color, b.out_acc_ps, b.out_depth, final_T, n_contrib, tile_last,
                                     b.grad_records, clear_bytes, s, &fa));
        tm.end(MSGS_K_BLEND_FWD);
        if ((rc = debug_sync(view, s))) return rc;

        // ---------------- slab B: the complete lists of the tiles slab A left open ----------------
        tm.begin(MSGS_K_SLAB_B);
        uint32_t* offs_b = (uint32_t*)(geom + GL.offs_b);
        HIP_TRY(launch_slab_recount(vp, P, geom, open_bits, open_list, D, D_dev, s));
        // the recount has consumed the cell ranges stage 1's scan left in offs_b (pad[0] = 1) and left its counts there: this
        // scan clears pad[0] (block 0, behind the recount in stream order), so that a second stage 2 on this geom — the redo of
        // a speculative one the view outgrew — recounts without the cell prefilter instead of decoding scan offsets as ranges
        HIP_TRY(exclusive_scan_u32(offs_b, nullptr, offs_b, P, (uint64_t*)(geom + GL.scan_b), &hdr->total_b, s, nullptr, nullptr, 0,
                                   (const uint32_t*)(geom + GL.nvalid), &hdr->DB, (uint64_t)cap_b, nullptr, heavy_q, &hdr->pad0,
                                   0xFFFFFFFFu, nullptr, &hdr->pad[0]));
        // (slab A's emit cleared the ranges; slab B's sub-steps are timed as a whole)
        if ((rc = bin_pass(&hdr->DB, cap_b, (uint32_t)n_a_max, 2, open_bits, /*clear_ranges*/ false, /*ranges_prezeroed*/ true, 0,
                           Timer{nullptr, s})))
            return rc;
        const FwdSlabArgs fb{2, open_bits, open_list, &hdr->n_open, dtrav};
        HIP_TRY(launch_blend_forward(vp, geom, ids, ranges, b.out_color, b.out_acc_ps, b.out_depth, final_T, n_contrib, tile_last,
                                     nullptr, 0, s, &fb));
        tm.end(MSGS_K_SLAB_B);
    }
    if (b.backward_follows && !literal)  // give the backward's one-wave-per-tile kernel a heaviest-first launch order
        HIP_TRY(launch_tile_order(vp, tile_last, (uint32_t*)(image + IL.tile_order), s));
    if (feedback) {
        const GeomLayout GL(P);
        HIP_TRY(launch_forward_feedback(dtrav, reinterpret_cast<const SlabHeader*>(geom + GL.slab_hdr), slab ? 1 : 0, D,
                                        D_dev, (uint32_t)view->feedback_tag, fb_ticket, fb_dev, s));
    }
    if (!slab) tm.end(MSGS_K_BLEND_FWD);
    return debug_sync(view, s);
}
}  // namespace

namespace {
// msgs_backward_with_depth (cam = NULL, dL_dalpha = NULL), msgs_backward_with_camera and msgs_backward_with_alpha
int backward_impl(const msgs_view_t* view, const msgs_gaussians_t* g, const int32_t* radii, const void* geom_v,
                  size_t geom_bytes, int64_t D, const void* binning_v, size_t binning_bytes, const void* image_v,
                  size_t image_bytes, const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha, void* scratch_v,
                  size_t scratch_bytes, const msgs_grads_t* grads, const CameraGrads* cam, const msgs_timing_t* timing,
                  void* stream);

// msgs_backward_with_camera (dL_dalpha = NULL) and msgs_backward_with_alpha: the camera arguments are checked in one place.
// No camera pointer: every mode of msgs_backward_with_depth (the optimizer step in the per-Gaussian kernel included)
int backward_camera_alpha(const msgs_view_t* view, const msgs_gaussians_t* g, const int32_t* radii, const void* geom_v,
                          size_t geom_bytes, int64_t D, const void* binning_v, size_t binning_bytes, const void* image_v,
                          size_t image_bytes, const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                          void* scratch_v, size_t scratch_bytes, const msgs_grads_t* grads, float* dL_dviewmatrix,
                          float* dL_dprojmatrix, float* dL_dcampos, void* camera_scratch, size_t camera_scratch_bytes,
                          const msgs_timing_t* timing, void* stream) {
    if (!dL_dviewmatrix && !dL_dprojmatrix && !dL_dcampos)
        return backward_impl(view, g, radii, geom_v, geom_bytes, D, binning_v, binning_bytes, image_v, image_bytes, dL_dcolor,
                             dL_ddepth, dL_dalpha, scratch_v, scratch_bytes, grads, nullptr, timing, stream);
    int rc = check_inputs(view, g);
    if (rc) return rc;
    if (!grads || grads->adam_in_backward) return MSGS_ERR_INVALID_ARG;      // out of scope: refused, not silently wrong
    if (g->P > 0 && !camera_scratch) return MSGS_ERR_INVALID_ARG;
    if (g->P > 0 && camera_scratch_bytes < msgs_camera_grad_scratch_bytes(g->P)) return MSGS_ERR_CAPACITY;
    CameraGrads cam{dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, (double*)camera_scratch};
    return backward_impl(view, g, radii, geom_v, geom_bytes, D, binning_v, binning_bytes, image_v, image_bytes, dL_dcolor,
                         dL_ddepth, dL_dalpha, scratch_v, scratch_bytes, grads, &cam, timing, stream);
}

// The forward state an opt-in replay reads (geometry, binning and image buffers of a P-Gaussian, D-instance forward of `view`) as
// the pointers its launcher takes.  MSGS_ERR_INVALID_ARG for a missing buffer, then MSGS_ERR_CAPACITY for one too small for
// msgs_geom_bytes / msgs_binning_bytes / msgs_image_bytes.  The caller has checked view, P, D and the image size.
int replay_inputs(const msgs_view_t* view, int32_t P, const void* geom, size_t geom_bytes, int64_t D, const void* binning_v,
                  size_t binning_bytes, const void* image_v, size_t image_bytes, ReplayInputs* in) {
    if (!geom || !binning_v || !image_v) return MSGS_ERR_INVALID_ARG;
    const int W = view->image_width, H = view->image_height;
    if (geom_bytes < msgs_geom_bytes(P) || binning_bytes < msgs_binning_bytes(D, W, H) || image_bytes < msgs_image_bytes(W, H))
        return MSGS_ERR_CAPACITY;
    in->vp = make_view_params(view);
    const BinningLayout BL(D, in->vp.gx * in->vp.gy);
    const ImageLayout IL(W, H);
    const char* binning = (const char*)binning_v;
    const char* image = (const char*)image_v;
    in->rec = (const GaussRec*)geom;                                         // GeomLayout::rec == 0
    in->ids = (const uint32_t*)(binning + BL.ids);
    in->ranges = (const uint2*)(binning + BL.ranges);
    in->final_T = (const float*)(image + IL.final_T);
    in->n_contrib = (const uint32_t*)(image + IL.n_contrib);
    return MSGS_OK;
}
}  // namespace

extern "C" {

int msgs_backward(const msgs_view_t* view, const msgs_gaussians_t* g, const int32_t* radii, const void* geom_v,
                  size_t geom_bytes, int64_t D, const void* binning_v, size_t binning_bytes, const void* image_v,
                  size_t image_bytes, const float* dL_dcolor, void* scratch_v, size_t scratch_bytes,
                  const msgs_grads_t* grads, const msgs_timing_t* timing, void* stream) {
    return msgs_backward_with_depth(view, g, radii, geom_v, geom_bytes, D, binning_v, binning_bytes, image_v, image_bytes,
                                    dL_dcolor, nullptr, scratch_v, scratch_bytes, grads, timing, stream);
}

int msgs_backward_with_depth(const msgs_view_t* view, const msgs_gaussians_t* g, const int32_t* radii, const void* geom_v,
                             size_t geom_bytes, int64_t D, const void* binning_v, size_t binning_bytes, const void* image_v,
                             size_t image_bytes, const float* dL_dcolor, const float* dL_ddepth, void* scratch_v,
                             size_t scratch_bytes, const msgs_grads_t* grads, const msgs_timing_t* timing, void* stream) {
    return backward_impl(view, g, radii, geom_v, geom_bytes, D, binning_v, binning_bytes, image_v, image_bytes, dL_dcolor,
                         dL_ddepth, nullptr, scratch_v, scratch_bytes, grads, nullptr, timing, stream);
}

size_t msgs_camera_grad_scratch_bytes(int32_t P) { return camera_grad_rows_bytes(P); }

int msgs_backward_with_camera(const msgs_view_t* view, const msgs_gaussians_t* g, const int32_t* radii, const void* geom_v,
                              size_t geom_bytes, int64_t D, const void* binning_v, size_t binning_bytes, const void* image_v,
                              size_t image_bytes, const float* dL_dcolor, const float* dL_ddepth, void* scratch_v,
                              size_t scratch_bytes, const msgs_grads_t* grads, float* dL_dviewmatrix, float* dL_dprojmatrix,
                              float* dL_dcampos, void* camera_scratch, size_t camera_scratch_bytes,
                              const msgs_timing_t* timing, void* stream) {
    return backward_camera_alpha(view, g, radii, geom_v, geom_bytes, D, binning_v, binning_bytes, image_v, image_bytes, dL_dcolor,
                                 dL_ddepth, nullptr, scratch_v, scratch_bytes, grads, dL_dviewmatrix, dL_dprojmatrix, dL_dcampos,
                                 camera_scratch, camera_scratch_bytes, timing, stream);
}

// (dL_dalpha = NULL: exactly msgs_backward_with_camera — the same call)
int msgs_backward_with_alpha(const msgs_view_t* view, const msgs_gaussians_t* g, const int32_t* radii, const void* geom_v,
                             size_t geom_bytes, int64_t D, const void* binning_v, size_t binning_bytes, const void* image_v,
                             size_t image_bytes, const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                             void* scratch_v, size_t scratch_bytes, const msgs_grads_t* grads, float* dL_dviewmatrix,
                             float* dL_dprojmatrix, float* dL_dcampos, void* camera_scratch, size_t camera_scratch_bytes,
                             const msgs_timing_t* timing, void* stream) {
    return backward_camera_alpha(view, g, radii, geom_v, geom_bytes, D, binning_v, binning_bytes, image_v, image_bytes, dL_dcolor,
                                 dL_ddepth, dL_dalpha, scratch_v, scratch_bytes, grads, dL_dviewmatrix, dL_dprojmatrix, dL_dcampos,
                                 camera_scratch, camera_scratch_bytes, timing, stream);
}

int msgs_alpha_map(const msgs_view_t* view, const void* image_v, size_t image_bytes, float* out_alpha, void* stream) {
    if (!view || !image_v || !out_alpha || view->image_width < 1 || view->image_height < 1) return MSGS_ERR_INVALID_ARG;
    const int W = view->image_width, H = view->image_height;
    if (image_bytes < msgs_image_bytes(W, H)) return MSGS_ERR_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    const ImageLayout IL(W, H);
    HIP_TRY(launch_alpha_map((const float*)((const char*)image_v + IL.final_T), out_alpha, (size_t)W * H, s));
    return debug_sync(view, s);
}

size_t msgs_bg_grad_scratch_bytes(int32_t width, int32_t height) {
    if (width < 1 || height < 1) return 0;
    return bg_grad_rows_bytes((size_t)width * height);
}

int msgs_bg_grad(const msgs_view_t* view, const void* image_v, size_t image_bytes, const float* dL_dcolor, float* dL_dbg,
                 void* scratch, size_t scratch_bytes, void* stream) {
    if (!view || !dL_dcolor || !dL_dbg || !scratch || view->image_width < 1 || view->image_height < 1)
        return MSGS_ERR_INVALID_ARG;
    if ((uintptr_t)scratch & 7) return MSGS_ERR_INVALID_ARG;                 // rows of doubles
    const int W = view->image_width, H = view->image_height;
    if (image_v && image_bytes < msgs_image_bytes(W, H)) return MSGS_ERR_CAPACITY;
    if (scratch_bytes < msgs_bg_grad_scratch_bytes(W, H)) return MSGS_ERR_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    const ImageLayout IL(W, H);
    HIP_TRY(launch_bg_grad(image_v ? (const float*)((const char*)image_v + IL.final_T) : nullptr, dL_dcolor, (size_t)W * H, dL_dbg,
                           (double*)scratch, s));
    return debug_sync(view, s);
}

size_t msgs_absgrad_scratch_bytes(int32_t P) { return 2 * sizeof(double) * (size_t)(P > 0 ? P : 1); }

int msgs_absgrad(const msgs_view_t* view, int32_t P, const void* geom_v, size_t geom_bytes, int64_t D, const void* binning_v,
                 size_t binning_bytes, const void* image_v, size_t image_bytes, const float* dL_dcolor, const float* dL_ddepth,
                 const float* dL_dalpha, void* scratch, size_t scratch_bytes, float* out_absgrad, void* stream) {
    if (!view || P < 0 || D < 0 || view->image_width < 1 || view->image_height < 1) return MSGS_ERR_INVALID_ARG;
    if (P == 0) return MSGS_OK;                                              // nothing to zero: out is [0, 3]
    if (!out_absgrad || !dL_dcolor || !scratch || !view->bg) return MSGS_ERR_INVALID_ARG;
    if ((uintptr_t)scratch & 7) return MSGS_ERR_INVALID_ARG;                 // rows of doubles
    ReplayInputs in;
    const int st = replay_inputs(view, P, geom_v, geom_bytes, D, binning_v, binning_bytes, image_v, image_bytes, &in);
    if (st != MSGS_OK) return st;
    if (scratch_bytes < msgs_absgrad_scratch_bytes(P)) return MSGS_ERR_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_blend_absgrad(in, P, dL_dcolor, dL_ddepth, dL_dalpha, (double*)scratch, out_absgrad, s));
    return debug_sync(view, s);
}

size_t msgs_contrib_scratch_bytes(int32_t P) { return CONTRIB_ACC_BYTES * (size_t)(P > 0 ? P : 1); }

int msgs_contrib_accumulate(const msgs_view_t* view, int32_t P, const void* geom_v, size_t geom_bytes, int64_t D,
                            const void* binning_v, size_t binning_bytes, const void* image_v, size_t image_bytes,
                            const float* pixel_weights, void* acc, size_t acc_bytes, int32_t clear_first, void* stream) {
    if (!view || P < 0 || D < 0 || view->image_width < 1 || view->image_height < 1 || !acc) return MSGS_ERR_INVALID_ARG;
    if ((uintptr_t)acc & 7) return MSGS_ERR_INVALID_ARG;                     // rows of {double, uint64, uint32}
    if (acc_bytes < msgs_contrib_scratch_bytes(P)) return MSGS_ERR_CAPACITY;
    const bool replay = P > 0 && D > 0;                                      // no instance: no pair, nothing to add
    ReplayInputs in;
    if (replay) {
        const int st = replay_inputs(view, P, geom_v, geom_bytes, D, binning_v, binning_bytes, image_v, image_bytes, &in);
        if (st != MSGS_OK) return st;
    }
    hipStream_t s = (hipStream_t)stream;
    if (clear_first && P > 0) HIP_TRY(launch_zero(acc, CONTRIB_ACC_BYTES * (size_t)P, s));
    if (!replay) return debug_sync(view, s);
    HIP_TRY(launch_blend_contrib(in, pixel_weights, acc, s));
    return debug_sync(view, s);
}

int msgs_contrib_finish(int32_t P, const void* acc, size_t acc_bytes, float* weight_sum, float* weight_max, int64_t* pixel_count,
                        void* stream) {
    if (P < 0) return MSGS_ERR_INVALID_ARG;
    if (P == 0) return MSGS_OK;                                              // the outputs are [0]
    if (!acc || !weight_sum || !weight_max || !pixel_count || ((uintptr_t)acc & 7)) return MSGS_ERR_INVALID_ARG;
    if (acc_bytes < msgs_contrib_scratch_bytes(P)) return MSGS_ERR_CAPACITY;
    HIP_TRY(launch_contrib_finish(P, acc, weight_sum, weight_max, pixel_count, (hipStream_t)stream));
    return MSGS_OK;
}

size_t msgs_features_scratch_bytes(int32_t P, int32_t C) { (void)C; return features_scratch_bytes(P); }

int msgs_features_forward(const msgs_view_t* view, int32_t P, const void* geom_v, size_t geom_bytes, int64_t D,
                          const void* binning_v, size_t binning_bytes, const void* image_v, size_t image_bytes,
                          const float* features, int32_t C, float* out, void* stream) {
    if (!view || P < 0 || D < 0 || C < 1 || view->image_width < 1 || view->image_height < 1 || !out) return MSGS_ERR_INVALID_ARG;
    if (g_deterministic.load() != 0) return MSGS_ERR_INVALID_ARG;            // not offered in the verification mode
    const int W = view->image_width, H = view->image_height;
    hipStream_t s = (hipStream_t)stream;
    if (P == 0 || D == 0) {                                                  // no instance: no pair, every pixel is 0
        HIP_TRY(launch_zero(out, sizeof(float) * (size_t)C * W * H, s));
        return debug_sync(view, s);
    }
    if (!features || ((uintptr_t)features & 3)) return MSGS_ERR_INVALID_ARG;
    ReplayInputs in;
    const int st = replay_inputs(view, P, geom_v, geom_bytes, D, binning_v, binning_bytes, image_v, image_bytes, &in);
    if (st != MSGS_OK) return st;
    HIP_TRY(launch_blend_features_forward(in, features, C, out, s));
    return debug_sync(view, s);
}

int msgs_features_backward(const msgs_view_t* view, int32_t P, const void* geom_v, size_t geom_bytes, int64_t D,
                           const void* binning_v, size_t binning_bytes, const void* image_v, size_t image_bytes,
                           const float* features, int32_t C, const float* dL_dfeature_map, void* grad_records,
                           size_t grad_records_bytes, void* scratch, size_t scratch_bytes, float* dL_dfeatures, void* stream) {
    if (!view || P < 0 || D < 0 || C < 1 || view->image_width < 1 || view->image_height < 1) return MSGS_ERR_INVALID_ARG;
    if (g_deterministic.load() != 0) return MSGS_ERR_INVALID_ARG;            // its scratch holds another layout
    if (P == 0) return MSGS_OK;                                              // dL_dfeatures is [0, C]
    if (!dL_dfeatures) return MSGS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (D == 0) {                                                            // no pair: zero gradients, nothing for the records
        HIP_TRY(launch_zero(dL_dfeatures, sizeof(float) * (size_t)P * C, s));
        return debug_sync(view, s);
    }
    if (!features || !dL_dfeature_map || !scratch) return MSGS_ERR_INVALID_ARG;
    if (((uintptr_t)features & 3) || ((uintptr_t)scratch & 7) || ((uintptr_t)grad_records & 7)) return MSGS_ERR_INVALID_ARG;
    ReplayInputs in;
    const int st = replay_inputs(view, P, geom_v, geom_bytes, D, binning_v, binning_bytes, image_v, image_bytes, &in);
    if (st != MSGS_OK) return st;
    if (scratch_bytes < features_scratch_bytes(P) || (grad_records && grad_records_bytes < msgs_backward_scratch_bytes(P)))
        return MSGS_ERR_CAPACITY;
    HIP_TRY(launch_blend_features_backward(in, P, features, C, dL_dfeature_map, (grad_acc_t*)grad_records, (double*)scratch,
                                           dL_dfeatures, s));
    return debug_sync(view, s);
}

int msgs_distortion_forward(const msgs_view_t* view, int32_t P, const void* geom_v, size_t geom_bytes, int64_t D,
                            const void* binning_v, size_t binning_bytes, const void* image_v, size_t image_bytes,
                            float* out_distortion, float* out_moment, void* stream) {
    if (!view || P < 0 || D < 0 || view->image_width < 1 || view->image_height < 1 || !out_distortion || !out_moment)
        return MSGS_ERR_INVALID_ARG;
    if (g_deterministic.load() != 0) return MSGS_ERR_INVALID_ARG;            // not offered in the verification mode
    const int W = view->image_width, H = view->image_height;
    hipStream_t s = (hipStream_t)stream;
    if (P == 0 || D == 0) {                                                  // no instance: no pair, every pixel is 0
        HIP_TRY(launch_zero(out_distortion, sizeof(float) * (size_t)W * H, s));
        HIP_TRY(launch_zero(out_moment, sizeof(float) * (size_t)W * H, s));
        return debug_sync(view, s);
    }
    ReplayInputs in;
    const int st = replay_inputs(view, P, geom_v, geom_bytes, D, binning_v, binning_bytes, image_v, image_bytes, &in);
    if (st != MSGS_OK) return st;
    HIP_TRY(launch_blend_distortion_forward(in, out_distortion, out_moment, s));
    return debug_sync(view, s);
}

int msgs_distortion_backward(const msgs_view_t* view, int32_t P, const void* geom_v, size_t geom_bytes, int64_t D,
                             const void* binning_v, size_t binning_bytes, const void* image_v, size_t image_bytes,
                             const float* moment, const float* dL_ddistortion, void* grad_records, size_t grad_records_bytes,
                             void* stream) {
    if (!view || P < 0 || D < 0 || view->image_width < 1 || view->image_height < 1) return MSGS_ERR_INVALID_ARG;
    if (g_deterministic.load() != 0) return MSGS_ERR_INVALID_ARG;            // its scratch holds another layout
    if (P == 0 || D == 0) return MSGS_OK;                                    // no pair: nothing for the records
    if (!moment || !dL_ddistortion || !grad_records || ((uintptr_t)grad_records & 7)) return MSGS_ERR_INVALID_ARG;
    ReplayInputs in;
    const int st = replay_inputs(view, P, geom_v, geom_bytes, D, binning_v, binning_bytes, image_v, image_bytes, &in);
    if (st != MSGS_OK) return st;
    if (grad_records_bytes < msgs_backward_scratch_bytes(P)) return MSGS_ERR_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_blend_distortion_backward(in, moment, dL_ddistortion, (grad_acc_t*)grad_records, s));
    return debug_sync(view, s);
}

int msgs_median_depth_forward(const msgs_view_t* view, int32_t P, const void* geom_v, size_t geom_bytes, int64_t D,
                              const void* binning_v, size_t binning_bytes, const void* image_v, size_t image_bytes,
                              float* out_median_depth, int32_t* out_median_id, void* stream) {
    if (!view || P < 0 || D < 0 || view->image_width < 1 || view->image_height < 1 || !out_median_depth || !out_median_id)
        return MSGS_ERR_INVALID_ARG;
    if (g_deterministic.load() != 0) return MSGS_ERR_INVALID_ARG;            // not offered in the verification mode
    const int W = view->image_width, H = view->image_height;
    hipStream_t s = (hipStream_t)stream;
    if (P == 0 || D == 0) {                                                  // no instance: nothing blended anywhere
        HIP_TRY(launch_zero(out_median_depth, sizeof(float) * (size_t)W * H, s));
        HIP_TRY(hipMemsetAsync(out_median_id, 0xFF, sizeof(int32_t) * (size_t)W * H, s));      // every id -1
        return debug_sync(view, s);
    }
    ReplayInputs in;
    const int st = replay_inputs(view, P, geom_v, geom_bytes, D, binning_v, binning_bytes, image_v, image_bytes, &in);
    if (st != MSGS_OK) return st;
    HIP_TRY(launch_blend_median_depth_forward(in, out_median_depth, out_median_id, s));
    return debug_sync(view, s);
}

int msgs_median_depth_backward(const msgs_view_t* view, int32_t P, const int32_t* median_id, const float* dL_dmedian_depth,
                               void* grad_records, size_t grad_records_bytes, void* stream) {
    if (!view || P < 0 || view->image_width < 1 || view->image_height < 1) return MSGS_ERR_INVALID_ARG;
    if (g_deterministic.load() != 0) return MSGS_ERR_INVALID_ARG;            // its scratch holds another layout
    if (P == 0) return MSGS_OK;                                              // every id is -1: nothing for the records
    if (!median_id || !dL_dmedian_depth || !grad_records || ((uintptr_t)grad_records & 7)) return MSGS_ERR_INVALID_ARG;
    if (grad_records_bytes < msgs_backward_scratch_bytes(P)) return MSGS_ERR_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    const ViewParams vp = make_view_params(view);
    HIP_TRY(launch_median_depth_backward(vp, P, median_id, dL_dmedian_depth, (grad_acc_t*)grad_records, s));
    return debug_sync(view, s);
}

// ---- antialiasing: the opacity compensation of the 2-D screen filter, in front of K1 (SPEC M14) ----
}  // extern "C"
namespace {
// the view's geometry and the activated inputs of the reference API: nothing else enters rho
inline int check_compensation_inputs(const msgs_view_t* v, const msgs_gaussians_t* g) {
    if (!v || !g || g->P < 0 || v->image_width <= 0 || v->image_height <= 0 || !v->viewmatrix) return MSGS_ERR_INVALID_ARG;
    if (g->raw_params != 0) return MSGS_ERR_INVALID_ARG;
    if (g->P == 0) return MSGS_OK;
    if (!g->means3D || !g->opacities) return MSGS_ERR_INVALID_ARG;
    const bool sr = g->scales != nullptr && g->rotations != nullptr;
    if ((g->scales != nullptr) != (g->rotations != nullptr) || sr == (g->cov3D_precomp != nullptr)) return MSGS_ERR_INVALID_ARG;
    return MSGS_OK;
}
}  // namespace
extern "C" {

size_t msgs_screen_compensation_scratch_bytes(int32_t P) { return screen_compensation_rows_bytes(P); }

int msgs_screen_compensation_forward(const msgs_view_t* view, const msgs_gaussians_t* g, float* o_eff, void* stream) {
    const int rc = check_compensation_inputs(view, g);
    if (rc != MSGS_OK) return rc;
    if (g->P == 0) return MSGS_OK;
    if (!o_eff) return MSGS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_screen_compensation_forward(make_view_params(view), *g, o_eff, s));
    return debug_sync(view, s);
}

int msgs_screen_compensation_backward(const msgs_view_t* view, const msgs_gaussians_t* g, const float* dL_do_eff,
                                      float* dL_dopacity, float* dL_dmeans3D, float* dL_dscales, float* dL_drotations,
                                      float* dL_dcov3D, float* dL_dV, void* scratch, size_t scratch_bytes, void* stream) {
    const int rc = check_compensation_inputs(view, g);
    if (rc != MSGS_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (g->P == 0) {                                                         // no Gaussian: the camera sums are zero
        if (dL_dV) HIP_TRY(launch_zero(dL_dV, sizeof(float) * 16, s));
        return debug_sync(view, s);
    }
    if (!dL_do_eff) return MSGS_ERR_INVALID_ARG;
    // a gradient the inputs have no tensor for would be written from zeros: refuse the pointer instead
    if ((g->cov3D_precomp && (dL_dscales || dL_drotations)) || (!g->cov3D_precomp && dL_dcov3D)) return MSGS_ERR_INVALID_ARG;
    if (dL_dV) {
        if (!scratch || ((uintptr_t)scratch & 7)) return MSGS_ERR_INVALID_ARG;
        if (scratch_bytes < msgs_screen_compensation_scratch_bytes(g->P)) return MSGS_ERR_CAPACITY;
    }
    HIP_TRY(launch_screen_compensation_backward(make_view_params(view), *g, dL_do_eff, dL_dopacity, dL_dmeans3D, dL_dscales,
                                                dL_drotations, dL_dcov3D, dL_dV, (double*)scratch, s));
    return debug_sync(view, s);
}
}  // extern "C"

// ---- 3-D smoothing filter: the camera sweep and the filtered getters (SPEC M16) ----
extern "C" {
size_t msgs_filter3d_scratch_bytes(int32_t P, int32_t n_cameras) { (void)P; (void)n_cameras; return 256; }

int msgs_filter3d_sweep(int32_t P, const float* means3D, int32_t n_cameras, const float* cameras, int32_t rule, float variance,
                        float* filter_3D, uint8_t* valid, void* scratch, size_t scratch_bytes, void* stream) {
    if (P < 0 || n_cameras < 1 || !(variance > 0.0f)) return MSGS_ERR_INVALID_ARG;
    if (rule != MSGS_FILTER3D_RULE_PER_CAMERA && rule != MSGS_FILTER3D_RULE_MIP_SPLATTING) return MSGS_ERR_INVALID_ARG;
    if (P == 0) return MSGS_OK;
    if (!means3D || !cameras || !filter_3D || !valid || !scratch || ((uintptr_t)scratch & 3)) return MSGS_ERR_INVALID_ARG;
    if (scratch_bytes < msgs_filter3d_scratch_bytes(P, n_cameras)) return MSGS_ERR_CAPACITY;
    HIP_TRY(launch_filter3d_sweep(P, means3D, n_cameras, cameras, rule, variance, filter_3D, valid, (uint32_t*)scratch,
                                  (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_smoothing_filter_forward(int32_t P, int32_t raw, const float* scales, const float* opacities, const float* filter_3D,
                                  float* scales_eff, float* opacities_eff, void* stream) {
    if (P < 0) return MSGS_ERR_INVALID_ARG;
    if (P == 0) return MSGS_OK;
    if (!scales || !opacities || !filter_3D || !scales_eff || !opacities_eff) return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_smoothing_filter_forward(P, raw != 0, scales, opacities, filter_3D, scales_eff, opacities_eff,
                                            (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_smoothing_filter_backward(int32_t P, int32_t raw, const float* scales, const float* opacities, const float* filter_3D,
                                   const float* dL_dscales_eff, const float* dL_dopacities_eff, float* dL_dscales,
                                   float* dL_dopacities, void* stream) {
    if (P < 0) return MSGS_ERR_INVALID_ARG;
    if (P == 0) return MSGS_OK;
    if (!scales || !opacities || !filter_3D || !dL_dscales || !dL_dopacities) return MSGS_ERR_INVALID_ARG;
    if (!dL_dscales_eff && !dL_dopacities_eff) return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_smoothing_filter_backward(P, raw != 0, scales, opacities, filter_3D, dL_dscales_eff, dL_dopacities_eff,
                                             dL_dscales, dL_dopacities, (hipStream_t)stream));
    return MSGS_OK;
}
}  // extern "C"

// ---- normal maps: Gaussian normals and depth-to-normal (SPEC M17) ----
namespace {
// the kernels index pixels in int and tile the image with a 2-D grid
bool depth_normal_shape_ok(int32_t W, int32_t H) {
    if (W < 0 || H < 0) return false;
    if (W == 0 || H == 0) return true;
    return (int64_t)W * H <= INT32_MAX / 4 && (H + MSGS_DEPTH_NORMAL_TILE_H - 1) / MSGS_DEPTH_NORMAL_TILE_H <= 65535;
}
}  // namespace

extern "C" {
int msgs_gaussian_normals_forward(int32_t P, const float* means3D, const float* scales, const float* rotations,
                                  const float* viewmatrix, const float* campos, int32_t world, float* normals, uint8_t* flags,
                                  void* stream) {
    if (P < 0) return MSGS_ERR_INVALID_ARG;
    if (P == 0) return MSGS_OK;
    if (!means3D || !scales || !rotations || !viewmatrix || !campos || !normals || !flags) return MSGS_ERR_INVALID_ARG;
    if ((uintptr_t)rotations & 15) return MSGS_ERR_INVALID_ARG;          // read as float4 rows
    HIP_TRY(launch_gaussian_normals_forward(P, means3D, scales, rotations, viewmatrix, campos, world != 0, normals, flags,
                                            (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_gaussian_normals_backward(int32_t P, const float* rotations, const uint8_t* flags, const float* viewmatrix,
                                   int32_t world, const float* dL_dnormals, float* dL_drotations, void* stream) {
    if (P < 0) return MSGS_ERR_INVALID_ARG;
    if (P == 0) return MSGS_OK;
    if (!rotations || !flags || !dL_dnormals || !dL_drotations || (!world && !viewmatrix)) return MSGS_ERR_INVALID_ARG;
    if (((uintptr_t)rotations | (uintptr_t)dL_drotations) & 15) return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_gaussian_normals_backward(P, rotations, flags, viewmatrix, world != 0, dL_dnormals, dL_drotations,
                                             (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_depth_normal_forward(int32_t W, int32_t H, float tanfovx, float tanfovy, const float* depth, const float* viewmatrix,
                              int32_t world, float* normal, void* stream) {
    if (!depth_normal_shape_ok(W, H)) return MSGS_ERR_INVALID_ARG;
    if (W == 0 || H == 0) return MSGS_OK;
    if (!depth || !normal || (world && !viewmatrix)) return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_depth_normal_forward(W, H, tanfovx, tanfovy, depth, viewmatrix, world != 0, normal, (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_depth_normal_backward(int32_t W, int32_t H, float tanfovx, float tanfovy, const float* depth, const float* viewmatrix,
                               int32_t world, const float* dL_dnormal, float* dL_ddepth, void* stream) {
    if (!depth_normal_shape_ok(W, H)) return MSGS_ERR_INVALID_ARG;
    if (W == 0 || H == 0) return MSGS_OK;
    if (!depth || !dL_dnormal || !dL_ddepth || (world && !viewmatrix)) return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_depth_normal_backward(W, H, tanfovx, tanfovy, depth, viewmatrix, world != 0, dL_dnormal, dL_ddepth,
                                         (hipStream_t)stream));
    return MSGS_OK;
}
}  // extern "C"

namespace {
int backward_impl(const msgs_view_t* view, const msgs_gaussians_t* g, const int32_t* radii, const void* geom_v,
                  size_t geom_bytes, int64_t D, const void* binning_v, size_t binning_bytes, const void* image_v,
                  size_t image_bytes, const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha, void* scratch_v,
                  size_t scratch_bytes, const msgs_grads_t* grads, const CameraGrads* cam, const msgs_timing_t* timing,
                  void* stream) {
    int rc = check_inputs(view, g);
    if (rc) return rc;
    if (!grads || !dL_dcolor) return MSGS_ERR_INVALID_ARG;
    const int P = g->P, W = view->image_width, H = view->image_height;
    if (P == 0) {
        if (cam) {                      // no Gaussian: zero camera gradients (always overwritten)
            hipStream_t s0 = (hipStream_t)stream;
            if (cam->dL_dviewmatrix) HIP_TRY(hipMemsetAsync(cam->dL_dviewmatrix, 0, 16 * sizeof(float), s0));
            if (cam->dL_dprojmatrix) HIP_TRY(hipMemsetAsync(cam->dL_dprojmatrix, 0, 16 * sizeof(float), s0));
            if (cam->dL_dcampos) HIP_TRY(hipMemsetAsync(cam->dL_dcampos, 0, 3 * sizeof(float), s0));
        }
        return MSGS_OK;
    }
    if (!radii || !geom_v || !binning_v || !image_v || !scratch_v) return MSGS_ERR_INVALID_ARG;
    const bool det = g_deterministic.load() != 0;
    if (geom_bytes < msgs_geom_bytes(P) || binning_bytes < msgs_binning_bytes(D, W, H) ||
        image_bytes < msgs_image_bytes(W, H) ||
        scratch_bytes < (det ? (dL_ddepth ? msgs_backward_scratch_bytes_deterministic_depth(P, D)
                                          : msgs_backward_scratch_bytes_deterministic(P, D))
                             : msgs_backward_scratch_bytes(P)))
        return MSGS_ERR_CAPACITY;
    if (g->shs && !g->raw_params && !grads->dL_dshs) return MSGS_ERR_INVALID_ARG;
    // raw modes: either both SH gradient tensors, or neither plus dL_dcolors (factored SH gradient, msgs.h)
    if (g->raw_params && (!grads->dL_dfeatures_dc != !grads->dL_dfeatures_rest)) return MSGS_ERR_INVALID_ARG;
    if (g->raw_params && !grads->dL_dfeatures_dc && !grads->dL_dcolors && !grads->adam_in_backward) return MSGS_ERR_INVALID_ARG;
    if (const msgs_adam_in_backward_t* ad = grads->adam_in_backward) {
        // the optimizer step inside the per-Gaussian kernel (msgs.h): gradients of the LEAVES, on the staged SH rows, one view
        if (g->raw_params != 1 || !g->features_dc || !g->features_rest || g->shs || g->colors_precomp || g->cov3D_precomp ||
            !g->scales || !g->rotations || view->sh_coeffs != 16 || grads->accumulate || grads->wait_before_accumulate ||
            ad->step < 1)
            return MSGS_ERR_INVALID_ARG;
        uintptr_t bits = (uintptr_t)g->means3D | (uintptr_t)g->features_dc | (uintptr_t)g->features_rest |
                         (uintptr_t)g->opacities | (uintptr_t)g->scales | (uintptr_t)g->rotations;
        for (int t = 0; t < 6; ++t) {
            if (!ad->t[t].exp_avg || !ad->t[t].exp_avg_sq) return MSGS_ERR_INVALID_ARG;
            bits |= (uintptr_t)ad->t[t].exp_avg | (uintptr_t)ad->t[t].exp_avg_sq;
        }
        if (bits & 15) return MSGS_ERR_INVALID_ARG;
    }
    // accumulate mode is implemented on the staged SH rows (K = 16) and not for the factored SH gradient
    if (grads->accumulate && ((g->shs && !g->raw_params && view->sh_coeffs != 16) ||
                              (g->raw_params && !grads->dL_dfeatures_dc)))
        return MSGS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    const char* geom = (const char*)geom_v;
    const char* binning = (const char*)binning_v;
    const char* image = (const char*)image_v;
    const ViewParams vp = make_view_params(view);
    const BinningLayout BL(D, vp.gx * vp.gy);
    const ImageLayout IL(W, H);
    const Timer tm{timing, s};
    grad_acc_t* grad_rec = (grad_acc_t*)scratch_v;

    // deterministic mode writes its own scratch layout from scratch: a "cleared by the forward" claim cannot hold there
    if (det && grads->scratch_is_clear) return MSGS_ERR_INVALID_ARG;
    if (!grads->scratch_is_clear)           // (else: cleared by the blend kernel of this view's forward, msgs.h)
        HIP_TRY(launch_zero(grad_rec, GRAD_REC_BYTES * (size_t)P, s));
    tm.begin(MSGS_K_BLEND_BWD);
    if (det)      // grad_rec is the first region of the deterministic scratch layout
        HIP_TRY(launch_blend_backward_det(vp, P, geom, (const uint32_t*)(binning + BL.ids), D,
                                          (const uint2*)(binning + BL.ranges), (const float*)(image + IL.final_T),
                                          (const uint32_t*)(image + IL.n_contrib), dL_dcolor, (char*)scratch_v, s, dL_ddepth,
                                          dL_dalpha));
    else
        HIP_TRY(launch_blend_backward(vp, geom, (const uint32_t*)(binning + BL.ids), (const uint2*)(binning + BL.ranges),
                                      (const float*)(image + IL.final_T), (const uint32_t*)(image + IL.n_contrib),
                                      dL_dcolor, grad_rec, s, (const uint32_t*)(image + IL.tile_order), dL_ddepth,
                                      dL_dalpha));
    tm.end(MSGS_K_BLEND_BWD);
    if ((rc = debug_sync(view, s))) return rc;

    tm.begin(MSGS_K_PREPROCESS_BWD);
    // det: the nine TEXTBOOK sums per Gaussian ([P, 9] doubles; [P, 10] with depth) as they are
    HIP_TRY(launch_preprocess_backward(vp, *g, radii, geom, grad_rec, *grads, s, det, dL_ddepth != nullptr, cam));
    tm.end(MSGS_K_PREPROCESS_BWD);
    return debug_sync(view, s);
}
}  // namespace

extern "C" {

int msgs_backward_per_gaussian(const msgs_view_t* view, const msgs_gaussians_t* g, const int32_t* radii,
                               const void* geom_v, size_t geom_bytes, const double* sums2d, const msgs_grads_t* grads,
                               void* stream) {
    int rc = check_inputs(view, g);
    if (rc) return rc;
    if (!grads || g->raw_params || grads->adam_in_backward) return MSGS_ERR_INVALID_ARG;
    // the textbook branch of the per-Gaussian kernel neither waits for `wait_before_accumulate` nor records `accumulated`:
    // accumulation across views is msgs_backward's contract only
    if (grads->accumulate || grads->wait_before_accumulate || grads->accumulated) return MSGS_ERR_INVALID_ARG;
    const int P = g->P;
    if (P == 0) return MSGS_OK;
    if (!radii || !geom_v || !sums2d) return MSGS_ERR_INVALID_ARG;
    if (geom_bytes < msgs_geom_bytes(P)) return MSGS_ERR_CAPACITY;
    if (g->shs && !grads->dL_dshs) return MSGS_ERR_INVALID_ARG;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_preprocess_backward(make_view_params(view), *g, radii, (const char*)geom_v,
                                       reinterpret_cast<const grad_acc_t*>(sums2d), *grads, s, true));
    return debug_sync(view, s);
}

int msgs_sh_grad_from_views(int32_t P, int32_t n_views, int32_t sh_degree, const float* means3D, const float* campos,
                            int64_t campos_stride, const float* drgb, int64_t drgb_stride, float scale,
                            float* dL_dfeatures_dc, float* dL_dfeatures_rest, void* stream) {
    if (P < 0 || n_views < 1 || sh_degree < 0 || sh_degree > 3 || campos_stride < 0 || drgb_stride < 0)
        return MSGS_ERR_INVALID_ARG;
    if (P > 0 && (!means3D || !campos || !drgb || !dL_dfeatures_dc || !dL_dfeatures_rest)) return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_sh_grad_from_views(P, n_views, sh_degree, means3D, campos, campos_stride, drgb, drgb_stride, scale,
                                      dL_dfeatures_dc, dL_dfeatures_rest, (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                      uint8_t* present, void* stream) {
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_mark_visible(P, means3D, viewmatrix, projmatrix, present, (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_binning_stats(const msgs_view_t* view, int32_t P, const int32_t* radii, const void* binning,
                       size_t binning_bytes, const void* image_v, size_t image_bytes, void* scratch,
                       size_t scratch_bytes, int64_t* out_host, void* stream) {
    (void)binning; (void)binning_bytes;
    if (!view || !image_v || !scratch || !out_host || scratch_bytes < 16) return MSGS_ERR_INVALID_ARG;
    const int W = view->image_width, H = view->image_height;
    if (image_bytes < msgs_image_bytes(W, H)) return MSGS_ERR_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    const ViewParams vp = make_view_params(view);
    const ImageLayout IL(W, H);
    unsigned long long* dev = (unsigned long long*)scratch;
    HIP_TRY(launch_binning_stats(vp, P, radii, (const uint32_t*)((const char*)image_v + IL.n_contrib), dev, s));
    unsigned long long host[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(host, dev, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out_host[0] = (int64_t)host[0];
    out_host[1] = (int64_t)host[1];
    return MSGS_OK;
}

int msgs_forward_info(int64_t* out_host) {
    if (!out_host) return MSGS_ERR_INVALID_ARG;
    out_host[0] = (int64_t)(t_last_info & 0xFFFFFFFFull);
    out_host[1] = (int64_t)(t_last_info >> 32) != 0 ? 1 : 0;
    // feedback publication (forward_feedback_kernel): {D_trav | overflow << 63, tag | n_open << 32, DA | DB << 32, D | ticket << 40}
    const uint64_t w4 = t_last_feedback[0], w5 = t_last_feedback[1], w6 = t_last_feedback[2], w7 = t_last_feedback[3];
    const uint32_t n_open = (uint32_t)(w5 >> 32);
    out_host[2] = (int64_t)(w5 & 0xFFFFFFFFull);                       // tag (0: nothing published yet)
    out_host[3] = (int64_t)(w7 & 0xFFFFFFFFFFull);                     // D
    out_host[4] = (int64_t)(w4 & ~(1ull << 63));                       // D_trav
    out_host[5] = n_open == 0xFFFFFFFFu ? -1 : (int64_t)n_open;        // tiles left open by slab A (-1: single pass)
    out_host[6] = (int64_t)(w6 & 0xFFFFFFFFull);                       // DA
    out_host[7] = (w4 >> 63) ? -1 : (int64_t)(w6 >> 32);               // DB (-1: slab B outgrew its buffers — never observed)
    return MSGS_OK;
}

int msgs_slab_stats(const void* geom_v, size_t geom_bytes, int32_t P, int64_t* out_host, void* stream) {
    if (!geom_v || !out_host || P <= 0) return MSGS_ERR_INVALID_ARG;
    if (geom_bytes < msgs_geom_bytes(P)) return MSGS_ERR_CAPACITY;
    const GeomLayout GL(P);
    SlabHeader h;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(&h, (const char*)geom_v + GL.slab_hdr, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out_host[0] = h.active;
    out_host[1] = h.rA;
    out_host[2] = h.DA;
    out_host[3] = h.n_open;
    out_host[4] = (int64_t)h.total_b;
    out_host[5] = h.pad0;          // 1: slab B outgrew its buffers (never observed)
    return MSGS_OK;
}

int msgs_depth_sort_stats(const void* geom_v, size_t geom_bytes, int32_t P, int64_t* out_host, void* stream) {
    if (!geom_v || !out_host || P <= 0) return MSGS_ERR_INVALID_ARG;
    if (geom_bytes < msgs_geom_bytes(P)) return MSGS_ERR_CAPACITY;
    static_assert(sizeof(SlabHeader) <= DEPTH_SORT_INFO_OFFSET && DEPTH_SORT_INFO_OFFSET + 8 <= 256, "inside the slab header's slot");
    const GeomLayout GL(P);
    uint32_t info[2], V;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(info, (const char*)geom_v + GL.slab_hdr + DEPTH_SORT_INFO_OFFSET, sizeof(info), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&V, (const char*)geom_v + GL.nvalid, sizeof(V), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out_host[0] = info[0];
    out_host[1] = info[1];
    out_host[2] = V;
    return MSGS_OK;
}

int msgs_occlusion_stats(const void* geom_v, size_t geom_bytes, int32_t P, int64_t* out_host, void* stream) {
    if (!geom_v || !out_host || P <= 0) return MSGS_ERR_INVALID_ARG;
    if (geom_bytes < msgs_geom_bytes(P)) return MSGS_ERR_CAPACITY;
    const GeomLayout GL(P);
    OccHeader h;
    hipStream_t s = (hipStream_t)stream;
    static uint32_t table[OCC_MAX_BLOCKS];               // (diagnostic entry: serialised by the synchronisation below)
    HIP_TRY(hipMemcpyAsync(&h, (const char*)geom_v + GL.occ_hdr, sizeof(h), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 8; ++k) out_host[k] = 0;
    out_host[0] = h.enabled ? (h.watchdog ? 2 : 1) : 0;     // 2: a barrier wait of the pass expired (never observed)
    if (!h.enabled) return MSGS_OK;
    const int n_blocks = (int)(h.nbx * h.nby);
    if (n_blocks < 0 || n_blocks > OCC_MAX_BLOCKS) return MSGS_ERR_INTERNAL;
    if (h.any_closed) {       // (a view in which nothing closed leaves the table unwritten: nobody reads it)
        HIP_TRY(hipMemcpyAsync(table, (const char*)geom_v + GL.occ_cut, 4 * (size_t)n_blocks, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    } else {
        for (int k = 0; k < n_blocks; ++k) table[k] = 0xFFFFu;
    }
    // cut-offs are depth buckets (0xFFFF = open): reported as the depth key at the far end of the bucket
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    int closed = 0;
    for (int k = 0; k < n_blocks; ++k) {
        const uint32_t key = table[k] >= 0xFFFFu ? 0xFFFFFFFFu : (((table[k] + OCC_KEY_BASE + 1u) << OCC_KEY_SHIFT) - 1u);
        closed += key != 0xFFFFFFFFu;
        lo = key < lo ? key : lo;
        hi = key > hi ? key : hi;
    }
    out_host[1] = h.n_heavy;
    out_host[2] = h.n_cand;
    out_host[3] = closed;
    out_host[4] = n_blocks;
    out_host[5] = 1u << h.block_log2;
    out_host[6] = lo;
    out_host[7] = hi;
    return MSGS_OK;
}

int msgs_blend_lane_stats(const msgs_view_t* view, const void* geom, size_t geom_bytes, int32_t P, int64_t D,
                          const void* binning_v, size_t binning_bytes, const void* image_v, size_t image_bytes,
                          void* scratch, size_t scratch_bytes, int64_t* out_host, void* stream) {
    if (!view || !geom || !binning_v || !scratch || !out_host || scratch_bytes < 64 || P < 0) return MSGS_ERR_INVALID_ARG;
    const int W = view->image_width, H = view->image_height;
    if (geom_bytes < msgs_geom_bytes(P) || binning_bytes < msgs_binning_bytes(D, W, H)) return MSGS_ERR_CAPACITY;
    if (image_v && image_bytes < msgs_image_bytes(W, H)) return MSGS_ERR_CAPACITY;
    hipStream_t s = (hipStream_t)stream;
    const ViewParams vp = make_view_params(view);
    const BinningLayout BL(D, vp.gx * vp.gy);
    const ImageLayout IL(W, H);
    const char* binning = (const char*)binning_v;
    unsigned long long* dev = (unsigned long long*)scratch;
    HIP_TRY(launch_blend_lane_stats(vp, (const char*)geom, (const uint32_t*)(binning + BL.ids),
                                    (const uint2*)(binning + BL.ranges), dev, s));
    if (image_v)
        HIP_TRY(launch_blend_backward_lane_stats(vp, (const char*)geom, (const uint32_t*)(binning + BL.ids),
                                                 (const uint2*)(binning + BL.ranges),
                                                 (const float*)((const char*)image_v + IL.final_T),
                                                 (const uint32_t*)((const char*)image_v + IL.n_contrib), dev + 4, s));
    unsigned long long host[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(host, dev, 64, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 3; ++k) out_host[k] = (int64_t)host[k];
    for (int k = 0; k < 4; ++k) out_host[3 + k] = image_v ? (int64_t)host[4 + k] : -1;
    return MSGS_OK;
}

int msgs_adam_step(const msgs_adam_tensor_t* tensors, int32_t n_tensors, int64_t step, double beta1, double beta2,
                   double eps, void* stream) {
    if (n_tensors < 0 || n_tensors > MSGS_ADAM_MAX_TENSORS || step < 1 || (n_tensors && !tensors))
        return MSGS_ERR_INVALID_ARG;
    for (int k = 0; k < n_tensors; ++k) {
        const msgs_adam_tensor_t& t = tensors[k];
        if (t.n < 0 || (t.n > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq))) return MSGS_ERR_INVALID_ARG;
        if (t.n > (int64_t)1 << 40) return MSGS_ERR_TOO_MANY;
    }
    HIP_TRY(launch_adam(tensors, n_tensors, step, beta1, beta2, eps, (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_densify_stats(const msgs_densify_stats_t* d, void* stream) {
    if (!d || d->P < 0 || d->reso_lvls < 1 || d->reso_lvl < 0 || d->reso_lvl >= d->reso_lvls) return MSGS_ERR_INVALID_ARG;
    if (d->P == 0 || d->flags == 0) return MSGS_OK;
    if (!d->radii) return MSGS_ERR_INVALID_ARG;
    if ((d->flags & MSGS_STATS_BASE_MASK) && !d->base_mask) return MSGS_ERR_INVALID_ARG;
    if ((d->flags & MSGS_STATS_PIXEL_SIZES) &&
        (!d->pixel_sizes || !d->target_reso_lvl || !d->max_pixel_sizes || !d->min_pixel_sizes)) return MSGS_ERR_INVALID_ARG;
    if ((d->flags & MSGS_STATS_DENSIFY) && (!d->means2D_grad || !d->xyz_gradient_accum || !d->denom || !d->max_radii2D))
        return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_densify_stats(*d, (hipStream_t)stream));
    return MSGS_OK;
}

size_t msgs_densify_scratch_bytes(int64_t P, int64_t n_append) {
    return densify_scratch_bytes(P > 0 ? P : 0, n_append > 0 ? n_append : 0);
}

int msgs_densify_select(const msgs_densify_select_t* sel, void* scratch, size_t scratch_bytes, int64_t* counts_host,
                        void* stream) {
    if (!sel || !counts_host || !scratch) return MSGS_ERR_INVALID_ARG;
    if (int rc = densify_check_select(*sel)) return rc;
    if (scratch_bytes < densify_scratch_bytes(sel->P, sel->n_append)) return MSGS_ERR_CAPACITY;
    return densify_select(*sel, (char*)scratch, counts_host, (hipStream_t)stream);
}

int msgs_densify_apply(const msgs_densify_apply_t* apply, const void* scratch, size_t scratch_bytes, void* stream) {
    if (!apply || !scratch) return MSGS_ERR_INVALID_ARG;
    if (int rc = densify_check_apply(*apply)) return rc;
    if (scratch_bytes < densify_scratch_bytes(apply->P, apply->n_append)) return MSGS_ERR_CAPACITY;
    return densify_apply(*apply, (const char*)scratch, (hipStream_t)stream);
}

// ---- MCMC densification: sampling, relocation, position noise (SPEC M18) ----
size_t msgs_mcmc_scratch_bytes(int64_t P) { return mcmc_scratch_bytes(P > 0 ? P : 0); }

static int mcmc_rows_ok(int64_t P, const float* opacity, const void* scratch, size_t scratch_bytes) {
    if (P < 0 || !scratch || (P > 0 && !opacity)) return MSGS_ERR_INVALID_ARG;
    if (P >= ((int64_t)1 << 31)) return MSGS_ERR_TOO_MANY;
    if (scratch_bytes < mcmc_scratch_bytes(P)) return MSGS_ERR_CAPACITY;
    return MSGS_OK;
}

int msgs_mcmc_prepare(int64_t P, const float* opacity, const uint8_t* dead, void* scratch, size_t scratch_bytes,
                      int64_t* counts_host, void* stream) {
    if (!counts_host) return MSGS_ERR_INVALID_ARG;
    if (int rc = mcmc_rows_ok(P, opacity, scratch, scratch_bytes)) return rc;
    counts_host[0] = counts_host[1] = counts_host[2] = counts_host[3] = 0;
    if (P == 0) return MSGS_OK;
    return mcmc_prepare(P, opacity, dead, (char*)scratch, counts_host, (hipStream_t)stream);
}

int msgs_mcmc_sample(int64_t P, const float* opacity, const uint8_t* dead, int64_t n, const double* u, int32_t* source,
                     int32_t* count, void* scratch, size_t scratch_bytes, void* stream) {
    if (n < 0 || (n > 0 && (!u || !source || !count))) return MSGS_ERR_INVALID_ARG;
    if (int rc = mcmc_rows_ok(P, opacity, scratch, scratch_bytes)) return rc;
    if (n == 0) return MSGS_OK;
    if (P == 0) return MSGS_ERR_NO_WEIGHT;
    if (n >= ((int64_t)1 << 31)) return MSGS_ERR_TOO_MANY;
    return mcmc_sample(P, opacity, dead, n, u, source, count, (char*)scratch, (hipStream_t)stream);
}

int msgs_mcmc_relocate(const msgs_mcmc_relocate_t* r, void* scratch, size_t scratch_bytes, void* stream) {
    if (!r || !scratch) return MSGS_ERR_INVALID_ARG;
    if (int rc = mcmc_check_relocate(*r)) return rc;
    if (scratch_bytes < mcmc_scratch_bytes(r->P)) return MSGS_ERR_CAPACITY;
    if (r->P == 0 || r->n == 0) return MSGS_OK;
    return mcmc_relocate(*r, (char*)scratch, (hipStream_t)stream);
}

int msgs_mcmc_noise(int64_t P, float* xyz, const float* scaling, const float* rotation, const float* opacity,
                    const float* draws, float gain, void* stream) {
    if (P < 0 || (P > 0 && (!xyz || !scaling || !rotation || !opacity || !draws))) return MSGS_ERR_INVALID_ARG;
    if (P >= ((int64_t)1 << 31)) return MSGS_ERR_TOO_MANY;
    HIP_TRY(launch_mcmc_noise(P, xyz, scaling, rotation, opacity, draws, gain, (hipStream_t)stream));
    return MSGS_OK;
}

// ---- bilateral-grid colour correction (SPEC M19) ----
static int bilagrid_shape_ok(int32_t W, int32_t H, int32_t GX, int32_t GY, int32_t GL) {
    if (GX < 1 || GY < 1 || GL < 1 || GX > MSGS_BILAGRID_MAX_XY || GY > MSGS_BILAGRID_MAX_XY || GL > MSGS_BILAGRID_MAX_L) return 0;
    if (W < 1 || H < 1 || (int64_t)W * H >= ((int64_t)1 << 29)) return 0;
    return (H + MSGS_BILAGRID_TILE_H - 1) / MSGS_BILAGRID_TILE_H <= 65535;
}

static int64_t bilagrid_bank_elements(int64_t N, int32_t GX, int32_t GY, int32_t GL) {
    if (N < 0 || GX < 1 || GY < 1 || GL < 1 || GX > MSGS_BILAGRID_MAX_XY || GY > MSGS_BILAGRID_MAX_XY || GL > MSGS_BILAGRID_MAX_L)
        return -1;
    const int64_t per = (int64_t)12 * GL * GY * GX;
    if (N > (((int64_t)1 << 38) / per)) return -1;          // the backward's launch: one thread per element
    return N * per;
}

size_t msgs_bilagrid_scratch_bytes(int32_t W, int32_t H, int32_t GX, int32_t GY, int32_t GL) {
    return bilagrid_shape_ok(W, H, GX, GY, GL) ? bilagrid_scratch_bytes(W, H, GX, GY, GL) : 0;
}

int msgs_bilagrid_slice_forward(int32_t W, int32_t H, int32_t GX, int32_t GY, int32_t GL, const float* image,
                                const float* grid, float* out, void* stream) {
    if (!bilagrid_shape_ok(W, H, GX, GY, GL) || !image || !grid || !out) return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_bilagrid_slice_forward(W, H, GX, GY, GL, image, grid, out, (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_bilagrid_slice_backward(int32_t W, int32_t H, int32_t GX, int32_t GY, int32_t GL, const float* image,
                                 const float* grid, const float* dL_dout, int32_t want, float* dL_dimage, float* dL_dgrid,
                                 void* scratch, size_t scratch_bytes, void* stream) {
    if (!bilagrid_shape_ok(W, H, GX, GY, GL) || !image || !grid || !dL_dout) return MSGS_ERR_INVALID_ARG;
    if (want & ~(MSGS_BILAGRID_GRAD_IMAGE | MSGS_BILAGRID_GRAD_GRID)) return MSGS_ERR_INVALID_ARG;
    const bool wi = want & MSGS_BILAGRID_GRAD_IMAGE, wg = want & MSGS_BILAGRID_GRAD_GRID;
    if ((wi && !dL_dimage) || (wg && (!dL_dgrid || !scratch || ((uintptr_t)scratch & 15)))) return MSGS_ERR_INVALID_ARG;
    if (wg && scratch_bytes < bilagrid_scratch_bytes(W, H, GX, GY, GL)) return MSGS_ERR_CAPACITY;
    if (!wi && !wg) return MSGS_OK;
    HIP_TRY(launch_bilagrid_slice_backward(W, H, GX, GY, GL, image, grid, dL_dout, wi ? dL_dimage : nullptr,
                                           wg ? dL_dgrid : nullptr, (char*)scratch, (hipStream_t)stream));
    return MSGS_OK;
}

size_t msgs_bilagrid_tv_scratch_bytes(int64_t n_elements) { return bilagrid_tv_scratch_bytes(n_elements < 0 ? 0 : n_elements); }

int msgs_bilagrid_tv_forward(int64_t N, int32_t GX, int32_t GY, int32_t GL, const float* grids, float* tv, void* scratch,
                             size_t scratch_bytes, void* stream) {
    const int64_t n = bilagrid_bank_elements(N, GX, GY, GL);
    if (n < 0 || !tv || !scratch || ((uintptr_t)scratch & 7) || (n > 0 && !grids)) return MSGS_ERR_INVALID_ARG;
    if (scratch_bytes < bilagrid_tv_scratch_bytes(n)) return MSGS_ERR_CAPACITY;
    HIP_TRY(launch_bilagrid_tv_forward(N, GX, GY, GL, grids, tv, (char*)scratch, (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_bilagrid_tv_backward(int64_t N, int32_t GX, int32_t GY, int32_t GL, const float* grids, const float* upstream,
                              float* dL_dgrids, void* stream) {
    const int64_t n = bilagrid_bank_elements(N, GX, GY, GL);
    if (n < 0 || (n > 0 && (!grids || !dL_dgrids))) return MSGS_ERR_INVALID_ARG;
    if (n == 0) return MSGS_OK;
    HIP_TRY(launch_bilagrid_tv_backward(N, GX, GY, GL, grids, upstream, dL_dgrids, (hipStream_t)stream));
    return MSGS_OK;
}

// ---- TSDF fusion and mesh extraction (SPEC M20) ----
static int tsdf_geometry_ok(const msgs_tsdf_volume_t* v) {
    if (!v || !(v->voxel_size > 0.f) || !(v->voxel_size < INFINITY)) return 0;
    for (int a = 0; a < 3; ++a)
        if (v->nb[a] < 1 || v->nb[a] > MSGS_TSDF_MAX_BLOCKS_PER_AXIS || !(fabsf(v->origin[a]) < INFINITY)) return 0;
    return 1;
}

static int tsdf_pool_ok(const msgs_tsdf_volume_t* v) {
    if (!tsdf_geometry_ok(v) || v->n_slots < 0 || v->n_slots > MSGS_TSDF_MAX_SLOTS) return 0;
    return v->n_slots == 0 || (v->table && v->slot_block && v->tsdf_sum && v->weight_sum);
}

static int tsdf_frames_ok(const msgs_tsdf_frames_t* f) {
    if (!f || f->n < 0 || f->n > 65535 || f->W < 1 || f->H < 1 || (int64_t)f->W * f->H >= ((int64_t)1 << 29)) return 0;
    if (!(f->sdf_trunc > 0.f) || !(f->sdf_trunc < INFINITY) || !(f->depth_trunc > 0.f)) return 0;
    return f->n == 0 || (f->cameras && f->depth);
}

int msgs_tsdf_mark_blocks(const msgs_tsdf_volume_t* v, const msgs_tsdf_frames_t* f, int32_t steps, uint8_t* marks, void* stream) {
    if (!tsdf_geometry_ok(v) || !tsdf_frames_ok(f) || steps < 1 || steps > (1 << 16) || !marks) return MSGS_ERR_INVALID_ARG;
    if (f->n == 0) return MSGS_OK;
    HIP_TRY(launch_tsdf_mark_blocks(*v, *f, steps, marks, (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_tsdf_integrate(const msgs_tsdf_volume_t* v, const msgs_tsdf_frames_t* f, void* stream) {
    if (!tsdf_pool_ok(v) || !tsdf_frames_ok(f)) return MSGS_ERR_INVALID_ARG;
    if (f->n > 0 && f->colour && !v->colour_sum) return MSGS_ERR_INVALID_ARG;      // colours with nowhere to go
    if (f->n > 0 && v->n_slots > 0 && v->colour_sum && !f->colour) return MSGS_ERR_INVALID_ARG;
    if (v->n_slots == 0 || f->n == 0) return MSGS_OK;
    HIP_TRY(launch_tsdf_integrate(*v, *f, (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_tsdf_count(const msgs_tsdf_volume_t* v, uint8_t* edge_mask, int32_t* vertex_count, int32_t* triangle_count,
                    void* stream) {
    if (!tsdf_pool_ok(v)) return MSGS_ERR_INVALID_ARG;
    if (v->n_slots == 0) return MSGS_OK;
    if (!edge_mask || !vertex_count || !triangle_count) return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_tsdf_count(*v, edge_mask, vertex_count, triangle_count, (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_tsdf_emit(const msgs_tsdf_volume_t* v, const msgs_tsdf_mesh_t* m, void* stream) {
    if (!tsdf_pool_ok(v) || !m || m->n_vertices < 0 || m->n_faces < 0) return MSGS_ERR_INVALID_ARG;
    if (v->n_slots == 0 || (m->n_vertices == 0 && m->n_faces == 0)) return MSGS_OK;
    if (!m->edge_mask || !m->vertex_offset || !m->triangle_offset) return MSGS_ERR_INVALID_ARG;
    if ((m->n_vertices > 0 && (!m->vertices || (v->colour_sum && !m->colours))) || (m->n_faces > 0 && !m->faces))
        return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_tsdf_emit(*v, *m, (hipStream_t)stream));
    return MSGS_OK;
}

// ---- k-means vector quantisation (SPEC M21) ----
static int vq_shape_ok(int64_t P, int32_t D, int32_t K) {
    return P >= 0 && P < ((int64_t)1 << 31) && D >= 1 && D <= MSGS_VQ_MAX_DIM && K >= 1 && K <= MSGS_VQ_MAX_CODES;
}

size_t msgs_vq_scratch_bytes(int64_t P, int32_t D, int32_t K) {
    if (!vq_shape_ok(P, D, K)) return 0;
    const size_t a = vq_assign_scratch_bytes(D, K), u = vq_update_scratch_bytes(P, D, K);
    return a > u ? a : u;
}

int msgs_vq_assign(int64_t P, int32_t D, int32_t K, const float* x, const float* codebook, int32_t* idx, float* err,
                   void* scratch, size_t scratch_bytes, void* stream) {
    if (!vq_shape_ok(P, D, K) || !codebook) return MSGS_ERR_INVALID_ARG;
    if (P == 0) return MSGS_OK;
    if (!x || !idx || !scratch || ((uintptr_t)scratch & 15)) return MSGS_ERR_INVALID_ARG;
    if (scratch_bytes < vq_assign_scratch_bytes(D, K)) return MSGS_ERR_CAPACITY;
    HIP_TRY(launch_vq_assign(P, D, K, x, codebook, idx, err, (char*)scratch, (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_vq_update(int64_t P, int32_t D, int32_t K, const float* x, const float* w, const int64_t* order, const int32_t* offsets,
                   const int32_t* chunk_offsets, const float* codebook, float* new_codebook, double* mass, int32_t* count,
                   void* scratch, size_t scratch_bytes, void* stream) {
    if (!vq_shape_ok(P, D, K) || !offsets || !chunk_offsets || !codebook || !new_codebook || !mass || !count)
        return MSGS_ERR_INVALID_ARG;
    if ((P > 0 && (!x || !order)) || !scratch || ((uintptr_t)scratch & 15)) return MSGS_ERR_INVALID_ARG;
    if (scratch_bytes < vq_update_scratch_bytes(P, D, K)) return MSGS_ERR_CAPACITY;
    HIP_TRY(launch_vq_update(P, D, K, x, w, order, offsets, chunk_offsets, codebook, new_codebook, mass, count, (char*)scratch,
                             (hipStream_t)stream));
    return MSGS_OK;
}

// ---- connected components and mesh clean-up (SPEC M22) ----
int msgs_graph_components(int64_t N, int64_t E, const int32_t* a, const int32_t* b, int32_t* parent_scratch, int32_t* label,
                          void* stream) {
    if (N < 0 || E < 0 || N >= ((int64_t)1 << 31) || E >= ((int64_t)1 << 31)) return MSGS_ERR_INVALID_ARG;
    if ((E > 0 && (!a || !b)) || (N > 0 && (!parent_scratch || !label))) return MSGS_ERR_INVALID_ARG;
    if (N == 0) return E == 0 ? MSGS_OK : MSGS_ERR_INVALID_ARG;                     // an edge needs a node
    HIP_TRY(launch_graph_components((int32_t)N, E, a, b, parent_scratch, label, (hipStream_t)stream));
    return MSGS_OK;
}

static int mesh_faces_ok(int64_t F) { return F >= 0 && 3 * F < ((int64_t)1 << 31); }

int msgs_mesh_corner_keys(int64_t F, const int32_t* faces, int32_t mode, int64_t* keys, int32_t* face_of_key, void* stream) {
    if (!mesh_faces_ok(F) || (mode != MSGS_MESH_EDGE && mode != MSGS_MESH_VERTEX)) return MSGS_ERR_INVALID_ARG;
    if (F == 0) return MSGS_OK;
    if (!faces || !keys || !face_of_key) return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_mesh_corner_keys(F, faces, mode == MSGS_MESH_VERTEX, keys, face_of_key, (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_mesh_link_sorted(int64_t F, int64_t n_keys, const int64_t* keys_sorted, const int32_t* face_sorted,
                          int32_t* parent_scratch, int32_t* label, void* stream) {
    if (!mesh_faces_ok(F) || n_keys < 0 || n_keys >= ((int64_t)1 << 31)) return MSGS_ERR_INVALID_ARG;
    if (F == 0) return n_keys == 0 ? MSGS_OK : MSGS_ERR_INVALID_ARG;                // a key needs a face
    if ((n_keys > 0 && (!keys_sorted || !face_sorted)) || !parent_scratch || !label) return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_mesh_link_sorted((int32_t)F, n_keys, keys_sorted, face_sorted, parent_scratch, label, (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_mesh_edge_report(int64_t n_keys, const int64_t* keys_sorted, int64_t* counts3, void* stream) {
    if (n_keys < 0 || n_keys >= ((int64_t)1 << 31) || !counts3 || (n_keys > 0 && !keys_sorted)) return MSGS_ERR_INVALID_ARG;
    HIP_TRY(launch_mesh_edge_report(n_keys, keys_sorted, counts3, (hipStream_t)stream));
    return MSGS_OK;
}

static int loss_args_ok(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, float lambda) {
    if (!img || !gt || C < 1 || H < 1 || W < 1 || !(lambda >= 0.f && lambda <= 1.f)) return MSGS_ERR_INVALID_ARG;
    if ((int64_t)C * H * W > (int64_t)1 << 31 || C > 65535) return MSGS_ERR_TOO_MANY;
    return MSGS_OK;
}

size_t msgs_loss_scratch_bytes(int32_t C, int32_t H, int32_t W) {
    if (C < 1 || H < 1 || W < 1) return 0;
    return loss_scratch_bytes(C, H, W);
}

int msgs_loss_forward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                      float* out3, void* scratch, size_t scratch_bytes, int32_t keep_for_backward, void* stream) {
    if (int rc = loss_args_ok(img, gt, C, H, W, lambda_dssim)) return rc;
    if (!out3 || !scratch) return MSGS_ERR_INVALID_ARG;
    if (scratch_bytes < loss_scratch_bytes(C, H, W)) return MSGS_ERR_CAPACITY;
    HIP_TRY(launch_loss_forward(img, gt, C, H, W, lambda_dssim, out3, (char*)scratch, keep_for_backward != 0,
                                (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_loss_backward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                       const float* upstream, const void* scratch, size_t scratch_bytes, float* dL_dimg, void* stream) {
    if (int rc = loss_args_ok(img, gt, C, H, W, lambda_dssim)) return rc;
    if (!dL_dimg || !scratch) return MSGS_ERR_INVALID_ARG;
    if (scratch_bytes < loss_scratch_bytes(C, H, W)) return MSGS_ERR_CAPACITY;
    HIP_TRY(launch_loss_backward(img, gt, C, H, W, lambda_dssim, upstream, (const char*)scratch, dL_dimg,
                                 (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_ssim_window(float* taps11_host) {
    if (!taps11_host) return MSGS_ERR_INVALID_ARG;
    ssim_window_host(taps11_host);
    return MSGS_OK;
}

size_t msgs_knn_scratch_bytes(int64_t P) { return knn_scratch_bytes(P); }

int msgs_dist2_knn3(const float* points, int64_t P, float* mean_dist2, void* scratch, size_t scratch_bytes,
                    void* stream) {
    if (P < 4 || !points || !mean_dist2 || !scratch) return MSGS_ERR_INVALID_ARG;
    if (P > 0x7FFFFFFFll) return MSGS_ERR_TOO_MANY;
    if (scratch_bytes < knn_scratch_bytes(P)) return MSGS_ERR_CAPACITY;
    HIP_TRY(knn_mean_dist2(points, P, mean_dist2, (char*)scratch, (hipStream_t)stream));
    return MSGS_OK;
}

size_t msgs_voxel_pool_scratch_bytes(int64_t M) { return voxel_pool_scratch_bytes(M); }

int msgs_voxel_pool_build(const float* positions, int64_t M, float voxel_size, uint32_t* order, uint32_t* seg_start,
                          int32_t* voxel_index, void* scratch, size_t scratch_bytes, int64_t* num_voxels_host,
                          void* stream) {
    if (!num_voxels_host || M < 0 || !(voxel_size > 0.f)) return MSGS_ERR_INVALID_ARG;
    *num_voxels_host = 0;
    if (M == 0) return MSGS_OK;
    if (M > 0x7FFFFFFFll) return MSGS_ERR_TOO_MANY;
    if (!positions || !order || !seg_start || !scratch) return MSGS_ERR_INVALID_ARG;
    if (scratch_bytes < voxel_pool_scratch_bytes(M)) return MSGS_ERR_CAPACITY;
    HIP_TRY(voxel_pool_build(positions, M, voxel_size, order, seg_start, voxel_index, (char*)scratch, num_voxels_host,
                             (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_voxel_pool_average(const float* features, int32_t F, const uint32_t* order, const uint32_t* seg_start,
                            int64_t num_voxels, float* out, void* stream) {
    if (F < 0 || num_voxels < 0) return MSGS_ERR_INVALID_ARG;
    if (F == 0 || num_voxels == 0) return MSGS_OK;
    if (!features || !order || !seg_start || !out) return MSGS_ERR_INVALID_ARG;
    HIP_TRY(voxel_pool_average(features, F, order, seg_start, num_voxels, out, (hipStream_t)stream));
    return MSGS_OK;
}

int msgs_timing_create(msgs_timing_t* t) {
    if (!t) return MSGS_ERR_INVALID_ARG;
    std::memset(t, 0, sizeof(*t));
    for (int i = 0; i < 2 * MSGS_K_COUNT; ++i) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        t->ev[i] = (void*)e;
    }
    return MSGS_OK;
}

int msgs_timing_destroy(msgs_timing_t* t) {
    if (!t) return MSGS_ERR_INVALID_ARG;
    for (int i = 0; i < 2 * MSGS_K_COUNT; ++i)
        if (t->ev[i]) { (void)hipEventDestroy((hipEvent_t)t->ev[i]); t->ev[i] = nullptr; }
    return MSGS_OK;
}

int msgs_timing_read(const msgs_timing_t* t, float* ms_host) {
    if (!t || !ms_host) return MSGS_ERR_INVALID_ARG;
    for (int k = 0; k < MSGS_K_COUNT; ++k) {
        float ms = -1.0f;
        if (t->ev[2 * k] && t->ev[2 * k + 1]) {
            if (hipEventElapsedTime(&ms, (hipEvent_t)t->ev[2 * k], (hipEvent_t)t->ev[2 * k + 1]) != hipSuccess) {
                ms = -1.0f;
                (void)hipGetLastError();
            }
        }
        ms_host[k] = ms;
    }
    return MSGS_OK;
}

}  // extern "C"

/*
 * msgs.h — C ABI of libmsgs_hip.so, the MI355X (gfx950) multi-scale 3D-Gaussian rasterizer.
 *
 * This is the drop-in boundary for the reference's un-vendored native module
 * `diff_gaussian_rasterization._C` (imported at /root/reference/gaussian_renderer/__init__.py:14,
 * constructed :37-55, called :94-108).  The reference binds that module with pybind11/torch; this
 * library is bound with ctypes from ms-gs_amd/diff_gaussian_rasterization/__init__.py (see
 * INTEGRATION.md for the stub a maintainer adds).  Plain pointers and sizes only: no torch types,
 * no C++ types, nothing thrown across the boundary.
 *
 *   reference entry point (upstream name)                 replaced by
 *   ---------------------------------------------------   ---------------------------------------
 *   _C.rasterize_gaussians(...)            (forward)      msgs_forward_stage1 + msgs_forward_stage2
 *   _C.rasterize_gaussians_backward(...)   (backward)     msgs_backward
 *   _C.mark_visible(...)                   (unused by the reference)
 *                                                          msgs_mark_visible
 *   resize-callback byte tensors (geom/binning/img state)  msgs_*_bytes size queries; the CALLER
 *                                                          allocates (torch caching allocator) and
 *                                                          keeps the buffers alive for backward
 *
 * Ownership: every pointer is owned by the caller; the library never allocates device memory,
 * never frees or retains a pointer past the call.  All `const float*` / `float*` arguments are
 * DEVICE pointers unless the name says `host`.  Calls are asynchronous on `stream` except that
 * msgs_forward_stage1 synchronises the stream once to return the instance count (the same D2H
 * `num_rendered` read the reference's forward performs).
 *
 * Threading: re-entrant (forward is called from the Python main thread, backward from PyTorch's
 * autograd thread).  Not stateless:
 *   - four PROCESS-WIDE mode flags: msgs_set_deterministic, msgs_set_backward_generation, msgs_set_blend_granularity,
 *     msgs_set_occlusion (the last three only choose between code paths that give the same results);
 *   - five environment variables latched on first use (process-wide): the initial values of the four flags
 *     (MSGS_DETERMINISTIC, MSGS_BWD_GEN, MSGS_BLEND_GRANULARITY, MSGS_NO_OCCLUSION) and MSGS_BLOCKING_SYNC — how the
 *     host learns the instance count; none changes a result.
 *     The A/B switches of rounds 1-5 (sort / scan / emit / forward-list variants, MSGS_DEPTH_SORT_BEGIN_BIT) are gone from the
 *     product together with the code paths they selected;
 *   - one 64-byte pinned status block per calling host thread for the calls that WAIT for the instance count
 *     (msgs_forward, msgs_forward_stage1), and one per msgs_status_t handle for msgs_forward_launch /
 *     msgs_forward_finish — any number of forwards may be in flight from one host thread on any streams, one per handle.
 *
 * Return value: 0 = MSGS_OK; < 0 = invalid argument / capacity (MSGS_ERR_*); > 0 = hipError_t.
 */
#ifndef MSGS_H_
#define MSGS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSGS_ABI_VERSION 11

#define MSGS_OK 0
#define MSGS_ERR_INVALID_ARG (-1)  /* NULL / inconsistent pointers (both or neither of shs|colors, ...) */
#define MSGS_ERR_CAPACITY (-2)     /* a caller-supplied buffer is smaller than the size query says   */
#define MSGS_ERR_TOO_MANY (-3)     /* more than 2^32-1 tile instances                                */
#define MSGS_ERR_SH_DEGREE (-4)    /* sh_degree outside 0..3 or (sh_degree+1)^2 > sh_coeffs          */
#define MSGS_ERR_INTERNAL (-5)     /* a bounded inter-workgroup wait expired (sort/scan look-back)     */
#define MSGS_ERR_NO_WEIGHT (-6)    /* msgs_mcmc_sample: no row of positive weight to draw from         */

#define MSGS_TILE 16               /* 16x16 pixel tiles                     */

/* View / raster settings: the 15 fields of GaussianRasterizationSettings
 * (/root/reference/gaussian_renderer/__init__.py:37-53). */
typedef struct msgs_view {
    int32_t image_height;
    int32_t image_width;
    float tanfovx;
    float tanfovy;
    float scale_modifier;
    float fade_size;
    int32_t sh_degree;        /* active degree 0..3                                                 */
    int32_t sh_coeffs;        /* K: coefficients stored per Gaussian in `shs` ((max_degree+1)^2)    */
    int32_t filter_small;     /* bool */
    int32_t filter_large;     /* bool */
    int32_t prefiltered;      /* bool (accepted; the reference always passes False)                  */
    int32_t debug;            /* bool: synchronise + return the first HIP error after every stage   */
    int32_t no_heavy_queue;   /* bool (not a reference field), a performance hint only: "an ordinary view" — Gaussians with more than
                               * 96 tile instances are emitted by their wave inside the emit kernel instead of being queued for a
                               * second launch that gives each a workgroup (binning.hip).  The queue pays off when opaque covers
                               * closed blocks and the nearest depth ranks are all giants (0.28 -> 0.05 ms on the multi-scale model
                               * rendered without its filters); on an ordinary view it is one wasted launch (~3 us).  A caller that
                               * renders similar views in a loop sets it while msgs_forward_info says no block closed lately.
                               * Same outputs either way                                                                      */
    int32_t feedback_tag;     /* (not a reference field) non-zero: the forward ends with one small kernel that publishes what
                               * this view cost — instances D, traversed tile-list entries D_trav (sum over tiles of the last list
                               * position any pixel blended), and the slab numbers below — together with this tag in the pinned
                               * status block; msgs_forward_info returns the most recent publication, so a caller that renders
                               * similar views in a loop learns, one frame late and without any synchronisation, whether depth
                               * slabs pay off for that kind of view.  0: nothing is published (no extra launch)               */
    float slab_fraction;      /* (not a reference field) > 0: DEPTH-SLAB BINNING (round 6).  Stage 2 first bins and blends only the
                               * nearest depth ranks — up to this fraction of the D tile instances (slab A) —; the forward blend
                               * marks the tiles in which a pixel is still blending at the end of its slab-A list; the rest of
                               * the view (slab B) is then counted, emitted and sorted into THOSE tiles only (their complete
                               * lists, slab-A entries included) and they are blended again over the complete list.  A tile
                               * whose every pixel terminated inside slab A never evaluates an entry behind it (Q7), so every
                               * output, n_contrib, final_T and every gradient is bit-identical to the single-pass path; what
                               * shrinks is the work of emit / tile sort / ranges on instances nobody walks (BASELINE C5: 54.9 M
                               * instances, 4.35 M walked).  Needs binning >= msgs_binning_bytes_slab(D, W, H, fraction); ignored
                               * (single pass) with fewer than 2048 tiles, in deterministic mode, with fine blend granularity
                               * forced, or when the buffers are too small.  0: single pass.  With the two-call form pass the
                               * SAME value to msgs_forward_stage1: its scan then hands slab B's count the coarse screen-cell
                               * range of every Gaussian in depth order; without them (stage 1 called with 0) slab B still gives
                               * the same results but fetches every Gaussian's record to learn that it has nothing to add   */
    int32_t reserved1;        /* 0 */
    const float* bg;          /* [3]   device                                                        */
    const float* viewmatrix;  /* [16]  device; world_view_transform = W2C^T row-major (cameras.py:54) */
    const float* projmatrix;  /* [16]  device; full_proj_transform (cameras.py:55-56)                */
    const float* campos;      /* [3]   device; camera_center (cameras.py:57)                         */
} msgs_view_t;

/* Per-Gaussian inputs: the 13 kwargs of GaussianRasterizer.forward
 * (/root/reference/gaussian_renderer/__init__.py:95-107).  means2D carries no data forward (it is
 * the gradient sink, :27-31) and therefore only appears in msgs_backward. */
typedef struct msgs_gaussians {
    int32_t P;
    int32_t raw_params;            /* 0: activated inputs, the reference's op API.  1: RAW GaussianModel parameters
                                    * (opt-in): opacities = logits, scales = log-scales,
                                    * rotations = un-normalised quaternions, SH given as features_dc + features_rest
                                    * (shs / colors_precomp / cov3D_precomp must be NULL, sh_coeffs = 16); the
                                    * activations of scene/gaussian_model.py:39-47,127-153 (exp, sigmoid, normalize)
                                    * and the torch.cat of :144-149 are evaluated inside the kernels and msgs_backward
                                    * returns gradients w.r.t. the raw parameters.
                                    * 2: CHAINED gradients: opacities / scales / rotations are the ACTIVATED values
                                    * exactly as in mode 0 (the forward is bit-identical to mode 0), the SH
                                    * coefficients are read from features_dc + features_rest (whose concatenation the
                                    * reference passes as `shs`; `shs` may be given as well and is then the one read:
                                    * aligned rows, only the visible ones), rotations_raw holds the raw quaternions, and
                                    * msgs_backward applies the chain rule of sigmoid / exp / normalize / cat itself:
                                    * dL_dopacities, dL_dscales, dL_drotations, dL_dfeatures_dc/_rest are gradients
                                    * w.r.t. the RAW parameters — what autograd would produce by running the backward
                                    * of the reference's getters after the op */
    const float* means3D;          /* [P,3]                                                          */
    const float* shs;              /* [P,K,3]  xor colors_precomp                                    */
    const float* colors_precomp;   /* [P,3]                                                          */
    const float* opacities;        /* [P] (the reference passes [P,1])                               */
    const float* scales;           /* [P,3]    with rotations, xor cov3D_precomp                     */
    const float* rotations;        /* [P,4]    (w,x,y,z), pre-normalised (gaussian_model.py:132-133) */
    const float* cov3D_precomp;    /* [P,6]    xx,xy,xz,yy,yz,zz (general_utils.py:64-73)            */
    const float* max_pixel_sizes;  /* [P]      -1 = unset (gaussian_model.py:224)                    */
    const float* min_pixel_sizes;  /* [P]      -1 = unset (gaussian_model.py:225)                    */
    const float* occ_multiplier;   /* [P,4]    never read: the caller guarantees all ones (SPEC M5)   */
    const float* dc_delta;         /* [P,12]   never read: the caller guarantees all zeros (SPEC M5)  */
    const uint8_t* base_mask;      /* [P]      bool                                                  */
    const float* features_dc;      /* [P,1,3]  modes 1, 2    (gaussian_model.py:55)                          */
    const float* features_rest;    /* [P,15,3] modes 1, 2    (gaussian_model.py:56)                          */
    const float* rotations_raw;    /* [P,4]    mode 2 only: the un-normalised quaternions (gaussian_model.py:58)  */
} msgs_gaussians_t;

/* Optimizer step INSIDE the per-Gaussian backward (msgs_grads_t::adam_in_backward; ABI 11).  The reference's iteration is
 * loss.backward() -> optimizer.step() (/root/reference/train.py:216, :416-418) with torch.optim.Adam(lr = 0.0, eps = 1e-15) over
 * the leaf tensors (/root/reference/scene/gaussian_model.py:235-248): backward writes 59 gradient floats per Gaussian (236 B at
 * SH degree 3, zeros for Gaussians the view did not render) and the optimizer reads them back.  With this struct the kernel that
 * FORMS the raw-parameter gradients applies the Adam update to the parameter and its two moments on the spot — same arithmetic,
 * term by term, as msgs_adam_step (bit-identical parameters and moments) — and the gradient tensors are neither written nor
 * read.  Raw mode 1 only (the gradients must be those of the leaves), scales + rotations and SH given as features_dc /
 * features_rest with sh_coeffs == 16, no accumulate, no factored SH gradient.  The parameters are the tensors of
 * msgs_gaussians_t (means3D, features_dc, features_rest, opacities, scales, rotations — written through their const pointers),
 * every row is updated (a Gaussian that was not rendered has gradient zero: its moments decay and it moves, as under
 * torch.optim.Adam with dense zero gradients).  All 18 tensors 16-byte aligned.  dL_dmeans2D is still stored. */
typedef struct msgs_adam_moments {
    float* exp_avg;            /* same shape as the parameter                                        */
    float* exp_avg_sq;
    double lr;                 /* this tensor's learning rate (param_group["lr"])                    */
} msgs_adam_moments_t;
typedef struct msgs_adam_in_backward {
    int64_t step;              /* the step being taken, >= 1 (bias corrections 1 - beta^step)        */
    double beta1, beta2, eps;
    msgs_adam_moments_t t[6];  /* means3D, features_dc, features_rest, opacities, scales, rotations  */
} msgs_adam_in_backward_t;

/* Gradient outputs of msgs_backward.  Every non-NULL buffer is fully written (zeros for
 * Gaussians that were not rendered), so the caller may pass uninitialised memory. */
typedef struct msgs_grads {
    float* dL_dmeans3D;        /* [P,3]                                                              */
    float* dL_dmeans2D;        /* [P,3]   (x,y in the NDC-ish units of SURVEY App. A.3; z = 0)       */
    float* dL_dshs;            /* [P,K,3] when shs was given                                         */
    float* dL_dcolors;         /* [P,3]   when colors_precomp was given; also in the raw modes with both
                                *          dL_dfeatures_* NULL: the FACTORED SH gradient — the clamp-masked dL/drgb
                                *          of this view, from which msgs_sh_grad_from_views rebuilds dL/dSH      */
    float* dL_dopacities;      /* [P]                                                                */
    float* dL_dscales;         /* [P,3]   when scales/rotations were given                           */
    float* dL_drotations;      /* [P,4]                                                              */
    float* dL_dcov3D;          /* [P,6]   when cov3D_precomp was given                               */
    float* dL_dfeatures_dc;    /* [P,1,3]  raw mode only                                                     */
    float* dL_dfeatures_rest;  /* [P,15,3] raw mode only                                                     */
    void* factors_ready;       /* optional hipEvent_t, factored SH gradient only: dL_dcolors is written by a kernel of its
                                * own BEFORE the per-Gaussian backward and this event is recorded right behind it, so that
                                * the caller can start the all-gather of the factors while the rest of msgs_backward runs */
    int32_t scratch_is_clear;  /* non-zero: the first msgs_backward_scratch_bytes(P) bytes of `scratch` were handed to the
                                * forward of THIS view as grad_records (it cleared them during the blend) and nothing has
                                * written them since: msgs_backward skips its own fill launch.  0: msgs_backward clears them.
                                * Also non-zero when the records hold sums that are to be INCLUDED: msgs_features_backward adds
                                * its geometry sums to cleared records in front of msgs_backward*, which then adds on top */
    int32_t accumulate;        /* non-zero: ADD this view's gradients to what the output tensors hold (dL_dmeans3D, dL_dshs /
                                * dL_dfeatures_*, dL_dcolors, dL_dopacities, dL_dscales, dL_drotations, dL_dcov3D), leaving the
                                * rows of Gaussians this view did not render untouched — the views of one optimizer step
                                * accumulate into ONE gradient bucket without zero rows and without a separate accumulation
                                * pass (the reference's autograd does `param.grad += view_grad`: 3 x 236 B per Gaussian and
                                * view at SH degree 3).  dL_dmeans2D stays per view (always stored).  The first view of a step
                                * is called with 0 (it initialises every row).  Not with sh_coeffs != 16 on the reference API. */
    void* wait_before_accumulate; /* optional hipEvent_t: the per-Gaussian kernel waits for it — the `accumulated` event of the
                                * previous view into the same tensors when that view ran on ANOTHER stream */
    void* accumulated;         /* optional hipEvent_t recorded behind the per-Gaussian kernel */
    const msgs_adam_in_backward_t* adam_in_backward;   /* NULL (default) or the optimizer step to take inside the per-Gaussian
                                * kernel (above): dL_dmeans3D, dL_dfeatures_*, dL_dopacities, dL_dscales, dL_drotations are then
                                * ignored and may be NULL */
} msgs_grads_t;

/* Optional per-kernel timing (bench.py's roofline leg).  The caller owns the events; the library
 * records ev[2*k] before and ev[2*k+1] after kernel class k on `stream`.  NULL = no timing. */
enum {
    MSGS_K_PREPROCESS = 0, MSGS_K_DEPTH_SORT = 1, MSGS_K_SCAN = 2, MSGS_K_EMIT = 3,
    MSGS_K_TILE_SORT = 4, MSGS_K_RANGES = 5, MSGS_K_BLEND_FWD = 6, MSGS_K_BLEND_BWD = 7,
    MSGS_K_PREPROCESS_BWD = 8,
    MSGS_K_SLAB_B = 9,        /* slab mode only: the whole second pass (count, scan, emit, tile sort, ranges, blend of the open tiles) */
    MSGS_K_COUNT = 10
};
typedef struct msgs_timing {
    void* ev[2 * MSGS_K_COUNT];   /* hipEvent_t handles created by the caller (msgs_timing_create) */
} msgs_timing_t;

int msgs_abi_version(void);
const char* msgs_error_string(int code);

/* ---- size queries (bytes) -------------------------------------------------------------------- */
/* per-Gaussian state written by stage 1, read by stage 2 and by backward */
size_t msgs_geom_bytes(int32_t P);
/* scratch of stage 1 (depth sort double buffers, scan partials); dead after stage 1 returns */
size_t msgs_stage1_scratch_bytes(int32_t P);
/* per-instance state written by stage 2 (sorted Gaussian ids + tile ranges), read by backward */
size_t msgs_binning_bytes(int64_t num_instances, int32_t width, int32_t height);
/* the same for a call with msgs_view_t.slab_fraction = fraction > 0: room for slab A's instances in front of the open tiles'
 * complete lists (<= (1 + fraction) D + one instance per tile) */
size_t msgs_binning_bytes_slab(int64_t num_instances, int32_t width, int32_t height, float slab_fraction);
size_t msgs_stage2_scratch_bytes_slab(int64_t num_instances, int32_t width, int32_t height);
/* scratch of stage 2 (tile sort double buffers, histograms); dead after stage 2 returns */
size_t msgs_stage2_scratch_bytes(int64_t num_instances, int32_t width, int32_t height);
/* per-pixel state written by stage 2 (final transmittance, last contributor), read by backward */
size_t msgs_image_bytes(int32_t width, int32_t height);
/* scratch of backward (per-Gaussian 2-D gradient records) */
size_t msgs_backward_scratch_bytes(int32_t P);

/* ---- forward --------------------------------------------------------------------------------- */
/* Stage 1: preprocess (projection, EWA splat, SH->RGB, pixel size, multi-scale filters, exact
 * tile-overlap count), depth sort of the Gaussians, exclusive scan of the overlap counts.
 * Writes radii[P] (int32, 0 = not rendered) and pixel_sizes[P]; returns the number of tile
 * instances through *num_instances_host after ONE stream synchronisation. */
int msgs_forward_stage1(const msgs_view_t* view, const msgs_gaussians_t* g,
                        int32_t* radii, float* pixel_sizes,
                        void* geom, size_t geom_bytes,
                        void* scratch, size_t scratch_bytes,
                        int64_t* num_instances_host,
                        const msgs_timing_t* timing, void* stream);

/* Stage 2: emit (tile, Gaussian) instances in depth order, stable radix sort by tile, tile ranges,
 * per-tile front-to-back alpha blend.  Writes out_color[3,H,W], out_acc_pixel_size[H,W],
 * out_depth[H,W]. */
int msgs_forward_stage2(const msgs_view_t* view, const msgs_gaussians_t* g,
                        const void* geom, size_t geom_bytes,
                        int64_t num_instances,
                        void* binning, size_t binning_bytes,
                        void* scratch, size_t scratch_bytes,
                        void* image_state, size_t image_bytes,
                        float* out_color, float* out_acc_pixel_size, float* out_depth,
                        void* grad_records, size_t grad_records_bytes, int32_t backward_follows,
                        const msgs_timing_t* timing, void* stream);
/* backward_follows: non-zero when msgs_backward will be called on this forward's state — the forward then also leaves the
 * backward's heaviest-first tile launch order behind (one small kernel).  Independent of grad_records.
 * grad_records (optional, NULL = none): the buffer the caller will pass to msgs_backward as `scratch`
 * (>= msgs_backward_scratch_bytes(P)).  The per-Gaussian gradient records in it have to start from zero; the blend
 * kernel of the forward clears them on the side (it is instruction-bound, the stores are free there), and a
 * msgs_backward called with msgs_grads_t.scratch_is_clear = 1 saves the fill launch. */

/* ---- backward -------------------------------------------------------------------------------- */
/* dL_dcolor is [3,H,W].  acc_pixel_size / depth / pixel_sizes carry no gradient here (they never
 * enter the reference's loss, /root/reference/train.py:205-216); msgs_backward_with_depth adds the depth map's. */
int msgs_backward(const msgs_view_t* view, const msgs_gaussians_t* g,
                  const int32_t* radii,
                  const void* geom, size_t geom_bytes,
                  int64_t num_instances,
                  const void* binning, size_t binning_bytes,
                  const void* image_state, size_t image_bytes,
                  const float* dL_dcolor,
                  void* scratch, size_t scratch_bytes,
                  const msgs_grads_t* grads,
                  const msgs_timing_t* timing, void* stream);

/* msgs_backward_with_depth: msgs_backward plus the gradient of the depth map (D_p = sum_i z_i alpha_i T_i,
 * no background term).  dL_ddepth is [H,W] float32, NULL = none — then exactly msgs_backward (same kernels, same bits).
 * Non-NULL: the depth variants of the blend-backward and per-Gaussian kernels run; depth's share z_i dL/dD enters
 * dL/dalpha (-> opacity, conic, mean2D and everything behind them) and dL/dz_i = sum_p dL/dD alpha_i T_i reaches dL/dmeans3D
 * through the view matrix.  acc_pixel_size, radii and pixel_sizes stay without gradient.  In the verification mode
 * (msgs_set_deterministic) the scratch buffer must hold msgs_backward_scratch_bytes_deterministic_depth(P, D) bytes. */
int msgs_backward_with_depth(const msgs_view_t* view, const msgs_gaussians_t* g,
                             const int32_t* radii,
                             const void* geom, size_t geom_bytes,
                             int64_t num_instances,
                             const void* binning, size_t binning_bytes,
                             const void* image_state, size_t image_bytes,
                             const float* dL_dcolor, const float* dL_ddepth,
                             void* scratch, size_t scratch_bytes,
                             const msgs_grads_t* grads,
                             const msgs_timing_t* timing, void* stream);

/* msgs_backward_with_camera: msgs_backward_with_depth plus the gradients of the camera: dL_dviewmatrix [16],
 * dL_dprojmatrix [16] and dL_dcampos [3], float32 device pointers in the layout of msgs_view_t's viewmatrix / projmatrix /
 * campos, each NULL = not wanted.  All three NULL: exactly msgs_backward_with_depth (same kernels, same bits).  Otherwise the
 * camera variant of the per-Gaussian kernel writes one row of double partial sums per workgroup to camera_scratch
 * (>= msgs_camera_grad_scratch_bytes(P)) and two small launches add the rows in a fixed partition and order: no atomics, the
 * same bits on every run.  The camera outputs are always overwritten (also under grads->accumulate), with 0 where an entry never enters
 * the computation (viewmatrix column 3: flat 3, 7, 11, 15; projmatrix column 2: flat 2, 6, 10, 14) and for P = 0.  Culling,
 * radii, tile assignment, sort order, filter weights and pixel sizes are constants; tanfovx / tanfovy and bg get no
 * gradient.  Not with grads->adam_in_backward (MSGS_ERR_INVALID_ARG). */
int msgs_backward_with_camera(const msgs_view_t* view, const msgs_gaussians_t* g,
                              const int32_t* radii,
                              const void* geom, size_t geom_bytes,
                              int64_t num_instances,
                              const void* binning, size_t binning_bytes,
                              const void* image_state, size_t image_bytes,
                              const float* dL_dcolor, const float* dL_ddepth,
                              void* scratch, size_t scratch_bytes,
                              const msgs_grads_t* grads,
                              float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos,
                              void* camera_scratch, size_t camera_scratch_bytes,
                              const msgs_timing_t* timing, void* stream);
/* bytes of msgs_backward_with_camera's camera_scratch for P Gaussians (no clearing needed) */
size_t msgs_camera_grad_scratch_bytes(int32_t P);

/* ---- alpha map and background gradient -------------------------------------- */
/* msgs_alpha_map: the accumulated opacity of every pixel, out_alpha [H,W] float32 = 1 - final_T, from the transmittance the
 * forward of this view left in image_state (>= msgs_image_bytes(W, H)); one float32 subtraction per pixel, 0 where nothing was
 * blended.  In exact arithmetic sum_i alpha_i T_i: the colour of a render with colour 1 over background 0.  Call it behind
 * the forward that filled image_state, on the same stream (again behind a stage 2 that was run a second time). */
int msgs_alpha_map(const msgs_view_t* view, const void* image_state, size_t image_bytes, float* out_alpha, void* stream);

/* msgs_backward_with_alpha: msgs_backward_with_camera plus the gradient of the alpha map.  dL_dalpha is [H,W] float32,
 * NULL = none — then exactly msgs_backward_with_camera (same kernels, same bits).  Non-NULL: the alpha variants of the
 * blend-backward kernels run; G_p = dL/dA_p adds G_p T_final / (1 - alpha_i) to dL/dalpha_i (the background term with -G_p
 * beside bg . dL/dC) and reaches opacity, conic, mean2D and everything behind them; alpha carries no colour or SH gradient.
 * The sums, the records, the per-Gaussian kernel and every scratch size are those of the call without dL_dalpha; every mode
 * of msgs_backward_with_camera is served (raw_params 0 / 1 / 2, accumulate, factored SH, depth, the verification mode, and
 * adam_in_backward when no camera gradient is wanted). */
int msgs_backward_with_alpha(const msgs_view_t* view, const msgs_gaussians_t* g,
                             const int32_t* radii,
                             const void* geom, size_t geom_bytes,
                             int64_t num_instances,
                             const void* binning, size_t binning_bytes,
                             const void* image_state, size_t image_bytes,
                             const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                             void* scratch, size_t scratch_bytes,
                             const msgs_grads_t* grads,
                             float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos,
                             void* camera_scratch, size_t camera_scratch_bytes,
                             const msgs_timing_t* timing, void* stream);

/* msgs_bg_grad: the gradient of the background colour, dL_dbg [3] float32 (device) = sum_p final_T_p dL/dC_{c,p} — view->bg
 * enters every pixel as final_T bg.  image_state = NULL: final_T = 1 everywhere (a view without Gaussians, which has no image
 * state).  Each product is rounded to float32 and added in double: one [3] row of doubles per workgroup goes to `scratch`
 * (>= msgs_bg_grad_scratch_bytes(W, H), no clearing needed) in a partition that depends on W H alone, and a second launch adds
 * the rows in index order — no atomics, the same bits on every run.  Independent of the backward calls: dL_dbg is always
 * overwritten and msgs_grads_t.accumulate does not reach it. */
size_t msgs_bg_grad_scratch_bytes(int32_t width, int32_t height);
int msgs_bg_grad(const msgs_view_t* view, const void* image_state, size_t image_bytes, const float* dL_dcolor,
                 float* dL_dbg, void* scratch, size_t scratch_bytes, void* stream);

/* ---- absgrad: absolute screen-space gradients for densification (DESIGN.md SPEC M10, 4.10) ------ */
/* msgs_absgrad: out_absgrad [P,3] float32 = {ln2 W sum_p |q_ip u_ip|, ln2 H sum_p |q_ip w_ip|, 0} — dL/dmean2D with the
 * absolute value of every pixel's contribution summed instead of the signed one (AbsGS; gsplat's absgrad), in the units of
 * msgs_grads_t.dL_dmeans2D.  A Gaussian that some pixels pull one way and others the other cancels in dL_dmeans2D and not here;
 * |absgrad| >= |dL_dmeans2D| componentwise, equality for a loss on one pixel, 0 for a Gaussian in no tile list.  One replay of
 * the blend backward's walk over exactly the pairs msgs_backward* counts, with dL_ddepth / dL_dalpha (NULL = none) entering as
 * they do there.  Reads what the forward of this view left in geom / binning / image_state (single pass, depth slabs or
 * occlusion cut-off alike); independent of the msgs_backward* calls, before or behind them on the same stream.  `scratch`
 * (>= msgs_absgrad_scratch_bytes(P), 8-byte aligned, no clearing needed) holds [P,2] doubles: float32 totals per (tile
 * quadrant, entry) are added there, which is exact — the same bits on every run.  P == 0: nothing is launched. */
size_t msgs_absgrad_scratch_bytes(int32_t P);
int msgs_absgrad(const msgs_view_t* view, int32_t P,
                 const void* geom, size_t geom_bytes,
                 int64_t num_instances,
                 const void* binning, size_t binning_bytes,
                 const void* image_state, size_t image_bytes,
                 const float* dL_dcolor, const float* dL_ddepth, const float* dL_dalpha,
                 void* scratch, size_t scratch_bytes,
                 float* out_absgrad, void* stream);

/* ---- contribution scores: what a Gaussian did to the images, for pruning (DESIGN.md SPEC M11, 4.11) ------ */
/* With w_ip = alpha_ip T_ip the blend weight of Gaussian i in pixel p (the weight of dL/dC in the colour gradient) and an
 * optional weight map m_p >= 0 (pixel_weights [H,W] float32, device; NULL = 1 everywhere; a negative or NaN weight counts as 0):
 *     weight_sum_i = sum_p m_p w_ip,   weight_max_i = max_p m_p w_ip,   pixel_count_i = #{p : m_p > 0, pair (i,p) blended}
 * over exactly the pairs msgs_backward* counts.  A Gaussian in no tile list, or with radii = 0, gets (0, 0, 0).  No gradients.
 * msgs_contrib_accumulate adds ONE view to the caller's accumulator `acc` (>= msgs_contrib_scratch_bytes(P), 8-byte aligned):
 * clear_first != 0 zero-fills it first, clear_first == 0 adds to what it holds — sum, max and sum across views, so N views need
 * one accumulator and no per-view [P] arrays.  One replay of the blend backward's walk; reads what the forward of this view
 * left in geom / binning / image_state (single pass, speculative stage 2 or its redo, depth slabs, occlusion cut-off, quadrant
 * or fine forward alike); independent of msgs_backward* and msgs_absgrad.  Per (tile quadrant, entry) a float32 total goes to a
 * double, a maximum to an unsigned integer maximum of the float's bits, a count to a 64-bit integer: all three exact and
 * independent of the order of arrival — the same bits on every run.  P == 0 or num_instances == 0: no replay, only the clear.
 * msgs_contrib_finish converts the accumulator: weight_sum [P] float32, weight_max [P] float32, pixel_count [P] int64. */
size_t msgs_contrib_scratch_bytes(int32_t P);
int msgs_contrib_accumulate(const msgs_view_t* view, int32_t P,
                            const void* geom, size_t geom_bytes,
                            int64_t num_instances,
                            const void* binning, size_t binning_bytes,
                            const void* image_state, size_t image_bytes,
                            const float* pixel_weights, /* [H,W] or NULL */
                            void* acc, size_t acc_bytes, int32_t clear_first, void* stream);
int msgs_contrib_finish(int32_t P, const void* acc, size_t acc_bytes,
                        float* weight_sum, float* weight_max, int64_t* pixel_count, void* stream);

/* ---- feature channels: per-Gaussian vectors splatted with the blend weights (DESIGN.md SPEC M12, 4.12) ------ */
/* features [P,C] float32 (device, C >= 1, 4-byte aligned; 16-byte row loads where C % 4 == 0 and the base allow).  With
 * w_ip = alpha_ip T_ip the blend weight of Gaussian i in pixel p, over exactly the pairs msgs_backward* counts:
 *     msgs_features_forward:   out [C,H,W] float32,  F[c,p] = sum_i f_ic w_ip
 * with NO background term (a pixel with no blended entry gets 0.0f; compose a background outside with the alpha map).  Rows of
 * Gaussians in no tile list are never read.
 *     msgs_features_backward:  dL_dfeatures [P,C] float32 (always overwritten),  dL/df_ic = sum_p G_cp w_ip,  G = dL_dfeature_map
 * exactly 0 for a Gaussian in no list.  grad_records (NULL = no geometry share; else >= msgs_backward_scratch_bytes(P), the
 * buffer handed to msgs_backward* as `scratch`): the features act as C more colour channels over background 0, and the six
 * sums of their q_f (sum q dx, q dy, q dx^2, q dx dy, q dy^2, q) are ADDED to record slots 0..5.  The records must already be
 * zero (cleared by the forward of this view, or by the caller) or hold sums that are to be included; msgs_backward* is then
 * called with msgs_grads_t.scratch_is_clear = 1, adds its own sums on top, and its per-Gaussian stage consumes the total:
 * means, opacity, scales / rotations / cov3D and the camera receive the features' share, SH and colours nothing.
 * `scratch` (>= msgs_features_scratch_bytes(P, C), 8-byte aligned, no clearing needed): one block of double accumulators.
 * Both read what the forward of this view left in geom / binning / image_state (single pass, speculative stage 2 or its redo,
 * depth slabs, occlusion cut-off alike).  P == 0 or num_instances == 0: the forward zero-fills out, the backward zero-fills
 * dL_dfeatures, no replay runs.  Not offered in the verification mode (MSGS_ERR_INVALID_ARG). */
size_t msgs_features_scratch_bytes(int32_t P, int32_t C);
int msgs_features_forward(const msgs_view_t* view, int32_t P,
                          const void* geom, size_t geom_bytes,
                          int64_t num_instances,
                          const void* binning, size_t binning_bytes,
                          const void* image_state, size_t image_bytes,
                          const float* features, int32_t C,
                          float* out, void* stream);
int msgs_features_backward(const msgs_view_t* view, int32_t P,
                           const void* geom, size_t geom_bytes,
                           int64_t num_instances,
                           const void* binning, size_t binning_bytes,
                           const void* image_state, size_t image_bytes,
                           const float* features, int32_t C,
                           const float* dL_dfeature_map,
                           void* grad_records, size_t grad_records_bytes,
                           void* scratch, size_t scratch_bytes,
                           float* dL_dfeatures, void* stream);

/* ---- depth distortion: the spread of a ray's blended mass along the view axis (DESIGN.md SPEC M13, 4.13) ------ */
/* With w_ip = alpha_ip T_ip and z_i the view depth the depth map blends, over exactly the pairs msgs_backward* counts, in
 * tile-list order i = 1..n (front to back):
 *     msgs_distortion_forward:   out_distortion [H,W] float32,  Dist_p = 2 sum_{j<i} w_ip w_jp (z_i - z_j)
 * the signed list-order form of the Mip-NeRF 360 distortion sum_i sum_j w_i w_j |z_i - z_j| (equal to it on a depth-sorted
 * list, and without a kink at ties).  No background term; exactly 0.0f for a pixel with fewer than two counted pairs.
 * out_moment [H,W] float32: sum_i w_ip (z_i - z_ref) with z_ref the view depth of the tile's first list entry — meaningful
 * to msgs_distortion_backward of the same view only, which takes it as `moment`.
 *     msgs_distortion_backward:  dL_ddistortion [H,W] float32 = G.  G dDist/dw_i acts as the only colour channel of pair i over
 * background 0: the six sums of its q (sum q dx, q dy, q dx^2, q dx dy, q dy^2, q) are ADDED to record slots 0..5 of
 * grad_records (>= msgs_backward_scratch_bytes(P), the buffer handed to msgs_backward* as `scratch`) and sum_p G dDist/dz_i to
 * slot 9.  The records must already be zero (cleared by the forward of this view, or by the caller) or hold sums that are to
 * be included; msgs_backward* is then called with msgs_grads_t.scratch_is_clear = 1 and a non-NULL dL_ddepth (a zero map when
 * the loss has no depth term), so that the depth variant of its per-Gaussian stage consumes slot 9: means, opacity, scales /
 * rotations / cov3D and the camera receive the distortion's share, SH and colours nothing.
 * Both read what the forward of this view left in geom / binning / image_state (single pass, speculative stage 2 or its redo,
 * depth slabs, occlusion cut-off alike).  P == 0 or num_instances == 0: the forward zero-fills both maps, the backward launches
 * nothing.  Not offered in the verification mode (MSGS_ERR_INVALID_ARG). */
int msgs_distortion_forward(const msgs_view_t* view, int32_t P,
                            const void* geom, size_t geom_bytes,
                            int64_t num_instances,
                            const void* binning, size_t binning_bytes,
                            const void* image_state, size_t image_bytes,
                            float* out_distortion, float* out_moment, void* stream);
int msgs_distortion_backward(const msgs_view_t* view, int32_t P,
                             const void* geom, size_t geom_bytes,
                             int64_t num_instances,
                             const void* binning, size_t binning_bytes,
                             const void* image_state, size_t image_bytes,
                             const float* moment, const float* dL_ddistortion,
                             void* grad_records, size_t grad_records_bytes, void* stream);

/* ---- median depth and Gaussian id: the Gaussian at which a ray's transmittance falls through 1/2 (DESIGN.md SPEC M15, 4.15) -- */
/* The blended entries i = 1..n of a pixel p are exactly the pairs the forward blended and msgs_backward* counts, in tile-list
 * order (front to back, depth ties in index order): list position below n_contrib[p], exponent passing the sign test,
 * alpha >= 1/255.  Transmittance is the forward's own float32 recurrence, T_1 = 1, T_{i+1} = fmaf(-T_i, alpha_i, T_i) with
 * alpha_i = min(0.99, ...) — not a T rebuilt from final_T by division — so the maps are a deterministic function of what the
 * render blended.  The median entry m(p) is the LAST blended entry with T_i > 0.5 (strict; the 2DGS / gsplat rule): the entry
 * whose blending takes T to <= 1/2, or the last blended entry of a ray that never gets there.
 *     msgs_median_depth_forward:   out_median_depth [H,W] float32 = z_m(p), the float32 view depth the depth map blends;
 *                                  0.0f where nothing was blended.
 *                                  out_median_id [H,W] int32 = the row of that Gaussian in the model; -1 where nothing was
 *                                  blended.  Never differentiable.
 * Reads what the forward of this view left in geom / binning / image_state (single pass, speculative stage 2 or its redo,
 * depth slabs, occlusion cut-off alike).  P == 0 or num_instances == 0: the depth map is zero-filled, the id map filled with -1.
 *     msgs_median_depth_backward:  d median_depth_p / dz_i = [i = m(p)], nothing through the selection.  With
 * dL_dmedian_depth [H,W] float32 = G, sum_{p: median_id[p] = i} G_p is ADDED to slot 9 (dL/dz) of record i of grad_records
 * (>= msgs_backward_scratch_bytes(P), the buffer handed to msgs_backward* as `scratch`); an id outside [0, P) adds nothing.
 * The records must already be zero (cleared by the forward of this view, or by the caller) or hold sums that are to be
 * included; msgs_backward* is then called with msgs_grads_t.scratch_is_clear = 1 and a non-NULL dL_ddepth (a zero map when the
 * loss has no depth term), so that the depth variant of its per-Gaussian stage consumes slot 9: the means and, when asked, the
 * camera receive the map's share; opacity, scales, rotations, means2D, SH and colours exactly nothing.  P == 0: launches
 * nothing.  Neither is offered in the verification mode (MSGS_ERR_INVALID_ARG). */
int msgs_median_depth_forward(const msgs_view_t* view, int32_t P,
                              const void* geom, size_t geom_bytes,
                              int64_t num_instances,
                              const void* binning, size_t binning_bytes,
                              const void* image_state, size_t image_bytes,
                              float* out_median_depth, int32_t* out_median_id, void* stream);
int msgs_median_depth_backward(const msgs_view_t* view, int32_t P,
                               const int32_t* median_id, const float* dL_dmedian_depth,
                               void* grad_records, size_t grad_records_bytes, void* stream);

/* ---- antialiasing: the opacity compensation of the 2-D screen filter as a pre-pass (DESIGN.md SPEC M14, 4.14) ------ */
/* The +0.3 dilation of the projected covariance (Q3) brightens every Gaussian smaller than a pixel.  Mip-Splatting's
 * compensation — upstream 3DGS's antialiasing=True, gsplat's rasterize_mode="antialiased" — scales the opacity by
 *     rho_i = sqrt(max(0.000025, det0 / det1)),   det0 = a0 c0 - b^2,   det1 = (a0 + 0.3)(c0 + 0.3) - b^2
 * with (a0, b, c0) the entries of T Sigma3D T^T before the dilation, the same float32 values msgs_forward* forms for this view
 * (tanfov, image size, scale_modifier and viewmatrix of `view`; scales + rotations or cov3D_precomp of `g`).  An antialiased
 * render IS the plain render — any msgs_forward* / msgs_backward* entry, any opt-in output — of the same model with
 *     msgs_screen_compensation_forward:   o_eff [P] float32,  o_eff_i = o_i rho_i
 * in the place of the opacities; pixel sizes and the multi-scale filters then see o_eff.  rho_i = 1 exactly (o_eff_i = o_i bit
 * for bit, no geometry gradient) where the view depth is <= 0.2 (Q1), where det1 == 0, or where an input of the row or the
 * result is not finite: rows the renderer skips anyway.
 *     msgs_screen_compensation_backward:  from dL_do_eff [P]:  dL_dopacity [P] = rho dL_do_eff;  dL_dmeans3D [P,3];
 *     dL_dscales [P,3] + dL_drotations [P,4], or dL_dcov3D [P,6] (off-diagonals doubled, as msgs_backward writes them) — every row
 *     is written, zeros where rho is 1 or sits on its floor; each pointer may be NULL (not wanted), one for a tensor `g` does
 *     not carry is MSGS_ERR_INVALID_ARG.  dL_dV [16] (may be NULL): dL/dviewmatrix in the flat layout of
 *     msgs_backward_with_camera, through the view-space point and the rotation block, summed over the Gaussians in double in
 *     a fixed order (the same bits on every run); it needs scratch >= msgs_screen_compensation_scratch_bytes(P), 8-byte
 *     aligned.  projmatrix, campos and bg do not enter rho.  The projection is recomputed: nothing is kept from the forward.
 * Reference-API inputs only (raw_params = 0, MSGS_ERR_INVALID_ARG otherwise); exactly one of (scales, rotations) /
 * cov3D_precomp; shs, colours and the pixel-size inputs of `g`, and bg / projmatrix / campos of `view`, are not read.
 * P == 0: nothing is launched (dL_dV, when given, is zero-filled). */
size_t msgs_screen_compensation_scratch_bytes(int32_t P);
int msgs_screen_compensation_forward(const msgs_view_t* view, const msgs_gaussians_t* g, float* o_eff, void* stream);
int msgs_screen_compensation_backward(const msgs_view_t* view, const msgs_gaussians_t* g, const float* dL_do_eff,
                                      float* dL_dopacity, float* dL_dmeans3D, float* dL_dscales, float* dL_drotations,
                                      float* dL_dcov3D, float* dL_dV, void* scratch, size_t scratch_bytes, void* stream);

/* ---- 3-D smoothing filter of Mip-Splatting: camera sweep and filtered getters (DESIGN.md SPEC M16, 4.17) ------------------- */
/* The 3-D filter bounds the size of every Gaussian from below by the highest sampling rate nu (pixels per world unit) at which
 * any camera of a set sees its centre.  `cameras` is a device table [n_cameras, MSGS_FILTER3D_CAMERA_FLOATS] float32, row n =
 * { M_n[16] (world_view_transform in the layout of msgs_view_t::viewmatrix), fx_n, fy_n, W_n, H_n }, fx = W / (2 tan(FoVx / 2)).
 * With t = the view-space centre (float32, the operations of msgs_forward*), zc = max(t.z, 0.001),
 * x = t.x / zc fx + W / 2, y = t.y / zc fy + H / 2, camera n SEES the centre iff
 *     t.z > 0.2   and   -0.15 W <= x <= 1.15 W   and   -0.15 H <= y <= 1.15 H       (a NaN / Inf anywhere: not seen)
 *     rule MSGS_FILTER3D_RULE_PER_CAMERA:     nu = max over the seeing cameras of fx_n / t.z          (the paper)
 *     rule MSGS_FILTER3D_RULE_MIP_SPLATTING:  nu = (max over ALL cameras of fx_n) / (min over the seeing cameras of t.z)
 *                                                                                                      (the published code)
 * msgs_filter3d_sweep writes valid [P] (one byte per Gaussian, 1 = some camera sees it) and filter_3D [P] float32 =
 * sqrt(variance) / nu; a Gaussian no camera sees takes the smallest nu of those that are seen (the largest filter); when none
 * is seen filter_3D is 0 everywhere, which the getters below read as "no filter".  Min and max only: the same bits on every run
 * and for every launch geometry.  scratch >= msgs_filter3d_scratch_bytes(P, n_cameras), 4-byte aligned; everything on `stream`,
 * no synchronisation.  P == 0: nothing is launched.
 *
 * The filtered getters, for f = filter_3D, s the scales [P,3] and o the opacities [P]:
 *     s_eff_k = sqrt(s_k^2 + f^2),   o_eff = o r_0 r_1 r_2,   r_k = s_k / s_eff_k      (= o sqrt(det S^2 / det(S^2 + f^2 I)))
 * A filtered render IS the plain render of the same model with (s_eff, o_eff) in the place of (s, o).  A row with f == 0 passes
 * s and o through bit for bit; s_k == 0 with f > 0 gives s_eff_k = f, o_eff = 0 and finite gradients.  raw != 0: `scales` are
 * log-scales and `opacities` logits, activated here with the expressions of msgs_gaussians_t::raw_params == 1, and the backward
 * returns the gradients of those raw values.  msgs_smoothing_filter_backward writes every row of dL_dscales [P,3] and
 * dL_dopacities [P]; one of dL_dscales_eff / dL_dopacities_eff may be NULL (that output did not enter the loss: zeros). */
#define MSGS_FILTER3D_CAMERA_FLOATS 20
#define MSGS_FILTER3D_CAMERA_CHUNK 64          /* camera rows staged per pass of the sweep (tests straddle it) */
#define MSGS_FILTER3D_RULE_PER_CAMERA 0
#define MSGS_FILTER3D_RULE_MIP_SPLATTING 1
size_t msgs_filter3d_scratch_bytes(int32_t P, int32_t n_cameras);
int msgs_filter3d_sweep(int32_t P, const float* means3D, int32_t n_cameras, const float* cameras, int32_t rule, float variance,
                        float* filter_3D, uint8_t* valid, void* scratch, size_t scratch_bytes, void* stream);
int msgs_smoothing_filter_forward(int32_t P, int32_t raw, const float* scales, const float* opacities, const float* filter_3D,
                                  float* scales_eff, float* opacities_eff, void* stream);
int msgs_smoothing_filter_backward(int32_t P, int32_t raw, const float* scales, const float* opacities, const float* filter_3D,
                                   const float* dL_dscales_eff, const float* dL_dopacities_eff, float* dL_dscales,
                                   float* dL_dopacities, void* stream);

/* ---- normal maps: Gaussian normals and depth-to-normal (DESIGN.md SPEC M17, 4.18) ------------------------------------------ */
/* msgs_gaussian_normals_forward: normals [P,3] float32, the shortest axis of every Gaussian turned towards the camera.
 *     k = 0; if s_1 < s_k: k = 1; if s_2 < s_k: k = 2        (strict; comparisons only: log-scales, activated and filtered
 *                                                             scales select the same axis)
 *     q = r / max(||r||, 1e-12),   n = column k of R(q)      (the R of Sigma = R S^2 R^T; raw or normalised quaternions)
 *     sigma = -1 iff n . (campos - p) < 0, else +1
 *     world != 0: sigma n;   world == 0: the view-space vector sigma sum_j n_j viewmatrix[4 j + c]
 * viewmatrix [16] (the layout of msgs_view_t::viewmatrix) and campos [3] are DEVICE pointers.  A row with a non-finite input or
 * result is exactly (0, 0, 0).  flags [P] (one byte per row: k, the sign, valid) is all the backward keeps.
 * msgs_gaussian_normals_backward writes every row of dL_drotations [P,4]: through column k of R and through the normalisation
 * (no gradient through the norm where its clamp is active); k, sigma and the camera are constants, an invalid row gets zeros.
 * means3D and scales have no gradient.
 *
 * msgs_depth_normal_forward: normal [3,H,W] float32 from a map depth [H,W] of view depths.  Pixel (x, y) back-projects to
 * P = (a_x z, a_y z, z), a_x = ((2 x + 1) / W - 1) tanfovx, a_y likewise; u = P(x, y+1) - P(x, y-1), v = P(x+1, y) - P(x-1, y),
 * c = u x v, n = c / ||c|| (a fronto-parallel plane: (0, 0, -1)).  Valid iff 1 <= x <= W-2, 1 <= y <= H-2, the four depths are
 * finite and > 0 and ||c||^2 is finite and > 0; every other pixel is exactly 0.  world != 0: rotated into world space,
 * w_j = sum_k viewmatrix[4 j + k] n_k (viewmatrix: DEVICE pointer, may be NULL with world == 0).
 * msgs_depth_normal_backward writes every pixel of dL_ddepth [H,W]: a gather, in a fixed order, of the shares of the (up to
 * four) valid stencils a pixel belongs to; no atomics, the same bits on every run.  The camera is a constant.
 * All four: everything on `stream`, no synchronisation; P == 0 / W H == 0: nothing is launched. */
#define MSGS_DEPTH_NORMAL_TILE_W 64            /* the tile of the depth-to-normal kernels (tests place seams from these) */
#define MSGS_DEPTH_NORMAL_TILE_H 8
int msgs_gaussian_normals_forward(int32_t P, const float* means3D, const float* scales, const float* rotations,
                                  const float* viewmatrix, const float* campos, int32_t world, float* normals, uint8_t* flags,
                                  void* stream);
int msgs_gaussian_normals_backward(int32_t P, const float* rotations, const uint8_t* flags, const float* viewmatrix,
                                   int32_t world, const float* dL_dnormals, float* dL_drotations, void* stream);
int msgs_depth_normal_forward(int32_t W, int32_t H, float tanfovx, float tanfovy, const float* depth, const float* viewmatrix,
                              int32_t world, float* normal, void* stream);
int msgs_depth_normal_backward(int32_t W, int32_t H, float tanfovx, float tanfovy, const float* depth, const float* viewmatrix,
                               int32_t world, const float* dL_dnormal, float* dL_ddepth, void* stream);

/* msgs_backward_per_gaussian: the per-Gaussian half of msgs_backward ALONE (2-D covariance backward, projection, SH,
 * scale / quaternion chain — upstream's computeCov2DCUDA + preprocessCUDA backward, SURVEY 2.2 K8 + K9) on per-Gaussian
 * 2-D gradients supplied by the caller instead of the blend backward's sums: sums2d [P,9] DOUBLES (device) =
 * {dL/dmean2D x, y (the NDC-ish units of dL_dmeans2D), dL/dconic A, B, C, dL/d(effective opacity), dL/drgb[3]}, rounded to
 * float once like the library's own records.  `geom` and `radii` are those of the forward of the same view.  For the
 * parity tests: fed the oracle's sums, the two per-Gaussian stages are compared on bit-identical inputs
 * (tests/test_k8_isolation_gpu.py); also usable by a caller that blends elsewhere.  Reference-API inputs only
 * (raw_params = 0); grads->accumulate / wait_before_accumulate / accumulated must be zero / NULL (MSGS_ERR_INVALID_ARG
 * otherwise: accumulation across views is msgs_backward's contract). */
int msgs_backward_per_gaussian(const msgs_view_t* view, const msgs_gaussians_t* g, const int32_t* radii,
                               const void* geom, size_t geom_bytes, const double* sums2d, const msgs_grads_t* grads,
                               void* stream);

/* ---- view-parallel gradient exchange (new relative to the single-GPU reference) -------------------
 * The SH part of one view's gradient (48 of the 59 floats per Gaussian) is the outer product of the 16 SH basis values
 * of the viewing direction and the 3 floats dL/drgb: msgs_backward delivers just dL/drgb (msgs_grads_t.dL_dcolors in
 * the raw modes), the ranks all-gather those [P,3] factors and every rank rebuilds
 *     dL/dfeatures_{dc,rest}[i] = scale * sum_v basis(normalize(means3D[i] - campos[v])) x drgb[v][i]
 * with the products msgs_backward itself would have formed (bit-identical per view), added in view order.
 * View v's camera centre is campos + v * campos_stride (3 floats), its factors drgb + v * drgb_stride ([P,3] floats,
 * zeros where the view did not render the Gaussian) — strides in floats, so the rows of one all-gathered buffer
 * {factors | camera centre} can be read in place.  Outputs are fully written. */
int msgs_sh_grad_from_views(int32_t P, int32_t n_views, int32_t sh_degree, const float* means3D, const float* campos,
                            int64_t campos_stride, const float* drgb, int64_t drgb_stride, float scale,
                            float* dL_dfeatures_dc, float* dL_dfeatures_rest, void* stream);

/* ---- optional -------------------------------------------------------------------------------- */
/* visibility mask only (upstream markVisible; present[P] uint8) */
int msgs_mark_visible(int32_t P, const float* means3D, const float* viewmatrix,
                      const float* projmatrix, uint8_t* present, void* stream);

/* Statistics of the last-built binning (for the algorithmic-bytes formula of DESIGN.md):
 * out_host[0] = sum over tiles of max-over-pixels last contributor (D_trav),
 * out_host[1] = number of Gaussians with radii > 0 (V).  Synchronises `stream`. */
int msgs_binning_stats(const msgs_view_t* view, int32_t P, const int32_t* radii,
                       const void* binning, size_t binning_bytes,
                       const void* image_state, size_t image_bytes,
                       void* scratch, size_t scratch_bytes,
                       int64_t* out_host, void* stream);

/* Diagnostic: lane efficiency of the blend kernels.  Replays the quadrant-list blend forward and — when
 * image_state is given — the one-wave-per-tile backward on the state a forward left behind (nothing is written to geom / binning /
 * image or to any output) with scalar counters:
 *   out_host[0] = forward (wave, entry) evaluations — each evaluates 64 lanes; [1] = lanes still blending summed over them;
 *   [2] = lanes that blended (alpha >= 1/255, power <= 0, before termination);
 *   [3] = backward (tile, entry) visits; [4] = backward (quadrant, entry) evaluations — each 64 lanes; [5] = lanes that
 *   contributed a gradient; [6] = visits with at least one contributing lane (= reductions + atomic instructions); -1 each
 *   without image_state.  out_host holds 7 values; scratch >= 64 bytes.  Synchronises `stream`. */
int msgs_blend_lane_stats(const msgs_view_t* view, const void* geom, size_t geom_bytes, int32_t P, int64_t D,
                          const void* binning, size_t binning_bytes, const void* image_state, size_t image_bytes,
                          void* scratch, size_t scratch_bytes, int64_t* out_host, void* stream);

/* Deterministic (verification) mode (process-wide switch; initial value from the environment variable
 * MSGS_DETERMINISTIC=1).  The forward is always bitwise reproducible.  The default backward adds the float32 sum each
 * tile delivers for a Gaussian into DOUBLE accumulators with float64 atomics: the sums are exact, so the result does not
 * depend on the order the atomics arrive in (reproducible in practice: a double total can move by 1e-16, which changes the
 * rounded float about once in 1e9 values).  With the switch on, msgs_backward accumulates the per-pixel float32 factors in
 * double inside the tile as well, stores the nine sums of every tile entry, groups them by Gaussian with a stable sort and
 * adds them in ascending tile order: reproducible by construction and the accumulation structure of the CPU oracle; about
 * 1.4 ms slower at C3, and the scratch buffer must hold msgs_backward_scratch_bytes_deterministic(P, D) bytes.
 * msgs_set_deterministic returns the previous value. */
int msgs_set_deterministic(int32_t on);
int msgs_get_deterministic(void);
size_t msgs_backward_scratch_bytes_deterministic(int32_t P, int64_t D);
/* the same for msgs_backward_with_depth with a non-NULL dL_ddepth (ten sums per tile entry instead of nine) */
size_t msgs_backward_scratch_bytes_deterministic_depth(int32_t P, int64_t D);

/* Which of the two blend-backward kernels msgs_backward launches: 0 (default) = by tile count (one wave per tile from
 * 4096 tiles up, four waves per tile below), 1 | 2 = force one — for the parity tests and A/B measurements.  Initial
 * value from MSGS_BWD_GEN.  Returns the previous value. */
int msgs_set_backward_generation(int32_t gen);

/* Pixel granularity of the blend kernels' workgroups: 0 (default) = by tile count, 1 = always one wave64 per 8x8 pixel
 * quadrant (forward) / per quadrant or tile (backward, see above), 2 = always the fine-grained kernels — sixteen waves
 * per 16x16 tile, one per 4x4 pixel sub-block — which the default picks below 300 tiles (the low levels of the
 * resolution pyramid MS-GS trains on, utils/camera_utils.py:38-39), where the blend kernels are latency-bound and a
 * shorter per-wave entry list matters more than idle lanes.  Same per-pixel arithmetic in the same order: forward
 * results are bit-identical across granularities.  2 overrides msgs_set_backward_generation.  Initial value from
 * MSGS_BLEND_GRANULARITY.  Returns the previous value. */
int msgs_set_blend_granularity(int32_t mode);

/* Exact per-tile occlusion cut-off (round 5; process-wide switch, on by default, initial value off with MSGS_NO_OCCLUSION=1).
 * Between the per-Gaussian stage and the depth sort the forward finds, per block of tiles, the view depth behind which every
 * pixel of the block has provably met the reference's termination rule T (1 - alpha) < 1e-4 — from the Gaussians whose
 * alpha >= 1/255 level set contains the whole block, their smallest alpha over it, and the product of (1 - alpha_min) front to
 * back with a factor 2 of slack — and neither counts, emits nor sorts the tile instances behind it.  The lists the pixels
 * walk are unchanged entry for entry: every output and gradient is bit-identical to the uncut path; only the instance count D
 * shrinks (the multi-scale model rendered without its filters, /root/reference/render.py:32: 427 M -> a few million at
 * 1080p).  One launch (a persistent grid, four phases behind grid barriers); a view without cover candidates leaves it after
 * the first barrier (~5 us), so the pass runs on EVERY forward while the switch is on.  msgs_set_occlusion returns the
 * previous value.
 * msgs_occlusion_stats reads what the pass did for the forward that last wrote `geom`: out_host[8] = {ran (0 / 1; 2 = a barrier
 * wait of the pass expired: the cut is valid but weaker — never observed), Gaussians
 * with more than 96 tile instances, cover candidates kept from them (the nearest by depth, at most 32 768), cover blocks that received a cut-off,
 * cover blocks of the view, tiles per side of a cover block, smallest and largest cut-off (float32 bits of a view depth;
 * 0xFFFFFFFF = a block stayed open)}.  (The instances removed = the instance count of the same view with the pass switched
 * off minus the one with it on.)  Synchronises `stream`; not re-entrant (a diagnostic). */
int msgs_set_occlusion(int32_t on);
/* Which depth sort the forward runs (process-wide switch; both give the same arrays bit for bit, ties in index order):
 * 0 (default) = by P — up to 1.5 M Gaussians the bucket path (a histogram of the keys over fine depth bins balances 255 buckets,
 * one compacting pass distributes the keys, one workgroup per bucket finishes it in LDS: five launches), above that the four
 * 8-bit LSD passes (eight launches); 1 = always the LSD passes; 2 = the bucket path for every P it can run at (up to 2 097 152).
 * The choice never depends on device data.  Initial value from MSGS_DEPTH_SORT.  Returns the previous value.
 * msgs_depth_sort_stats reads what the sort did for the forward that last wrote `geom`: out_host[3] = {1 when the bucket path
 * ran, buckets that outgrew one workgroup's LDS (8192 pairs) and were sorted in chunks through HBM — correct, only slow; it
 * takes thousands of Gaussians within 1/512 octave of depth —, V = Gaussians that stayed in the sort}.  Synchronises `stream`. */
int msgs_set_depth_sort(int32_t mode);
int msgs_depth_sort_stats(const void* geom, size_t geom_bytes, int32_t P, int64_t* out_host, void* stream);
/* What the last forward that RETURNED ITS INSTANCE COUNT on the calling host thread (msgs_forward, msgs_forward_stage1,
 * msgs_forward_finish) learned besides the count — the words travel with it, no extra device access: out_host[0] = cover
 * candidates of its occlusion pass (0 when the pass did not run), out_host[1] = 1 when the pass closed at least one block.
 * out_host[2..7] = the most recent FEEDBACK publication that has landed in the status block of that forward (the thread's, or
 * the msgs_status_t handle's) — normally that of an EARLIER forward, its stage 2 having finished since:
 *   [2] its msgs_view_t.feedback_tag (0: none yet), [3] its instance count D, [4] its D_trav, [5] tiles left open by slab A
 *   (-1: it ran single-pass), [6] instances of slab A, [7] instances slab B emitted.  out_host holds 8 values. */
int msgs_forward_info(int64_t* out_host);
int msgs_occlusion_stats(const void* geom, size_t geom_bytes, int32_t P, int64_t* out_host, void* stream);
/* Diagnostic: what depth-slab binning did for the forward that last wrote `geom`: out_host[6] = {ran in slab mode (0 / 1), depth
 * ranks in slab A, instances of slab A, tiles slab A left open, instances slab B emitted, overflow flag (always 0)}.
 * Synchronises `stream`. */
int msgs_slab_stats(const void* geom, size_t geom_bytes, int32_t P, int64_t* out_host, void* stream);

/* msgs_forward: both stages in ONE call.  The caller passes `binning` and `scratch2` sized for a GUESS of the instance count
 * (the previous frame's D plus a margin).  Stage 1 is launched, stage 2 is launched right behind it on those buffers — sized for
 * their capacity, the kernels read min(D, capacity) from a device word the scan writes — and only then the host waits for D (one
 * poll of pinned host words): the GPU never idles while the host learns D.  D <= capacity (the normal case): *stage2_done = 1.
 * Otherwise (first frame of a shape, or the scene outgrew the margin) *stage2_done = 0 and *num_instances_host = D: grow the
 * buffers and call msgs_forward_stage2, which overwrites the truncated result (same stream).  The binning buffer's internal
 * layout depends neither on D nor on the capacity (tile ranges first).  view->debug, an empty view, buffers below 4096
 * instances and the look-back sort variants take the sequential route (wait for D, then launch stage 2 if the buffers
 * suffice). */
int msgs_forward(const msgs_view_t* view, const msgs_gaussians_t* gaussians, int32_t* radii, float* pixel_sizes,
                 void* geom, size_t geom_bytes, void* scratch1, size_t scratch1_bytes, void* binning,
                 size_t binning_bytes, void* scratch2, size_t scratch2_bytes, void* image, size_t image_bytes,
                 float* out_color, float* out_acc_pixel_size, float* out_depth, void* grad_records,
                 size_t grad_records_bytes, int32_t backward_follows, int64_t* num_instances_host, int32_t* stage2_done,
                 const msgs_timing_t* timing, void* stream);

/* ---- forward without the host wait: several views in flight from one host thread -------------------------------------
 * msgs_forward splits into msgs_forward_launch (everything msgs_forward enqueues: stage 1 and — on capacity-sized buffers
 * — stage 2, nothing waited for) and msgs_forward_finish (the wait for the instance count).  Between the two the caller
 * may launch other forwards (each on its own msgs_status_t and its own buffers, on the same or on other streams) and
 * backwards of finished views: the reference's multi-view loops (/root/reference/train.py:282-299,337-341 insertion sweeps,
 * :488-496 evaluation, render.py:37-49, render_traj.py:99-105) and the views of one optimizer step are independent, so two
 * views on two streams let the instruction-bound blend kernels of one run beside the HBM- / latency-bound kernels of the
 * other.  A handle owns one 64-byte pinned status block; create it once and reuse it launch after launch.
 * msgs_forward_finish: *stage2_done = 1 when stage 2 ran on the launch's buffers (D <= their capacity); 0 when the caller
 * has to call msgs_forward_stage2 on buffers sized for *num_instances_host (no guess yet, debug mode, or the scene outgrew
 * the guess) on the same stream — exactly msgs_forward's contract.  Every buffer passed to the launch stays owned by the
 * caller and must outlive the work enqueued on `stream`. */
typedef struct msgs_status msgs_status_t;
int msgs_status_create(msgs_status_t** out);
int msgs_status_destroy(msgs_status_t* status);
int msgs_forward_launch(const msgs_view_t* view, const msgs_gaussians_t* gaussians, int32_t* radii, float* pixel_sizes,
                        void* geom, size_t geom_bytes, void* scratch1, size_t scratch1_bytes, void* binning,
                        size_t binning_bytes, void* scratch2, size_t scratch2_bytes, void* image, size_t image_bytes,
                        float* out_color, float* out_acc_pixel_size, float* out_depth, void* grad_records,
                        size_t grad_records_bytes, int32_t backward_follows, msgs_status_t* status,
                        const msgs_timing_t* timing, void* stream);
int msgs_forward_finish(msgs_status_t* status, int64_t* num_instances_host, int32_t* stage2_done);

/* msgs_preprocess_only: the per-Gaussian stage alone (frustum cull, multi-scale filters, projection) — radii and
 * pixel_sizes exactly as msgs_forward_stage1 writes them, without sorting, binning or blending.  For the camera
 * sweeps of the reference that render a view only to read visibility_filter / pixel_sizes
 * (/root/reference/train.py:283-300 before insert_large_gaussians, :334-338 after it).  No host synchronisation. */
int msgs_preprocess_only(const msgs_view_t* view, const msgs_gaussians_t* gaussians, int32_t* radii,
                         float* pixel_sizes, void* geom, size_t geom_bytes, void* stream);

/* ---- voxel-average pooling (large-Gaussian insertion) ------------------------------------------------------
 * GPU replacement for the eleven CPU calls of open3d.ml.torch.layers.VoxelPooling(position_fn='center',
 * feature_fn='average') in /root/reference/scene/gaussian_model.py:802-816 (third-party, un-vendored; restated
 * from its published behaviour: voxel = floor(p / voxel_size), features = mean over the voxel's points).
 * Build the grouping once per position set, then average any number of [M,F] feature tensors with it.
 *   order[M]          point ids grouped by voxel (voxels ascending in (z,y,x) voxel index, points ascending by id)
 *   seg_start[M+1]    first num_voxels+1 entries valid: voxel v owns order[seg_start[v] .. seg_start[v+1])
 *   voxel_index[M,3]  (nullable) integer voxel coordinates, first num_voxels rows valid
 * msgs_voxel_pool_build synchronises the stream once to return num_voxels. */
size_t msgs_voxel_pool_scratch_bytes(int64_t M);
int msgs_voxel_pool_build(const float* positions, int64_t M, float voxel_size, uint32_t* order, uint32_t* seg_start,
                          int32_t* voxel_index, void* scratch, size_t scratch_bytes, int64_t* num_voxels_host,
                          void* stream);
int msgs_voxel_pool_average(const float* features, int32_t F, const uint32_t* order, const uint32_t* seg_start,
                            int64_t num_voxels, float* out, void* stream);

/* ---- train-step epilogue ------------------------------------------------------------------
 * msgs_adam_step replaces torch.optim.Adam(l, lr=0.0, eps=1e-15).step() over the model's leaf tensors
 * (/root/reference/scene/gaussian_model.py:235-248, /root/reference/train.py:416-418) with ONE launch; the state
 * tensors are the optimizer's own state["exp_avg"], state["exp_avg_sq"] (the reference's densification code slices
 * and concatenates them: gaussian_model.py:419-476), `step` is the 1-based step count after increment, `lr` the
 * group's current learning rate.  Semantics: torch Adam with amsgrad=False, weight_decay=0, maximize=False. */
#define MSGS_ADAM_MAX_TENSORS 8
typedef struct msgs_adam_tensor {
    float* param;            /* [n] updated in place */
    const float* grad;       /* [n] */
    float* exp_avg;          /* [n] updated in place */
    float* exp_avg_sq;       /* [n] updated in place */
    int64_t n;               /* number of floats */
    double lr;               /* double like the Python float in param_group["lr"]: scalars are rounded to float once */
} msgs_adam_tensor_t;
int msgs_adam_step(const msgs_adam_tensor_t* tensors, int32_t n_tensors, int64_t step, double beta1, double beta2,
                   double eps, void* stream);

/* msgs_densify_stats: every per-Gaussian statistic the reference updates between backward() and optimizer.step(),
 * in one launch, all masked by visibility_filter = radii > 0 (/root/reference/train.py:239-250):
 *   MSGS_STATS_BASE_MASK    base_mask |= visible                         (gaussian_model.py:702-704)
 *   MSGS_STATS_PIXEL_SIZES  update_pixel_sizes(visible, pixel_sizes, reso_lvl)   (gaussian_model.py:663-687)
 *   MSGS_STATS_DENSIFY      max_radii2D = max(max_radii2D, radii); xyz_gradient_accum[:, reso_lvl] += |grad_xy|;
 *                           denom[:, reso_lvl] += 1                      (train.py:247-250, gaussian_model.py:698-701)
 * Pointers of a group that is not selected may be NULL. */
#define MSGS_STATS_BASE_MASK 1
#define MSGS_STATS_PIXEL_SIZES 2
#define MSGS_STATS_DENSIFY 4
typedef struct msgs_densify_stats {
    int32_t P;
    int32_t flags;
    int32_t reso_lvl;                /* resolution level trained this iteration (train.py reso_idx) */
    int32_t reso_lvls;               /* number of levels (second dim of xyz_gradient_accum / denom) */
    const int32_t* radii;            /* [P] output of the forward */
    const float* pixel_sizes;        /* [P] output of the forward */
    const float* means2D_grad;       /* [P,3] viewspace_points.grad */
    const int64_t* target_reso_lvl;  /* [P] torch.long, gaussian_model.py:227 */
    float* xyz_gradient_accum;       /* [P, reso_lvls, 1] */
    float* denom;                    /* [P, reso_lvls, 1] */
    float* max_radii2D;              /* [P] */
    float* max_pixel_sizes;          /* [P] */
    float* min_pixel_sizes;          /* [P] */
    uint8_t* base_mask;              /* [P] torch.bool */
} msgs_densify_stats_t;
int msgs_densify_stats(const msgs_densify_stats_t* stats, void* stream);

/* ---- model surgery: clone, split, prune, grow, append (densification mechanism) ---------------------------------
 * The reference's GaussianModel.densify_and_prune / grow_large_gaussians / prune_points / densification_postfix
 * (/root/reference/scene/gaussian_model.py:452-537,599-662) as two calls over every per-Gaussian tensor (DESIGN.md SPEC D1):
 *   msgs_densify_select  one thread per source row decides its fate (kept, cloned, split, children kept, grown), clears
 *                        column reso_lvl of xyz_gradient_accum / denom IN PLACE as the reference does, and builds the row
 *                        map of the output in `scratch` (stable placement, no atomics).  Reads the segment sizes back:
 *                        the call's only host synchronisation.
 *                        counts_host[8] = { kept, clones kept, children kept (per child), split, grown, appended, P_out, 0 }
 *   msgs_densify_apply   one launch writes every output tensor from the map, with one rule per tensor and row kind.
 * Output rows: kept source rows, then clones, first children, second children, grown rows, appended rows (each in source
 * order).  Thresholds are float32 (the rounding torch applies to a Python float compared with a float32 tensor). */
#define MSGS_DENSIFY_PRUNE 0        /* densify_and_prune: clone + split + prune                         */
#define MSGS_DENSIFY_GROW 1         /* grow_large_gaussians                                             */
#define MSGS_DENSIFY_PRUNE_MASK 2   /* prune_points(mask)                                               */
#define MSGS_DENSIFY_APPEND 3       /* densification_postfix                                            */
typedef struct msgs_densify_select {
    int32_t mode;                    /* MSGS_DENSIFY_* */
    int32_t reso_lvl;                /* column of accum / denom read (GROW) and cleared (PRUNE: 0, GROW, APPEND) */
    int32_t reso_lvls;               /* L: second dim of accum / denom */
    int32_t has_max_screen_size;     /* PRUNE: `if max_screen_size:` of the reference */
    int64_t P;                       /* source rows */
    int64_t n_append;                /* APPEND: rows appended */
    float grad_threshold;            /* PRUNE: max_grad; GROW: grad_threshold */
    float min_opacity;               /* PRUNE */
    float scale_limit;               /* PRUNE: percent_dense * extent */
    float big_world_limit;           /* PRUNE: 0.1 * extent */
    float max_screen_size;           /* PRUNE, when has_max_screen_size */
    int32_t reserved;
    const float* opacity;            /* [P] logits (PRUNE) */
    const float* scaling;            /* [P,3] log scales (PRUNE) */
    float* xyz_gradient_accum;       /* [P,L,1] (PRUNE, GROW, APPEND) */
    float* denom;                    /* [P,L,1] (PRUNE, GROW, APPEND) */
    const int64_t* target_reso_lvl;  /* [P] (PRUNE) */
    const uint8_t* prune_mask;       /* [P] bool, true = remove (PRUNE_MASK) */
} msgs_densify_select_t;
size_t msgs_densify_scratch_bytes(int64_t P, int64_t n_append);
int msgs_densify_select(const msgs_densify_select_t* sel, void* scratch, size_t scratch_bytes, int64_t* counts_host,
                        void* stream);

/* rules of msgs_densify_tensor_t.rule[kind], kind = 0 kept, 1 clone, 2 first child, 3 second child, 4 grown, 5 appended */
#define MSGS_DR_COPY 0               /* the source row */
#define MSGS_DR_ZERO 1               /* zeros (false for bool) */
#define MSGS_DR_COPY_CLEAR_COL 2     /* the source row with element reso_lvl zeroed (accum / denom) */
#define MSGS_DR_SPLIT_XYZ 3          /* R(q) (z * exp(s)) + xyz, z = draws row (split ordinal, + n_split for the 2nd child) */
#define MSGS_DR_SPLIT_SCALE 4        /* log(exp(s) / 1.6) */
#define MSGS_DR_SPLIT_DIV 5          /* x / 1.6 */
#define MSGS_DR_GROW_OPACITY 6       /* inverse_sigmoid(sigmoid(o) / 2) */
#define MSGS_DR_GROW_SCALE 7         /* log(exp(s) * 2) */
#define MSGS_DR_GROW_MUL 8           /* x * 2 */
#define MSGS_DR_CONST 9              /* `constant` (int64 tensors) */
#define MSGS_DR_APPEND 10            /* row of append_src */
#define MSGS_DENSIFY_MAX_TENSORS 32
typedef struct msgs_densify_tensor {
    void* dst;                       /* [P_out, width] */
    const void* src;                 /* [P, width] */
    const void* append_src;          /* [n_append, width] (MSGS_DR_APPEND) */
    int64_t constant;                /* MSGS_DR_CONST */
    int32_t width;                   /* elements per row */
    int32_t elem_bytes;              /* 4 float32, 8 int64, 1 bool */
    uint8_t rule[8];                 /* per row kind (6 used) */
} msgs_densify_tensor_t;
typedef struct msgs_densify_apply {
    int64_t P;                       /* as in the select call that filled `scratch` */
    int64_t n_append;                /* as in the select call */
    int64_t P_out;                   /* counts_host[6] of the select call */
    int64_t n_split;                 /* counts_host[3] */
    int32_t n_tensors;
    int32_t reso_lvl;                /* column zeroed by MSGS_DR_COPY_CLEAR_COL */
    const float* xyz;                /* [P,3] sources of MSGS_DR_SPLIT_XYZ */
    const float* scaling;            /* [P,3] */
    const float* rotation;           /* [P,4] */
    const float* draws;              /* [2*n_split, 3] standard normal draws */
    const msgs_densify_tensor_t* tensors;
} msgs_densify_apply_t;
int msgs_densify_apply(const msgs_densify_apply_t* apply, const void* scratch, size_t scratch_bytes, void* stream);

/* ---- MCMC densification: sampling, relocation, capped growth, position noise (DESIGN.md SPEC M18, 4.19) -----------------
 * The model surgery of "3D Gaussian Splatting as Markov Chain Monte Carlo" for a trainer with a fixed budget of Gaussians.
 *
 * Sampling.  w_i = sigmoid(opacity_i) in double, 0 where dead[i] (dead may be NULL) or the logit is NaN; the CDF is the inclusive
 * prefix sum of w in double, summed in one fixed order, monotone, and exactly flat over rows of weight 0.  Draw j takes the first
 * row whose CDF exceeds u_j * total (u float64 in [0,1)); a product that rounds up to the total takes the last row of positive
 * weight.  A row of weight 0 is never taken; the same inputs give the same bits on every run.
 *   msgs_mcmc_prepare   builds the CDF and the stable list of dead rows in `scratch` and reads back
 *                       counts_host[4] = { dead rows, rows of positive weight, 0, 0 }: the call's only host synchronisation.
 *   msgs_mcmc_sample    prepare + draw: source[n] int32 (row of each draw), count[P] int32 (draws per row).  n == 0 launches
 *                       nothing; no row of positive weight: MSGS_ERR_NO_WEIGHT, source and count are not written.
 *
 * Relocation rule, for a row drawn count times, N = min(count + 1, MSGS_MCMC_N_MAX), logit x, log-scales s, in double:
 *     log(1 - o) = -softplus(x),  o_new = -expm1(log(1 - o) / N),
 *     D = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k / sqrt(k+1) o_new^(k+1),  c = o / D,
 *     s_new = s + log c (all three axes),  x_new = logit(clamp(o_new, 0.005, 1 - 2^-24)) = log o_new - log(1 - o) / N unclamped.
 *
 *   msgs_mcmc_relocate  after msgs_mcmc_prepare on the same scratch and the same opacity: draws n rows with u [n], computes
 *                       (x_new, s_new, c) of every drawn row from its old values into scratch, then writes
 *                         in_place != 0: dead row number j (row order) <- draw j; n must be the number of dead rows
 *                         in_place == 0: row j of every tensor's `fresh` block <- draw j (tensors with fresh == NULL: skipped)
 *                       by each tensor's rule, and every drawn row itself: x_new, s_new, pixel sizes * c, and zeros in its rows of
 *                       exp_avg / exp_avg_sq wherever a tensor carries them.  Rows neither written nor drawn are not touched.
 *                       No host synchronisation.  n <= P.
 *
 *   msgs_mcmc_noise     xyz += R S^2 R^T xi * gain / (1 + exp(-100 (0.005 - sigmoid(opacity)))) in place, float32; S = exp(scaling),
 *                       R the rotation of rotation / max(|rotation|, 1e-12) as msgs_forward* forms it, xi = draws [P,3],
 *                       gain = noise_lr * xyz_lr.  One streaming launch, no synchronisation. */
#define MSGS_MCMC_N_MAX 51
#define MSGS_MCMC_MAX_TENSORS 16
#define MSGS_MR_COPY 0               /* the source's row                              */
#define MSGS_MR_ZERO 1               /* zeros (false for bool)                        */
#define MSGS_MR_OPACITY 2            /* x_new of the source            (width 1)      */
#define MSGS_MR_SCALE 3              /* s_new of the source            (width 3)      */
#define MSGS_MR_PIX_MAX 4            /* the source's max_pixel_sizes * c (width 1)    */
#define MSGS_MR_PIX_MIN 5            /* the source's min_pixel_sizes * c (width 1)    */
typedef struct msgs_mcmc_tensor {
    void* data;                      /* [P, width] the model's tensor: source rows are read; written rows when in place */
    void* fresh;                     /* [n, width] the new rows when not in place, or NULL */
    float* exp_avg;                  /* [P, width] optimizer moments zeroed in drawn rows, or NULL */
    float* exp_avg_sq;
    int32_t width;                   /* elements per row */
    int32_t elem_bytes;              /* 4 float32, 8 int64, 1 bool (COPY and ZERO only) */
    int32_t rule;                    /* MSGS_MR_*; exactly one OPACITY and one SCALE tensor */
    int32_t reserved;
} msgs_mcmc_tensor_t;
typedef struct msgs_mcmc_relocate {
    int64_t P;
    int64_t n;                       /* draws */
    int32_t in_place;
    int32_t n_tensors;
    const double* u;                 /* [n] uniforms in [0,1) */
    const msgs_mcmc_tensor_t* tensors;
} msgs_mcmc_relocate_t;
size_t msgs_mcmc_scratch_bytes(int64_t P);
int msgs_mcmc_prepare(int64_t P, const float* opacity, const uint8_t* dead, void* scratch, size_t scratch_bytes,
                      int64_t* counts_host, void* stream);
int msgs_mcmc_sample(int64_t P, const float* opacity, const uint8_t* dead, int64_t n, const double* u, int32_t* source,
                     int32_t* count, void* scratch, size_t scratch_bytes, void* stream);
int msgs_mcmc_relocate(const msgs_mcmc_relocate_t* r, void* scratch, size_t scratch_bytes, void* stream);
int msgs_mcmc_noise(int64_t P, float* xyz, const float* scaling, const float* rotation, const float* opacity,
                    const float* draws, float gain, void* stream);

/* ---- bilateral-grid colour correction (DESIGN.md SPEC M19, 4.20) -------------------------------------------------------------
 * A per-image grid [12,GL,GY,GX] float32 of 3x4 affine colour transforms (channel 4 c + j = entry (c, j)) over (x, y, guide),
 * sliced per pixel of image [3,H,W] float32 with trilinear interpolation:
 *     fx = (x + 0.5) / W (GX - 1),  fy = (y + 0.5) / H (GY - 1),  z = 0.299 r + 0.587 g + 0.114 b,  fz = clamp(z, 0, 1) (GL - 1)
 *     along an axis of size G > 1: cell k = min(floor(f), G - 2), weights 1 - t and t, t = f - k; size 1: coordinate 0, weight 1
 *     A = sum over the 8 corners of w grid[:, kz, ky, kx],   out_c = A[c,0] r + A[c,1] g + A[c,2] b + A[c,3]
 * (grid_sample, bilinear, border padding, align_corners).  1 <= GX, GY <= 256, 1 <= GL <= 32, W, H >= 1, W H < 2^29; anything
 * else returns MSGS_ERR_INVALID_ARG and launches nothing.  A non-finite pixel never indexes outside the grid; only its own
 * output, its own dL_dimage and the grid nodes it touches can carry its NaN.
 * msgs_bilagrid_slice_backward: `want` selects the halves (MSGS_BILAGRID_GRAD_IMAGE: dL_dimage [3,H,W], every pixel written;
 * MSGS_BILAGRID_GRAD_GRID: dL_dgrid [12,GL,GY,GX], every entry written); the pointer of a half that is not wanted is ignored.
 * dL_dimage is the direct term A[:, :3]^T dL_dout plus, where 0 < z < 1 (open at both ends), the guide term
 * (sum_c dL_dout_c dout_c/dfz) (GL - 1) (0.299, 0.587, 0.114).  dL_dgrid is summed in one fixed order without float atomics
 * (per wave, then per node over the slab of wave windows in `scratch`): the same bits on every run.  scratch (>=
 * msgs_bilagrid_scratch_bytes, 16-byte aligned, no clearing needed) is only used for the grid half.
 * msgs_bilagrid_tv_forward: tv [1] (device) = sum over the three spatial axes of the mean squared forward difference of the
 * bank grids [N,12,GL,GY,GX] along that axis (an axis of size 1 adds 0), summed in double in a fixed order; scratch >=
 * msgs_bilagrid_tv_scratch_bytes(N 12 GL GY GX), 8-byte aligned.  msgs_bilagrid_tv_backward: dL_dgrids = upstream * dtv/dgrids,
 * a gather; upstream is a DEVICE scalar (NULL = 1).  Everything on `stream`, no synchronisation. */
#define MSGS_BILAGRID_TILE_W 64            /* the pixel tile of the slice kernels (tests place seams from these) */
#define MSGS_BILAGRID_TILE_H 16
#define MSGS_BILAGRID_WINDOW_CELLS 16      /* xy grid nodes a tile's LDS window holds; larger windows read global memory */
#define MSGS_BILAGRID_MAX_XY 256
#define MSGS_BILAGRID_MAX_L 32
#define MSGS_BILAGRID_GRAD_IMAGE 1
#define MSGS_BILAGRID_GRAD_GRID 2
size_t msgs_bilagrid_scratch_bytes(int32_t W, int32_t H, int32_t GX, int32_t GY, int32_t GL);
int msgs_bilagrid_slice_forward(int32_t W, int32_t H, int32_t GX, int32_t GY, int32_t GL, const float* image,
                                const float* grid, float* out, void* stream);
int msgs_bilagrid_slice_backward(int32_t W, int32_t H, int32_t GX, int32_t GY, int32_t GL, const float* image,
                                 const float* grid, const float* dL_dout, int32_t want, float* dL_dimage, float* dL_dgrid,
                                 void* scratch, size_t scratch_bytes, void* stream);
size_t msgs_bilagrid_tv_scratch_bytes(int64_t n_elements);
int msgs_bilagrid_tv_forward(int64_t N, int32_t GX, int32_t GY, int32_t GL, const float* grids, float* tv, void* scratch,
                             size_t scratch_bytes, void* stream);
int msgs_bilagrid_tv_backward(int64_t N, int32_t GX, int32_t GY, int32_t GL, const float* grids, const float* upstream,
                              float* dL_dgrids, void* stream);

/* ---- TSDF fusion of depth maps and mesh extraction (DESIGN.md SPEC M20, 4.22) -------------------------------------------------
 * A block-sparse volume over the lattice p(i,j,k) = origin + voxel_size (i,j,k), 0 <= i,j,k < 8 nb: `table` [nb z, nb y, nb x] int32
 * holds the pool slot of every block of 8x8x8 lattice points (x fastest) or -1, `slot_block` [n_slots] int32 the linear table
 * index of every slot.  Per slot tsdf_sum [512] and weight_sum [512] float32, and colour_sum [3][512] (channel planes, so that a
 * wave reads and writes 256 contiguous bytes per plane) or NULL.  1 <= nb <= MSGS_TSDF_MAX_BLOCKS_PER_AXIS, n_slots <=
 * MSGS_TSDF_MAX_SLOTS; anything else returns MSGS_ERR_INVALID_ARG and launches nothing.
 * Frames: n rows of the camera table of msgs_filter3d_sweep (all of width W and height H), depth [n,H,W], colour [n,3,H,W] or
 * NULL, weight [n,H,W] or NULL (1), float32.  A pixel is a surface sample iff 0 < d <= depth_trunc and d is finite.
 *   msgs_tsdf_mark_blocks  writes 1 into marks [nb z nb y nb x] (bytes, cleared by the caller) for every block that holds one of
 *                          the points of a surface sample's ray at the view depths (d - r) + k (2 r / steps), k = 0..steps,
 *                          r = sdf_trunc + 2 voxel_size (depths <= 0 are left out); the view matrices must be rigid.
 *   msgs_tsdf_integrate    lattice point p, camera row M: t = p M, pixel (floor(t.x / t.z fx + W/2), floor(t.y / t.z fy + H/2));
 *                          skipped iff t.z <= 0, the pixel is outside, it is no surface sample, its weight is not positive and
 *                          finite, or d - t.z < -sdf_trunc; otherwise tsdf_sum += w min(1, (d - t.z) / sdf_trunc), weight_sum += w,
 *                          colour_sum += w c, in camera order from the stored values.  One read and one write of the pool.
 *   msgs_tsdf_count        a lattice point is observed iff weight_sum > 0 and inside iff it is observed and tsdf_sum < 0.  Per
 *                          lattice point: edge_mask (bit d - 1: the edge to the lattice point at +d, d = dx + 2 dy + 4 dz in 1..7,
 *                          has both ends observed and exactly one inside) and vertex_count = its bit count; per cube (stored at its
 *                          lowest corner; meshed iff all 8 corners are observed) triangle_count of its six Kuhn tetrahedra.
 *   msgs_tsdf_emit         with the exclusive scans of both counts: vertices / colours [n_vertices,3] float32 (colours NULL
 *                          without colour_sum), faces [n_faces,3] int32, normals towards positive TSDF; nothing is written past
 *                          n_vertices / n_faces.
 * All arrays per lattice point are [n_slots, 512].  No atomics: the same bits on every run.  Everything on `stream`, no
 * synchronisation; n_slots == 0 or n == 0 launches nothing. */
#define MSGS_TSDF_CAMERA_CHUNK 64          /* camera rows staged per pass of the integration (tests straddle it) */
#define MSGS_TSDF_MAX_BLOCKS_PER_AXIS 256
#define MSGS_TSDF_MAX_SLOTS (1 << 22)
typedef struct msgs_tsdf_volume {
    float origin[3];
    float voxel_size;
    int32_t nb[3];                   /* blocks along x, y, z */
    int32_t n_slots;
    const int32_t* table;
    const int32_t* slot_block;
    float* tsdf_sum;
    float* weight_sum;
    float* colour_sum;               /* or NULL */
} msgs_tsdf_volume_t;
typedef struct msgs_tsdf_frames {
    int32_t n;
    int32_t W;
    int32_t H;
    int32_t reserved;
    const float* cameras;            /* [n, MSGS_FILTER3D_CAMERA_FLOATS] */
    const float* depth;
    const float* colour;             /* or NULL */
    const float* weight;             /* or NULL */
    float sdf_trunc;
    float depth_trunc;
} msgs_tsdf_frames_t;
typedef struct msgs_tsdf_mesh {
    const uint8_t* edge_mask;
    const int32_t* vertex_offset;
    const int32_t* triangle_offset;
    int32_t n_vertices;
    int32_t n_faces;
    float* vertices;
    float* colours;                  /* or NULL */
    int32_t* faces;
} msgs_tsdf_mesh_t;
int msgs_tsdf_mark_blocks(const msgs_tsdf_volume_t* v, const msgs_tsdf_frames_t* f, int32_t steps, uint8_t* marks, void* stream);
int msgs_tsdf_integrate(const msgs_tsdf_volume_t* v, const msgs_tsdf_frames_t* f, void* stream);
int msgs_tsdf_count(const msgs_tsdf_volume_t* v, uint8_t* edge_mask, int32_t* vertex_count, int32_t* triangle_count,
                    void* stream);
int msgs_tsdf_emit(const msgs_tsdf_volume_t* v, const msgs_tsdf_mesh_t* m, void* stream);

/* ---- k-means vector quantisation (DESIGN.md SPEC M21, 4.23) --------------------------------------------------------------------
 * x [P,D] and codebook [K,D] float32, contiguous rows; 1 <= D <= MSGS_VQ_MAX_DIM, 1 <= K <= MSGS_VQ_MAX_CODES, 0 <= P < 2^31;
 * anything else returns MSGS_ERR_INVALID_ARG and launches nothing.  Inputs are assumed finite and are not checked on the device.
 *   msgs_vq_assign   n_k = float32(1/2 sum_d double(c_kd)^2) (double, ascending d, rounded once); s(i,k) the float32 chain
 *                    s = n_k; for d = 0 .. D-1: s = fmaf(-x_id, c_kd, s) — what the f32 MFMA leaves in an accumulator preloaded
 *                    with n_k; idx [P] int32: the smallest k of minimal score under strict < from (best = +inf, idx = 0), a NaN
 *                    score never wins (a row whose every score is NaN or +inf gets 0); err [P] float32 or NULL: e = 0;
 *                    for d: t = x_id - c_{idx,d}; e = fmaf(t, t, e), from the two rows, not from the score.
 *   msgs_vq_update   the members of code k are the rows order[offsets[k] .. offsets[k+1]) (order [P] int64: the rows sorted by
 *                    code, stable, so ascending within a code; offsets [K+1] int32, offsets[K] = P); chunk_offsets [K+1] int32 is
 *                    the exclusive scan of ceil(members / MSGS_VQ_UPDATE_CHUNK).  Per code and column the double sums of
 *                    double(w_i) double(x_id) and of double(w_i) (w [P] float32 >= 0, or NULL: 1) are taken in member order within
 *                    chunks of MSGS_VQ_UPDATE_CHUNK consecutive members, the chunk partials are added in chunk order, and
 *                    new_codebook[k] = float32(sum / mass), mass [K] double, count [K] int32.  A code of mass 0 copies its row
 *                    of `codebook`; new_codebook may be codebook.  No atomics: the same bits whatever the launch geometry.
 * scratch: msgs_vq_scratch_bytes(P, D, K) bytes (0 for unsupported sizes), 16-byte aligned, no clearing needed, for either call.
 * Everything on `stream`, no synchronisation; P == 0 launches nothing in msgs_vq_assign. */
#define MSGS_VQ_MAX_DIM 64
#define MSGS_VQ_MAX_CODES 65536
#define MSGS_VQ_CODE_CHUNK 64              /* codes per LDS chunk of the search (tests straddle it) */
#define MSGS_VQ_UPDATE_CHUNK 256           /* members per partial sum of the update: part of the result's definition */
size_t msgs_vq_scratch_bytes(int64_t P, int32_t D, int32_t K);
int msgs_vq_assign(int64_t P, int32_t D, int32_t K, const float* x, const float* codebook, int32_t* idx, float* err,
                   void* scratch, size_t scratch_bytes, void* stream);
int msgs_vq_update(int64_t P, int32_t D, int32_t K, const float* x, const float* w, const int64_t* order, const int32_t* offsets,
                   const int32_t* chunk_offsets, const float* codebook, float* new_codebook, double* mass, int32_t* count,
                   void* scratch, size_t scratch_bytes, void* stream);

/* ---- connected components and mesh clean-up (DESIGN.md SPEC M22, 4.24) ----------------------------------------------------------
 * All indices int32, all keys int64; sizes outside 0 <= N, E, n_keys < 2^31 and 0 <= 3 F < 2^31, an unknown mode, and a NULL
 * pointer with a non-zero size return MSGS_ERR_INVALID_ARG and launch nothing.
 *   msgs_graph_components  label [N]: label[x] = the smallest node of x's connected component under the E undirected edges
 *                          (a[i], b[i]), 0 <= a, b < N (the caller's contract: an edge that breaks it is left out); self-loops
 *                          and repeated edges are allowed.  The result is defined by the input alone, so it has the same bits on
 *                          every run.  parent_scratch [N] int32, no clearing needed.  Three launches: identity, link (a union-find
 *                          written by atomicMin only, whose loops wait on no other lane), flatten.  N == 0 launches nothing.
 *   msgs_mesh_corner_keys  faces [F,3]; for corner c = 3 f + k: face_of_key[c] = f and keys[c] = (min(u,v) << 32) | max(u,v) of
 *                          the edge from u = faces[f][k] to v = faces[f][(k+1) % 3] (MSGS_MESH_EDGE) or keys[c] = u
 *                          (MSGS_MESH_VERTEX).  Indices are not dereferenced and not checked.  F == 0 launches nothing.
 *   msgs_mesh_link_sorted  keys_sorted [n_keys] ascending with face_sorted [n_keys] permuted alike (values in [0, F)): the graph
 *                          on the F faces in which face_sorted[i] and face_sorted[i+1] are joined wherever keys_sorted[i] ==
 *                          keys_sorted[i+1]; label [F] and parent_scratch [F] as in msgs_graph_components.  The order among equal
 *                          keys does not matter: a run of equal keys joins all its faces either way.  F == 0 launches nothing.
 *   msgs_mesh_edge_report  counts3 [3] int64 (cleared here): the number of distinct keys that occur once, twice and more often
 *                          in keys_sorted — over MSGS_MESH_EDGE keys the boundary, manifold and non-manifold edges.
 * Everything on `stream`, no synchronisation; the library allocates and keeps nothing. */
#define MSGS_MESH_EDGE 0
#define MSGS_MESH_VERTEX 1
int msgs_graph_components(int64_t N, int64_t E, const int32_t* a, const int32_t* b, int32_t* parent_scratch, int32_t* label,
                          void* stream);
int msgs_mesh_corner_keys(int64_t F, const int32_t* faces, int32_t mode, int64_t* keys, int32_t* face_of_key, void* stream);
int msgs_mesh_link_sorted(int64_t F, int64_t n_keys, const int64_t* keys_sorted, const int32_t* face_sorted,
                          int32_t* parent_scratch, int32_t* label, void* stream);
int msgs_mesh_edge_report(int64_t n_keys, const int64_t* keys_sorted, int64_t* counts3, void* stream);

/* ---- fused photometric loss ----------------------------------------------------------------
 * loss = (1 - lambda_dssim) * l1_loss(img, gt) + lambda_dssim * (1 - ssim(img, gt))   (/root/reference/train.py:209-211)
 * with l1_loss / ssim of /root/reference/utils/loss_utils.py:17-18,32-63 (window 11, sigma 1.5, zero padding, mean).
 * img, gt: [C,H,W] float32 device tensors.  msgs_loss_forward writes out3 = {loss, l1 mean, ssim mean} (device) and,
 * when keep_for_backward != 0, the derivative maps into scratch; msgs_loss_backward then writes
 * dL_dimg[C,H,W] = upstream * dloss/dimg (upstream: device scalar, NULL = 1) — the layout msgs_backward consumes.
 * The loss value is summed in a fixed order (run-to-run identical).  msgs_ssim_window returns the 11 window taps. */
size_t msgs_loss_scratch_bytes(int32_t C, int32_t H, int32_t W);
int msgs_loss_forward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                      float* out3, void* scratch, size_t scratch_bytes, int32_t keep_for_backward, void* stream);
int msgs_loss_backward(const float* img, const float* gt, int32_t C, int32_t H, int32_t W, float lambda_dssim,
                       const float* upstream, const void* scratch, size_t scratch_bytes, float* dL_dimg, void* stream);
int msgs_ssim_window(float* taps11_host);

/* ---- distCUDA2 --------------------------------------------------------------------------------
 * mean_dist2[i] = mean of the squared distances from points[i] to its 3 nearest OTHER points (exact, float32) —
 * `distCUDA2(points)` of the un-vendored simple-knn submodule, used once at initialisation
 * (/root/reference/scene/gaussian_model.py:26,199).  points: [P,3] device, P >= 4. */
size_t msgs_knn_scratch_bytes(int64_t P);
int msgs_dist2_knn3(const float* points, int64_t P, float* mean_dist2, void* scratch, size_t scratch_bytes,
                    void* stream);

/* timing helpers: create/destroy the 2*MSGS_K_COUNT events and read elapsed ms per kernel class
 * (ms_host[MSGS_K_COUNT]; a class that was not recorded reads as -1).  The caller synchronises
 * the stream before msgs_timing_read. */
int msgs_timing_create(msgs_timing_t* t);
int msgs_timing_destroy(msgs_timing_t* t);
int msgs_timing_read(const msgs_timing_t* t, float* ms_host);

#ifdef __cplusplus
}
#endif
#endif /* MSGS_H_ */

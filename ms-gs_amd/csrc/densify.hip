// Model surgery (DESIGN.md SPEC D1): the reference's densify_and_prune / grow_large_gaussians / prune_points /
// densification_postfix (/root/reference/scene/gaussian_model.py:452-537,599-662) as one streaming pass over every
// per-Gaussian tensor, instead of ~90 boolean-mask reads back to the host, ~400 launches and four full copies of the model.
//
//   select  one thread per source row: its fate as flag bits, per-workgroup counts per output segment
//   scan    one workgroup: exclusive offsets of every workgroup's rows in each segment, segment totals
//   place   one thread per source row: the row map of the output (uint32 per output row: kind << 29 | index), stable
//   apply   one multi-tensor launch (the msgs_adam_step table style): each workgroup writes 2048 consecutive elements of one
//           output tensor, lanes spread across rows, so the output is written in full 256-B wave stores and kept source rows
//           are read in order; the rule per tensor and row kind says what the element is.
// The host reads the segment totals once, between place and apply (it needs them to size the outputs and draw z).
#include "msgs_internal.h"

#pragma clang fp contract(off)

namespace msgs {

#define HIP_TRY_ERR(expr)                               \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) return (int)_e;           \
    } while (0)

namespace {

constexpr int SEL_THREADS = 256;
constexpr int NCNT = 5;                        // counters per workgroup: kept, clones kept, children kept, split, grown
constexpr int APPLY_THREADS = 256;
constexpr int APPLY_ITERS = 8;
constexpr int APPLY_EPB = APPLY_THREADS * APPLY_ITERS;   // elements per workgroup
constexpr uint32_t IDX_MASK = (1u << 29) - 1;
constexpr int64_t MAX_ROWS = (int64_t)1 << 29;

enum : uint8_t { F_KEEP = 1, F_CLONE = 2, F_SPLIT = 4, F_CHILD = 8, F_GROW = 16 };
enum : uint32_t { K_KEEP = 0, K_CLONE = 1, K_CHILD1 = 2, K_CHILD2 = 3, K_GROW = 4, K_APPEND = 5 };

// torch's GPU division of a tensor by a CPU scalar is a multiplication by the scalar's reciprocal, formed in float
// (ATen div_true_kernel_cuda): x / (0.8 * N) with N = 2 is x * (1.0f / 1.6f), and 1.0f / 1.6f rounds to 0.625f.
constexpr float SPLIT_INV = 1.0f / (float)(0.8 * 2);

struct Layout {
    size_t flags, bcount, boff, totals, map, split_src, total;
    int64_t nb;
    Layout(int64_t P, int64_t n_append) {
        nb = (P + SEL_THREADS - 1) / SEL_THREADS;
        size_t o = 0;
        flags = o;     o += align256((size_t)(P > 0 ? P : 1));
        bcount = o;    o += align256(sizeof(uint32_t) * NCNT * (size_t)(nb > 0 ? nb : 1));
        boff = o;      o += align256(sizeof(uint32_t) * NCNT * (size_t)(nb > 0 ? nb : 1));
        totals = o;    o += 256;
        map = o;       o += align256(sizeof(uint32_t) * (size_t)(2 * P + n_append > 0 ? 2 * P + n_append : 1));
        split_src = o; o += align256(sizeof(uint32_t) * (size_t)(P > 0 ? P : 1));
        total = o;
    }
};

__device__ inline float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }      // ATen sigmoid_kernel_cuda

__device__ inline float max3_nan(float a, float b, float c) {                      // torch.max(dim=1): NaN propagates
    if (a != a || b != b || c != c) return __builtin_nanf("");
    return fmaxf(fmaxf(a, b), c);
}

// prune mask of densify_and_prune (gaussian_model.py:611-623) for a row of opacity logit o, max activated scale m, target t;
// max_radii2D is all zeros there (the postfix before it reset it)
__device__ inline bool prune_row(float o, float m, int64_t t, const msgs_densify_select_t& s) {
    bool pm = sigmoid_f(o) < s.min_opacity;
    if (s.has_max_screen_size) {
        const bool big_vs = 0.f > s.max_screen_size;
        const bool big_ws = m > s.big_world_limit;
        pm = pm || ((big_vs || big_ws) && t == 0);
    }
    return pm && t == 0;
}

__device__ inline uint64_t lanemask_lt() {
    const int lane = threadIdx.x & 63;
    return lane == 0 ? 0ull : (~0ull >> (64 - lane));
}

__global__ __launch_bounds__(SEL_THREADS) void select_kernel(const msgs_densify_select_t s, uint8_t* __restrict__ flags,
                                                              uint32_t* __restrict__ bcount) {
    const int64_t i = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    uint32_t f = 0;
    if (i < s.P) {
        const int L = s.reso_lvls;
        if (s.mode == MSGS_DENSIFY_PRUNE_MASK) {
            f = s.prune_mask[i] ? 0u : F_KEEP;
        } else if (s.mode == MSGS_DENSIFY_APPEND) {
            const int64_t k = i * L + s.reso_lvl;
            s.xyz_gradient_accum[k] = 0.f;          // the postfix's in-place clear of the tensor it then replaces
            s.denom[k] = 0.f;
            f = F_KEEP;
        } else {
            const int64_t k = i * L + s.reso_lvl;
            float g = s.xyz_gradient_accum[k] / s.denom[k];
            if (g != g) g = 0.f;
            s.xyz_gradient_accum[k] = 0.f;
            s.denom[k] = 0.f;
            if (s.mode == MSGS_DENSIFY_GROW) {
                f = F_KEEP | (sqrtf(g * g) >= s.grad_threshold ? F_GROW : 0u);      // torch.norm over a [N,1] row
            } else {
                const int64_t t = s.target_reso_lvl[i];
                if (t != 0) g = 0.f;
                const float e0 = expf(s.scaling[3 * i]), e1 = expf(s.scaling[3 * i + 1]), e2 = expf(s.scaling[3 * i + 2]);
                const float m = max3_nan(e0, e1, e2);
                const bool clone = sqrtf(g * g) >= s.grad_threshold && m <= s.scale_limit;
                const bool split = g >= s.grad_threshold && m > s.scale_limit;
                const float o = s.opacity[i];
                const bool pruned = prune_row(o, m, t, s);        // a clone has its source's values: same verdict
                if (split) {
                    f = F_SPLIT;
                    const float c0 = expf(logf(e0 * SPLIT_INV)), c1 = expf(logf(e1 * SPLIT_INV)), c2 = expf(logf(e2 * SPLIT_INV));
                    if (!prune_row(o, max3_nan(c0, c1, c2), t, s)) f |= F_CHILD;      // both children are equal here
                } else {
                    f = pruned ? 0u : F_KEEP;
                    if (clone && !pruned) f |= F_CLONE;
                }
            }
        }
        flags[i] = (uint8_t)f;
    }
    __shared__ uint32_t wc[SEL_THREADS / 64][NCNT];
    const int w = threadIdx.x >> 6;
    const uint32_t bits[NCNT] = {F_KEEP, F_CLONE, F_CHILD, F_SPLIT, F_GROW};
#pragma unroll
    for (int c = 0; c < NCNT; ++c) {
        const uint32_t n = (uint32_t)__popcll(__ballot((f & bits[c]) != 0));
        if ((threadIdx.x & 63) == 0) wc[w][c] = n;
    }
    __syncthreads();
    if (threadIdx.x < NCNT) {
        uint32_t n = 0;
        for (int k = 0; k < SEL_THREADS / 64; ++k) n += wc[k][threadIdx.x];
        bcount[(int64_t)blockIdx.x * NCNT + threadIdx.x] = n;
    }
}

// one workgroup: thread t owns a run of consecutive workgroup entries, sums it, the workgroup scans the run sums
constexpr int DENS_SCAN_THREADS = 1024;
__global__ __launch_bounds__(DENS_SCAN_THREADS) void scan_kernel(const uint32_t* __restrict__ bcount, uint32_t* __restrict__ boff,
                                                            int64_t nb, int64_t n_append, uint64_t* __restrict__ totals) {
    __shared__ uint32_t sh[DENS_SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t per = (nb + DENS_SCAN_THREADS - 1) / DENS_SCAN_THREADS;
    const int64_t lo = t * per, hi = lo + per < nb ? lo + per : nb;
    for (int c = 0; c < NCNT; ++c) {
        uint32_t sum = 0;
        for (int64_t j = lo; j < hi; ++j) sum += bcount[j * NCNT + c];
        sh[t] = sum;
        __syncthreads();
        for (int d = 1; d < DENS_SCAN_THREADS; d <<= 1) {        // inclusive Hillis-Steele
            const uint32_t v = t >= d ? sh[t - d] : 0u;
            __syncthreads();
            sh[t] += v;
            __syncthreads();
        }
        uint32_t run = sh[t] - sum;
        for (int64_t j = lo; j < hi; ++j) {
            boff[j * NCNT + c] = run;
            run += bcount[j * NCNT + c];
        }
        if (t == DENS_SCAN_THREADS - 1) totals[c] = sh[t];
        __syncthreads();
    }
    if (t == 0) {
        totals[5] = (uint64_t)n_append;
        totals[6] = totals[0] + totals[1] + 2 * totals[2] + totals[4] + (uint64_t)n_append;
        totals[7] = 0;
    }
}

__global__ __launch_bounds__(SEL_THREADS) void place_kernel(const uint8_t* __restrict__ flags, const uint32_t* __restrict__ boff,
                                                             const uint64_t* __restrict__ totals, int64_t P, int64_t nb,
                                                             int64_t n_append, uint32_t* __restrict__ map,
                                                             uint32_t* __restrict__ split_src) {
    const uint64_t s1 = totals[0], s2 = s1 + totals[1], s3 = s2 + totals[2], s4 = s3 + totals[2], s5 = s4 + totals[4];
    if ((int64_t)blockIdx.x >= nb) {                                 // appended rows
        const int64_t a = ((int64_t)blockIdx.x - nb) * SEL_THREADS + threadIdx.x;
        if (a < n_append) map[s5 + a] = (K_APPEND << 29) | (uint32_t)a;
        return;
    }
    const int64_t i = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    const uint32_t f = i < P ? flags[i] : 0u;
    __shared__ uint32_t wc[SEL_THREADS / 64][NCNT];
    const int w = threadIdx.x >> 6;
    const uint32_t bits[NCNT] = {F_KEEP, F_CLONE, F_CHILD, F_SPLIT, F_GROW};
    uint32_t rank[NCNT];
    const uint64_t lt = lanemask_lt();
#pragma unroll
    for (int c = 0; c < NCNT; ++c) {
        const uint64_t b = __ballot((f & bits[c]) != 0);
        rank[c] = (uint32_t)__popcll(b & lt);
        if ((threadIdx.x & 63) == 0) wc[w][c] = (uint32_t)__popcll(b);
    }
    __syncthreads();
    if (i >= P) return;
    const uint32_t* bo = boff + (int64_t)blockIdx.x * NCNT;
#pragma unroll
    for (int c = 0; c < NCNT; ++c) {
        uint32_t r = rank[c] + bo[c];
        for (int k = 0; k < w; ++k) r += wc[k][c];
        rank[c] = r;
    }
    const uint32_t row = (uint32_t)i;
    if (f & F_KEEP) map[rank[0]] = (K_KEEP << 29) | row;
    if (f & F_CLONE) map[s1 + rank[1]] = (K_CLONE << 29) | row;
    if (f & F_SPLIT) {
        const uint32_t j = rank[3];
        split_src[j] = row;
        if (f & F_CHILD) {
            map[s2 + rank[2]] = (K_CHILD1 << 29) | j;
            map[s3 + rank[2]] = (K_CHILD2 << 29) | j;
        }
    }
    if (f & F_GROW) map[s4 + rank[4]] = (K_GROW << 29) | row;
}

// ------------------------------------------------------------------------------------------------------------------------
// apply
// ------------------------------------------------------------------------------------------------------------------------
struct ApplySlot {
    void* dst;
    const void* src;
    const void* app;
    int64_t constant;
    int64_t n;             // output elements
    int32_t W;
    int32_t esz;
    float invW;
    uint8_t rule[8];
};

struct ApplyTable {
    ApplySlot t[MSGS_DENSIFY_MAX_TENSORS];
    uint32_t first_block[MSGS_DENSIFY_MAX_TENSORS + 1];
    int n;
    int lvl;
    int64_t n_split;
    const float* xyz;
    const float* scaling;
    const float* rotation;
    const float* draws;
    const uint32_t* map;
    const uint32_t* split_src;
};

// children's position: build_rotation (utils/general_utils.py:78-99) op by op, samples = z * exp(s) + 0 (torch.normal with
// mean 0), then R · samples (torch.bmm there: the one value not reproduced bit for bit) + xyz
__device__ inline float split_xyz(const ApplyTable& a, int64_t src, int64_t j, int col) {
    const float r0 = a.rotation[4 * src], r1 = a.rotation[4 * src + 1], r2 = a.rotation[4 * src + 2], r3 = a.rotation[4 * src + 3];
    const float nrm = sqrtf(((r0 * r0 + r1 * r1) + r2 * r2) + r3 * r3);
    const float r = r0 / nrm, x = r1 / nrm, y = r2 / nrm, z = r3 / nrm;
    float R0, R1, R2;
    if (col == 0) {
        R0 = 1.f - 2.f * (y * y + z * z); R1 = 2.f * (x * y - r * z); R2 = 2.f * (x * z + r * y);
    } else if (col == 1) {
        R0 = 2.f * (x * y + r * z); R1 = 1.f - 2.f * (x * x + z * z); R2 = 2.f * (y * z - r * x);
    } else {
        R0 = 2.f * (x * z - r * y); R1 = 2.f * (y * z + r * x); R2 = 1.f - 2.f * (x * x + y * y);
    }
    const float s0 = a.draws[3 * j] * expf(a.scaling[3 * src]) + 0.f;
    const float s1 = a.draws[3 * j + 1] * expf(a.scaling[3 * src + 1]) + 0.f;
    const float s2 = a.draws[3 * j + 2] * expf(a.scaling[3 * src + 2]) + 0.f;
    return ((R0 * s0 + R1 * s1) + R2 * s2) + a.xyz[3 * src + col];
}

template <typename T>
__device__ inline T elem_value(const ApplyTable& a, const ApplySlot& S, uint32_t m, int64_t col) {
    const uint32_t kind = m >> 29, idx = m & IDX_MASK;
    const int rule = S.rule[kind];
    const bool child = kind == K_CHILD1 || kind == K_CHILD2;
    const int64_t src = child ? (int64_t)a.split_src[idx] : (int64_t)idx;
    const T* __restrict__ X = static_cast<const T*>(S.src);
    const int64_t at = src * S.W + col;
    if constexpr (sizeof(T) == 4) {
        switch (rule) {
            case MSGS_DR_COPY: return X[at];
            case MSGS_DR_COPY_CLEAR_COL: return col == a.lvl ? 0.f : X[at];
            case MSGS_DR_SPLIT_XYZ: return split_xyz(a, src, (int64_t)idx + (kind == K_CHILD2 ? a.n_split : 0), (int)col);
            case MSGS_DR_SPLIT_SCALE: return logf(expf(X[at]) * SPLIT_INV);
            case MSGS_DR_SPLIT_DIV: return X[at] * SPLIT_INV;
            case MSGS_DR_GROW_OPACITY: {
                const float x = sigmoid_f(X[at]) * 0.5f;           // get_opacity / 2, then inverse_sigmoid
                return logf(x / (1.f - x));
            }
            case MSGS_DR_GROW_SCALE: return logf(expf(X[at]) * 2.f);
            case MSGS_DR_GROW_MUL: return X[at] * 2.f;
            case MSGS_DR_APPEND: return static_cast<const T*>(S.app)[(int64_t)idx * S.W + col];
            default: return 0.f;
        }
    } else {
        switch (rule) {
            case MSGS_DR_COPY: return X[at];
            case MSGS_DR_CONST: return (T)S.constant;
            case MSGS_DR_APPEND: return static_cast<const T*>(S.app)[(int64_t)idx * S.W + col];
            default: return (T)0;
        }
    }
}

template <typename T>
__device__ inline void apply_slot(const ApplyTable& a, const ApplySlot& S, int64_t base) {
    const int64_t W = S.W;
    const int64_t row0 = base / W;
    const uint32_t off0 = (uint32_t)(base - row0 * W);
    T v[APPLY_ITERS];
#pragma unroll
    for (int it = 0; it < APPLY_ITERS; ++it) {
        const int64_t e = base + it * APPLY_THREADS + threadIdx.x;
        if (e >= S.n) continue;
        const uint32_t loc = off0 + (uint32_t)(it * APPLY_THREADS + threadIdx.x);
        int32_t q = (int32_t)((float)loc * S.invW);                  // loc < 2^23: q is off by at most one
        int32_t r = (int32_t)loc - q * S.W;
        if (r < 0) { --q; r += S.W; } else if (r >= S.W) { ++q; r -= S.W; }
        v[it] = elem_value<T>(a, S, a.map[row0 + q], r);
    }
    T* __restrict__ D = static_cast<T*>(S.dst);
#pragma unroll
    for (int it = 0; it < APPLY_ITERS; ++it) {
        const int64_t e = base + it * APPLY_THREADS + threadIdx.x;
        if (e < S.n) D[e] = v[it];
    }
}

__global__ __launch_bounds__(APPLY_THREADS) void apply_kernel(const ApplyTable a) {
    int ti = 0;
    for (int k = 1; k < a.n; ++k) ti += blockIdx.x >= a.first_block[k] ? 1 : 0;
    const ApplySlot& S = a.t[ti];
    const int64_t base = (int64_t)(blockIdx.x - a.first_block[ti]) * APPLY_EPB;
    if (S.esz == 4) apply_slot<float>(a, S, base);
    else if (S.esz == 8) apply_slot<int64_t>(a, S, base);
    else apply_slot<uint8_t>(a, S, base);
}

bool rule_reads_src(int r) {
    return r == MSGS_DR_COPY || r == MSGS_DR_COPY_CLEAR_COL || r == MSGS_DR_SPLIT_SCALE || r == MSGS_DR_SPLIT_DIV ||
           r == MSGS_DR_GROW_OPACITY || r == MSGS_DR_GROW_SCALE || r == MSGS_DR_GROW_MUL;
}

}  // namespace

size_t densify_scratch_bytes(int64_t P, int64_t n_append) { return Layout(P, n_append).total; }

int densify_select(const msgs_densify_select_t& s, char* scratch, int64_t* counts_host, hipStream_t st) {
    const Layout L(s.P, s.n_append);
    uint8_t* flags = (uint8_t*)(scratch + L.flags);
    uint32_t* bcount = (uint32_t*)(scratch + L.bcount);
    uint32_t* boff = (uint32_t*)(scratch + L.boff);
    uint64_t* totals = (uint64_t*)(scratch + L.totals);
    uint32_t* map = (uint32_t*)(scratch + L.map);
    uint32_t* split_src = (uint32_t*)(scratch + L.split_src);
    if (L.nb > 0) hipLaunchKernelGGL(select_kernel, dim3((unsigned)L.nb), dim3(SEL_THREADS), 0, st, s, flags, bcount);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(DENS_SCAN_THREADS), 0, st, bcount, boff, L.nb, s.n_append, totals);
    const int64_t nblk = L.nb + (s.n_append + SEL_THREADS - 1) / SEL_THREADS;
    if (nblk > 0)
        hipLaunchKernelGGL(place_kernel, dim3((unsigned)nblk), dim3(SEL_THREADS), 0, st, flags, boff, totals, s.P, L.nb,
                           s.n_append, map, split_src);
    HIP_TRY_ERR(hipGetLastError());
    uint64_t host[8];
    HIP_TRY_ERR(hipMemcpyAsync(host, totals, sizeof(host), hipMemcpyDeviceToHost, st));
    HIP_TRY_ERR(hipStreamSynchronize(st));
    for (int k = 0; k < 8; ++k) counts_host[k] = (int64_t)host[k];
    return MSGS_OK;
}

int densify_apply(const msgs_densify_apply_t& a, const char* scratch, hipStream_t st) {
    const Layout L(a.P, a.n_append);
    ApplyTable t{};
    t.n = a.n_tensors;
    t.lvl = a.reso_lvl;
    t.n_split = a.n_split;
    t.xyz = a.xyz; t.scaling = a.scaling; t.rotation = a.rotation; t.draws = a.draws;
    t.map = (const uint32_t*)(scratch + L.map);
    t.split_src = (const uint32_t*)(scratch + L.split_src);
    uint64_t blocks = 0;
    for (int k = 0; k < a.n_tensors; ++k) {
        const msgs_densify_tensor_t& d = a.tensors[k];
        ApplySlot& S = t.t[k];
        S.dst = d.dst; S.src = d.src; S.app = d.append_src; S.constant = d.constant;
        S.W = d.width; S.esz = d.elem_bytes; S.n = a.P_out * d.width;
        S.invW = 1.0f / (float)d.width;
        for (int r = 0; r < 8; ++r) S.rule[r] = d.rule[r];
        t.first_block[k] = (uint32_t)blocks;
        blocks += (uint64_t)((S.n + APPLY_EPB - 1) / APPLY_EPB);
    }
    for (int k = a.n_tensors; k <= MSGS_DENSIFY_MAX_TENSORS; ++k) t.first_block[k] = (uint32_t)blocks;
    if (blocks > 0xFFFFFFFFull) return MSGS_ERR_TOO_MANY;
    if (blocks == 0) return MSGS_OK;
    hipLaunchKernelGGL(apply_kernel, dim3((unsigned)blocks), dim3(APPLY_THREADS), 0, st, t);
    HIP_TRY_ERR(hipGetLastError());
    return MSGS_OK;
}

// argument checks shared by the two entries (api.hip calls them before launching anything)
int densify_check_select(const msgs_densify_select_t& s) {
    if (s.P < 0 || s.n_append < 0 || s.P >= MAX_ROWS || s.n_append >= MAX_ROWS || 2 * s.P + s.n_append >= MAX_ROWS)
        return s.P < 0 || s.n_append < 0 ? MSGS_ERR_INVALID_ARG : MSGS_ERR_TOO_MANY;
    if (s.mode < MSGS_DENSIFY_PRUNE || s.mode > MSGS_DENSIFY_APPEND) return MSGS_ERR_INVALID_ARG;
    if (s.mode != MSGS_DENSIFY_APPEND && s.n_append != 0) return MSGS_ERR_INVALID_ARG;
    if (s.P == 0) return MSGS_OK;
    if (s.mode == MSGS_DENSIFY_PRUNE_MASK) return s.prune_mask ? MSGS_OK : MSGS_ERR_INVALID_ARG;
    if (s.reso_lvls < 1 || s.reso_lvl < 0 || s.reso_lvl >= s.reso_lvls || !s.xyz_gradient_accum || !s.denom)
        return MSGS_ERR_INVALID_ARG;
    if (s.mode == MSGS_DENSIFY_PRUNE && (s.reso_lvl != 0 || !s.opacity || !s.scaling || !s.target_reso_lvl))
        return MSGS_ERR_INVALID_ARG;
    return MSGS_OK;
}

int densify_check_apply(const msgs_densify_apply_t& a) {
    if (a.P < 0 || a.n_append < 0 || a.P_out < 0 || a.n_split < 0 || a.n_tensors < 0 ||
        a.n_tensors > MSGS_DENSIFY_MAX_TENSORS || (a.n_tensors && !a.tensors))
        return MSGS_ERR_INVALID_ARG;
    if (a.P_out > 2 * a.P + a.n_append || a.n_split > a.P) return MSGS_ERR_INVALID_ARG;
    for (int k = 0; k < a.n_tensors; ++k) {
        const msgs_densify_tensor_t& d = a.tensors[k];
        if (d.width < 1 || (d.elem_bytes != 1 && d.elem_bytes != 4 && d.elem_bytes != 8)) return MSGS_ERR_INVALID_ARG;
        if (a.P_out > 0 && !d.dst) return MSGS_ERR_INVALID_ARG;
        if ((int64_t)d.width * (a.P_out > a.P ? a.P_out : a.P) >= ((int64_t)1 << 40)) return MSGS_ERR_TOO_MANY;
        for (int r = 0; r < 6; ++r) {
            const int rule = d.rule[r];
            if (rule > MSGS_DR_APPEND) return MSGS_ERR_INVALID_ARG;
            if (d.elem_bytes != 4 && rule != MSGS_DR_COPY && rule != MSGS_DR_ZERO && rule != MSGS_DR_CONST &&
                rule != MSGS_DR_APPEND)
                return MSGS_ERR_INVALID_ARG;
            if (d.elem_bytes == 4 && rule == MSGS_DR_CONST) return MSGS_ERR_INVALID_ARG;
            if (rule_reads_src(rule) && a.P > 0 && !d.src) return MSGS_ERR_INVALID_ARG;
            if (rule == MSGS_DR_APPEND && a.n_append > 0 && !d.append_src) return MSGS_ERR_INVALID_ARG;
            if (rule == MSGS_DR_SPLIT_XYZ && (d.width != 3 || (a.n_split > 0 && (!a.xyz || !a.scaling || !a.rotation || !a.draws))))
                return MSGS_ERR_INVALID_ARG;
        }
    }
    return MSGS_OK;
}

}  // namespace msgs

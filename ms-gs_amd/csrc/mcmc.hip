// MCMC densification (DESIGN.md SPEC M18, 4.19): the model surgery of "3D Gaussian Splatting as Markov Chain Monte Carlo" —
// opacity-weighted sampling with replacement, the relocation rule, dead rows rewritten in place or new rows built for a capped
// growth, and the per-step covariance-shaped position noise.
//
//   weights   one thread per row: w = sigmoid(x) in double (0 for dead rows), per-workgroup sum, dead / positive counts
//   scan      one workgroup: the offsets of every workgroup's rows in the CDF and in the dead-row list, the totals
//   cdf       one thread per row: cdf[i] (inclusive, double) and the stable list of dead rows
//   draw      one thread per draw: binary search of u * total in the CDF, count[row] += 1 (integer atomics: exact)
//   ratio     one thread per row, drawn rows only: (x_new, s_new, pixel sizes * c) from the row's OLD values into scratch
//   rows      one thread per element of a written row (a dead row, or a new row of a fresh block): copies of the source's fields,
//             the source's new values from scratch, zeros
//   sources   one thread per row, drawn rows only: the row's own new values from scratch, its optimizer moments zeroed
//   noise     one thread per row, streaming: xyz += R S^2 R^T xi * gain / (1 + exp(-100 (0.005 - o)))
//
// Every sum of the CDF is taken in one fixed order and so that it is MONOTONE and exactly FLAT over weight-0 rows: a value is
// fl(a + fl(b + c)) with c the sequential inclusive sum inside the workgroup, b the sequential sum of the workgroups before it in
// its scan thread's run and a the sequential sum of the scan threads before that one — each level's last value IS the next
// level's increment, so the row after a boundary starts from exactly the bits the row before it ended on.  A draw therefore
// never lands on a row of weight 0: it takes the first row whose CDF exceeds u * total, and such a row has raised the CDF.
#include "msgs_internal.h"

#pragma clang fp contract(off)

namespace msgs {

#define HIP_TRY_ERR(expr)                               \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) return (int)_e;           \
    } while (0)

namespace {

constexpr int ROW_THREADS = 256;               // rows per workgroup of weights / cdf (one row per thread)
constexpr int MCMC_SCAN_THREADS = 1024;
constexpr int N_VALS = 6;                      // scratch floats per drawn row: x_new, s_new[3], max_pixel_size * c, min_pixel_size * c

struct Totals {
    double total;
    uint64_t n_dead, n_positive, reserved;
};

struct Layout {
    size_t cdf, bsum, boff, bcnt, bdoff, totals, count, source, dead_list, vals, total;
    int64_t nb;
    explicit Layout(int64_t P) {
        const size_t p = (size_t)(P > 0 ? P : 1);
        nb = (P + ROW_THREADS - 1) / ROW_THREADS;
        const size_t b = (size_t)(nb > 0 ? nb : 1);
        size_t o = 0;
        cdf = o;       o += align256(sizeof(double) * p);
        bsum = o;      o += align256(sizeof(double) * b);
        boff = o;      o += align256(sizeof(double) * 2 * b);      // per workgroup: {a, b} of the header
        bcnt = o;      o += align256(sizeof(uint32_t) * 2 * b);    // per workgroup: dead rows, rows of positive weight
        bdoff = o;     o += align256(sizeof(uint32_t) * b);        // per workgroup: dead rows before it
        totals = o;    o += 256;
        count = o;     o += align256(sizeof(int32_t) * p);
        source = o;    o += align256(sizeof(int32_t) * p);
        dead_list = o; o += align256(sizeof(uint32_t) * p);
        vals = o;      o += align256(sizeof(float) * N_VALS * p);
        total = o;
    }
};

__device__ inline double weight_of(const float* __restrict__ opacity, const uint8_t* __restrict__ dead, int64_t i, int64_t P) {
    if (i >= P || (dead && dead[i])) return 0.0;
    const double w = 1.0 / (1.0 + exp(-(double)opacity[i]));
    return w > 0.0 ? w : 0.0;                  // a NaN logit has no weight
}

// inclusive sums of the workgroup's weights in row order, by ONE thread (see the header: a tree would not be flat)
__device__ inline double block_inclusive(double w, double* sh) {
    sh[threadIdx.x] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        double run = 0.0;
        for (int k = 0; k < ROW_THREADS; ++k) {
            run += sh[k];
            sh[k] = run;
        }
    }
    __syncthreads();
    return sh[threadIdx.x];
}

__global__ __launch_bounds__(ROW_THREADS) void mcmc_weights_kernel(int64_t P, const float* __restrict__ opacity,
                                                                    const uint8_t* __restrict__ dead, double* __restrict__ bsum,
                                                                    uint32_t* __restrict__ bcnt) {
    __shared__ double sh[ROW_THREADS];
    __shared__ uint32_t wc[ROW_THREADS / 64][2];
    const int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x;
    const double w = weight_of(opacity, dead, i, P);
    const bool is_dead = i < P && dead && dead[i];
    const uint32_t nd = (uint32_t)__popcll(__ballot(is_dead)), np = (uint32_t)__popcll(__ballot(w > 0.0));
    if ((threadIdx.x & 63) == 0) { wc[threadIdx.x >> 6][0] = nd; wc[threadIdx.x >> 6][1] = np; }
    block_inclusive(w, sh);
    if (threadIdx.x == 0) bsum[blockIdx.x] = sh[ROW_THREADS - 1];
    if (threadIdx.x < 2) {
        uint32_t n = 0;
        for (int k = 0; k < ROW_THREADS / 64; ++k) n += wc[k][threadIdx.x];
        bcnt[2 * (int64_t)blockIdx.x + threadIdx.x] = n;
    }
}

// thread t owns a run of consecutive workgroups and sums it in order; thread 0 then chains the run sums in order
__global__ __launch_bounds__(MCMC_SCAN_THREADS) void mcmc_scan_kernel(const double* __restrict__ bsum,
                                                                       const uint32_t* __restrict__ bcnt, int64_t nb,
                                                                       double* __restrict__ boff, uint32_t* __restrict__ bdoff,
                                                                       Totals* __restrict__ totals) {
    __shared__ double sh[MCMC_SCAN_THREADS];
    __shared__ uint32_t shd[MCMC_SCAN_THREADS], shp[MCMC_SCAN_THREADS];
    const int t = threadIdx.x;
    const int64_t per = (nb + MCMC_SCAN_THREADS - 1) / MCMC_SCAN_THREADS;
    const int64_t lo = t * per < nb ? t * per : nb, hi = lo + per < nb ? lo + per : nb;
    double run = 0.0;
    uint32_t nd = 0, np = 0;
    for (int64_t j = lo; j < hi; ++j) {
        run += bsum[j];
        nd += bcnt[2 * j];
        np += bcnt[2 * j + 1];
    }
    sh[t] = run; shd[t] = nd; shp[t] = np;
    __syncthreads();
    if (t == 0) {
        double acc = 0.0;
        uint64_t ad = 0, ap = 0;
        for (int k = 0; k < MCMC_SCAN_THREADS; ++k) {
            const double v = sh[k];
            const uint32_t d = shd[k];
            sh[k] = acc; shd[k] = (uint32_t)ad;
            acc += v; ad += d; ap += shp[k];
        }
        totals->total = acc;
        totals->n_dead = ad;
        totals->n_positive = ap;
        totals->reserved = 0;
    }
    __syncthreads();
    const double a = sh[t];
    double b = 0.0;
    uint32_t d = shd[t];
    for (int64_t j = lo; j < hi; ++j) {
        boff[2 * j] = a;
        boff[2 * j + 1] = b;
        bdoff[j] = d;
        b += bsum[j];
        d += bcnt[2 * j];
    }
}

__global__ __launch_bounds__(ROW_THREADS) void mcmc_cdf_kernel(int64_t P, const float* __restrict__ opacity,
                                                                const uint8_t* __restrict__ dead,
                                                                const double* __restrict__ boff, const uint32_t* __restrict__ bdoff,
                                                                double* __restrict__ cdf, uint32_t* __restrict__ dead_list) {
    __shared__ double sh[ROW_THREADS];
    __shared__ uint32_t wc[ROW_THREADS / 64];
    const int64_t i = (int64_t)blockIdx.x * ROW_THREADS + threadIdx.x;
    const double w = weight_of(opacity, dead, i, P);
    const bool is_dead = i < P && dead && dead[i];
    const uint64_t bal = __ballot(is_dead);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wc[wave] = (uint32_t)__popcll(bal);
    const double c = block_inclusive(w, sh);                         // (its barriers also publish wc)
    if (i >= P) return;
    cdf[i] = boff[2 * (int64_t)blockIdx.x] + (boff[2 * (int64_t)blockIdx.x + 1] + c);
    if (is_dead) {
        uint32_t r = bdoff[blockIdx.x] + (uint32_t)__popcll(bal & (lane == 0 ? 0ull : (~0ull >> (64 - lane))));
        for (int k = 0; k < wave; ++k) r += wc[k];
        dead_list[r] = (uint32_t)i;                                  // r < n_dead <= P
    }
}

// draw j takes the first row whose CDF exceeds u_j * total; when the product rounds up to the total (or u is not below 1), the
// last row of positive weight, which is the first row whose CDF equals the total
__global__ __launch_bounds__(256) void mcmc_draw_kernel(int64_t P, int64_t n, const double* __restrict__ u,
                                                         const double* __restrict__ cdf, int32_t* __restrict__ source,
                                                         int32_t* __restrict__ count) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const double total = cdf[P - 1];
    if (!(total > 0.0)) {                      // no row of positive weight: nothing to select (the host reports it)
        source[j] = -1;
        return;
    }
    const double v = u[j] * total;
    int64_t lo = 0, hi = P;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cdf[mid] > v) hi = mid; else lo = mid + 1;
    }
    if (lo == P) {
        lo = 0; hi = P - 1;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (cdf[mid] >= total) hi = mid; else lo = mid + 1;
        }
    }
    source[j] = (int32_t)lo;
    atomicAdd(&count[lo], 1);
}

// SPEC M18 (b), everything in double.  The double sum over i and k collapses by the hockey-stick identity
// sum_{i=k+1..N} C(i-1, k) = C(N, k+1) to D = sum_{k=0..N-1} C(N, k+1) (-1)^k / sqrt(k+1) o_new^(k+1): the same terms grouped by
// k, so its sum of magnitudes (and with it the condition number) is no larger than the double sum's.  C(N, k+1) is run up from
// C(N, k) (N - k) / (k + 1): every product stays below 2^53 for N <= 51, so each binomial is exact.
__global__ __launch_bounds__(256) void mcmc_ratio_kernel(int64_t P, const int32_t* __restrict__ count,
                                                          const float* __restrict__ opacity, const float* __restrict__ scaling,
                                                          const float* __restrict__ max_pix, const float* __restrict__ min_pix,
                                                          float* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int cnt = count[i];
    if (cnt <= 0) return;
    const int N = cnt + 1 < MSGS_MCMC_N_MAX ? cnt + 1 : MSGS_MCMC_N_MAX;
    const double x = (double)opacity[i];
    const double log1mo = -((x > 0.0 ? x : 0.0) + log1p(exp(-fabs(x))));     // log(1 - o) = -softplus(x)
    const double o = 1.0 / (1.0 + exp(-x));
    const double l = log1mo / (double)N;                                       // log(1 - o_new)
    const double on = -expm1(l);
    double D = 0.0, p = on, binom = 1.0;
    for (int k = 0; k < N; ++k) {
        binom = binom * (double)(N - k) / (double)(k + 1);                     // C(N, k+1)
        const double term = binom / sqrt((double)(k + 1)) * p;
        D += (k & 1) ? -term : term;
        p *= on;
    }
    const double c = o / D;
    const double logc = log(c);
    const double lo_o = 0.005, hi_o = 1.0 - 0x1p-24;
    double xn;
    if (on < lo_o) xn = log(lo_o) - log1p(-lo_o);
    else if (on > hi_o) xn = log(hi_o) - log(0x1p-24);
    else xn = log(on) - l;
    float* v = vals + N_VALS * i;
    v[0] = (float)xn;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[1 + k] = (float)((double)scaling[3 * i + k] + logc);
    const float cf = (float)c;
    v[4] = max_pix ? max_pix[i] * cf : 0.f;
    v[5] = min_pix ? min_pix[i] * cf : 0.f;
}

struct Slot {
    void* data;            // [P, W] the model's tensor
    void* fresh;           // [n, W] new rows (growth), or null
    float* exp_avg;        // [P, W] or null
    float* exp_avg_sq;
    int32_t W, esz, rule;
};

struct Table {
    Slot t[MSGS_MCMC_MAX_TENSORS];
    int32_t n_slots, in_place;
    int64_t P, n;
    const int32_t* source;
    const int32_t* count;
    const uint32_t* dead_list;
    const float* vals;
    const Totals* totals;
};

// grid (elements of the widest tensor, tensors): element e of tensor blockIdx.y is column e % W of written row e / W.  It reads
// the source's fields that nobody writes, and the source's new values from scratch.
__global__ __launch_bounds__(256) void mcmc_rows_kernel(const Table a) {
    const Slot& S = a.t[blockIdx.y];
    char* __restrict__ dst = static_cast<char*>(a.in_place ? S.data : S.fresh);
    if (!dst) return;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n * S.W) return;
    const int64_t j = e / S.W;
    const int col = (int)(e - j * S.W);
    const int64_t r = a.source[j];
    if (r < 0) return;
    int64_t row = j;
    if (a.in_place) {
        if ((uint64_t)j >= a.totals->n_dead) return;              // more draws than dead rows: nothing to write them to
        row = a.dead_list[j];
    }
    const int64_t at = row * S.W + col, from = r * S.W + col;
    if (S.esz == 4) {
        const float* __restrict__ X = static_cast<const float*>(S.data);
        const float* __restrict__ v = a.vals + N_VALS * r;
        float y;
        switch (S.rule) {
            case MSGS_MR_COPY: y = X[from]; break;
            case MSGS_MR_OPACITY: y = v[0]; break;
            case MSGS_MR_SCALE: y = v[1 + col]; break;
            case MSGS_MR_PIX_MAX: y = v[4]; break;
            case MSGS_MR_PIX_MIN: y = v[5]; break;
            default: y = 0.f;
        }
        reinterpret_cast<float*>(dst)[at] = y;
    } else if (S.esz == 8) {
        reinterpret_cast<int64_t*>(dst)[at] = S.rule == MSGS_MR_COPY ? static_cast<const int64_t*>(S.data)[from] : (int64_t)0;
    } else {
        reinterpret_cast<uint8_t*>(dst)[at] = S.rule == MSGS_MR_COPY ? static_cast<const uint8_t*>(S.data)[from] : (uint8_t)0;
    }
}

// every drawn source: its own new opacity, scales and pixel sizes, and zero moments in every tensor that carries them
__global__ __launch_bounds__(256) void mcmc_sources_kernel(const Table a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.P || a.count[i] <= 0) return;
    const float* __restrict__ v = a.vals + N_VALS * i;
    for (int k = 0; k < a.n_slots; ++k) {
        const Slot& S = a.t[k];
        float* __restrict__ X = static_cast<float*>(S.data);
        switch (S.rule) {
            case MSGS_MR_OPACITY: X[i] = v[0]; break;
            case MSGS_MR_SCALE: X[3 * i] = v[1]; X[3 * i + 1] = v[2]; X[3 * i + 2] = v[3]; break;
            case MSGS_MR_PIX_MAX: X[i] = v[4]; break;
            case MSGS_MR_PIX_MIN: X[i] = v[5]; break;
            default: break;
        }
        if (S.exp_avg)
            for (int c = 0; c < S.W; ++c) S.exp_avg[i * S.W + c] = 0.f;
        if (S.exp_avg_sq)
            for (int c = 0; c < S.W; ++c) S.exp_avg_sq[i * S.W + c] = 0.f;
    }
}

// one row per lane, 68 bytes moved per Gaussian: q = raw / max(|raw|, 1e-12) as the rasterizer's preprocess forms it, R the
// rotation of build_rotation, t = R^T xi, t_k *= exp(s_k)^2, d = R t
__global__ __launch_bounds__(256) void mcmc_noise_kernel(int64_t P, float* __restrict__ xyz, const float* __restrict__ scaling,
                                                          const float* __restrict__ rotation, const float* __restrict__ opacity,
                                                          const float* __restrict__ draws, float gain) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const float4 q4 = reinterpret_cast<const float4*>(rotation)[i];
    const float xi0 = draws[3 * i], xi1 = draws[3 * i + 1], xi2 = draws[3 * i + 2];
    const float l0 = scaling[3 * i], l1 = scaling[3 * i + 1], l2 = scaling[3 * i + 2];
    const float p0 = xyz[3 * i], p1 = xyz[3 * i + 1], p2 = xyz[3 * i + 2];
    const float ox = opacity[i];
    const float nrm = fmaxf(sqrtf(((q4.x * q4.x + q4.y * q4.y) + q4.z * q4.z) + q4.w * q4.w), 1e-12f);
    const float r = q4.x / nrm, x = q4.y / nrm, y = q4.z / nrm, z = q4.w / nrm;
    const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
    const float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
    const float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
    const float s0 = expf(l0), s1 = expf(l1), s2 = expf(l2);
    const float t0 = ((R00 * xi0 + R10 * xi1) + R20 * xi2) * (s0 * s0);
    const float t1 = ((R01 * xi0 + R11 * xi1) + R21 * xi2) * (s1 * s1);
    const float t2 = ((R02 * xi0 + R12 * xi1) + R22 * xi2) * (s2 * s2);
    const float d0 = (R00 * t0 + R01 * t1) + R02 * t2;
    const float d1 = (R10 * t0 + R11 * t1) + R12 * t2;
    const float d2 = (R20 * t0 + R21 * t1) + R22 * t2;
    const float o = 1.f / (1.f + expf(-ox));
    const float g = gain / (1.f + expf(-100.f * (0.005f - o)));
    xyz[3 * i] = p0 + d0 * g;
    xyz[3 * i + 1] = p1 + d1 * g;
    xyz[3 * i + 2] = p2 + d2 * g;
}

void launch_cdf(int64_t P, const float* opacity, const uint8_t* dead, char* scratch, hipStream_t st) {
    const Layout L(P);
    double* bsum = (double*)(scratch + L.bsum);
    double* boff = (double*)(scratch + L.boff);
    uint32_t* bcnt = (uint32_t*)(scratch + L.bcnt);
    uint32_t* bdoff = (uint32_t*)(scratch + L.bdoff);
    hipLaunchKernelGGL(mcmc_weights_kernel, dim3((unsigned)L.nb), dim3(ROW_THREADS), 0, st, P, opacity, dead, bsum, bcnt);
    hipLaunchKernelGGL(mcmc_scan_kernel, dim3(1), dim3(MCMC_SCAN_THREADS), 0, st, (const double*)bsum, (const uint32_t*)bcnt, L.nb,
                       boff, bdoff, (Totals*)(scratch + L.totals));
    hipLaunchKernelGGL(mcmc_cdf_kernel, dim3((unsigned)L.nb), dim3(ROW_THREADS), 0, st, P, opacity, dead, (const double*)boff,
                       (const uint32_t*)bdoff, (double*)(scratch + L.cdf), (uint32_t*)(scratch + L.dead_list));
}

}  // namespace

size_t mcmc_scratch_bytes(int64_t P) { return Layout(P).total; }

// the CDF and the dead-row list into scratch; counts_host = { dead rows, rows of positive weight, 0, 0 }: the one host read
int mcmc_prepare(int64_t P, const float* opacity, const uint8_t* dead, char* scratch, int64_t* counts_host, hipStream_t st) {
    const Layout L(P);
    launch_cdf(P, opacity, dead, scratch, st);
    HIP_TRY_ERR(hipGetLastError());
    Totals host;
    HIP_TRY_ERR(hipMemcpyAsync(&host, scratch + L.totals, sizeof(host), hipMemcpyDeviceToHost, st));
    HIP_TRY_ERR(hipStreamSynchronize(st));
    counts_host[0] = (int64_t)host.n_dead;
    counts_host[1] = (int64_t)host.n_positive;
    counts_host[2] = counts_host[3] = 0;
    return MSGS_OK;
}

int mcmc_sample(int64_t P, const float* opacity, const uint8_t* dead, int64_t n, const double* u, int32_t* source, int32_t* count,
                char* scratch, hipStream_t st) {
    const Layout L(P);
    int64_t counts[4];
    if (int rc = mcmc_prepare(P, opacity, dead, scratch, counts, st)) return rc;
    if (counts[1] == 0) return MSGS_ERR_NO_WEIGHT;
    HIP_TRY_ERR(hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)P, st));
    hipLaunchKernelGGL(mcmc_draw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P, n, u,
                       (const double*)(scratch + L.cdf), source, count);
    HIP_TRY_ERR(hipGetLastError());
    return MSGS_OK;
}

int mcmc_relocate(const msgs_mcmc_relocate_t& a, char* scratch, hipStream_t st) {
    const Layout L(a.P);
    Table t{};
    t.n_slots = a.n_tensors;
    t.in_place = a.in_place != 0;
    t.P = a.P;
    t.n = a.n;
    int32_t* source = (int32_t*)(scratch + L.source);
    int32_t* count = (int32_t*)(scratch + L.count);
    float* vals = (float*)(scratch + L.vals);
    t.source = source; t.count = count; t.vals = vals;
    t.dead_list = (const uint32_t*)(scratch + L.dead_list);
    t.totals = (const Totals*)(scratch + L.totals);
    const float *opacity = nullptr, *scaling = nullptr, *max_pix = nullptr, *min_pix = nullptr;
    int wmax = 1;
    for (int k = 0; k < a.n_tensors; ++k) {
        const msgs_mcmc_tensor_t& d = a.tensors[k];
        Slot& S = t.t[k];
        S.data = d.data; S.fresh = d.fresh; S.exp_avg = d.exp_avg; S.exp_avg_sq = d.exp_avg_sq;
        S.W = d.width; S.esz = d.elem_bytes; S.rule = d.rule;
        if (d.width > wmax) wmax = d.width;
        if (d.rule == MSGS_MR_OPACITY) opacity = (const float*)d.data;
        if (d.rule == MSGS_MR_SCALE) scaling = (const float*)d.data;
        if (d.rule == MSGS_MR_PIX_MAX) max_pix = (const float*)d.data;
        if (d.rule == MSGS_MR_PIX_MIN) min_pix = (const float*)d.data;
    }
    const unsigned row_blocks = (unsigned)((a.P + 255) / 256);
    HIP_TRY_ERR(hipMemsetAsync(count, 0, sizeof(int32_t) * (size_t)a.P, st));
    hipLaunchKernelGGL(mcmc_draw_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, a.P, a.n, a.u,
                       (const double*)(scratch + L.cdf), source, count);
    hipLaunchKernelGGL(mcmc_ratio_kernel, dim3(row_blocks), dim3(256), 0, st, a.P, (const int32_t*)count, opacity, scaling, max_pix,
                       min_pix, vals);
    const uint64_t eblocks = ((uint64_t)a.n * (uint64_t)wmax + 255) / 256;
    if (eblocks > 0x7FFFFFFFull) return MSGS_ERR_TOO_MANY;
    hipLaunchKernelGGL(mcmc_rows_kernel, dim3((unsigned)eblocks, (unsigned)a.n_tensors), dim3(256), 0, st, t);
    hipLaunchKernelGGL(mcmc_sources_kernel, dim3(row_blocks), dim3(256), 0, st, t);
    HIP_TRY_ERR(hipGetLastError());
    return MSGS_OK;
}

int mcmc_check_relocate(const msgs_mcmc_relocate_t& a) {
    if (a.P < 0 || a.n < 0 || a.n_tensors < 0 || a.n_tensors > MSGS_MCMC_MAX_TENSORS || (a.n_tensors && !a.tensors))
        return MSGS_ERR_INVALID_ARG;
    if (a.P >= ((int64_t)1 << 31)) return MSGS_ERR_TOO_MANY;
    if (a.n > a.P) return MSGS_ERR_INVALID_ARG;                     // no more draws than rows: dead rows, or 5 % growth
    if (a.n > 0 && !a.u) return MSGS_ERR_INVALID_ARG;
    int n_op = 0, n_sc = 0;
    for (int k = 0; k < a.n_tensors; ++k) {
        const msgs_mcmc_tensor_t& d = a.tensors[k];
        if (d.width < 1 || d.width > 4096 || (d.elem_bytes != 1 && d.elem_bytes != 4 && d.elem_bytes != 8)) return MSGS_ERR_INVALID_ARG;
        if (d.rule < MSGS_MR_COPY || d.rule > MSGS_MR_PIX_MIN || !d.data) return MSGS_ERR_INVALID_ARG;
        if (d.elem_bytes != 4 && (d.rule > MSGS_MR_ZERO || d.exp_avg || d.exp_avg_sq)) return MSGS_ERR_INVALID_ARG;
        if ((d.rule == MSGS_MR_OPACITY || d.rule == MSGS_MR_PIX_MAX || d.rule == MSGS_MR_PIX_MIN) && d.width != 1)
            return MSGS_ERR_INVALID_ARG;
        if (d.rule == MSGS_MR_SCALE && d.width != 3) return MSGS_ERR_INVALID_ARG;
        n_op += d.rule == MSGS_MR_OPACITY;
        n_sc += d.rule == MSGS_MR_SCALE;
    }
    if (a.P > 0 && a.n > 0 && (n_op != 1 || n_sc != 1)) return MSGS_ERR_INVALID_ARG;
    return MSGS_OK;
}

hipError_t launch_mcmc_noise(int64_t P, float* xyz, const float* scaling, const float* rotation, const float* opacity,
                             const float* draws, float gain, hipStream_t st) {
    if (P == 0) return hipSuccess;
    hipLaunchKernelGGL(mcmc_noise_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, P, xyz, scaling, rotation, opacity,
                       draws, gain);
    return hipGetLastError();
}

}  // namespace msgs

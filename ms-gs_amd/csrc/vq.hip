// vq.hip — k-means vector quantisation: nearest-code search on the f32 MFMA and a deterministic centroid update (SPEC M21;
// 4.23).
//
//   vq_norms_kernel           one lane per padded code: n_k = float32(1/2 sum_d double(c_kd)^2) (double, ascending d, rounded once) and
//                             the chunk records the search streams: per VQ_CODE_CHUNK codes [2 KS rows d][64 codes] then [64 norms];
//                             rows d >= D and codes >= K are zero, padded codes get n_k = +inf
//   vq_assign_kernel<KS>      256 lanes = 4 waves x 64 points.  The codes are the A operand, -x the B operand of
//                             v_mfma_f32_32x32x2_f32: a lane holds ONE point (column lane & 31) and 16 codes of a tile (rows), so the
//                             argmin over the codes of a tile pair is a lane's own affair and the cross-lane step is one exchange with
//                             lane ^ 32 per point tile at the very end.  The accumulator is preloaded with n_k, so after KS steps it
//                             holds s(i,k) = fmaf chain over d of (-x_id) c_kd from n_k — no epilogue arithmetic.  Running
//                             (best, tile base) per accumulator element under strict <, tiles in ascending code order.
//   vq_update_partial_kernel  one lane per (chunk of VQ_UPDATE_CHUNK consecutive members of one code, column j): the double sum of
//                             w_i x_ij in member order (column D: of w_i)
//   vq_update_finish_kernel   one lane per (code, column): chunk partials added in chunk order, divided, rounded once
//
// No atomics anywhere; no order depends on the launch geometry.  fmaf(a, b, c) = fmaf(b, a, c), so which of x and c is the A operand
// cannot change a bit; the k order inside one MFMA is ascending (k = lane >> 5), so d ascends.
#include "msgs_internal.h"

#pragma clang fp contract(off)

namespace msgs {

namespace {

constexpr int CODE_CHUNK = MSGS_VQ_CODE_CHUNK;      // 64 = two 32-code tiles
constexpr int UPDATE_CHUNK = MSGS_VQ_UPDATE_CHUNK;
constexpr int ASSIGN_THREADS = 256;                 // 4 waves
constexpr int POINTS_PER_WAVE = 64;                 // two 32-point tiles
constexpr int POINTS_PER_BLOCK = 4 * POINTS_PER_WAVE;

typedef float f32x16 __attribute__((ext_vector_type(16)));

static_assert(CODE_CHUNK == 64, "vq_assign_kernel multiplies one chunk as two 32-code tiles");

// k-steps of the kernel instance that serves D columns: 8, 16, 24 or 32 (a zero step leaves the chain's value: fmaf(0, 0, s) = s)
inline int vq_ksteps(int D) { return ((D + 15) / 16) * 8; }
inline int64_t vq_chunks(int K) { return (K + CODE_CHUNK - 1) / CODE_CHUNK; }
inline size_t vq_record_floats(int D) { return (size_t)(2 * vq_ksteps(D) + 1) * CODE_CHUNK; }

// row of accumulator register `reg` in a 32x32 tile for lane half h (the C/D map of every 32x32 MFMA on gfx950)
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

__global__ __launch_bounds__(256) void vq_norms_kernel(int D, int K, int DP, const float* __restrict__ codebook,
                                                       float* __restrict__ records) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;          // < padded K: the grid is exact
    float* rec = records + (size_t)(k / CODE_CHUNK) * (DP + 1) * CODE_CHUNK + (k % CODE_CHUNK);
    double n = 0.0;
    for (int d = 0; d < DP; ++d) {
        const float c = (k < K && d < D) ? codebook[(size_t)k * D + d] : 0.f;
        n += (double)c * (double)c;
        rec[d * CODE_CHUNK] = c;
    }
    rec[DP * CODE_CHUNK] = k < K ? (float)(0.5 * n) : INFINITY;
}

template <int KS>
__global__ __launch_bounds__(ASSIGN_THREADS) void vq_assign_kernel(int64_t P, int D, int K, int n_chunks,
                                                                   const float* __restrict__ x,
                                                                   const float* __restrict__ codebook,
                                                                   const float4* __restrict__ records, int32_t* __restrict__ idx,
                                                                   float* __restrict__ err) {
    constexpr int DP = 2 * KS;
    constexpr int REC4 = (DP + 1) * CODE_CHUNK / 4;               // float4 per chunk record
    constexpr int NLD = (REC4 + ASSIGN_THREADS - 1) / ASSIGN_THREADS;
    __shared__ float4 lds[2][REC4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, r = lane & 31;
    const int64_t base = (int64_t)blockIdx.x * POINTS_PER_BLOCK + wave * POINTS_PER_WAVE;

    // B operand: lane l holds -x[point l & 31][d = 2 s + (l >> 5)] of either point tile, for the whole kernel
    float xf[2][KS];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int64_t p = base + t * 32 + r;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int d = 2 * s + h;
            xf[t][s] = (p < P && d < D) ? -x[p * D + d] : 0.f;
        }
    }

    float best[2][16];
    int btile[2][16];                                             // first code of the winning tile, -1: nothing has won yet
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            best[t][i] = INFINITY;
            btile[t][i] = -1;
        }

#pragma unroll
    for (int j = 0; j < NLD; ++j)
        if (j * ASSIGN_THREADS + tid < REC4) lds[0][j * ASSIGN_THREADS + tid] = records[j * ASSIGN_THREADS + tid];
    __syncthreads();

    for (int c = 0; c < n_chunks; ++c) {
        // the next chunk travels while this one is multiplied; it lands in the other buffer, which every wave left at the last barrier
        float4 next[NLD];
        const bool more = c + 1 < n_chunks;
        if (more) {
            const float4* src = records + (size_t)(c + 1) * REC4;
#pragma unroll
            for (int j = 0; j < NLD; ++j)
                if (j * ASSIGN_THREADS + tid < REC4) next[j] = src[j * ASSIGN_THREADS + tid];
        }

        const float* B = reinterpret_cast<const float*>(lds[c & 1]);
        f32x16 acc[2][2];                                         // [code tile][point tile]
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 n = *reinterpret_cast<const float4*>(B + DP * CODE_CHUNK + ct * 32 + 8 * g + 4 * h);
                acc[ct][0][4 * g + 0] = n.x, acc[ct][0][4 * g + 1] = n.y, acc[ct][0][4 * g + 2] = n.z, acc[ct][0][4 * g + 3] = n.w;
                acc[ct][1][4 * g + 0] = n.x, acc[ct][1][4 * g + 1] = n.y, acc[ct][1][4 * g + 2] = n.z, acc[ct][1][4 * g + 3] = n.w;
            }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            // A operand: lane l holds c[code l & 31][d = 2 s + (l >> 5)]: 32 consecutive words per lane half, conflict-free
            const float a0 = B[(2 * s + h) * CODE_CHUNK + r];
            const float a1 = B[(2 * s + h) * CODE_CHUNK + 32 + r];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, xf[0][s], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, xf[1][s], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, xf[0][s], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, xf[1][s], acc[1][1], 0, 0, 0);
        }
        // an element sees its codes in ascending order, so strict < keeps the lowest index of a tie; a NaN never compares less
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int tile = c * CODE_CHUNK + ct * 32;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float sc = acc[ct][t][i];
                    const bool wins = sc < best[t][i];
                    best[t][i] = wins ? sc : best[t][i];
                    btile[t][i] = wins ? tile : btile[t][i];
                }
        }

        if (more) {
            float4* dst = lds[(c + 1) & 1];
#pragma unroll
            for (int j = 0; j < NLD; ++j)
                if (j * ASSIGN_THREADS + tid < REC4) dst[j * ASSIGN_THREADS + tid] = next[j];
        }
        __syncthreads();
    }

    // (score, index) lexicographically: over the lane's 16 elements, then with the other half of the rows in lane ^ 32
    int winner[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        float bs = INFINITY;
        int bi = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float sc = best[t][i];
            const int k = btile[t][i] < 0 ? 0 : btile[t][i] + acc_row(i, h);
            if (sc < bs || (sc == bs && k < bi)) bs = sc, bi = k;
        }
        const float os = __shfl_xor(bs, 32);
        const int oi = __shfl_xor(bi, 32);
        if (os < bs || (os == bs && oi < bi)) bi = oi;
        winner[t] = bi;
    }

    // lane l finishes point base + l: the index once, and the error from the two rows
    const int64_t p = base + lane;
    if (p >= P) return;
    const int k = h ? winner[1] : winner[0];
    idx[p] = k;
    if (err) {
        const float* xr = x + p * D;
        const float* cr = codebook + (size_t)k * D;
        float e = 0.f;
        for (int d = 0; d < D; ++d) {
            const float t = xr[d] - cr[d];
            e = fmaf(t, t, e);
        }
        err[p] = e;
    }
}

// the code of a chunk: the largest k with chunk_offsets[k] <= chunk (empty codes share an offset with their successor)
__device__ __forceinline__ int code_of_chunk(const int32_t* __restrict__ chunk_offsets, int K, int chunk) {
    int lo = 0, hi = K;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_offsets[mid] <= chunk) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void vq_update_partial_kernel(int D, int K, int64_t n_lanes, const float* __restrict__ x,
                                                                const float* __restrict__ w, const int64_t* __restrict__ order,
                                                                const int32_t* __restrict__ offsets,
                                                                const int32_t* __restrict__ chunk_offsets,
                                                                double* __restrict__ partial) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_lanes) return;
    const int chunk = (int)(g / (D + 1)), j = (int)(g % (D + 1));
    if (chunk >= chunk_offsets[K]) return;
    const int k = code_of_chunk(chunk_offsets, K, chunk);
    const int64_t m0 = (int64_t)offsets[k] + (int64_t)(chunk - chunk_offsets[k]) * UPDATE_CHUNK;
    const int64_t end = offsets[k + 1];
    const int64_t m1 = m0 + UPDATE_CHUNK < end ? m0 + UPDATE_CHUNK : end;
    double acc = 0.0;
    for (int64_t m = m0; m < m1; ++m) {
        const int64_t i = order[m];
        const double wi = w ? (double)w[i] : 1.0;
        acc += j < D ? wi * (double)x[i * D + j] : wi;            // the product of two float32 is exact in double
    }
    partial[g] = acc;
}

__global__ __launch_bounds__(256) void vq_update_finish_kernel(int D, int K, const int32_t* __restrict__ offsets,
                                                               const int32_t* __restrict__ chunk_offsets,
                                                               const double* __restrict__ partial, const float* codebook,
                                                               float* new_codebook, double* __restrict__ mass,
                                                               int32_t* __restrict__ count) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (int64_t)K * (D + 1)) return;
    const int k = (int)(g / (D + 1)), j = (int)(g % (D + 1));
    const int c0 = chunk_offsets[k], c1 = chunk_offsets[k + 1];
    double sum = 0.0, m = 0.0;
    for (int c = c0; c < c1; ++c) {
        sum += partial[(int64_t)c * (D + 1) + j];
        m += partial[(int64_t)c * (D + 1) + D];
    }
    if (j == D) {
        mass[k] = m;
        count[k] = offsets[k + 1] - offsets[k];
    } else {
        const float old = codebook[(size_t)k * D + j];
        new_codebook[(size_t)k * D + j] = m > 0.0 ? (float)(sum / m) : old;
    }
}

template <int KS>
void launch_assign(int64_t P, int D, int K, const float* x, const float* codebook, const float* records, int32_t* idx, float* err,
                   hipStream_t s) {
    const dim3 grid((unsigned)((P + POINTS_PER_BLOCK - 1) / POINTS_PER_BLOCK)), block(ASSIGN_THREADS);
    hipLaunchKernelGGL(vq_assign_kernel<KS>, grid, block, 0, s, P, D, K, (int)vq_chunks(K), x, codebook,
                       reinterpret_cast<const float4*>(records), idx, err);
}

}  // namespace

size_t vq_assign_scratch_bytes(int D, int K) { return (size_t)vq_chunks(K) * vq_record_floats(D) * sizeof(float); }

size_t vq_update_scratch_bytes(int64_t P, int D, int K) {
    return (size_t)(P / UPDATE_CHUNK + K) * (size_t)(D + 1) * sizeof(double);
}

hipError_t launch_vq_assign(int64_t P, int D, int K, const float* x, const float* codebook, int32_t* idx, float* err, char* scratch,
                            hipStream_t s) {
    float* records = reinterpret_cast<float*>(scratch);
    const int KS = vq_ksteps(D);
    hipLaunchKernelGGL(vq_norms_kernel, dim3((unsigned)(vq_chunks(K) * CODE_CHUNK / 64)), dim3(64), 0, s, D, K, 2 * KS, codebook,
                       records);
    switch (KS) {
        case 8: launch_assign<8>(P, D, K, x, codebook, records, idx, err, s); break;
        case 16: launch_assign<16>(P, D, K, x, codebook, records, idx, err, s); break;
        case 24: launch_assign<24>(P, D, K, x, codebook, records, idx, err, s); break;
        default: launch_assign<32>(P, D, K, x, codebook, records, idx, err, s); break;
    }
    return hipGetLastError();
}

hipError_t launch_vq_update(int64_t P, int D, int K, const float* x, const float* w, const int64_t* order, const int32_t* offsets,
                            const int32_t* chunk_offsets, const float* codebook, float* new_codebook, double* mass, int32_t* count,
                            char* scratch, hipStream_t s) {
    double* partial = reinterpret_cast<double*>(scratch);
    const int64_t n_lanes = (P / UPDATE_CHUNK + K) * (int64_t)(D + 1);       // an upper bound of the chunk count, times the columns
    hipLaunchKernelGGL(vq_update_partial_kernel, dim3((unsigned)((n_lanes + 255) / 256)), dim3(256), 0, s, D, K, n_lanes, x, w, order,
                       offsets, chunk_offsets, partial);
    const int64_t n_out = (int64_t)K * (D + 1);
    hipLaunchKernelGGL(vq_update_finish_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, D, K, offsets, chunk_offsets,
                       (const double*)partial, codebook, new_codebook, mass, count);
    return hipGetLastError();
}

}  // namespace msgs

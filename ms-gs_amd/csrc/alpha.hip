// alpha.hip — the two image-sized kernels of SPEC M9 that touch no Gaussian:
//   * alpha_map_kernel: A = 1 - final_T, the accumulated opacity of every pixel, from the transmittance the forward left in the
//     image state (one float32 subtraction per pixel; the blend kernels are not involved);
//   * bg_grad_partial_kernel + bg_grad_finish_kernel: dL/dbg_c = sum_p final_T_p dL/dC_{c,p}.  Every product is rounded to
//     float32 and added in DOUBLE; the partition of the pixels over lanes, waves and workgroups depends on N alone, the wave and
//     workgroup reductions are fixed trees and the second launch adds the workgroups' rows in index order: no atomics, the same
//     bits on every run (the pattern of the camera-gradient rows, preprocess.hip).
// Both stream: 16-byte accesses where the base addresses (and, for the three dL/dC planes, N) allow, scalar accesses otherwise —
// the same elements in the same order either way, so the alignment of a caller's buffer never changes a bit of the result.
#include "msgs_internal.h"

namespace msgs {

namespace {

constexpr int AM_THREADS = 256;
constexpr int AM_MAX_BLOCKS = 2048;           // 8 workgroups per CU: a grid-stride loop beyond that

// VEC: final_T and out are 16-byte aligned — n4 = N / 4 float4 words, then a scalar tail of N % 4 (N may be odd);
// !VEC: n4 = 0, every element is "tail"
__global__ __launch_bounds__(AM_THREADS) void alpha_map_kernel(const float* __restrict__ final_T, float* __restrict__ out,
                                                               size_t n4, size_t N) {
    const size_t stride = (size_t)gridDim.x * AM_THREADS;
    const size_t t = (size_t)blockIdx.x * AM_THREADS + threadIdx.x;
    const float4* src = reinterpret_cast<const float4*>(final_T);
    float4* dst = reinterpret_cast<float4*>(out);
    for (size_t i = t; i < n4; i += stride) {
        const float4 v = src[i];
        dst[i] = make_float4(1.0f - v.x, 1.0f - v.y, 1.0f - v.z, 1.0f - v.w);
    }
    for (size_t i = 4 * n4 + t; i < N; i += stride) out[i] = 1.0f - final_T[i];
}

// ---- background gradient ----
// A lane owns GROUPS of four consecutive pixels (group g = its global thread index + k * threads of the grid) and adds the four
// products of a group in pixel order, whether they arrived as one 16-byte load or as four scalar ones.
constexpr int BG_THREADS = 256;
constexpr int BG_MAX_BLOCKS = 256;            // rows the second launch adds (one workgroup per CU)
constexpr int BG_GROUPS_PER_THREAD = 4;       // a workgroup more for every 4096 pixels, up to BG_MAX_BLOCKS

inline int bg_blocks(size_t N) {
    const size_t groups = (N + 3) / 4;
    const size_t per_block = (size_t)BG_THREADS * BG_GROUPS_PER_THREAD;
    const size_t b = (groups + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > (size_t)BG_MAX_BLOCKS ? (size_t)BG_MAX_BLOCKS : b));
}

// four consecutive floats of p from element i (i % 4 == 0); elements at or beyond N read as zero
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* __restrict__ p, size_t i, size_t N) {
    if (VEC && i + 4 <= N) return *reinterpret_cast<const float4*>(p + i);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < N) v.x = p[i];
    if (i + 1 < N) v.y = p[i + 1];
    if (i + 2 < N) v.z = p[i + 2];
    if (i + 3 < N) v.w = p[i + 3];
    return v;
}

// HAS_T = false (no image state: P = 0, nothing was blended): final_T = 1 everywhere
template <bool HAS_T, bool VEC>
__global__ __launch_bounds__(BG_THREADS) void bg_grad_partial_kernel(const float* __restrict__ final_T,
                                                                     const float* __restrict__ dL_dcolor, size_t N,
                                                                     double* __restrict__ rows) {
    __shared__ double s_part[BG_THREADS / 64][3];
    const size_t groups = (N + 3) / 4;
    const size_t stride = (size_t)gridDim.x * BG_THREADS;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (size_t g = (size_t)blockIdx.x * BG_THREADS + threadIdx.x; g < groups; g += stride) {
        const size_t i = 4 * g;
        const float4 T = HAS_T ? load4<VEC>(final_T, i, N) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 d0 = load4<VEC>(dL_dcolor, i, N), d1 = load4<VEC>(dL_dcolor + N, i, N), d2 = load4<VEC>(dL_dcolor + 2 * N, i, N);
        // (a product is rounded to float32 before it is widened: __fmul_rn is never contracted into the addition)
        a0 += (double)__fmul_rn(T.x, d0.x); a0 += (double)__fmul_rn(T.y, d0.y); a0 += (double)__fmul_rn(T.z, d0.z); a0 += (double)__fmul_rn(T.w, d0.w);
        a1 += (double)__fmul_rn(T.x, d1.x); a1 += (double)__fmul_rn(T.y, d1.y); a1 += (double)__fmul_rn(T.z, d1.z); a1 += (double)__fmul_rn(T.w, d1.w);
        a2 += (double)__fmul_rn(T.x, d2.x); a2 += (double)__fmul_rn(T.y, d2.y); a2 += (double)__fmul_rn(T.z, d2.z); a2 += (double)__fmul_rn(T.w, d2.w);
    }
    a0 = wave_sum_f64(a0); a1 = wave_sum_f64(a1); a2 = wave_sum_f64(a2);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s_part[w][0] = a0; s_part[w][1] = a1; s_part[w][2] = a2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        rows[3 * (size_t)blockIdx.x + c] = ((s_part[0][c] + s_part[1][c]) + s_part[2][c]) + s_part[3][c];
    }
}
static_assert(BG_THREADS == 256, "bg_grad_partial_kernel adds four waves");

// one workgroup: lane c adds the rows' component c in index order
__global__ __launch_bounds__(64) void bg_grad_finish_kernel(const double* __restrict__ rows, int n_rows, float* __restrict__ dL_dbg) {
    const int c = threadIdx.x;
    if (c >= 3) return;
    double acc = 0.0;
    for (int r = 0; r < n_rows; ++r) acc += rows[3 * (size_t)r + c];
    dL_dbg[c] = (float)acc;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

hipError_t launch_alpha_map(const float* final_T, float* out_alpha, size_t N, hipStream_t s) {
    if (N == 0) return hipSuccess;
    const size_t n4 = aligned16(final_T) && aligned16(out_alpha) ? N / 4 : 0;
    const size_t work = n4 ? n4 + 3 : N;          // (the tail is at most three elements)
    const size_t blocks = (work + AM_THREADS - 1) / AM_THREADS;
    const int grid = (int)(blocks > (size_t)AM_MAX_BLOCKS ? (size_t)AM_MAX_BLOCKS : blocks);
    hipLaunchKernelGGL(alpha_map_kernel, dim3(grid), dim3(AM_THREADS), 0, s, final_T, out_alpha, n4, N);
    return hipGetLastError();
}

size_t bg_grad_rows_bytes(size_t N) { return 3 * sizeof(double) * (size_t)bg_blocks(N); }

hipError_t launch_bg_grad(const float* final_T, const float* dL_dcolor, size_t N, float* dL_dbg, double* rows, hipStream_t s) {
    const int blocks = bg_blocks(N);
    // the planes dL/dC_1, dL/dC_2 start N and 2 N floats behind the base: 16-byte loads need N % 4 == 0 as well
    const bool vec = aligned16(dL_dcolor) && N % 4 == 0 && (!final_T || aligned16(final_T));
    with_bool(final_T != nullptr, [&](auto HAS_T) { with_bool(vec, [&](auto VEC) {
        hipLaunchKernelGGL((bg_grad_partial_kernel<decltype(HAS_T)::value, decltype(VEC)::value>), dim3(blocks), dim3(BG_THREADS), 0, s,
                           final_T, dL_dcolor, N, rows);
    }); });
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bg_grad_finish_kernel, dim3(1), dim3(64), 0, s, (const double*)rows, blocks, dL_dbg);
    return hipGetLastError();
}

}  // namespace msgs

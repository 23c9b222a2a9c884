// filter3d.hip — opt-in 3-D smoothing filter of Mip-Splatting (SPEC M16; 4.17).
//
//   filter3d_sweep_kernel               per Gaussian, over a set of V cameras: is it seen at all, and at which highest sampling
//                                       rate nu (pixels per world unit)?  plus the smallest nu of the seen Gaussians (one integer
//                                       atomic min per workgroup on the bits of the positive float)
//   filter3d_finish_kernel              filter_3D = sqrt(variance) / nu; a Gaussian no camera sees takes the smallest nu, i.e.
//                                       the largest filter; nobody seen: 0 everywhere (the filter is the identity)
//   smoothing_filter_forward_kernel     s_eff_k = sqrt(s_k^2 + f^2),  o_eff = o r_0 r_1 r_2,  r_k = s_k / s_eff_k
//   smoothing_filter_backward_kernel    dL/ds, dL/do from dL/ds_eff, dL/do_eff;  <RAW>: log-scales and logits in, their
//                                       gradients out (the exp and the sigmoid of the model's getters evaluated here)
//
// A filtered render is the plain render of the same model with (s_eff, o_eff) in the place of the scales and the opacity:
// K1, K9 and the blend kernels are not touched.  Camera n sees the centre p iff, with t = view_point(p, M_n) (restated from
// preprocess.hip operation for operation, contraction OFF) and zc = max(t.z, 0.001),
//     t.z > 0.2,   -0.15 W <= t.x / zc fx + W / 2 <= 1.15 W,   -0.15 H <= t.y / zc fy + H / 2 <= 1.15 H
// (a NaN or Inf anywhere: every comparison is false).  Both rules come from one sweep: a lane keeps max fx / t.z and min t.z
// over the cameras that see it, and the largest fx of ALL cameras is the same in every lane.  Min and max do not depend on
// the order, so the result has the same bits whatever the grid.
//
// The sweep is one lane per Gaussian with the centre in registers; the camera rows (20 floats: M, fx, fy, W, H) are staged in
// LDS FILTER3D_CAMERA_CHUNK at a time and read back as broadcasts.  The two getter kernels are streaming kernels, one lane per
// Gaussian: 20 B in / 16 B out forward, 36 B in / 16 B out backward.
#include "msgs_internal.h"

#pragma clang fp contract(off)

namespace msgs {

namespace {

constexpr int CAM_F = MSGS_FILTER3D_CAMERA_FLOATS;
constexpr int CHUNK = MSGS_FILTER3D_CAMERA_CHUNK;
constexpr uint32_t NO_MIN = 0xFFFFFFFFu;      // the fallback word before any seen Gaussian: above the bits of every float

// = preprocess.hip
__device__ __forceinline__ void view_point(const float* V, const float* p, float* t) {
    t[0] = ((V[0] * p[0] + V[4] * p[1]) + V[8] * p[2]) + V[12];
    t[1] = ((V[1] * p[0] + V[5] * p[1]) + V[9] * p[2]) + V[13];
    t[2] = ((V[2] * p[0] + V[6] * p[1]) + V[10] * p[2]) + V[14];
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off));
    return v;
}

// nu [P]: the sampling rate of a seen Gaussian, 0 otherwise (the finish kernel turns it into the filter in place);
// valid [P]: 1 / 0;  fallback[0]: min over the seen Gaussians of the bits of nu (NO_MIN at entry)
__global__ __launch_bounds__(256) void filter3d_sweep_kernel(int P, const float* __restrict__ means3D, int V,
                                                             const float* __restrict__ cameras, int rule,
                                                             float* __restrict__ nu_out, uint8_t* __restrict__ valid,
                                                             uint32_t* __restrict__ fallback) {
    __shared__ float s_cam[CHUNK * CAM_F];
    __shared__ uint32_t s_min[4];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in_range = i < P;
    float p[3] = {0.f, 0.f, 0.f};
    if (in_range) { p[0] = means3D[3 * (size_t)i]; p[1] = means3D[3 * (size_t)i + 1]; p[2] = means3D[3 * (size_t)i + 2]; }
    float max_rate = 0.f;                     // max over the seeing cameras of fx / t.z
    float min_z = INFINITY;                   // min over the seeing cameras of t.z
    float max_fx = 0.f;                       // max over ALL cameras of fx
    bool seen = false;
    for (int c0 = 0; c0 < V; c0 += CHUNK) {
        const int nc = min(CHUNK, V - c0);
        __syncthreads();                      // the previous chunk has been read
        for (int k = threadIdx.x; k < nc * CAM_F; k += blockDim.x) s_cam[k] = cameras[(size_t)c0 * CAM_F + k];
        __syncthreads();
        for (int n = 0; n < nc; ++n) {
            const float* cam = s_cam + n * CAM_F;
            const float fx = cam[16], fy = cam[17], W = cam[18], H = cam[19];
            max_fx = fmaxf(max_fx, fx);
            float t[3];
            view_point(cam, p, t);
            const float zc = fmaxf(t[2], 0.001f);
            const float x = (t[0] / zc) * fx + W / 2.0f;
            const float y = (t[1] / zc) * fy + H / 2.0f;
            const bool ok = t[2] > 0.2f && x >= -0.15f * W && x <= 1.15f * W && y >= -0.15f * H && y <= 1.15f * H;
            if (ok) {
                seen = true;
                max_rate = fmaxf(max_rate, fx / t[2]);
                min_z = fminf(min_z, t[2]);
            }
        }
    }
    const float nu = rule == MSGS_FILTER3D_RULE_MIP_SPLATTING ? max_fx / min_z : max_rate;
    // only a positive, finite rate is a sampling rate (a camera row with a non-finite or non-positive focal length gives none)
    seen = in_range && seen && nu > 0.f && nu < INFINITY;
    if (in_range) {
        nu_out[i] = seen ? nu : 0.f;
        valid[i] = seen ? 1 : 0;
    }
    const uint32_t m = wave_min_u32(seen ? __float_as_uint(nu) : NO_MIN);
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t b = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
        if (b != NO_MIN) atomicMin(fallback, b);
    }
}

// in place: filter[i] holds nu (0: not seen) and receives sqrt(variance) / nu
__global__ __launch_bounds__(256) void filter3d_finish_kernel(int P, float sd, const uint32_t* __restrict__ fallback,
                                                              float* __restrict__ filter) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint32_t fb = fallback[0];
    const float nu = filter[i];
    float f = 0.f;                            // nobody is seen: the identity
    if (nu > 0.f) f = sd / nu;
    else if (fb != NO_MIN) f = sd / __uint_as_float(fb);
    filter[i] = f;
}

// = preprocess.hip's act_scales / act_opacity (raw_params == 1): torch.exp, torch.sigmoid
template <bool RAW>
__device__ __forceinline__ void load_row(const float* __restrict__ scales, const float* __restrict__ opacities, int i, float* s,
                                         float& o) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float x = scales[3 * (size_t)i + k]; s[k] = RAW ? expf(x) : x; }
    const float x = opacities[i];
    o = RAW ? 1.0f / (1.0f + expf(-x)) : x;
}

// s_eff, r = s / s_eff and q = f / s_eff of one axis (f > 0).  s_eff >= max(s, f) up to rounding, so r, q <= 1; s_eff == 0 needs
// s^2 and f^2 to underflow together: the axis then has no extent and no gradient
__device__ __forceinline__ void axis(float s, float f, float& s_eff, float& r, float& q) {
    s_eff = sqrtf(s * s + f * f);
    const bool pos = s_eff > 0.f;
    r = pos ? s / s_eff : 0.f;
    q = pos ? f / s_eff : 0.f;
}

template <bool RAW>
__global__ __launch_bounds__(256) void smoothing_filter_forward_kernel(int P, const float* __restrict__ scales,
                                                                       const float* __restrict__ opacities,
                                                                       const float* __restrict__ filter,
                                                                       float* __restrict__ scales_eff,
                                                                       float* __restrict__ opacities_eff) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    float s[3], o;
    load_row<RAW>(scales, opacities, i, s, o);
    const float f = filter[i];
    float se[3] = {s[0], s[1], s[2]}, oe = o;
    if (f != 0.f) {                           // f == 0: the row's own bits, by selection
        float r[3], q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) axis(s[k], f, se[k], r[k], q[k]);
        oe = ((o * r[0]) * r[1]) * r[2];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) scales_eff[3 * (size_t)i + k] = se[k];
    opacities_eff[i] = oe;
}

// dL/ds_k = r_k dL/ds_eff_k + (d o_eff / d s_k) dL/do_eff,   dL/do = r_0 r_1 r_2 dL/do_eff, with
//     d o_eff / d s_k = o_eff f^2 / (s_k s_eff_k^2) = o r_j r_l q_k^2 / s_eff_k     (j, l the other two axes)
// — the second form has no s_k in a denominator: it is finite at s_k = 0, where o_eff = 0 and the first is 0 / 0.
// <RAW>: times ds/dx = s and do/dx = o (1 - o).  dL_dscales_eff / dL_dopacities_eff NULL: that output was not used (zeros).
template <bool RAW>
__global__ __launch_bounds__(256) void smoothing_filter_backward_kernel(int P, const float* __restrict__ scales,
                                                                        const float* __restrict__ opacities,
                                                                        const float* __restrict__ filter,
                                                                        const float* __restrict__ dL_dscales_eff,
                                                                        const float* __restrict__ dL_dopacities_eff,
                                                                        float* __restrict__ dL_dscales,
                                                                        float* __restrict__ dL_dopacities) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    float s[3], o;
    load_row<RAW>(scales, opacities, i, s, o);
    const float f = filter[i];
    float gs[3] = {0.f, 0.f, 0.f};
    if (dL_dscales_eff) {
#pragma unroll
        for (int k = 0; k < 3; ++k) gs[k] = dL_dscales_eff[3 * (size_t)i + k];
    }
    const float go = dL_dopacities_eff ? dL_dopacities_eff[i] : 0.f;
    float ds[3] = {gs[0], gs[1], gs[2]}, d_o = go;
    if (f != 0.f) {
        float se[3], r[3], q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) axis(s[k], f, se[k], r[k], q[k]);
        d_o = ((r[0] * r[1]) * r[2]) * go;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float others = r[(k + 1) % 3] * r[(k + 2) % 3];
            const float doe = se[k] > 0.f ? (((o * others) * q[k]) * q[k]) / se[k] : 0.f;
            ds[k] = r[k] * gs[k] + doe * go;
        }
    }
    if constexpr (RAW) {
#pragma unroll
        for (int k = 0; k < 3; ++k) ds[k] = ds[k] * s[k];
        d_o = d_o * (o * (1.0f - o));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) dL_dscales[3 * (size_t)i + k] = ds[k];
    dL_dopacities[i] = d_o;
}

}  // namespace

hipError_t launch_filter3d_sweep(int P, const float* means3D, int V, const float* cameras, int rule, float variance,
                                 float* filter_3D, uint8_t* valid, uint32_t* fallback, hipStream_t s) {
    if (P == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(fallback, 0xFF, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const dim3 grid((P + 255) / 256), block(256);
    hipLaunchKernelGGL(filter3d_sweep_kernel, grid, block, 0, s, P, means3D, V, cameras, rule, filter_3D, valid, fallback);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(filter3d_finish_kernel, grid, block, 0, s, P, sqrtf(variance), (const uint32_t*)fallback, filter_3D);
    return hipGetLastError();
}

hipError_t launch_smoothing_filter_forward(int P, bool raw, const float* scales, const float* opacities, const float* filter_3D,
                                           float* scales_eff, float* opacities_eff, hipStream_t s) {
    if (P == 0) return hipSuccess;
    const dim3 grid((P + 255) / 256), block(256);
    if (raw)
        hipLaunchKernelGGL(smoothing_filter_forward_kernel<true>, grid, block, 0, s, P, scales, opacities, filter_3D, scales_eff,
                           opacities_eff);
    else
        hipLaunchKernelGGL(smoothing_filter_forward_kernel<false>, grid, block, 0, s, P, scales, opacities, filter_3D, scales_eff,
                           opacities_eff);
    return hipGetLastError();
}

hipError_t launch_smoothing_filter_backward(int P, bool raw, const float* scales, const float* opacities, const float* filter_3D,
                                            const float* dL_dscales_eff, const float* dL_dopacities_eff, float* dL_dscales,
                                            float* dL_dopacities, hipStream_t s) {
    if (P == 0) return hipSuccess;
    const dim3 grid((P + 255) / 256), block(256);
    if (raw)
        hipLaunchKernelGGL(smoothing_filter_backward_kernel<true>, grid, block, 0, s, P, scales, opacities, filter_3D,
                           dL_dscales_eff, dL_dopacities_eff, dL_dscales, dL_dopacities);
    else
        hipLaunchKernelGGL(smoothing_filter_backward_kernel<false>, grid, block, 0, s, P, scales, opacities, filter_3D,
                           dL_dscales_eff, dL_dopacities_eff, dL_dscales, dL_dopacities);
    return hipGetLastError();
}

}  // namespace msgs

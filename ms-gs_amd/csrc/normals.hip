// normals.hip — opt-in normal maps (SPEC M17; 4.18): the two halves of a depth-normal consistency loss.
//
//   gaussian_normals_forward_kernel     per Gaussian: the shortest axis of the ellipsoid, column k of R(q), turned towards the
//                                       camera; in world space or rotated into view space.  One byte per row is kept for the
//                                       backward: k, the sign, and whether the row is valid
//   gaussian_normals_backward_kernel    dL/drotations through column k of R and through q = r / max(||r||, 1e-12) with
//                                       preprocess.hip's two branches (normalize_backward); recomputed from the quaternion
//   depth_normal_forward_kernel         per pixel: n = c / ||c||, c = u x v of the back-projected 4-neighbour stencil of a
//                                       depth map (2DGS's depth_to_normal: a fronto-parallel plane gives (0, 0, -1))
//   depth_normal_backward_kernel        dL/ddepth as a GATHER in a fixed order: every stencil centre of tile + halo 1 leaves
//                                       the four shares of its neighbours in LDS, every pixel of the tile adds up its four
//
// Both sit outside K1, K9 and the blend kernels: a render with normals is the plain render with with_features(normals).
// k: 0; s_1 < s_k: 1; s_2 < s_k: 2 (strict: ties go to the lowest index; comparisons only, so log-scales, activated scales and
// filtered scales select the same axis).  sigma = -1 iff n . (campos - p) < 0.  A row with a non-finite input or result is
// exactly (0, 0, 0) and has no gradient.  The selection, the sign and the camera are constants of the backward.
//
// Pixel (x, y) back-projects to P = (a_x z, a_y z, z), a_x = ((2 x + 1) / W - 1) tanfovx: the ray through the pixel centre of
// ndc2Pix.  u = P(x, y+1) - P(x, y-1), v = P(x+1, y) - P(x-1, y).  Valid iff 1 <= x <= W-2, 1 <= y <= H-2, the four depths are
// finite and > 0 and ||c||^2 is finite and > 0; everything else is exactly 0 and passes no gradient.  The centre's own depth
// does not enter.  With dL/dc = (g - n (n.g)) / ||c||, dL/du = v x dL/dc, dL/dv = dL/dc x u and dP/dz = (a_x, a_y, 1) the
// share of a stencil to its lower neighbour is dP/dz(x, y+1) . dL/du, to the upper one -dP/dz(x, y-1) . dL/du, to the right
// one dP/dz(x+1, y) . dL/dv and to the left one -dP/dz(x-1, y) . dL/dv.  No atomics: the same bits on every run.
#include "msgs_internal.h"

#pragma clang fp contract(off)

namespace msgs {

namespace {

constexpr int TW = MSGS_DEPTH_NORMAL_TILE_W;      // one wavefront-wide row segment
constexpr int TH = MSGS_DEPTH_NORMAL_TILE_H;      // 256 threads: TH / 4 pixels each
static_assert(TW == 64 && TH % 4 == 0, "a wave per row segment, 4 rows per pass");

constexpr uint8_t FLAG_AXIS = 3, FLAG_NEG = 4, FLAG_VALID = 8;

__device__ __forceinline__ bool finite3(const float* a) { return isfinite(a[0]) && isfinite(a[1]) && isfinite(a[2]); }

// column k of R(q), q = (r, x, y, z): build_rotation of the reference, the R of Sigma = R S^2 R^T
__device__ __forceinline__ void rot_column(int k, const float* q, float* n) {
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    if (k == 0) {
        n[0] = 1.f - 2.f * (y * y + z * z); n[1] = 2.f * (x * y + r * z); n[2] = 2.f * (x * z - r * y);
    } else if (k == 1) {
        n[0] = 2.f * (x * y - r * z); n[1] = 1.f - 2.f * (x * x + z * z); n[2] = 2.f * (y * z + r * x);
    } else {
        n[0] = 2.f * (x * z + r * y); n[1] = 2.f * (y * z - r * x); n[2] = 1.f - 2.f * (x * x + y * y);
    }
}

// dL/dq from a = dL/dn, n = column k of R(q)
__device__ __forceinline__ void rot_column_backward(int k, const float* q, const float* a, float* dq) {
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    if (k == 0) {
        dq[0] = 2.f * (z * a[1] - y * a[2]);
        dq[1] = 2.f * (y * a[1] + z * a[2]);
        dq[2] = 2.f * ((x * a[1] - r * a[2]) - 2.f * (y * a[0]));
        dq[3] = 2.f * ((r * a[1] + x * a[2]) - 2.f * (z * a[0]));
    } else if (k == 1) {
        dq[0] = 2.f * (x * a[2] - z * a[0]);
        dq[1] = 2.f * ((y * a[0] + r * a[2]) - 2.f * (x * a[1]));
        dq[2] = 2.f * (x * a[0] + z * a[2]);
        dq[3] = 2.f * ((y * a[2] - r * a[0]) - 2.f * (z * a[1]));
    } else {
        dq[0] = 2.f * (y * a[0] - x * a[1]);
        dq[1] = 2.f * ((z * a[0] - r * a[1]) - 2.f * (x * a[2]));
        dq[2] = 2.f * ((r * a[0] + z * a[1]) - 2.f * (y * a[2]));
        dq[3] = 2.f * (x * a[0] + y * a[1]);
    }
}

// = preprocess.hip's act_rotation for raw quaternions: q = raw / max(||raw||, 1e-12); returns ||raw|| before the clamp
__device__ __forceinline__ float normalize_quaternion(const float4 r4, float* q) {
    q[0] = r4.x; q[1] = r4.y; q[2] = r4.z; q[3] = r4.w;
    const float rn = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float n = fmaxf(rn, 1e-12f);
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = q[k] / n;
    return rn;
}

// 40 B in, 12 B + 1 B out per row
template <bool WORLD>
__global__ __launch_bounds__(256) void gaussian_normals_forward_kernel(int P, const float* __restrict__ means3D,
                                                                       const float* __restrict__ scales,
                                                                       const float* __restrict__ rotations,
                                                                       const float* __restrict__ viewmatrix,
                                                                       const float* __restrict__ campos,
                                                                       float* __restrict__ normals, uint8_t* __restrict__ flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    float p[3], s[3], q[4];
#pragma unroll
    for (int k = 0; k < 3; ++k) { p[k] = means3D[3 * (size_t)i + k]; s[k] = scales[3 * (size_t)i + k]; }
    const float4 r4 = reinterpret_cast<const float4*>(rotations)[i];
    int k = 0;
    if (s[1] < s[k]) k = 1;
    if (s[2] < s[k]) k = 2;
    normalize_quaternion(r4, q);
    float n[3];
    rot_column(k, q, n);
    const float d[3] = {campos[0] - p[0], campos[1] - p[1], campos[2] - p[2]};
    const float facing = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
    const bool neg = facing < 0.f;
    float o[3];
    if constexpr (WORLD) {
        o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (n[0] * viewmatrix[c] + n[1] * viewmatrix[4 + c]) + n[2] * viewmatrix[8 + c];
    }
    if (neg) { o[0] = -o[0]; o[1] = -o[1]; o[2] = -o[2]; }
    const bool in_ok = finite3(p) && finite3(s) && isfinite(r4.x) && isfinite(r4.y) && isfinite(r4.z) && isfinite(r4.w);
    const bool ok = in_ok && isfinite(facing) && finite3(o);
#pragma unroll
    for (int c = 0; c < 3; ++c) normals[3 * (size_t)i + c] = ok ? o[c] : 0.f;
    flags[i] = ok ? (uint8_t)(k | (neg ? FLAG_NEG : 0) | FLAG_VALID) : (uint8_t)0;
}

// 29 B in, 16 B out per row
template <bool WORLD>
__global__ __launch_bounds__(256) void gaussian_normals_backward_kernel(int P, const float* __restrict__ rotations,
                                                                        const uint8_t* __restrict__ flags,
                                                                        const float* __restrict__ viewmatrix,
                                                                        const float* __restrict__ dL_dnormals,
                                                                        float* __restrict__ dL_drotations) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const uint8_t f = flags[i];
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (f & FLAG_VALID) {
        const float4 r4 = reinterpret_cast<const float4*>(rotations)[i];
        float g[3], q[4], a[3], dq[4];
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = dL_dnormals[3 * (size_t)i + c];
        if (f & FLAG_NEG) { g[0] = -g[0]; g[1] = -g[1]; g[2] = -g[2]; }
        if constexpr (WORLD) {
            a[0] = g[0]; a[1] = g[1]; a[2] = g[2];
        } else {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                a[j] = (g[0] * viewmatrix[4 * j] + g[1] * viewmatrix[4 * j + 1]) + g[2] * viewmatrix[4 * j + 2];
        }
        const float rn = normalize_quaternion(r4, q);
        rot_column_backward(f & FLAG_AXIS, q, a, dq);
        // = preprocess.hip's normalize_backward: no gradient through the norm where the clamp is active
        const float nrm = fmaxf(rn, 1e-12f);
        const float dotq = rn < 1e-12f ? 0.f : ((q[0] * dq[0] + q[1] * dq[1]) + q[2] * dq[2]) + q[3] * dq[3];
        out = make_float4((dq[0] - q[0] * dotq) / nrm, (dq[1] - q[1] * dotq) / nrm, (dq[2] - q[2] * dotq) / nrm,
                          (dq[3] - q[3] * dotq) / nrm);
    }
    reinterpret_cast<float4*>(dL_drotations)[i] = out;
}

// ---- depth to normal ----
struct Rays {               // a_x = ((2 x + 1) / W - 1) tanfovx, a_y likewise
    float W, H, tx, ty;
    __device__ __forceinline__ float ax(int x) const { return ((2.0f * (float)x + 1.0f) / W - 1.0f) * tx; }
    __device__ __forceinline__ float ay(int y) const { return ((2.0f * (float)y + 1.0f) / H - 1.0f) * ty; }
};

// the depth of tile + halo into LDS, 0 (a hole) outside the image: rows of TW + 2 HALO consecutive floats
// ... and the ray slopes of its columns and rows (s_ax [TW + 2 HALO], s_ay [TH + 2 HALO]): one division per column and row of
// the tile instead of six per stencil
template <int HALO>
__device__ __forceinline__ void stage_depth(const float* __restrict__ depth, int W, int H, int x0, int y0, const Rays& r,
                                            float* s_z, float* s_ax, float* s_ay) {
    constexpr int LW = TW + 2 * HALO, LH = TH + 2 * HALO;
    static_assert(LW + LH <= 256, "one pass");
    if (threadIdx.x < LW) s_ax[threadIdx.x] = r.ax(x0 - HALO + (int)threadIdx.x);
    else if (threadIdx.x < LW + LH) s_ay[threadIdx.x - LW] = r.ay(y0 - HALO + (int)threadIdx.x - LW);
    for (int e = threadIdx.x; e < LW * LH; e += 256) {
        const int ly = e / LW, lx = e - ly * LW;
        const int gx = x0 - HALO + lx, gy = y0 - HALO + ly;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        s_z[e] = in ? depth[(size_t)gy * W + gx] : 0.f;
    }
}

__device__ __forceinline__ bool depth_ok(float z) { return isfinite(z) && z > 0.f; }

// the stencil of centre (x, y) from its four depths and the slopes of its three columns (ax[-1 .. 1]) and rows (ay[-1 .. 1]):
// u, v, c = u x v, ||c||^2; false: no normal here
__device__ __forceinline__ bool stencil(int W, int H, int x, int y, const float* ax3, const float* ay3, float z_up, float z_dn,
                                        float z_lf, float z_rt, float* u, float* v, float* c, float& cc) {
    const float ax = ax3[0], ay = ay3[0];
    const float ay_up = ay3[-1], ay_dn = ay3[1], ax_lf = ax3[-1], ax_rt = ax3[1];
    u[0] = ax * z_dn - ax * z_up; u[1] = ay_dn * z_dn - ay_up * z_up; u[2] = z_dn - z_up;
    v[0] = ax_rt * z_rt - ax_lf * z_lf; v[1] = ay * z_rt - ay * z_lf; v[2] = z_rt - z_lf;
    c[0] = u[1] * v[2] - u[2] * v[1];
    c[1] = u[2] * v[0] - u[0] * v[2];
    c[2] = u[0] * v[1] - u[1] * v[0];
    cc = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
    const bool inside = x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2;
    return inside && depth_ok(z_up) && depth_ok(z_dn) && depth_ok(z_lf) && depth_ok(z_rt) && isfinite(cc) && cc > 0.f;
}

// view -> world: w_j = sum_k V[4 j + k] n_k (the transpose of the rotation that takes world to view)
__device__ __forceinline__ void to_world(const float* __restrict__ V, const float* n, float* w) {
#pragma unroll
    for (int j = 0; j < 3; ++j) w[j] = (V[4 * j] * n[0] + V[4 * j + 1] * n[1]) + V[4 * j + 2] * n[2];
}

// 4 N in, 12 N out
template <bool WORLD>
__global__ __launch_bounds__(256) void depth_normal_forward_kernel(int W, int H, float tanfovx, float tanfovy,
                                                                   const float* __restrict__ depth,
                                                                   const float* __restrict__ viewmatrix,
                                                                   float* __restrict__ normal) {
    constexpr int LW = TW + 2;
    __shared__ float s_z[LW * (TH + 2)], s_ax[LW], s_ay[TH + 2];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const Rays r{(float)W, (float)H, tanfovx, tanfovy};
    stage_depth<1>(depth, W, H, x0, y0, r, s_z, s_ax, s_ay);
    __syncthreads();
    const size_t N = (size_t)W * H;
    const int lx = threadIdx.x & (TW - 1);
    for (int ly = threadIdx.x / TW; ly < TH; ly += 256 / TW) {
        const int x = x0 + lx, y = y0 + ly;
        const float* z = s_z + (ly + 1) * LW + (lx + 1);
        float u[3], v[3], c[3], cc;
        const bool ok = stencil(W, H, x, y, s_ax + lx + 1, s_ay + ly + 1, z[-LW], z[LW], z[-1], z[1], u, v, c, cc);
        float n[3] = {0.f, 0.f, 0.f};
        if (ok) {
            const float len = sqrtf(cc);
            float nv[3] = {c[0] / len, c[1] / len, c[2] / len};
            if constexpr (WORLD) to_world(viewmatrix, nv, n);
            else { n[0] = nv[0]; n[1] = nv[1]; n[2] = nv[2]; }
        }
        if (x < W && y < H) {
            const size_t at = (size_t)y * W + x;
            normal[at] = n[0]; normal[N + at] = n[1]; normal[2 * N + at] = n[2];
        }
    }
}

// 16 N in, 4 N out
template <bool WORLD>
__global__ __launch_bounds__(256) void depth_normal_backward_kernel(int W, int H, float tanfovx, float tanfovy,
                                                                    const float* __restrict__ depth,
                                                                    const float* __restrict__ viewmatrix,
                                                                    const float* __restrict__ dL_dnormal,
                                                                    float* __restrict__ dL_ddepth) {
    constexpr int LW = TW + 4;                    // depth: halo 2
    constexpr int CW = TW + 2, CH = TH + 2;       // stencil centres: halo 1
    __shared__ float s_z[LW * (TH + 4)], s_ax[LW], s_ay[TH + 4];
    __shared__ float s_up[CW * CH], s_dn[CW * CH], s_lf[CW * CH], s_rt[CW * CH];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const Rays r{(float)W, (float)H, tanfovx, tanfovy};
    stage_depth<2>(depth, W, H, x0, y0, r, s_z, s_ax, s_ay);
    __syncthreads();
    const size_t N = (size_t)W * H;
    for (int e = threadIdx.x; e < CW * CH; e += 256) {
        const int cy = e / CW, cx = e - cy * CW;
        const int x = x0 - 1 + cx, y = y0 - 1 + cy;
        const float* z = s_z + (cy + 1) * LW + (cx + 1);
        float u[3], v[3], c[3], cc;
        const float *ax3 = s_ax + cx + 1, *ay3 = s_ay + cy + 1;
        const bool ok = stencil(W, H, x, y, ax3, ay3, z[-LW], z[LW], z[-1], z[1], u, v, c, cc);
        float up = 0.f, dn = 0.f, lf = 0.f, rt = 0.f;
        if (ok) {                                 // (inside the image: the loads below are in bounds)
            const size_t at = (size_t)y * W + x;
            const float gw[3] = {dL_dnormal[at], dL_dnormal[N + at], dL_dnormal[2 * N + at]};
            float g[3];
            if constexpr (WORLD) {                // world -> view: the transpose of to_world
#pragma unroll
                for (int k = 0; k < 3; ++k) g[k] = (viewmatrix[k] * gw[0] + viewmatrix[4 + k] * gw[1]) + viewmatrix[8 + k] * gw[2];
            } else { g[0] = gw[0]; g[1] = gw[1]; g[2] = gw[2]; }
            const float len = sqrtf(cc);
            const float n[3] = {c[0] / len, c[1] / len, c[2] / len};
            const float ng = (n[0] * g[0] + n[1] * g[1]) + n[2] * g[2];
            const float dc[3] = {(g[0] - n[0] * ng) / len, (g[1] - n[1] * ng) / len, (g[2] - n[2] * ng) / len};
            const float du[3] = {v[1] * dc[2] - v[2] * dc[1], v[2] * dc[0] - v[0] * dc[2], v[0] * dc[1] - v[1] * dc[0]};
            const float dv[3] = {dc[1] * u[2] - dc[2] * u[1], dc[2] * u[0] - dc[0] * u[2], dc[0] * u[1] - dc[1] * u[0]};
            dn = (ax3[0] * du[0] + ay3[1] * du[1]) + du[2];
            up = -((ax3[0] * du[0] + ay3[-1] * du[1]) + du[2]);
            rt = (ax3[1] * dv[0] + ay3[0] * dv[1]) + dv[2];
            lf = -((ax3[-1] * dv[0] + ay3[0] * dv[1]) + dv[2]);
        }
        s_up[e] = up; s_dn[e] = dn; s_lf[e] = lf; s_rt[e] = rt;
    }
    __syncthreads();
    const int lx = threadIdx.x & (TW - 1);
    for (int ly = threadIdx.x / TW; ly < TH; ly += 256 / TW) {
        const int x = x0 + lx, y = y0 + ly;
        const int e = (ly + 1) * CW + (lx + 1);
        // the stencils above, below, left and right of this pixel, in this order
        const float dz = ((s_dn[e - CW] + s_up[e + CW]) + s_rt[e - 1]) + s_lf[e + 1];
        if (x < W && y < H) dL_ddepth[(size_t)y * W + x] = dz;
    }
}

}  // namespace

hipError_t launch_gaussian_normals_forward(int P, const float* means3D, const float* scales, const float* rotations,
                                           const float* viewmatrix, const float* campos, bool world, float* normals,
                                           uint8_t* flags, hipStream_t s) {
    if (P == 0) return hipSuccess;
    const dim3 grid((P + 255) / 256), block(256);
    if (world)
        hipLaunchKernelGGL(gaussian_normals_forward_kernel<true>, grid, block, 0, s, P, means3D, scales, rotations, viewmatrix,
                           campos, normals, flags);
    else
        hipLaunchKernelGGL(gaussian_normals_forward_kernel<false>, grid, block, 0, s, P, means3D, scales, rotations, viewmatrix,
                           campos, normals, flags);
    return hipGetLastError();
}

hipError_t launch_gaussian_normals_backward(int P, const float* rotations, const uint8_t* flags, const float* viewmatrix,
                                            bool world, const float* dL_dnormals, float* dL_drotations, hipStream_t s) {
    if (P == 0) return hipSuccess;
    const dim3 grid((P + 255) / 256), block(256);
    if (world)
        hipLaunchKernelGGL(gaussian_normals_backward_kernel<true>, grid, block, 0, s, P, rotations, flags, viewmatrix,
                           dL_dnormals, dL_drotations);
    else
        hipLaunchKernelGGL(gaussian_normals_backward_kernel<false>, grid, block, 0, s, P, rotations, flags, viewmatrix,
                           dL_dnormals, dL_drotations);
    return hipGetLastError();
}

hipError_t launch_depth_normal_forward(int W, int H, float tanfovx, float tanfovy, const float* depth, const float* viewmatrix,
                                       bool world, float* normal, hipStream_t s) {
    if (W == 0 || H == 0) return hipSuccess;
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH), block(256);
    if (world)
        hipLaunchKernelGGL(depth_normal_forward_kernel<true>, grid, block, 0, s, W, H, tanfovx, tanfovy, depth, viewmatrix,
                           normal);
    else
        hipLaunchKernelGGL(depth_normal_forward_kernel<false>, grid, block, 0, s, W, H, tanfovx, tanfovy, depth, viewmatrix,
                           normal);
    return hipGetLastError();
}

hipError_t launch_depth_normal_backward(int W, int H, float tanfovx, float tanfovy, const float* depth, const float* viewmatrix,
                                        bool world, const float* dL_dnormal, float* dL_ddepth, hipStream_t s) {
    if (W == 0 || H == 0) return hipSuccess;
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH), block(256);
    if (world)
        hipLaunchKernelGGL(depth_normal_backward_kernel<true>, grid, block, 0, s, W, H, tanfovx, tanfovy, depth, viewmatrix,
                           dL_dnormal, dL_ddepth);
    else
        hipLaunchKernelGGL(depth_normal_backward_kernel<false>, grid, block, 0, s, W, H, tanfovx, tanfovy, depth, viewmatrix,
                           dL_dnormal, dL_ddepth);
    return hipGetLastError();
}

}  // namespace msgs

// antialias.hip — opt-in antialiasing as an opacity pre-pass in front of K1 (SPEC M14; 4.14).
//
//   screen_compensation_forward_kernel    o_eff = o * rho,  rho = sqrt(max(0.000025, det0 / det1)) — the opacity compensation
//                                          of Mip-Splatting's 2-D screen filter (upstream 3DGS's h_convolution_scaling)
//   screen_compensation_backward_kernel   dL/do, dL/dmeans3D, dL/dscales + dL/drotations or dL/dcov3D from dL/do_eff; with a
//                                          camera pointer also one row of double partial sums of dL/dviewmatrix per workgroup
//   screen_compensation_finish_kernel     adds those rows in a fixed order
//
// det0 is the determinant of the projected covariance T Sigma T^T BEFORE the +0.3 dilation of Q3 and det1 the one after it.
// An antialiased render is the plain render of the same model with o_eff in the place of the opacity: K1, K9 and the blend
// kernels are not touched and never learn of it.  (a0, b, c0) must be the float32 values K1 forms, so view_point,
// cov3d_from_scale_rot, the pre-dilation part of compute_cov2d and the K9 maps behind (dL/da, dL/db, dL/dc) are restated here
// operation for operation from preprocess.hip's anonymous namespace; floating-point contraction is OFF, as it is there.
//
// All three are streaming kernels, one lane per Gaussian, 256-thread workgroups: 44 B in / 4 B out per Gaussian forward,
// 48 B in / 36 - 48 B out backward (the projection is recomputed: nothing is saved but the inputs).
#include "msgs_internal.h"

#pragma clang fp contract(off)

namespace msgs {

namespace {

constexpr float DILATION = 0.3f;              // Q3
constexpr float RHO2_FLOOR = 0.000025f;       // rho >= 0.005
constexpr int AA_V_SUMS = 12;                 // dL/dV[4j + k], j = 0..3, k = 0..2, at [3j + k] (column 3 of V never enters)
constexpr int AA_FINISH_GROUPS = 64;
constexpr int AA_FINISH_THREADS = AA_FINISH_GROUPS * AA_V_SUMS;

// = preprocess.hip
__device__ __forceinline__ void view_point(const float* V, const float* p, float* t) {
    t[0] = ((V[0] * p[0] + V[4] * p[1]) + V[8] * p[2]) + V[12];
    t[1] = ((V[1] * p[0] + V[5] * p[1]) + V[9] * p[2]) + V[13];
    t[2] = ((V[2] * p[0] + V[6] * p[1]) + V[10] * p[2]) + V[14];
}

// = preprocess.hip
__device__ __forceinline__ void cov3d_from_scale_rot(const float* s, float mod, const float* q, float* cov) {
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    const float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
                           {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
                           {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
    const float S[3] = {mod * s[0], mod * s[1], mod * s[2]};
    float M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[i][j] = R[i][j] * S[j];
    cov[0] = M[0][0] * M[0][0] + M[0][1] * M[0][1] + M[0][2] * M[0][2];
    cov[1] = M[0][0] * M[1][0] + M[0][1] * M[1][1] + M[0][2] * M[1][2];
    cov[2] = M[0][0] * M[2][0] + M[0][1] * M[2][1] + M[0][2] * M[2][2];
    cov[3] = M[1][0] * M[1][0] + M[1][1] * M[1][1] + M[1][2] * M[1][2];
    cov[4] = M[1][0] * M[2][0] + M[1][1] * M[2][1] + M[1][2] * M[2][2];
    cov[5] = M[2][0] * M[2][0] + M[2][1] * M[2][1] + M[2][2] * M[2][2];
}

// compute_cov2d of preprocess.hip up to, and without, the +0.3: (a0, b, c0) are the sums K1 adds the dilation to
struct Cov2D0 {
    float T[2][3];
    float a0, b, c0;
    float tx_c, ty_c, tz, x_mul, y_mul;
};

__device__ __forceinline__ void compute_cov2d_undilated(const float* t, const ViewParams& vp, const float* cov3D, const float* V,
                                                        Cov2D0& o) {
    const float limx = 1.3f * vp.tanfovx, limy = 1.3f * vp.tanfovy;
    const float txtz = t[0] / t[2], tytz = t[1] / t[2];
    o.x_mul = (txtz < -limx || txtz > limx) ? 0.f : 1.f;
    o.y_mul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
    o.tx_c = fminf(limx, fmaxf(-limx, txtz)) * t[2];
    o.ty_c = fminf(limy, fmaxf(-limy, tytz)) * t[2];
    o.tz = t[2];
    const float J[2][3] = {{vp.fx / t[2], 0.f, -(vp.fx * o.tx_c) / (t[2] * t[2])},
                           {0.f, vp.fy / t[2], -(vp.fy * o.ty_c) / (t[2] * t[2])}};
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            o.T[r][c] = J[r][0] * V[4 * c + 0] + J[r][1] * V[4 * c + 1] + J[r][2] * V[4 * c + 2];
    const float S[3][3] = {{cov3D[0], cov3D[1], cov3D[2]}, {cov3D[1], cov3D[3], cov3D[4]},
                           {cov3D[2], cov3D[4], cov3D[5]}};
    float ST[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 3; ++i) ST[r][i] = S[i][0] * o.T[r][0] + S[i][1] * o.T[r][1] + S[i][2] * o.T[r][2];
    o.a0 = o.T[0][0] * ST[0][0] + o.T[0][1] * ST[0][1] + o.T[0][2] * ST[0][2];
    o.b = o.T[0][0] * ST[1][0] + o.T[0][1] * ST[1][1] + o.T[0][2] * ST[1][2];
    o.c0 = o.T[1][0] * ST[1][0] + o.T[1][1] * ST[1][1] + o.T[1][2] * ST[1][2];
}

__device__ __forceinline__ bool finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

// one Gaussian's row and what the compensation is made of
struct Row {
    float p[3], o;
    float s[3], q[4];            // scales / rotations given
    float cov3D[6];
    float t[3];
    Cov2D0 c2;
    float det1, r, rho;
    bool ok;                     // false: an exceptional row (SPEC M14) — rho = 1 exactly, no geometry gradient
};

__device__ __forceinline__ void load_view(const ViewParams& vp, float* V) {
#pragma unroll
    for (int k = 0; k < 16; ++k) V[k] = vp.viewmatrix[k];
}

__device__ __forceinline__ void compensation(const ViewParams& vp, const float* V, const msgs_gaussians_t& g, int i, Row& w) {
    w.p[0] = g.means3D[3 * i]; w.p[1] = g.means3D[3 * i + 1]; w.p[2] = g.means3D[3 * i + 2];
    w.o = g.opacities[i];
    bool fin = finite3(w.p) && isfinite(w.o);
    if (g.cov3D_precomp) {
#pragma unroll
        for (int k = 0; k < 6; ++k) w.cov3D[k] = g.cov3D_precomp[6 * i + k];
        fin = fin && finite3(w.cov3D) && finite3(w.cov3D + 3);
    } else {
        w.s[0] = g.scales[3 * i]; w.s[1] = g.scales[3 * i + 1]; w.s[2] = g.scales[3 * i + 2];
        const float4 q4 = reinterpret_cast<const float4*>(g.rotations)[i];
        w.q[0] = q4.x; w.q[1] = q4.y; w.q[2] = q4.z; w.q[3] = q4.w;
        fin = fin && finite3(w.s) && finite3(w.q) && isfinite(w.q[3]);
        cov3d_from_scale_rot(w.s, vp.scale_modifier, w.q, w.cov3D);
    }
    view_point(V, w.p, w.t);
    w.rho = 1.0f; w.r = 1.0f; w.det1 = 1.0f;
    w.ok = false;
    if (!fin || !(w.t[2] > 0.2f)) return;                            // Q1 (and a NaN depth)
    compute_cov2d_undilated(w.t, vp, w.cov3D, V, w.c2);
    const float a0 = w.c2.a0, b = w.c2.b, c0 = w.c2.c0;
    const float det0 = a0 * c0 - b * b;
    const float det1 = (a0 + DILATION) * (c0 + DILATION) - b * b;
    if (det1 == 0.0f) return;
    const float r = det0 / det1;
    const float rho = sqrtf(fmaxf(RHO2_FLOOR, r));
    if (!isfinite(r) || !isfinite(w.o * rho)) return;
    w.det1 = det1; w.r = r; w.rho = rho;
    w.ok = true;
}

__global__ __launch_bounds__(256) void screen_compensation_forward_kernel(ViewParams vp, msgs_gaussians_t g,
                                                                          float* __restrict__ o_eff) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.P) return;
    float V[16];
    load_view(vp, V);
    Row w;
    compensation(vp, V, g, i, w);
    o_eff[i] = w.ok ? w.o * w.rho : w.o;
}

// CAMERA: `rows` receives AA_V_SUMS doubles per workgroup — the 64 lanes of a wave in a fixed butterfly, the four waves in
// order: the same bits on every run
template <bool CAMERA>
__global__ __launch_bounds__(256) void screen_compensation_backward_kernel(ViewParams vp, msgs_gaussians_t g,
                                                                           const float* __restrict__ dL_do_eff,
                                                                           float* __restrict__ dL_dopacity,
                                                                           float* __restrict__ dL_dmeans3D,
                                                                           float* __restrict__ dL_dscales,
                                                                           float* __restrict__ dL_drotations,
                                                                           float* __restrict__ dL_dcov3D,
                                                                           double* __restrict__ rows) {
    __shared__ double s_v[4][AA_V_SUMS];
    const int P = g.P;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool in_range = i < P;

    float dopac = 0.f;
    float dmean[3] = {0.f, 0.f, 0.f};
    float dcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float dscale[3] = {0.f, 0.f, 0.f};
    float dq[4] = {0.f, 0.f, 0.f, 0.f};
    float p[3] = {0.f, 0.f, 0.f};
    float cdt[3] = {0.f, 0.f, 0.f}, cjt[9] = {};         // dL/dt and (J dT)[c][k] = dL/dWr through T = J Wr, as in K9

    if (in_range) {
        float V[16];
        load_view(vp, V);
        Row w;
        compensation(vp, V, g, i, w);
        const float gi = dL_do_eff[i];
        dopac = w.rho * gi;                              // (rho = 1 on an exceptional row)
        // the floor's gradient is exactly zero
        if (w.ok && w.r > RHO2_FLOOR) {
            p[0] = w.p[0]; p[1] = w.p[1]; p[2] = w.p[2];
            const Cov2D0& c2 = w.c2;
            const float a0 = c2.a0, b = c2.b, c0 = c2.c0;
            // r = det0 / det1: with det1 - det0 = h (a0 + c0) + h^2 the numerators of SPEC M14 expand to sums of positive terms,
            //   c0 det1 - det0 (c0 + h) = h (c0^2 + b^2) + h^2 c0,   a0 det1 - det0 (a0 + h) = h (a0^2 + b^2) + h^2 a0,
            //   2 b (det0 - det1) = -2 b (h (a0 + c0) + h^2)
            // — the same numbers without the cancellation, and 1 / det1 applied twice so that det1^2 cannot overflow
            constexpr float h = DILATION, h2 = DILATION * DILATION;
            const float inv = 1.0f / w.det1;
            const float dr = ((w.o * gi) / (2.0f * w.rho));
            const float dL_da = dr * (((h * (c0 * c0 + b * b) + h2 * c0) * inv) * inv);
            const float dL_dc = dr * (((h * (a0 * a0 + b * b) + h2 * a0) * inv) * inv);
            const float dL_db = dr * (((-2.0f * b * (h * (a0 + c0) + h2)) * inv) * inv);
            // ---- from here on: K9 (preprocess.hip, "2-D covariance backward" and "3-D covariance backward") ----
            const float(*T)[3] = c2.T;
            dcov[0] = T[0][0] * T[0][0] * dL_da + T[0][0] * T[1][0] * dL_db + T[1][0] * T[1][0] * dL_dc;
            dcov[3] = T[0][1] * T[0][1] * dL_da + T[0][1] * T[1][1] * dL_db + T[1][1] * T[1][1] * dL_dc;
            dcov[5] = T[0][2] * T[0][2] * dL_da + T[0][2] * T[1][2] * dL_db + T[1][2] * T[1][2] * dL_dc;
            dcov[1] = 2 * T[0][0] * T[0][1] * dL_da + (T[0][0] * T[1][1] + T[0][1] * T[1][0]) * dL_db + 2 * T[1][0] * T[1][1] * dL_dc;
            dcov[2] = 2 * T[0][0] * T[0][2] * dL_da + (T[0][0] * T[1][2] + T[0][2] * T[1][0]) * dL_db + 2 * T[1][0] * T[1][2] * dL_dc;
            dcov[4] = 2 * T[0][2] * T[0][1] * dL_da + (T[0][1] * T[1][2] + T[0][2] * T[1][1]) * dL_db + 2 * T[1][1] * T[1][2] * dL_dc;
            {
                const float* cov3D = w.cov3D;
                const float Sg[3][3] = {{cov3D[0], cov3D[1], cov3D[2]}, {cov3D[1], cov3D[3], cov3D[4]},
                                        {cov3D[2], cov3D[4], cov3D[5]}};
                float ST0[3], ST1[3], dT0[3], dT1[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    ST0[k] = Sg[k][0] * c2.T[0][0] + Sg[k][1] * c2.T[0][1] + Sg[k][2] * c2.T[0][2];
                    ST1[k] = Sg[k][0] * c2.T[1][0] + Sg[k][1] * c2.T[1][1] + Sg[k][2] * c2.T[1][2];
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    dT0[k] = 2 * ST0[k] * dL_da + ST1[k] * dL_db;
                    dT1[k] = 2 * ST1[k] * dL_dc + ST0[k] * dL_db;
                }
                const float dJ00 = V[0] * dT0[0] + V[4] * dT0[1] + V[8] * dT0[2];          // Wr[k][c] = V[4*c + k]
                const float dJ02 = V[2] * dT0[0] + V[6] * dT0[1] + V[10] * dT0[2];
                const float dJ11 = V[1] * dT1[0] + V[5] * dT1[1] + V[9] * dT1[2];
                const float dJ12 = V[2] * dT1[0] + V[6] * dT1[1] + V[10] * dT1[2];
                const float tz = 1.f / c2.tz, tz2 = tz * tz, tz3 = tz2 * tz;
                const float dtx = c2.x_mul * -vp.fx * tz2 * dJ02;                           // Q2
                const float dty = c2.y_mul * -vp.fy * tz2 * dJ12;
                const float dtz = -vp.fx * tz2 * dJ00 - vp.fy * tz2 * dJ11 + (2 * vp.fx * c2.tx_c) * tz3 * dJ02 +
                                  (2 * vp.fy * c2.ty_c) * tz3 * dJ12;
#pragma unroll
                for (int j = 0; j < 3; ++j) dmean[j] = V[4 * j + 0] * dtx + V[4 * j + 1] * dty + V[4 * j + 2] * dtz;
                if constexpr (CAMERA) {
                    // J exactly as compute_cov2d formed it; T[r][c] = sum_k J[r][k] V[4c + k]
                    const float J00 = vp.fx / c2.tz, J02 = -(vp.fx * c2.tx_c) / (c2.tz * c2.tz);
                    const float J11 = vp.fy / c2.tz, J12 = -(vp.fy * c2.ty_c) / (c2.tz * c2.tz);
                    cdt[0] = dtx; cdt[1] = dty; cdt[2] = dtz;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        cjt[3 * c + 0] = J00 * dT0[c];
                        cjt[3 * c + 1] = J11 * dT1[c];
                        cjt[3 * c + 2] = J02 * dT0[c] + J12 * dT1[c];
                    }
                }
            }
            if (!g.cov3D_precomp) {
                const float qr = w.q[0], qx = w.q[1], qy = w.q[2], qz = w.q[3];
                const float S[3] = {vp.scale_modifier * w.s[0], vp.scale_modifier * w.s[1], vp.scale_modifier * w.s[2]};
                const float R[3][3] = {{1.f - 2.f * (qy * qy + qz * qz), 2.f * (qx * qy - qr * qz), 2.f * (qx * qz + qr * qy)},
                                       {2.f * (qx * qy + qr * qz), 1.f - 2.f * (qx * qx + qz * qz), 2.f * (qy * qz - qr * qx)},
                                       {2.f * (qx * qz - qr * qy), 2.f * (qy * qz + qr * qx), 1.f - 2.f * (qx * qx + qy * qy)}};
                const float Gm[3][3] = {{dcov[0], 0.5f * dcov[1], 0.5f * dcov[2]},
                                        {0.5f * dcov[1], dcov[3], 0.5f * dcov[4]},
                                        {0.5f * dcov[2], 0.5f * dcov[4], dcov[5]}};
                float dM[3][3], dR[3][3];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float acc = 0.f;
#pragma unroll
                        for (int k = 0; k < 3; ++k) acc += Gm[a][k] * (R[k][c] * S[c]);
                        dM[a][c] = 2.f * acc;
                    }
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float ds = dM[0][j] * R[0][j] + dM[1][j] * R[1][j] + dM[2][j] * R[2][j];
                    dscale[j] = vp.scale_modifier * ds;
#pragma unroll
                    for (int a = 0; a < 3; ++a) dR[a][j] = dM[a][j] * S[j];
                }
                const float r = qr, x = qx, y = qy, z = qz;
                dq[0] = 2.f * (-z * dR[0][1] + y * dR[0][2] + z * dR[1][0] - x * dR[1][2] - y * dR[2][0] + x * dR[2][1]);
                dq[1] = 2.f * (y * dR[0][1] + z * dR[0][2] + y * dR[1][0] - 2.f * x * dR[1][1] - r * dR[1][2] + z * dR[2][0] + r * dR[2][1] - 2.f * x * dR[2][2]);
                dq[2] = 2.f * (-2.f * y * dR[0][0] + x * dR[0][1] + r * dR[0][2] + x * dR[1][0] + z * dR[1][2] - r * dR[2][0] + z * dR[2][1] - 2.f * y * dR[2][2]);
                dq[3] = 2.f * (-2.f * z * dR[0][0] - r * dR[0][1] + x * dR[0][2] + r * dR[1][0] - 2.f * z * dR[1][1] + y * dR[1][2] + x * dR[2][0] + y * dR[2][1]);
            }
        }
        if (dL_dopacity) dL_dopacity[i] = dopac;
        if (dL_dmeans3D) { dL_dmeans3D[3 * i] = dmean[0]; dL_dmeans3D[3 * i + 1] = dmean[1]; dL_dmeans3D[3 * i + 2] = dmean[2]; }
        if (dL_dscales) { dL_dscales[3 * i] = dscale[0]; dL_dscales[3 * i + 1] = dscale[1]; dL_dscales[3 * i + 2] = dscale[2]; }
        if (dL_drotations) reinterpret_cast<float4*>(dL_drotations)[i] = make_float4(dq[0], dq[1], dq[2], dq[3]);
        if (dL_dcov3D) {
#pragma unroll
            for (int k = 0; k < 6; ++k) dL_dcov3D[6 * i + k] = dcov[k];
        }
    }
    if constexpr (CAMERA) {
        // M8's flat convention: dL/dV[4j + k] = sum_i ph_j dL/dt_k (+ (J dT)[j][k] for j < 3), ph = (p, 1); lanes without a
        // gradient carry zeros
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double v = (j < 3 ? (double)p[j] : 1.0) * (double)cdt[k] + (j < 3 ? (double)cjt[3 * j + k] : 0.0);
                const double sum = wave_sum_f64(v);
                if (lane == 0) s_v[wv][3 * j + k] = sum;
            }
        __syncthreads();
        if (threadIdx.x < AA_V_SUMS) {
            const int m = threadIdx.x;
            rows[(size_t)blockIdx.x * AA_V_SUMS + m] = ((s_v[0][m] + s_v[1][m]) + s_v[2][m]) + s_v[3][m];
        }
    }
}

// One workgroup: group t / 12 adds column t % 12 of the rows t / 12, t / 12 + 64, ... in index order, the 64 groups then meet in
// a fixed pairwise tree in LDS.  Double throughout, rounded to float once; no atomics.
__global__ __launch_bounds__(AA_FINISH_THREADS) void screen_compensation_finish_kernel(const double* __restrict__ rows, int nrows,
                                                                                       float* __restrict__ dL_dV) {
    __shared__ double s_sum[AA_FINISH_GROUPS][AA_V_SUMS];
    const int m = threadIdx.x % AA_V_SUMS, grp = threadIdx.x / AA_V_SUMS;
    double acc = 0.0;
    for (int r = grp; r < nrows; r += AA_FINISH_GROUPS) acc += rows[(size_t)r * AA_V_SUMS + m];
    s_sum[grp][m] = acc;
    __syncthreads();
#pragma unroll
    for (int h = AA_FINISH_GROUPS / 2; h > 0; h >>= 1) {
        if (grp < h) s_sum[grp][m] += s_sum[grp + h][m];
        __syncthreads();
    }
    if (threadIdx.x < 16) {
        const int j = threadIdx.x >> 2, k = threadIdx.x & 3;
        dL_dV[threadIdx.x] = k < 3 ? (float)s_sum[0][3 * j + k] : 0.f;
    }
}

}  // namespace

size_t screen_compensation_rows_bytes(int P) { return sizeof(double) * AA_V_SUMS * (size_t)(((P > 0 ? P : 1) + 255) / 256); }

hipError_t launch_screen_compensation_forward(const ViewParams& vp, const msgs_gaussians_t& g, float* o_eff, hipStream_t s) {
    if (g.P == 0) return hipSuccess;
    hipLaunchKernelGGL(screen_compensation_forward_kernel, dim3((g.P + 255) / 256), dim3(256), 0, s, vp, g, o_eff);
    return hipGetLastError();
}

hipError_t launch_screen_compensation_backward(const ViewParams& vp, const msgs_gaussians_t& g, const float* dL_do_eff,
                                               float* dL_dopacity, float* dL_dmeans3D, float* dL_dscales, float* dL_drotations,
                                               float* dL_dcov3D, float* dL_dV, double* rows, hipStream_t s) {
    if (g.P == 0) return hipSuccess;
    const dim3 grid((g.P + 255) / 256), block(256);
    if (!dL_dV) {
        hipLaunchKernelGGL(screen_compensation_backward_kernel<false>, grid, block, 0, s, vp, g, dL_do_eff, dL_dopacity,
                           dL_dmeans3D, dL_dscales, dL_drotations, dL_dcov3D, (double*)nullptr);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(screen_compensation_backward_kernel<true>, grid, block, 0, s, vp, g, dL_do_eff, dL_dopacity, dL_dmeans3D,
                       dL_dscales, dL_drotations, dL_dcov3D, rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(screen_compensation_finish_kernel, dim3(1), dim3(AA_FINISH_THREADS), 0, s, rows, (int)grid.x, dL_dV);
    return hipGetLastError();
}

}  // namespace msgs

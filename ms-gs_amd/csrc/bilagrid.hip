// Bilateral-grid colour correction (DESIGN.md SPEC M19, 4.20): a per-image grid [12,GL,GY,GX] of 3x4 affine colour transforms
// over (x, y, luminance), sliced per pixel with trilinear interpolation, and the total-variation regulariser of a bank of grids.
//
//   slice forward    one workgroup per 64x16 pixel tile.  The xy nodes the tile touches (its window) are staged in LDS once,
//                    all GL planes x 12 channels, as [node][plane][12]; a lane owns 4 adjacent pixels of one row and reads the 8
//                    corners of each as 3 x 16 B.  A window of more than BILAGRID_WINDOW_CELLS nodes is read from global memory
//                    instead (small images under large grids: the L2 holds the grid).
//   slice backward   the same tile; dL/dimage per pixel.  dL/dgrid: every WAVE (a 64x4 strip of the tile) sums, for every
//                    (node, plane) its strip touches, the 12 channel sums over its 256 pixels in one fixed order — 4 pixels in
//                    the lane, then the DPP / permlane butterfly of wave_allreduce_sum — and stores them with plain stores into
//                    its own window of a slab in scratch.  (node, plane) pairs nobody in the wave touches (found by ballot) are
//                    stored as zeros without arithmetic.
//   slice reduce     one workgroup per xy node: the strips whose window holds the node form a rectangle of the strip raster that
//                    follows from the geometry; their slab entries are added in raster order into a double, rounded once.
//   tv forward       one streaming pass, three per-workgroup partial sums (one per axis) in double, then one workgroup adds the
//                    partials in a fixed order.
//   tv backward      a gather of at most six neighbours per element, scaled by the upstream scalar read on the device.
//
// No float atomics anywhere: every sum has one order, so all results repeat bit for bit.
//
// An interpolation is written lerp(a, b, t) = a + t (b - a), innermost along x, then y, then the guide: equal corners give
// exactly that value, so an identity grid returns the image bit for bit.  A non-finite pixel only has a non-finite guide; it is
// clamped to [0, 1] BEFORE the conversion to int (fmaxf / fminf drop a NaN), so every index is in range.
#include <algorithm>

#include "msgs_internal.h"

#pragma clang fp contract(off)

namespace msgs {

namespace {

constexpr int TW = MSGS_BILAGRID_TILE_W, TH = MSGS_BILAGRID_TILE_H;      // 64 x 16 pixels, 256 threads
constexpr int SH = 4;                                                     // rows of a wave's strip
constexpr int WIN = MSGS_BILAGRID_WINDOW_CELLS;                           // xy nodes a tile's LDS window holds
constexpr int BG_THREADS = 256;
static_assert(TW == 64 && TH == 16 && TH / SH == BG_THREADS / 64, "lane layout: 16 lanes x 4 pixels per row, 4 rows per wave");

struct Geo {
    int W, H, GX, GY, GL;
};

// cell and weight of integer pixel coordinate x on an axis of n pixels and G nodes; monotone in x
__host__ __device__ inline int axis_cell(int x, int n, int G, float* t) {
    if (G == 1) { *t = 0.f; return 0; }
    const float f = (((float)x + 0.5f) / (float)n) * (float)(G - 1);
    int k = (int)floorf(f);
    k = k < 0 ? 0 : (k > G - 2 ? G - 2 : k);
    *t = f - (float)k;
    return k;
}
__host__ __device__ inline int axis_cell(int x, int n, int G) { float t; return axis_cell(x, n, G, &t); }

// nodes [first, first + count) touched by pixels [x0, x0 + len) of the axis (clipped to n; x0 < n)
__host__ __device__ inline int axis_window(int x0, int len, int n, int G, int* count) {
    if (G == 1) { *count = 1; return 0; }
    const int x1 = x0 + len - 1 < n - 1 ? x0 + len - 1 : n - 1;
    const int a = axis_cell(x0, n, G), b = axis_cell(x1, n, G);
    *count = b - a + 2;
    return a;
}

__device__ __forceinline__ float guide_of(float r, float g, float b) { return (0.299f * r + 0.587f * g) + 0.114f * b; }

// guide cell: clamp first, then convert (a NaN guide becomes 0, +-Inf an end of the range)
__device__ __forceinline__ int guide_cell(float z, int GL, float* t) {
    if (GL == 1) { *t = 0.f; return 0; }
    const float zc = fminf(fmaxf(z, 0.f), 1.f);
    const float f = zc * (float)(GL - 1);
    int k = (int)floorf(f);
    k = k < 0 ? 0 : (k > GL - 2 ? GL - 2 : k);
    *t = f - (float)k;
    return k;
}

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

// the 12 entries of the xy-interpolated plane p: from the LDS window [node][plane][12] ...
__device__ __forceinline__ void plane_lds(const float* __restrict__ win, int GL, int n00, int n01, int n10, int n11, int p,
                                          float tx, float ty, float out[12]) {
    const float4* a = reinterpret_cast<const float4*>(win + ((size_t)n00 * GL + p) * 12);
    const float4* b = reinterpret_cast<const float4*>(win + ((size_t)n01 * GL + p) * 12);
    const float4* c = reinterpret_cast<const float4*>(win + ((size_t)n10 * GL + p) * 12);
    const float4* d = reinterpret_cast<const float4*>(win + ((size_t)n11 * GL + p) * 12);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const float4 va = a[q], vb = b[q], vc = c[q], vd = d[q];
        out[4 * q + 0] = lerp(lerp(va.x, vb.x, tx), lerp(vc.x, vd.x, tx), ty);
        out[4 * q + 1] = lerp(lerp(va.y, vb.y, tx), lerp(vc.y, vd.y, tx), ty);
        out[4 * q + 2] = lerp(lerp(va.z, vb.z, tx), lerp(vc.z, vd.z, tx), ty);
        out[4 * q + 3] = lerp(lerp(va.w, vb.w, tx), lerp(vc.w, vd.w, tx), ty);
    }
}

// ... or from the grid in global memory [12][GL][GY][GX]
__device__ __forceinline__ void plane_global(const float* __restrict__ grid, const Geo& g, int kx0, int kx1, int ky0, int ky1,
                                             int p, float tx, float ty, float out[12]) {
    const size_t cs = (size_t)g.GL * g.GY * g.GX;
    const size_t r0 = ((size_t)p * g.GY + ky0) * g.GX, r1 = ((size_t)p * g.GY + ky1) * g.GX;
#pragma unroll
    for (int c = 0; c < 12; ++c) {
        const float* G = grid + c * cs;
        out[c] = lerp(lerp(G[r0 + kx0], G[r0 + kx1], tx), lerp(G[r1 + kx0], G[r1 + kx1], tx), ty);
    }
}

struct Window {
    int x0, nx, y0, ny;           // first node and node count per axis
    bool lds;
};

__device__ __forceinline__ Window tile_window(const Geo& g, int px0, int py0) {
    Window w;
    w.x0 = axis_window(px0, TW, g.W, g.GX, &w.nx);
    w.y0 = axis_window(py0, TH, g.H, g.GY, &w.ny);
    w.lds = w.nx * w.ny <= WIN;
    return w;
}

// every thread of the workgroup; ends with a barrier
__device__ __forceinline__ void stage_window(const float* __restrict__ grid, const Geo& g, const Window& w, float* win) {
    if (w.lds) {
        const int per_c = w.nx * w.ny * g.GL, total = per_c * 12;
        for (int i = threadIdx.x; i < total; i += BG_THREADS) {
            const int ix = i % w.nx;
            int r = i / w.nx;
            const int iy = r % w.ny; r /= w.ny;
            const int p = r % g.GL, c = r / g.GL;
            const int gx = min(w.x0 + ix, g.GX - 1), gy = min(w.y0 + iy, g.GY - 1);     // (a window never leaves the grid)
            win[((size_t)(iy * w.nx + ix) * g.GL + p) * 12 + c] = grid[(((size_t)c * g.GL + p) * g.GY + gy) * g.GX + gx];
        }
    }
    __syncthreads();
}

// one pixel: B0 and D = B1 - B0 (the xy-interpolated planes kz and kz + 1), so that A = B0 + tz D
struct PixelCoord {
    int kx, ky, kz;
    float tx, ty, tz;
};

__device__ __forceinline__ void pixel_planes(const float* __restrict__ grid, const float* __restrict__ win, const Geo& g,
                                             const Window& w, const PixelCoord& pc, float B0[12], float D[12]) {
    const int kx1 = g.GX > 1 ? pc.kx + 1 : pc.kx, ky1 = g.GY > 1 ? pc.ky + 1 : pc.ky, kz1 = g.GL > 1 ? pc.kz + 1 : pc.kz;
    float B1[12];
    if (w.lds) {
        const int lx0 = pc.kx - w.x0, lx1 = kx1 - w.x0, ly0 = pc.ky - w.y0, ly1 = ky1 - w.y0;
        const int n00 = ly0 * w.nx + lx0, n01 = ly0 * w.nx + lx1, n10 = ly1 * w.nx + lx0, n11 = ly1 * w.nx + lx1;
        plane_lds(win, g.GL, n00, n01, n10, n11, pc.kz, pc.tx, pc.ty, B0);
        plane_lds(win, g.GL, n00, n01, n10, n11, kz1, pc.tx, pc.ty, B1);
    } else {
        plane_global(grid, g, pc.kx, kx1, pc.ky, ky1, pc.kz, pc.tx, pc.ty, B0);
        plane_global(grid, g, pc.kx, kx1, pc.ky, ky1, kz1, pc.tx, pc.ty, B1);
    }
#pragma unroll
    for (int c = 0; c < 12; ++c) D[c] = B1[c] - B0[c];
}

// 4 adjacent pixels of one plane row: one 16-byte access when the rows allow it
__device__ __forceinline__ void load4(const float* __restrict__ p, size_t o, bool vec, int nvalid, float v[4]) {
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(p + o);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < nvalid ? p[o + j] : 0.f;
    }
}
__device__ __forceinline__ void store4(float* __restrict__ p, size_t o, bool vec, int nvalid, const float v[4]) {
    if (vec) {
        *reinterpret_cast<float4*>(p + o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nvalid) p[o + j] = v[j];
    }
}

extern __shared__ __align__(16) float bg_lds[];

}  // namespace

// vec: W % 4 == 0 and every plane pointer 16-byte aligned
__global__ __launch_bounds__(BG_THREADS) void bilagrid_slice_forward_kernel(Geo g, const float* __restrict__ image,
                                                                             const float* __restrict__ grid,
                                                                             float* __restrict__ out, int vec) {
    const int px0 = blockIdx.x * TW, py0 = blockIdx.y * TH;
    const Window w = tile_window(g, px0, py0);
    stage_window(grid, g, w, bg_lds);
    const int x = px0 + (threadIdx.x & 15) * 4, y = py0 + (threadIdx.x >> 4);
    if (x >= g.W || y >= g.H) return;
    const int nvalid = min(4, g.W - x);
    const size_t plane = (size_t)g.H * g.W, o = (size_t)y * g.W + x;
    float r[4], gr[4], b[4], o0[4] = {0.f, 0.f, 0.f, 0.f}, o1[4] = {0.f, 0.f, 0.f, 0.f}, o2[4] = {0.f, 0.f, 0.f, 0.f};
    load4(image, o, vec, nvalid, r);
    load4(image + plane, o, vec, nvalid, gr);
    load4(image + 2 * plane, o, vec, nvalid, b);
    PixelCoord pc;
    pc.ky = axis_cell(y, g.H, g.GY, &pc.ty);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= nvalid) break;
        pc.kx = axis_cell(x + j, g.W, g.GX, &pc.tx);
        pc.kz = guide_cell(guide_of(r[j], gr[j], b[j]), g.GL, &pc.tz);
        float B0[12], D[12];
        pixel_planes(grid, bg_lds, g, w, pc, B0, D);
        float A[12];
#pragma unroll
        for (int c = 0; c < 12; ++c) A[c] = B0[c] + pc.tz * D[c];
        o0[j] = ((A[0] * r[j] + A[1] * gr[j]) + A[2] * b[j]) + A[3];
        o1[j] = ((A[4] * r[j] + A[5] * gr[j]) + A[6] * b[j]) + A[7];
        o2[j] = ((A[8] * r[j] + A[9] * gr[j]) + A[10] * b[j]) + A[11];
    }
    store4(out, o, vec, nvalid, o0);
    store4(out + plane, o, vec, nvalid, o1);
    store4(out + 2 * plane, o, vec, nvalid, o2);
}

// slab: per strip (strip row * strip columns + strip column) a window [sny][snx][GL][12] of floats, sny / snx the largest node
// counts of any strip (host, from the same axis_window)
__global__ __launch_bounds__(BG_THREADS) void bilagrid_slice_backward_kernel(Geo g, const float* __restrict__ image,
                                                                              const float* __restrict__ grid,
                                                                              const float* __restrict__ dL_dout,
                                                                              float* __restrict__ dL_dimage,
                                                                              float* __restrict__ slab, int snx, int sny, int vec) {
    const int px0 = blockIdx.x * TW, py0 = blockIdx.y * TH;
    const Window w = tile_window(g, px0, py0);
    stage_window(grid, g, w, bg_lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sy0 = py0 + wave * SH;                                   // the wave's strip: rows sy0 .. sy0 + 3, 64 columns
    if (sy0 >= g.H) return;                                            // wave-uniform
    const int x = px0 + (lane & 15) * 4, y = sy0 + (lane >> 4);
    const int nvalid = (x < g.W && y < g.H) ? min(4, g.W - x) : 0;
    const size_t plane = (size_t)g.H * g.W, o = (size_t)y * g.W + x;
    const bool v4 = vec && nvalid == 4;
    float r[4], gr[4], b[4], d0[4], d1[4], d2[4];
    if (nvalid > 0) {
        load4(image, o, v4, nvalid, r);
        load4(image + plane, o, v4, nvalid, gr);
        load4(image + 2 * plane, o, v4, nvalid, b);
        load4(dL_dout, o, v4, nvalid, d0);
        load4(dL_dout + plane, o, v4, nvalid, d1);
        load4(dL_dout + 2 * plane, o, v4, nvalid, d2);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = gr[j] = b[j] = d0[j] = d1[j] = d2[j] = 0.f;
    }
    PixelCoord pc[4];
    float ty = 0.f;
    const int ky = nvalid > 0 ? axis_cell(y, g.H, g.GY, &ty) : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        pc[j].ky = ky; pc[j].ty = ty;
        pc[j].kx = 0; pc[j].kz = 0; pc[j].tx = pc[j].tz = 0.f;
        if (j < nvalid) {
            pc[j].kx = axis_cell(x + j, g.W, g.GX, &pc[j].tx);
            pc[j].kz = guide_cell(guide_of(r[j], gr[j], b[j]), g.GL, &pc[j].tz);
        }
    }
    if (dL_dimage && nvalid > 0) {
        float g0[4], g1[4], g2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            g0[j] = g1[j] = g2[j] = 0.f;
            if (j >= nvalid) continue;
            float B0[12], D[12];
            pixel_planes(grid, bg_lds, g, w, pc[j], B0, D);
            float A[12];
#pragma unroll
            for (int c = 0; c < 12; ++c) A[c] = B0[c] + pc[j].tz * D[c];
            g0[j] = (A[0] * d0[j] + A[4] * d1[j]) + A[8] * d2[j];
            g1[j] = (A[1] * d0[j] + A[5] * d1[j]) + A[9] * d2[j];
            g2[j] = (A[2] * d0[j] + A[6] * d1[j]) + A[10] * d2[j];
            const float z = guide_of(r[j], gr[j], b[j]);
            if (g.GL > 1 && z > 0.f && z < 1.f) {                     // the open interval: no guide term at z = 0 or 1, or NaN
                const float s0 = ((D[0] * r[j] + D[1] * gr[j]) + D[2] * b[j]) + D[3];
                const float s1 = ((D[4] * r[j] + D[5] * gr[j]) + D[6] * b[j]) + D[7];
                const float s2 = ((D[8] * r[j] + D[9] * gr[j]) + D[10] * b[j]) + D[11];
                const float gz = ((d0[j] * s0 + d1[j] * s1) + d2[j] * s2) * (float)(g.GL - 1);
                g0[j] += gz * 0.299f;
                g1[j] += gz * 0.587f;
                g2[j] += gz * 0.114f;
            }
        }
        store4(dL_dimage, o, v4, nvalid, g0);
        store4(dL_dimage + plane, o, v4, nvalid, g1);
        store4(dL_dimage + 2 * plane, o, v4, nvalid, g2);
    }
    if (!slab) return;
    // dL/dgrid of the strip: v[j][4 c + k] = dL/dout_c (r, g, b, 1)_k of pixel j
    float v[4][12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float d[3] = {d0[j], d1[j], d2[j]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[j][4 * c + 0] = d[c] * r[j];
            v[j][4 * c + 1] = d[c] * gr[j];
            v[j][4 * c + 2] = d[c] * b[j];
            v[j][4 * c + 3] = d[c];
        }
    }
    int wnx, wny;
    const int wx0 = axis_window(px0, TW, g.W, g.GX, &wnx), wy0 = axis_window(sy0, SH, g.H, g.GY, &wny);
    const int strip = (blockIdx.y * (TH / SH) + wave) * gridDim.x + blockIdx.x;
    float* __restrict__ mine = slab + (size_t)strip * ((size_t)sny * snx * g.GL * 12);
    wnx = min(wnx, snx); wny = min(wny, sny);                          // (equal by construction: the host ran the same function)
    for (int iy = 0; iy < wny; ++iy) {
        const int ny_ = wy0 + iy;
        // weight of this node row for the lane's pixels (one row per lane)
        const bool hy0 = ny_ == ky, hy1 = g.GY > 1 && ny_ == ky + 1;
        const float wy = hy0 ? 1.f - ty : ty;
        const bool hy = nvalid > 0 && (hy0 || hy1);
        for (int ix = 0; ix < wnx; ++ix) {
            const int nx_ = wx0 + ix;
            float wxy[4];
            bool hxy[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool hx0 = nx_ == pc[j].kx, hx1 = g.GX > 1 && nx_ == pc[j].kx + 1;
                hxy[j] = hy && j < nvalid && (hx0 || hx1);
                wxy[j] = (hx0 ? 1.f - pc[j].tx : pc[j].tx) * wy;
            }
            float* __restrict__ dst = mine + ((size_t)(iy * snx + ix) * g.GL) * 12;
            for (int p = 0; p < g.GL; ++p) {
                float s[12];
#pragma unroll
                for (int c = 0; c < 12; ++c) s[c] = 0.f;
                bool any = false;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool hz0 = p == pc[j].kz, hz1 = g.GL > 1 && p == pc[j].kz + 1;
                    if (hxy[j] && (hz0 || hz1)) {
                        any = true;
                        const float wgt = wxy[j] * (hz0 ? 1.f - pc[j].tz : pc[j].tz);
#pragma unroll
                        for (int c = 0; c < 12; ++c) s[c] += wgt * v[j][c];
                    }
                }
                float mine_c = 0.f;
                if (__ballot(any) != 0ull) {                          // wave-uniform: all 64 lanes run the butterfly
#pragma unroll
                    for (int c = 0; c < 12; ++c) {
                        const float t = wave_allreduce_sum(s[c]);
                        if (lane == c) mine_c = t;
                    }
                }
                if (lane < 12) dst[p * 12 + lane] = mine_c;
            }
        }
    }
}

// one workgroup per xy node: 8 parts of 128 threads.  Thread (part, t) owns (plane, channel) slots t, t + 128, ... over the part's
// contiguous share of the strip rows; the 8 partial sums of a slot are then added in part order.
constexpr int RED_PARTS = 8, RED_SLOTS = 128;
__global__ __launch_bounds__(RED_PARTS * RED_SLOTS) void bilagrid_slice_reduce_kernel(Geo g, const float* __restrict__ slab, int snx,
                                                                                      int sny, int ncols, int nrows,
                                                                                      float* __restrict__ dL_dgrid) {
    __shared__ int lim[4];                                             // strip columns [lim0, lim1], strip rows [lim2, lim3]
    __shared__ double parts[RED_PARTS][RED_SLOTS];
    const int ix = blockIdx.x % g.GX, iy = blockIdx.x / g.GX;
    if (threadIdx.x == 0) { lim[0] = ncols; lim[1] = -1; lim[2] = nrows; lim[3] = -1; }
    __syncthreads();
    for (int c = threadIdx.x; c < ncols; c += blockDim.x) {
        int n;
        const int a = axis_window(c * TW, TW, g.W, g.GX, &n);
        if (ix >= a && ix < a + n) { atomicMin(&lim[0], c); atomicMax(&lim[1], c); }
    }
    for (int r = threadIdx.x; r < nrows; r += blockDim.x) {
        int n;
        const int a = axis_window(r * SH, SH, g.H, g.GY, &n);
        if (iy >= a && iy < a + n) { atomicMin(&lim[2], r); atomicMax(&lim[3], r); }
    }
    __syncthreads();
    const int c_lo = lim[0], c_hi = lim[1], r_lo = lim[2], r_hi = lim[3];
    const int part = threadIdx.x / RED_SLOTS, t = threadIdx.x % RED_SLOTS;
    const int share = (r_hi - r_lo + RED_PARTS) / RED_PARTS;           // rows per part (0 rows: share = 0 or the loop is empty)
    const int my_lo = r_lo + part * share, my_hi = min(my_lo + share - 1, r_hi);
    const int slots = g.GL * 12;
    const size_t stride = (size_t)sny * snx * slots;
    for (int s0 = 0; s0 < slots; s0 += RED_SLOTS) {                    // (uniform trip count: the barriers are reached by all)
        const int s = s0 + t;
        double acc = 0.0;
        if (s < slots) {
            for (int r = my_lo; r <= my_hi; ++r) {
                int n;
                const int ly = iy - axis_window(r * SH, SH, g.H, g.GY, &n);
                if (ly < 0 || ly >= sny) continue;
                for (int c = c_lo; c <= c_hi; ++c) {
                    const int lx = ix - axis_window(c * TW, TW, g.W, g.GX, &n);
                    if (lx < 0 || lx >= snx) continue;
                    acc += (double)slab[((size_t)r * ncols + c) * stride + (size_t)(ly * snx + lx) * slots + s];
                }
            }
        }
        parts[part][t] = acc;
        __syncthreads();
        if (part == 0 && s < slots) {
            double total = 0.0;
            for (int k = 0; k < RED_PARTS; ++k) total += parts[k][t];
            const int p = s / 12, ch = s % 12;
            dL_dgrid[(((size_t)ch * g.GL + p) * g.GY + iy) * g.GX + ix] = (float)total;
        }
        __syncthreads();
    }
}

namespace {
constexpr int TV_THREADS = 256;
constexpr int TV_MAX_BLOCKS = 1024;

// sums of the three per-axis squared forward differences (x, y, guide) of the workgroup's elements, in double
__device__ __forceinline__ void tv_block_sums(double s[3], double (*sh)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) s[a] = wave_sum_f64(s[a]);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; ++a) sh[wave][a] = s[a];
    __syncthreads();
}
}  // namespace

// grid (chunks of a volume, volumes): a volume is one [GL,GY,GX] block of the bank (N * 12 of them, V elements each), so the
// coordinates are 32-bit arithmetic; partial (blockIdx.y * gridDim.x + blockIdx.x)
__global__ __launch_bounds__(TV_THREADS) void bilagrid_tv_forward_kernel(int64_t volumes, int GX, int GY, int GL,
                                                                          const float* __restrict__ grids,
                                                                          double* __restrict__ partials) {
    __shared__ double sh[TV_THREADS / 64][3];
    double s[3] = {0.0, 0.0, 0.0};
    const unsigned sy = GX, sz = (unsigned)GX * GY, V = sz * GL;
    for (int64_t vol = blockIdx.y; vol < volumes; vol += gridDim.y) {
        const float* __restrict__ G = grids + vol * V;
        for (unsigned j = blockIdx.x * TV_THREADS + threadIdx.x; j < V; j += gridDim.x * TV_THREADS) {
            const unsigned x = j % sy, y = (j / sy) % (unsigned)GY, z = j / sz;
            const double c = (double)G[j];
            if (x + 1 < (unsigned)GX) { const double d = (double)G[j + 1] - c; s[0] += d * d; }
            if (y + 1 < (unsigned)GY) { const double d = (double)G[j + sy] - c; s[1] += d * d; }
            if (z + 1 < (unsigned)GL) { const double d = (double)G[j + sz] - c; s[2] += d * d; }
        }
    }
    tv_block_sums(s, sh);
    if (threadIdx.x < 3) {
        double t = 0.0;
        for (int k = 0; k < TV_THREADS / 64; ++k) t += sh[k][threadIdx.x];
        partials[3 * ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) + threadIdx.x] = t;
    }
}

// one workgroup: the partials in a fixed order, each axis divided by its own count (0 for an axis of size 1)
__global__ __launch_bounds__(TV_THREADS) void bilagrid_tv_finish_kernel(int nblocks, const double* __restrict__ partials,
                                                                         double inv_x, double inv_y, double inv_z,
                                                                         float* __restrict__ tv) {
    __shared__ double sh[TV_THREADS / 64][3];
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblocks; i += TV_THREADS)
        for (int a = 0; a < 3; ++a) s[a] += partials[3 * i + a];
    tv_block_sums(s, sh);
    if (threadIdx.x == 0) {
        double t[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < TV_THREADS / 64; ++k)
            for (int a = 0; a < 3; ++a) t[a] += sh[k][a];
        tv[0] = (float)((t[0] * inv_x + t[1] * inv_y) + t[2] * inv_z);
    }
}

__global__ __launch_bounds__(TV_THREADS) void bilagrid_tv_backward_kernel(int64_t volumes, int GX, int GY, int GL,
                                                                           const float* __restrict__ grids,
                                                                           const float* __restrict__ upstream, double inv_x,
                                                                           double inv_y, double inv_z,
                                                                           float* __restrict__ dL_dgrids) {
    const unsigned sy = GX, sz = (unsigned)GX * GY, V = sz * GL;
    const unsigned j = blockIdx.x * TV_THREADS + threadIdx.x;
    if (j >= V) return;
    const unsigned x = j % sy, y = (j / sy) % (unsigned)GY, z = j / sz;
    const double up = 2.0 * (upstream ? (double)upstream[0] : 1.0);
    for (int64_t vol = blockIdx.y; vol < volumes; vol += gridDim.y) {
        const float* __restrict__ G = grids + vol * V;
        const double c = (double)G[j];
        double gx = 0.0, gy = 0.0, gz = 0.0;
        if (x > 0) gx += c - (double)G[j - 1];
        if (x + 1 < (unsigned)GX) gx -= (double)G[j + 1] - c;
        if (y > 0) gy += c - (double)G[j - sy];
        if (y + 1 < (unsigned)GY) gy -= (double)G[j + sy] - c;
        if (z > 0) gz += c - (double)G[j - sz];
        if (z + 1 < (unsigned)GL) gz -= (double)G[j + sz] - c;
        dL_dgrids[vol * V + j] = (float)(up * ((gx * inv_x + gy * inv_y) + gz * inv_z));
    }
}

namespace {
struct SlabShape {
    int ncols, nrows, snx, sny;
    size_t bytes;
};

SlabShape slab_shape(const Geo& g) {
    SlabShape s;
    s.ncols = (g.W + TW - 1) / TW;
    s.nrows = (g.H + SH - 1) / SH;
    s.snx = s.sny = 1;
    for (int c = 0; c < s.ncols; ++c) {
        int n;
        axis_window(c * TW, TW, g.W, g.GX, &n);
        if (n > s.snx) s.snx = n;
    }
    for (int r = 0; r < s.nrows; ++r) {
        int n;
        axis_window(r * SH, SH, g.H, g.GY, &n);
        if (n > s.sny) s.sny = n;
    }
    s.bytes = align256((size_t)s.ncols * s.nrows * s.sny * s.snx * g.GL * 12 * sizeof(float));
    return s;
}

size_t window_lds_bytes(int GL) { return (size_t)WIN * GL * 12 * sizeof(float); }

bool rows_vectorise(const Geo& g, const void* a, const void* b, const void* c, const void* d) {
    return g.W % 4 == 0 && ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0);
}
}  // namespace

size_t bilagrid_scratch_bytes(int W, int H, int GX, int GY, int GL) { return slab_shape(Geo{W, H, GX, GY, GL}).bytes; }

hipError_t launch_bilagrid_slice_forward(int W, int H, int GX, int GY, int GL, const float* image, const float* grid, float* out,
                                         hipStream_t st) {
    const Geo g{W, H, GX, GY, GL};
    const dim3 tiles((W + TW - 1) / TW, (H + TH - 1) / TH);
    hipLaunchKernelGGL(bilagrid_slice_forward_kernel, tiles, dim3(BG_THREADS), window_lds_bytes(GL), st, g, image, grid, out,
                       (int)rows_vectorise(g, image, out, nullptr, nullptr));
    return hipGetLastError();
}

hipError_t launch_bilagrid_slice_backward(int W, int H, int GX, int GY, int GL, const float* image, const float* grid,
                                          const float* dL_dout, float* dL_dimage, float* dL_dgrid, char* scratch, hipStream_t st) {
    const Geo g{W, H, GX, GY, GL};
    const SlabShape s = slab_shape(g);
    const dim3 tiles((W + TW - 1) / TW, (H + TH - 1) / TH);
    float* slab = dL_dgrid ? (float*)scratch : nullptr;
    hipLaunchKernelGGL(bilagrid_slice_backward_kernel, tiles, dim3(BG_THREADS), window_lds_bytes(GL), st, g, image, grid, dL_dout,
                       dL_dimage, slab, s.snx, s.sny, (int)rows_vectorise(g, image, dL_dout, dL_dimage, nullptr));
    if (dL_dgrid)
        hipLaunchKernelGGL(bilagrid_slice_reduce_kernel, dim3((unsigned)(GX * GY)), dim3(RED_PARTS * RED_SLOTS), 0, st, g, (const float*)slab, s.snx,
                           s.sny, s.ncols, s.nrows, dL_dgrid);
    return hipGetLastError();
}

namespace {
// forward launch: chunks of a volume x volumes, at most TV_MAX_BLOCKS workgroups (= partials) in all
dim3 tv_forward_grid(int64_t volumes, int V) {
    const int bx = std::min((V + TV_THREADS - 1) / TV_THREADS, 32);
    const int64_t by = std::min<int64_t>(std::max<int64_t>(volumes, 1), TV_MAX_BLOCKS / bx);
    return dim3((unsigned)bx, (unsigned)by);
}
// 1 / (number of forward differences along the axis); 0 for an axis of size 1
double tv_inv_count(int64_t n, int G) { return G > 1 ? 1.0 / ((double)(n / G) * (double)(G - 1)) : 0.0; }
}  // namespace

size_t bilagrid_tv_scratch_bytes(int64_t) { return align256(sizeof(double) * 3 * (size_t)TV_MAX_BLOCKS); }

hipError_t launch_bilagrid_tv_forward(int64_t N, int GX, int GY, int GL, const float* grids, float* tv, char* scratch,
                                      hipStream_t st) {
    const int V = GL * GY * GX;
    const int64_t volumes = N * 12, n = volumes * V;
    const dim3 grid = tv_forward_grid(volumes, V);
    hipLaunchKernelGGL(bilagrid_tv_forward_kernel, grid, dim3(TV_THREADS), 0, st, volumes, GX, GY, GL, grids, (double*)scratch);
    hipLaunchKernelGGL(bilagrid_tv_finish_kernel, dim3(1), dim3(TV_THREADS), 0, st, (int)(grid.x * grid.y), (const double*)scratch,
                       tv_inv_count(n, GX), tv_inv_count(n, GY), tv_inv_count(n, GL), tv);
    return hipGetLastError();
}

hipError_t launch_bilagrid_tv_backward(int64_t N, int GX, int GY, int GL, const float* grids, const float* upstream,
                                       float* dL_dgrids, hipStream_t st) {
    const int V = GL * GY * GX;
    const int64_t volumes = N * 12, n = volumes * V;
    const dim3 grid((unsigned)((V + TV_THREADS - 1) / TV_THREADS), (unsigned)std::min<int64_t>(volumes, 4096));
    hipLaunchKernelGGL(bilagrid_tv_backward_kernel, grid, dim3(TV_THREADS), 0, st, volumes, GX, GY, GL, grids, upstream,
                       tv_inv_count(n, GX), tv_inv_count(n, GY), tv_inv_count(n, GL), dL_dgrids);
    return hipGetLastError();
}

}  // namespace msgs

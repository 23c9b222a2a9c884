// tsdf.hip — TSDF fusion of depth maps into a block-sparse volume and marching-tetrahedra extraction (SPEC M20; 4.22).
//
//   tsdf_mark_blocks_kernel   one lane per depth pixel: walks the ray over view depths d -+ (sdf_trunc + 2 voxels) in `steps` equal
//                             steps and writes 1 into the byte of every block a sample falls in (the same byte by every writer)
//   tsdf_integrate_kernel     one workgroup per pool slot, one lane per lattice point (x in adjacent lanes): the point's sums stay
//                             in registers over all cameras of the call; camera rows staged in LDS TSDF_CAMERA_CHUNK at a time; a
//                             block whose bounding sphere lies behind or beside a camera skips it as a whole
//   tsdf_count_kernel         one workgroup per slot: flags of its 9^3 neighbourhood in LDS (own 8^3 and the +1 halo of up to 7
//                             neighbour blocks); per lattice point the mask of its crossing owned edges and their count, per cube
//                             its triangle count
//   tsdf_emit_kernel          the same neighbourhood with T, masks and vertex offsets: vertices, colours, faces
//
// No atomics anywhere: a lattice point has one lane, a vertex one owner, a face one cube.  The two exclusive scans between count
// and emit are the caller's.  Sums, not averages, are stored, so integrate(A); integrate(B) leaves the bits of integrate(A + B).
// Projection restates filter3d.hip's view_point operation for operation, contraction OFF.
#include "msgs_internal.h"

#pragma clang fp contract(off)

namespace msgs {

namespace {

constexpr int CAM_F = MSGS_FILTER3D_CAMERA_FLOATS;
constexpr int CHUNK = MSGS_TSDF_CAMERA_CHUNK;
constexpr int BLOCK_POINTS = 512;             // 8 x 8 x 8 lattice points, x fastest
constexpr int HALO_POINTS = 729;              // 9 x 9 x 9
constexpr uint8_t F_OBSERVED = 1, F_INSIDE = 2;

// = filter3d.hip
__device__ __forceinline__ void view_point(const float* V, const float* p, float* t) {
    t[0] = ((V[0] * p[0] + V[4] * p[1]) + V[8] * p[2]) + V[12];
    t[1] = ((V[1] * p[0] + V[5] * p[1]) + V[9] * p[2]) + V[13];
    t[2] = ((V[2] * p[0] + V[6] * p[1]) + V[10] * p[2]) + V[14];
}

struct Geometry {
    float origin[3];
    float voxel;
    int nb[3];
};

__device__ __forceinline__ void block_of(const Geometry& g, int b, int* bc) {
    bc[0] = b % g.nb[0];
    bc[1] = (b / g.nb[0]) % g.nb[1];
    bc[2] = b / (g.nb[0] * g.nb[1]);
}

// offset of corner / direction code (dx + 2 dy + 4 dz) inside the 9^3 neighbourhood
__device__ __forceinline__ int halo_off(int code) { return (code & 1) + 9 * ((code >> 1) & 1) + 81 * ((code >> 2) & 1); }

// ---- activation ----
// grid (ceil(H W / 256), n): sample k of pixel (x, y) of camera n sits at view depth z_k = (d - r) + k h, r = sdf_trunc + 2 voxel,
// h = 2 r / steps, at the view point (a_x z, a_y z, z) and, M being rigid, at the world point (q - T) R^T
__global__ __launch_bounds__(256) void tsdf_mark_blocks_kernel(Geometry g, int W, int H, const float* __restrict__ cameras,
                                                               const float* __restrict__ depth, float sdf_trunc,
                                                               float depth_trunc, int steps, uint8_t* __restrict__ marks) {
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = blockIdx.y;
    if (pix >= W * H) return;
    const float d = depth[(size_t)n * W * H + pix];
    if (!(d > 0.f && d <= depth_trunc && d < INFINITY)) return;
    const float* cam = cameras + (size_t)n * CAM_F;
    const int x = pix % W, y = pix / W;
    const float Wf = (float)W, Hf = (float)H;
    const float tx = Wf / (2.0f * cam[16]), ty = Hf / (2.0f * cam[17]);
    const float ax = ((2.0f * (float)x + 1.0f) / Wf - 1.0f) * tx;
    const float ay = ((2.0f * (float)y + 1.0f) / Hf - 1.0f) * ty;
    const float r = sdf_trunc + 2.0f * g.voxel;
    const float h = (2.0f * r) / (float)steps;
    const float z0 = d - r;
    const float bs = 8.0f * g.voxel;
    for (int k = 0; k <= steps; ++k) {
        const float z = z0 + (float)k * h;
        if (!(z > 0.f)) continue;
        const float q[3] = {ax * z - cam[12], ay * z - cam[13], z - cam[14]};
        bool in = true;
        int bc[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float p = (q[0] * cam[4 * a] + q[1] * cam[4 * a + 1]) + q[2] * cam[4 * a + 2];
            const float f = floorf((p - g.origin[a]) / bs);
            in = in && f >= 0.f && f < (float)g.nb[a];             // a NaN fails both
            bc[a] = (int)f;
        }
        if (in) marks[((size_t)bc[2] * g.nb[1] + bc[1]) * g.nb[0] + bc[0]] = 1;
    }
}

// ---- integration ----
struct Frames {
    int n, W, H;
    const float* cameras;
    const float* depth;
    const float* colour;
    const float* weight;
    float sdf_trunc, depth_trunc;
};

// can no lattice point of the block (centre c, radius rho around it) project into the image of this camera?  Conservative: one
// pixel and the inflated radius absorb the rounding of the per-point projection
__device__ __forceinline__ bool block_outside(const float* cam, const float* c, float rho, float Wf, float Hf) {
    float t[3];
    view_point(cam, c, t);
    const float zmax = t[2] + rho;
    if (!(zmax > 0.f)) return true;                                // all behind (or a NaN row: no point passes t.z > 0 either)
    if (!(t[2] - rho > 0.f)) return false;
    const float fx = cam[16], fy = cam[17];
    const float xl = t[0] + rho, xr = t[0] - rho, yl = t[1] + rho, yr = t[1] - rho;
    if (xl < 0.f && (xl / zmax) * fx + Wf / 2.0f < -1.0f) return true;
    if (xr > 0.f && (xr / zmax) * fx + Wf / 2.0f > Wf + 1.0f) return true;
    if (yl < 0.f && (yl / zmax) * fy + Hf / 2.0f < -1.0f) return true;
    if (yr > 0.f && (yr / zmax) * fy + Hf / 2.0f > Hf + 1.0f) return true;
    return false;
}

template <bool COLOUR>
__global__ __launch_bounds__(BLOCK_POINTS) void tsdf_integrate_kernel(Geometry g, const int32_t* __restrict__ slot_block,
                                                                      float* __restrict__ tsdf_sum,
                                                                      float* __restrict__ weight_sum,
                                                                      float* __restrict__ colour_sum, Frames f) {
    __shared__ float s_cam[CHUNK * CAM_F];
    __shared__ uint8_t s_skip[CHUNK];
    const int slot = blockIdx.x, tid = threadIdx.x;
    int bc[3];
    block_of(g, slot_block[slot], bc);
    const int li[3] = {tid & 7, (tid >> 3) & 7, tid >> 6};
    float p[3], c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = g.origin[a] + g.voxel * (float)(8 * bc[a] + li[a]);
        c[a] = g.origin[a] + g.voxel * ((float)(8 * bc[a]) + 3.5f);
    }
    const float rho = g.voxel * 6.07f;                             // 3.5 sqrt(3) = 6.062
    const float Wf = (float)f.W, Hf = (float)f.H;
    const size_t HW = (size_t)f.W * f.H;
    const size_t at = (size_t)slot * BLOCK_POINTS + tid;
    float ts = tsdf_sum[at], ws = weight_sum[at];
    float cs[3] = {0.f, 0.f, 0.f};
    if constexpr (COLOUR) {
#pragma unroll
        for (int k = 0; k < 3; ++k) cs[k] = colour_sum[((size_t)slot * 3 + k) * BLOCK_POINTS + tid];
    }
    for (int c0 = 0; c0 < f.n; c0 += CHUNK) {
        const int nc = min(CHUNK, f.n - c0);
        __syncthreads();                                           // the previous chunk has been read
        for (int k = tid; k < nc * CAM_F; k += BLOCK_POINTS) s_cam[k] = f.cameras[(size_t)c0 * CAM_F + k];
        __syncthreads();
        if (tid < nc) s_skip[tid] = block_outside(s_cam + tid * CAM_F, c, rho, Wf, Hf) ? 1 : 0;
        __syncthreads();
        for (int n = 0; n < nc; ++n) {
            if (s_skip[n]) continue;                               // the same in every lane of the workgroup
            const float* cam = s_cam + n * CAM_F;
            float t[3];
            view_point(cam, p, t);
            if (!(t[2] > 0.f)) continue;
            const float x = (t[0] / t[2]) * cam[16] + Wf / 2.0f;
            const float y = (t[1] / t[2]) * cam[17] + Hf / 2.0f;
            if (!(x >= 0.f && x < Wf && y >= 0.f && y < Hf)) continue;
            const size_t pix = (size_t)(c0 + n) * HW + (size_t)((int)y) * f.W + (int)x;
            const float d = f.depth[pix];
            const float w = f.weight ? f.weight[pix] : 1.0f;
            if (!(d > 0.f && d <= f.depth_trunc && d < INFINITY && w > 0.f && w < INFINITY)) continue;
            const float sdf = d - t[2];
            if (sdf < -f.sdf_trunc) continue;
            ts = ts + w * fminf(1.0f, sdf / f.sdf_trunc);
            ws = ws + w;
            if constexpr (COLOUR) {
                const size_t cp = (size_t)(c0 + n) * 3 * HW + (size_t)((int)y) * f.W + (int)x;
#pragma unroll
                for (int k = 0; k < 3; ++k) cs[k] = cs[k] + w * f.colour[cp + k * HW];
            }
        }
    }
    tsdf_sum[at] = ts;
    weight_sum[at] = ws;
    if constexpr (COLOUR) {
#pragma unroll
        for (int k = 0; k < 3; ++k) colour_sum[((size_t)slot * 3 + k) * BLOCK_POINTS + tid] = cs[k];
    }
}

// ---- extraction ----
// The six Kuhn tetrahedra of a cube: permutation (a, b, c) of the axes gives the corners 0, e_a, e_a + e_b, 7 (corner codes
// dx + 2 dy + 4 dz); its orientation is the permutation's parity.  Case m (bit u: chain corner u is inside) of a POSITIVE
// tetrahedron, i the lone corner / i < j the inside pair, the others ascending and the last two swapped when (i, j, k, l) is odd:
//     one inside:  (e_ij, e_ik, e_il)       three inside: (e_ij, e_il, e_ik)       two: the quad (e_ik, e_il, e_jl, e_jk) as
//     (q0, q1, q2), (q0, q2, q3)            — normals towards the outside corners; a negative tetrahedron swaps the last two
// vertices of every triangle.  An edge is stored as (owner corner code, direction code): the lower end owns it.
struct TetTable {
    uint8_t n[16];
    uint8_t owner[6][16][6];
    uint8_t dir[6][16][6];
};

constexpr TetTable make_tet_table() {
    TetTable T{};
    const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const bool positive[6] = {true, false, false, true, true, false};
    for (int q = 0; q < 6; ++q) {
        const int code[4] = {0, 1 << perm[q][0], (1 << perm[q][0]) | (1 << perm[q][1]), 7};
        for (int m = 0; m < 16; ++m) {
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
            for (int u = 0; u < 4; ++u) {
                if ((m >> u) & 1) in[ni++] = u;
                else out[no++] = u;
            }
            int e[6][2] = {};                                      // chain corners (u, v) of each emitted vertex
            int nt = 0;
            if (ni == 1 || ni == 3) {
                const int i = ni == 1 ? in[0] : out[0];
                const int* rest = ni == 1 ? out : in;
                int j = rest[0], k = rest[1], l = rest[2];
                if (i & 1) { const int s = k; k = l; l = s; }      // (i, ascending rest) has the parity of i
                if (ni == 3) { const int s = k; k = l; l = s; }
                e[0][0] = i; e[0][1] = j; e[1][0] = i; e[1][1] = k; e[2][0] = i; e[2][1] = l;
                nt = 1;
            } else if (ni == 2) {
                const int i = in[0], j = in[1];
                int k = out[0], l = out[1];
                const int inversions = (i > k) + (i > l) + (j > k) + (j > l);
                if (inversions & 1) { const int s = k; k = l; l = s; }
                const int quad[4][2] = {{i, k}, {i, l}, {j, l}, {j, k}};
                const int order[6] = {0, 1, 2, 0, 2, 3};
                for (int v = 0; v < 6; ++v) { e[v][0] = quad[order[v]][0]; e[v][1] = quad[order[v]][1]; }
                nt = 2;
            }
            T.n[m] = (uint8_t)nt;
            for (int tr = 0; tr < nt; ++tr)
                for (int v = 0; v < 3; ++v) {
                    const int src = 3 * tr + (positive[q] || v == 0 ? v : 3 - v);
                    const int u0 = e[src][0] < e[src][1] ? e[src][0] : e[src][1];
                    const int u1 = e[src][0] < e[src][1] ? e[src][1] : e[src][0];
                    T.owner[q][m][3 * tr + v] = (uint8_t)code[u0];
                    T.dir[q][m][3 * tr + v] = (uint8_t)(code[u1] ^ code[u0]);
                }
        }
    }
    return T;
}

__constant__ const TetTable TET = make_tet_table();

// the 4 inside bits of tetrahedron q from the 8 inside bits of the cube's corners (bit = corner code)
__device__ __forceinline__ int tet_case(int q, int cube) {
    constexpr int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
    const int c1 = 1 << perm[q][0], c2 = c1 | (1 << perm[q][1]);
    return (cube & 1) | (((cube >> c1) & 1) << 1) | (((cube >> c2) & 1) << 2) | (((cube >> 7) & 1) << 3);
}

// the slots of the 8 blocks the 9^3 neighbourhood reads (code dx + 2 dy + 4 dz; -1: outside the table or not active)
__device__ __forceinline__ void stage_slots(const Geometry& g, const int32_t* __restrict__ table, const int* bc, int* s_slot) {
    if (threadIdx.x < 8) {
        const int nx = bc[0] + (threadIdx.x & 1), ny = bc[1] + ((threadIdx.x >> 1) & 1), nz = bc[2] + (threadIdx.x >> 2);
        int s = -1;
        if (nx < g.nb[0] && ny < g.nb[1] && nz < g.nb[2]) s = table[((size_t)nz * g.nb[1] + ny) * g.nb[0] + nx];
        s_slot[threadIdx.x] = s;
    }
}

// halo entry e (i + 9 j + 81 k): the slot it lives in and its index there
__device__ __forceinline__ void halo_source(int e, const int* s_slot, int& slot, int& local) {
    const int i = e % 9, j = (e / 9) % 9, k = e / 81;
    slot = s_slot[(i >> 3) | ((j >> 3) << 1) | ((k >> 3) << 2)];
    local = (i & 7) + 8 * (j & 7) + 64 * (k & 7);
}

__global__ __launch_bounds__(BLOCK_POINTS) void tsdf_count_kernel(Geometry g, const int32_t* __restrict__ table,
                                                                  const int32_t* __restrict__ slot_block,
                                                                  const float* __restrict__ tsdf_sum,
                                                                  const float* __restrict__ weight_sum,
                                                                  uint8_t* __restrict__ edge_mask,
                                                                  int32_t* __restrict__ vertex_count,
                                                                  int32_t* __restrict__ triangle_count) {
    __shared__ int s_slot[8];
    __shared__ uint8_t s_flag[HALO_POINTS];
    const int slot = blockIdx.x, tid = threadIdx.x;
    int bc[3];
    block_of(g, slot_block[slot], bc);
    stage_slots(g, table, bc, s_slot);
    __syncthreads();
    for (int e = tid; e < HALO_POINTS; e += BLOCK_POINTS) {
        int src, local;
        halo_source(e, s_slot, src, local);
        uint8_t fl = 0;
        if (src >= 0) {
            const size_t a = (size_t)src * BLOCK_POINTS + local;
            if (weight_sum[a] > 0.f) fl = F_OBSERVED | (tsdf_sum[a] < 0.f ? F_INSIDE : 0);
        }
        s_flag[e] = fl;
    }
    __syncthreads();
    const int L = (tid & 7) + 9 * ((tid >> 3) & 7) + 81 * (tid >> 6);
    const int fa = s_flag[L];
    int mask = 0, cube = fa & F_INSIDE ? 1 : 0, all = fa & F_OBSERVED;
#pragma unroll
    for (int d = 1; d < 8; ++d) {
        const int fb = s_flag[L + halo_off(d)];
        if ((fa & fb & F_OBSERVED) && ((fa ^ fb) & F_INSIDE)) mask |= 1 << (d - 1);
        all &= fb;
        cube |= (fb & F_INSIDE ? 1 : 0) << d;
    }
    int tris = 0;
    if (all & F_OBSERVED) {
#pragma unroll
        for (int q = 0; q < 6; ++q) tris += TET.n[tet_case(q, cube)];
    }
    const size_t at = (size_t)slot * BLOCK_POINTS + tid;
    edge_mask[at] = (uint8_t)mask;
    vertex_count[at] = __popc(mask);
    triangle_count[at] = tris;
}

template <bool COLOUR>
__global__ __launch_bounds__(BLOCK_POINTS) void tsdf_emit_kernel(Geometry g, const int32_t* __restrict__ table,
                                                                 const int32_t* __restrict__ slot_block,
                                                                 const float* __restrict__ tsdf_sum,
                                                                 const float* __restrict__ weight_sum,
                                                                 const float* __restrict__ colour_sum,
                                                                 const uint8_t* __restrict__ edge_mask,
                                                                 const int32_t* __restrict__ vertex_offset,
                                                                 const int32_t* __restrict__ triangle_offset,
                                                                 int n_vertices, int n_faces, float* __restrict__ vertices,
                                                                 float* __restrict__ colours, int32_t* __restrict__ faces) {
    __shared__ int s_slot[8];
    __shared__ float s_T[HALO_POINTS];
    __shared__ int32_t s_voff[HALO_POINTS];
    __shared__ uint8_t s_flag[HALO_POINTS];
    __shared__ uint8_t s_mask[HALO_POINTS];
    const int slot = blockIdx.x, tid = threadIdx.x;
    int bc[3];
    block_of(g, slot_block[slot], bc);
    stage_slots(g, table, bc, s_slot);
    __syncthreads();
    for (int e = tid; e < HALO_POINTS; e += BLOCK_POINTS) {
        int src, local;
        halo_source(e, s_slot, src, local);
        uint8_t fl = 0, mk = 0;
        float T = 0.f;
        int32_t vo = 0;
        if (src >= 0) {
            const size_t a = (size_t)src * BLOCK_POINTS + local;
            const float w = weight_sum[a], ts = tsdf_sum[a];
            if (w > 0.f) {
                fl = F_OBSERVED | (ts < 0.f ? F_INSIDE : 0);
                T = ts / w;
            }
            mk = edge_mask[a];
            vo = vertex_offset[a];
        }
        s_flag[e] = fl;
        s_mask[e] = mk;
        s_T[e] = T;
        s_voff[e] = vo;
    }
    __syncthreads();
    const int li[3] = {tid & 7, (tid >> 3) & 7, tid >> 6};
    const int L = li[0] + 9 * li[1] + 81 * li[2];
    const size_t at = (size_t)slot * BLOCK_POINTS + tid;
    // the vertices of the owned crossing edges
    const int mask = s_mask[L];
    if (mask) {
        const float Ta = s_T[L], wa = weight_sum[at];
        float pa[3], ca[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < 3; ++a) pa[a] = g.origin[a] + g.voxel * (float)(8 * bc[a] + li[a]);
        if constexpr (COLOUR) {
#pragma unroll
            for (int k = 0; k < 3; ++k) ca[k] = colour_sum[((size_t)slot * 3 + k) * BLOCK_POINTS + tid] / wa;
        }
        int id = s_voff[L];
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            if (!((mask >> (d - 1)) & 1) || id >= n_vertices) continue;       // (offsets that are not this volume's scan)
            const int e = L + halo_off(d);
            const float t = Ta / (Ta - s_T[e]);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float pb = g.origin[a] + g.voxel * (float)(8 * bc[a] + li[a] + ((d >> a) & 1));
                vertices[3 * (size_t)id + a] = pa[a] + t * (pb - pa[a]);
            }
            if constexpr (COLOUR) {
                int src, local;
                halo_source(e, s_slot, src, local);                // active: the edge crosses, so its upper end is observed
                const float wb = weight_sum[(size_t)src * BLOCK_POINTS + local];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float cb = colour_sum[((size_t)src * 3 + k) * BLOCK_POINTS + local] / wb;
                    colours[3 * (size_t)id + k] = ca[k] + t * (cb - ca[k]);
                }
            }
            ++id;
        }
    }
    // the faces of the cube this lattice point is the lowest corner of
    int cube = 0, all = F_OBSERVED;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const int fb = s_flag[L + halo_off(d)];
        all &= fb;
        cube |= (fb & F_INSIDE ? 1 : 0) << d;
    }
    if (all & F_OBSERVED) {
        size_t out = 3 * (size_t)triangle_offset[at];
        const size_t end = 3 * (size_t)n_faces;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const int m = tet_case(q, cube);
            const int nv = 3 * TET.n[m];
            for (int v = 0; v < nv && out < end; ++v) {
                const int o = L + halo_off(TET.owner[q][m][v]);
                const int below = (1 << (TET.dir[q][m][v] - 1)) - 1;
                faces[out++] = s_voff[o] + __popc(s_mask[o] & below);
            }
        }
    }
}

Geometry geometry_of(const msgs_tsdf_volume_t& v) {
    Geometry g;
    for (int a = 0; a < 3; ++a) { g.origin[a] = v.origin[a]; g.nb[a] = v.nb[a]; }
    g.voxel = v.voxel_size;
    return g;
}

}  // namespace

hipError_t launch_tsdf_mark_blocks(const msgs_tsdf_volume_t& v, const msgs_tsdf_frames_t& f, int steps, uint8_t* marks,
                                   hipStream_t s) {
    const dim3 grid((unsigned)(((int64_t)f.W * f.H + 255) / 256), (unsigned)f.n), block(256);
    hipLaunchKernelGGL(tsdf_mark_blocks_kernel, grid, block, 0, s, geometry_of(v), f.W, f.H, f.cameras, f.depth, f.sdf_trunc,
                       f.depth_trunc, steps, marks);
    return hipGetLastError();
}

hipError_t launch_tsdf_integrate(const msgs_tsdf_volume_t& v, const msgs_tsdf_frames_t& f, hipStream_t s) {
    const Frames fr{f.n, f.W, f.H, f.cameras, f.depth, f.colour, f.weight, f.sdf_trunc, f.depth_trunc};
    const dim3 grid((unsigned)v.n_slots), block(BLOCK_POINTS);
    if (v.colour_sum)
        hipLaunchKernelGGL(tsdf_integrate_kernel<true>, grid, block, 0, s, geometry_of(v), v.slot_block, v.tsdf_sum, v.weight_sum,
                           v.colour_sum, fr);
    else
        hipLaunchKernelGGL(tsdf_integrate_kernel<false>, grid, block, 0, s, geometry_of(v), v.slot_block, v.tsdf_sum,
                           v.weight_sum, v.colour_sum, fr);
    return hipGetLastError();
}

hipError_t launch_tsdf_count(const msgs_tsdf_volume_t& v, uint8_t* edge_mask, int32_t* vertex_count, int32_t* triangle_count,
                             hipStream_t s) {
    const dim3 grid((unsigned)v.n_slots), block(BLOCK_POINTS);
    hipLaunchKernelGGL(tsdf_count_kernel, grid, block, 0, s, geometry_of(v), v.table, v.slot_block, (const float*)v.tsdf_sum,
                       (const float*)v.weight_sum, edge_mask, vertex_count, triangle_count);
    return hipGetLastError();
}

hipError_t launch_tsdf_emit(const msgs_tsdf_volume_t& v, const msgs_tsdf_mesh_t& m, hipStream_t s) {
    const dim3 grid((unsigned)v.n_slots), block(BLOCK_POINTS);
    if (v.colour_sum)
        hipLaunchKernelGGL(tsdf_emit_kernel<true>, grid, block, 0, s, geometry_of(v), v.table, v.slot_block,
                           (const float*)v.tsdf_sum, (const float*)v.weight_sum, (const float*)v.colour_sum, m.edge_mask,
                           m.vertex_offset, m.triangle_offset, m.n_vertices, m.n_faces, m.vertices, m.colours, m.faces);
    else
        hipLaunchKernelGGL(tsdf_emit_kernel<false>, grid, block, 0, s, geometry_of(v), v.table, v.slot_block,
                           (const float*)v.tsdf_sum, (const float*)v.weight_sum, (const float*)v.colour_sum, m.edge_mask,
                           m.vertex_offset, m.triangle_offset, m.n_vertices, m.n_faces, m.vertices, m.colours, m.faces);
    return hipGetLastError();
}

}  // namespace msgs

// mesh.hip — connected components of a graph and of a triangle mesh, and the mesh's edge report (SPEC M22; 4.24).
//
//   graph_init_kernel         parent[x] = x
//   mesh_corner_keys_kernel   one lane per face corner: the int64 key of the corner's outgoing undirected edge (min << 32 | max) or
//                             of its vertex, and the face it belongs to.  The caller sorts the keys.
//   graph_link_kernel         one lane per edge: unite(a[i], b[i]), or, for a mesh, unite(face[i], face[i + 1]) where the sorted
//                             keys i and i + 1 are equal — a union-find over parent[]
//   graph_flatten_kernel      a launch of its own behind the links: label[x] = root(x)
//   mesh_edge_report_kernel   one lane per sorted key: the head of a run of equal keys classifies it by its length (1, 2, more)
//
// The union-find waits on nobody.  parent[] is written only by atomicMin and read only by relaxed atomic loads, so that
//     parent[x] <= x,     parent[x] only decreases,     parent[x] is a node of x's component
// hold at every instant.  find() walks a strictly decreasing chain; unite() retries only with a strictly smaller larger member
// (4.24 has the argument).  No loop here depends on what another lane or workgroup does next, and none repeats an operation until
// it wins.  The root of a finished component is its smallest node, whatever the schedule was: the labels are a property of the
// input, not of the run.
#include "msgs_internal.h"

namespace msgs {

namespace {

constexpr int LANES = 256;
constexpr unsigned REPORT_BLOCKS = 2048;      // the edge report's grid: 8 workgroups per CU, 3 atomics per wave

__device__ __forceinline__ int32_t parent_of(const int32_t* parent, int32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the node at the end of x's chain.  Every step goes to a strictly smaller non-negative index, so the walk ends after at most x
// steps whatever the memory holds (a word that breaks parent[x] <= x, which no code here writes, ends it at once).
__device__ __forceinline__ int32_t find_root(const int32_t* parent, int32_t x) {
    for (;;) {
        const int32_t p = parent_of(parent, x);
        if ((uint32_t)p >= (uint32_t)x) return x;
        x = p;
    }
}

// joins the trees of a and b.  The larger of the two roots, hi, is hung under the smaller, lo, with one atomicMin.  If hi had
// stopped being a root in the meantime (old != hi), parent[hi] now holds min(old, lo) and the pair (old, lo) is still to be
// united; both are smaller than hi, so the larger member of the pair strictly decreases from round to round.
__device__ __forceinline__ void unite(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicMin(parent + hi, lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
}

__global__ __launch_bounds__(LANES) void graph_init_kernel(int32_t N, int32_t* __restrict__ parent) {
    const int64_t x = (int64_t)blockIdx.x * LANES + threadIdx.x;
    if (x < N) parent[x] = (int32_t)x;
}

// SORTED: edge i joins node[i] and node[i + 1] where key[i] == key[i + 1] (E = n_keys - 1); otherwise it joins a[i] and b[i].
// A node outside [0, N) is the caller's error (the wrappers refuse it); such an edge is left out, never followed.
template <bool SORTED>
__global__ __launch_bounds__(LANES) void graph_link_kernel(int32_t N, int64_t E, const int32_t* __restrict__ a,
                                                           const int32_t* __restrict__ b, const int64_t* __restrict__ key,
                                                           int32_t* parent) {
    const int64_t i = (int64_t)blockIdx.x * LANES + threadIdx.x;
    if (i >= E) return;
    int32_t u, v;
    if constexpr (SORTED) {
        if (key[i] != key[i + 1]) return;
        u = a[i];
        v = a[i + 1];
    } else {
        u = a[i];
        v = b[i];
    }
    if ((uint32_t)u >= (uint32_t)N || (uint32_t)v >= (uint32_t)N || u == v) return;
    unite(parent, u, v);
}

// behind the kernel boundary nothing writes parent[] any more
__global__ __launch_bounds__(LANES) void graph_flatten_kernel(int32_t N, const int32_t* parent, int32_t* __restrict__ label) {
    const int64_t x = (int64_t)blockIdx.x * LANES + threadIdx.x;
    if (x < N) label[x] = find_root(parent, (int32_t)x);
}

template <bool VERTEX>
__global__ __launch_bounds__(LANES) void mesh_corner_keys_kernel(int64_t n_corners, const int32_t* __restrict__ faces,
                                                                 int64_t* __restrict__ keys, int32_t* __restrict__ face_of_key) {
    const int64_t c = (int64_t)blockIdx.x * LANES + threadIdx.x;
    if (c >= n_corners) return;
    const int64_t f = c / 3;
    const int k = (int)(c - 3 * f);
    const int32_t u = faces[c];
    int64_t key = u;
    if constexpr (!VERTEX) {
        const int32_t v = faces[3 * f + (k == 2 ? 0 : k + 1)];
        const int32_t lo = u < v ? u : v, hi = u < v ? v : u;
        key = (int64_t)(((uint64_t)(uint32_t)lo << 32) | (uint32_t)hi);
    }
    keys[c] = key;
    face_of_key[c] = (int32_t)f;
}

// counts3: runs of equal keys of length 1, 2 and more.  A grid-stride loop whose trip count is the same in every lane of a wave
// (it depends on the wave's first key only), the three tallies kept per wave from ballots, then one atomic per wave and class:
// with one atomic per 64 keys instead, 223 000 of them queued on one word and the kernel took 2.7 ms at 14 M keys.
// Integer sums: order-free.
__global__ __launch_bounds__(LANES) void mesh_edge_report_kernel(int64_t n, const int64_t* __restrict__ key,
                                                                 unsigned long long* counts3) {
    const int64_t stride = (int64_t)gridDim.x * LANES;
    const int lane = threadIdx.x & 63;
    unsigned long long tally[3] = {0, 0, 0};
    for (int64_t base = (int64_t)blockIdx.x * LANES + (threadIdx.x - lane); base < n; base += stride) {
        const int64_t i = base + lane;
        int len = 0;                                               // 0: not the head of a run
        if (i < n) {
            const int64_t k = key[i];
            if (i == 0 || key[i - 1] != k)
                len = 1 + (i + 1 < n && key[i + 1] == k ? 1 + (i + 2 < n && key[i + 2] == k ? 1 : 0) : 0);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) tally[c] += (unsigned long long)__popcll(__ballot(len == c + 1));
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
            if (tally[c]) atomicAdd(counts3 + c, tally[c]);
    }
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + LANES - 1) / LANES); }

}  // namespace

hipError_t launch_graph_components(int32_t N, int64_t E, const int32_t* a, const int32_t* b, int32_t* parent, int32_t* label,
                                   hipStream_t s) {
    hipLaunchKernelGGL(graph_init_kernel, dim3(blocks_for(N)), dim3(LANES), 0, s, N, parent);
    if (E > 0)
        hipLaunchKernelGGL(graph_link_kernel<false>, dim3(blocks_for(E)), dim3(LANES), 0, s, N, E, a, b, (const int64_t*)nullptr,
                           parent);
    hipLaunchKernelGGL(graph_flatten_kernel, dim3(blocks_for(N)), dim3(LANES), 0, s, N, (const int32_t*)parent, label);
    return hipGetLastError();
}

hipError_t launch_mesh_corner_keys(int64_t F, const int32_t* faces, bool vertex_mode, int64_t* keys, int32_t* face_of_key,
                                   hipStream_t s) {
    const int64_t n = 3 * F;
    if (vertex_mode)
        hipLaunchKernelGGL(mesh_corner_keys_kernel<true>, dim3(blocks_for(n)), dim3(LANES), 0, s, n, faces, keys, face_of_key);
    else
        hipLaunchKernelGGL(mesh_corner_keys_kernel<false>, dim3(blocks_for(n)), dim3(LANES), 0, s, n, faces, keys, face_of_key);
    return hipGetLastError();
}

hipError_t launch_mesh_link_sorted(int32_t F, int64_t n_keys, const int64_t* keys_sorted, const int32_t* face_sorted,
                                   int32_t* parent, int32_t* label, hipStream_t s) {
    hipLaunchKernelGGL(graph_init_kernel, dim3(blocks_for(F)), dim3(LANES), 0, s, F, parent);
    if (n_keys > 1)
        hipLaunchKernelGGL(graph_link_kernel<true>, dim3(blocks_for(n_keys - 1)), dim3(LANES), 0, s, F, n_keys - 1, face_sorted,
                           (const int32_t*)nullptr, keys_sorted, parent);
    hipLaunchKernelGGL(graph_flatten_kernel, dim3(blocks_for(F)), dim3(LANES), 0, s, F, (const int32_t*)parent, label);
    return hipGetLastError();
}

hipError_t launch_mesh_edge_report(int64_t n_keys, const int64_t* keys_sorted, int64_t* counts3, hipStream_t s) {
    hipError_t e = hipMemsetAsync(counts3, 0, 3 * sizeof(int64_t), s);
    if (e != hipSuccess) return e;
    if (n_keys > 0) {
        const unsigned blocks = blocks_for(n_keys);
        hipLaunchKernelGGL(mesh_edge_report_kernel, dim3(blocks < REPORT_BLOCKS ? blocks : REPORT_BLOCKS), dim3(LANES), 0, s,
                           n_keys, keys_sorted, (unsigned long long*)counts3);
    }
    return hipGetLastError();
}

}  // namespace msgs

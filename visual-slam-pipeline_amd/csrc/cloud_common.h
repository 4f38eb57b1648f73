// cloud_common.h — what cloud.hip and densify.hip share and no other translation unit needs: the search's constants
// and scratch, knn_merge, Scatter3 / scatter_eig, block_rank, Carver / carve_buf and the entry points' size check.
// The arithmetic here is pinned to the last bit by the tests of both files: keep every order as written.
#pragma once

#include "pnp_solvers.h"
#include "vs_internal.h"

namespace vs {

constexpr int kKnnLanes = 256;    // queries per workgroup
constexpr int kKnnMaxSplit = 64;  // workgroups per query block
constexpr int kNoIdx = 0x7fffffff;  // an empty list slot (d2 = +inf)
constexpr int kAxisBits = 21, kAxisBias = 1 << 20;  // a packed cell or voxel coordinate: 21 bits per axis
// a count that exists only on the device (launches are sized for the host's upper bound n_max)
__device__ __forceinline__ int dev_count(const int* d_n, int n_max) { return d_n ? min(*d_n, n_max) : n_max; }
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// cloud.hip's search: the context's scratch for clouds of up to n points, k neighbours and S partial lists;
// k_cloud_knn writes part_d2 / part_idx [S][k][n_max], each list ascending by (d2, index).
struct CloudScratch {
    double *part_d2, *mean, *pts_a, *pts_b;
    int *part_idx, *idx_a, *idx_b;
    uint8_t* flags;
};
int knn_split(vs_ctx* ctx, int n, int forced);
int cloud_scratch(vs_ctx* ctx, int n, int k, int S, CloudScratch* cs);
void launch_knn(const CloudScratch& cs, const double* d_pts, const int* d_n, int n_max, int k, int S, int skip_small,
                hipStream_t s);
// cloud_grid.hip's search on a cell grid: the same lists as launch_knn with S = 1, written to cs.part_d2 / part_idx
// [k][n_max].  cell_edge 0: derived on the device; max_rings 0: the default; d_stats (nullable) [2] = queries finished
// by the rings, by the full scan.  The grid's own scratch is the context's (cloud_grid), sized here.
int launch_knn_grid(vs_ctx* ctx, const CloudScratch& cs, const double* d_pts, const int* d_n, int n_max, int k,
                    int skip_small, double cell_edge, int max_rings, int* d_stats, hipStream_t s);
// the S partial lists merged into vs_cloud_knn_dev's [n][k] output (k_cloud_reduce's list mode)
int cloud_knn_lists(const CloudScratch& cs, const double* d_pts, int n, int k, int* d_nbr, double* d_d2, hipStream_t s,
                    int S = 1);
// VS_ERR_CAPACITY (and the message) when n or k is above what the search holds; called once per entry path
int cloud_size_check(const char* who, int n, int k, int max_points = VS_CLOUD_MAX_POINTS);
// the host-buffer calls behind vs_cloud_filter / vs_cloud_filter_grid and vs_cloud_normals / vs_cloud_normals_grid
int cloud_filter_host(vs_ctx* ctx, const double* pts, int n, const vs_cloud_filter_config* cfg, double* out, int* idx,
                      int counts[3], bool grid);
int cloud_normals_host(vs_ctx* ctx, const double* pts, int n, int k, double* normals, double* eig, bool grid);
// a caller's configuration, or the defaults that def writes
template <class C>
C config_or(const C* cfg, void (*def)(C*)) {
    C c;
    if (cfg)
        c = *cfg;
    else
        def(&c);
    return c;
}

// The count smallest entries of query q's S partial lists (each len long) by (d2, index), in that order:
// emit(rank, d2, index); an empty slot arrives as (+inf, kNoIdx).  cur: the lane's column of a [list][lane] LDS
// array, the entries of each list consumed; a consumed list is skipped.
template <class F>
__device__ __forceinline__ void knn_merge(const double* part_d2, const int* part_idx, int S, int len, int n_max, int q,
                                          uint8_t* cur, int count, F&& emit) {
    for (int s = 0; s < S; s++) cur[s * kKnnLanes] = 0;
    const size_t nm = (size_t)n_max, list = (size_t)len * nm;
    for (int t = 0; t < count; t++) {
        double bd = INFINITY;
        int bi = kNoIdx, bs = 0;
        for (int s = 0; s < S; s++) {
            const int c = cur[s * kKnnLanes];
            if (c >= len) continue;
            const size_t at = (size_t)s * list + (size_t)c * nm + q;
            const double d = part_d2[at];
            const int i = part_idx[at];
            if (d < bd || (d == bd && i < bi)) bd = d, bi = i, bs = s;
        }
        cur[bs * kKnnLanes]++;
        emit(t, bd, bi);
    }
}

// Three cell or voxel coordinates (each in [0, 2^21)) in one word, and the bucket or slot of such a word.
__device__ __forceinline__ unsigned long long pack3(long long x, long long y, long long z) {
    return ((unsigned long long)x << (2 * kAxisBits)) | ((unsigned long long)y << kAxisBits) | (unsigned long long)z;
}
__device__ __forceinline__ bool fits(long long v) { return v >= 0 && v < (1ll << kAxisBits); }
__device__ __forceinline__ unsigned hash_bits(unsigned long long key, int shift) {
    return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> shift);
}

// The six sums of a 3 x 3 scatter matrix, each in the order of the add calls.
struct Scatter3 {
    double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
    __device__ __forceinline__ void add(double dx, double dy, double dz) {
        c00 += dx * dx, c01 += dx * dy, c02 += dx * dz;
        c11 += dy * dy, c12 += dy * dz, c22 += dz * dz;
    }
    __device__ __forceinline__ void fill(double A[9]) const {
        A[0] = c00, A[1] = c01, A[2] = c02, A[3] = c01, A[4] = c11, A[5] = c12, A[6] = c02, A[7] = c12, A[8] = c22;
    }
};

// main.cpp:589-631, :657-669: centroid and scatter of pts[nbr[t * kKnnLanes]], t < count, summed in list order;
// w (descending) and V (columns) as sym_eig_static<3> leaves them (sym_eig<3>'s rotations, indices static).
__device__ __forceinline__ void scatter_eig(const double* pts, const int* nbr, int count, double w[3], double V[9]) {
    double cx = 0, cy = 0, cz = 0;
    for (int t = 0; t < count; t++) {
        const double* p = pts + 3 * (size_t)nbr[t * kKnnLanes];
        cx += p[0], cy += p[1], cz += p[2];
    }
    cx /= (double)count, cy /= (double)count, cz /= (double)count;
    Scatter3 sc;
    for (int t = 0; t < count; t++) {
        const double* p = pts + 3 * (size_t)nbr[t * kKnnLanes];
        sc.add(p[0] - cx, p[1] - cy, p[2] - cz);
    }
    double A[9];
    sc.fill(A);
    vs_pnp::sym_eig_static<3>(A, w, V);
}

// A 1,024-thread block, every thread calling: the number of flagged threads below this one, and the block's
// total.  One barrier; s_w is free again after the next one.
__device__ __forceinline__ int block_rank(bool keep, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s_w[wv] = __popcll(bal);
    __syncthreads();
    int rank = __popcll(bal & ((1ull << lane) - 1ull));
    total = 0;
    for (int w = 0; w < 16; w++) {
        if (w < wv) rank += s_w[w];
        total += s_w[w];
    }
    return rank;
}

// A buffer cut into pieces of whole 256 bytes.  A layout is a function of a Carver&: it runs on a null base for
// the size (the pointers it hands out are null), then on the buffer, so the size and the pieces cannot disagree.
struct Carver {
    char* base;
    size_t used = 0;
    template <class T>
    T* take(size_t count) {
        T* r = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += up256(count * sizeof(T));
        return r;
    }
};
template <class Layout>
int carve_buf(DevBuf& buf, Layout&& layout) {
    Carver size{nullptr};
    layout(size);
    VS_CHECK(buf.ensure(size.used));
    Carver c{buf.as<char>()};
    layout(c);
    return VS_OK;
}

}  // namespace vs

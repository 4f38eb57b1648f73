// cloud.hip — the sparse-map cloud filter (reference src/main.cpp:1185-1215 per processed frame and
// :1340-1368 before the final PLY): a bounding-box clip, statistical_outlier_removal (:512-563) and
// surface_aware_filter (:568-642).  Both filters are an exact k-nearest-neighbour search of every
// point among the others in fp64 (nanoflann kd-tree, L2_Simple_Adaptor) followed by a per-point
// reduction; here the search is brute force, which gives the same distance lists.
//
// Kernels (all enqueue-only; counts that exist only on the device are read from device memory by
// launches sized for the host's upper bound N):
//   k_cloud_knn        one query per lane, 256 queries per workgroup; candidates staged through LDS in
//                      tiles of 1,024 points as x / y / z fp64 arrays (every lane reads the same candidate:
//                      a broadcast).  Per candidate: 3 sub, 3 mul, 2 add in nanoflann's order
//                      ((dx dx + dy dy) + dz dz, no contraction) and one compare against the lane's k-th
//                      distance in a register.  The lane's sorted (d2, index) list lives in LDS as
//                      [slot][lane] and is touched only by an insertion (about k ln(N / k) per query);
//                      insertions are batched per wave through pending slots (knn_flush).
//                      The candidate range is split over S workgroups per query block (grid.y) so that
//                      a small cloud still covers the CUs; each writes its partial list to [S][k][N].
//   k_cloud_reduce     one point per lane: merges the S partial lists by (d2, index) and computes the
//                      mean neighbour distance (stage A), the scatter matrix's eigenvalues and the
//                      keep flag (stage B), or writes the merged list (vs_cloud_knn_dev).  The merge, the
//                      scatter and eigen-solve, the compaction's block rank and the scratch carving are
//                      cloud_common.h's knn_merge, scatter_eig, block_rank and Carver, shared with densify.hip.
//   k_cloud_threshold  one workgroup: mean and population variance of the mean distances in a fixed
//                      order, threshold = mean + std_ratio * std, keep flags.
//   k_cloud_box        keep flags of the inclusive box clip (and of a caller's validity bytes).
//   k_cloud_compact    stable compaction of the flagged points and their original indices; a block
//                      finds its base by summing the flag bytes before it (no second pass, no state).
// Ties: neighbours are ordered by (d2, index); candidates arrive in ascending index, so inside one
// partial list a strict d2 compare keeps the lowest index, and the merge compares both explicitly.
// Matrix instructions do not fit: |a|^2 + |b|^2 - 2 a.b rounds differently from (a - b)^2 and
// cancels for near neighbours.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "block_reduce.h"
#include "cloud_common.h"

namespace vs {

constexpr int kKnnTile = 1024;   // candidates per LDS tile
constexpr int kKnnGroup = 8;     // candidates tested per loop trip (a power of two)
constexpr int kKnnPend = 12;     // pending candidates per lane (> kKnnGroup: a group may append that many)
constexpr int kKnnMinChunk = 512;  // automatic split: at least this many candidates per workgroup
constexpr int kCompact = 1024;   // points per compaction block

enum { kReduceKnn = 0, kReduceMean = 1, kReduceSurface = 2 };

// The lane's sorted list and its pending candidates in LDS, both [slot][lane].  A candidate below the
// lane's k-th distance is only appended to the pending slots (one write); the wave inserts every
// lane's pending candidates together once some lane holds more than kKnnPend - kKnnGroup of them, in
// uniform control flow: with 64 lanes, some lane meets such a candidate in almost every group, so a
// per-lane insertion loop would keep the whole wave in the divergent path.  The k-th distance in the
// register is stale between flushes (it only admits candidates that the flush then rejects).
// A flush stages the lane's list in registers (every index static: VS_CLOUD_MAX_K slots, those past k
// carry the next larger entries and are never read out), inserts the pending candidates there and
// writes the list back, so the LDS round trips are paid once per flush and not once per list slot.
// One insertion: entries above d move up one slot (the last drops out), (d, j) takes the first such
// slot; entries equal to d came earlier, have a lower index and stay in front.
__device__ __forceinline__ double knn_flush(double* l_d2, int* l_idx, const double* p_d2, const int* p_idx, int k,
                                            int cnt) {
    constexpr int K = VS_CLOUD_MAX_K;
    double L[K];
    int I[K];
#pragma unroll
    for (int t = 0; t < K; t++) L[t] = l_d2[t * kKnnLanes], I[t] = l_idx[t * kKnnLanes];
    for (int b = 0; __any(b < cnt); b++) {
        const bool has = b < cnt;
        const double d = has ? p_d2[b * kKnnLanes] : INFINITY;  // +inf: nothing moves
        const int j = has ? p_idx[b * kKnnLanes] : kNoIdx;
        bool above = L[K - 1] > d;
#pragma unroll
        for (int pos = K - 1; pos >= 1; pos--) {
            const bool next_above = L[pos - 1] > d;
            L[pos] = above ? (next_above ? L[pos - 1] : d) : L[pos];
            I[pos] = above ? (next_above ? I[pos - 1] : j) : I[pos];
            above = next_above;
        }
        L[0] = above ? d : L[0];
        I[0] = above ? j : I[0];
    }
#pragma unroll
    for (int t = 0; t < K; t++) l_d2[t * kKnnLanes] = L[t], l_idx[t * kKnnLanes] = I[t];
    return l_d2[(k - 1) * kKnnLanes];
}

// grid (ceil(n_max / 256), S).  part_d2 / part_idx: [S][k][n_max].  skip_small: a filter stage with
// n <= k returns its input unchanged (main.cpp:516, :572), so the search is not needed.
__global__ __launch_bounds__(kKnnLanes) void k_cloud_knn(const double* __restrict__ pts, const int* d_n, int n_max,
                                                         int k, int skip_small, double* __restrict__ part_d2,
                                                         int* __restrict__ part_idx) {
    __shared__ __attribute__((aligned(16))) double s_x[kKnnTile + kKnnGroup], s_y[kKnnTile + kKnnGroup],
        s_z[kKnnTile + kKnnGroup];
    __shared__ double s_d2[VS_CLOUD_MAX_K * kKnnLanes];
    __shared__ int s_idx[VS_CLOUD_MAX_K * kKnnLanes];
    __shared__ double s_pd2[kKnnPend * kKnnLanes];
    __shared__ int s_pidx[kKnnPend * kKnnLanes];
    const int n = dev_count(d_n, n_max);
    const int tid = threadIdx.x, q = blockIdx.x * kKnnLanes + tid;
    if (blockIdx.x * kKnnLanes >= n || (skip_small && n <= k)) return;
    const int S = gridDim.y, chunk = (n + S - 1) / S;
    const int c0 = min(n, (int)blockIdx.y * chunk), c1 = min(n, c0 + chunk);
    const bool live = q < n;
    double qx = 0, qy = 0, qz = 0;
    if (live) {
        qx = pts[3 * (size_t)q];
        qy = pts[3 * (size_t)q + 1];
        qz = pts[3 * (size_t)q + 2];
    }
    double* l_d2 = s_d2 + tid;
    int* l_idx = s_idx + tid;
    double* p_d2 = s_pd2 + tid;
    int* p_idx = s_pidx + tid;
    int pend = 0;
    for (int t = 0; t < VS_CLOUD_MAX_K; t++) {
        l_d2[t * kKnnLanes] = INFINITY;
        l_idx[t * kKnnLanes] = kNoIdx;
    }
    double kth = live ? INFINITY : -1.0;  // a dead lane never appends

    for (int t0 = c0; t0 < c1; t0 += kKnnTile) {
        const int cnt = min(kKnnTile, c1 - t0);
        __syncthreads();  // the previous tile has been read by every lane
        for (int i = tid; i < cnt; i += kKnnLanes) {
            const double* p = pts + 3 * (size_t)(t0 + i);
            s_x[i] = p[0];
            s_y[i] = p[1];
            s_z[i] = p[2];
        }
        // the last group's tail: +inf coordinates give d2 = +inf, which is never below the k-th distance
        if (tid < kKnnGroup && cnt + tid < ((cnt + kKnnGroup - 1) & ~(kKnnGroup - 1)))
            s_x[cnt + tid] = s_y[cnt + tid] = s_z[cnt + tid] = INFINITY;
        __syncthreads();
        // groups of kKnnGroup candidates, the next group's coordinates read from LDS while this one is
        // tested (one wave per SIMD: nothing else hides the LDS latency)
        const int groups = (cnt + kKnnGroup - 1) / kKnnGroup;
        double nx[kKnnGroup], ny[kKnnGroup], nz[kKnnGroup];
#pragma unroll
        for (int u = 0; u < kKnnGroup; u++) nx[u] = s_x[u], ny[u] = s_y[u], nz[u] = s_z[u];
        for (int g = 0; g < groups; g++) {
            const int jj = g * kKnnGroup;
            double d[kKnnGroup];
            bool any = false;
#pragma unroll
            for (int u = 0; u < kKnnGroup; u++) {
                const double dx = qx - nx[u], dy = qy - ny[u], dz = qz - nz[u];
                d[u] = dx * dx + dy * dy + dz * dz;
                any |= d[u] < kth;
            }
#pragma unroll
            for (int u = 0; u < kKnnGroup; u++)  // group g + 1 (the arrays carry one group of slack)
                nx[u] = s_x[jj + kKnnGroup + u], ny[u] = s_y[jj + kKnnGroup + u], nz[u] = s_z[jj + kKnnGroup + u];
            if (__any(any)) {
#pragma unroll
                for (int u = 0; u < kKnnGroup; u++)
                    if (d[u] < kth && t0 + jj + u != q) {
                        p_d2[pend * kKnnLanes] = d[u];
                        p_idx[pend * kKnnLanes] = t0 + jj + u;
                        pend++;
                    }
                if (__any(pend > kKnnPend - kKnnGroup)) {
                    const double now = knn_flush(l_d2, l_idx, p_d2, p_idx, k, pend);
                    kth = live ? now : -1.0;
                    pend = 0;
                }
            }
        }
    }
    if (__any(pend > 0)) knn_flush(l_d2, l_idx, p_d2, p_idx, k, pend);
    if (!live) return;
    const size_t base = (size_t)blockIdx.y * k * n_max + q;
    for (int t = 0; t < k; t++) {
        part_d2[base + (size_t)t * n_max] = l_d2[t * kKnnLanes];
        part_idx[base + (size_t)t * n_max] = l_idx[t * kKnnLanes];
    }
}

struct ReduceArgs {
    const double* pts;
    const int* d_n;
    int n_max, k, S, mode;
    const double* part_d2;
    const int* part_idx;
    double min_anisotropy;
    double* mean;    // kReduceMean: [n]
    uint8_t* flags;  // kReduceSurface: [n]
    int* out_nbr;    // kReduceKnn: [n][k] (-1 = no such neighbour)
    double* out_d2;  //             [n][k] (+inf)
};

__global__ __launch_bounds__(kKnnLanes) void k_cloud_reduce(ReduceArgs a) {
    __shared__ uint8_t s_cur[kKnnMaxSplit * kKnnLanes];  // [list][lane]: entries of the list consumed
    __shared__ int s_nbr[VS_CLOUD_MAX_K * kKnnLanes];    // [slot][lane]: the merged neighbours (stage B)
    const int n = dev_count(a.d_n, a.n_max);
    const int tid = threadIdx.x, q = blockIdx.x * kKnnLanes + tid;
    if (q >= n) return;
    const int k = a.k, S = a.S;
    if (a.mode != kReduceKnn && n <= k) {  // the stage returns its input unchanged
        if (a.mode == kReduceSurface) a.flags[q] = 1;
        return;
    }
    double sum = 0;
    knn_merge(a.part_d2, a.part_idx, S, k, a.n_max, q, s_cur + tid, k, [&](int t, double d2, int idx) {
        if (a.mode == kReduceKnn) {
            a.out_d2[(size_t)q * k + t] = d2;
            a.out_nbr[(size_t)q * k + t] = idx == kNoIdx ? -1 : idx;
        } else if (a.mode == kReduceMean) {
            sum += sqrt(d2);  // main.cpp:536, ascending
        } else {
            s_nbr[t * kKnnLanes + tid] = idx == kNoIdx ? q : idx;  // only with non-finite coordinates
        }
    });
    if (a.mode == kReduceMean) {
        a.mean[q] = sum / k;  // main.cpp:540
    } else if (a.mode == kReduceSurface) {
        // main.cpp:589-631: centroid, scatter summed in neighbour order, eigenvalues, anisotropy
        double w[3], V[9];
        scatter_eig(a.pts, s_nbr + tid, k, w, V);
        const double l1 = w[0], l3 = w[2];
        a.flags[q] = !(l1 < 1e-12) && 1.0 - l3 / l1 >= a.min_anisotropy;
    }
}

// main.cpp:543-557 with a fixed summation order (lane-strided partial sums, then block_sum's tree)
__global__ __launch_bounds__(1024) void k_cloud_threshold(const double* __restrict__ mean, const int* d_n, int n_max,
                                                          int k, double std_ratio, uint8_t* __restrict__ flags) {
    __shared__ double s_red[16];
    const int n = dev_count(d_n, n_max);
    const int tid = threadIdx.x;
    if (n <= k) {
        for (int i = tid; i < n; i += 1024) flags[i] = 1;
        return;
    }
    double v[1] = {0}, tot[1];
    for (int i = tid; i < n; i += 1024) v[0] += mean[i];
    block_sum<1, 16>(v, s_red, tot);
    const double gmean = tot[0] / n;
    v[0] = 0;
    for (int i = tid; i < n; i += 1024) v[0] += (mean[i] - gmean) * (mean[i] - gmean);
    block_sum<1, 16>(v, s_red, tot);
    const double thr = gmean + std_ratio * sqrt(tot[0] / n);
    for (int i = tid; i < n; i += 1024) flags[i] = mean[i] <= thr;
}

struct Box {
    double lo[3], hi[3];
};

// main.cpp:1203-1205 (inclusive), and-ed with the caller's validity bytes when given
__global__ __launch_bounds__(256) void k_cloud_box(const double* __restrict__ pts, int n, const uint8_t* pre, int use_box,
                                                   Box b, uint8_t* __restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool keep = pre ? pre[i] != 0 : true;
    if (use_box) {
        const double x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        keep = keep && x >= b.lo[0] && x <= b.hi[0] && y >= b.lo[1] && y <= b.hi[1] && z >= b.lo[2] && z <= b.hi[2];
    }
    flags[i] = keep;
}

// Stable compaction: out / idx_out receive the flagged points (flags == nullptr: all) in input order,
// *d_n_out their count.  flags holds 0 / 1 bytes, 16-byte aligned.  Block b owns points [1024 b,
// 1024 b + 1024) and finds its base as the number of set bytes before them (b x 64 16-byte words,
// read by the whole block).  idx_in == nullptr: identity.  in and out must not overlap.
__global__ __launch_bounds__(kCompact) void k_cloud_compact(const double* __restrict__ in, const int* __restrict__ idx_in,
                                                            const uint8_t* __restrict__ flags, const int* d_n_in,
                                                            int n_max, double* __restrict__ out,
                                                            int* __restrict__ idx_out, int* __restrict__ d_n_out) {
    __shared__ int s_w[16];
    __shared__ int s_base;
    const int n = dev_count(d_n_in, n_max);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int first = blockIdx.x * kCompact, i = first + tid;
    if (first >= n && blockIdx.x > 0) return;
    int before = 0;
    if (flags) {
        const uint4* f4 = reinterpret_cast<const uint4*>(flags);
        for (int w = tid; w < (int)blockIdx.x * (kCompact / 16); w += kCompact) {
            const uint4 v = f4[w];
            before += __popc(v.x & 0x01010101u) + __popc(v.y & 0x01010101u) + __popc(v.z & 0x01010101u) +
                      __popc(v.w & 0x01010101u);
        }
        for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o);
        if (lane == 0) s_w[wv] = before;
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < 16; w++) t += s_w[w];
            s_base = t;
        }
        __syncthreads();
        before = s_base;
        __syncthreads();
    } else {
        before = first;
    }
    const bool keep = i < n && (flags ? flags[i] != 0 : true);
    int total;
    const int rank = before + block_rank(keep, s_w, total);
    if (keep) {
        out[3 * (size_t)rank] = in[3 * (size_t)i];
        out[3 * (size_t)rank + 1] = in[3 * (size_t)i + 1];
        out[3 * (size_t)rank + 2] = in[3 * (size_t)i + 2];
        idx_out[rank] = idx_in ? idx_in[i] : i;
    }
    if (tid == 0 && first + kCompact >= n) *d_n_out = before + total;  // the block of the last point (or block 0)
}

// workgroups per query block: enough for blocks x S to cover the CUs, chunks of >= kKnnMinChunk candidates
int knn_split(vs_ctx* ctx, int n, int forced) {
    if (forced > 0) return std::min(forced, kKnnMaxSplit);
    if (ctx->cloud_cus == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus <= 0)
            cus = 256;
        ctx->cloud_cus = cus;
    }
    const int blocks = (n + kKnnLanes - 1) / kKnnLanes;
    const int want = (ctx->cloud_cus + blocks - 1) / blocks;
    return std::max(1, std::min({want, n / kKnnMinChunk, kKnnMaxSplit}));
}

// The context's scratch for clouds of up to n points, k neighbours and S partial lists (cloud_common.h).
int cloud_scratch(vs_ctx* ctx, int n, int k, int S, CloudScratch* cs) {
    const size_t nk = (size_t)std::max(S, 1) * std::max(k, 1) * n;
    return carve_buf(ctx->cloud, [&](Carver& c) {
        cs->part_d2 = c.take<double>(nk);
        cs->part_idx = c.take<int>(nk);
        cs->pts_a = c.take<double>((size_t)n * 3);
        cs->pts_b = c.take<double>((size_t)n * 3);
        cs->idx_a = c.take<int>(n);
        cs->idx_b = c.take<int>(n);
        cs->mean = c.take<double>(n);
        cs->flags = c.take<uint8_t>((size_t)n + kCompact);  // k_cloud_compact reads whole 16-byte words below n
    });
}

int cloud_size_check(const char* who, int n, int k, int max_points) {
    if (n <= max_points && k <= VS_CLOUD_MAX_K) return VS_OK;
    set_error(std::string(who) + (n <= max_points                   ? ": more than VS_CLOUD_MAX_K neighbours"
                                  : max_points == VS_CLOUD_MAX_POINTS ? ": more than VS_CLOUD_MAX_POINTS points"
                                                                      : ": more than VS_CLOUD_GRID_MAX_POINTS points"));
    return VS_ERR_CAPACITY;
}

void launch_knn(const CloudScratch& cs, const double* d_pts, const int* d_n, int n_max, int k, int S, int skip_small,
                hipStream_t s) {
    hipLaunchKernelGGL(k_cloud_knn, dim3((n_max + kKnnLanes - 1) / kKnnLanes, S), dim3(kKnnLanes), 0, s, d_pts, d_n,
                       n_max, k, skip_small, cs.part_d2, cs.part_idx);
}

// the partial lists [S][k][n] (S = 1: a grid search's single list) as vs_cloud_knn_dev's [n][k] output
// (k_cloud_reduce's list mode)
int cloud_knn_lists(const CloudScratch& cs, const double* d_pts, int n, int k, int* d_nbr, double* d_d2, hipStream_t s,
                    int S) {
    ReduceArgs r{d_pts, nullptr, n, k, S, kReduceKnn, cs.part_d2, cs.part_idx, 0.0, nullptr, nullptr, d_nbr, d_d2};
    hipLaunchKernelGGL(k_cloud_reduce, dim3((n + kKnnLanes - 1) / kKnnLanes), dim3(kKnnLanes), 0, s, r);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

namespace {

void launch_compact(const double* in, const int* idx_in, const uint8_t* flags, const int* d_n_in, int n_max,
                    double* out, int* idx_out, int* d_n_out, hipStream_t s) {
    hipLaunchKernelGGL(k_cloud_compact, dim3(std::max(1, (n_max + kCompact - 1) / kCompact)), dim3(kCompact), 0, s, in,
                       idx_in, flags, d_n_in, n_max, out, idx_out, d_n_out);
}

int filter_check(const vs_cloud_filter_config& c, int n, bool grid) {
    VS_ARG(c.sor_k >= 0 && c.surf_k >= 0, "vs_cloud_filter: negative neighbour count");
    return cloud_size_check("vs_cloud_filter", n, std::max(c.sor_k, c.surf_k),
                            grid ? VS_CLOUD_GRID_MAX_POINTS : VS_CLOUD_MAX_POINTS);
}

// the launches of cloud_filter; the caller has run filter_check
int filter_enqueue(vs_ctx* ctx, const double* d_pts, int n, const uint8_t* d_pre, const vs_cloud_filter_config& c,
                   double* d_out, int* d_idx, int* d_counts, hipStream_t s, bool grid) {
    const int S = n > 0 && !grid ? knn_split(ctx, n, 0) : 1;
    CloudScratch cs;
    VS_CHECK(cloud_scratch(ctx, std::max(n, 1), std::max(c.sor_k, c.surf_k), S, &cs));
    ProfScope ps(ctx, grid ? "cloud_filter_grid" : "cloud_filter", s);
    // a stage's search: brute force, or the cell grid rebuilt on the stage's points (cloud_grid.hip)
    auto search = [&](const double* pts, const int* d_n, int k) {
        if (grid) return launch_knn_grid(ctx, cs, pts, d_n, n, k, 1, 0.0, 0, nullptr, s);
        launch_knn(cs, pts, d_n, n, k, S, 1, s);
        return (int)VS_OK;
    };
    const int qblocks = std::max(1, (n + kKnnLanes - 1) / kKnnLanes);
    // the clip (main.cpp:1193-1209)
    const bool clip = c.use_bbox || d_pre;
    if (clip && n > 0) {
        Box b;
        for (int a = 0; a < 3; a++) b.lo[a] = c.bbox_min[a], b.hi[a] = c.bbox_max[a];
        hipLaunchKernelGGL(k_cloud_box, dim3((n + 255) / 256), dim3(256), 0, s, d_pts, n, d_pre, c.use_bbox, b, cs.flags);
    }
    launch_compact(d_pts, nullptr, clip ? cs.flags : nullptr, nullptr, n, cs.pts_a, cs.idx_a, d_counts, s);
    // stage A (main.cpp:512-563) on the clipped points
    if (c.sor_k > 0 && n > 0) {
        VS_CHECK(search(cs.pts_a, d_counts, c.sor_k));
        ReduceArgs r{cs.pts_a, d_counts, n, c.sor_k, S, kReduceMean, cs.part_d2, cs.part_idx, 0.0, cs.mean, nullptr,
                     nullptr, nullptr};
        hipLaunchKernelGGL(k_cloud_reduce, dim3(qblocks), dim3(kKnnLanes), 0, s, r);
        hipLaunchKernelGGL(k_cloud_threshold, dim3(1), dim3(1024), 0, s, cs.mean, d_counts, n, c.sor_k, c.sor_std_ratio,
                           cs.flags);
    }
    launch_compact(cs.pts_a, cs.idx_a, c.sor_k > 0 ? cs.flags : nullptr, d_counts, n, cs.pts_b, cs.idx_b, d_counts + 1,
                   s);
    // stage B (main.cpp:568-642) on stage A's survivors
    if (c.surf_k > 0 && n > 0) {
        VS_CHECK(search(cs.pts_b, d_counts + 1, c.surf_k));
        ReduceArgs r{cs.pts_b, d_counts + 1, n, c.surf_k, S, kReduceSurface, cs.part_d2, cs.part_idx,
                     c.surf_min_anisotropy, nullptr, cs.flags, nullptr, nullptr};
        hipLaunchKernelGGL(k_cloud_reduce, dim3(qblocks), dim3(kKnnLanes), 0, s, r);
    }
    launch_compact(cs.pts_b, cs.idx_b, c.surf_k > 0 ? cs.flags : nullptr, d_counts + 1, n, d_out, d_idx, d_counts + 2,
                   s);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

}  // namespace

int cloud_filter(vs_ctx* ctx, const double* d_pts, int n, const uint8_t* d_pre, const vs_cloud_filter_config& c,
                 double* d_out, int* d_idx, int* d_counts, hipStream_t s, bool grid) {
    VS_CHECK(filter_check(c, n, grid));
    return filter_enqueue(ctx, d_pts, n, d_pre, c, d_out, d_idx, d_counts, s, grid);
}

int cloud_filter_host(vs_ctx* ctx, const double* pts, int n, const vs_cloud_filter_config* cfg, double* out, int* idx,
                      int counts[3], bool grid) {
    VS_ARG(ctx && out && idx && counts && n >= 0 && (n == 0 || pts), "vs_cloud_filter: null argument");
    const vs_cloud_filter_config c = config_or(cfg, vs_cloud_filter_default_config);
    VS_CHECK(filter_check(c, n, grid));  // before the staging is sized by n
    VS_HIP(hipSetDevice(ctx->device));
    const hipStream_t s = ctx->stream;
    const size_t cnt = (size_t)std::max(n, 1);
    double *d_in, *d_out;
    int *d_idx, *d_counts;
    VS_CHECK(carve_buf(ctx->h_aux0, [&](Carver& h) {
        d_in = h.take<double>(cnt * 3);
        d_out = h.take<double>(cnt * 3);
        d_idx = h.take<int>(cnt);
        d_counts = h.take<int>(3);
    }));
    if (n > 0) VS_HIP(hipMemcpyAsync(d_in, pts, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    VS_CHECK(filter_enqueue(ctx, d_in, n, nullptr, c, d_out, d_idx, d_counts, s, grid));
    VS_HIP(hipMemcpyAsync(counts, d_counts, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
    VS_HIP(hipStreamSynchronize(s));
    const int m = counts[2];
    if (m > 0) {
        VS_HIP(hipMemcpyAsync(out, d_out, (size_t)m * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
        VS_HIP(hipMemcpyAsync(idx, d_idx, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, s));
        VS_HIP(hipStreamSynchronize(s));
    }
    return VS_OK;
}

}  // namespace vs

using namespace vs;

extern "C" {

void vs_cloud_filter_default_config(vs_cloud_filter_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->sor_k = 25;  // main.cpp:1211, :1368
    c->sor_std_ratio = 0.6;
    c->surf_k = 25;
    c->surf_min_anisotropy = 0.4;
}

int vs_cloud_knn_dev(vs_ctx* ctx, const double* d_pts, int n, int k, int split, int* d_nbr, double* d_d2,
                     void* stream) {
    VS_ARG(ctx && d_pts && d_nbr && d_d2, "vs_cloud_knn_dev: null argument");
    VS_ARG(n >= 0 && k >= 1 && split >= 0 && split <= kKnnMaxSplit, "vs_cloud_knn_dev: bad size");
    VS_CHECK(cloud_size_check("vs_cloud_knn_dev", n, k));
    if (n == 0) return VS_OK;
    VS_HIP(hipSetDevice(ctx->device));
    const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const int S = knn_split(ctx, n, split);
    CloudScratch cs;
    VS_CHECK(cloud_scratch(ctx, n, k, S, &cs));
    ProfScope ps(ctx, "cloud_knn", s);
    launch_knn(cs, d_pts, nullptr, n, k, S, 0, s);
    ReduceArgs r{d_pts, nullptr, n, k, S, kReduceKnn, cs.part_d2, cs.part_idx, 0.0, nullptr, nullptr, d_nbr, d_d2};
    hipLaunchKernelGGL(k_cloud_reduce, dim3((n + kKnnLanes - 1) / kKnnLanes), dim3(kKnnLanes), 0, s, r);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int vs_cloud_filter_dev(vs_ctx* ctx, const double* d_pts, int n, const vs_cloud_filter_config* cfg, double* d_out,
                        int* d_idx, int* d_counts, void* stream) {
    VS_ARG(ctx && d_out && d_idx && d_counts && n >= 0 && (n == 0 || d_pts), "vs_cloud_filter_dev: null argument");
    VS_HIP(hipSetDevice(ctx->device));
    return cloud_filter(ctx, d_pts, n, nullptr, config_or(cfg, vs_cloud_filter_default_config), d_out, d_idx, d_counts,
                        stream ? (hipStream_t)stream : ctx->stream);
}

int vs_cloud_filter(vs_ctx* ctx, const double* pts, int n, const vs_cloud_filter_config* cfg, double* out, int* idx,
                    int counts[3]) {
    return cloud_filter_host(ctx, pts, n, cfg, out, idx, counts, false);
}

}  // extern "C"

// cloud_mesh.hip — compute_mesh (reference src/main.cpp:689-774) on the device: the local fan triangulation that
// turns the filtered, densified cloud and its normals into an index triple list.  All arithmetic is fp64 in the
// written order, compiled without contraction; sums of three products are (a + b) + c.
//
// For every point i, in input order: its min(k, n) - 1 nearest others by (d2, index) (cloud.hip's brute-force search
// or cloud_grid.hip's, merged to an [n][k - 1] list by k_cloud_reduce; neither search changes); a tangent basis from
// the caller's normal; the neighbours within max_edge whose normal is nearly parallel; their angles in the tangent
// plane, sorted by (angle, list position); one triangle (i, b, c) per cyclically consecutive pair that passes the
// gap and the long-edge test.  Triangles come out by centre point, then by fan position.
//
// The unit of work is one point and its <= 31 neighbours: one point per half-wave, lane t = neighbour t, two points
// per wave, 8 per 256-lane workgroup.  Every exchange is a shuffle or a ballot inside the half-wave; no LDS.
//   k_mesh_fan    gather: lane t loads its neighbour's index and d2 from the list, then that neighbour's point and
//                 normal (the one random HBM access); lane 0's centre point and normal are broadcast by shuffle and
//                 the basis is computed redundantly in every lane.  The validity ballot's half is the 32-bit mask of
//                 the point.  Sort: a 32-lane bitonic network (15 compare-exchange steps of __shfl_xor) over
//                 (angle, list position) with +inf as an invalid lane's angle, so the m valid lanes end in front;
//                 only the key travels: afterwards the lane fetches index and point from the list position's lane.
//                 Fan walk: lane j reads lane (j + 1 mod m)'s angle, index and point by shuffle and applies the gap
//                 and edge tests; the ballot over lanes < m is the emit mask.  Writes the sorted indices [n][k - 1],
//                 the emit mask and m: 4 (k - 1) + 8 bytes per point, no triangle slots.  A half-wave with m < 2 or
//                 past the last point runs through with nothing valid: the wave's other half may be working.
//   k_mesh_sums   tiles of 4,096 points: the tile's triangle count and its points with a triangle
//   k_mesh_offs   the exclusive prefix sum of the counts: a tile's base is the sum of the tile sums before it (at most
//                 2,048 of them, summed by the workgroup: no third launch, no state), then a scan inside the tile;
//                 the first workgroup writes d_counts
//   k_mesh_emit   again one point per half-wave: lane j with its mask bit set writes (i, b, c) at
//                 offset[i] + popcount(mask below j) when that is below cap.  No atomic takes part in a position: the
//                 list is in the reference's order by construction and the same from run to run.
// The triangle total is at most n (k - 1) <= 2^23 x 31 < 2^31, so offsets and counts are 32-bit (static_assert).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "cloud_common.h"

namespace vs {

namespace {

constexpr int kHalf = 32;                      // lanes per point
constexpr int kMeshBlock = 256;                // 8 points per workgroup
constexpr int kPerBlock = kMeshBlock / kHalf;
constexpr int kTile = 4096;                    // points per workgroup of the offset scan, 4 per lane
constexpr int kNormalK = 20;                   // main.cpp:1379: the normals the host call computes when given none
static_assert(VS_CLOUD_MAX_K <= kHalf, "a point's neighbours must fit the half-wave");
static_assert((long long)VS_CLOUD_GRID_MAX_POINTS * (VS_CLOUD_MAX_K - 1) <= INT_MAX, "32-bit triangle offsets");
static_assert(VS_CLOUD_GRID_MAX_POINTS / kTile <= 2 * 1024, "k_mesh_offs sums two tile sums per lane");

struct Mesh {
    const double* pts;      // [n][3]
    const double* normals;  // [n][3]
    int n, kk;              // kk = k - 1: the list's row length
    double max_edge2, long_edge2, normal_thresh, max_gap;
    const int* nbr;     // [n][kk] by (d2, index), -1 past the n - 1 others
    const double* d2;   // [n][kk]
    int* sorted;        // [n][kk] neighbour indices by (angle, list position), the valid ones first
    uint2* fan;         // [n] {emit mask, valid neighbours m}
    int* off;           // [n] triangles before point i
    int2* tsum;         // [tiles] {triangles, points with a triangle}
    int cap;
    int* tri;           // [cap][3]
    int* counts;        // [2]
};

__device__ __forceinline__ double dot3(double ax, double ay, double az, double bx, double by, double bz) {
    return (ax * bx + ay * by) + az * bz;
}
// this half-wave's 32 bits of a wave ballot
__device__ __forceinline__ unsigned half_ballot(bool b) { return (unsigned)(__ballot(b) >> (threadIdx.x & kHalf)); }

__global__ __launch_bounds__(kMeshBlock) void k_mesh_fan(Mesh a) {
    const int t = threadIdx.x & (kHalf - 1);
    const int i = blockIdx.x * kPerBlock + (threadIdx.x >> 5);
    const bool live = i < a.n;
    const size_t row = (size_t)(live ? i : 0) * a.kk;

    // ---- gather: the list entry, the neighbour's point and normal; the centre once per half-wave
    int j = -1;
    double d2 = INFINITY;
    if (live && t < a.kk) j = a.nbr[row + t], d2 = a.d2[row + t];
    const bool has = j >= 0;
    double qx = 0, qy = 0, qz = 0, mx = 0, my = 0, mz = 0;
    if (has) {
        const double *p = a.pts + 3 * (size_t)j, *m = a.normals + 3 * (size_t)j;
        qx = p[0], qy = p[1], qz = p[2], mx = m[0], my = m[1], mz = m[2];
    }
    double cx = 0, cy = 0, cz = 0, nx = 0, ny = 0, nz = 0;
    if (live && t == 0) {
        const double *p = a.pts + 3 * (size_t)i, *m = a.normals + 3 * (size_t)i;
        cx = p[0], cy = p[1], cz = p[2], nx = m[0], ny = m[1], nz = m[2];
    }
    cx = __shfl(cx, 0, kHalf), cy = __shfl(cy, 0, kHalf), cz = __shfl(cz, 0, kHalf);
    nx = __shfl(nx, 0, kHalf), ny = __shfl(ny, 0, kHalf), nz = __shfl(nz, 0, kHalf);

    // ---- the tangent basis (main.cpp:726-732): up = the axis of the smallest |n| component, u = normalize(n x up),
    // v = n x u; a zero cross product stays zero (Eigen's normalized())
    const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
    const bool up_x = ax <= ay && ax <= az, up_y = !up_x && ay <= az;
    const double ox = up_x ? 1.0 : 0.0, oy = up_y ? 1.0 : 0.0, oz = (up_x || up_y) ? 0.0 : 1.0;
    double ux = ny * oz - nz * oy, uy = nz * ox - nx * oz, uz = nx * oy - ny * ox;
    const double un = dot3(ux, uy, uz, ux, uy, uz);
    if (un > 0) {
        const double len = sqrt(un);
        ux /= len, uy /= len, uz /= len;
    }
    const double vx = ny * uz - nz * uy, vy = nz * ux - nx * uz, vz = nx * uy - ny * ux;

    // ---- valid neighbours (main.cpp:737-746): > and < reject
    const bool valid = has && !(d2 > a.max_edge2) && !(fabs(dot3(nx, ny, nz, mx, my, mz)) < a.normal_thresh);
    const int m = __popc(half_ballot(valid));
    const double dx = qx - cx, dy = qy - cy, dz = qz - cz;
    double ang = valid ? atan2(dot3(dx, dy, dz, vx, vy, vz), dot3(dx, dy, dz, ux, uy, uz)) : INFINITY;
    int pos = t;

    // ---- bitonic sort of (angle, list position), ascending over the 32 lanes
#pragma unroll
    for (int k2 = 2; k2 <= kHalf; k2 <<= 1)
#pragma unroll
        for (int o = k2 >> 1; o > 0; o >>= 1) {
            const double oa = __shfl_xor(ang, o, kHalf);
            const int op = __shfl_xor(pos, o, kHalf);
            const bool other_less = oa < ang || (oa == ang && op < pos);
            const bool want_min = ((t & o) == 0) == ((t & k2) == 0);  // k2 = 32: every lane ascending
            if (other_less == want_min) ang = oa, pos = op;
        }

    // ---- the fan (main.cpp:754-772): sorted lane s < m against lane s + 1, the last against lane 0
    const int b = __shfl(j, pos, kHalf);
    const double bx = __shfl(qx, pos, kHalf), by = __shfl(qy, pos, kHalf), bz = __shfl(qz, pos, kHalf);
    const bool wrap = t + 1 >= m;
    const int nxt = wrap ? 0 : t + 1;
    const double na = __shfl(ang, nxt, kHalf);
    const double ex = bx - __shfl(bx, nxt, kHalf), ey = by - __shfl(by, nxt, kHalf), ez = bz - __shfl(bz, nxt, kHalf);
    double gap = na - ang;
    if (wrap) gap += 2.0 * M_PI;
    const bool emit = m >= 2 && t < m && !(gap > a.max_gap) && !(dot3(ex, ey, ez, ex, ey, ez) > a.long_edge2);
    const unsigned mask = half_ballot(emit);
    if (live && t < a.kk) a.sorted[row + t] = b;
    if (live && t == 0) a.fan[i] = make_uint2(mask, (unsigned)m);
}

// A 1,024-lane workgroup's exclusive prefix of v over its lanes, and the total.  s_w [16]; one barrier.
__device__ __forceinline__ int block_prefix(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = 0; w < 16; w++) {
        if (w < wv) before += s_w[w];
        total += s_w[w];
    }
    return before + inc - v;
}

// the triangle counts of the lane's four points (tile b, entries 4 tid .. 4 tid + 3; 0 past n)
__device__ __forceinline__ void tile_counts(const Mesh& a, int c[4]) {
    const int first = blockIdx.x * kTile + 4 * threadIdx.x;
    for (int e = 0; e < 4; e++) c[e] = first + e < a.n ? __popc(a.fan[first + e].x) : 0;
}

__global__ __launch_bounds__(1024) void k_mesh_sums(Mesh a) {
    __shared__ int s_w[16];
    int c[4], tris, with;
    tile_counts(a, c);
    block_prefix(c[0] + c[1] + c[2] + c[3], s_w, tris);
    __syncthreads();  // s_w is read before the second use
    block_prefix((c[0] > 0) + (c[1] > 0) + (c[2] > 0) + (c[3] > 0), s_w, with);
    if (threadIdx.x == 0) a.tsum[blockIdx.x] = make_int2(tris, with);
}

__global__ __launch_bounds__(1024) void k_mesh_offs(Mesh a) {
    __shared__ int s_w[16];
    const int tid = threadIdx.x, tiles = gridDim.x;
    int before = 0, tris = 0, with = 0;  // this lane's share of the tile sums: in front of this tile, and all
    for (int w = tid; w < tiles; w += 1024) {
        const int2 s = a.tsum[w];
        if (w < (int)blockIdx.x) before += s.x;
        tris += s.x, with += s.y;
    }
    int base, all_tris, all_with, unused;
    block_prefix(before, s_w, base);
    __syncthreads();
    block_prefix(tris, s_w, all_tris);
    __syncthreads();
    block_prefix(with, s_w, all_with);
    __syncthreads();
    if (blockIdx.x == 0 && tid == 0) a.counts[0] = all_tris, a.counts[1] = all_with;
    int c[4];
    tile_counts(a, c);
    int run = base + block_prefix(c[0] + c[1] + c[2] + c[3], s_w, unused);
    const int first = blockIdx.x * kTile + 4 * tid;
    for (int e = 0; e < 4 && first + e < a.n; e++) {
        a.off[first + e] = run;
        run += c[e];
    }
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_emit(Mesh a) {
    const int t = threadIdx.x & (kHalf - 1);
    const int i = blockIdx.x * kPerBlock + (threadIdx.x >> 5);
    if (i >= a.n) return;  // nothing below is exchanged between lanes
    const uint2 f = a.fan[i];
    if (!((f.x >> t) & 1u)) return;
    const int at = a.off[i] + __popc(f.x & ((1u << t) - 1u));
    if (at >= a.cap) return;
    const size_t row = (size_t)i * a.kk;  // a set bit t: t < m <= kk
    int* out = a.tri + 3 * (size_t)at;
    out[0] = i;
    out[1] = a.sorted[row + t];
    out[2] = a.sorted[row + (t + 1 >= (int)f.y ? 0 : t + 1)];
}

__global__ void k_mesh_empty(int* counts) {
    if (threadIdx.x < 2) counts[threadIdx.x] = 0;
}

int mesh_check(const char* who, const vs_cloud_mesh_config& c, int n) {
    if (c.k < 2 || !(c.max_edge > 0) || !std::isfinite(c.max_edge) || !std::isfinite(c.normal_thresh) ||
        !std::isfinite(c.max_ang_gap)) {
        set_error(std::string(who) + ": k < 2, max_edge not positive, or a threshold that is not finite");
        return VS_ERR_ARG;
    }
    return cloud_size_check(who, n, c.k, c.use_grid ? VS_CLOUD_GRID_MAX_POINTS : VS_CLOUD_MAX_POINTS);
}

// the launches; the caller has run mesh_check
int mesh_enqueue(vs_ctx* ctx, const double* d_pts, const double* d_normals, int n, const vs_cloud_mesh_config& c,
                 int cap, int* d_tri, int* d_counts, hipStream_t s) {
    if (n < 3) {  // main.cpp:699
        hipLaunchKernelGGL(k_mesh_empty, dim3(1), dim3(64), 0, s, d_counts);
        VS_HIP(hipGetLastError());
        return VS_OK;
    }
    const bool grid = c.use_grid != 0;
    Mesh a{};
    a.pts = d_pts, a.normals = d_normals, a.n = n, a.kk = c.k - 1;
    a.max_edge2 = c.max_edge * c.max_edge;  // main.cpp:710, :764
    a.long_edge2 = a.max_edge2 * 2.5;
    a.normal_thresh = c.normal_thresh, a.max_gap = c.max_ang_gap;
    a.cap = cap, a.tri = d_tri, a.counts = d_counts;
    const int tiles = (n + kTile - 1) / kTile;
    int* nbr;
    double* d2;
    VS_CHECK(carve_buf(ctx->cloud_mesh, [&](Carver& p) {
        nbr = p.take<int>((size_t)n * a.kk);
        d2 = p.take<double>((size_t)n * a.kk);
        a.sorted = p.take<int>((size_t)n * a.kk);
        a.fan = p.take<uint2>(n);
        a.off = p.take<int>(n);
        a.tsum = p.take<int2>(tiles);
    }));
    a.nbr = nbr, a.d2 = d2;
    // the search with k - 1 and the merge of its S partial lists into [n][k - 1]
    const int S = grid ? 1 : knn_split(ctx, n, 0);
    CloudScratch cs;
    VS_CHECK(cloud_scratch(ctx, n, a.kk, S, &cs));
    if (grid) {
        VS_CHECK(launch_knn_grid(ctx, cs, d_pts, nullptr, n, a.kk, 0, 0.0, 0, nullptr, s));
    } else {
        ProfScope ps(ctx, "k_cloud_knn", s);
        launch_knn(cs, d_pts, nullptr, n, a.kk, S, 0, s);
    }
    {
        ProfScope ps(ctx, "k_cloud_reduce", s);
        VS_CHECK(cloud_knn_lists(cs, d_pts, n, a.kk, nbr, d2, s, S));
    }
    const int pblocks = (n + kPerBlock - 1) / kPerBlock;
#define MESH_LAUNCH(kernel, grid, block)                                \
    do {                                                                \
        ProfScope ps_(ctx, #kernel, s);                                 \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, a);   \
    } while (0)
    MESH_LAUNCH(k_mesh_fan, pblocks, kMeshBlock);
    MESH_LAUNCH(k_mesh_sums, tiles, 1024);
    MESH_LAUNCH(k_mesh_offs, tiles, 1024);
    MESH_LAUNCH(k_mesh_emit, pblocks, kMeshBlock);
#undef MESH_LAUNCH
    VS_HIP(hipGetLastError());
    return VS_OK;
}

}  // namespace

}  // namespace vs

using namespace vs;

extern "C" {

void vs_cloud_mesh_default_config(vs_cloud_mesh_config* c) {
    if (!c) return;
    c->k = 20;  // main.cpp:708-711, :696
    c->max_edge = 0.12;
    c->normal_thresh = 0.5;
    c->max_ang_gap = 1.2;
    c->use_grid = 0;
}

int vs_cloud_mesh_dev(vs_ctx* ctx, const double* d_pts, const double* d_normals, int n, const vs_cloud_mesh_config* cfg,
                      int cap, int* d_tri, int* d_counts, void* stream) {
    VS_ARG(ctx && d_counts && n >= 0 && cap >= 0 && (cap == 0 || d_tri) && (n == 0 || (d_pts && d_normals)),
           "vs_cloud_mesh_dev: null argument or bad size");
    const vs_cloud_mesh_config c = config_or(cfg, vs_cloud_mesh_default_config);
    VS_CHECK(mesh_check("vs_cloud_mesh_dev", c, n));
    VS_HIP(hipSetDevice(ctx->device));
    return mesh_enqueue(ctx, d_pts, d_normals, n, c, cap, d_tri, d_counts, stream ? (hipStream_t)stream : ctx->stream);
}

int vs_cloud_mesh(vs_ctx* ctx, const double* pts, const double* normals, int n, const vs_cloud_mesh_config* cfg, int cap,
                  int* tri, int counts[2], double* normals_out, double* tri_verts, double* tri_normals) {
    VS_ARG(ctx && counts && n >= 0 && cap >= 0 && (cap == 0 || tri) && (n == 0 || pts),
           "vs_cloud_mesh: null argument or bad size");
    const vs_cloud_mesh_config c = config_or(cfg, vs_cloud_mesh_default_config);
    VS_CHECK(mesh_check("vs_cloud_mesh", c, n));  // before the staging is sized by n
    VS_HIP(hipSetDevice(ctx->device));
    const hipStream_t s = ctx->stream;
    const size_t pb = (size_t)n * 3 * sizeof(double);
    double *d_in, *d_nrm;
    int *d_tri, *d_counts;
    VS_CHECK(carve_buf(ctx->h_aux0, [&](Carver& h) {
        d_in = h.take<double>((size_t)std::max(n, 1) * 3);
        d_nrm = h.take<double>((size_t)std::max(n, 1) * 3);
        d_tri = h.take<int>((size_t)std::max(cap, 1) * 3);
        d_counts = h.take<int>(2);
    }));
    if (n > 0) VS_HIP(hipMemcpyAsync(d_in, pts, pb, hipMemcpyHostToDevice, s));
    if (n > 0 && normals) {
        VS_HIP(hipMemcpyAsync(d_nrm, normals, pb, hipMemcpyHostToDevice, s));
    } else if (n > 0) {  // the chain of main.cpp:1379-1415: estimate_normals with k = 20, then the mesh
        VS_CHECK(cloud_normals(ctx, d_in, n, kNormalK, d_nrm, nullptr, s, c.use_grid != 0));
    }
    VS_CHECK(mesh_enqueue(ctx, d_in, d_nrm, n, c, cap, d_tri, d_counts, s));
    VS_HIP(hipMemcpyAsync(counts, d_counts, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    std::vector<double> own;  // the normals on the host when tri_normals needs them and the caller keeps none
    const double* h_nrm = normals;
    if (n > 0 && !normals && (normals_out || tri_normals)) {
        if (!normals_out) own.resize((size_t)n * 3);
        double* dst = normals_out ? normals_out : own.data();
        VS_HIP(hipMemcpyAsync(dst, d_nrm, pb, hipMemcpyDeviceToHost, s));
        h_nrm = dst;
    } else if (n > 0 && normals && normals_out && normals_out != normals) {
        std::copy(normals, normals + (size_t)n * 3, normals_out);
    }
    VS_HIP(hipStreamSynchronize(s));
    const int m = std::min(cap, counts[0]);
    if (m > 0) {
        VS_HIP(hipMemcpyAsync(tri, d_tri, (size_t)m * 3 * sizeof(int), hipMemcpyDeviceToHost, s));
        VS_HIP(hipStreamSynchronize(s));
    }
    // the reference's tri_verts / tri_normals are gathers of the index list
    for (size_t e = 0; e < (size_t)m * 3; e++)
        for (int ax = 0; ax < 3; ax++) {
            if (tri_verts) tri_verts[3 * e + ax] = pts[3 * (size_t)tri[e] + ax];
            if (tri_normals) tri_normals[3 * e + ax] = h_nrm[3 * (size_t)tri[e] + ax];
        }
    return VS_OK;
}

}  // extern "C"

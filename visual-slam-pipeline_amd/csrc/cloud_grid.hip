// cloud_grid.hip — the exact k-nearest-neighbour search of cloud.hip on a uniform cell grid: the same (d2, index)
// lists as k_cloud_knn, bit for bit, in time that grows with n and not with n^2, for clouds of up to
// VS_CLOUD_GRID_MAX_POINTS points.  All arithmetic is fp64 without contraction; d2 = (dx dx + dy dy) + dz dz;
// neighbours are ordered by (d2, index), the point itself excluded.  The result goes to the partial-list arrays of
// cloud.hip ([S = 1][k][n_max]), so k_cloud_reduce, k_cloud_normals and the filter's chain consume it unchanged.
//
// The grid is densify.hip's: a counting sort of the points by the hash of their packed cell coordinates (21 bits
// per axis) into a power-of-two bucket table, every sorted entry carrying index, cell key and coordinates.  The
// order inside a bucket depends on the atomics' scheduling and reaches no result: a query's candidates pass
// through a selection by the total order (d2, index), and each point is offered to it exactly once.
//
// Kernels (enqueue-only; the point count may exist only on the device, launches are sized for the host's bound):
//   k_cg_init     clears the bucket histogram and cursors (every level), the state words and the bounding box
//   k_cg_box      the cloud's bounding box (block reduction, then 64-bit atomics on order-preserving keys)
//   k_cg_sample   edge 0 only: 64 sample points, one workgroup each, histogram the d2 to every point by binary
//                 exponent; the first bin at which the count reaches k + 1 bounds the sample's k-th distance
//   k_cg_edge     one wave: the edge (the caller's, or the square root of the samples' median bound), clamped so
//                 that |p / edge| <= 2^19 for every point, and per level the edge and the cells' bounding box
//   k_cg_cells    cell key and bucket count per point
//   k_cg_scan     one workgroup: exclusive scan of the bucket counts (tables of up to kScanTiled buckets)
//   k_cg_tiles    larger tables: tile sums, k_cg_scan over the sums, then the scan inside every tile
//   k_cg_fill     scatters index, key and coordinates into the sorted arrays
//   k_cg_search   one wave (one 64-lane workgroup) per query, queries in sorted-cell order.  Lanes 0..26 look up
//                 the buckets of the 27 cells of rings 0 and 1, a wave scan concatenates their ranges and the 64
//                 lanes stride over the concatenation; later rings take their shell's cells 64 at a time in the
//                 same way.  A candidate below the current k-th entry by (d2, index) (uniform, in registers) is
//                 appended to an LDS list of 128 by ballot; when the list holds more than 64 it is bitonic-sorted
//                 and cut to k.  After ring R every unvisited point is at least (R + min(f, 1 - f)) edge away
//                 along some axis (f: the query's fractional position in its cell; the minimum over the axes);
//                 the query is finished when its k-th d2 is strictly below that bound (shrunk by 2^-20 relative
//                 and 2^-30 cells for the rounding of floor(p / edge)) squared, or when the rings cover the
//                 cells' bounding box.  A query not finished after max_rings rings is appended to a device list.
//   the levels    the listed queries are searched again on a grid with 5 times the edge, their leftovers on one
//                 with 25 times the edge (cells, scan, fill, search over the list): an isolated outlier costs a
//                 few coarse cells there and not a pass over the cloud
//   k_cg_rest     what is still listed: one wave per query, lanes striding over all sorted points, the same
//                 selection; writes the stats pair
// LDS per k_cg_search / k_cg_rest workgroup: 128 x (8 + 4) list + 65 + 64 ints + 64 keys = 2.5 KB.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "cloud_common.h"

namespace vs {

namespace {

constexpr int kList = 128;          // the selection's LDS list (a sort is due above kList - 64 entries)
constexpr int kSamples = 64;        // sample queries of the derived edge
constexpr int kBins = 128;          // d2 exponent bins: bin b > 0 holds 2^(b - 64) <= d2 < 2^(b - 63)
constexpr int kLevels = 3;          // grids: edge, 5 edge, 25 edge
constexpr double kLevelScale = 5.0;
constexpr int kDefaultRings = 4;
constexpr int kMaxRings = 1 << 16;  // |cell| <= 2^19 + 1, so a ring's cells stay inside 21 bits
constexpr int kScanTile = 4096;     // buckets per workgroup of the tiled scan
constexpr int kScanTiled = 1 << 13; // tables above this many buckets take the tiled scan
constexpr int kRestBlocks = 1024;

// state words: unfinished queries per level, then per level the cells' bounding box (biased, min xyz, max xyz)
enum { kGsLeft = 0, kGsCbox = kLevels, kGsWords = kLevels + 6 * kLevels };

struct Cg {
    const double* pts;
    const int* d_n;
    int n_max, k, skip_small;
    int T, t_shift, max_rings, level;
    double edge_req;
    double* par;               // [kLevels] the level's edge
    unsigned long long* box;   // [6] order-preserving keys of min xyz, max xyz
    double* est;               // [kSamples]
    int* state;                // [kGsWords]
    int* hist;                 // [T + 1] bucket counts, then starts
    int* cursor;               // [T]
    int* bsum;                 // [T / kScanTile + 1]
    unsigned long long* pkey;  // [n_max]
    unsigned long long* skey;  // sorted by bucket: cell key, input index, coordinates
    int* sidx;
    double* spts;
    int* left[2];              // [n_max] unfinished queries, level l writes left[l & 1]
    double* part_d2;           // [k][n_max]
    int* part_idx;
    int* stats;                // [2], nullable
};

__device__ __forceinline__ bool cg_live(const Cg& a, int n) { return n > 0 && !(a.skip_small && n <= a.k); }
// the queries of this level: all points (level 0) or the previous level's unfinished ones
__device__ __forceinline__ int cg_queries(const Cg& a, int n) { return a.level == 0 ? n : a.state[kGsLeft + a.level - 1]; }

// doubles as unsigned keys in the same order
__device__ __forceinline__ unsigned long long ord_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ord_val(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__global__ __launch_bounds__(256) void k_cg_init(Cg a) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i <= (size_t)a.T; i += stride) {
        a.hist[i] = 0;
        if (i < (size_t)a.T) a.cursor[i] = 0;
        if (a.level == 0 && i < kGsWords) a.state[i] = 0;
        if (a.level == 0 && i < 6) a.box[i] = i < 3 ? ~0ull : 0ull;
    }
}

__global__ __launch_bounds__(256) void k_cg_box(Cg a) {
    __shared__ double s_lo[3][4], s_hi[3][4];
    const int n = dev_count(a.d_n, a.n_max), tid = threadIdx.x;
    if (!cg_live(a, n)) return;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < (size_t)n; i += (size_t)gridDim.x * 256)
        for (int ax = 0; ax < 3; ax++) {
            const double p = a.pts[3 * i + ax];
            lo[ax] = fmin(lo[ax], p), hi[ax] = fmax(hi[ax], p);
        }
    for (int ax = 0; ax < 3; ax++) {
        for (int o = 32; o > 0; o >>= 1) {
            lo[ax] = fmin(lo[ax], __shfl_xor(lo[ax], o));
            hi[ax] = fmax(hi[ax], __shfl_xor(hi[ax], o));
        }
        if ((tid & 63) == 0) s_lo[ax][tid >> 6] = lo[ax], s_hi[ax][tid >> 6] = hi[ax];
    }
    __syncthreads();
    if (tid < 3) {
        const double l = fmin(fmin(s_lo[tid][0], s_lo[tid][1]), fmin(s_lo[tid][2], s_lo[tid][3]));
        const double h = fmax(fmax(s_hi[tid][0], s_hi[tid][1]), fmax(s_hi[tid][2], s_hi[tid][3]));
        atomicMin(&a.box[tid], ord_key(l));
        atomicMax(&a.box[3 + tid], ord_key(h));
    }
}

// grid kSamples: sample b is point floor(b n / kSamples)
__global__ __launch_bounds__(1024) void k_cg_sample(Cg a) {
    __shared__ int s_h[kBins];
    const int n = dev_count(a.d_n, a.n_max), tid = threadIdx.x, lane = tid & 63;
    if (!cg_live(a, n)) return;
    if (tid < kBins) s_h[tid] = 0;
    __syncthreads();
    const size_t q = (size_t)((long long)blockIdx.x * n / kSamples);
    const double qx = a.pts[3 * q], qy = a.pts[3 * q + 1], qz = a.pts[3 * q + 2];
    for (int i0 = 0; i0 < n; i0 += 1024) {
        const int i = i0 + tid;
        int bin = -1;
        if (i < n) {
            const double dx = qx - a.pts[3 * (size_t)i], dy = qy - a.pts[3 * (size_t)i + 1],
                         dz = qz - a.pts[3 * (size_t)i + 2];
            const double d2 = dx * dx + dy * dy + dz * dz;
            bin = d2 > 0 ? min(max(ilogb(d2), -63), 63) + 64 : 0;
        }
        // one LDS atomic per distinct bin of the wave (far points share a few bins)
        unsigned long long todo = __ballot(bin >= 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int b = __shfl(bin, leader);
            const unsigned long long same = __ballot(bin == b);
            if (lane == leader) atomicAdd(&s_h[b], __popcll(same));
            todo &= ~same;
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int want = min(a.k + 1, n);  // the sample itself is counted (bin 0)
        int cum = 0, b = 0;
        for (; b < kBins - 1; b++) {
            cum += s_h[b];
            if (cum >= want) break;
        }
        a.est[blockIdx.x] = ldexp(1.0, b - 63);  // the k-th neighbour's d2 is below this
    }
}

// The cell of coordinate p on a grid of the given edge (biased); k_cg_edge keeps |p / edge| <= 2^19.
__device__ __forceinline__ long long cg_cell(double p, double edge) { return (long long)floor(p / edge) + kAxisBias; }

__global__ __launch_bounds__(64) void k_cg_edge(Cg a) {
    __shared__ double s_e[kSamples];
    const int n = dev_count(a.d_n, a.n_max), lane = threadIdx.x;
    if (!cg_live(a, n)) return;
    double edge = a.edge_req;
    if (!(edge > 0)) {  // the upper median of the samples' bounds: every lane ends with the same value
        const double mine = a.est[lane];
        s_e[lane] = mine;
        __syncthreads();
        int rank = 0;
        for (int t = 0; t < kSamples; t++) rank += s_e[t] < mine || (s_e[t] == mine && t < lane);
        const unsigned long long has = __ballot(rank == kSamples / 2);
        edge = sqrt(__shfl(mine, __ffsll((long long)has) - 1));
    }
    double m = 0, lo[3], hi[3];
    for (int ax = 0; ax < 3; ax++) {
        lo[ax] = ord_val(a.box[ax]), hi[ax] = ord_val(a.box[3 + ax]);
        m = fmax(m, fmax(fabs(lo[ax]), fabs(hi[ax])));
    }
    edge = fmax(edge, m / 524288.0);  // |p / edge| <= 2^19 (1 + 2^-52): 21 bits per axis hold any cloud
    if (!(edge > 0) || !isfinite(edge)) edge = 1.0;
    if (lane < kLevels) {
        double e = edge;
        for (int l = 0; l < lane; l++) e *= kLevelScale;
        if (!isfinite(e)) e = edge;
        a.par[lane] = e;
        for (int ax = 0; ax < 3; ax++) {  // floor(p / e) is monotonic in p: no point's cell lies outside
            a.state[kGsCbox + 6 * lane + ax] = (int)cg_cell(lo[ax], e);
            a.state[kGsCbox + 6 * lane + 3 + ax] = (int)cg_cell(hi[ax], e);
        }
    }
}

__global__ __launch_bounds__(256) void k_cg_cells(Cg a) {
    const int n = dev_count(a.d_n, a.n_max), i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !cg_live(a, n) || cg_queries(a, n) == 0) return;
    const double edge = a.par[a.level];
    const unsigned long long key = pack3(cg_cell(a.pts[3 * (size_t)i], edge), cg_cell(a.pts[3 * (size_t)i + 1], edge),
                                         cg_cell(a.pts[3 * (size_t)i + 2], edge));
    a.pkey[i] = key;
    atomicAdd(&a.hist[hash_bits(key, a.t_shift)], 1);
}

// data[0 .. count) -> its exclusive prefix sums, data[count] = the total (densify.hip's k_dz_scan)
__global__ __launch_bounds__(1024) void k_cg_scan(int* data, int count) {
    __shared__ int s_sum[1024];
    const int tid = threadIdx.x, per = (count + 1023) / 1024;
    const int lo = min(count, tid * per), hi = min(count, lo + per);
    int sum = 0;
    for (int i = lo; i < hi; i++) sum += data[i];
    s_sum[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = tid >= o ? s_sum[tid - o] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    int run = s_sum[tid] - sum;
    for (int i = lo; i < hi; i++) {
        const int v = data[i];
        data[i] = run;
        run += v;
    }
    if (tid == 1023) data[count] = s_sum[1023];
}

// The tiled scan: workgroup b owns data[kScanTile b, kScanTile (b + 1)) (count is a multiple of kScanTile), four
// consecutive entries per lane.  apply 0: bsum[b] = the tile's sum.  apply 1 (bsum scanned): the exclusive prefix
// sums inside the tile, offset by bsum[b]; data[count] = the total.
__global__ __launch_bounds__(1024) void k_cg_tiles(int* data, int count, int* bsum, int apply) {
    __shared__ int s_w[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t at = (size_t)blockIdx.x * kScanTile + 4 * (size_t)tid;
    const int4 v = *reinterpret_cast<const int4*>(data + at);
    const int sum = v.x + v.y + v.z + v.w;
    int inc = sum;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < 16; w++) {
        if (w < wv) before += s_w[w];
        total += s_w[w];
    }
    if (!apply) {
        if (tid == 0) bsum[blockIdx.x] = total;
        return;
    }
    const int run = bsum[blockIdx.x] + before + inc - sum;
    *reinterpret_cast<int4*>(data + at) = make_int4(run, run + v.x, run + v.x + v.y, run + v.x + v.y + v.z);
    if (blockIdx.x == 0 && tid == 0) data[count] = bsum[gridDim.x];
}

__global__ __launch_bounds__(256) void k_cg_fill(Cg a) {
    const int n = dev_count(a.d_n, a.n_max), i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || !cg_live(a, n) || cg_queries(a, n) == 0) return;
    const unsigned long long key = a.pkey[i];
    const unsigned b = hash_bits(key, a.t_shift);
    const int pos = a.hist[b] + atomicAdd(&a.cursor[b], 1);  // < hist[b + 1] <= n
    a.sidx[pos] = i;
    a.skey[pos] = key;
    a.spts[3 * (size_t)pos] = a.pts[3 * (size_t)i];
    a.spts[3 * (size_t)pos + 1] = a.pts[3 * (size_t)i + 1];
    a.spts[3 * (size_t)pos + 2] = a.pts[3 * (size_t)i + 2];
}

// One wave's selection of the k smallest candidates by (d2, index): an LDS list of cnt <= kList entries, of which
// the first min(cnt, k) are final once sorted; (kd, ki) is the k-th entry of the last sort, (+inf, kNoIdx) before
// the list first held k.  Every member is uniform over the wave; every call is made by the whole wave.
struct Sel {
    double* d2;
    int* idx;
    int k, cnt;
    bool dirty;
    double kd;
    int ki;
};

// Bitonic sort over 64 or 128 slots (the tail padded with empty entries), then the cut to k.
__device__ __forceinline__ void cg_sort(Sel& s, int lane) {
    const int P = s.cnt > 64 ? 128 : 64;
    for (int t = s.cnt + lane; t < P; t += 64) s.d2[t] = INFINITY, s.idx[t] = kNoIdx;
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < P / 2; t += 64) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
                const double dl = s.d2[lo], dh = s.d2[hi];
                const int il = s.idx[lo], ih = s.idx[hi];
                const bool gt = dl > dh || (dl == dh && il > ih), lt = dh > dl || (dl == dh && ih > il);
                if ((lo & k2) == 0 ? gt : lt) {
                    s.d2[lo] = dh;
                    s.d2[hi] = dl;
                    s.idx[lo] = ih;
                    s.idx[hi] = il;
                }
            }
            __syncthreads();
        }
    s.cnt = min(s.cnt, s.k);
    if (s.cnt == s.k) s.kd = s.d2[s.k - 1], s.ki = s.idx[s.k - 1];
    s.dirty = false;
    __syncthreads();  // the k-th entry has been read before the next append
}

// One candidate per lane (has): appended when it is below the k-th entry.  s.cnt <= 64 on entry.
__device__ __forceinline__ void cg_offer(Sel& s, bool has, double d2, int j, int lane) {
    const bool hit = has && (d2 < s.kd || (d2 == s.kd && j < s.ki));
    const unsigned long long bal = __ballot(hit);
    if (bal == 0) return;
    if (hit) {
        const int pos = s.cnt + __popcll(bal & ((1ull << lane) - 1ull));  // < 64 + 64
        s.d2[pos] = d2;
        s.idx[pos] = j;
    }
    s.cnt += __popcll(bal);
    s.dirty = true;
    if (s.cnt > kList - 64) cg_sort(s, lane);
}

struct Query {
    int q;
    double x, y, z;
};

// Up to 64 cells, one per lane (use: the lane has one, ck its key): their buckets' ranges are concatenated by a
// wave scan and the lanes stride over the members; a member of another cell in the same bucket fails the key
// compare.  s_pre [65], s_beg [64], s_ck [64].
__device__ __forceinline__ void cg_visit(const Cg& a, const Query& Q, Sel& s, bool use, unsigned long long ck, int lane,
                                         int* s_pre, int* s_beg, unsigned long long* s_ck) {
    int beg = 0, c = 0;
    if (use) {
        const unsigned b = hash_bits(ck, a.t_shift);
        beg = a.hist[b];
        c = a.hist[b + 1] - beg;
    }
    int inc = c;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    s_pre[lane + 1] = inc;
    if (lane == 0) s_pre[0] = 0;
    s_beg[lane] = beg;
    s_ck[lane] = ck;
    __syncthreads();
    const int total = s_pre[64];
    for (int t0 = 0; t0 < total; t0 += 64) {
        const int t = t0 + lane;
        bool has = false;
        double d2 = 0;
        int j = 0;
        if (t < total) {
            int lo = 0, hi = 64;  // s_pre[lo] <= t < s_pre[hi]: ends at the one cell that holds member t
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_pre[mid] <= t)
                    lo = mid;
                else
                    hi = mid;
            }
            const int m = s_beg[lo] + t - s_pre[lo];  // < hist[b + 1] <= n
            if (a.skey[m] == s_ck[lo]) {
                j = a.sidx[m];
                const double dx = Q.x - a.spts[3 * (size_t)m], dy = Q.y - a.spts[3 * (size_t)m + 1],
                             dz = Q.z - a.spts[3 * (size_t)m + 2];
                d2 = dx * dx + dy * dy + dz * dz;
                has = j != Q.q;
            }
        }
        cg_offer(s, has, d2, j, lane);
    }
    __syncthreads();  // the ranges are free for the next cells
}

// the finished list (sorted, empty slots (+inf, kNoIdx)) to [k][n_max]
__device__ __forceinline__ void cg_write(const Cg& a, const Sel& s, int q, int lane) {
    if (lane < a.k) {
        a.part_d2[(size_t)lane * a.n_max + q] = s.d2[lane];
        a.part_idx[(size_t)lane * a.n_max + q] = s.idx[lane];
    }
}

// grid n_max workgroups of one wave; every __syncthreads is this wave's own.
__global__ __launch_bounds__(64) void k_cg_search(Cg a) {
    __shared__ double s_d2[kList];
    __shared__ int s_idx[kList];
    __shared__ int s_pre[65], s_beg[64];
    __shared__ unsigned long long s_ck[64];
    const int n = dev_count(a.d_n, a.n_max), lane = threadIdx.x;
    if (!cg_live(a, n) || (int)blockIdx.x >= cg_queries(a, n)) return;
    Query Q;
    if (a.level == 0) {  // sorted-cell order: neighbouring waves read the same buckets
        Q.q = a.sidx[blockIdx.x];
        Q.x = a.spts[3 * (size_t)blockIdx.x], Q.y = a.spts[3 * (size_t)blockIdx.x + 1];
        Q.z = a.spts[3 * (size_t)blockIdx.x + 2];
    } else {
        Q.q = a.left[(a.level - 1) & 1][blockIdx.x];
        Q.x = a.pts[3 * (size_t)Q.q], Q.y = a.pts[3 * (size_t)Q.q + 1], Q.z = a.pts[3 * (size_t)Q.q + 2];
    }
    const double edge = a.par[a.level];
    const double p[3] = {Q.x, Q.y, Q.z};
    long long c[3];
    int lo[3], hi[3];
    double mf = 1.0;
    for (int ax = 0; ax < 3; ax++) {
        const double f = p[ax] / edge, fr = f - floor(f);  // the division of cg_cell
        c[ax] = (long long)floor(f) + kAxisBias;
        mf = fmin(mf, fmin(fr, 1.0 - fr));
        lo[ax] = a.state[kGsCbox + 6 * a.level + ax], hi[ax] = a.state[kGsCbox + 6 * a.level + 3 + ax];
    }
    Sel s{s_d2, s_idx, a.k, 0, true, INFINITY, kNoIdx};
    auto visit = [&](bool use, int dx, int dy, int dz) {
        const long long x = c[0] + dx, y = c[1] + dy, z = c[2] + dz;
        use = use && x >= lo[0] && x <= hi[0] && y >= lo[1] && y <= hi[1] && z >= lo[2] && z <= hi[2];
        if (!__any(use)) return;  // no point lives outside the cells' box
        cg_visit(a, Q, s, use, use ? pack3(x, y, z) : 0ull, lane, s_pre, s_beg, s_ck);
    };
    visit(lane < 27, lane % 3 - 1, (lane / 3) % 3 - 1, lane / 9 - 1);  // rings 0 and 1
    bool done;
    for (int R = 1;; R++) {
        if (s.dirty) cg_sort(s, lane);
        bool all = true;
        for (int ax = 0; ax < 3; ax++) all = all && c[ax] - R <= lo[ax] && c[ax] + R >= hi[ax];
        // positions in cell units are known to 2^-33 (|p / edge| < 2^20), d2 to a few 2^-53 relative
        const double b = (((double)R + mf) * (1.0 - 1.0 / 1048576.0) - 1.0 / 1073741824.0) * edge;
        done = all || (s.cnt == s.k && b > 0 && s.kd < b * b);
        if (done || R >= a.max_rings) break;
        // shell R + 1: the faces z = -+r (w x w cells), y = -+r (w x v), x = -+r (v x v)
        const int r = R + 1, w = 2 * r + 1, v = 2 * r - 1, A = w * w, B = w * v, C = v * v, shell = 2 * (A + B + C);
        for (int t0 = 0; t0 < shell; t0 += 64) {
            int t = t0 + lane, dx, dy, dz;
            const bool use = t < shell;
            if (t < 2 * A) {
                dz = t >= A ? r : -r, t -= t >= A ? A : 0;
                dx = t % w - r, dy = t / w - r;
            } else if (t < 2 * (A + B)) {
                t -= 2 * A;
                dy = t >= B ? r : -r, t -= t >= B ? B : 0;
                dx = t % w - r, dz = t / w - (r - 1);
            } else {
                t -= 2 * (A + B);
                dx = t >= C ? r : -r, t -= t >= C ? C : 0;
                dy = t % v - (r - 1), dz = t / v - (r - 1);
            }
            visit(use, dx, dy, dz);
        }
    }
    if (done) {
        cg_write(a, s, Q.q, lane);
    } else if (lane == 0) {
        a.left[a.level & 1][atomicAdd(&a.state[kGsLeft + a.level], 1)] = Q.q;  // fewer than n_max queries
    }
}

// What the levels left: a pass over all sorted points per query.  Also the stats pair.
__global__ __launch_bounds__(64) void k_cg_rest(Cg a) {
    __shared__ double s_d2[kList];
    __shared__ int s_idx[kList];
    const int n = dev_count(a.d_n, a.n_max), lane = threadIdx.x;
    const bool live = cg_live(a, n);
    const int m = live ? a.state[kGsLeft + kLevels - 1] : 0;
    if (blockIdx.x == 0 && lane == 0 && a.stats) a.stats[0] = live ? n - m : 0, a.stats[1] = m;
    for (int e = blockIdx.x; e < m; e += gridDim.x) {
        Query Q;
        Q.q = a.left[(kLevels - 1) & 1][e];
        Q.x = a.pts[3 * (size_t)Q.q], Q.y = a.pts[3 * (size_t)Q.q + 1], Q.z = a.pts[3 * (size_t)Q.q + 2];
        Sel s{s_d2, s_idx, a.k, 0, true, INFINITY, kNoIdx};
        for (int t0 = 0; t0 < n; t0 += 64) {
            const int t = t0 + lane;
            bool has = false;
            double d2 = 0;
            int j = 0;
            if (t < n) {
                j = a.sidx[t];
                const double dx = Q.x - a.spts[3 * (size_t)t], dy = Q.y - a.spts[3 * (size_t)t + 1],
                             dz = Q.z - a.spts[3 * (size_t)t + 2];
                d2 = dx * dx + dy * dy + dz * dz;
                has = j != Q.q;
            }
            cg_offer(s, has, d2, j, lane);
        }
        if (s.dirty) cg_sort(s, lane);
        cg_write(a, s, Q.q, lane);
        __syncthreads();  // the list is free for the next query
    }
}

int log2_ceil(size_t v) {
    int b = 0;
    while (((size_t)1 << b) < v) b++;
    return b;
}

}  // namespace

int launch_knn_grid(vs_ctx* ctx, const CloudScratch& cs, const double* d_pts, const int* d_n, int n_max, int k,
                    int skip_small, double cell_edge, int max_rings, int* d_stats, hipStream_t s) {
    Cg a{};
    a.pts = d_pts, a.d_n = d_n, a.n_max = n_max, a.k = k, a.skip_small = skip_small;
    const int t_bits = std::min(23, std::max(12, log2_ceil((size_t)n_max)));  // about one point per bucket
    a.T = 1 << t_bits, a.t_shift = 64 - t_bits;
    a.max_rings = std::min(max_rings > 0 ? max_rings : kDefaultRings, kMaxRings);
    a.edge_req = cell_edge;
    a.part_d2 = cs.part_d2, a.part_idx = cs.part_idx, a.stats = d_stats;
    const int tiles = a.T / kScanTile;
    VS_CHECK(carve_buf(ctx->cloud_grid, [&](Carver& p) {
        a.par = p.take<double>(kLevels);
        a.box = p.take<unsigned long long>(6);
        a.est = p.take<double>(kSamples);
        a.state = p.take<int>(kGsWords);
        a.hist = p.take<int>((size_t)a.T + 1);
        a.cursor = p.take<int>(a.T);
        a.bsum = p.take<int>(tiles + 1);
        a.pkey = p.take<unsigned long long>(n_max);
        a.skey = p.take<unsigned long long>(n_max);
        a.sidx = p.take<int>(n_max);
        a.spts = p.take<double>((size_t)n_max * 3);
        a.left[0] = p.take<int>(n_max);
        a.left[1] = p.take<int>(n_max);
    }));
    const int pblocks = (n_max + 255) / 256;
    // one profile stage per kernel (events only while the context's profile is on)
#define CG_LAUNCH(kernel, grid, block, ...)                                      \
    do {                                                                         \
        ProfScope ps_(ctx, #kernel, s);                                          \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, __VA_ARGS__);  \
    } while (0)
    for (a.level = 0; a.level < kLevels; a.level++) {
        CG_LAUNCH(k_cg_init, std::min(a.T / 256 + 1, 2048), 256, a);
        if (a.level == 0) {
            CG_LAUNCH(k_cg_box, std::min(pblocks, 1024), 256, a);
            if (!(cell_edge > 0)) CG_LAUNCH(k_cg_sample, kSamples, 1024, a);
            CG_LAUNCH(k_cg_edge, 1, 64, a);
        }
        CG_LAUNCH(k_cg_cells, pblocks, 256, a);
        if (a.T <= kScanTiled) {
            CG_LAUNCH(k_cg_scan, 1, 1024, a.hist, a.T);
        } else {
            CG_LAUNCH(k_cg_tiles, tiles, 1024, a.hist, a.T, a.bsum, 0);
            CG_LAUNCH(k_cg_scan, 1, 1024, a.bsum, tiles);
            CG_LAUNCH(k_cg_tiles, tiles, 1024, a.hist, a.T, a.bsum, 1);
        }
        CG_LAUNCH(k_cg_fill, pblocks, 256, a);
        CG_LAUNCH(k_cg_search, n_max, 64, a);
    }
    CG_LAUNCH(k_cg_rest, std::min(n_max, kRestBlocks), 64, a);
#undef CG_LAUNCH
    VS_HIP(hipGetLastError());
    return VS_OK;
}

}  // namespace vs

using namespace vs;

extern "C" {

int vs_cloud_knn_grid_dev(vs_ctx* ctx, const double* d_pts, int n, int k, double cell_edge, int max_rings, int* d_nbr,
                          double* d_d2, int* d_stats, void* stream) {
    VS_ARG(ctx && d_pts && d_nbr && d_d2, "vs_cloud_knn_grid_dev: null argument");
    VS_ARG(n >= 0 && k >= 1 && cell_edge >= 0 && std::isfinite(cell_edge) && max_rings >= 0,
           "vs_cloud_knn_grid_dev: bad size, edge or ring count");
    VS_CHECK(cloud_size_check("vs_cloud_knn_grid_dev", n, k, VS_CLOUD_GRID_MAX_POINTS));
    if (n == 0) return VS_OK;
    VS_HIP(hipSetDevice(ctx->device));
    const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    CloudScratch cs;
    VS_CHECK(cloud_scratch(ctx, n, k, 1, &cs));
    VS_CHECK(launch_knn_grid(ctx, cs, d_pts, nullptr, n, k, 0, cell_edge, max_rings, d_stats, s));
    ProfScope ps(ctx, "k_cloud_reduce", s);
    return cloud_knn_lists(cs, d_pts, n, k, d_nbr, d_d2, s);
}

int vs_cloud_normals_grid_dev(vs_ctx* ctx, const double* d_pts, int n, int k, double* d_normals, double* d_eig,
                              void* stream) {
    VS_ARG(ctx && d_normals && n >= 0 && (n == 0 || d_pts) && k >= 1,
           "vs_cloud_normals_grid_dev: null argument or bad size");
    VS_CHECK(cloud_size_check("vs_cloud_normals_grid_dev", n, k, VS_CLOUD_GRID_MAX_POINTS));
    VS_HIP(hipSetDevice(ctx->device));
    return cloud_normals(ctx, d_pts, n, k, d_normals, d_eig, stream ? (hipStream_t)stream : ctx->stream, true);
}

int vs_cloud_normals_grid(vs_ctx* ctx, const double* pts, int n, int k, double* normals, double* eig) {
    return cloud_normals_host(ctx, pts, n, k, normals, eig, true);
}

int vs_cloud_filter_grid_dev(vs_ctx* ctx, const double* d_pts, int n, const vs_cloud_filter_config* cfg, double* d_out,
                             int* d_idx, int* d_counts, void* stream) {
    VS_ARG(ctx && d_out && d_idx && d_counts && n >= 0 && (n == 0 || d_pts), "vs_cloud_filter_grid_dev: null argument");
    VS_HIP(hipSetDevice(ctx->device));
    return cloud_filter(ctx, d_pts, n, nullptr, config_or(cfg, vs_cloud_filter_default_config), d_out, d_idx, d_counts,
                        stream ? (hipStream_t)stream : ctx->stream, true);
}

int vs_cloud_filter_grid(vs_ctx* ctx, const double* pts, int n, const vs_cloud_filter_config* cfg, double* out,
                         int* idx, int counts[3]) {
    return cloud_filter_host(ctx, pts, n, cfg, out, idx, counts, true);
}

}  // extern "C"

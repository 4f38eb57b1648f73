// cloud_poisson.hip — a closed surface from oriented points: Poisson reconstruction on a dense R^3 grid of fp64 nodes
// (the stage the reference reaches by writing estimated_map.ply and running PoissonRecon, main.cpp:1379-1458).  The
// semantics are stated in include/vslam_abi.h; all arithmetic is fp64 in the written order, compiled without
// contraction, sums of three products as (a + b) + c.
//
//   orientation   k_po_orient: one point per lane, the views streamed past it; the nearest view by (d2, index) decides
//                 the normal's sign.
//   grid          k_ps_box (per-workgroup min / max) and k_ps_grid (one workgroup: the box, then o and h) leave the
//                 grid in the state block on the device: no host round trip.
//   splat         the points are sorted by base cell, ascending point index inside a cell: k_ps_count (the cells' counts,
//                 scanned to their starts) and a stable radix sort of (cell, index), 9 bits a pass (k_rs_hist, the
//                 tiled scan, k_rs_scatter; linear in n whatever the cells hold).  Then k_ps_gather: one node per lane
//                 adds the points of its <= 8 adjacent cells, cells in the order dx, dy, dz (dx fastest), points
//                 ascending inside a cell.  No floating-point atomic: V is the same from run to run.
//   divergence    k_ps_div: one node per lane, six reads of V (neighbouring lanes share them in the caches).
//   solve         conjugate gradients, two kernels per iteration, no host synchronisation inside:
//     k_cg_apply    q = A p with p·q.  A workgroup owns a 32 x 8 column of nodes and marches kZChunk planes along z:
//                   the plane of p sits in LDS with a one-node halo ((8 + 2) x (32 + 2) fp64, 2.7 KB), the lane's own
//                   column (z - 1, z, z + 1) in registers, so a p value comes from HBM once (the halo ring and the two
//                   end planes of a chunk are re-read, from L2 when the neighbouring workgroup is resident).
//                   p = r + beta p_old is folded in here: every value that is loaded, halo included, is formed from r
//                   and p_old by the same expression, and the owner stores it to the other p buffer (two buffers, so
//                   no workgroup reads what another has already replaced).
//     k_cg_update   x += alpha p, r -= alpha q with r·r: 4,096 consecutive nodes per workgroup.
//                 Each dot product is summed in a fixed order: the lane's terms in index order, block_sum's tree over
//                 the workgroup, and the workgroups' partials by the workgroup that arrives last at a ticket (lane t
//                 takes partials t, t + 256, ...; then the same tree).  Which workgroup is last varies; what it adds
//                 does not.  That workgroup's first lane computes alpha (k_cg_apply) or beta, the iteration count and
//                 the stop flag (k_cg_update) in the state block.  Once the flag is set every later launch returns at
//                 its first instruction, so vs_cloud_poisson_dev enqueues max_iter iterations without looking; the
//                 host call, which may wait, reads the flag every kPoll iterations and stops enqueueing.
//   iso value     k_ps_iso: one point per lane, the same fixed-order sum.
//   extraction    marching tetrahedra on the Kuhn subdivision.  k_iso_mask: per node the 7-bit mask of its edges that
//                 carry a vertex, its popcount and the cube's triangle count; the tiled scan turns both counts into
//                 offsets; k_iso_verts and k_iso_tris emit.  A vertex id is offset[node] + popcount(mask below kind):
//                 no array of 7 R^3 keys, no atomic in a position.
// Memory: five arrays of R^3 fp64 (V's three, div, one more) become x, the two p buffers, r and q; the cells' starts
// and the extraction's mask and offsets live inside arrays that are dead at the time: 40 R^3 bytes (+ 24 n for the
// point sort): 0.67 GB at R = 256, 5.4 GB at R = 512.  No MFMA: an fp64 7-point stencil has no matrix product in it.
// Steps 2b, 4s and 7 (point_weight, trim, the density outputs) are template variants here — k_ps_gather<true> (W and
// the occupied cells), k_iso_mask / k_iso_verts / k_iso_tris<true> — and poisson_screen.hip's loop; W is a sixth array,
// screening a seventh and the cells' starts apart (poisson_plan).  With both settings 0 none of them is launched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "poisson_common.h"

namespace vs {

namespace {

constexpr int kBoxBlocks = 256;
constexpr int kRsBits = 9, kRsBins = 1 << kRsBits;  // the point sort's digit
constexpr int kPoll = 64;                        // the host call reads the stop flag every kPoll iterations
constexpr int kScPoll = 8;                       // ... and every kScPoll of the screened loop's preconditioned ones
constexpr int kScIters = 192;                    // max_iter = 0 for the preconditioned screened loop: twice the 92 measured
constexpr int kNormalK = 20;                     // main.cpp:1379
static_assert((size_t)VS_POISSON_MAX_RES * VS_POISSON_MAX_RES * VS_POISSON_MAX_RES <= (size_t)kMaxTiles * kTile,
              "k_scan_top's tile sums");
static_assert(12ll * VS_POISSON_MAX_RES * VS_POISSON_MAX_RES * VS_POISSON_MAX_RES < (1ll << 31), "32-bit offsets");
static_assert(VS_CLOUD_GRID_MAX_POINTS / 256 <= kMaxTiles, "k_ps_iso's partials");

struct Ps {
    const double *pts, *nrm;
    int n, R;
    double scale, tol;
    int max_iter;
    PsState* st;
    double* arr[7];  // R^3 (padded to whole tiles) fp64 each; [5] = W and [6] only where the call needs them
    double* part;    // [kMaxTiles] partial sums
    double* lohi;    // [kBoxBlocks][6]
    int *hist, *sidx, *bsum;
    int *key[2], *idx[2], *rs_hist;  // the radix sort's two (key, index) buffers and its [digit][workgroup] counts
    double *fs, *sp;                 // the screened solve's sorted fractions [3][n] and (B p) [n]
};

// ---- orientation ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_po_orient(const double* pts, double* nrm, int n, const double* views, int m) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double px = pts[3 * (size_t)i], py = pts[3 * (size_t)i + 1], pz = pts[3 * (size_t)i + 2];
    double best = INFINITY, cx = 0, cy = 0, cz = 0;
    for (int v = 0; v < m; v++) {
        const double dx = views[3 * v] - px, dy = views[3 * v + 1] - py, dz = views[3 * v + 2] - pz;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < best) best = d2, cx = dx, cy = dy, cz = dz;
    }
    double* q = nrm + 3 * (size_t)i;
    if ((q[0] * cx + q[1] * cy) + q[2] * cz < 0) q[0] = -q[0], q[1] = -q[1], q[2] = -q[2];
}

// ---- the tiled exclusive scan of an int array (count a multiple of kTile), in place; *total = the sum ----------
__device__ __forceinline__ int block_prefix1024(int v, int* s_w, int& total) {
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

// apply 0: bsum[tile] = the tile's sum.  apply 1 (bsum scanned): the prefix sums inside the tile, offset by bsum[tile]
__global__ __launch_bounds__(1024) void k_scan_tiles(int* data, int* bsum, int apply) {
    __shared__ int s_w[16];
    const size_t at = (size_t)blockIdx.x * kTile + 4 * (size_t)threadIdx.x;
    const int4 v = *reinterpret_cast<const int4*>(data + at);
    const int sum = v.x + v.y + v.z + v.w;
    int total;
    const int before = block_prefix1024(sum, s_w, total);
    if (!apply) {
        if (threadIdx.x == 0) bsum[blockIdx.x] = total;
        return;
    }
    const int run = bsum[blockIdx.x] + before;
    *reinterpret_cast<int4*>(data + at) = make_int4(run, run + v.x, run + v.x + v.y, run + v.x + v.y + v.z);
}

// one workgroup: bsum[0 .. tiles) -> its exclusive prefix sums; *total (nullable) = the sum
__global__ __launch_bounds__(1024) void k_scan_top(int* bsum, int tiles, int* total) {
    __shared__ int s_w[16];
    const int per = (tiles + 1023) / 1024;
    const int lo = min(tiles, (int)threadIdx.x * per), hi = min(tiles, lo + per);
    int sum = 0;
    for (int t = lo; t < hi; t++) sum += bsum[t];
    int all;
    int run = block_prefix1024(sum, s_w, all);
    for (int t = lo; t < hi; t++) {
        const int v = bsum[t];
        bsum[t] = run;
        run += v;
    }
    if (total && threadIdx.x == 0) *total = all;
}

// ---- the grid ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ps_box(Ps a) {
    __shared__ double s_lo[3][4], s_hi[3][4];
    const int tid = threadIdx.x;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < (size_t)a.n; i += (size_t)kBoxBlocks * 256)
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
        a.lohi[6 * blockIdx.x + tid] = fmin(fmin(s_lo[tid][0], s_lo[tid][1]), fmin(s_lo[tid][2], s_lo[tid][3]));
        a.lohi[6 * blockIdx.x + 3 + tid] = fmax(fmax(s_hi[tid][0], s_hi[tid][1]), fmax(s_hi[tid][2], s_hi[tid][3]));
    }
}

// one wave: the box of the workgroups' boxes, then the grid.  A cloud without extent leaves a unit grid and ok = 0.
__global__ __launch_bounds__(64) void k_ps_grid(Ps a) {
    const int lane = threadIdx.x;
    double lo[3], hi[3];
    for (int ax = 0; ax < 3; ax++) {
        double l = INFINITY, h = -INFINITY;
        for (int b = lane; b < kBoxBlocks; b += 64) l = fmin(l, a.lohi[6 * b + ax]), h = fmax(h, a.lohi[6 * b + 3 + ax]);
        for (int o = 32; o > 0; o >>= 1) l = fmin(l, __shfl_xor(l, o)), h = fmax(h, __shfl_xor(h, o));
        lo[ax] = l, hi[ax] = h;
    }
    if (lane != 0) return;
    PsState& st = *a.st;
    const double ext = fmax(fmax(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
    const double side = a.scale * ext;
    st.ok = side > 0 && isfinite(side);
    st.h = st.ok ? side / (double)(a.R - 1) : 1.0;
    for (int ax = 0; ax < 3; ax++) st.o[ax] = st.ok ? (lo[ax] + hi[ax]) / 2.0 - side / 2.0 : lo[ax];
    st.rho = st.alpha = st.beta = st.rhs_norm = st.iso = 0;
    st.done = st.converged = st.iters = 0;
    st.ticket = 0;
    st.cells = st.go = 0;
    st.lambda = st.rz = 0;
}

// point i's base node b and fractions f: g = (p - o) / h, b = floor(g) kept inside [0, R - 2]
__device__ __forceinline__ void ps_base(const Ps& a, size_t i, int b[3], double f[3]) {
    for (int ax = 0; ax < 3; ax++) {
        const double g = (a.pts[3 * i + ax] - a.st->o[ax]) / a.st->h;
        b[ax] = min(max((int)floor(g), 0), a.R - 2);
        f[ax] = g - (double)b[ax];
    }
}

// ---- the splat: a stable sort of the points by base cell, then one gather per node --------------------------------
__global__ __launch_bounds__(256) void k_ps_clear(int* hist, size_t count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) hist[i] = 0;
}

// key[i] = point i's base cell, hist[cell] = its points.  A cloud without extent counts nothing: no node gathers.
__global__ __launch_bounds__(256) void k_ps_count(Ps a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    int b[3] = {0, 0, 0};
    double f[3];
    if (a.st->ok) ps_base(a, i, b, f);
    const size_t c = lin(b[0], b[1], b[2], a.R);
    a.key[0][i] = (int)c;
    if (a.st->ok) atomicAdd(&a.hist[c], 1);
}

// One pass of a least-significant-digit radix sort of (key, point index) on kRsBits bits of the key: k_rs_hist counts
// each workgroup's items per digit into hist [digit][workgroup], the tiled scan turns that into positions, k_rs_scatter
// moves the items.  Every pass is stable and the input is in index order, so equal keys end in ascending point index:
// the work is linear in n whatever the cells' occupancy, and no atomic decides a position.
struct Rs {
    const int *key_in, *idx_in;  // idx_in null: the identity (the first pass)
    int *key_out, *idx_out, *hist;
    int n, shift, nblocks;
};

// The lane's item: its digit and the number of items of its workgroup with the same digit in front of it; s_cnt
// [wave][digit] = the wave's items per digit.  Lanes past n hold nothing.
__device__ __forceinline__ int rs_rank(const Rs& a, int (*s_cnt)[kRsBins], int& key, int& digit, bool& live) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    live = i < a.n;
    key = live ? a.key_in[i] : 0;
    digit = (key >> a.shift) & (kRsBins - 1);
    for (int t = threadIdx.x; t < 4 * kRsBins; t += 256) (&s_cnt[0][0])[t] = 0;
    __syncthreads();
    unsigned long long peers = __ballot(live);  // the wave's live lanes with this lane's digit
    for (int b = 0; b < kRsBits; b++) {
        const bool bit = (digit >> b) & 1;
        const unsigned long long m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    if (live && rank == 0) s_cnt[wv][digit] = __popcll(peers);
    __syncthreads();
    int before = rank;
    for (int w = 0; w < wv; w++) before += s_cnt[w][digit];
    return before;
}

__global__ __launch_bounds__(256) void k_rs_hist(Rs a) {
    __shared__ int s_cnt[4][kRsBins];
    int key, digit;
    bool live;
    rs_rank(a, s_cnt, key, digit, live);
    for (int d = threadIdx.x; d < kRsBins; d += 256)
        a.hist[(size_t)d * a.nblocks + blockIdx.x] = (s_cnt[0][d] + s_cnt[1][d]) + (s_cnt[2][d] + s_cnt[3][d]);
}

__global__ __launch_bounds__(256) void k_rs_scatter(Rs a) {
    __shared__ int s_cnt[4][kRsBins];
    int key, digit;
    bool live;
    const int before = rs_rank(a, s_cnt, key, digit, live);
    if (!live) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int at = a.hist[(size_t)digit * a.nblocks + blockIdx.x] + before;  // < n: the scanned counts of n items
    a.key_out[at] = key;
    a.idx_out[at] = a.idx_in ? a.idx_in[i] : i;
}

// DENSITY: step 2b's W as a fourth accumulator (the same weights in the same order), and the number of base cells
// that hold a point — an integer count, so the atomic's order does not show.
template <bool DENSITY>
__global__ __launch_bounds__(256) void k_ps_gather(Ps a, size_t nodes) {
    const size_t nd = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (nd >= nodes) return;
    const int R = a.R, i = (int)(nd % R), j = (int)(nd / R % R), k = (int)(nd / ((size_t)R * R));
    double vx = 0, vy = 0, vz = 0, ws = 0;
    for (int d = 0; d < 8 && a.st->ok; d++) {
        const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
        const int ci = i - dx, cj = j - dy, ck = k - dz;
        if (ci < 0 || cj < 0 || ck < 0 || ci > R - 2 || cj > R - 2 || ck > R - 2) continue;
        const size_t c = lin(ci, cj, ck, R);
        const int first = a.hist[c], cnt = a.hist[c + 1] - first;  // c + 1 < R^3: the last node is no cell
        for (int t = 0; t < cnt; t++) {
            const size_t p = (size_t)a.sidx[first + t];
            int b[3];
            double f[3];
            ps_base(a, p, b, f);
            const double w = ((dx ? f[0] : 1.0 - f[0]) * (dy ? f[1] : 1.0 - f[1])) * (dz ? f[2] : 1.0 - f[2]);
            vx += w * a.nrm[3 * p], vy += w * a.nrm[3 * p + 1], vz += w * a.nrm[3 * p + 2];
            if (DENSITY) ws += w;
        }
    }
    a.arr[0][nd] = vx, a.arr[1][nd] = vy, a.arr[2][nd] = vz;
    if (DENSITY) {
        a.arr[5][nd] = ws;
        const bool cell = a.st->ok && i <= R - 2 && j <= R - 2 && k <= R - 2 && a.hist[nd + 1] > a.hist[nd];
        const unsigned long long m = __ballot(cell);
        if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&a.st->cells, __popcll(m));
    }
}

// the sorted point t's fractions, fs[axis][t]: the values k_ps_gather's weights are made of
__global__ __launch_bounds__(256) void k_sc_frac(Ps a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n) return;
    int b[3];
    double f[3];
    ps_base(a, (size_t)a.sidx[t], b, f);
    for (int ax = 0; ax < 3; ax++) a.fs[(size_t)ax * a.n + t] = f[ax];
}

__global__ __launch_bounds__(256) void k_ps_div(Ps a, size_t nodes) {
    const size_t nd = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (nd >= nodes) return;
    const int R = a.R, i = (int)(nd % R), j = (int)(nd / R % R), k = (int)(nd / ((size_t)R * R));
    const size_t sy = R, sz = (size_t)R * R;
    const double *vx = a.arr[0], *vy = a.arr[1], *vz = a.arr[2];
    const double gx = (i + 1 < R ? vx[nd + 1] : 0.0) - (i > 0 ? vx[nd - 1] : 0.0);
    const double gy = (j + 1 < R ? vy[nd + sy] : 0.0) - (j > 0 ? vy[nd - sy] : 0.0);
    const double gz = (k + 1 < R ? vz[nd + sz] : 0.0) - (k > 0 ? vz[nd - sz] : 0.0);
    a.arr[3][nd] = ((gx + gy) + gz) / (2.0 * a.st->h);
}

// ---- conjugate gradients -----------------------------------------------------------------------------------------
struct Cg {
    PsState* st;
    double *__restrict__ x, *__restrict__ r, *__restrict__ q, *__restrict__ p_in, *__restrict__ p_out, *part;
    int R, max_iter;
    size_t nodes;
    double tol;
};

// r = -div in place, x = 0, rho = r·r
__global__ __launch_bounds__(256) void k_cg_start(Cg a) {
    double acc = 0;
#pragma unroll
    for (int e = 0; e < kTile / 256; e++) {  // predicated, not cut short: the loads of all 16 terms go out together
        const size_t i = (size_t)blockIdx.x * kTile + e * 256 + threadIdx.x;
        if (i < a.nodes) {
            const double r = -a.r[i];
            a.r[i] = r, a.x[i] = 0.0;
            acc += r * r;
        }
    }
    double total;
    if (grid_sum(acc, a.part, &a.st->ticket, total) && threadIdx.x == 0) {
        a.st->rho = total;
        a.st->rhs_norm = sqrt(total);
        if (total == 0 || a.max_iter == 0) a.st->done = 1;
        if (total == 0) a.st->converged = 1;
    }
}

// the search direction at a node: r on the first iteration, r + beta p_old later; 0 outside the grid
__device__ __forceinline__ double cg_p(const Cg& a, bool first, double beta, int x, int y, int z) {
    if (x < 0 || y < 0 || z < 0 || x >= a.R || y >= a.R || z >= a.R) return 0.0;
    const size_t i = lin(x, y, z, a.R);
    return first ? a.r[i] : a.r[i] + beta * a.p_in[i];
}

__global__ __launch_bounds__(256) void k_cg_apply(Cg a) {
    __shared__ double s_p[kTY + 2][kTX + 2];
    PsState& st = *a.st;
    if (st.done) return;
    const int tid = threadIdx.x, tx = tid & (kTX - 1), ty = tid / kTX;
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY, z0 = blockIdx.z * kZChunk;
    const int x = x0 + tx, y = y0 + ty, z1 = min(z0 + kZChunk, a.R);
    const bool first = st.iters == 0, own = x < a.R && y < a.R;
    const double beta = st.beta, h2 = st.h * st.h;
    // this lane's node of the halo ring: the rows above and below the tile, then the columns left and right of it
    int hx = 0, hy = 0;
    if (tid < kTX) hx = tid + 1, hy = 0;
    else if (tid < 2 * kTX) hx = tid - kTX + 1, hy = kTY + 1;
    else if (tid < 2 * kTX + kTY) hx = 0, hy = tid - 2 * kTX + 1;
    else if (tid < kHalo) hx = kTX + 1, hy = tid - 2 * kTX - kTY + 1;
    double below = own ? cg_p(a, first, beta, x, y, z0 - 1) : 0.0, cur = own ? cg_p(a, first, beta, x, y, z0) : 0.0;
    double acc = 0;
    for (int z = z0; z < z1; z++) {
        const double above = own ? cg_p(a, first, beta, x, y, z + 1) : 0.0;
        s_p[ty + 1][tx + 1] = cur;
        if (tid < kHalo) s_p[hy][hx] = cg_p(a, first, beta, x0 + hx - 1, y0 + hy - 1, z);
        __syncthreads();
        if (own) {
            const double sum = ((((s_p[ty + 1][tx] + s_p[ty + 1][tx + 2]) + s_p[ty][tx + 1]) + s_p[ty + 2][tx + 1]) + below) + above;
            const double q = (6.0 * cur - sum) / h2;
            const size_t i = lin(x, y, z, a.R);
            a.q[i] = q, a.p_out[i] = cur;
            acc += cur * q;
        }
        __syncthreads();
        below = cur, cur = above;
    }
    double total;
    if (grid_sum(acc, a.part, &st.ticket, total) && tid == 0) st.alpha = st.rho / total;
}

__global__ __launch_bounds__(256) void k_cg_update(Cg a) {
    PsState& st = *a.st;
    if (st.done) return;
    const double alpha = st.alpha;
    double acc = 0;
#pragma unroll
    for (int e = 0; e < kTile / 256; e++) {
        const size_t i = (size_t)blockIdx.x * kTile + e * 256 + threadIdx.x;
        if (i < a.nodes) {
            a.x[i] = a.x[i] + alpha * a.p_out[i];
            const double r = a.r[i] - alpha * a.q[i];
            a.r[i] = r;
            acc += r * r;
        }
    }
    double total;
    if (grid_sum(acc, a.part, &st.ticket, total) && threadIdx.x == 0) {
        st.iters++;
        st.beta = total / st.rho;
        st.rho = total;
        if (sqrt(total) <= a.tol * st.rhs_norm) st.converged = 1, st.done = 1;
        if (st.iters >= a.max_iter) st.done = 1;
    }
}

// ---- the iso value: the mean over the points of chi interpolated at the point ------------------------------------
__global__ __launch_bounds__(256) void k_ps_iso(Ps a, const double* chi) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    double v = 0;
    if (i < a.n) {
        int b[3];
        double f[3];
        ps_base(a, i, b, f);
        for (int d = 0; d < 8; d++) {
            const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
            const double w = ((dx ? f[0] : 1.0 - f[0]) * (dy ? f[1] : 1.0 - f[1])) * (dz ? f[2] : 1.0 - f[2]);
            v += w * chi[lin(b[0] + dx, b[1] + dy, b[2] + dz, a.R)];
        }
    }
    double total;
    if (grid_sum(v, a.part, &a.st->ticket, total) && threadIdx.x == 0) a.st->iso = total / (double)a.n;
}

// ---- marching tetrahedra ---------------------------------------------------------------------------------------
// geo = {origin x, y, z, h, iso} on the device.  A cube corner is c = dx + 2 dy + 4 dz; an edge runs from corner ca to
// cb with ca's bits inside cb's, its kind is kKind[cb - ca], its owner the node at ca.
struct Iso {
    const double* field;
    const double* geo;
    int R, vcap, tcap;
    size_t nodes;
    uint8_t* mask;  // [R^3] bit kind: the edge carries a vertex
    int *voff, *toff;
    double* verts;
    int* tri;
    // step 7 and the density output: W (null without either), the threshold, rho per written vertex (nullable)
    const double* W;
    double trim;
    double* vdens;
};
__device__ const int kKind[8] = {-1, 0, 1, 3, 2, 4, 5, 6};
__device__ const int kCorner[7] = {1, 2, 4, 3, 5, 6, 7};

// bit c: corner c of the cube at (i, j, k) is in the grid and below
__device__ __forceinline__ void iso_corners(const Iso& a, int i, int j, int k, unsigned& below, unsigned& valid) {
    const double iso = a.geo[4];
    below = valid = 0;
    for (int c = 0; c < 8; c++) {
        const int x = i + (c & 1), y = j + ((c >> 1) & 1), z = k + (c >> 2);
        if (x >= a.R || y >= a.R || z >= a.R) continue;
        valid |= 1u << c;
        if (a.field[lin(x, y, z, a.R)] < iso) below |= 1u << c;
    }
}
// tetrahedron t's corners: 0, e_p1, e_p1 + e_p2, 7 for the permutations xyz, xzy, yxz, yzx, zxy, zyx
__device__ __forceinline__ void tet_corners(int t, int vc[4]) {
    const int p1 = t >> 1, p2 = (t & 1) ? (p1 == 2 ? 1 : 2) : (p1 == 0 ? 1 : 0);
    vc[0] = 0, vc[1] = 1 << p1, vc[2] = vc[1] | (1 << p2), vc[3] = 7;
}

// The triangles of the cube whose corners below are the bits of below, in step 6's order: emit(ea, eb, Dx, Dy, Dz) with
// the triangle's three edges ea[e] -> eb[e] (cube corners, ea's bits inside eb's) and the direction from below to above.
template <class F>
__device__ __forceinline__ void cube_triangles(unsigned below, F&& emit) {
    for (int t = 0; t < 6; t++) {
        int vc[4];
        tet_corners(t, vc);
        int lo[4], hi[4], nb = 0, na = 0;  // tetrahedron vertices below and above, ascending
        int Sb[3] = {0, 0, 0}, Sa[3] = {0, 0, 0};
        for (int v = 0; v < 4; v++) {
            const bool b = (below >> vc[v]) & 1u;
            (b ? lo[nb++] : hi[na++]) = v;
            for (int ax = 0; ax < 3; ax++) (b ? Sb : Sa)[ax] += (vc[v] >> ax) & 1;
        }
        if (nb == 0 || na == 0) continue;
        // na nb (mean of the above corners - mean of the below corners)
        const int Dx = nb * Sa[0] - na * Sb[0], Dy = nb * Sa[1] - na * Sb[1], Dz = nb * Sa[2] - na * Sb[2];
        auto edge = [&](int u, int w, int& ca, int& cb) { ca = vc[min(u, w)], cb = vc[max(u, w)]; };
        int ea[3], eb[3];
        if (nb == 2) {
            int qa[4], qb[4];  // ac, ad, bd, bc
            edge(lo[0], hi[0], qa[0], qb[0]), edge(lo[0], hi[1], qa[1], qb[1]);
            edge(lo[1], hi[1], qa[2], qb[2]), edge(lo[1], hi[0], qa[3], qb[3]);
            for (int e = 0; e < 3; e++) ea[e] = qa[e], eb[e] = qb[e];
            emit(ea, eb, Dx, Dy, Dz);
            ea[1] = qa[2], eb[1] = qb[2], ea[2] = qa[3], eb[2] = qb[3];
            emit(ea, eb, Dx, Dy, Dz);
        } else {
            const int s = nb == 1 ? lo[0] : hi[0];
            for (int v = 0, e = 0; v < 4; v++)
                if (v != s) edge(s, v, ea[e], eb[e]), e++;
            emit(ea, eb, Dx, Dy, Dz);
        }
    }
}

// Step 7 inside a cube with all eight corners: bit 8 ca + cb = the vertex on the edge ca -> cb exists and survives,
// rho = W[a] + t (W[b] - W[a]) >= trim with step 6's t.  The expression is the one the edge's owner evaluates in
// k_iso_verts, on the same operands: every cube that shares an edge decides alike.  Corners outside the grid read 0 and
// their edges stay dead.  The loops are unrolled, so the corner values stay in registers.
__device__ __forceinline__ unsigned long long iso_alive(const Iso& a, size_t nd, unsigned below, unsigned valid) {
    const double iso = a.geo[4];
    const size_t R = a.R;
    double f[8], w[8];
#pragma unroll
    for (int c = 0; c < 8; c++) {
        const size_t at = nd + (c & 1) + ((c >> 1) & 1) * R + (c >> 2) * R * R;
        const bool in = (valid >> c) & 1u;
        f[c] = in ? a.field[at] : 0.0, w[c] = in ? a.W[at] : 0.0;
    }
    unsigned long long alive = 0;
#pragma unroll
    for (int ca = 0; ca < 7; ca++)
#pragma unroll
        for (int cb = ca + 1; cb < 8; cb++) {
            if ((ca & cb) != ca || !((valid >> cb) & 1u)) continue;  // cb in the grid: ca is too
            if (((below >> ca) & 1u) == ((below >> cb) & 1u)) continue;
            const double t = (iso - f[ca]) / (f[cb] - f[ca]);
            if (w[ca] + t * (w[cb] - w[ca]) >= a.trim) alive |= 1ull << (8 * ca + cb);
        }
    return alive;
}

// TRIM (step 7): the mask keeps the surviving vertices only, and a cube counts the triangles whose three vertices
// survive, so the scans hand out compacted ids and offsets and nothing is compacted afterwards.
template <bool TRIM>
__global__ __launch_bounds__(256) void k_iso_mask(Iso a, size_t padded) {
    const size_t nd = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (nd >= padded) return;
    if (nd >= a.nodes) {  // the scan's padding
        a.voff[nd] = 0, a.toff[nd] = 0;
        return;
    }
    const int R = a.R, i = (int)(nd % R), j = (int)(nd / R % R), k = (int)(nd / ((size_t)R * R));
    unsigned below, valid;
    iso_corners(a, i, j, k, below, valid);
    unsigned long long alive = 0;
    if (TRIM && below != 0 && below != valid) alive = iso_alive(a, nd, below, valid);
    unsigned mask = 0;
    for (int c = 1; c < 8; c++)
        if (((valid >> c) & 1u) && ((below >> c) & 1u) != (below & 1u) && (!TRIM || ((alive >> c) & 1ull)))
            mask |= 1u << kKind[c];
    int tris = 0;
    if (valid == 0xffu) {
        if (TRIM) {
            cube_triangles(below, [&](const int ea[3], const int eb[3], int, int, int) {
                tris += (int)((alive >> (8 * ea[0] + eb[0])) & (alive >> (8 * ea[1] + eb[1])) & (alive >> (8 * ea[2] + eb[2])) & 1ull);
            });
        } else {
            for (int t = 0; t < 6; t++) {
                int vc[4];
                tet_corners(t, vc);
                const int nb = ((below >> vc[0]) & 1) + ((below >> vc[1]) & 1) + ((below >> vc[2]) & 1) + ((below >> vc[3]) & 1);
                tris += nb == 2 ? 2 : (nb == 1 || nb == 3) ? 1 : 0;
            }
        }
    }
    a.mask[nd] = (uint8_t)mask;
    a.voff[nd] = __popc(mask), a.toff[nd] = tris;
}

// DENSITY: rho of each written vertex goes to vdens
template <bool DENSITY>
__global__ __launch_bounds__(256) void k_iso_verts(Iso a) {
    const size_t nd = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (nd >= a.nodes) return;
    const unsigned mask = a.mask[nd];
    if (!mask) return;
    const int R = a.R, ijk[3] = {(int)(nd % R), (int)(nd / R % R), (int)(nd / ((size_t)R * R))};
    const double h = a.geo[3], iso = a.geo[4], fa = a.field[nd];
    int at = a.voff[nd];
    for (int kind = 0; kind < 7; kind++) {
        if (!((mask >> kind) & 1u)) continue;
        if (at >= a.vcap) return;
        const int c = kCorner[kind], d[3] = {c & 1, (c >> 1) & 1, c >> 2};
        const size_t nb = lin(ijk[0] + d[0], ijk[1] + d[1], ijk[2] + d[2], R);
        const double fb = a.field[nb];
        const double t = (iso - fa) / (fb - fa);
        if (DENSITY) a.vdens[at] = a.W[nd] + t * (a.W[nb] - a.W[nd]);
        for (int ax = 0; ax < 3; ax++) {
            const double pa = a.geo[ax] + h * (double)ijk[ax], pb = a.geo[ax] + h * (double)(ijk[ax] + d[ax]);
            a.verts[3 * (size_t)at + ax] = pa + t * (pb - pa);
        }
        at++;
    }
}

// TRIM: a triangle is written when the masks of its three edges' owners still hold the vertices (k_iso_mask counted
// it by the same rule)
template <bool TRIM>
__global__ __launch_bounds__(256) void k_iso_tris(Iso a) {
    const size_t nd = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (nd >= a.nodes) return;
    const int R = a.R, i = (int)(nd % R), j = (int)(nd / R % R), k = (int)(nd / ((size_t)R * R));
    if (i > R - 2 || j > R - 2 || k > R - 2) return;
    unsigned below, valid;
    iso_corners(a, i, j, k, below, valid);
    if (below == 0 || below == 0xffu) return;
    int at = a.toff[nd];
    // the vertex on the edge between corners ca and cb (ca's bits inside cb's)
    auto vid = [&](int ca, int cb) {
        const size_t owner = nd + (ca & 1) + (size_t)((ca >> 1) & 1) * R + (size_t)(ca >> 2) * R * R;
        return a.voff[owner] + __popc(a.mask[owner] & ((1u << kKind[cb - ca]) - 1u));
    };
    auto alive = [&](int ca, int cb) {
        const size_t owner = nd + (ca & 1) + (size_t)((ca >> 1) & 1) * R + (size_t)(ca >> 2) * R * R;
        return (a.mask[owner] >> kKind[cb - ca]) & 1u;
    };
    // a triangle over the edges (ea[e], eb[e]): wound from below to above on the doubled edge midpoints, smallest id first
    cube_triangles(below, [&](const int ea[3], const int eb[3], int Dx, int Dy, int Dz) {
        if (TRIM && !(alive(ea[0], eb[0]) && alive(ea[1], eb[1]) && alive(ea[2], eb[2]))) return;  // not counted either
        const int slot = at++;
        if (slot >= a.tcap) return;
        int m[3][3], id[3];
        for (int e = 0; e < 3; e++) {
            id[e] = vid(ea[e], eb[e]);
            for (int ax = 0; ax < 3; ax++) m[e][ax] = ((ea[e] >> ax) & 1) + ((eb[e] >> ax) & 1);
        }
        const int ux = m[1][0] - m[0][0], uy = m[1][1] - m[0][1], uz = m[1][2] - m[0][2];
        const int wx = m[2][0] - m[0][0], wy = m[2][1] - m[0][1], wz = m[2][2] - m[0][2];
        const int dot = (uy * wz - uz * wy) * Dx + (uz * wx - ux * wz) * Dy + (ux * wy - uy * wx) * Dz;
        if (!(dot > 0)) {
            const int s = id[1];
            id[1] = id[2], id[2] = s;
        }
        const int f = id[0] < id[1] ? (id[0] < id[2] ? 0 : 2) : (id[1] < id[2] ? 1 : 2);
        int* out = a.tri + 3 * (size_t)slot;
        out[0] = id[f], out[1] = id[(f + 1) % 3], out[2] = id[(f + 2) % 3];
    });
}

__global__ void k_iso_geo(double* geo, double ox, double oy, double oz, double h, double iso) {
    if (threadIdx.x == 0) geo[0] = ox, geo[1] = oy, geo[2] = oz, geo[3] = h, geo[4] = iso;
}

// the solver's report; the extraction reads its grid and iso from here too
__global__ void k_ps_info(PsState* st, double* geo, double* info, int* counts, int final_pass) {
    if (threadIdx.x != 0) return;
    if (!final_pass) {
        geo[0] = st->o[0], geo[1] = st->o[1], geo[2] = st->o[2], geo[3] = st->h, geo[4] = st->iso;
        return;
    }
    info[0] = (double)st->iters;
    info[1] = st->rhs_norm > 0 ? sqrt(st->rho) / st->rhs_norm : 0.0;
    info[2] = st->iso;
    info[3] = st->ok ? (double)st->converged : -1.0;
    if (!st->ok) counts[0] = counts[1] = 0;
}

#define PS_LAUNCH_AS(name, kernel, grid, block, ...)                                 \
    do {                                                                             \
        ProfScope ps_(ctx, name, s);                                                 \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, __VA_ARGS__);      \
    } while (0)
#define PS_LAUNCH(kernel, grid, block, ...) PS_LAUNCH_AS(#kernel, kernel, grid, block, __VA_ARGS__)

size_t pad_tile(size_t v) { return (v + kTile - 1) / kTile * kTile; }
// the point sort's workgroups, a multiple of 8 so that kRsBins counts each are whole scan tiles (the spare ones are empty)
int rs_blocks(int n) { return ((n + 255) / 256 + 7) / 8 * 8; }
static_assert(kRsBins * 8 == kTile, "rs_blocks pads the counts to whole tiles");
static_assert((size_t)kRsBins * ((VS_CLOUD_GRID_MAX_POINTS / 256 + 7) / 8 * 8) <= (size_t)kMaxTiles * kTile, "the sort's counts fit the scan");
unsigned blocks256(size_t v) { return (unsigned)((v + 255) / 256); }

// data[0 .. padded) -> exclusive prefix sums in place, *total = the sum
int scan_enqueue(vs_ctx* ctx, int* data, size_t padded, int* bsum, int* total, hipStream_t s) {
    const int tiles = (int)(padded / kTile);
    PS_LAUNCH(k_scan_tiles, tiles, 1024, data, bsum, 0);
    PS_LAUNCH(k_scan_top, 1, 1024, bsum, tiles, total);
    PS_LAUNCH(k_scan_tiles, tiles, 1024, data, bsum, 1);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// the extraction's launches; mask [R^3] bytes, voff / toff [padded] ints, bsum [kMaxTiles], geo set on the device
int iso_enqueue(vs_ctx* ctx, Iso a, int* bsum, int* d_counts, hipStream_t s) {
    const size_t padded = pad_tile(a.nodes);
    const bool trim = a.trim > 0;  // the variants are taken only then: the plain call runs the code it always ran
    if (trim) PS_LAUNCH_AS("k_iso_mask", k_iso_mask<true>, blocks256(padded), 256, a, padded);
    else PS_LAUNCH_AS("k_iso_mask", k_iso_mask<false>, blocks256(padded), 256, a, padded);
    VS_CHECK(scan_enqueue(ctx, a.voff, padded, bsum, d_counts, s));
    VS_CHECK(scan_enqueue(ctx, a.toff, padded, bsum, d_counts + 1, s));
    if (a.vdens) PS_LAUNCH_AS("k_iso_verts", k_iso_verts<true>, blocks256(a.nodes), 256, a);
    else PS_LAUNCH_AS("k_iso_verts", k_iso_verts<false>, blocks256(a.nodes), 256, a);
    if (trim) PS_LAUNCH_AS("k_iso_tris", k_iso_tris<true>, blocks256(a.nodes), 256, a);
    else PS_LAUNCH_AS("k_iso_tris", k_iso_tris<false>, blocks256(a.nodes), 256, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int res_check(const char* who, int R, int min_r) {
    if (R < min_r) {
        set_error(std::string(who) + ": resolution below " + std::to_string(min_r));
        return VS_ERR_ARG;
    }
    if (R > VS_POISSON_MAX_RES) {
        set_error(std::string(who) + ": resolution above VS_POISSON_MAX_RES");
        return VS_ERR_CAPACITY;
    }
    return VS_OK;
}

// sc_iter: the screened loop's iterations; a max_iter of 0 is 8 R there too without a preconditioner, kScIters with it
int poisson_check(const char* who, vs_cloud_poisson_config& c, int n, int* sc_iter) {
    VS_CHECK(res_check(who, c.resolution, VS_POISSON_MIN_RES));
    if (!(c.point_weight >= 0) || !std::isfinite(c.point_weight) || !(c.trim >= 0) || !std::isfinite(c.trim)) {
        set_error(std::string(who) + ": point_weight or trim negative or not finite");
        return VS_ERR_ARG;
    }
    if (n < 1 || !(c.scale > 1) || !std::isfinite(c.scale) || !(c.tol >= 0) || !std::isfinite(c.tol) || c.max_iter < 0) {
        set_error(std::string(who) + ": no points, scale not above 1, or a negative tol or max_iter");
        return VS_ERR_ARG;
    }
    if (c.solver != VS_POISSON_SOLVER_CG && c.solver != VS_POISSON_SOLVER_DIRECT) {
        set_error(std::string(who) + ": solver is neither VS_POISSON_SOLVER_CG nor VS_POISSON_SOLVER_DIRECT");
        return VS_ERR_ARG;
    }
    *sc_iter = c.max_iter ? c.max_iter : c.solver == VS_POISSON_SOLVER_DIRECT ? kScIters : 8 * c.resolution;
    if (c.max_iter == 0) c.max_iter = 8 * c.resolution;
    return cloud_size_check(who, n, 1, VS_CLOUD_GRID_MAX_POINTS);
}

// The pipeline in three parts, so that the host call can copy div out and watch the stop flag between them.
struct Plan {
    Ps a;
    Cg cg;
    Iso iso;
    Sc sc;
    double* geo;
    size_t nodes, padded;
    int passes;  // radix passes that cover a cell index
    bool density, screened;  // W is computed (arr[5]); step 4s runs (arr[6], the cells' starts apart, fs and sp)
};

// want_w: a density output is asked for.  Memory, fp64 arrays of R^3: five; six with W (trimming or a density output);
// seven and the cells' starts as R^3 ints of their own with screening, whose loop needs the starts to the end:
// 40, 48 and 60 R^3 bytes (+ 24 n for the point sort, + 32 n for the screened loop's sorted fractions and B p).
int poisson_plan(vs_ctx* ctx, const double* d_pts, const double* d_nrm, int n, const vs_cloud_poisson_config& c,
                 int sc_iter, bool want_w, Plan* pl) {
    Ps& a = pl->a;
    a = Ps{};
    pl->screened = c.point_weight > 0, pl->density = pl->screened || c.trim > 0 || want_w;
    const int arrays = pl->screened ? 7 : pl->density ? 6 : 5;
    a.pts = d_pts, a.nrm = d_nrm, a.n = n, a.R = c.resolution, a.scale = c.scale, a.tol = c.tol, a.max_iter = c.max_iter;
    const size_t nodes = (size_t)a.R * a.R * a.R, padded = pad_tile(nodes);
    pl->nodes = nodes, pl->padded = padded;
    pl->passes = 1;
    while (((nodes - 1) >> (pl->passes * kRsBits)) != 0) pl->passes++;  // nodes <= 2^27: at most 3
    VS_CHECK(carve_buf(ctx->cloud_poisson, [&](Carver& p) {
        for (int e = 0; e < arrays; e++) a.arr[e] = p.take<double>(padded);
        a.st = p.take<PsState>(1);
        pl->geo = p.take<double>(5);
        a.part = p.take<double>(kMaxTiles);
        a.lohi = p.take<double>(6 * kBoxBlocks);
        for (int e = 0; e < 2; e++) a.key[e] = p.take<int>(n), a.idx[e] = p.take<int>(n);
        a.rs_hist = p.take<int>((size_t)kRsBins * rs_blocks(n));
        a.bsum = p.take<int>(kMaxTiles);
        if (pl->screened) a.hist = p.take<int>(padded), a.fs = p.take<double>(3 * (size_t)n), a.sp = p.take<double>(n);
    }));
    if (!pl->screened) a.hist = reinterpret_cast<int*>(a.arr[4]);  // free until the first k_cg_apply writes q
    a.sidx = a.idx[pl->passes & 1];
    Cg& g = pl->cg;
    g = Cg{};
    g.st = a.st, g.x = a.arr[0], g.r = a.arr[3], g.q = a.arr[4], g.part = a.part;
    g.R = a.R, g.max_iter = a.max_iter, g.nodes = nodes, g.tol = a.tol;
    Iso& o = pl->iso;  // after the solve r and both p buffers are free
    o = Iso{};
    o.field = a.arr[0], o.geo = pl->geo, o.R = a.R, o.nodes = nodes;
    o.mask = reinterpret_cast<uint8_t*>(a.arr[3]);
    o.voff = reinterpret_cast<int*>(a.arr[1]), o.toff = reinterpret_cast<int*>(a.arr[2]);
    o.W = pl->density ? a.arr[5] : nullptr, o.trim = c.trim;
    // Step 4s.  x, r, q and the p buffers are step 4's; arr[6] is z under the preconditioner, and the copy of div that
    // conjugate gradients (which turn arr[3] into their residual) leave for b otherwise, where z is r.
    const bool direct = c.solver == VS_POISSON_SOLVER_DIRECT;
    Sc& sc = pl->sc;
    sc = Sc{};
    sc.st = a.st, sc.x = a.arr[0], sc.r = a.arr[3], sc.z = direct ? a.arr[6] : a.arr[3], sc.q = a.arr[4];
    sc.p[0] = a.arr[1], sc.p[1] = a.arr[2], sc.W = a.arr[5], sc.div = direct ? a.arr[3] : a.arr[6];
    sc.sp = a.sp, sc.part = a.part, sc.fs = a.fs, sc.skey = a.key[pl->passes & 1], sc.starts = a.hist;
    sc.n = n, sc.R = a.R, sc.max_iter = sc_iter, sc.direct = direct, sc.nodes = nodes;
    sc.tol = c.tol, sc.point_weight = c.point_weight;
    return VS_OK;
}

// points and normals -> div in arr[3]
int poisson_rhs(vs_ctx* ctx, Plan& pl, hipStream_t s) {
    const Ps& a = pl.a;
    PS_LAUNCH(k_ps_box, kBoxBlocks, 256, a);
    PS_LAUNCH(k_ps_grid, 1, 64, a);
    PS_LAUNCH(k_ps_clear, blocks256(pl.padded), 256, a.hist, pl.padded);
    PS_LAUNCH(k_ps_count, blocks256(a.n), 256, a);
    VS_CHECK(scan_enqueue(ctx, a.hist, pl.padded, a.bsum, nullptr, s));
    Rs rs{};
    rs.hist = a.rs_hist, rs.n = a.n, rs.nblocks = rs_blocks(a.n);
    for (int pass = 0; pass < pl.passes; pass++) {  // the last pass writes idx[passes & 1] = a.sidx
        rs.key_in = a.key[pass & 1], rs.idx_in = pass ? a.idx[pass & 1] : nullptr;
        rs.key_out = a.key[(pass + 1) & 1], rs.idx_out = a.idx[(pass + 1) & 1], rs.shift = pass * kRsBits;
        PS_LAUNCH(k_rs_hist, rs.nblocks, 256, rs);
        VS_CHECK(scan_enqueue(ctx, rs.hist, (size_t)kRsBins * rs.nblocks, a.bsum, nullptr, s));
        PS_LAUNCH(k_rs_scatter, rs.nblocks, 256, rs);
    }
    if (pl.density) PS_LAUNCH_AS("k_ps_gather", k_ps_gather<true>, blocks256(pl.nodes), 256, a, pl.nodes);
    else PS_LAUNCH_AS("k_ps_gather", k_ps_gather<false>, blocks256(pl.nodes), 256, a, pl.nodes);
    if (pl.screened) PS_LAUNCH(k_sc_frac, blocks256(a.n), 256, a);
    PS_LAUNCH(k_ps_div, blocks256(pl.nodes), 256, a, pl.nodes);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int cg_start(vs_ctx* ctx, Plan& pl, hipStream_t s) {
    PS_LAUNCH(k_cg_start, (unsigned)(pl.padded / kTile), 256, pl.cg);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// iterations [from, to)
int cg_iterate(vs_ctx* ctx, Plan& pl, int from, int to, hipStream_t s) {
    const int R = pl.a.R;
    const dim3 grid((R + kTX - 1) / kTX, (R + kTY - 1) / kTY, (R + kZChunk - 1) / kZChunk);
    for (int it = from; it < to; it++) {
        Cg g = pl.cg;
        g.p_in = pl.a.arr[1 + (it & 1)], g.p_out = pl.a.arr[1 + ((it + 1) & 1)];
        PS_LAUNCH(k_cg_apply, grid, 256, g);
        PS_LAUNCH(k_cg_update, (unsigned)(pl.padded / kTile), 256, g);
    }
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// VS_POISSON_SOLVER_DIRECT: div in arr[3] -> chi in arr[0] by poisson_dst.hip's sine transforms, through arr[1] and
// arr[2].  arr[0] still holds the splat's zeros when the cloud has no extent: the transforms then write nothing.
int direct_solve(vs_ctx* ctx, Plan& pl, hipStream_t s) {
    PsState* st = pl.a.st;
    const DstState ds{&st->ok, &st->h, &st->rho, &st->rhs_norm, &st->converged};
    return poisson_dst_enqueue(ctx, pl.a.arr[3], pl.a.arr[0], pl.a.arr[1], pl.a.arr[2], pl.a.R, 0.0, &ds, nullptr, s);
}

// step 4's chi in arr[0] -> tau (step 5 on chi0, left in st->iso), then the screened loop's start
int screened_start(vs_ctx* ctx, Plan& pl, hipStream_t s) {
    PS_LAUNCH(k_ps_iso, blocks256(pl.a.n), 256, pl.a, (const double*)pl.a.arr[0]);
    VS_HIP(hipGetLastError());
    return screen_start(ctx, pl.sc, s);
}

// chi in arr[0] -> iso, the mesh and the report
int poisson_finish(vs_ctx* ctx, Plan& pl, int vcap, int tcap, double* d_verts, int* d_tri, int* d_counts,
                   double* d_info, double* d_vdens, hipStream_t s) {
    PS_LAUNCH(k_ps_iso, blocks256(pl.a.n), 256, pl.a, (const double*)pl.a.arr[0]);
    PS_LAUNCH(k_ps_info, 1, 64, pl.a.st, pl.geo, d_info, d_counts, 0);
    Iso o = pl.iso;
    o.vcap = vcap, o.tcap = tcap, o.verts = d_verts, o.tri = d_tri, o.vdens = d_vdens;
    VS_CHECK(iso_enqueue(ctx, o, pl.a.bsum, d_counts, s));
    PS_LAUNCH(k_ps_info, 1, 64, pl.a.st, pl.geo, d_info, d_counts, 1);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int orient_check(const char* who, int n, int m) {
    VS_ARG(n >= 0 && m >= 1, std::string(who) + ": n < 0 or no view");
    if (m > VS_POISSON_MAX_VIEWS) {
        set_error(std::string(who) + ": more views than VS_POISSON_MAX_VIEWS");
        return VS_ERR_CAPACITY;
    }
    return VS_OK;
}

int orient_enqueue(vs_ctx* ctx, const double* d_pts, double* d_nrm, int n, const double* d_views, int m, hipStream_t s) {
    if (n == 0) return VS_OK;
    PS_LAUNCH(k_po_orient, blocks256(n), 256, d_pts, d_nrm, n, d_views, m);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int iso_check(const char* who, int R, const double* origin, double h, double iso) {
    VS_CHECK(res_check(who, R, 2));
    VS_ARG(origin && h > 0 && std::isfinite(h) && std::isfinite(iso) && std::isfinite(origin[0]) &&
               std::isfinite(origin[1]) && std::isfinite(origin[2]),
           std::string(who) + ": h not positive, or an origin or iso that is not finite");
    return VS_OK;
}

int iso_standalone(vs_ctx* ctx, const double* d_field, int R, const double* origin, double h, double iso, int vcap,
                   int tcap, double* d_verts, int* d_tri, int* d_counts, hipStream_t s) {
    Iso a{};
    a.field = d_field, a.R = R, a.vcap = vcap, a.tcap = tcap, a.verts = d_verts, a.tri = d_tri;
    a.nodes = (size_t)R * R * R;
    const size_t padded = pad_tile(a.nodes);
    double* geo;
    int* bsum;
    VS_CHECK(carve_buf(ctx->cloud_poisson, [&](Carver& p) {
        a.voff = p.take<int>(padded);
        a.toff = p.take<int>(padded);
        a.mask = p.take<uint8_t>(a.nodes);
        geo = p.take<double>(5);
        bsum = p.take<int>(kMaxTiles);
    }));
    a.geo = geo;
    PS_LAUNCH(k_iso_geo, 1, 64, geo, origin[0], origin[1], origin[2], h, iso);
    return iso_enqueue(ctx, a, bsum, d_counts, s);
}

}  // namespace

}  // namespace vs

using namespace vs;

extern "C" {

void vs_cloud_poisson_default_config(vs_cloud_poisson_config* c) {
    if (!c) return;
    c->resolution = 256;  // PoissonRecon --depth 8 (main.cpp:1425)
    c->scale = 1.1;       // PoissonRecon's --scale default
    c->tol = 1e-6;
    c->max_iter = 0;      // 8 * resolution
    c->solver = VS_POISSON_SOLVER_CG;
    c->point_weight = 0;  // PoissonRecon --pointWeight; the reference's command passes 6
    c->trim = 0;          // SurfaceTrimmer --trim, in units of W
}

int vs_cloud_orient_normals_dev(vs_ctx* ctx, const double* d_pts, double* d_normals, int n, const double* d_views, int m,
                                void* stream) {
    VS_ARG(ctx && d_views && (n <= 0 || (d_pts && d_normals)), "vs_cloud_orient_normals_dev: null argument");
    VS_CHECK(orient_check("vs_cloud_orient_normals_dev", n, m));
    VS_HIP(hipSetDevice(ctx->device));
    return orient_enqueue(ctx, d_pts, d_normals, n, d_views, m, stream ? (hipStream_t)stream : ctx->stream);
}

int vs_cloud_orient_normals(vs_ctx* ctx, const double* pts, double* normals, int n, const double* views, int m) {
    VS_ARG(ctx && views && (n <= 0 || (pts && normals)), "vs_cloud_orient_normals: null argument");
    VS_CHECK(orient_check("vs_cloud_orient_normals", n, m));
    if (n == 0) return VS_OK;
    VS_HIP(hipSetDevice(ctx->device));
    const hipStream_t s = ctx->stream;
    const size_t pb = (size_t)n * 3 * sizeof(double), vb = (size_t)m * 3 * sizeof(double);
    double *d_in, *d_nrm, *d_views;
    VS_CHECK(carve_buf(ctx->h_aux0, [&](Carver& h) {
        d_in = h.take<double>((size_t)n * 3);
        d_nrm = h.take<double>((size_t)n * 3);
        d_views = h.take<double>((size_t)m * 3);
    }));
    VS_HIP(hipMemcpyAsync(d_in, pts, pb, hipMemcpyHostToDevice, s));
    VS_HIP(hipMemcpyAsync(d_nrm, normals, pb, hipMemcpyHostToDevice, s));
    VS_HIP(hipMemcpyAsync(d_views, views, vb, hipMemcpyHostToDevice, s));
    VS_CHECK(orient_enqueue(ctx, d_in, d_nrm, n, d_views, m, s));
    VS_HIP(hipMemcpyAsync(normals, d_nrm, pb, hipMemcpyDeviceToHost, s));
    VS_HIP(hipStreamSynchronize(s));
    return VS_OK;
}

int vs_grid_isosurface_dev(vs_ctx* ctx, const double* d_field, int resolution, const double origin[3], double h,
                           double iso, int vcap, int tcap, double* d_verts, int* d_tri, int* d_counts, void* stream) {
    VS_ARG(ctx && d_field && d_counts && vcap >= 0 && tcap >= 0 && (vcap == 0 || d_verts) && (tcap == 0 || d_tri),
           "vs_grid_isosurface_dev: null argument or bad size");
    VS_CHECK(iso_check("vs_grid_isosurface_dev", resolution, origin, h, iso));
    VS_HIP(hipSetDevice(ctx->device));
    return iso_standalone(ctx, d_field, resolution, origin, h, iso, vcap, tcap, d_verts, d_tri, d_counts,
                          stream ? (hipStream_t)stream : ctx->stream);
}

// the first min(cap, count) vertices and triangles to the host, after counts arrived
static int mesh_to_host(hipStream_t s, const int counts[2], int vcap, int tcap, const double* d_verts, const int* d_tri,
                        double* verts, int* tri) {
    const int nv = std::min(vcap, counts[0]), nt = std::min(tcap, counts[1]);
    if (nv > 0) VS_HIP(hipMemcpyAsync(verts, d_verts, (size_t)nv * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (nt > 0) VS_HIP(hipMemcpyAsync(tri, d_tri, (size_t)nt * 3 * sizeof(int), hipMemcpyDeviceToHost, s));
    VS_HIP(hipStreamSynchronize(s));
    return VS_OK;
}

int vs_grid_isosurface(vs_ctx* ctx, const double* field, int resolution, const double origin[3], double h, double iso,
                       int vcap, int tcap, double* verts, int* tri, int counts[2]) {
    VS_ARG(ctx && field && counts && vcap >= 0 && tcap >= 0 && (vcap == 0 || verts) && (tcap == 0 || tri),
           "vs_grid_isosurface: null argument or bad size");
    VS_CHECK(iso_check("vs_grid_isosurface", resolution, origin, h, iso));
    VS_HIP(hipSetDevice(ctx->device));
    const hipStream_t s = ctx->stream;
    const size_t nodes = (size_t)resolution * resolution * resolution;
    double *d_field, *d_verts;
    int *d_tri, *d_counts;
    VS_CHECK(carve_buf(ctx->h_aux0, [&](Carver& p) {
        d_field = p.take<double>(nodes);
        d_verts = p.take<double>((size_t)std::max(vcap, 1) * 3);
        d_tri = p.take<int>((size_t)std::max(tcap, 1) * 3);
        d_counts = p.take<int>(2);
    }));
    VS_HIP(hipMemcpyAsync(d_field, field, nodes * sizeof(double), hipMemcpyHostToDevice, s));
    VS_CHECK(iso_standalone(ctx, d_field, resolution, origin, h, iso, vcap, tcap, d_verts, d_tri, d_counts, s));
    VS_HIP(hipMemcpyAsync(counts, d_counts, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    VS_HIP(hipStreamSynchronize(s));
    return mesh_to_host(s, counts, vcap, tcap, d_verts, d_tri, verts, tri);
}

int vs_cloud_poisson_density_dev(vs_ctx* ctx, const double* d_pts, const double* d_normals, int n,
                                 const vs_cloud_poisson_config* cfg, int vcap, int tcap, double* d_verts, int* d_tri,
                                 int* d_counts, double* d_info, double* d_vert_density, void* stream) {
    VS_ARG(ctx && d_pts && d_normals && d_counts && d_info && vcap >= 0 && tcap >= 0 && (vcap == 0 || d_verts) &&
               (tcap == 0 || d_tri),
           "vs_cloud_poisson_dev: null argument or bad size");
    vs_cloud_poisson_config c = config_or(cfg, vs_cloud_poisson_default_config);
    int sc_iter;
    VS_CHECK(poisson_check("vs_cloud_poisson_dev", c, n, &sc_iter));
    VS_HIP(hipSetDevice(ctx->device));
    const hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    Plan pl;
    VS_CHECK(poisson_plan(ctx, d_pts, d_normals, n, c, sc_iter, d_vert_density != nullptr, &pl));
    VS_CHECK(poisson_rhs(ctx, pl, s));
    if (c.solver == VS_POISSON_SOLVER_DIRECT) {
        VS_CHECK(direct_solve(ctx, pl, s));
    } else {
        if (pl.screened) VS_HIP(hipMemcpyAsync(pl.a.arr[6], pl.a.arr[3], pl.nodes * sizeof(double), hipMemcpyDeviceToDevice, s));
        VS_CHECK(cg_start(ctx, pl, s));
        VS_CHECK(cg_iterate(ctx, pl, 0, c.max_iter, s));
    }
    if (pl.screened) {
        VS_CHECK(screened_start(ctx, pl, s));
        VS_CHECK(screen_iterate(ctx, pl.sc, 0, sc_iter, s));
    }
    return poisson_finish(ctx, pl, vcap, tcap, d_verts, d_tri, d_counts, d_info, d_vert_density, s);
}

int vs_cloud_poisson_dev(vs_ctx* ctx, const double* d_pts, const double* d_normals, int n,
                         const vs_cloud_poisson_config* cfg, int vcap, int tcap, double* d_verts, int* d_tri,
                         int* d_counts, double* d_info, void* stream) {
    return vs_cloud_poisson_density_dev(ctx, d_pts, d_normals, n, cfg, vcap, tcap, d_verts, d_tri, d_counts, d_info,
                                        nullptr, stream);
}

int vs_cloud_poisson(vs_ctx* ctx, const double* pts, const double* normals, int n, const double* views, int m,
                     const vs_cloud_poisson_config* cfg, int vcap, int tcap, double* verts, int* tri, int counts[2],
                     double info[4], double* normals_out, double* rhs_out, double* field_out) {
    return vs_cloud_poisson_density(ctx, pts, normals, n, views, m, cfg, vcap, tcap, verts, tri, counts, info,
                                    normals_out, rhs_out, field_out, nullptr, nullptr);
}

int vs_cloud_poisson_density(vs_ctx* ctx, const double* pts, const double* normals, int n, const double* views, int m,
                             const vs_cloud_poisson_config* cfg, int vcap, int tcap, double* verts, int* tri,
                             int counts[2], double info[4], double* normals_out, double* rhs_out, double* field_out,
                             double* density_out, double* vert_density) {
    VS_ARG(ctx && pts && counts && info && vcap >= 0 && tcap >= 0 && (vcap == 0 || verts) && (tcap == 0 || tri) &&
               (normals || views),
           "vs_cloud_poisson: null argument, bad size, or neither normals nor views");
    vs_cloud_poisson_config c = config_or(cfg, vs_cloud_poisson_default_config);
    int sc_iter;
    VS_CHECK(poisson_check("vs_cloud_poisson", c, n, &sc_iter));
    if (views) VS_CHECK(orient_check("vs_cloud_poisson", n, m));
    double ext = 0;  // the box's largest edge, before the staging is sized
    for (int ax = 0; ax < 3; ax++) {
        double lo = pts[ax], hi = pts[ax];
        for (size_t i = 1; i < (size_t)n; i++) lo = std::fmin(lo, pts[3 * i + ax]), hi = std::fmax(hi, pts[3 * i + ax]);
        ext = std::fmax(ext, hi - lo);
    }
    VS_ARG(c.scale * ext > 0 && std::isfinite(c.scale * ext), "vs_cloud_poisson: the points have no extent");
    VS_HIP(hipSetDevice(ctx->device));
    const hipStream_t s = ctx->stream;
    const size_t pb = (size_t)n * 3 * sizeof(double);
    double *d_in, *d_nrm, *d_views, *d_verts, *d_info, *d_vdens = nullptr;
    int *d_tri, *d_counts;
    VS_CHECK(carve_buf(ctx->h_aux0, [&](Carver& h) {
        d_in = h.take<double>((size_t)n * 3);
        d_nrm = h.take<double>((size_t)n * 3);
        d_views = h.take<double>((size_t)std::max(m, 1) * 3);
        d_verts = h.take<double>((size_t)std::max(vcap, 1) * 3);
        d_tri = h.take<int>((size_t)std::max(tcap, 1) * 3);
        d_counts = h.take<int>(2);
        d_info = h.take<double>(4);
        if (vert_density) d_vdens = h.take<double>(std::max(vcap, 1));
    }));
    VS_HIP(hipMemcpyAsync(d_in, pts, pb, hipMemcpyHostToDevice, s));
    if (normals) {
        VS_HIP(hipMemcpyAsync(d_nrm, normals, pb, hipMemcpyHostToDevice, s));
    } else {  // main.cpp:1379: estimate_normals with k = 20; the grid search returns the same lists above 2^18 points
        VS_CHECK(cloud_normals(ctx, d_in, n, kNormalK, d_nrm, nullptr, s, n > VS_CLOUD_MAX_POINTS));
    }
    if (views) {
        VS_HIP(hipMemcpyAsync(d_views, views, (size_t)m * 3 * sizeof(double), hipMemcpyHostToDevice, s));
        VS_CHECK(orient_enqueue(ctx, d_in, d_nrm, n, d_views, m, s));
    }
    if (normals_out) VS_HIP(hipMemcpyAsync(normals_out, d_nrm, pb, hipMemcpyDeviceToHost, s));
    Plan pl;
    VS_CHECK(poisson_plan(ctx, d_in, d_nrm, n, c, sc_iter, density_out || vert_density, &pl));
    VS_CHECK(poisson_rhs(ctx, pl, s));
    if (rhs_out) VS_HIP(hipMemcpyAsync(rhs_out, pl.a.arr[3], pl.nodes * sizeof(double), hipMemcpyDeviceToHost, s));
    if (density_out) VS_HIP(hipMemcpyAsync(density_out, pl.a.arr[5], pl.nodes * sizeof(double), hipMemcpyDeviceToHost, s));
    const bool direct = c.solver == VS_POISSON_SOLVER_DIRECT;
    if (!direct && pl.screened) VS_HIP(hipMemcpyAsync(pl.a.arr[6], pl.a.arr[3], pl.nodes * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (direct) VS_CHECK(direct_solve(ctx, pl, s));
    else VS_CHECK(cg_start(ctx, pl, s));
    for (int it = 0; it < c.max_iter && !direct; it += kPoll) {
        int done = 0;
        VS_HIP(hipMemcpyAsync(&done, &pl.a.st->done, sizeof(int), hipMemcpyDeviceToHost, s));
        VS_HIP(hipStreamSynchronize(s));
        if (done) break;
        VS_CHECK(cg_iterate(ctx, pl, it, std::min(it + kPoll, c.max_iter), s));
    }
    if (pl.screened) VS_CHECK(screened_start(ctx, pl, s));
    const int poll = direct ? kScPoll : kPoll;
    for (int it = 0; it < sc_iter && pl.screened; it += poll) {
        int go = 0;
        VS_HIP(hipMemcpyAsync(&go, &pl.a.st->go, sizeof(int), hipMemcpyDeviceToHost, s));
        VS_HIP(hipStreamSynchronize(s));
        if (!go) break;
        VS_CHECK(screen_iterate(ctx, pl.sc, it, std::min(it + poll, sc_iter), s));
    }
    if (field_out) VS_HIP(hipMemcpyAsync(field_out, pl.a.arr[0], pl.nodes * sizeof(double), hipMemcpyDeviceToHost, s));
    VS_CHECK(poisson_finish(ctx, pl, vcap, tcap, d_verts, d_tri, d_counts, d_info, d_vdens, s));
    VS_HIP(hipMemcpyAsync(counts, d_counts, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
    VS_HIP(hipMemcpyAsync(info, d_info, 4 * sizeof(double), hipMemcpyDeviceToHost, s));
    VS_HIP(hipStreamSynchronize(s));
    const int nv = std::min(vcap, counts[0]);
    if (vert_density && nv > 0) VS_HIP(hipMemcpyAsync(vert_density, d_vdens, (size_t)nv * sizeof(double), hipMemcpyDeviceToHost, s));
    return mesh_to_host(s, counts, vcap, tcap, d_verts, d_tri, verts, tri);
}

}  // extern "C"

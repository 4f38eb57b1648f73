// densify.hip — estimate_normals (reference src/main.cpp:645-672) and densify_surfaces (:846-965) on the device,
// the two steps that follow the cloud filter (cloud.hip) after every processed frame (:1212) and before the final
// PLY (:1369-1387).  All arithmetic is fp64 in the reference's order, compiled without contraction.
//
// Normals: cloud.hip's exact brute-force search gives every point its k - 1 nearest others by (d2, index);
//   k_cloud_normals  one point per lane: merges the S partial lists (knn_merge), sums the centroid and the scatter
//                    matrix in list order, the point itself first, and takes the eigenvector of the smallest
//                    eigenvalue (scatter_eig; these, block_rank and Carver come from cloud_common.h).
// Densification: the radius search runs on a uniform cell grid in HBM (edge = radius (1 + 2^-20), so a neighbour
// inside the radius sits in one of the 27 surrounding cells whatever the rounding of the cell index).  The grid is
// a counting sort of the points by the hash of their packed cell coordinates (21 bits per axis) into a power-of-two
// bucket table; every sorted entry carries its cell key, so two cells that share a bucket cost key compares and
// nothing else.  The order inside a bucket depends on the atomics' scheduling and reaches no result: the radius
// matches are sorted by (d2, index), the 1-NN test is an "any".
//   k_dz_init    clears the bucket histogram, the voxel table and the call's state words
//   k_dz_cells   cell key and bucket count per point (integer atomics), the cloud's minimum voxel coordinates
//   k_dz_scan    one workgroup: exclusive scan (bucket starts; later the compaction's block sums)
//   k_dz_fill    scatters index, key and coordinates into the sorted arrays
//   k_dz_plane   one wave (one 64-lane workgroup) per input point:
//                lanes 0..26 look up the 27 buckets, a wave scan concatenates their ranges and the 64 lanes stride
//                over the concatenation (two dependent global reads per member instead of 27 bucket walks);
//                matches (d2 < r^2, strict) are appended to an LDS list by ballot (VS_DENSIFY_MAX_NEIGHBOURS
//                entries; more: the point generates nothing and is counted); a bitonic sort in LDS orders the
//                list by (d2, index); the coplanar filter compacts it, again by ballot, into x / y / z arrays
//                (the point itself first); centroid, scatter and extents are lane-strided partial results joined by
//                an xor butterfly (a fixed order, and the same bits in every lane, so the eigen-solve and the
//                branches after it are uniform); then one lattice node per lane (slot [iu][iv], u and v built by
//                repeated addition): the near test walks the coplanar list in LDS (a broadcast read), the 1-NN test
//                walks only those of the candidate's 27 cells that the bound sqrt(0.2) step can reach and leaves at
//                the first input point below it.  Accepted candidates go to slot [i][iu][iv] with a flag byte.
//   k_dz_insert  every entry (input points, then the candidate slots: the entry number is the insertion rank)
//                claims its voxel's slot of an open-addressing table with a 64-bit compare-and-swap and lowers the
//                slot's rank with atomicMin: the minimum does not depend on the scheduling
//   k_dz_count / k_dz_scan / k_dz_emit   an entry wins when its rank is its voxel's; block sums, their scan, and
//                the stable compaction of the winners into d_out / d_src and the counts
// LDS per k_dz_plane workgroup: 3 x 4 KB coordinates (the first array holds d2 until the sort is done) + 2 KB indices
// + 0.4 KB cell ranges = 14.4 KB, 11 workgroups per CU.  No kernel keeps state between launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "cloud_common.h"

namespace vs {

namespace {

constexpr int kCap = VS_DENSIFY_MAX_NEIGHBOURS;
constexpr int kBlk = 1024;                   // entries per compaction block
constexpr long long kMaxEntries = 1ll << 24; // n (1 + lattice nodes)
constexpr unsigned long long kEmpty = ~0ull;
constexpr int kNormalK = 20;  // main.cpp:861
constexpr int kMinPoints = 20;  // main.cpp:850

enum { kStErr = 0, kStSkipped = 1, kStVmin = 2, kStWords = 5 };

// The sign rule: the component of largest magnitude is positive; on equal magnitudes the lowest index decides.
__device__ __forceinline__ void orient(double& x, double& y, double& z) {
    const double ax = fabs(x), ay = fabs(y), az = fabs(z);
    const double lead = (ax >= ay && ax >= az) ? x : (ay >= az ? y : z);
    if (lead < 0) x = -x, y = -y, z = -z;
}

struct NormalArgs {
    const double* pts;
    int n_max, k, S;
    const double* part_d2;  // [S][k - 1][n_max]
    const int* part_idx;
    double* normals;  // [n][3]
    double* eig;      // [n][3] descending, nullable
};

__global__ __launch_bounds__(kKnnLanes) void k_cloud_normals(NormalArgs a) {
    __shared__ uint8_t s_cur[kKnnMaxSplit * kKnnLanes];  // [list][lane]: entries of the list consumed
    __shared__ int s_nbr[VS_CLOUD_MAX_K * kKnnLanes];    // [slot][lane]: the point, then its neighbours
    const int n = a.n_max;
    const int tid = threadIdx.x, q = blockIdx.x * kKnnLanes + tid;
    if (q >= n) return;
    const int found = min(a.k, n);  // the reference's query returns the point itself as well
    double nx = 0, ny = 0, nz = 1, w[3] = {0, 0, 0};  // main.cpp:655
    if (found >= 3) {
        s_nbr[tid] = q;
        knn_merge(a.part_d2, a.part_idx, a.S, a.k - 1, a.n_max, q, s_cur + tid, found - 1, [&](int t, double, int idx) {
            s_nbr[(t + 1) * kKnnLanes + tid] = idx == kNoIdx ? q : idx;  // only with non-finite coordinates
        });
        double V[9];
        scatter_eig(a.pts, s_nbr + tid, found, w, V);
        nx = V[2], ny = V[5], nz = V[8];  // the smallest eigenvalue's column
        orient(nx, ny, nz);
    }
    a.normals[3 * (size_t)q] = nx;
    a.normals[3 * (size_t)q + 1] = ny;
    a.normals[3 * (size_t)q + 2] = nz;
    if (a.eig) {
        a.eig[3 * (size_t)q] = w[0];
        a.eig[3 * (size_t)q + 1] = w[1];
        a.eig[3 * (size_t)q + 2] = w[2];
    }
}

// One densification call: the configuration's derived constants and the context's scratch.
struct Dz {
    const double* pts;
    int n_max;
    double r2, step, thresh, edge, voxel, near2, min2, reach;  // reach: the 1-NN bound in cells, with slack
    int Gs, G;            // lattice nodes per axis and per point
    int T, t_shift;       // buckets of the cell grid (a power of two), 64 - log2 T
    int slot_shift;       // the voxel table: 64 - log2 slots
    unsigned slot_mask;
    int vmargin;          // voxels a candidate can lie below the inputs' minimum
    int n_pad, E, nblk;   // entries: inputs at [0, n_pad), candidate slot s at n_pad + s; nblk blocks of kBlk
    double* normals;      // [n_max][3]
    unsigned long long* pkey;  // [n_max] packed cell per point
    int* hist;            // [T + 1] bucket counts, then starts
    int* cursor;          // [T]
    int* sidx;            // sorted by bucket: input index, cell key, coordinates
    unsigned long long* skey;
    double* spts;
    int* state;           // kStWords
    double* cand;         // [n_max G][3]
    uint8_t* cflag;       // [n_max G]
    unsigned long long* tkeys;  // [slots] packed voxel or kEmpty
    int* tranks;          // [slots] lowest entry number
    int* eslot;           // [E] the entry's slot
    int* bsum;            // [nblk + 1]
    int cap;
    double* out;
    int* src;
    int* counts;
};

// One loop over the voxel table's slots clears the shorter arrays too: T + 1 <= slots (T <= max(1024, 2 n) and
// slots >= 2 (n_pad + n G) with n_pad >= 1024, G >= 1), which cloud_densify checks, and kStWords <= slots.
__global__ __launch_bounds__(256) void k_dz_init(Dz a) {
    const size_t slots = (size_t)a.slot_mask + 1, stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < slots; i += stride) {
        a.tkeys[i] = kEmpty;
        a.tranks[i] = INT_MAX;
        if (i <= (size_t)a.T) a.hist[i] = 0;
        if (i < (size_t)a.T) a.cursor[i] = 0;
        if (i < kStWords) a.state[i] = i >= kStVmin ? INT_MAX : 0;
    }
}

__global__ __launch_bounds__(256) void k_dz_cells(Dz a) {
    const int n = a.n_max, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || n < kMinPoints) return;
    long long c[3];
    bool ok = true;
    for (int ax = 0; ax < 3; ax++) {
        const double p = a.pts[3 * (size_t)i + ax];
        const double cell = floor(p / a.edge), vox = floor(p / a.voxel);
        ok = ok && fabs(cell) < (double)(kAxisBias - 1) && fabs(vox) < 1073741824.0;
        c[ax] = ok ? (long long)cell + kAxisBias : 0;
        if (ok) atomicMin(&a.state[kStVmin + ax], (int)vox);
    }
    if (!ok) {
        atomicOr(&a.state[kStErr], 1);
        return;
    }
    const unsigned long long key = pack3(c[0], c[1], c[2]);
    a.pkey[i] = key;
    atomicAdd(&a.hist[hash_bits(key, a.t_shift)], 1);
}

// data[0 .. count) -> its exclusive prefix sums, data[count] = the total
__global__ __launch_bounds__(1024) void k_dz_scan(int* data, int count) {
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

__global__ __launch_bounds__(256) void k_dz_fill(Dz a) {
    const int n = a.n_max, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || n < kMinPoints || a.state[kStErr]) return;
    const unsigned long long key = a.pkey[i];
    const unsigned b = hash_bits(key, a.t_shift);
    const int pos = a.hist[b] + atomicAdd(&a.cursor[b], 1);  // < hist[b + 1] <= n
    a.sidx[pos] = i;
    a.skey[pos] = key;
    a.spts[3 * (size_t)pos] = a.pts[3 * (size_t)i];
    a.spts[3 * (size_t)pos + 1] = a.pts[3 * (size_t)i + 1];
    a.spts[3 * (size_t)pos + 2] = a.pts[3 * (size_t)i + 2];
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// True when an input point lies closer than sqrt(min2) to c (the reference's 1-NN query, main.cpp:925-926).
__device__ bool dz_close_to_input(const Dz& a, double x, double y, double z) {
    const double c[3] = {x, y, z};
    long long cell[3];
    int lo[3], hi[3];
    for (int ax = 0; ax < 3; ax++) {
        const double f = c[ax] / a.edge, fl = floor(f);
        cell[ax] = (long long)fl + kAxisBias;
        lo[ax] = f - fl < a.reach ? -1 : 0;  // the neighbour cell is within the bound's reach
        hi[ax] = 1.0 - (f - fl) < a.reach ? 1 : 0;
    }
    for (int dz = lo[2]; dz <= hi[2]; dz++)
        for (int dy = lo[1]; dy <= hi[1]; dy++)
            for (int dx = lo[0]; dx <= hi[0]; dx++) {
                const long long nx = cell[0] + dx, ny = cell[1] + dy, nz = cell[2] + dz;
                if (!fits(nx) || !fits(ny) || !fits(nz)) continue;  // no input point lives there
                const unsigned long long key = pack3(nx, ny, nz);
                const unsigned b = hash_bits(key, a.t_shift);
                const int end = a.hist[b + 1];
                for (int m = a.hist[b]; m < end; m++) {
                    if (a.skey[m] != key) continue;
                    const double ex = x - a.spts[3 * (size_t)m], ey = y - a.spts[3 * (size_t)m + 1],
                                 ez = z - a.spts[3 * (size_t)m + 2];
                    if (ex * ex + ey * ey + ez * ez < a.min2) return true;
                }
            }
    return false;
}

// grid n_max workgroups of one wave: point i = blockIdx.x.  Every __syncthreads is this wave's own.
__global__ __launch_bounds__(64) void k_dz_plane(Dz a) {
    __shared__ double s_x[kCap], s_y[kCap], s_z[kCap];  // s_x holds d2 until the sort is done
    __shared__ int s_idx[kCap];
    __shared__ int s_pre[28], s_beg[27];
    __shared__ unsigned long long s_ck[27];
    const int n = a.n_max, i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    const int G = a.G;
    for (int node = lane; node < G; node += 64) a.cflag[(size_t)i * G + node] = 0;
    if (n < kMinPoints || a.state[kStErr]) return;
    const double px = a.pts[3 * (size_t)i], py = a.pts[3 * (size_t)i + 1], pz = a.pts[3 * (size_t)i + 2];

    // ---- the radius search over the 27 cells around the point
    const unsigned long long key = a.pkey[i];
    int cnt27 = 0;
    if (lane < 27) {
        const long long nx = (long long)((key >> (2 * kAxisBits)) & 0x1FFFFF) + lane % 3 - 1;
        const long long ny = (long long)((key >> kAxisBits) & 0x1FFFFF) + (lane / 3) % 3 - 1;
        const long long nz = (long long)(key & 0x1FFFFF) + lane / 9 - 1;
        const unsigned long long k2 = pack3(nx, ny, nz);  // k_dz_cells keeps every axis off the range's ends
        const unsigned b = hash_bits(k2, a.t_shift);
        const int beg = a.hist[b];
        cnt27 = a.hist[b + 1] - beg;
        s_ck[lane] = k2;
        s_beg[lane] = beg;
    }
    int inc = cnt27;
    for (int o = 1; o < 32; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane < 27) s_pre[lane + 1] = inc;
    if (lane == 0) s_pre[0] = 0;
    __syncthreads();
    const int total = s_pre[27];
    const unsigned long long below = (1ull << lane) - 1ull;
    int cnt = 0;
    for (int t0 = 0; t0 < total; t0 += 64) {
        const int t = t0 + lane;
        bool hit = false;
        double d2 = 0;
        int j = 0;
        if (t < total) {
            int c = 0;
            while (s_pre[c + 1] <= t) c++;  // t < s_pre[27]: c stays below 27
            const int m = s_beg[c] + t - s_pre[c];
            if (a.skey[m] == s_ck[c]) {
                const double dx = px - a.spts[3 * (size_t)m], dy = py - a.spts[3 * (size_t)m + 1],
                             dz = pz - a.spts[3 * (size_t)m + 2];
                d2 = dx * dx + dy * dy + dz * dz;
                hit = d2 < a.r2;  // strict (nanoflann's RadiusResultSet)
                j = a.sidx[m];
            }
        }
        const unsigned long long bal = __ballot(hit);
        const int pos = cnt + __popcll(bal & below);
        if (hit && pos < kCap) {
            s_x[pos] = d2;
            s_idx[pos] = j;
        }
        cnt += __popcll(bal);
    }
    if (cnt > kCap) {  // the deviation from the reference: counted, nothing generated
        if (lane == 0) atomicAdd(&a.state[kStSkipped], 1);
        return;
    }

    // ---- bitonic sort by (d2, index) over the next power of two
    int P = 64;
    while (P < cnt) P <<= 1;
    for (int t = cnt + lane; t < P; t += 64) {
        s_x[t] = INFINITY;
        s_idx[t] = kNoIdx;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < P / 2; t += 64) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo + j;
                const double dl = s_x[lo], dh = s_x[hi];
                const int il = s_idx[lo], ih = s_idx[hi];
                const bool gt = dl > dh || (dl == dh && il > ih), lt = dh > dl || (dl == dh && ih > il);
                if ((lo & k2) == 0 ? gt : lt) {
                    s_x[lo] = dh;
                    s_x[hi] = dl;
                    s_idx[lo] = ih;
                    s_idx[hi] = il;
                }
            }
            __syncthreads();
        }

    // ---- the coplanar list (main.cpp:879-889): the point, then the neighbours whose normal is nearly parallel
    const double nix = a.normals[3 * (size_t)i], niy = a.normals[3 * (size_t)i + 1], niz = a.normals[3 * (size_t)i + 2];
    int m = 1;
    for (int t0 = 0; t0 < cnt; t0 += 64) {
        const int t = t0 + lane;
        bool keep = false;
        int j = 0;
        if (t < cnt) {
            j = s_idx[t];
            if (j != i) {
                const double* nj = a.normals + 3 * (size_t)j;
                keep = fabs(nix * nj[0] + niy * nj[1] + niz * nj[2]) >= a.thresh;
            }
        }
        const unsigned long long bal = __ballot(keep);
        const int pos = m + __popcll(bal & below);  // < cnt <= kCap: the point itself is a match and is not kept
        if (keep) {
            s_x[pos] = a.pts[3 * (size_t)j];
            s_y[pos] = a.pts[3 * (size_t)j + 1];
            s_z[pos] = a.pts[3 * (size_t)j + 2];
        }
        m += __popcll(bal);
    }
    if (lane == 0) s_x[0] = px, s_y[0] = py, s_z[0] = pz;
    __syncthreads();
    if (m < 4) return;

    // ---- the plane fit (main.cpp:891-909)
    double sx = 0, sy = 0, sz = 0;
    for (int t = lane; t < m; t += 64) sx += s_x[t], sy += s_y[t], sz += s_z[t];
    const double cx = wave_sum(sx) / (double)m, cy = wave_sum(sy) / (double)m, cz = wave_sum(sz) / (double)m;
    Scatter3 sc;
    for (int t = lane; t < m; t += 64) sc.add(s_x[t] - cx, s_y[t] - cy, s_z[t] - cz);
    sc.c00 = wave_sum(sc.c00), sc.c01 = wave_sum(sc.c01), sc.c02 = wave_sum(sc.c02);
    sc.c11 = wave_sum(sc.c11), sc.c12 = wave_sum(sc.c12), sc.c22 = wave_sum(sc.c22);
    double A[9], w[3], V[9];
    sc.fill(A);
    vs_pnp::sym_eig_static<3>(A, w, V);
    const double l1 = w[0], l3 = w[2];
    if (l1 < 1e-12 || l3 / l1 > 0.15) return;
    double ux = V[0], uy = V[3], uz = V[6], vx = V[1], vy = V[4], vz = V[7];
    orient(ux, uy, uz);
    orient(vx, vy, vz);
    double u_lo = 1e9, u_hi = -1e9, v_lo = 1e9, v_hi = -1e9;
    for (int t = lane; t < m; t += 64) {
        const double dx = s_x[t] - cx, dy = s_y[t] - cy, dz = s_z[t] - cz;
        const double u = dx * ux + dy * uy + dz * uz, v = dx * vx + dy * vy + dz * vz;
        u_lo = fmin(u_lo, u), u_hi = fmax(u_hi, u);
        v_lo = fmin(v_lo, v), v_hi = fmax(v_hi, v);
    }
    u_lo = wave_min(u_lo), u_hi = wave_max(u_hi), v_lo = wave_min(v_lo), v_hi = wave_max(v_hi);

    // ---- the lattice (main.cpp:920-940): node (iu, iv) per lane
    for (int node0 = 0; node0 < G; node0 += 64) {
        const int node = node0 + lane, iu = node / a.Gs, iv = node % a.Gs;
        double u = u_lo, v = v_lo;
        for (int t = 0; t < iu; t++) u += a.step;
        for (int t = 0; t < iv; t++) v += a.step;
        bool act = node < G && u <= u_hi && v <= v_hi;
        const double x = cx + u * ux + v * vx, y = cy + u * uy + v * vy, z = cz + u * uz + v * vz;
        if (act) {  // lanes past the lattice or the extents skip the walk
            bool near = false;
            for (int t = 0; t < m && !near; t++) {
                const double dx = x - s_x[t], dy = y - s_y[t], dz = z - s_z[t];
                near = dx * dx + dy * dy + dz * dz < a.near2;
            }
            act = near;
        }
        if (act && dz_close_to_input(a, x, y, z)) act = false;
        if (act) {
            const size_t slot = (size_t)i * G + node;
            a.cand[3 * slot] = x;
            a.cand[3 * slot + 1] = y;
            a.cand[3 * slot + 2] = z;
            a.cflag[slot] = 1;
        }
    }
}

// Entry e: the input point e (e < n_pad) or candidate slot e - n_pad.  Its coordinates when it takes part.
__device__ __forceinline__ const double* dz_entry(const Dz& a, int n, int e) {
    if (e < a.n_pad) return e < n ? a.pts + 3 * (size_t)e : nullptr;
    const int s = e - a.n_pad;
    if (e >= a.E || s / a.G >= n || !a.cflag[s]) return nullptr;
    return a.cand + 3 * (size_t)s;
}

__global__ __launch_bounds__(256) void k_dz_insert(Dz a) {
    const int n = a.n_max, e = blockIdx.x * 256 + threadIdx.x;
    if (n < kMinPoints || a.state[kStErr]) return;
    const double* p = dz_entry(a, n, e);
    if (!p) return;
    long long v[3];
    bool ok = true;
    for (int ax = 0; ax < 3; ax++) {
        const double vox = floor(p[ax] / a.voxel);  // a division, as main.cpp:953-955
        ok = ok && fabs(vox) < 1073741824.0;
        v[ax] = ok ? (long long)vox - ((long long)a.state[kStVmin + ax] - a.vmargin) : -1;
        ok = ok && fits(v[ax]);
    }
    if (!ok) {
        atomicOr(&a.state[kStErr], 1);
        return;
    }
    const unsigned long long key = pack3(v[0], v[1], v[2]);
    unsigned h = hash_bits(key, a.slot_shift);
    for (unsigned probe = 0; probe <= a.slot_mask; probe++) {  // the table has twice the entries' slots
        const unsigned long long prev = atomicCAS(&a.tkeys[h], kEmpty, key);
        if (prev == kEmpty || prev == key) {
            atomicMin(&a.tranks[h], e);
            a.eslot[e] = (int)h;
            return;
        }
        h = (h + 1) & a.slot_mask;
    }
}

__device__ __forceinline__ bool dz_wins(const Dz& a, int n, int e) {
    if (n < kMinPoints) return e < n;  // main.cpp:850: the input unchanged
    return dz_entry(a, n, e) && a.tranks[a.eslot[e]] == e;
}

__global__ __launch_bounds__(kBlk) void k_dz_count(Dz a) {
    __shared__ int s_w[16];
    const int n = a.n_max, tid = threadIdx.x, e = blockIdx.x * kBlk + tid;
    int total;
    block_rank(!a.state[kStErr] && dz_wins(a, n, e), s_w, total);
    if (tid == 0) a.bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlk) void k_dz_emit(Dz a) {
    __shared__ int s_w[16];
    const int n = a.n_max, tid = threadIdx.x, e = blockIdx.x * kBlk + tid;
    const bool err = a.state[kStErr] != 0;
    if (blockIdx.x == 0 && tid == 0) {
        const int kept = a.bsum[a.n_pad / kBlk], total = a.bsum[a.nblk];
        a.counts[0] = err ? 0 : kept;
        a.counts[1] = err ? 0 : total - kept;
        a.counts[2] = err ? -1 : total;
        a.counts[3] = a.state[kStSkipped];
    }
    if (err) return;
    const bool win = dz_wins(a, n, e);
    int total;
    const int rank = a.bsum[blockIdx.x] + block_rank(win, s_w, total);
    if (!win || rank >= a.cap) return;
    const double* p = dz_entry(a, n, e);
    a.out[3 * (size_t)rank] = p[0];
    a.out[3 * (size_t)rank + 1] = p[1];
    a.out[3 * (size_t)rank + 2] = p[2];
    const int i = e < a.n_pad ? e : (e - a.n_pad) / a.G;
    a.src[rank] = e < a.n_pad ? i : -(i + 1);
}

__global__ void k_dz_empty(int* counts) {
    if (threadIdx.x < 4) counts[threadIdx.x] = 0;
}

int log2_ceil(size_t v) {
    int b = 0;
    while (((size_t)1 << b) < v) b++;
    return b;
}

}  // namespace

int cloud_normals(vs_ctx* ctx, const double* d_pts, int n_max, int k, double* d_normals, double* d_eig,
                  hipStream_t s, bool grid) {
    if (n_max == 0) return VS_OK;
    const int S = grid ? 1 : knn_split(ctx, n_max, 0);
    CloudScratch cs;
    VS_CHECK(cloud_scratch(ctx, n_max, std::max(k - 1, 1), S, &cs));
    if (k >= 3 && grid) {  // k < 3: every normal is (0, 0, 1)
        VS_CHECK(launch_knn_grid(ctx, cs, d_pts, nullptr, n_max, k - 1, 0, 0.0, 0, nullptr, s));
    } else if (k >= 3) {
        ProfScope ps(ctx, "k_cloud_knn", s);
        launch_knn(cs, d_pts, nullptr, n_max, k - 1, S, 0, s);
    }
    ProfScope ps(ctx, "k_cloud_normals", s);
    NormalArgs a{d_pts, n_max, k, S, cs.part_d2, cs.part_idx, d_normals, d_eig};
    hipLaunchKernelGGL(k_cloud_normals, dim3((n_max + kKnnLanes - 1) / kKnnLanes), dim3(kKnnLanes), 0, s, a);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

// n_max <= VS_CLOUD_MAX_POINTS is the entry points' check (cloud_size_check, before they size their staging by it).
int cloud_densify(vs_ctx* ctx, const double* d_pts, int n_max, const vs_cloud_densify_config& c,
                  int cap, double* d_out, int* d_src, int* d_counts, hipStream_t s) {
    const double r = c.search_radius, step = c.fill_step;
    if (!(r > 0) || !(step > 0) || !std::isfinite(r) || !std::isfinite(step) || !std::isfinite(c.normal_thresh)) {
        set_error("vs_cloud_densify: search_radius and fill_step must be positive and finite");
        return VS_ERR_ARG;
    }
    if (step * step * 0.2 > r * r) {  // the 1-NN bound would reach past the 27 cells; nothing could be filled anyway
        set_error("vs_cloud_densify: fill_step above sqrt(5) search_radius");
        return VS_ERR_ARG;
    }
    const double per_axis = std::floor(2.0 * r / step) + 1.0;
    if (per_axis * per_axis > VS_DENSIFY_MAX_GRID) {
        set_error("vs_cloud_densify: more than VS_DENSIFY_MAX_GRID lattice nodes per point");
        return VS_ERR_CAPACITY;
    }
    const int Gs = (int)per_axis, G = Gs * Gs;
    if ((long long)n_max * (1 + G) > kMaxEntries) {
        set_error("vs_cloud_densify: more than 2^24 points and lattice nodes");
        return VS_ERR_CAPACITY;
    }
    if (n_max == 0) {
        hipLaunchKernelGGL(k_dz_empty, dim3(1), dim3(64), 0, s, d_counts);
        VS_HIP(hipGetLastError());
        return VS_OK;
    }
    Dz a{};
    a.pts = d_pts, a.n_max = n_max;
    a.r2 = r * r, a.step = step, a.thresh = c.normal_thresh;
    a.edge = r * (1.0 + 1.0 / 1048576.0);
    a.voxel = step * 0.7;
    a.near2 = a.r2 * 0.5;
    a.min2 = step * step * 0.2;
    // a neighbour cell is visited when the candidate's fractional position is within the bound of the shared face:
    // 2^-20 relative and 2^-30 absolute slack cover the rounding of p / edge for |p / edge| < 2^20
    a.reach = std::sqrt(a.min2) / a.edge * (1.0 + 1.0 / 1048576.0) + 1.0 / 1073741824.0;
    a.Gs = Gs, a.G = G;
    const int t_bits = std::min(18, std::max(10, log2_ceil((size_t)n_max)));
    a.T = 1 << t_bits, a.t_shift = 64 - t_bits;
    a.n_pad = (n_max + kBlk - 1) / kBlk * kBlk;
    a.E = a.n_pad + n_max * G;
    a.nblk = (a.E + kBlk - 1) / kBlk;
    const int s_bits = log2_ceil(2 * (size_t)a.E);
    a.slot_shift = 64 - s_bits, a.slot_mask = (unsigned)(((size_t)1 << s_bits) - 1);
    a.vmargin = (int)std::ceil(std::sqrt(a.near2) / a.voxel) + 2;  // a candidate lies within sqrt(near2) of an input
    a.cap = cap, a.out = d_out, a.src = d_src, a.counts = d_counts;

    const size_t slots = (size_t)a.slot_mask + 1, nG = (size_t)n_max * G;
    if ((size_t)a.T + 1 > slots) {  // k_dz_init's loop; cannot fire for an n and G that densify_check admits
        set_error("vs_cloud_densify: the voxel table is shorter than the cell grid's histogram");
        return VS_ERR_CAPACITY;
    }
    VS_CHECK(carve_buf(ctx->densify, [&](Carver& p) {
        a.normals = p.take<double>((size_t)n_max * 3);
        a.spts = p.take<double>((size_t)n_max * 3);
        a.pkey = p.take<unsigned long long>(n_max);
        a.skey = p.take<unsigned long long>(n_max);
        a.sidx = p.take<int>(n_max);
        a.hist = p.take<int>(a.T + 1);
        a.cursor = p.take<int>(a.T);
        a.state = p.take<int>(kStWords);
        a.cand = p.take<double>(nG * 3);
        a.cflag = p.take<uint8_t>(nG);
        a.tkeys = p.take<unsigned long long>(slots);
        a.tranks = p.take<int>(slots);
        a.eslot = p.take<int>(a.E);
        a.bsum = p.take<int>(a.nblk + 1);
    }));

    const int pblocks = (n_max + 255) / 256;
    const bool work = n_max >= kMinPoints;  // below: the input unchanged
    if (work) VS_CHECK(cloud_normals(ctx, d_pts, n_max, kNormalK, a.normals, nullptr, s));
    // one profile stage per kernel (events only while the context's profile is on)
#define DZ_LAUNCH(kernel, grid, block, ...)                                      \
    do {                                                                         \
        ProfScope ps_(ctx, #kernel, s);                                          \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, __VA_ARGS__);  \
    } while (0)
    DZ_LAUNCH(k_dz_init, (unsigned)std::min<size_t>((slots + 255) / 256, 4096), 256, a);
    if (work) {
        DZ_LAUNCH(k_dz_cells, pblocks, 256, a);
        DZ_LAUNCH(k_dz_scan, 1, 1024, a.hist, a.T);
        DZ_LAUNCH(k_dz_fill, pblocks, 256, a);
        DZ_LAUNCH(k_dz_plane, n_max, 64, a);
        DZ_LAUNCH(k_dz_insert, (a.E + 255) / 256, 256, a);
    }
    DZ_LAUNCH(k_dz_count, a.nblk, kBlk, a);
    DZ_LAUNCH(k_dz_scan, 1, 1024, a.bsum, a.nblk);
    DZ_LAUNCH(k_dz_emit, a.nblk, kBlk, a);
#undef DZ_LAUNCH
    VS_HIP(hipGetLastError());
    return VS_OK;
}

}  // namespace vs

using namespace vs;

extern "C" {

void vs_cloud_densify_default_config(vs_cloud_densify_config* c) {
    if (!c) return;
    c->search_radius = 0.12;  // main.cpp:847-849
    c->fill_step = 0.05;
    c->normal_thresh = 0.95;
}

int vs_cloud_normals_dev(vs_ctx* ctx, const double* d_pts, int n, int k, double* d_normals, double* d_eig,
                         void* stream) {
    VS_ARG(ctx && d_normals && n >= 0 && (n == 0 || d_pts) && k >= 1, "vs_cloud_normals_dev: null argument or bad size");
    VS_CHECK(cloud_size_check("vs_cloud_normals_dev", n, k));
    VS_HIP(hipSetDevice(ctx->device));
    return cloud_normals(ctx, d_pts, n, k, d_normals, d_eig, stream ? (hipStream_t)stream : ctx->stream);
}

int vs_cloud_normals(vs_ctx* ctx, const double* pts, int n, int k, double* normals, double* eig) {
    return cloud_normals_host(ctx, pts, n, k, normals, eig, false);
}

}  // extern "C"

int vs::cloud_normals_host(vs_ctx* ctx, const double* pts, int n, int k, double* normals, double* eig, bool grid) {
    VS_ARG(ctx && normals && n >= 0 && (n == 0 || pts), "vs_cloud_normals: null argument");
    if (n == 0) return VS_OK;
    // before the staging is sized by n
    VS_CHECK(cloud_size_check("vs_cloud_normals", n, k, grid ? VS_CLOUD_GRID_MAX_POINTS : VS_CLOUD_MAX_POINTS));
    VS_ARG(k >= 1, "vs_cloud_normals: bad size");
    VS_HIP(hipSetDevice(ctx->device));
    const hipStream_t s = ctx->stream;
    const size_t pb = (size_t)n * 3 * sizeof(double);
    double *d_in, *d_nrm, *d_eig;
    VS_CHECK(carve_buf(ctx->h_aux0, [&](Carver& h) {
        d_in = h.take<double>((size_t)n * 3);
        d_nrm = h.take<double>((size_t)n * 3);
        d_eig = h.take<double>((size_t)n * 3);
    }));
    VS_HIP(hipMemcpyAsync(d_in, pts, pb, hipMemcpyHostToDevice, s));
    VS_CHECK(cloud_normals(ctx, d_in, n, k, d_nrm, d_eig, s, grid));
    VS_HIP(hipMemcpyAsync(normals, d_nrm, pb, hipMemcpyDeviceToHost, s));
    if (eig) VS_HIP(hipMemcpyAsync(eig, d_eig, pb, hipMemcpyDeviceToHost, s));
    VS_HIP(hipStreamSynchronize(s));
    return VS_OK;
}

extern "C" {

int vs_cloud_densify_dev(vs_ctx* ctx, const double* d_pts, int n, const vs_cloud_densify_config* cfg, int cap,
                         double* d_out, int* d_src, int* d_counts, void* stream) {
    VS_ARG(ctx && d_out && d_src && d_counts && n >= 0 && cap >= 0 && (n == 0 || d_pts),
           "vs_cloud_densify_dev: null argument or bad size");
    VS_CHECK(cloud_size_check("vs_cloud_densify", n, 0));
    VS_HIP(hipSetDevice(ctx->device));
    return cloud_densify(ctx, d_pts, n, config_or(cfg, vs_cloud_densify_default_config), cap, d_out, d_src, d_counts,
                         stream ? (hipStream_t)stream : ctx->stream);
}

int vs_cloud_densify(vs_ctx* ctx, const double* pts, int n, const vs_cloud_densify_config* cfg, int cap, double* out,
                     int* src, int counts[4]) {
    VS_ARG(ctx && out && src && counts && n >= 0 && cap >= 0 && (n == 0 || pts), "vs_cloud_densify: null argument");
    VS_CHECK(cloud_size_check("vs_cloud_densify", n, 0));
    VS_HIP(hipSetDevice(ctx->device));
    const hipStream_t s = ctx->stream;
    double *d_in, *d_out;
    int *d_src, *d_counts;
    VS_CHECK(carve_buf(ctx->h_aux0, [&](Carver& h) {
        d_in = h.take<double>((size_t)std::max(n, 1) * 3);
        d_out = h.take<double>((size_t)std::max(cap, 1) * 3);
        d_src = h.take<int>(std::max(cap, 1));
        d_counts = h.take<int>(4);
    }));
    if (n > 0) VS_HIP(hipMemcpyAsync(d_in, pts, (size_t)n * 3 * sizeof(double), hipMemcpyHostToDevice, s));
    VS_CHECK(cloud_densify(ctx, d_in, n, config_or(cfg, vs_cloud_densify_default_config), cap, d_out, d_src, d_counts,
                           s));
    VS_HIP(hipMemcpyAsync(counts, d_counts, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    VS_HIP(hipStreamSynchronize(s));
    if (counts[2] < 0) {
        set_error("vs_cloud_densify: the cloud's cells or voxels do not fit 21 bits per axis");
        return VS_ERR_CAPACITY;
    }
    const int m = std::min(cap, counts[2]);
    if (m > 0) {
        VS_HIP(hipMemcpyAsync(out, d_out, (size_t)m * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
        VS_HIP(hipMemcpyAsync(src, d_src, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, s));
        VS_HIP(hipStreamSynchronize(s));
    }
    return VS_OK;
}

}  // extern "C"

// poisson_screen.hip — step 4s of the Poisson reconstruction (include/vslam_abi.h): the screened system
//   (A + lambda B^T B) chi = -div + lambda tau W
// by preconditioned conjugate gradients from step 4's chi.  B (n x R^3, step 2's trilinear weights) is never
// assembled: the points are a surface, n << R^3, and a 27-point variable stencil would cost 27 R^3 doubles.
//
//   k_sc_interp   s = B p: one point per lane in the splat's sorted order, so a wave's eight node reads fall in few
//                 lines; the eight terms added in offset order.  p = z + beta p_old is formed here by the expression
//                 k_sc_apply uses, so both see the same bits without p being stored first.
//   k_sc_apply    q = A p + lambda B^T s with p.q.  k_cg_apply's split: a workgroup owns a 32 x 8 column of nodes and
//                 marches kZChunk planes along z, the plane of p in LDS with a one-node halo, the lane's own column in
//                 registers, p = z + beta p_old folded into every load and stored to the other p buffer by its owner.
//                 A node with W != 0 then adds lambda sum w s over the points of its <= 8 adjacent cells, cells and
//                 points in k_ps_gather's order, w from the sorted fractions.  W == 0 (most nodes: one read) skips
//                 the eight cell ranges.  A crowded cell costs its lane a loop that is linear in the cell's points, as
//                 in k_ps_gather; nothing here balances that.
//   k_sc_update   x += alpha p, r -= alpha q with r.r, the iteration count and the stop flag.
//   preconditioner  z = A^-1 r by poisson_dst.hip's five sine-transform passes (solver = DIRECT), through q and the idle
//                 p buffer; then k_sc_rz: r.z and beta.  Without it (solver = CG) z is r and k_sc_update has beta.
//   start         k_sc_begin (lambda), k_sc_interp / k_sc_apply on chi0, k_sc_bnorm (|b|), k_sc_start
//                 (r = b - (A + lambda B^T B) chi0, r.r, the stop flag), the preconditioner.
// Every dot product is poisson_common.h's fixed-order sum; alpha, beta and the stop flag st->go live in the state
// block, and every kernel — the sine transforms too, which take &st->go as their "ok" — returns at its first
// instruction once the flag is down: max_iter iterations are enqueued without a host round trip.
// fp64 without contraction.  No MFMA outside the preconditioner: the operator is a 7-point stencil and a gather.
#include <hip/hip_runtime.h>

#include <cmath>

#include "poisson_common.h"

namespace vs {

namespace {

struct It : Sc {
    const double* p_in;  // the search direction of the iteration before (unread on the first)
    double* p_out;
};

// the search direction at node i; INIT: chi0 itself
template <bool INIT>
__device__ __forceinline__ double sc_p(const It& a, bool first, double beta, size_t i) {
    if (INIT) return a.x[i];
    return first ? a.z[i] : a.z[i] + beta * a.p_in[i];
}

// step 2's weight of the sorted point t at offset d = dx + 2 dy + 4 dz
__device__ __forceinline__ double sc_w(const It& a, int t, int d) {
    const double f0 = a.fs[t], f1 = a.fs[(size_t)a.n + t], f2 = a.fs[2 * (size_t)a.n + t];
    return (((d & 1) ? f0 : 1.0 - f0) * ((d & 2) ? f1 : 1.0 - f1)) * ((d & 4) ? f2 : 1.0 - f2);
}

__global__ void k_sc_begin(It a) {
    if (threadIdx.x != 0) return;
    PsState& st = *a.st;
    st.go = st.iters = st.converged = 0;
    st.alpha = st.beta = st.rz = st.rho = 0;
    const double dbar = st.cells > 0 ? (double)a.n / (double)st.cells : 1.0;
    st.lambda = st.ok ? a.point_weight / ((st.h * st.h) * dbar) : 0.0;
}

template <bool INIT>
__global__ __launch_bounds__(256) void k_sc_interp(It a) {
    const PsState& st = *a.st;
    if (INIT ? !st.ok : !st.go) return;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n) return;
    const bool first = st.iters == 0;
    const double beta = st.beta;
    const int R = a.R, c = a.skey[t], bi = c % R, bj = c / R % R, bk = c / (R * R);  // a base cell: <= R - 2 per axis
    double v = 0;
    for (int d = 0; d < 8; d++)
        v += sc_w(a, t, d) * sc_p<INIT>(a, first, beta, lin(bi + (d & 1), bj + ((d >> 1) & 1), bk + (d >> 2), R));
    a.sp[t] = v;
}

// (B^T s)[node (i, j, k)]: k_ps_gather's order
__device__ __forceinline__ double sc_gather(const It& a, int i, int j, int k) {
    const int R = a.R;
    double g = 0;
    for (int d = 0; d < 8; d++) {
        const int ci = i - (d & 1), cj = j - ((d >> 1) & 1), ck = k - (d >> 2);
        if (ci < 0 || cj < 0 || ck < 0 || ci > R - 2 || cj > R - 2 || ck > R - 2) continue;
        const size_t c = lin(ci, cj, ck, R);
        const int lo = a.starts[c], hi = a.starts[c + 1];  // c + 1 < R^3: the last node is no cell
        for (int t = lo; t < hi; t++) g += sc_w(a, t, d) * a.sp[t];
    }
    return g;
}

template <bool INIT>
__global__ __launch_bounds__(256) void k_sc_apply(It a) {
    __shared__ double s_p[kTY + 2][kTX + 2];
    PsState& st = *a.st;
    if (INIT ? !st.ok : !st.go) return;
    const int tid = threadIdx.x, tx = tid & (kTX - 1), ty = tid / kTX, R = a.R;
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY, z0 = blockIdx.z * kZChunk;
    const int x = x0 + tx, y = y0 + ty, z1 = min(z0 + kZChunk, R);
    const bool first = st.iters == 0, own = x < R && y < R;
    const double beta = st.beta, h2 = st.h * st.h, lambda = st.lambda;
    auto load = [&](int px, int py, int pz) {
        if (px < 0 || py < 0 || pz < 0 || px >= R || py >= R || pz >= R) return 0.0;
        return sc_p<INIT>(a, first, beta, lin(px, py, pz, R));
    };
    // this lane's node of the halo ring: the rows above and below the tile, then the columns left and right of it
    int hx = 0, hy = 0;
    if (tid < kTX) hx = tid + 1, hy = 0;
    else if (tid < 2 * kTX) hx = tid - kTX + 1, hy = kTY + 1;
    else if (tid < 2 * kTX + kTY) hx = 0, hy = tid - 2 * kTX + 1;
    else if (tid < kHalo) hx = kTX + 1, hy = tid - 2 * kTX - kTY + 1;
    double below = own ? load(x, y, z0 - 1) : 0.0, cur = own ? load(x, y, z0) : 0.0;
    double acc = 0;
    for (int z = z0; z < z1; z++) {
        const double above = own ? load(x, y, z + 1) : 0.0;
        s_p[ty + 1][tx + 1] = cur;
        if (tid < kHalo) s_p[hy][hx] = load(x0 + hx - 1, y0 + hy - 1, z);
        __syncthreads();
        if (own) {
            const double sum = ((((s_p[ty + 1][tx] + s_p[ty + 1][tx + 2]) + s_p[ty][tx + 1]) + s_p[ty + 2][tx + 1]) + below) + above;
            const size_t i = lin(x, y, z, R);
            double q = (6.0 * cur - sum) / h2;
            if (a.W[i] != 0.0) q = q + lambda * sc_gather(a, x, y, z);
            a.q[i] = q;
            if (!INIT) a.p_out[i] = cur;
            acc += cur * q;
        }
        __syncthreads();
        below = cur, cur = above;
    }
    if (INIT) return;
    double total;
    if (grid_sum(acc, a.part, &st.ticket, total) && tid == 0) st.alpha = st.rz / total;
}

// b at node i: -div + (lambda tau) W
__device__ __forceinline__ double sc_b(const It& a, const PsState& st, size_t i) {
    return -a.div[i] + (st.lambda * st.iso) * a.W[i];
}

__global__ __launch_bounds__(256) void k_sc_bnorm(It a) {
    PsState& st = *a.st;
    if (!st.ok) return;
    double acc = 0;
#pragma unroll
    for (int e = 0; e < kTile / 256; e++) {
        const size_t i = (size_t)blockIdx.x * kTile + e * 256 + threadIdx.x;
        if (i < a.nodes) {
            const double b = sc_b(a, st, i);
            acc += b * b;
        }
    }
    double total;
    if (grid_sum(acc, a.part, &st.ticket, total) && threadIdx.x == 0) st.rhs_norm = sqrt(total);
}

// r = b - q (q = (A + lambda B^T B) chi0) with r.r; r may be written over div
__global__ __launch_bounds__(256) void k_sc_start(It a) {
    PsState& st = *a.st;
    if (!st.ok) return;
    double acc = 0;
#pragma unroll
    for (int e = 0; e < kTile / 256; e++) {
        const size_t i = (size_t)blockIdx.x * kTile + e * 256 + threadIdx.x;
        if (i < a.nodes) {
            const double r = sc_b(a, st, i) - a.q[i];
            a.r[i] = r;
            acc += r * r;
        }
    }
    double total;
    if (grid_sum(acc, a.part, &st.ticket, total) && threadIdx.x == 0) {
        st.rho = total;
        if (!a.direct) st.rz = total;
        const bool small = !(sqrt(total) > a.tol * st.rhs_norm);
        st.converged = small;
        st.go = !small && a.max_iter > 0;
    }
}

__global__ __launch_bounds__(256) void k_sc_update(It a) {
    PsState& st = *a.st;
    if (!st.go) return;
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
        st.rho = total;
        if (!a.direct) st.beta = total / st.rz, st.rz = total;
        if (sqrt(total) <= a.tol * st.rhs_norm) st.converged = 1, st.go = 0;
        if (st.iters >= a.max_iter) st.go = 0;
    }
}

// r.z; from the second time on also beta = r.z / the r.z before
__global__ __launch_bounds__(256) void k_sc_rz(It a) {
    PsState& st = *a.st;
    if (!st.go) return;
    double acc = 0;
#pragma unroll
    for (int e = 0; e < kTile / 256; e++) {
        const size_t i = (size_t)blockIdx.x * kTile + e * 256 + threadIdx.x;
        if (i < a.nodes) acc += a.r[i] * a.z[i];
    }
    double total;
    if (grid_sum(acc, a.part, &st.ticket, total) && threadIdx.x == 0) {
        if (st.iters > 0) st.beta = total / st.rz;
        st.rz = total;
    }
}

#define SC_LAUNCH(name, kernel, grid, block, arg)                          \
    do {                                                                   \
        ProfScope ps_(ctx, name, s);                                       \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, arg);    \
    } while (0)

dim3 column_grid(int R) { return dim3((R + kTX - 1) / kTX, (R + kTY - 1) / kTY, (R + kZChunk - 1) / kZChunk); }
unsigned tiles(size_t nodes) { return (unsigned)((nodes + kTile - 1) / kTile); }

// z = A^-1 r through q and t1, then r.z
int precondition(vs_ctx* ctx, const It& g, double* t1, hipStream_t s) {
    PsState* st = g.st;
    DstState ds{&st->go, &st->h, nullptr, nullptr, nullptr, 1};
    VS_CHECK(poisson_dst_enqueue(ctx, g.r, g.z, g.q, t1, g.R, 0.0, &ds, nullptr, s));
    SC_LAUNCH("k_sc_rz", k_sc_rz, tiles(g.nodes), 256, g);
    return VS_OK;
}

}  // namespace

int screen_start(vs_ctx* ctx, const Sc& a, hipStream_t s) {
    It g{};
    static_cast<Sc&>(g) = a;
    SC_LAUNCH("k_sc_begin", k_sc_begin, 1, 64, g);
    SC_LAUNCH("k_sc_interp", k_sc_interp<true>, (a.n + 255) / 256, 256, g);
    SC_LAUNCH("k_sc_apply", k_sc_apply<true>, column_grid(a.R), 256, g);
    SC_LAUNCH("k_sc_bnorm", k_sc_bnorm, tiles(a.nodes), 256, g);
    SC_LAUNCH("k_sc_start", k_sc_start, tiles(a.nodes), 256, g);
    if (a.direct) VS_CHECK(precondition(ctx, g, a.p[0], s));
    VS_HIP(hipGetLastError());
    return VS_OK;
}

int screen_iterate(vs_ctx* ctx, const Sc& a, int from, int to, hipStream_t s) {
    It g{};
    static_cast<Sc&>(g) = a;
    for (int it = from; it < to; it++) {
        g.p_in = a.p[it & 1], g.p_out = a.p[(it + 1) & 1];
        SC_LAUNCH("k_sc_interp", k_sc_interp<false>, (a.n + 255) / 256, 256, g);
        SC_LAUNCH("k_sc_apply", k_sc_apply<false>, column_grid(a.R), 256, g);
        SC_LAUNCH("k_sc_update", k_sc_update, tiles(a.nodes), 256, g);
        if (a.direct) VS_CHECK(precondition(ctx, g, a.p[it & 1], s));  // p_in's buffer is idle until the next apply writes it
    }
    VS_HIP(hipGetLastError());
    return VS_OK;
}

}  // namespace vs

// poisson_common.h — what cloud_poisson.hip and poisson_screen.hip share: the state block on the device, the fixed-order
// sum over a grid of workgroups, the stencil tile's shape, and the screened solve's interface.
#pragma once

#include <hip/hip_runtime.h>

#include "block_reduce.h"
#include "cloud_common.h"

namespace vs {

constexpr int kTX = 32, kTY = 8, kZChunk = 32;  // the stencil kernels' column of nodes and its planes per workgroup
constexpr int kHalo = 2 * kTX + 2 * kTY;         // the plane's halo ring without its corners
constexpr int kTile = 4096;                      // entries per workgroup of the scan and of the update kernels
constexpr int kMaxTiles = 32 * 1024;             // 512^3 / kTile; k_scan_top holds 32 per lane
static_assert(kHalo <= 256 && kTX * kTY == 256, "one halo node per lane");

// the state block on the device
struct PsState {
    double o[3], h;                          // the grid
    double rho, alpha, beta, rhs_norm, iso;  // the solver's scalars
    int ok, done, converged, iters;
    unsigned ticket;
    // the screened solve (step 4s)
    int cells, go;       // base cells that hold a point; 1 while the screened loop runs
    double lambda, rz;   // point_weight / (h h dbar); r.z of the current iteration
};

__device__ __forceinline__ size_t lin(int i, int j, int k, int R) { return ((size_t)k * R + j) * R + i; }

// The sum of v over every lane of the grid: block_sum's tree over the workgroup's 256 lanes, then the workgroups'
// partials added by the workgroup that takes the last ticket.  True in that workgroup only, total in every lane.
__device__ __forceinline__ bool grid_sum(double v, double* part, unsigned* ticket, double& total) {
    __shared__ double s_red[4];
    __shared__ int s_last;
    const int nb = gridDim.x * gridDim.y * gridDim.z;
    const int bid = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    double in[1] = {v}, out[1];
    block_sum<1>(in, s_red, out);
    if (threadIdx.x == 0) {
        part[bid] = out[0];
        __threadfence();  // the partial is visible to the device before the ticket is
        s_last = atomicAdd(ticket, 1u) == (unsigned)nb - 1u;
    }
    __syncthreads();
    if (!s_last) return false;
    __threadfence();  // every partial was released before its ticket: none is read from a stale line
    double acc = 0;
    const volatile double* vp = part;
    for (int b = threadIdx.x; b < nb; b += 256) acc += vp[b];
    in[0] = acc;
    block_sum<1>(in, s_red, out);
    total = out[0];
    if (threadIdx.x == 0) *ticket = 0;  // the next launch starts counting again
    return true;
}

// The screened solve (poisson_screen.hip): (A + lambda B^T B) chi = -div + lambda tau W by preconditioned conjugate
// gradients from the chi of step 4, in x.  The points arrive in the splat's order: sorted position t holds the
// point of base cell skey[t] with fractions fs[3 t ..], and cell c's points are t in [starts[c], starts[c + 1]).
struct Sc {
    PsState* st;
    double *x, *r, *z, *q, *p[2];  // R^3 each; z == r without a preconditioner; q and the idle p buffer carry the sine transforms
    const double* W;               // step 2b's density
    const double* div;             // step 3's div (r may be the same array: k_sc_start reads a node's div, then writes its r)
    double *sp, *part;             // [n] (B p) per sorted point; the partial sums
    const double* fs;
    const int *skey, *starts;
    int n, R, max_iter, direct;    // direct: the preconditioner is step 4's sine-transform solve; else none
    size_t nodes;
    double tol, point_weight;
};
// x = chi0 and st->iso = tau are set: lambda, the first residual, its preconditioned form, and the stop flag
int screen_start(vs_ctx* ctx, const Sc& a, hipStream_t s);
// iterations [from, to); each launch returns at its first instruction once the loop has stopped
int screen_iterate(vs_ctx* ctx, const Sc& a, int from, int to, hipStream_t s);

}  // namespace vs

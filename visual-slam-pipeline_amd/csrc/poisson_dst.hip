// poisson_dst.hip — the direct solve of step 4 of the Poisson reconstruction (include/vslam_abi.h): the 7-point
// Dirichlet Laplacian on R^3 nodes is diagonal in the sine basis S[a][b] = sin(pi a b / (R + 1)), so
//   chi = (2 / (R + 1))^3 (S x S x S) [ (S x S x S)(-div) / lambda ]
// is six products of the dense R x R table with one axis of the [k][j][i] field: fp64 GEMMs on
// v_mfma_f64_16x16x4_f64 (D = A B + C, A 16 x 4, B 4 x 16; lane l holds A[l % 16][l / 16], B[l / 16][l % 16] and
// D[4 r + l / 16][l % 16] in register r).  No transpose pass, no BLAS.
//
//   k_dst_axis<NT, SWAP, MODE>   out[m][n] = sum_k S[m][k] x[k][n] for one axis.  The K (= M) index and the N index
//     walk the field with strides (sk, sn): (1, R) along i with N = the R^2 rows, (R, 1) along j inside each of the R
//     z-planes (the batch), (R^2, 1) along k with N = the R^2 columns.  A workgroup (4 waves) owns 16 values of n and
//     every m: the whole output slab sits in accumulators (wave w owns the 16-row tiles w, w + 4, ...: NT = 1, 2, 4, 8
//     tiles per wave for R <= 64, 128, 256, 512), so a field value comes from HBM once and goes back once.  K is
//     walked in chunks of 8: the chunk of S (8 x Rp, read as rows of the symmetric table: coalesced) and of the
//     field (8 x 16) go through LDS; the next chunk's global loads are in flight in registers while the MFMAs of this
//     one run.  S is zero-padded to Rp = the next multiple of 16 on both axes, so the K loop has no bounds branch;
//     field loads past R or N give 0 and stores there are dropped.  Along i the operands are swapped (the MFMA then
//     forms the transposed tile), so that 16 consecutive lanes still store 16 consecutive doubles.
//     MODE 1: the result is multiplied by -(2 / (R + 1))^3 / lambda before the store.  MODE 2 (Rp <= kFusedMaxRp):
//     the z pair in one kernel — the scaled slab goes to LDS (Rp x 16 fp64, 32 KB at R = 256) and is the B operand
//     of a second product with S, so the solve is five passes: i, j, z pair, j, i.  Above kFusedMaxRp = 256 the slab
//     and the S chunk together pass 64 KB of LDS, and the z pair is two passes (MODE 1, then MODE 0).
//   k_dst_residual / k_dst_report   |A chi + div|_2 / |div|_2: block_sum's tree per workgroup of 4,096 nodes, the
//     workgroups' partials added by one workgroup (lane t takes t, t + 256, ...; the same tree).
// Every sum has a fixed order: K index k always goes to MFMA step k / 4 of its chunk and lane group k % 4, chunks in
// ascending order; chi is the same bits from run to run.  Compiled without contraction.  Every kernel returns at its
// first instruction when the state block says that the cloud has no extent.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "block_reduce.h"
#include "cloud_common.h"

namespace vs {

namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int kKC = 8;            // K per LDS chunk: two MFMA steps
constexpr int kTN = 16;           // values of n per workgroup: one MFMA tile
constexpr int kFusedMaxRp = 256;  // the z pair is one kernel up to here
constexpr int kResTile = 4096;    // nodes per workgroup of the residual pass
constexpr int kResMaxBlocks = VS_POISSON_MAX_RES * VS_POISSON_MAX_RES / kResTile * VS_POISSON_MAX_RES;

struct Dst {
    const double* x;
    double* y;
    const double *tab, *ev;  // S [Rp][Rp] and e [Rp], zero padded
    const int* ok;           // the state block's flag (null: a field given by the caller)
    const double* d_h;       // the state block's h (null: h below)
    double h, c3;            // c3 = (2 / (R + 1))^3
    int R, Rp, N;
    long long sk, sn, sb;    // strides of the K / M index, the N index and the batch
};

// -(2 / (R + 1))^3 t / lambda at transform index m along z and column c = j R + i
__device__ __forceinline__ double dst_scale(const Dst& a, double t, int m, long long c, double h) {
    const int j = (int)(c / a.R), i = (int)(c % a.R);
    const double lam = (2.0 / (h * h)) * ((a.ev[m] + a.ev[j]) + a.ev[i]);
    return -(t / lam) * a.c3;
}

template <int NT, bool SWAP, int MODE>
__global__ __launch_bounds__(256) void k_dst_axis(Dst a) {
    constexpr int MR = 64 * NT, LD = MR + 16;  // + 16: the rows of two lane groups fall into different banks
    __shared__ double s_s[kKC][LD];
    __shared__ double s_b[kKC][kTN];
    __shared__ double s_y[MODE == 2 ? MR : 1][kTN];
    if (a.ok && !*a.ok) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, lr = lane & 15, lq = lane >> 4;
    const int R = a.R, Rp = a.Rp;
    const double h = a.d_h ? *a.d_h : a.h;
    const long long n0 = (long long)blockIdx.x * kTN;
    const double* x = a.x + (long long)blockIdx.y * a.sb;
    double* y = a.y + (long long)blockIdx.y * a.sb;
    // this thread's element of the field chunk: consecutive threads along the axis that is contiguous in memory
    const int bk = SWAP ? tid & 7 : tid >> 4, bn = SWAP ? (tid >> 3) & 15 : tid & 15;
    const bool bload = tid < kKC * kTN && n0 + bn < a.N;
    const double* bp = x + (n0 + bn) * a.sn;
    v4d acc[NT];
    double ps[2 * NT], pb = 0.0;
    auto fetch = [&](int k0, bool field) {
#pragma unroll
        for (int u = 0; u < 2 * NT; u++) {
            const int e = tid + 256 * u, kk = e / MR, m = e % MR;
            ps[u] = m < Rp ? a.tab[(size_t)(k0 + kk) * Rp + m] : 0.0;
        }
        if (field) pb = bload && k0 + bk < R ? bp[(long long)(k0 + bk) * a.sk] : 0.0;
    };
    // acc = S (the field's slab, or s_y): chunks ascending, two MFMA steps each
    auto product = [&](bool field) {
#pragma unroll
        for (int u = 0; u < NT; u++) acc[u] = v4d{0.0, 0.0, 0.0, 0.0};
        fetch(0, field);
        for (int k0 = 0; k0 < Rp; k0 += kKC) {
            __syncthreads();  // the previous chunk has been read
#pragma unroll
            for (int u = 0; u < 2 * NT; u++) {
                const int e = tid + 256 * u;
                s_s[e / MR][e % MR] = ps[u];
            }
            if (field && tid < kKC * kTN) s_b[bk][bn] = pb;
            __syncthreads();
            if (k0 + kKC < Rp) fetch(k0 + kKC, field);
#pragma unroll
            for (int st = 0; st < kKC / 4; st++) {
                const double b = field ? s_b[4 * st + lq][lr] : s_y[MODE == 2 ? k0 + 4 * st + lq : 0][lr];
#pragma unroll
                for (int u = 0; u < NT; u++) {
                    const int t = wv + 4 * u;
                    if (16 * t < Rp) {  // the same for the whole wave
                        const double s = s_s[4 * st + lq][16 * t + lr];
                        acc[u] = SWAP ? __builtin_amdgcn_mfma_f64_16x16x4f64(b, s, acc[u], 0, 0, 0)
                                      : __builtin_amdgcn_mfma_f64_16x16x4f64(s, b, acc[u], 0, 0, 0);
                    }
                }
            }
        }
    };
    product(true);
    if (MODE == 2) {
        const long long c = n0 + lr;
#pragma unroll
        for (int u = 0; u < NT; u++) {
            const int t = wv + 4 * u;
            if (16 * t < Rp)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int m = 16 * t + 4 * r + lq;
                    s_y[m][lr] = m < R && c < a.N ? dst_scale(a, acc[u][r], m, c, h) : 0.0;
                }
        }
        product(false);  // its first barrier orders s_y's stores before its reads
    }
#pragma unroll
    for (int u = 0; u < NT; u++) {
        const int t = wv + 4 * u;
        if (16 * t >= Rp) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = SWAP ? 16 * t + lr : 16 * t + 4 * r + lq;
            const long long n = n0 + (SWAP ? 4 * r + lq : lr);
            if (m < R && n < a.N) y[m * a.sk + n * a.sn] = MODE == 1 ? dst_scale(a, acc[u][r], m, n, h) : acc[u][r];
        }
    }
}

// ---- the residual ------------------------------------------------------------------------------------------------
struct DstRes {
    const double *chi, *rhs;
    double* part;  // [blocks][2]
    const int* ok;
    const double* d_h;
    double h;
    int R, blocks;
    size_t nodes;
    double *rho, *rhs_norm;  // the state block's (nullable)
    int* converged;
    double* info;  // {0, relative residual} (nullable)
};

__global__ __launch_bounds__(256) void k_dst_residual(DstRes a) {
    __shared__ double s_red[8];
    if (a.ok && !*a.ok) return;
    const double h = a.d_h ? *a.d_h : a.h, h2 = h * h;
    const int R = a.R;
    const size_t sy = R, sz = (size_t)R * R;
    double acc[2] = {0.0, 0.0}, out[2];
#pragma unroll
    for (int e = 0; e < kResTile / 256; e++) {
        const size_t nd = (size_t)blockIdx.x * kResTile + e * 256 + threadIdx.x;
        if (nd < a.nodes) {
            const int i = (int)(nd % R), j = (int)(nd / R % R), k = (int)(nd / sz);
            const double* c = a.chi + nd;
            const double xm = i > 0 ? c[-1] : 0.0, xp = i + 1 < R ? c[1] : 0.0;
            const double ym = j > 0 ? *(c - sy) : 0.0, yp = j + 1 < R ? c[sy] : 0.0;
            const double zm = k > 0 ? *(c - sz) : 0.0, zp = k + 1 < R ? c[sz] : 0.0;
            const double sum = ((((xm + xp) + ym) + yp) + zm) + zp, b = a.rhs[nd];
            const double r = (6.0 * c[0] - sum) / h2 + b;
            acc[0] += r * r, acc[1] += b * b;
        }
    }
    block_sum<2>(acc, s_red, out);
    if (threadIdx.x == 0) a.part[2 * blockIdx.x] = out[0], a.part[2 * blockIdx.x + 1] = out[1];
}

__global__ __launch_bounds__(256) void k_dst_report(DstRes a) {
    __shared__ double s_red[8];
    if (a.ok && !*a.ok) return;
    double acc[2] = {0.0, 0.0}, out[2];
    for (int b = threadIdx.x; b < a.blocks; b += 256) acc[0] += a.part[2 * b], acc[1] += a.part[2 * b + 1];
    block_sum<2>(acc, s_red, out);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(out[1]);
    if (a.rho) *a.rho = out[0], *a.rhs_norm = norm, *a.converged = 1;
    if (a.info) a.info[0] = 0.0, a.info[1] = norm > 0 ? sqrt(out[0]) / norm : 0.0;
}

#define DST_LAUNCH(name, kernel, grid, arg)                               \
    do {                                                                  \
        ProfScope ps_(ctx, name, s);                                      \
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, arg);           \
    } while (0)

// the instantiation for a.Rp; MODE 2 only up to kFusedMaxRp
template <bool SWAP, int MODE>
void launch_axis(vs_ctx* ctx, const char* name, const Dst& a, dim3 grid, hipStream_t s) {
    if (a.Rp <= 64) DST_LAUNCH(name, (k_dst_axis<1, SWAP, MODE>), grid, a);
    else if (a.Rp <= 128) DST_LAUNCH(name, (k_dst_axis<2, SWAP, MODE>), grid, a);
    else if (a.Rp <= 256) DST_LAUNCH(name, (k_dst_axis<4, SWAP, MODE>), grid, a);
    else if constexpr (MODE != 2) DST_LAUNCH(name, (k_dst_axis<8, SWAP, MODE>), grid, a);
}

// S and e for R, built once per R in extended precision and kept in the context.  a b is reduced modulo 2 (R + 1) in
// integers and folded into the first quadrant, so that S[a][b] and S[b][a] are the same sine of the same argument.
int dst_table(vs_ctx* ctx, int R, hipStream_t s, const double** tab, const double** ev, double** part) {
    const int Rp = (R + 15) / 16 * 16, M = R + 1;
    const size_t count = (size_t)Rp * Rp + Rp;
    const bool fresh = ctx->poisson_dst_R != R;
    if (fresh) VS_HIP(hipStreamSynchronize(s));  // a solve with the previous table may still be running
    ctx->poisson_dst_R = 0;
    VS_CHECK(carve_buf(ctx->poisson_dst, [&](Carver& p) {
        *part = p.take<double>(2 * (size_t)kResMaxBlocks);
        *tab = p.take<double>(count);
    }));
    *ev = *tab + (size_t)Rp * Rp;
    if (fresh) {
        const long double pi = 3.14159265358979323846264338327950288L;
        std::vector<double> quarter(M / 2 + 1), host(count, 0.0);
        for (int p = 0; p <= M / 2; p++) quarter[p] = (double)sinl(pi * (long double)p / (long double)M);
        for (int r = 1; r <= R; r++) {
            for (int c = 1; c <= R; c++) {
                int p = (int)((long long)r * c % (2 * M));
                const bool neg = p >= M;
                if (neg) p -= M;
                if (2 * p > M) p = M - p;
                host[(size_t)(r - 1) * Rp + (c - 1)] = neg ? -quarter[p] : quarter[p];
            }
            const long double sn = sinl(pi * (long double)r / (long double)(2 * M));
            host[(size_t)Rp * Rp + (r - 1)] = (double)(2.0L * sn * sn);
        }
        VS_HIP(hipMemcpy(const_cast<double*>(*tab), host.data(), count * sizeof(double), hipMemcpyHostToDevice));
    }
    ctx->poisson_dst_R = R;
    return VS_OK;
}

int solve_check(const char* who, int R, double h) {
    VS_ARG(R >= 2 && h > 0 && std::isfinite(h), std::string(who) + ": resolution below 2, or h not positive and finite");
    if (R > VS_POISSON_MAX_RES) {
        set_error(std::string(who) + ": resolution above VS_POISSON_MAX_RES");
        return VS_ERR_CAPACITY;
    }
    return VS_OK;
}

int solve_standalone(vs_ctx* ctx, const double* d_rhs, int R, double h, double* d_chi, double* d_info, hipStream_t s) {
    const size_t nodes = (size_t)R * R * R;
    double* t[3];
    VS_CHECK(carve_buf(ctx->cloud_poisson, [&](Carver& p) {
        for (double*& v : t) v = p.take<double>(nodes);
    }));
    if (d_chi == d_rhs) {  // the residual reads the right-hand side after chi has replaced it
        VS_HIP(hipMemcpyAsync(t[2], d_rhs, nodes * sizeof(double), hipMemcpyDeviceToDevice, s));
        d_rhs = t[2];
    }
    return poisson_dst_enqueue(ctx, d_rhs, d_chi, t[0], t[1], R, h, nullptr, d_info, s);
}

}  // namespace

int poisson_dst_enqueue(vs_ctx* ctx, const double* d_div, double* d_chi, double* t0, double* t1, int R, double h,
                        const DstState* st, double* d_info, hipStream_t s) {
    Dst a{};
    double* part;
    VS_CHECK(dst_table(ctx, R, s, &a.tab, &a.ev, &part));
    a.R = R, a.Rp = (R + 15) / 16 * 16, a.h = h;
    a.c3 = (2.0 / (double)(R + 1)) * (2.0 / (double)(R + 1)) * (2.0 / (double)(R + 1));
    if (st) a.ok = st->ok, a.d_h = st->h;
    if (st && st->precond) a.c3 = -a.c3;
    const long long R1 = R, R2 = R1 * R1;
    const unsigned cols = (unsigned)((R2 + kTN - 1) / kTN), rowt = (unsigned)((R + kTN - 1) / kTN);
    auto along_i = [&](const double* x, double* y) {
        a.x = x, a.y = y, a.sk = 1, a.sn = R1, a.sb = 0, a.N = (int)R2;
        launch_axis<true, 0>(ctx, "k_dst_i", a, dim3(cols), s);
    };
    auto along_j = [&](const double* x, double* y) {
        a.x = x, a.y = y, a.sk = R1, a.sn = 1, a.sb = R2, a.N = R;
        launch_axis<false, 0>(ctx, "k_dst_j", a, dim3(rowt, R), s);
    };
    along_i(d_div, t0);
    along_j(t0, t1);
    a.x = t1, a.y = t0, a.sk = R2, a.sn = 1, a.sb = 0, a.N = (int)R2;
    if (a.Rp <= kFusedMaxRp) {
        launch_axis<false, 2>(ctx, "k_dst_zz", a, dim3(cols), s);
    } else {  // the slab does not fit beside the S chunk: two passes, the first one scaled
        DST_LAUNCH("k_dst_z", (k_dst_axis<8, false, 1>), dim3(cols), a);
        a.x = t0, a.y = t1;
        DST_LAUNCH("k_dst_z", (k_dst_axis<8, false, 0>), dim3(cols), a);
        std::swap(t0, t1);
    }
    along_j(t0, t1);
    along_i(t1, d_chi);
    if (st && st->precond) {
        VS_HIP(hipGetLastError());
        return VS_OK;
    }
    DstRes r{};
    r.chi = d_chi, r.rhs = d_div, r.part = part, r.ok = a.ok, r.d_h = a.d_h, r.h = h, r.R = R;
    r.nodes = (size_t)R2 * R, r.blocks = (int)((r.nodes + kResTile - 1) / kResTile), r.info = d_info;
    if (st) r.rho = st->rho, r.rhs_norm = st->rhs_norm, r.converged = st->converged;
    DST_LAUNCH("k_dst_residual", k_dst_residual, dim3(r.blocks), r);
    DST_LAUNCH("k_dst_report", k_dst_report, dim3(1), r);
    VS_HIP(hipGetLastError());
    return VS_OK;
}

}  // namespace vs

using namespace vs;

extern "C" {

int vs_grid_poisson_solve_dev(vs_ctx* ctx, const double* d_rhs, int resolution, double h, double* d_chi, double* d_info,
                              void* stream) {
    VS_ARG(ctx && d_rhs && d_chi && d_info, "vs_grid_poisson_solve_dev: null argument");
    VS_CHECK(solve_check("vs_grid_poisson_solve_dev", resolution, h));
    VS_HIP(hipSetDevice(ctx->device));
    return solve_standalone(ctx, d_rhs, resolution, h, d_chi, d_info, stream ? (hipStream_t)stream : ctx->stream);
}

int vs_grid_poisson_solve(vs_ctx* ctx, const double* rhs, int resolution, double h, double* chi, double info[2]) {
    VS_ARG(ctx && rhs && chi && info, "vs_grid_poisson_solve: null argument");
    VS_CHECK(solve_check("vs_grid_poisson_solve", resolution, h));
    VS_HIP(hipSetDevice(ctx->device));
    const hipStream_t s = ctx->stream;
    const size_t nodes = (size_t)resolution * resolution * resolution;
    double *d_rhs, *d_chi, *d_info;
    VS_CHECK(carve_buf(ctx->h_aux0, [&](Carver& p) {
        d_rhs = p.take<double>(nodes);
        d_chi = chi == rhs ? d_rhs : p.take<double>(nodes);  // in place on the host: in place on the device
        d_info = p.take<double>(2);
    }));
    VS_HIP(hipMemcpyAsync(d_rhs, rhs, nodes * sizeof(double), hipMemcpyHostToDevice, s));
    VS_CHECK(solve_standalone(ctx, d_rhs, resolution, h, d_chi, d_info, s));
    VS_HIP(hipMemcpyAsync(chi, d_chi, nodes * sizeof(double), hipMemcpyDeviceToHost, s));
    VS_HIP(hipMemcpyAsync(info, d_info, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    VS_HIP(hipStreamSynchronize(s));
    return VS_OK;
}

}  // extern "C"

// The float64 path (gfx950): the dense layers and node_norm of a float64 module in float64 arithmetic.
//
// The reference is dtype-generic and its own tests run in float64 (tests/test_equivariance.py:6, 1e-6 bars at default-scale
// weights): a module converted with .double() computes everything in float64.  The fast kernels carry ~22 significant bits per
// product, so a float64 module takes these kernels instead (egnn_pytorch_amd/layer.py::_forward_exact with dtype float64), together
// with the float64 instantiations of the plain edge pass (edge_exact.hip: egnn_edge_exact_f64) and of the neighbour selection
// (knn_rows.hip: egnn_knn_select_f64):
//   egnn_linear_f64      :178-179, :196-201, :287, :336-337   C = act(A W^T + bias) (+ residual) on v_mfma_f64_16x16x4_f64
//   egnn_node_prep_f64   :335-336                  [LayerNorm(feats) | m_i]
// Correct and deterministic first, fast second (the float64 matrix rate of this part is 1/32 of its fp16 rate): never what
// bench.py times.
#include "egnn_common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ dense layer
constexpr int DM = 64, DN = 64, DK = 16;       // workgroup tile; 4 waves as 2 x 2, each 32 x 32 = 2 x 2 MFMA tiles of 16 x 16
constexpr int DLD = DK + 2;                    // padded LDS row, doubles (144 B)
constexpr int D_THREADS = 256;

__device__ __forceinline__ double silu64(double x) { return x / (1.0 + exp(-x)); }

template <int ACT, bool HAS_RES>
__global__ __launch_bounds__(D_THREADS) void linear_f64_kernel(
    const double* __restrict__ A, int64_t lda, const double* __restrict__ W, int64_t ldw, const double* __restrict__ bias,
    const double* __restrict__ R, int64_t ldr, double* __restrict__ C, int64_t ldc, int64_t M, int N, int K, int ntn)
{
    __shared__ __attribute__((aligned(16))) double lds[2 * 2 * DM * DLD];          // [buf][A | W][64][18]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t m0 = (int64_t)(blockIdx.x / ntn) * DM;
    const int n0 = (int)(blockIdx.x % ntn) * DN;
    // staging: thread t moves doubles [row t / 4][4 (t % 4) .. + 3] of both tiles
    const int srow = tid >> 2, sk = (tid & 3) * 4;
    double ra[4], rw[4];
    auto gload = [&](int kt) {
        const int k0 = kt * DK + sk;
        const int64_t ar = m0 + srow;
        const int64_t wr = (int64_t)n0 + srow;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ra[u] = (ar < M && k0 + u < K) ? A[ar * lda + k0 + u] : 0.0;
            rw[u] = (wr < N && k0 + u < K) ? W[wr * ldw + k0 + u] : 0.0;
        }
    };
    auto lstore = [&](int buf) {
        double* as = lds + buf * (2 * DM * DLD) + srow * DLD + sk;
        double* ws = as + DM * DLD;
#pragma unroll
        for (int u = 0; u < 4; ++u) { as[u] = ra[u]; ws[u] = rw[u]; }
    };
    f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int nk = (K + DK - 1) / DK;
    gload(0);
    lstore(0);
    __syncthreads();
    const int fr = lane & 15, fk = lane >> 4;       // fragment row / k slot of this lane (A: [m = fr][k = fk], B: [k = fk][n = fr])
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) gload(kt + 1);
        const double* as = lds + buf * (2 * DM * DLD) + (wm * 32 + fr) * DLD + fk;
        const double* ws = lds + buf * (2 * DM * DLD) + DM * DLD + (wn * 32 + fr) * DLD + fk;
#pragma unroll
        for (int s = 0; s < DK / 4; ++s) {
            const double a0 = as[4 * s], a1 = as[16 * DLD + 4 * s];
            const double b0 = ws[4 * s], b1 = ws[16 * DLD + 4 * s];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (kt + 1 < nk) lstore(buf ^ 1);
        __syncthreads();
    }
    // D of v_mfma_f64_16x16x4_f64: lane (g = lane / 16, c = lane % 16), register r: row 4 r + g, column c (not the fp32 shape's 4 g + r)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int gn = n0 + wn * 32 + j * 16 + fr;
            if (gn >= N) continue;
            const double bv = bias ? bias[gn] : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t gm = m0 + wm * 32 + i * 16 + 4 * r + fk;
                if (gm >= M) continue;
                double x = acc[i][j][r] + bv;
                if (ACT == 1) x = silu64(x);
                if (HAS_RES) x += R[gm * ldr + gn];
                C[gm * ldc + gn] = x;
            }
        }
}

// ------------------------------------------------------------------------------------------------ node_norm + concat
// butterfly sum of a double over the wave: the two 32-bit halves through ds_bpermute (every lane ends with the same bits)
__device__ __forceinline__ double wave_sum64(double v)
{
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t u = (uint64_t)__double_as_longlong(v);
        const int src = (lane ^ o) << 2;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)u);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)(uint32_t)(u >> 32));
        v += __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
    }
    return v;
}

__global__ __launch_bounds__(256) void node_prep_f64_kernel(const double* __restrict__ feats, const double* __restrict__ m_i,
                                                            const double* __restrict__ gamma, const double* __restrict__ beta,
                                                            double eps, double* __restrict__ out, int64_t rows, int dim, int m_dim)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int od = dim + m_dim;
    for (int64_t r = wave0; r < rows; r += nwaves) {
        const double* x = feats + r * dim;
        double* y = out + r * od;
        if (gamma) {                                   // two-pass statistics, as torch's LayerNorm
            double s = 0.0;
            for (int c = lane; c < dim; c += 64) s += x[c];
            const double mean = wave_sum64(s) / (double)dim;
            double v = 0.0;
            for (int c = lane; c < dim; c += 64) { const double d = x[c] - mean; v += d * d; }
            const double var = wave_sum64(v) / (double)dim;
            const double rstd = 1.0 / sqrt(var + eps);
            for (int c = lane; c < dim; c += 64) y[c] = (x[c] - mean) * rstd * gamma[c] + beta[c];
        } else {
            for (int c = lane; c < dim; c += 64) y[c] = x[c];
        }
        for (int c = lane; c < m_dim; c += 64) y[dim + c] = m_i ? m_i[r * m_dim + c] : 0.0;
    }
}

}  // namespace

extern "C" int egnn_linear_f64(const double* A, int64_t lda, const double* W, int64_t ldw, const double* bias, const double* residual,
                               int64_t ldr, double* C, int64_t ldc, int64_t M, int N, int K, int act, void* stream)
{
    if (!A || !W || !C) return EGNN_E_NULLPTR;
    if (M <= 0 || N <= 0 || K <= 0 || lda < K || ldw < K || ldc < N) return EGNN_E_SHAPE;
    if (residual && ldr < N) return EGNN_E_SHAPE;
    if (act != 0 && act != 1) return EGNN_E_UNSUPPORTED;
    const int64_t ntm = (M + DM - 1) / DM, ntn = (N + DN - 1) / DN;
    if (ntm * ntn > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(ntm * ntn)), block(D_THREADS);
    if (act == 0) {
        if (residual) hipLaunchKernelGGL((linear_f64_kernel<0, true>), grid, block, 0, s, A, lda, W, ldw, bias, residual, ldr, C, ldc, M, N, K, (int)ntn);
        else hipLaunchKernelGGL((linear_f64_kernel<0, false>), grid, block, 0, s, A, lda, W, ldw, bias, residual, ldr, C, ldc, M, N, K, (int)ntn);
    } else {
        if (residual) hipLaunchKernelGGL((linear_f64_kernel<1, true>), grid, block, 0, s, A, lda, W, ldw, bias, residual, ldr, C, ldc, M, N, K, (int)ntn);
        else hipLaunchKernelGGL((linear_f64_kernel<1, false>), grid, block, 0, s, A, lda, W, ldw, bias, residual, ldr, C, ldc, M, N, K, (int)ntn);
    }
    return egnn_launch_status();
}

extern "C" int egnn_node_prep_f64(const double* feats, const double* m_i, const double* gamma, const double* beta, double eps,
                                  double* out, int64_t rows, int dim, int m_dim, void* stream)
{
    if (!feats || !out) return EGNN_E_NULLPTR;
    if ((gamma == nullptr) != (beta == nullptr)) return EGNN_E_NULLPTR;
    if (rows <= 0 || dim <= 0 || m_dim < 0) return EGNN_E_SHAPE;
    int64_t blocks = (rows + 3) / 4;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(node_prep_f64_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), feats, m_i, gamma, beta,
                       eps, out, rows, dim, m_dim);
    return egnn_launch_status();
}

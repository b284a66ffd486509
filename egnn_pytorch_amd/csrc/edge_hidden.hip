// The E x H block of the layer as a twice-differentiable op: egnn_pytorch_amd/autograd.py::EdgeHidden / EdgeHiddenGrad, whose closed
// forms (`edge_hidden_backward_spec`, `edge_hidden_double_backward_spec`) are the specification of these kernels.  Per edge e = (b, i, k)
// with neighbour j and d the dropout factor (the forward's hash mask / keep, or 1):
//     x = d (P_i[i] + P_j[j] + W_s s_e);  sig = sigmoid(x);  a = x sig;  a1 = SiLU'(x);  a2 = SiLU''(x);  u_e = W2 a + b2
//   forward:       u (E, m)
//   first order:   g_a = W2^T gU_e;  dz = d a1 g_a  ->  A_T, DZ_T (H, E) and ds_e = W_s^T dz (E, S)
//   second order:  v = Pbar_i[i] + Pbar_j[j] + Wbar_s s_e + W_s sbar_e;  r = d (d a2 g_a v + a1 Wbar2^T gU_e)
//                  ->  d/d gU_e = W2 (d a1 v) + Wbar2 a + bbar2 (E, m),  d/d s_e = W_s^T r + Wbar_s^T dz (E, S),
//                      DAV_T = d a1 v, R_T = r, DZ_T = dz (H, E)
// The sums over all edges (d/d W_s, d/d W2) are C = X W^T products of egnn_linear_f32 / _f64 over the transposed tables, the per-node
// sums (d/d P_i, d/d P_j) egnn_edge_exact_node_sums_* over them: fixed orders, no float atomics.  One thread per edge, in the shape of
// csrc/edge_exact_bwd.hip: the weights are read wave-uniformly (every thread of a wave walks the same hidden unit), the edge's scalars
// and their gradients sit in columns of LDS.  The host cuts the batch into chunks of graphs that keep the (H, E) tables within a budget.
// Correct first: plain arithmetic in the parameters' precision, no split-f16 products.
#include "egnn_common.h"

namespace {

constexpr int EH_THREADS = 256;

__device__ __forceinline__ float eh_exp(float x) { return expf(x); }
__device__ __forceinline__ double eh_exp(double x) { return exp(x); }
__device__ __forceinline__ float eh_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double eh_fma(double a, double b, double c) { return fma(a, b, c); }

template <typename T>
struct EhArgs {
    int B, N, K, m_dim, H, S;
    const int32_t* idx;
    const T *Pi, *Pj, *s, *Ws, *W2, *b2, *gU;
    const T *cPi, *cPj, *cs, *cWs, *cW2, *cb2;
    T *u, *A_T, *DZ_T, *g_s, *g_gU, *DAV_T, *R_T;
    uint32_t drop_thr, drop_seed;
    float drop_inv_keep;
    int64_t drop_eid0;
};

// (edge q) -> the rows of its source node i and its neighbour j in the (B N, H) tables
struct EhEdge {
    int64_t src, dst;
};

template <typename T>
__device__ __forceinline__ EhEdge eh_edge(const EhArgs<T>& p, int64_t q)
{
    const int64_t node = q / p.K;
    const int k = (int)(q - node * p.K);
    const int64_t bN = node / p.N * p.N;
    const int j = p.idx ? p.idx[q] : k;
    return EhEdge{node, bN + j};
}

// z for hidden unit h and the dropout factor d (the forward's mask of this edge's row, column h)
template <typename T>
__device__ __forceinline__ T eh_pre(const EhArgs<T>& p, const T* pi, const T* pj, const T* sc, int h, uint32_t ekey, T& dk)
{
    T x = pi[h] + pj[h];
    const T* ws = p.Ws + (size_t)h * p.S;
    for (int s = 0; s < p.S; ++s) x = eh_fma(sc[s * EH_THREADS], ws[s], x);
    dk = (T)1;
    if (p.drop_thr) dk = egnn_drop_hash(ekey, (uint32_t)h) >= p.drop_thr ? (T)p.drop_inv_keep : (T)0;
    return x * dk;
}

// MB: message channels kept in registers (16 / 32 / 64); 0: any m_dim, accumulated in the output row itself
template <typename T, int MB>
__global__ __launch_bounds__(EH_THREADS) void edge_hidden_fwd_kernel(const EhArgs<T> p)
{
    const int64_t E = (int64_t)p.B * p.N * p.K;
    const int64_t q = (int64_t)blockIdx.x * EH_THREADS + threadIdx.x;
    if (q >= E) return;
    const int m = p.m_dim, H = p.H, S = p.S;
    const EhEdge ed = eh_edge(p, q);
    extern __shared__ __attribute__((aligned(16))) char eh_raw[];
    T* const sc = reinterpret_cast<T*>(eh_raw) + threadIdx.x;
    for (int s = 0; s < S; ++s) sc[s * EH_THREADS] = p.s[(size_t)q * S + s];
    const T* pi = p.Pi + (size_t)ed.src * H;
    const T* pj = p.Pj + (size_t)ed.dst * H;
    T* urow = p.u + (size_t)q * m;
    constexpr int MR = MB > 0 ? MB : 1;
    T acc[MR];
    if (MB > 0) {
#pragma unroll
        for (int c = 0; c < MR; ++c) acc[c] = c < m ? p.b2[c] : (T)0;
    } else {
        for (int c = 0; c < m; ++c) urow[c] = p.b2[c];
    }
    const uint32_t ekey = p.drop_thr ? egnn_drop_base(p.drop_seed, EGNN_DROP_SITE_EDGE, (uint32_t)(q + p.drop_eid0)) : 0u;
    for (int h = 0; h < H; ++h) {
        T dk;
        const T x = eh_pre(p, pi, pj, sc, h, ekey, dk);
        const T a = x / ((T)1 + eh_exp(-x));
        const T* w2 = p.W2 + h;
        if (MB > 0) {
#pragma unroll
            for (int c = 0; c < MR; ++c)
                if (c < m) acc[c] = eh_fma(w2[(size_t)c * H], a, acc[c]);
        } else {
            for (int c = 0; c < m; ++c) urow[c] = eh_fma(w2[(size_t)c * H], a, urow[c]);
        }
    }
    if (MB > 0) {
#pragma unroll
        for (int c = 0; c < MR; ++c)
            if (c < m) urow[c] = acc[c];
    }
}

// first order: A_T, DZ_T (H, E) and ds (E, S)
template <typename T, int MB>
__global__ __launch_bounds__(EH_THREADS) void edge_hidden_bwd_kernel(const EhArgs<T> p)
{
    const int64_t E = (int64_t)p.B * p.N * p.K;
    const int64_t q = (int64_t)blockIdx.x * EH_THREADS + threadIdx.x;
    if (q >= E) return;
    const int m = p.m_dim, H = p.H, S = p.S;
    const EhEdge ed = eh_edge(p, q);
    extern __shared__ __attribute__((aligned(16))) char eh_raw[];
    T* const sc = reinterpret_cast<T*>(eh_raw) + threadIdx.x;
    T* const gs = sc + (size_t)S * EH_THREADS;
    for (int s = 0; s < S; ++s) {
        sc[s * EH_THREADS] = p.s[(size_t)q * S + s];
        gs[s * EH_THREADS] = (T)0;
    }
    const T* pi = p.Pi + (size_t)ed.src * H;
    const T* pj = p.Pj + (size_t)ed.dst * H;
    const T* gu = p.gU + (size_t)q * m;
    constexpr int MR = MB > 0 ? MB : 1;
    T g[MR];
    if (MB > 0) {
#pragma unroll
        for (int c = 0; c < MR; ++c) g[c] = c < m ? gu[c] : (T)0;
    }
    const uint32_t ekey = p.drop_thr ? egnn_drop_base(p.drop_seed, EGNN_DROP_SITE_EDGE, (uint32_t)(q + p.drop_eid0)) : 0u;
    for (int h = 0; h < H; ++h) {
        T dk;
        const T x = eh_pre(p, pi, pj, sc, h, ekey, dk);
        const T sig = (T)1 / ((T)1 + eh_exp(-x));
        const T a = x * sig;
        const T a1 = sig * ((T)1 + x * ((T)1 - sig));
        const T* w2 = p.W2 + h;
        T ga = (T)0;
        if (MB > 0) {
#pragma unroll
            for (int c = 0; c < MR; ++c)
                if (c < m) ga = eh_fma(w2[(size_t)c * H], g[c], ga);
        } else {
            for (int c = 0; c < m; ++c) ga = eh_fma(w2[(size_t)c * H], gu[c], ga);
        }
        const T dz = dk * a1 * ga;
        p.A_T[(size_t)h * E + q] = a;
        p.DZ_T[(size_t)h * E + q] = dz;
        const T* ws = p.Ws + (size_t)h * S;
        for (int s = 0; s < S; ++s) gs[s * EH_THREADS] = eh_fma(ws[s], dz, gs[s * EH_THREADS]);
    }
    for (int s = 0; s < S; ++s) p.g_s[(size_t)q * S + s] = gs[s * EH_THREADS];
}

// second order: d/d gU (E, m), d/d s (E, S), DAV_T, R_T, DZ_T (H, E)
template <typename T, int MB>
__global__ __launch_bounds__(EH_THREADS) void edge_hidden_bwd2_kernel(const EhArgs<T> p)
{
    const int64_t E = (int64_t)p.B * p.N * p.K;
    const int64_t q = (int64_t)blockIdx.x * EH_THREADS + threadIdx.x;
    if (q >= E) return;
    const int m = p.m_dim, H = p.H, S = p.S;
    const EhEdge ed = eh_edge(p, q);
    extern __shared__ __attribute__((aligned(16))) char eh_raw[];
    T* const sc = reinterpret_cast<T*>(eh_raw) + threadIdx.x;    // s_e
    T* const cs = sc + (size_t)S * EH_THREADS;                     // sbar_e
    T* const gs = cs + (size_t)S * EH_THREADS;                     // d/d s_e
    for (int s = 0; s < S; ++s) {
        sc[s * EH_THREADS] = p.s[(size_t)q * S + s];
        cs[s * EH_THREADS] = p.cs[(size_t)q * S + s];
        gs[s * EH_THREADS] = (T)0;
    }
    const T* pi = p.Pi + (size_t)ed.src * H;
    const T* pj = p.Pj + (size_t)ed.dst * H;
    const T* cpi = p.cPi + (size_t)ed.src * H;
    const T* cpj = p.cPj + (size_t)ed.dst * H;
    const T* gu = p.gU + (size_t)q * m;
    T* ggu = p.g_gU + (size_t)q * m;
    constexpr int MR = MB > 0 ? MB : 1;
    T g[MR], acc[MR];
    if (MB > 0) {
#pragma unroll
        for (int c = 0; c < MR; ++c) {
            g[c] = c < m ? gu[c] : (T)0;
            acc[c] = c < m ? p.cb2[c] : (T)0;
        }
    } else {
        for (int c = 0; c < m; ++c) ggu[c] = p.cb2[c];
    }
    const uint32_t ekey = p.drop_thr ? egnn_drop_base(p.drop_seed, EGNN_DROP_SITE_EDGE, (uint32_t)(q + p.drop_eid0)) : 0u;
    for (int h = 0; h < H; ++h) {
        T dk;
        const T x = eh_pre(p, pi, pj, sc, h, ekey, dk);
        const T sig = (T)1 / ((T)1 + eh_exp(-x));
        const T om = (T)1 - sig;
        const T a = x * sig;
        const T a1 = sig * ((T)1 + x * om);
        const T a2 = sig * om * ((T)2 + x * (om - sig));
        const T* ws = p.Ws + (size_t)h * S;
        const T* cws = p.cWs + (size_t)h * S;
        T v = cpi[h] + cpj[h];
        for (int s = 0; s < S; ++s) {
            v = eh_fma(cws[s], sc[s * EH_THREADS], v);
            v = eh_fma(ws[s], cs[s * EH_THREADS], v);
        }
        const T* w2 = p.W2 + h;
        const T* cw2 = p.cW2 + h;
        T ga = (T)0, wb = (T)0;
        if (MB > 0) {
#pragma unroll
            for (int c = 0; c < MR; ++c)
                if (c < m) {
                    ga = eh_fma(w2[(size_t)c * H], g[c], ga);
                    wb = eh_fma(cw2[(size_t)c * H], g[c], wb);
                }
        } else {
            for (int c = 0; c < m; ++c) {
                ga = eh_fma(w2[(size_t)c * H], gu[c], ga);
                wb = eh_fma(cw2[(size_t)c * H], gu[c], wb);
            }
        }
        const T dz = dk * a1 * ga;
        const T dav = dk * a1 * v;
        const T r = dk * (dk * a2 * ga * v + a1 * wb);
        if (MB > 0) {
#pragma unroll
            for (int c = 0; c < MR; ++c)
                if (c < m) acc[c] = eh_fma(cw2[(size_t)c * H], a, eh_fma(w2[(size_t)c * H], dav, acc[c]));
        } else {
            for (int c = 0; c < m; ++c) ggu[c] = eh_fma(cw2[(size_t)c * H], a, eh_fma(w2[(size_t)c * H], dav, ggu[c]));
        }
        for (int s = 0; s < S; ++s) gs[s * EH_THREADS] = eh_fma(cws[s], dz, eh_fma(ws[s], r, gs[s * EH_THREADS]));
        p.DZ_T[(size_t)h * E + q] = dz;
        p.DAV_T[(size_t)h * E + q] = dav;
        p.R_T[(size_t)h * E + q] = r;
    }
    if (MB > 0) {
#pragma unroll
        for (int c = 0; c < MR; ++c)
            if (c < m) ggu[c] = acc[c];
    }
    for (int s = 0; s < S; ++s) p.g_s[(size_t)q * S + s] = gs[s * EH_THREADS];
}

enum { EH_FWD = 0, EH_BWD = 1, EH_BWD2 = 2 };

template <typename T>
int edge_hidden_launch(const egnn_edge_hidden_args* args, int which, void* stream)
{
    if (!args) return EGNN_E_NULLPTR;
    const egnn_edge_hidden_args& a = *args;
    if (!a.Pi || !a.Pj || !a.s || !a.Ws || !a.W2) return EGNN_E_NULLPTR;
    if (which == EH_FWD && (!a.b2 || !a.u)) return EGNN_E_NULLPTR;
    if (which == EH_BWD && (!a.gU || !a.A_T || !a.DZ_T || !a.g_s)) return EGNN_E_NULLPTR;
    if (which == EH_BWD2 && (!a.gU || !a.cPi || !a.cPj || !a.cs || !a.cWs || !a.cW2 || !a.cb2 || !a.g_gU || !a.g_s || !a.DZ_T || !a.DAV_T || !a.R_T))
        return EGNN_E_NULLPTR;
    if (a.B <= 0 || a.N <= 0 || a.K <= 0 || a.H <= 0 || a.S <= 0 || a.m_dim <= 0) return EGNN_E_SHAPE;
    if (!a.idx && a.K != a.N) return EGNN_E_SHAPE;
    const int cols = which == EH_FWD ? 1 : (which == EH_BWD ? 2 : 3);    // LDS columns per thread: s [, sbar], d/d s
    const size_t lds = (size_t)cols * a.S * EH_THREADS * sizeof(T);
    if (lds > 160 * 1024) return EGNN_E_UNSUPPORTED;
    const int64_t E = (int64_t)a.B * a.N * a.K;
    const int64_t blocks = (E + EH_THREADS - 1) / EH_THREADS;
    if (blocks > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;
    if (a.drop_thr && (!(a.drop_inv_keep >= 1.f) || a.drop_eid0 < 0 || a.drop_eid0 + E > 0xffffffffLL)) return EGNN_E_SHAPE;
    EhArgs<T> p;
    p.B = a.B; p.N = a.N; p.K = a.K; p.m_dim = a.m_dim; p.H = a.H; p.S = a.S; p.idx = a.idx;
    p.Pi = static_cast<const T*>(a.Pi); p.Pj = static_cast<const T*>(a.Pj); p.s = static_cast<const T*>(a.s);
    p.Ws = static_cast<const T*>(a.Ws); p.W2 = static_cast<const T*>(a.W2); p.b2 = static_cast<const T*>(a.b2);
    p.gU = static_cast<const T*>(a.gU);
    p.cPi = static_cast<const T*>(a.cPi); p.cPj = static_cast<const T*>(a.cPj); p.cs = static_cast<const T*>(a.cs);
    p.cWs = static_cast<const T*>(a.cWs); p.cW2 = static_cast<const T*>(a.cW2); p.cb2 = static_cast<const T*>(a.cb2);
    p.u = static_cast<T*>(a.u); p.A_T = static_cast<T*>(a.A_T); p.DZ_T = static_cast<T*>(a.DZ_T); p.g_s = static_cast<T*>(a.g_s);
    p.g_gU = static_cast<T*>(a.g_gU); p.DAV_T = static_cast<T*>(a.DAV_T); p.R_T = static_cast<T*>(a.R_T);
    p.drop_thr = a.drop_thr; p.drop_seed = a.drop_seed; p.drop_inv_keep = a.drop_inv_keep; p.drop_eid0 = a.drop_eid0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto run = [&](auto kern) -> int {
        if (lds > 64 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return (int)e;
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(EH_THREADS), lds, st, p);
        return egnn_launch_status();
    };
    const int m = a.m_dim;
    constexpr bool f64 = sizeof(T) == 8;                               // (float64: half the channels per register file)
    if (which == EH_FWD) {
        if (m <= 16) return run(edge_hidden_fwd_kernel<T, 16>);
        if (m <= 32) return run(edge_hidden_fwd_kernel<T, 32>);
        if constexpr (!f64) {                                            // (constexpr: the double kernel is not even instantiated)
            if (m <= 64) return run(edge_hidden_fwd_kernel<T, 64>);
        }
        return run(edge_hidden_fwd_kernel<T, 0>);
    }
    if (which == EH_BWD) {
        if (m <= 16) return run(edge_hidden_bwd_kernel<T, 16>);
        if (m <= 32) return run(edge_hidden_bwd_kernel<T, 32>);
        if (m <= 64) return run(edge_hidden_bwd_kernel<T, 64>);
        return run(edge_hidden_bwd_kernel<T, 0>);
    }
    // (two register arrays of m_dim values: up to 32 channels (16 in float64) in registers, wider heads through their output row)
    if (m <= 16) return run(edge_hidden_bwd2_kernel<T, 16>);
    if constexpr (!f64) {
        if (m <= 32) return run(edge_hidden_bwd2_kernel<T, 32>);
    }
    return run(edge_hidden_bwd2_kernel<T, 0>);
}

}  // namespace

extern "C" int egnn_edge_hidden_fwd_f32(const egnn_edge_hidden_args* args, void* stream) { return edge_hidden_launch<float>(args, EH_FWD, stream); }
extern "C" int egnn_edge_hidden_fwd_f64(const egnn_edge_hidden_args* args, void* stream) { return edge_hidden_launch<double>(args, EH_FWD, stream); }
extern "C" int egnn_edge_hidden_bwd_f32(const egnn_edge_hidden_args* args, void* stream) { return edge_hidden_launch<float>(args, EH_BWD, stream); }
extern "C" int egnn_edge_hidden_bwd_f64(const egnn_edge_hidden_args* args, void* stream) { return edge_hidden_launch<double>(args, EH_BWD, stream); }
extern "C" int egnn_edge_hidden_bwd2_f32(const egnn_edge_hidden_args* args, void* stream) { return edge_hidden_launch<float>(args, EH_BWD2, stream); }
extern "C" int egnn_edge_hidden_bwd2_f64(const egnn_edge_hidden_args* args, void* stream) { return edge_hidden_launch<double>(args, EH_BWD2, stream); }

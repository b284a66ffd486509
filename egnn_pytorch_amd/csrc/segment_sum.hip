// Deterministic row gather-sum: out[r, :] = sum over p in [seg_ptr[r], seg_ptr[r+1]) of rows[order[p], :], in that order.
//
// The backward of the neighbour gather (egnn_pytorch.py:275, feats_j = batched_index_select(feats, nbhd_indices)):
// d loss / d P_j[j] is the sum of dz over every edge (i, k) whose neighbour is j.  `order` lists the edges sorted by
// destination (stable, so ties stay in edge order) -- the transposed neighbour list -- which makes the sum a fixed-order
// read-only reduction: no float atomics, bit-reproducible.  One WAVE per destination row (four rows per workgroup: narrow rows --
// the c3 layer's 1152 bytes -- would leave most of a 256-thread workgroup idle); every wave instruction reads 1 KB of one source
// row; HBM-bound (each source row is read exactly once).
#include "egnn_common.h"

namespace {

__global__ __launch_bounds__(256) void rows_gather_sum_kernel(const float* __restrict__ rows, int64_t ld, const int64_t* __restrict__ order,
                                                              const int64_t* __restrict__ seg_ptr, int64_t n_out, int cols,
                                                              float* __restrict__ out, int64_t ldo, uint32_t* __restrict__ amax_bits)
{
    __shared__ uint32_t amax_slot;
    uint32_t mx = 0u;
    const int64_t r_raw = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = r_raw < n_out;
    const int64_t r = live ? r_raw : n_out - 1;
    const int64_t p0 = seg_ptr[r], p1 = live ? seg_ptr[r + 1] : p0;
    for (int c = (threadIdx.x & 63) * 4; live && c < cols; c += 64 * 4) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        int64_t p = p0;
        for (; p + 1 < p1; p += 2) {                                   // two rows in flight
            const f32x4 a = *reinterpret_cast<const f32x4*>(rows + order[p] * ld + c);
            const f32x4 b = *reinterpret_cast<const f32x4*>(rows + order[p + 1] * ld + c);
            acc += a;
            acc += b;
        }
        if (p < p1) acc += *reinterpret_cast<const f32x4*>(rows + order[p] * ld + c);
        *reinterpret_cast<f32x4*>(out + r * ldo + c) = acc;
        if (amax_bits) {
#pragma unroll
            for (int u = 0; u < 4; ++u) { const uint32_t t = egnn_abs_bits(acc[u]); mx = mx > t ? mx : t; }
        }
    }
    if (amax_bits) egnn_block_absmax_commit(mx, &amax_slot, amax_bits);
}

}  // namespace

extern "C" int egnn_rows_gather_sum_f32(const float* rows, int64_t ld, const int64_t* order, const int64_t* seg_ptr, int64_t n_out,
                                        int cols, float* out, int64_t ldo, uint32_t* amax_bits, void* stream)
{
    if (!rows || !order || !seg_ptr || !out) return EGNN_E_NULLPTR;
    if (n_out <= 0 || cols <= 0 || (cols % 4) != 0 || ld < cols || ldo < cols || (ld % 4) != 0 || (ldo % 4) != 0) return EGNN_E_SHAPE;
    if (n_out > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(rows) & 15) || (reinterpret_cast<uintptr_t>(out) & 15)) return EGNN_E_ALIGN;
    if (amax_bits && hipMemsetAsync(amax_bits, 0, sizeof(uint32_t), static_cast<hipStream_t>(stream)) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(rows_gather_sum_kernel, dim3((unsigned)((n_out + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), rows, ld, order,
                       seg_ptr, n_out, cols, out, ldo, amax_bits);
    return egnn_launch_status();
}


// ---------------------------------------------------------------------------------------------------------------------------
// EGNN_Network front-end (egnn_pytorch.py:410-432): the per-pair edge features of the K selected pairs of every node, looked up
// from the embedding tables -- see include/egnn_hip.h::egnn_edge_features_gather_f32 / _f64 (T = float / double: a copy, the same
// kernel for both).  One thread per (edge, column).
namespace {

// SLOT: `deg` holds the labels of the selected pairs themselves, (B,N,K) bytes read at the slot (egnn_csr_slot_labels_u8 made them from a
// label CSR), instead of the (B,N,N) map read at [b, i, j] -- the _slot entries; the same kernel otherwise.
template <typename T, bool SLOT = false>
__global__ __launch_bounds__(256) void edge_features_gather_kernel(const T* __restrict__ edges, const int64_t* __restrict__ tok,
                                                                   const T* __restrict__ tok_emb, int d1,
                                                                   const uint8_t* __restrict__ deg, const T* __restrict__ deg_emb,
                                                                   int d2, const int32_t* __restrict__ idx, int N, int K, int64_t total,
                                                                   T* __restrict__ out)
{
    const int w = d1 + d2;
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t edge = o / w;
        const int col = (int)(o - edge * w);
        const int64_t node = edge / K;                              // b * N + i
        const int k = (int)(edge - node * K);
        const int j = idx ? idx[edge] : k;
        const int64_t pair = node * N + j;
        T v;
        if (col < d1) v = tok ? tok_emb[tok[pair] * d1 + col] : edges[pair * d1 + col];
        else v = deg_emb[(int64_t)deg[SLOT ? edge : pair] * d2 + (col - d1)];
        out[o] = v;
    }
}

template <typename T, bool SLOT = false>
int edge_features_gather(const T* edges, const int64_t* edge_tok, const T* edge_tok_emb, int d1, const uint8_t* adj_deg,
                         const T* adj_deg_emb, int d2, const int32_t* idx, int B, int N, int K, T* out, void* stream)
{
    if (!out) return EGNN_E_NULLPTR;
    if (B <= 0 || N <= 0 || K <= 0 || d1 < 0 || d2 < 0 || d1 + d2 <= 0) return EGNN_E_SHAPE;
    if (d1 > 0 && !edges && !(edge_tok && edge_tok_emb)) return EGNN_E_NULLPTR;
    if (d2 > 0 && (!adj_deg || !adj_deg_emb)) return EGNN_E_NULLPTR;
    if (!idx && K != N) return EGNN_E_SHAPE;
    const int64_t total = (int64_t)B * N * K * (d1 + d2);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL((edge_features_gather_kernel<T, SLOT>), dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), edges,
                       edge_tok, edge_tok_emb, d1, adj_deg, adj_deg_emb, d2, idx, N, K, total, out);
    return egnn_launch_status();
}

}  // namespace

extern "C" int egnn_edge_features_gather_f32(const float* edges, const int64_t* edge_tok, const float* edge_tok_emb, int d1,
                                             const uint8_t* adj_deg, const float* adj_deg_emb, int d2, const int32_t* idx,
                                             int B, int N, int K, float* out, void* stream)
{
    return edge_features_gather<float>(edges, edge_tok, edge_tok_emb, d1, adj_deg, adj_deg_emb, d2, idx, B, N, K, out, stream);
}

extern "C" int egnn_edge_features_gather_f64(const double* edges, const int64_t* edge_tok, const double* edge_tok_emb, int d1,
                                             const uint8_t* adj_deg, const double* adj_deg_emb, int d2, const int32_t* idx,
                                             int B, int N, int K, double* out, void* stream)
{
    return edge_features_gather<double>(edges, edge_tok, edge_tok_emb, d1, adj_deg, adj_deg_emb, d2, idx, B, N, K, out, stream);
}

extern "C" int egnn_edge_features_gather_slot_f32(const float* edges, const int64_t* edge_tok, const float* edge_tok_emb, int d1,
                                                  const uint8_t* slot_deg, const float* adj_deg_emb, int d2, const int32_t* idx,
                                                  int B, int N, int K, float* out, void* stream)
{
    return edge_features_gather<float, true>(edges, edge_tok, edge_tok_emb, d1, slot_deg, adj_deg_emb, d2, idx, B, N, K, out, stream);
}

extern "C" int egnn_edge_features_gather_slot_f64(const double* edges, const int64_t* edge_tok, const double* edge_tok_emb, int d1,
                                                  const uint8_t* slot_deg, const double* adj_deg_emb, int d2, const int32_t* idx,
                                                  int B, int N, int K, double* out, void* stream)
{
    return edge_features_gather<double, true>(edges, edge_tok, edge_tok_emb, d1, slot_deg, adj_deg_emb, d2, idx, B, N, K, out, stream);
}


// ---------------------------------------------------------------------------------------------------------------------------
// Its transpose, the backward of EGNN_Network's per-pair edge features under autograd -- see
// include/egnn_hip.h::egnn_edge_features_grad_f32 / _f64.  The gradient of an embedding table is a sum over the edges that carry each
// label; like every sum over edges here it has a fixed order and no float atomics:
//   launch 1: G workgroups (G a function of E and the table sizes only), each reduces a contiguous range of edges into a (V, D)
//             partial.  Its four waves take consecutive quarters of the range; a wave splits into P = 64 / D lane groups (one lane
//             per column), group p walks edges p, p + P, ... of the quarter in order into an LDS table of its own; the 4 P tables
//             are then summed in (wave, group) order.  Vocabularies whose tables do not fit the wave's LDS table run in label
//             blocks, one blockIdx.y per block: every label's sum still visits the same edges in the same order, so the bits do not
//             depend on the block size.
//   launch 2: one thread per output element sums the G partials in index order.
// Dense float edges (no token table) have no reduction: the pairs of one row are distinct, so their gradient rows are stored.
// T = float / double: the same kernels.  The LDS budget is the same in bytes, so a wave's table holds half as many doubles (label
// blocks half as large); G, the walk and the order of every sum do not depend on T.
namespace {

constexpr int FGRAD_LDS_WAVE_BYTES = 8192;                     // 8 KB per wave, 32 KB per workgroup
template <typename T> constexpr int FGRAD_LDS_WAVE_ELEMS = FGRAD_LDS_WAVE_BYTES / (int)sizeof(T);   // float: 2048, double: 1024
constexpr int FGRAD_EDGES_PER_GROUP = 2048;                    // edges per workgroup of launch 1 at most, before the G cap

struct FeatGradTable {
    int V, D, Vb, nb, col0;                                    // vocabulary, width, labels per block, blocks, first column in g
    int64_t off;                                               // offset of this table in a partial
};

__device__ __forceinline__ int fgrad_groups(int D) { return D <= 64 ? 64 / D : 1; }

// CSR: the first table's labels are the values of a CSR (egnn_pytorch_amd.SparseEdges), `tok` (nnz) read at pos[e] -- the position
// egnn_edge_features_gather_csr_f32 / _f64 found for slot e; a slot whose row does not hold its pair (pos < 0) carries token 0, as the
// dense image does.  The same walk and the same sums otherwise: the _csr entries.
template <typename T, bool SLOT = false, bool CSR = false>
__global__ __launch_bounds__(256) void edge_features_grad_part_kernel(const T* __restrict__ g, int64_t ld,
                                                                      const int64_t* __restrict__ tok, const uint8_t* __restrict__ deg,
                                                                      const int32_t* __restrict__ idx, const int32_t* __restrict__ pos,
                                                                      int N, int K, int64_t E,
                                                                      int64_t per, FeatGradTable t1, FeatGradTable t2,
                                                                      T* __restrict__ part, int64_t stride)
{
    constexpr int WAVE_ELEMS = FGRAD_LDS_WAVE_ELEMS<T>;
    __shared__ T tab[4 * WAVE_ELEMS];
    const bool second = (int)blockIdx.y >= t1.nb;
    const FeatGradTable t = second ? t2 : t1;
    const int blk = second ? (int)blockIdx.y - t1.nb : (int)blockIdx.y;
    const int D = t.D, P = fgrad_groups(D), Vb = t.Vb;
    const int vb0 = blk * Vb;
    const int vn = min(Vb, t.V - vb0);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int o = threadIdx.x; o < 4 * WAVE_ELEMS; o += 256) tab[o] = T(0);
    __syncthreads();

    const int64_t e0 = (int64_t)blockIdx.x * per;
    const int64_t e1 = min(E, e0 + per);
    const int64_t q = e1 > e0 ? (e1 - e0 + 3) / 4 : 0;
    const int64_t ws = e0 + wave * q;
    const int64_t we = min(e1, ws + q);
    const int p = D <= 64 ? lane / D : 0;
    const int c0 = D <= 64 ? lane - p * D : lane;
    T* mine = tab + wave * WAVE_ELEMS + p * Vb * D;
    const T* gcol = g + t.col0;
    auto label = [&](int64_t e) -> int {                       // this block's row of edge e's label, or -1
        const int64_t node = e / K;                            // b * N + i
        const int k = (int)(e - node * K);
        const int j = idx ? idx[e] : k;
        if ((unsigned)j >= (unsigned)N) return -1;
        const int64_t pair = node * N + j;
        int64_t v;
        if (second) v = (int64_t)deg[SLOT ? e : pair];
        else if (CSR) { const int32_t ps = pos[e]; v = ps >= 0 ? tok[ps] : (int64_t)0; }
        else v = tok[pair];
        v -= vb0;
        return (v >= 0 && v < vn) ? (int)v : -1;
    };
    if (p < P) {
        int64_t e = ws + p;
        for (; e + 3 * (int64_t)P < we; e += 4 * (int64_t)P) { // four edges in flight, added in order
            int r[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = label(e + u * (int64_t)P);
            for (int c = c0; c < D; c += 64) {
                T x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) x[u] = gcol[(e + u * (int64_t)P) * ld + c];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (r[u] >= 0) mine[r[u] * D + c] += x[u];
            }
        }
        for (; e < we; e += P) {
            const int r = label(e);
            if (r < 0) continue;
            for (int c = c0; c < D; c += 64) mine[r * D + c] += gcol[e * ld + c];
        }
    }
    __syncthreads();
    const int tables = 4 * P;
    T* out = part + (int64_t)blockIdx.x * stride + t.off + (int64_t)vb0 * D;
    for (int o = threadIdx.x; o < vn * D; o += 256) {
        T s = T(0);
        for (int w = 0; w < tables; ++w) s += tab[(w / P) * WAVE_ELEMS + (w % P) * Vb * D + o];
        out[o] = s;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void edge_features_grad_sum_kernel(const T* __restrict__ part, int64_t stride, int G,
                                                                     int64_t n1, T* __restrict__ out1, T* __restrict__ out2)
{
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= stride) return;
    T s = T(0);
    int gi = 0;
    for (; gi + 4 <= G; gi += 4) {                             // four loads in flight, added in index order
        const T a = part[(int64_t)gi * stride + o], b = part[(int64_t)(gi + 1) * stride + o];
        const T c = part[(int64_t)(gi + 2) * stride + o], d = part[(int64_t)(gi + 3) * stride + o];
        s += a;
        s += b;
        s += c;
        s += d;
    }
    for (; gi < G; ++gi) s += part[(int64_t)gi * stride + o];
    if (o < n1) out1[o] = s;
    else out2[o - n1] = s;
}

template <typename T>
__global__ __launch_bounds__(256) void edge_features_grad_dense_kernel(const T* __restrict__ g, int64_t ld,
                                                                       const int32_t* __restrict__ idx, int N, int K, int d1,
                                                                       int64_t total, T* __restrict__ g_edges)
{
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t e = o / d1;
        const int c = (int)(o - e * d1);
        const int64_t node = e / K;
        const int k = (int)(e - node * K);
        const int j = idx ? idx[e] : k;
        if ((unsigned)j >= (unsigned)N) continue;
        g_edges[(node * N + j) * d1 + c] = g[e * ld + c];
    }
}

// ... and of float CSR values: g_values[pos[e], :] = g[e, :d1] where the row holds the pair -- a plain store as well (the K pairs of a row
// are distinct and rows are per graph, so no two slots share a position)
template <typename T>
__global__ __launch_bounds__(256) void edge_features_grad_values_kernel(const T* __restrict__ g, int64_t ld,
                                                                        const int32_t* __restrict__ pos, int d1, int64_t total,
                                                                        T* __restrict__ g_values)
{
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t e = o / d1;
        const int c = (int)(o - e * d1);
        const int32_t ps = pos[e];
        if (ps < 0) continue;
        g_values[(int64_t)ps * d1 + c] = g[e * ld + c];
    }
}

FeatGradTable fgrad_table(bool on, int V, int D, int col0, int64_t off, int wave_elems)
{
    FeatGradTable t{};
    if (!on) return t;
    const int P = D <= 64 ? 64 / D : 1;
    t.V = V;
    t.D = D;
    t.Vb = wave_elems / (P * D) > 1 ? wave_elems / (P * D) : 1;
    t.nb = (V + t.Vb - 1) / t.Vb;
    t.col0 = col0;
    t.off = off;
    return t;
}

// CSR (with SLOT): edge_tok holds the tokens of a CSR's entries and g_edges is g_values (nnz, d1), both reached through pos (B,N,K)
template <typename T, bool SLOT = false, bool CSR = false>
int edge_features_grad(const T* g, int64_t ld, const int64_t* edge_tok, int V1, int d1, const uint8_t* adj_deg, int V2, int d2,
                       const int32_t* idx, int B, int N, int K, T* g_tok_emb, T* g_deg_emb, T* g_edges, T* work,
                       int64_t* work_floats, void* stream, const int32_t* pos = nullptr)
{
    constexpr int WAVE_ELEMS = FGRAD_LDS_WAVE_ELEMS<T>;
    if (!work_floats) return EGNN_E_NULLPTR;
    if (B <= 0 || N <= 0 || K <= 0 || d1 < 0 || d2 < 0 || d1 + d2 <= 0 || ld < d1 + d2) return EGNN_E_SHAPE;
    if (!idx && K != N) return EGNN_E_SHAPE;
    const bool on1 = g_tok_emb != nullptr, on2 = g_deg_emb != nullptr;
    if ((on1 && (!edge_tok || V1 <= 0 || d1 <= 0)) || (on2 && (!adj_deg || V2 <= 0 || d2 <= 0))) return EGNN_E_SHAPE;
    if (g_edges && (edge_tok || d1 <= 0)) return EGNN_E_SHAPE;
    if ((on1 && d1 > WAVE_ELEMS) || (on2 && d2 > WAVE_ELEMS)) return EGNN_E_UNSUPPORTED;
    const FeatGradTable t1 = fgrad_table(on1, V1, d1, 0, 0, WAVE_ELEMS),
                        t2 = fgrad_table(on2, V2, d2, d1, on1 ? (int64_t)V1 * d1 : 0, WAVE_ELEMS);
    if ((int64_t)t1.nb + t2.nb > 65535) return EGNN_E_UNSUPPORTED;
    const int64_t E = (int64_t)B * N * K;
    const int64_t n1 = on1 ? (int64_t)V1 * d1 : 0, n2 = on2 ? (int64_t)V2 * d2 : 0;
    const int64_t stride = n1 + n2;
    int64_t G = 0;
    if (stride > 0) {
        // a function of E and the table sizes only: the partition, and with it every bit of the result, is the same on any device
        int64_t cap = (int64_t(1) << 24) / stride;
        cap = cap < 1 ? 1 : (cap > 1024 ? 1024 : cap);
        G = (E + FGRAD_EDGES_PER_GROUP - 1) / FGRAD_EDGES_PER_GROUP;
        G = G < cap ? G : cap;
    }
    if (!work) {                                                 // size query: nothing is launched
        *work_floats = G * stride;
        return EGNN_OK;
    }
    if (*work_floats < G * stride) return EGNN_E_SHAPE;
    if (!g || (CSR && !pos)) return EGNN_E_NULLPTR;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (g_edges) {
        const int64_t total = E * d1;
        int64_t blocks = (total + 255) / 256;
        if (blocks > 65536) blocks = 65536;
        if (CSR)
            hipLaunchKernelGGL(edge_features_grad_values_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, g, ld, pos, d1, total,
                               g_edges);
        else
            hipLaunchKernelGGL(edge_features_grad_dense_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, g, ld, idx, N, K, d1, total,
                               g_edges);
        const int rc = egnn_launch_status();
        if (rc) return rc;
    }
    if (stride == 0) return EGNN_OK;
    const int64_t per = (E + G - 1) / G;
    hipLaunchKernelGGL((edge_features_grad_part_kernel<T, SLOT, CSR>), dim3((unsigned)G, (unsigned)(t1.nb + t2.nb)), dim3(256), 0, st, g,
                       ld, edge_tok, adj_deg, idx, pos, N, K, E, per, t1, t2, work, stride);
    int rc = egnn_launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(edge_features_grad_sum_kernel<T>, dim3((unsigned)((stride + 255) / 256)), dim3(256), 0, st, work, stride, (int)G,
                       n1, g_tok_emb, g_deg_emb);
    return egnn_launch_status();
}

}  // namespace

extern "C" int egnn_edge_features_grad_f32(const float* g, int64_t ld, const int64_t* edge_tok, int V1, int d1,
                                           const uint8_t* adj_deg, int V2, int d2, const int32_t* idx, int B, int N, int K,
                                           float* g_tok_emb, float* g_deg_emb, float* g_edges, float* work, int64_t* work_floats,
                                           void* stream)
{
    return edge_features_grad<float>(g, ld, edge_tok, V1, d1, adj_deg, V2, d2, idx, B, N, K, g_tok_emb, g_deg_emb, g_edges, work,
                                     work_floats, stream);
}

extern "C" int egnn_edge_features_grad_f64(const double* g, int64_t ld, const int64_t* edge_tok, int V1, int d1,
                                           const uint8_t* adj_deg, int V2, int d2, const int32_t* idx, int B, int N, int K,
                                           double* g_tok_emb, double* g_deg_emb, double* g_edges, double* work, int64_t* work_floats,
                                           void* stream)
{
    return edge_features_grad<double>(g, ld, edge_tok, V1, d1, adj_deg, V2, d2, idx, B, N, K, g_tok_emb, g_deg_emb, g_edges, work,
                                      work_floats, stream);
}

extern "C" int egnn_edge_features_grad_slot_f32(const float* g, int64_t ld, const int64_t* edge_tok, int V1, int d1,
                                                const uint8_t* slot_deg, int V2, int d2, const int32_t* idx, int B, int N, int K,
                                                float* g_tok_emb, float* g_deg_emb, float* g_edges, float* work, int64_t* work_floats,
                                                void* stream)
{
    return edge_features_grad<float, true>(g, ld, edge_tok, V1, d1, slot_deg, V2, d2, idx, B, N, K, g_tok_emb, g_deg_emb, g_edges, work,
                                           work_floats, stream);
}

extern "C" int egnn_edge_features_grad_slot_f64(const double* g, int64_t ld, const int64_t* edge_tok, int V1, int d1,
                                                const uint8_t* slot_deg, int V2, int d2, const int32_t* idx, int B, int N, int K,
                                                double* g_tok_emb, double* g_deg_emb, double* g_edges, double* work, int64_t* work_floats,
                                                void* stream)
{
    return edge_features_grad<double, true>(g, ld, edge_tok, V1, d1, slot_deg, V2, d2, idx, B, N, K, g_tok_emb, g_deg_emb, g_edges, work,
                                            work_floats, stream);
}

// The CSR first table (egnn_pytorch_amd.SparseEdges): tokens (nnz) / g_values (nnz, d1) reached through pos (B,N,K), the positions
// egnn_edge_features_gather_csr_f32 / _f64 wrote; the degree labels per slot.
extern "C" int egnn_edge_features_grad_csr_f32(const float* g, int64_t ld, const int32_t* pos, const int64_t* tokens, int V1, int d1,
                                               const uint8_t* slot_deg, int V2, int d2, const int32_t* idx, int B, int N, int K,
                                               float* g_tok_emb, float* g_deg_emb, float* g_values, float* work, int64_t* work_floats,
                                               void* stream)
{
    if (!pos) return EGNN_E_NULLPTR;
    return edge_features_grad<float, true, true>(g, ld, tokens, V1, d1, slot_deg, V2, d2, idx, B, N, K, g_tok_emb, g_deg_emb, g_values,
                                                 work, work_floats, stream, pos);
}

extern "C" int egnn_edge_features_grad_csr_f64(const double* g, int64_t ld, const int32_t* pos, const int64_t* tokens, int V1, int d1,
                                               const uint8_t* slot_deg, int V2, int d2, const int32_t* idx, int B, int N, int K,
                                               double* g_tok_emb, double* g_deg_emb, double* g_values, double* work,
                                               int64_t* work_floats, void* stream)
{
    if (!pos) return EGNN_E_NULLPTR;
    return edge_features_grad<double, true, true>(g, ld, tokens, V1, d1, slot_deg, V2, d2, idx, B, N, K, g_tok_emb, g_deg_emb, g_values,
                                                  work, work_floats, stream, pos);
}

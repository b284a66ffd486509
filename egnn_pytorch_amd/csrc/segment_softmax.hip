// Per-graph softmax of a PACKED batch (gfx950): the statistics (m, l) of every (graph, column), the normalised weights, the attention
// pool out[g, h, :] = sum_i softmax(s[:, h])_i v[i, h, :] over the rows of graph g, and the first-order backward of that pool.
// No float atomics; every result of a graph is a function of its own rows, its size n and the column count only.
//
// THE ORDER (the pieces are those of segment_reduce.hip, taken from segment_core.h):
//   m        the maximum of the graph's column, a NaN winning over every number: a result that no order of comparisons changes.  It
//            walks the chunks, strands and tree of the sum and is FINISHED (partials combined) before anything is exponentiated.
//   l        sum_i exp(x_i - m) with that final m: the subtraction first, then the accurate exp / expf, the terms added in the order
//            of segment_reduce's sum -- chunks of R = 128 rows from the graph's own first row, S = 256 / TC strands, the fixed LDS
//            tree, the partials in chunk order.  An empty graph stores (m, l) = (-inf, 0).
//   apply    y = exp(x - m) / l per element: one subtraction, one exp, one division.
//   pool     the numerator sum_i exp(s[i, h] - m[g, h]) v[i, h, c] is the sum above over the flattened (T, H Dv) matrix -- a thread
//            owns 4 adjacent flattened columns, S follows from H Dv -- each term formed as fma(w, v, acc) with w = exp(s - m) taken
//            PER COLUMN (Dv % 4 != 0 puts a head boundary inside a thread's four columns); then ONE division by l[g, h].  An empty
//            graph stores 0.
// A column that is all -inf has m = -inf, so x - m = NaN and l, y and the pool come out NaN, as in torch; a NaN in a column makes m, l
// and everything derived from them NaN for that (graph, column) and touches nothing else; exp(-inf - m) = +0 exactly for a finite m.
// The 16-byte path (D % 4 == 0, base and pitch 16-byte aligned) and the scalar path give every thread the same columns and rows, so the
// same values meet the same operations in the same order.  Every element of every output is stored by a kernel; table entries out of
// range are clamped into their arrays.
//
// backward of the pool (first order): with w = exp(s - m) / l, d_values[t, h, c] = w g[seg, h, c] and
// d_scores[t, h] = w sum_c g[seg, h, c] (v[t, h, c] - out[seg, h, c]) -- the difference first, then fma into the sum.  L = the power of
// two >= Dv, at most 64, lanes share a (row, head): lane j adds the columns j, j + L, ... in that order, then the fixed LDS tree of the
// sum combines the L lanes: an order that depends on Dv only.
#include "segment_core.h"

namespace {

enum { SS_MAX = 0, SS_EXPSUM = 1, SS_POOL = 2 };

__device__ __forceinline__ float ss_exp(float v) { return expf(v); }
__device__ __forceinline__ double ss_exp(double v) { return exp(v); }
__device__ __forceinline__ float ss_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double ss_fma(double a, double b, double c) { return fma(a, b, c); }

// the larger of two, a NaN winning (and staying)
template <typename T>
__device__ __forceinline__ T ss_max(T a, T b) { return (b != b || b > a) ? b : a; }

template <typename T>
__device__ __forceinline__ T ss_neg_inf() { return -(T)INFINITY; }

__device__ __forceinline__ int ss_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// One chunk of one graph, 4 adjacent columns per thread, the strands and the tree of segment_reduce.hip.
//   SS_MAX     x (T, D) -> m: the running maximum
//   SS_EXPSUM  x (T, D), m (G, D) -> l: the sum of exp(x - m)
//   SS_POOL    x = values (T, D = H Dv), s = scores (T, H), m, l (G, H) -> out (G, D): the sum of exp(s - m) v, divided by l
// stat_in: m (SS_EXPSUM, SS_POOL); stat_l: l (SS_POOL).  The only chunk of a graph stores its row of `out`, the others their partial.
template <typename T, bool VEC, int MODE>
__global__ __launch_bounds__(SR_THREADS) void segment_softmax_chunks_kernel(
    const T* __restrict__ x, int64_t ld, const T* __restrict__ sc, int64_t lds, const T* __restrict__ stat_in, const T* __restrict__ stat_l,
    const int64_t* __restrict__ offsets, const int32_t* __restrict__ chunk_row, const int32_t* __restrict__ chunk_seg,
    const int32_t* __restrict__ chunk_slot, int G, int64_t NT, int D, int H, int Dv, int tcl, int n_slots, T* __restrict__ out,
    T* __restrict__ part)
{
    __shared__ T sm[4 * SR_THREADS];
    const int tid = threadIdx.x, S = SR_THREADS >> tcl;
    const int s = tid >> tcl, c = (((int)blockIdx.y << tcl) + (tid & ((1 << tcl) - 1))) * 4;
    const SrChunk k = sr_chunk(offsets, chunk_row, chunk_seg, (int)blockIdx.x, G, NT);
    const T init = MODE == SS_MAX ? ss_neg_inf<T>() : T(0);
    T acc[4] = {init, init, init, init};
    int hu[4] = {0, 0, 0, 0};                            // SS_POOL: the head of each of the four columns
    if (c < D) {
        T mu[4] = {T(0), T(0), T(0), T(0)};
        if constexpr (MODE == SS_EXPSUM) {
#pragma unroll
            for (int u = 0; u < 4; ++u) mu[u] = stat_in[(int64_t)k.seg * D + (c + u < D ? c + u : D - 1)];
        } else if constexpr (MODE == SS_POOL) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                hu[u] = ss_clamp((c + u) / Dv, H);
                mu[u] = stat_in[(int64_t)k.seg * H + hu[u]];
            }
        }
        const T* p = x + k.r0 * ld + c;
        const T* ps = sc + k.r0 * lds;                   // (SS_POOL only)
#pragma unroll 2
        for (int r = s; r < k.m; r += S) {
            T v[4];
            sr_load4<T, VEC>(p + (int64_t)r * ld, c, D, init, v);
            if constexpr (MODE == SS_MAX) {
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = ss_max(acc[u], v[u]);
            } else if constexpr (MODE == SS_EXPSUM) {
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] += ss_exp(v[u] - mu[u]);
            } else {
                const T* q = ps + (int64_t)r * lds;
                T w[4];
                w[0] = ss_exp(q[hu[0]] - mu[0]);
#pragma unroll
                for (int u = 1; u < 4; ++u) {            // (the same head: the same bits, so the exponential is taken once)
                    if (hu[u] == hu[u - 1]) w[u] = w[u - 1];
                    else w[u] = ss_exp(q[hu[u]] - mu[u]);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] = ss_fma(w[u], v[u], acc[u]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) sm[u * SR_THREADS + tid] = acc[u];
    for (int h = S >> 1; h >= 1; h >>= 1) {
        __syncthreads();
        if (s < h) {                                     // (reads strands [h, 2h), writes strands [0, h): disjoint within a round)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const T o = sm[u * SR_THREADS + tid + (h << tcl)];
                acc[u] = MODE == SS_MAX ? ss_max(acc[u], o) : acc[u] + o;
                sm[u * SR_THREADS + tid] = acc[u];
            }
        }
    }
    if (s != 0 || c >= D) return;
    const int slot = chunk_slot[(int)blockIdx.x];
    if (slot < 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (c + u < D) {
                T r = acc[u];
                if constexpr (MODE == SS_POOL) r = k.n > 0 ? acc[u] / stat_l[(int64_t)k.seg * H + hu[u]] : T(0);
                out[(int64_t)k.seg * D + c + u] = r;
            }
    } else if (slot < n_slots) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (c + u < D) part[(int64_t)slot * D + c + u] = acc[u];
    }
}

// the partials of one graph longer than R, in chunk order; one thread per (graph, column)
template <typename T, int MODE>
__global__ __launch_bounds__(SR_THREADS) void segment_softmax_combine_kernel(
    const T* __restrict__ part, const T* __restrict__ stat_l, const int64_t* __restrict__ offsets, const int32_t* __restrict__ multi_seg,
    const int32_t* __restrict__ multi_slot, int G, int D, int H, int Dv, int n_slots, T* __restrict__ out)
{
    const int c = (int)blockIdx.y * SR_THREADS + threadIdx.x;
    if (c >= D) return;
    const int seg = ss_clamp(multi_seg[blockIdx.x], G);
    const int64_t n = offsets[seg + 1] - offsets[seg];
    const int slot0 = ss_clamp(multi_slot[blockIdx.x], n_slots);
    int64_t nch = (n + SR_ROWS - 1) / SR_ROWS;
    nch = nch < 1 ? 1 : (nch > n_slots - slot0 ? n_slots - slot0 : nch);
    const T* p = part + (int64_t)slot0 * D + c;
    T acc = p[0];
    int64_t q = 1;
    for (; q + 16 <= nch; q += 16) {                     // sixteen loads in flight, combined in chunk order
        T v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = p[(q + u) * D];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = MODE == SS_MAX ? ss_max(acc, v[u]) : acc + v[u];
    }
    for (; q < nch; ++q) acc = MODE == SS_MAX ? ss_max(acc, p[q * D]) : acc + p[q * D];
    if constexpr (MODE == SS_POOL) acc = n > 0 ? acc / stat_l[(int64_t)seg * H + ss_clamp(c / Dv, H)] : T(0);
    out[(int64_t)seg * D + c] = acc;
}

// y[t, c] = exp(x[t, c] - m[g, c]) / l[g, c], g = segment_of[t]; a thread owns 4 adjacent columns of one row
template <typename T, bool VEC>
__global__ __launch_bounds__(SR_THREADS) void segment_softmax_apply_kernel(const T* __restrict__ x, int64_t ld, const T* __restrict__ m,
                                                                           const T* __restrict__ l, const int32_t* __restrict__ segment_of,
                                                                           int G, int D, int groups, int64_t total, T* __restrict__ y)
{
    for (int64_t o = (int64_t)blockIdx.x * SR_THREADS + threadIdx.x; o < total; o += (int64_t)gridDim.x * SR_THREADS) {
        const int64_t t = o / groups;
        const int c = (int)(o - t * groups) * 4;
        const int64_t sb = (int64_t)ss_clamp(segment_of[t], G) * D + c;
        T v[4], mm[4], ll[4];
        sr_load4<T, VEC>(x + t * ld + c, c, D, T(0), v);
        sr_load4<T, VEC>(m + sb, c, D, T(0), mm);
        sr_load4<T, VEC>(l + sb, c, D, T(1), ll);
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = ss_exp(v[u] - mm[u]) / ll[u];
        T* py = y + t * D + c;
        if constexpr (VEC && sizeof(T) == 4) {
            f32x4 q;
            q[0] = v[0]; q[1] = v[1]; q[2] = v[2]; q[3] = v[3];
            *reinterpret_cast<f32x4*>(py) = q;
        } else if constexpr (VEC) {
            f64x2 a, b;
            a[0] = v[0]; a[1] = v[1]; b[0] = v[2]; b[1] = v[3];
            *reinterpret_cast<f64x2*>(py) = a;
            *reinterpret_cast<f64x2*>(py + 2) = b;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (c + u < D) py[u] = v[u];
        }
    }
}

// L = 1 << ll lanes share one (row, head); 256 / L pairs per workgroup and round; the trip count is the workgroup's, so every barrier
// is reached by all of its threads
template <typename T>
__global__ __launch_bounds__(SR_THREADS) void segment_pool_bwd_kernel(
    const T* __restrict__ g, const T* __restrict__ out, const T* __restrict__ sc, int64_t lds, const T* __restrict__ values, int64_t ldv,
    const T* __restrict__ m, const T* __restrict__ l, const int32_t* __restrict__ segment_of, int G, int H, int Dv, int ll, int64_t pairs,
    T* __restrict__ d_scores, T* __restrict__ d_values)
{
    __shared__ T sm[SR_THREADS];
    const int tid = threadIdx.x, L = 1 << ll, lane = tid & (L - 1), per = SR_THREADS >> ll;
    for (int64_t base = (int64_t)blockIdx.x * per; base < pairs; base += (int64_t)gridDim.x * per) {
        const int64_t pair = base + (tid >> ll);
        T acc = T(0), w = T(0);
        if (pair < pairs) {
            const int64_t t = pair / H;
            const int h = (int)(pair - t * H);
            const int64_t gh = (int64_t)ss_clamp(segment_of[t], G) * H + h;
            w = ss_exp(sc[t * lds + h] - m[gh]) / l[gh];
            const T* gp = g + gh * Dv;
            const T* op = out + gh * Dv;
            const T* vp = values + t * ldv + (int64_t)h * Dv;
            T* dp = d_values + pair * Dv;
            for (int c = lane; c < Dv; c += L) {
                const T gv = gp[c];
                acc = ss_fma(gv, vp[c] - op[c], acc);
                dp[c] = w * gv;
            }
        }
        __syncthreads();                                 // (the previous round's tree has been read)
        sm[tid] = acc;
        for (int hh = L >> 1; hh >= 1; hh >>= 1) {
            __syncthreads();
            if (lane < hh) {
                acc += sm[tid + hh];
                sm[tid] = acc;
            }
        }
        if (lane == 0 && pair < pairs) d_scores[pair] = w * acc;
    }
}

unsigned ss_flat_blocks(int64_t blocks) { return (unsigned)(blocks > 65536 ? 65536 : (blocks < 1 ? 1 : blocks)); }

struct SsTables {
    const int64_t* offsets;
    const int32_t *chunk_row, *chunk_seg, *chunk_slot;
    int n_chunks;
    const int32_t *multi_seg, *multi_slot;
    int n_multi;
};

// the checks the chunked entries share (D: the columns the strands walk)
int ss_check_tables(const SsTables& tb, int G, int64_t NT, int64_t D, const void* workspace, size_t workspace_bytes, size_t elem)
{
    if (!tb.offsets || !tb.chunk_row || !tb.chunk_seg || !tb.chunk_slot) return EGNN_E_NULLPTR;
    if (tb.n_multi > 0 && (!tb.multi_seg || !tb.multi_slot || !workspace)) return EGNN_E_NULLPTR;
    if (G <= 0 || NT <= 0 || D <= 0 || tb.n_chunks < G || tb.n_multi < 0 || tb.n_multi > tb.n_chunks) return EGNN_E_SHAPE;
    if (NT > 0x7fffffffLL || D > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;
    const int tcl = sr_col_threads_log2((int)D);
    if ((D + (4 << tcl) - 1) / (4 << tcl) > 65535 || (D + SR_THREADS - 1) / SR_THREADS > 65535) return EGNN_E_UNSUPPORTED;
    if (tb.n_multi > 0 && workspace_bytes < sr_workspace_bytes(G, NT, D, elem)) return EGNN_E_SHAPE;
    if (tb.n_multi > 0 && (reinterpret_cast<uintptr_t>(workspace) & 15)) return EGNN_E_ALIGN;
    return EGNN_OK;
}

// one walk over the chunks (and the combine of the graphs longer than one): MODE over x (T, D)
template <typename T, int MODE>
int ss_walk(const T* x, int64_t ld, const T* sc, int64_t lds, const T* stat_in, const T* stat_l, const SsTables& tb, int G, int64_t NT, int D,
            int H, int Dv, T* out, void* workspace, hipStream_t st)
{
    const int tcl = sr_col_threads_log2(D);
    const unsigned tiles = (unsigned)((D + (4 << tcl) - 1) / (4 << tcl));
    const int n_slots = tb.n_multi > 0 ? (int)sr_slots(G, NT) : 0;
    T* part = static_cast<T*>(workspace);
    const bool vec = D % 4 == 0 && (ld * (int64_t)sizeof(T)) % 16 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    auto kern = vec ? segment_softmax_chunks_kernel<T, true, MODE> : segment_softmax_chunks_kernel<T, false, MODE>;
    hipLaunchKernelGGL(kern, dim3((unsigned)tb.n_chunks, tiles), dim3(SR_THREADS), 0, st, x, ld, sc, lds, stat_in, stat_l, tb.offsets,
                       tb.chunk_row, tb.chunk_seg, tb.chunk_slot, G, NT, D, H, Dv, tcl, n_slots, out, part);
    int rc = egnn_launch_status();
    if (rc || tb.n_multi == 0) return rc;
    hipLaunchKernelGGL((segment_softmax_combine_kernel<T, MODE>), dim3((unsigned)tb.n_multi, (unsigned)((D + SR_THREADS - 1) / SR_THREADS)),
                       dim3(SR_THREADS), 0, st, part, stat_l, tb.offsets, tb.multi_seg, tb.multi_slot, G, D, H, Dv, n_slots, out);
    return egnn_launch_status();
}

template <typename T>
int segment_softmax_stats(const T* x, int64_t ldx, const SsTables& tb, int G, int64_t NT, int D, T* m, T* l, void* workspace,
                          size_t workspace_bytes, void* stream)
{
    if (!x || !m || !l) return EGNN_E_NULLPTR;
    int rc = ss_check_tables(tb, G, NT, D, workspace, workspace_bytes, sizeof(T));
    if (rc) return rc;
    if (ldx < D) return EGNN_E_SHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = ss_walk<T, SS_MAX>(x, ldx, nullptr, 0, nullptr, nullptr, tb, G, NT, D, 1, 1, m, workspace, st);
    if (rc) return rc;
    return ss_walk<T, SS_EXPSUM>(x, ldx, nullptr, 0, m, nullptr, tb, G, NT, D, 1, 1, l, workspace, st);
}

template <typename T>
int segment_softmax_apply(const T* x, int64_t ldx, const T* m, const T* l, const int32_t* segment_of, int G, int64_t NT, int D, T* y,
                          void* stream)
{
    if (!x || !m || !l || !segment_of || !y) return EGNN_E_NULLPTR;
    if (G <= 0 || NT <= 0 || D <= 0 || ldx < D) return EGNN_E_SHAPE;
    if (NT > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;
    const int groups = (D + 3) / 4;
    const int64_t total = NT * groups;
    // m, l and y are contiguous (G, D) / (T, D): with D % 4 == 0 their rows are 16-byte aligned when their bases are
    const bool vec = D % 4 == 0 && (ldx * (int64_t)sizeof(T)) % 16 == 0 &&
                     ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(l) |
                       reinterpret_cast<uintptr_t>(y)) & 15) == 0;
    auto kern = vec ? segment_softmax_apply_kernel<T, true> : segment_softmax_apply_kernel<T, false>;
    hipLaunchKernelGGL(kern, dim3(ss_flat_blocks((total + SR_THREADS - 1) / SR_THREADS)), dim3(SR_THREADS), 0,
                       static_cast<hipStream_t>(stream), x, ldx, m, l, segment_of, G, D, groups, total, y);
    return egnn_launch_status();
}

template <typename T>
int segment_pool(const T* scores, int64_t lds, const T* values, int64_t ldv, const T* m, const T* l, const SsTables& tb, int G, int64_t NT,
                 int H, int Dv, T* out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!scores || !values || !m || !l || !out) return EGNN_E_NULLPTR;
    if (H <= 0 || Dv <= 0) return EGNN_E_SHAPE;
    const int64_t D = (int64_t)H * Dv;
    int rc = ss_check_tables(tb, G, NT, D, workspace, workspace_bytes, sizeof(T));
    if (rc) return rc;
    if (lds < H || ldv < D) return EGNN_E_SHAPE;
    return ss_walk<T, SS_POOL>(values, ldv, scores, lds, m, l, tb, G, NT, (int)D, H, Dv, out, workspace, static_cast<hipStream_t>(stream));
}

template <typename T>
int segment_pool_bwd(const T* g, const T* out, const T* scores, int64_t lds, const T* values, int64_t ldv, const T* m, const T* l,
                     const int32_t* segment_of, int G, int64_t NT, int H, int Dv, T* d_scores, T* d_values, void* stream)
{
    if (!g || !out || !scores || !values || !m || !l || !segment_of || !d_scores || !d_values) return EGNN_E_NULLPTR;
    if (G <= 0 || NT <= 0 || H <= 0 || Dv <= 0 || lds < H || ldv < (int64_t)H * Dv) return EGNN_E_SHAPE;
    if (NT > 0x7fffffffLL || (int64_t)H * Dv > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;
    int ll = 0;
    while ((1 << ll) < Dv && ll < 6) ++ll;
    const int64_t pairs = NT * H, per = SR_THREADS >> ll;
    hipLaunchKernelGGL(segment_pool_bwd_kernel<T>, dim3(ss_flat_blocks((pairs + per - 1) / per)), dim3(SR_THREADS), 0,
                       static_cast<hipStream_t>(stream), g, out, scores, lds, values, ldv, m, l, segment_of, G, H, Dv, ll, pairs, d_scores,
                       d_values);
    return egnn_launch_status();
}

}  // namespace

#define SS_TABLES SsTables{offsets, chunk_row, chunk_seg, chunk_slot, n_chunks, multi_seg, multi_slot, n_multi}

extern "C" int egnn_segment_softmax_stats_f32(const float* x, int64_t ldx, const int64_t* offsets, const int32_t* chunk_row,
                                              const int32_t* chunk_seg, const int32_t* chunk_slot, int n_chunks, const int32_t* multi_seg,
                                              const int32_t* multi_slot, int n_multi, int G, int64_t T, int D, float* m, float* l,
                                              void* workspace, size_t workspace_bytes, void* stream)
{
    return segment_softmax_stats<float>(x, ldx, SS_TABLES, G, T, D, m, l, workspace, workspace_bytes, stream);
}

extern "C" int egnn_segment_softmax_stats_f64(const double* x, int64_t ldx, const int64_t* offsets, const int32_t* chunk_row,
                                              const int32_t* chunk_seg, const int32_t* chunk_slot, int n_chunks, const int32_t* multi_seg,
                                              const int32_t* multi_slot, int n_multi, int G, int64_t T, int D, double* m, double* l,
                                              void* workspace, size_t workspace_bytes, void* stream)
{
    return segment_softmax_stats<double>(x, ldx, SS_TABLES, G, T, D, m, l, workspace, workspace_bytes, stream);
}

extern "C" int egnn_segment_softmax_apply_f32(const float* x, int64_t ldx, const float* m, const float* l, const int32_t* segment_of, int G,
                                              int64_t T, int D, float* y, void* stream)
{
    return segment_softmax_apply<float>(x, ldx, m, l, segment_of, G, T, D, y, stream);
}

extern "C" int egnn_segment_softmax_apply_f64(const double* x, int64_t ldx, const double* m, const double* l, const int32_t* segment_of, int G,
                                              int64_t T, int D, double* y, void* stream)
{
    return segment_softmax_apply<double>(x, ldx, m, l, segment_of, G, T, D, y, stream);
}

extern "C" int egnn_segment_pool_f32(const float* scores, int64_t lds, const float* values, int64_t ldv, const float* m, const float* l,
                                     const int64_t* offsets, const int32_t* chunk_row, const int32_t* chunk_seg, const int32_t* chunk_slot,
                                     int n_chunks, const int32_t* multi_seg, const int32_t* multi_slot, int n_multi, int G, int64_t T, int H,
                                     int Dv, float* out, void* workspace, size_t workspace_bytes, void* stream)
{
    return segment_pool<float>(scores, lds, values, ldv, m, l, SS_TABLES, G, T, H, Dv, out, workspace, workspace_bytes, stream);
}

extern "C" int egnn_segment_pool_f64(const double* scores, int64_t lds, const double* values, int64_t ldv, const double* m, const double* l,
                                     const int64_t* offsets, const int32_t* chunk_row, const int32_t* chunk_seg, const int32_t* chunk_slot,
                                     int n_chunks, const int32_t* multi_seg, const int32_t* multi_slot, int n_multi, int G, int64_t T, int H,
                                     int Dv, double* out, void* workspace, size_t workspace_bytes, void* stream)
{
    return segment_pool<double>(scores, lds, values, ldv, m, l, SS_TABLES, G, T, H, Dv, out, workspace, workspace_bytes, stream);
}

extern "C" int egnn_segment_pool_bwd_f32(const float* g, const float* out, const float* scores, int64_t lds, const float* values, int64_t ldv,
                                         const float* m, const float* l, const int32_t* segment_of, int G, int64_t T, int H, int Dv,
                                         float* d_scores, float* d_values, void* stream)
{
    return segment_pool_bwd<float>(g, out, scores, lds, values, ldv, m, l, segment_of, G, T, H, Dv, d_scores, d_values, stream);
}

extern "C" int egnn_segment_pool_bwd_f64(const double* g, const double* out, const double* scores, int64_t lds, const double* values,
                                         int64_t ldv, const double* m, const double* l, const int32_t* segment_of, int G, int64_t T, int H,
                                         int Dv, double* d_scores, double* d_values, void* stream)
{
    return segment_pool_bwd<double>(g, out, scores, lds, values, ldv, m, l, segment_of, G, T, H, Dv, d_scores, d_values, stream);
}

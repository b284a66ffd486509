// Per-graph readout of a PACKED batch (gfx950): x (T, D) node rows -> out (G, D) graph rows, graph g owning the rows
// [offsets[g], offsets[g + 1]) -- sum / mean / max / min -- and the way back (broadcast, scatter to the winning rows, gather at them).
// No float atomics: every result is a fixed-order reduction, and the order for a graph is a function of its own size n and of D only.
//
// THE ORDER (sum, mean; DESIGN.md §4 writes it down once more, tests/_segment_reduce_order.py restates it in numpy):
//   chunks   a segment is cut into chunks of R = SR_ROWS = 128 rows counted from ITS OWN first row: chunk k holds the segment's rows
//            [k R, min(n, (k + 1) R)).  A chunk never straddles a segment; an empty segment is one chunk of no rows.
//   strands  a thread owns 4 adjacent columns.  TC = the power of two >= ceil(D / 4), at most 16, threads lie along the columns (a column
//            tile is 4 TC <= 64 columns), which leaves S = 256 / TC row strands in the 256-thread workgroup.  Strand s starts at +0 and
//            adds the chunk's rows s, s + S, s + 2 S, ... in that order.
//   tree     the S strand sums are combined in LDS by a fixed binary tree: for h = S / 2, S / 4, ..., 1: strand s < h adds strand s + h
//            (a strand that received no row holds +0).  Strand 0 then holds the chunk's partial.
//   combine  a segment of one chunk is finished: the chunk kernel writes its row of `out`.  Otherwise the partials go to the workspace and
//            a second launch adds them in chunk order: p0, + p1, + p2, ...
//   mean     the sum, then ONE division by (T)n (an empty graph: 0).
// S depends on D alone, the rest on n alone; nothing depends on G, on the segment's offset, on its neighbours, or on how the rows were
// loaded: the 16-byte path (D % 4 == 0, base and row pitch 16-byte aligned) and the scalar path (anything else: D = 3 puts rows at
// 12-byte steps) give every thread the same 4 columns and the same rows, so they add the same values in the same order.
//
// max / min carry (value, row) pairs through the same strands, tree and combine.  The winner is the extreme under one total order --
// a NaN beats every number, equal values (and two NaNs) go to the LOWER row -- so it does not depend on R, S or the tree; rows_out
// (G, D) int32 holds the winning row of the packed batch.
//
// Every element of out / rows_out is written by a kernel (the rows of empty graphs and the columns past the last multiple of 4 included).
// The chunk tables are built by the host from the offsets it already holds (egnn_pytorch_amd.GraphSegments caches them on the device):
// no launch reads anything back.  Entries out of range are clamped into the arrays, like knn_segments.hip does.
#include "segment_core.h"

namespace {

constexpr int SR_NONE = 0x7fffffff;                      // the row of a pair that holds no candidate yet
enum { SR_SUM = 0, SR_MEAN = 1, SR_MAX = 2, SR_MIN = 3 };

// does (av, ar) beat (bv, br)?  One total order: a pair without a candidate loses; a NaN beats every number; equal values and two NaNs
// go to the lower row.  Written as one boolean expression and applied with selects, so the kernels hold no divergent branch here.
template <typename T, bool MAX>
__device__ __forceinline__ bool sr_beats(T av, int ar, T bv, int br)
{
    const bool a_in = ar != SR_NONE, b_in = br != SR_NONE;
    const bool an = av != av, bn = bv != bv;
    const bool further = MAX ? av > bv : av < bv;                    // (false when either is a NaN)
    const bool level = av == bv || (an && bn);
    const bool value_wins = (an && !bn) || further;
    return a_in && (!b_in || value_wins || (level && ar < br));
}

template <typename T, bool VEC>
__global__ __launch_bounds__(SR_THREADS) void segment_sum_chunks_kernel(
    const T* __restrict__ x, int64_t ld, const int64_t* __restrict__ offsets, const int32_t* __restrict__ chunk_row,
    const int32_t* __restrict__ chunk_seg, const int32_t* __restrict__ chunk_slot, int G, int64_t NT, int D, int tcl, int n_slots,
    int mean, T* __restrict__ out, T* __restrict__ part)
{
    __shared__ T sm[4 * SR_THREADS];
    const int tid = threadIdx.x, S = SR_THREADS >> tcl;
    const int s = tid >> tcl, c = (((int)blockIdx.y << tcl) + (tid & ((1 << tcl) - 1))) * 4;
    const SrChunk k = sr_chunk(offsets, chunk_row, chunk_seg, (int)blockIdx.x, G, NT);
    T acc[4] = {T(0), T(0), T(0), T(0)};
    if (c < D) {
        const T* p = x + k.r0 * ld + c;
#pragma unroll 4
        for (int r = s; r < k.m; r += S) {
            T v[4];
            sr_load4<T, VEC>(p + (int64_t)r * ld, c, D, T(0), v);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] += v[u];
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) sm[u * SR_THREADS + tid] = acc[u];
    for (int h = S >> 1; h >= 1; h >>= 1) {
        __syncthreads();
        if (s < h) {                                     // (reads strands [h, 2h), writes strands [0, h): disjoint within a round)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc[u] += sm[u * SR_THREADS + tid + (h << tcl)];
                sm[u * SR_THREADS + tid] = acc[u];
            }
        }
    }
    if (s != 0 || c >= D) return;
    const int slot = chunk_slot[(int)blockIdx.x];
    if (slot < 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (c + u < D) out[(int64_t)k.seg * D + c + u] = mean ? (k.n > 0 ? acc[u] / (T)k.n : T(0)) : acc[u];
    } else if (slot < n_slots) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (c + u < D) part[(int64_t)slot * D + c + u] = acc[u];
    }
}

template <typename T, bool VEC, bool MAX>
__global__ __launch_bounds__(SR_THREADS) void segment_ext_chunks_kernel(
    const T* __restrict__ x, int64_t ld, const int64_t* __restrict__ offsets, const int32_t* __restrict__ chunk_row,
    const int32_t* __restrict__ chunk_seg, const int32_t* __restrict__ chunk_slot, int G, int64_t NT, int D, int tcl, int n_slots,
    T* __restrict__ out, int32_t* __restrict__ rows_out, T* __restrict__ part, int32_t* __restrict__ part_rows)
{
    __shared__ T sm[4 * SR_THREADS];
    __shared__ int smr[4 * SR_THREADS];
    const int tid = threadIdx.x, S = SR_THREADS >> tcl;
    const int s = tid >> tcl, c = (((int)blockIdx.y << tcl) + (tid & ((1 << tcl) - 1))) * 4;
    const SrChunk k = sr_chunk(offsets, chunk_row, chunk_seg, (int)blockIdx.x, G, NT);
    T bv[4] = {T(0), T(0), T(0), T(0)};
    int br[4] = {SR_NONE, SR_NONE, SR_NONE, SR_NONE};
    if (c < D) {
        const T* p = x + k.r0 * ld + c;
#pragma unroll 4
        for (int r = s; r < k.m; r += S) {
            T v[4];
            sr_load4<T, VEC>(p + (int64_t)r * ld, c, D, T(0), v);
            const int row = (int)(k.r0 + r);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool take = sr_beats<T, MAX>(v[u], row, bv[u], br[u]);
                bv[u] = take ? v[u] : bv[u];
                br[u] = take ? row : br[u];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) { sm[u * SR_THREADS + tid] = bv[u]; smr[u * SR_THREADS + tid] = br[u]; }
    for (int h = S >> 1; h >= 1; h >>= 1) {
        __syncthreads();
        if (s < h) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const T ov = sm[u * SR_THREADS + tid + (h << tcl)];
                const int orow = smr[u * SR_THREADS + tid + (h << tcl)];
                const bool take = sr_beats<T, MAX>(ov, orow, bv[u], br[u]);
                bv[u] = take ? ov : bv[u];
                br[u] = take ? orow : br[u];
                sm[u * SR_THREADS + tid] = bv[u];
                smr[u * SR_THREADS + tid] = br[u];
            }
        }
    }
    if (s != 0 || c >= D) return;
    const int slot = chunk_slot[(int)blockIdx.x];
    if (slot < 0) {                                      // (an empty segment -- refused by the caller -- writes 0 and row -1)
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (c + u < D) {
                out[(int64_t)k.seg * D + c + u] = bv[u];
                rows_out[(int64_t)k.seg * D + c + u] = br[u] == SR_NONE ? -1 : br[u];
            }
    } else if (slot < n_slots) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (c + u < D) { part[(int64_t)slot * D + c + u] = bv[u]; part_rows[(int64_t)slot * D + c + u] = br[u]; }
    }
}

// the partials of one segment longer than R, in chunk order; one thread per (segment, column)
template <typename T, int OP>
__global__ __launch_bounds__(SR_THREADS) void segment_combine_kernel(
    const T* __restrict__ part, const int32_t* __restrict__ part_rows, const int64_t* __restrict__ offsets,
    const int32_t* __restrict__ multi_seg, const int32_t* __restrict__ multi_slot, int G, int D, int n_slots,
    T* __restrict__ out, int32_t* __restrict__ rows_out)
{
    const int c = (int)blockIdx.y * SR_THREADS + threadIdx.x;
    if (c >= D) return;
    const int sg = multi_seg[blockIdx.x];
    const int seg = sg < 0 ? 0 : (sg >= G ? G - 1 : sg);
    const int64_t n = offsets[seg + 1] - offsets[seg];
    int slot0 = multi_slot[blockIdx.x];
    slot0 = slot0 < 0 ? 0 : (slot0 >= n_slots ? n_slots - 1 : slot0);
    int64_t nch = (n + SR_ROWS - 1) / SR_ROWS;
    nch = nch < 1 ? 1 : (nch > n_slots - slot0 ? n_slots - slot0 : nch);
    const T* p = part + (int64_t)slot0 * D + c;
    if constexpr (OP == SR_SUM || OP == SR_MEAN) {
        T acc = p[0];
        int64_t q = 1;
        for (; q + 16 <= nch; q += 16) {                 // sixteen loads in flight (the walk is latency-bound), added in chunk order
            T v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = p[(q + u) * D];
#pragma unroll
            for (int u = 0; u < 16; ++u) acc += v[u];
        }
        for (; q < nch; ++q) acc += p[q * D];
        out[(int64_t)seg * D + c] = OP == SR_MEAN ? (n > 0 ? acc / (T)n : T(0)) : acc;
    } else {
        const int32_t* pr = part_rows + (int64_t)slot0 * D + c;
        T bv = p[0];
        int br = pr[0];
        for (int64_t q = 1; q < nch; ++q) {
            const T ov = p[q * D];
            const int orow = pr[q * D];
            const bool take = sr_beats<T, OP == SR_MAX>(ov, orow, bv, br);
            bv = take ? ov : bv;
            br = take ? orow : br;
        }
        out[(int64_t)seg * D + c] = bv;
        rows_out[(int64_t)seg * D + c] = br == SR_NONE ? -1 : br;
    }
}

// out[t, :] = g[segment_of[t], :]: consecutive threads write consecutive elements
template <typename T>
__global__ __launch_bounds__(SR_THREADS) void segment_broadcast_kernel(const T* __restrict__ g, const int32_t* __restrict__ segment_of, int G,
                                                                       int D, int64_t total, T* __restrict__ out)
{
    for (int64_t o = (int64_t)blockIdx.x * SR_THREADS + threadIdx.x; o < total; o += (int64_t)gridDim.x * SR_THREADS) {
        const int64_t t = o / D;
        const int c = (int)(o - t * D);
        const int sg = segment_of[t];
        const int seg = sg < 0 ? 0 : (sg >= G ? G - 1 : sg);
        out[o] = g[(int64_t)seg * D + c];
    }
}

// out[t, c] = g[seg, c] where t is the winning row of (seg = segment_of[t], c), else 0: every element is stored once, by its own thread
template <typename T>
__global__ __launch_bounds__(SR_THREADS) void segment_scatter_rows_kernel(const T* __restrict__ g, const int32_t* __restrict__ rows,
                                                                          const int32_t* __restrict__ segment_of, int G, int D, int64_t total,
                                                                          T* __restrict__ out)
{
    for (int64_t o = (int64_t)blockIdx.x * SR_THREADS + threadIdx.x; o < total; o += (int64_t)gridDim.x * SR_THREADS) {
        const int64_t t = o / D;
        const int c = (int)(o - t * D);
        const int sg = segment_of[t];
        const int seg = sg < 0 ? 0 : (sg >= G ? G - 1 : sg);
        const int64_t q = (int64_t)seg * D + c;
        out[o] = (int64_t)rows[q] == t ? g[q] : T(0);
    }
}

// out[seg, c] = x[rows[seg, c], c] (0 where rows holds no row)
template <typename T>
__global__ __launch_bounds__(SR_THREADS) void segment_gather_rows_kernel(const T* __restrict__ x, const int32_t* __restrict__ rows, int D,
                                                                         int64_t NT, int64_t total, T* __restrict__ out)
{
    for (int64_t o = (int64_t)blockIdx.x * SR_THREADS + threadIdx.x; o < total; o += (int64_t)gridDim.x * SR_THREADS) {
        const int c = (int)(o % D);
        const int64_t r = rows[o];
        out[o] = (r >= 0 && r < NT) ? x[r * D + c] : T(0);
    }
}

unsigned sr_flat_blocks(int64_t total)
{
    int64_t blocks = (total + SR_THREADS - 1) / SR_THREADS;
    return (unsigned)(blocks > 65536 ? 65536 : blocks);
}

template <typename T>
int segment_reduce(const T* x, int64_t ldx, const int64_t* offsets, const int32_t* chunk_row, const int32_t* chunk_seg,
                   const int32_t* chunk_slot, int n_chunks, const int32_t* multi_seg, const int32_t* multi_slot, int n_multi, int G,
                   int64_t NT, int D, int op, T* out, int32_t* rows_out, void* workspace, size_t workspace_bytes, void* stream)
{
    if (!x || !offsets || !chunk_row || !chunk_seg || !chunk_slot || !out) return EGNN_E_NULLPTR;
    if (n_multi > 0 && (!multi_seg || !multi_slot || !workspace)) return EGNN_E_NULLPTR;
    if ((op == SR_MAX || op == SR_MIN) && !rows_out) return EGNN_E_NULLPTR;
    if (G <= 0 || NT <= 0 || D <= 0 || ldx < D || n_chunks < G || n_multi < 0 || n_multi > n_chunks) return EGNN_E_SHAPE;
    if (op < SR_SUM || op > SR_MIN || NT > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;
    if (n_multi > 0 && workspace_bytes < sr_workspace_bytes(G, NT, D, sizeof(T))) return EGNN_E_SHAPE;
    if (n_multi > 0 && (reinterpret_cast<uintptr_t>(workspace) & 15)) return EGNN_E_ALIGN;
    const int tcl = sr_col_threads_log2(D);
    const int64_t tiles = ((int64_t)D + (4 << tcl) - 1) / (4 << tcl);
    if (tiles > 65535 || ((int64_t)D + SR_THREADS - 1) / SR_THREADS > 65535) return EGNN_E_UNSUPPORTED;
    const int n_slots = n_multi > 0 ? (int)sr_slots(G, NT) : 0;
    T* part = static_cast<T*>(workspace);
    int32_t* part_rows = n_multi > 0 ? reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + sr_up256((size_t)n_slots * D * sizeof(T)))
                                     : nullptr;
    const bool vec = D % 4 == 0 && (ldx * (int64_t)sizeof(T)) % 16 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n_chunks, (unsigned)tiles), cgrid((unsigned)n_multi, (unsigned)((D + SR_THREADS - 1) / SR_THREADS));
    if (op == SR_SUM || op == SR_MEAN) {
        auto kern = vec ? segment_sum_chunks_kernel<T, true> : segment_sum_chunks_kernel<T, false>;
        hipLaunchKernelGGL(kern, grid, dim3(SR_THREADS), 0, st, x, ldx, offsets, chunk_row, chunk_seg, chunk_slot, G, NT, D, tcl, n_slots,
                           (int)(op == SR_MEAN), out, part);
    } else {
        auto kern = op == SR_MAX ? (vec ? segment_ext_chunks_kernel<T, true, true> : segment_ext_chunks_kernel<T, false, true>)
                                 : (vec ? segment_ext_chunks_kernel<T, true, false> : segment_ext_chunks_kernel<T, false, false>);
        hipLaunchKernelGGL(kern, grid, dim3(SR_THREADS), 0, st, x, ldx, offsets, chunk_row, chunk_seg, chunk_slot, G, NT, D, tcl, n_slots,
                           out, rows_out, part, part_rows);
    }
    int rc = egnn_launch_status();
    if (rc || n_multi == 0) return rc;
    auto comb = op == SR_SUM ? segment_combine_kernel<T, SR_SUM>
              : op == SR_MEAN ? segment_combine_kernel<T, SR_MEAN>
              : op == SR_MAX ? segment_combine_kernel<T, SR_MAX> : segment_combine_kernel<T, SR_MIN>;
    hipLaunchKernelGGL(comb, cgrid, dim3(SR_THREADS), 0, st, part, part_rows, offsets, multi_seg, multi_slot, G, D, n_slots, out, rows_out);
    return egnn_launch_status();
}

template <typename T>
int segment_broadcast(const T* g, const int32_t* segment_of, int G, int64_t NT, int D, T* out, void* stream)
{
    if (!g || !segment_of || !out) return EGNN_E_NULLPTR;
    if (G <= 0 || NT <= 0 || D <= 0) return EGNN_E_SHAPE;
    if (NT > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;
    const int64_t total = NT * D;
    hipLaunchKernelGGL(segment_broadcast_kernel<T>, dim3(sr_flat_blocks(total)), dim3(SR_THREADS), 0, static_cast<hipStream_t>(stream), g,
                       segment_of, G, D, total, out);
    return egnn_launch_status();
}

template <typename T>
int segment_scatter_rows(const T* g, const int32_t* rows, const int32_t* segment_of, int G, int64_t NT, int D, T* out, void* stream)
{
    if (!g || !rows || !segment_of || !out) return EGNN_E_NULLPTR;
    if (G <= 0 || NT <= 0 || D <= 0) return EGNN_E_SHAPE;
    if (NT > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;
    const int64_t total = NT * D;
    hipLaunchKernelGGL(segment_scatter_rows_kernel<T>, dim3(sr_flat_blocks(total)), dim3(SR_THREADS), 0, static_cast<hipStream_t>(stream), g,
                       rows, segment_of, G, D, total, out);
    return egnn_launch_status();
}

template <typename T>
int segment_gather_rows(const T* x, const int32_t* rows, int G, int64_t NT, int D, T* out, void* stream)
{
    if (!x || !rows || !out) return EGNN_E_NULLPTR;
    if (G <= 0 || NT <= 0 || D <= 0) return EGNN_E_SHAPE;
    if (NT > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;
    const int64_t total = (int64_t)G * D;
    hipLaunchKernelGGL(segment_gather_rows_kernel<T>, dim3(sr_flat_blocks(total)), dim3(SR_THREADS), 0, static_cast<hipStream_t>(stream), x,
                       rows, D, NT, total, out);
    return egnn_launch_status();
}

}  // namespace

extern "C" int egnn_segment_reduce_chunk_rows(void) { return SR_ROWS; }

extern "C" size_t egnn_segment_reduce_workspace_bytes(int G, int64_t T, int D, int elem_bytes)
{
    if (G <= 0 || T <= 0 || D <= 0 || (elem_bytes != 4 && elem_bytes != 8)) return 0;
    return sr_workspace_bytes(G, T, D, (size_t)elem_bytes);
}

extern "C" int egnn_segment_reduce_f32(const float* x, int64_t ldx, const int64_t* offsets, const int32_t* chunk_row, const int32_t* chunk_seg,
                                       const int32_t* chunk_slot, int n_chunks, const int32_t* multi_seg, const int32_t* multi_slot,
                                       int n_multi, int G, int64_t T, int D, int op, float* out, int32_t* rows_out, void* workspace,
                                       size_t workspace_bytes, void* stream)
{
    return segment_reduce<float>(x, ldx, offsets, chunk_row, chunk_seg, chunk_slot, n_chunks, multi_seg, multi_slot, n_multi, G, T, D, op, out,
                                 rows_out, workspace, workspace_bytes, stream);
}

extern "C" int egnn_segment_reduce_f64(const double* x, int64_t ldx, const int64_t* offsets, const int32_t* chunk_row, const int32_t* chunk_seg,
                                       const int32_t* chunk_slot, int n_chunks, const int32_t* multi_seg, const int32_t* multi_slot,
                                       int n_multi, int G, int64_t T, int D, int op, double* out, int32_t* rows_out, void* workspace,
                                       size_t workspace_bytes, void* stream)
{
    return segment_reduce<double>(x, ldx, offsets, chunk_row, chunk_seg, chunk_slot, n_chunks, multi_seg, multi_slot, n_multi, G, T, D, op, out,
                                  rows_out, workspace, workspace_bytes, stream);
}

extern "C" int egnn_segment_broadcast_f32(const float* g, const int32_t* segment_of, int G, int64_t T, int D, float* out, void* stream)
{
    return segment_broadcast<float>(g, segment_of, G, T, D, out, stream);
}

extern "C" int egnn_segment_broadcast_f64(const double* g, const int32_t* segment_of, int G, int64_t T, int D, double* out, void* stream)
{
    return segment_broadcast<double>(g, segment_of, G, T, D, out, stream);
}

extern "C" int egnn_segment_scatter_rows_f32(const float* g, const int32_t* rows, const int32_t* segment_of, int G, int64_t T, int D,
                                             float* out, void* stream)
{
    return segment_scatter_rows<float>(g, rows, segment_of, G, T, D, out, stream);
}

extern "C" int egnn_segment_scatter_rows_f64(const double* g, const int32_t* rows, const int32_t* segment_of, int G, int64_t T, int D,
                                             double* out, void* stream)
{
    return segment_scatter_rows<double>(g, rows, segment_of, G, T, D, out, stream);
}

extern "C" int egnn_segment_gather_rows_f32(const float* x, const int32_t* rows, int G, int64_t T, int D, float* out, void* stream)
{
    return segment_gather_rows<float>(x, rows, G, T, D, out, stream);
}

extern "C" int egnn_segment_gather_rows_f64(const double* x, const int32_t* rows, int G, int64_t T, int D, double* out, void* stream)
{
    return segment_gather_rows<double>(x, rows, G, T, D, out, stream);
}

// k-NN selection with a row's keys in LDS (gfx950): graphs beyond what a wave keeps in registers (knn_select.hip: 8192 nodes with 3-D
// coordinates, 4096 otherwise), float coordinates with more than 8 components, and every double call (egnn_knn_select_f64) -- up to
// the N whose keys fit 160 KiB; beyond that the streaming kernel (knn_stream.hip), which recomputes the keys on every pass.
//
// One WORKGROUP per query row.  The row's N ranking keys (knn_core.h::egnn_knn_key_of: the same bit-exact values as every other
// selection kernel) are computed once into LDS; the K-th smallest key by bitwise radix descent (per-thread counts over a contiguous
// slice, wave sums, one cross-wave sum per step), the index-ordered pick among the ties with the K-th key through a block-wide
// exclusive scan, the K selected written in (key, index) order.  Coordinates are read from global memory (a graph's coordinates are
// L2-resident).  Deterministic, same tie policy; ~10 us per row, rows spread over the chip: a rarely used path (the reference's topk
// has no size limit, egnn_pytorch.py:258), not a fast one.
#include "knn_core.h"

namespace {

constexpr int KR_THREADS = 256, KR_WAVES = KR_THREADS / 64;

// CDM: 3 = egnn_sqdist (float, C == 3), 8 = egnn_sqdist_n<8> (float, C <= 8), the query's coordinates in registers;
//      0 = egnn_sqdist_any through pointers (float C > 8, every double C)
template <typename T, int CDM>
__global__ __launch_bounds__(KR_THREADS) void knn_select_rows_kernel(
    const T* __restrict__ coors, const uint8_t* __restrict__ mask, const uint8_t* __restrict__ adj, int64_t adj_bstride,
    int N, int K, int Cdim, int32_t* __restrict__ idx_out, T* __restrict__ rank_out)
{
    typedef typename egnn_knn_key<T>::type key_t;
    constexpr int BITS = 8 * (int)sizeof(key_t);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    key_t* keys = reinterpret_cast<key_t*>(smem);                        // [N]
    key_t* selk = keys + N;                                              // [K] keys of the selected
    int* selj = reinterpret_cast<int*>(selk + K);                        // [K] their indices
    int* red = selj + K;                                                 // [2 * KR_WAVES]
    const int C = (CDM == 3) ? 3 : Cdim;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, i = blockIdx.x;
    const T* cb = coors + (size_t)b * N * C;
    const uint8_t* mb = mask ? mask + (size_t)b * N : nullptr;
    const bool mi = mb ? mb[i] != 0 : true;
    const uint8_t* adjrow = adj ? adj + (size_t)b * adj_bstride + (size_t)i * N : nullptr;
    const size_t obase = ((size_t)b * N + i) * K;
    if (!mi && !adjrow) {
        // a masked (padded) row: every pair is masked, the whole ranking row is 1e5 (:240-242) and the selection the first K indices
        for (int k = tid; k < K; k += KR_THREADS) { idx_out[obase + k] = k; rank_out[obase + k] = (T)1e5; }
        return;
    }
    constexpr int CR = CDM == 0 ? 1 : CDM;
    T ci[CR];
#pragma unroll
    for (int c = 0; c < CR; ++c) ci[c] = (CDM != 0 && c < C) ? cb[(size_t)i * C + c] : (T)0;
    const T* qi = CDM == 0 ? cb + (size_t)i * C : ci;
    for (int j = tid; j < N; j += KR_THREADS)
        keys[j] = egnn_knn_key_of<T, CDM>(qi, cb + (size_t)j * C, 1, C, mi, mb, adjrow, i, j);
    __syncthreads();

    // block-wide sum of a per-thread count (every thread gets it)
    auto block_sum = [&](int v, int slot) {
        v = egnn_wave_sum(v);
        if (lane == 0) red[slot * KR_WAVES + wave] = v;
        __syncthreads();
        int t = 0;
#pragma unroll
        for (int w = 0; w < KR_WAVES; ++w) t += red[slot * KR_WAVES + w];
        return t;
    };
    // contiguous slice of candidate indices per thread (index order = thread order: the tie pick below relies on it)
    const int per = (N + KR_THREADS - 1) / KR_THREADS;
    const int j0 = tid * per < N ? tid * per : N, j1 = (j0 + per) < N ? (j0 + per) : N;

    // ---- exact K-th smallest key Tk by bitwise radix descent
    key_t Tk = 0;
    int below = 0;
    for (int bit = BITS - 1; bit >= 0; --bit) {
        const key_t want = Tk >> bit;
        int cnt = 0;
        for (int j = j0; j < j1; ++j) cnt += (keys[j] >> bit) == want ? 1 : 0;
        cnt = block_sum(cnt, bit & 1);                                   // (alternating slots: one barrier per step)
        if (below + cnt < K) {
            below += cnt;
            Tk |= ((key_t)1 << bit);
        }
    }
    // ---- pick: everything below Tk, then the lowest-index `need` candidates equal to Tk
    const int need = K - below;
    int nless = 0, neq = 0;
    for (int j = j0; j < j1; ++j) {
        nless += keys[j] < Tk ? 1 : 0;
        neq += keys[j] == Tk ? 1 : 0;
    }
    // exclusive scans over the threads (wave scan + cross-wave offsets)
    __syncthreads();
    const int il = egnn_wave_inclusive_scan(nless), ie = egnn_wave_inclusive_scan(neq);
    if (lane == 63) { red[wave] = il; red[KR_WAVES + wave] = ie; }
    __syncthreads();
    int pl = il - nless, pe = ie - neq;
    for (int w = 0; w < wave; ++w) { pl += red[w]; pe += red[KR_WAVES + w]; }
    // selected entries: the `below` smaller ones first (any order), then the ties in index order
    for (int j = j0; j < j1; ++j) {
        const key_t kj = keys[j];
        if (kj < Tk) { selk[pl] = kj; selj[pl] = j; ++pl; }
        else if (kj == Tk) {
            if (pe < need) { selk[below + pe] = kj; selj[below + pe] = j; }
            ++pe;
        }
    }
    __syncthreads();
    egnn_knn_write_sorted<T>(selk, selj, K, K, tid, KR_THREADS, 0, idx_out + obase, rank_out + obase);
}

// (arguments checked by the entry)
template <typename T>
int knn_rows_launch(const T* coors, const uint8_t* mask, const uint8_t* adj, int64_t adj_bstride, int B, int N, int K, int C,
                    int32_t* idx_out, T* rank_out, void* stream)
{
    typedef typename egnn_knn_key<T>::type key_t;
    const size_t lds = ((size_t)N * sizeof(key_t) + 7) / 8 * 8 + (size_t)K * (sizeof(key_t) + 4) + 2 * KR_WAVES * sizeof(int) + 8;
    if (lds > 160 * 1024) {                                               // N > ~ 20 000 (double) / 40 000 (float): keys recomputed per pass
        if constexpr (sizeof(T) == 8) return egnn_knn_select_stream_f64(coors, mask, adj, adj_bstride, B, N, K, C, idx_out, rank_out, stream);
        else return egnn_knn_select_stream_f32(coors, mask, adj, adj_bstride, B, N, K, C, idx_out, rank_out, stream);
    }
    auto kern = knn_select_rows_kernel<T, 0>;
    if constexpr (sizeof(T) == 4) {
        if (C == 3) kern = knn_select_rows_kernel<T, 3>;
        else if (C <= 8) kern = knn_select_rows_kernel<T, 8>;
    }
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3(N, B), dim3(KR_THREADS), lds, static_cast<hipStream_t>(stream), coors, mask, adj, adj_bstride, N, K, C,
                       idx_out, rank_out);
    return egnn_launch_status();
}

}  // namespace

// internal (knn_select.hip: egnn_knn_select_f32 beyond the register kernel's N, or with more than 8 coordinates)
int egnn_knn_select_rows_f32(const float* coors, const uint8_t* mask, const uint8_t* adj, int64_t adj_batch_stride, int B, int N, int K,
                             int coor_dim, int32_t* idx_out, float* rank_out, void* stream)
{
    return knn_rows_launch<float>(coors, mask, adj, adj_batch_stride, B, N, K, coor_dim, idx_out, rank_out, stream);
}

extern "C" int egnn_knn_select_f64(const double* coors, const uint8_t* mask, const uint8_t* adj, int64_t adj_batch_stride, int B, int N,
                                   int K, int coor_dim, int32_t* idx_out, double* rank_out, void* stream)
{
    const int rc = egnn_knn_check_args(coors, idx_out, rank_out, B, N, K, coor_dim);
    if (rc != EGNN_OK) return rc;
    return knn_rows_launch<double>(coors, mask, adj, adj_batch_stride, B, N, K, coor_dim, idx_out, rank_out, stream);
}

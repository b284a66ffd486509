// Streaming k-NN selection (gfx950): rows whose ranking keys do not fit in LDS -- graphs beyond the one-workgroup-per-row kernels
// (knn_rows.hip: 32 768 nodes with C <= 8; otherwise ~40 000 (float) / ~20 000 (double) nodes).  The reference's topk
// (egnn_pytorch.py:258) has no size limit.
//
// No key is stored.  Every pass recomputes a row's N ranking values from the coordinates, the mask and the adjacency row (the same
// operations as the other selection kernels: knn_core.h::egnn_knn_key_of); the
// graph's coordinates stay in L2.  Selection is a radix select over 8-bit digits of the composite (key, index) -- the key's digits
// first, then the index's -- which is unique per candidate, so the K smallest composites are exactly the top-K with the lowest-index
// tie policy and no index-ordered scan is needed:
//   pass:  every candidate whose composite matches the row's resolved prefix bumps the LDS histogram bin of its next digit;
//          the bin holding the K-th smallest becomes the prefix's next digit.  A row is resolved once that bin holds exactly as many
//          candidates as are still missing (distinct distances: after 2-3 passes; all digits in the worst case -- 4 + 1..4 passes
//          for float keys, 8 + 1..4 for double keys).
//   pick:  every candidate whose composite prefix is <= the resolved one (exactly K) is appended to the row's LDS list (integer
//          slot atomics: the list's order varies, its content does not), then ranked by counting on (key, index).
// R query rows per workgroup share every pass (R histograms in LDS; lane l works for row l % R on the candidates j = l / R + S t,
// S = 256 / R), so the coordinate stream is read once for R rows.  Deterministic: only integer counters are atomic, and the output
// order is the (key, index) order.
// Instantiations: the adjacency as a byte row or as CSR rows (CSR), every row or only the rows a flag byte names (FL: the rows the cell-grid
// selection hands over, knn_grid.hip) -- all four combinations; `rowflag` and `col` are separate arguments.
#include "knn_core.h"

namespace {

constexpr int KS_THREADS = 256;
constexpr int KS_RMAX = 16;                 // query rows per workgroup (fewer for large K: the pick lists live in LDS)
constexpr int KS_HSTRIDE = 257;             // histogram row stride (words): rows' equal bins on different banks

// CDM: 3 = egnn_sqdist (float, C == 3), 8 = egnn_sqdist_n (float, C <= 8), 0 = egnn_sqdist_any (float C > 8, every double C)
// FL: only the rows with rowflag[b N + i] != 0 are selected and written (the rows the cell-grid selection hands over, knn_grid.hip); a
// workgroup without such a row returns at once.  Instantiated for C == 3: <float, 3> and, for the float64 grid, <double, 0>.
// CSR: the adjacency as sorted column ranges (egnn_knn_select_csr_f32 / _f64) -- adj = rowptr, int64 absolute offsets, (N + 1) per graph
// at a graph stride of adj_bstride entries (0: one graph's rows for all); col = the flat int32 column array (NULL without CSR).  Every
// row then has an adjacency; its ranking values come from the merging overload of egnn_knn_rank.
// FL and CSR together: the rows the cell-grid selection with CSR rows hands over (egnn_knn_select_grid_csr_f32) -- masked rows
// included, which have an adjacency like every other row.
template <bool CSR> struct KsAdj { typedef uint8_t adj_t; };
template <> struct KsAdj<true> { typedef int64_t adj_t; };

template <typename T, int CDM, bool FL = false, bool CSR = false>
__global__ __launch_bounds__(KS_THREADS) void knn_select_stream_kernel(
    const T* __restrict__ coors, const uint8_t* __restrict__ mask, const typename KsAdj<CSR>::adj_t* __restrict__ adj, int64_t adj_bstride,
    int N, int K, int C, int R, int IBP, int32_t* __restrict__ idx_out, T* __restrict__ rank_out,
    const uint8_t* __restrict__ rowflag, const int32_t* __restrict__ col)
{
    typedef typename egnn_knn_key<T>::type key_t;
    constexpr int KD = (int)sizeof(key_t);               // key digits
    extern __shared__ __attribute__((aligned(16))) char smem[];
    key_t* pk = reinterpret_cast<key_t*>(smem);                          // [KS_RMAX] resolved key prefix (right-aligned)
    uint32_t* pj = reinterpret_cast<uint32_t*>(pk + KS_RMAX);           // [KS_RMAX] resolved index prefix
    int* lvl = reinterpret_cast<int*>(pj + KS_RMAX);                     // [KS_RMAX] digits resolved
    int* need = lvl + KS_RMAX;                                           // [KS_RMAX] candidates still missing in the prefix's bin
    int* state = need + KS_RMAX;                                         // [KS_RMAX] 0 = selecting, 1 = resolved, 2 = no work
    int* cnt = state + KS_RMAX;                                          // [KS_RMAX] pick list fill
    int* active = cnt + KS_RMAX;                                         // [1] rows still selecting
    int* hist = active + 4;                                              // [R][KS_HSTRIDE]
    key_t* selk = reinterpret_cast<key_t*>(hist + ((R * KS_HSTRIDE + 1) & ~1));      // [R][K] (8-byte aligned)
    int* selj = reinterpret_cast<int*>(selk + (size_t)R * K);            // [R][K]
    T* qs = reinterpret_cast<T*>(selj + (size_t)R * K + (((size_t)R * K) & 1));       // [R][C] query coordinates (CDM == 0)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y;
    const int S = KS_THREADS / R;
    const int r = tid % R, s = tid / R;
    const int i = blockIdx.x * R + r;
    const T* cb = coors + (size_t)b * N * C;
    const uint8_t* mb = mask ? mask + (size_t)b * N : nullptr;
    const bool mi = (i < N && mb) ? mb[i] != 0 : true;
    bool fl = true;
    if constexpr (FL) {
        bool any = false;
        for (int rr = 0; rr < R; ++rr) {
            const int ir = blockIdx.x * R + rr;
            any = any || (ir < N && rowflag[(size_t)b * N + ir] != 0);
        }
        if (!any) return;                                                // (the same for every thread of the workgroup)
        fl = i < N && rowflag[(size_t)b * N + i] != 0;
    }
    // (CSR: adjrow only says that the row has an adjacency -- never read; the row itself is the cursor's column range)
    const uint8_t* adjrow;
    egnn_csr_cursor csr = {nullptr, 0, 0, 0x7fffffff};
    if constexpr (CSR) {
        adjrow = i < N ? reinterpret_cast<const uint8_t*>(adj) : nullptr;
        if (i < N) {
            const int64_t* rp = adj + (size_t)b * adj_bstride + i;
            const int64_t lo = rp[0];
            csr.col = col + lo;
            csr.len = (int)(rp[1] - lo);
        }
    } else {
        adjrow = (adj && i < N) ? adj + (size_t)b * adj_bstride + (size_t)i * N : nullptr;
    }

    for (int o = tid; o < R * KS_HSTRIDE; o += KS_THREADS) hist[o] = 0;
    if (s == 0) {
        pk[r] = 0;
        pj[r] = 0u;
        lvl[r] = 0;
        need[r] = K;
        cnt[r] = 0;
        state[r] = (i >= N || !fl || (!mi && !adjrow)) ? 2 : 0;
    }
    if (tid == 0) *active = 0;
    if constexpr (CDM == 0) {
        for (int o = tid; o < R * C; o += KS_THREADS) {
            const int ir = blockIdx.x * R + o / C;
            qs[o] = ir < N ? cb[(size_t)ir * C + o % C] : (T)0;
        }
    }
    __syncthreads();
    if (s == 0 && state[r] == 0) atomicAdd(active, 1);
    // a masked row without an adjacency: every pair is masked, the ranking row is all 1e5 and the selection the first K indices
    if (i < N && fl && !mi && !adjrow) {
        const size_t ob = ((size_t)b * N + i) * K;
        for (int k = s; k < K; k += S) { idx_out[ob + k] = k; rank_out[ob + k] = (T)1e5; }
    }
    constexpr int CR = CDM == 0 ? 1 : CDM;
    T ci[CR];
#pragma unroll
    for (int c = 0; c < CR; ++c) ci[c] = (CDM != 0 && c < C && i < N) ? cb[(size_t)i * C + c] : (T)0;
    const T* qi = CDM == 0 ? qs + (size_t)r * C : ci;

    const int CJ = CDM == 3 ? 3 : C;                                     // a node's coordinates in memory (a constant where CDM fixes it)
    auto key_of = [&](int j) -> key_t {
        if constexpr (CSR) return egnn_knn_key_of<T, CDM>(qi, cb + (size_t)j * CJ, 1, C, mi, mb, csr, i, j);
        else return egnn_knn_key_of<T, CDM>(qi, cb + (size_t)j * CJ, 1, C, mi, mb, adjrow, i, j);
    };
    __syncthreads();

    // ---- radix passes (the workgroup loops while any of its rows is unresolved; `active` is read behind a barrier)
    while (*active > 0) {
        const int L = lvl[r];
        const bool mine = state[r] == 0;
        const key_t P = pk[r];
        const uint32_t PJ = pj[r];
        if (mine) {
            int* h = hist + r * KS_HSTRIDE;
            if constexpr (CSR) egnn_csr_rewind(csr);
            for (int j = s; j < N; j += S) {
                const key_t kj = key_of(j);
                if (!egnn_knn_has_prefix(kj, (uint32_t)j, P, PJ, L, IBP)) continue;
                atomicAdd(&h[egnn_knn_digit(kj, (uint32_t)j, L, IBP)], 1);
            }
        }
        __syncthreads();
        // one wave per row: the bin holding the need-th candidate (lane l owns bins 4 l .. 4 l + 3); the bins are cleared behind it
        for (int rr = wave; rr < R; rr += KS_THREADS / 64) {
            if (state[rr] != 0) continue;                                // (wave-uniform)
            int* h = hist + rr * KS_HSTRIDE;
            int c4[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { c4[q] = h[4 * lane + q]; h[4 * lane + q] = 0; }
            const int nd = need[rr];
            egnn_knn_bin bin;
            egnn_knn_find_bin(c4, nd, lane, bin);                        // (found: the row holds >= nd candidates with its prefix)
            if (lane == 0) {
                const int L0 = lvl[rr];
                if (L0 < KD) pk[rr] = (pk[rr] << 8) | (key_t)bin.digit;
                else pj[rr] = (pj[rr] << 8) | (uint32_t)bin.digit;
                lvl[rr] = L0 + 1;
                need[rr] = nd - bin.before;
                if (bin.in_bin == nd - bin.before) { state[rr] = 1; atomicSub(active, 1); }
            }
        }
        __syncthreads();
    }

    // ---- pick: the K candidates whose composite prefix is <= the resolved one, into the row's list
    if (state[r] == 1) {
        const int L = lvl[r];
        const key_t P = pk[r];
        const uint32_t PJ = pj[r];
        key_t* sk = selk + (size_t)r * K;
        int* sj = selj + (size_t)r * K;
        if constexpr (CSR) egnn_csr_rewind(csr);
        for (int j = s; j < N; j += S) {
            const key_t kj = key_of(j);
            if (egnn_knn_take(kj, (uint32_t)j, P, PJ, L, IBP)) {                  // (L >= 1: at least one pass)
                const int pos = atomicAdd(&cnt[r], 1);
                if (pos < K) { sk[pos] = kj; sj[pos] = j; }
            }
        }
    }
    __syncthreads();
    // ---- rank by counting on (key, index)
    for (int o = tid; o < R * K; o += KS_THREADS) {
        const int rr = o / K, t = o - rr * K;
        if (state[rr] != 1) continue;
        const key_t* sk = selk + (size_t)rr * K;
        const int* sj = selj + (size_t)rr * K;
        const key_t mk = sk[t];
        const int mj = sj[t];
        const int rnk = egnn_knn_rank_in(sk, sj, K, mk, mj);
        const size_t ob = ((size_t)b * N + (size_t)blockIdx.x * R + rr) * K;
        idx_out[ob + rnk] = mj;
        rank_out[ob + rnk] = (T)egnn_rank_from_key(mk);
    }
}

template <typename T, bool CSR = false>
int knn_stream_launch(const T* coors, const uint8_t* mask, const typename KsAdj<CSR>::adj_t* adj, int64_t adj_bstride, int B, int N, int K,
                      int C, int32_t* idx_out, T* rank_out, void* stream, const uint8_t* rowflag = nullptr, const int32_t* col = nullptr)
{
    const int rc = egnn_knn_check_args(coors, idx_out, rank_out, B, N, K, C);
    if (rc != EGNN_OK) return rc;
    typedef typename egnn_knn_key<T>::type key_t;
    // rows per workgroup: 16, fewer where the R pick lists ((key, index) per entry) would pass 64 KB
    int R = KS_RMAX;
    while (R > 1 && (size_t)R * K * (sizeof(key_t) + 4) > 64 * 1024) R >>= 1;
    int ibits = 1;                                                       // index digits: ceil(bits(N - 1) / 8) bytes
    while (ibits < 31 && ((int64_t)1 << ibits) < N) ++ibits;
    const int IBP = (ibits + 7) / 8 * 8;
    const size_t head = KS_RMAX * (sizeof(key_t) + 4 + 4 * 5) + 4 * 4;
    const size_t lds = head + (size_t)((R * KS_HSTRIDE + 1) & ~1) * 4 + (size_t)R * K * sizeof(key_t) +
                       ((size_t)R * K + (((size_t)R * K) & 1)) * 4 + (size_t)R * C * sizeof(T);
    auto kern = knn_select_stream_kernel<T, 0, false, CSR>;
    if constexpr (sizeof(T) == 4) {
        if (C == 3) kern = knn_select_stream_kernel<T, 3, false, CSR>;
        else if (C <= 8) kern = knn_select_stream_kernel<T, 8, false, CSR>;
        if (rowflag) {
            if (C != 3) return EGNN_E_UNSUPPORTED;
            kern = knn_select_stream_kernel<T, 3, true, CSR>;
        }
    } else if (rowflag) {                                                // (double: egnn_sqdist_any at every C; the grid is 3-D)
        if (C != 3) return EGNN_E_UNSUPPORTED;
        kern = knn_select_stream_kernel<T, 0, true, CSR>;
    }
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    const dim3 grid((unsigned)((N + R - 1) / R), (unsigned)B);
    hipLaunchKernelGGL(kern, grid, dim3(KS_THREADS), lds, static_cast<hipStream_t>(stream), coors, mask, adj, adj_bstride, N, K, C, R,
                       IBP, idx_out, rank_out, rowflag, col);
    return egnn_launch_status();
}

}  // namespace

int egnn_knn_stream_flagged_f32(const float* coors, const uint8_t* mask, int B, int N, int K, const uint8_t* rowflag, int32_t* idx_out,
                                float* rank_out, void* stream)
{
    if (!rowflag) return EGNN_E_NULLPTR;
    return knn_stream_launch<float>(coors, mask, nullptr, 0, B, N, K, 3, idx_out, rank_out, stream, rowflag);
}

int egnn_knn_stream_flagged_csr_f32(const float* coors, const uint8_t* mask, const int64_t* rowptr, const int32_t* col,
                                    int64_t rowptr_graph_stride, int B, int N, int K, const uint8_t* rowflag, int32_t* idx_out,
                                    float* rank_out, void* stream)
{
    if (!rowflag || !rowptr) return EGNN_E_NULLPTR;
    return knn_stream_launch<float, true>(coors, mask, rowptr, rowptr_graph_stride, B, N, K, 3, idx_out, rank_out, stream, rowflag, col);
}

int egnn_knn_stream_flagged_f64(const double* coors, const uint8_t* mask, int B, int N, int K, const uint8_t* rowflag, int32_t* idx_out,
                                double* rank_out, void* stream)
{
    if (!rowflag) return EGNN_E_NULLPTR;
    return knn_stream_launch<double>(coors, mask, nullptr, 0, B, N, K, 3, idx_out, rank_out, stream, rowflag);
}

int egnn_knn_stream_flagged_csr_f64(const double* coors, const uint8_t* mask, const int64_t* rowptr, const int32_t* col,
                                    int64_t rowptr_graph_stride, int B, int N, int K, const uint8_t* rowflag, int32_t* idx_out,
                                    double* rank_out, void* stream)
{
    if (!rowflag || !rowptr) return EGNN_E_NULLPTR;
    return knn_stream_launch<double, true>(coors, mask, rowptr, rowptr_graph_stride, B, N, K, 3, idx_out, rank_out, stream, rowflag, col);
}

extern "C" int egnn_knn_select_stream_f32(const float* coors, const uint8_t* mask, const uint8_t* adj, int64_t adj_batch_stride, int B,
                                          int N, int K, int coor_dim, int32_t* idx_out, float* rank_out, void* stream)
{
    return knn_stream_launch<float>(coors, mask, adj, adj_batch_stride, B, N, K, coor_dim, idx_out, rank_out, stream);
}

extern "C" int egnn_knn_select_stream_f64(const double* coors, const uint8_t* mask, const uint8_t* adj, int64_t adj_batch_stride, int B,
                                          int N, int K, int coor_dim, int32_t* idx_out, double* rank_out, void* stream)
{
    return knn_stream_launch<double>(coors, mask, adj, adj_batch_stride, B, N, K, coor_dim, idx_out, rank_out, stream);
}

// The same selection with the adjacency as CSR rows (include/egnn_hip.h): the one kernel at every N.
template <typename T>
static int knn_csr(const T* coors, const uint8_t* mask, const int64_t* rowptr, const int32_t* col, int64_t rowptr_graph_stride, int B, int N,
                   int K, int C, int32_t* idx_out, T* rank_out, void* stream)
{
    if (!rowptr) return EGNN_E_NULLPTR;
    if (N > 0 && rowptr_graph_stride != 0 && rowptr_graph_stride != (int64_t)N + 1) return EGNN_E_SHAPE;
    return knn_stream_launch<T, true>(coors, mask, rowptr, rowptr_graph_stride, B, N, K, C, idx_out, rank_out, stream, nullptr, col);
}

extern "C" int egnn_knn_select_csr_f32(const float* coors, const uint8_t* mask, const int64_t* rowptr, const int32_t* col,
                                       int64_t rowptr_graph_stride, int B, int N, int K, int coor_dim, int32_t* idx_out, float* rank_out,
                                       void* stream)
{
    return knn_csr<float>(coors, mask, rowptr, col, rowptr_graph_stride, B, N, K, coor_dim, idx_out, rank_out, stream);
}

extern "C" int egnn_knn_select_csr_f64(const double* coors, const uint8_t* mask, const int64_t* rowptr, const int32_t* col,
                                       int64_t rowptr_graph_stride, int B, int N, int K, int coor_dim, int32_t* idx_out, double* rank_out,
                                       void* stream)
{
    return knn_csr<double>(coors, mask, rowptr, col, rowptr_graph_stride, B, N, K, coor_dim, idx_out, rank_out, stream);
}

// What the k-NN selection kernels (knn_select.hip, knn_rows.hip, knn_stream.hip, knn_segments.hip, knn_grid.hip) agree on, stated once:
// the key of a ranking value, the ranking key of a candidate, the arithmetic of the radix select over the composite (key, index), the
// final order of a selected list, and the argument checks of the entries.  A selection returns its K candidates ascending by key, ties
// by ascending index; every kernel gets that order from the functions below, never from a copy of them.
#pragma once
#include "egnn_common.h"

// The order-preserving unsigned image of a ranking value of type T (egnn_rank_key) and V, the lanes of the vector type whose summation
// tree egnn_sqdist_any follows for T.
template <typename T> struct egnn_knn_key;
template <> struct egnn_knn_key<float> { typedef uint32_t type; static constexpr int V = 8; };
template <> struct egnn_knn_key<double> { typedef uint64_t type; static constexpr int V = 4; };

// Same-wave LDS hand-off: DS operations of one wave execute in issue order; the explicit wait makes the store -> other-lane load
// dependency independent of that, the wave barrier pins the compiler's ordering.
__device__ __forceinline__ void egnn_wave_lds_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// The ranking key of candidate j for query i (egnn_pytorch.py:232-233, 237-256): squared distance, then egnn_knn_rank's edits for the
// mask (mi = the query's bit; mb = the graph's mask bytes, NULL: none -- candidate j's byte is read here, behind the distance, where the
// kernels' schedules had it) and the adjacency -- `adj` is row i as bytes (NULL: none) or as an egnn_csr_cursor -- then egnn_rank_key.
// CDM picks the distance: 3 = egnn_sqdist and 8 = egnn_sqdist_n<8> (float; q = the query's CDM components in registers, zeros beyond
// C), 0 = egnn_sqdist_any (q = the query's C components in memory).  cj = the candidate's first component, the others cstride apart
// (1 in a node-major array; CDM == 0 reads cj[0 .. C) whatever cstride is).
template <typename T, int CDM, typename Adj>
__device__ __forceinline__ typename egnn_knn_key<T>::type egnn_knn_key_of(const T* q, const T* cj, int cstride, int C, bool mi, const uint8_t* __restrict__ mb,
                                                                          Adj&& adj, int i, int j)
{
    T d;
    if constexpr (CDM == 3) {
        float dx, dy, dz;
        d = egnn_sqdist(q[0], q[1], q[2], cj[0], cj[cstride], cj[2 * cstride], dx, dy, dz);
    } else if constexpr (CDM == 8) {
        float a[8], b[8], rel[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            a[c] = q[c];
            b[c] = c < C ? cj[c * cstride] : 0.f;
        }
        d = egnn_sqdist_n<8>(a, b, C, rel);
    } else {
        d = egnn_sqdist_any<T, egnn_knn_key<T>::V>(q, cj, C);
    }
    return egnn_rank_key(egnn_knn_rank<T>(d, mi, mb ? mb[j] != 0 : true, adj, i, j));
}

// ---- radix select over the 8-bit digits of the composite (key, index): the key's digits first, then the index's (IBP bits, a multiple
// of 8).  The composite is unique per candidate, so its K smallest are the selection.  A resolved prefix is (P, PJ, L): L digits, the
// key's in P and the index's in PJ, both right-aligned.
//
// Does (kj, j) carry the prefix?
template <typename key_t>
__device__ __forceinline__ bool egnn_knn_has_prefix(key_t kj, uint32_t j, key_t P, uint32_t PJ, int L, int IBP)
{
    constexpr int KB = 8 * (int)sizeof(key_t), KD = KB / 8;
    const int kl = L < KD ? L : KD, il = L - kl;                        // resolved key / index digits
    if (kl > 0 && (kj >> (KB - 8 * kl)) != P) return false;
    if (il > 0 && (j >> (IBP - 8 * il)) != PJ) return false;
    return true;
}
// Digit L of (kj, j): the one behind a prefix of L digits.
template <typename key_t>
__device__ __forceinline__ int egnn_knn_digit(key_t kj, uint32_t j, int L, int IBP)
{
    constexpr int KB = 8 * (int)sizeof(key_t), KD = KB / 8;
    return L < KD ? (int)((kj >> (KB - 8 * (L + 1))) & 0xff) : (int)((j >> (IBP - 8 * (L - KD + 1))) & 0xffu);
}

// The pick pass's test: is the composite prefix of (kj, j) at or below the resolved one (L >= 1)?
template <typename key_t>
__device__ __forceinline__ bool egnn_knn_take(key_t kj, uint32_t j, key_t P, uint32_t PJ, int L, int IBP)
{
    constexpr int KB = 8 * (int)sizeof(key_t), KD = KB / 8;
    const int kl = L < KD ? L : KD, il = L - kl;
    const key_t kp = kj >> (KB - 8 * kl);
    bool take = kp < P;
    if (kp == P) take = il == 0 || (j >> (IBP - 8 * il)) <= PJ;
    return take;
}

// The bin of a 256-bin histogram that holds the need-th candidate, by one wave: lane l passes the counts of bins 4 l .. 4 l + 3.
// digit = that bin, before = the candidates in the bins below it, in_bin = its own count (wave-uniform).  False when the histogram holds
// fewer than `need`.
struct egnn_knn_bin { int digit, before, in_bin; };
__device__ __forceinline__ bool egnn_knn_find_bin(const int (&c4)[4], int need, int lane, egnn_knn_bin& bin)
{
    int sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) sum += c4[q];
    const int incl = egnn_wave_inclusive_scan(sum);
    const uint64_t hit = __ballot(incl >= need);
    const int src = hit ? __builtin_ctzll(hit) : 0;                     // (no such bin: lane 0 finds none either, in_bin = 0)
    int dig = 0, before = incl - sum, inbin = 0;
    if (lane == src) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (before + c4[q] >= need) { dig = 4 * lane + q; inbin = c4[q]; break; }
            before += c4[q];
        }
    }
    bin.digit = __builtin_amdgcn_readlane(dig, src);
    bin.before = __builtin_amdgcn_readlane(before, src);
    bin.in_bin = __builtin_amdgcn_readlane(inbin, src);
    return hit != 0ull;
}

// ---- the final order: entry (mk, mj) of a list of n distinct (key, index) pairs ranks behind the entries that are smaller by key, then
// by index.
template <typename key_t>
__device__ __forceinline__ int egnn_knn_rank_in(const key_t* sk, const int* sj, int n, key_t mk, int mj)
{
    int rnk = 0;
    for (int u = 0; u < n; ++u) rnk += (sk[u] < mk || (sk[u] == mk && sj[u] < mj)) ? 1 : 0;
    return rnk;
}
// The first `keep` of the n listed pairs, sorted, into a row of the outputs: idx = jbase + index, rank = the key's value.  Entries
// t = first, first + stride, ... are this thread's (a workgroup: threadIdx.x and its size; a wave: the lane and 64).
template <typename T>
__device__ __forceinline__ void egnn_knn_write_sorted(const typename egnn_knn_key<T>::type* sk, const int* sj, int n, int keep, int first,
                                                      int stride, int jbase, int32_t* __restrict__ idx_row, T* __restrict__ rank_row)
{
    for (int t = first; t < n; t += stride) {
        const typename egnn_knn_key<T>::type mk = sk[t];
        const int mj = sj[t];
        const int rnk = egnn_knn_rank_in(sk, sj, n, mk, mj);
        if (keep >= n || rnk < keep) {
            idx_row[rnk] = jbase + mj;
            rank_row[rnk] = (T)egnn_rank_from_key(mk);
        }
    }
}

// ---- the argument checks every all-pairs entry starts with, in the order the entries report them (include/egnn_hip.h)
static inline int egnn_knn_check_args(const void* coors, const void* idx_out, const void* rank_out, int B, int N, int K, int coor_dim)
{
    if (!coors || !idx_out || !rank_out) return EGNN_E_NULLPTR;
    if (B <= 0 || N <= 0 || K <= 0) return EGNN_E_SHAPE;
    if (coor_dim < 1 || coor_dim > 64) return EGNN_E_UNSUPPORTED;
    if (K > N) return EGNN_E_K_GT_N;
    if (K > 1024 || B > 65535) return EGNN_E_UNSUPPORTED;
    return EGNN_OK;
}

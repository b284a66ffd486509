// Segmented k-NN selection (gfx950): a PACKED batch -- the nodes of G graphs concatenated as (T, C), graph g owning the rows
// [offsets[g], offsets[g + 1]) -- ranked graph by graph.  Row i of segment [lo, hi) receives the min(K, hi - lo) candidates j in [lo, hi)
// with the smallest squared distance (the node itself included, at distance 0: egnn_pytorch.py:232-233, 258 on one graph), ascending by
// value, ties by ascending index; idx holds rows of the packed batch (lo + local), so the one-graph kernels downstream gather with them
// unchanged.  Slots k >= hi - lo are empty: idx = i (a safe gather), rank = +inf.  This is what the padded call with a prefix mask
// selects on the real nodes (its padding candidates rank at 1e5, behind every real one), without the padding.
//
// Work: tiles of SG_ROWS consecutive rows of the packed batch, one workgroup (4 waves) per tile, one wave per query row.  A tile does
// not care where graphs begin: segment_of[first row] and segment_of[last row] name the segments it touches, so sixteen 2-node graphs
// share one workgroup and an empty graph costs nothing.  The tile's WINDOW -- the rows [offsets[first segment], ... + W) -- is loaded
// into LDS once and shared by the tile's rows: component-major (SoA, lane l reads x[c W + l]: conflict-free) for float coordinates with
// C <= 8, node-major at an odd stride (C | 1) where the distance walks a node's coordinates through pointers (egnn_sqdist_any: C > 8,
// every double).  A row whose segment lies inside the window reads its candidates from LDS; a row whose segment does not fit streams
// them from memory (the packed coordinates are L2-resident) -- the same code on another source, decided per row, wave-uniform.
//
// Selection (both sources): nothing is stored per candidate.  Radix select over the 8-bit digits of the composite (key, local index)
// -- egnn_rank_key's digits first, then the index's -- knn_stream.hip's, on the same arithmetic (knn_core.h), with one wave and one 256-bin LDS histogram per row:
//   pass:  every candidate whose composite matches the resolved prefix bumps the bin of its next digit (integer LDS atomics); the bin
//          holding the K-th smallest extends the prefix; the row is resolved once that bin holds exactly what is still missing.
//   pick:  the candidates whose composite prefix is <= the resolved one (exactly min(K, n)) are compacted into the wave's list by
//          ballot prefix -- index order, no atomics -- and ranked by counting on (key, index).
// A segment with n <= K skips the passes: every candidate is taken.
// K <= 64 goes a shorter way first (knn_select.hip's pruning, with the keys recomputed instead of held in registers): one walk for the
// smallest key of every lane (K > 32: the two smallest), whose K-th smallest -- found on the keys' leading bits by ballot descent --
// bounds the K-th smallest candidate; a second walk compacts the candidates at or below that bound, typically ~1.3 K of them, into the
// wave's list, where they are ranked by counting and the first K written.  No atomics, two walks instead of three or four.  A row whose
// survivors do not fit the list (heavily tied keys) takes the radix passes after all.
// Deterministic: the output order is the (key, index) order and only integer counters are atomic.
#include "knn_core.h"

namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_WAVES = SG_THREADS / 64;
constexpr int SG_ROWS = 32;                              // query rows per tile (eight per wave)
constexpr size_t SG_LDS_BYTES = 64 * 1024;               // per workgroup: two workgroups per CU at the largest window (160 KiB per CU)

int g_lds_nodes = 0;                                     // egnn_knn_segments_lds_nodes: 0 = the built-in budget

template <bool V> struct SgSrc { static constexpr bool lds = V; };

__host__ __device__ constexpr size_t sg_up8(size_t b) { return (b + 7) / 8 * 8; }
// LDS bytes of one wave's block: the pick list (keys, local indices), the histogram, the query's coordinates (CDM == 0)
template <typename T> __host__ __device__ constexpr size_t sg_wave_bytes(int Lp, int CQ) {
    return sg_up8((size_t)Lp * (sizeof(typename egnn_knn_key<T>::type) + 4) + 256 * 4 + (size_t)CQ * sizeof(T));
}
constexpr int SG_SURVIVORS = 128;                        // the least the pick list holds: what the pruning path may rank (two per lane)

// CDM: 3 = egnn_sqdist (float, C == 3), 8 = egnn_sqdist_n<8> (float, C <= 8), 0 = egnn_sqdist_any (float C > 8, every double C)
// W: nodes of the LDS window (0: every row streams); Lp: entries of a wave's pick list, even, >= max(K, SG_SURVIVORS)
template <typename T, int CDM>
__global__ __launch_bounds__(SG_THREADS) void knn_select_segments_kernel(
    const T* __restrict__ coors, const int64_t* __restrict__ offsets, const int32_t* __restrict__ segment_of, int G, int NT, int K, int C,
    int W, int Lp, int32_t* __restrict__ idx_out, T* __restrict__ rank_out)
{
    typedef typename egnn_knn_key<T>::type key_t;
    constexpr int KB = 8 * (int)sizeof(key_t);           // key bits
    constexpr int KD = KB / 8;                           // key digits
    constexpr int PB = KB / 2;                           // leading key bits the pruning bound resolves (float: sign, exponent, 7 mantissa bits)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int CS = CDM == 0 ? (C | 1) : C;               // node stride of the node-major window
    T* xs = reinterpret_cast<T*>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    char* wb = smem + sg_up8((size_t)W * CS * sizeof(T)) + (size_t)wave * sg_wave_bytes<T>(Lp, CDM == 0 ? C : 0);
    key_t* selk = reinterpret_cast<key_t*>(wb);          // [Lp]
    int* selj = reinterpret_cast<int*>(selk + Lp);       // [Lp]
    int* hist = selj + Lp;                               // [256]
    T* qs = reinterpret_cast<T*>(hist + 256);            // [C] (CDM == 0)

    auto seg_at = [&](int row) {
        const int s = segment_of[row];
        return s < 0 ? 0 : (s >= G ? G - 1 : s);
    };
    const int r0 = blockIdx.x * SG_ROWS;
    const int rl = (r0 + SG_ROWS < NT ? r0 + SG_ROWS : NT) - 1;
    // ---- the window: from the first row's segment on, at most W nodes, never beyond the last row's segment
    int64_t wlo = offsets[seg_at(r0)], whi = offsets[seg_at(rl) + 1];
    wlo = wlo < 0 ? 0 : (wlo > r0 ? r0 : wlo);
    whi = whi > NT ? NT : whi;
    if (whi > wlo + W) whi = wlo + W;
    if (W > 0) {
        const int total = (int)(whi - wlo) * C;          // (<= W C: fits an int)
        const T* src = coors + (size_t)wlo * C;
        for (int o = tid; o < total; o += SG_THREADS) {
            const int jn = o / C, c = o - jn * C;
            if constexpr (CDM == 0) xs[(size_t)jn * CS + c] = src[o];
            else xs[(size_t)c * W + jn] = src[o];
        }
    }
    __syncthreads();

    const uint64_t lt_mask = (1ull << lane) - 1ull;
    for (int r = wave; r < SG_ROWS; r += SG_WAVES) {
        const int i = r0 + r;
        if (i >= NT) break;                              // wave-uniform
        const int s = seg_at(i);
        // (offsets are validated by the caller; the clamps only keep a broken table inside the arrays)
        int64_t lo64 = offsets[s], hi64 = offsets[s + 1];
        lo64 = lo64 < 0 ? 0 : (lo64 > i ? i : lo64);
        hi64 = hi64 > NT ? NT : (hi64 <= i ? i + 1 : hi64);
        const int lo = (int)lo64, n = (int)(hi64 - lo64);
        const bool inwin = lo64 >= wlo && hi64 <= whi;
        const int Ksel = K < n ? K : n;
        const size_t ob = (size_t)i * K;

        constexpr int CR = CDM == 0 ? 1 : CDM;
        T ci[CR];
#pragma unroll
        for (int c = 0; c < CR; ++c) ci[c] = (CDM != 0 && c < C) ? coors[(size_t)i * C + c] : (T)0;
        if constexpr (CDM == 0) {
            for (int c = lane; c < C; c += 64) qs[c] = coors[(size_t)i * C + c];
        }

        auto select_row = [&](auto source) {
            constexpr bool LDS = decltype(source)::lds;
            const int w0 = lo - (int)wlo;                // the segment's first node in the window (LDS)
            const T* cb = coors + (size_t)lo * C;        // ... and in memory
            // (no mask, no adjacency: the key of the squared distance itself.  The window is component-major for CDM != 0)
            const T* qi = CDM == 0 ? qs : ci;
            auto key_of = [&](int jl) -> key_t {
                const T* cj = !LDS ? cb + (size_t)jl * (CDM == 3 ? 3 : C) : (CDM == 0 ? xs + (size_t)(w0 + jl) * CS : xs + w0 + jl);
                return egnn_knn_key_of<T, CDM>(qi, cj, (LDS && CDM != 0) ? W : 1, C, true, nullptr, (const uint8_t*)nullptr, i, jl);
            };

            const bool all = n <= K;                     // every candidate is selected: no search
            // ---- K <= 64: prune with the lanes' smallest keys.  M = the K-th smallest of the 64 (K > 32: 128) smallest-per-lane keys,
            // rounded up to its PB leading bits: at least K candidates are <= M, so the K smallest all are.
            if (!all && K <= 64) {
                const bool two = K > 32;                 // wave-uniform
                key_t lmin = ~(key_t)0, lmin2 = ~(key_t)0;
                for (int jl = lane; jl < n; jl += 64) {
                    const key_t kc = key_of(jl);
                    if (two) lmin2 = kc < lmin ? lmin : (kc < lmin2 ? kc : lmin2);
                    lmin = kc < lmin ? kc : lmin;
                }
                key_t M = 0;
                int belowm = 0;
                for (int bit = KB - 1; bit >= KB - PB; --bit) {
                    int cnt = __popcll(__ballot((lmin >> bit) == (M >> bit)));
                    if (two) cnt += __popcll(__ballot((lmin2 >> bit) == (M >> bit)));
                    if (belowm + cnt < K) { belowm += cnt; M |= (key_t)1 << bit; }
                }
                M |= ((key_t)1 << (KB - PB)) - 1;
                int S = 0;                               // survivors, compacted in index order while they fit the list
                for (int j0 = 0; j0 < n; j0 += 64) {
                    const int jl = j0 + lane;
                    key_t kj = 0;
                    bool take = false;
                    if (jl < n) { kj = key_of(jl); take = kj <= M; }
                    const uint64_t bs = __ballot(take);
                    const int pos = S + __popcll(bs & lt_mask);
                    if (take && pos < SG_SURVIVORS) { selk[pos] = kj; selj[pos] = jl; }
                    S += __popcll(bs);
                }
                egnn_wave_lds_sync();
                if (S <= SG_SURVIVORS) {                 // wave-uniform (S >= K)
                    egnn_knn_write_sorted<T>(selk, selj, S, K, lane, 64, lo, idx_out + ob, rank_out + ob);
                    return;
                }
                egnn_wave_lds_sync();                      // (the ranking above did not run, but the list is rewritten below)
            }

            // ---- radix passes over (key, local index); all control flow is wave-uniform
            key_t P = 0;                                 // resolved key prefix (right-aligned)
            uint32_t PJ = 0u;                            // resolved index prefix
            int L = 0, need = Ksel;
            int ibits = 1;
            while (ibits < 31 && (1 << ibits) < n) ++ibits;
            const int IBP = (ibits + 7) / 8 * 8;         // index digits: ceil(bits(n - 1) / 8) bytes
            while (!all && L < KD + IBP / 8) {
#pragma unroll
                for (int q = 0; q < 4; ++q) hist[4 * lane + q] = 0;
                egnn_wave_lds_sync();
                for (int jl = lane; jl < n; jl += 64) {
                    const key_t kj = key_of(jl);
                    if (!egnn_knn_has_prefix(kj, (uint32_t)jl, P, PJ, L, IBP)) continue;
                    atomicAdd(&hist[egnn_knn_digit(kj, (uint32_t)jl, L, IBP)], 1);
                }
                egnn_wave_lds_sync();
                // the bin holding the need-th candidate (lane l owns bins 4 l .. 4 l + 3)
                int c4[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) c4[q] = hist[4 * lane + q];
                egnn_knn_bin bin;
                if (!egnn_knn_find_bin(c4, need, lane, bin)) break;      // (cannot happen: the prefix holds >= need candidates)
                if (L < KD) P = (P << 8) | (key_t)bin.digit;
                else PJ = (PJ << 8) | (uint32_t)bin.digit;
                ++L;
                need -= bin.before;
                if (bin.in_bin == need) break;           // resolved: the bin is taken whole
            }

            // ---- pick: the candidates whose composite prefix is <= the resolved one, in index order
            int base = 0;
            for (int j0 = 0; j0 < n; j0 += 64) {
                const int jl = j0 + lane;
                bool take = false;
                key_t kj = 0;
                if (jl < n) {
                    kj = key_of(jl);
                    take = all || egnn_knn_take(kj, (uint32_t)jl, P, PJ, L, IBP);        // (L >= 1 unless `all`)
                }
                const uint64_t bs = __ballot(take);
                const int pos = base + __popcll(bs & lt_mask);
                if (take && pos < Ksel) { selk[pos] = kj; selj[pos] = jl; }
                base += __popcll(bs);
            }
            egnn_wave_lds_sync();
            // ---- rank by counting on (key, index)
            egnn_knn_write_sorted<T>(selk, selj, Ksel, Ksel, lane, 64, lo, idx_out + ob, rank_out + ob);
        };
        egnn_wave_lds_sync();                              // (the query's coordinates, CDM == 0)
        if (inwin) select_row(SgSrc<true>());
        else select_row(SgSrc<false>());
        // ---- empty slots of a graph smaller than K
        for (int k = Ksel + lane; k < K; k += 64) { idx_out[ob + k] = i; rank_out[ob + k] = (T)__builtin_inff(); }
        egnn_wave_lds_sync();                              // the next row reuses the list, the histogram and the query
    }
}

template <typename T>
int knn_segments_launch(const T* coors, const int64_t* offsets, const int32_t* segment_of, int G, int NT, int K, int C, int max_segment,
                        int32_t* idx_out, T* rank_out, void* stream)
{
    if (!offsets || !segment_of) return EGNN_E_NULLPTR;
    // (one batch of NT nodes; the segment table's shape conditions are reported where the batch count's would be)
    const int rc = egnn_knn_check_args(coors, idx_out, rank_out, (G > 0 && max_segment > 0 && max_segment <= NT) ? 1 : 0, NT, K, C);
    if (rc != EGNN_OK) return rc;
    const bool any = sizeof(T) == 8 || C > 8;
    const int Lp = K > SG_SURVIVORS ? (K + 1) & ~1 : SG_SURVIVORS;
    const size_t waves = SG_WAVES * sg_wave_bytes<T>(Lp, any ? C : 0);
    const size_t node = (size_t)(any ? (C | 1) : C) * sizeof(T);
    // the window: what the budget leaves, never more than a tile can touch (its rows, and the rest of its first and last segments)
    int64_t W = SG_LDS_BYTES > waves + 8 ? (int64_t)((SG_LDS_BYTES - waves - 8) / node) : 0;
    const int64_t span = (int64_t)SG_ROWS + 2 * (int64_t)max_segment;
    if (W > span) W = span;
    if (g_lds_nodes > 0 && W > g_lds_nodes) W = g_lds_nodes;
    const size_t lds = sg_up8((size_t)W * node) + waves;
    auto kern = knn_select_segments_kernel<T, 0>;
    if constexpr (sizeof(T) == 4) {
        if (C == 3) kern = knn_select_segments_kernel<T, 3>;
        else if (C <= 8) kern = knn_select_segments_kernel<T, 8>;
    }
    const dim3 grid((unsigned)((NT + SG_ROWS - 1) / SG_ROWS));
    hipLaunchKernelGGL(kern, grid, dim3(SG_THREADS), lds, static_cast<hipStream_t>(stream), coors, offsets, segment_of, G, NT, K, C, (int)W,
                       Lp, idx_out, rank_out);
    return egnn_launch_status();
}

}  // namespace

extern "C" int egnn_knn_select_segments_f32(const float* coors, const int64_t* offsets, const int32_t* segment_of, int G, int T, int K,
                                            int coor_dim, int max_segment, int32_t* idx_out, float* rank_out, void* stream)
{
    return knn_segments_launch<float>(coors, offsets, segment_of, G, T, K, coor_dim, max_segment, idx_out, rank_out, stream);
}

extern "C" int egnn_knn_select_segments_f64(const double* coors, const int64_t* offsets, const int32_t* segment_of, int G, int T, int K,
                                            int coor_dim, int max_segment, int32_t* idx_out, double* rank_out, void* stream)
{
    return knn_segments_launch<double>(coors, offsets, segment_of, G, T, K, coor_dim, max_segment, idx_out, rank_out, stream);
}

extern "C" int egnn_knn_segments_lds_nodes(int limit)
{
    const int before = g_lds_nodes;
    if (limit >= 0) g_lds_nodes = limit;
    return before;
}

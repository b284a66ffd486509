// The transposed neighbour list of the backward, built by ONE pair of launches instead of sort / bincount /
// cumsum / searchsorted passes (~1.5 ms of small ATen kernels per step at the north-star shape).
//
// d loss / d P_j[n] (autograd of the neighbour gather, egnn_pytorch.py:275) is a sum over the edges (i, k) that ARRIVE at n.  The
// backward walks them in a fixed order -- ascending edge id -- so that the sums are bit-reproducible (no float atomics).  What it
// needs is the edge ids sorted stably by destination, in two forms:
//     csr:  order[p] = edge id, p in [csr_seg[n], csr_seg[n+1])                       (egnn_rows_gather_sum_f32)
//     ent:  the same, every destination's entries padded with -1 to whole 16-entry tiles: tile range [tile_seg[n], tile_seg[n+1])
//           (the entry list of egnn_edge_bwd_pass_f32 with by_dest = 1; the list is padded with -1 to a multiple of 128 entries)
// A counting sort per graph: the destinations of one source row are distinct (top-k of distinct candidates; j = k on the dense
// path), so a wave that walks its rows in order can claim list positions with LDS counters without two lanes of one instruction
// ever meeting on a counter -- positions come out in ascending edge id with no sort.  One workgroup per graph; four waves own
// consecutive quarters of the rows, each with its own histogram (pass 1) turned into its own start offsets (pass 2).
// Graphs beyond N = 20 415 (whose histograms do not fit in LDS): the same placement per band of destinations, bands in parallel.
#include "egnn_common.h"

namespace {

constexpr int EL_MAX_THREADS = 1024;     // up to 16 waves per graph, each with its own histogram (as many as fit in LDS)
#ifndef EGNN_EL_ROWS_AHEAD
#define EGNN_EL_ROWS_AHEAD 16
#endif
constexpr int EL_ROWS_AHEAD = EGNN_EL_ROWS_AHEAD;   // rows whose index loads are in flight together (round 5, with the parallel scan below: 0.18 -> 0.09 ms per call at the north-star shape)

// hist[w][j] = number of edges of wave w's rows that arrive at j;  then (pass 2) per destination j: deg, tiles, and the
// graph-local exclusive scans first[j] (entries) / tseg[j] (tiles); returns the graph's totals through LDS slots
__device__ __forceinline__ void hist_and_scan(const int32_t* __restrict__ idx, int b, int N, int K, int* hist, int* scan_e, int* scan_t,
                                              int* totals)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int EL_THREADS = blockDim.x, EL_WAVES = blockDim.x >> 6;
    for (int o = tid; o < EL_WAVES * N; o += EL_THREADS) hist[o] = 0;
    __syncthreads();
    const int rows_per_wave = (N + EL_WAVES - 1) / EL_WAVES;
    const int r0 = wave * rows_per_wave, r1 = (r0 + rows_per_wave) < N ? (r0 + rows_per_wave) : N;
    // (K <= 64 -- one column per lane: four rows' indices in flight per step; the loop is bound by the latency of the index loads -- one
    // workgroup per graph -- and only the LDS counters have to be bumped in row order)
    if (idx && K <= 64) {
        for (int i = r0; i < r1; i += EL_ROWS_AHEAD) {
            int jv[EL_ROWS_AHEAD];
#pragma unroll
            for (int u = 0; u < EL_ROWS_AHEAD; ++u) jv[u] = (lane < K && i + u < r1) ? idx[((size_t)b * N + i + u) * K + lane] : -1;
#pragma unroll
            for (int u = 0; u < EL_ROWS_AHEAD; ++u)
                if (jv[u] >= 0) atomicAdd(&hist[wave * N + jv[u]], 1);
        }
    } else {
        for (int i = r0; i < r1; ++i)
            for (int k = lane; k < K; k += 64) {
                const int j = idx ? idx[((size_t)b * N + i) * K + k] : k;
                atomicAdd(&hist[wave * N + j], 1);
            }
    }
    __syncthreads();
    // per thread: a contiguous range of destinations; local sums, then a scan over the 256 threads
    const int per = (N + EL_THREADS - 1) / EL_THREADS;
    const int j0 = tid * per, j1 = (j0 + per) < N ? (j0 + per) : N;
    int se = 0, st = 0;
    for (int j = j0; j < j1; ++j) {
        int deg = 0;
        for (int w = 0; w < EL_WAVES; ++w) deg += hist[w * N + j];
        se += deg;
        st += (deg + 15) >> 4;
    }
    // exclusive scans over the workgroup's threads: inside the waves on the DPP network, the (up to 16) wave totals through LDS (round 5:
    // this was one thread walking all 1024 entries -- half of the two kernels' time)
    const int ie = egnn_wave_inclusive_scan(se), it = egnn_wave_inclusive_scan(st);
    int* wtot = totals + 2;                              // [2][16]
    if (lane == 63) { wtot[wave] = ie; wtot[16 + wave] = it; }
    __syncthreads();
    int be = 0, bt = 0;
    for (int w = 0; w < wave; ++w) { be += wtot[w]; bt += wtot[16 + w]; }
    scan_e[tid] = be + ie - se;
    scan_t[tid] = bt + it - st;
    if (tid == EL_THREADS - 1) { totals[0] = be + ie; totals[1] = bt + it; }
    __syncthreads();
}

__global__ __launch_bounds__(EL_MAX_THREADS) void dest_totals_kernel(const int32_t* __restrict__ idx, int N, int K, int64_t* __restrict__ tiles_per_graph)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int EL_THREADS = blockDim.x, EL_WAVES = blockDim.x >> 6;
    int* hist = reinterpret_cast<int*>(smem);
    int* scan_e = hist + EL_WAVES * N;
    int* scan_t = scan_e + EL_THREADS;
    int* totals = scan_t + EL_THREADS;
    hist_and_scan(idx, blockIdx.x, N, K, hist, scan_e, scan_t, totals);
    if (threadIdx.x == 0) tiles_per_graph[blockIdx.x] = totals[1];
}

__global__ __launch_bounds__(EL_MAX_THREADS) void dest_lists_kernel(const int32_t* __restrict__ idx, int B, int N, int K,
                                                                const int64_t* __restrict__ tiles_per_graph, int32_t* __restrict__ ent,
                                                                int64_t* __restrict__ tile_seg, int64_t* __restrict__ csr_order,
                                                                int64_t* __restrict__ csr_seg)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int EL_THREADS = blockDim.x, EL_WAVES = blockDim.x >> 6;
    int* hist = reinterpret_cast<int*>(smem);
    int* scan_e = hist + EL_WAVES * N;
    int* scan_t = scan_e + EL_THREADS;
    int* totals = scan_t + EL_THREADS;
    int* first = totals + 2 + 32;                    // [N] graph-local first entry of destination j in the csr list (behind the wave totals)
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    hist_and_scan(idx, b, N, K, hist, scan_e, scan_t, totals);
    // tiles of the graphs in front of this one: one graph per thread, summed over the workgroup (integer: any order gives the same sum)
    int64_t tbase = 0;
    {
        int part = 0;
        for (int g = tid; g < b; g += EL_THREADS) part += (int)tiles_per_graph[g];
        part = egnn_wave_inclusive_scan(part);
        int* wtot = totals + 2;                              // (free again: hist_and_scan ended with a barrier behind its last use)
        if (lane == 63) wtot[wave] = part;
        __syncthreads();
        for (int w = 0; w < EL_WAVES; ++w) tbase += wtot[w];
    }
    const int64_t ebase = (int64_t)b * N * K;        // every graph has exactly N K edges
    // start offsets per (wave, destination): hist[w][j] <- position of wave w's first entry of j inside j's tiles (graph-local,
    // in entries), first[j] <- csr start; tile_seg / csr_seg of this graph's destinations
    const int per = (N + EL_THREADS - 1) / EL_THREADS;
    const int j0 = tid * per, j1 = (j0 + per) < N ? (j0 + per) : N;
    int ae = scan_e[tid], at = scan_t[tid];
    for (int j = j0; j < j1; ++j) {
        int run = 0;
        for (int w = 0; w < EL_WAVES; ++w) {
            const int h = hist[w * N + j];
            hist[w * N + j] = at * 16 + run;         // padded position (entries) of this wave's first entry of j
            run += h;
        }
        first[j] = ae - at * 16;                      // csr position = first[j] + padded position  (entries of j are contiguous in both)
        tile_seg[(int64_t)b * N + j] = tbase + at;
        csr_seg[(int64_t)b * N + j] = ebase + ae;
        ae += run;
        at += (run + 15) >> 4;
    }
    if (b == B - 1 && tid == EL_THREADS - 1) {       // (the last thread's range ends at N: its running sums are the graph totals)
        tile_seg[(int64_t)B * N] = tbase + totals[1];
        csr_seg[(int64_t)B * N] = ebase + totals[0];
    }
    __syncthreads();
    // placement: rows in ascending order within the wave, the waves' row ranges in ascending order -> ascending edge id per destination
    const int rows_per_wave = (N + EL_WAVES - 1) / EL_WAVES;
    const int r0 = wave * rows_per_wave, r1 = (r0 + rows_per_wave) < N ? (r0 + rows_per_wave) : N;
    if (idx && K <= 64) {
        // (as in the histogram pass: four rows' index loads in flight, the counters bumped in row order)
        for (int i = r0; i < r1; i += EL_ROWS_AHEAD) {
            int jv[EL_ROWS_AHEAD];
#pragma unroll
            for (int u = 0; u < EL_ROWS_AHEAD; ++u) jv[u] = (lane < K && i + u < r1) ? idx[ebase + (int64_t)(i + u) * K + lane] : -1;
#pragma unroll
            for (int u = 0; u < EL_ROWS_AHEAD; ++u) {
                if (jv[u] < 0) continue;
                const int64_t eid = ebase + (int64_t)(i + u) * K + lane;
                const int pos = atomicAdd(&hist[wave * N + jv[u]], 1);   // distinct destinations within a row: no two lanes share a counter
                ent[tbase * 16 + pos] = (int32_t)eid;
                csr_order[ebase + first[jv[u]] + pos] = eid;
            }
        }
    } else {
        for (int i = r0; i < r1; ++i)
            for (int k = lane; k < K; k += 64) {
                const int64_t eid = ebase + (int64_t)i * K + k;
                const int j = idx ? idx[eid] : k;
                const int pos = atomicAdd(&hist[wave * N + j], 1);       // distinct destinations within a row: no two lanes share a counter
                ent[tbase * 16 + pos] = (int32_t)eid;
                csr_order[ebase + first[j] + pos] = eid;
            }
    }
}

// ---- graphs beyond the LDS of one workgroup (N > 20 415): the same lists from four launches.
//   dest_degree_kernel   in-degrees, integer atomics over all edges (order-free), into tile_seg as scratch
//   dest_totals_kernel_band  tiles per graph (one workgroup per graph)
//   dest_offsets_kernel  csr_seg / tile_seg: exclusive scans per graph behind the tiles of the graphs in front (one workgroup per graph)
//   dest_place_kernel    one workgroup per band of EL_BAND destinations: the single-workgroup placement above restricted to the band --
//                        per-wave LDS counters over the band, the waves owning consecutive row ranges, rows in order within a wave --
//                        so every destination's edges land in ascending edge id, as before.  Each band reads all of its graph's indices
//                        (twice); the bands run in parallel.
constexpr int EL_BAND = 1024;
constexpr int EL_BAND_THREADS = 1024;      // 16 waves: per-wave counters of one band fill 64 KB of LDS

__global__ __launch_bounds__(256) void dest_degree_kernel(const int32_t* __restrict__ idx, int N, int K, int64_t edges,
                                                          unsigned long long* __restrict__ deg)
{
    const int64_t nk = (int64_t)N * K;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < edges; e += (int64_t)gridDim.x * 256) {
        const int64_t b = e / nk;
        const int j = idx ? idx[e] : (int)(e % K);
        atomicAdd(&deg[b * N + j], 1ull);
    }
}

// per thread a contiguous range of the graph's destinations; exclusive scans of a per-thread value over the workgroup (wave scans on the
// DPP network, wave totals through LDS); returns the thread's offset, *total = the workgroup's sum
__device__ __forceinline__ int64_t block_exclusive_scan(int64_t v, int64_t* wtot, int64_t* total)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int waves = blockDim.x >> 6;
    // (int64 over the DPP scan: two 32-bit halves would carry; a graph's counts stay below 2^31, so the int scan is exact)
    const int incl = egnn_wave_inclusive_scan((int)v);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int64_t before = 0, all = 0;
    for (int w = 0; w < waves; ++w) {
        if (w < wave) before += wtot[w];
        all += wtot[w];
    }
    *total = all;
    __syncthreads();
    return before + incl - v;
}

__global__ __launch_bounds__(EL_MAX_THREADS) void dest_totals_kernel_band(const int64_t* __restrict__ deg, int N,
                                                                      int64_t* __restrict__ tiles_per_graph)
{
    __shared__ int64_t wtot[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int per = (N + blockDim.x - 1) / blockDim.x;
    const int j0 = tid * per < N ? tid * per : N, j1 = (j0 + per) < N ? (j0 + per) : N;
    int64_t st = 0;
    for (int j = j0; j < j1; ++j) st += (deg[(int64_t)b * N + j] + 15) >> 4;
    int64_t total;
    block_exclusive_scan(st, wtot, &total);
    if (tid == 0) tiles_per_graph[b] = total;
}

__global__ __launch_bounds__(EL_MAX_THREADS) void dest_offsets_kernel(int B, int N, int K, const int64_t* __restrict__ tiles_per_graph,
                                                                  int64_t* __restrict__ tile_seg, int64_t* __restrict__ csr_seg)
{
    __shared__ int64_t wtot[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t tbase = 0;                               // tiles of the graphs in front of this one (integer: any order gives the same sum)
    for (int g = 0; g < b; ++g) tbase += tiles_per_graph[g];
    const int64_t ebase = (int64_t)b * N * K;
    const int per = (N + blockDim.x - 1) / blockDim.x;
    const int j0 = tid * per < N ? tid * per : N, j1 = (j0 + per) < N ? (j0 + per) : N;
    int64_t* degs = tile_seg + (int64_t)b * N;       // (in place: every thread reads its own destinations before it overwrites them)
    int64_t se = 0, st = 0;
    for (int j = j0; j < j1; ++j) {
        se += degs[j];
        st += (degs[j] + 15) >> 4;
    }
    int64_t tot_e, tot_t;
    int64_t ae = block_exclusive_scan(se, wtot, &tot_e);
    int64_t at = block_exclusive_scan(st, wtot, &tot_t);
    for (int j = j0; j < j1; ++j) {
        const int64_t d = degs[j];
        csr_seg[(int64_t)b * N + j] = ebase + ae;
        degs[j] = tbase + at;
        ae += d;
        at += (d + 15) >> 4;
    }
    if (b == B - 1 && tid == 0) {
        tile_seg[(int64_t)B * N] = tbase + tot_t;
        csr_seg[(int64_t)B * N] = ebase + tot_e;
    }
}

__global__ __launch_bounds__(EL_BAND_THREADS) void dest_place_kernel(const int32_t* __restrict__ idx, int N, int K,
                                                                     const int64_t* __restrict__ tile_seg, const int64_t* __restrict__ csr_seg,
                                                                     int32_t* __restrict__ ent, int64_t* __restrict__ csr_order)
{
    __shared__ int hist[EL_BAND_THREADS / 64][EL_BAND];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int WAVES = EL_BAND_THREADS / 64;
    const int b = blockIdx.y;
    const int d0 = blockIdx.x * EL_BAND;
    const int64_t ebase = (int64_t)b * N * K;
    for (int o = tid; o < WAVES * EL_BAND; o += EL_BAND_THREADS) hist[o / EL_BAND][o % EL_BAND] = 0;
    __syncthreads();
    const int rows_per_wave = (N + WAVES - 1) / WAVES;
    const int r0 = wave * rows_per_wave < N ? wave * rows_per_wave : N, r1 = (r0 + rows_per_wave) < N ? (r0 + rows_per_wave) : N;
    // the wave's rows in order; `place` = false: count, true: claim positions and write (distinct destinations within a row: no two
    // lanes of one instruction share a counter)
    auto walk = [&](const bool place) {
        auto visit = [&](int64_t eid, int j) {
            const int jl = j - d0;
            if ((unsigned)jl >= (unsigned)EL_BAND) return;
            const int pos = atomicAdd(&hist[wave][jl], 1);
            if (place) {
                const int64_t dn = (int64_t)b * N + j;
                ent[tile_seg[dn] * 16 + pos] = (int32_t)eid;
                csr_order[csr_seg[dn] + pos] = eid;
            }
        };
        if (idx && K <= 64) {
            for (int i = r0; i < r1; i += EL_ROWS_AHEAD) {
                int jv[EL_ROWS_AHEAD];
#pragma unroll
                for (int u = 0; u < EL_ROWS_AHEAD; ++u) jv[u] = (lane < K && i + u < r1) ? idx[ebase + (int64_t)(i + u) * K + lane] : -1;
#pragma unroll
                for (int u = 0; u < EL_ROWS_AHEAD; ++u)
                    if (jv[u] >= 0) visit(ebase + (int64_t)(i + u) * K + lane, jv[u]);
            }
        } else {
            for (int i = r0; i < r1; ++i)
                for (int k = lane; k < K; k += 64) {
                    const int64_t eid = ebase + (int64_t)i * K + k;
                    visit(eid, idx ? idx[eid] : k);
                }
        }
    };
    walk(false);
    __syncthreads();
    // per destination of the band: wave w's counter <- the position of its first entry (the entries of the waves in front come first)
    if (d0 + tid < N && tid < EL_BAND) {
        int run = 0;
        for (int w = 0; w < WAVES; ++w) {
            const int h = hist[w][tid];
            hist[w][tid] = run;
            run += h;
        }
    }
    __syncthreads();
    walk(true);
}

}  // namespace

extern "C" size_t egnn_dest_lists_capacity(int B, int N, int K)
{
    // upper bound on the padded list: every destination wastes less than one tile; rounded up to whole rounds of 128 entries
    const int64_t tiles = (int64_t)B * ((int64_t)N * K / 16 + N) + 8;
    return (size_t)((tiles * 16 + 127) / 128 * 128);
}

extern "C" int egnn_dest_lists_i32(const int32_t* idx, int B, int N, int K, int32_t* ent, size_t ent_capacity, int64_t* tile_seg,
                                   int64_t* csr_order, int64_t* csr_seg, int64_t* tiles_per_graph, void* stream)
{
    if (!ent || !tile_seg || !csr_order || !csr_seg || !tiles_per_graph) return EGNN_E_NULLPTR;
    if (B <= 0 || N <= 0 || K <= 0) return EGNN_E_SHAPE;
    if (!idx && K != N) return EGNN_E_SHAPE;
    if ((int64_t)B * N * K > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;       // edge ids are int32 in the entry list
    if (ent_capacity < egnn_dest_lists_capacity(B, N, K)) return EGNN_E_SHAPE;
    // as many waves per graph as histograms fit in LDS (16, 8 or 4): one workgroup per graph is all the parallelism there is
    // (large graphs -- N beyond ~8000 -- trade waves for histogram space: 2 waves up to N = 13 500, 1 wave up to N = 20 400; beyond
    // that the banded kernels below the single-workgroup ones)
    int waves = 16;
    auto lds_for = [&](int w) { return ((size_t)w * N + 2 * (size_t)w * 64 + 2 + 32 + N) * sizeof(int); };
    while (waves > 4 && lds_for(waves) > 96 * 1024) waves >>= 1;
    while (waves > 1 && lds_for(waves) > 160 * 1024) waves >>= 1;
    const size_t lds = lds_for(waves);
    const int EL_THREADS = waves * 64;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (lds > 160 * 1024) {                                                 // N > 20 415 destinations per graph: bands of destinations
        if (hipMemsetAsync(ent, 0xFF, ent_capacity * sizeof(int32_t), s) != hipSuccess) return (int)hipGetLastError();
        if (hipMemsetAsync(tile_seg, 0, ((size_t)B * N + 1) * sizeof(int64_t), s) != hipSuccess) return (int)hipGetLastError();
        const int64_t edges = (int64_t)B * N * K;
        int64_t blocks = (edges + 255) / 256;
        if (blocks > 16384) blocks = 16384;
        hipLaunchKernelGGL(dest_degree_kernel, dim3((unsigned)blocks), dim3(256), 0, s, idx, N, K, edges,
                           reinterpret_cast<unsigned long long*>(tile_seg));
        hipLaunchKernelGGL(dest_totals_kernel_band, dim3(B), dim3(EL_MAX_THREADS), 0, s, tile_seg, N, tiles_per_graph);
        hipLaunchKernelGGL(dest_offsets_kernel, dim3(B), dim3(EL_MAX_THREADS), 0, s, B, N, K, tiles_per_graph, tile_seg, csr_seg);
        hipLaunchKernelGGL(dest_place_kernel, dim3((N + EL_BAND - 1) / EL_BAND, B), dim3(EL_BAND_THREADS), 0, s, idx, N, K, tile_seg,
                           csr_seg, ent, csr_order);
        return egnn_launch_status();
    }
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(dest_totals_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(dest_lists_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    if (hipMemsetAsync(ent, 0xFF, ent_capacity * sizeof(int32_t), s) != hipSuccess) return (int)hipGetLastError();     // -1 = padding
    hipLaunchKernelGGL(dest_totals_kernel, dim3(B), dim3(EL_THREADS), lds, s, idx, N, K, tiles_per_graph);
    hipLaunchKernelGGL(dest_lists_kernel, dim3(B), dim3(EL_THREADS), lds, s, idx, B, N, K, tiles_per_graph, ent, tile_seg, csr_order, csr_seg);
    return egnn_launch_status();
}

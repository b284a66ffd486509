// Cell-grid k-NN selection (gfx950): fp32 or double coordinates (below: "Double coordinates"; the text before it speaks of fp32),
// coor_dim == 3, optional mask, no adjacency or one given as CSR rows (below: "With CSR rows").  Outputs bit-identical to the
// streaming selection (knn_stream.hip) for every input with finite coordinates, at a cost per row that is bounded by the row's
// neighbourhood instead of N.  Distances are egnn_sqdist and keys egnn_knn_rank / egnn_rank_key (egnn_common.h), like every
// other selection kernel: equality is by construction.
//
// Per graph (no host read-back anywhere; every launch is unconditional, so the sequence can be captured):
//   bbox    partial sums over fixed chunks of the nodes: bounding box, first and second moments, valid count, non-finite flag
//   setup   one workgroup: the robust box [max(min, mean - 4 sd), min(max, mean + 4 sd)] per axis, the cell edge h for a mean
//           occupancy of KG_OCC nodes per cell (axes thinner than h get one cell: h is then chosen over the remaining axes),
//           at most KG_GMAX cells per axis; nodes outside the box are clamped into its border cells.  Clears the cell counters.
//   count   cell id per valid node, integer atomic count per cell
//   scan    one workgroup: cell starts; a graph whose fullest cell holds more than max(4096, N / 64) nodes is flagged
//   place   (x, y, z, index) of every valid node into its cell's range (an integer cursor per cell: the order inside a cell
//           varies from run to run, the outputs do not depend on it -- the search selects by the unique composite (key, index))
//   search  one wave per valid query, queries in cell order.  The cube of Chebyshev radius 1 around the query's cell first, then the
//           shells r = 2, 3, ...; a cube or shell is a list of x-runs of cells, i.e. of contiguous ranges of the sorted nodes, whose
//           bounds 64 lanes fetch at once.  The K best composites are kept in LDS: a candidate below the current K-th best is
//           appended, and a full buffer is ranked by counting, which leaves the K best sorted.
//   finish  rows the grid does not answer are flagged and finished by the streaming kernel (knn_stream.hip, its flagged
//           instantiation: workgroups without a flagged row return at once).  Flagged: every row of a graph with a non-finite
//           coordinate, an extent beyond 1e18, fewer than K valid nodes or an overfull cell; a valid row whose K-th best d^2 is
//           >= 1e5 while the graph has masked nodes (the reference interleaves them at exactly 1e5).  Masked rows of other graphs
//           are written here: the first K indices at rank 1e5.
//
// The stop rule and its margin.  Cells are c = trunc(fl(fl(x - x0) * inv_h)) per axis, clamped to [0, G - 1], G <= 1024.  Both
// roundings are relative (2^-24 each; a denormal difference is exact), so with u = (x - x0) * inv_h exact, |fl - u| <= 2^-23 u
// <= 2^-12 inside the box, and a node in cell c has u in [c - 2^-12, c + 1 + 2^-12); a clamped node lies beyond its border cell, on
// the far side.  After ring r every unvisited node differs from the query's cell by >= r + 1 on some axis, so |u_j - u_q| > r - 2^-11
// there and the true squared distance is >= (r h')^2 (1 - 2^-10), h' = 1 / inv_h.  egnn_sqdist computes fl(fl(fl(dx)^2 + fl(dy)^2)
// + fl(dz)^2) with dx = fl(xi - xj): five roundings on non-negative terms, relative error < 2^-21 (h >= 1e-15 keeps (r h)^2 far
// above the denormal range; extents <= 1e18 keep every term finite).  The bound itself -- fl(fl(r h) fl(r h)) with h = fl(1 / inv_h)
// -- is off by < 2^-21.  Together < 2^-9; the kernel uses (r h)^2 (1 - 2^-8).  A row stops once its K-th best d^2 is STRICTLY below
// that: every unvisited node then has a computed d^2 above the K-th key, so none can equal it and the lowest-index tie policy is
// decided among visited nodes only.  A row that never stops has visited every cell.
//
// With CSR rows (kg_search_kernel<true>, egnn_knn_select_grid_csr_f32).  The ranking value of (i, j) is overwritten AFTER the mask: -1 for
// j == i, 0 for j in row i of the adjacency -- an adjacent masked node ranks 0, a masked row keeps itself and its bonds.  The build passes
// do not change (only valid nodes go into the grid).  A valid row seeds its buffer with (key(-1), i) and (key(0), j) for the first
// min(len, K) columns j != i of its row (ascending on one key: the first are the best; <= K + 1 entries, the buffer holds max(2 K, K + 64))
// and marks it dirty; in the cells it drops i and every member of the row -- a binary search of the sorted columns, only for a candidate
// that already passed comp < tau -- so composites stay unique.  The stop rule is untouched: a K-th key of -1 or 0 is below
// (r h)^2 (1 - 2^-8) after ring 1, so a saturated row stops there, but it DOES visit ring 1: a node outside the row that coincides with i
// (d^2 = +0) has the key of an adjacent node and enters by its lower index.  Adjacent nodes the search has not visited are seeds already,
// so the rule's argument about unvisited nodes is about non-adjacent ones, as before.  A masked row of a graph the grid answers is written
// directly: i at -1, the columns != i at 0, then the lowest indices outside both at 1e5, cut at K -- one thread per entry, a binary search
// in the first K + 1 columns, whatever the degree.  Flagged rows (masked rows of a flagged graph too) go to the streaming kernel's flagged
// CSR instantiation.  The instantiation without an adjacency is the code it was: its three CSR arguments are appended and never read.
//
// Double coordinates (every kernel is a template on the coordinate type T; egnn_knn_select_grid_f64 / _grid_csr_f64).  The same seven
// launches on the same workspace layout, with three things wider.  The header's origin, inv_h and h are double, and cells are computed
// from the double coordinates themselves -- never from a value rounded to float, which could put a node in another cell than the one the
// stop rule assumes.  The sorted record is (x, y, z, index) in double, 32 bytes per node (egnn_knn_grid_workspace_bytes_f64).  Keys are
// the 64-bit egnn_rank_key(double), so the composite is the pair (key, index) in 16 bytes, compared key first, then index: as unique per
// candidate as the packed word, and the candidate buffer, kg_compact, the CSR seeds and tau all compare through kg_less.  Distances are
// egnn_sqdist_any<double, 4> as knn_stream.hip calls it for double -- for C = 3 fl(fl(fl(dx)^2 + fl(dy)^2) + fl(dz)^2) after additions of
// +0 that change no bit -- and the outputs are bit-identical to egnn_knn_select_stream_f64 / egnn_knn_select_csr_f64; flagged rows go
// to that kernel's flagged double instantiations.
// The stop rule in double.  Cells are c = trunc(fl(fl(x - x0) * inv_h)) clamped to [0, G - 1], G <= 1024, in double arithmetic.  Both
// roundings are relative (2^-53 each; a denormal difference is exact), so with u = (x - x0) * inv_h exact, |fl - u| <= 2^-52 u <= 2^-42
// inside the box, and a node in cell c has u in [c - 2^-42, c + 1 + 2^-42); a clamped node lies beyond its border cell, on the far side.
// After ring r every unvisited node differs from the query's cell by >= r + 1 on some axis, so |u_j - u_q| > r - 2^-41 there and the true
// squared distance is >= (r h')^2 (1 - 2^-40), h' = 1 / inv_h.  The computed distance has five roundings on non-negative terms, relative
// error < 2^-50 (h >= 1e-15, set by kg_setup_kernel, keeps (r h)^2 >= 1e-30, far above the denormal range of double as well; extents
// <= 1e18 -- the same flag condition, kept so that both types hand over the same graphs -- keep every term below 3e36, finite).  The
// bound fl(fl(r h) fl(r h)), h = fl(1 / inv_h), is off by < 2^-50.  Together < 2^-39, far inside the margin (r h)^2 (1 - 2^-8) that
// the kernel keeps for both types; the rest of the argument -- strictly below, unvisited keys above the K-th, ties decided among
// visited nodes -- does not depend on the type.
#include "knn_core.h"

namespace {

constexpr int KG_KMAX = 128;                 // K limit (the candidate buffer of a wave: 2 K entries)
constexpr int KG_OCC = 16;                   // target mean occupancy of a cell
constexpr int KG_GMAX = 1024;                // cells per axis
constexpr int KG_THREADS = 256;
constexpr int KG_SLOTS = 16;                 // query slots per search workgroup (4 per wave)
constexpr int KG_PARTS = 64;                 // chunks of the bbox pass
constexpr int KG_PW = 16;                    // doubles per chunk record
constexpr int KG_CAP = 2 * KG_KMAX;          // candidate buffer entries per wave

template <typename T> struct KgHdr;
template <> struct KgHdr<float> {
    float x0, y0, z0, inv_h, h;
    int gx, gy, gz, nvalid, flag;
    int pad[6];
};
template <> struct KgHdr<double> {
    double x0, y0, z0, inv_h, h;
    int gx, gy, gz, nvalid, flag;
    int pad[1];
};
static_assert(sizeof(KgHdr<float>) == 64 && sizeof(KgHdr<double>) == 64, "one 64-byte header per graph");

// the sorted record (x, y, z, index) and the composite (key, index) per coordinate type.  float: a float4 with the index's bits in w, and
// one 64-bit word (key << 32 | index); double: 32 and 16 bytes
struct alignas(16) KgRec64 { double x, y, z; int32_t j; int32_t pad; };
struct alignas(16) KgComp64 { uint64_t key; uint32_t j; uint32_t pad; };
template <typename T> struct KgTypes;
template <> struct KgTypes<float> { typedef float4 rec_t; typedef uint64_t comp_t; };
template <> struct KgTypes<double> { typedef KgRec64 rec_t; typedef KgComp64 comp_t; };

__device__ __forceinline__ float4 kg_rec(float x, float y, float z, int j) { return make_float4(x, y, z, __int_as_float(j)); }
__device__ __forceinline__ KgRec64 kg_rec(double x, double y, double z, int j) { return KgRec64{x, y, z, j, 0}; }
__device__ __forceinline__ int kg_rec_index(const float4& r) { return __float_as_int(r.w); }
__device__ __forceinline__ int kg_rec_index(const KgRec64& r) { return r.j; }
__device__ __forceinline__ float kg_rec_sqdist(const float4& a, const float4& b)
{
    float dx, dy, dz;
    return egnn_sqdist(a.x, a.y, a.z, b.x, b.y, b.z, dx, dy, dz);
}
__device__ __forceinline__ double kg_rec_sqdist(const KgRec64& a, const KgRec64& b)
{
    const double pa[3] = {a.x, a.y, a.z}, pb[3] = {b.x, b.y, b.z};
    return egnn_sqdist_any<double, 4>(pa, pb, 3);
}

__device__ __forceinline__ uint64_t kg_comp(float rank, int j) { return ((uint64_t)egnn_rank_key(rank) << 32) | (uint32_t)j; }
__device__ __forceinline__ KgComp64 kg_comp(double rank, int j) { return KgComp64{egnn_rank_key(rank), (uint32_t)j, 0u}; }
__device__ __forceinline__ bool kg_less(uint64_t a, uint64_t b) { return a < b; }
__device__ __forceinline__ bool kg_less(const KgComp64& a, const KgComp64& b) { return a.key < b.key || (a.key == b.key && a.j < b.j); }
__device__ __forceinline__ int32_t kg_comp_index(uint64_t c) { return (int32_t)(uint32_t)c; }
__device__ __forceinline__ int32_t kg_comp_index(const KgComp64& c) { return (int32_t)c.j; }
__device__ __forceinline__ float kg_comp_rank(uint64_t c) { return egnn_rank_from_key((uint32_t)(c >> 32)); }
__device__ __forceinline__ double kg_comp_rank(const KgComp64& c) { return egnn_rank_from_key(c.key); }
// above every composite a finite ranking value can form
template <typename C> __device__ __forceinline__ C kg_comp_top();
template <> __device__ __forceinline__ uint64_t kg_comp_top<uint64_t>() { return ~0ull; }
template <> __device__ __forceinline__ KgComp64 kg_comp_top<KgComp64>() { return KgComp64{~0ull, ~0u, 0u}; }

__device__ __forceinline__ float kg_min(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double kg_min(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float kg_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double kg_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ bool kg_finite(float v) { return fabsf(v) < __builtin_inff(); }
__device__ __forceinline__ bool kg_finite(double v) { return fabs(v) < __builtin_inf(); }

__host__ __device__ inline int kg_cell_cap(int N) { return N / 4 + 64; }

struct KgLayout { size_t hdr, part, flag, cell, cnt, start, sorted, total; };

// rec: bytes per sorted record (16: float, 32: double); nothing else depends on the coordinate type
inline KgLayout kg_layout(int B, int N, size_t rec)
{
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    KgLayout L;
    size_t o = 0;
    L.hdr = o; o = up(o + (size_t)B * sizeof(KgHdr<float>));
    L.part = o; o = up(o + (size_t)B * KG_PARTS * KG_PW * sizeof(double));
    L.flag = o; o = up(o + (size_t)B * N);
    L.cell = o; o = up(o + (size_t)B * N * 4);
    L.cnt = o; o = up(o + (size_t)B * kg_cell_cap(N) * 4);
    L.start = o; o = up(o + (size_t)B * (kg_cell_cap(N) + 1) * 4);
    L.sorted = o; o = up(o + (size_t)B * N * rec);
    L.total = o;
    return L;
}

// ---- bbox: chunk p of graph b -> 16 doubles: sum x y z, sum x^2 y^2 z^2, min x y z, max x y z, valid count, non-finite count
template <typename T>
__global__ __launch_bounds__(KG_THREADS) void kg_bbox_kernel(const T* __restrict__ coors, const uint8_t* __restrict__ mask, int N,
                                                             int P, double* __restrict__ part)
{
    __shared__ double sd[6][KG_THREADS];
    __shared__ T sf[6][KG_THREADS];
    __shared__ int si[2][KG_THREADS];
    const int tid = threadIdx.x, b = blockIdx.y, p = blockIdx.x;
    const int chunk = (N + P - 1) / P;
    const int lo = p * chunk, hi = min(N, lo + chunk);
    const T* cb = coors + (size_t)b * N * 3;
    const uint8_t* mb = mask ? mask + (size_t)b * N : nullptr;
    double s[6] = {0, 0, 0, 0, 0, 0};
    T mn[3] = {(T)__builtin_inff(), (T)__builtin_inff(), (T)__builtin_inff()};
    T mx[3] = {(T)-__builtin_inff(), (T)-__builtin_inff(), (T)-__builtin_inff()};
    int cnt = 0, bad = 0;
    for (int i = lo + tid; i < hi; i += KG_THREADS) {
        if (mb && !mb[i]) continue;
        ++cnt;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const T v = cb[(size_t)i * 3 + a];
            if (!kg_finite(v)) { ++bad; continue; }
            s[a] += (double)v;
            s[3 + a] += (double)v * (double)v;
            mn[a] = kg_min(mn[a], v);
            mx[a] = kg_max(mx[a], v);
        }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) sd[a][tid] = s[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) { sf[a][tid] = mn[a]; sf[3 + a][tid] = mx[a]; }
    si[0][tid] = cnt;
    si[1][tid] = bad;
    __syncthreads();
    for (int w = KG_THREADS / 2; w > 0; w >>= 1) {               // fixed tree: the same sums on every run
        if (tid < w) {
#pragma unroll
            for (int a = 0; a < 6; ++a) sd[a][tid] += sd[a][tid + w];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                sf[a][tid] = kg_min(sf[a][tid], sf[a][tid + w]);
                sf[3 + a][tid] = kg_max(sf[3 + a][tid], sf[3 + a][tid + w]);
            }
            si[0][tid] += si[0][tid + w];
            si[1][tid] += si[1][tid + w];
        }
        __syncthreads();
    }
    if (tid < KG_PW) {
        double v = 0.0;
        if (tid < 6) v = sd[tid][0];
        else if (tid < 12) v = (double)sf[tid - 6][0];
        else if (tid == 12) v = (double)si[0][0];
        else if (tid == 13) v = (double)si[1][0];
        part[((size_t)b * KG_PARTS + p) * KG_PW + tid] = v;
    }
}

// ---- setup: the graph's header from its chunk records (thread 0, fixed order), then the cell counters cleared
template <typename T>
__global__ __launch_bounds__(KG_THREADS) void kg_setup_kernel(const double* __restrict__ part, int N, int K, int P, KgHdr<T>* __restrict__ hdr,
                                                              int* __restrict__ cnt)
{
    __shared__ int ncells;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        const double* pb = part + (size_t)b * KG_PARTS * KG_PW;
        double s[6] = {0, 0, 0, 0, 0, 0}, mn[3], mx[3], n = 0, bad = 0;
        for (int a = 0; a < 3; ++a) { mn[a] = __builtin_inf(); mx[a] = -__builtin_inf(); }
        for (int p = 0; p < P; ++p) {
            const double* r = pb + (size_t)p * KG_PW;
            for (int a = 0; a < 6; ++a) s[a] += r[a];
            for (int a = 0; a < 3; ++a) { mn[a] = fmin(mn[a], r[6 + a]); mx[a] = fmax(mx[a], r[9 + a]); }
            n += r[12];
            bad += r[13];
        }
        KgHdr<T> H;
        H.x0 = H.y0 = H.z0 = (T)0;
        H.inv_h = H.h = (T)1;
        H.gx = H.gy = H.gz = 1;
        H.nvalid = (int)n;
        H.flag = (bad > 0 || n < (double)K || n < 1) ? 1 : 0;
        for (int a = 0; a < (int)(sizeof(H.pad) / sizeof(int)); ++a) H.pad[a] = 0;
        if (!H.flag) {
            double lo[3], ext[3], emax = 0;
            for (int a = 0; a < 3; ++a) {
                const double mean = s[a] / n;
                const double var = fmax(s[3 + a] / n - mean * mean, 0.0);
                const double sdv = sqrt(var);
                lo[a] = fmax(mn[a], mean - 4.0 * sdv);
                const double hi = fmin(mx[a], mean + 4.0 * sdv);
                ext[a] = fmax(hi - lo[a], 0.0);
                emax = fmax(emax, ext[a]);
                if (!(mx[a] - mn[a] <= 1e18)) H.flag = 1;
            }
            // the cell edge for KG_OCC nodes per cell over the axes that are at least one cell thick
            bool act[3] = {ext[0] > 0, ext[1] > 0, ext[2] > 0};
            double h = emax > 0 ? emax : 1.0;
            for (int it = 0; it < 3; ++it) {
                int d = 0;
                double V = 1.0;
                for (int a = 0; a < 3; ++a) if (act[a]) { ++d; V *= ext[a]; }
                if (d == 0) break;
                h = pow(V * (double)KG_OCC / n, 1.0 / (double)d);
                bool changed = false;
                for (int a = 0; a < 3; ++a) if (act[a] && ext[a] < h) { act[a] = false; changed = true; }
                if (!changed) break;
            }
            h = fmax(h, emax / (double)(KG_GMAX - 1));
            h = fmax(h, 1e-15);
            int g[3];
            const double cap = (double)kg_cell_cap(N);
            for (int it = 0; it < 64; ++it) {
                for (int a = 0; a < 3; ++a) g[a] = (int)fmin((double)KG_GMAX, floor(ext[a] / h) + 1.0);
                if ((double)g[0] * (double)g[1] * (double)g[2] <= cap) break;
                h *= 1.2599210498948732;
            }
            if ((double)g[0] * (double)g[1] * (double)g[2] > cap) g[0] = g[1] = g[2] = 1;
            H.inv_h = (T)(1.0 / h);
            H.h = (T)(1.0 / (double)H.inv_h);
            H.x0 = (T)lo[0]; H.y0 = (T)lo[1]; H.z0 = (T)lo[2];
            H.gx = g[0]; H.gy = g[1]; H.gz = g[2];
        }
        hdr[b] = H;
        ncells = H.gx * H.gy * H.gz;
    }
    __syncthreads();
    int* cb = cnt + (size_t)b * kg_cell_cap(N);
    for (int c = tid; c < ncells; c += KG_THREADS) cb[c] = 0;
}

template <typename T>
__device__ __forceinline__ int kg_axis_cell(T x, T x0, T inv_h, int g)
{
    const T t = (x - x0) * inv_h;
    return t > (T)0 ? (int)kg_min(t, (T)(g - 1)) : 0;
}

// ---- count: the cell of every valid node (-1: masked), one integer atomic per node
template <typename T>
__global__ __launch_bounds__(KG_THREADS) void kg_count_kernel(const T* __restrict__ coors, const uint8_t* __restrict__ mask, int N,
                                                              const KgHdr<T>* __restrict__ hdr, int* __restrict__ cell_of, int* __restrict__ cnt)
{
    const int b = blockIdx.y, i = blockIdx.x * KG_THREADS + threadIdx.x;
    const KgHdr<T> H = hdr[b];
    if (H.flag || i >= N) return;
    int c = -1;
    if (!mask || mask[(size_t)b * N + i]) {
        const T* p = coors + ((size_t)b * N + i) * 3;
        const int cx = kg_axis_cell(p[0], H.x0, H.inv_h, H.gx), cy = kg_axis_cell(p[1], H.y0, H.inv_h, H.gy),
                  cz = kg_axis_cell(p[2], H.z0, H.inv_h, H.gz);
        c = (cz * H.gy + cy) * H.gx + cx;
        atomicAdd(&cnt[(size_t)b * kg_cell_cap(N) + c], 1);
    }
    cell_of[(size_t)b * N + i] = c;
}

// ---- scan: cell starts (exclusive prefix sums of the counts), the fullest cell against the fallback limit
template <typename T>
__global__ __launch_bounds__(1024) void kg_scan_kernel(int N, KgHdr<T>* __restrict__ hdr, const int* __restrict__ cnt, int* __restrict__ start)
{
    __shared__ int sums[1024];
    __shared__ int smax;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (hdr[b].flag) return;                                              // (uniform: written by an earlier launch)
    const int nc = hdr[b].gx * hdr[b].gy * hdr[b].gz;
    const int* cb = cnt + (size_t)b * kg_cell_cap(N);
    int* sb = start + (size_t)b * (kg_cell_cap(N) + 1);
    const int per = (nc + 1023) / 1024;
    const int lo = min(nc, tid * per), hi = min(nc, lo + per);
    int sum = 0, m = 0;
    for (int c = lo; c < hi; ++c) { sum += cb[c]; m = max(m, cb[c]); }
    sums[tid] = sum;
    if (tid == 0) smax = 0;
    __syncthreads();
    atomicMax(&smax, m);
    for (int w = 1; w < 1024; w <<= 1) {
        const int v = tid >= w ? sums[tid - w] : 0;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    int run = sums[tid] - sum;
    for (int c = lo; c < hi; ++c) { sb[c] = run; run += cb[c]; }
    if (tid == 1023) sb[nc] = sums[1023];
    if (tid == 0 && smax > max(4096, N / 64)) hdr[b].flag = 1;
}

// ---- place: (x, y, z, index) into the cell's range; the counter of a cell doubles as its cursor (it counts back down to 0)
template <typename T>
__global__ __launch_bounds__(KG_THREADS) void kg_place_kernel(const T* __restrict__ coors, int N, const KgHdr<T>* __restrict__ hdr,
                                                              const int* __restrict__ cell_of, int* __restrict__ cnt,
                                                              const int* __restrict__ start,
                                                              typename KgTypes<T>::rec_t* __restrict__ sorted)
{
    const int b = blockIdx.y, i = blockIdx.x * KG_THREADS + threadIdx.x;
    if (hdr[b].flag || i >= N) return;
    const int c = cell_of[(size_t)b * N + i];
    if (c < 0) return;
    const int pos = start[(size_t)b * (kg_cell_cap(N) + 1) + c] + atomicSub(&cnt[(size_t)b * kg_cell_cap(N) + c], 1) - 1;
    const T* p = coors + ((size_t)b * N + i) * 3;
    if (pos >= 0 && pos < N) sorted[(size_t)b * N + pos] = kg_rec(p[0], p[1], p[2], i);
}

// the cnt entries of buf ranked by counting: the min(cnt, K) smallest end up sorted in buf[0 ..), tau = the K-th once there are K
template <typename C>
__device__ __forceinline__ void kg_compact(C* buf, C* tmp, int& cnt, C& tau, int K, int lane)
{
    egnn_wave_lds_sync();
    for (int t = lane; t < cnt; t += 64) {
        const C c = buf[t];
        int rnk = 0;
        for (int u = 0; u < cnt; ++u) rnk += kg_less(buf[u], c) ? 1 : 0;
        if (rnk < K) tmp[rnk] = c;
    }
    egnn_wave_lds_sync();
    const int n = cnt < K ? cnt : K;
    for (int t = lane; t < n; t += 64) buf[t] = tmp[t];
    egnn_wave_lds_sync();
    cnt = n;
    if (n == K) tau = buf[K - 1];
}

// j among the `len` strictly ascending columns at `col`
__device__ __forceinline__ bool kg_csr_member(const int32_t* __restrict__ col, int len, int j)
{
    int lo = 0, hi = len;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    return lo < len && col[lo] == j;
}

// CSR: every row has an adjacency, row i of graph b = the columns col[rowptr[b rp_stride + i] .. rowptr[b rp_stride + i + 1]); without
// it the three last arguments are not read.
template <typename T, bool CSR>
__global__ __launch_bounds__(KG_THREADS) void kg_search_kernel(const uint8_t* __restrict__ mask, const KgHdr<T>* __restrict__ hdr,
                                                               const int* __restrict__ cell_of, const int* __restrict__ start,
                                                               const typename KgTypes<T>::rec_t* __restrict__ sorted,
                                                               uint8_t* __restrict__ rowflag, int N, int K,
                                                               int32_t* __restrict__ idx_out, T* __restrict__ rank_out,
                                                               const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                               int64_t rp_stride)
{
    typedef typename KgTypes<T>::rec_t rec_t;
    typedef typename KgTypes<T>::comp_t comp_t;
    __shared__ comp_t sbuf[KG_THREADS / 64][KG_CAP];                      // (float: 8 KB + 4 KB; double: 16 KB + 8 KB)
    __shared__ comp_t stmp[KG_THREADS / 64][KG_KMAX];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, base = blockIdx.x * KG_SLOTS;
    const KgHdr<T> H = hdr[b];
    uint8_t* fb = rowflag + (size_t)b * N;
    if (H.flag) {                                                         // the whole graph goes to the streaming kernel
        if (tid < KG_SLOTS && base + tid < N) fb[base + tid] = 1;
        return;
    }
    if (mask) {                                                           // masked rows: the first K indices at rank 1e5
        const uint8_t* mb = mask + (size_t)b * N;
        for (int o = tid; o < KG_SLOTS * K; o += KG_THREADS) {
            const int rr = o / K, k = o - rr * K, i = base + rr;
            if (i < N && !mb[i]) {
                const size_t ob = ((size_t)b * N + i) * K;
                if constexpr (CSR) {
                    // ... behind i itself at -1 and the row's columns != i at 0: entry k of the merge of 0, 1, 2, ... against the sorted
                    // row.  Only the first K + 1 columns can matter; indices at 1e5 appear only when the whole row lies among them.
                    const int64_t* rp = rowptr + (size_t)b * rp_stride + i;
                    const int64_t lo = rp[0];
                    const int64_t len = rp[1] - lo;
                    const int32_t* cr = col + lo;                          // (not read when len == 0: col may be NULL)
                    const int lim = (int)(len < (int64_t)K + 1 ? len : (int64_t)K + 1);
                    int ip = 0;                                           // columns below i among the first lim
                    for (int hi = lim; ip < hi;) {
                        const int mid = (ip + hi) >> 1;
                        if (cr[mid] < i) ip = mid + 1;
                        else hi = mid;
                    }
                    const bool diag = ip < lim && cr[ip] == i;
                    const int nadj = lim - (diag ? 1 : 0);
                    int j;
                    T rk;
                    if (k == 0) {
                        j = i;
                        rk = (T)-1;
                    } else if (k - 1 < nadj) {
                        const int t = k - 1;
                        j = cr[(diag && t >= ip) ? t + 1 : t];
                        rk = (T)0;
                    } else {
                        // the m-th index outside S = {i} u row (sorted, L entries): m + t for the first t with S[t] - t > m
                        const int m = k - 1 - nadj, L = lim + (diag ? 0 : 1);
                        auto S = [&](int t) -> int { return diag ? cr[t] : (t < ip ? cr[t] : (t == ip ? i : cr[t - 1])); };
                        int t = 0;
                        for (int hi = L; t < hi;) {
                            const int mid = (t + hi) >> 1;
                            if (S(mid) - mid > m) hi = mid;
                            else t = mid + 1;
                        }
                        j = m + t;
                        rk = (T)1e5;
                    }
                    idx_out[ob + k] = j;
                    rank_out[ob + k] = rk;
                } else {
                    idx_out[ob + k] = k;
                    rank_out[ob + k] = (T)1e5;
                }
                if (k == 0) fb[i] = 0;
            }
        }
    }
    comp_t* buf = sbuf[wave];
    comp_t* tmp = stmp[wave];
    const int* st = start + (size_t)b * (kg_cell_cap(N) + 1);
    const rec_t* srt = sorted + (size_t)b * N;
    const int cap = K + 64 > 2 * K ? (K + 64 + 63) / 64 * 64 : 2 * K;      // (<= KG_CAP: K <= KG_KMAX)
    const int qend = min(base + KG_SLOTS, H.nvalid);
    for (int q = base + wave; q < qend; q += KG_THREADS / 64) {
        const rec_t me = srt[q];
        const int i = __builtin_amdgcn_readfirstlane(kg_rec_index(me));
        const int c = __builtin_amdgcn_readfirstlane(cell_of[(size_t)b * N + i]);
        const int cx = c % H.gx, cy = (c / H.gx) % H.gy, cz = c / (H.gx * H.gy);
        const int rmax = max(max(max(cx, H.gx - 1 - cx), max(cy, H.gy - 1 - cy)), max(max(cz, H.gz - 1 - cz), 1));
        int cnt = 0;
        bool dirty = false;
        comp_t tau = kg_comp_top<comp_t>();
        const int32_t* cr = nullptr;
        int clen = 0;
        if constexpr (CSR) {
            // the seeds: i itself at -1, then the first K columns != i at 0 -- ascending and on one key, so the first are the best; the
            // grid's candidates never repeat them (below).  At most K + 1 entries, sorted by the first compaction.
            const int64_t* rp = rowptr + (size_t)b * rp_stride + i;
            const int64_t lo = rp[0];
            clen = (int)(rp[1] - lo);
            cr = col + lo;                                                // (not read when clen == 0: col may be NULL)
            if (lane == 0) buf[0] = kg_comp((T)-1, i);
            cnt = 1;
            const int lim = min(clen, K + 1);
            for (int t0 = 0; t0 < lim; t0 += 64) {
                const int t = t0 + lane;
                const int j = t < lim ? cr[t] : i;
                const bool pass = j != i;
                const uint64_t bal = __ballot(pass);
                if (pass) {
                    const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
                    buf[cnt + below] = kg_comp((T)0, j);
                }
                cnt += __builtin_popcountll(bal);
            }
            cnt = min(cnt, K + 1);                                        // (the K + 1-th column, kept when the diagonal was not among them)
            dirty = true;
        }
        for (int r = 1;; ++r) {
            const int nrow = 2 * r + 1;
            const int nouter = nrow * nrow;
            const int nseg = r == 1 ? 9 : nouter + (nrow - 2) * (nrow - 2);
            for (int sb = 0; sb < nseg; sb += 64) {
                // 64 x-runs of cells at once: the bounds of their ranges in the sorted nodes
                const int sg = sb + lane;
                int s = 0, e = 0;
                if (sg < nseg) {
                    int dz, dy, xa, xb;
                    if (sg < nouter) {
                        dz = sg / nrow - r;
                        dy = sg % nrow - r;
                        const bool face = r == 1 || dz == r || dz == -r || dy == r || dy == -r;
                        xa = cx - r;
                        xb = face ? cx + r : cx - r;
                    } else {
                        const int t = sg - nouter, w = nrow - 2;
                        dz = t / w - (r - 1);
                        dy = t % w - (r - 1);
                        xa = xb = cx + r;
                    }
                    const int z = cz + dz, y = cy + dy;
                    xa = max(xa, 0);
                    xb = min(xb, H.gx - 1);
                    if (z >= 0 && z < H.gz && y >= 0 && y < H.gy && xa <= xb) {
                        const int row = (z * H.gy + y) * H.gx;
                        s = st[row + xa];
                        e = st[row + xb + 1];
                    }
                }
                const int nl = min(64, nseg - sb);
                for (int t = 0; t < nl; ++t) {
                    const int s_t = __builtin_amdgcn_readlane(s, t), e_t = min(__builtin_amdgcn_readlane(e, t), H.nvalid);
                    for (int p0 = s_t; p0 < e_t; p0 += 64) {
                        if (cnt + 64 > cap) kg_compact(buf, tmp, cnt, tau, K, lane);
                        const int p = p0 + lane;
                        bool pass = false;
                        comp_t comp = comp_t();
                        if (p < e_t) {
                            const rec_t cj = srt[p];
                            const T d = kg_rec_sqdist(me, cj);
                            const int j = kg_rec_index(cj);
                            comp = kg_comp(egnn_knn_rank<T>(d, true, true, nullptr, i, j), j);
                            pass = kg_less(comp, tau);
                            // (CSR: i and its row are seeded; the row is searched only for a candidate that would be kept)
                            if constexpr (CSR) pass = pass && j != i && !kg_csr_member(cr, clen, j);
                        }
                        const uint64_t bal = __ballot(pass);
                        if (pass) {
                            const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
                            buf[cnt + below] = comp;
                        }
                        const int add = __builtin_popcountll(bal);
                        cnt += add;
                        dirty = dirty || add > 0;
                    }
                }
            }
            if (cnt >= K) {
                if (dirty) { kg_compact(buf, tmp, cnt, tau, K, lane); dirty = false; }
                const T d2k = kg_comp_rank(tau);
                const T rh = (T)r * H.h;
                if (d2k < rh * rh * ((T)1 - (T)0.00390625)) break;
            }
            if (r >= rmax) break;
        }
        // (every cell visited or the rule above met; nvalid >= K, so K entries, sorted -- CSR: the seeds and the valid nodes outside
        // them are distinct and no fewer)
        egnn_wave_lds_sync();
        const T d2k = kg_comp_rank(tau);
        const bool hand_over = cnt < K || (d2k >= (T)1e5 && H.nvalid < N);
        if (!hand_over) {
            const size_t ob = ((size_t)b * N + i) * K;
            for (int t = lane; t < K; t += 64) {
                const comp_t cc = buf[t];
                idx_out[ob + t] = kg_comp_index(cc);
                rank_out[ob + t] = kg_comp_rank(cc);
            }
        }
        if (lane == 0) fb[i] = hand_over ? 1 : 0;
        egnn_wave_lds_sync();
    }
}

}  // namespace

extern "C" size_t egnn_knn_grid_workspace_bytes(int B, int N, int K)
{
    (void)K;
    if (B <= 0 || N <= 0) return 256;
    return kg_layout(B, N, sizeof(KgTypes<float>::rec_t)).total;
}

extern "C" size_t egnn_knn_grid_workspace_bytes_f64(int B, int N, int K)
{
    (void)K;
    if (B <= 0 || N <= 0) return 256;
    return kg_layout(B, N, sizeof(KgTypes<double>::rec_t)).total;
}

extern "C" size_t egnn_knn_grid_rowflag_offset_f64(int B, int N)
{
    if (B <= 0 || N <= 0) return 0;
    return kg_layout(B, N, sizeof(KgTypes<double>::rec_t)).flag;
}

static int kg_stream_flagged(const float* coors, const uint8_t* mask, const int64_t* rowptr, const int32_t* col, int64_t rp_stride, int B,
                             int N, int K, const uint8_t* rowflag, int32_t* idx_out, float* rank_out, void* stream)
{
    if (rowptr) return egnn_knn_stream_flagged_csr_f32(coors, mask, rowptr, col, rp_stride, B, N, K, rowflag, idx_out, rank_out, stream);
    return egnn_knn_stream_flagged_f32(coors, mask, B, N, K, rowflag, idx_out, rank_out, stream);
}
static int kg_stream_flagged(const double* coors, const uint8_t* mask, const int64_t* rowptr, const int32_t* col, int64_t rp_stride, int B,
                             int N, int K, const uint8_t* rowflag, int32_t* idx_out, double* rank_out, void* stream)
{
    if (rowptr) return egnn_knn_stream_flagged_csr_f64(coors, mask, rowptr, col, rp_stride, B, N, K, rowflag, idx_out, rank_out, stream);
    return egnn_knn_stream_flagged_f64(coors, mask, B, N, K, rowflag, idx_out, rank_out, stream);
}

// every entry: rowptr == NULL selects without an adjacency
template <typename T>
static int kg_select(const T* coors, const uint8_t* mask, const int64_t* rowptr, const int32_t* col, int64_t rp_stride, int B, int N,
                     int K, int coor_dim, int32_t* idx_out, T* rank_out, void* workspace, size_t workspace_bytes, void* stream)
{
    typedef typename KgTypes<T>::rec_t rec_t;
    if (!coors || !idx_out || !rank_out || !workspace) return EGNN_E_NULLPTR;
    if (B <= 0 || N <= 0 || K <= 0 || K > N) return EGNN_E_SHAPE;
    if (rowptr && rp_stride != 0 && rp_stride != (int64_t)N + 1) return EGNN_E_SHAPE;
    if (coor_dim != 3 || K > KG_KMAX || B > 65535) return EGNN_E_UNSUPPORTED;
    const KgLayout L = kg_layout(B, N, sizeof(rec_t));
    if (workspace_bytes < L.total) return EGNN_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return EGNN_E_ALIGN;
    char* ws = static_cast<char*>(workspace);
    KgHdr<T>* hdr = reinterpret_cast<KgHdr<T>*>(ws + L.hdr);
    double* part = reinterpret_cast<double*>(ws + L.part);
    uint8_t* rowflag = reinterpret_cast<uint8_t*>(ws + L.flag);
    int* cell_of = reinterpret_cast<int*>(ws + L.cell);
    int* cnt = reinterpret_cast<int*>(ws + L.cnt);
    int* start = reinterpret_cast<int*>(ws + L.start);
    rec_t* sorted = reinterpret_cast<rec_t*>(ws + L.sorted);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int P = min(KG_PARTS, (N + 4095) / 4096);
    const dim3 nodes((unsigned)((N + KG_THREADS - 1) / KG_THREADS), (unsigned)B);
    hipLaunchKernelGGL(kg_bbox_kernel<T>, dim3((unsigned)P, (unsigned)B), dim3(KG_THREADS), 0, st, coors, mask, N, P, part);
    hipLaunchKernelGGL(kg_setup_kernel<T>, dim3((unsigned)B), dim3(KG_THREADS), 0, st, (const double*)part, N, K, P, hdr, cnt);
    hipLaunchKernelGGL(kg_count_kernel<T>, nodes, dim3(KG_THREADS), 0, st, coors, mask, N, (const KgHdr<T>*)hdr, cell_of, cnt);
    hipLaunchKernelGGL(kg_scan_kernel<T>, dim3((unsigned)B), dim3(1024), 0, st, N, hdr, (const int*)cnt, start);
    hipLaunchKernelGGL(kg_place_kernel<T>, nodes, dim3(KG_THREADS), 0, st, coors, N, (const KgHdr<T>*)hdr, (const int*)cell_of, cnt,
                       (const int*)start, sorted);
    const dim3 slots((unsigned)((N + KG_SLOTS - 1) / KG_SLOTS), (unsigned)B);
    if (rowptr)
        hipLaunchKernelGGL((kg_search_kernel<T, true>), slots, dim3(KG_THREADS), 0, st, mask, (const KgHdr<T>*)hdr, (const int*)cell_of,
                           (const int*)start, (const rec_t*)sorted, rowflag, N, K, idx_out, rank_out, rowptr, col, rp_stride);
    else
        hipLaunchKernelGGL((kg_search_kernel<T, false>), slots, dim3(KG_THREADS), 0, st, mask, (const KgHdr<T>*)hdr, (const int*)cell_of,
                           (const int*)start, (const rec_t*)sorted, rowflag, N, K, idx_out, rank_out, (const int64_t*)nullptr,
                           (const int32_t*)nullptr, (int64_t)0);
    int rc = egnn_launch_status();
    if (rc != EGNN_OK) return rc;
    return kg_stream_flagged(coors, mask, rowptr, col, rp_stride, B, N, K, rowflag, idx_out, rank_out, stream);
}

extern "C" int egnn_knn_select_grid_f32(const float* coors, const uint8_t* mask, int B, int N, int K, int coor_dim, int32_t* idx_out,
                                        float* rank_out, void* workspace, size_t workspace_bytes, void* stream)
{
    return kg_select<float>(coors, mask, nullptr, nullptr, 0, B, N, K, coor_dim, idx_out, rank_out, workspace, workspace_bytes, stream);
}

extern "C" int egnn_knn_select_grid_csr_f32(const float* coors, const uint8_t* mask, const int64_t* rowptr, const int32_t* col,
                                            int64_t rowptr_graph_stride, int B, int N, int K, int coor_dim, int32_t* idx_out, float* rank_out,
                                            void* workspace, size_t workspace_bytes, void* stream)
{
    if (!rowptr) return EGNN_E_NULLPTR;
    return kg_select<float>(coors, mask, rowptr, col, rowptr_graph_stride, B, N, K, coor_dim, idx_out, rank_out, workspace, workspace_bytes,
                            stream);
}

extern "C" int egnn_knn_select_grid_f64(const double* coors, const uint8_t* mask, int B, int N, int K, int coor_dim, int32_t* idx_out,
                                        double* rank_out, void* workspace, size_t workspace_bytes, void* stream)
{
    return kg_select<double>(coors, mask, nullptr, nullptr, 0, B, N, K, coor_dim, idx_out, rank_out, workspace, workspace_bytes, stream);
}

extern "C" int egnn_knn_select_grid_csr_f64(const double* coors, const uint8_t* mask, const int64_t* rowptr, const int32_t* col,
                                            int64_t rowptr_graph_stride, int B, int N, int K, int coor_dim, int32_t* idx_out, double* rank_out,
                                            void* workspace, size_t workspace_bytes, void* stream)
{
    if (!rowptr) return EGNN_E_NULLPTR;
    return kg_select<double>(coors, mask, rowptr, col, rowptr_graph_stride, B, N, K, coor_dim, idx_out, rank_out, workspace, workspace_bytes,
                             stream);
}

// The N-degree adjacency expansion of EGNN_Network (egnn_pytorch.py:414-427; adj_expand.hip is its dense form) on CSR rows, and the
// degree labels of the selected pairs -- nothing of size N^2 (include/egnn_hip.h, "Sparse adjacency").
//
// One degree step:  nxt = pattern(cur . cur)  (row i of nxt = the union of the rows cur[j], j in cur[i]: the boolean product, :422),
// changed = nxt XOR cur (:423 -- an entry of cur that nxt lacks is relabelled too: graphs without a diagonal), labels[changed] = degree
// (:424), cur = nxt.  The labels are a CSR of their own over every pair that ever received one: L' = L u nxt (cur is a subset of L by
// induction, so L u changed = L u nxt), values = degree where changed, the old label elsewhere.
//
// A row is built as a bit set over its column RANGE [first column of any source row, last column of any source row]: three bit maps --
// nxt, cur, L -- in LDS when the range fits (ADJC_CAP_WORDS 32-bit words each: 131 072 columns), else in the workgroup's slice of the
// global workspace (the same code on another pointer: slower, any row length, any N).  Bits are set with integer atomicOr (the result does
// not depend on the order), counted with popcount, and emitted in ascending column order from a workgroup-wide prefix sum of the words'
// popcounts: sorted rows without a sort, deterministic.  Two passes per degree, as any CSR product: `count` (row lengths, then the
// exclusive scan that makes the row pointers and the two totals the caller reads back to size the column arrays) and `fill`.
// One workgroup per row, rows taken grid-stride (the global bit maps are per workgroup).
#include "egnn_common.h"

namespace {

constexpr int ADJC_THREADS = 256;
constexpr int ADJC_CAP_WORDS = 4096;          // per bit map in LDS: 3 x 16 KB
constexpr int ADJC_MAX_GRID = 1024;           // workgroups (and global bit-map slices)
constexpr int ADJC_SCAN_THREADS = 1024;

struct AdjcRow {                              // one row's view of the three CSR inputs
    const int32_t* cc; int cn;                // cur row i
    const int32_t* lc; int ln;                // label row i (columns)
    int64_t lbase;                            // its offset (the values' too)
};

__device__ __forceinline__ int block_sum(int v, int* red)          // red: [4] words of LDS; every thread gets the sum
{
    v = egnn_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// exclusive prefix of v over the workgroup's threads (thread order); red: [4]
__device__ __forceinline__ int block_exclusive(int v, int* red)
{
    const int incl = egnn_wave_inclusive_scan(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 63) red[wave] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += red[w];
    return base + incl - v;
}

// FILL = false: counts[row] = |nxt row|, counts[rows + row] = |L' row|.  FILL = true: the columns of nxt, the columns and values of L'.
template <bool FILL>
__global__ __launch_bounds__(ADJC_THREADS) void adj_csr_square_kernel(
    const int64_t* __restrict__ cur_rp, const int32_t* __restrict__ cur_col, const int64_t* __restrict__ lab_rp,
    const int32_t* __restrict__ lab_col, const uint8_t* __restrict__ lab_val, int G, int N, int degree, int force_global,
    uint32_t* __restrict__ gbits, int64_t gwords, int32_t* __restrict__ counts, const int64_t* __restrict__ nxt_rp,
    int32_t* __restrict__ nxt_col, const int64_t* __restrict__ new_rp, int32_t* __restrict__ new_col, uint8_t* __restrict__ new_val)
{
    __shared__ uint32_t lbits[3 * ADJC_CAP_WORDS];
    __shared__ int range[2];
    __shared__ int red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t rows = (int64_t)G * N;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int g = (int)(row / N), i = (int)(row - (int64_t)g * N);
        const int64_t* crp = cur_rp + (int64_t)g * (N + 1);
        const int64_t* lrp = lab_rp + (int64_t)g * (N + 1);
        AdjcRow r;
        r.cc = cur_col + crp[i];
        r.cn = (int)(crp[i + 1] - crp[i]);
        r.lbase = lrp[i];
        r.lc = lab_col + r.lbase;
        r.ln = (int)(lrp[i + 1] - r.lbase);
        // ---- the column range of everything this row touches (rows are sorted: first and last entry)
        if (tid == 0) { range[0] = 0x7fffffff; range[1] = -1; }
        __syncthreads();
        int lo = 0x7fffffff, hi = -1;
        if (tid == 0 && r.cn > 0) { lo = min(lo, r.cc[0]); hi = max(hi, r.cc[r.cn - 1]); }
        if (tid == 1 && r.ln > 0) { lo = min(lo, r.lc[0]); hi = max(hi, r.lc[r.ln - 1]); }
        for (int p = tid; p < r.cn; p += ADJC_THREADS) {
            const int j = r.cc[p];
            const int64_t a = crp[j], e = crp[j + 1];
            if (e > a) { lo = min(lo, cur_col[a]); hi = max(hi, cur_col[e - 1]); }
        }
        if (hi >= 0) { atomicMin(&range[0], lo); atomicMax(&range[1], hi); }
        __syncthreads();
        const int w0 = range[1] < 0 ? 0 : range[0] >> 5;
        const int nw = range[1] < 0 ? 0 : (range[1] >> 5) - w0 + 1;          // words per bit map
        const bool in_lds = nw <= ADJC_CAP_WORDS && !force_global;

        auto body = [&](uint32_t* bn, uint32_t* bc, uint32_t* bl) {
            for (int w = tid; w < nw; w += ADJC_THREADS) { bn[w] = 0u; bc[w] = 0u; bl[w] = 0u; }
            __syncthreads();
            for (int p = tid; p < r.cn; p += ADJC_THREADS) {
                const int c = r.cc[p];
                atomicOr(&bc[(c >> 5) - w0], 1u << (c & 31));
            }
            for (int p = tid; p < r.ln; p += ADJC_THREADS) {
                const int c = r.lc[p];
                atomicOr(&bl[(c >> 5) - w0], 1u << (c & 31));
            }
            for (int p = wave; p < r.cn; p += ADJC_THREADS / 64) {          // one wave per source row j, its lanes over the row
                const int j = r.cc[p];
                const int64_t a = crp[j], e = crp[j + 1];
                for (int64_t q = a + lane; q < e; q += 64) {
                    const int c = cur_col[q];
                    atomicOr(&bn[(c >> 5) - w0], 1u << (c & 31));
                }
            }
            __syncthreads();
            // ---- each thread owns a contiguous chunk of words; popcounts, then (fill) a prefix over the threads
            const int per = (nw + ADJC_THREADS - 1) / ADJC_THREADS;
            const int wa = min(nw, tid * per), wb = min(nw, wa + per);
            int sn = 0, su = 0, sl = 0;
            for (int w = wa; w < wb; ++w) {
                sn += __popc(bn[w]);
                su += __popc(bn[w] | bl[w]);
                sl += __popc(bl[w]);
            }
            if constexpr (!FILL) {
                const int tn = block_sum(sn, red);
                const int tu = block_sum(su, red);
                if (tid == 0) { counts[row] = tn; counts[rows + row] = tu; }
            } else {
                int pn = block_exclusive(sn, red);
                int pu = block_exclusive(su, red);
                int pl = block_exclusive(sl, red);
                int32_t* oc = nxt_col + nxt_rp[(int64_t)g * (N + 1) + i];
                const int64_t nb = new_rp[(int64_t)g * (N + 1) + i];
                for (int w = wa; w < wb; ++w) {
                    const uint32_t n = bn[w], c = bc[w], l = bl[w];
                    const int col0 = (w0 + w) << 5;
                    for (uint32_t x = n; x; x &= x - 1) oc[pn++] = col0 + __builtin_ctz(x);
                    const uint32_t ch = n ^ c;                               // :423  next != adj
                    for (uint32_t x = n | l; x; x &= x - 1) {
                        const int bit = __builtin_ctz(x);
                        new_col[nb + pu] = col0 + bit;
                        // (an unchanged pair of L': in L already -- its old label sits at its rank in the old row)
                        new_val[nb + pu] = ((ch >> bit) & 1u) ? (uint8_t)degree : lab_val[r.lbase + pl + __popc(l & ((1u << bit) - 1u))];
                        ++pu;
                    }
                    pl += __popc(l);
                }
            }
            __syncthreads();                                                 // (the bit maps are reused by the next row)
        };
        if (in_lds) body(lbits, lbits + ADJC_CAP_WORDS, lbits + 2 * ADJC_CAP_WORDS);
        else {
            uint32_t* gb = gbits + (int64_t)blockIdx.x * 3 * gwords;
            body(gb, gb + gwords, gb + 2 * gwords);
        }
    }
}

// counts (2, rows) int32 -> the two (G, N + 1) row-pointer arrays (absolute offsets from 0) and totals[a]; workgroup a = array a
__global__ __launch_bounds__(ADJC_SCAN_THREADS) void adj_csr_scan_kernel(const int32_t* __restrict__ counts, int G, int N,
                                                                         int64_t* __restrict__ rp0, int64_t* __restrict__ rp1,
                                                                         int64_t* __restrict__ totals)
{
    __shared__ int64_t part[ADJC_SCAN_THREADS];
    const int64_t rows = (int64_t)G * N;
    const int32_t* cnt = counts + (int64_t)blockIdx.x * rows;
    int64_t* rp = blockIdx.x == 0 ? rp0 : rp1;
    const int64_t per = (rows + ADJC_SCAN_THREADS - 1) / ADJC_SCAN_THREADS;
    const int64_t a = min(rows, (int64_t)threadIdx.x * per), e = min(rows, a + per);
    int64_t s = 0;
    for (int64_t x = a; x < e; ++x) s += cnt[x];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t run = 0;
        for (int t = 0; t < ADJC_SCAN_THREADS; ++t) { const int64_t v = part[t]; part[t] = run; run += v; }
        totals[blockIdx.x] = run;
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t x = a; x < e; ++x) {
        const int64_t g = x / N, i = x - g * N;
        rp[g * (N + 1) + i] = run;
        run += cnt[x];
        if (i == N - 1) rp[g * (N + 1) + N] = run;
    }
}

// out[b, i, k] = the label of pair (i, idx[b, i, k]) (idx NULL: j = k) in row i of the label CSR, 0 where the row does not hold it
__global__ __launch_bounds__(256) void csr_slot_labels_kernel(const int64_t* __restrict__ rp, const int32_t* __restrict__ col,
                                                              const uint8_t* __restrict__ val, int64_t gstride,
                                                              const int32_t* __restrict__ idx, int N, int K, int64_t total,
                                                              uint8_t* __restrict__ out)
{
    for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
        const int64_t node = o / K;                                          // b N + i
        const int k = (int)(o - node * K);
        const int64_t b = node / N;
        const int i = (int)(node - b * N);
        const int j = idx ? idx[o] : k;
        const int64_t* r = rp + b * gstride + i;
        int64_t lo = r[0], hi = r[1];                                        // first entry >= j in [lo, hi)
        const int64_t end = hi;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (col[mid] < j) lo = mid + 1;
            else hi = mid;
        }
        out[o] = (lo < end && col[lo] == j) ? val[lo] : (uint8_t)0;
    }
}

int adjc_grid(int G, int N)
{
    const int64_t rows = (int64_t)G * N;
    return (int)(rows < ADJC_MAX_GRID ? rows : ADJC_MAX_GRID);
}
int64_t adjc_words(int N) { return ((int64_t)N + 31) / 32; }

}  // namespace

extern "C" size_t egnn_adj_csr_workspace_bytes(int G, int N)
{
    if (G <= 0 || N <= 0) return 0;
    // the row lengths (2, G N) int32, then ADJC_MAX_GRID slices of three N-bit maps
    const size_t counts = ((size_t)2 * G * N * sizeof(int32_t) + 255) / 256 * 256;
    return counts + (size_t)adjc_grid(G, N) * 3 * (size_t)adjc_words(N) * sizeof(uint32_t);
}

static int adjc_check(const int64_t* cur_rowptr, const int64_t* lab_rowptr, int G, int N, int degree, void* workspace,
                      size_t workspace_bytes)
{
    if (!cur_rowptr || !lab_rowptr || !workspace) return EGNN_E_NULLPTR;
    if (G <= 0 || N <= 0 || degree < 2) return EGNN_E_SHAPE;
    if (degree > 255 || G > 65535) return EGNN_E_UNSUPPORTED;
    if (workspace_bytes < egnn_adj_csr_workspace_bytes(G, N)) return EGNN_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return EGNN_E_ALIGN;
    return EGNN_OK;
}

extern "C" int egnn_adj_csr_square_count(const int64_t* cur_rowptr, const int32_t* cur_col, const int64_t* lab_rowptr,
                                         const int32_t* lab_col, int G, int N, int64_t* nxt_rowptr, int64_t* new_lab_rowptr,
                                         int64_t* totals, void* workspace, size_t workspace_bytes, int flags, void* stream)
{
    const int rc = adjc_check(cur_rowptr, lab_rowptr, G, N, 2, workspace, workspace_bytes);
    if (rc) return rc;
    if (!nxt_rowptr || !new_lab_rowptr || !totals) return EGNN_E_NULLPTR;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t* counts = static_cast<int32_t*>(workspace);
    const size_t coff = ((size_t)2 * G * N * sizeof(int32_t) + 255) / 256 * 256;
    uint32_t* gbits = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + coff);
    hipLaunchKernelGGL(adj_csr_square_kernel<false>, dim3((unsigned)adjc_grid(G, N)), dim3(ADJC_THREADS), 0, s, cur_rowptr, cur_col,
                       lab_rowptr, lab_col, (const uint8_t*)nullptr, G, N, 0, flags & 1, gbits, adjc_words(N), counts,
                       (const int64_t*)nullptr, (int32_t*)nullptr, (const int64_t*)nullptr, (int32_t*)nullptr, (uint8_t*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(adj_csr_scan_kernel, dim3(2), dim3(ADJC_SCAN_THREADS), 0, s, counts, G, N, nxt_rowptr, new_lab_rowptr, totals);
    return egnn_launch_status();
}

extern "C" int egnn_adj_csr_square_fill(const int64_t* cur_rowptr, const int32_t* cur_col, const int64_t* lab_rowptr,
                                        const int32_t* lab_col, const uint8_t* lab_val, int G, int N, int degree,
                                        const int64_t* nxt_rowptr, int32_t* nxt_col, int64_t nxt_nnz, const int64_t* new_lab_rowptr,
                                        int32_t* new_lab_col, uint8_t* new_lab_val, int64_t new_lab_nnz, void* workspace,
                                        size_t workspace_bytes, int flags, void* stream)
{
    const int rc = adjc_check(cur_rowptr, lab_rowptr, G, N, degree, workspace, workspace_bytes);
    if (rc) return rc;
    if (!nxt_rowptr || !new_lab_rowptr) return EGNN_E_NULLPTR;
    if (nxt_nnz < 0 || new_lab_nnz < 0 || nxt_nnz > 0x7fffffffLL || new_lab_nnz > 0x7fffffffLL) return EGNN_E_SHAPE;
    if ((nxt_nnz > 0 && !nxt_col) || (new_lab_nnz > 0 && (!new_lab_col || !new_lab_val))) return EGNN_E_NULLPTR;
    const size_t coff = ((size_t)2 * G * N * sizeof(int32_t) + 255) / 256 * 256;
    uint32_t* gbits = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + coff);
    hipLaunchKernelGGL(adj_csr_square_kernel<true>, dim3((unsigned)adjc_grid(G, N)), dim3(ADJC_THREADS), 0,
                       static_cast<hipStream_t>(stream), cur_rowptr, cur_col, lab_rowptr, lab_col, lab_val, G, N, degree, flags & 1, gbits,
                       adjc_words(N), (int32_t*)nullptr, nxt_rowptr, nxt_col, new_lab_rowptr, new_lab_col, new_lab_val);
    return egnn_launch_status();
}

extern "C" int egnn_csr_slot_labels_u8(const int64_t* rowptr, const int32_t* col, const uint8_t* val, int64_t rowptr_graph_stride,
                                       const int32_t* idx, int B, int N, int K, uint8_t* out, void* stream)
{
    if (!rowptr || !out) return EGNN_E_NULLPTR;
    if (B <= 0 || N <= 0 || K <= 0) return EGNN_E_SHAPE;
    if (rowptr_graph_stride != 0 && rowptr_graph_stride != (int64_t)N + 1) return EGNN_E_SHAPE;
    if (!idx && K != N) return EGNN_E_SHAPE;
    const int64_t total = (int64_t)B * N * K;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(csr_slot_labels_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), rowptr, col, val,
                       rowptr_graph_stride, idx, N, K, total, out);
    return egnn_launch_status();
}

// Per-pair edge features given as CSR values (egnn_pytorch_amd.SparseEdges): the position look-up fused with the gather -- see
// include/egnn_hip.h::egnn_edge_features_gather_csr_f32 / _f64.  For every slot (b, i, k), j = idx[b,i,k]:
//   pos[b,i,k]   = the absolute offset of j in row i of graph b (-1: the row does not hold it, or j outside [0, N))
//   out[b,i,k,:] = [ values[pos] | tok_emb[tokens[pos]]   (pos < 0: zeros | tok_emb[0])   |   deg_emb[slot_deg[b,i,k]] ]
// T = float / double: a copy, the same kernel for both -- out holds the tables' own bits.
//
// A wave owns a node (four nodes per workgroup) and reads its row range once, as scalars.  Per chunk of 64 slots: lane l finds the
// position of slot l -- a binary search in the sorted row -- and leaves it in the wave's 64 words of LDS; then the wave writes the
// chunk's 64 (d1 + d2) contiguous output elements, lane after lane along the last dimension, each element fetching its slot's position
// from LDS.  (The LDS exchange is wave-private: LDS operations of one wave complete in issue order, no workgroup barrier.  The
// cross-lane shuffles are not used in this library: egnn_common.h.)  The transpose lives with its dense siblings in segment_sum.hip.
// Rows of up to 64 entries held one column per lane and matched by ballot, one slot at a time, were measured and dropped: twice the
// time of the search at bond-list rows as at rows of 48.
#include "egnn_common.h"

namespace {

constexpr int ECSR_MAX_GRID = 8192;                                // workgroups at most; the nodes beyond are walked grid-stride

template <typename T>
__global__ __launch_bounds__(256) void edge_csr_gather_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                              const T* __restrict__ values, const int64_t* __restrict__ tokens,
                                                              const T* __restrict__ tok_emb, int d1,
                                                              const uint8_t* __restrict__ slot_deg, const T* __restrict__ deg_emb,
                                                              int d2, const int32_t* __restrict__ idx, int N, int K, int64_t nodes,
                                                              int32_t* __restrict__ pos, T* __restrict__ out)
{
    __shared__ int32_t spos[4][64];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const int w = d1 + d2;
    int32_t* mine = spos[wave];
    for (int64_t node = (int64_t)blockIdx.x * 4 + wave; node < nodes; node += (int64_t)gridDim.x * 4) {
        const int64_t b = node / N;
        const int64_t* rp = rowptr + node + b;                     // b (N + 1) + i
        const int64_t r0 = rp[0], r1 = rp[1];
        for (int k0 = 0; k0 < K; k0 += 64) {
            const int nk = min(64, K - k0);
            const int64_t e0 = node * K + k0;                      // the chunk's first slot
            int32_t p = -1;
            if (lane < nk) {
                const int j = idx ? idx[e0 + lane] : k0 + lane;
                if ((unsigned)j < (unsigned)N) {
                    int64_t lo = r0, hi = r1;                      // first entry >= j in [r0, r1)
                    while (lo < hi) {
                        const int64_t mid = lo + ((hi - lo) >> 1);
                        if (col[mid] < j) lo = mid + 1;
                        else hi = mid;
                    }
                    if (lo < r1 && col[lo] == j) p = (int32_t)lo;
                }
                pos[e0 + lane] = p;
            }
            mine[lane] = p;
            __builtin_amdgcn_wave_barrier();
            const int tot = nk * w;
            T* o_base = out + e0 * w;
            for (int o = lane; o < tot; o += 64) {
                const int s = o / w, c = o - s * w;
                T v;
                if (c < d1) {
                    const int32_t ps = mine[s];
                    if (tokens) v = tok_emb[(ps >= 0 ? tokens[ps] : (int64_t)0) * d1 + c];
                    else v = ps >= 0 ? values[(int64_t)ps * d1 + c] : T(0);
                } else {
                    v = deg_emb[(int64_t)slot_deg[e0 + s] * d2 + (c - d1)];
                }
                o_base[o] = v;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

template <typename T>
int edge_features_gather_csr(const int64_t* rowptr, const int32_t* col, const T* values, const int64_t* tokens, const T* edge_tok_emb,
                             int d1, const uint8_t* slot_deg, const T* adj_deg_emb, int d2, const int32_t* idx, int B, int N, int K,
                             int32_t* pos, T* out, void* stream)
{
    if (!rowptr || !pos || !out) return EGNN_E_NULLPTR;
    if (B <= 0 || N <= 0 || K <= 0 || d1 <= 0 || d2 < 0) return EGNN_E_SHAPE;
    if ((values != nullptr) == (tokens != nullptr)) return EGNN_E_SHAPE;        // exactly one first table
    if (tokens && !edge_tok_emb) return EGNN_E_NULLPTR;
    if (d2 > 0 && (!slot_deg || !adj_deg_emb)) return EGNN_E_NULLPTR;
    if (!idx && K != N) return EGNN_E_SHAPE;
    const int64_t nodes = (int64_t)B * N;
    int64_t blocks = (nodes + 3) / 4;
    if (blocks > ECSR_MAX_GRID) blocks = ECSR_MAX_GRID;
    hipLaunchKernelGGL(edge_csr_gather_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), rowptr, col,
                       values, tokens, edge_tok_emb, d1, slot_deg, adj_deg_emb, d2, idx, N, K, nodes, pos, out);
    return egnn_launch_status();
}

}  // namespace

extern "C" int egnn_edge_features_gather_csr_f32(const int64_t* rowptr, const int32_t* col, const float* values, const int64_t* tokens,
                                                 const float* edge_tok_emb, int d1, const uint8_t* slot_deg,
                                                 const float* adj_deg_emb, int d2, const int32_t* idx, int B, int N, int K,
                                                 int32_t* pos, float* out, void* stream)
{
    return edge_features_gather_csr<float>(rowptr, col, values, tokens, edge_tok_emb, d1, slot_deg, adj_deg_emb, d2, idx, B, N, K, pos,
                                           out, stream);
}

extern "C" int egnn_edge_features_gather_csr_f64(const int64_t* rowptr, const int32_t* col, const double* values, const int64_t* tokens,
                                                 const double* edge_tok_emb, int d1, const uint8_t* slot_deg,
                                                 const double* adj_deg_emb, int d2, const int32_t* idx, int B, int N, int K,
                                                 int32_t* pos, double* out, void* stream)
{
    return edge_features_gather_csr<double>(rowptr, col, values, tokens, edge_tok_emb, d1, slot_deg, adj_deg_emb, d2, idx, B, N, K, pos,
                                            out, stream);
}

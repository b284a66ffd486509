// N-degree adjacency expansion of EGNN_Network (reference: egnn_pytorch/egnn_pytorch.py:414-427) as bit-set algebra.
//
// The reference labels 2nd, 3rd, ... degree neighbours by repeatedly squaring the adjacency with a FLOAT matmul
// ((adj.float() @ adj.float()) > 0: 2 N^3 flops per graph and degree) and marks the entries where the squared
// adjacency differs from the current one ((next.float() - adj.float()).bool() -- an XOR).  Here a row of the adjacency
// is a bit set of W = ceil(N/64) 64-bit words held one word per lane, and
//     next[i] = OR over { j : adj[i][j] } of adj[j]
// is N/64 wave-wide OR instructions per set bit: integer/byte work, bounded by reading adj once and writing the labels
// and the expanded adjacency once (3 bytes per ordered pair).  Results are bit-exact by construction.
//
// One wave per row; rows of the current bit matrix live in a ping-pong workspace (2 x B x N x W words).  adj_square_kernel holds
// one word per lane (W <= 64: N <= 4096); adj_square_wide_kernel takes any N: each lane owns R words of a column
// chunk of 64 R words, the chunks loop, and only the changed label bytes are stored.
#include "egnn_common.h"

namespace {

__global__ __launch_bounds__(256) void adj_pack_kernel(const uint8_t* __restrict__ adj, int64_t bstride, int N, int W,
                                                       uint64_t* __restrict__ bits, uint8_t* __restrict__ labels, int B)
{
    const int lane = threadIdx.x & 63;
    const int64_t row_g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);       // global row = b * N + i
    const int b = (int)(row_g / N), i = (int)(row_g % N);
    if (b >= B) return;
    const uint8_t* src = adj + (size_t)b * bstride + (size_t)i * N;
    for (int w = 0; w < W; ++w) {
        const int j = w * 64 + lane;
        const bool v = j < N && src[j] != 0;
        const uint64_t word = __ballot(v);
        if (lane == 0) bits[((size_t)b * N + i) * W + w] = word;
        if (j < N) labels[((size_t)b * N + i) * N + j] = v ? 1 : 0;           // adj_indices = adj_mat.long()  (:419)
    }
}

__global__ __launch_bounds__(256) void adj_square_kernel(const uint64_t* __restrict__ cur, uint64_t* __restrict__ nxt, int N, int W,
                                                         int degree, uint8_t* __restrict__ labels, uint8_t* __restrict__ adj_out, int B)
{
    const int lane = threadIdx.x & 63;
    const int64_t row_g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = (int)(row_g / N), i = (int)(row_g % N);
    if (b >= B) return;
    const uint64_t* gb = cur + (size_t)b * N * W;
    const uint64_t mine = lane < W ? gb[(size_t)i * W + lane] : 0ull;         // word `lane` of row i
    uint64_t acc = 0ull;
    for (int w = 0; w < W; ++w) {
        uint64_t word = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(mine & 0xffffffffu), w) |
                        ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(mine >> 32), w) << 32);
        while (word) {                                                         // wave-uniform
            const int j = w * 64 + __builtin_ctzll(word);
            word &= word - 1;
            if (lane < W) acc |= gb[(size_t)j * W + lane];                     // :422  (adj @ adj) > 0
        }
    }
    if (lane < W) nxt[((size_t)b * N + i) * W + lane] = acc;
    const uint64_t changed = acc ^ mine;                                       // :423  next != adj
    for (int w = 0; w < W; ++w) {
        const uint64_t cw = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(changed & 0xffffffffu), w) |
                            ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(changed >> 32), w) << 32);
        const uint64_t aw = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(acc & 0xffffffffu), w) |
                            ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(acc >> 32), w) << 32);
        const int j = w * 64 + lane;
        if (j < N) {
            if ((cw >> lane) & 1ull) labels[((size_t)b * N + i) * N + j] = (uint8_t)degree;     // :424
            if (adj_out) adj_out[((size_t)b * N + i) * N + j] = (uint8_t)((aw >> lane) & 1ull); // :425 (last step)
        }
    }
}

__device__ inline uint64_t readlane64(uint64_t v, int k)                   // k wave-uniform
{
    return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v & 0xffffffffu), k) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), k) << 32);
}

// Any N.  One wave per global row b * N + i; lane owns words c0 + 64 r + lane (r < R) of the column chunk [c0, c0 + 64 R).  For
// each chunk the wave walks the set bits j of row i (64 words per coalesced load, the nonzero ones through a ballot, their bits in
// order: wave-uniform) and ORs the chunk of row j into its accumulators -- R independent coalesced 8-byte loads per lane and bit.
// Stores: the new row (nxt); the label bytes only where a bit changed (a ballot skips the unchanged words; each changed word is
// one coalesced 64-byte masked store), so labels of earlier degrees stay where nothing changed; on the last degree all of adj_out,
// 64 bytes per wave store.  Tail bits past N are zero in every row (adj_pack_kernel) and ORs of zeros stay zero.
template <int R>
__global__ __launch_bounds__(256) void adj_square_wide_kernel(const uint64_t* __restrict__ cur, uint64_t* __restrict__ nxt, int N,
                                                              int W, int degree, uint8_t* __restrict__ labels,
                                                              uint8_t* __restrict__ adj_out, int B)
{
    const int lane = threadIdx.x & 63;
    const int64_t row_g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row_g >= (int64_t)B * N) return;
    const uint64_t* gb = cur + (size_t)(row_g / N) * N * W;
    const uint64_t* ri = cur + (size_t)row_g * W;
    uint8_t* lab = labels + (size_t)row_g * N;
    for (int c0 = 0; c0 < W; c0 += 64 * R) {
        uint64_t acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0ull;
        for (int g = 0; g < W; g += 64) {                                      // :422  (adj @ adj) > 0
            const uint64_t wl = g + lane < W ? ri[g + lane] : 0ull;
            uint64_t nz = __ballot(wl != 0ull);
            while (nz) {
                const int k = __builtin_ctzll(nz);
                nz &= nz - 1;
                uint64_t word = readlane64(wl, k);
                while (word) {
                    const size_t j = (size_t)(g + k) * 64 + __builtin_ctzll(word);
                    word &= word - 1;
                    const uint64_t* rj = gb + j * W + c0 + lane;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if (c0 + 64 * r + lane < W) acc[r] |= rj[64 * r];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int wb = c0 + 64 * r;                                        // first word of this slice
            const bool in = wb + lane < W;
            const uint64_t mine = in ? ri[wb + lane] : 0ull;
            if (in) nxt[(size_t)row_g * W + wb + lane] = acc[r];
            const uint64_t changed = acc[r] ^ mine;                            // :423  next != adj
            uint64_t nzc = __ballot(changed != 0ull);
            while (nzc) {
                const int k = __builtin_ctzll(nzc);
                nzc &= nzc - 1;
                const uint64_t cw = readlane64(changed, k);
                const size_t col = (size_t)(wb + k) * 64 + lane;
                if (((cw >> lane) & 1ull) && col < (size_t)N) lab[col] = (uint8_t)degree;        // :424
            }
            if (adj_out) {                                                     // :425 (last step)
                uint8_t* ao = adj_out + (size_t)row_g * N;
                for (int k = 0; k < 64 && wb + k < W; ++k) {
                    const uint64_t aw = readlane64(acc[r], k);
                    const size_t col = (size_t)(wb + k) * 64 + lane;
                    if (col < (size_t)N) ao[col] = (uint8_t)((aw >> lane) & 1ull);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void adj_copy_kernel(const uint8_t* __restrict__ adj, int64_t bstride, int N,
                                                       uint8_t* __restrict__ adj_out)
{
    const int64_t per = (int64_t)N * N;
    const int b = blockIdx.y;
    for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < per; x += (int64_t)gridDim.x * 256)
        adj_out[(size_t)b * per + x] = adj[(size_t)b * bstride + x] ? 1 : 0;
}

}  // namespace

extern "C" size_t egnn_adj_expand_workspace_bytes(int B, int N)
{
    const size_t W = (size_t)(N + 63) / 64;
    return 2 * (size_t)B * N * W * sizeof(uint64_t);
}

// wide = 0: the one-word-per-lane square kernel up to 4 096 nodes, adj_square_wide_kernel beyond; wide = 1: the wide kernel always
static int adj_expand(const uint8_t* adj, int64_t adj_batch_stride, int B, int N, int num_adj_degrees, uint8_t* adj_out,
                      uint8_t* degree_out, void* workspace, void* stream, bool wide)
{
    if (!adj || !adj_out || !degree_out || !workspace) return EGNN_E_NULLPTR;
    if (B <= 0 || N <= 0 || num_adj_degrees < 1) return EGNN_E_SHAPE;
    if (num_adj_degrees > 255 || B > 65535) return EGNN_E_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int W = (N + 63) / 64;
    wide = wide || W > 64;
    uint64_t* buf0 = static_cast<uint64_t*>(workspace);
    uint64_t* buf1 = buf0 + (size_t)B * N * W;
    const int64_t rows = (int64_t)B * N;
    if ((rows + 3) / 4 > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;
    dim3 g2((unsigned)((rows + 3) / 4));                              // one wave per global row b * N + i
    hipLaunchKernelGGL(adj_pack_kernel, g2, dim3(256), 0, s, adj, adj_batch_stride, N, W, buf0, degree_out, B);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    if (num_adj_degrees == 1) {
        hipLaunchKernelGGL(adj_copy_kernel, dim3(256, B), dim3(256), 0, s, adj, adj_batch_stride, N, adj_out);
        return egnn_launch_status();
    }
    uint64_t *cur = buf0, *nxt = buf1;
    for (int d = 2; d <= num_adj_degrees; ++d) {
        uint8_t* ao = d == num_adj_degrees ? adj_out : nullptr;
        if (!wide)
            hipLaunchKernelGGL(adj_square_kernel, g2, dim3(256), 0, s, cur, nxt, N, W, d, degree_out, ao, B);
        else if (W <= 64)
            hipLaunchKernelGGL(adj_square_wide_kernel<1>, g2, dim3(256), 0, s, cur, nxt, N, W, d, degree_out, ao, B);
        else if (W <= 128)
            hipLaunchKernelGGL(adj_square_wide_kernel<2>, g2, dim3(256), 0, s, cur, nxt, N, W, d, degree_out, ao, B);
        else if (W <= 256)
            hipLaunchKernelGGL(adj_square_wide_kernel<4>, g2, dim3(256), 0, s, cur, nxt, N, W, d, degree_out, ao, B);
        else if (W <= 512)
            hipLaunchKernelGGL(adj_square_wide_kernel<8>, g2, dim3(256), 0, s, cur, nxt, N, W, d, degree_out, ao, B);
        else                                                          // 65 536 columns per chunk; more columns loop over chunks
            hipLaunchKernelGGL(adj_square_wide_kernel<16>, g2, dim3(256), 0, s, cur, nxt, N, W, d, degree_out, ao, B);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        uint64_t* t = cur; cur = nxt; nxt = t;
    }
    return EGNN_OK;
}

extern "C" int egnn_adj_expand_u8(const uint8_t* adj, int64_t adj_batch_stride, int B, int N, int num_adj_degrees,
                                  uint8_t* adj_out, uint8_t* degree_out, void* workspace, void* stream)
{
    return adj_expand(adj, adj_batch_stride, B, N, num_adj_degrees, adj_out, degree_out, workspace, stream, false);
}

extern "C" int egnn_adj_expand_wide_u8(const uint8_t* adj, int64_t adj_batch_stride, int B, int N, int num_adj_degrees,
                                       uint8_t* adj_out, uint8_t* degree_out, void* workspace, void* stream)
{
    return adj_expand(adj, adj_batch_stride, B, N, num_adj_degrees, adj_out, degree_out, workspace, stream, true);
}

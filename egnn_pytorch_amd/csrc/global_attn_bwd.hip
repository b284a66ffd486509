// Backward of EGNN_Network's induced-set attention block (forward: global_attn.hip; reference: egnn_pytorch/egnn_pytorch.py:83-144).
//
//   egnn_induced_attn_bwd_f32   attn1's core: d/d q (B,T,inner) and d/d kv (B N, 2 inner) from d/d out
//   egnn_token_attn_bwd_f32     attn2's core: d/d q (B N, inner) and d/d kv_tok (B,T,2 inner)
//   egnn_gelu_bwd_f32           the feed-forward's exact (erf) GELU and its derivative in one pass
//   egnn_layer_norm_bwd_f32     LayerNorm over node rows: d/d x per row, d/d gamma and d/d beta as column sums
//
// All of them are streams over node rows (T <= 8 tokens: there is no N x N tile and nothing for the matrix cores); fp32 throughout.
// No float atomics anywhere: a sum over nodes is per-wave registers -> four waves merged in LDS in fixed order -> (where several
// workgroups share a result) one partial table per workgroup, added up in workgroup order by parts_sum_kernel.  Two runs give the
// same bits.
//
// The softmax statistics of attn1 (running max / sum per token) are NOT saved by the forward: the backward recomputes them in a first
// streaming kernel over the K half of the node rows with the forward's own online update and four-wave merge.  That costs one more read
// of B N inner floats -- a third of what the second pass moves -- and keeps the forward kernel, its ABI entry and the inference path
// untouched; a forward variant that wrote (max, sum) would save that read and add a (B,T,heads,2) tensor to what every training step keeps.
#include "egnn_common.h"
#include <float.h>

namespace {

constexpr int TMAX = 8;            // global tokens per graph
constexpr int DPL_MAX = 4;         // dim_head <= 256: floats per lane
constexpr int LN_UMAX = 16;        // LayerNorm backward: dim <= 1024 (columns per lane)
constexpr int LN_MAX_BLOCKS = 256;
constexpr int TOK_MAX_CHUNKS = 256;
constexpr int IND_MAX_CHUNKS = 32;

// out[i] = parts[0][i] + parts[1][i] + ... in that order
__global__ __launch_bounds__(256) void parts_sum_kernel(const float* __restrict__ parts, int nparts, int64_t count, float* __restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
        float acc = 0.f;
        for (int p = 0; p < nparts; ++p) acc += parts[(size_t)p * count + i];
        out[i] = acc;
    }
}

void launch_parts_sum(const float* parts, int nparts, int64_t count, float* out, hipStream_t s)
{
    int64_t blocks = (count + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(parts_sum_kernel, dim3((unsigned)blocks), dim3(256), 0, s, parts, nparts, count, out);
}

// ---- attn1: one workgroup per (graph, head, chunk of nodes), four waves striding the chunk, lane l owns dims l, l + 64, ... (the
// forward's wave shape; the forward's grid of B heads workgroups leaves most of the chip idle, so the nodes are cut into chunks here).
// p_tn = exp(s_tn - max_t) / sum_t;  D_t = g_o[t] . o[t];  g_v[n] = sum_t p_tn g_o[t];  g_s = p_tn (g_o[t] . v_n - D_t);
// g_k[n] = scale sum_t g_s q_t;  g_q[t] = scale sum_n g_s k_n.  A masked node's logit is the constant -FLT_MAX (masked_fill): no
// gradient reaches its k or the queries through it, and its p is 0 -- except in a graph whose mask is all False, where p = 1 / N and
// g_v flows.  Two kernels: the statistics of each chunk (running max / sum with the forward's online update and four-wave merge), then
// the gradients -- every workgroup merges the chunks' statistics of its (graph, head) in chunk order, writes its nodes' g_kv rows and one
// partial g_q table per chunk (added up in chunk order by parts_sum_kernel).
template <int DPL>
__global__ __launch_bounds__(256) void induced_stats_kernel(const float* __restrict__ q, const float* __restrict__ kv, int64_t ldkv,
                                                            const uint8_t* __restrict__ mask, int N, int T, int heads, int dh, float scale,
                                                            int chunk, float* __restrict__ stats)
{
    __shared__ float sm[4][TMAX][2];                    // per wave: running max, running sum
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inner = heads * dh;
    const int n0 = blockIdx.y * chunk, n1 = min(N, n0 + chunk);
    float qr[TMAX][DPL];
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
#pragma unroll
        for (int u = 0; u < DPL; ++u) {
            const int d = lane + 64 * u;
            qr[t][u] = (t < T && d < dh) ? q[((size_t)b * T + t) * inner + h * dh + d] * scale : 0.f;
        }
    float m[TMAX], l[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; ++t) { m[t] = -FLT_MAX; l[t] = 0.f; }
    for (int n = n0 + wave; n < n1; n += 4) {
        const float* row = kv + ((size_t)b * N + n) * ldkv + h * dh;
        float kr[DPL];
#pragma unroll
        for (int u = 0; u < DPL; ++u) {
            const int d = lane + 64 * u;
            kr[u] = d < dh ? row[d] : 0.f;
        }
        const bool keep = mask ? mask[(size_t)b * N + n] != 0 : true;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            if (t < T) {
                float s = 0.f;
#pragma unroll
                for (int u = 0; u < DPL; ++u) s += qr[t][u] * kr[u];
                s = egnn_wave_sum(s);
                if (!keep) s = -FLT_MAX;
                const float mn = fmaxf(m[t], s);
                l[t] = l[t] * expf(m[t] - mn) + expf(s - mn);
                m[t] = mn;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
        if (lane == 0) { sm[wave][t][0] = m[t]; sm[wave][t][1] = l[t]; }
    __syncthreads();
    if (threadIdx.x < TMAX) {                           // the chunk's (max, sum) per token: four waves merged in fixed order
        const int t = threadIdx.x;
        float mm = -FLT_MAX;
        for (int w = 0; w < 4; ++w) mm = fmaxf(mm, sm[w][t][0]);
        float den = 0.f;
        for (int w = 0; w < 4; ++w) den += sm[w][t][1] * expf(sm[w][t][0] - mm);
        float* st = stats + (((size_t)blockIdx.x * gridDim.y + blockIdx.y) * TMAX + t) * 2;
        st[0] = mm; st[1] = den;
    }
}

template <int DPL>
__global__ __launch_bounds__(256) void induced_attn_bwd_kernel(const float* __restrict__ q, const float* __restrict__ kv, int64_t ldkv,
                                                               const uint8_t* __restrict__ mask, const float* __restrict__ o,
                                                               const float* __restrict__ g_o, int N, int T, int heads, int dh, float scale,
                                                               int chunk, const float* __restrict__ stats, float* __restrict__ parts,
                                                               int64_t part_stride, float* __restrict__ g_kv)
{
    __shared__ float sq[4][TMAX][64 * DPL];             // per wave: its share of sum_n g_s k_n
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inner = heads * dh;
    const int n0 = blockIdx.y * chunk, n1 = min(N, n0 + chunk);
    float qr[TMAX][DPL], gor[TMAX][DPL], dt[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        float acc = 0.f;
#pragma unroll
        for (int u = 0; u < DPL; ++u) {
            const int d = lane + 64 * u;
            const bool in = t < T && d < dh;
            const size_t at = ((size_t)b * T + t) * inner + h * dh + d;
            qr[t][u] = in ? q[at] * scale : 0.f;
            gor[t][u] = in ? g_o[at] : 0.f;
            const float ov = in ? o[at] : 0.f;
            acc += gor[t][u] * ov;                      // (the form of g_o . v_n below: with one node o = v and g_s comes out exactly 0)
        }
        dt[t] = egnn_wave_sum(acc);
    }
    // the softmax statistics of the whole graph: the chunks' merged in chunk order (every workgroup of a (graph, head): the same bits)
    float m[TMAX], l[TMAX];
    const float* st = stats + (size_t)blockIdx.x * gridDim.y * TMAX * 2;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
        float mm = -FLT_MAX;
        for (unsigned c = 0; c < gridDim.y; ++c) mm = fmaxf(mm, st[(c * TMAX + t) * 2]);
        float den = 0.f;
        for (unsigned c = 0; c < gridDim.y; ++c) den += st[(c * TMAX + t) * 2 + 1] * expf(st[(c * TMAX + t) * 2] - mm);
        m[t] = mm;
        l[t] = t < T ? 1.0f / den : 0.f;
    }
    // the gradients; every (node row, head) slice of g_kv is written exactly once
    float gq[TMAX][DPL];
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
#pragma unroll
        for (int u = 0; u < DPL; ++u) gq[t][u] = 0.f;
    for (int n = n0 + wave; n < n1; n += 4) {
        const float* row = kv + ((size_t)b * N + n) * ldkv + h * dh;
        float kr[DPL], vr[DPL], gk[DPL], gv[DPL];
#pragma unroll
        for (int u = 0; u < DPL; ++u) {
            const int d = lane + 64 * u;
            kr[u] = d < dh ? row[d] : 0.f;
            vr[u] = d < dh ? row[inner + d] : 0.f;
            gk[u] = 0.f; gv[u] = 0.f;
        }
        const bool keep = mask ? mask[(size_t)b * N + n] != 0 : true;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            if (t < T) {
                float s = 0.f, dpv = 0.f;
#pragma unroll
                for (int u = 0; u < DPL; ++u) { s += qr[t][u] * kr[u]; dpv += gor[t][u] * vr[u]; }
                s = egnn_wave_sum(s);
                dpv = egnn_wave_sum(dpv);
                if (!keep) s = -FLT_MAX;
                const float p = expf(s - m[t]) * l[t];
                const float gs = keep ? p * (dpv - dt[t]) : 0.f;
#pragma unroll
                for (int u = 0; u < DPL; ++u) {
                    gv[u] += p * gor[t][u];
                    gk[u] += gs * qr[t][u];
                    gq[t][u] += gs * kr[u];
                }
            }
        }
        float* grow = g_kv + ((size_t)b * N + n) * 2 * inner + h * dh;
#pragma unroll
        for (int u = 0; u < DPL; ++u) {
            const int d = lane + 64 * u;
            if (d < dh) { grow[d] = gk[u]; grow[inner + d] = gv[u]; }
        }
    }
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
#pragma unroll
        for (int u = 0; u < DPL; ++u) sq[wave][t][lane + 64 * u] = gq[t][u];
    __syncthreads();
    float* part = parts + (size_t)blockIdx.y * part_stride;
    for (int idx = threadIdx.x; idx < T * dh; idx += 256) {
        const int t = idx / dh, d = idx - t * dh;
        part[((size_t)b * T + t) * inner + h * dh + d] = scale * (((sq[0][t][d] + sq[1][t][d]) + sq[2][t][d]) + sq[3][t][d]);
    }
}

// ---- attn2: one workgroup per (graph, head, chunk of nodes); one wave per node recomputes its T probabilities and writes its g_q
// slice; d/d kv_tok is a sum over the nodes: per-wave registers, merged in LDS, one partial table per chunk.
template <int DPL>
__global__ __launch_bounds__(256) void token_attn_bwd_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ kv_tok,
                                                             const float* __restrict__ g_out, int64_t ldg, int N, int T, int heads, int dh,
                                                             float scale, int chunk, float* __restrict__ g_q, float* __restrict__ parts,
                                                             int64_t part_stride)
{
    __shared__ float sacc[4][TMAX][64 * DPL];
    const int b = blockIdx.x / heads, h = blockIdx.x % heads;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inner = heads * dh;
    const int n0 = blockIdx.y * chunk, n1 = min(N, n0 + chunk);
    float kr[TMAX][DPL], vr[TMAX][DPL], gk[TMAX][DPL], gv[TMAX][DPL];
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
#pragma unroll
        for (int u = 0; u < DPL; ++u) {
            const int d = lane + 64 * u;
            const bool in = t < T && d < dh;
            const size_t at = ((size_t)b * T + t) * 2 * inner + h * dh + d;
            kr[t][u] = in ? kv_tok[at] : 0.f;
            vr[t][u] = in ? kv_tok[at + inner] : 0.f;
            gk[t][u] = 0.f; gv[t][u] = 0.f;
        }
    for (int n = n0 + wave; n < n1; n += 4) {
        const int64_t r = (int64_t)b * N + n;
        float qr[DPL], gr[DPL];
#pragma unroll
        for (int u = 0; u < DPL; ++u) {
            const int d = lane + 64 * u;
            qr[u] = d < dh ? q[r * ldq + h * dh + d] * scale : 0.f;
            gr[u] = d < dh ? g_out[r * ldg + h * dh + d] : 0.f;
        }
        float p[TMAX], dp[TMAX], mx = -FLT_MAX;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            float s = 0.f, e = 0.f;
#pragma unroll
            for (int u = 0; u < DPL; ++u) { s += qr[u] * kr[t][u]; e += gr[u] * vr[t][u]; }
            p[t] = egnn_wave_sum(s);
            dp[t] = egnn_wave_sum(e);
            if (t < T) mx = fmaxf(mx, p[t]);
        }
        float den = 0.f;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) { p[t] = t < T ? expf(p[t] - mx) : 0.f; den += p[t]; }
        const float inv = 1.0f / den;
        float dd = 0.f;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) { p[t] *= inv; dd += p[t] * dp[t]; }
        float gqv[DPL];
#pragma unroll
        for (int u = 0; u < DPL; ++u) gqv[u] = 0.f;
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            const float gs = p[t] * (dp[t] - dd);
#pragma unroll
            for (int u = 0; u < DPL; ++u) {
                gqv[u] += gs * kr[t][u];
                gk[t][u] += gs * qr[u];
                gv[t][u] += p[t] * gr[u];
            }
        }
#pragma unroll
        for (int u = 0; u < DPL; ++u) {
            const int d = lane + 64 * u;
            if (d < dh) g_q[r * inner + h * dh + d] = scale * gqv[u];
        }
    }
    float* part = parts + (size_t)blockIdx.y * part_stride;
    for (int half = 0; half < 2; ++half) {              // d/d k of the tokens, then d/d v, through the same LDS table
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
#pragma unroll
            for (int u = 0; u < DPL; ++u) sacc[wave][t][lane + 64 * u] = half ? gv[t][u] : gk[t][u];
        __syncthreads();
        for (int idx = threadIdx.x; idx < T * dh; idx += 256) {
            const int t = idx / dh, d = idx - t * dh;
            part[((size_t)b * T + t) * 2 * inner + half * inner + h * dh + d] =
                ((sacc[0][t][d] + sacc[1][t][d]) + sacc[2][t][d]) + sacc[3][t][d];
        }
        __syncthreads();
    }
}

// ---- exact GELU (nn.GELU default; the forward's epilogue, linear_hl.hip ACT == 2) and its derivative Phi(z) + z phi(z)
__device__ __forceinline__ void gelu_pair(float z, float g, float& a, float& gz)
{
    const float cdf = 0.5f * (1.0f + erff(z * 0.70710678118654752f));
    const float pdf = 0.3989422804014327f * expf(-0.5f * z * z);
    a = z * cdf;
    gz = g * (cdf + z * pdf);
}

__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float* z, const float* g, float* a_out, float* gz_out, int64_t count,
                                                       uint32_t* amax_bits)
{
    __shared__ uint32_t slot_a, slot_g;
    uint32_t ma = 0u, mg = 0u;
    const int64_t quads = count >> 2;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (int64_t)gridDim.x * 256) {
        const f32x4 zv = reinterpret_cast<const f32x4*>(z)[i];
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 av, dv;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float a, d;
            gelu_pair(zv[u], gv[u], a, d);
            av[u] = a; dv[u] = d;
            const uint32_t ta = egnn_abs_bits(a), tg = egnn_abs_bits(d);
            ma = ma > ta ? ma : ta;
            mg = mg > tg ? mg : tg;
        }
        reinterpret_cast<f32x4*>(a_out)[i] = av;
        reinterpret_cast<f32x4*>(gz_out)[i] = dv;
    }
    if (blockIdx.x == 0) {                              // count % 4 elements at the end
        const int64_t i = quads * 4 + threadIdx.x;
        if (threadIdx.x < 3 && i < count) {
            float a, d;
            gelu_pair(z[i], g[i], a, d);
            a_out[i] = a; gz_out[i] = d;
            const uint32_t ta = egnn_abs_bits(a), tg = egnn_abs_bits(d);
            ma = ma > ta ? ma : ta;
            mg = mg > tg ? mg : tg;
        }
    }
    if (amax_bits) {
        egnn_block_absmax_commit(ma, &slot_a, amax_bits);
        egnn_block_absmax_commit(mg, &slot_g, amax_bits + 1);
    }
}

// ---- LayerNorm backward over node rows: one wave per row, lane l owns columns l, l + 64, ...; x_hat and 1 / sigma recomputed from the
// saved input row with the forward's two-pass statistics.  g_x = (g_hat - mean(g_hat) - x_hat mean(g_hat x_hat)) / sigma (+ add),
// g_hat = g gamma; the column sums sum_rows g x_hat (d/d gamma) and sum_rows g (d/d beta): registers -> LDS -> one row of `parts` per
// workgroup.
template <int U>
__global__ __launch_bounds__(256) void layer_norm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                             const float* __restrict__ gamma, float eps, const float* __restrict__ add,
                                                             int64_t rows, int dim, float* __restrict__ g_x, float* __restrict__ parts)
{
    __shared__ float sp[4][2][64 * U];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float gam[U], ag[U], ab[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int c = lane + 64 * u;
        gam[u] = c < dim ? gamma[c] : 0.f;
        ag[u] = 0.f; ab[u] = 0.f;
    }
    const float inv_dim = 1.0f / (float)dim;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
        float xv[U], gv[U];
        float s = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = lane + 64 * u;
            xv[u] = c < dim ? x[r * dim + c] : 0.f;
            gv[u] = c < dim ? g[r * dim + c] : 0.f;
            s += xv[u];
        }
        const float mean = egnn_wave_sum(s) * inv_dim;
        float v = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float d = (lane + 64 * u) < dim ? xv[u] - mean : 0.f;
            xv[u] = d;
            v += d * d;
        }
        const float rstd = 1.0f / sqrtf(egnn_wave_sum(v) * inv_dim + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            xv[u] *= rstd;                              // x_hat (0 beyond dim)
            const float gh = gv[u] * gam[u];
            s1 += gh;
            s2 += gh * xv[u];
            ag[u] += gv[u] * xv[u];
            ab[u] += gv[u];
        }
        const float m1 = egnn_wave_sum(s1) * inv_dim, m2 = egnn_wave_sum(s2) * inv_dim;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = lane + 64 * u;
            if (c < dim) {
                float out = (gv[u] * gam[u] - m1 - xv[u] * m2) * rstd;
                if (add) out += add[r * dim + c];
                g_x[r * dim + c] = out;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) { sp[wave][0][lane + 64 * u] = ag[u]; sp[wave][1][lane + 64 * u] = ab[u]; }
    __syncthreads();
    for (int idx = threadIdx.x; idx < 2 * dim; idx += 256) {
        const int j = idx / dim, c = idx - j * dim;
        parts[(size_t)blockIdx.x * 2 * dim + idx] = ((sp[0][j][c] + sp[1][j][c]) + sp[2][j][c]) + sp[3][j][c];
    }
}

int induced_chunking(int N, int* chunk_out)               // chunks of >= 64 nodes, at most 32 of them
{
    int nch = (N + 63) / 64;
    if (nch > IND_MAX_CHUNKS) nch = IND_MAX_CHUNKS;
    const int chunk = (N + nch - 1) / nch;
    if (chunk_out) *chunk_out = chunk;
    return (N + chunk - 1) / chunk;
}

int token_chunking(int N, int* chunk_out)
{
    int nch = (N + 63) / 64;
    if (nch > TOK_MAX_CHUNKS) nch = TOK_MAX_CHUNKS;
    const int chunk = (N + nch - 1) / nch;
    if (chunk_out) *chunk_out = chunk;
    return (N + chunk - 1) / chunk;
}

}  // namespace

extern "C" int64_t egnn_induced_attn_bwd_work_floats(int B, int N, int T, int heads, int dim_head)
{
    if (B <= 0 || N <= 0 || T < 1 || heads < 1 || dim_head < 1) return 0;
    const int64_t nch = induced_chunking(N, nullptr);
    return nch * ((int64_t)B * heads * TMAX * 2 + (int64_t)B * T * heads * dim_head);
}

extern "C" int egnn_induced_attn_bwd_f32(const float* q, const float* kv, int64_t ldkv, const uint8_t* mask, const float* o, const float* g_o,
                                         int B, int N, int T, int heads, int dim_head, float scale, float* work, float* g_q, float* g_kv,
                                         void* stream)
{
    if (!q || !kv || !o || !g_o || !work || !g_q || !g_kv) return EGNN_E_NULLPTR;
    if (B <= 0 || N <= 0 || T < 1 || heads < 1 || dim_head < 1 || ldkv < 2 * (int64_t)heads * dim_head) return EGNN_E_SHAPE;
    if (T > TMAX || dim_head > 64 * DPL_MAX || (int64_t)B * heads > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int chunk = 0;
    const int nch = induced_chunking(N, &chunk);
    float* stats = work;                                                   // (B heads, chunks, TMAX, 2)
    float* parts = work + (size_t)nch * B * heads * TMAX * 2;              // (chunks, B, T, inner)
    const int64_t stride = (int64_t)B * T * heads * dim_head;
    const dim3 grid((unsigned)(B * heads), (unsigned)nch), block(256);
#define EGNN_IND_BWD(D) do { \
        hipLaunchKernelGGL(induced_stats_kernel<D>, grid, block, 0, s, q, kv, ldkv, mask, N, T, heads, dim_head, scale, chunk, stats); \
        hipLaunchKernelGGL(induced_attn_bwd_kernel<D>, grid, block, 0, s, q, kv, ldkv, mask, o, g_o, N, T, heads, dim_head, scale, chunk, \
                           stats, parts, stride, g_kv); } while (0)
    if (dim_head <= 64) EGNN_IND_BWD(1);
    else if (dim_head <= 128) EGNN_IND_BWD(2);
    else EGNN_IND_BWD(4);
#undef EGNN_IND_BWD
    int rc = egnn_launch_status();
    if (rc != EGNN_OK) return rc;
    launch_parts_sum(parts, nch, stride, g_q, s);
    return egnn_launch_status();
}

extern "C" int egnn_token_attn_bwd_chunks(int N)
{
    return N > 0 ? token_chunking(N, nullptr) : 0;
}

extern "C" int egnn_token_attn_bwd_f32(const float* q, int64_t ldq, const float* kv_tok, const float* g_out, int64_t ldg, int B, int N, int T,
                                       int heads, int dim_head, float scale, float* g_q, float* parts, float* g_kv_tok, void* stream)
{
    if (!q || !kv_tok || !g_out || !g_q || !parts || !g_kv_tok) return EGNN_E_NULLPTR;
    const int64_t inner = (int64_t)heads * dim_head;
    if (B <= 0 || N <= 0 || T < 1 || heads < 1 || dim_head < 1 || ldq < inner || ldg < inner) return EGNN_E_SHAPE;
    if (T > TMAX || dim_head > 64 * DPL_MAX || (int64_t)B * heads > 0x7fffffffLL) return EGNN_E_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int chunk = 0;
    const int nch = token_chunking(N, &chunk);
    const int64_t stride = (int64_t)B * T * 2 * inner;
    const dim3 grid((unsigned)(B * heads), (unsigned)nch), block(256);
    if (dim_head <= 64) hipLaunchKernelGGL(token_attn_bwd_kernel<1>, grid, block, 0, s, q, ldq, kv_tok, g_out, ldg, N, T, heads, dim_head, scale, chunk, g_q, parts, stride);
    else if (dim_head <= 128) hipLaunchKernelGGL(token_attn_bwd_kernel<2>, grid, block, 0, s, q, ldq, kv_tok, g_out, ldg, N, T, heads, dim_head, scale, chunk, g_q, parts, stride);
    else hipLaunchKernelGGL(token_attn_bwd_kernel<4>, grid, block, 0, s, q, ldq, kv_tok, g_out, ldg, N, T, heads, dim_head, scale, chunk, g_q, parts, stride);
    int rc = egnn_launch_status();
    if (rc != EGNN_OK) return rc;
    launch_parts_sum(parts, nch, stride, g_kv_tok, s);
    return egnn_launch_status();
}

extern "C" int egnn_gelu_bwd_f32(const float* z, const float* g, float* a_out, float* gz_out, int64_t count, uint32_t* amax_bits, void* stream)
{
    if (!z || !g || !a_out || !gz_out) return EGNN_E_NULLPTR;
    if (count <= 0) return EGNN_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(a_out) | reinterpret_cast<uintptr_t>(gz_out)) & 15)
        return EGNN_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int64_t blocks = (count / 4 + 256 * 4 - 1) / (256 * 4);
    blocks = blocks < 1 ? 1 : (blocks > 8192 ? 8192 : blocks);
    if (amax_bits && hipMemsetAsync(amax_bits, 0, 2 * sizeof(uint32_t), s) != hipSuccess) return (int)hipGetLastError();
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, s, z, g, a_out, gz_out, count, amax_bits);
    return egnn_launch_status();
}

extern "C" int egnn_layer_norm_bwd_parts(int64_t rows)
{
    if (rows <= 0) return 0;
    const int64_t blocks = (rows + 3) / 4;
    return (int)(blocks > LN_MAX_BLOCKS ? LN_MAX_BLOCKS : blocks);
}

extern "C" int egnn_layer_norm_bwd_f32(const float* x, const float* g, const float* gamma, float eps, const float* add, int64_t rows, int dim,
                                       float* g_x, float* parts, float* g_gamma_beta, void* stream)
{
    if (!x || !g || !gamma || !g_x || !parts || !g_gamma_beta) return EGNN_E_NULLPTR;
    if (rows <= 0 || dim <= 0) return EGNN_E_SHAPE;
    if (dim > 64 * LN_UMAX) return EGNN_E_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int blocks = egnn_layer_norm_bwd_parts(rows);
    const dim3 grid((unsigned)blocks), block(256);
#define EGNN_LN_BWD(U) hipLaunchKernelGGL(layer_norm_bwd_kernel<U>, grid, block, 0, s, x, g, gamma, eps, add, rows, dim, g_x, parts)
    if (dim <= 64) EGNN_LN_BWD(1);
    else if (dim <= 128) EGNN_LN_BWD(2);
    else if (dim <= 256) EGNN_LN_BWD(4);
    else if (dim <= 512) EGNN_LN_BWD(8);
    else EGNN_LN_BWD(16);
#undef EGNN_LN_BWD
    int rc = egnn_launch_status();
    if (rc != EGNN_OK) return rc;
    launch_parts_sum(parts, blocks, 2 * (int64_t)dim, g_gamma_beta, s);
    return egnn_launch_status();
}

// What the per-graph kernels of a packed batch (segment_reduce.hip, segment_softmax.hip) agree on, stated once: the chunk of R rows a
// workgroup owns, the strands a chunk's rows are dealt to, the four adjacent columns of a thread and how they are loaded, and the
// partial slots of the graphs longer than a chunk.  THE ORDER these pieces add up to is written down in segment_reduce.hip and in
// DESIGN.md §4.1a; every kernel takes the pieces from here, never from a copy of them.
#pragma once
#include "egnn_common.h"

namespace {

constexpr int SR_THREADS = 256;
constexpr int SR_ROWS = 128;                             // R: rows of a chunk

typedef double f64x2 __attribute__((ext_vector_type(2)));

int sr_col_threads_log2(int D)
{
    const int groups = (D + 3) / 4;
    int l = 0;
    while ((1 << l) < groups && l < 4) ++l;
    return l;
}

// partial slots a batch can need: only the chunks of segments longer than R are parked, at most n / R + 1 each
size_t sr_slots(int64_t G, int64_t T)
{
    const int64_t full = T / SR_ROWS;
    return (size_t)((G < full ? G : full) + full + 1);
}
size_t sr_up256(size_t b) { return (b + 255) / 256 * 256; }
size_t sr_workspace_bytes(int64_t G, int64_t T, int64_t D, size_t elem) { return sr_up256(sr_slots(G, T) * (size_t)D * elem) + sr_up256(sr_slots(G, T) * (size_t)D * 4); }

// 4 adjacent elements of a row, from column c on.  VEC: 16-byte loads (c + 3 < D: D % 4 == 0); else scalar loads, `fill` past D.
template <typename T, bool VEC>
__device__ __forceinline__ void sr_load4(const T* __restrict__ p, int c, int D, T fill, T (&v)[4])
{
    if constexpr (VEC && sizeof(T) == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else if constexpr (VEC) {
        const f64x2 a = *reinterpret_cast<const f64x2*>(p), b = *reinterpret_cast<const f64x2*>(p + 2);
        v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = c + u < D ? p[u] : fill;
    }
}

struct SrChunk {
    int seg;
    int64_t n, r0;                                       // the segment's size, the chunk's first row
    int m;                                               // the chunk's rows
};

__device__ __forceinline__ SrChunk sr_chunk(const int64_t* __restrict__ offsets, const int32_t* __restrict__ chunk_row,
                                            const int32_t* __restrict__ chunk_seg, int chunk, int G, int64_t NT)
{
    SrChunk k;
    const int s = chunk_seg[chunk];
    k.seg = s < 0 ? 0 : (s >= G ? G - 1 : s);
    int64_t lo = offsets[k.seg], hi = offsets[k.seg + 1];
    lo = lo < 0 ? 0 : (lo > NT ? NT : lo);
    hi = hi > NT ? NT : (hi < lo ? lo : hi);
    int64_t r0 = chunk_row[chunk];
    r0 = r0 < lo ? lo : (r0 > hi ? hi : r0);
    k.n = hi - lo;
    k.r0 = r0;
    k.m = (int)(hi - r0 < SR_ROWS ? hi - r0 : SR_ROWS);
    return k;
}

}  // namespace

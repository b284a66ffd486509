"""The addition order of `GraphSegments.reduce(x, "sum")` on the device (csrc/segment_reduce.hip), restated in numpy with
explicit additions in the working precision -- what the kernel must reproduce element for element -- and the depth of that order: the
largest number of additions any one input passes through, which is what the standard error bound of a summation scales with.

The order for one graph of n rows and D columns (a function of n and D, nothing else):
  chunks   rows [k R, min(n, (k + 1) R)) of the graph, R = 128;
  strands  S = 256 / TC, TC = the power of two >= ceil(D / 4), at most 16; strand s starts at +0 and adds the chunk's rows
           s, s + S, s + 2 S, ... in that order;
  tree     for h = S / 2, S / 4, ..., 1: strand s < h adds strand s + h; strand 0 is the chunk's partial;
  combine  p0, + p1, + p2, ... in chunk order.
Every column of a row goes the same way (the strand of a value depends on its row only), so the restatement adds whole rows."""
import numpy as np

R = 128
THREADS = 256


def strands(d):
    groups = (d + 3) // 4
    tc = 1
    while tc < groups and tc < 16:
        tc *= 2
    return THREADS // tc


def chunks(n):
    """[(first row, rows)] of a graph of n rows, from its own first row; an empty graph is one chunk without rows"""
    if n == 0:
        return [(0, 0)]
    return [(k, min(R, n - k)) for k in range(0, n, R)]


def strand_rows(m, s_count):
    """the rows of a chunk of m rows that each strand adds, in order"""
    return [list(range(s, m, s_count)) for s in range(s_count)]


def chunk_partial(x):
    """x: (m, D) rows of one chunk, m <= R, already in the working dtype -> (D,)"""
    m, d = x.shape
    s_count = strands(d)
    acc = np.zeros((s_count, d), dtype=x.dtype)
    for first in range(0, m, s_count):                   # round j: strand s adds row first + s
        rows = x[first:first + s_count]
        acc[:rows.shape[0]] = acc[:rows.shape[0]] + rows
    h = s_count // 2
    while h >= 1:
        acc[:h] = acc[:h] + acc[h:2 * h]
        h //= 2
    return acc[0].copy()


def segment_sum(x):
    """x: (n, D) float32 / float64 rows of ONE graph -> (D,) in the same dtype, added in the documented order"""
    assert x.ndim == 2 and x.dtype in (np.float32, np.float64)
    parts = [chunk_partial(x[a:a + m]) for a, m in chunks(x.shape[0])]
    total = parts[0]
    for p in parts[1:]:
        total = total + p
    return total


def batch_sum(x, sizes):
    """x: (T, D), sizes of the graphs -> (G, D)"""
    out, a = [], 0
    for n in sizes:
        out.append(segment_sum(x[a:a + n]))
        a += n
    return np.stack(out)


def depth(n, d):
    """the largest number of additions one input of a graph of n rows and d columns passes through: the strand's own additions (its
    first row starts the sum: +0 is exact), the levels of the tree, the partials before the last"""
    if n == 0:
        return 0
    s_count = strands(d)
    per_strand = -(-min(n, R) // s_count)
    levels = s_count.bit_length() - 1
    return max(per_strand - 1, 0) + levels + (len(chunks(n)) - 1)

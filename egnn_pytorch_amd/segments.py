"""`GraphSegments`: the boundaries of a PACKED batch -- the nodes of G graphs of any sizes concatenated as (T, ...) rows, graph g owning
the rows offsets[g] : offsets[g + 1] -- the layout molecular and protein data loaders produce (PyG's `batch` vector, a list of sizes).

`EGNN.forward(feats, coors, mask=segments)` and `EGNN_Network.forward(...)` take one where they take the node mask of a padded batch,
with feats (T, dim) and coors (T, C), and return (T, dim) and (T, C): what the padded call with a prefix mask returns on the real nodes,
without allocating, reading or writing a padded row.  To the kernels a packed batch is ONE graph of T nodes whose neighbour lists never
cross a segment boundary; the segmented selection (csrc/knn_segments.hip, `_ops.knn_select_segments`) is what keeps them inside.

It is built once by the caller, like `SparseAdjacency`, and keeps the offsets on the device (for the kernel) and on the host (sizes,
the largest graph, the chunking of `split`): no forward synchronises to read them.  Construction, `pack` and `unpack` are ordinary
tensor code on whatever device the inputs live on, so they work on CPU tensors.

Graph-level work stays packed: `reduce` takes (T, ...) node rows to (G, ...) graph rows (sum, mean, max, min), `broadcast` goes back and
`center` removes every graph's mean.  On the device they run the ordered, atomic-free kernels of csrc/segment_reduce.hip -- the bits
of a graph's result depend on its own rows only -- and are differentiable to any order; on CPU tensors, ordinary torch code with the
same tie and empty-graph rules.  `softmax`, `logsumexp` and `attention_pool` normalise node scores over the nodes of each graph and pool
node features with those weights (csrc/segment_softmax.hip: the same order, no atomics, one pass over the values), with torch's NaN and
-inf rules on the rows of each graph.
"""
from __future__ import annotations

import collections

import torch

# rows of a chunk of the segmented reduction (csrc/segment_reduce.hip: SR_ROWS; egnn_segment_reduce_chunk_rows() of the library)
SEGMENT_CHUNK_ROWS = 128

_ReduceTables = collections.namedtuple("_ReduceTables", "chunk_row chunk_seg chunk_slot n_chunks multi_seg multi_slot n_multi")


class GraphSegments:
    def __init__(self, offsets, device=None, validate=True):
        """The raw constructor (`from_offsets`).  offsets: int64 (G + 1,), offsets[0] = 0, non-decreasing; a tensor (its device is the
        segments' unless `device` says otherwise: one device->host read) or a sequence of ints (no read)."""
        if torch.is_tensor(offsets):
            if offsets.dtype != torch.int64:
                raise TypeError(f"offsets must be int64 (got {offsets.dtype})")
            if offsets.dim() != 1 or offsets.numel() < 2:
                raise ValueError(f"offsets shape {tuple(offsets.shape)}: expected (G + 1,) with G >= 1")
            if device is None:
                device = offsets.device
            host = [int(v) for v in offsets.tolist()]
        else:
            host = list(offsets)
            if not all(isinstance(v, int) and not isinstance(v, bool) for v in host):
                raise TypeError("offsets must be an int64 tensor or a sequence of ints")
            if len(host) < 2:
                raise ValueError(f"offsets holds {len(host)} entries: expected G + 1 with G >= 1")
        if validate:
            if host[0] != 0:
                raise ValueError(f"offsets must start at 0 (got {host[0]})")
            if any(b < a for a, b in zip(host, host[1:])):
                raise ValueError("offsets must be non-decreasing")
            if host[-1] >= 2 ** 31:
                raise ValueError(f"a packed batch holds fewer than 2^31 nodes (got {host[-1]})")
        self._host = tuple(host)
        dev = torch.device("cpu" if device is None else device)
        self.offsets = torch.tensor(host, dtype=torch.int64, device=dev)
        self._derived = None
        self._slots = None                                   # (B, N) of the padded batch `from_mask` came from, and its real slots
        self._tables = None                                  # the chunk tables of `reduce` on the device
        self._inv = {}                                       # dtype -> (G, 1) 1 / size

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_offsets(cls, ptr, device=None):
        """From the (G + 1,) boundaries (PyG's `ptr`)."""
        return cls(ptr, device=device)

    @classmethod
    def from_sizes(cls, sizes, device=None):
        """From the node count of every graph: a sequence of ints or an int64 (G,) tensor; zeros (empty graphs) allowed."""
        if torch.is_tensor(sizes):
            if sizes.dtype != torch.int64:
                raise TypeError(f"sizes must be int64 (got {sizes.dtype})")
            if sizes.dim() != 1 or sizes.numel() < 1:
                raise ValueError(f"sizes shape {tuple(sizes.shape)}: expected (G,) with G >= 1")
            if device is None:
                device = sizes.device
            sizes = sizes.tolist()
        sizes = list(sizes)
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in sizes):
            raise TypeError("sizes must be an int64 tensor or a sequence of ints")
        if len(sizes) < 1:
            raise ValueError("sizes is empty: expected G >= 1 graphs")
        if any(v < 0 for v in sizes):
            raise ValueError("sizes must be non-negative")
        host = [0]
        for v in sizes:
            host.append(host[-1] + v)
        return cls(host, device=device)

    @classmethod
    def from_batch(cls, batch, num_graphs=None):
        """From a PyG-style (T,) int64 vector holding the graph of every node; it must be non-decreasing (the nodes of a graph are
        contiguous).  num_graphs: G when trailing graphs are empty; None: batch[-1] + 1."""
        if not torch.is_tensor(batch) or batch.dtype != torch.int64:
            raise TypeError(f"batch must be an int64 tensor (got {getattr(batch, 'dtype', type(batch).__name__)})")
        if batch.dim() != 1:
            raise ValueError(f"batch shape {tuple(batch.shape)}: expected (T,)")
        if batch.numel():
            if bool((batch[1:] < batch[:-1]).any()):
                raise ValueError("batch must be non-decreasing: the nodes of a graph are contiguous in a packed batch")
            if int(batch[0]) < 0:
                raise ValueError("batch holds a negative graph index")
        g = (int(batch[-1]) + 1 if batch.numel() else 1) if num_graphs is None else int(num_graphs)
        if g < 1 or (batch.numel() and int(batch[-1]) >= g):
            raise ValueError(f"batch names graph {int(batch[-1]) if batch.numel() else 0} of num_graphs = {g}")
        return cls.from_sizes(torch.bincount(batch, minlength=g), device=batch.device)

    @classmethod
    def from_mask(cls, mask):
        """From the (B, N) bool node mask of a padded batch -- any pattern, not only prefixes: graph b's nodes are its True slots in
        slot order.  `pack` then gathers exactly those slots and `unpack` scatters back to them."""
        if not torch.is_tensor(mask) or mask.dtype != torch.bool:
            raise TypeError(f"mask must be a torch.bool tensor (got {getattr(mask, 'dtype', type(mask).__name__)})")
        if mask.dim() != 2 or mask.shape[0] < 1:
            raise ValueError(f"mask shape {tuple(mask.shape)}: expected (B, N) with B >= 1")
        seg = cls.from_sizes(mask.sum(-1).to(torch.int64), device=mask.device)
        seg._slots = (tuple(mask.shape), mask.reshape(-1).nonzero().reshape(-1))
        return seg

    # ------------------------------------------------------------------ what the batch looks like
    @property
    def num_graphs(self):
        return len(self._host) - 1

    @property
    def num_nodes(self):
        return self._host[-1]

    @property
    def sizes(self):
        """the node count of every graph (host ints: no device read)"""
        return tuple(b - a for a, b in zip(self._host, self._host[1:]))

    @property
    def max_size(self):
        return max(self.sizes)

    @property
    def host_offsets(self):
        return self._host

    @property
    def device(self):
        return self.offsets.device

    def to(self, device):
        offsets = self.offsets.to(device)
        if offsets is self.offsets:                                  # (already there: Tensor.to returns the tensor itself)
            return self
        seg = GraphSegments(self._host, device=offsets.device, validate=False)
        if self._slots is not None:
            seg._slots = (self._slots[0], self._slots[1].to(offsets.device))
        return seg

    def _derive(self):
        if self._derived is None:
            sizes = self.offsets[1:] - self.offsets[:-1]
            seg = torch.repeat_interleave(torch.arange(self.num_graphs, device=self.device), sizes, output_size=self.num_nodes)
            pos = torch.arange(self.num_nodes, device=self.device) - self.offsets[:-1][seg]
            self._derived = (seg.to(torch.int32), pos)
        return self._derived

    @property
    def segment_of(self):
        """int32 (T,): the graph of every row"""
        return self._derive()[0]

    @property
    def positions(self):
        """int64 (T,): the index of every node inside its graph"""
        return self._derive()[1]

    # ------------------------------------------------------------------ padded <-> packed
    def _padded_slots(self, b, n):
        """flat slot (b N + position) of every packed row in a padded (B, N) batch"""
        if self._slots is not None and self._slots[0] == (b, n):
            return self._slots[1]
        return self.segment_of.to(torch.int64) * n + self.positions

    def pack(self, x):
        """(B, N, ...) padded -> (T, ...): graph g's nodes are x[g, :sizes[g]] (after `from_mask`: the mask's True slots of x[g]).
        Differentiable."""
        if x.dim() < 2 or x.shape[0] != self.num_graphs:
            raise ValueError(f"pack: x shape {tuple(x.shape)}: expected ({self.num_graphs}, N, ...)")
        b, n = x.shape[:2]
        if self._slots is not None and self._slots[0] != (b, n):
            raise ValueError(f"pack: x shape {tuple(x.shape)}: these segments come from a mask of shape {self._slots[0]}")
        if n < self.max_size:
            raise ValueError(f"pack: x holds {n} slots per graph, the largest graph {self.max_size} nodes")
        return x.reshape(b * n, *x.shape[2:]).index_select(0, self._padded_slots(b, n))

    def unpack(self, x, fill=0):
        """(T, ...) -> (B, N_max, ...) padded, `fill` in the slots no node owns (after `from_mask`: (B, N) of the mask, nodes back in
        their slots).  Differentiable."""
        if x.dim() < 1 or x.shape[0] != self.num_nodes:
            raise ValueError(f"unpack: x shape {tuple(x.shape)}: expected ({self.num_nodes}, ...)")
        b, n = self._slots[0] if self._slots is not None else (self.num_graphs, self.max_size)
        out = x.new_full((b * n, *x.shape[1:]), fill)
        return out.index_copy(0, self._padded_slots(b, n), x).reshape(b, n, *x.shape[1:])

    def prefix_mask(self):
        """bool (G, N_max): the node mask of the padded batch `unpack` builds (without `from_mask`)"""
        sizes = self.offsets[1:] - self.offsets[:-1]
        return torch.arange(self.max_size, device=self.device)[None, :] < sizes[:, None]

    # ------------------------------------------------------------------ readout: node rows <-> graph rows
    def _reduce_tables(self):
        """The chunk tables of csrc/segment_reduce.hip (include/egnn_hip.h: egnn_segment_reduce_f32), built on the host from the host
        offsets, uploaded once and kept: every graph cut into chunks of SEGMENT_CHUNK_ROWS rows from its own first row (an empty graph:
        one chunk without rows); the chunks of a graph that has several own consecutive partial slots."""
        if self._tables is None:
            r = SEGMENT_CHUNK_ROWS
            off = torch.tensor(self._host, dtype=torch.int64)
            sizes = off[1:] - off[:-1]
            nch = torch.clamp((sizes + (r - 1)) // r, min=1)
            seg = torch.repeat_interleave(torch.arange(self.num_graphs), nch)
            first = torch.cumsum(nch, 0) - nch                                       # the first chunk of every graph
            row = off[:-1][seg] + (torch.arange(seg.numel()) - first[seg]) * r
            multi = nch > 1
            slot0 = torch.cumsum(torch.where(multi, nch, torch.zeros_like(nch)), 0) - nch   # (read at the graphs of several chunks only)
            slot = torch.where(multi[seg], slot0[seg] + (torch.arange(seg.numel()) - first[seg]), torch.full_like(seg, -1))
            mseg = multi.nonzero().reshape(-1)

            def up(t):
                return t.to(torch.int32).to(self.device)

            self._tables = _ReduceTables(up(row), up(seg), up(slot), int(seg.numel()), up(mseg) if mseg.numel() else None,
                                         up(slot0[mseg]) if mseg.numel() else None, int(mseg.numel()))
        return self._tables

    def _inv_sizes(self, dtype):
        """(G, 1): 1 / n of every graph, 0 for an empty one -- host sizes, uploaded once per dtype"""
        if dtype not in self._inv:
            self._inv[dtype] = torch.tensor([1.0 / n if n else 0.0 for n in self.sizes], dtype=torch.float64).to(dtype).to(self.device)[:, None]
        return self._inv[dtype]

    def _readout_rows(self, x, rows, what, lead):
        """the checks of `reduce` / `broadcast` -> x as a (rows, D) matrix in the dtype the kernels run (float32 or float64)"""
        if not torch.is_tensor(x):
            raise TypeError(f"{what}: expected a tensor (got {type(x).__name__})")
        if not x.dtype.is_floating_point:
            raise TypeError(f"{what} takes floating-point values (got {x.dtype})")
        if x.dim() < 1 or x.shape[0] != rows:
            raise ValueError(f"{what}: x shape {tuple(x.shape)}: expected ({rows}, ...): one row per {lead} of these segments")
        if x.device != self.device:
            raise RuntimeError(f"Expected all tensors to be on the same device: x is on {x.device}, the segments on {self.device}")
        d = 1
        for v in x.shape[1:]:
            d *= v
        if d < 1:
            raise ValueError(f"{what}: x shape {tuple(x.shape)} holds no column")
        x2 = x.reshape(rows, d)
        if x2.dtype in (torch.float16, torch.bfloat16):
            x2 = x2.float()                                                          # accumulated in fp32, returned in the caller's dtype
        return x2

    def reduce(self, x, op="sum"):
        """(T, ...) node rows -> (G, ...) graph rows: op "sum", "mean", "max" or "min" over the nodes of every graph, per column.
        Empty graphs give 0 for sum / mean (zero gradient); max / min of a batch that holds one raise ValueError.  max / min: a NaN
        wins (as in torch.amax), ties go to the lowest row, and the gradient goes to that row alone.  On the device: the ordered,
        atomic-free kernels of csrc/segment_reduce.hip -- a graph's bits depend on its own rows only, not on the batch around it;
        float16 / bfloat16 accumulate in fp32.  Differentiable to any order; reads nothing back."""
        if op not in ("sum", "mean", "max", "min"):
            raise ValueError(f"reduce: op = {op!r}: expected \"sum\", \"mean\", \"max\" or \"min\"")
        x2 = self._readout_rows(x, self.num_nodes, "reduce", "node")
        if op in ("max", "min") and min(self.sizes) == 0:
            raise ValueError(f"reduce: {op} of an empty graph is undefined (graph {self.sizes.index(0)} holds no node)")
        if op in ("sum", "mean"):
            if self.num_nodes == 0:
                out = x2.new_zeros(self.num_graphs, x2.shape[1]) + x2.sum(0, keepdim=True)
            elif x2.is_cuda:
                out = _SegmentSum.apply(x2, self, op == "mean")
            else:
                out = torch.zeros(self.num_graphs, x2.shape[1], dtype=x2.dtype).index_add(0, self.segment_of.to(torch.int64), x2)
                if op == "mean":
                    out = out * self._inv_sizes(x2.dtype)
        elif x2.is_cuda:
            out = _SegmentExtreme.apply(x2, self, op == "max")
        else:
            out = x2.gather(0, self._winners_host(x2.detach(), op == "max").to(torch.int64))
        return out.to(x.dtype).reshape(self.num_graphs, *x.shape[1:])

    def _winners_host(self, x2, is_max):
        """CPU tensors: int32 (G, D), the row `reduce` selects -- the first NaN of a column, else the first occurrence of the extreme"""
        rows = []
        for a, b in zip(self._host, self._host[1:]):
            s = x2[a:b]
            best = s.amax(0, keepdim=True) if is_max else s.amin(0, keepdim=True)
            hit = torch.where(torch.isnan(best), torch.isnan(s), s == best)
            at = torch.arange(a, b, dtype=torch.int64)[:, None].expand_as(s)
            rows.append(torch.where(hit, at, torch.full_like(at, b)).amin(0))
        return torch.stack(rows).to(torch.int32)

    def broadcast(self, g):
        """(G, ...) graph rows -> (T, ...): every node receives its graph's row.  Differentiable to any order (its backward is
        reduce "sum")."""
        g2 = self._readout_rows(g, self.num_graphs, "broadcast", "graph")
        if self.num_nodes == 0:
            out = g2[:0]
        elif g2.is_cuda:
            out = _SegmentBroadcast.apply(g2, self)
        else:
            out = g2.index_select(0, self.segment_of.to(torch.int64))
        return out.to(g.dtype).reshape(self.num_nodes, *g.shape[1:])

    def center(self, x):
        """x - broadcast(reduce(x, "mean")): every graph moved to zero mean (coordinates: the zero-centre-of-mass projection)"""
        return x - self.broadcast(self.reduce(x, "mean"))

    # ------------------------------------------------------------------ per-graph softmax: normalised node scores, learned readouts
    def _graph_rows(self):
        return zip(self._host, self._host[1:])

    def softmax(self, x):
        """(T, ...) -> (T, ...): the softmax over the nodes of every graph, per column -- torch.softmax(x[a:b], 0) on the rows [a, b) of
        each graph.  A NaN makes its (graph, column) NaN and touches nothing else; a column that is all -inf gives NaN; -inf next to a
        finite score gives exactly 0.  On the device: the ordered, atomic-free kernels of csrc/segment_softmax.hip (a graph's bits depend
        on its own rows only); float16 / bfloat16 are computed in fp32.  Differentiable to any order; reads nothing back."""
        x2 = self._readout_rows(x, self.num_nodes, "softmax", "node")
        if x2.is_cuda and self.num_nodes > 0:
            y = _SegmentSoftmax.apply(x2, self)
        else:
            y = torch.cat([torch.softmax(x2[a:b], 0) for a, b in self._graph_rows()])
        return y.to(x.dtype).reshape(x.shape)

    def logsumexp(self, x):
        """(T, ...) -> (G, ...): torch.logsumexp(x[a:b], 0) on the rows of every graph, per column; an empty graph and a column that is
        all -inf give -inf.  Device, dtypes and autograd as `softmax`."""
        x2 = self._readout_rows(x, self.num_nodes, "logsumexp", "node")
        if x2.is_cuda and self.num_nodes > 0:
            out = _SegmentLogSumExp.apply(x2, self)
        else:
            out = torch.stack([torch.logsumexp(x2[a:b], 0) for a, b in self._graph_rows()])
        return out.to(x.dtype).reshape(self.num_graphs, *x.shape[1:])

    def attention_pool(self, scores, values):
        """scores (T, H), values (T, H, Dv) -> (G, H, Dv): (torch.softmax(scores[a:b], 0)[..., None] * values[a:b]).sum(0) on the rows of
        every graph -- a learned readout with H heads; the shorthand scores (T,), values (T, Dv) -> (G, Dv) is H = 1.  An empty graph gives
        a row of zeros with zero gradient; NaN and -inf as `softmax`.  On the device one pass over `values` (csrc/segment_softmax.hip)
        that forms neither the weights nor the products in memory; float16 / bfloat16 are computed in fp32.  Differentiable to any
        order; reads nothing back."""
        t = self.num_nodes
        for what, v in (("scores", scores), ("values", values)):
            if not torch.is_tensor(v):
                raise TypeError(f"attention_pool: {what}: expected a tensor (got {type(v).__name__})")
            if not v.dtype.is_floating_point:
                raise TypeError(f"attention_pool takes floating-point {what} (got {v.dtype})")
        if scores.dtype != values.dtype:
            raise TypeError(f"attention_pool: scores are {scores.dtype}, values {values.dtype}: expected one dtype")
        if scores.dim() not in (1, 2) or scores.shape[0] != t or (scores.dim() == 2 and scores.shape[1] < 1):
            raise ValueError(f"attention_pool: scores shape {tuple(scores.shape)}: expected ({t}, H) with H >= 1, or ({t},): one row per node "
                             f"of these segments")
        want = (t, "Dv") if scores.dim() == 1 else (t, scores.shape[1], "Dv")
        if values.dim() != scores.dim() + 1 or values.shape[:-1] != scores.shape or values.shape[-1] < 1:
            raise ValueError(f"attention_pool: values shape {tuple(values.shape)}: expected ({', '.join(str(v) for v in want)}) with Dv >= 1 "
                             f"for scores of shape {tuple(scores.shape)}")
        for what, v in (("scores", scores), ("values", values)):
            if v.device != self.device:
                raise RuntimeError(f"Expected all tensors to be on the same device: {what} is on {v.device}, the segments on {self.device}")
        h = 1 if scores.dim() == 1 else scores.shape[1]
        s2, v3 = scores.reshape(t, h), values.reshape(t, h, values.shape[-1])
        if s2.dtype in (torch.float16, torch.bfloat16):
            s2, v3 = s2.float(), v3.float()                                              # computed in fp32, returned in the caller's dtype
        if s2.is_cuda and t > 0:
            out = _SegmentPool.apply(s2, v3, self)
        else:
            out = torch.stack([(torch.softmax(s2[a:b], 0)[..., None] * v3[a:b]).sum(0) if b > a else v3.new_zeros(v3.shape[1:])
                               for a, b in self._graph_rows()])
        return out.to(values.dtype).reshape(self.num_graphs, *values.shape[1:])

    # ------------------------------------------------------------------ chunks
    def split(self, max_nodes):
        """Yields (row_slice, GraphSegments) pieces cut at graph boundaries, each with at most `max_nodes` rows -- greedily, in order.
        A single graph larger than `max_nodes` forms a piece of its own (with the empty graphs next to it: no piece is without rows
        unless the whole batch is)."""
        max_nodes = int(max_nodes)
        if max_nodes < 1:
            raise ValueError(f"split: max_nodes = {max_nodes}")
        off, g = self._host, self.num_graphs
        start = 0
        while start < g:
            end = start + 1
            while end < g and (off[end] == off[start] or off[end + 1] == off[end] or off[end + 1] - off[start] <= max_nodes):
                end += 1
            piece = GraphSegments([v - off[start] for v in off[start:end + 1]], device=self.device, validate=False)
            yield slice(off[start], off[end]), piece
            start = end

    def __repr__(self):
        return f"GraphSegments(graphs={self.num_graphs}, nodes={self.num_nodes}, max_size={self.max_size}, device={self.device})"


# ---------------------------------------------------------------------- the readout under autograd (device tensors)
# Each backward is a call of another Function of this group, so a graph recorded with create_graph=True differentiates again without a
# path of its own: sum / mean <-> broadcast, max / min -> scatter to the winning rows <-> gather at them.
class _SegmentSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seg, mean):
        from . import _ops
        ctx.seg, ctx.mean = seg, mean
        return _ops.segment_reduce(x, seg, "mean" if mean else "sum")

    @staticmethod
    def backward(ctx, g):
        if ctx.mean:
            g = g * ctx.seg._inv_sizes(g.dtype)
        return _SegmentBroadcast.apply(g, ctx.seg), None, None


class _SegmentBroadcast(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, seg):
        from . import _ops
        ctx.seg = seg
        return _ops.segment_broadcast(g, seg)

    @staticmethod
    def backward(ctx, g):
        return _SegmentSum.apply(g, ctx.seg, False), None


class _SegmentExtreme(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seg, is_max):
        from . import _ops
        out, rows = _ops.segment_reduce(x, seg, "max" if is_max else "min")
        ctx.seg, ctx.rows = seg, rows
        return out

    @staticmethod
    def backward(ctx, g):
        return _SegmentScatter.apply(g, ctx.rows, ctx.seg), None, None


class _SegmentScatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, rows, seg):
        from . import _ops
        ctx.seg, ctx.rows = seg, rows
        return _ops.segment_scatter_rows(g, rows, seg)

    @staticmethod
    def backward(ctx, g):
        return _SegmentGather.apply(g, ctx.rows, ctx.seg), None, None


class _SegmentGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, rows, seg):
        from . import _ops
        ctx.seg, ctx.rows = seg, rows
        return _ops.segment_gather_rows(x, rows, seg)

    @staticmethod
    def backward(ctx, g):
        return _SegmentScatter.apply(g, ctx.rows, ctx.seg), None, None


# ---------------------------------------------------------------------- the per-graph softmax under autograd (device tensors)
# softmax saves its OUTPUT, whose history is the Function itself, and its backward is made of differentiable pieces (products,
# _SegmentSum, _SegmentBroadcast): recorded with create_graph=True it differentiates again.  logsumexp and the pool run their kernels
# for the ordinary first-order step and, when the backward itself is being recorded, the same formula through the Functions.
class _SegmentSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seg):
        from . import _ops
        m, l = _ops.segment_softmax_stats(x, seg)
        y = _ops.segment_softmax_apply(x, m, l, seg)
        ctx.seg = seg
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return y * (g - _SegmentBroadcast.apply(_SegmentSum.apply(y * g, ctx.seg, False), ctx.seg)), None


def _lse_of_stats(m, l):
    """m + log(l); m itself where it is infinite (a column of -inf, an empty graph: -inf; a +inf score: +inf, as torch.logsumexp)"""
    return torch.where(torch.isinf(m), m, m + torch.log(l))


class _SegmentLogSumExp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seg):
        from . import _ops
        m, l = _ops.segment_softmax_stats(x, seg)
        ctx.seg, ctx.stats = seg, (m, l)
        ctx.save_for_backward(x)
        return _lse_of_stats(m, l)

    @staticmethod
    def backward(ctx, g):
        from . import _ops
        x, = ctx.saved_tensors
        y = _SegmentSoftmax.apply(x, ctx.seg) if torch.is_grad_enabled() else _ops.segment_softmax_apply(x, *ctx.stats, ctx.seg)
        return _SegmentBroadcast.apply(g, ctx.seg) * y, None


class _SegmentPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, values, seg):
        from . import _ops
        m, l = _ops.segment_softmax_stats(scores, seg)
        out = _ops.segment_pool(scores, values, m, l, seg)
        ctx.seg, ctx.stats = seg, (m, l)
        ctx.save_for_backward(scores, values, out)
        return out

    @staticmethod
    def backward(ctx, g):
        from . import _ops
        scores, values, out = ctx.saved_tensors
        seg = ctx.seg
        if not torch.is_grad_enabled():
            d_scores, d_values = _ops.segment_pool_bwd(g, out, scores, values, *ctx.stats, seg)
            return d_scores, d_values, None
        # create_graph=True: d_values = w g, d_scores = w sum_c g (v - out), through the differentiable Functions (the saved `out`
        # carries this Function as its history)
        t, h, dv = values.shape
        w = _SegmentSoftmax.apply(scores, seg)
        gb = _SegmentBroadcast.apply(g.reshape(-1, h * dv), seg).reshape(t, h, dv)
        ob = _SegmentBroadcast.apply(out.reshape(-1, h * dv), seg).reshape(t, h, dv)
        return w * (gb * (values - ob)).sum(-1), w[..., None] * gb, None

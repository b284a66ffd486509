"""`SparseAdjacency`: the bonds of a graph as CSR rows instead of an (N, N) byte map.

`EGNN.forward(adj_mat=...)` takes one wherever it takes a dense boolean adjacency and returns the same bits as the same call with
`to_dense()` (the neighbour selection reads a sorted column range where the dense call reads a byte row: csrc/knn_stream.hip,
egnn_knn_select_csr_f32 / _f64).  `EGNN_Network(num_adj_degrees=...)` expands it on CSR rows as well (csrc/adj_csr.hip,
`_ops.adj_expand_csr`) and keeps the degree labels as a `SparseLabels`.  Nothing of size N^2 is built from it.

Storage: `rowptr` int64 (G, N + 1), G = 1 (one graph's rows, shared by every graph of a batch) or G = B, ABSOLUTE offsets into one flat
int32 `col`; row i of graph g is col[rowptr[g, i] : rowptr[g, i + 1]], strictly ascending.  A batch of ONE graph (`from_dense` of a
(1, N, N) map, `from_edge_index(..., graph=...)` with one graph) is `batched` all the same: its dense image is (1, N, N) and
`sharding.shard_batch` slices it like the dense tensor.  Absolute offsets make `graphs(lo, hi)` a
slice of `rowptr` that shares `col`.  The adjacency is directed as given (the reference does not symmetrise, egnn_pytorch.py:249-256)
and a diagonal entry is kept: it counts in `max_degree()` (:249) and the ranking overwrites it (:252-256).

Construction and `to_dense()` are ordinary tensor code on whatever device the inputs live on (they run once per input, not in the
step), so they work on CPU tensors.
"""
from __future__ import annotations

import torch


class SparseAdjacency:
    def __init__(self, rowptr, col, n, validate=True, batched=None):
        """The raw constructor.  rowptr: int64 (N + 1,) or (G, N + 1); col: int32 (nnz,); n: the node count.  validate=True checks
        shapes, dtypes, offsets, column range and order (reads the device once).  batched: the rows are per graph (the dense image is
        (G, N, N), also for G = 1: a batch of one graph) rather than one graph's rows shared by every graph of a batch ((N, N));
        None: batched iff G > 1."""
        if not (torch.is_tensor(rowptr) and torch.is_tensor(col)):
            raise TypeError("rowptr and col must be tensors")
        if rowptr.dim() == 1:
            rowptr = rowptr[None]
        if batched is False and rowptr.shape[0] != 1:
            raise ValueError(f"a shared adjacency holds one graph's rows (rowptr has {rowptr.shape[0]})")
        self.batched = bool(rowptr.shape[0] > 1 if batched is None else batched)
        self.n = int(n)
        self.rowptr = rowptr.contiguous()
        self.col = col.contiguous()
        if validate:
            self._validate()

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_dense(cls, adj):
        """From a boolean (N, N) or (B, N, N) adjacency; `to_dense()` gives it back."""
        if adj.dtype != torch.bool:
            raise TypeError(f"adj must be torch.bool (got {adj.dtype})")
        if adj.dim() not in (2, 3) or adj.shape[-1] != adj.shape[-2]:
            raise ValueError(f"adj shape {tuple(adj.shape)}: expected (N, N) or (B, N, N)")
        n = adj.shape[-1]
        g = adj.shape[0] if adj.dim() == 3 else 1
        nz = adj.reshape(g * n, n).nonzero()                        # row-major: rows ascending, columns ascending within a row
        return cls._from_sorted(nz[:, 0], nz[:, 1], n, g, adj.dim() == 3)

    @classmethod
    def from_edge_index(cls, edge_index, n, graph=None, num_graphs=1):
        """From a (2, E) int64 list of directed edges (row, column), in any order, duplicates merged.  graph: (E,) int64 graph of each
        edge for a batched adjacency of `num_graphs` graphs; None: one graph (shared by every graph of a batch)."""
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
            raise ValueError("edge_index must be an int64 tensor of shape (2, E)")
        n, num_graphs = int(n), int(num_graphs)
        if n < 0 or num_graphs < 1:
            raise ValueError(f"bad sizes: n = {n}, num_graphs = {num_graphs}")
        row, col = edge_index[0], edge_index[1]
        if row.numel() and (int(edge_index.min()) < 0 or int(edge_index.max()) >= n):
            raise ValueError(f"edge_index holds a node outside [0, {n})")
        if graph is None:
            if num_graphs != 1:
                raise ValueError("num_graphs > 1 needs the graph of every edge (graph=)")
        else:
            if graph.dtype != torch.int64 or tuple(graph.shape) != (row.numel(),):
                raise ValueError("graph must be an int64 tensor of shape (E,)")
            if graph.numel() and (int(graph.min()) < 0 or int(graph.max()) >= num_graphs):
                raise ValueError(f"graph holds an index outside [0, {num_graphs})")
            row = graph * n + row
        key = torch.unique(row * n + col)                           # sorted, duplicates merged
        return cls._from_sorted(torch.div(key, max(n, 1), rounding_mode="floor"), key % max(n, 1), n, num_graphs, graph is not None)

    @classmethod
    def from_torch_sparse(cls, t):
        """From a 2-D square torch sparse tensor (COO or CSR layout): the pattern of its non-zero values."""
        if t.dim() != 2 or t.shape[0] != t.shape[1]:
            raise ValueError(f"expected a square 2-D sparse tensor (got {tuple(t.shape)})")
        if t.layout == torch.sparse_csr:
            t = t.to_sparse_coo()
        elif t.layout != torch.sparse_coo:
            raise TypeError(f"expected a sparse COO or CSR tensor (got layout {t.layout})")
        t = t.coalesce()
        return cls.from_edge_index(t.indices()[:, t.values() != 0].contiguous(), t.shape[0])

    @classmethod
    def _from_sorted(cls, grow, col, n, g, batched):
        """grow = g N + i ascending, col ascending within equal grow, no duplicates"""
        counts = torch.bincount(grow, minlength=g * n)[:g * n] if g * n else grow.new_zeros(0)
        cum = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
        at = torch.arange(g, device=cum.device)[:, None] * n + torch.arange(n + 1, device=cum.device)[None]
        return cls(cum[at], col.to(torch.int32), n, validate=False, batched=batched)

    # ------------------------------------------------------------------ what the dense image would say
    @property
    def num_graphs(self):
        return self.rowptr.shape[0]

    @property
    def shared(self):
        """one graph's rows for every graph of a batch (the dense image is (N, N))"""
        return not self.batched

    @property
    def shape(self):
        """the dense image's"""
        return (self.n, self.n) if self.shared else (self.num_graphs, self.n, self.n)

    def dim(self):
        return len(self.shape)

    @property
    def device(self):
        return self.rowptr.device

    @property
    def is_cuda(self):
        return self.rowptr.is_cuda

    dtype = torch.bool

    def contiguous(self):
        return self                                                  # (made contiguous at construction)

    def to(self, device):
        rowptr, col = self.rowptr.to(device), self.col.to(device)
        if rowptr is self.rowptr and col is self.col:                # (already there: Tensor.to returns the tensor itself)
            return self
        return SparseAdjacency(rowptr, col, self.n, validate=False, batched=self.batched)

    def cuda(self):
        return self.to("cuda")

    def graphs(self, lo, hi):
        """Graphs [lo, hi) of a batched adjacency (a slice of `rowptr`; `col` is shared).  A shared adjacency is every graph's: itself."""
        if self.shared:
            return self
        if not 0 <= lo <= hi <= self.num_graphs:
            raise IndexError(f"graphs [{lo}, {hi}) of {self.num_graphs}")
        return SparseAdjacency(self.rowptr[lo:hi], self.col, self.n, validate=False, batched=True)

    def row_lengths(self):
        return self.rowptr[:, 1:] - self.rowptr[:, :-1]

    def max_degree(self):
        """The longest row -- `int(adj_mat.float().sum(-1).max())` of the dense image (egnn_pytorch.py:249), the diagonal counted when
        given: one device->host read, the synchronisation the dense call and the reference have at the same place."""
        if self.n == 0 or self.num_graphs == 0:
            return 0
        return int(self.row_lengths().max().item())

    def _entries(self):
        """(global row g N + i, column) of every entry, rows ascending"""
        g, n = self.num_graphs, self.n
        counts = self.row_lengths().reshape(-1)
        rows = torch.repeat_interleave(torch.arange(g * n, device=self.device), counts)
        first = counts.cumsum(0) - counts                            # position of each row's first entry in the row-major listing
        within = torch.arange(rows.numel(), device=self.device) - first[rows]
        return rows, self.col[self.rowptr[:, :-1].reshape(-1)[rows] + within]

    def to_dense(self):
        """bool (N, N) for a shared adjacency, (B, N, N) for a batched one"""
        g, n = self.num_graphs, self.n
        out = torch.zeros(g * n, n, dtype=torch.bool, device=self.device)
        rows, cols = self._entries()
        out[rows, cols.long()] = True
        return out.view(n, n) if self.shared else out.view(g, n, n)

    def _validate(self):
        rp, col, n = self.rowptr, self.col, self.n
        if rp.dtype != torch.int64 or col.dtype != torch.int32:
            raise TypeError(f"rowptr must be int64 and col int32 (got {rp.dtype}, {col.dtype})")
        if n < 0 or rp.dim() != 2 or rp.shape[0] < 1 or rp.shape[1] != n + 1 or col.dim() != 1:
            raise ValueError(f"rowptr shape {tuple(rp.shape)} / col shape {tuple(col.shape)}: expected (G, {n + 1}) and (nnz,)")
        if rp.device != col.device:
            raise ValueError(f"rowptr is on {rp.device}, col on {col.device}")
        if int(rp.min()) < 0 or int(rp.max()) > col.numel() or bool((rp[:, 1:] < rp[:, :-1]).any()):
            raise ValueError("rowptr must hold non-decreasing offsets into col")
        if n and int(self.row_lengths().max()) > n:
            raise ValueError("a row holds more than N entries")
        rows, cols = self._entries()
        if cols.numel():
            if int(cols.min()) < 0 or int(cols.max()) >= n:
                raise ValueError(f"col holds a node outside [0, {n})")
            if bool(((rows[1:] == rows[:-1]) & (cols[1:] <= cols[:-1])).any()):
                raise ValueError("the columns of a row must be strictly ascending")

    def __repr__(self):
        return f"SparseAdjacency(n={self.n}, graphs={self.num_graphs}, nnz={int(self.row_lengths().sum())}, device={self.device})"


class SparseLabels:
    """The adjacency-degree labels of EGNN_Network (egnn_pytorch.py:414-427) as a CSR over every pair that received one: `rowptr` / `col`
    as in SparseAdjacency, `val` one byte per entry; a pair the rows do not hold has label 0.  What `_ops.adj_expand_csr` returns and
    `EdgeLookup.deg` may hold in place of the (B, N, N) byte map."""

    def __init__(self, rowptr, col, val, n):
        self.rowptr, self.col, self.val, self.n = rowptr.contiguous(), col.contiguous(), val.contiguous(), int(n)

    @property
    def num_graphs(self):
        return self.rowptr.shape[0]

    @property
    def shared(self):
        return self.rowptr.shape[0] == 1

    @property
    def device(self):
        return self.rowptr.device

    def contiguous(self):
        return self

    def graphs(self, lo, hi):
        """graphs [lo, hi) of a batched label CSR (a slice of `rowptr`); a shared one is every graph's"""
        return self if self.shared else SparseLabels(self.rowptr[lo:hi], self.col, self.val, self.n)

    def to_dense(self, b=None):
        """uint8 (B, N, N): the map `_ops.adj_expand` returns (a shared CSR repeated for `b` graphs)"""
        g, n = self.num_graphs, self.n
        rows, cols = SparseAdjacency(self.rowptr, self.col, n, validate=False)._entries()
        counts = (self.rowptr[:, 1:] - self.rowptr[:, :-1]).reshape(-1)
        within = torch.arange(rows.numel(), device=self.device) - (counts.cumsum(0) - counts)[rows]
        out = torch.zeros(g * n, n, dtype=torch.uint8, device=self.device)
        out[rows, cols.long()] = self.val[self.rowptr[:, :-1].reshape(-1)[rows] + within]
        out = out.view(g, n, n)
        return out.expand(b, n, n).contiguous() if (b is not None and g == 1 and b != 1) else out

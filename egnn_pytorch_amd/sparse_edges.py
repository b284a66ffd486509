"""`SparseEdges`: the per-pair features of a graph's bonds as the values of CSR rows instead of a (B, N, N, ...) tensor.

`EGNN.forward(edges=...)` takes one with float values (B, N, N, edge_dim would be the dense form) and
`EGNN_Network.forward(edges=...)` one with int64 token values when `num_edge_tokens` is set, else floats.  The object stands for the dense
tensor `to_dense()` -- zeros (token 0) at the pairs its rows do not hold -- and every call returns the bits of the same call with
`to_dense()`.  Nothing of size N^2 is built from it: the kernels look every selected pair up in its row
(csrc/edge_csr.hip, egnn_edge_features_gather_csr_f32 / _f64) and the gradient of float values comes back with their own shape (nnz, d).

Storage: `rowptr` int64 (B, N + 1) and `col` int32 (nnz,) exactly as in `SparseAdjacency` -- absolute offsets into one flat `col`, strictly
ascending columns within a row, directed as given, diagonal entries allowed -- and `values`, float (nnz, d) or int64 (nnz,).  The pattern is
the object's own: it need not be that of the adjacency the same call is given.  Unlike a `SparseAdjacency` it is always per graph
(the reference's `edges` has no form shared by a batch): `num_graphs` must be the batch size of the call.

Construction and `to_dense()` are ordinary tensor code on whatever device the inputs live on, so they work on CPU tensors.
"""
from __future__ import annotations

import torch

from .sparse_adj import SparseAdjacency

_NNZ_MAX = 2 ** 31 - 1                                              # (the kernels hold a position in an int32)


class SparseEdges:
    def __init__(self, rowptr, col, values, n, validate=True):
        """The raw constructor.  rowptr: int64 (N + 1,) or (B, N + 1); col: int32 (nnz,); values: float (nnz, d) or int64 (nnz,); n: the
        node count.  validate=True checks shapes, dtypes, offsets, column range and order (reads the device once)."""
        if not (torch.is_tensor(rowptr) and torch.is_tensor(col) and torch.is_tensor(values)):
            raise TypeError("rowptr, col and values must be tensors")
        if rowptr.dim() == 1:
            rowptr = rowptr[None]
        self.n = int(n)
        self.rowptr = rowptr.contiguous()
        self.col = col.contiguous()
        self.values = values if values.is_contiguous() else values.contiguous()     # (the caller's own tensor: it may require grad)
        if validate:
            self._validate()

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_dense(cls, edges, pattern=None):
        """From dense float edges (B, N, N, d) or an int64 token map (B, N, N).  pattern: bool (B, N, N), the pairs to keep (an entry whose
        value is 0 included); None: the pairs with a non-zero channel / a token != 0.  Differentiable in float `edges`."""
        tokens = not edges.is_floating_point()
        if tokens and edges.dtype != torch.int64:
            raise TypeError(f"edges must be floating point (B, N, N, d) or int64 tokens (B, N, N) (got {edges.dtype})")
        if edges.dim() != (3 if tokens else 4) or edges.shape[1] != edges.shape[2]:
            raise ValueError(f"edges shape {tuple(edges.shape)}: expected (B, N, N, d) floats or (B, N, N) tokens")
        b, n = edges.shape[:2]
        if pattern is None:
            pattern = (edges != 0) if tokens else (edges != 0).any(dim=-1)
        elif pattern.dtype != torch.bool or tuple(pattern.shape) != (b, n, n):
            raise ValueError(f"pattern must be a bool tensor of shape {(b, n, n)}")
        adj = SparseAdjacency.from_dense(pattern)
        flat = pattern.reshape(-1).nonzero().reshape(-1)            # row-major: the order of the CSR entries
        values = edges.reshape(-1)[flat] if tokens else edges.reshape(b * n * n, edges.shape[-1])[flat]
        return cls(adj.rowptr, adj.col, values, n, validate=False)._checked_size()

    @classmethod
    def from_edge_index(cls, edge_index, values, n, graph=None, num_graphs=1):
        """From a (2, E) int64 list of directed edges (row, column) in any order with their values, float (E, d) or int64 (E,).  graph:
        (E,) int64 graph of each edge, for `num_graphs` graphs; None: one graph (a B = 1 call).  A pair given twice raises ValueError."""
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
            raise ValueError("edge_index must be an int64 tensor of shape (2, E)")
        n, num_graphs = int(n), int(num_graphs)
        if n < 0 or num_graphs < 1:
            raise ValueError(f"bad sizes: n = {n}, num_graphs = {num_graphs}")
        row, col = edge_index[0], edge_index[1]
        if values.shape[:1] != row.shape:
            raise ValueError(f"values holds {values.shape[0] if values.dim() else 0} entries, edge_index {row.numel()}")
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
        key, order = torch.sort(row * n + col)
        if bool((key[1:] == key[:-1]).any()):
            raise ValueError("edge_index holds a pair twice")
        adj = SparseAdjacency._from_sorted(torch.div(key, max(n, 1), rounding_mode="floor"), key % max(n, 1), n, num_graphs, True)
        return cls(adj.rowptr, adj.col, values[order], n, validate=False)._checked_values()

    @classmethod
    def from_adjacency(cls, adj, values):
        """The pattern of a SparseAdjacency (batched, or one graph for B = 1 calls) with one value per entry, in the order of `adj.col`."""
        if not isinstance(adj, SparseAdjacency):
            raise TypeError("adj must be a SparseAdjacency")
        return cls(adj.rowptr, adj.col, values, adj.n, validate=False)._checked_values()

    def _checked_size(self):
        if self.col.numel() > _NNZ_MAX:
            raise ValueError(f"a SparseEdges holds at most 2^31 - 1 entries (got {self.col.numel()})")
        return self

    def _checked_values(self):
        """the checks of `_validate` that concern `values` (the constructors build rowptr / col themselves)"""
        v = self.values
        if not (v.is_floating_point() or v.dtype == torch.int64):
            raise TypeError(f"values must be floating point (nnz, d) or int64 tokens (nnz,) (got {v.dtype})")
        if v.dim() != (2 if v.is_floating_point() else 1) or v.shape[0] != self.col.numel():
            raise ValueError(f"values shape {tuple(v.shape)}: expected ({self.col.numel()}, d) floats or ({self.col.numel()},) tokens")
        if v.device != self.col.device:
            raise ValueError(f"values is on {v.device}, col on {self.col.device}")
        return self._checked_size()

    # ------------------------------------------------------------------ what the dense image would say
    @property
    def num_graphs(self):
        return self.rowptr.shape[0]

    @property
    def is_tokens(self):
        return not self.values.is_floating_point()

    @property
    def width(self):
        """the channels of float values (None for tokens)"""
        return None if self.is_tokens else self.values.shape[1]

    @property
    def shape(self):
        """the dense image's"""
        b, n = self.num_graphs, self.n
        return (b, n, n) if self.is_tokens else (b, n, n, self.values.shape[1])

    def dim(self):
        return len(self.shape)

    @property
    def dtype(self):
        return self.values.dtype

    @property
    def device(self):
        return self.rowptr.device

    @property
    def is_cuda(self):
        return self.rowptr.is_cuda

    @property
    def requires_grad(self):
        return self.values.requires_grad

    def is_floating_point(self):
        return self.values.is_floating_point()

    def contiguous(self):
        return self                                                  # (made contiguous at construction)

    def to(self, device):
        rowptr, col, values = self.rowptr.to(device), self.col.to(device), self.values.to(device)
        if rowptr is self.rowptr and col is self.col and values is self.values:
            return self
        return SparseEdges(rowptr, col, values, self.n, validate=False)

    def cuda(self):
        return self.to("cuda")

    def graphs(self, lo, hi):
        """Graphs [lo, hi) (a slice of `rowptr`; `col` and `values` are shared, the offsets stay absolute)."""
        if not 0 <= lo <= hi <= self.num_graphs:
            raise IndexError(f"graphs [{lo}, {hi}) of {self.num_graphs}")
        return SparseEdges(self.rowptr[lo:hi], self.col, self.values, self.n, validate=False)

    def adjacency(self):
        """the pattern as a (batched) SparseAdjacency sharing `rowptr` and `col`"""
        return SparseAdjacency(self.rowptr, self.col, self.n, validate=False, batched=True)

    def to_dense(self):
        """(B, N, N, d) with zeros at the pairs the rows do not hold, or (B, N, N) int64 with token 0 there.  Differentiable in float
        `values`."""
        b, n = self.num_graphs, self.n
        adj = self.adjacency()
        rows, cols = adj._entries()
        counts = adj.row_lengths().reshape(-1)
        within = torch.arange(rows.numel(), device=self.device) - (counts.cumsum(0) - counts)[rows]
        at = self.rowptr[:, :-1].reshape(-1)[rows] + within          # each listed entry's offset into col / values
        flat = rows * n + cols.long()
        if self.is_tokens:
            out = torch.zeros(b * n * n, dtype=torch.int64, device=self.device)
            out[flat] = self.values[at]
            return out.view(b, n, n)
        d = self.values.shape[1]
        out = torch.zeros(b * n * n, d, dtype=self.values.dtype, device=self.device)
        return out.index_put((flat,), self.values[at]).view(b, n, n, d)

    def _validate(self):
        self.adjacency()._validate()
        self._checked_values()

    def __repr__(self):
        kind = "tokens" if self.is_tokens else f"d={self.values.shape[1]}"
        return f"SparseEdges(n={self.n}, graphs={self.num_graphs}, nnz={self.col.numel()}, {kind}, device={self.device})"

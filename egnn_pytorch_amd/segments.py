"""`GraphSegments`: the boundaries of a PACKED batch -- the nodes of G graphs of any sizes concatenated as (T, ...) rows, graph g owning
the rows offsets[g] : offsets[g + 1] -- the layout molecular and protein data loaders produce (PyG's `batch` vector, a list of sizes).

`EGNN.forward(feats, coors, mask=segments)` and `EGNN_Network.forward(...)` take one where they take the node mask of a padded batch,
with feats (T, dim) and coors (T, C), and return (T, dim) and (T, C): what the padded call with a prefix mask returns on the real nodes,
without allocating, reading or writing a padded row.  To the kernels a packed batch is ONE graph of T nodes whose neighbour lists never
cross a segment boundary; the segmented selection (csrc/knn_segments.hip, `_ops.knn_select_segments`) is what keeps them inside.

It is built once by the caller, like `SparseAdjacency`, and keeps the offsets on the device (for the kernel) and on the host (sizes,
the largest graph, the chunking of `split`): no forward synchronises to read them.  Construction, `pack` and `unpack` are ordinary
tensor code on whatever device the inputs live on, so they work on CPU tensors.
"""
from __future__ import annotations

import torch


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

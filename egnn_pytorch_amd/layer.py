"""Drop-in `EGNN` / `EGNN_Network` modules whose forward runs on the gfx950 HIP kernels.

Boundary mirrored: constructor keywords, `forward` signatures (note the different
positional order of the two entry points), parameter names / shapes of the reference's
`state_dict`, error behaviour (asserts at construction, `topk` out-of-range when K > N).
Reference: egnn_pytorch/egnn_pytorch.py:148-341 (EGNN), :343-454 (EGNN_Network).

The forward pass runs ONLY on a CUDA(HIP) device, in fp32 (or, for a module converted with .double(), in float64 on the float64
kernels).  There is no CPU or PyTorch-eager fallback for it: anything the kernels do not cover raises.  Under autograd (grad mode on
and an input or a parameter requires grad) the same HIP forward is wrapped in an autograd.Function whose backward runs on the HIP
kernels (the E x H work of every shape the fused forward covers) or recomputes the layer a few graphs at a time
(egnn_pytorch_amd/autograd.py).
"""
from __future__ import annotations

import contextlib
import copy
import contextvars
import os
import warnings

import torch
from torch import nn

from . import _abi, _dropout, _ops, _weights, autograd as _autograd
from .attention import GlobalLinearAttention
from .segments import GraphSegments
from .sparse_adj import SparseAdjacency, SparseLabels
from .sparse_edges import SparseEdges

_SPATIAL_ORDER = os.environ.get("EGNN_SPATIAL_ORDER", "1") != "0"     # scheduling knob only; results do not depend on it
_SLOT_PREP = os.environ.get("EGNN_SLOT_PREP", "1") != "0"             # per-slot records for the edge pass's setup (same results)
# egnn_edge_args.algo: 0 = the library chooses (persistent wave-per-node kernel where it applies), 1 = the general edge kernel always
# (A/B measurements; tests/test_gpu_kernels.py checks the two against each other)
_EDGE_ALGO = int(os.environ.get("EGNN_EDGE_ALGO", "0"))
# Arithmetic.  "fast" (default): split-fp16 products on the matrix cores (fp32-class accuracy, values up to fp16's 65504 at the cast
# sites); a call that leaves that range is re-run automatically in plain fp32 -- the reference's arithmetic class, several times
# slower -- when the range status word is read synchronously (EGNN_RANGE_CHECK=sync, the default) and no graph is being recorded;
# otherwise it raises EGNNRangeError.  "exact": always the plain-fp32 kernels (inference only).
_PRECISION = os.environ.get("EGNN_PRECISION", "fast")
_DENSE_PW = os.environ.get("EGNN_DENSE_PW", "1") != "0"            # dense layers with N % 32 == 0 on the wave-per-node edge kernel
# Inference forwards as ONE call of the C whole-layer entry (egnn_layer_forward_opts_f32: the same kernels in the same order, enqueued from
# C) instead of a dozen Python-side launches: ~200 us of host time per forward become a few tens.  Only with every scheduling switch
# above at its default -- the C entry implements the default policy -- and never while per-kernel timing is on.
_C_FORWARD = os.environ.get("EGNN_C_FORWARD", "1") != "0"
# k-NN graphs of at least this many nodes select their neighbours on the cell grid (csrc/knn_grid.hip: fp32 or, in a float64 module,
# float64; 3-D, no adjacency or a SparseAdjacency, K <= 128; the same neighbour list bit for bit) instead of the all-pairs kernels.  The
# default moves no graph up to 65 536 nodes.  One threshold for both kinds of call and both dtypes: with CSR rows the grid beat the CSR
# streaming kernel in every case measured at 65 536 nodes, the smallest size measured (DESIGN.md section 4.1 has the measurements).
_KNN_GRID_MIN_N = int(os.environ.get("EGNN_KNN_GRID_MIN_N", "65537"))


# A packed batch (`mask=GraphSegments`) is one graph of T nodes to the kernels, so the single-graph limits would apply to T: the fused
# kernels' 32-bit offsets (`EGNN._fused_covers`) and, under autograd, the fused backward's (autograd.FusedBackwardLimit).  Graphs are
# independent: a packed call beyond the limit is cut at graph boundaries into several calls.  None: the limit of each call from those
# rules (`EGNN._packed_node_limit`); an int: that many nodes (tests lower it).
_PACKED_MAX_NODES = None
# the GraphSegments of the packed call in flight (per thread / context, like `_exact_now`): the neighbour selection of the layer's
# launch sequence takes the segmented kernel while it is set
_segments_now = contextvars.ContextVar("egnn_segments_now", default=None)


def _packed_pieces(segments, limit, k):
    """[(row slice, GraphSegments)] of a packed batch beyond `limit` nodes: `segments.split` pieces, cut at graph boundaries.  A piece
    of fewer than K rows (the selection needs K <= T, as every call does) joins a neighbour: the split leaves K - 1 rows of room for
    that, so a piece passes the limit only where such a piece has no neighbour but graphs that leave no such room on their own."""
    room = limit - (k - 1) if limit >= 2 * k else limit
    pieces = list(segments.split(max(room, 1)))
    i = 0
    while len(pieces) > 1 and i < len(pieces):
        if pieces[i][1].num_nodes >= k:
            i += 1
            continue
        fits = [j for j in (i - 1, i + 1) if 0 <= j < len(pieces) and pieces[j][1].num_nodes + pieces[i][1].num_nodes <= limit]
        j = fits[0] if fits else (i - 1 if i > 0 else i + 1)
        lo, hi = min(i, j), max(i, j)
        merged = GraphSegments.from_sizes(pieces[lo][1].sizes + pieces[hi][1].sizes, device=segments.device)
        pieces[lo:hi + 1] = [(slice(pieces[lo][0].start, pieces[hi][0].stop), merged)]
        i = lo
    return pieces


def _default_policy():
    """every scheduling switch at its default (read at call time: tests flip them on the module)"""
    return _SPATIAL_ORDER and _SLOT_PREP and _EDGE_ALGO == 0
_exact_now = contextvars.ContextVar("egnn_exact_now", default=False)       # per thread / context: concurrent forwards do not see each other's
_warned_rerun = False


@contextlib.contextmanager
def exact_arithmetic():
    """Run the enclosed forwards on the plain-fp32 (wide-range) kernels: include/egnn_hip.h, "The wide-range path"."""
    tok = _exact_now.set(True)
    try:
        yield
    finally:
        _exact_now.reset(tok)


def exact_active():
    return _exact_now.get() or _PRECISION == "exact"


def _warn_rerun(err):
    """Once per process: the automatic plain-fp32 re-run is several times slower than the fast path and costs a host synchronisation."""
    global _warned_rerun
    if not _warned_rerun:
        _warned_rerun = True
        warnings.warn("egnn_pytorch_amd: a forward left the range of the split-fp16 fast path and is being re-run on the plain-fp32 "
                      f"kernels (several times slower; this warning is issued once). Cause: {err}", RuntimeWarning, stacklevel=3)


def _rerun_exact_ok(module, *tensors):
    """A forward that tripped the range status word may be re-run in plain fp32: the word was read for THIS call (sync mode) and no
    stream capture is going on.  Under autograd too (round 5): the re-run's forward is the plain-fp32 kernels and its backward the
    recompute path -- plain fp32 ATen arithmetic over the neighbour list those kernels selected, no fp16 cast site anywhere -- so that
    reference-legal inputs such as feats x 1e6 TRAIN instead of raising (slower: it is the wide-range path).  With training-mode
    dropout as well: the plain kernels evaluate the same hash masks (the re-run draws a fresh seed, like any other forward)."""
    if _ops.RANGE_CHECK != "sync" or exact_active():
        return False
    return not torch.cuda.is_current_stream_capturing()
# The kernels compute in fp32-class arithmetic (split-f16 products, fp32 accumulation: DESIGN.md §2).  Other floating dtypes
# -- the reference is dtype-generic and its own tests run in float64 -- are accepted at the boundary: inputs are converted to
# fp32, outputs back to the callers' dtype.  For bf16 / fp16 that is at least the reference's precision; for float64 it is
# NOT (products carry ~22 significant bits): the reference's 1e-6 fp64 equivariance bars hold only for small weights.
_FLOAT_DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16)


class EdgeLookup:
    """Per-pair edge features given as look-up tables instead of a materialised (B,N,N,edge_dim) tensor: what EGNN_Network's
    front-end produces (egnn_pytorch.py:410-432) -- [edge_emb(edge tokens) or float edges | adj_emb(adjacency-degree labels)].
    The edge kernel reads the tables for the K selected pairs of each node (egnn_edge_features_gather_f32).  `edges`, `tok_emb` and
    `deg_emb` (`live`) are the caller's tensors -- the dense float edges and the embedding weights -- and the kernels read detached
    copies of them in `dtype`, the compute dtype of the layers that consume them: float32, or float64 for float64 modules
    (egnn_edge_features_gather_f64).  Under autograd the layer hands the live ones to autograd.EGNNFunction as differentiable inputs:
    their gradients come from egnn_edge_features_grad_f32 / _f64, a reduction over the selected pairs only.
    `csr`: the first table as a SparseEdges -- its float values (nnz, d) take the place of `edges` (live[0], differentiable, with the
    detached copy in `dtype`) or its tokens (nnz,) that of `tok`, both read through the positions the kernel finds in `csr`'s rows
    (egnn_edge_features_gather_csr_f32 / _f64); nothing of size N^2 then stands behind the first table."""

    def __init__(self, edges=None, tok=None, tok_emb=None, deg=None, deg_emb=None, dtype=torch.float32, csr=None):
        self.csr = csr
        if csr is not None:
            edges, tok = (None, csr.values) if csr.is_tokens else (csr.values, None)
        self.live = (edges, tok_emb if tok is not None else None, deg_emb if deg is not None else None)
        self.tok = None if tok is None else tok.contiguous().long()
        self.deg = None if deg is None else deg.contiguous()
        self._copy_tables(dtype)
        self.d1 = self.tok_emb.shape[1] if self.tok is not None else (self.edges.shape[-1] if self.edges is not None else 0)
        self.d2 = self.deg_emb.shape[1] if self.deg is not None else 0

    def _copy_tables(self, dtype):
        """the kernel-side copies of `live` in `dtype` (converted from the caller's tensors themselves, never from another copy)"""
        edges, tok_emb, deg_emb = self.live
        self.dtype = dtype
        self.edges = None if edges is None else _ops.aligned(edges.detach().to(dtype))
        self.tok_emb = None if tok_emb is None else tok_emb.detach().contiguous().to(dtype)
        self.deg_emb = None if deg_emb is None else deg_emb.detach().contiguous().to(dtype)
        self._casts = {}                                        # (dtype -> a copy in that dtype; never holds the object itself)

    @property
    def width(self):
        return self.d1 + self.d2

    def to(self, dtype):
        """The same look-up with its table copies in `dtype`: itself when they are already, else a copy made once from `live` and kept
        (the layers of a network share one EdgeLookup: one conversion per forward, not one per layer).  The copy does not point back, so
        an EdgeLookup is freed by its reference count like any tensor holder: it pins N^2-sized label maps."""
        if dtype == self.dtype:
            return self
        out = self._casts.get(dtype)
        if out is None:
            out = copy.copy(self)
            out._copy_tables(dtype)
            self._casts[dtype] = out
        return out

    def graphs(self, lo, hi):
        """The same tables for graphs [lo, hi) of the batch (the labels and dense edges sliced, the embedding tables shared)."""
        out = copy.copy(self)
        out._casts = {}
        if self.csr is not None:                                # (a slice of rowptr: values / tokens are shared, offsets absolute)
            out.csr = self.csr.graphs(lo, hi)
        else:
            out.live = (None if self.live[0] is None else self.live[0][lo:hi],) + tuple(self.live[1:])
            out.edges = None if self.edges is None else self.edges[lo:hi]
            out.tok = None if self.tok is None else self.tok[lo:hi]
        out.deg = None if self.deg is None else (self.deg.graphs(lo, hi) if isinstance(self.deg, SparseLabels) else self.deg[lo:hi])
        return out


def _mlp(d_in, d_hidden, d_out, dropout, final_act):
    """Linear -> dropout|Identity -> SiLU -> Linear [-> SiLU]; indices 0 and 3 hold the Linears, which is
    what gives the reference's state_dict keys (`edge_mlp.0.*`, `edge_mlp.3.*`, ...)."""
    mods = [nn.Linear(d_in, d_hidden), dropout, nn.SiLU(), nn.Linear(d_hidden, d_out)]
    if final_act:
        mods.append(nn.SiLU())
    return nn.Sequential(*mods)


class CoorsNorm(nn.Module):
    """Holder of the learned `scale` of the reference's CoorsNorm (egnn_pytorch.py:67-77); the
    normalisation itself (x / max(|x|, eps) * scale) happens inside the fused edge kernel."""

    def __init__(self, eps=1e-8, scale_init=1.0):
        super().__init__()
        self.eps = eps
        self.scale = nn.Parameter(torch.full((1,), float(scale_init)))


class EGNN(nn.Module):
    def __init__(self, dim, edge_dim=0, m_dim=16, fourier_features=0, num_nearest_neighbors=0,
                 dropout=0.0, init_eps=1e-3, norm_feats=False, norm_coors=False,
                 norm_coors_scale_init=1e-2, update_feats=True, update_coors=True,
                 only_sparse_neighbors=False, valid_radius=float("inf"), m_pool_method="sum",
                 soft_edges=False, coor_weights_clamp_value=None):
        super().__init__()
        assert m_pool_method in {"sum", "mean"}, "pool method must be either sum or mean"
        assert update_feats or update_coors, "you must update either features, coordinates, or both"

        self.dim = dim
        self.edge_dim = edge_dim
        self.m_dim = m_dim
        self.fourier_features = fourier_features
        self.num_nearest_neighbors = num_nearest_neighbors
        self.only_sparse_neighbors = only_sparse_neighbors
        self.valid_radius = valid_radius
        self.m_pool_method = m_pool_method
        self.coor_weights_clamp_value = coor_weights_clamp_value
        self.norm_feats = norm_feats
        self.norm_coors = norm_coors
        self.dropout_p = dropout
        self.init_eps = init_eps

        edge_input_dim = 2 * fourier_features + 2 * dim + edge_dim + 1
        drop = nn.Dropout(dropout) if dropout > 0 else nn.Identity()     # one shared instance, as upstream

        self.edge_mlp = _mlp(edge_input_dim, 2 * edge_input_dim, m_dim, drop, final_act=True)
        self.edge_gate = nn.Sequential(nn.Linear(m_dim, 1), nn.Sigmoid()) if soft_edges else None
        self.node_norm = nn.LayerNorm(dim) if norm_feats else nn.Identity()
        self.coors_norm = CoorsNorm(scale_init=norm_coors_scale_init) if norm_coors else nn.Identity()
        self.node_mlp = _mlp(dim + m_dim, 2 * dim, dim, drop, final_act=False) if update_feats else None
        self.coors_mlp = _mlp(m_dim, 4 * m_dim, 1, drop, final_act=False) if update_coors else None

        for mod in self.modules():                                       # upstream init_: N(0, init_eps)
            if type(mod) is nn.Linear:
                nn.init.normal_(mod.weight, std=init_eps)

        self._packed = None
        self._packed_key = None

    def __getstate__(self):
        """copy.deepcopy / pickle / torch.save(module): without the kernel-side caches (re-laid-out weights on the device, the C entry's
        blob, the cached parameter list) -- they are rebuilt at the copy's first forward."""
        st = self.__dict__.copy()
        st["_packed"] = st["_packed_key"] = None
        for k in ("_c_packed", "_param_cache", "_param_cache_mods", "_param_cache_tree", "_param_cache_counts"):
            st.pop(k, None)
        return st

    # ------------------------------------------------------------------ kernel-side weights
    def packed_weights(self):
        key = _weights.version_key(self)
        if self._packed is None or key != self._packed_key:
            self._packed = _weights.pack(self)
            self._packed_key = key
        return self._packed

    # ------------------------------------------------------------------ forward
    def _check_inputs(self, feats, coors, edges, mask, adj_mat):
        if not feats.is_cuda:
            raise RuntimeError("egnn_pytorch_amd.EGNN runs only on an MI355X (cuda/HIP) device; "
                               "there is no CPU fallback (move the module and inputs with .cuda())")
        if feats.dtype not in _FLOAT_DTYPES or coors.dtype not in _FLOAT_DTYPES:
            raise NotImplementedError(f"the gfx950 path takes floating-point feats / coors (got {feats.dtype}/{coors.dtype})")
        if feats.dim() != 3 or coors.dim() != 3 or feats.shape[:2] != coors.shape[:2]:
            raise ValueError(f"feats {tuple(feats.shape)} / coors {tuple(coors.shape)}: expected (B,N,dim) and (B,N,C)")
        if not 1 <= coors.shape[-1] <= 64:
            raise NotImplementedError("the gfx950 path supports coordinate dimensions 1..64 (beyond 8 on the plain kernels)")
        if feats.shape[-1] != self.dim:
            raise ValueError(f"feats last dim {feats.shape[-1]} != dim {self.dim}")
        if (edges is not None) != (self.edge_dim > 0):
            raise ValueError("`edges` must be passed if and only if edge_dim > 0")
        b, n = feats.shape[:2]
        if isinstance(edges, EdgeLookup):                           # (a SparseEdges arrives as one: `forward` wraps it)
            if edges.width != self.edge_dim:
                raise ValueError(f"edge look-up tables give {edges.width} features per pair, edge_dim is {self.edge_dim}")
            if edges.csr is not None:
                if tuple(edges.csr.shape[:3]) != (b, n, n):
                    raise ValueError(f"SparseEdges shape {tuple(edges.csr.shape)} != {(b, n, n)} + features: it is per graph, its graph "
                                     "count must equal the batch size")
                if edges.csr.device != feats.device:
                    raise RuntimeError(f"Expected all tensors to be on the same device: feats is on {feats.device}, edges on "
                                       f"{edges.csr.device}")
        elif edges is not None and tuple(edges.shape) != (b, n, n, self.edge_dim):
            raise ValueError(f"edges shape {tuple(edges.shape)} != {(b, n, n, self.edge_dim)}")
        if mask is not None and tuple(mask.shape) != (b, n):
            raise ValueError(f"mask shape {tuple(mask.shape)} != {(b, n)}")
        if adj_mat is not None and self._use_nearest():               # (a dense layer does not read the adjacency)
            want = (b, n, n) if adj_mat.dim() == 3 else (n, n)      # (a SparseAdjacency answers with its dense image's shape)
            if tuple(adj_mat.shape) != want:
                raise ValueError(f"adj_mat shape {tuple(adj_mat.shape)} != {want}")
        # the kernels take raw device pointers: a tensor on another device (or on the host) would be read as garbage, not rejected
        for name, t in (("coors", coors), ("mask", mask), ("adj_mat", adj_mat), ("edges", None if isinstance(edges, EdgeLookup) else edges)):
            if t is not None and t.device != feats.device:
                raise RuntimeError(f"Expected all tensors to be on the same device: feats is on {feats.device}, {name} on {t.device}")

    def _sparse_edges_lookup(self, edges):
        """A SparseEdges of float values as the look-up table the kernels read (EdgeLookup with a CSR first table): the layer then takes
        `_forward_hip` / `_forward_exact`, as for every EdgeLookup."""
        if edges.is_tokens:
            raise TypeError("EGNN takes a SparseEdges of float values (nnz, edge_dim); bond tokens are EGNN_Network(num_edge_tokens=...)'s")
        if edges.values.dtype not in _FLOAT_DTYPES:
            raise NotImplementedError(f"the gfx950 path takes floating-point edges (got {edges.values.dtype})")
        return EdgeLookup(csr=edges, dtype=self.compute_dtype())

    def forward(self, feats, coors, edges=None, mask=None, adj_mat=None):
        out = None
        if isinstance(edges, SparseEdges):
            edges = self._sparse_edges_lookup(edges)
        try:
            with _ops.early_publish():                              # (the one-call C forward may publish the status words itself)
                out = self._call(feats, coors, edges, mask, adj_mat, None)[:2]
                _ops.range_check_after_forward(feats.device)        # EGNN_RANGE_CHECK: sync (default) | deferred | off
        except _abi.EGNNRangeError as err:
            if err.origin == "backward" or not _rerun_exact_ok(self, feats, coors, edges):
                raise
            _warn_rerun(err)
            out = None                                              # (under autograd the first attempt holds u and the projection table)
            with exact_arithmetic():                                # reference-legal inputs beyond the fp16 cast sites: plain fp32
                out = self._call(feats, coors, edges, mask, adj_mat, None)[:2]
        return out

    def _call(self, feats, coors, edges, mask, adj_mat, order_hint):
        """(node_out, coors_out, order): inference under no_grad, or -- when a graph has to be recorded -- through
        autograd.EGNNFunction (HIP forward, recompute-in-backward)."""
        if isinstance(mask, GraphSegments):                         # a packed batch: feats (T, dim), coors (T, C)
            return self._call_packed(feats, coors, edges, mask, adj_mat, order_hint)
        if _ops.RANGE_CHECK == "deferred" and feats.is_cuda:
            _ops.check_range(feats.device, wait=False)              # an earlier call's status, if it has arrived
        if isinstance(edges, EdgeLookup):
            edges = edges.to(self.compute_dtype())                  # (the table copies in the dtype this layer's kernels read)
        lookup = edges if isinstance(edges, EdgeLookup) else None
        # (edge look-up tables: the dense float edges and the two embedding weights they were built from are differentiable inputs)
        dense, tok_w, deg_w = lookup.live if lookup is not None else (edges, None, None)
        if _autograd.wants_grad(self, feats, coors, dense, tok_w, deg_w):
            node_out, coors_out = _autograd.EGNNFunction.apply(self, order_hint, mask, adj_mat, feats, coors, dense, lookup, tok_w, deg_w,
                                                               *self.parameters())
            order = None                                            # (scheduling hint only; recomputed by the next layer)
        else:
            with torch.no_grad():
                node_out, coors_out, order = self._forward_with_hint(feats, coors, edges, mask, adj_mat, order_hint)[:3]
        return node_out, coors_out, order

    # ------------------------------------------------------------------ packed batches
    def _check_packed(self, feats, coors, edges, segments, adj_mat):
        """the refusals and shape checks of a packed call, before any launch"""
        if adj_mat is not None:
            raise NotImplementedError("a packed batch (mask=GraphSegments) with adj_mat is not supported: the adjacency ranking of the "
                                      "segmented selection is a follow-up (DESIGN.md section 9); pad the batch, or drop adj_mat")
        if edges is not None:
            raise NotImplementedError("a packed batch (mask=GraphSegments) with edges is not supported: per-pair edge features of a "
                                      "packed batch are a follow-up (DESIGN.md section 9); pad the batch, or drop edges")
        if self.num_nearest_neighbors <= 0:
            raise NotImplementedError("a packed batch (mask=GraphSegments) on a dense layer (num_nearest_neighbors = 0) is not supported: "
                                      "all pairs of a ragged batch have no fixed K (DESIGN.md section 9); set num_nearest_neighbors")
        if feats.dim() != 2 or coors.dim() != 2 or feats.shape[0] != coors.shape[0]:
            raise ValueError(f"feats {tuple(feats.shape)} / coors {tuple(coors.shape)}: a packed batch takes (T,dim) and (T,C)")
        if feats.shape[0] != segments.num_nodes:
            raise ValueError(f"feats holds {feats.shape[0]} rows, the segments {segments.num_nodes} nodes")
        if segments.device != feats.device:
            raise RuntimeError(f"Expected all tensors to be on the same device: feats is on {feats.device}, the segments on "
                               f"{segments.device}")

    def _packed_node_limit(self, k, training):
        """the most nodes one call of a packed batch may hold (`_PACKED_MAX_NODES`): what `_fused_covers` admits for one graph whatever K
        is and, under autograd, what the fused backward does; the plain kernels (float64 modules, the wide-range path) address with 64 bits"""
        if _PACKED_MAX_NODES is not None:
            return int(_PACKED_MAX_NODES)
        if self.float64_kernels() or exact_active():
            return 2 ** 31 - 1
        h = 2 * (2 * self.fourier_features + 2 * self.dim + self.edge_dim + 1)
        limit = 0x80000000 // ((h + 32) * 8)
        if training:
            limit = min(limit, _autograd._fused_largest_graph(k, _abi.load().egnn_padded_hidden(h)))
        return limit

    def _call_packed(self, feats, coors, edges, segments, adj_mat, order_hint):
        """`_call` for feats (T, dim), coors (T, C) and a GraphSegments: one call with B = 1, N = T whose neighbour lists stay inside
        the segments -- or, beyond `_packed_node_limit`, one call per `_packed_pieces` piece, concatenated (under autograd each piece
        records its own EGNNFunction)."""
        self._check_packed(feats, coors, edges, segments, adj_mat)
        t, k = segments.num_nodes, self.num_nearest_neighbors
        if k > t:
            raise RuntimeError("selected index k out of range")      # torch.topk's error upstream: K against T (a graph below K is legal)
        limit = self._packed_node_limit(k, _autograd.wants_grad(self, feats, coors))
        if segments.num_graphs > 1 and t > limit:
            outs = [self._call_packed_one(feats[sl], coors[sl], piece, None) for sl, piece in _packed_pieces(segments, limit, k)]
            return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]), None
        return self._call_packed_one(feats, coors, segments, order_hint)

    def _call_packed_one(self, feats, coors, segments, order_hint):
        # The edge kernels and the backward consult a slot's validity only when a node mask is present, and the empty slots of a graph
        # below K are told by it (rank = +inf > the radius): the call carries an all-true mask.
        mask = torch.ones(1, feats.shape[0], dtype=torch.bool, device=feats.device)
        if sum(1 for n in segments.sizes if n) == 1:
            # one graph: the ordinary one-graph call, on today's selection (the cell grid beyond 65 536 nodes included)
            node_out, coors_out, order = self._call(feats[None], coors[None], None, mask, None, order_hint)
        else:
            tok = _segments_now.set(segments)
            try:
                node_out, coors_out, order = self._call(feats[None], coors[None], None, mask, None, order_hint)
            finally:
                _segments_now.reset(tok)
        return node_out[0], coors_out[0], order

    def _forward_hip_checked(self, feats, coors, edges, mask, adj_mat, order_hint, want_u=False, drop_seed=None):
        """(node_out, coors_out, order, idx, rank, valid_radius, u, proj) -- what autograd.EGNNFunction.forward needs; u = the
        (B*N*K, 16) pre-activation of edge_mlp's second SiLU when `want_u` (the native backward differentiates from it), proj =
        ((B*N, 2 Hp) projection table P_i | P_j, pi_split) the edge pass read (kept for the backward instead of a second GEMM)."""
        return self._forward_with_hint(feats, coors, edges, mask, adj_mat, order_hint, want_u=want_u, drop_seed=drop_seed, selection=True)

    def dropout_active(self):
        """training mode with dropout > 0: every forward draws a fresh mask seed (egnn_pytorch_amd/_dropout.py)"""
        return self.training and self.dropout_p > 0

    def _forward_with_hint(self, feats, coors, edges, mask, adj_mat, order_hint, want_u=False, drop_seed=None, selection=False):
        """forward + the scheduling permutation it used (EGNN_Network hands layer 0's on to the next layers).  selection: the caller
        reads the neighbour list (idx, rank) from the returned tuple -- the one-call C forward keeps it in its workspace."""
        self._check_inputs(feats, coors, edges, mask, adj_mat)
        _abi.load()
        f_dtype, c_dtype = feats.dtype, coors.dtype
        f64 = self.float64_kernels()
        if not f64 and torch.float64 in (f_dtype, c_dtype):
            _warn_float64_once()
        b, n = feats.shape[:2]
        if b == 0 or (n == 0 and not self._use_nearest()):
            # empty batch / empty dense graphs: the reference returns empty outputs (N = 0 on the k-NN path: topk's error)
            return torch.empty_like(feats), torch.empty_like(coors), None, None, None, self.valid_radius, None, None
        if f64:
            # a float64 module computes in float64, as the reference does (its own tests run in float64, tests/test_equivariance.py:6):
            # the plain kernels instantiated for double (include/egnn_hip.h, "The float64 path")
            with torch.cuda.device(feats.device):
                if self.dropout_active() and drop_seed is None:
                    drop_seed = _dropout.draw_seed()
                out = self._forward_exact(feats.double(), coors.double(),
                                          edges if (edges is None or isinstance(edges, EdgeLookup)) else edges.double(), mask, adj_mat,
                                          self._neighbour_count(n, adj_mat, torch.float64),
                                          dtype=torch.float64, want_u=want_u,
                                          drop=(self.dropout_p, drop_seed) if self.dropout_active() else None)
            if f_dtype != torch.float64 or c_dtype != torch.float64:
                out = (out[0].to(f_dtype), out[1].to(c_dtype)) + tuple(out[2:])
            return out
        if (_C_FORWARD and _default_policy() and not want_u and not selection and drop_seed is None and f_dtype == torch.float32
                and c_dtype == torch.float32 and _ops._timer is None and not self.dropout_active() and not exact_active()
                and _segments_now.get() is None):                 # (a packed batch: the C entry selects inside the library)
            out = self._forward_c(feats, coors, edges, mask, adj_mat, order_hint)
            if out is not None:
                return out
        kr = self._neighbour_count(n, adj_mat)                    # (the C entry declined before reading it)
        with torch.cuda.device(feats.device):
            if self.dropout_active() and drop_seed is None:
                drop_seed = _dropout.draw_seed()
            out = self._forward_hip(feats.float(), coors.float(),
                                    edges if (edges is None or isinstance(edges, EdgeLookup)) else edges.float(), mask, adj_mat, order_hint,
                                    want_u=want_u, drop=(self.dropout_p, drop_seed) if self.dropout_active() else None, kr=kr)
        if f_dtype != torch.float32 or c_dtype != torch.float32:
            out = (out[0].to(f_dtype), out[1].to(c_dtype)) + tuple(out[2:])
        return out

    def compute_dtype(self):
        """float64 for a module converted with .double() (every kernel of its forward then is a float64 kernel), else float32 (half /
        bfloat16 modules are converted at the boundary: at least their own precision)."""
        p = next(self.parameters(), None)
        return torch.float64 if (p is not None and p.dtype == torch.float64) else torch.float32

    def float64_kernels(self):
        """A float64 module runs on the float64 kernels (training-mode dropout included: the plain kernels evaluate the same hash masks)."""
        return self.compute_dtype() == torch.float64

    # ------------------------------------------------------------------ dispatch rules (each stated once, for both launch paths)
    def _use_nearest(self):
        """the k-NN path (a neighbour list of K per node) rather than the dense all-pairs one"""
        return self.num_nearest_neighbors > 0 or self.only_sparse_neighbors

    def _neighbour_count(self, n, adj_mat, dtype=torch.float32):
        """(K, valid_radius) of a call on N-node graphs (egnn_pytorch.py:240-252): N on the dense path; on the k-NN path the module's
        K -- or, for only_sparse_neighbors with an adjacency, its maximum degree and radius 0.  A packed call (`_segments_now`) caps the
        radius at the largest finite value of `dtype`, the dtype of its ranks: the empty slots of a graph below K rank at +inf and must
        fail `rank <= valid_radius` in the forward and in what the backward saves."""
        if not self._use_nearest():
            return n, self.valid_radius
        k, valid_radius = self.num_nearest_neighbors, self.valid_radius
        if _segments_now.get() is not None:
            valid_radius = min(valid_radius, torch.finfo(dtype).max)
        if adj_mat is not None and self.only_sparse_neighbors:
            with torch.cuda.device(adj_mat.device):
                k, valid_radius = _ops.adj_max_degree(adj_mat), 0.0   # host sync, as upstream (:249)
        if k > n:
            raise RuntimeError("selected index k out of range")      # torch.topk's error upstream
        return k, valid_radius

    def _order(self, coors, adj_mat, order_hint):
        """The Morton order the k-NN edge pass schedules by: `order_hint` when it fits, else a new (B,N) buffer for it (allocated on the
        launch stream); None when no order is used.  Neighbours are spatial, so workgroups that own Morton-adjacent nodes share gathered
        rows in L1.  Scheduling only (results do not depend on it), so a stack of layers reuses the first layer's order: coordinates
        move by small steps per layer and the locality survives."""
        b, n, cdim = coors.shape
        if not (_SPATIAL_ORDER and self._use_nearest() and adj_mat is None and cdim == 3 and 64 <= n <= 4096):
            return None
        if order_hint is not None and tuple(order_hint.shape) == (b, n) and order_hint.dtype == torch.int32 and order_hint.is_contiguous():
            return order_hint
        return _ops.empty(b, n, dtype=torch.int32, device=coors.device)

    def _dense_pw(self, b, n, cdim):
        """A dense layer on the wave-per-node edge kernel (csrc/edge_pw.hip), which reads per-slot records, here with j = k: with
        N % 32 == 0 and the standard layer's shape, and only when the batch fills the chip with one wave per node (measured, round 5:
        B N = 16 384 ... 32 768 nodes -2 ... -6.5 %; BASELINE.json's c2 -- 2048 nodes, each wave walking 8 rounds -- +25 %, so c2 stays
        on the general kernel, which splits a node's slots over workgroups).  The records are 16 B N^2 bytes: bounded."""
        return (_SLOT_PREP and _DENSE_PW and b * n >= 8192 and n % 32 == 0 and 32 <= n <= 4096 and cdim == 3 and self.m_dim <= 16
                and self.edge_dim == 0 and self.fourier_features == 0 and not self.dropout_active() and b * n * n * 16 <= (1 << 28))

    def _fused_covers(self, n, k):
        """One graph's rows of the (N, 2 Hp) fp32 projection table fit the 32-bit byte offsets of the fused edge kernels
        (egnn_edge_fused_covers: 4 GB per graph -- 258 111 nodes at dim 512; 2 GB where 6 <= K and K % 32 != 0).  A larger graph runs on the
        plain-fp32 kernels, which address with 64 bits: the same layer several times slower, never a wrapped offset."""
        h = 2 * (2 * self.fourier_features + 2 * self.dim + self.edge_dim + 1)
        if k <= 0 or n * (h + 32) * 8 <= 0x80000000:                      # (every ordinary shape: no call into the library)
            return True
        return _abi.load().egnn_edge_fused_covers(n, k, 2 * _abi.load().egnn_padded_hidden(h)) == 1

    def _use_grid(self, coors, adj_mat, k):
        """the neighbour selection of this call on the cell grid (egnn_knn_select_grid_f32; with a SparseAdjacency
        egnn_knn_select_grid_csr_f32) rather than the all-pairs kernels.  A dense adjacency stays there: its byte map is N^2 already.
        float64 coordinates are a float64 module's (`_forward_exact(dtype=torch.float64)`: egnn_knn_select_grid_f64 / _grid_csr_f64);
        every other caller has converted to float32 before it asks."""
        return (_segments_now.get() is None and coors.dtype in (torch.float32, torch.float64) and coors.shape[-1] == 3
                and (adj_mat is None or isinstance(adj_mat, SparseAdjacency))
                and 0 < k <= _ops.KNN_GRID_KMAX and coors.shape[1] >= _KNN_GRID_MIN_N)

    def _proj_row_mask(self, mask8, b, n, k, cdim, w, want_u, drop):
        """The projection GEMM's row mask (M-tiles of padded nodes are not computed), or None.  Only where the rows of padded nodes are
        read by masked-out edges alone: a k-NN layer whose edge pass is the wave-per-node kernel.  Not under autograd or dropout: the
        backward differentiates through every edge."""
        if (mask8 is None or want_u or drop is not None or not self._use_nearest() or k < 6 or not _SLOT_PREP or _EDGE_ALGO != 0
                or _abi.load().egnn_edge_pw_covers(b, n, k, w["S"], self.fourier_features, self.edge_dim, self.m_dim, cdim, 2 * w["Hp"]) != 1):
            return None
        return mask8.view(-1)

    def _select_outputs(self, coors, adj_mat, order_hint, k):
        """The four outputs of the k-NN selection (idx, rank, order or None, slots or None) and the workspace of the cell-grid selection
        (None where the all-pairs kernels select: `_use_grid`), allocated on the LAUNCH stream: the launch
        stream waits for the side stream before it reads them, so when they are freed every use is ordered before the launch stream's
        later work and the allocator may reuse the blocks at once.  (Allocated inside the fork they belonged to the side stream's pool
        and needed record_stream(): four calls per forward and frees deferred to events.)  order is the taken hint, if any."""
        b, n = coors.shape[:2]
        dev = coors.device
        return (_ops.empty(b, n, k, dtype=torch.int32, device=dev), _ops.empty(b, n, k, dtype=torch.float32, device=dev),
                self._order(coors, adj_mat, order_hint),
                _ops.empty(b * n * k, 4, dtype=torch.int32, device=dev) if (_SLOT_PREP and coors.shape[-1] == 3) else None,
                _ops.knn_grid_workspace(b, n, k, dev) if self._use_grid(coors, adj_mat, k) else None)

    def _knn_route(self, coors, mask, adj_mat, k, out=None, ws=None):
        """(idx, rank), both (B, N, K), of this call's neighbour selection on the route its inputs decide: a packed batch (B = 1) inside
        every node's own graph, else the cell grid where `_use_grid` says so, else the all-pairs kernels -- the same list bit for bit on
        the last two.  out = (idx, rank), ws = the grid's workspace: allocated by the caller (`_select_outputs`), or here when None."""
        segments = _segments_now.get()
        if segments is not None:
            idx, rank = _ops.knn_select_segments(coors[0], segments, k, out=None if out is None else (out[0][0], out[1][0]))
            return idx[None], rank[None]
        if self._use_grid(coors, adj_mat, k):                            # (sub-quadratic: `_KNN_GRID_MIN_N`)
            return _ops.knn_select_grid(coors, mask, k, out=out, ws=ws, adj=adj_mat)
        return _ops.knn_select(coors, mask, adj_mat, k, out=out)

    def _select_neighbors(self, coors, mask, adj_mat, order_hint, k, valid_radius, outs, fork=None):
        """(idx, rank, order, slots) of egnn_pytorch.py:230-260 for fp32 coordinates on the device, K > 0: the K nearest neighbours, the
        Morton order the edge pass schedules by, the per-slot records, written into `outs` (`_select_outputs`).  Neighbour selection
        (VALU / scalar bound, no MFMA) and the Morton order (one workgroup per graph) depend on the coordinates only; the projection GEMM
        (MFMA bound) on the features only: launched on the side stream they share the CUs instead of queueing, and whoever consumes the
        result joins that stream first.  fork: an event of the launch stream -- recorded at the layer's entry, before its node-level
        launches -- the side stream waits for instead of the stream's tail, so the selection runs beside node_prep and the projection
        although it is enqueued behind them.  It reads only what existed at that event: coors, mask, adj_mat and `outs`."""
        idx_o, rank_o, order_o, slots_o, grid_ws = outs
        mask8 = _ops._u8(mask)                                      # (a view: the caller made the mask contiguous before the fork)

        def select():
            # (the Morton order launched AHEAD of the selection was measured in round 6: +- 0.3 %, not kept)
            idx_, rank_ = self._knn_route(coors, mask, adj_mat, k, out=(idx_o, rank_o), ws=grid_ws)
            order_ = order_o if order_o is None or order_o is order_hint else _ops.spatial_order(coors, out=order_o, mask8=mask8)
            # the edge pass's setup as one coalesced record per slot instead of a chain of dependent loads
            slots_ = _ops.slot_prep(coors, mask8, idx_, rank_, order_, valid_radius, out=slots_o) if slots_o is not None else None
            return idx_, rank_, order_, slots_

        if _ops._timer is not None:
            return select()             # (one stream while per-kernel timing is on: events on two would charge one kernel's wait to another)
        side = _ops.side_stream(coors.device)
        if fork is not None:
            side.wait_event(fork)
        else:
            side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            return select()

    def _c_state(self, device):
        """(desc, info, blob on `device`, fused node_mlp image or None) of the C whole-layer entry for the current parameters; None when the
        C entry does not cover this layer's shape."""
        w = self.packed_weights()                                    # (re-laid out on the device once per parameter version)
        key = (self._packed_key, device)
        st = self.__dict__.get("_c_packed")
        if st is None or st[0] != key:
            try:
                desc, info, blob_dev = _ops.pack_weights_blob(self, w, device)
            except _abi.EGNNHipError:
                st = (key, None)
            else:
                img = w.get("nmf_img")
                st = (key, (desc, info, blob_dev, img.to(device) if img is not None else None))
            self.__dict__["_c_packed"] = st
        return st[1]

    def _forward_c(self, feats, coors, edges, mask, adj_mat, order_hint):
        """The fp32 inference forward as one call of egnn_layer_forward_opts_f32 (include/egnn_hip.h; csrc/layer_api.hip mirrors
        `_forward_hip_impl` launch for launch, so the outputs are the same bits).  Returns `_forward_hip`'s tuple, or None when the call is
        outside what the C entry covers (edge look-up tables, wide shapes, the wave-per-node kernel on dense batches, another current
        device, a graph whose neighbours the cell grid selects -- the C entry keeps its streaming selection): the Python launch sequence then runs it.  K is read after those checks, and a call with K = 0 goes to the Python launch
        sequence from here, with that K: the adjacency's maximum degree is read once per call."""
        b, n, dim = feats.shape
        cdim = coors.shape[-1]
        use_nearest = self._use_nearest()
        dev = feats.device
        if (isinstance(edges, EdgeLookup) or cdim > 8 or self.m_dim > 64 or 2 * self.fourier_features + 1 + self.edge_dim > 16
                or dev.index != torch.cuda.current_device() or (adj_mat is not None and adj_mat.dtype != torch.bool)
                or isinstance(adj_mat, SparseAdjacency)             # (the C entry keeps its dense signature)
                or (not use_nearest and self._dense_pw(b, n, cdim))
                or (use_nearest and self._use_grid(coors, adj_mat, self.num_nearest_neighbors))):
            return None
        st = self._c_state(dev)
        if st is None:
            return None
        desc, info, blob_dev, img = st
        kr = k, valid_radius = self._neighbour_count(n, adj_mat)
        if k == 0 or not self._fused_covers(n, k):                  # (no messages / a graph beyond the fused kernels' offsets: not the C entry's)
            return self._forward_hip(feats, coors, edges, mask, adj_mat, order_hint, kr=kr)
        feats, coors = _ops.aligned(feats), _ops.aligned(coors)     # (any layout of the caller's: `_ops.aligned`)
        if edges is not None:
            edges = _ops.aligned(edges.float())
        m8, a8 = _ops._u8(mask), _ops._u8(adj_mat)
        stride = n * n if (a8 is not None and a8.dim() == 3) else 0
        lib = _abi.load()
        nbytes = lib.egnn_workspace_bytes(desc, b, n, k)
        # every buffer is allocated HERE, on the launch stream (the side stream writes the selection's part of the workspace between the
        # two events of this call: `_select_outputs` has the argument)
        ws = _ops.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        node_out = _ops.empty(b, n, dim, dtype=torch.float32, device=dev) if self.node_mlp is not None else feats
        coors_out = _ops.empty(b, n, cdim, dtype=torch.float32, device=dev) if self.coors_mlp is not None else coors
        opts = _abi.ForwardOpts()
        order = self._order(coors, adj_mat, order_hint)
        if order is not None:
            opts.order, opts.order_is_hint = order.data_ptr(), int(order is order_hint)
        if use_nearest:
            opts.side_stream, opts.ev_fork, opts.ev_join = _ops.side_handles(dev)
        if img is not None:
            opts.nmf_img = img.data_ptr()
        # the range check that follows this call (sync mode): the status words are published by the C entry, behind its last launch that
        # can write them, and `_ops.range_check_after_forward` only waits for the sequence number requested here
        pub = _ops.status_request(dev)
        if pub is not None:
            opts.status_pub, opts.status_words, opts.status_seq = pub
        rc = lib.egnn_layer_forward_opts_f32(desc, info, blob_dev.data_ptr(), feats.data_ptr(), coors.data_ptr(), _ops._ptr(edges), _ops._ptr(m8),
                                             _ops._ptr(a8), stride, b, n, k, cdim, node_out.data_ptr(), coors_out.data_ptr(), ws.data_ptr(),
                                             nbytes, _ops._status_ptr(dev), _ops._stream(), opts)
        if rc != 0 and opts.side_stream:
            # the selection may still be writing into the workspace on the side stream: join it before the buffers are freed
            torch.cuda.current_stream().wait_stream(_ops.side_stream(dev))
        _abi.check(rc, "egnn_layer_forward_opts_f32")
        return node_out, coors_out, order, None, None, valid_radius, None, None

    def _forward_hip(self, feats, coors, edges, mask, adj_mat, order_hint=None, want_u=False, drop=None, kr=None):
        """The Python launch sequence; kr = (K, valid_radius) of `_neighbour_count` when the caller has read it already."""
        if kr is None:
            kr = self._neighbour_count(feats.shape[1], adj_mat)
        try:
            return self._forward_hip_impl(feats, coors, edges, mask, adj_mat, kr, order_hint, want_u, drop)
        except BaseException:
            # the neighbour selection may still be writing its outputs on the side stream: join it before they are freed (they belong
            # to the launch stream's pool: `_select_outputs`)
            if feats.is_cuda:
                torch.cuda.current_stream().wait_stream(_ops.side_stream(feats.device))
            raise

    def _forward_hip_impl(self, feats, coors, edges, mask, adj_mat, kr, order_hint, want_u, drop):
        # more per-edge scalars than the split-fp16 edge kernels carry (2 fourier + 1 + edge_dim > 16, up to 160): the plain-fp32 kernels
        # ... and more than 8 coordinates (the fused kernels keep x_i - x_j in registers up to 8)
        # ... and heads wider than 64 message channels (the fused kernels hold up to four 16-channel accumulator tiles per edge tile)
        # ... and a single graph whose rows of the projection table the fused kernels' 32-bit byte offsets do not reach (`_fused_covers`)
        wide_shape = (2 * self.fourier_features + 1 + self.edge_dim > 16 or coors.shape[-1] > 8 or self.m_dim > 64
                      or not self._fused_covers(feats.shape[1], kr[0]))
        if exact_active() or wide_shape:
            return self._forward_exact(feats, coors, edges, mask, adj_mat, kr, want_u=want_u, drop=drop)
        b, n, dim = feats.shape
        k, valid_radius = kr
        w = self.packed_weights()
        feats = _ops.aligned(feats)                                 # (any layout of the caller's: contiguous, at a 16-byte boundary)
        coors = _ops.aligned(coors)
        # What the neighbour selection reads on the side stream -- coors, mask, adj_mat -- is made contiguous HERE, before the fork event
        # below, and every `_u8` of it is a view from then on: a copy enqueued behind that event (a sliced or expanded mask) would be a
        # kernel the side stream does not wait for, and the selection could read its output before it is written.
        mask = None if mask is None else mask.contiguous()
        adj_mat = None if adj_mat is None else adj_mat.contiguous()
        mask8 = _ops._u8(mask)
        feats2d = feats.view(b * n, dim)
        lookup = edges if isinstance(edges, EdgeLookup) else None
        if lookup is not None:
            edges = lookup.edges
        elif edges is not None:
            edges = _ops.aligned(edges.float())

        # ---- neighbour selection (egnn_pytorch.py:230-260)
        use_nearest = self._use_nearest()
        sel = outs = fork = None
        if not use_nearest:
            sel = None, None, None, (_ops.slot_prep(coors, mask8, None, None, None, valid_radius) if self._dense_pw(b, n, coors.shape[-1])
                                     else None)
        elif k > 0:
            outs = self._select_outputs(coors, adj_mat, order_hint, k)
            if adj_mat is not None and self.only_sparse_neighbors:
                sel = self._select_neighbors(coors, mask, adj_mat, order_hint, k, valid_radius, outs)
            else:
                # When K is known without looking at the data (not only_sparse_neighbors with an adjacency, whose K is its maximum
                # degree), the node-level launches go FIRST and the selection -- on the side stream, needed by the edge pass only -- is
                # enqueued behind them, although it depends on nothing they write: fork point = here.  The first kernel of the forward
                # starts ~30 us earlier, which is what a synchronous range check exposes per call.
                fork = _ops.fork_event(feats.device)

        node_out, coors_out = feats, coors
        node_in = u_pre = proj_kept = idx = rank = order = None
        if k > 0:
            # ---- node-level projections P = feats [W_i ; W_j]^T + [b1 ; 0]
            # (K >= 6: the edge pass feeds P_i to its first-layer MFMA as (fp16 hi, fp16 lo) words)
            hp = w["Hp"]
            pi_split = k >= 6
            if self.node_mlp is not None:
                # one pass over feats: its (hi, lo) split for the projection AND [LayerNorm(feats) | 0] for node_mlp
                # (egnn_pytorch.py:335-336); the edge pass drops m_i into the zero columns
                # (node_norm = Identity, the reference's default: the two are the same values -- the projection reads the first
                # `dim` columns of the [feats | 0] image, egnn_linear_hl_lda_f32; 134 MB less to write at the north-star shape)
                if w.get("gamma") is None:
                    node_in = feats_hl = _ops.node_prep_hl(feats2d, None, None, None, 1e-5, self.m_dim)
                else:
                    node_in, feats_hl = _ops.node_prep_hl(feats2d, None, w.get("gamma"), w.get("beta"), w.get("ln_eps", 1e-5),
                                                          self.m_dim, with_raw=True)
            else:
                feats_hl = _ops.split_f16(feats2d)
            proj = _ops.linear_hl(feats_hl, w["Wcat_split"], 2 * hp, w["bcat"], name="node_proj", split_cols=hp if pi_split else 0,
                                  row_mask=self._proj_row_mask(mask8, b, n, k, coors.shape[-1], w, want_u, drop))
            del feats_hl
            if sel is None:
                sel = self._select_neighbors(coors, mask, adj_mat, order_hint, k, valid_radius, outs, fork)
            idx, rank, order, slots = sel
            side_join = use_nearest and _ops._timer is None
            a = _abi.EdgeArgs()
            a.B, a.N, a.K, a.dim, a.m_dim = b, n, k, dim, self.m_dim
            a.H, a.Hp = w["H"], hp
            a.fourier, a.edge_dim, a.S, a.pi_split = self.fourier_features, self.edge_dim, w["S"], int(pi_split)
            a.Pi = proj.data_ptr()
            a.Pj = proj.data_ptr() + 4 * hp
            a.ldp = 2 * hp
            a.Wst, a.W2h, a.b2 = w["Wst"].data_ptr(), w["W2h"].data_ptr(), w["b2"].data_ptr()
            a.ws_inv_scale, a.wst_terms = w["ws_inv_scale"], w["Wst"].shape[1]
            a.w2_inv_scale = w["w2_inv_scale"]
            if self.edge_gate is not None:
                a.gate_w, a.gate_b = w["gate_w"].data_ptr(), w["gate_b"].data_ptr()
            if self.coors_mlp is not None:
                a.W3h, a.b3, a.W4, a.b4 = (w[x].data_ptr() for x in ("W3h", "b3", "W4", "b4"))
                a.w3_inv_scale = w["w3_inv_scale"]
                coors_out = _ops.empty(*coors.shape, dtype=coors.dtype, device=coors.device)
                a.coors_out = coors_out.data_ptr()
            if self.norm_coors:
                a.coors_scale = w["coors_scale"].data_ptr()
            a.coors, a.coor_dim = coors.data_ptr(), coors.shape[-1]
            if lookup is not None:
                # the features of the K selected pairs only, read by the kernel in neighbour-list order
                if side_join:
                    torch.cuda.current_stream().wait_stream(_ops.side_stream(feats.device))
                edges = _ops.edge_features_gather(lookup, idx, b, n, k)
                a.edges_by_k = 1
            a.edges = _ops._ptr(edges)
            a.mask = _ops._ptr(mask8)
            if side_join:
                torch.cuda.current_stream().wait_stream(_ops.side_stream(feats.device))
            a.idx, a.rank = _ops._ptr(idx), _ops._ptr(rank)
            a.order, a.slots = _ops._ptr(order), _ops._ptr(slots)
            a.valid_radius = float(min(valid_radius, 3.0e38))
            cv = self.coor_weights_clamp_value
            a.clamp = -1.0 if cv is None else float(cv)
            a.pool_mean = int(self.m_pool_method == "mean")
            if self.node_mlp is not None:
                a.node_hi, a.node_lo, a.node_kp = node_in.hi.data_ptr(), node_in.lo.data_ptr(), node_in.kp
            if drop is not None:                                  # training-mode dropout: the mask is a hash, see _dropout.py
                a.drop_thr, a.drop_seed, a.drop_inv_keep = _dropout.threshold(drop[0]), int(drop[1]), _dropout.inv_keep(drop[0])
            if want_u:                                            # (rows of whole 16-channel accumulator tiles, pad channels 0)
                u_pre = _ops.empty(b * n * k, 16 * _weights.m_blocks(self.m_dim), dtype=torch.float32, device=feats.device)
                a.U_out = u_pre.data_ptr()
            a.algo = _EDGE_ALGO
            _ops.edge_fused(a, feats.device)
            if u_pre is not None:
                proj_kept = (proj, pi_split)
            del proj
        elif self.node_mlp is not None:                                   # K == 0: no messages, m_i = 0
            node_in = _ops.node_prep_hl(feats2d, None, w.get("gamma"), w.get("beta"), w.get("ln_eps", 1e-5), self.m_dim)

        # ---- node update (egnn_pytorch.py:335-337)
        if self.node_mlp is not None:
            if drop is None and "nmf_img" in w:
                # narrow layers (dim <= 256): both Linears in one launch, the hidden activation stays in registers
                node_out = _ops.node_mlp_fused(node_in, w["nmf_img"], w["W5_split"][2], w["b5"], w["W6_split"][2], w["b6"], feats2d,
                                               dim, self.m_dim).view(b, n, dim)
            else:
                hid = _ops.linear_hl(node_in, w["W5_split"], 2 * dim, w["b5"], act=1, out_f32=False, out_hl=True,
                                     name="node_mlp0", drop=drop)
                node_out = _ops.linear_hl(hid, w["W6_split"], dim, w["b6"], residual=feats2d, name="node_mlp1").view(b, n, dim)
        return node_out, coors_out, order, idx, rank, valid_radius, u_pre, proj_kept


    def _forward_exact(self, feats, coors, edges, mask, adj_mat, kr, dtype=torch.float32, want_u=False, drop=None):
        """The layer on the plain-fp32 kernels (include/egnn_hip.h, "The wide-range path"): exact-fp32 GEMMs, fp32 node_norm, the edge
        pass as fp32 VALU arithmetic on the module's own weight tensors.  Same arguments (kr = (K, valid_radius) of `_neighbour_count`),
        same neighbour selection, same return tuple as _forward_hip.
        dtype = torch.float64: the same kernels instantiated for double ("The float64 path"; feats / coors / edges are float64).
        drop = (p, seed): training-mode dropout -- the fused kernels' hash masks at the three sites (egnn_edge_exact_args.drop_*,
        egnn_drop_silu_*)."""
        esz = 8 if dtype == torch.float64 else 4
        b, n, dim = feats.shape
        feats = _ops.aligned(feats)
        coors = _ops.aligned(coors)
        feats2d = feats.view(b * n, dim)
        lookup = edges if isinstance(edges, EdgeLookup) else None
        if lookup is not None:
            edges = lookup.edges
        elif edges is not None:
            edges = _ops.aligned(edges.to(dtype))
        mask8 = _ops._u8(mask)
        k, valid_radius = kr
        idx = rank = None
        if self._use_nearest() and k > 0:
            idx, rank = self._knn_route(coors, mask, adj_mat, k)
        f32 = lambda t: t.detach().to(dtype).contiguous()                # noqa: E731  (the module's tensors in the compute dtype)
        node_out, coors_out, m_i = feats, coors, None
        u_pre = proj_keep = None                                         # want_u (forward under autograd): u (E, m_dim) and the projection table
        if k > 0:
            lin0, lin3 = self.edge_mlp[0], self.edge_mlp[3]
            w1 = f32(lin0.weight)                                        # (H, Din): [W_i | W_j | scalar columns]
            h, din = w1.shape
            hq = (h + 3) // 4 * 4
            proj = _ops.empty(b * n, 2 * hq, dtype=dtype, device=feats.device)
            _ops.linear_f32(feats2d, w1, h, dim, bias=f32(lin0.bias), out=proj[:, :h], name="node_proj_f32")
            _ops.linear_f32(feats2d, w1[:, dim:], h, dim, out=proj[:, hq:hq + h], name="node_proj_f32")
            a = _abi.EdgeExactArgs()
            a.B, a.N, a.K, a.m_dim, a.H = b, n, k, self.m_dim, h
            a.fourier, a.edge_dim, a.coor_dim = self.fourier_features, self.edge_dim, coors.shape[-1]
            a.pool_mean = int(self.m_pool_method == "mean")
            a.Pi, a.Pj, a.ldp = proj.data_ptr(), proj.data_ptr() + esz * hq, 2 * hq
            a.Ws, a.ldws = w1.data_ptr() + esz * 2 * dim, din
            keep = [w1, f32(lin3.weight), f32(lin3.bias)]
            a.W2, a.b2 = keep[1].data_ptr(), keep[2].data_ptr()
            if self.edge_gate is not None:
                keep += [f32(self.edge_gate[0].weight).view(-1), f32(self.edge_gate[0].bias)]
                a.gate_w, a.gate_b = keep[-2].data_ptr(), keep[-1].data_ptr()
            if self.coors_mlp is not None:
                c0, c3 = self.coors_mlp[0], self.coors_mlp[3]
                keep += [f32(c0.weight), f32(c0.bias), f32(c3.weight).view(-1), f32(c3.bias)]
                a.W3, a.b3, a.W4, a.b4 = (t.data_ptr() for t in keep[-4:])
                coors_out = _ops.empty(*coors.shape, dtype=dtype, device=coors.device)
                a.coors_out = coors_out.data_ptr()
            if self.norm_coors:
                keep.append(f32(self.coors_norm.scale))
                a.coors_scale = keep[-1].data_ptr()
            a.coors = coors.data_ptr()
            if lookup is not None:
                edges = _ops.edge_features_gather(lookup, idx, b, n, k)
                a.edges_by_k = 1
            a.edges, a.mask = _ops._ptr(edges), _ops._ptr(mask8)
            a.idx, a.rank = _ops._ptr(idx), _ops._ptr(rank)
            a.valid_radius = float(valid_radius) if dtype == torch.float64 else float(min(valid_radius, 3.0e38))
            cv = self.coor_weights_clamp_value
            a.clamp = -1.0 if cv is None else float(cv)
            if self.node_mlp is not None:
                m_i = _ops.empty(b * n, self.m_dim, dtype=dtype, device=feats.device)
                a.m_i = m_i.data_ptr()
            if want_u:
                u_pre = _ops.empty(b * n * k, self.m_dim, dtype=dtype, device=feats.device)
                a.U_out = u_pre.data_ptr()
                proj_keep = (proj, False)
            _ops.set_drop(a, drop)
            _ops.edge_exact(a, feats.device, dtype)
            del proj, keep
        elif self.node_mlp is not None:
            m_i = torch.zeros(b * n, self.m_dim, dtype=dtype, device=feats.device)        # K == 0: no messages
        if self.node_mlp is not None:
            ln = self.node_norm if isinstance(self.node_norm, nn.LayerNorm) else None
            node_in = _ops.node_prep_f32(feats2d, m_i, f32(ln.weight) if ln is not None else None,
                                         f32(ln.bias) if ln is not None else None, ln.eps if ln is not None else 1e-5, self.m_dim)
            n0, n3 = self.node_mlp[0], self.node_mlp[3]
            if drop is None:
                hid = _ops.linear_f32(node_in, f32(n0.weight), 2 * dim, dim + self.m_dim, bias=f32(n0.bias), act=1, name="node_mlp0_f32")
            else:                                                        # Linear -> Dropout -> SiLU (egnn_pytorch.py:196-201)
                hid = _ops.drop_silu_(_ops.linear_f32(node_in, f32(n0.weight), 2 * dim, dim + self.m_dim, bias=f32(n0.bias), name="node_mlp0_f32"), drop)
            node_out = _ops.linear_f32(hid, f32(n3.weight), dim, 2 * dim, bias=f32(n3.bias), residual=feats2d,
                                       name="node_mlp1_f32").view(b, n, dim)
        return node_out, coors_out, None, idx, rank, valid_radius, u_pre, proj_keep


_FP64_WARNED = False


def _embed_pairs(emb, idx):
    """emb(idx) for a (B,N,N) index tensor of any size: the materialised (B,N,N,D) recipe of egnn_pytorch.py:410-432, which no module
    here runs any more (EGNN_Network reads look-up tables in every dtype) -- kept for the timing tools under tools/ only.
    torch's device embedding fails to launch (invalid configuration) on (1, 8192, 8192) indices on the MI355X; up to 2^24 indices it is
    one call, beyond that chunks of at most 2^24 indices and 2^26 outputs (the sizes it handles), concatenated.  Under autograd: the
    weight's gradient sums the chunks' in turn."""
    n = idx.numel()
    if n <= 1 << 24:
        return emb(idx)
    step = max(1, min(1 << 24, (1 << 26) // max(1, emb.embedding_dim)))
    flat = idx.reshape(-1)
    return torch.cat([emb(flat[lo:lo + step]) for lo in range(0, n, step)]).view(*idx.shape, emb.embedding_dim)


def _warn_float64_once():
    """float64 callers get float64 tensors back, computed with fp32-class arithmetic (split-fp16 products, ~22 significant
    bits, fp32 accumulation): say so once per process instead of silently."""
    global _FP64_WARNED
    if _FP64_WARNED:
        return
    _FP64_WARNED = True
    import warnings
    warnings.warn("egnn_pytorch_amd: float64 inputs / modules are converted at the boundary and computed with fp32-class "
                  "arithmetic on the gfx950 kernels (about 22 significant bits; results are returned as float64). "
                  "The reference computes float64 in float64.", RuntimeWarning, stacklevel=4)


class EGNN_Network(nn.Module):
    """Stack of EGNN layers (egnn_pytorch.py:343-454).  The layer loop -- the part BASELINE.json's
    configs exercise -- runs on the HIP kernels; the token / position / edge / adjacency-degree
    front-end is ordinary tensor plumbing on the device, and so is the optional induced-set attention between
    layers (`global_linear_attn_every > 0`, egnn_pytorch_amd/attention.py: outside the per-edge hot path)."""

    def __init__(self, *, depth, dim, num_tokens=None, num_edge_tokens=None, num_positions=None,
                 edge_dim=0, num_adj_degrees=None, adj_dim=0, global_linear_attn_every=0,
                 global_linear_attn_heads=8, global_linear_attn_dim_head=64, num_global_tokens=4,
                 **kwargs):
        super().__init__()
        assert not (num_adj_degrees is not None and num_adj_degrees < 1), \
            "make sure adjacent degrees is greater than 1"
        self.num_positions = num_positions
        self.token_emb = nn.Embedding(num_tokens, dim) if num_tokens is not None else None
        self.pos_emb = nn.Embedding(num_positions, dim) if num_positions is not None else None
        self.edge_emb = nn.Embedding(num_edge_tokens, edge_dim) if num_edge_tokens is not None else None
        self.has_edges = edge_dim > 0
        self.num_adj_degrees = num_adj_degrees
        self.adj_emb = nn.Embedding(num_adj_degrees + 1, adj_dim) \
            if (num_adj_degrees is not None and adj_dim > 0) else None
        edge_dim = edge_dim if self.has_edges else 0
        adj_dim = adj_dim if num_adj_degrees is not None else 0
        has_global_attn = global_linear_attn_every > 0
        self.global_tokens = nn.Parameter(torch.randn(num_global_tokens, dim)) if has_global_attn else None

        self.layers = nn.ModuleList()
        for ind in range(depth):
            # index 0 of each pair is the optional attention block: keys `layers.{l}.0.*` / `layers.{l}.1.*` (:381-388)
            is_global = has_global_attn and ind % global_linear_attn_every == 0
            self.layers.append(nn.ModuleList([
                GlobalLinearAttention(dim=dim, heads=global_linear_attn_heads,
                                      dim_head=global_linear_attn_dim_head) if is_global else None,
                EGNN(dim=dim, edge_dim=edge_dim + adj_dim, norm_feats=True, **kwargs)]))

    def forward(self, feats, coors, adj_mat=None, edges=None, mask=None, return_coor_changes=False):
        if _ops.RANGE_CHECK == "deferred" and coors.is_cuda:
            _ops.check_range(coors.device, wait=False)
        # under autograd the embeddings are ordinary differentiable modules, every EGNN layer records its own autograd.Function and
        # every attention block its four (attention.py: the node-sized steps on the HIP kernels, the token-sized ones in ATen);
        # otherwise nothing is recorded
        grad = torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters()) or
                                            any(torch.is_tensor(t) and t.is_floating_point() and t.requires_grad
                                                for t in (feats, coors, edges.values if isinstance(edges, SparseEdges) else edges)))
        try:
            with _ops.early_publish(last=False) as early:           # (`_forward` sets `last` in front of the last layer)
                with torch.enable_grad() if grad else torch.no_grad():
                    out = self._forward(feats, coors, adj_mat, edges, mask, return_coor_changes, early)
                _ops.range_check_after_forward(coors.device)        # once per network forward, not per layer
        except _abi.EGNNRangeError as err:
            if err.origin == "backward" or not _rerun_exact_ok(self, feats, coors, edges):
                raise
            _warn_rerun(err)
            with exact_arithmetic(), (torch.enable_grad() if grad else torch.no_grad()):    # the whole stack again, in plain fp32
                out = self._forward(feats, coors, adj_mat, edges, mask, return_coor_changes)
        return out

    def _forward_packed(self, feats, coors, adj_mat, edges, segments, return_coor_changes, early=None):
        """`_forward` for a packed batch: tokens (T,) or features (T, dim), coors (T, C), a GraphSegments where the mask goes; the
        position embedding is indexed by each node's index inside its own graph."""
        if self.global_tokens is not None:
            raise NotImplementedError("a packed batch (mask=GraphSegments) with global_linear_attn_every > 0 is not supported: attention "
                                      "segmented by graph is a kernel of its own (DESIGN.md section 9); pad the batch")
        if self.num_adj_degrees is not None:
            raise NotImplementedError("a packed batch (mask=GraphSegments) with num_adj_degrees is not supported: the adjacency of a "
                                      "packed batch is a follow-up (DESIGN.md section 9); pad the batch")
        if edges is not None or self.has_edges:
            raise NotImplementedError("a packed batch (mask=GraphSegments) with edges is not supported: per-pair edge features of a "
                                      "packed batch are a follow-up (DESIGN.md section 9); pad the batch")
        if adj_mat is not None:
            raise NotImplementedError("a packed batch (mask=GraphSegments) with adj_mat is not supported: the adjacency ranking of the "
                                      "segmented selection is a follow-up (DESIGN.md section 9); pad the batch, or drop adj_mat")
        if feats.dim() != (1 if self.token_emb is not None else 2) or feats.shape[0] != segments.num_nodes:
            raise ValueError(f"feats shape {tuple(feats.shape)}: a packed batch of {segments.num_nodes} nodes takes "
                             f"{'tokens (T,)' if self.token_emb is not None else 'features (T,dim)'}")
        if self.token_emb is not None:
            feats = self.token_emb(feats)
        if self.pos_emb is not None:
            n = segments.max_size
            assert n <= self.num_positions, \
                f"given sequence length {n} must be less than the number of positions {self.num_positions} set at init"
            feats = feats + self.pos_emb(segments.positions)
        coor_changes = [coors]
        order = None
        for ind, (_, egnn) in enumerate(self.layers):
            if early is not None:
                early.last = ind == len(self.layers) - 1
            feats, coors, order = egnn._call(feats, coors, None, segments, None, order)
            coor_changes.append(coors)
        if return_coor_changes:
            return feats, coors, coor_changes
        return feats, coors

    def _forward(self, feats, coors, adj_mat, edges, mask, return_coor_changes, early=None):
        if isinstance(mask, GraphSegments):
            return self._forward_packed(feats, coors, adj_mat, edges, mask, return_coor_changes, early)
        b = feats.shape[0]
        if self.token_emb is not None:
            feats = self.token_emb(feats)
        if self.pos_emb is not None:
            n = feats.shape[1]
            assert n <= self.num_positions, \
                f"given sequence length {n} must be less than the number of positions {self.num_positions} set at init"
            feats = feats + self.pos_emb(torch.arange(n, device=feats.device))[None]
        # Edge features for the layers: look-up tables (EdgeLookup) -- the (B,N,N,edge_dim+adj_dim) tensor of :410-432 is never
        # materialised, the edge kernel reads the embedding rows of the K selected pairs of each node.  Under autograd the embedding
        # weights (and dense float edges) are inputs of each layer's autograd.EGNNFunction, whose backward reduces their gradients over
        # the same pairs (egnn_edge_features_grad_f32 / _f64).  The tables' kernel-side copies take the layers' compute dtype, made once
        # here for all of them: float64 for a float64 network, which runs on the tables like any other.
        lookup_dtype = self.layers[0][1].compute_dtype() if len(self.layers) else torch.float32
        tok = tok_emb = csr = None
        if isinstance(edges, SparseEdges):
            # bond tokens / bond features on CSR rows: the first table of the look-up, read through the positions the kernel finds in
            # the rows (csrc/edge_csr.hip) -- no (B,N,N) token map, no (B,N,N,edge_dim) tensor and no gradient of that size
            if edges.is_tokens != (self.edge_emb is not None):
                raise TypeError("a SparseEdges holds int64 tokens for a network with num_edge_tokens, float values otherwise "
                                f"(got {edges.values.dtype})")
            if not edges.is_tokens and edges.values.dtype not in _FLOAT_DTYPES:
                raise NotImplementedError(f"the gfx950 path takes floating-point edges (got {edges.values.dtype})")
            csr, edges = edges, None
            tok_emb = self.edge_emb.weight if csr.is_tokens else None
        elif edges is not None and self.edge_emb is not None:
            tok, tok_emb, edges = edges, self.edge_emb.weight, None

        if self.num_adj_degrees is not None:
            assert adj_mat is not None, "adjacency matrix must be passed in (keyword argument adj_mat)"
            if not adj_mat.is_cuda:
                raise RuntimeError("egnn_pytorch_amd.EGNN_Network runs only on an MI355X (cuda/HIP) device")
            # N-degree expansion (egnn_pytorch.py:414-427) as bit-set algebra on the device instead of float matmuls
            # (a SparseAdjacency: the same expansion on CSR rows, csrc/adj_csr.hip -- the expanded adjacency and the labels stay CSR)
            if isinstance(adj_mat, SparseAdjacency):
                adj_mat, adj_indices = _ops.adj_expand_csr(adj_mat, b, self.num_adj_degrees)
            else:
                adj_mat, adj_indices = _ops.adj_expand(adj_mat, b, self.num_adj_degrees)
            if self.adj_emb is not None:
                edges = EdgeLookup(edges=edges, tok=tok, tok_emb=tok_emb, deg=adj_indices, deg_emb=self.adj_emb.weight, dtype=lookup_dtype,
                                   csr=csr)
                tok = csr = None
        if tok is not None or csr is not None:                      # edge tokens / a SparseEdges without adjacency degrees
            edges = EdgeLookup(tok=tok, tok_emb=tok_emb, dtype=lookup_dtype, csr=csr)

        global_tokens = None
        if self.global_tokens is not None:
            global_tokens = self.global_tokens[None].expand(b, -1, -1)
        coor_changes = [coors]
        order = None
        for ind, (global_attn, egnn) in enumerate(self.layers):
            if global_attn is not None:
                feats, global_tokens = global_attn(feats, global_tokens, mask=mask)           # :445-446
            if early is not None:
                early.last = ind == len(self.layers) - 1            # nothing behind the last layer writes the status word
            feats, coors, order = egnn._call(feats, coors, edges, mask, adj_mat, order)
            coor_changes.append(coors)
        if return_coor_changes:
            return feats, coors, coor_changes
        return feats, coors

"""Thin wrappers: torch tensors (device memory + stream plumbing) -> C-ABI calls of libegnn_hip.so.

Nothing here computes: each function validates, allocates outputs with torch (caching allocator) and
enqueues one HIP kernel on torch's current stream.
"""
from __future__ import annotations

import contextlib
import contextvars
import threading
import time
import os
from ctypes import byref, c_int64

import torch

from . import _abi
from .segments import GraphSegments
from .sparse_adj import SparseAdjacency, SparseLabels


class PhaseTimer:
    """Optional per-kernel timing with events on the launch stream (used by bench.py / profiling).

    with phase_timer() as t: layer(...)   ->  t.summary() = {kernel: [ms, ...]}
    """

    def __init__(self):
        self.records = []

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, e0, e1 in self.records:
            out.setdefault(name, []).append(e0.elapsed_time(e1))
        return out


_timer = None


@contextlib.contextmanager
def phase_timer():
    global _timer
    prev, _timer = _timer, PhaseTimer()
    try:
        yield _timer
    finally:
        _timer = prev


@contextlib.contextmanager
def _timed(name):
    if _timer is None:
        yield
        return
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    yield
    e1.record()
    _timer.records.append((name, e0, e1))


_POISON = os.environ.get("EGNN_POISON_ALLOC", "0") == "1"


def empty(*shape, dtype, device):
    """torch.empty for kernel outputs / workspaces.  EGNN_POISON_ALLOC=1 (test aid) fills them with NaN / 0x7f bytes
    first: an element a kernel forgets to write can then not hide behind stale-but-correct data that the caching
    allocator hands back from the previous call."""
    t = torch.empty(*shape, dtype=dtype, device=device)
    if _POISON:
        if t.dtype.is_floating_point:
            t.fill_(float("nan"))
        else:
            t.view(torch.uint8).fill_(0x7F)
    return t


def _stream():
    """The raw hipStream_t of torch's current stream on the current device.  Through the C binding when it exists: the public
    torch.cuda.current_stream() builds a Stream object through three layers of device-index helpers (8 us a call, thirteen calls per
    forward: a third of the host time of a forward, tools/host_overhead_probe.py)."""
    try:
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    except AttributeError:
        return torch.cuda.current_stream().cuda_stream


_side = {}


def side_stream(device):
    """One extra HIP stream per device for work that is independent of the main launch sequence (layer.py)."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    st = _side.get(key)
    if st is None:
        st = _side[key] = torch.cuda.Stream(device=torch.device("cuda", key))
    return st


_side_handles = {}


def side_handles(device):
    """(raw hipStream_t of the side stream, raw hipEvent_t fork, raw hipEvent_t join) for the C whole-layer entry (egnn_forward_opts);
    one pair of events per device and thread, kept alive here (an event may be re-recorded once the call that used it is enqueued)."""
    import threading
    key = (device.index, threading.get_ident())
    h = _side_handles.get(key)
    if h is None:
        side = side_stream(device)
        evs = (torch.cuda.Event(), torch.cuda.Event())
        for ev in evs:
            ev.record(side)                                   # (torch creates the hipEvent_t at the first record)
        h = _side_handles[key] = (side.cuda_stream, evs[0].cuda_event, evs[1].cuda_event, side, evs)
    return h[:3]


_fork_events = {}


def fork_event(device):
    """An event recorded NOW on the current stream of `device` (one cached event object per device and thread: a later record
    replaces the earlier one, and whoever waits for it does so right behind the record -- layer.py::_forward_hip_impl)."""
    import threading
    key = (torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device(), threading.get_ident())
    ev = _fork_events.get(key)
    if ev is None:
        ev = _fork_events[key] = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(torch.device("cuda", key[0])))
    return ev


def _ptr(t):
    return None if t is None else t.data_ptr()


def aligned(t):
    """`t` as the kernels take a caller's tensor: contiguous and at a 16-byte boundary (they load four floats at a time, and several
    entries return EGNN_E_ALIGN otherwise).  `t` itself when it is that already -- two integer tests on the host, no launch -- else a
    fresh contiguous copy: `.contiguous()` is not enough, it returns a contiguous view at a 4- or 8-byte offset (a `narrow` of a
    buffer) as it is.  The boundary of the module for every layout a pipeline produces -- sliced, transposed, expanded, offset views
    -- applied where a caller's memory enters: the forward entries of layer.py / attention.py, the cotangents at the top of every
    autograd.Function's backward, `absmax_async`.  Under autograd the copy is a differentiable clone.  None passes through."""
    if t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0):
        return t
    return t.clone(memory_format=torch.contiguous_format)


def _u8(t):
    """bool tensor -> same storage viewed as bytes."""
    if t is None:
        return None
    if t.dtype != torch.bool:
        raise TypeError(f"mask / adj_mat must be torch.bool (got {t.dtype})")
    return t.contiguous().view(torch.uint8)


# ---------------------------------------------------------------------------------------------- numerical-range status
# One int32 status word per device (include/egnn_hip.h: EGNN_RANGE_*).  Kernels OR bits into it when a finite value leaves
# what the split-fp16 arithmetic carries (the value turns into inf / NaN).  When it is read back is the caller's choice:
#   EGNN_RANGE_CHECK=sync      (default) every forward ends with one 4-byte device->host read and raises EGNNRangeError
#   EGNN_RANGE_CHECK=deferred  no synchronisation: the word is copied to pinned memory after each forward and examined at
#                              the start of the next one (or by egnn_pytorch_amd.check_range()); bench.py uses this
#   EGNN_RANGE_CHECK=off       never read (outputs are still non-finite when it happens)
RANGE_CHECK = os.environ.get("EGNN_RANGE_CHECK", "sync")
_SPIN = os.environ.get("EGNN_RANGE_SPIN", "1") != "0"
_SPIN_SECONDS = float(os.environ.get("EGNN_RANGE_SPIN_SECONDS", "2.0"))   # spinning on the pinned word, then the copy + synchronise fallback
_status = {}


class _Status:
    """Two words per device: [0] is OR-ed by the kernels of a forward, [1] by the kernels of a backward (`backward_status()`), so that
    bits a backward leaves behind are reported as what they are instead of being attributed to -- and re-run as -- the next forward."""

    def __init__(self, device):
        self.dev = torch.zeros(2, dtype=torch.int32, device=device)
        self.host = torch.zeros(2, dtype=torch.int32).pin_memory()
        self.event = None
        # sync mode: the words + a sequence number written by a one-thread kernel into pinned memory the host spins on (egnn_status_publish)
        self.pub = torch.zeros(4, dtype=torch.int32).pin_memory()
        self.pub_np = self.pub.numpy()
        self.seq = 0
        self.lock = threading.Lock()


_status_slot = contextvars.ContextVar("egnn_status_slot", default=0)


@contextlib.contextmanager
def backward_status():
    """Kernels launched inside (the native backward) report range problems in the backward's status word."""
    tok = _status_slot.set(1)
    try:
        yield
    finally:
        _status_slot.reset(tok)


def _status_ptr(device):
    return status_word(device).dev.data_ptr() + 4 * _status_slot.get()


def status_word(device):
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    st = _status.get(key)
    if st is None:
        st = _status[key] = _Status(torch.device("cuda", key))
    return st


def _raise_range(bits, when, origin="call"):
    what = "; ".join(msg for bit, msg in _abi.RANGE_BITS.items() if bits & bit)
    err = _abi.EGNNRangeError(
        f"egnn_pytorch_amd ({when}): a value left the range of the split-fp16 arithmetic of the gfx950 path: {what}. "
        f"The outputs of that call are non-finite. (The reference computes in plain fp32 and has no such limit; rescale the "
        f"inputs / weights, or see DESIGN.md section 2.)")
    err.origin, err.bits = origin, int(bits)
    raise err


class _EarlyPublish:
    """One forward's hand-over between the module entry whose range check follows it (`early_publish`), the one C whole-layer call that
    may publish the status words itself (`status_request`) and `range_check_after_forward`, which then only spins."""
    __slots__ = ("last", "pending")

    def __init__(self):
        self.last = True           # the next EGNN layer call is the last one that can write the status word before the check
        self.pending = None        # (status, sequence number) requested from the C entry; the status's lock is held while set


_early = contextvars.ContextVar("egnn_early_publish", default=None)


def _early_publish_on():
    """EGNN_STATUS_EARLY=0: the status words are published behind the whole forward again (read at every call; A/B and tests)."""
    return os.environ.get("EGNN_STATUS_EARLY", "1") != "0"


@contextlib.contextmanager
def early_publish(last=True):
    """Around a module forward AND the `range_check_after_forward` that follows it: the C whole-layer entry may publish the status words
    from inside the forward, directly behind its last launch that can write them (egnn_forward_opts.status_pub), instead of this
    module publishing them behind the forward's last kernel.  `last`: False while layers that can still write the word follow
    (EGNN_Network sets it in front of its last layer).  A request the check never consumed (an exception in between) is dropped here."""
    ep = _EarlyPublish()
    ep.last = last
    tok = _early.set(ep)
    try:
        yield ep
    finally:
        _early.reset(tok)
        if ep.pending is not None:
            st, ep.pending = ep.pending[0], None
            st.lock.release()


def status_request(device):
    """(pinned words, word count, sequence number) for egnn_forward_opts when THIS call's launches are the last that can write the status
    word before `range_check_after_forward` reads it -- sync mode, spinning on, no stream capture, inside `early_publish` with `last`
    set, the forward's status word current -- else None.  Takes the device's lock: `range_check_after_forward` (or `early_publish`'s
    exit) releases it, so the sequence number and the pinned words stay this thread's from the request to the end of the spin."""
    ep = _early.get()
    if (ep is None or not ep.last or ep.pending is not None or RANGE_CHECK != "sync" or not _SPIN or _status_slot.get() != 0
            or not _early_publish_on() or torch.cuda.is_current_stream_capturing()):
        return None
    st = status_word(device)
    st.lock.acquire()
    st.seq = (st.seq % 0x7ffffff0) + 1
    ep.pending = (st, st.seq)
    return st.pub.data_ptr(), 2, st.seq


def _spin_for(st, seq):
    """Spin on the pinned sequence number (bounded by TIME: a count of Python iterations is seconds on one host and minutes on another);
    (forward word, backward word), or (None, None) past the limit."""
    view, spins = st.pub_np, 0
    deadline = None
    while view[2] != seq:
        spins += 1
        if (spins & 0xFFF) == 0:
            now = time.perf_counter()
            if deadline is None:
                deadline = now + _SPIN_SECONDS
            elif now > deadline:
                break
    if view[2] == seq:
        return int(view[0]), int(view[1])
    return None, None


def range_check_after_forward(device, mode=None):
    """Called by the modules when a forward has been enqueued."""
    mode = mode or RANGE_CHECK
    ep = _early.get()
    pending = None
    if ep is not None and ep.pending is not None:
        pending, ep.pending = ep.pending, None          # (whatever happens below, the lock taken by `status_request` is released once)
    if pending is not None and mode != "sync":          # (requests are made in sync mode only: a mode flipped in between)
        pending[0].lock.release()
        pending = None
    if mode == "off" or torch.cuda.is_current_stream_capturing():      # (graph capture: graphed() checks after each replay)
        if pending is not None:
            pending[0].lock.release()
        return
    st = status_word(device)
    if mode == "sync":
        # the one host synchronisation of the forward: 8 bytes into pinned memory + a stream synchronisation (a .tolist() / .item() goes
        # through a staged pageable copy: slower per forward; a one-thread kernel writing the words into pinned memory for the host to spin
        # on was measured too: no faster -- what the synchronisation costs is the host time from forward() entry to its first launch)
        fwd = bwd = None
        if pending is not None:
            # the C whole-layer entry has published already, behind its last launch that can write the word: nothing to launch, the
            # sequence number requested there is the one to wait for (the lock has been held since that request)
            try:
                if pending[0] is st:
                    fwd, bwd = _spin_for(st, pending[1])
            finally:
                pending[0].lock.release()
        elif _SPIN:
            # publish + spin under the device's lock: the sequence number and the pinned words are per device, and two threads running
            # forwards on one device would overwrite each other's (one of them then spun out its whole limit).  The spin is bounded by
            # TIME (a count of Python iterations is seconds on one host and minutes on another); past it: the copy + synchronise below.
            with st.lock:
                st.seq = (st.seq % 0x7ffffff0) + 1
                with torch.cuda.device(st.dev.device):
                    rc = _abi.load().egnn_status_publish(st.dev.data_ptr(), st.pub.data_ptr(), 2, st.seq, _stream())
                _abi.check(rc, "egnn_status_publish")
                fwd, bwd = _spin_for(st, st.seq)
        if fwd is None:                                 # (EGNN_RANGE_SPIN=0, or the pinned word never changed: copy + synchronise)
            st.host.copy_(st.dev, non_blocking=True)
            torch.cuda.current_stream(st.dev.device).synchronize()
            fwd, bwd = int(st.host[0]), int(st.host[1])
        if fwd or bwd:
            st.dev.zero_()
            st.host.zero_()
        if bwd and not fwd:                             # left by an earlier backward: not this call's, never a reason to re-run it
            _raise_range(bwd, "an earlier backward", origin="backward")
        if fwd:
            _raise_range(fwd | bwd, "this call")
        return
    # deferred: examined by the next call / check_range().  Attribution is relaxed in this mode: the copy runs on the side stream and may
    # overlap the next forward's kernels OR-ing into the word (and check_range()'s zero_() on the launch stream), so a bit set by step
    # n + 1 can be reported with step n, or be reported twice -- the OR is sticky, detection itself is never lost.  The copy is a blit kernel: on the side stream, behind this forward's
    # last kernel, it does not sit between this step and the next one on the launch stream (two launch gaps + 4 us per step)
    cur = torch.cuda.current_stream(st.dev.device)
    side = side_stream(st.dev.device)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        st.host.copy_(st.dev, non_blocking=True)
        st.event = torch.cuda.Event()
        st.event.record(side)


def check_range(device=None, wait=True):
    """Examine the status word of earlier (deferred-mode) forwards; raises EGNNRangeError if a value left the range."""
    if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
        return                                          # event queries are illegal inside a stream capture (graphed())
    for key, st in list(_status.items()):
        if device is not None and torch.device(device).index not in (None, key):
            continue
        if st.event is None:
            continue
        if wait:
            st.event.synchronize()
        elif not st.event.query():
            continue
        bits = int(st.host[0]) | int(st.host[1])
        st.event = None
        if bits:
            st.dev.zero_()
            st.host.zero_()
            _raise_range(bits, "an earlier call", origin="earlier")


def _dtype_suffix(dtype):
    """the suffix of an entry's float32 / float64 twins for tensors of `dtype`"""
    return "_f64" if dtype == torch.float64 else "_f32"


def _knn_outputs(out, coors, *shape):
    """(idx int32, rank in the coordinates' dtype) of a selection, both of `shape`: `out` where the caller allocated them, else new on
    the current stream"""
    if out is not None:
        return out
    return empty(*shape, dtype=torch.int32, device=coors.device), empty(*shape, dtype=coors.dtype, device=coors.device)


def _csr_args(adj, coors):
    """(rowptr, col, graph stride of rowptr) as the CSR entries take them, of a SparseAdjacency checked against (B, N, C) coordinates"""
    b, n = coors.shape[:2]
    if adj.n != n or (adj.batched and adj.num_graphs != b):
        raise ValueError(f"adj_mat shape {tuple(adj.shape)} != {(b, n, n)} or {(n, n)}")
    if adj.device != coors.device:
        raise RuntimeError(f"Expected all tensors to be on the same device: coors is on {coors.device}, adj_mat on {adj.device}")
    return _ptr(adj.rowptr), _ptr(adj.col) if adj.col.numel() else None, 0 if adj.shared else n + 1


def knn_select(coors, mask, adj_mat, k, out=None):
    """(idx int32 (B,N,K), rank (B,N,K) in the coordinates' dtype) -- egnn_knn_select_f32; float64 coordinates (a float64 module):
    egnn_knn_select_f64.  out = (idx, rank): caller-allocated outputs (the side-stream fork allocates them on the launch stream)."""
    if isinstance(adj_mat, SparseAdjacency):
        return knn_select_csr(coors, mask, adj_mat, k, out)
    return _knn_select(coors, mask, adj_mat, k, out, "egnn_knn_select")


def knn_select_csr(coors, mask, adj, k, out=None):
    """knn_select with the adjacency as a SparseAdjacency -- egnn_knn_select_csr_f32 / _f64: the streaming kernel on sorted column ranges
    at every N; the same outputs bit for bit as knn_select with `adj.to_dense()`, without the (N, N) map."""
    b, n, cdim = coors.shape
    csr = _csr_args(adj, coors)
    idx, rank = _knn_outputs(out, coors, b, n, k)
    m8 = _u8(mask)
    name = "egnn_knn_select_csr" + _dtype_suffix(coors.dtype)
    with _timed("knn_select"):
        rc = getattr(_abi.load(), name)(_ptr(coors), _ptr(m8), *csr, b, n, k, cdim, _ptr(idx), _ptr(rank), _stream())
    _abi.check(rc, name)
    return idx, rank


def knn_select_stream(coors, mask, adj_mat, k, out=None):
    """knn_select on the streaming kernel (egnn_knn_select_stream_f32 / _f64) whatever the graph's size: the kernel the two entries
    above take for graphs whose keys do not fit in LDS; the same outputs bit for bit."""
    return _knn_select(coors, mask, adj_mat, k, out, "egnn_knn_select_stream")


# `knn_select_segments`: the most nodes a workgroup's LDS window holds (egnn_knn_segments_lds_nodes); None = the kernel's own budget.
# Segments beyond the window are streamed from memory -- the same result: tests lower it to meet both sources at small sizes.
KNN_SEGMENTS_LDS_NODES = None


def knn_select_segments(coors, segments, k, out=None):
    """(idx int32 (T,K), rank (T,K) in the coordinates' dtype) of a packed batch -- egnn_knn_select_segments_f32 / _f64
    (csrc/knn_segments.hip): row i of graph [lo, hi) gets its min(K, hi - lo) nearest nodes of that graph as rows of the packed batch,
    ascending, ties by ascending index; the slots beyond hold (i, +inf).  coors: (T, C) float32 / float64; segments: a GraphSegments on
    the same device.  out = (idx, rank): caller-allocated outputs."""
    if not isinstance(segments, GraphSegments):
        raise TypeError(f"segments must be a GraphSegments (got {type(segments).__name__})")
    if coors.dim() != 2 or coors.shape[0] != segments.num_nodes:
        raise ValueError(f"coors shape {tuple(coors.shape)}: expected ({segments.num_nodes}, C) for these segments")
    if coors.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"knn_select_segments takes float32 or float64 coordinates (got {coors.dtype})")
    if segments.device != coors.device:
        raise RuntimeError(f"Expected all tensors to be on the same device: coors is on {coors.device}, the segments on {segments.device}")
    t, cdim = coors.shape
    coors = aligned(coors)
    idx, rank = _knn_outputs(out, coors, t, k)
    lib = _abi.load()
    lib.egnn_knn_segments_lds_nodes(int(KNN_SEGMENTS_LDS_NODES or 0))
    name = "egnn_knn_select_segments" + _dtype_suffix(coors.dtype)
    with _timed("knn_select_segments"):
        rc = getattr(lib, name)(_ptr(coors), _ptr(segments.offsets), _ptr(segments.segment_of), segments.num_graphs, t, k, cdim,
                                max(segments.max_size, 1), _ptr(idx), _ptr(rank), _stream())
    _abi.check(rc, name)
    return idx, rank


SEGMENT_OPS = {"sum": 0, "mean": 1, "max": 2, "min": 3}


def _segment_args(x, segments, rows, what):
    """the checks the segment readout wrappers share: a (rows, D) float32 / float64 matrix on the segments' device"""
    if not isinstance(segments, GraphSegments):
        raise TypeError(f"segments must be a GraphSegments (got {type(segments).__name__})")
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what} takes float32 or float64 rows (got {x.dtype})")
    if x.dim() != 2 or x.shape[0] != rows or x.shape[1] < 1:
        raise ValueError(f"{what}: shape {tuple(x.shape)}: expected ({rows}, D) with D >= 1 for these segments")
    if segments.device != x.device:
        raise RuntimeError(f"Expected all tensors to be on the same device: the rows are on {x.device}, the segments on {segments.device}")
    if segments.num_nodes < 1:
        raise ValueError(f"{what}: a packed batch without a node has no kernel to run")
    return _dtype_suffix(x.dtype)


def _segment_rows_in_place(x, d):
    """x (T, d): rows read in place at their pitch; anything else (a transposed view) is copied first"""
    return x if x.stride(1) == 1 and x.stride(0) >= d else x.contiguous()


def _segment_workspace(lib, tab, g, t, d, like):
    if not tab.n_multi:
        return None
    return empty(lib.egnn_segment_reduce_workspace_bytes(g, t, d, like.element_size()), dtype=torch.uint8, device=like.device)


def segment_reduce(x, segments, op="sum"):
    """(T, D) node rows -> (G, D) graph rows -- egnn_segment_reduce_f32 / _f64 (csrc/segment_reduce.hip): op "sum" / "mean" return out,
    "max" / "min" return (out, rows int32 (G, D): the winning row of the packed batch per graph and column).  Fixed order, no atomics;
    the order for a graph depends on its size and D only.  x: float32 / float64; rows at any pitch (a column slice of a wider matrix is
    read in place, 16-byte loads where D, the pitch and the base allow them -- the same bits either way); anything else (a transposed
    view) is copied first."""
    sfx = _segment_args(x, segments, segments.num_nodes, "segment_reduce")
    if op not in SEGMENT_OPS:
        raise ValueError(f"segment_reduce: op = {op!r}: expected one of {tuple(SEGMENT_OPS)}")
    t, d = x.shape
    x = _segment_rows_in_place(x, d)
    g = segments.num_graphs
    tab = segments._reduce_tables()
    out = empty(g, d, dtype=x.dtype, device=x.device)
    rows = empty(g, d, dtype=torch.int32, device=x.device) if SEGMENT_OPS[op] >= 2 else None
    lib = _abi.load()
    ws = _segment_workspace(lib, tab, g, t, d, x)
    name = "egnn_segment_reduce" + sfx
    with _timed("segment_reduce"):
        rc = getattr(lib, name)(_ptr(x), x.stride(0), _ptr(segments.offsets), _ptr(tab.chunk_row), _ptr(tab.chunk_seg), _ptr(tab.chunk_slot),
                                tab.n_chunks, _ptr(tab.multi_seg), _ptr(tab.multi_slot), tab.n_multi, g, t, d, SEGMENT_OPS[op], _ptr(out),
                                _ptr(rows), _ptr(ws), 0 if ws is None else ws.numel(), _stream())
    _abi.check(rc, name)
    return out if rows is None else (out, rows)


def segment_broadcast(g, segments):
    """(G, D) graph rows -> (T, D): every node receives its graph's row -- egnn_segment_broadcast_f32 / _f64"""
    sfx = _segment_args(g, segments, segments.num_graphs, "segment_broadcast")
    g = g.contiguous()
    out = empty(segments.num_nodes, g.shape[1], dtype=g.dtype, device=g.device)
    name = "egnn_segment_broadcast" + sfx
    with _timed("segment_broadcast"):
        rc = getattr(_abi.load(), name)(_ptr(g), _ptr(segments.segment_of), segments.num_graphs, segments.num_nodes, g.shape[1], _ptr(out),
                                        _stream())
    _abi.check(rc, name)
    return out


def _segment_rows(rows, g):
    if rows.dtype != torch.int32 or tuple(rows.shape) != tuple(g) or not rows.is_contiguous():
        raise ValueError(f"rows must be a contiguous int32 {tuple(g)} tensor (got {rows.dtype} {tuple(rows.shape)})")
    return rows


def segment_scatter_rows(g, rows, segments):
    """(G, D) graph rows -> (T, D): g[s, c] at row rows[s, c] of column c, 0 elsewhere (the backward of `segment_reduce`'s max / min:
    one store per element, no atomics) -- egnn_segment_scatter_rows_f32 / _f64"""
    sfx = _segment_args(g, segments, segments.num_graphs, "segment_scatter_rows")
    g = g.contiguous()
    _segment_rows(rows, g.shape)
    out = empty(segments.num_nodes, g.shape[1], dtype=g.dtype, device=g.device)
    name = "egnn_segment_scatter_rows" + sfx
    with _timed("segment_scatter_rows"):
        rc = getattr(_abi.load(), name)(_ptr(g), _ptr(rows), _ptr(segments.segment_of), segments.num_graphs, segments.num_nodes, g.shape[1],
                                        _ptr(out), _stream())
    _abi.check(rc, name)
    return out


def segment_gather_rows(x, rows, segments):
    """(T, D) node rows -> (G, D): x[rows[s, c], c] (the transpose of `segment_scatter_rows`) -- egnn_segment_gather_rows_f32 / _f64"""
    sfx = _segment_args(x, segments, segments.num_nodes, "segment_gather_rows")
    x = x.contiguous()
    _segment_rows(rows, (segments.num_graphs, x.shape[1]))
    out = empty(segments.num_graphs, x.shape[1], dtype=x.dtype, device=x.device)
    name = "egnn_segment_gather_rows" + sfx
    with _timed("segment_gather_rows"):
        rc = getattr(_abi.load(), name)(_ptr(x), _ptr(rows), segments.num_graphs, segments.num_nodes, x.shape[1], _ptr(out), _stream())
    _abi.check(rc, name)
    return out


def _segment_stats_pair(m, l, like, shape, what):
    for name, s in (("m", m), ("l", l)):
        if s.dtype != like.dtype or s.device != like.device or tuple(s.shape) != tuple(shape) or not s.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous {like.dtype} {tuple(shape)} tensor on {like.device} "
                             f"(got {s.dtype} {tuple(s.shape)} on {s.device})")


def segment_softmax_stats(x, segments):
    """(T, D) node rows -> (m, l), both (G, D): the maximum of every graph's column (a NaN wins) and l = sum exp(x - m), added in the
    order of `segment_reduce`'s sum -- egnn_segment_softmax_stats_f32 / _f64 (csrc/segment_softmax.hip).  An empty graph: (-inf, 0).
    Rows at any pitch are read in place (the same bits on the 16-byte and the scalar path); a transposed view is copied first."""
    sfx = _segment_args(x, segments, segments.num_nodes, "segment_softmax_stats")
    t, d = x.shape
    x = _segment_rows_in_place(x, d)
    g = segments.num_graphs
    tab = segments._reduce_tables()
    m, l = empty(g, d, dtype=x.dtype, device=x.device), empty(g, d, dtype=x.dtype, device=x.device)
    lib = _abi.load()
    ws = _segment_workspace(lib, tab, g, t, d, x)
    name = "egnn_segment_softmax_stats" + sfx
    with _timed("segment_softmax_stats"):
        rc = getattr(lib, name)(_ptr(x), x.stride(0), _ptr(segments.offsets), _ptr(tab.chunk_row), _ptr(tab.chunk_seg), _ptr(tab.chunk_slot),
                                tab.n_chunks, _ptr(tab.multi_seg), _ptr(tab.multi_slot), tab.n_multi, g, t, d, _ptr(m), _ptr(l), _ptr(ws),
                                0 if ws is None else ws.numel(), _stream())
    _abi.check(rc, name)
    return m, l


def segment_softmax_apply(x, m, l, segments):
    """(T, D) node rows and the (G, D) statistics of `segment_softmax_stats` -> y (T, D) = exp(x - m[g]) / l[g] --
    egnn_segment_softmax_apply_f32 / _f64"""
    sfx = _segment_args(x, segments, segments.num_nodes, "segment_softmax_apply")
    t, d = x.shape
    _segment_stats_pair(m, l, x, (segments.num_graphs, d), "segment_softmax_apply")
    x = _segment_rows_in_place(x, d)
    y = empty(t, d, dtype=x.dtype, device=x.device)
    name = "egnn_segment_softmax_apply" + sfx
    with _timed("segment_softmax_apply"):
        rc = getattr(_abi.load(), name)(_ptr(x), x.stride(0), _ptr(m), _ptr(l), _ptr(segments.segment_of), segments.num_graphs, t, d, _ptr(y),
                                        _stream())
    _abi.check(rc, name)
    return y


def _segment_pool_args(scores, values, m, l, segments, what):
    """scores (T, H), values (T, H, Dv), m / l (G, H) -> (suffix, scores, values as rows at a pitch, H, Dv)"""
    sfx = _segment_args(scores, segments, segments.num_nodes, what)
    t, h = scores.shape
    if values.dtype != scores.dtype:
        raise TypeError(f"{what}: scores are {scores.dtype}, values {values.dtype}: expected one dtype")
    if values.device != scores.device:
        raise RuntimeError(f"Expected all tensors to be on the same device: scores are on {scores.device}, values on {values.device}")
    if values.dim() != 3 or values.shape[:2] != (t, h) or values.shape[2] < 1:
        raise ValueError(f"{what}: values shape {tuple(values.shape)}: expected ({t}, {h}, Dv) with Dv >= 1 for scores {tuple(scores.shape)}")
    dv = values.shape[2]
    _segment_stats_pair(m, l, scores, (segments.num_graphs, h), what)
    scores = _segment_rows_in_place(scores, h)
    if not (values.stride(2) == 1 and values.stride(1) == dv and values.stride(0) >= h * dv):
        values = values.contiguous()
    return sfx, scores, values, h, dv


def segment_pool(scores, values, m, l, segments):
    """scores (T, H), values (T, H, Dv) and the (G, H) statistics of the scores -> out (G, H, Dv) = sum_i softmax(scores)_i values_i over
    the nodes of every graph -- egnn_segment_pool_f32 / _f64: one pass over `values`, the numerator in the order of `segment_reduce`'s
    sum over the flattened (T, H Dv) matrix, one division by l; neither the weights nor the products are formed in memory."""
    sfx, scores, values, h, dv = _segment_pool_args(scores, values, m, l, segments, "segment_pool")
    g, t = segments.num_graphs, segments.num_nodes
    tab = segments._reduce_tables()
    out = empty(g, h, dv, dtype=values.dtype, device=values.device)
    lib = _abi.load()
    ws = _segment_workspace(lib, tab, g, t, h * dv, values)
    name = "egnn_segment_pool" + sfx
    with _timed("segment_pool"):
        rc = getattr(lib, name)(_ptr(scores), scores.stride(0), _ptr(values), values.stride(0), _ptr(m), _ptr(l), _ptr(segments.offsets),
                                _ptr(tab.chunk_row), _ptr(tab.chunk_seg), _ptr(tab.chunk_slot), tab.n_chunks, _ptr(tab.multi_seg),
                                _ptr(tab.multi_slot), tab.n_multi, g, t, h, dv, _ptr(out), _ptr(ws), 0 if ws is None else ws.numel(),
                                _stream())
    _abi.check(rc, name)
    return out


def segment_pool_bwd(g, out, scores, values, m, l, segments):
    """the first-order backward of `segment_pool`: the cotangent g and the forward's out, both (G, H, Dv) -> (d_scores (T, H),
    d_values (T, H, Dv)) -- egnn_segment_pool_bwd_f32 / _f64: one pass over `values`"""
    sfx, scores, values, h, dv = _segment_pool_args(scores, values, m, l, segments, "segment_pool_bwd")
    shape = (segments.num_graphs, h, dv)
    for name, s in (("g", g), ("out", out)):
        if s.dtype != values.dtype or s.device != values.device or tuple(s.shape) != shape:
            raise ValueError(f"segment_pool_bwd: {name} must be a {values.dtype} {shape} tensor on {values.device} "
                             f"(got {s.dtype} {tuple(s.shape)} on {s.device})")
    g, out = g.contiguous(), out.contiguous()
    t = segments.num_nodes
    d_scores = empty(t, h, dtype=values.dtype, device=values.device)
    d_values = empty(t, h, dv, dtype=values.dtype, device=values.device)
    name = "egnn_segment_pool_bwd" + sfx
    with _timed("segment_pool_bwd"):
        rc = getattr(_abi.load(), name)(_ptr(g), _ptr(out), _ptr(scores), scores.stride(0), _ptr(values), values.stride(0), _ptr(m), _ptr(l),
                                        _ptr(segments.segment_of), segments.num_graphs, t, h, dv, _ptr(d_scores), _ptr(d_values), _stream())
    _abi.check(rc, name)
    return d_scores, d_values


KNN_GRID_KMAX = 128           # the K limit of egnn_knn_select_grid_f32 / _f64 and _grid_csr_f32 / _f64 (csrc/knn_grid.hip: KG_KMAX)


def _grid_suffix(dtype):
    """the entry suffix of the cell-grid selection for coordinates of `dtype`: float32, or float64 (a float64 module)"""
    if dtype not in (torch.float32, torch.float64):
        raise TypeError(f"knn_select_grid takes float32 or float64 coordinates (got {dtype})")
    return _dtype_suffix(dtype)


def knn_grid_workspace(b, n, k, device, dtype=torch.float32):
    """the workspace of `knn_select_grid` for (B, N, K) and coordinates of `dtype`: egnn_knn_grid_workspace_bytes bytes (float64:
    egnn_knn_grid_workspace_bytes_f64 -- its sorted records are twice as wide), allocated on the current stream"""
    query = "egnn_knn_grid_workspace_bytes" + ("_f64" if _grid_suffix(dtype) == "_f64" else "")
    return empty(getattr(_abi.load(), query)(b, n, k), dtype=torch.uint8, device=device)


def knn_select_grid(coors, mask, k, out=None, ws=None, adj=None):
    """knn_select on the cell-grid kernels (egnn_knn_select_grid_f32; float64 coordinates: egnn_knn_select_grid_f64, rank in float64):
    coor_dim == 3, K <= 128; the same outputs bit for bit at a cost per row bounded by its neighbourhood, not by N.  Any other dtype:
    TypeError.  ws: the workspace (`knn_grid_workspace` for the coordinates' dtype), allocated here on the current stream when None
    -- a caller that runs this on a side stream allocates `out` and `ws` on its launch stream.
    adj: None or a SparseAdjacency (egnn_knn_select_grid_csr_f32 / _f64: the outputs of `knn_select_csr`); a dense map has no grid entry."""
    b, n, cdim = coors.shape
    sfx = _grid_suffix(coors.dtype)
    csr = ()
    if adj is not None:
        if not isinstance(adj, SparseAdjacency):
            raise TypeError("knn_select_grid takes the adjacency as a SparseAdjacency (a dense map selects on the all-pairs kernels)")
        csr = _csr_args(adj, coors)
    idx, rank = _knn_outputs(out, coors, b, n, k)
    m8 = _u8(mask)
    if ws is None:
        ws = knn_grid_workspace(b, n, k, coors.device, coors.dtype)
    name = ("egnn_knn_select_grid_csr" if csr else "egnn_knn_select_grid") + sfx
    with _timed("knn_select_grid"):
        rc = getattr(_abi.load(), name)(_ptr(coors), _ptr(m8), *csr, b, n, k, cdim, _ptr(idx), _ptr(rank), _ptr(ws), ws.numel(), _stream())
    _abi.check(rc, name)
    return idx, rank


def _knn_select(coors, mask, adj_mat, k, out, entry):
    b, n, cdim = coors.shape
    idx, rank = _knn_outputs(out, coors, b, n, k)
    m8 = _u8(mask)
    a8 = _u8(adj_mat)
    stride = 0
    if a8 is not None:
        if a8.dim() == 3:
            if a8.shape != (b, n, n):
                raise ValueError(f"adj_mat shape {tuple(a8.shape)} != {(b, n, n)}")
            stride = n * n
        elif a8.shape != (n, n):
            raise ValueError(f"adj_mat shape {tuple(a8.shape)} != {(n, n)}")
    name = entry + _dtype_suffix(coors.dtype)
    with _timed("knn_select"):
        rc = getattr(_abi.load(), name)(_ptr(coors), _ptr(m8), _ptr(a8), stride, b, n, k, cdim, _ptr(idx), _ptr(rank), _stream())
    _abi.check(rc, name)
    return idx, rank


def spatial_order(coors, out=None, mask8=None):
    """(B,N) int32 Morton permutation -- egnn_spatial_order_masked_f32 (scheduling aid for the edge pass; the padded nodes of mask8,
    (B,N) bytes, behind the real ones)."""
    b, n, _ = coors.shape
    order = out if out is not None else empty(b, n, dtype=torch.int32, device=coors.device)
    with _timed("spatial_order"):
        rc = _abi.load().egnn_spatial_order_masked_f32(_ptr(coors), _ptr(mask8), b, n, _ptr(order), _stream())
    _abi.check(rc, "egnn_spatial_order_masked_f32")
    return order


def slot_prep(coors, mask8, idx, rank, order, valid_radius, out=None):
    """(B*N*K, 4) int32 per-slot records {j | pair_ok << 31, x_i - x_j} in the edge pass's consumption order --
    egnn_slot_prep_f32 (flattens the setup's index chain: include/egnn_hip.h).  idx None: the dense all-pairs layer (K = N, j = k)."""
    if idx is None:
        b, n, k = coors.shape[0], coors.shape[1], coors.shape[1]
    else:
        b, n, k = idx.shape
    slots = out if out is not None else empty(b * n * k, 4, dtype=torch.int32, device=coors.device)
    with _timed("slot_prep"):
        rc = _abi.load().egnn_slot_prep_f32(_ptr(coors), _ptr(mask8), _ptr(idx), _ptr(rank), _ptr(order),
                                            float(min(valid_radius, 3.0e38)), b, n, k, _ptr(slots), _stream())
    _abi.check(rc, "egnn_slot_prep_f32")
    return slots


def adj_expand(adj_mat, b, num_adj_degrees):
    """N-degree adjacency expansion (egnn_pytorch.py:414-427) -- egnn_adj_expand_u8.
    Returns (expanded adjacency (B,N,N) bool, adj_indices (B,N,N) uint8)."""
    return _adj_expand(adj_mat, b, num_adj_degrees, "egnn_adj_expand_u8")


def adj_expand_wide(adj_mat, b, num_adj_degrees):
    """adj_expand on the any-N kernel (egnn_adj_expand_wide_u8) whatever the graph's size: the kernel adj_expand takes above 4 096
    nodes; the same outputs bit for bit."""
    return _adj_expand(adj_mat, b, num_adj_degrees, "egnn_adj_expand_wide_u8")


def _adj_expand(adj_mat, b, num_adj_degrees, entry):
    a8 = _u8(adj_mat)
    n = a8.shape[-1]
    stride = n * n if a8.dim() == 3 else 0
    if a8.dim() == 3 and a8.shape[0] != b:
        raise ValueError(f"adj_mat batch {a8.shape[0]} != {b}")
    dev = a8.device
    adj_out = empty(b, n, n, dtype=torch.uint8, device=dev)
    deg = empty(b, n, n, dtype=torch.uint8, device=dev)
    ws = empty(_abi.load().egnn_adj_expand_workspace_bytes(b, n), dtype=torch.uint8, device=dev)
    with _timed("adj_expand"):
        rc = getattr(_abi.load(), entry)(_ptr(a8), stride, b, n, num_adj_degrees, _ptr(adj_out), _ptr(deg), _ptr(ws), _stream())
    _abi.check(rc, entry)
    return adj_out.view(torch.bool), deg


def adj_expand_csr(adj, b, num_adj_degrees, force_global=False):
    """adj_expand on a SparseAdjacency (csrc/adj_csr.hip): (expanded adjacency as a SparseAdjacency, labels as a SparseLabels), whose
    dense images are adj_expand(adj.to_dense(), b, D)'s outputs bit for bit; a shared adjacency (G = 1) stays shared.  Per degree a
    count and a fill call, with ONE device->host read between them (the two totals that size the column arrays): not capturable in a
    HIP graph.  force_global: every row on the kernels' global-memory bit maps (tests)."""
    n, g = adj.n, adj.num_graphs
    if adj.batched and g != b:
        raise ValueError(f"adj_mat batch {g} != {b}")
    dev = adj.device
    labels = SparseLabels(adj.rowptr, adj.col, torch.ones(adj.col.numel(), dtype=torch.uint8, device=dev), n)
    if num_adj_degrees == 1 or n == 0:
        return adj, labels
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("EGNN_Network(num_adj_degrees > 1) with a SparseAdjacency cannot be captured in a HIP graph: the CSR expansion "
                           "reads each degree's entry count back to size the next buffers (expand outside the capture, or pass the "
                           "dense adjacency)")
    lib = _abi.load()
    ws = empty(max(1, lib.egnn_adj_csr_workspace_bytes(g, n)), dtype=torch.uint8, device=dev)
    flags = 1 if force_global else 0
    cur = adj
    for degree in range(2, num_adj_degrees + 1):
        nxt_rp = empty(g, n + 1, dtype=torch.int64, device=dev)
        lab_rp = empty(g, n + 1, dtype=torch.int64, device=dev)
        totals = empty(2, dtype=torch.int64, device=dev)
        with _timed("adj_expand"):
            rc = lib.egnn_adj_csr_square_count(_ptr(cur.rowptr), _ptr(cur.col), _ptr(labels.rowptr), _ptr(labels.col), g, n, _ptr(nxt_rp),
                                               _ptr(lab_rp), _ptr(totals), _ptr(ws), ws.numel(), flags, _stream())
        _abi.check(rc, "egnn_adj_csr_square_count")
        nnz, lnz = totals.tolist()                                  # the one read of this degree
        nxt_col = empty(max(1, min(nnz, 2 ** 31 - 1)), dtype=torch.int32, device=dev)[:nnz]
        lab_col = empty(max(1, min(lnz, 2 ** 31 - 1)), dtype=torch.int32, device=dev)[:lnz]
        lab_val = empty(max(1, min(lnz, 2 ** 31 - 1)), dtype=torch.uint8, device=dev)[:lnz]
        with _timed("adj_expand"):
            rc = lib.egnn_adj_csr_square_fill(_ptr(cur.rowptr), _ptr(cur.col), _ptr(labels.rowptr), _ptr(labels.col), _ptr(labels.val), g, n,
                                              degree, _ptr(nxt_rp), _ptr(nxt_col), nnz, _ptr(lab_rp), _ptr(lab_col), _ptr(lab_val), lnz,
                                              _ptr(ws), ws.numel(), flags, _stream())
        _abi.check(rc, "egnn_adj_csr_square_fill")
        cur = SparseAdjacency(nxt_rp, nxt_col, n, validate=False, batched=adj.batched)
        labels = SparseLabels(lab_rp, lab_col, lab_val, n)
    return cur, labels


def csr_slot_labels(labels, idx, b, n, k):
    """(B,N,K) bytes: the label of every selected pair (i, idx[b,i,k]) (idx None: the dense layer, j = k) from a SparseLabels --
    egnn_csr_slot_labels_u8; what the _slot gather / gradient entries read in place of the (B,N,N) map."""
    if labels.n != n or labels.num_graphs not in (1, b):
        raise ValueError(f"labels for {labels.num_graphs} graphs of {labels.n} nodes, call on {b} graphs of {n}")
    if idx is not None and (idx.dtype != torch.int32 or not idx.is_contiguous() or tuple(idx.shape) != (b, n, k)):
        raise ValueError(f"csr_slot_labels: idx must be a contiguous ({b}, {n}, {k}) int32 tensor (got {tuple(idx.shape)} {idx.dtype})")
    out = empty(b, n, k, dtype=torch.uint8, device=labels.device)
    rc = _abi.load().egnn_csr_slot_labels_u8(_ptr(labels.rowptr), _ptr(labels.col), _ptr(labels.val), 0 if labels.shared else n + 1,
                                             _ptr(idx), b, n, k, _ptr(out), _stream())
    _abi.check(rc, "egnn_csr_slot_labels_u8")
    return out


def adj_max_degree(adj_mat):
    """int(adj_mat.float().sum(-1).max()) -- one device->host read, like the reference's .item() (:249)."""
    if isinstance(adj_mat, SparseAdjacency):
        return adj_mat.max_degree()
    a8 = _u8(adj_mat)
    n = a8.shape[-1]
    rows = a8.numel() // n
    out = torch.empty(1, dtype=torch.int32, device=a8.device)
    rc = _abi.load().egnn_adj_max_degree_u8(_ptr(a8), rows, n, _ptr(out), _stream())
    _abi.check(rc, "egnn_adj_max_degree_u8")
    return int(out.item())


def _kpad(k):
    return (k + 31) // 32 * 32


def _packed_empty(rows, kp, device, zero=False):
    n = (rows + 31) // 32 * 32 * kp
    if zero:
        return torch.zeros(n, dtype=torch.float16, device=device)
    return empty(n, dtype=torch.float16, device=device)


class PackedHL:
    """A (rows, kp) matrix as fp16 (hi, lo) images in the packed tile-major layout (include/egnn_hip.h)."""
    __slots__ = ("hi", "lo", "rows", "kp")

    def __init__(self, hi, lo, rows, kp):
        self.hi, self.lo, self.rows, self.kp = hi, lo, rows, kp

    def dense(self):
        """Row-major fp32 reconstruction hi + lo (tests / debugging)."""
        from ._weights import unpack_tiles
        return (unpack_tiles(self.hi, self.rows, self.kp).float() + unpack_tiles(self.lo, self.rows, self.kp).float())[: self.rows]


def split_f16(x2d):
    """fp32 (rows, cols) -> packed fp16 (hi, lo) pair for egnn_linear_hl_f32 -- egnn_split_f16."""
    rows, cols = x2d.shape
    # a view of rows of a wider matrix goes in by its row stride; any other layout (transposed, expanded, off a 16-byte boundary) as a copy
    ldx = x2d.stride(0) if rows > 1 else cols
    if x2d.stride(1) != 1 or ldx < cols or x2d.data_ptr() % 16 or (ldx != cols and ldx % 4):
        x2d, ldx = aligned(x2d.contiguous()), cols
    kp = _kpad(cols)
    hi = _packed_empty(rows, kp, x2d.device)
    lo = _packed_empty(rows, kp, x2d.device)
    with _timed("split_f16"):
        rc = _abi.load().egnn_split_f16(_ptr(x2d), ldx, rows, cols, _ptr(hi), _ptr(lo), kp, _status_ptr(x2d.device),
                                        _stream())
    _abi.check(rc, "egnn_split_f16")
    return PackedHL(hi, lo, rows, kp)


def linear_hl(a: "PackedHL", wsplit, n, bias=None, residual=None, act=0, out_f32=True, out_hl=False, name="linear",
              split_cols=0, drop=None, row_mask=None):
    """act(A @ W.T + bias) (+ residual) with pre-split packed fp16 (hi, lo) operands -- egnn_linear_hl_f32.
    Returns fp32 C, or a PackedHL (padded to 32 columns for the next GEMM) when out_hl, or both.
    split_cols: columns [0, split_cols) of C hold (fp16 hi, fp16 lo) words instead of fp32 values.
    row_mask: (M,) bytes -- M-tiles without a set row are skipped, their rows of C stay unwritten (egnn_linear_hl_lda_rows_f32: the
    projection table of a padded batch, inference only)."""
    whi, wlo, inv, w_rows = wsplit
    m, kp = a.rows, a.kp
    kp_a = 0
    if whi.numel() != w_rows * kp:
        # the A image is wider than the contraction: the product runs over its first kp columns (egnn_linear_hl_lda_f32 -- the
        # projection reads feats out of the [feats | m_i] image of node_mlp's input)
        kp_a, kp = kp, whi.numel() // w_rows
        assert kp < kp_a and kp % 32 == 0 and drop is None
    assert whi.numel() == w_rows * kp and w_rows >= n
    dev = a.hi.device
    c = empty(m, n, dtype=torch.float32, device=dev) if out_f32 else None
    out = None
    kp_out = 0
    if out_hl:
        kp_out = _kpad(n)
        zero = kp_out != n                                   # pad columns must read as zero in the next GEMM
        out = PackedHL(_packed_empty(m, kp_out, dev, zero), _packed_empty(m, kp_out, dev, zero), m, kp_out)
    ldr = 0
    if residual is not None:
        assert residual.shape == (m, n) and residual.is_contiguous()
        ldr = n
    with _timed(name):
        if row_mask is not None:
            assert drop is None and row_mask.numel() == m and row_mask.is_contiguous()
            rc = _abi.load().egnn_linear_hl_lda_rows_f32(_ptr(a.hi), _ptr(a.lo), kp_a, _ptr(whi), _ptr(wlo), float(inv), _ptr(bias),
                                                         _ptr(residual), ldr, _ptr(c), n, _ptr(out.hi) if out else None,
                                                         _ptr(out.lo) if out else None, kp_out, m, n, kp, w_rows, act, int(split_cols),
                                                         _ptr(row_mask), _status_ptr(dev), _stream())
        elif kp_a:
            rc = _abi.load().egnn_linear_hl_lda_f32(_ptr(a.hi), _ptr(a.lo), kp_a, _ptr(whi), _ptr(wlo), float(inv), _ptr(bias),
                                                    _ptr(residual), ldr, _ptr(c), n, _ptr(out.hi) if out else None,
                                                    _ptr(out.lo) if out else None, kp_out, m, n, kp, w_rows, act, int(split_cols),
                                                    _status_ptr(dev), _stream())
        elif drop is None:
            rc = _abi.load().egnn_linear_hl_f32(_ptr(a.hi), _ptr(a.lo), _ptr(whi), _ptr(wlo), float(inv), _ptr(bias),
                                                _ptr(residual), ldr, _ptr(c), n, _ptr(out.hi) if out else None,
                                                _ptr(out.lo) if out else None, kp_out, m, n, kp, w_rows, act, int(split_cols),
                                                _status_ptr(dev), _stream())
        else:                                               # (p, seed): nn.Dropout between the Linear and its activation
            from . import _dropout
            p_drop, seed = drop
            rc = _abi.load().egnn_linear_hl_drop_f32(_ptr(a.hi), _ptr(a.lo), _ptr(whi), _ptr(wlo), float(inv), _ptr(bias),
                                                     _ptr(residual), ldr, _ptr(c), n, _ptr(out.hi) if out else None,
                                                     _ptr(out.lo) if out else None, kp_out, m, n, kp, w_rows, act, int(split_cols),
                                                     _dropout.threshold(p_drop), int(seed), _dropout.inv_keep(p_drop),
                                                     _status_ptr(dev), _stream())
    _abi.check(rc, "egnn_linear_hl_f32")
    if out_f32 and out_hl:
        return c, out
    return out if out_hl else c


def node_mlp_fused_supported(dim, m_dim):
    """egnn_node_mlp_fused_f32 is built for this layer width (m_dim = 16, dim in {32, 64, 128, 256})."""
    return _abi.load().egnn_node_mlp_fused_halves(int(dim), int(m_dim)) > 0


def node_mlp_fused_image(w5_split, w6_split, dim, m_dim):
    """The fused kernel's weight image (fp16 tensor) from the two packed (hi, lo) weight images of egnn_linear_hl_f32."""
    lib = _abi.load()
    n = lib.egnn_node_mlp_fused_halves(int(dim), int(m_dim))
    assert n > 0
    img = empty(n, dtype=torch.float16, device=w5_split[0].device)
    rc = lib.egnn_node_mlp_fused_pack_f16(_ptr(w5_split[0]), _ptr(w5_split[1]), _ptr(w6_split[0]), _ptr(w6_split[1]), int(dim), int(m_dim),
                                          _ptr(img), _stream())
    _abi.check(rc, "egnn_node_mlp_fused_pack_f16")
    return img


def node_mlp_fused(node_in: "PackedHL", image, w5_inv, b5, w6_inv, b6, residual, dim, m_dim):
    """W6 SiLU(W5 [LayerNorm(h) | m_i] + b5) + b6 + residual in one launch (egnn_node_mlp_fused_f32): (rows, dim) fp32."""
    m = node_in.rows
    assert residual.shape == (m, dim) and residual.is_contiguous() and node_in.kp == _kpad(dim + m_dim)
    out = empty(m, dim, dtype=torch.float32, device=residual.device)
    with _timed("node_mlp"):
        rc = _abi.load().egnn_node_mlp_fused_f32(_ptr(node_in.hi), _ptr(node_in.lo), _ptr(image), float(w5_inv), _ptr(b5), float(w6_inv),
                                                 _ptr(b6), _ptr(residual), _ptr(out), m, int(dim), int(m_dim),
                                                 _status_ptr(residual.device), _stream())
    _abi.check(rc, "egnn_node_mlp_fused_f32")
    return out


# ---- the wide-range path: the same layer in plain fp32 (include/egnn_hip.h, "The wide-range path")
def linear_f32(a, w, n, k, bias=None, residual=None, act=0, out=None, name="linear_f32"):
    """act(a @ w[:n, :k].T + bias) (+ residual) in exact fp32 (v_mfma_f32_32x32x2_f32) -- egnn_linear_f32.  a (M, >= k) and w
    (>= n rows, row stride w.stride(0)) may be column slices of wider tensors (unit column stride); `out` likewise (M, >= n)."""
    m = a.shape[0]
    assert a.stride(1) == 1 and w.stride(1) == 1 and a.dtype == w.dtype and a.dtype in (torch.float32, torch.float64)
    f64 = a.dtype == torch.float64                   # (a float64 module: egnn_linear_f64, v_mfma_f64_16x16x4_f64)
    if out is None:
        out = empty(m, n, dtype=a.dtype, device=a.device)
    assert out.stride(1) == 1 and out.shape[0] == m
    ld = lambda t, width: t.stride(0) if t.shape[0] > 1 else max(t.stride(0), width)      # noqa: E731  (a one-row matrix may carry any stride)
    ldr = 0
    if residual is not None:
        assert residual.stride(1) == 1 and residual.shape[0] == m
        ldr = ld(residual, n)
    with _timed(name):
        fn = _abi.load().egnn_linear_f64 if f64 else _abi.load().egnn_linear_f32
        rc = fn(_ptr(a), ld(a, k), _ptr(w), ld(w, k), _ptr(bias), _ptr(residual), ldr, _ptr(out), ld(out, n), m, n, k, act, _stream())
    _abi.check(rc, "egnn_linear_f64" if f64 else "egnn_linear_f32")
    return out


def node_prep_f32(feats2d, m_i, gamma, beta, eps, m_dim):
    """[LayerNorm(feats) | m_i] as a plain (rows, dim + m_dim) matrix in feats2d's dtype -- egnn_node_prep_f32 / egnn_node_prep_f64."""
    rows, dim = feats2d.shape
    out = empty(rows, dim + m_dim, dtype=feats2d.dtype, device=feats2d.device)
    with _timed("node_prep_f32"):
        fn = _abi.load().egnn_node_prep_f64 if feats2d.dtype == torch.float64 else _abi.load().egnn_node_prep_f32
        rc = fn(_ptr(feats2d), _ptr(m_i), _ptr(gamma), _ptr(beta), float(eps), _ptr(out), rows, dim, m_dim, _stream())
    _abi.check(rc, "egnn_node_prep_f32")
    return out


def edge_exact(args: "_abi.EdgeExactArgs", device, dtype=torch.float32):
    """egnn_edge_exact_f32 / egnn_edge_exact_f64 (dtype: what the data pointers of args hold); allocates the per-edge workspace the
    entry asks for."""
    lib = _abi.load()
    nbytes = lib.egnn_edge_exact_workspace_bytes(args.B, args.N, args.K, args.m_dim, args.coor_dim)
    ws = empty(max(1, nbytes // 4), dtype=dtype, device=device)
    args.edge_ws = ws.data_ptr()
    with _timed("edge_exact"):
        rc = (lib.egnn_edge_exact_f64 if dtype == torch.float64 else lib.egnn_edge_exact_f32)(byref(args), _stream())
    _abi.check(rc, "egnn_edge_exact_f64" if dtype == torch.float64 else "egnn_edge_exact_f32")
    return ws


def set_drop(args, drop, eid0=0):
    """drop = (p, seed) -> the drop_* fields of an argument block of the plain kernels (None: no dropout)"""
    if drop is not None:
        from . import _dropout
        args.drop_thr, args.drop_seed, args.drop_inv_keep, args.drop_eid0 = (_dropout.threshold(drop[0]), int(drop[1]),
                                                                             _dropout.inv_keep(drop[0]), int(eid0))


def drop_silu_(z, drop, row0=0):
    """z (rows, cols) <- SiLU(dropout(z)) in place (egnn_drop_silu_f32 / _f64): nn.Dropout between node_mlp's first Linear and its SiLU on
    the plain kernels, the mask = the kernels' hash of node rows row0 .. (drop = (p, seed); None: plain SiLU)."""
    from . import _dropout
    assert z.dim() == 2 and z.stride(1) == 1 and z.dtype in (torch.float32, torch.float64)
    lib = _abi.load()
    thr, seed, inv = (0, 0, 1.0) if drop is None else (_dropout.threshold(drop[0]), int(drop[1]), _dropout.inv_keep(drop[0]))
    with _timed("drop_silu"):
        rc = (lib.egnn_drop_silu_f64 if z.dtype == torch.float64 else lib.egnn_drop_silu_f32)(_ptr(z), z.stride(0) if z.shape[0] > 1 else z.shape[1],
                                                                                            z.shape[0], z.shape[1], thr, seed, inv, int(row0), _stream())
    _abi.check(rc, "egnn_drop_silu")
    return z


def edge_exact_bwd(args: "_abi.EdgeExactBwdArgs", dtype):
    """egnn_edge_exact_bwd_f32 / _f64: a^T, dz^T (H, E) and d/d scalars (E, S) of a chunk of graphs (include/egnn_hip.h)."""
    lib = _abi.load()
    f64 = dtype == torch.float64
    with _timed("edge_exact_bwd"):
        rc = (lib.egnn_edge_exact_bwd_f64 if f64 else lib.egnn_edge_exact_bwd_f32)(byref(args), _stream())
    _abi.check(rc, "egnn_edge_exact_bwd_f64" if f64 else "egnn_edge_exact_bwd_f32")


def edge_hidden(which, args: "_abi.EdgeHiddenArgs", dtype):
    """egnn_edge_hidden_{fwd, bwd, bwd2}_f32 / _f64 (include/egnn_hip.h): the E x H block of the layer -- forward, first-order and
    second-order backward -- for one chunk of graphs; dtype = what the data pointers of args hold."""
    name = f"egnn_edge_hidden_{which}_{'f64' if dtype == torch.float64 else 'f32'}"
    with _timed("edge_hidden_" + which):
        rc = getattr(_abi.load(), name)(byref(args), _stream())
    _abi.check(rc, name)


def edge_exact_node_sums(dz_t, nodes, k, order, seg):
    """egnn_edge_exact_node_sums_*: (d/d P_i, its transpose, d/d P_j, its transpose) -- (nodes, H), (H, nodes) twice -- from dz^T (H, E):
    the K edges leaving a node and the edges arriving at it (CSR lists of egnn_dest_lists_i32), summed in a fixed order."""
    h, e = dz_t.shape
    f64 = dz_t.dtype == torch.float64
    gpi, gpj = (empty(nodes, h, dtype=dz_t.dtype, device=dz_t.device) for _ in range(2))
    gpi_t, gpj_t = (empty(h, nodes, dtype=dz_t.dtype, device=dz_t.device) for _ in range(2))
    lib = _abi.load()
    with _timed("edge_exact_node_sums"):
        rc = (lib.egnn_edge_exact_node_sums_f64 if f64 else lib.egnn_edge_exact_node_sums_f32)(
            _ptr(dz_t), e, h, nodes, k, _ptr(order), _ptr(seg), _ptr(gpi), _ptr(gpi_t), _ptr(gpj), _ptr(gpj_t), _stream())
    _abi.check(rc, "egnn_edge_exact_node_sums")
    return gpi, gpi_t, gpj, gpj_t


def edge_tail_exact(u, coors, idx32, pair_mask, g_coors_out, g_msum, w3, b3, w4, b4, scale, eps, clamp, gate, b, n, k, drop=None, eid0=0):
    """egnn_edge_tail_exact_bwd_f32 / _f64: the per-edge chain behind u in closed form for any head width <= 64 / coordinate dimension,
    in u's dtype.  u (E, m); coors (B, N, C); g_coors_out (B N, C); g_msum (B N, m) or None; w3 .. b4 = coors_mlp's tensors or None
    (update_coors=False); scale = coors_norm.scale or None; gate = (weight (m), bias (1)) or None.  Returns a dict: gU (E, m), g_rel_t
    (C, E) -- transposed: its per-node sums come from egnn_edge_exact_node_sums_* -- and the transposed operands of the parameter
    gradients ghid_t, a3_t (4m, E), mm_t, m0_t (m, E), g_w, g_scale, g_gate (E).  drop = (p, seed), eid0: training-mode dropout in
    coors_mlp -- the forward's hash mask of edge rows eid0 .. re-evaluated."""
    e, m = u.shape
    dt, dev = u.dtype, u.device
    cdim = coors.shape[-1]
    a = _abi.EdgeTailExactArgs()
    a.B, a.N, a.K, a.m_dim, a.coor_dim, a.norm_coors = b, n, k, m, cdim, int(scale is not None)
    a.eps, a.clamp = float(eps), -1.0 if clamp is None else float(clamp)
    out = dict(gU=empty(e, m, dtype=dt, device=dev), g_rel_t=empty(cdim, e, dtype=dt, device=dev), mm_t=empty(m, e, dtype=dt, device=dev))
    keep = [t.contiguous() for t in (u, coors, g_coors_out)]
    a.u, a.coors, a.g_coors_out = (t.data_ptr() for t in keep)
    a.idx, a.pair_mask = _ptr(idx32), _ptr(pair_mask)
    if g_msum is not None:
        keep.append(g_msum.contiguous())
        a.g_msum = keep[-1].data_ptr()
    if w3 is not None:
        keep += [t.detach().to(dt).contiguous() for t in (w3, b3, w4.reshape(-1), b4.reshape(-1))]
        a.W3, a.b3, a.W4, a.b4 = (t.data_ptr() for t in keep[-4:])
        out.update(ghid_t=empty(4 * m, e, dtype=dt, device=dev), a3_t=empty(4 * m, e, dtype=dt, device=dev), g_w=empty(e, dtype=dt, device=dev))
        a.ghid_t, a.a3_t, a.g_w = out["ghid_t"].data_ptr(), out["a3_t"].data_ptr(), out["g_w"].data_ptr()
        if scale is not None:
            keep.append(scale.detach().to(dt).contiguous())
            a.scale = keep[-1].data_ptr()
            out["g_scale"] = empty(e, dtype=dt, device=dev)
            a.g_scale = out["g_scale"].data_ptr()
    else:
        a.norm_coors = 0
    if gate is not None:
        keep += [gate[0].detach().to(dt).reshape(-1).contiguous(), gate[1].detach().to(dt).reshape(-1).contiguous()]
        a.gate_w, a.gate_b = keep[-2].data_ptr(), keep[-1].data_ptr()
        out.update(m0_t=empty(m, e, dtype=dt, device=dev), g_gate=empty(e, dtype=dt, device=dev))
        a.m0_t, a.g_gate = out["m0_t"].data_ptr(), out["g_gate"].data_ptr()
    a.gU, a.g_rel, a.mm_t = out["gU"].data_ptr(), out["g_rel_t"].data_ptr(), out["mm_t"].data_ptr()
    if drop is not None:
        from . import _dropout
        a.drop_thr, a.drop_seed, a.drop_inv_keep, a.drop_eid0 = _dropout.threshold(drop[0]), int(drop[1]), _dropout.inv_keep(drop[0]), int(eid0)
    lib = _abi.load()
    f64 = dt == torch.float64
    with _timed("edge_tail_exact"):
        rc = (lib.egnn_edge_tail_exact_bwd_f64 if f64 else lib.egnn_edge_tail_exact_bwd_f32)(byref(a), _stream())
    _abi.check(rc, "egnn_edge_tail_exact_bwd")
    return out


def node_prep_hl(feats2d, m_i, gamma, beta, eps, m_dim, with_raw=False):
    """[LayerNorm(feats) | m_i] as a packed fp16 (hi, lo) pair -- egnn_node_prep_hl.  m_i None: those columns are
    zero (the edge pass writes them in place).  with_raw: also return feats itself as a packed pair (the projection's
    A operand), produced in the same pass."""
    rows, dim = feats2d.shape
    feats2d, m_i = aligned(feats2d), aligned(m_i)            # (the entry reads rows of `dim` floats: a strided view goes in as a copy)
    kp = _kpad(dim + m_dim)
    hi = _packed_empty(rows, kp, feats2d.device)
    lo = _packed_empty(rows, kp, feats2d.device)
    raw = None
    if with_raw:
        rkp = _kpad(dim)
        raw = PackedHL(_packed_empty(rows, rkp, feats2d.device), _packed_empty(rows, rkp, feats2d.device), rows, rkp)
    with _timed("node_prep"):
        rc = _abi.load().egnn_node_prep_hl(_ptr(feats2d), _ptr(m_i), _ptr(gamma), _ptr(beta), float(eps), _ptr(hi), _ptr(lo),
                                           kp, _ptr(raw.hi) if raw else None, _ptr(raw.lo) if raw else None,
                                           raw.kp if raw else 0, rows, dim, m_dim, _status_ptr(feats2d.device),
                                           _stream())
    _abi.check(rc, "egnn_node_prep_hl")
    out = PackedHL(hi, lo, rows, kp)
    return (out, raw) if with_raw else out


def edge_fused(args: _abi.EdgeArgs, device):
    args.status = _status_ptr(device)
    with _timed("edge_fused"):
        rc = _abi.load().egnn_edge_fused_f32(byref(args), _stream())
    _abi.check(rc, "egnn_edge_fused_f32")


def _lookup_dtype(lookup, what):
    """The one dtype of an EdgeLookup's detached tables (float32 or float64): which of the _f32 / _f64 entries reads them."""
    dts = {t.dtype for t in (lookup.edges, lookup.tok_emb, lookup.deg_emb) if t is not None}
    if len(dts) != 1 or not dts <= {torch.float32, torch.float64}:
        raise TypeError(f"{what}: the look-up tables must all be float32 or all float64 (got {sorted(str(d) for d in dts)})")
    return dts.pop()


def _deg_labels(deg, idx, b, n, k):
    """(label bytes, entry infix) of an EdgeLookup's degree labels: the (B,N,N) map itself, or -- a SparseLabels -- the (B,N,K) labels of
    the selected pairs and the _slot entries that read them"""
    if isinstance(deg, SparseLabels):
        return csr_slot_labels(deg, idx, b, n, k), "_slot"
    return deg, ""


def _slot_deg_labels(deg, idx, b, n, k):
    """(B,N,K) label bytes of the selected pairs, what the _csr entries read: from a SparseLabels (egnn_csr_slot_labels_u8) or from the
    (B,N,N) map a dense adjacency was expanded to (a byte gather; the dense layer's slots are the map itself)"""
    if deg is None:
        return None
    if isinstance(deg, SparseLabels):
        return csr_slot_labels(deg, idx, b, n, k)
    return deg if idx is None else deg.reshape(b * n, n).gather(1, idx.reshape(b * n, k).long()).view(b, n, k)


def _csr_checked(lookup, what, idx, b, n, k):
    csr = lookup.csr
    if csr.num_graphs != b or csr.n != n:
        raise ValueError(f"{what}: SparseEdges for {csr.num_graphs} graphs of {csr.n} nodes, call on {b} graphs of {n} "
                         "(a SparseEdges is per graph: its graph count must equal the batch size)")
    if idx is not None and (idx.dtype != torch.int32 or not idx.is_contiguous() or tuple(idx.shape) != (b, n, k)):
        raise ValueError(f"{what}: idx must be a contiguous ({b}, {n}, {k}) int32 tensor")
    if idx is None and k != n:
        raise ValueError(f"{what}: the dense layer has K = N (got K = {k}, N = {n})")
    return csr


def _csr_first_table(lookup):
    """(values, tokens) of a CSR first table as the entries take them: one of the two, never an empty tensor (whose pointer is NULL) --
    a SparseEdges without entries gets one row that no position refers to"""
    vals, tok = lookup.edges, lookup.tok
    if vals is not None and vals.shape[0] == 0:
        vals = vals.new_zeros(1, lookup.d1)
    if tok is not None and tok.shape[0] == 0:
        tok = tok.new_zeros(1)
    return vals, tok


def edge_features_gather(lookup, idx, b, n, k, with_pos=False):
    """(B,N,K,edge_dim) features of the selected pairs from EGNN_Network's look-up tables, in the tables' dtype --
    egnn_edge_features_gather_f32 / _f64.  A look-up whose first table is a SparseEdges (`lookup.csr`): egnn_edge_features_gather_csr_f32 /
    _f64, which also finds `pos` (B,N,K) int32, every selected pair's offset into the CSR or -1 -- returned too when `with_pos` (the
    gradient entry and the second-order path read it)."""
    dtype = _lookup_dtype(lookup, "edge_features_gather")
    if getattr(lookup, "csr", None) is not None:
        csr = _csr_checked(lookup, "edge_features_gather", idx, b, n, k)
        dev = csr.device
        name = "egnn_edge_features_gather_csr" + ("_f64" if dtype == torch.float64 else "_f32")
        deg = _slot_deg_labels(lookup.deg, idx, b, n, k)
        out = empty(b, n, k, lookup.width, dtype=dtype, device=dev)
        pos = empty(b, n, k, dtype=torch.int32, device=dev)
        vals, tok = _csr_first_table(lookup)
        with _timed("edge_features"):
            rc = getattr(_abi.load(), name)(_ptr(csr.rowptr), _ptr(csr.col), _ptr(vals), _ptr(tok), _ptr(lookup.tok_emb),
                                            lookup.d1, _ptr(deg), _ptr(lookup.deg_emb), lookup.d2, _ptr(idx), b, n, k, _ptr(pos),
                                            _ptr(out), _stream())
        _abi.check(rc, name)
        return (out, pos) if with_pos else out
    if with_pos:
        raise ValueError("edge_features_gather: positions exist for a SparseEdges first table only")
    dev = (lookup.deg if lookup.deg is not None else (lookup.tok if lookup.tok is not None else lookup.edges)).device
    deg, slot = _deg_labels(lookup.deg, idx, b, n, k)
    name = "egnn_edge_features_gather" + slot + ("_f64" if dtype == torch.float64 else "_f32")
    out = empty(b, n, k, lookup.width, dtype=dtype, device=dev)
    with _timed("edge_features"):
        rc = getattr(_abi.load(), name)(_ptr(lookup.edges), _ptr(lookup.tok), _ptr(lookup.tok_emb), lookup.d1,
                                        _ptr(deg), _ptr(lookup.deg_emb), lookup.d2, _ptr(idx), b, n, k,
                                        _ptr(out), _stream())
    _abi.check(rc, name)
    return out


def _edge_features_grad_csr(lookup, idx, b, n, k, g, dtype, on1, on2, g_values, pos):
    """`edge_features_grad` for a SparseEdges first table: egnn_edge_features_grad_csr_f32 / _f64"""
    dev = g.device
    csr = _csr_checked(lookup, "edge_features_grad", idx, b, n, k)
    if pos is None:
        pos = edge_features_gather(lookup, idx, b, n, k, with_pos=True)[1]
    if pos.dtype != torch.int32 or not pos.is_contiguous() or tuple(pos.shape) != (b, n, k):
        raise ValueError(f"edge_features_grad: pos must be a contiguous ({b}, {n}, {k}) int32 tensor")
    if g_values is not None and (lookup.tok is not None or g_values.dtype != dtype or not g_values.is_contiguous()
                                 or tuple(g_values.shape) != (csr.col.numel(), lookup.d1)):
        raise ValueError(f"edge_features_grad: g_values must be a contiguous (nnz, d1) {dtype} tensor for float SparseEdges values")
    name = "egnn_edge_features_grad_csr" + ("_f64" if dtype == torch.float64 else "_f32")
    deg = _slot_deg_labels(lookup.deg, idx, b, n, k) if on2 else None
    v1 = lookup.tok_emb.shape[0] if on1 else 0
    v2 = lookup.deg_emb.shape[0] if on2 else 0
    g_tok = empty(v1, lookup.d1, dtype=dtype, device=dev) if on1 else None
    g_deg = empty(v2, lookup.d2, dtype=dtype, device=dev) if on2 else None
    entry = getattr(_abi.load(), name)
    args = (_ptr(g), g.stride(0), _ptr(pos), _ptr(_csr_first_table(lookup)[1]) if on1 else None, v1, lookup.d1, _ptr(deg), v2,
            lookup.d2, _ptr(idx), b, n, k, _ptr(g_tok), _ptr(g_deg), _ptr(g_values))
    nw = c_int64(0)
    _abi.check(entry(*args, None, byref(nw), _stream()), name)
    work = empty(max(1, nw.value), dtype=dtype, device=dev)
    nw = c_int64(work.numel())
    with _timed("edge_features_grad"):
        rc = entry(*args, _ptr(work), byref(nw), _stream())
    _abi.check(rc, name)
    return g_tok, g_deg


def edge_features_grad(lookup, idx, b, n, k, g, want_tok=True, want_deg=True, g_edges=None, pos=None):
    """The transpose of `edge_features_gather` -- egnn_edge_features_grad_f32 / _f64: g (B N K, >= edge_dim) rows in the tables' dtype
    whose first lookup.width columns are d loss / d the gathered features (row stride g.stride(0)) -> (g_tok_emb (V1, d1) or None,
    g_deg_emb (V2, d2) or None) in that dtype, sums in a fixed order.  g_edges: a zeroed (B,N,N,d1) tensor of that dtype for dense
    float edges, which receives its rows in place.  lookup's label tensors are read for graphs [0, b): pass a lookup sliced to the
    graphs of g.  A SparseEdges first table (`lookup.csr`): g_edges is the zeroed (nnz, d1) gradient of its float values -- the whole
    one, whichever graphs the call covers: the offsets are absolute -- and pos (B,N,K) the positions `edge_features_gather` returned
    for these graphs (None: looked up again)."""
    dev = g.device
    if g.dim() != 2 or g.stride(1) != 1 or g.shape[0] != b * n * k or g.shape[1] < lookup.width:
        raise ValueError(f"edge_features_grad: g {tuple(g.shape)} / strides {g.stride()} for {b * n * k} edges of width {lookup.width}")
    dtype = _lookup_dtype(lookup, "edge_features_grad")
    if g.dtype != dtype:
        raise TypeError(f"edge_features_grad: g must be float32 or float64, matching the tables (g is {g.dtype}, the tables {dtype})")
    on1 = want_tok and lookup.tok is not None
    on2 = want_deg and lookup.deg is not None
    if getattr(lookup, "csr", None) is not None:
        return _edge_features_grad_csr(lookup, idx, b, n, k, g, dtype, on1, on2, g_edges, pos)
    deg, slot = _deg_labels(lookup.deg, idx, b, n, k) if on2 else (None, "_slot" if isinstance(lookup.deg, SparseLabels) else "")
    name = "egnn_edge_features_grad" + slot + ("_f64" if dtype == torch.float64 else "_f32")
    v1 = lookup.tok_emb.shape[0] if on1 else 0
    v2 = lookup.deg_emb.shape[0] if on2 else 0
    g_tok = empty(v1, lookup.d1, dtype=dtype, device=dev) if on1 else None
    g_deg = empty(v2, lookup.d2, dtype=dtype, device=dev) if on2 else None
    if g_edges is not None and (g_edges.dtype != dtype or not g_edges.is_contiguous()
                                or tuple(g_edges.shape) != (b, n, n, lookup.d1)):
        raise ValueError(f"edge_features_grad: g_edges must be a contiguous (B,N,N,d1) {dtype} tensor")
    if idx is not None and (idx.dtype != torch.int32 or not idx.is_contiguous() or tuple(idx.shape) != (b, n, k)):
        raise ValueError(f"edge_features_grad: idx must be a contiguous ({b}, {n}, {k}) int32 tensor")
    for lab in ((lookup.tok,) if on1 else ()) + ((deg,) if on2 else ()):
        if not lab.is_contiguous() or tuple(lab.shape) != ((b, n, k) if (slot and lab is deg) else (b, n, n)):
            raise ValueError(f"edge_features_grad: labels {tuple(lab.shape)} != {(b, n, n)}")
    entry = getattr(_abi.load(), name)
    args = (_ptr(g), g.stride(0), _ptr(lookup.tok) if on1 else None, v1, lookup.d1, _ptr(deg) if on2 else None, v2,
            lookup.d2, _ptr(idx), b, n, k, _ptr(g_tok), _ptr(g_deg), _ptr(g_edges))
    nw = c_int64(0)
    _abi.check(entry(*args, None, byref(nw), _stream()), name)
    work = empty(max(1, nw.value), dtype=dtype, device=dev)
    nw = c_int64(work.numel())
    with _timed("edge_features_grad"):
        rc = entry(*args, _ptr(work), byref(nw), _stream())
    _abi.check(rc, name)
    return g_tok, g_deg


def induced_attn(q, kv, mask, b, n, heads, dim_head, scale):
    """attn1 core of the induced-set attention block: T tokens attend over the nodes -- egnn_induced_attn_f32."""
    t = q.shape[1]
    out = empty(b, t, heads * dim_head, dtype=torch.float32, device=kv.device)
    with _timed("induced_attn"):
        rc = _abi.load().egnn_induced_attn_f32(_ptr(q.contiguous()), _ptr(kv), kv.stride(0), _ptr(_u8(mask)), b, n, t, heads, dim_head,
                                               float(scale), _ptr(out), _stream())
    _abi.check(rc, "egnn_induced_attn_f32")
    return out


def token_attn(q, kv_tok, b, n, heads, dim_head, scale):
    """attn2 core: every node attends over the T induced tokens -- egnn_token_attn_f32."""
    t = kv_tok.shape[1]
    out = empty(b * n, heads * dim_head, dtype=torch.float32, device=q.device)
    with _timed("token_attn"):
        rc = _abi.load().egnn_token_attn_f32(_ptr(q), q.stride(0), _ptr(kv_tok.contiguous()), b, n, t, heads, dim_head, float(scale),
                                             _ptr(out), out.stride(0), _stream())
    _abi.check(rc, "egnn_token_attn_f32")
    return out


def induced_attn_bwd(q, kv, mask, o, g_o, b, n, heads, dim_head, scale):
    """Backward of `induced_attn`: (d/d q (B,T,inner), d/d kv (B N, 2 inner)) from the forward's inputs, its output o and
    g_o = d loss / d o -- egnn_induced_attn_bwd_f32 (the nodes in chunks: per-chunk softmax statistics and partial d/d q tables,
    merged in chunk order)."""
    t = q.shape[1]
    inner = heads * dim_head
    g_q = empty(b, t, inner, dtype=torch.float32, device=kv.device)
    g_kv = empty(b * n, 2 * inner, dtype=torch.float32, device=kv.device)
    lib = _abi.load()
    work = empty(int(lib.egnn_induced_attn_bwd_work_floats(b, n, t, heads, dim_head)), dtype=torch.float32, device=kv.device)
    with _timed("induced_attn_bwd"):
        rc = lib.egnn_induced_attn_bwd_f32(_ptr(q.contiguous()), _ptr(kv), kv.stride(0), _ptr(_u8(mask)), _ptr(o.contiguous()),
                                           _ptr(g_o.contiguous()), b, n, t, heads, dim_head, float(scale), _ptr(work), _ptr(g_q), _ptr(g_kv),
                                           _stream())
    _abi.check(rc, "egnn_induced_attn_bwd_f32")
    return g_q, g_kv


def token_attn_bwd(q, kv_tok, g_out, b, n, heads, dim_head, scale):
    """Backward of `token_attn`: (d/d q (B N, inner), d/d kv_tok (B,T,2 inner)) -- egnn_token_attn_bwd_f32 (the sum over a graph's
    nodes: per-chunk partial tables added up in chunk order)."""
    t = kv_tok.shape[1]
    inner = heads * dim_head
    lib = _abi.load()
    g_q = empty(b * n, inner, dtype=torch.float32, device=q.device)
    g_kv = empty(b, t, 2 * inner, dtype=torch.float32, device=q.device)
    parts = empty(int(lib.egnn_token_attn_bwd_chunks(n)), b * t * 2 * inner, dtype=torch.float32, device=q.device)
    g_out = g_out if g_out.stride(-1) == 1 else g_out.contiguous()
    with _timed("token_attn_bwd"):
        rc = lib.egnn_token_attn_bwd_f32(_ptr(q), q.stride(0), _ptr(kv_tok.contiguous()), _ptr(g_out), g_out.stride(0), b, n, t, heads,
                                         dim_head, float(scale), _ptr(g_q), _ptr(parts), _ptr(g_kv), _stream())
    _abi.check(rc, "egnn_token_attn_bwd_f32")
    return g_q, g_kv


def gelu_bwd_(z, g):
    """z <- GELU(z) (exact), g <- g * GELU'(z), in place, one pass (egnn_gelu_bwd_f32).  Returns (z, g, bits) as `silu_bwd_`."""
    bits = torch.empty(2, dtype=torch.int32, device=z.device)
    with _timed("gelu_bwd"):
        rc = _abi.load().egnn_gelu_bwd_f32(_ptr(z), _ptr(g), _ptr(z), _ptr(g), z.numel(), _ptr(bits), _stream())
    _abi.check(rc, "egnn_gelu_bwd_f32")
    return z, g, bits


def layer_norm_bwd(x2d, g2d, gamma, eps, add=None):
    """Backward of LayerNorm over the rows of x2d (rows, dim <= 1024), statistics recomputed from x2d: (d/d x (+ add), d/d gamma,
    d/d beta) -- egnn_layer_norm_bwd_f32 (column sums: one partial row per workgroup, added up in workgroup order)."""
    rows, dim = x2d.shape
    assert x2d.is_contiguous() and g2d.is_contiguous() and g2d.shape == x2d.shape and (add is None or (add.is_contiguous() and add.shape == x2d.shape))
    lib = _abi.load()
    g_x = empty(rows, dim, dtype=torch.float32, device=x2d.device)
    g_gb = empty(2, dim, dtype=torch.float32, device=x2d.device)
    parts = empty(int(lib.egnn_layer_norm_bwd_parts(rows)), 2 * dim, dtype=torch.float32, device=x2d.device)
    with _timed("layer_norm_bwd"):
        rc = lib.egnn_layer_norm_bwd_f32(_ptr(x2d), _ptr(g2d), _ptr(gamma), float(eps), _ptr(add), rows, dim, _ptr(g_x), _ptr(parts),
                                         _ptr(g_gb), _stream())
    _abi.check(rc, "egnn_layer_norm_bwd_f32")
    return g_x, g_gb[0], g_gb[1]


class HostRead:
    """A few words of device memory on their way to the host WITHOUT draining the stream: created right behind the kernel that writes
    them -- a copy to pinned memory and an event behind that copy -- and waited for (`tensor()` / `floats()` / `ints()`) only where the
    values are needed.  The backward chooses its power-of-two scales from max |x| words that its kernels leave behind; read with
    `.tolist()` each of them waited for EVERYTHING queued so far and left the device idle until the host had caught up (eight times per
    training step: profiles/r05_experiments/train_step_timeline.txt).  With the wait pinned to the producing kernel the host goes on
    queueing independent work in between and wakes up while the device is still busy."""

    def __init__(self, t):
        self.dtype = t.dtype
        if t.is_cuda:
            self.buf = torch.empty(t.numel(), dtype=t.dtype, pin_memory=True)
            with torch.cuda.device(t.device):                # (the copy and the event on the tensor's device's current stream)
                self.buf.copy_(t.reshape(-1), non_blocking=True)
                self.ev = torch.cuda.Event()
                self.ev.record(torch.cuda.current_stream(t.device))
        else:
            self.buf, self.ev = t.reshape(-1), None

    def tensor(self):
        if self.ev is not None:
            self.ev.synchronize()
            self.ev = None
        return self.buf

    def floats(self):
        """max-|x| bit patterns (egnn_absmax_f32's contract) as Python floats"""
        t = self.tensor()
        return (t.view(torch.float32) if t.dtype == torch.int32 else t).tolist()

    def ints(self):
        return self.tensor().tolist()


def bits_to_floats(bits):
    """The floats behind a tensor of max-|x| bit patterns (egnn_absmax_f32's contract), in ONE host read (or behind a HostRead)."""
    if isinstance(bits, HostRead):
        return bits.floats()
    return bits.view(torch.float32).tolist()


def rows_gather_sum(rows, order, seg_ptr, n_out, want_amax=False):
    """out[r] = sum of rows[order[p]] over p in [seg_ptr[r], seg_ptr[r+1]), fixed order -- egnn_rows_gather_sum_f32.
    want_amax: returns (out, bits) with bits = a 1-element int32 tensor holding the bit pattern of max |out| (a by-product)."""
    cols = rows.shape[1]
    out = empty(n_out, cols, dtype=torch.float32, device=rows.device)
    bits = torch.empty(1, dtype=torch.int32, device=rows.device) if want_amax else None
    with _timed("rows_gather_sum"):
        rc = _abi.load().egnn_rows_gather_sum_f32(_ptr(rows), rows.stride(0), _ptr(order), _ptr(seg_ptr), n_out, cols, _ptr(out),
                                                  cols, _ptr(bits), _stream())
    _abi.check(rc, "egnn_rows_gather_sum_f32")
    return (out, bits) if want_amax else out


def split_scaled(x2d, scale, transposed=False, w_image=False):
    """packed fp16 (hi, lo) images of scale * x2d (or of its transpose) -- egnn_split_scaled_f16.  w_image: allocate whole 128-row
    tiles (zero filled), as the W operand of egnn_linear_hl_f32 wants."""
    rows, cols = x2d.shape
    img_rows, k_extent = (cols, rows) if transposed else (rows, cols)
    kp = _kpad(k_extent)
    alloc_rows = (img_rows + 127) // 128 * 128 if w_image else img_rows
    hi = _packed_empty(alloc_rows, kp, x2d.device, zero=w_image)
    lo = _packed_empty(alloc_rows, kp, x2d.device, zero=w_image)
    with _timed("split_scaled"):
        rc = _abi.load().egnn_split_scaled_f16(_ptr(x2d), x2d.stride(0), rows, cols, float(scale), int(transposed), _ptr(hi), _ptr(lo), kp,
                                               _status_ptr(x2d.device), _stream())
    _abi.check(rc, "egnn_split_scaled_f16")
    return PackedHL(hi, lo, img_rows, kp), alloc_rows


def split_scaled_both(x2d, scale, colsum=False):
    """(plain image, transposed image) of scale * x2d from one read -- egnn_split_scaled_both_f16.  colsum: also the column sums of
    x2d (cols,), a by-product of the same read: per 64-row block inside the kernel, the blocks added up in fixed order (`sum_rows`)."""
    rows, cols = x2d.shape
    kp, kpt = _kpad(cols), _kpad(rows)
    hi, lo = _packed_empty(rows, kp, x2d.device), _packed_empty(rows, kp, x2d.device)
    hit, lot = _packed_empty(cols, kpt, x2d.device), _packed_empty(cols, kpt, x2d.device)
    lib = _abi.load()
    parts, ld = None, (cols + 3) // 4 * 4
    if colsum:
        parts = empty(int(lib.egnn_split_scaled_colsum_rows(rows, kpt)), ld, dtype=torch.float32, device=x2d.device)
    with _timed("split_scaled"):
        rc = lib.egnn_split_scaled_both_f16(_ptr(x2d), x2d.stride(0), rows, cols, float(scale), _ptr(hi), _ptr(lo), kp,
                                            _ptr(hit), _ptr(lot), kpt, _status_ptr(x2d.device), _ptr(parts), ld, _stream())
    _abi.check(rc, "egnn_split_scaled_both_f16")
    if colsum:
        return PackedHL(hi, lo, rows, kp), PackedHL(hit, lot, cols, kpt), sum_rows(parts, 1.0 / float(scale))[:cols]
    return PackedHL(hi, lo, rows, kp), PackedHL(hit, lot, cols, kpt)


def silu_bwd_(z, g, drop=None, row0=0):
    """z <- SiLU(z), g <- g * SiLU'(z), in place, one pass (egnn_silu_bwd_f32).  Returns (z, g, bits): bits = the bit patterns of
    max |SiLU(z)| and max |g SiLU'(z)| (2-element int32 tensor; bits_to_floats).  drop = (p, seed): training-mode dropout between
    the Linear that produced z (rows, cols) and the SiLU -- the forward's hash mask of rows row0 .. (egnn_silu_bwd_drop_f32)."""
    bits = torch.empty(2, dtype=torch.int32, device=z.device)
    with _timed("silu_bwd"):
        if drop is None:
            rc = _abi.load().egnn_silu_bwd_f32(_ptr(z), _ptr(g), _ptr(z), _ptr(g), z.numel(), _ptr(bits), _stream())
        else:
            from . import _dropout
            rc = _abi.load().egnn_silu_bwd_drop_f32(_ptr(z), _ptr(g), _ptr(z), _ptr(g), z.numel(), _ptr(bits), _dropout.threshold(drop[0]),
                                                    int(drop[1]), _dropout.inv_keep(drop[0]), int(row0), z.shape[-1], _stream())
    _abi.check(rc, "egnn_silu_bwd_f32")
    return z, g, bits


class GradOperand:
    """A gradient matrix g (R, M) prepared once for its two products: .plain = image of s g (the A operand of g @ W), .t = image of
    (s g)^T (the A operand of g^T @ x), .scale = s (a power of two, grad_scale); .zero: g is all zero / not finite."""

    def __init__(self, g2d, amax=None, colsum=False):
        self.shape = g2d.shape
        self.scale = grad_scale(absmax(g2d) if amax is None else amax)
        self.zero = self.scale is None
        self.plain = self.t = self.colsum = None
        if not self.zero and self.scale is not NONFINITE:
            if colsum:                       # (the column sums -- a bias gradient -- ride along with the split's read of g)
                self.plain, self.t, self.colsum = split_scaled_both(g2d, self.scale, colsum=True)
            else:
                self.plain, self.t = split_scaled_both(g2d, self.scale)
        elif colsum:
            self.colsum = g2d.sum(dim=0)     # (all zero, or not finite: the sum says so)


def absmax(x):
    """max |x| as a Python float (one host read) -- egnn_absmax_f32: one pass over x where `x.abs().max()` makes two and a copy.
    What the power-of-two scales of the gradient GEMMs and of the edge backward are chosen from.  (Host tensors -- the CPU tests of
    the backward's host logic -- go through torch.)"""
    if not x.is_cuda:
        return float(x.abs().max())
    return absmax_async(x).floats()[0]


def absmax_async(x):
    """`absmax` whose host read can wait: the launch now, a HostRead of the bit pattern (`.floats()[0]` = max |x|)."""
    if not x.is_cuda:
        return HostRead(x.abs().max().reshape(1).float())
    x = aligned(x)                                   # (a chunk of graphs sliced out of a saved tensor starts wherever the chunk does)
    out = torch.empty(1, dtype=torch.int32, device=x.device)
    with _timed("absmax"):
        rc = _abi.load().egnn_absmax_f32(_ptr(x), x.numel(), _ptr(out), _stream())
    _abi.check(rc, "egnn_absmax_f32")
    return HostRead(out)


def unsplit_words_(table, cols):
    """egnn_unsplit_words_f32: columns [0, cols) of the fp32 table hold (fp16 hi, fp16 lo) words -> hi + lo, in place."""
    with _timed("unsplit_words"):
        rc = _abi.load().egnn_unsplit_words_f32(_ptr(table), table.stride(0), table.shape[0], cols, _stream())
    _abi.check(rc, "egnn_unsplit_words_f32")
    return table


NONFINITE = "nonfinite"          # grad_scale of an operand that holds a NaN / inf: its products are NaN, like any fp32 product would be


def grad_scale(amax):
    """The power of two that brings max |x| into [2^12, 2^13) (fp16 hi halves well inside the range, lo halves off the subnormals);
    None for an all-zero operand (the product is zero), NONFINITE for one that holds a NaN or an inf (the product is NaN)."""
    from . import _weights
    if amax != amax or amax == float("inf"):
        return NONFINITE
    if not (amax > 0.0):
        return None
    # (clamped: for max |x| below ~2^-88 the scale -- a C float in the ABI -- and the inverse scales built from it would leave fp32's
    # normal range; such an operand is split with 2^100 instead, its values then sit in fp16's subnormals or flush to zero, which is
    # what the fp32 product they replace would have given at that magnitude: ~0)
    return min(_weights.pow2_scale(amax) * 4096.0, 2.0 ** 100)


def grad_nn(g2d, wsplit_t, n, residual=None, name="grad_nn", amax=None):
    """g2d (R, K) fp32 @ W (K, n), W given as the packed split image of W^T (n rows, K): on the split-f16 GEMM of the forward,
    g2d pre-scaled by a power of two (gradients are small: their fp16 lo halves must stay off the subnormals).  amax: max |g2d| if
    the caller has it already; g2d may be a GradOperand (both of its products share one split)."""
    if isinstance(g2d, GradOperand):
        op = g2d
        scale, a, rows, dev = op.scale, op.plain, op.shape[0], (residual.device if residual is not None else wsplit_t[0].device)
    else:
        scale, rows, dev = grad_scale(absmax(g2d) if amax is None else amax), g2d.shape[0], g2d.device
        a = None if (scale is None or scale is NONFINITE) else split_scaled(g2d, scale)[0]      # max |scale * g| in [2^12, 2^13)
    if scale is NONFINITE:
        return torch.full((rows, n), float("nan"), dtype=torch.float32, device=dev)
    if scale is None:
        out = torch.zeros(rows, n, dtype=torch.float32, device=dev)
        return out if residual is None else out + residual
    whi, wlo, inv, w_rows = wsplit_t
    return linear_hl(a, (whi, wlo, inv / scale, w_rows), n, None, residual=residual, name=name)


def grad_tn_operand(x2d, amax=None):
    """The right-hand operand of grad_tn, prepared once for several products with the same x2d: (packed image of (s x2d)^T, rows, s)
    or None when x2d is all zero / not finite.  amax: max |x2d| if the caller has it."""
    sx = grad_scale(absmax(x2d) if amax is None else amax)
    if sx is None or sx is NONFINITE:
        return sx
    w, w_rows = split_scaled(x2d, sx, transposed=True, w_image=True)  # (n rows, K = r)
    return w, w_rows, sx


def grad_tn(g2d, x2d, k_splits=None, name="grad_tn", amax=None, x_operand=None):
    """g2d (R, M)^T @ x2d (R, N) -> (M, N): the weight-gradient contraction over R = B N nodes, split-K on the split-f16 GEMM.
    amax: max |g2d| if known; x_operand: grad_tn_operand(x2d) if several products share x2d."""
    op = g2d if isinstance(g2d, GradOperand) else None
    r, m = (op.shape if op is not None else g2d.shape)
    n = x2d.shape[1]
    sg = op.scale if op is not None else grad_scale(absmax(g2d) if amax is None else amax)
    if x_operand is None:
        x_operand = grad_tn_operand(x2d)
    if sg is NONFINITE or x_operand is NONFINITE:
        return torch.full((m, n), float("nan"), dtype=torch.float32, device=x2d.device)
    if sg is None or x_operand is None:
        return torch.zeros(m, n, dtype=torch.float32, device=x2d.device)
    w, w_rows, sx = x_operand
    a = op.t if op is not None else split_scaled(g2d, sg, transposed=True)[0]                    # (m rows, K = r)
    nkt = a.kp // 16
    if k_splits is None:
        tiles = ((m + 127) // 128) * ((n + 127) // 128)
        k_splits = 1
        while tiles * k_splits < 512 and nkt // (2 * k_splits) >= 64:
            k_splits *= 2
    mp = m
    parts = empty(k_splits, mp, n, dtype=torch.float32, device=x2d.device)
    with _timed(name):
        rc = _abi.load().egnn_linear_hl_splitk_f32(_ptr(a.hi), _ptr(a.lo), _ptr(w.hi), _ptr(w.lo), 1.0, _ptr(parts), n, m, n, a.kp, w_rows,
                                                   k_splits, _stream())
    _abi.check(rc, "egnn_linear_hl_splitk_f32")
    out = empty(m, n, dtype=torch.float32, device=x2d.device)
    count = m * n
    if count % 4 != 0:
        return parts.sum(dim=0) / (sg * sx)
    rc = _abi.load().egnn_sum_parts_f32(_ptr(parts), k_splits, count, 1.0 / (sg * sx), _ptr(out), _stream())
    _abi.check(rc, "egnn_sum_parts_f32")
    return out


class DestLists:
    """The edges sorted stably by destination (egnn_dest_lists_i32): `ent` / `tile_seg` = the padded entry list of
    egnn_edge_bwd_pass_f32 (by_dest = 1), `order` / `seg` = the CSR form egnn_rows_gather_sum_f32 reads."""

    def __init__(self, ent, tile_seg, order, seg, tiles=None):
        self._ent, self.tile_seg, self.order, self.seg, self._tiles = ent, tile_seg, order, seg, tiles

    @property
    def ent(self):
        """the entry list cut to its length -- the one host read (the number of tiles), taken when the list is first used"""
        if self._tiles is not None:
            tiles = int(self._tiles.ints()[0])
            self._ent, self._tiles = self._ent[:max(128, (tiles * 16 + 127) // 128 * 128)], None
        return self._ent


def dest_lists(idx32, b, n, k, device):
    """idx32 (B,N,K) int32 or None (dense: destination = k).  One host read: the number of tiles (sizes the entry list)."""
    lib = _abi.load()
    cap = lib.egnn_dest_lists_capacity(b, n, k)
    ent = torch.empty(cap, dtype=torch.int32, device=device)
    tile_seg = torch.empty(b * n + 1, dtype=torch.int64, device=device)
    order = torch.empty(b * n * k, dtype=torch.int64, device=device)
    seg = torch.empty(b * n + 1, dtype=torch.int64, device=device)
    scratch = torch.empty(b, dtype=torch.int64, device=device)
    with _timed("dest_lists"):
        rc = lib.egnn_dest_lists_i32(_ptr(idx32), b, n, k, _ptr(ent), cap, _ptr(tile_seg), _ptr(order), _ptr(seg), _ptr(scratch), _stream())
    _abi.check(rc, "egnn_dest_lists_i32")
    return DestLists(ent, tile_seg, order, seg, HostRead(tile_seg[-1:]))


def sum_rows(part, scale=1.0):
    """scale * column sums of a (rows, count) fp32 array with many rows, in a fixed order, on egnn_sum_parts_f32 (which walks its parts
    one after the other per output element: made for a handful of split-K parts): first the rows p G + g over p for each of G groups
    (the array read as (rows / G) parts of G * count elements), then the G group sums."""
    rows, count = part.shape
    lib = _abi.load()
    g = 1
    while g < 256 and rows % (2 * g) == 0 and rows // (2 * g) >= 1:
        g *= 2
    out = empty(count, dtype=torch.float32, device=part.device)
    with _timed("sum_rows"):
        if g > 1 and rows // g > 1:
            mid = empty(g, count, dtype=torch.float32, device=part.device)
            _abi.check(lib.egnn_sum_parts_f32(_ptr(part), rows // g, g * count, 1.0, _ptr(mid), _stream()), "egnn_sum_parts_f32")
            part, rows = mid, g
        _abi.check(lib.egnn_sum_parts_f32(_ptr(part), rows, count, float(scale), _ptr(out), _stream()), "egnn_sum_parts_f32")
    return out


def edge_pool(u16, gate, pair_mask, b, n, k):
    """egnn_edge_pool_f32: (B, N, 16) sum over k of pair_mask * SiLU(u) * gate -- the pooled messages the backward's node-level part
    starts from.  gate = (gate_w (16) zero padded, gate_b (1)) or None; pair_mask (E) uint8 or None."""
    out = empty(b, n, 16, dtype=torch.float32, device=u16.device)
    with _timed("edge_pool"):
        rc = _abi.load().egnn_edge_pool_f32(_ptr(u16), _ptr(gate[0]) if gate is not None else None, _ptr(gate[1]) if gate is not None else None,
                                            _ptr(pair_mask), b, n, k, _ptr(out), _stream())
    _abi.check(rc, "egnn_edge_pool_f32")
    return out


# The `sums` row of `edge_tail_bwd(reduce=True)`: the columns of one wave's row of `part` (csrc/edge_tail.hip: PART_*), of
# TAIL_PART_FLOATS = egnn_edge_tail_part_floats() floats -- what follows the last slice is zero padding.
TAIL_PART_FLOATS = 1192
TAIL_SUMS = {
    "W3": slice(0, 1024),            # d/d coors_mlp.0.weight, (64, 16) zero padded
    "b3": slice(1024, 1088),         # d/d coors_mlp.0.bias
    "W4": slice(1088, 1152),         # d/d coors_mlp.3.weight
    "gU": slice(1152, 1168),         # column sums of gU = d/d edge_mlp's last bias
    "gate_w": slice(1168, 1184),     # d/d edge_gate.0.weight
    "b4": slice(1184, 1185),         # d/d coors_mlp.3.bias
    "scale": slice(1185, 1186),      # d/d CoorsNorm.scale
    "gate_b": slice(1186, 1187),     # d/d edge_gate.0.bias
}


def edge_tail_bwd(u16, coors, idx32, pair_mask, g_coors_out, g_msum16, w3p, b3p, w4p, b4, scale, eps, clamp, b, n, k, gate=None,
                  reduce=False, want_rel=False, drop=None, eid0=0):
    """egnn_edge_tail_bwd_f32 (include/egnn_hip.h): the per-edge closed-form backward behind edge_mlp's second Linear.
    Returns (gU (E, 16), g_rel (E, 4), g_hid (E, 64), a3 (E, 64), g_w (E,), g_scale (E,) or None); with gate = (gate_w (16) zero
    padded, gate_b (1)) -- soft_edges -- a seventh element g_gate (E,) = d loss / d (gate pre-activation).
    reduce: the kernel sums the parameter gradients' per-edge terms itself -- returns (gU, g_rel, sums (TAIL_PART_FLOATS,), rel (E, 4)
    or None, dist (E,) or None, bits of max |gU| (1-element int32 tensor)), sums laid out as TAIL_SUMS says; want_rel: also x_i - x_j
    and |x_i - x_j|^2 per edge."""
    dev = u16.device
    e = b * n * k
    f32 = dict(dtype=torch.float32, device=dev)
    lib = _abi.load()
    gu = empty(e, 16, **f32)
    g_rel = empty(e, 4, **f32)
    a = _abi.EdgeTailArgs()
    a.B, a.N, a.K, a.norm_coors = b, n, k, int(scale is not None)
    a.clamp = -1.0 if clamp is None else float(clamp)
    a.eps = float(eps)
    a.u, a.coors, a.idx, a.pair_mask = u16.data_ptr(), coors.data_ptr(), _ptr(idx32), _ptr(pair_mask)
    a.g_coors_out, a.g_msum = g_coors_out.data_ptr(), g_msum16.data_ptr()
    a.W3, a.b3, a.W4, a.b4, a.scale = w3p.data_ptr(), b3p.data_ptr(), w4p.data_ptr(), b4.data_ptr(), _ptr(scale)
    a.gU, a.g_rel = gu.data_ptr(), g_rel.data_ptr()
    if gate is not None:
        a.gate_w, a.gate_b = gate[0].data_ptr(), gate[1].data_ptr()
    if reduce:
        pf = lib.egnn_edge_tail_part_floats()
        assert pf == TAIL_PART_FLOATS, pf
        part = empty((e + 255) // 256 * 4, pf, **f32)           # one row per wave of 64 edges
        gu_bits = torch.empty(1, dtype=torch.int32, device=dev)
        a.part, a.amax_gu = part.data_ptr(), gu_bits.data_ptr()
        if drop is not None:                                  # training-mode dropout in coors_mlp: the forward's hash mask (p, seed), edges numbered from eid0
            from . import _dropout
            a.drop_thr, a.drop_seed, a.drop_inv_keep, a.drop_eid0 = _dropout.threshold(drop[0]), int(drop[1]), _dropout.inv_keep(drop[0]), int(eid0)
        rel = dist = None
        if want_rel:
            rel, dist = empty(e, 4, **f32), empty(e, **f32)
            a.rel_out, a.dist_out = rel.data_ptr(), dist.data_ptr()
    else:
        g_hid, a3, g_w = empty(e, 64, **f32), empty(e, 64, **f32), empty(e, **f32)
        g_scale = empty(e, **f32) if scale is not None else None
        g_gate = empty(e, **f32) if gate is not None else None
        a.g_hid, a.a3, a.g_w, a.g_scale, a.g_gate = g_hid.data_ptr(), a3.data_ptr(), g_w.data_ptr(), _ptr(g_scale), _ptr(g_gate)
    with _timed("edge_tail_bwd"):
        rc = lib.egnn_edge_tail_bwd_f32(byref(a), _stream())
    _abi.check(rc, "egnn_edge_tail_bwd_f32")
    if reduce:
        return gu, g_rel, sum_rows(part), rel, dist, gu_bits
    return (gu, g_rel, g_hid, a3, g_w, g_scale) + (() if gate is None else (g_gate,))


# rounds (of 128 entries) one workgroup of egnn_edge_bwd_pass_f32 streams through its column chunk: short enough that the
# workgroups of one graph and one chunk (they share the gathered rows) are many and run side by side on an XCD
ROUNDS_PER_SLAB = 8


def edge_bwd_pass(w, proj, idx32, gu16, gu_scale, scal, ent, b, n, k, by_dest, ws_nat=None, want_w2=False, n_slabs=None, row_pairs=False,
                  drop=None, eid0=0, want_amax=False, block=0):
    """One pass of egnn_edge_bwd_pass_f32 (include/egnn_hip.h) over the entry list ent (autograd.entry_list).  proj = (B*N, 2 Hp)
    fp32 P_i | P_j rows.  Returns a dict: rows (L / 16, Hp) partial rows, one per tile; with want_w2: w2 = d/d W_2 (16, Hp); with ws_nat (the
    natural-units scalar weights (Hp, S)): ws = d/d W_s (Hp, S) and scal = d/d scalars (E, S) -- the partial arrays of the
    kernel already summed (fixed order).  row_pairs (by source, 16 < K <= 32, with ws_nat): rows = one row per node (L / 32, Hp).
    block: the block of 16 message channels gu16 holds (m_dim > 16: the pass is linear in gU, one call per block) -- its rows of W_2."""
    lib = _abi.load()
    hp, s_in = w["Hp"], w["S"]
    dev = proj.device
    e = b * n * k
    l = ent.numel()
    if n_slabs is None:
        n_slabs = max(1, (l // 128 + ROUNDS_PER_SLAB - 1) // ROUNDS_PER_SLAB)
    n_rows = l // 32 if row_pairs else l // 16
    rows = empty(n_rows + 1, hp, dtype=torch.float32, device=dev)
    a = _abi.EdgeBwdArgs()
    a.B, a.N, a.K, a.Hp, a.S, a.by_dest, a.n_slabs = b, n, k, hp, s_in, int(by_dest), n_slabs
    a.wst_terms = w["Wst"].shape[1]
    a.L, a.E = l, e
    a.ent = ent.data_ptr()
    a.Pi, a.Pj, a.ldp = proj.data_ptr(), proj.data_ptr() + 4 * hp, proj.stride(0)
    a.Wst, a.ws_inv_scale = w["Wst"].data_ptr(), w["ws_inv_scale"]
    a.idx = _ptr(idx32)
    a.W2Th, a.gU, a.gu_scale = w["W2Th_blocks"][block].data_ptr(), gu16.data_ptr(), gu_scale
    a.inv_scale = 1.0 / (gu_scale * w["w2t_scale"])
    a.scal = scal.data_ptr()
    a.part_rows, a.ld_rows = rows.data_ptr(), hp
    a.row_pairs = int(row_pairs)
    amax_bits = None
    if want_amax and (s_in == 1 or ws_nat is None):           # (by-product of the fp32 tile sums: max |rows|)
        amax_bits = torch.empty(1, dtype=torch.int32, device=dev)
        a.rows_amax = amax_bits.data_ptr()
    if drop is not None:                                      # training-mode dropout in edge_mlp: the forward's hash mask (p, seed)
        from . import _dropout
        a.drop_thr, a.drop_seed, a.drop_inv_keep, a.drop_eid0 = _dropout.threshold(drop[0]), int(drop[1]), _dropout.inv_keep(drop[0]), int(eid0)
    if want_w2:
        dw2 = empty(n_slabs, 16, hp, dtype=torch.float32, device=dev)
        a.dW2_part = dw2.data_ptr()
    if ws_nat is not None:
        ch = lib.egnn_edge_bwd_chunk_steps()
        n_chunks = (hp // 32 + ch - 1) // ch
        ws_nat = ws_nat.contiguous()
        dws = empty(n_slabs * 16 if s_in > 1 else n_slabs, s_in, hp, dtype=torch.float32, device=dev)
        ds = empty(n_chunks, e, s_in, dtype=torch.float32, device=dev)
        a.Ws, a.dWs_part, a.ds_part = ws_nat.data_ptr(), dws.data_ptr(), ds.data_ptr()
        if s_in > 5:                                          # d/d s on the matrix cores: W_s^T fragments (_weights.pack)
            a.WsTh, a.wst_inv_scale = w["WsTh"].data_ptr(), 1.0 / w["wst_scale"]
        if s_in > 1:
            # d/d W_s on the matrix cores: the scalars enter as split-fp16 fragments, each column brought into [1, 2) at its maximum
            amax = scal.abs().amax(dim=0)
            col_scale = torch.where(amax > 0, torch.exp2(-torch.floor(torch.log2(amax.clamp_min(1e-30)))), torch.ones_like(amax)).contiguous()
            a.scal_scale = col_scale.data_ptr()
    wb = lib.egnn_edge_bwd_work_bytes(l, s_in, int(want_w2), int(ws_nat is not None))
    work = empty(max(wb, 16), dtype=torch.uint8, device=dev)
    a.work, a.work_bytes = work.data_ptr(), wb
    with _timed("edge_bwd_by_dest" if by_dest else "edge_bwd_by_src"):
        rc = lib.egnn_edge_bwd_pass_f32(byref(a), _stream())
    _abi.check(rc, "egnn_edge_bwd_pass_f32")
    out = {"rows": rows[:n_rows], "amax_bits": amax_bits}
    if want_w2:
        out["w2"] = dw2.sum(dim=0)          # (340 MB of per-slab partials at the north-star shape: 0.19 ms; `sum_rows` measured 0.21)
    if ws_nat is not None:
        if s_in > 1:                                          # one partial per wave (every 4th row of the array), times col_scale
            out["ws"] = (dws.view(n_slabs * 4, 4, s_in, hp)[:, 0].sum(dim=0) / col_scale[:, None]).t().contiguous()
        else:
            out["ws"] = dws.sum(dim=0).t().contiguous()
        out["scal"] = ds.sum(dim=0)
    return out


# ---------------------------------------------------------------------------------------------- whole-layer C interface
def pack_weights_c(layer):
    """egnn_pack_weights_host on the module's parameters: (desc, info, blob uint8 CPU tensor).  The Python module itself
    re-lays its weights on the device with _weights.pack (same layout, bit-identical: tests/test_host_logic.py); this is the
    path a binding without torch takes, and what `forward_c` uses."""
    import ctypes
    lib = _abi.load()
    desc = _abi.layer_desc(layer)
    sd = {k.replace(".", "_"): v.detach().float().cpu().contiguous() for k, v in layer.state_dict().items()}
    params = _abi.LayerParams()
    for f in _abi.PARAM_FIELDS:
        setattr(params, f, sd[f].data_ptr() if f in sd else None)
    nbytes = lib.egnn_packed_weights_bytes(byref(desc))
    if nbytes == 0:
        raise _abi.EGNNHipError("egnn_packed_weights_bytes: descriptor outside what the gfx950 kernels are built for")
    blob = torch.zeros(nbytes, dtype=torch.uint8)
    info = _abi.PackedInfo()
    _abi.check(lib.egnn_pack_weights_host(byref(desc), byref(params), blob.data_ptr(), byref(info)), "egnn_pack_weights_host")
    assert info.bytes == nbytes
    return desc, info, blob


def pack_weights_blob(layer, w, device):
    """The blob of the C whole-layer entry assembled ON THE DEVICE from the module's own re-laid-out tensors `w` (_weights.pack: the same
    formats, bit for bit -- tests/test_host_logic.py::test_c_weight_packer_matches_python holds the piece-by-piece mapping used here):
    (desc, info, blob uint8 on `device`).  ~0.3 ms of small copies where egnn_pack_weights_host needs 60 ms at dim 512.
    Raises EGNNHipError for a descriptor outside what the C entry is built for."""
    lib = _abi.load()
    desc = _abi.layer_desc(layer)
    info = _abi.PackedInfo()
    _abi.check(lib.egnn_packed_layout(byref(desc), byref(info)), "egnn_packed_layout")
    if (info.H, info.Hp, info.S) != (w["H"], w["Hp"], w["S"]) or 4 * info.NM != w["Wst"].shape[1]:
        raise _abi.EGNNHipError("egnn_packed_layout disagrees with _weights.pack")
    blob = torch.zeros(info.bytes, dtype=torch.uint8, device=device)

    def put(off, t):
        flat = t.to(device).contiguous().reshape(-1).view(torch.uint8)
        blob[off:off + flat.numel()].copy_(flat)

    def put_split(key, o_hi, o_lo, rows_c):
        hi, lo, inv, rows = w[key]
        if rows != rows_c:
            raise _abi.EGNNHipError(f"{key}: {rows} packed rows, the C layout expects {rows_c}")
        put(o_hi, hi)
        put(o_lo, lo)
        return float(inv)

    info.wcat_inv_scale = put_split("Wcat_split", info.wcat_hi, info.wcat_lo, info.wcat_rows)
    put(info.bcat, w["bcat"])
    put(info.wst, w["Wst"])
    put(info.w2h, w["W2h"])
    put(info.b2, w["b2"])
    info.ws_inv_scale, info.w2_inv_scale = float(w["ws_inv_scale"]), float(w["w2_inv_scale"])
    if "gate_w" in w:
        put(info.gate_w, w["gate_w"])
        put(info.gate_b, w["gate_b"])
    if "W3h" in w:
        put(info.w3h, w["W3h"])
        put(info.b3, w["b3"])
        put(info.w4, w["W4"])
        put(info.b4, w["b4"])
        info.w3_inv_scale = float(w["w3_inv_scale"])
    if "coors_scale" in w:
        put(info.coors_scale, w["coors_scale"])
    if "W5_split" in w:
        info.w5_inv_scale = put_split("W5_split", info.w5_hi, info.w5_lo, info.w5_rows)
        info.w6_inv_scale = put_split("W6_split", info.w6_hi, info.w6_lo, info.w6_rows)
        put(info.b5, w["b5"])
        put(info.b6, w["b6"])
    if "gamma" in w:
        put(info.gamma, w["gamma"])
        put(info.beta, w["beta"])
    return desc, info, blob


def forward_c(layer, feats, coors, edges=None, mask=None, adj_mat=None, packed=None):
    """One EGNN.forward through the single-call C entry egnn_layer_forward_f32 (what a non-Python binding uses); returns
    (node_out, coors_out).  `packed` = (desc, info, blob_on_device) to reuse a previous pack."""
    lib = _abi.load()
    if packed is None:
        desc, info, blob = pack_weights_c(layer)
        packed = (desc, info, blob.to(feats.device))
    desc, info, blob_dev = packed
    b, n, _ = feats.shape
    feats, coors = aligned(feats), aligned(coors)
    if edges is not None:
        edges = aligned(edges.float())
    m8, a8 = _u8(mask), _u8(adj_mat)
    stride = n * n if (a8 is not None and a8.dim() == 3) else 0
    k = layer.num_nearest_neighbors
    if adj_mat is not None and layer.only_sparse_neighbors:
        k = adj_max_degree(adj_mat)
    if not (layer.num_nearest_neighbors > 0 or layer.only_sparse_neighbors):
        k = n
    nbytes = lib.egnn_workspace_bytes(byref(desc), b, n, min(k, n))
    ws = empty(max(nbytes, 1), dtype=torch.uint8, device=feats.device)
    node_out, coors_out = torch.empty_like(feats), torch.empty_like(coors)
    rc = lib.egnn_layer_forward_f32(byref(desc), byref(info), _ptr(blob_dev), _ptr(feats), _ptr(coors), _ptr(edges), _ptr(m8),
                                    _ptr(a8), stride, b, n, k, coors.shape[-1], _ptr(node_out), _ptr(coors_out), _ptr(ws),
                                    nbytes, _status_ptr(feats.device), _stream())
    _abi.check(rc, "egnn_layer_forward_f32")
    return node_out, coors_out

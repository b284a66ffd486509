"""Memory layouts of the callers' tensors.  Every other GPU test hands the kernels contiguous tensors at the start of an allocation and
cotangents fresh from `(out * r).sum()`.  A drop-in for egnn_pytorch receives whatever a pipeline produces: coordinates sliced out of
an xyzw tensor, features that are a `narrow` of a buffer, edges expanded over the batch, the stride-0 cotangent of `.sum()`.

The same call is made twice: with one operand in an awkward layout, and with `operand.clone(memory_format=torch.contiguous_format)`.
Outputs -- and under autograd every gradient -- must be the same bits (forward and backward are bit-reproducible, and the contiguous
layout is pinned to the reference and to float64 autograd by the rest of the suite), so there is no tolerance to choose.  Every case
asserts its own precondition first (the pointer really is misaligned / the tensor really is not contiguous, and it holds the values
of its contiguous clone).  The contiguous forward of every configuration is compared once with the numpy oracle at the bar of
tests/test_gpu_fuzz.py, so that "same bits" is not a comparison of two wrong answers."""
import numpy as np
import pytest
import torch

from oracle import egnn_oracle as O

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------- layouts
INPUT_KINDS = ("off4", "off8", "sliced_last", "sliced_rows", "transposed", "expanded")
COT_KINDS = ("off4", "off8", "expanded", "expanded_scalar", "transposed", "sliced_last")


def _poison(t):
    """fill a buffer with what a kernel must not read: NaN / another token / a set flag"""
    if t.dtype.is_floating_point:
        return t.fill_(float("nan"))
    return t.fill_(1)


def relayout(t, kind):
    """`t`'s values (for the two `expanded` kinds: those of its first graph / ones) in another memory layout.
    off4 / off8: a contiguous view 4 / 8 bytes into a 16-byte-aligned buffer -- +1 / +2 float32 elements; float64 has no 4-byte
    offset and off8 is +1 element; one-byte dtypes (bool, uint8): +1 / +3 bytes; int64: +1 / +3 elements (8 bytes past a 16-byte
    boundary both times: an int64 tensor cannot sit at any other offset).  off16: +16 bytes, the aligned control of a view at an
    offset.  sliced_last: [..., :d] of a (..., d + 1) tensor.  sliced_rows: [:, ::2] of a tensor twice as long.  transposed: the
    first two non-batch dimensions (a two-dimensional tensor's two) swapped in memory.  expanded: stride 0 over the first
    dimension.  expanded_scalar: ones(()).expand(shape), what `.sum()` sends back."""
    esz = t.element_size()
    if kind in ("off4", "off8", "off16"):
        if esz == 1:
            off = {"off4": 1, "off8": 3, "off16": 16}[kind]
        elif esz == 4:
            off = {"off4": 1, "off8": 2, "off16": 4}[kind]
        else:
            assert esz == 8 and (kind != "off4" or not t.dtype.is_floating_point)
            off = {"off4": 1, "off8": 3 if not t.dtype.is_floating_point else 1, "off16": 2}[kind]
        buf = _poison(torch.empty(t.numel() + off + 16, dtype=t.dtype, device=t.device))
        assert buf.data_ptr() % 16 == 0
        out = buf[off:off + t.numel()].view(t.shape)
    elif kind == "sliced_last":
        out = _poison(torch.empty(*t.shape[:-1], t.shape[-1] + 1, dtype=t.dtype, device=t.device))[..., :t.shape[-1]]
    elif kind == "sliced_rows":
        out = _poison(torch.empty(t.shape[0], 2 * t.shape[1], *t.shape[2:], dtype=t.dtype, device=t.device))[:, ::2]
    elif kind == "transposed":
        d0 = 0 if t.dim() == 2 else 1
        shape = list(t.shape)
        shape[d0], shape[d0 + 1] = shape[d0 + 1], shape[d0]
        out = torch.empty(shape, dtype=t.dtype, device=t.device).transpose(d0, d0 + 1)
    elif kind == "expanded":
        return t[:1].clone(memory_format=torch.contiguous_format).expand(t.shape)
    elif kind == "expanded_scalar":
        return torch.ones((), dtype=t.dtype, device=t.device).expand(t.shape)
    else:
        raise KeyError(kind)
    out.copy_(t)
    return out


def check_layout(t, kind):
    """the case's precondition: it cannot silently test the canonical layout"""
    if kind in ("off4", "off8"):
        assert t.is_contiguous()
        if t.element_size() == 1:
            assert t.data_ptr() % 2 == 1, (kind, t.data_ptr())
        elif t.element_size() == 8:
            assert t.data_ptr() % 16 == 8, (kind, t.data_ptr())
        else:
            assert t.data_ptr() % 16 == (4 if kind == "off4" else 8), (kind, t.data_ptr())
    elif kind == "off16":
        assert t.is_contiguous() and t.data_ptr() % 16 == 0 and t.storage_offset() > 0
    else:
        assert not t.is_contiguous(), (kind, t.shape, t.stride())
    if kind.startswith("expanded"):
        assert 0 in t.stride()
    assert torch.equal(t, t.clone())


def _same_bits(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (what, i)
        if g is not None:
            assert g.shape == w.shape and g.dtype == w.dtype, (what, i)
            assert torch.isfinite(w).all(), (what, i)
            assert torch.equal(g, w), (what, i, float((g.double() - w.double()).abs().max()))


# ------------------------------------------------------------------------------------------------------------------ paths
# name -> dict(kw = EGNN's / EGNN_Network's arguments, b, n, cdim; grad: gradients of the inputs and of every parameter too;
#              patch: ((module name, attribute, value), ...) set while the path runs; exact: inside exact_arithmetic();
#              double: a .double() module; train: training mode (dropout), re-seeded before every run; net: an EGNN_Network)
_KNN8 = dict(dim=32, m_dim=16, num_nearest_neighbors=8)
PATHS = {
    # node_mlp in one launch; the one-call C forward, the Python launch sequence, and under autograd (the native backward with the tail kernel)
    "fused_c": dict(kw=_KNN8, b=3, n=40, mask=True),
    "fused_py": dict(kw=_KNN8, b=3, n=40, mask=True, patch=(("layer", "_C_FORWARD", False),)),
    "fused_grad": dict(kw=_KNN8, b=3, n=40, mask=True, grad=True),
    # node_mlp as two GEMMs with the residual in the second one's epilogue: K tails and the epilogue's alignment switch
    "hl_dim24_m20": dict(kw=dict(dim=24, m_dim=20, num_nearest_neighbors=8), b=3, n=40, mask=True),
    "hl_dim40": dict(kw=dict(dim=40, num_nearest_neighbors=8), b=3, n=37),
    # a dense graph on the general edge kernel, with edge features
    "dense_edges": dict(kw=dict(dim=16, edge_dim=3, fourier_features=1), b=2, n=20, mask=True),
    "dense_edges_grad": dict(kw=dict(dim=16, edge_dim=3, fourier_features=1), b=2, n=20, mask=True, grad=True),
    # a dense batch on the wave-per-node kernel (B N >= 8192, N % 32 == 0)
    "dense_pw": dict(kw=dict(dim=32), b=256, n=32, dense_pw=True),
    # only_sparse_neighbors; N % 16 == 0 beyond 128 nodes: the selection loads the adjacency 16 bytes at a time when it can
    "sparse_adj": dict(kw=dict(dim=32, only_sparse_neighbors=True), b=2, n=144, adj=2),
    # the plain fp32 kernels: on request, and for the shapes beyond the fused kernels; a float64 module (`_backward_exact` each)
    "exact_fp32": dict(kw=dict(dim=24, num_nearest_neighbors=8), b=3, n=37, mask=True, grad=True, exact=True),
    "wide_coors11": dict(kw=dict(dim=16, num_nearest_neighbors=6), b=2, n=24, cdim=11, grad=True),
    "wide_fourier8": dict(kw=dict(dim=16, fourier_features=8, num_nearest_neighbors=6), b=2, n=24, mask=True, grad=True),
    "double": dict(kw=dict(dim=16, num_nearest_neighbors=6, norm_feats=True), b=2, n=21, mask=True, grad=True, double=True),
    # the native backward without the tail kernel (a wide head, 2-D coordinates), the recompute path, graphs in chunks of one
    "native_m32_2d": dict(kw=dict(dim=32, m_dim=32, num_nearest_neighbors=8), b=3, n=40, cdim=2, mask=True, grad=True),
    "recompute": dict(kw=dict(dim=24, num_nearest_neighbors=6), b=2, n=20, mask=True, grad=True, patch=(("autograd", "_NATIVE", False),)),
    "chunked": dict(kw=_KNN8, b=3, n=37, grad=True, patch=(("autograd", "_FUSED_MAX_GRAPHS", 1),)),
    "dropout": dict(kw=dict(dim=32, num_nearest_neighbors=8, dropout=0.25), b=3, n=40, mask=True, grad=True, train=True),
    # EGNN_Network: attention blocks on float features; token / edge-token / adjacency-degree look-up tables; inference and training
    "net_attn": dict(net=True, kw=dict(depth=2, dim=32, global_linear_attn_every=1, global_linear_attn_heads=2, global_linear_attn_dim_head=8,
                                       num_nearest_neighbors=8), b=2, n=40, mask=True),
    "net_attn_train": dict(net=True, kw=dict(depth=2, dim=32, global_linear_attn_every=1, global_linear_attn_heads=2,
                                             global_linear_attn_dim_head=8, num_nearest_neighbors=8), b=2, n=40, mask=True, grad=True),
    "net_lookup": dict(net=True, kw=dict(depth=2, dim=32, num_tokens=11, num_edge_tokens=6, edge_dim=4, num_adj_degrees=2, adj_dim=2,
                                         num_nearest_neighbors=8), b=2, n=40, mask=True, adj=3),
    "net_lookup_train": dict(net=True, kw=dict(depth=2, dim=32, num_tokens=11, num_edge_tokens=6, edge_dim=4, num_adj_degrees=2, adj_dim=2,
                                               num_nearest_neighbors=8), b=2, n=40, mask=True, adj=3, grad=True),
}
GRAD_PATHS = tuple(p for p, s in PATHS.items() if s.get("grad"))


def _operands(spec):
    """the tensors of a path that a caller passes, in the order of `_Path.inputs`"""
    names = ["feats", "coors"]
    if spec["kw"].get("edge_dim", 0) > 0:
        names.append("edges")
    if spec.get("mask"):
        names.append("mask")
    if spec.get("adj"):
        names.append("adj_mat")
    return names


# Combinations that cannot exist.  Nothing is left out because it fails.
IMPOSSIBLE = (
    ("double", "feats", "off4"),        # float64: an element is 8 bytes, a view cannot start 4 bytes past a 16-byte boundary
    ("double", "coors", "off4"),
    ("double", "g_node", "off4"),
    ("double", "g_coors", "off4"),
)


def _input_cases():
    out = []
    for path, spec in PATHS.items():
        for op in _operands(spec):
            kinds = INPUT_KINDS + (("off16",) if path == "sparse_adj" and op == "adj_mat" else ())      # (off16: the aligned control)
            out += [(path, op, k) for k in kinds if (path, op, k) not in IMPOSSIBLE]
    return out


def _cot_cases():
    out = []
    for path in GRAD_PATHS:
        for which in ("g_node", "g_coors"):
            out += [(path, which, k) for k in COT_KINDS if (path, which, k) not in IMPOSSIBLE]
    return out


class _Path:
    """One configuration: its module, its canonical (contiguous, aligned) inputs and cotangents, and `run`."""

    def __init__(self, name):
        from egnn_pytorch_amd import EGNN, EGNN_Network
        spec = PATHS[name]
        self.name, self.spec = name, spec
        kw, b, n, cdim = spec["kw"], spec["b"], spec["n"], spec.get("cdim", 3)
        seed = sorted(PATHS).index(name)
        rng = np.random.default_rng(77 + seed)
        self.net = bool(spec.get("net"))
        dt = np.float64 if spec.get("double") else np.float32
        np_in = {}
        if self.net:
            torch.manual_seed(seed)
            mod = EGNN_Network(**kw)
            with torch.no_grad():                      # (tests/test_gpu_fuzz.py's scales for a stack of layers)
                for pname, m in mod.named_modules():
                    if type(m) is torch.nn.Linear:
                        torch.nn.init.xavier_normal_(m.weight)
                        if pname.endswith("coors_mlp.3"):
                            m.weight.mul_(0.125 * 0.05)
                        if pname.endswith("edge_mlp.3"):
                            m.weight.mul_(2.0 / 8 ** 0.5)
                        if pname.endswith("node_mlp.3"):
                            m.weight.mul_(0.5)
            self.params_np = {k: v.detach().numpy().copy() for k, v in mod.state_dict().items()}
            np_in["feats"] = rng.integers(0, 11, (b, n)) if "num_tokens" in kw else rng.standard_normal((b, n, kw["dim"])).astype(dt)
            if kw.get("edge_dim", 0) > 0:
                np_in["edges"] = rng.integers(0, 6, (b, n, n))
        else:
            cfg = O.EGNNConfig(**kw)
            params = O.random_params(cfg, seed=seed)
            k_eff = kw.get("num_nearest_neighbors", 0) or (3 if kw.get("only_sparse_neighbors") else n)
            params["coors_mlp.3.weight"] = params["coors_mlp.3.weight"] * np.float32(min(1.0, 8.0 / k_eff))
            params["edge_mlp.3.weight"] = params["edge_mlp.3.weight"] * np.float32(min(1.0, 4.0 / np.sqrt(k_eff)))
            mod = EGNN(**kw)
            mod.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
            self.cfg, self.params_np = cfg, params
            np_in["feats"] = rng.standard_normal((b, n, kw["dim"])).astype(dt)
            if kw.get("edge_dim", 0) > 0:
                np_in["edges"] = rng.standard_normal((b, n, n, kw["edge_dim"])).astype(dt)
        np_in["coors"] = rng.standard_normal((b, n, cdim)).astype(dt)
        if spec.get("mask"):
            lens = rng.integers(max(kw.get("num_nearest_neighbors", 1), n // 2), n, size=b)
            np_in["mask"] = np.stack([rng.permutation(np.arange(n) < ln) for ln in lens])
        if spec.get("adj"):
            i = np.arange(n)
            adj = (np.abs(i[:, None] - i[None, :]) <= 1) | (rng.random((n, n)) < 0.02)
            adj = adj | adj.T
            np_in["adj_mat"] = adj if spec["adj"] == 2 else np.stack([adj, adj.T | (np.abs(i[:, None] - i[None, :]) <= 2)][:b])
        if spec.get("double"):
            mod = mod.double()
        self.module = mod.cuda().train(bool(spec.get("train")))
        self.np_in = np_in
        self.inputs = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in np_in.items()}
        g = torch.Generator().manual_seed(500 + seed)
        tdt = torch.float64 if spec.get("double") else torch.float32
        self.cots = {"g_node": torch.randn(b, n, kw["dim"], generator=g, dtype=tdt).cuda(),
                     "g_coors": torch.randn(b, n, cdim, generator=g, dtype=tdt).cuda()}
        self.params = [p for p in self.module.parameters()]
        self.cache = {}

    def patched(self, monkeypatch):
        import egnn_pytorch_amd.autograd as A
        import egnn_pytorch_amd.layer as L
        for modname, attr, value in self.spec.get("patch", ()):
            monkeypatch.setattr({"layer": L, "autograd": A}[modname], attr, value)
        return self

    def _forward(self, t):
        if self.net:
            return self.module(t["feats"], t["coors"], adj_mat=t.get("adj_mat"), edges=t.get("edges"), mask=t.get("mask"))
        return self.module(t["feats"], t["coors"], t.get("edges"), t.get("mask"), t.get("adj_mat"))

    def run(self, inputs, cots=None):
        """(node_out, coors_out) -- and with `grad` the gradients of the floating-point inputs and of every parameter for the
        cotangents `cots` (a missing / None entry: that output does not enter the loss)."""
        import contextlib
        from egnn_pytorch_amd import layer as L
        t = dict(inputs)
        with L.exact_arithmetic() if self.spec.get("exact") else contextlib.nullcontext():
            if self.spec.get("train"):
                torch.manual_seed(1234)                          # (the dropout seed is drawn from the CPU generator)
            if not self.spec.get("grad"):
                with torch.no_grad():
                    out = self._forward(t)
                torch.cuda.synchronize()
                return tuple(out)
            leaves = []
            for k in ("feats", "coors", "edges"):
                if k in t and t[k].is_floating_point():
                    t[k] = t[k].detach().requires_grad_(True)
                    assert t[k].stride() == inputs[k].stride() and t[k].data_ptr() == inputs[k].data_ptr()
                    leaves.append(t[k])
            with torch.enable_grad():
                node, co = self._forward(t)
            cots = self.cots if cots is None else cots
            pairs = [(o, cots.get(k)) for o, k in ((node, "g_node"), (co, "g_coors")) if cots.get(k) is not None]
            grads = torch.autograd.grad([o for o, _ in pairs], leaves + self.params, grad_outputs=[g for _, g in pairs], allow_unused=True)
        torch.cuda.synchronize()
        return (node.detach(), co.detach()) + tuple(grads)

    def baseline(self, key, inputs, cots=None):
        """`run` on contiguous tensors, once per set of values"""
        if key not in self.cache:
            self.cache[key] = self.run(inputs, cots)
        return self.cache[key]


_paths = {}


def _path(name, monkeypatch):
    if name not in _paths:
        _paths[name] = _Path(name)
    return _paths[name].patched(monkeypatch)


def _contig(t):
    return t.clone(memory_format=torch.contiguous_format)


# ------------------------------------------------------------------------------------------------------------------ tests
# what a run of each path must go through (+) / must not go through (-): "c" = the one-call C forward took the call, "fused" = node_mlp
# in one launch, "tail" = the tail kernel, the rest = the backward of that name
ROUTES = {
    "fused_c": "+c", "fused_py": "-c +fused", "fused_grad": "-c +fused +native +tail", "hl_dim24_m20": "+c", "hl_dim40": "+c",
    "dense_edges": "+c", "dense_edges_grad": "+native", "dense_pw": "-c +fused", "sparse_adj": "+c", "exact_fp32": "+exact -native",
    "wide_coors11": "+exact -native", "wide_fourier8": "+exact -native", "double": "+exact -native", "native_m32_2d": "+native -tail -fused",
    "recompute": "+recompute -native", "chunked": "+native +tail", "dropout": "+native -fused", "net_attn": "+c", "net_attn_train": "+native",
    "net_lookup": "-c", "net_lookup_train": "+native",
}


@pytest.mark.parametrize("name", list(PATHS))
def test_path_runs_the_code_it_is_named_for(name, monkeypatch):
    import egnn_pytorch_amd.autograd as A
    import egnn_pytorch_amd.layer as L
    from egnn_pytorch_amd import _ops
    p = _path(name, monkeypatch)
    seen = set()

    def spy(obj, attr, tag, taken=lambda out: True):
        orig = getattr(obj, attr)

        def wrapper(*a, **kw):
            out = orig(*a, **kw)
            if taken(out):
                seen.add(tag)
            return out
        monkeypatch.setattr(obj, attr, wrapper)

    spy(L.EGNN, "_forward_c", "c", lambda out: out is not None)
    spy(_ops, "node_mlp_fused", "fused")
    spy(_ops, "edge_tail_bwd", "tail")
    for tag in ("native", "exact", "recompute"):
        spy(A, "_backward_" + tag, tag)
    if "chunked" == name:
        chunks = []
        orig = _ops.edge_tail_bwd
        monkeypatch.setattr(_ops, "edge_tail_bwd", lambda *a, **kw: chunks.append(1) or orig(*a, **kw))
    p.run(p.inputs)
    for want in ROUTES[name].split():
        assert (want[1:] in seen) == (want[0] == "+"), (name, want, sorted(seen))
    if "chunked" == name:
        assert len(chunks) == p.spec["b"]                        # one graph per chunk


@pytest.mark.parametrize("name", list(PATHS))
def test_contiguous_forward_matches_the_oracle(name, monkeypatch):
    """The configuration itself against the numpy oracle (eval mode), 1e-4 of the output's scale as in tests/test_gpu_fuzz.py."""
    p = _path(name, monkeypatch)
    spec, kw, x = p.spec, p.spec["kw"], p.np_in
    if spec.get("dense_pw"):
        assert p.module._dense_pw(spec["b"], spec["n"], 3)
    if p.net:
        cfg = O.EGNNConfig(dim=kw["dim"], edge_dim=kw.get("edge_dim", 0) + kw.get("adj_dim", 0), norm_feats=True,
                           num_nearest_neighbors=kw["num_nearest_neighbors"])
        want = O.egnn_network_forward(kw["depth"], cfg, p.params_np, x["feats"], x["coors"], adj_mat=x.get("adj_mat"), edges=x.get("edges"),
                                      mask=x.get("mask"), num_adj_degrees=kw.get("num_adj_degrees"),
                                      global_linear_attn_every=kw.get("global_linear_attn_every", 0),
                                      global_linear_attn_heads=kw.get("global_linear_attn_heads", 8))[:2]
        scale, depth = 16.0, kw["depth"]
    else:
        want = O.egnn_forward(p.cfg, p.params_np, x["feats"], x["coors"], x.get("edges"), x.get("mask"), x.get("adj_mat"))
        scale, depth = 256.0, 1
    was = p.module.training
    p.module.eval()
    try:
        got = p.baseline("canon", p.inputs) if not was else p.run(p.inputs)
    finally:
        p.module.train(was)
    for g, w in zip(got[:2], want):
        assert np.isfinite(w).all()
        tol = 1e-4 * max(1.0, float(np.abs(w).max()) / scale) * depth
        err = float(np.abs(g.cpu().numpy() - w).max())
        print(f"{name}: max |got - oracle| = {err:.3e} (bar {tol:.3e})")
        assert err <= tol, (name, err, tol)


@pytest.mark.parametrize("name,operand,kind", _input_cases(), ids=lambda v: str(v))
def test_input_layout_gives_the_bits_of_the_contiguous_call(name, operand, kind, monkeypatch):
    p = _path(name, monkeypatch)
    awkward = relayout(p.inputs[operand], kind)
    check_layout(awkward, kind)
    inputs = dict(p.inputs)
    inputs[operand] = _contig(awkward)
    same_values = torch.equal(inputs[operand], p.inputs[operand])
    assert same_values or kind == "expanded"
    want = p.baseline("canon" if same_values else ("in", operand, kind), inputs)
    inputs[operand] = awkward
    got = p.run(inputs)
    _same_bits(got, want, (name, operand, kind))


@pytest.mark.parametrize("name,which,kind", _cot_cases(), ids=lambda v: str(v))
def test_cotangent_layout_gives_the_bits_of_the_contiguous_cotangent(name, which, kind, monkeypatch):
    p = _path(name, monkeypatch)
    awkward = relayout(p.cots[which], kind)
    check_layout(awkward, kind)
    cots = dict(p.cots)
    cots[which] = _contig(awkward)
    same_values = torch.equal(cots[which], p.cots[which])
    assert same_values or kind.startswith("expanded")
    want = p.baseline("canon" if same_values else ("cot", which, kind), p.inputs, cots)
    cots[which] = awkward
    got = p.run(p.inputs, cots)
    _same_bits(got, want, (name, which, kind))


def _missing_cases():
    out = []
    for path in GRAD_PATHS:
        for which, kind in (("g_node", "off4"), ("g_node", "expanded_scalar"), ("g_coors", "off8"), ("g_coors", "transposed")):
            out.append((path, which, "off8" if (path, which, kind) in IMPOSSIBLE else kind))
    return out


@pytest.mark.parametrize("name,which,kind", _missing_cases(), ids=lambda v: str(v))
def test_one_cotangent_missing_the_other_in_an_awkward_layout(name, which, kind, monkeypatch):
    """An output the loss does not depend on arrives in the backward as None; the other one's cotangent in an awkward layout."""
    p = _path(name, monkeypatch)
    awkward = relayout(p.cots[which], kind)
    check_layout(awkward, kind)
    want = p.baseline(("only", which, kind), p.inputs, {which: _contig(awkward)})
    got = p.run(p.inputs, {which: awkward})
    _same_bits(got, want, (name, which, kind))
    assert any(g is not None and bool(g.ne(0).any()) for g in got[2:])


@pytest.mark.parametrize("kw,cdim,dtype", [(dict(dim=16, num_nearest_neighbors=6), 3, torch.float32),
                                           (dict(dim=8, num_nearest_neighbors=4, norm_feats=True), 3, torch.float64)])
def test_create_graph_with_expanded_cotangents_in_both_backwards(kw, cdim, dtype):
    """create_graph=True: the first backward receives the stride-0 cotangent of `.sum()` for one output and a sliced one for the other,
    the second backward expanded cotangents again -- against the same calls with contiguous clones."""
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(11)
    layer = EGNN(**kw)
    with torch.no_grad():
        for m in layer.modules():
            if type(m) is torch.nn.Linear:
                torch.nn.init.xavier_normal_(m.weight)
    layer = layer.to(dtype).cuda()
    g = torch.Generator().manual_seed(12)
    b, n = 2, 14
    feats = relayout(torch.randn(b, n, kw["dim"], generator=g, dtype=dtype).cuda(), "sliced_last")
    coors = relayout(torch.randn(b, n, cdim, generator=g, dtype=dtype).cuda(), "off8")
    check_layout(feats, "sliced_last")
    check_layout(coors, "off8")
    gn = relayout(torch.empty(b, n, kw["dim"], dtype=dtype).cuda(), "expanded_scalar")
    gc = relayout(torch.randn(b, n, cdim, generator=g, dtype=dtype).cuda(), "sliced_last")
    c2f = relayout(torch.randn(b, n, kw["dim"], generator=g, dtype=dtype).cuda(), "expanded")
    c2c = relayout(torch.empty(b, n, cdim, dtype=dtype).cuda(), "expanded_scalar")
    for t, kind in ((gn, "expanded_scalar"), (gc, "sliced_last"), (c2f, "expanded"), (c2c, "expanded_scalar")):
        check_layout(t, kind)

    def run(fix):
        f, c = fix(feats).detach().requires_grad_(True), fix(coors).detach().requires_grad_(True)
        with torch.enable_grad():
            node, co = layer(f, c)
            first = torch.autograd.grad([node, co], [f, c], grad_outputs=[fix(gn), fix(gc)], create_graph=True)
            second = torch.autograd.grad(list(first), [f, c] + list(layer.parameters()), grad_outputs=[fix(c2f), fix(c2c)], allow_unused=True)
        torch.cuda.synchronize()
        return (node.detach(), co.detach()) + tuple(t.detach() for t in first) + tuple(second)

    got, want = run(lambda t: t), run(_contig)
    _same_bits(got, want, (kw, str(dtype)))
    assert any(s is not None and bool(s.ne(0).any()) for s in got[4:])

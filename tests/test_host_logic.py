"""CPU-side checks of the shipped host code: the C-ABI library loads and exports every symbol the binding
names (the binding against the header: tests/test_abi_agreement.py), the drop-in modules keep the reference's constructor / state_dict contract, the weight re-layout
is algebraically exact, and the product path refuses to run without a GPU (no fallback)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import egnn_oracle as O
from tests._util import golden_names, layer_kwargs, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_library_loads_and_exports_header_symbols():
    """(The header against the binding, symbol by symbol and type by type: tests/test_abi_agreement.py.)"""
    from egnn_pytorch_amd import _abi
    lib = _abi.load()                                   # no compute call: loading needs no GPU
    for sym in _abi.SYMBOLS:
        assert hasattr(lib, sym), sym
    assert lib.egnn_abi_version() == _abi.ABI_VERSION
    assert lib.egnn_padded_hidden(2050) == 2080 and lib.egnn_padded_hidden(64) == 64
    from egnn_pytorch_amd import _weights
    for s_ in range(1, 17):                             # host mirror of the kernel's instantiation table
        assert lib.egnn_edge_mfmas(s_) == _weights.edge_mfmas(s_) and 4 * _weights.edge_mfmas(s_) >= 3 * s_
    assert b"out of range" in lib.egnn_error_string(-5)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from egnn_pytorch_amd import _abi
    monkeypatch.setattr(_abi, "_lib", None)
    monkeypatch.setenv("EGNN_HIP_LIB", str(tmp_path / "nope.so"))
    with pytest.raises(_abi.EGNNHipError):
        _abi.load()


def test_no_cpu_fallback():
    from egnn_pytorch_amd import EGNN
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EGNN(dim=8)(torch.randn(1, 4, 8), torch.randn(1, 4, 3))


def test_autograd_mode_is_decided_before_no_grad():
    """ADVICE r1 (superseded by autograd support): whether a graph is recorded is decided BEFORE any no_grad block -- with
    grad mode on and something requiring grad the call goes through autograd.EGNNFunction, under no_grad it does not.  (On
    the CPU both end at the no-CPU-fallback error; the GPU behaviour is in tests/test_autograd.py.)"""
    from egnn_pytorch_amd import EGNN, autograd
    layer = EGNN(dim=8)
    x = torch.randn(1, 4, 8, requires_grad=True)
    assert autograd.wants_grad(layer, x) and autograd.wants_grad(layer, torch.randn(1, 4, 8))
    with torch.no_grad():
        assert not autograd.wants_grad(layer, x)
    for p in layer.parameters():
        p.requires_grad_(False)
    assert not autograd.wants_grad(layer, torch.randn(1, 4, 8)) and autograd.wants_grad(layer, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(x, torch.randn(1, 4, 3))


def test_product_code_never_imports_oracle():
    pkg = os.path.join(ROOT, "egnn_pytorch_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.replace("checks it against the CPU oracle", ""), f


@pytest.mark.parametrize("name", golden_names())
def test_state_dict_roundtrip_with_reference_keys(name):
    """The reference's state_dict (stored in the golden file) loads strictly into the drop-in module."""
    from egnn_pytorch_amd import EGNN, EGNN_Network
    meta, params, _ = load_golden(name)
    net = EGNN(**meta["kwargs"]) if meta["kind"] == "layer" else EGNN_Network(**meta["kwargs"])
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    res = net.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert list(net.state_dict().keys()) == list(sd.keys())            # same registration order too
    for k, v in net.state_dict().items():
        assert v.shape == sd[k].shape


def test_global_attention_block_matches_oracle():
    """The induced-set attention block (device-agnostic tensor plumbing) against the oracle's
    restatement of egnn_pytorch.py:81-144, with the reference's parameters from the golden file."""
    from egnn_pytorch_amd.attention import GlobalLinearAttention
    from oracle import egnn_oracle as O
    meta, params, d = load_golden("net_global_attn")
    kw = meta["kwargs"]
    blk = GlobalLinearAttention(dim=kw["dim"], heads=kw["global_linear_attn_heads"],
                                dim_head=kw["global_linear_attn_dim_head"]).eval()
    pre = "layers.0.0."
    blk.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in params.items() if k.startswith(pre)}, strict=True)
    x, mask = d["feats"], d["mask"]
    tok = np.broadcast_to(params["global_tokens"][None], (x.shape[0],) + params["global_tokens"].shape).copy()
    with torch.no_grad():
        got_x, got_q = blk(torch.from_numpy(x), torch.from_numpy(tok), mask=torch.from_numpy(mask))
    ref_x, ref_q = O.global_linear_attention(params, pre, x, tok, kw["global_linear_attn_heads"], mask=mask)
    np.testing.assert_allclose(got_x.numpy(), ref_x, atol=2e-5, rtol=0)
    np.testing.assert_allclose(got_q.numpy(), ref_q, atol=2e-5, rtol=0)


def test_global_attention_fully_masked_graph_stays_finite():
    """a graph whose mask row is all False (a fully padded batch entry) -- the reference fills the logits with
    -finfo.max and softmaxes to a uniform distribution (egnn_pytorch.py:102-107); outputs stay finite and equal the
    oracle's."""
    from egnn_pytorch_amd.attention import GlobalLinearAttention
    from oracle import egnn_oracle as O
    meta, params, d = load_golden("net_global_attn")
    kw = meta["kwargs"]
    blk = GlobalLinearAttention(dim=kw["dim"], heads=kw["global_linear_attn_heads"],
                                dim_head=kw["global_linear_attn_dim_head"]).eval()
    pre = "layers.0.0."
    blk.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in params.items() if k.startswith(pre)}, strict=True)
    x, mask = d["feats"], d["mask"].copy()
    mask[0, :] = False
    tok = np.broadcast_to(params["global_tokens"][None], (x.shape[0],) + params["global_tokens"].shape).copy()
    with torch.no_grad():
        got_x, got_q = blk(torch.from_numpy(x), torch.from_numpy(tok), mask=torch.from_numpy(mask))
    assert torch.isfinite(got_x).all() and torch.isfinite(got_q).all()
    ref_x, ref_q = O.global_linear_attention(params, pre, x, tok, kw["global_linear_attn_heads"], mask=mask)
    np.testing.assert_allclose(got_x.numpy(), ref_x, atol=2e-5, rtol=0)
    np.testing.assert_allclose(got_q.numpy(), ref_q, atol=2e-5, rtol=0)


def test_constructor_contract():
    from egnn_pytorch_amd import EGNN, EGNN_Network
    with pytest.raises(AssertionError):
        EGNN(dim=8, m_pool_method="max")
    with pytest.raises(AssertionError):
        EGNN(dim=8, update_feats=False, update_coors=False)
    with pytest.raises(AssertionError):
        EGNN_Network(depth=1, dim=8, num_adj_degrees=0)
    layer = EGNN(dim=16)
    w = layer.edge_mlp[0].weight
    assert abs(float(w.std()) - 1e-3) < 3e-4                        # init_: N(0, init_eps)
    net = EGNN_Network(depth=2, dim=8, num_nearest_neighbors=3, norm_coors=True)
    assert all(l[1].norm_feats for l in net.layers)                 # forced on, egnn_pytorch.py:387


@pytest.mark.parametrize("kw", [dict(dim=20, m_dim=8, edge_dim=3, fourier_features=2, soft_edges=True),
                                dict(dim=64), dict(dim=33, edge_dim=1), dict(dim=24, m_dim=32), dict(dim=16, m_dim=40)])
def test_weight_relayout_is_exact(kw):
    """Evaluate the factorised / padded / fragment-ordered weights with plain numpy on random edges and
    compare with the oracle's unfactorised Linear(cat(h_i, h_j, scal)): same numbers to fp32 round-off."""
    from egnn_pytorch_amd import EGNN, _weights
    torch.manual_seed(0)
    layer = EGNN(**kw)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn_like(p) * 0.2)
    w = {k: (v.numpy() if torch.is_tensor(v) else v) for k, v in _weights.pack(layer).items()}
    dim, m = kw["dim"], kw.get("m_dim", 16)
    s = w["S"]
    rng = np.random.default_rng(0)
    hi = rng.standard_normal((7, dim)).astype(np.float32)
    hj = rng.standard_normal((7, dim)).astype(np.float32)
    sc = rng.standard_normal((7, s)).astype(np.float32)
    sd = {k: v.detach().numpy() for k, v in layer.state_dict().items()}
    x_ref = np.concatenate([hi, hj, sc], -1) @ sd["edge_mlp.0.weight"].T + sd["edge_mlp.0.bias"]
    hp, h = w["Hp"], w["H"]
    assert hp % 32 == 0 and hp >= h and w["Ws"].shape == (s, hp)
    # the kernel's variable is y = -log2(e) * x ...
    pi = hi @ w["Wcat"][:hp].T + w["bcat"][:hp]
    pj = hj @ w["Wcat"][hp:].T + w["bcat"][hp:]
    y = pi + pj + sc @ w["Ws"]
    np.testing.assert_allclose(y[:, :h] / -np.log2(np.e), x_ref, atol=3e-5)
    assert np.all(y[:, h:] == 0)
    # the scalar columns as first-layer MFMA fragments: five fp16 products per (scalar, hidden unit) rebuild W * s
    nt = 4 * _weights.edge_mfmas(s)
    assert w["Wst"].dtype == np.float16 and w["Wst"].shape == (hp, nt, 2) and 3 * s <= nt
    plain = _weights.swizzle_terms(torch.from_numpy(np.ascontiguousarray(w["Wst"]))).numpy()    # (an involution: undoes the pair swap of units 8 .. 15)
    assert np.all(plain[:, 3 * s:] == 0)
    tab = plain[:, :3 * s].astype(np.float64).reshape(hp, s, 3, 2)     # (hidden unit, scalar, kind, hi|lo)
    sp = sc.astype(np.float64) * w["ws_inv_scale"]                    # what the kernel splits: s' = s / ws_scale
    s1 = (sp / 1024).astype(np.float16).astype(np.float64)
    r = sp - 1024 * s1
    rh = r.astype(np.float16).astype(np.float64)
    rl = (r - rh).astype(np.float16).astype(np.float64)
    ys = np.einsum("es,hs->eh", s1, tab[:, :, 0].sum(-1)) + np.einsum("es,hs->eh", rh, tab[:, :, 1].sum(-1)) \
        + np.einsum("es,hs->eh", rl, tab[:, :, 2, 0])
    np.testing.assert_allclose(ys, sc.astype(np.float64) @ w["Ws"].astype(np.float64), atol=2e-6)
    # ... hidden = y / (1 + 2^y) = SiLU(x) / (-ln 2), contracted with hi + lo fp16 fragments of -ln2 * scale * W2
    nb = _weights.m_blocks(m)
    mp = 16 * nb
    w2h = w["W2h"].astype(np.float64)                                 # (Hp/32, NB, 2, 64, 8)
    assert w["W2h"].dtype == np.float16 and w2h.shape == (hp // 32, nb, 2, 64, 8)
    # [step][nb][lane = 16 g + c][t = 4 hb + r] holds channel 16 nb + c, hidden unit 32 step + 16 hb + 4 g + r
    unfrag = lambda f: f.reshape(hp // 32, nb, 4, 16, 2, 4).transpose(1, 3, 0, 4, 2, 5).reshape(mp, hp)
    w2 = (unfrag(w2h[:, :, 0]) + unfrag(w2h[:, :, 1])) * w["w2_inv_scale"]
    # 22 significant bits for elements near the tensor's max; lo of much smaller elements falls into fp16
    # subnormals (spacing 2^-24 of the scaled max), i.e. the absolute error stays at fp32 level of the max
    w2_true = -np.log(2.0) * sd["edge_mlp.3.weight"].astype(np.float64)
    np.testing.assert_allclose(w2[:m, :h], w2_true, rtol=4e-7, atol=2.0 ** -24 * np.abs(w2_true).max())
    assert np.all(w2[m:] == 0) and np.all(w2[:, h:] == 0)
    lg = np.log2(w["w2_inv_scale"])
    assert lg == np.round(lg) and 1.0 <= np.abs(unfrag(w2h[:, :, 0])).max() < 2.0      # power-of-two range scale
    hid = y.astype(np.float64) / (1.0 + np.exp2(y.astype(np.float64)))
    m_ref = O.silu(O.silu(x_ref) @ sd["edge_mlp.3.weight"].T + sd["edge_mlp.3.bias"])
    m_new = O.silu((hid @ w2.T + w["b2"]).astype(np.float32))
    np.testing.assert_allclose(m_new[:, :m], m_ref, atol=2e-5)
    assert np.all(m_new[:, m:] == 0)
    np.testing.assert_array_equal(w["W3"][:4 * m, :m], sd["coors_mlp.0.weight"])
    assert w["W3"].shape == (64 * nb, 16 * nb) and np.all(w["W3"][4 * m:] == 0)


def test_packed_weights_cache_tracks_parameter_updates():
    from egnn_pytorch_amd import EGNN
    layer = EGNN(dim=8)
    a = layer.packed_weights()
    assert layer.packed_weights() is a
    with torch.no_grad():
        layer.edge_mlp[0].weight.add_(1.0)
    b = layer.packed_weights()
    assert b is not a and not torch.equal(a["Wcat"], b["Wcat"])


def test_packed_weights_cache_tracks_replaced_submodules():
    """A whole submodule replaced between two forwards (the old module's own _parameters never change): the packed tables must follow."""
    from egnn_pytorch_amd import EGNN
    torch.manual_seed(0)
    layer = EGNN(dim=8, norm_feats=True)
    a = layer.packed_weights()
    assert layer.packed_weights() is a
    new_first = torch.nn.Linear(layer.edge_mlp[0].in_features, layer.edge_mlp[0].out_features)
    layer.edge_mlp[0] = new_first                                   # nn.Sequential.__setitem__
    b = layer.packed_weights()
    assert b is not a and not torch.equal(a["Wcat"], b["Wcat"])
    assert layer.packed_weights() is b
    norm = torch.nn.LayerNorm(8)
    with torch.no_grad():
        norm.weight.fill_(3.0)
    layer.node_norm = norm                                          # nn.Module.__setattr__
    c = layer.packed_weights()
    assert c is not b and float(c["gamma"][0]) == 3.0
    assert layer.packed_weights() is c


@pytest.mark.parametrize("m_dim", [16, 40])
def test_backward_leaves_the_packed_weights_as_they_were(m_dim):
    """A backward reads the layer's cached packed weights and writes nothing into them: the same keys and the same tensor objects before
    and after, whole and with one call per block of 16 message channels (m_dim 40) -- the block is an argument of `_ops.edge_bwd_pass`.
    The one exception is the cache of padded parameter copies the backward keeps there, `bwd_pads`."""
    from tests.test_autograd import _emulated_backward, _emulated_case
    layer, feats, coors, idx, rank, gn, gc = _emulated_case(dict(dim=8, num_nearest_neighbors=7, m_dim=m_dim))
    written = []

    class Recording(dict):                                                       # (a write that is undone afterwards counts too)
        def __setitem__(self, key, value):
            written.append(key)
            dict.__setitem__(self, key, value)

        def pop(self, key, *default):
            written.append(key)
            return dict.pop(self, key, *default)

    w = layer._packed = Recording(layer.packed_weights())
    before = {k: v for k, v in w.items() if k != "bwd_pads"}
    blocks = list(w["W2Th_blocks"])
    got = _emulated_backward(layer, feats, coors, None, idx, rank, 0.8, gn, gc)
    assert all(g is not None and float(g.abs().max()) > 0 for g in got)         # (a backward did run)
    assert layer.packed_weights() is w and set(written) <= {"bwd_pads"}, written
    after = {k: v for k, v in w.items() if k != "bwd_pads"}
    assert list(after) == list(before)
    assert all(after[k] is before[k] for k in before)
    assert len(w["W2Th_blocks"]) == len(blocks) and all(a is b for a, b in zip(w["W2Th_blocks"], blocks))


def test_packed_tile_layout_matches_header_formula():
    """_weights.pack_tiles / unpack_tiles against the offset formula documented in include/egnn_hip.h."""
    from egnn_pytorch_amd import _weights
    r, kp = 96, 64
    x = torch.arange(r * kp, dtype=torch.float32).reshape(r, kp)
    flat = _weights.pack_tiles(x)
    assert flat.numel() == r * kp
    rng = np.random.default_rng(0)
    for _ in range(500):
        row, k = int(rng.integers(r)), int(rng.integers(kp))
        off = ((((row >> 5) * (kp // 16) + (k >> 4)) * 32 + (row & 31)) * 2 + (((k >> 3) & 1) ^ (((row & 31) >> 3) & 1))) * 8 + (k & 7)
        assert float(flat[off]) == float(x[row, k])
    assert torch.equal(_weights.unpack_tiles(flat, r, kp), x)
    hi, lo, inv, w_rows = _weights.split_f16(torch.randn(130, 70))
    assert w_rows == 256 and hi.numel() == 256 * 96 and hi.dtype == torch.float16
    back = (_weights.unpack_tiles(hi, 256, 96).float() + _weights.unpack_tiles(lo, 256, 96).float()) * inv
    assert float(back[130:].abs().max()) == 0 and float(back[:, 70:].abs().max()) == 0


@pytest.mark.parametrize("kw", [dict(dim=20, m_dim=8, edge_dim=3, fourier_features=2, soft_edges=True, norm_feats=True, norm_coors=True),
                                dict(dim=64, num_nearest_neighbors=8), dict(dim=33, edge_dim=1, update_coors=False),
                                dict(dim=16, update_feats=False), dict(dim=512, num_nearest_neighbors=32),
                                dict(dim=24, m_dim=32, soft_edges=True), dict(dim=24, m_dim=40, edge_dim=2),
                                dict(dim=16, m_dim=64, fourier_features=1)])
def test_c_weight_packer_matches_python(kw):
    """egnn_pack_weights_host (C, host) == egnn_pytorch_amd/_weights.py::pack (torch): every re-laid-out tensor and every
    power-of-two scale, bit for bit -- a binding without torch gets exactly the weights the Python module computes with."""
    from egnn_pytorch_amd import EGNN, _ops, _weights
    torch.manual_seed(1)
    layer = EGNN(**kw)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn_like(p) * 0.3)
    w = _weights.pack(layer)
    desc, info, blob = _ops.pack_weights_c(layer)
    assert (info.H, info.Hp, info.S) == (w["H"], w["Hp"], w["S"]) and 4 * info.NM == w["Wst"].shape[1]

    def piece(off, ref):
        ref = ref.contiguous()
        nbytes = ref.numel() * ref.element_size()
        got = blob[off:off + nbytes].view(ref.dtype).view(ref.shape)
        assert torch.equal(got, ref), off

    hi, lo, inv, rows = w["Wcat_split"]
    assert info.wcat_rows == rows and info.wcat_inv_scale == inv
    piece(info.wcat_hi, hi); piece(info.wcat_lo, lo); piece(info.bcat, w["bcat"])
    piece(info.wst, w["Wst"]); assert info.ws_inv_scale == w["ws_inv_scale"]
    piece(info.w2h, w["W2h"]); assert info.w2_inv_scale == w["w2_inv_scale"]
    piece(info.b2, w["b2"])
    if "gate_w" in w:
        piece(info.gate_w, w["gate_w"]); piece(info.gate_b, w["gate_b"])
    if "W3h" in w:
        piece(info.w3h, w["W3h"]); assert info.w3_inv_scale == w["w3_inv_scale"]
        piece(info.b3, w["b3"]); piece(info.w4, w["W4"]); piece(info.b4, w["b4"])
    if "coors_scale" in w:
        piece(info.coors_scale, w["coors_scale"])
    if "W5_split" in w:
        for key, o_hi, o_lo, o_b, inv_c, rows_c in (("W5", info.w5_hi, info.w5_lo, info.b5, info.w5_inv_scale, info.w5_rows),
                                                    ("W6", info.w6_hi, info.w6_lo, info.b6, info.w6_inv_scale, info.w6_rows)):
            hi, lo, inv, rows = w[key + "_split"]
            assert rows_c == rows and inv_c == inv
            piece(o_hi, hi); piece(o_lo, lo); piece(o_b, w["b" + key[1]])
    if "gamma" in w:
        piece(info.gamma, w["gamma"]); piece(info.beta, w["beta"])


def test_workspace_bytes_and_descriptor_checks():
    from ctypes import byref
    from egnn_pytorch_amd import EGNN, _abi
    lib = _abi.load()
    d = _abi.layer_desc(EGNN(dim=512, num_nearest_neighbors=32))
    need = lib.egnn_workspace_bytes(byref(d), 64, 1024, 32)
    rows = 64 * 1024
    hp = lib.egnn_padded_hidden(2 * (2 * 512 + 1))
    assert need >= rows * 2 * hp * 4 + 2 * rows * 32 * 4                       # at least P and the neighbour list
    assert need < 2 * (rows * 2 * hp * 4)                                      # ... and not wildly more (P dominates)
    assert lib.egnn_workspace_bytes(byref(d), 0, 1024, 32) == 0
    bad = _abi.layer_desc(EGNN(dim=8, m_dim=16))
    bad.m_dim = 65                                                             # beyond the four accumulator tiles
    assert lib.egnn_packed_weights_bytes(byref(bad)) == 0 and lib.egnn_workspace_bytes(byref(bad), 1, 4, 4) == 0


def test_host_read_and_lazy_destination_lists_on_the_cpu():
    """_ops.HostRead on host tensors (the CPU tests of the backward run through it): the values themselves, no event; max-|x| bit
    patterns decode to floats; DestLists cuts its entry list to length on first use, from the tile count it was given as a HostRead."""
    from egnn_pytorch_amd import _ops
    bits = torch.tensor([1.5, 0.0, float("inf")], dtype=torch.float32).view(torch.int32)
    hr = _ops.HostRead(bits)
    assert hr.ev is None and hr.floats() == [1.5, 0.0, float("inf")]
    assert _ops.bits_to_floats(hr) == [1.5, 0.0, float("inf")] and _ops.bits_to_floats(bits) == [1.5, 0.0, float("inf")]
    assert _ops.HostRead(torch.tensor([7, 9], dtype=torch.int64)).ints() == [7, 9]
    assert _ops.absmax_async(torch.tensor([[-3.0, 2.0]])).floats()[0] == 3.0
    ent = torch.arange(1024, dtype=torch.int32)
    dl = _ops.DestLists(ent, torch.zeros(3, dtype=torch.int64), torch.zeros(4, dtype=torch.int64), torch.zeros(3, dtype=torch.int64),
                        _ops.HostRead(torch.tensor([20], dtype=torch.int64)))
    assert dl.ent.numel() == 384 and dl.ent.numel() == 384            # 20 tiles x 16 entries, whole 128-entry rounds; resolved once
    assert _ops.DestLists(ent[:256], None, None, None).ent.numel() == 256


def test_aligned_returns_the_tensor_itself_or_an_aligned_contiguous_copy():
    """_ops.aligned, the boundary for the callers' memory layouts: identity -- the same object, no copy -- for a contiguous tensor at a
    16-byte boundary; for a contiguous view 4 bytes into a buffer (which `.contiguous()` returns as it is), a slice of a wider tensor
    and a stride-0 expansion a copy with the same values, contiguous, at a 16-byte boundary, that leaves the source alone."""
    from egnn_pytorch_amd import _ops
    g = torch.Generator().manual_seed(0)
    base = torch.randn(3, 10, 8, generator=g)
    assert base.data_ptr() % 16 == 0 and _ops.aligned(base) is base and _ops.aligned(None) is None
    view16 = torch.randn(4 + base.numel(), generator=g)[4:].view(base.shape)        # an offset view at a 16-byte boundary: itself
    assert view16.data_ptr() % 16 == 0 and _ops.aligned(view16) is view16
    buf = torch.zeros(base.numel() + 1)
    off4 = buf[1:].view(base.shape).copy_(base)
    sliced_last = torch.randn(3, 10, 4, generator=g)[..., :3]
    expanded = torch.randn(1, 10, 8, generator=g).expand(3, 10, 8)
    scalar = torch.ones(()).expand(3, 10, 8)
    flags = torch.zeros(31, dtype=torch.bool)[1:].view(3, 10)                       # one-byte elements at an odd address
    assert off4.is_contiguous() and off4.data_ptr() % 16 == 4 and off4.contiguous() is off4
    assert not sliced_last.is_contiguous() and not expanded.is_contiguous() and not scalar.is_contiguous() and flags.data_ptr() % 2 == 1
    for t in (off4, sliced_last, expanded, scalar, flags):
        before = t.clone()
        out = _ops.aligned(t)
        assert out is not t and out.is_contiguous() and out.data_ptr() % 16 == 0 and out.stride() == before.contiguous().stride()
        assert out.dtype == t.dtype and torch.equal(out, before) and torch.equal(t, before)
        assert out.untyped_storage().data_ptr() != t.untyped_storage().data_ptr()
        assert _ops.aligned(out) is out
    leaf = off4.clone().requires_grad_(True)                                        # under autograd: a differentiable copy
    view = leaf[..., :5]
    out = _ops.aligned(view)
    out.sum().backward()
    assert torch.equal(leaf.grad[..., :5], torch.ones(3, 10, 5)) and torch.equal(leaf.grad[..., 5:], torch.zeros(3, 10, 3))


def test_copies_and_pickles_of_a_module_leave_the_kernel_side_caches_behind():
    """copy.deepcopy / pickle / torch.save of an EGNN carry the reference's state only: the re-laid-out weights, the C entry's blob and
    the cached parameter list (device tensors, ctypes structs, references to the ORIGINAL's Parameter objects) are rebuilt by the copy."""
    import copy
    import io
    import pickle
    from egnn_pytorch_amd import EGNN, _weights
    layer = EGNN(dim=16, num_nearest_neighbors=4, norm_feats=True)
    _weights.version_key(layer)                                   # (fills the parameter-list cache)
    layer.__dict__["_c_packed"] = (("key",), None)
    layer._packed, layer._packed_key = {"stale": 1}, ("key",)
    for make in (copy.deepcopy, lambda m: pickle.loads(pickle.dumps(m)),
                 lambda m: (lambda b: (torch.save(m, b), b.seek(0), torch.load(b, weights_only=False))[2])(io.BytesIO())):
        twin = make(layer)
        assert twin._packed is None and twin._packed_key is None
        assert not any(k in twin.__dict__ for k in ("_c_packed", "_param_cache", "_param_cache_mods", "_param_cache_tree", "_param_cache_counts"))
        assert all(torch.equal(a, b) for a, b in zip(layer.state_dict().values(), twin.state_dict().values()))
        # the copy's key is built from ITS parameters
        assert all(p is q for p, q in zip(twin.__dict__.get("_param_cache") or (_weights.version_key(twin) and twin.__dict__["_param_cache"]),
                                          twin.parameters()))
    assert layer.__dict__["_c_packed"] == (("key",), None) and layer._packed == {"stale": 1}      # (the original keeps its caches)


@pytest.mark.parametrize("kw", [dict(dim=24, num_nearest_neighbors=6), dict(dim=32, edge_dim=3, fourier_features=2, soft_edges=True, norm_coors=True,
                                                                               norm_feats=True), dict(dim=16, update_feats=False),
                                dict(dim=16, update_coors=False, m_dim=40), dict(dim=64, norm_feats=True)])
def test_blob_assembled_from_the_torch_packer_equals_the_c_host_packer(kw):
    """_ops.pack_weights_blob (the module's own re-laid-out tensors copied to the offsets of egnn_packed_layout: what the one-call inference
    forward runs on) == egnn_pack_weights_host's blob, byte for byte, and the same info struct."""
    from egnn_pytorch_amd import EGNN, _abi, _ops, _weights
    torch.manual_seed(2)
    layer = EGNN(**kw)
    with torch.no_grad():
        for p in layer.parameters():
            p.copy_(torch.randn_like(p) * 0.2)
    desc_c, info_c, blob_c = _ops.pack_weights_c(layer)
    desc_t, info_t, blob_t = _ops.pack_weights_blob(layer, _weights.pack(layer), torch.device("cpu"))
    assert bytes(desc_c) == bytes(desc_t)
    for name, _ in _abi.PackedInfo._fields_:
        assert getattr(info_c, name) == getattr(info_t, name), name
    assert blob_c.numel() == blob_t.numel() and torch.equal(blob_c, blob_t)


# ------------------------------------------------------------------ size limits decided on the host (tests/test_gpu_offset_limits.py crosses them)
def _bwd_pass_accepts(lib, g, n, k, hp):
    """the three size conditions egnn_edge_bwd_pass_f32 (csrc/edge_bwd.hip) checks of a call over g graphs, with the longest entry list
    such a call is handed (egnn_dest_lists_capacity; the by-source list is never longer): E and L below 2^31, the P table and the
    partial rows below 2^31 bytes"""
    e, l = g * n * k, lib.egnn_dest_lists_capacity(g, n, k)
    assert l >= (g * n * ((k + 15) // 16) * 16 + 127) // 128 * 128          # (autograd.entry_list by source)
    return e < 2 ** 31 and l < 2 ** 31, g * n * (2 * hp) * 4 < 2 ** 31, (l >> 4) * hp * 4 < 2 ** 31


def test_fused_backward_chunk_size_meets_the_kernel_limits_tightly():
    """autograd._fused_graphs_per_chunk: for (N, K, Hp) on either side of each of its three bounds every returned step satisfies what
    the kernel checks, step + 1 violates some of it, and 0 means that one graph alone does not fit."""
    from egnn_pytorch_amd import _abi, autograd as A
    lib = _abi.load()
    shapes = set()
    for hp in (64, 288, 544, 2080):
        table_n = (2 ** 31 - 1) // (2 * hp * 4)                              # the P table's bound for one graph
        for k in (1, 8, 16, 17, 32, 64, 100):
            rows_n = (2 ** 31) // ((k // 16 + 1) * hp * 4)                   # about the partial rows' bound for one graph
            for n in (64, 1000, 1024, 4096, 40000, table_n - 1, table_n, table_n + 1, table_n // 2, table_n // 2 + 1,
                      rows_n - 16, rows_n - 1, rows_n, rows_n + 1, rows_n // 2, rows_n // 3 + 1):
                if n >= max(k, 1):
                    shapes.add((n, k, hp))
    for k in (16, 32, 2048):                                                # E = g N K around 2^31 (narrow layers)
        for n in (2 ** 31 // k // 7, 2 ** 31 // k // 7 + 1, 2 ** 20):
            shapes.add((n, k, 32))
    binding = set()
    for n, k, hp in sorted(shapes):
        for b in (1, 3, 10 ** 6):
            step = A._fused_graphs_per_chunk(b, n, k, hp)
            one = all(_bwd_pass_accepts(lib, 1, n, k, hp))
            assert (step == 0) == (not one), (b, n, k, hp, step)
            if step == 0:
                continue
            assert 1 <= step <= b
            assert all(_bwd_pass_accepts(lib, step, n, k, hp)), (b, n, k, hp, step)
            if step < b:
                ok = _bwd_pass_accepts(lib, step + 1, n, k, hp)
                assert not all(ok), (b, n, k, hp, step)
                binding.update(i for i, v in enumerate(ok) if not v)
    # (the partial rows take L Hp / 4 bytes with Hp >= 32: E, L < 2^31 alone never decides)
    assert binding == {1, 2}                                                # the P table and the partial rows each decided somewhere
    assert A._fused_entry_capacity(3, 1000, 17) == lib.egnn_dest_lists_capacity(3, 1000, 17)
    assert A._fused_graphs_per_chunk(160, 1024, 32, 2080) < 126             # K = 32: the partial rows bind before the P table
    # one graph at dim 512 (Hp = 2080): beyond the P table's 2^31 bytes no chunk exists -- the limit the Python layer names
    assert A._fused_graphs_per_chunk(1, 129056, 8, 2080) == 0 and A._fused_graphs_per_chunk(1, 129055, 8, 2080) == 1
    with pytest.raises(A.FusedBackwardLimit, match=r"2\^31"):
        raise A.FusedBackwardLimit(A._fused_limit_message(1, 139264, 32, 2080))
    # the number the message names IS the largest graph admitted, for K that are no multiple of 16 as well (the partial rows take
    # N K / 16 + N tiles: the bound moves with every K)
    for k, hp in ((24, 288), (17, 288), (31, 2080), (47, 288), (8, 544), (32, 2080), (100, 64)):
        most = A._fused_largest_graph(k, hp)
        assert A._fused_graphs_per_chunk(1, most, k, hp) == 1 and A._fused_graphs_per_chunk(1, most + 1, k, hp) == 0, (k, hp, most)
        assert all(_bwd_pass_accepts(lib, 1, most, k, hp)) and not all(_bwd_pass_accepts(lib, 1, most + 1, k, hp))
        msg = A._fused_limit_message(1, most + 1, k, hp)
        assert f"at most {most} nodes per graph" in msg and f"{most + 1} nodes" in msg, msg
    assert A._fused_largest_graph(24, 288) == 745648 and A._fused_largest_graph(32, 2080) == 86032


def test_edge_kernels_cover_predicates_at_their_limits():
    """egnn_edge_pw_covers and egnn_edge_fused_covers (host functions) at N ldp 4 = 2^32 - 4 / 2^32 and B N K 16 = 2^32 - 16 / 2^32, and
    egnn_edge_fused_f32 itself: beyond what its kernels address it returns EGNN_E_UNSUPPORTED -- before it touches the device."""
    from egnn_pytorch_amd import _abi
    lib = _abi.load()
    pw = lambda b, n, k, ldp: lib.egnn_edge_pw_covers(b, n, k, 1, 0, 0, 16, 3, ldp)      # noqa: E731
    fused = lib.egnn_edge_fused_covers
    # one graph's table rows, N ldp 4 bytes: 2^32 - 4 / 2^32 (one node, so that the records stay small)
    assert pw(1, 1, 32, 2 ** 30 - 1) == 1 and pw(1, 1, 32, 2 ** 30) == 0
    assert fused(1, 32, 2 ** 30 - 1) == 1 and fused(1, 32, 2 ** 30) == 0
    assert fused(2 ** 30 - 1, 32, 1) == 1 and fused(2 ** 30, 32, 1) == 0
    ldp_hi = 2 ** 32 // (4096 * 4)                                          # ... and with 4096 nodes: 2^32 - 16 384 / 2^32
    assert pw(1, 4096, 32, ldp_hi - 1) == 1 and pw(1, 4096, 32, ldp_hi) == 0
    assert fused(4096, 32, ldp_hi - 1) == 1 and fused(4096, 32, ldp_hi) == 0
    # the slot records, B N K 16 bytes: the kernel's K is a multiple of 32, so 2^32 - 16 is no shape -- the nearest one below, 2^32 - 512,
    # and 2^32
    assert pw(1, 2 ** 23 - 1, 32, 4) == 1 and pw(1, 2 ** 23, 32, 4) == 0
    assert pw(2 ** 13 - 1, 1024, 32, 128) == 1 and pw(2 ** 13, 1024, 32, 128) == 0 and (2 ** 13) * 1024 * 32 * 16 == 2 ** 32
    # tiles that carry several nodes' P_i rows (6 <= K, K % 32 != 0) keep offset 0x80000000 free: "no such row, read zeros"
    assert fused(2 ** 29, 16, 1) == 1 and fused(2 ** 29 + 1, 16, 1) == 0
    assert fused(2 ** 29 + 1, 3, 1) == 1 and fused(2 ** 29 + 1, 64, 1) == 1
    # dim 512: ldp = 4160 floats, 258 111 nodes
    ldp = 2 * lib.egnn_padded_hidden(2050)
    assert lib.egnn_edge_fused_covers(258111, 32, ldp) == 1 and lib.egnn_edge_fused_covers(258112, 32, ldp) == 0
    # egnn_edge_fused_f32: every argument check passes, then the size guard answers.  The pointers are made up, so this call is made
    # only where no device is present: there a guard that failed could launch nothing, on a device it would launch on garbage
    if torch.cuda.is_available():
        return
    a = _abi.EdgeArgs()
    fake = 1 << 20
    a.B, a.N, a.K, a.dim, a.m_dim, a.H, a.Hp = 1, 258112, 32, 512, 16, 2050, 2080
    a.S, a.pi_split, a.ldp, a.coor_dim, a.wst_terms = 1, 1, ldp, 3, 4
    a.Pi = a.Pj = a.Wst = a.W2h = a.b2 = a.coors = a.idx = a.m_i = fake
    a.ws_inv_scale = a.w2_inv_scale = 1.0
    a.algo = 1
    assert lib.egnn_edge_fused_f32(ctypes.byref(a), None) == -3            # EGNN_E_UNSUPPORTED
    a.algo = 0
    assert lib.egnn_edge_fused_f32(ctypes.byref(a), None) == -3
    a.coor_dim = 2                                                         # (the generic-dimension compilation holds the same guard)
    assert lib.egnn_edge_fused_f32(ctypes.byref(a), None) == -3


@pytest.mark.skipif(torch.cuda.is_available(), reason="calls the entry with made-up pointers: only where no device could be launched on")
def test_c_layer_forward_refuses_a_graph_beyond_the_edge_kernels_offsets():
    """egnn_layer_forward_f32 holds egnn_edge_fused_covers' limit itself, in front of its workspace check and of every launch: one node
    beyond 4 GB of table rows per graph (dim 512: 258 112 nodes) it returns EGNN_E_UNSUPPORTED whatever the workspace; at the limit the
    next check answers (EGNN_E_SHAPE for a workspace of 0 bytes).  The pointers are never read: both calls return before the device
    is touched -- and the test runs only where there is none."""
    from ctypes import byref
    from egnn_pytorch_amd import EGNN, _abi, _ops
    desc, info, _ = _ops.pack_weights_c(EGNN(dim=512, num_nearest_neighbors=32))
    lib = _abi.load()
    fake = 1 << 20

    def call(n, ws_bytes):
        return lib.egnn_layer_forward_f32(byref(desc), byref(info), fake, fake, fake, None, None, None, 0, 1, n, 32, 3, fake, fake, fake,
                                          ws_bytes, None, None)
    assert call(258112, 1 << 50) == -3 and call(258112, 0) == -3          # EGNN_E_UNSUPPORTED
    assert call(258111, 0) == -2                                          # EGNN_E_SHAPE: the workspace check, behind the guard


def _route_cases():
    """(constructor arguments, coordinate dimension) -> the route of step 1 for (native device, native host, exact): written down from the
    rule -- standard: m_dim <= 16, coors_mlp hidden <= 64, C = 3, coors_mlp and node_mlp present, native only; closed: m_dim <= 64, on the
    native path only for device tensors; else autograd."""
    s, c, a = "standard", "closed", "autograd"
    rows = []
    for m in (16, 17, 64, 65):
        for cdim in (3, 5):
            wide = m > 64
            nat_dev = a if wide else (s if (m <= 16 and cdim == 3) else c)
            rows.append((dict(m_dim=m), cdim, (nat_dev, s if nat_dev == s else a, a if wide else c)))
    rows.append((dict(m_dim=16, update_coors=False), 3, (c, a, c)))
    rows.append((dict(m_dim=16, update_feats=False), 3, (c, a, c)))
    return rows


@pytest.mark.parametrize("kw,cdim,want", _route_cases())
def test_behind_u_route_table(kw, cdim, want):
    """autograd._behind_u_route: one rule for `_backward_native`, `_backward_exact` and `_dropout_native_ok`."""
    from egnn_pytorch_amd import EGNN, autograd as A
    layer = EGNN(dim=8, **kw)
    m = layer.m_dim
    if layer.coors_mlp is not None:
        assert layer.coors_mlp[0].weight.shape[0] == 4 * m           # (the hidden width the rule's "<= 64" is about)
    got = (A._behind_u_route(layer, m, cdim, True, True), A._behind_u_route(layer, m, cdim, False, True),
           A._behind_u_route(layer, m, cdim, True, False))
    assert got == want
    assert A._behind_u_route(layer, m, cdim, False, False) == want[2]                # (the exact path: the device does not enter)
    assert {A.ROUTE_STANDARD, A.ROUTE_CLOSED, A.ROUTE_AUTOGRAD} == {"standard", "closed", "autograd"}
    assert A._dropout_native_ok(layer) == (m <= 64)


def test_behind_u_route_wide_coors_mlp():
    """m_dim <= 16 with a coors_mlp hidden layer beyond the standard tail kernel's 64 columns: not the standard route"""
    from egnn_pytorch_amd import EGNN, autograd as A
    layer = EGNN(dim=8, m_dim=16)
    layer.coors_mlp[0], layer.coors_mlp[3] = torch.nn.Linear(16, 80), torch.nn.Linear(80, 1)
    assert A._behind_u_route(layer, 16, 3, True, True) == "closed" and A._behind_u_route(layer, 16, 3, False, True) == "autograd"


def test_tail_sums_layout():
    """_ops.TAIL_SUMS, the named columns of the tail kernel's summed `part` row: disjoint, ascending, inside EGNN_TAIL_PART_FLOATS"""
    from egnn_pytorch_amd import _abi, _ops
    spans = list(_ops.TAIL_SUMS.values())
    assert list(_ops.TAIL_SUMS) == ["W3", "b3", "W4", "gU", "gate_w", "b4", "scale", "gate_b"]
    assert spans[0].start == 0 and all(s.step is None and s.start < s.stop for s in spans)
    assert all(a.stop <= b.start for a, b in zip(spans, spans[1:]))
    assert [(s.start, s.stop) for s in spans] == [(0, 1024), (1024, 1088), (1088, 1152), (1152, 1168), (1168, 1184), (1184, 1185),
                                                  (1185, 1186), (1186, 1187)]
    assert spans[-1].stop == 1187 <= 1192 == _ops.TAIL_PART_FLOATS == _abi.load().egnn_edge_tail_part_floats()

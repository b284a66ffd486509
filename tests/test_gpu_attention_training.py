"""EGNN_Network's global attention blocks under autograd on the HIP kernels (egnn_pytorch_amd/attention.py: `_SeqProj`, `_InducedCore`,
`_TokenCore`, `_OutFF`; csrc/global_attn_bwd.hip): no library math on node-sized tensors, the backward kernels against float64 ATen,
whole networks against the reference's float64 autograd, bit reproducibility, the same step as the plain module with no more memory,
and the boundaries that keep the plain module."""
import pytest
import torch

from tests._reference import check_state, pack_grads, reference_result, state_digest, unpack_grads

pytestmark = pytest.mark.gpu


def _block(dim, heads, dim_head, seed=0, qk_scale=2.0):
    from egnn_pytorch_amd.attention import GlobalLinearAttention
    torch.manual_seed(seed)
    blk = GlobalLinearAttention(dim=dim, heads=heads, dim_head=dim_head)
    with torch.no_grad():                                   # (attention logits that are not near-uniform, LayerNorms that are not the identity)
        for name, p in blk.named_parameters():
            if "to_q" in name or "to_kv" in name:
                p.mul_(qk_scale)
            if "norm" in name or name.startswith("ff.0"):
                p.add_(0.1 * torch.randn_like(p))
    return blk


def _ragged(b, n, device="cuda"):
    lens = torch.tensor([max(1, n - (i * n) // (2 * b) - (i > 0)) for i in range(b)])
    return (torch.arange(n)[None] < lens[:, None]).to(device)


def _rel(got, want):
    want = want.to(torch.float64)
    return float((got.to(torch.float64) - want).abs().max()) / max(float(want.abs().max()), 1e-30)


# ------------------------------------------------------------------------------------------------ 1. no library math on node-sized tensors
def test_no_library_math_on_node_sized_tensors():
    from torch.utils._python_dispatch import TorchDispatchMode
    blk = _block(32, 2, 8).cuda()
    b, n, t = 2, 4096, 4
    g = torch.Generator().manual_seed(1)
    x = torch.randn(b, n, 32, generator=g).cuda().requires_grad_(True)
    tokens = torch.randn(b, t, 32, generator=g).cuda().requires_grad_(True)
    mask = _ragged(b, n)
    watched = ("mm", "bmm", "addmm", "baddbmm", "matmul", "linear", "_softmax", "_softmax_backward_data", "gelu", "gelu_backward",
               "native_layer_norm", "native_layer_norm_backward")
    limit = b * n
    big = []

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            name = func.overloadpacket.__name__
            if name in watched:
                flat = list(args) + list((kwargs or {}).values()) + list(out if isinstance(out, (tuple, list)) else (out,))
                for v in flat:
                    if isinstance(v, torch.Tensor) and v.numel() >= limit:
                        big.append((name, tuple(v.shape)))
            return out
    with Watch():
        out, tok_out = blk(x, tokens, mask=mask)
        ((out * out).sum() + tok_out.sum()).backward()
    torch.cuda.synchronize()
    assert not big, big
    for name, p in blk.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, name
    assert x.grad is not None and float(x.grad.abs().max()) > 0
    assert tokens.grad is not None and float(tokens.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 2. the kernels against float64 ATen
CORE_TOL = 2e-6        # of each output's max |.|: the bound tests/test_autograd.py puts on an fp32-class kernel result (worst measured over
                       # all cases below, N = 4096 included: 1.0e-6 -- no wider bound is needed for the long node sums)


def _mask_kinds(b, n):
    ragged = _ragged(b, n)
    dead = ragged.clone()
    dead[-1] = False
    return (("none", None), ("ragged", ragged), ("all_false_graph", dead))


@pytest.mark.parametrize("n", [1, 5, 257, 4096])
@pytest.mark.parametrize("dh", [8, 64, 96, 256])
@pytest.mark.parametrize("t", [1, 4, 8])
def test_induced_core_backward_against_float64(t, dh, n):
    from egnn_pytorch_amd import _ops
    from egnn_pytorch_amd.attention import attn_core_torch
    b, heads = 3, 2
    inner = heads * dh
    scale = dh ** -0.5
    g = torch.Generator().manual_seed(1000 * t + 10 * dh + n)
    q = torch.randn(b, t, inner, generator=g).cuda()
    kv = torch.randn(b * n, 2 * inner, generator=g).cuda()
    g_o = torch.randn(b, t, inner, generator=g).cuda()
    for kind, mask in _mask_kinds(b, n):
        o = _ops.induced_attn(q, kv, mask, b, n, heads, dh, scale)
        g_q, g_kv = _ops.induced_attn_bwd(q, kv, mask, o, g_o, b, n, heads, dh, scale)
        q64, kv64 = q.double().requires_grad_(True), kv.double().view(b, n, -1).requires_grad_(True)
        want_q, want_kv = torch.autograd.grad(attn_core_torch(q64, kv64, mask, heads, scale), (q64, kv64), g_o.double())
        eq, ekv = _rel(g_q, want_q), _rel(g_kv.view(b, n, -1), want_kv)
        print(f"induced t={t} dh={dh} n={n} {kind}: g_q {eq:.2e} g_kv {ekv:.2e}")
        assert torch.isfinite(g_q).all() and torch.isfinite(g_kv).all()
        assert eq <= CORE_TOL and ekv <= CORE_TOL, (kind, eq, ekv)
        if mask is not None:                                 # a masked node in a graph with valid nodes: an exactly zero row
            dead_rows = (~mask & mask.any(dim=1, keepdim=True)).view(-1)
            assert float(g_kv[dead_rows].abs().max() if dead_rows.any() else 0.0) == 0.0


@pytest.mark.parametrize("n", [1, 5, 257, 4096])
@pytest.mark.parametrize("dh", [8, 64, 96, 256])
@pytest.mark.parametrize("t", [1, 4, 8])
def test_token_core_backward_against_float64(t, dh, n):
    from egnn_pytorch_amd import _ops
    from egnn_pytorch_amd.attention import attn_core_torch
    b, heads = 3, 2
    inner = heads * dh
    scale = dh ** -0.5
    g = torch.Generator().manual_seed(2000 * t + 10 * dh + n)
    q = torch.randn(b * n, inner, generator=g).cuda()
    kv_tok = torch.randn(b, t, 2 * inner, generator=g).cuda()
    g_out = torch.randn(b * n, inner, generator=g).cuda()
    g_q, g_kv = _ops.token_attn_bwd(q, kv_tok, g_out, b, n, heads, dh, scale)
    q64, kv64 = q.double().view(b, n, -1).requires_grad_(True), kv_tok.double().requires_grad_(True)
    want_q, want_kv = torch.autograd.grad(attn_core_torch(q64, kv64, None, heads, scale), (q64, kv64), g_out.double().view(b, n, -1))
    eq, ekv = _rel(g_q.view(b, n, -1), want_q), _rel(g_kv, want_kv)
    print(f"token t={t} dh={dh} n={n}: g_q {eq:.2e} g_kv_tok {ekv:.2e}")
    assert eq <= CORE_TOL and ekv <= CORE_TOL, (eq, ekv)


@pytest.mark.parametrize("dim", [16, 33, 512])
def test_gelu_backward_against_float64(dim):
    from egnn_pytorch_amd import _ops
    rows = 1001                                              # (33 033 elements: the kernel's tail of count % 4 elements)
    g = torch.Generator().manual_seed(dim)
    z = (3 * torch.randn(rows, dim, generator=g)).cuda()
    go = torch.randn(rows, dim, generator=g).cuda()
    z64 = z.double().requires_grad_(True)
    a64 = torch.nn.functional.gelu(z64)
    want, = torch.autograd.grad(a64, z64, go.double())
    a, gz, bits = _ops.gelu_bwd_(z.clone(), go.clone())
    ea, eg = _rel(a, a64.detach()), _rel(gz, want)
    print(f"gelu dim={dim}: a {ea:.2e} g_z {eg:.2e}")
    assert ea <= CORE_TOL and eg <= CORE_TOL, (ea, eg)
    amax = _ops.bits_to_floats(bits)
    assert amax[0] == float(a.abs().max()) and amax[1] == float(gz.abs().max())


@pytest.mark.parametrize("dim", [16, 33, 512])
def test_layer_norm_backward_against_float64(dim):
    from egnn_pytorch_amd import _ops
    rows = 1001
    g = torch.Generator().manual_seed(dim + 1)
    x = (2 * torch.randn(rows, dim, generator=g) + 0.5).cuda()
    gamma, beta = torch.randn(dim, generator=g).cuda(), torch.randn(dim, generator=g).cuda()
    go = torch.randn(rows, dim, generator=g).cuda()
    add = torch.randn(rows, dim, generator=g).cuda()
    x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    want = torch.autograd.grad(torch.nn.functional.layer_norm(x64, (dim,), g64, b64, 1e-5), (x64, g64, b64), go.double())
    for extra in (None, add):
        got = _ops.layer_norm_bwd(x, go, gamma, 1e-5, add=extra)
        wx = want[0] if extra is None else want[0] + extra.double()
        errs = [_rel(got[0], wx), _rel(got[1], want[1]), _rel(got[2], want[2])]
        print(f"layer_norm dim={dim} add={extra is not None}: g_x {errs[0]:.2e} g_gamma {errs[1]:.2e} g_beta {errs[2]:.2e}")
        assert max(errs) <= CORE_TOL, errs


# ------------------------------------------------------------------------------------------------ 3. / 4. networks against the reference
# (kw, seed, factor on the EGNN layers' weights).  Seeds and factors were chosen on the reference alone: the 8th and 9th ranking values of
# every valid row of every layer differ by more than 1e-4 (`min_rank_gap`, stored with the results), and the outputs stay O(10) -- without
# norm_coors a stack of layers with larger weights moves the coordinates into the hundreds, where 3e-5 is below one fp32 ulp.
_NETS = {
    "attn_every2": (dict(depth=3, dim=32, num_nearest_neighbors=8, global_linear_attn_every=2, global_linear_attn_heads=2,
                         global_linear_attn_dim_head=8, num_global_tokens=4, coor_weights_clamp_value=2.0), 17, 10.0),
    "attn_every1_tokens_padded_graph": (dict(depth=2, dim=64, num_nearest_neighbors=8, global_linear_attn_every=1,
                                             global_linear_attn_heads=4, global_linear_attn_dim_head=16, num_global_tokens=8,
                                             num_tokens=21, num_positions=48, norm_coors=True), 12, 20.0),
}


def _net_case(name):
    from egnn_pytorch_amd import EGNN_Network
    kw, seed, scale = _NETS[name]
    torch.manual_seed(seed)
    net = EGNN_Network(**kw)
    with torch.no_grad():
        for attn, egnn in net.layers:                              # (the EGNN layers away from their vacuous default init)
            for p in egnn.parameters():
                p.mul_(scale)
            if attn is not None:                                   # (attention logits that are not near-uniform)
                for pname, p in attn.named_parameters():
                    if "to_q" in pname or "to_kv" in pname:
                        p.mul_(4.0)
        net.global_tokens.mul_(4.0)
    b, n = 2, 40
    g = torch.Generator().manual_seed(seed + 100)
    feats = torch.randint(0, 21, (b, n), generator=g) if "num_tokens" in kw else torch.randn(b, n, kw["dim"], generator=g)
    coors = torch.randn(b, n, 3, generator=g) * 1.5
    if "num_tokens" in kw:
        mask = torch.arange(n)[None] < torch.tensor([[n - 7], [0]])                  # the second graph is fully padded
    else:
        mask = torch.arange(n)[None] < torch.tensor([[n], [n - 9]])
    rn, rc = torch.randn(b, n, kw["dim"], generator=g), torch.randn(b, n, 3, generator=g)
    return net, kw, feats, coors, mask, rn, rc


def _net_step(model, feats, coors, mask, rn, rc, dev, dtype):
    f = feats.to(dev) if not feats.is_floating_point() else feats.to(dev, dtype).requires_grad_(True)
    c = coors.to(dev, dtype).requires_grad_(True)
    node, co = model(f, c, mask=mask.to(dev))
    wrt = [c] + ([f] if f.is_floating_point() else []) + list(model.parameters())
    loss = (node * rn.to(dev, dtype)).sum() + (co * rc.to(dev, dtype)).sum()
    return node.detach(), co.detach(), torch.autograd.grad(loss, wrt, allow_unused=True)


def _min_rank_gap(run, mask):
    """While recording: the smallest difference between the k-th and the (k + 1)-th ranking value over the valid rows of every layer of
    the reference (its `topk` re-run with one more entry) -- no tie decides a neighbour when it is well above the fp32 error of a
    squared distance."""
    orig, gaps = torch.Tensor.topk, []

    def spy(self, k_, *a, **kwargs):
        if self.shape[-1] > k_:
            vals = orig(self, k_ + 1, *a, **kwargs)[0]
            gaps.append(float((vals[..., k_] - vals[..., k_ - 1])[mask].min()))
        return orig(self, k_, *a, **kwargs)
    torch.Tensor.topk = spy
    try:
        out = run()
    finally:
        torch.Tensor.topk = orig
    return out, min(gaps), len(gaps)


@pytest.mark.parametrize("name", list(_NETS))
def test_network_gradients_match_the_reference(name):
    """Outputs (3e-5 absolute) and the gradients of coors, feats, global_tokens and every parameter (1e-4 of each gradient's scale)
    against the reference network's float64 autograd on the CPU -- DESIGN.md section 10's bounds for the native EGNN backward; the
    step twice: every gradient bit for bit the same."""
    net, kw, feats, coors, mask, rn, rc = _net_case(name)

    cache = {}

    def reference(ref, part):
        """The reference's results (computed once), stored as float32 -- 6e-8 of each value, far below the bounds -- in two files of
        alternating gradients: dim 64 with two attention blocks is 250 000 parameters."""
        if not cache:
            rnet = ref.EGNN_Network(**kw)
            rnet.load_state_dict(net.state_dict(), strict=True)
            digest = state_digest(rnet)
            rnet = rnet.double()
            (node, co, grads), gap, layers = _min_rank_gap(lambda: _net_step(rnet, feats, coors, mask, rn, rc, "cpu", torch.float64), mask)
            assert layers == kw["depth"]
            cache.update(pack_grads([None if g_ is None else g_.float() for g_ in grads]), node=node.float().numpy(),
                         coors=co.float().numpy(), min_rank_gap=gap, state_sha256=digest)
        keep = lambda k: int(k.split(".")[1]) % 2 == part if k.startswith("grad.") else (part == 0 or k == "n_grads")     # noqa: E731
        return {k: v for k, v in cache.items() if keep(k)}
    stored = {}
    for part in (1, 0):
        stored.update(reference_result(f"attention_training_{name}_part{part}", lambda ref, part=part: reference(ref, part), gpu=part == 0))
    assert float(stored["min_rank_gap"]) > 1e-4, stored["min_rank_gap"]          # no k-NN tie decides a neighbour
    check_state(net, stored)
    net = net.cuda()
    from egnn_pytorch_amd import _ops
    with _ops.phase_timer() as pt:
        node, co, got = _net_step(net, feats, coors, mask, rn, rc, "cuda", torch.float32)
    assert {"induced_attn_bwd", "token_attn_bwd", "gelu_bwd", "layer_norm_bwd"} <= set(pt.summary()), set(pt.summary())
    err_n = float((node.double().cpu() - torch.from_numpy(stored["node"])).abs().max())
    err_c = float((co.double().cpu() - torch.from_numpy(stored["coors"])).abs().max())
    print(f"{name}: outputs node {err_n:.2e} coors {err_c:.2e}")
    assert err_n <= 3e-5 and err_c <= 3e-5, (err_n, err_c)
    want = unpack_grads(stored)
    names = ["coors"] + (["feats"] if feats.is_floating_point() else []) + [k for k, _ in net.named_parameters()]
    assert len(got) == len(want) == len(names)
    worst = []
    for nm, gg, ww in zip(names, got, want):
        assert (gg is None) == (ww is None), nm
        if gg is not None:
            scale = max(1.0, float(ww.abs().max()))
            err = float((gg.double().cpu() - ww).abs().max())
            print(f"{name}: {nm} err {err:.2e} scale {scale:.2e}")
            if err > 1e-4 * scale:
                worst.append((nm, err, scale))
    assert not worst, worst
    # 4. bit-reproducible
    _, _, again = _net_step(net, feats, coors, mask, rn, rc, "cuda", torch.float32)
    for nm, a, b_ in zip(names, got, again):
        assert (a is None) == (b_ is None) and (a is None or torch.equal(a, b_)), nm


# ------------------------------------------------------------------------------------------------ 5. the same step as the plain module
def _block_step(blk, x, tokens, mask, rx, rt, exact=False):
    from egnn_pytorch_amd import exact_arithmetic
    import contextlib
    x = x.clone().requires_grad_(True)
    tokens = tokens.clone().requires_grad_(True)
    with (exact_arithmetic() if exact else contextlib.nullcontext()):
        out, tok = blk(x, tokens, mask=mask)
        loss = (out * rx).sum() + (tok * rt).sum()
        grads = torch.autograd.grad(loss, [x, tokens] + list(blk.parameters()))
    return out.detach(), tok.detach(), grads


def test_same_step_as_the_plain_module_with_no_more_memory():
    blk = _block(128, 8, 64, seed=4).cuda()
    b, n, t = 4, 1024, 4
    g = torch.Generator().manual_seed(5)
    x, tokens = torch.randn(b, n, 128, generator=g).cuda(), torch.randn(b, t, 128, generator=g).cuda()
    rx, rt = torch.randn(b, n, 128, generator=g).cuda(), torch.randn(b, t, 128, generator=g).cuda()
    mask = _ragged(b, n)
    peak = {}
    res = {}
    for which in ("hip", "aten", "hip", "aten"):             # (first round: warm-up of caches and workspaces)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res[which] = _block_step(blk, x, tokens, mask, rx, rt, exact=(which == "aten"))
        torch.cuda.synchronize()
        peak[which] = torch.cuda.max_memory_allocated() - base
    print(f"peak memory above the inputs: hip {peak['hip'] / 2**20:.1f} MiB, aten {peak['aten'] / 2**20:.1f} MiB")
    names = ["out", "tokens_out", "x", "tokens"] + [k for k, _ in blk.named_parameters()]
    flat = lambda r: [r[0], r[1]] + list(r[2])                                           # noqa: E731
    for nm, a, w in zip(names, flat(res["hip"]), flat(res["aten"])):
        err = _rel(a, w)
        print(f"block step {nm}: {err:.2e}")
        assert err <= 1e-4, (nm, err)
    assert peak["hip"] <= peak["aten"], peak


# ------------------------------------------------------------------------------------------------ 6. boundaries keep working
def _expr64(blk, x, tokens, mask, rx, rt, create_graph=False):
    """The block as the float64 expression (a deep copy of the module in float64, plain ATen)."""
    import copy
    b64 = copy.deepcopy(blk).double()
    x64, t64 = x.double().requires_grad_(True), tokens.double().requires_grad_(True)
    out, tok = b64(x64, t64, mask=mask)
    loss = (out * rx.double()).sum() + (tok * rt.double()).sum()
    return out.detach(), b64, x64, t64, loss


@pytest.mark.parametrize("kind,tol", [("nine_tokens", 1e-4), ("double", 1e-9), ("exact", 1e-4)])
def test_boundaries_keep_the_plain_module(kind, tol):
    from egnn_pytorch_amd import _ops
    blk = _block(32, 2, 8, seed=6).cuda()
    b, n = 2, 50
    t = 9 if kind == "nine_tokens" else 4
    g = torch.Generator().manual_seed(7)
    x, tokens = torch.randn(b, n, 32, generator=g).cuda(), torch.randn(b, t, 32, generator=g).cuda()
    rx, rt = torch.randn(b, n, 32, generator=g).cuda(), torch.randn(b, t, 32, generator=g).cuda()
    mask = _ragged(b, n)
    out64, b64, x64, t64, loss64 = _expr64(blk, x, tokens, mask, rx, rt)
    want = torch.autograd.grad(loss64, [x64, t64] + list(b64.parameters()))
    with _ops.phase_timer() as pt:
        if kind == "double":
            blk = blk.double()
            out, _, got = _block_step(blk, x.double(), tokens.double(), mask, rx.double(), rt.double())
        else:
            out, _, got = _block_step(blk, x, tokens, mask, rx, rt, exact=(kind == "exact"))
    assert not ({"induced_attn", "induced_attn_bwd", "token_attn_bwd"} & set(pt.summary())), set(pt.summary())
    assert _rel(out, out64) <= tol
    for a, w in zip(got, want):
        assert _rel(a, w) <= tol, _rel(a, w)


def test_create_graph_through_the_block():
    """A force-style loss: first-order gradients taken with create_graph=True through the HIP forward, then .backward() -- the
    first-order values against float64, the second-order gradients against those of the plain module in fp32."""
    from egnn_pytorch_amd import _ops, exact_arithmetic
    blk = _block(32, 2, 8, seed=8).cuda()
    b, n, t = 2, 50, 4
    g = torch.Generator().manual_seed(9)
    x, tokens = torch.randn(b, n, 32, generator=g).cuda(), torch.randn(b, t, 32, generator=g).cuda()
    rx, rt = torch.randn(b, n, 32, generator=g).cuda(), torch.randn(b, t, 32, generator=g).cuda()
    mask = _ragged(b, n)

    def second_order(module, x, tokens, rx, rt, ctx):
        x, tokens = x.clone().requires_grad_(True), tokens.clone().requires_grad_(True)
        with ctx:
            out, tok = module(x, tokens, mask=mask)
            energy = (out * rx).sum() + (tok * rt).sum()
            force, = torch.autograd.grad(energy, x, create_graph=True)
            wrt = [x, tokens] + list(module.parameters())
            return force.detach(), torch.autograd.grad(force.square().sum(), wrt, allow_unused=True)
    import contextlib
    import copy
    with _ops.phase_timer() as pt:
        force, got = second_order(blk, x, tokens, rx, rt, contextlib.nullcontext())
    assert "induced_attn" in pt.summary()                                    # (the forward ran on the HIP path)
    force_aten, want = second_order(blk, x, tokens, rx, rt, exact_arithmetic())
    b64 = copy.deepcopy(blk).double()
    force64, want64 = second_order(b64, x.double(), tokens.double(), rx.double(), rt.double(), contextlib.nullcontext())
    assert _rel(force, force64) <= 1e-4, _rel(force, force64)
    for a, w, w64 in zip(got, want, want64):
        assert (a is None) == (w is None)
        if a is not None:
            print(f"second order: vs fp32 ATen {_rel(a, w):.2e}, vs float64 {_rel(a, w64):.2e}")
            assert _rel(a, w) <= 1e-4 and _rel(a, w64) <= 1e-4

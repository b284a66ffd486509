"""The closed forms behind csrc/global_attn_bwd.hip (egnn_pytorch_amd/attention.py: `attn_core_backward_spec`, `gelu_backward_spec`,
`layer_norm_backward_spec`) against torch.autograd.grad of the literal expressions in float64, without a GPU; and the block's ATen
expression pieces (`attn_core_torch`) against `Attention.forward` itself."""
import pytest
import torch

from egnn_pytorch_amd import attention as AT

TOL = 1e-12


def _close(got, want, what):
    # (inputs and cotangents are O(1): a gradient that is exactly zero -- a one-node softmax -- is held to 1e-12 absolute)
    scale = max(float(want.detach().abs().max()), 1.0)
    err = float((got - want).abs().max())
    assert err <= TOL * scale, (what, err, scale)


def _masks(b, n, g):
    ragged = torch.rand(b, n, generator=g) > 0.3
    ragged[:, 0] = True
    dead = ragged.clone()
    dead[-1] = False                                         # a fully padded graph: uniform softmax, gradients only through v
    return {"none": None, "ragged": ragged, "all_false_graph": dead}


@pytest.mark.parametrize("mask_kind", ["none", "ragged", "all_false_graph"])
@pytest.mark.parametrize("t,heads,dh,n", [(1, 1, 8, 1), (4, 2, 8, 5), (8, 3, 16, 37)])
def test_induced_core_closed_form(t, heads, dh, n, mask_kind):
    g = torch.Generator().manual_seed(100 * t + n)
    b, inner = 3, heads * dh
    q = torch.randn(b, t, inner, generator=g, dtype=torch.float64, requires_grad=True)
    kv = torch.randn(b, n, 2 * inner, generator=g, dtype=torch.float64, requires_grad=True)
    g_o = torch.randn(b, t, inner, generator=g, dtype=torch.float64)
    mask = _masks(b, n, g)[mask_kind]
    scale = dh ** -0.5
    want = torch.autograd.grad(AT.attn_core_torch(q, kv, mask, heads, scale), (q, kv), g_o)
    got = AT.attn_core_backward_spec(g_o, q.detach(), kv.detach(), mask, heads, scale)
    _close(got[0], want[0], "g_q")
    _close(got[1], want[1], "g_kv")
    if mask_kind == "all_false_graph":
        inner_v = got[1][-1, :, inner:]
        assert float(inner_v.abs().max()) > 0 and float(got[1][-1, :, :inner].abs().max()) == 0 and float(got[0][-1].abs().max()) == 0
        # every node of the padded graph receives the same d/d v: p = 1 / N
        _close(inner_v, (g_o[-1].sum(dim=0) / n).expand(n, -1), "uniform g_v")


@pytest.mark.parametrize("t,heads,dh,n", [(1, 1, 8, 1), (4, 2, 8, 5), (8, 3, 16, 37)])
def test_token_core_closed_form(t, heads, dh, n):
    g = torch.Generator().manual_seed(7 * t + n)
    b, inner = 2, heads * dh
    q = torch.randn(b, n, inner, generator=g, dtype=torch.float64, requires_grad=True)
    kv_tok = torch.randn(b, t, 2 * inner, generator=g, dtype=torch.float64, requires_grad=True)
    g_o = torch.randn(b, n, inner, generator=g, dtype=torch.float64)
    want = torch.autograd.grad(AT.attn_core_torch(q, kv_tok, None, heads, dh ** -0.5), (q, kv_tok), g_o)
    got = AT.attn_core_backward_spec(g_o, q.detach(), kv_tok.detach(), None, heads, dh ** -0.5)
    _close(got[0], want[0], "g_q")
    _close(got[1], want[1], "g_kv_tok")


def test_core_expression_is_attention_forward():
    """`attn_core_torch` between the module's own projections reproduces `Attention.forward` (mask included)."""
    g = torch.Generator().manual_seed(3)
    attn = AT.Attention(12, heads=3, dim_head=4).double()
    x = torch.randn(2, 5, 12, generator=g, dtype=torch.float64)
    ctx = torch.randn(2, 9, 12, generator=g, dtype=torch.float64)
    mask = _masks(2, 9, g)["all_false_graph"]
    want = attn(x, ctx, mask=mask)
    got = attn.to_out(AT.attn_core_torch(attn.to_q(x), attn.to_kv(ctx), mask, attn.heads, attn.scale))
    _close(got, want, "attention")


@pytest.mark.parametrize("dim", [16, 33, 512])
def test_gelu_closed_form(dim):
    g = torch.Generator().manual_seed(dim)
    z = (3 * torch.randn(7, dim, generator=g, dtype=torch.float64)).requires_grad_(True)
    go = torch.randn(7, dim, generator=g, dtype=torch.float64)
    want, = torch.autograd.grad(torch.nn.functional.gelu(z), z, go)
    _close(AT.gelu_backward_spec(go, z.detach()), want, "g_z")


@pytest.mark.parametrize("dim", [16, 33, 512])
def test_layer_norm_closed_form(dim):
    g = torch.Generator().manual_seed(dim)
    x = (2 * torch.randn(9, dim, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    gamma = torch.randn(dim, generator=g, dtype=torch.float64, requires_grad=True)
    beta = torch.randn(dim, generator=g, dtype=torch.float64, requires_grad=True)
    go = torch.randn(9, dim, generator=g, dtype=torch.float64)
    want = torch.autograd.grad(torch.nn.functional.layer_norm(x, (dim,), gamma, beta, 1e-5), (x, gamma, beta), go)
    got = AT.layer_norm_backward_spec(go, x.detach(), gamma.detach(), 1e-5)
    for a, w, what in zip(got, want, ("g_x", "g_gamma", "g_beta")):
        _close(a, w, what)


def test_twice_gives_partial_gradients_when_one_input_depends_on_another():
    """`_twice` (a Function's backward under create_graph=True): the gradient of an input that another input was computed from is the
    partial one -- autograd adds the rest when it walks through the dependent input's own node -- and it carries a graph."""
    g = torch.Generator().manual_seed(1)
    a = torch.randn(5, generator=g, dtype=torch.float64, requires_grad=True)
    b = a.sin()
    go = torch.randn(5, generator=g, dtype=torch.float64)
    ga, gb, gn = AT._twice(lambda a, b, n: a * b * n, (a, b, 2), (go,))
    assert gn is None and ga.requires_grad and gb.requires_grad
    _close(ga.detach(), 2 * go * b.detach(), "d/d a")
    _close(gb.detach(), 2 * go * a.detach(), "d/d b")

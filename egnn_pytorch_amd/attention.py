"""Induced-set ("global linear") attention of EGNN_Network (egnn_pytorch/egnn_pytorch.py:81-144).

A handful of global tokens attend over the node features and the nodes attend back over the induced tokens.  Parameter
names and shapes are the reference's, so its `state_dict` loads unchanged (`layers.{l}.0.*`, `global_tokens`).

On the MI355X (`GlobalLinearAttention._forward_hip`, inference and training): every per-node projection -- attn1.to_kv,
attn2.to_q, attn2.to_out (+ residual), the feed-forward (Linear, exact GELU in the epilogue, Linear + residual) -- runs on the split-f16
GEMM (egnn_linear_hl_f32) with the LayerNorms fused into its operand packing (egnn_node_prep_hl), and the two attention cores
are HIP kernels (csrc/global_attn.hip: egnn_induced_attn_f32, egnn_token_attn_f32).  What stays in ATen is token-sized: the
LayerNorm and the three small Linears over the (B, T, dim) global tokens.

Under autograd the same sequence is recorded as four `torch.autograd.Function`s (`_SeqProj`, `_InducedCore`, `_TokenCore`, `_OutFF`) with
the token-sized ATen modules between them, so autograd stitches the token path.  Their backward is csrc/global_attn_bwd.hip (the two
cores, GELU, LayerNorm over node rows) and, for every node-sized product, `_ops.grad_nn` / `_ops.grad_tn` on the split-f16 GEMM.  Saved
per block: x, kv, q2, the attn2 output, x1 = attn2(x) + x and the token-sized tensors; LayerNorm outputs, the softmax statistics and
the 4 dim wide feed-forward activations are recomputed.  The closed forms the kernels implement are the `*_backward_spec` functions
below (tests/test_attention_backward_spec.py holds them against autograd in float64).  Under create_graph=True each Function
re-evaluates its step as the ATen expression from its saved inputs and lets autograd differentiate that (`_twice`).  On the CPU (where
only the tests run it), for float64 modules, under `exact_arithmetic()`, with more than 8 tokens or heads wider than 256 the block is
the plain differentiable module below."""
from __future__ import annotations

import torch
from torch import nn


class Attention(nn.Module):
    """Multi-head softmax attention of `x` over `context` (egnn_pytorch.py:83-113).  `mask` (B, n_context) removes
    context positions."""

    def __init__(self, dim, heads=8, dim_head=64):
        super().__init__()
        inner = heads * dim_head
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.to_q = nn.Linear(dim, inner, bias=False)
        self.to_kv = nn.Linear(dim, inner * 2, bias=False)
        self.to_out = nn.Linear(inner, dim)

    def forward(self, x, context, mask=None):
        b, n, _ = x.shape
        h = self.heads
        q = self.to_q(x).view(b, n, h, -1).transpose(1, 2)                           # (b, h, n, d)
        k, v = self.to_kv(context).view(b, context.shape[1], 2, h, -1).permute(2, 0, 3, 1, 4)
        dots = (q @ k.transpose(-1, -2)) * self.scale                                 # (b, h, n, n_context)
        if mask is not None:
            # as the reference (:102-105): masked logits become -finfo.max, so a context that is entirely masked (a fully
            # padded graph) softmaxes to a uniform distribution with finite outputs.  Spelled out instead of
            # F.scaled_dot_product_attention: its fused GPU kernels return something else for fully masked rows.
            dots = dots.masked_fill(~mask[:, None, None, :], -torch.finfo(dots.dtype).max)
        out = dots.softmax(dim=-1) @ v
        return self.to_out(out.transpose(1, 2).reshape(b, n, -1))


class GlobalLinearAttention(nn.Module):
    """norm -> tokens attend over the (masked) sequence -> sequence attends over the induced tokens -> residuals ->
    LayerNorm-Linear-GELU-Linear feed-forward with residual (egnn_pytorch.py:115-144)."""

    def __init__(self, *, dim, heads=8, dim_head=64):
        super().__init__()
        self.norm_seq = nn.LayerNorm(dim)
        self.norm_queries = nn.LayerNorm(dim)
        self.attn1 = Attention(dim, heads, dim_head)
        self.attn2 = Attention(dim, heads, dim_head)
        self.ff = nn.Sequential(nn.LayerNorm(dim), nn.Linear(dim, dim * 4), nn.GELU(), nn.Linear(dim * 4, dim))

    def forward(self, x, queries, mask=None):
        from . import layer as _layer
        if x.is_cuda and x.dtype == torch.float32 and queries.dtype == torch.float32 \
                and queries.shape[1] <= 8 and self.attn1.to_q.weight.shape[0] // self.attn1.heads <= 256 \
                and not _layer.exact_active():                    # (plain-fp32 mode: the differentiable module below, in fp32)
            from . import _ops
            x = _ops.aligned(x)                                   # (any layout of the caller's; under autograd a differentiable clone)
            if not (torch.is_grad_enabled() and (x.requires_grad or queries.requires_grad or
                                                 any(p.requires_grad for p in self.parameters()))):
                return self._forward_hip(x, queries, mask)
            # (the LayerNorm backward kernel holds a row's columns in registers: dim <= 1024; float64 / half modules: ATen)
            if x.shape[-1] <= 1024 and all(p.dtype == torch.float32 for p in self.parameters()):
                return self._forward_hip_autograd(x, queries, mask)
        seq, tok = self.norm_seq(x), self.norm_queries(queries)
        induced = self.attn1(tok, seq, mask=mask)
        x = self.attn2(seq, induced) + x
        return self.ff(x) + x, induced + queries

    # ------------------------------------------------------------------ gfx950 path
    def _packed(self):
        from . import _weights
        key = _weights.version_key(self)
        if getattr(self, "_pk", None) is None or self._pk_key != key:
            f = lambda w: _weights.split_f16(w.detach().float())
            v = lambda t: t.detach().float().contiguous()
            self._pk = dict(kv1=f(self.attn1.to_kv.weight), q2=f(self.attn2.to_q.weight), o2=f(self.attn2.to_out.weight),
                            ff1=f(self.ff[1].weight), ff2=f(self.ff[3].weight), bo2=v(self.attn2.to_out.bias),
                            bf1=v(self.ff[1].bias), bf2=v(self.ff[3].bias), g_seq=v(self.norm_seq.weight),
                            b_seq=v(self.norm_seq.bias), g_ff=v(self.ff[0].weight), b_ff=v(self.ff[0].bias))
            self._pk_key = key
        return self._pk

    def _forward_hip(self, x, queries, mask):
        from . import _ops
        b, n, dim = x.shape
        a1, a2 = self.attn1, self.attn2
        heads = a1.heads
        inner = a1.to_q.weight.shape[0]
        dh = inner // heads
        w = self._packed()
        x2d = x.contiguous().view(b * n, dim)
        seq_hl = _ops.node_prep_hl(x2d, None, w["g_seq"], w["b_seq"], self.norm_seq.eps, 0)            # LayerNorm(x), packed (hi, lo)
        kv = _ops.linear_hl(seq_hl, w["kv1"], 2 * inner, name="attn_kv")                               # attn1.to_kv
        tok = self.norm_queries(queries)                                                               # (B, T, dim): token-sized ATen
        induced = _ops.induced_attn(a1.to_q(tok), kv, mask, b, n, heads, dh, a1.scale)
        induced = a1.to_out(induced)                                                                   # (B, T, dim)
        q2 = _ops.linear_hl(seq_hl, w["q2"], inner, name="attn_q")                                     # attn2.to_q
        att = _ops.token_attn(q2, a2.to_kv(induced), b, n, heads, dh, a2.scale)
        x1 = _ops.linear_hl(_ops.split_f16(att), w["o2"], dim, w["bo2"], residual=x2d, name="attn_out")   # to_out + residual
        h_hl = _ops.node_prep_hl(x1, None, w["g_ff"], w["b_ff"], self.ff[0].eps, 0)
        hid = _ops.linear_hl(h_hl, w["ff1"], 4 * dim, w["bf1"], act=2, out_f32=False, out_hl=True, name="attn_ff0")
        x2 = _ops.linear_hl(hid, w["ff2"], dim, w["bf2"], residual=x1, name="attn_ff1")
        return x2.view(b, n, dim), induced + queries

    def _packed_t(self):
        """The split images of the transposed weights (the W operands of `_ops.grad_nn`), cached under `_packed`'s version key."""
        w = self._packed()
        if "kv1T" not in w:
            from . import _weights
            f = lambda p: _weights.split_f16(p.detach().float().t().contiguous())
            w.update(kv1T=f(self.attn1.to_kv.weight), q2T=f(self.attn2.to_q.weight), o2T=f(self.attn2.to_out.weight),
                     ff1T=f(self.ff[1].weight), ff2T=f(self.ff[3].weight))
        return w

    def _forward_hip_autograd(self, x, queries, mask):
        """`_forward_hip`'s sequence with each node-sized step an autograd.Function; the token-sized modules are ATen under autograd."""
        a1, a2 = self.attn1, self.attn2
        b, n, _ = x.shape
        heads = a1.heads
        dims = (b, n, heads, a1.to_q.weight.shape[0] // heads)
        kv, q2 = _SeqProj.apply(self, x, self.norm_seq.weight, self.norm_seq.bias, a1.to_kv.weight, a2.to_q.weight)
        tok = self.norm_queries(queries)
        induced = a1.to_out(_InducedCore.apply(a1.to_q(tok), kv, mask, dims, a1.scale))
        att = _TokenCore.apply(q2, a2.to_kv(induced), dims, a2.scale)
        x2 = _OutFF.apply(self, att, x, a2.to_out.weight, a2.to_out.bias, self.ff[0].weight, self.ff[0].bias,
                          self.ff[1].weight, self.ff[1].bias, self.ff[3].weight, self.ff[3].bias)
        return x2, induced + queries


# ---------------------------------------------------------------------------------------------- the backward's specification
def attn_core_torch(q, kv, mask, heads, scale):
    """The core of `Attention.forward` between its projections: q (B, nq, inner) attends over kv (B, nk, 2 inner) = [k | v]."""
    b, nq, inner = q.shape
    qh = q.view(b, nq, heads, -1).transpose(1, 2)
    k, v = kv.reshape(b, -1, 2, heads, inner // heads).permute(2, 0, 3, 1, 4)
    dots = (qh @ k.transpose(-1, -2)) * scale
    if mask is not None:
        dots = dots.masked_fill(~mask[:, None, None, :], -torch.finfo(dots.dtype).max)
    return (dots.softmax(dim=-1) @ v).transpose(1, 2).reshape(b, nq, inner)


def attn_core_backward_spec(g_o, q, kv, mask, heads, scale):
    """(d/d q, d/d kv) of `attn_core_torch` in closed form -- what egnn_induced_attn_bwd_f32 (nq = T tokens over the nodes, with mask)
    and egnn_token_attn_bwd_f32 (nq = the nodes over the T tokens, no mask) compute.  p = softmax(s), D = g_o . o,
    g_v = p^T g_o, g_s = p (g_o . v - D), g_k = scale g_s^T q, g_q = scale g_s k.  A masked logit is a constant (masked_fill): g_s = 0
    there; in a row whose mask is all False p is uniform, so g_v still flows."""
    b, nq, inner = q.shape
    dh = inner // heads
    qh = q.view(b, nq, heads, dh).transpose(1, 2)
    k, v = kv.reshape(b, -1, 2, heads, dh).permute(2, 0, 3, 1, 4)
    gh = g_o.view(b, nq, heads, dh).transpose(1, 2)
    s = (qh @ k.transpose(-1, -2)) * scale
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], -torch.finfo(s.dtype).max)
    p = s.softmax(dim=-1)                                # (max subtracted first: an all -max row comes out uniform)
    o = p @ v
    d = (gh * o).sum(dim=-1, keepdim=True)
    g_v = p.transpose(-1, -2) @ gh
    g_s = p * (gh @ v.transpose(-1, -2) - d)
    if mask is not None:
        g_s = g_s.masked_fill(~mask[:, None, None, :], 0.0)
    g_k = scale * (g_s.transpose(-1, -2) @ qh)
    g_q = scale * (g_s @ k)
    g_kv = torch.stack((g_k, g_v), dim=0).permute(1, 3, 0, 2, 4).reshape(b, -1, 2 * inner)
    return g_q.transpose(1, 2).reshape(b, nq, inner), g_kv


def gelu_backward_spec(g, z):
    """d/d z of the exact GELU z Phi(z): g (Phi(z) + z phi(z)) -- egnn_gelu_bwd_f32."""
    cdf = 0.5 * (1.0 + torch.erf(z * 0.7071067811865476))
    pdf = 0.3989422804014327 * torch.exp(-0.5 * z * z)
    return g * (cdf + z * pdf)


def layer_norm_backward_spec(g, x, gamma, eps):
    """(d/d x, d/d gamma, d/d beta) of LayerNorm over the last dimension of x (rows, dim) -- egnn_layer_norm_bwd_f32."""
    mean = x.mean(dim=-1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + eps)
    xh = (x - mean) * rstd
    gh = g * gamma
    g_x = (gh - gh.mean(dim=-1, keepdim=True) - xh * (gh * xh).mean(dim=-1, keepdim=True)) * rstd
    return g_x, (g * xh).sum(dim=0), g.sum(dim=0)


# ---------------------------------------------------------------------------------------------- autograd on the HIP kernels
def _twice(expr, inputs, g_outs):
    """A Function's backward under create_graph=True: its step re-evaluated as the ATen expression `expr` from the saved inputs
    themselves (not detached copies: the graph reaches the caller's tensors) and differentiated by autograd, as
    autograd._backward_twice does for the EGNN layer.  One gradient (or None) per input.  The expression reads each input through a
    view of its own and is differentiated with respect to those views: where one input is an ancestor of another (x of the attn2
    output in `_OutFF`) the gradient of the ancestor must be the partial one -- the rest arrives through the other input's node."""
    diff = [torch.is_tensor(t) and t.is_floating_point() and t.requires_grad for t in inputs]
    with torch.enable_grad():
        ins = [t.view_as(t) if d else t for t, d in zip(inputs, diff)]
        outs = expr(*ins)
        outs = outs if isinstance(outs, tuple) else (outs,)
        pairs = [(o, g) for o, g in zip(outs, g_outs) if g is not None and o.requires_grad]
        wrt = [t for t, d in zip(ins, diff) if d]
        grads = iter(torch.autograd.grad([o for o, _ in pairs], wrt, [g for _, g in pairs], create_graph=True, allow_unused=True)
                     if pairs and wrt else [None] * len(wrt))
    return tuple(next(grads) if d else None for d in diff)


class _SeqProj(torch.autograd.Function):
    """(kv, q2) = (attn1.to_kv, attn2.to_q)(norm_seq(x)): LayerNorm fused into the operand packing, two split-f16 GEMMs."""

    @staticmethod
    def forward(ctx, blk, x, gamma, beta, w_kv, w_q):
        from . import _ops
        b, n, dim = x.shape
        w = blk._packed()
        seq_hl = _ops.node_prep_hl(x.contiguous().view(b * n, dim), None, w["g_seq"], w["b_seq"], blk.norm_seq.eps, 0)
        kv = _ops.linear_hl(seq_hl, w["kv1"], w_kv.shape[0], name="attn_kv")
        q2 = _ops.linear_hl(seq_hl, w["q2"], w_q.shape[0], name="attn_q")
        ctx.blk = blk
        ctx.save_for_backward(x, gamma, beta, w_kv, w_q)
        return kv, q2

    @staticmethod
    def backward(ctx, g_kv, g_q2):
        from . import _ops
        x, gamma, beta, w_kv, w_q = ctx.saved_tensors
        blk = ctx.blk
        g_kv, g_q2 = _ops.aligned(g_kv), _ops.aligned(g_q2)
        if torch.is_grad_enabled():
            def expr(x, gamma, beta, w_kv, w_q):
                seq = torch.nn.functional.layer_norm(x, x.shape[-1:], gamma, beta, blk.norm_seq.eps).view(-1, x.shape[-1])
                return seq @ w_kv.t(), seq @ w_q.t()
            return (None,) + _twice(expr, (x, gamma, beta, w_kv, w_q), (g_kv, g_q2))
        b, n, dim = x.shape
        x2d = x.contiguous().view(b * n, dim)
        need = ctx.needs_input_grad
        with _ops.backward_status():
            w = blk._packed_t()
            seq = _ops.node_prep_f32(x2d, None, w["g_seq"], w["b_seq"], blk.norm_seq.eps, 0)
            g_kv, g_q2 = g_kv.contiguous(), g_q2.contiguous()
            # (max |.| of the three operands: launched together, one wait)
            hr = [_ops.absmax_async(t) for t in (g_kv, g_q2, seq)]
            xop = _ops.grad_tn_operand(seq, hr[2].floats()[0]) if (need[4] or need[5]) else None
            g_seq = g_wkv = g_wq = None
            for g, amax, wt, pos in ((g_kv, hr[0].floats()[0], "kv1T", 4), (g_q2, hr[1].floats()[0], "q2T", 5)):
                go = _ops.GradOperand(g, amax=amax)
                g_seq = _ops.grad_nn(go, w[wt], dim, residual=g_seq, name="bwd_attn_seq")
                if need[pos]:
                    g_w = _ops.grad_tn(go, seq, name="bwd_attn_seq_w", x_operand=xop)
                    g_wkv, g_wq = (g_w, g_wq) if pos == 4 else (g_wkv, g_w)
            g_x, g_gamma, g_beta = _ops.layer_norm_bwd(x2d, g_seq, w["g_seq"], blk.norm_seq.eps)
        return None, g_x.view(b, n, dim), g_gamma, g_beta, g_wkv, g_wq


class _InducedCore(torch.autograd.Function):
    """attn1's core: the T tokens attend over the (masked) nodes -- egnn_induced_attn_f32 / egnn_induced_attn_bwd_f32."""

    @staticmethod
    def forward(ctx, q, kv, mask, dims, scale):
        from . import _ops
        b, n, heads, dh = dims
        o = _ops.induced_attn(q, kv, mask, b, n, heads, dh, scale)
        ctx.dims, ctx.scale, ctx.mask = dims, scale, mask
        ctx.save_for_backward(q, kv, o)
        return o

    @staticmethod
    def backward(ctx, g_o):
        from . import _ops
        q, kv, o = ctx.saved_tensors
        b, n, heads, dh = ctx.dims
        g_o = _ops.aligned(g_o)
        if torch.is_grad_enabled():
            return _twice(lambda q, kv: attn_core_torch(q, kv.view(b, n, -1), ctx.mask, heads, ctx.scale), (q, kv), (g_o,)) + (None,) * 3
        g_q, g_kv = _ops.induced_attn_bwd(q, kv, ctx.mask, o, g_o, b, n, heads, dh, ctx.scale)
        return g_q, g_kv, None, None, None


class _TokenCore(torch.autograd.Function):
    """attn2's core: every node attends over the T induced tokens -- egnn_token_attn_f32 / egnn_token_attn_bwd_f32."""

    @staticmethod
    def forward(ctx, q, kv_tok, dims, scale):
        from . import _ops
        b, n, heads, dh = dims
        ctx.dims, ctx.scale = dims, scale
        ctx.save_for_backward(q, kv_tok)
        return _ops.token_attn(q, kv_tok, b, n, heads, dh, scale)

    @staticmethod
    def backward(ctx, g_att):
        from . import _ops
        q, kv_tok = ctx.saved_tensors
        b, n, heads, dh = ctx.dims
        g_att = _ops.aligned(g_att)
        if torch.is_grad_enabled():
            return _twice(lambda q, kv_tok: attn_core_torch(q.view(b, n, -1), kv_tok, None, heads, ctx.scale).view(b * n, -1),
                          (q, kv_tok), (g_att,)) + (None,) * 2
        g_q, g_kv = _ops.token_attn_bwd(q, kv_tok, g_att.contiguous(), b, n, heads, dh, ctx.scale)
        return g_q, g_kv, None, None


class _OutFF(torch.autograd.Function):
    """x1 = attn2.to_out(att) + x;  x2 = ff(x1) + x1 (LayerNorm, Linear, exact GELU, Linear).  Saved: att and x1; the backward
    recomputes the LayerNorm output and the 4 dim wide pre-activation by the forward's own GEMM (one more GEMM, no (B N, 4 dim)
    tensor kept between forward and backward)."""

    @staticmethod
    def forward(ctx, blk, att, x, w_o, b_o, gamma, beta, w1, b1, w2, b2):
        from . import _ops
        b, n, dim = x.shape
        w = blk._packed()
        x2d = x.contiguous().view(b * n, dim)
        x1 = _ops.linear_hl(_ops.split_f16(att), w["o2"], dim, w["bo2"], residual=x2d, name="attn_out")
        h_hl = _ops.node_prep_hl(x1, None, w["g_ff"], w["b_ff"], blk.ff[0].eps, 0)
        hid = _ops.linear_hl(h_hl, w["ff1"], 4 * dim, w["bf1"], act=2, out_f32=False, out_hl=True, name="attn_ff0")
        x2 = _ops.linear_hl(hid, w["ff2"], dim, w["bf2"], residual=x1, name="attn_ff1")
        ctx.blk = blk
        ctx.save_for_backward(att, x, w_o, b_o, gamma, beta, w1, b1, w2, b2, x1)
        return x2.view(b, n, dim)

    @staticmethod
    def backward(ctx, g_x2):
        from . import _ops
        *inputs, x1 = ctx.saved_tensors
        att, x, w_o, b_o, gamma, beta, w1, b1, w2, b2 = inputs
        blk = ctx.blk
        b, n, dim = x.shape
        g_x2 = _ops.aligned(g_x2)
        if torch.is_grad_enabled():
            def expr(att, x, w_o, b_o, gamma, beta, w1, b1, w2, b2):
                F = torch.nn.functional
                x1 = F.linear(att, w_o, b_o).view(b, n, dim) + x
                return F.linear(F.gelu(F.linear(F.layer_norm(x1, (dim,), gamma, beta, blk.ff[0].eps), w1, b1)), w2, b2) + x1
            return (None,) + _twice(expr, tuple(inputs), (g_x2,))
        need = ctx.needs_input_grad                      # (blk, att, x, w_o, b_o, gamma, beta, w1, b1, w2, b2)
        with _ops.backward_status():
            w = blk._packed_t()
            g2d = g_x2.contiguous().view(b * n, dim)
            h32 = _ops.node_prep_f32(x1, None, w["g_ff"], w["b_ff"], blk.ff[0].eps, 0) if need[7] else None
            # (max |.| of the operands that exist already: launched first, read behind the GEMM that is queued next -- one wait for all)
            hr_g, hr_att, hr_h = _ops.absmax_async(g2d), _ops.absmax_async(att), (_ops.absmax_async(h32) if need[7] else None)
            # the feed-forward's pre-activation again, by the forward's GEMM
            z = _ops.linear_hl(_ops.node_prep_hl(x1, None, w["g_ff"], w["b_ff"], blk.ff[0].eps, 0), w["ff1"], 4 * dim, w["bf1"],
                               name="bwd_attn_ff0")
            go = _ops.GradOperand(g2d, amax=hr_g.floats()[0], colsum=need[10])
            g_hid = _ops.grad_nn(go, w["ff2T"], 4 * dim, name="bwd_attn_ff1")
            hid, g_z, bits = _ops.gelu_bwd_(z, g_hid)
            amax_hid, amax_gz = _ops.HostRead(bits).floats()
            g_w2 = _ops.grad_tn(go, hid, name="bwd_attn_ff1_w", x_operand=_ops.grad_tn_operand(hid, amax_hid)) if need[9] else None
            g_b2 = go.colsum
            del go, hid, z, g_hid
            gz = _ops.GradOperand(g_z, amax=amax_gz, colsum=need[8])
            del g_z
            g_h = _ops.grad_nn(gz, w["ff1T"], dim, name="bwd_attn_ff0")
            g_x1, g_gamma, g_beta = _ops.layer_norm_bwd(x1, g_h, w["g_ff"], blk.ff[0].eps, add=g2d)      # + the residual's share
            hr_x1 = _ops.absmax_async(g_x1)              # (read behind the weight-gradient product queued next)
            g_w1 = _ops.grad_tn(gz, h32, name="bwd_attn_ff0_w", x_operand=_ops.grad_tn_operand(h32, hr_h.floats()[0])) if need[7] else None
            g_b1 = gz.colsum
            del gz, g_h, h32
            ga = _ops.GradOperand(g_x1, amax=hr_x1.floats()[0], colsum=need[4])
            g_att = _ops.grad_nn(ga, w["o2T"], att.shape[1], name="bwd_attn_out")
            g_wo = _ops.grad_tn(ga, att, name="bwd_attn_out_w", x_operand=_ops.grad_tn_operand(att, hr_att.floats()[0])) if need[3] else None
        return (None, g_att, g_x1.view(b, n, dim), g_wo, ga.colsum, g_gamma, g_beta, g_w1, g_b1, g_w2, g_b2)

"""Autograd support for the gfx950 EGNN layer (the reference is trained in practice,
denoise_sparse.py:70-78, and every op of egnn_pytorch.py:224-341 is differentiable).

Forward  = the HIP path (neighbour selection, fused edge pass, split-f16 GEMMs -- or the plain fp32 / float64 kernels for the layers
           that run there).  Nothing of size E x H is kept: the saved tensors are the inputs, the neighbour list, the projection table
           (node-level) and u (E x m), the output of edge_mlp's second Linear, which the forward edge kernel writes on the side when a
           graph is being recorded.
Backward, three paths:
  `_backward_native` -- fp32 (half / bfloat16 modules through an fp32 shadow), every shape the fused forward kernels cover (m_dim <= 64,
           coordinate dimension 1 .. 8, up to 16 per-edge scalars, with or without training-mode dropout):
             * behind u: node_norm / node_mlp on the split-f16 GEMMs (`_node_mlp_backward`), the per-edge chain (second SiLU, gate, masks,
               coors_mlp, CoorsNorm, clamp, coordinate update, pooling) on the route `_behind_u_route` names -- `_behind_u_standard`:
               egnn_edge_tail_bwd_f32 (csrc/edge_tail.hip, matrix cores) for m_dim <= 16 and 3-D coordinates; `_behind_u_closed`:
               egnn_edge_tail_exact_bwd_f32 (csrc/edge_exact_bwd.hip, one thread per edge) for wider heads / other coordinate
               dimensions; `tail_edge_backward` is their specification; `_behind_u_autograd`: autograd on E x m tensors (`layer_tail`),
               host tensors only  ->  gU, d/d (x_i - x_j) and those parameters' gradients.  `_backward_exact` takes the same routes
               (closed, or autograd beyond 64 channels).  The switches EGNN_BWD_TAIL_KERNEL, EGNN_BWD_TAIL_REDUCE, EGNN_TAIL_GENERIC and
               EGNN_BWD_DROP_NATIVE are retired;
             * the E x H work -- z = P_i + P_j + W_s s, a = SiLU(z), dz = (W2^T gU) SiLU'(z) and their contractions -- on
               egnn_edge_bwd_pass_f32 (csrc/edge_bwd.hip; `_edge_contract_fused`): one pass over the edges grouped by source node
               (d/d P_i, d/d W_s, d/d scalars) and one over the edges sorted by destination (d/d P_j, d/d W_2), everything recomputed
               and contracted in registers; heads wider than 16 channels: once per block of 16 channels (linear in gU;
               `_edge_contract_blocks`, the block an argument of `_ops.edge_bwd_pass`);
             * the node-level products -- d/d feats, d/d edge_mlp.0 (`_edge_mlp0_backward`), node_mlp -- on the forward's split-f16 GEMM
               (`_ops.grad_nn / grad_tn`); host tensors (the CPU tests) on matmuls;
             * d/d scalars -> coordinates and edge features (`_scalars_to_inputs`: the distance in closed form, else the scalars' own
               small graph, `_scalars_graph_backward`, which `_backward_exact` shares).
           Both native backwards start from one `_Start` record.  The four A/B switches of these steps (the distribution of the
           contractions over the two passes, library GEMMs, a recomputed projection table, the rounds per slab) are retired like the
           four above -- DESIGN.md section 10 names them: device or host is `is_cuda` alone.
  `_backward_exact` (round 5) -- the layers whose forward runs on the plain kernels (csrc/edge_exact.hip): float64 modules (the reference's
           own training recipe, denoise_sparse.py:11, 23-32), calls answered by the wide-range path (values beyond the split-fp16 range),
           more than 16 per-edge scalars / 8 coordinates / 64 message channels.  The per-edge tail in closed form (through autograd on
           E x m tensors beyond 64 channels), the E x H work on egnn_edge_exact_bwd_f32 / _f64 + egnn_edge_exact_node_sums_* (csrc/edge_exact_bwd.hip), every contraction on
           the exact GEMMs (egnn_linear_f32 / egnn_linear_f64), in the arithmetic of the forward.
  `_backward_recompute` -- what is left: more per-edge scalars than the exact backward keeps in LDS (80 in fp32, 40 in float64), EGNN_NATIVE_BACKWARD=0 /
           EGNN_NATIVE_BACKWARD_EXACT=0, CPU tensors (the tests); also the native paths' reference in the tests.  The whole layer
           re-evaluated a few graphs at a time as a differentiable chain of ATen ops over the neighbour list the HIP kernel selected,
           factorised like the forward, and differentiated by autograd.
Gradients of feats / coors / edges / every parameter agree with the reference's autograd (tests/test_autograd.py).  Every sum
over edges has a fixed order (partial rows + egnn_rows_gather_sum_f32, per-workgroup partials summed by index: no float
atomics) -- the native backward is bit-reproducible.

`layer_given_neighbors` is a restatement of egnn_pytorch.py:262-341 that takes the neighbour list as an input (the selection
itself, :237-260, is not differentiable: topk indices and the `<= valid_radius` comparison carry no gradient upstream
either).  It is also what the CPU tests compare with the reference, independently of the GPU.
"""
from __future__ import annotations

import os
from typing import Any, NamedTuple

import torch
from torch import nn

from .sparse_adj import SparseLabels

# EGNN_NATIVE_BACKWARD=0: always the pure-ATen recompute (the reference implementation of the backward)
_NATIVE_MODE = os.environ.get("EGNN_NATIVE_BACKWARD", "1")
_NATIVE = _NATIVE_MODE != "0"
_NATIVE_EXACT = os.environ.get("EGNN_NATIVE_BACKWARD_EXACT", "1") != "0"   # 0: float64 / wide-range / wide-shape layers on the recompute path
_EXACT_BWD_BYTES = int(float(os.environ.get("EGNN_EXACT_BWD_GB", "2")) * (1 << 30))   # budget of the a^T / dz^T tables per chunk of graphs
_FUSED_MAX_GRAPHS = 0                 # tests: force the chunking over graphs that very large batches need (0 = by size only)

# activations of the recompute per edge: a few E x H tensors (pre-activation, activation, gradients); 16 GB of the 288 GB
_BYTES_PER_EDGE_FACTOR = 5.0
_CHUNK_BUDGET_BYTES = 16 << 30


def _fourier(dist, num_encodings):
    """[sin(d / 2^k) (k < F), cos(d / 2^k) (k < F), d]  (egnn_pytorch.py:34-41)."""
    scales = 2.0 ** torch.arange(num_encodings, device=dist.device, dtype=dist.dtype)
    x = dist / scales                                        # (..., 1) / (F) -> (..., F)
    return torch.cat((x.sin(), x.cos(), dist), dim=-1)


def _tn(a, b):
    """a^T @ b for tall a (R, ca), b (R, cb): the contraction runs over the R rows and the output is small, so a single library
    GEMM leaves most of the 256 CUs idle (2.2 ms for 65536 x 2080 x 512, 1.8 ms for 2M x 64 x 16).  Split-K by hand: slabs of rows
    as a batched GEMM, partial products summed in fixed order (1.2 / 0.2 ms)."""
    r, ca = a.shape
    cb = b.shape[1]
    if not a.is_cuda or r < (1 << 14):
        return a.t() @ b
    tiles = ((ca + 127) // 128) * ((cb + 127) // 128)
    s = 1
    while s < 256 and tiles * s < 512 and r % (2 * s) == 0 and r // (2 * s) >= 512:
        s *= 2
    if s == 1:
        return a.t() @ b
    return torch.bmm(a.view(s, r // s, ca).transpose(1, 2), b.view(s, r // s, cb)).sum(dim=0)


class _TallLinear(torch.autograd.Function):
    """F.linear for per-edge inputs (millions of rows, a few dozen features): the weight gradient is a `_tn` product."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return torch.nn.functional.linear(x, w, b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1])
        gx = (g2 @ w).view_as(x) if ctx.needs_input_grad[0] else None
        gw = _tn(g2, x.reshape(-1, x.shape[-1])) if ctx.needs_input_grad[1] else None
        gb = g2.sum(dim=0) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return gx, gw, gb


def _per_edge(module, x):
    """module(x) for Sequentials of Linear / Dropout / SiLU / Sigmoid applied to very many rows -- the per-edge heads (edge_gate,
    coors_mlp) and the node-level node_mlp -- with the Linears' weight gradients computed by `_tn`."""
    if not x.is_cuda:
        return module(x)
    for sub in (module if isinstance(module, nn.Sequential) else [module]):
        if isinstance(sub, nn.Linear):
            x = _TallLinear.apply(x, sub.weight, sub.bias)
        else:
            x = sub(x)
    return x


def edge_scalars(layer, coors, edges, idx, edges_by_k=False):
    """rel = x_i - x_j and the per-edge scalars [fourier(d), d, e_ij] in the column order of edge_mlp.0.weight (:282-285).
    edges_by_k: `edges` are the (B,N,K,edge_dim) features of the selected pairs already (egnn_edge_features_gather_f32)."""
    b, n, _ = coors.shape
    if idx is None:
        rel = coors[:, :, None, :] - coors[:, None, :, :]                          # (B,N,N,C)
        e_ij = edges
    else:
        k = idx.shape[-1]
        bi = torch.arange(b, device=coors.device)[:, None, None]
        rel = coors[:, :, None, :] - coors[bi, idx]                               # (B,N,K,C)
        if edges is None or edges_by_k:
            e_ij = edges
        else:
            e_ij = torch.gather(edges, 2, idx[..., None].expand(b, n, k, edges.shape[-1]))
    dist = (rel ** 2).sum(dim=-1, keepdim=True)
    scal = _fourier(dist, layer.fourier_features) if layer.fourier_features > 0 else dist
    if e_ij is not None:
        scal = torch.cat((scal, e_ij), dim=-1)
    return rel, scal


def _mlp_drop(module, x, drop, site, rows):
    """A Linear -> Dropout -> SiLU -> Linear [-> SiLU] Sequential with its dropout given by the kernels' hash mask
    (drop = (p, seed); rows = the mask row of every leading index of x) instead of the module's own nn.Dropout."""
    from . import _dropout
    mods = list(module)
    h = _TallLinear.apply(x, mods[0].weight, mods[0].bias) if x.is_cuda else mods[0](x)
    h = _dropout.apply(h, drop[1], site, rows, drop[0])
    for sub in mods[2:]:
        h = _TallLinear.apply(h, sub.weight, sub.bias) if (isinstance(sub, nn.Linear) and h.is_cuda) else sub(h)
    return h


def _edge_rows(b, n, k, device, graph_offset):
    """global edge ids (b N K + i K + k) of a chunk of graphs that starts at graph `graph_offset`: (b, n, k) int64"""
    return (torch.arange(b * n * k, device=device) + graph_offset * n * k).view(b, n, k)


def _norm_twice(rel):
    """|rel| over the last dimension with finite derivatives of every order at rel = 0 (torch's norm has a NaN second derivative there:
    the self pair of every k-NN row).  Below sqrt(tiny) it is 0 -- inside CoorsNorm's clamp to eps, where the gradient is 0 either way."""
    sq = (rel * rel).sum(dim=-1, keepdim=True)
    tiny = torch.finfo(rel.dtype).tiny
    return torch.where(sq > tiny, sq.clamp(min=tiny).sqrt(), torch.zeros_like(sq))


def layer_tail(layer, feats, coors, u, rel, mask, idx, rank, valid_radius, drop=None, graph_offset=0, twice=False):
    """Everything of EGNN.forward behind the second Linear of edge_mlp (:183-341): u (B,N,K,m_dim) = edge_mlp[3](...) ->
    second SiLU, gate, masks, coors_mlp / CoorsNorm / clamp / coordinate update, pooling, node_norm + node_mlp + residual.
    drop = (p, seed): training-mode dropout with the kernels' hash masks (egnn_pytorch_amd/_dropout.py).
    twice: CoorsNorm's norm through `_norm_twice` (second-order autograd)."""
    from . import _dropout
    b = feats.shape[0]
    m_ij = layer.edge_mlp[4](u)
    if layer.edge_gate is not None:
        m_ij = m_ij * _per_edge(layer.edge_gate, m_ij)                            # (:289-290)

    pair_mask = None
    if mask is not None:                                                          # (:292-300) -- the radius / sparse-only cut
        if idx is None:                                                           # exists only together with `mask`
            pair_mask = mask[:, :, None] & mask[:, None, :]
        else:
            bi = torch.arange(b, device=feats.device)[:, None, None]
            pair_mask = mask[:, :, None] & mask[bi, idx] & (rank <= valid_radius)

    coors_out = coors
    if layer.coors_mlp is not None:
        if drop is not None:
            w = _mlp_drop(layer.coors_mlp, m_ij, drop, _dropout.SITE_COORS,
                          _edge_rows(b, m_ij.shape[1], m_ij.shape[2], m_ij.device, graph_offset)).squeeze(-1)
        else:
            w = _per_edge(layer.coors_mlp, m_ij).squeeze(-1)                      # (:303-304)
        if layer.norm_coors:                                                      # CoorsNorm (:67-77)
            norm = _norm_twice(rel) if twice else rel.norm(dim=-1, keepdim=True)
            rel = rel / norm.clamp(min=layer.coors_norm.eps) * layer.coors_norm.scale
        if pair_mask is not None:
            w = w.masked_fill(~pair_mask, 0.0)
        if layer.coor_weights_clamp_value is not None:
            c = layer.coor_weights_clamp_value
            w = w.clamp(min=-c, max=c)
        coors_out = (w[..., None] * rel).sum(dim=2) + coors                      # (:315)

    node_out = feats
    if layer.node_mlp is not None:
        if pair_mask is not None:
            m_ij = m_ij.masked_fill(~pair_mask[..., None], 0.0)
        if layer.m_pool_method == "mean":
            if pair_mask is not None:                                             # masked mean with safe_div (:13-16, :326-328)
                cnt = pair_mask.sum(dim=-1, keepdim=True).to(m_ij.dtype)
                m_i = m_ij.sum(dim=2) / cnt.clamp(min=1e-8)
                m_i = m_i.masked_fill(cnt == 0, 0.0)
            else:
                m_i = m_ij.mean(dim=2)
        else:
            m_i = m_ij.sum(dim=2)
        node_in = torch.cat((layer.node_norm(feats), m_i), dim=-1)
        if drop is not None:
            n_ = feats.shape[1]
            rows = (torch.arange(b * n_, device=feats.device) + graph_offset * n_).view(b, n_)
            node_out = _mlp_drop(layer.node_mlp, node_in, drop, _dropout.SITE_NODE, rows) + feats
        else:
            node_out = _per_edge(layer.node_mlp, node_in) + feats                 # (:335-337)
    return node_out, coors_out


def tail_edge_backward(layer, u, coors, idx, pair_mask, g_coors_out, g_msum):
    """The per-edge part of the backward of `layer_tail` in closed form (what csrc/edge_tail.hip evaluates one edge per lane;
    this torch version is its specification and the CPU tests' subject): given
        u (B,N,K,m) the output of edge_mlp's second Linear, g_coors_out (B,N,3) = d loss / d coors_out and
        g_msum (B,N,m) = d loss / d (sum over k of the pair-masked m_ij)  (sum pooling: d/d m_i; mean: that / count),
    returns d loss / d u (B,N,K,m), d loss / d rel (B,N,K,3; rel = x_i - x_j, without the distance path), and what the parameter
    gradients of coors_mlp / CoorsNorm are sums of: g_hid (E, 4m) = d/d (pre-activation of coors_mlp's SiLU), a3 (E, 4m) its
    activation, g_w (E,) = d/d (coors_mlp's output), g_scale (E,) the per-edge terms of d/d coors_norm.scale; with the edge gate
    (soft_edges, :289-290) also g_gate (E,) = d/d (the gate's pre-activation) and m0 = SiLU(u) next to the gated m.
    Covers: coordinate dimension 3; edge gate, masks, CoorsNorm, clamp as configured."""
    b, n, k, m = u.shape
    lin3, lin4 = layer.coors_mlp[0], layer.coors_mlp[3]
    w3, b3, w4, b4 = lin3.weight, lin3.bias, lin4.weight[0], lin4.bias[0]
    sg_u = torch.sigmoid(u)
    m0 = u * sg_u                                                               # SiLU(u)
    gate = layer.edge_gate is not None
    if gate:
        gw, gb = layer.edge_gate[0].weight[0], layer.edge_gate[0].bias[0]
        gt = torch.sigmoid(m0 @ gw + gb)[..., None]
        mm = m0 * gt                                                            # m_ij = SiLU(u) * sigmoid(gate(SiLU(u)))
    else:
        mm = m0
    hid = mm @ w3.t() + b3
    sg_h = torch.sigmoid(hid)
    a3 = hid * sg_h
    w = a3 @ w4 + b4                                                            # (B,N,K)
    if idx is None:
        rel = coors[:, :, None, :] - coors[:, None, :, :]
    else:
        bi = torch.arange(b, device=coors.device)[:, None, None]
        rel = coors[:, :, None, :] - coors[bi, idx]
    g_scale = None
    if layer.norm_coors:
        eps, scale = layer.coors_norm.eps, layer.coors_norm.scale
        rn = rel.norm(dim=-1, keepdim=True)
        den = rn.clamp(min=eps)
        relp = rel / den * scale
    else:
        relp = rel
    wm = w if pair_mask is None else w.masked_fill(~pair_mask, 0.0)
    c = layer.coor_weights_clamp_value
    wc = wm if c is None else wm.clamp(min=-c, max=c)
    g = g_coors_out[:, :, None, :]                                              # broadcast over k
    g_wc = (g * relp).sum(dim=-1)
    g_relp = wc[..., None] * g
    g_wm = g_wc if c is None else torch.where((wm >= -c) & (wm <= c), g_wc, torch.zeros_like(g_wc))
    g_w = g_wm if pair_mask is None else g_wm.masked_fill(~pair_mask, 0.0)
    g_a3 = g_w[..., None] * w4
    g_hid = g_a3 * (sg_h * (1 + hid * (1 - sg_h)))
    g_m = g_hid @ w3
    gm_pool = g_msum[:, :, None, :].expand(b, n, k, m)
    g_m = g_m + (gm_pool if pair_mask is None else gm_pool.masked_fill(~pair_mask[..., None], 0.0))
    g_gate = None
    if gate:
        g_s = (g_m * m0).sum(dim=-1, keepdim=True) * gt * (1 - gt)
        g_m = g_m * gt + g_s * gw
        g_gate = g_s.reshape(-1)
    g_u = g_m * (sg_u * (1 + u * (1 - sg_u)))
    if layer.norm_coors:
        dot = (g_relp * rel).sum(dim=-1, keepdim=True)
        g_scale = (dot / den).reshape(-1)
        g_rel = g_relp * (scale / den) - torch.where(rn >= eps, dot * scale / (den * den) * (rel / rn.clamp(min=1e-30)), torch.zeros_like(rel))
    else:
        g_rel = g_relp
    e = b * n * k
    return dict(g_u=g_u, g_rel=g_rel, g_hid=g_hid.reshape(e, -1), a3=a3.reshape(e, -1), g_w=g_w.reshape(e), g_scale=g_scale,
                m=mm.reshape(e, m), m0=m0.reshape(e, m), g_gate=g_gate)


def layer_given_neighbors(layer, feats, coors, edges, mask, idx, rank, valid_radius, factorised=True, drop=None, graph_offset=0,
                          edges_by_k=False, edge_hidden=False):
    """EGNN.forward (egnn_pytorch.py:262-341) for given neighbours.
    idx (B,N,K) int64 / rank (B,N,K): the selection of :258 (None, None = dense all-pairs, K = N).
    edges_by_k: `edges` are (B,N,K,edge_dim), the features of the selected pairs (see `edge_scalars`).
    Differentiable in feats, coors, edges and the parameters of `layer`.
    factorised: evaluate the first Linear of edge_mlp as (W_i h_i + b) + W_j h_j + W_s s_ij with the dim-wide products done
    once per node -- the same factorisation the HIP forward uses, 16x fewer flops than Linear(cat(...)) at
    the north-star shape, identical mathematics; False = the reference's literal cat + Linear.
    edge_hidden: the E x H block (first Linear, dropout, SiLU, second Linear) as `EdgeHidden`, twice differentiable without an E x H
    tensor in ATen -- what second-order autograd runs (`_backward_twice`)."""
    b, n, dim = feats.shape
    dense = idx is None
    rel, scal = edge_scalars(layer, coors, edges, idx, edges_by_k)
    if edge_hidden:
        # (x_i - x_i of a self pair is identically 0: written as a constant 0, so that CoorsNorm's 1 / eps Jacobian does not turn the
        # exact cancellation of its two terms into rounding noise -- what csrc/edge_tail.hip does at first order)
        own = (torch.eye(n, dtype=torch.bool, device=coors.device)[None] if dense else
               idx == torch.arange(n, device=coors.device)[None, :, None])
        rel = rel.masked_fill(own[..., None], 0.0)
        u = _edge_hidden_block(layer, feats, scal, idx, drop, graph_offset)
        return layer_tail(layer, feats, coors, u, rel, mask, idx, rank, valid_radius, drop, graph_offset, twice=True)
    lin = layer.edge_mlp[0]
    if factorised:
        w_i, w_j, w_s = lin.weight[:, :dim], lin.weight[:, dim:2 * dim], lin.weight[:, 2 * dim:]
        p_i = feats @ w_i.t() + lin.bias                                          # (B,N,H)
        p_j = feats @ w_j.t()
        bi = None if dense else torch.arange(b, device=feats.device)[:, None, None]
        z = p_i[:, :, None, :] + (p_j[:, None, :, :] if dense else p_j[bi, idx]) + scal @ w_s.t()
    else:
        bi = None if dense else torch.arange(b, device=feats.device)[:, None, None]
        feats_j = feats[:, None, :, :].expand(b, n, n, dim) if dense else feats[bi, idx]
        feats_i = feats[:, :, None, :].expand_as(feats_j)
        z = lin(torch.cat((feats_i, feats_j, scal), dim=-1))                      # (:287, first Linear)
    u = z
    if drop is not None:                                                          # (p, seed): the kernels' hash mask instead of nn.Dropout
        from . import _dropout
        u = _dropout.apply(u, drop[1], _dropout.SITE_EDGE, _edge_rows(b, u.shape[1], u.shape[2], u.device, graph_offset), drop[0])
        for mod in list(layer.edge_mlp)[2:4]:                                     # SiLU, Linear
            u = mod(u)
    else:
        for mod in list(layer.edge_mlp)[1:4]:                                     # dropout | Identity, SiLU, Linear
            u = mod(u)
    return layer_tail(layer, feats, coors, u, rel, mask, idx, rank, valid_radius, drop, graph_offset)


# ---------------------------------------------------------------------------------------------------------------------------------
# Second order (create_graph=True): the E x H block of `layer_given_neighbors` as a twice-differentiable op.  `EdgeHidden` computes
#     z = P_i[i] + P_j[j] + W_s s  ->  dropout  ->  SiLU  ->  Linear  ->  u (E, m)
# and its backward is `EdgeHiddenGrad`, whose forward is the block's first-order backward and whose backward (once_differentiable) is
# the second-order one.  On the device both run on csrc/edge_hidden.hip; on host tensors (the tests) they evaluate the closed forms
# below, which are the kernels' specification.  Per edge e = (b, i, k) with neighbour j; d = the dropout factor (hash mask / keep, or 1):
#     x = d (P_i[i] + P_j[j] + W_s s_e);  sig = sigmoid(x);  a = x sig
#     a1 = sig (1 + x (1 - sig))                      (SiLU')
#     a2 = sig (1 - sig) (2 + x (1 - 2 sig))          (SiLU'')
#     u_e = W2 a + b2
# First order, given gU_e:
#     g_a = W2^T gU_e;  dz_e = d a1 g_a
#     dP_i[n] = sum of dz_e over the edges leaving n;  dP_j[n] = over the edges arriving at n
#     dW_s = sum dz_e s_e^T;  ds_e = W_s^T dz_e;  dW2 = sum gU_e a_e^T;  db2 = sum gU_e
# Second order, given the cotangents Pbar_i, Pbar_j, Wbar_s, sbar, Wbar2, bbar2 of those six outputs:
#     v_e = Pbar_i[i] + Pbar_j[j] + Wbar_s s_e + W_s sbar_e
#     r_e = d (d a2 g_a v_e + a1 Wbar2^T gU_e)                           (d/d z_e)
#     d/d gU_e = W2 (d a1 v_e) + Wbar2 a_e + bbar2
#     d/d P_i[n] = sum of r_e leaving n;  d/d P_j[n] = sum of r_e arriving at n
#     d/d W_s = sum (r_e s_e^T + dz_e sbar_e^T);  d/d s_e = W_s^T r_e + Wbar_s^T dz_e
#     d/d W2 = sum gU_e (d a1 v_e)^T;  b2 gets nothing
# What the second-order graph keeps per layer: node tables, E x S and E x m tensors -- never E x H; the (H, E) tables of the kernels are
# transient, per chunk of graphs within _TWICE_BYTES.
_TWICE_BYTES = _EXACT_BWD_BYTES
_TWICE_MAX_GRAPHS = 0                 # tests: force the chunking over graphs (0 = by size only)
# the sums over all edges (d/d W_s, d/d W2) are taken per block of whole graphs of about this many edges and the blocks' partials summed
# at the end: the same bits whatever the chunking (the chunks are whole numbers of blocks)
_TWICE_BLOCK_EDGES = 1 << 16
_EDGE_HIDDEN_SPEC = False             # True: `_backward_twice` runs the block as its torch expression (tools/force_train_timing.py "aten")


def _edge_ends(idx, b, n, k, device):
    """(source row, neighbour row) (E,) int64 of every edge in the (B N, H) node tables; idx (B,N,K) or None (dense, K = N)"""
    src = torch.arange(b * n, device=device).repeat_interleave(k)
    base = (torch.arange(b, device=device) * n)[:, None, None]
    j = torch.arange(n, device=device)[None, None, :].expand(b, n, n) if idx is None else idx.long()
    return src, (base + j).reshape(-1)


def _edge_drop_factor(drop, e, h, dtype, device):
    """d (E, H): the forward's hash mask of edge_mlp's dropout (drop = (p, seed, first edge id)) times 1 / keep as the kernels hold it
    (an fp32 number); None without dropout"""
    if drop is None:
        return None
    from . import _dropout
    p, seed, eid0 = drop
    keep = _dropout.keep_mask(seed, _dropout.SITE_EDGE, torch.arange(e, device=device) + eid0, torch.arange(h, device=device), p)
    inv = float(torch.tensor(_dropout.inv_keep(p), dtype=torch.float32))
    return keep.to(dtype) * inv


def edge_hidden_torch(p_i, p_j, s, w_s, w2, b2, idx, drop, dims):
    """The block as a literal torch expression (differentiable by autograd to any order): u (E, m) from P_i, P_j (B N, H), s (E, S),
    W_s (H, S), W2 (m, H), b2 (m); idx (B,N,K) or None; drop = (p, seed, first edge id) or None; dims = (B, N, K)."""
    src, dst = _edge_ends(idx, *dims, p_i.device)
    z = p_i[src] + p_j[dst] + s @ w_s.t()
    d = _edge_drop_factor(drop, z.shape[0], z.shape[1], z.dtype, z.device)
    x = z if d is None else z * d
    return torch.nn.functional.silu(x) @ w2.t() + b2


def _silu_terms(p_i, p_j, s, w_s, idx, drop, dims):
    src, dst = _edge_ends(idx, *dims, p_i.device)
    z = p_i[src] + p_j[dst] + s @ w_s.t()
    d = _edge_drop_factor(drop, z.shape[0], z.shape[1], z.dtype, z.device)
    x = z if d is None else z * d
    sg = torch.sigmoid(x)
    om = 1 - sg
    return src, dst, (1.0 if d is None else d), x * sg, sg * (1 + x * om), sg * om * (2 + x * (1 - 2 * sg))


def edge_hidden_backward_spec(g_u, p_i, p_j, s, w_s, w2, idx, drop, dims):
    """First-order backward of the block in closed form -> (dP_i, dP_j, ds, dW_s, dW2, db2)."""
    src, dst, d, a, a1, _ = _silu_terms(p_i, p_j, s, w_s, idx, drop, dims)
    dz = d * a1 * (g_u @ w2)
    zeros = torch.zeros_like(p_i)
    return (zeros.index_add(0, src, dz), zeros.index_add(0, dst, dz), dz @ w_s, dz.t() @ s, g_u.t() @ a, g_u.sum(dim=0))


def edge_hidden_double_backward_spec(g_u, p_i, p_j, s, w_s, w2, idx, drop, dims, cot):
    """Second-order backward of the block in closed form: cot = the cotangents of (dP_i, dP_j, ds, dW_s, dW2, db2) ->
    (d/d gU, d/d P_i, d/d P_j, d/d s, d/d W_s, d/d W2)."""
    cpi, cpj, cs, cws, cw2, cb2 = cot
    src, dst, d, a, a1, a2 = _silu_terms(p_i, p_j, s, w_s, idx, drop, dims)
    g_a = g_u @ w2
    v = cpi[src] + cpj[dst] + s @ cws.t() + cs @ w_s.t()
    dz = d * a1 * g_a
    dav = d * a1 * v
    r = d * (d * a2 * g_a * v + a1 * (g_u @ cw2))
    zeros = torch.zeros_like(p_i)
    return (dav @ w2.t() + a @ cw2.t() + cb2, zeros.index_add(0, src, r), zeros.index_add(0, dst, r), r @ w_s + dz @ cws,
            r.t() @ s + dz.t() @ cs, g_u.t() @ dav)


def _eh_args(dims, lo, hi, p_i, p_j, s, w_s, w2, idx, drop):
    """egnn_edge_hidden_args for graphs [lo, hi): the node rows, edges and neighbour list of those graphs"""
    from . import _abi, _ops
    b, n, k = dims
    a = _abi.EdgeHiddenArgs()
    a.B, a.N, a.K, a.m_dim, a.H, a.S = hi - lo, n, k, w2.shape[0], w_s.shape[0], w_s.shape[1]
    a.idx = None if idx is None else idx[lo:hi].data_ptr()
    a.Pi, a.Pj = p_i[lo * n:hi * n].data_ptr(), p_j[lo * n:hi * n].data_ptr()
    a.s, a.Ws, a.W2 = s[lo * n * k:hi * n * k].data_ptr(), w_s.data_ptr(), w2.data_ptr()
    if drop is not None:
        _ops.set_drop(a, drop[:2], drop[2] + lo * n * k)
    return a


def _eh_plan(dims, h, tables, esz):
    """(graphs per chunk, graphs per contraction block): the chunks keep `tables` (H, E) tables within _TWICE_BYTES (a single graph whose
    tables alone exceed it is one chunk) and are whole numbers of blocks; the blocks depend on the shape and the budget only"""
    b, n, k = dims
    fit = max(1, min(b, int(_TWICE_BYTES // max(1, tables * n * k * h * esz))))     # graphs whose tables fit the budget (at least one)
    blk = max(1, min(fit, _TWICE_BLOCK_EDGES // max(1, n * k)))
    step = fit if _TWICE_MAX_GRAPHS <= 0 else min(fit, _TWICE_MAX_GRAPHS)
    return max(blk, step // blk * blk), blk


def _contig(*ts):
    return tuple(None if t is None else t.contiguous() for t in ts)


def _edge_hidden_fwd_gpu(p_i, p_j, s, w_s, w2, b2, idx, drop, dims):
    from . import _ops
    p_i, p_j, s, w_s, w2, b2, idx = _contig(p_i, p_j, s, w_s, w2, b2, idx)
    b, n, k = dims
    u = _ops.empty(b * n * k, w2.shape[0], dtype=p_i.dtype, device=p_i.device)
    if u.numel():
        a = _eh_args(dims, 0, b, p_i, p_j, s, w_s, w2, idx, drop)
        a.b2, a.u = b2.data_ptr(), u.data_ptr()
        _ops.edge_hidden("fwd", a, p_i.dtype)
    return u


def _edge_hidden_bwd_gpu(g_u, p_i, p_j, s, w_s, w2, idx, drop, dims, cot=None):
    """First order (cot None) -> (dP_i, dP_j, ds, dW_s, dW2, db2) or second order -> (d/d gU, d/d P_i, d/d P_j, d/d s, d/d W_s, d/d W2)
    on egnn_edge_hidden_bwd_* / _bwd2_*, per chunk of graphs: the per-node sums on egnn_edge_exact_node_sums_*, the sums over all edges
    on the exact GEMMs per block of graphs (partials summed at the end)."""
    from . import _ops
    g_u, p_i, p_j, s, w_s, w2, idx = _contig(g_u, p_i, p_j, s, w_s, w2, idx)
    second = cot is not None
    if second:
        cpi, cpj, cs, cws, cw2, cb2 = _contig(*(c.to(p_i.dtype) for c in cot))
    dt, dev = p_i.dtype, p_i.device
    b, n, k = dims
    h, sd = w_s.shape
    m = w2.shape[0]
    e = b * n * k
    g_pi, g_pj = torch.zeros_like(p_i), torch.zeros_like(p_i)
    g_s = torch.zeros(e, sd, dtype=dt, device=dev)
    g_gu = torch.zeros(e, m, dtype=dt, device=dev) if second else None
    step, blk = _eh_plan(dims, h, 3 if second else 2, 8 if dt == torch.float64 else 4)
    nb = (b + blk - 1) // blk
    p_ws = torch.zeros(nb, h, sd, dtype=dt, device=dev)
    p_w2 = torch.zeros(nb, m, h, dtype=dt, device=dev)
    if e:
        gu_t, s_t = g_u.t().contiguous(), s.t().contiguous()
        cs_t = cs.t().contiguous() if second else None
        for lo in range(0, b, step):
            hi = min(b, lo + step)
            ec, e0 = (hi - lo) * n * k, lo * n * k
            a = _eh_args(dims, lo, hi, p_i, p_j, s, w_s, w2, idx, drop)
            a.gU, a.g_s = g_u[e0:e0 + ec].data_ptr(), g_s[e0:e0 + ec].data_ptr()
            dz_t = _ops.empty(h, ec, dtype=dt, device=dev)
            a.DZ_T = dz_t.data_ptr()
            if second:
                dav_t, r_t = (_ops.empty(h, ec, dtype=dt, device=dev) for _ in range(2))
                a.cPi, a.cPj = cpi[lo * n:hi * n].data_ptr(), cpj[lo * n:hi * n].data_ptr()
                a.cs, a.cWs, a.cW2, a.cb2 = cs[e0:e0 + ec].data_ptr(), cws.data_ptr(), cw2.data_ptr(), cb2.data_ptr()
                a.g_gU, a.DAV_T, a.R_T = g_gu[e0:e0 + ec].data_ptr(), dav_t.data_ptr(), r_t.data_ptr()
                _ops.edge_hidden("bwd2", a, dt)
                node_t = r_t
            else:
                a_t = _ops.empty(h, ec, dtype=dt, device=dev)
                a.A_T = a_t.data_ptr()
                _ops.edge_hidden("bwd", a, dt)
                node_t = dz_t
            dl = _ops.dest_lists(None if idx is None else idx[lo:hi], hi - lo, n, k, dev)
            gpi, _, gpj, _ = _ops.edge_exact_node_sums(node_t, (hi - lo) * n, k, dl.order, dl.seg)
            g_pi[lo * n:hi * n], g_pj[lo * n:hi * n] = gpi, gpj
            for g0 in range(lo, hi, blk):
                c0, c1 = (g0 - lo) * n * k, (min(hi, g0 + blk) - lo) * n * k
                cols = slice(e0 + c0, e0 + c1)
                if second:                                           # d/d W_s = r^T s + dz^T sbar;  d/d W2 = gU^T (d a1 v)
                    t = _ops.linear_f32(r_t[:, c0:c1], s_t[:, cols], sd, c1 - c0, name="twice_dws")
                    _ops.linear_f32(dz_t[:, c0:c1], cs_t[:, cols], sd, c1 - c0, residual=t, out=p_ws[g0 // blk], name="twice_dws")
                    _ops.linear_f32(gu_t[:, cols], dav_t[:, c0:c1], h, c1 - c0, out=p_w2[g0 // blk], name="twice_dw2")
                else:                                                # d/d W_s = dz^T s;  d/d W2 = gU^T a
                    _ops.linear_f32(dz_t[:, c0:c1], s_t[:, cols], sd, c1 - c0, out=p_ws[g0 // blk], name="twice_dws")
                    _ops.linear_f32(gu_t[:, cols], a_t[:, c0:c1], h, c1 - c0, out=p_w2[g0 // blk], name="twice_dw2")
            del dz_t, node_t
    if second:
        return g_gu, g_pi, g_pj, g_s, p_ws.sum(dim=0), p_w2.sum(dim=0)
    return g_pi, g_pj, g_s, p_ws.sum(dim=0), p_w2.sum(dim=0), g_u.sum(dim=0)


class EdgeHidden(torch.autograd.Function):
    """u (E, m) = W2 SiLU(d (P_i[i] + P_j[j] + W_s s)) + b2, twice differentiable (the closed forms above).  Inputs: P_i, P_j (B N, H),
    s (E, S), W_s (H, S), W2 (m, H), b2 (m), idx int32 (B,N,K) or None (dense, K = N), drop = (p, seed, first edge id) or None,
    dims = (B, N, K)."""

    @staticmethod
    def forward(ctx, p_i, p_j, s, w_s, w2, b2, idx, drop, dims):
        ctx.save_for_backward(p_i, p_j, s, w_s, w2)
        ctx.meta = (idx, drop, dims)
        if not p_i.is_cuda:
            return edge_hidden_torch(p_i, p_j, s, w_s, w2, b2, idx, drop, dims)
        return _edge_hidden_fwd_gpu(p_i, p_j, s, w_s, w2, b2, idx, drop, dims)

    @staticmethod
    def backward(ctx, g_u):
        p_i, p_j, s, w_s, w2 = ctx.saved_tensors
        return EdgeHiddenGrad.apply(g_u, p_i, p_j, s, w_s, w2, *ctx.meta) + (None, None, None)


class EdgeHiddenGrad(torch.autograd.Function):
    """forward: the first-order backward of `EdgeHidden` -> (dP_i, dP_j, ds, dW_s, dW2, db2); backward: the second-order one
    (`EdgeHiddenGradGrad`: a third order raises)."""

    @staticmethod
    def forward(ctx, g_u, p_i, p_j, s, w_s, w2, idx, drop, dims):
        ctx.save_for_backward(g_u, p_i, p_j, s, w_s, w2)
        ctx.meta = (idx, drop, dims)
        if not g_u.is_cuda:
            return edge_hidden_backward_spec(g_u, p_i, p_j, s, w_s, w2, idx, drop, dims)
        return _edge_hidden_bwd_gpu(g_u, p_i, p_j, s, w_s, w2, idx, drop, dims)

    @staticmethod
    def backward(ctx, cpi, cpj, cs, cws, cw2, cb2):
        saved = ctx.saved_tensors
        if torch.is_grad_enabled():                  # (a graph of the second order: the primal operands behind the third-order guard)
            saved = _ThirdOrderGuard.apply(*saved)
        return EdgeHiddenGradGrad.apply(*saved, cpi, cpj, cs, cws, cw2, cb2, *ctx.meta) + (None, None, None)


class EdgeHiddenGradGrad(torch.autograd.Function):
    """The second-order backward of `EdgeHidden`: (gU, P_i, P_j, s, W_s, W2; the cotangents Pbar_i, Pbar_j, sbar, Wbar_s, Wbar2, bbar2) ->
    (d/d gU, P_i, P_j, s, W_s, W2).  It is linear in the cotangents; its derivative with respect to them (what
    torch.autograd.functional.hvp's double-backward trick asks for -- still second order) is the JVP of the first-order map F = EdgeHiddenGrad
    in the direction of the incoming gradients (gU', P_i', P_j', s', W_s', W2'):
        z' = P_i'[i] + P_j'[j] + W_s' s + W_s s';  dz' = d (d a2 g_a z' + a1 W2'^T gU) + d a1 W2^T gU'
        F' = (node sums of dz', dz' W_s + dz W_s', sum (dz' s^T + dz s'^T), sum (gU' a^T + gU (d a1 z')^T), sum gU')
    = this op with the cotangents (P_i', P_j', s', W_s', W2', 0) plus EdgeHiddenGrad with gU' -- both ops themselves, so the rule holds at
    every order it is asked at.  Its derivative with respect to the primal operands is a third derivative: those operands come through
    `_ThirdOrderGuard`, which raises when a gradient actually has to pass it."""

    @staticmethod
    def forward(ctx, g_u, p_i, p_j, s, w_s, w2, cpi, cpj, cs, cws, cw2, cb2, idx, drop, dims):
        saved, cot = (g_u, p_i, p_j, s, w_s, w2), (cpi, cpj, cs, cws, cw2, cb2)
        ctx.save_for_backward(*saved)
        ctx.meta = (idx, drop, dims)
        ctx.cb2_shape = cb2.shape
        if not g_u.is_cuda:
            return edge_hidden_double_backward_spec(*saved, idx, drop, dims, cot)
        return _edge_hidden_bwd_gpu(*saved, idx, drop, dims, cot=cot)

    @staticmethod
    def backward(ctx, d_gu, d_pi, d_pj, d_s, d_ws, d_w2):
        saved = ctx.saved_tensors
        g_u, p_i, p_j, s, w_s, w2 = saved
        zero = lambda t, like: torch.zeros_like(like) if t is None else t           # noqa: E731
        d_gu, d_pi, d_pj, d_s, d_ws, d_w2 = (zero(t, like) for t, like in zip((d_gu, d_pi, d_pj, d_s, d_ws, d_w2), saved))
        need = ctx.needs_input_grad
        cot_grads = (None,) * 6
        if any(need[6:12]):
            cb2_zero = torch.zeros(ctx.cb2_shape, dtype=w2.dtype, device=w2.device)
            jv = EdgeHiddenGradGrad.apply(*saved, d_pi, d_pj, d_s, d_ws, d_w2, cb2_zero, *ctx.meta)      # (_, dP_i', dP_j', ds', dW_s', dW2')
            fv = EdgeHiddenGrad.apply(d_gu, p_i, p_j, s, w_s, w2, *ctx.meta)                                  # terms linear in gU'
            cot_grads = (jv[1] + fv[0], jv[2] + fv[1], jv[3] + fv[2], jv[4] + fv[3], jv[5] + fv[4], fv[5])
        # the primal operands: a third derivative -- zeros here, handed to `_ThirdOrderGuard` (inputs of this op under a second-order graph),
        # which raises only if autograd needs a gradient through it
        primal = tuple(torch.zeros_like(t) if need[i] else None for i, t in enumerate(saved))
        return primal + cot_grads + (None, None, None)


class _ThirdOrderGuard(torch.autograd.Function):
    """Identity on the primal operands of `EdgeHiddenGradGrad`; its backward raises: a gradient through it is a third derivative.  (torch's
    once_differentiable hangs its error node on detached copies of the outputs, which torch.autograd.grad(..., inputs=...) prunes -- a
    third order would come out silently incomplete; this node stays connected to its inputs, so a third order reaches it and raises,
    while second-order products that differentiate only with respect to cotangents -- hvp's double-backward trick -- never visit it.)"""

    @staticmethod
    def forward(ctx, *ts):
        return tuple(t.clone() for t in ts)

    @staticmethod
    def backward(ctx, *grads):
        raise RuntimeError("egnn_pytorch_amd.EGNN is twice differentiable: a third-order derivative (through the edge MLP's E x H block, "
                           "autograd.EdgeHidden) is not supported; second-order products (torch.autograd.functional.hvp / vhp / hessian) are")


class _AlignedCotangent(torch.autograd.Function):
    """Identity on a gradient that `_backward_twice` returns; the cotangent a second backward sends into it enters the recorded graph
    contiguous and at a 16-byte boundary, in whatever layout it arrives (the second backward's share of `_ops.aligned`)."""

    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        from . import _ops
        return _ops.aligned(g)


def _edge_hidden_block(layer, feats, scal, idx, drop, graph_offset):
    """u (B,N,K,m) of `layer_given_neighbors` through `EdgeHidden`: the node tables P_i, P_j and the per-edge scalars in ATen, the
    E x H work in the op"""
    b, n, dim = feats.shape
    k = scal.shape[2]
    lin, lin2 = layer.edge_mlp[0], layer.edge_mlp[3]
    w_i, w_j, w_s = lin.weight[:, :dim], lin.weight[:, dim:2 * dim], lin.weight[:, 2 * dim:]
    p_i = (feats @ w_i.t() + lin.bias).reshape(b * n, -1)
    p_j = (feats @ w_j.t()).reshape(b * n, -1)
    s = scal.reshape(b * n * k, scal.shape[-1])                                  # (explicit widths: K = 0 has no elements)
    i32 = None if idx is None else idx.to(torch.int32).contiguous()
    dr = None if drop is None else (drop[0], drop[1], graph_offset * n * k)
    fn = edge_hidden_torch if (_EDGE_HIDDEN_SPEC or not edge_hidden_kernels_fit(s.shape[1], s.dtype)) else EdgeHidden.apply
    return fn(p_i, p_j, s, w_s, lin2.weight, lin2.bias, i32, dr, (b, n, k)).view(b, n, k, lin2.weight.shape[0])


def edge_hidden_kernels_fit(s_dim, dtype):
    """csrc/edge_hidden.hip keeps an edge's scalars, their cotangents and gradients in three LDS columns of 256 threads (at most 160 KB):
    up to 53 per-edge scalars in fp32, 26 in float64.  Wider layers run the block as its torch expression under autograd (`edge_hidden_torch`:
    E x H tensors in ATen)."""
    return 3 * s_dim * 256 * (8 if dtype == torch.float64 else 4) <= 160 * 1024


def _exact_active():
    from . import layer as _layer                         # (layer.py imports this module)
    return _layer.exact_active()


def _chunk_graphs(layer, n, k, batch):
    din = 2 * layer.dim + 2 * layer.fourier_features + 1 + layer.edge_dim
    per_graph = n * k * (2 * din) * 4.0 * _BYTES_PER_EDGE_FACTOR          # E x H pre-activation, activation, their gradients
    return max(1, min(batch, int(_CHUNK_BUDGET_BYTES // max(per_graph, 1.0))))


def _dropout_native_ok(layer):
    """Training-mode dropout on the native backward: the kernels that re-evaluate the forward's hash masks (egnn_edge_bwd_pass_f32 with
    drop_thr, the two tail kernels, egnn_silu_bwd_drop_f32) cover every shape of the fused forward kernels since round 5 -- heads up to 64
    channels, coordinate dimensions up to 8 (the generic tail kernel re-evaluates coors_mlp's mask), up to 16 per-edge scalars;
    EGNN_TAIL_SCALAR=1 (the per-lane tail kernel, which does not re-evaluate masks) sends the masked layer to the recompute path."""
    # (round 6: layers without coors_mlp / node_mlp -- update_coors=False / update_feats=False -- take the generic tail kernel, which
    # skips the absent module and its mask site; odd `dim`: egnn_silu_bwd_drop_f32 steps its (row, column) pair per element)
    # (behind u: one of the two kernel routes -- on the device the rule does not depend on the coordinate dimension)
    return (_behind_u_route(layer, layer.m_dim, 3, True, True) != ROUTE_AUTOGRAD
            and 2 * layer.fourier_features + 1 + layer.edge_dim <= 16 and os.environ.get("EGNN_TAIL_SCALAR", "0") != "1")


# ---------------------------------------------------------------------------------------------------------------------------
# Step 1 of `_backward_native` / `_backward_exact`, "behind u": everything downstream of edge_mlp's second Linear -- the pooled messages,
# node_norm and node_mlp, and the per-edge chain (second SiLU, gate, pair mask, coors_mlp, CoorsNorm, clamp, coordinate update).
# One rule says which of three routes a chunk of graphs takes (`_behind_u_route`), one function per route does it
# (`_behind_u_standard` / `_behind_u_closed` / `_behind_u_autograd`) and hands a `_BehindU` record to steps 2 and 3.
ROUTE_STANDARD = "standard"       # egnn_edge_tail_bwd_f32 (csrc/edge_tail.hip): pools, differentiates and sums its parameter gradients
ROUTE_CLOSED = "closed"           # egnn_edge_tail_exact_bwd_* (csrc/edge_exact_bwd.hip), parameter gradients on the exact GEMMs
ROUTE_AUTOGRAD = "autograd"       # `layer_tail` on E x m tensors, differentiated by autograd


def _behind_u_route(layer, m, cdim, on_device, native):
    """The route of step 1 for a layer of m message channels and cdim coordinates; on_device: the tensors are on the GPU; native:
    `_backward_native` asks (else `_backward_exact`).
      standard -- m <= 16, coors_mlp hidden width <= 64, 3-D coordinates, coors_mlp and node_mlp present; native only.  Also what host
                  tensors take (the tests, with `_ops.edge_tail_bwd` emulated): there without the kernel's own reductions;
      closed   -- m <= 64; on the native path only for device tensors (node_mlp runs on the split-f16 gradient GEMMs there);
      autograd -- what is left: wider heads, host tensors."""
    cm = layer.coors_mlp
    if native and cm is not None and layer.node_mlp is not None and m <= 16 and cm[0].weight.shape[0] <= 64 and cdim == 3:
        return ROUTE_STANDARD
    if m <= 64 and (not native or on_device):
        return ROUTE_CLOSED
    return ROUTE_AUTOGRAD


def _ops_mod():
    from . import _ops
    return _ops


# EGNNFunction's inputs ahead of the layer's parameters: (layer, order_hint, mask, adj, feats, coors, edges, lookup, tok_emb, deg_emb).
# The three backward paths see (and return) the layout without inputs 7 .. 9 -- (..., edges, *params) -- and EGNNFunction.backward
# adds the tables' gradients (ctx.table_grads) back in.
_NPRE = 10


def _need(ctx):
    """needs_input_grad in the layout of the backward paths: (layer, order_hint, mask, adj, feats, coors, edges, *params)"""
    need = ctx.needs_input_grad
    return need if not getattr(ctx, "table_inputs", False) else need[:7] + need[_NPRE:]


class _LookupGrads:
    """The gradients of an EdgeLookup's tables (EGNNFunction inputs 6, 8, 9) in the backward: per chunk of graphs `add` hands the
    edge columns of d loss / d per-edge scalars to egnn_edge_features_grad_f32 / _f64; the embedding gradients of the chunks are summed
    in chunk order, the dense float edges' rows are stored into a zeroed (B,N,N,d1) tensor.  Nothing else of size B N^2 is allocated.
    Everything is kept in the look-up's compute dtype (`dtype`: float64 for a float64 module) until `outputs` hands it back in the
    dtypes of the caller's tensors."""

    def __init__(self, ctx, b, n, device):
        self.ctx = ctx
        self.lookup = ctx.lookup
        self.dtype = self.lookup.dtype
        self.dtypes = ctx.table_dtypes
        need = ctx.needs_input_grad                         # (EGNNFunction's own layout: the tables are inputs 6, 8, 9)
        self.want = (bool(need[6]) and self.lookup.edges is not None, bool(need[8]), bool(need[9]))
        # (a SparseEdges first table: the gradient of its float values, (nnz, d1) -- every chunk stores into the one tensor, the
        # positions are absolute offsets)
        self.csr = self.lookup.csr is not None
        shape = tuple(self.lookup.edges.shape) if (self.csr and self.want[0]) else (b, n, n, self.lookup.d1)
        self.g_edges = torch.zeros(shape, dtype=self.dtype, device=device) if self.want[0] else None
        self.tok = self.deg = None

    @property
    def active(self):
        return any(self.want)

    def add(self, lo, hi, i32, n, k, g_rows):
        """graphs [lo, hi): i32 their neighbour list (None: dense), g_rows ((hi - lo) n k, >= width) rows whose first `width` columns are
        d loss / d the gathered features."""
        if not self.active or k == 0:
            return
        ge = None if self.g_edges is None else (self.g_edges if self.csr else self.g_edges[lo:hi])
        pos = self.ctx.csr_pos[lo:hi] if self.csr else None     # (the positions the forward's look-up found)
        t, d = _ops_mod().edge_features_grad(self.lookup.graphs(lo, hi), i32, hi - lo, n, k, g_rows, want_tok=self.want[1],
                                             want_deg=self.want[2], g_edges=ge, pos=pos)
        if t is not None:
            self.tok = t if self.tok is None else self.tok + t
        if d is not None:
            self.deg = d if self.deg is None else self.deg + d

    def outputs(self):
        """the gradient of the dense float edges (input 6, or None); those of tok_emb / deg_emb (inputs 8, 9) go to ctx.table_grads,
        where EGNNFunction.backward picks them up (the backward paths return the layout (..., edges, *params))"""
        live = self.lookup.live
        tables = []
        for on, g, w, dt in ((self.want[1], self.tok, live[1], self.dtypes[1]), (self.want[2], self.deg, live[2], self.dtypes[2])):
            tables.append((torch.zeros(w.shape, dtype=self.dtype, device=w.device) if g is None else g).to(dt) if on else None)
        self.ctx.table_grads = tuple(tables)
        return self.g_edges.to(self.dtypes[0]) if self.want[0] else None


class EGNNFunction(torch.autograd.Function):
    """forward: HIP kernels; backward: `_backward_native` / `_backward_exact` / `_backward_recompute` (module docstring)."""

    @staticmethod
    def forward(ctx, layer, order_hint, mask, adj_mat, feats, coors, edges, lookup, tok_emb, deg_emb, *params):
        # edges: a dense (B,N,N,edge_dim) tensor -- or, with `lookup` (layer.EdgeLookup), its dense float edges if it has any; tok_emb /
        # deg_emb: the embedding weights behind `lookup` (lookup.live), inputs here so that they receive gradients
        # the native backward computes in fp32 like the forward: float64 / bfloat16 / float16 modules and inputs pass through
        # the same boundary conversion (gradients are returned in the callers' dtypes)
        # training-mode dropout: the forward kernels draw their masks from a hash of (seed, site, row, unit); the backward re-evaluates
        # the same masks -- inside its kernels (`_dropout_native_ok`) or on the recompute path (egnn_pytorch_amd/_dropout.py)
        drop = None
        if layer.dropout_active():
            from . import _dropout
            drop = (layer.dropout_p, _dropout.draw_seed())
        # (every shape the fused forward kernels cover -- m_dim <= 64, coordinate dimension 1 .. 8, up to 16 scalars -- is native: the E x H
        # work and the per-edge chain behind u, which has its closed-form kernels for all of them)
        native = (_NATIVE and layer.m_dim <= 64 and coors.shape[-1] <= 8 and (drop is None or _dropout_native_ok(layer))
                  and 2 * layer.fourier_features + 1 + layer.edge_dim <= 16
                  and not layer.float64_kernels()            # (a float64 module: float64 forward kernels, `_backward_exact` in float64)
                  and not _exact_active())                   # (the wide-range re-run: plain-fp32 forward kernels, `_backward_exact`)
        # the layers that run on the plain kernels (csrc/edge_exact.hip) -- float64 modules, the wide-range re-run, shapes beyond the fused
        # kernels' limits -- have their own native backward (round 5: `_backward_exact`, csrc/edge_exact_bwd.hip)
        s_in = 2 * layer.fourier_features + 1 + layer.edge_dim
        f64 = layer.float64_kernels()
        exact_path = f64 or _exact_active() or s_in > 16 or coors.shape[-1] > 8 or layer.m_dim > 64
        exact_native = bool(_NATIVE_EXACT and exact_path and s_in <= (40 if f64 else 80) and feats.is_cuda)
        if native and feats.is_cuda:
            # a single graph beyond the backward kernels' 2^31-byte tables: said here, before the first launch (where only the
            # adjacency decides K, with K = 1: the projection table's bound holds for every K, `_backward_native` re-checks with the K it finds)
            use_nn = layer.num_nearest_neighbors > 0 or layer.only_sparse_neighbors
            k_known = feats.shape[1] if not use_nn else (1 if (adj_mat is not None and layer.only_sparse_neighbors) else layer.num_nearest_neighbors)
            check_fused_training_shape(layer, feats.shape[0], feats.shape[1], min(k_known, feats.shape[1]))
        with torch.no_grad():
            node_out, coors_out, order, idx, rank, valid_radius, u_pre, proj = layer._forward_hip_checked(
                feats, coors, edges if lookup is None else lookup, mask, adj_mat, order_hint, want_u=native or exact_native,
                drop_seed=None if drop is None else drop[1])
        ctx.drop = drop
        ctx.set_materialize_grads(False)
        ctx.exact_native = exact_native and u_pre is not None
        ctx.exact_dtype = torch.float64 if f64 else torch.float32
        use_nearest = layer.num_nearest_neighbors > 0 or layer.only_sparse_neighbors
        if use_nearest and idx is None:
            # neighbour path with K == 0 (only_sparse_neighbors and an empty adjacency): NO messages -- not the dense graph that
            # `idx is None` stands for everywhere else
            b, n = feats.shape[:2]
            idx = torch.empty(b, n, 0, dtype=torch.int32, device=feats.device)
            rank = torch.empty(b, n, 0, dtype=torch.float32, device=feats.device)
        ctx.lookup = lookup
        if lookup is not None:
            # the backward differentiates from the (B,N,K,edge_dim) features of the selected pairs, as the edge pass read them -- E x D,
            # not B N^2 D, in the look-up's compute dtype -- and hands d loss / d them to egnn_edge_features_grad_f32 / _f64 (`_LookupGrads`)
            b, n = feats.shape[:2]
            k = n if idx is None else idx.shape[-1]
            with torch.no_grad():
                edges = (_ops_mod().edge_features_gather(lookup, idx, b, n, k, with_pos=lookup.csr is not None) if k > 0 else
                         torch.empty(b, n, 0, lookup.width, dtype=lookup.dtype, device=feats.device))
            # (a SparseEdges first table: the position of every selected pair in its rows, kept for the gradient entry and `_lookup_rows`)
            ctx.csr_pos = None
            if lookup.csr is not None:
                edges, ctx.csr_pos = edges if k > 0 else (edges, torch.empty(b, n, 0, dtype=torch.int32, device=feats.device))
            ctx.table_dtypes = tuple(None if t is None else t.dtype for t in lookup.live)
        ctx.layer = layer
        ctx.has_u = u_pre is not None                    # (E, 16 ceil(m_dim / 16)) fp32: E x m, not E x H
        ctx.valid_radius = valid_radius
        ctx.has_edges = edges is not None
        ctx.edges_by_k = lookup is not None                  # (the saved `edges` are the gathered (B,N,K,D) features)
        none = feats.new_empty(0)
        ctx.save_for_backward(feats, coors, edges if edges is not None else none, mask if mask is not None else none,
                              idx if idx is not None else none, rank if rank is not None else none,
                              u_pre if u_pre is not None else none,
                              proj[0] if proj is not None else none)
        # the projection table as the forward's edge pass read it: P_i as (fp16 hi, fp16 lo) words when pi_split -- the backward turns
        # them into fp32 in place, once (a second backward over a retained graph finds them decoded)
        ctx.proj_words = bool(proj is not None and proj[1])
        ctx.flags = (mask is not None, idx is not None)
        # the backward reads the layer's parameters (and their packed images) as they are THEN: an in-place update between
        # forward and backward must fail like it does for any saved tensor
        ctx.param_versions = tuple(p._version for p in params)
        ctx.order = order
        # outputs must not alias the inputs of a custom Function
        if node_out is feats:
            node_out = feats.clone()
        if coors_out is coors:
            coors_out = coors.clone()
        return node_out, coors_out

    @staticmethod
    def backward(ctx, g_node, g_coors):
        # (set_materialize_grads(False): an output the loss does not depend on arrives as None, not as zeros)
        ctx.dead_outputs = (g_node is None, g_coors is None)
        if g_node is None and g_coors is None:
            return (None,) * (_NPRE + len(ctx.param_versions))
        for p, v in zip(ctx.layer.parameters(), ctx.param_versions):
            if p._version != v:
                raise RuntimeError("one of the variables needed for gradient computation has been modified by an inplace "
                                   "operation: a parameter of egnn_pytorch_amd.EGNN changed between forward and backward "
                                   f"(version {p._version}, expected {v})")
        ctx.table_inputs, ctx.table_grads = True, (None, None)
        # the cotangents in any layout -- the stride-0 one of `.sum()`, a view into the gradient of a torch.cat, a transposed one -- as
        # the kernels (and, bit for bit, ATen's reductions on the recompute paths) take them: contiguous, at a 16-byte boundary
        from . import _ops
        g_node, g_coors = _ops.aligned(g_node), _ops.aligned(g_coors)
        if torch.is_grad_enabled():                 # create_graph=True (also hvp / hessian): gradients that are functions themselves
            out = tuple(None if g is None else _AlignedCotangent.apply(g) for g in _backward_twice(ctx, g_node, g_coors))
            ctx.table_grads = tuple(None if g is None else _AlignedCotangent.apply(g) for g in ctx.table_grads)
        elif ctx.has_u:
            if getattr(ctx, "exact_native", False):
                out = _backward_exact(ctx, g_node, g_coors)
            else:
                with _ops.backward_status():        # range bits of these kernels go to the backward's status word
                    out = _backward_native(ctx, g_node, g_coors)
                out = _w2_in_range_or_recomputed(ctx, g_node, g_coors, out)
        else:
            out = _backward_recompute(ctx, g_node, g_coors)
        return tuple(out[:7]) + (None,) + ctx.table_grads + tuple(out[7:])


_W2_RANGE = 65504.0 / 64.0          # |SiLU(z)| that egnn_edge_bwd_pass_f32 carries for d/d W_2: fp16 x 2^6 (csrc/edge_bwd.hip: A_UP)
backward_reruns = 0                 # native backwards answered by `_backward_recompute` in this process (tests pin where that happens)
_warned_backward_rerun = False


def _silu_hidden_amax(ctx):
    """max |SiLU(z)| over the pairs as egnn_edge_bwd_pass_f32 evaluates them for d/d W_2 (z = W_i h_i + b + W_j h_j + W_s s; the scalars of
    pairs the masks remove read as 0; training-mode dropout: every unit taken as kept), one graph at a time.  Only called once a native
    backward has returned a non-finite d/d W_2."""
    layer = _f32_shadow(ctx.layer)
    feats, coors, edges, mask, idx32, rank = _unpack(ctx)
    feats, coors = feats.float(), coors.float()
    dim = feats.shape[-1]
    lin = layer.edge_mlp[0]
    w = lin.weight.detach()
    by_k = getattr(ctx, "edges_by_k", False)
    drop = getattr(ctx, "drop", None)
    amax = 0.0
    with torch.no_grad():
        for g in range(feats.shape[0]):
            i64 = None if idx32 is None else idx32[g:g + 1].long()
            e0 = None if edges is None else edges[g:g + 1].float()
            _, scal = edge_scalars(layer, coors[g:g + 1], e0, i64, by_k)
            pm = _pair_mask(None if mask is None else mask[g:g + 1], i64, None if rank is None else rank[g:g + 1], ctx.valid_radius)
            if pm is not None:
                scal = scal.masked_fill(~pm[..., None], 0.0)
            p_i = feats[g] @ w[:, :dim].t() + lin.bias.detach()
            p_j = feats[g] @ w[:, dim:2 * dim].t()
            z = p_i[:, None, :] + (p_j[None, :, :] if i64 is None else p_j[i64[0]]) + scal[0] @ w[:, 2 * dim:].t()
            if drop is not None:
                z = z / (1.0 - drop[0])
            amax = max(amax, float(torch.nn.functional.silu(z).abs().max()))
    return amax


def _w2_in_range_or_recomputed(ctx, g_node, g_coors, out):
    """The native backward's result -- or the same backward on `_backward_recompute` when d/d W_2 left the range of its kernel.
    egnn_edge_bwd_pass_f32 carries SiLU(z) as fp16 x 2^6 for d/d W_2 (up to 1023) where the forward carries it up to 65504: a layer whose
    forward is in range (a dense layer on 64 collinear nodes at unit spacing with xavier-scale weights: |x_i - x_j|^2 up to 3969,
    SiLU(z) ~ 1200) left an inf - inf there.  The trigger is exactly that: d/d W_2 non-finite (one word per chunk of graphs, read behind
    the pass like the max-|x| words: `_ops.HostRead`, no drained stream), finite incoming gradients, AND max |SiLU(z)| -- evaluated
    then -- beyond the range.  Any other non-finite value is returned as it is.  Like the forward's wide-range re-run: plain fp32
    arithmetic over the same neighbour list, several times slower, one warning per process, under the range word's rule
    (EGNN_RANGE_CHECK=sync, no stream capture); `backward_reruns` counts."""
    global _warned_backward_rerun, backward_reruns
    from . import _ops
    flags = getattr(ctx, "w2_finite", None)
    ctx.w2_finite = None
    if not flags or _ops.RANGE_CHECK != "sync" or torch.cuda.is_current_stream_capturing():
        return out
    if all(f.ints()[0] for f in flags):
        return out
    if any(g is not None and not bool(torch.isfinite(g).all()) for g in (g_node, g_coors)):
        return out                                    # (non-finite gradients came in: non-finite gradients go out, as in any autograd)
    if not _silu_hidden_amax(ctx) >= _W2_RANGE:
        return out                                    # (in range: not this limit's doing -- it surfaces)
    if not _warned_backward_rerun:
        _warned_backward_rerun = True
        import warnings
        warnings.warn("egnn_pytorch_amd: a backward left the range of the split-fp16 kernels (SiLU of edge_mlp's hidden layer beyond 1023) "
                      "and is being re-run in plain fp32 (several times slower; this warning is issued once).", RuntimeWarning, stacklevel=2)
    backward_reruns += 1
    ctx.table_grads = (None, None)
    return _backward_recompute(ctx, g_node, g_coors)


def _pair_mask(m0, i64, r0, valid_radius):
    """(B,N,K) bool: the pairs that pass the node masks and the radius (egnn_pytorch.py:292-300); None without a mask."""
    if m0 is None:
        return None
    if i64 is None:
        return m0[:, :, None] & m0[:, None, :]
    bi = torch.arange(m0.shape[0], device=m0.device)[:, None, None]
    return m0[:, :, None] & m0[bi, i64] & (r0 <= valid_radius)


def _pooled_messages(layer, u, m0, i64, r0, valid_radius):
    """(m_i, pair mask (B,N,K) bool or None, count or None) from u (B,N,K,m): egnn_pytorch.py:287-300, 319-333 on E x m tensors."""
    k = u.shape[2]
    pm = _pair_mask(m0, i64, r0, valid_radius)
    mm = torch.nn.functional.silu(u)
    if layer.edge_gate is not None:
        gl = layer.edge_gate[0]
        mm = mm * torch.sigmoid(mm @ gl.weight.detach().to(u.dtype)[0] + gl.bias.detach().to(u.dtype))[..., None]
    m_sum = (mm if pm is None else mm.masked_fill(~pm[..., None], 0.0)).sum(dim=2)
    m_i, cnt = _pooled(layer, m_sum, pm, k)
    return m_i, pm, cnt


def _mean_pool(x, cnt, k):
    """x over the number of pairs the masks keep per node, 0 where they keep none (safe_div: egnn_pytorch.py:13-16, :326-328); cnt
    None: all k pairs count.  Linear and diagonal, so its own adjoint: the summed messages forward, d loss / d m_i backward."""
    return (x / cnt.clamp(min=1e-8)).masked_fill(cnt == 0, 0.0) if cnt is not None else x / k


def _pooled(layer, m_sum, pm, k):
    """(m_i, cnt) from the per-node sums of the messages: m_pool_method "sum" or "mean" (cnt: the kept pairs per node (B,N,1), None
    without a mask or with "sum")"""
    if layer.m_pool_method != "mean":
        return m_sum, None
    cnt = None if pm is None else pm.sum(dim=-1, keepdim=True).to(m_sum.dtype)
    return _mean_pool(m_sum, cnt, k), cnt


def _node_mlp_backward_exact(layer, f2d, m_i, g_out, grads, drop=None, row0=0):
    """node_norm + node_mlp + residual (egnn_pytorch.py:196-201, 335-337) differentiated on the exact GEMMs (egnn_linear_f32 / _f64) in
    f2d's dtype: returns (d loss / d feats of this part (rows, dim), d loss / d m_i (rows, m)) and accumulates the parameter gradients.
    node_norm itself (a LayerNorm on node-level rows) goes through autograd.  drop = (p, seed), row0: training-mode dropout between the
    first Linear and its SiLU -- the forward's hash mask of node rows row0 .. (the torch twin of the kernels' hash, node-level)."""
    from . import _ops
    dt = f2d.dtype
    dim = f2d.shape[1]
    n0, n3 = layer.node_mlp[0], layer.node_mlp[3]
    with torch.enable_grad():
        fl = f2d.detach().requires_grad_(True)
        ln = layer.node_norm(fl)
    w5, w6 = n0.weight.detach().to(dt).contiguous(), n3.weight.detach().to(dt).contiguous()       # (2 dim, dim + m), (dim, 2 dim)
    node_in = torch.cat((ln.detach(), m_i.to(dt)), dim=-1).contiguous()
    kin, hid = node_in.shape[1], w5.shape[0]
    rows = f2d.shape[0]
    z1 = _ops.linear_f32(node_in, w5, hid, kin, bias=n0.bias.detach().to(dt).contiguous(), name="bwd_exact_node_mlp")
    dk = None
    if drop is not None:                                                       # z_d = z keep / (1 - p); d z_d / d z = keep / (1 - p)
        from . import _dropout
        dk = _dropout.apply(torch.ones_like(z1), drop[1], _dropout.SITE_NODE, torch.arange(row0, row0 + rows, device=z1.device), drop[0])
        z1 = z1 * dk
    sg = torch.sigmoid(z1)
    a1 = z1 * sg
    g_out = g_out.contiguous()
    g_a1 = _ops.linear_f32(g_out, w6.t().contiguous(), hid, dim, name="bwd_exact_node_mlp")                    # g_out W6
    g_z1 = g_a1 * (sg * (1 + z1 * (1 - sg)))
    if dk is not None:
        g_z1 = g_z1 * dk
    got = g_out.t().contiguous()
    grads[id(n3.weight)] += _ops.linear_f32(got, a1.t().contiguous(), hid, rows, name="bwd_exact_node_mlp")  # g_out^T a1
    grads[id(n3.bias)] += g_out.sum(dim=0)
    gzt = g_z1.t().contiguous()
    grads[id(n0.weight)] += _ops.linear_f32(gzt, node_in.t().contiguous(), kin, rows, name="bwd_exact_node_mlp")
    grads[id(n0.bias)] += g_z1.sum(dim=0)
    g_in = _ops.linear_f32(g_z1, w5.t().contiguous(), kin, hid, name="bwd_exact_node_mlp")                      # g_z1 W5
    g_f = g_out.clone()                                                        # the residual
    if ln.requires_grad:
        norm_params = [p for p in layer.node_norm.parameters() if p.requires_grad]
        tg = torch.autograd.grad([ln], [fl] + norm_params, [g_in[:, :dim].contiguous()], allow_unused=True)
        if tg[0] is not None:
            g_f += tg[0]
        for p, g in zip(norm_params, tg[1:]):
            if g is not None:
                grads[id(p)] += g
    return g_f, g_in[:, dim:].contiguous()


def _tail_closed_form(layer, u2d, c0, i32, pm, g_coors_chunk, g_msum, grads, dl, b, n, k, drop=None, eid0=0):
    """The per-edge chain behind u on egnn_edge_tail_exact_bwd_* (csrc/edge_exact_bwd.hip; `tail_edge_backward` is the specification)
    in u2d's dtype, its parameter gradients contracted on the exact GEMMs (the kernel leaves their operands transposed: the edges are the
    K dimension).  Returns gU (E, m) and d loss / d coors of this part (B, N, C): x_i - x_j reaches the coordinates at the source (sum
    over a node's K edges) and, negated, at the neighbour (fixed-order sum over the CSR lists)."""
    from . import _ops
    dt = u2d.dtype
    e, m = u2d.shape
    cm = layer.coors_mlp
    gate = None if layer.edge_gate is None else (layer.edge_gate[0].weight, layer.edge_gate[0].bias)
    norm = layer.norm_coors and cm is not None
    pm8 = None if pm is None else pm.contiguous().view(torch.uint8)
    out = _ops.edge_tail_exact(u2d, c0, i32, pm8, g_coors_chunk.reshape(b * n, -1), g_msum,
                               None if cm is None else cm[0].weight, None if cm is None else cm[0].bias,
                               None if cm is None else cm[3].weight, None if cm is None else cm[3].bias,
                               layer.coors_norm.scale if norm else None, layer.coors_norm.eps if norm else 0.0,
                               layer.coor_weights_clamp_value, gate, b, n, k, drop, eid0)
    one = lambda v: v.view(1, e)                                                # noqa: E731
    if cm is not None:
        grads[id(cm[0].weight)] += _ops.linear_f32(out["ghid_t"], out["mm_t"], m, e, name="bwd_exact_tail")           # g_hid^T m
        grads[id(cm[0].bias)] += out["ghid_t"].sum(dim=1)
        grads[id(cm[3].weight)] += _ops.linear_f32(one(out["g_w"]), out["a3_t"], 4 * m, e, name="bwd_exact_tail")    # g_w^T a3
        grads[id(cm[3].bias)] += out["g_w"].sum().reshape(1)
        if norm:
            grads[id(layer.coors_norm.scale)] += out["g_scale"].sum().reshape(1)
    if gate is not None:
        grads[id(gate[0])] += _ops.linear_f32(one(out["g_gate"]), out["m0_t"], m, e, name="bwd_exact_tail")           # g_gate^T m0
        grads[id(gate[1])] += out["g_gate"].sum().reshape(1)
    src, _, dst, _ = _ops.edge_exact_node_sums(out["g_rel_t"], b * n, k, dl.order, dl.seg)
    return out["gU"], (src - dst).view(b, n, -1)


class _Chunk:
    """Graphs [lo, hi) of one backward: the saved inputs (contiguous), the incoming cotangents, and the rows of d loss / d feats and
    d loss / d coors that the steps add their shares to."""

    def __init__(self, lo, hi, k, feats, coors, edges, mask, idx32, rank, g_node, g_coors, g_feats, g_coors_in):
        self.lo, self.hi, self.bc, self.n, self.k = lo, hi, hi - lo, feats.shape[1], k
        self.bn, self.ec = self.bc * self.n, self.bc * self.n * k
        self.f0, self.c0 = feats[lo:hi].contiguous(), coors[lo:hi].contiguous()
        self.e0 = None if edges is None else edges[lo:hi].contiguous()
        self.m0 = None if mask is None else mask[lo:hi]
        self.i32 = None if idx32 is None else idx32[lo:hi].contiguous()
        self.i64 = None if self.i32 is None else self.i32.long()
        self.r0 = None if rank is None else rank[lo:hi]
        self.g_node, self.g_coors = g_node[lo:hi], g_coors[lo:hi]
        self.g_feats, self.g_coors_in = g_feats[lo:hi], g_coors_in[lo:hi]


class _BehindU(NamedTuple):
    """What step 1 leaves for steps 2 and 3 (its shares of d/d feats, d/d coors and its parameter gradients are already added)."""
    g_u: torch.Tensor                   # d loss / d u, (E, m) -- or (E, pad_to)
    scal: torch.Tensor                  # the per-edge scalars (B,N,K,S): over the leaves c, e below unless closed_dist
    c: torch.Tensor                     # leaf copy of the chunk's coordinates ...
    e: Any                              # ... and of its edge features (None without), which `scal` is a graph over
    rel: Any = None                     # x_i - x_j per edge
    g_rel: Any = None                   # d loss / d (x_i - x_j) (E, 4) where the caller still has to take it to the coordinates
    closed_dist: bool = False           # the distance is the only scalar: the caller differentiates it in closed form, onto g_rel
    bias2: Any = None                   # column sums of gU (= d/d edge_mlp's last bias) where the kernel summed them
    gu_bits: Any = None                 # HostRead of the bits of max |gU| where the kernel found it
    pm: Any = None                      # the pair mask (B,N,K) bool (None: no mask, or not asked for)


def _scalars_graph(layer, ch, by_k, want_ge):
    """(c, e, rel, scal): the chunk's per-edge scalars as a small graph of their own over leaf copies of its coordinates and edge
    features -- d loss / d scalars goes back through it in the last step."""
    with torch.enable_grad():
        c = ch.c0.detach().requires_grad_(True)
        e = None if ch.e0 is None else ch.e0.detach().requires_grad_(want_ge)
        rel, scal = edge_scalars(layer, c, e, ch.i64, by_k)
    return c, e, rel, scal


def _scalars_graph_backward(ch, tail, g_scal, want_ge, g_edges):
    """Step 4 through `_scalars_graph`: d loss / d scalars (B,N,K,S) -> the chunk's rows of d/d coors (squared distance, fourier terms)
    and of d/d edges."""
    sg = torch.autograd.grad([tail.scal], [tail.c] + ([tail.e] if want_ge else []), [g_scal], allow_unused=True)
    if sg[0] is not None:
        ch.g_coors_in += sg[0]
    if want_ge and sg[1] is not None:
        g_edges[ch.lo:ch.hi] += sg[1]


def _self_pairs(ch):
    """(bc, N, K) bool: the pairs whose neighbour is the node itself (dense: the diagonal)"""
    me = torch.arange(ch.n, device=ch.c0.device)
    if ch.i64 is None:
        return (me[:, None] == me[None, :])[None].expand(ch.bc, ch.n, ch.n)
    return ch.i64 == me[None, :, None]


def _gu_rows(g_u, ec, m, pad_to):
    """gU as (E, m) rows; pad_to: as (E, pad_to) with zero pad channels (the fused passes take whole blocks of 16 channels)"""
    if pad_to is None:
        return g_u.reshape(ec, m).contiguous()
    out = torch.zeros(ec, pad_to, dtype=g_u.dtype, device=g_u.device)
    out[:, :m] = g_u.reshape(ec, m)
    return out


def _pad_cached(pads, name, shape, src):
    """the parameter (view) `src` zero padded to `shape` in fp32, made once per set of packed weights (`bwd_pads`: rebuilt whenever a
    parameter changes, so once per optimizer step)"""
    if name not in pads:
        t = torch.zeros(shape, dtype=torch.float32, device=pads["device"])
        t[tuple(slice(0, s) for s in src.shape)] = src
        pads[name] = t
    return pads[name]


def _behind_u_standard(layer, w, ch, u_all, grads, early, drop, valid_radius, by_k, want_ge):
    """Route "standard" (native only): the node-level modules from the pooled messages (egnn_edge_pool_f32; node_mlp on the split-f16
    GEMMs, `_node_mlp_backward`), the per-edge chain in closed form on egnn_edge_tail_bwd_f32, which also sums its parameter gradients
    -- `tail_edge_backward` is its specification.  Host tensors (the tests, `_ops.edge_tail_bwd` emulated): pooling, node_mlp and the
    sums over edges in ATen.  early: queues the launches that depend on the saved inputs only."""
    from . import _ops
    pads = w["bwd_pads"]
    bc, n, k, ec, m, s_in = ch.bc, ch.n, ch.k, ch.ec, layer.m_dim, w["S"]
    f0, c0 = ch.f0, ch.c0
    dev = f0.device
    on_device = f0.is_cuda               # (the kernels pool the messages and sum the parameter gradients' terms themselves; node_mlp on
                                         #  the split-f16 GEMMs.  Host tensors: ATen)
    with torch.no_grad():
        u16 = u_all[ch.lo:ch.hi].contiguous()
        pm = _pair_mask(ch.m0, ch.i64, ch.r0, valid_radius)
        pm8 = None if pm is None else pm.contiguous().view(torch.uint8)
        gate, mm_pre, mm = None, None, None
        if layer.edge_gate is not None:                                              # soft_edges (:289-290)
            gate = (_pad_cached(pads, "gw16", (16,), layer.edge_gate[0].weight.detach()[0]), layer.edge_gate[0].bias.detach().contiguous())
        if on_device:
            m_sum = _ops.edge_pool(u16, gate, pm8, bc, n, k)
        else:
            mm = torch.nn.functional.silu(u16)                                       # (bc, n, k, 16), columns >= m are 0
            if gate is not None:
                mm_pre = mm
                mm = mm_pre * torch.sigmoid(mm_pre @ gate[0] + gate[1])[..., None]
            m_sum = (mm if pm is None else mm.masked_fill(~pm[..., None], 0.0)).sum(dim=2)
        m_i, cnt = _pooled(layer, m_sum, pm, k)
        del m_sum
    with torch.enable_grad():
        f = f0.detach().requires_grad_(True)
        c = c0.detach().requires_grad_(True)
        e = None if ch.e0 is None else ch.e0.detach().requires_grad_(want_ge)
        closed_dist = s_in == 1                       # the distance is the only per-edge scalar: its backward in closed form (caller)
        rel = scal = None
        if closed_dist:
            if not on_device:                            # (on the device: x_i - x_j and the distance are by-products of the tail kernel)
                with torch.no_grad():
                    rel, scal = edge_scalars(layer, c0, None, ch.i64)
        else:
            rel, scal = edge_scalars(layer, c, e, ch.i64, by_k)                      # (only the scalars' graph is used by the caller)
    if on_device:
        g_f, g_mi = _node_mlp_backward(layer, w, f, m_i[..., :m], ch.g_node, grads, drop, ch.lo * n, overlap=early)
        ch.g_feats += g_f
    else:
        with torch.enable_grad():
            mi = m_i[..., :m].detach().requires_grad_(True)
            out_n = _per_edge(layer.node_mlp, torch.cat((layer.node_norm(f), mi), dim=-1)) + f      # (split-K weight gradients)
            # (only what requires grad may be differentiated: a frozen parameter in the list makes autograd.grad raise)
            node_params = [p for p in list(layer.node_norm.parameters()) + list(layer.node_mlp.parameters()) if p.requires_grad]
            tg = torch.autograd.grad([out_n], [f, mi] + node_params, [ch.g_node], allow_unused=True)
        if tg[0] is not None:
            ch.g_feats += tg[0]
        for p, g in zip(node_params, tg[2:]):
            if g is not None:
                grads[id(p)] += g
        g_mi = tg[1]
    with torch.no_grad():
        g_msum = torch.zeros(bc, n, 16, dtype=torch.float32, device=dev)
        if g_mi is not None:
            if layer.m_pool_method == "mean":
                g_mi = _mean_pool(g_mi, cnt, k)
            g_msum[..., :m] = g_mi
        lin_a, lin_b = layer.coors_mlp[0], layer.coors_mlp[3]
        hid3 = lin_a.weight.shape[0]
        w3p = _pad_cached(pads, "w3p", (64, 16), lin_a.weight.detach())
        b3p = _pad_cached(pads, "b3p", (64,), lin_a.bias.detach())
        w4p = _pad_cached(pads, "w4p", (64,), lin_b.weight.detach()[0])
        norm = layer.norm_coors
        tail_args = (u16, c0, ch.i32, pm8, ch.g_coors.contiguous(), g_msum, w3p, b3p, w4p, lin_b.bias.detach().contiguous(),
                     layer.coors_norm.scale.detach() if norm else None, layer.coors_norm.eps if norm else 0.0,
                     layer.coor_weights_clamp_value, bc, n, k)
        bias2 = gu_bits = None
        if on_device:
            gu16, g_rel, sums, rel4, dist, gu_bits = _ops.edge_tail_bwd(*tail_args, gate=gate, reduce=True, want_rel=closed_dist,
                                                                       drop=drop, eid0=ch.lo * n * k)
            gu_bits = _ops.HostRead(gu_bits)                              # (read in step 2, behind the small launches below)
            at = _ops.TAIL_SUMS
            grads[id(lin_a.weight)] += sums[at["W3"]].view(64, 16)[:hid3, :m]
            grads[id(lin_a.bias)] += sums[at["b3"]][:hid3]
            grads[id(lin_b.weight)] += sums[at["W4"]][:hid3][None, :]
            grads[id(lin_b.bias)] += sums[at["b4"]]
            if norm:
                grads[id(layer.coors_norm.scale)] += sums[at["scale"]]
            if gate is not None:
                grads[id(layer.edge_gate[0].weight)] += sums[at["gate_w"]][:m][None, :]
                grads[id(layer.edge_gate[0].bias)] += sums[at["gate_b"]]
            bias2 = sums[at["gU"]][:m]                                    # column sums of gU = d loss / d edge_mlp's last bias
            if closed_dist:
                rel, scal = rel4, dist.view(bc, n, k, 1)
        else:
            tail_out = _ops.edge_tail_bwd(*tail_args, gate=gate)
            gu16, g_rel, g_hid, a3, g_w, g_sc = tail_out[:6]
            if gate is not None:
                g_gate = tail_out[6]
                grads[id(layer.edge_gate[0].weight)] += _tn(g_gate[:, None], mm_pre.view(ec, 16))[:, :m]
                grads[id(layer.edge_gate[0].bias)] += g_gate.sum()[None]
            grads[id(lin_a.weight)] += _tn(g_hid, mm.view(ec, 16))[:hid3, :m]
            grads[id(lin_a.bias)] += g_hid.sum(dim=0)[:hid3]
            grads[id(lin_b.weight)] += _tn(g_w[:, None], a3)[:, :hid3]
            grads[id(lin_b.bias)] += g_w.sum()[None]
            if norm:
                grads[id(layer.coors_norm.scale)] += g_sc.sum()[None]
        ch.g_coors_in += ch.g_coors                                       # (the residual; g_rel reaches the coordinates in the caller)
        early()
    return _BehindU(gu16, scal, c, e, rel=rel, g_rel=g_rel, closed_dist=closed_dist, bias2=bias2, gu_bits=gu_bits, pm=pm)


def _behind_u_closed(layer, ch, u_all, grads, node_bwd, early, drop, valid_radius, by_k, want_ge, pad_to):
    """Route "closed": the pooled messages on E x m tensors, node_norm / node_mlp on node_bwd(ch, m_i, overlap) -> (d/d feats (bc, n,
    dim), d/d m_i (bc, n, m)), the per-edge chain in closed form on egnn_edge_tail_exact_bwd_* (one thread per edge; `_tail_closed_form`)
    with its parameter gradients on the exact GEMMs.  early() -> the chunk's destination lists, queueing them if the caller has not."""
    m, k = layer.m_dim, ch.k
    c, e, rel, scal = _scalars_graph(layer, ch, by_k, want_ge)
    with torch.no_grad():
        u4 = u_all[ch.lo:ch.hi, :, :, :m]
        m_i, pm, cnt = _pooled_messages(layer, u4, ch.m0, ch.i64, ch.r0, valid_radius)
        g_msum = None
        if layer.node_mlp is not None:
            g_f, g_mi = node_bwd(ch, m_i, early)
            ch.g_feats += g_f
            if layer.m_pool_method == "mean":
                g_mi = _mean_pool(g_mi, cnt, k)
            g_msum = g_mi.reshape(ch.bn, m).contiguous()
        else:
            ch.g_feats += ch.g_node                                       # (update_feats=False: node_out is feats)
        ch.g_coors_in += ch.g_coors                                       # the residual of the coordinate update
        dl = early()
        g_u, g_c = _tail_closed_form(layer, u4.reshape(ch.ec, m).contiguous(), ch.c0, ch.i32, pm, ch.g_coors, g_msum, grads, dl, ch.bc, ch.n,
                                     k, drop, ch.lo * ch.n * k)
        ch.g_coors_in += g_c
        g_u = _gu_rows(g_u, ch.ec, m, pad_to)
    return _BehindU(g_u, scal, c, e, rel=rel, pm=pm)


def _behind_u_autograd(layer, ch, u_all, grads, tail_params, drop, valid_radius, by_k, want_ge, pad_to, want_pm):
    """Route "autograd": `layer_tail` on E x m / node-level tensors, differentiated by autograd (heads wider than 64 channels; host
    tensors).  tail_params: the layer's parameters behind u."""
    m = layer.m_dim
    c, e, rel, scal = _scalars_graph(layer, ch, by_k, want_ge)
    with torch.enable_grad():
        f = ch.f0.detach().requires_grad_(True)
        u = u_all[ch.lo:ch.hi, :, :, :m].detach().requires_grad_(True)
        pm = _pair_mask(ch.m0, ch.i64, ch.r0, valid_radius) if want_pm else None
        rel_tail = rel
        if layer.norm_coors and layer.coors_mlp is not None:
            # A self pair (j == i) has rel = x_i - x_i: what CoorsNorm sends back through it reaches x_i once with each sign and cancels
            # identically, but each copy is scale / eps = 1e8 times the coordinate weight, and autograd's two sums left rounding noise of
            # that size in d/d coors (2.7e-2 of its maximum in fp32).  Taken out of the graph, as the closed-form kernels write it as zero.
            rel_tail = torch.where(_self_pairs(ch)[..., None], rel.detach(), rel)
        out_n, out_c = layer_tail(layer, f, c, u, rel_tail, ch.m0, ch.i64, ch.r0, valid_radius, drop=drop, graph_offset=ch.lo)
        outs, gouts = [], []
        for o, g in ((out_n, ch.g_node), (out_c, ch.g_coors)):
            if o.requires_grad:
                outs.append(o)
                gouts.append(g)
        live_tail = [p for p in tail_params if p.requires_grad]
        tg = torch.autograd.grad(outs, [u, f, c] + live_tail, gouts, allow_unused=True, retain_graph=True)
    if tg[1] is not None:
        ch.g_feats += tg[1]
    if tg[2] is not None:
        ch.g_coors_in += tg[2]
    for p, g in zip(live_tail, tg[3:]):
        if g is not None:
            grads[id(p)] += g
    return _BehindU(_gu_rows(tg[0] if tg[0] is not None else torch.zeros_like(u), ch.ec, m, pad_to), scal, c, e, rel=rel, pm=pm)


class _Start:
    """What `_backward_native` (dtype fp32) and `_backward_exact` (fp32 / float64) start from: the layer and the saved inputs in the
    compute dtype, the cotangents (zeros for an output nobody used), the zeroed gradient accumulators; `finish` hands them back."""

    def __init__(self, ctx, g_node, g_coors, dtype):
        self.ctx = ctx
        self.orig_params = list(ctx.layer.parameters())
        self.layer = layer = ctx.layer if dtype == torch.float64 else _f32_shadow(ctx.layer)     # (fp32: the layer itself unless it is a half module)
        feats, coors, edges, self.mask, self.idx32, rank = _unpack(ctx)
        self.in_dtypes = (feats.dtype, coors.dtype, None if edges is None else edges.dtype)
        self.feats, self.coors = feats, coors = feats.to(dtype), coors.to(dtype)
        self.edges = edges = None if edges is None else edges.to(dtype)
        self.rank = None if rank is None else rank.to(dtype)
        g_node = None if g_node is None else g_node.to(dtype)
        g_coors = None if g_coors is None else g_coors.to(dtype)
        self.k = self.idx32.shape[-1] if self.idx32 is not None else feats.shape[1]
        params = list(layer.parameters())
        head = {id(p) for p in layer.edge_mlp.parameters()}
        self.tail_params = [p for p in params if id(p) not in head]             # (the parameters behind u)
        # (one zero fill for all parameter gradients: views of a flat buffer)
        flat = torch.zeros(sum(p.numel() for p in params), dtype=dtype, device=feats.device)
        self.grads, off = {}, 0
        for p in params:
            self.grads[id(p)] = flat[off:off + p.numel()].view(p.shape)
            off += p.numel()
        self.g_feats, self.g_coors_in = torch.zeros_like(feats), torch.zeros_like(coors)
        self.by_k = getattr(ctx, "edges_by_k", False)
        self.lk = _LookupGrads(ctx, feats.shape[0], feats.shape[1], feats.device) if self.by_k else None     # (edge look-up tables: their gradients per chunk)
        # (the (B,N,N,edge_dim) input: its gradient only if somebody asked for it)
        self.want_ge = edges is not None and _need(ctx)[6] and not self.by_k
        self.g_edges = torch.zeros_like(edges) if self.want_ge else None
        self.g_node = torch.zeros_like(feats) if g_node is None else g_node
        self.g_coors = torch.zeros_like(coors) if g_coors is None else g_coors
        self.drop = getattr(ctx, "drop", None)              # (p, seed) of a training-mode forward: the same hash masks re-evaluated

    def chunk(self, lo, hi):
        return _Chunk(lo, hi, self.k, self.feats, self.coors, self.edges, self.mask, self.idx32, self.rank, self.g_node, self.g_coors,
                      self.g_feats, self.g_coors_in)

    def finish(self):
        return _returned_gradients(self.ctx, self.layer, self.orig_params, self.grads, self.g_feats, self.g_coors_in, self.g_edges, self.lk,
                                   self.in_dtypes)


def _returned_gradients(ctx, layer, orig_params, grads, g_feats, g_coors_in, g_edges, lk, in_dtypes):
    """The tuple a backward path returns, in the layout (layer, order_hint, mask, adj, feats, coors, edges, *params): every gradient
    in its owner's dtype, None where nobody asked or no output depends on the parameter (`_unused_params`)."""
    need = _need(ctx)
    unused = _unused_params(layer, ctx)
    out_params = [grads[id(p)].to(op.dtype) if (need[7 + i] and id(p) not in unused) else None
                  for i, (p, op) in enumerate(zip(layer.parameters(), orig_params))]
    return (None, None, None, None, g_feats.to(in_dtypes[0]) if need[4] else None, g_coors_in.to(in_dtypes[1]) if need[5] else None,
            lk.outputs() if lk is not None else (g_edges.to(in_dtypes[2]) if g_edges is not None else None), *out_params)


def _backward_exact(ctx, g_node, g_coors):
    """The backward of the layers that run on the plain kernels -- float64 modules (the reference's own training recipe,
    denoise_sparse.py:11, 23-32), calls answered by the wide-range path, shapes beyond the fused kernels' limits -- in the arithmetic of
    their forward (float64 / plain fp32), per chunk of graphs:
      1. behind u (saved by the forward kernel): the per-edge tail and the node-level modules, by `_behind_u_route` in closed form
         (`_behind_u_closed`, m_dim <= 64) or through autograd on E x m / node-level tensors (`_behind_u_autograd`)
         ->  gU = d loss / d u, their parameters' gradients, the tail's share of d/d feats, d/d coors;
      2. the E x H work on egnn_edge_exact_bwd_* (csrc/edge_exact_bwd.hip): z, a recomputed, dz = (W2^T gU) SiLU'(z); a^T, dz^T (H, E) and
         d/d scalars; the per-node sums of dz over outgoing / incoming edges on egnn_edge_exact_node_sums_* (fixed order);
      3. every contraction a C = X W^T product of egnn_linear_f32 / _f64 (exact v_mfma_f32 / v_mfma_f64): d/d W2 = gU^T a and
         d/d W_s = dz^T s with the edges as the contraction, d/d feats = dP_i W_i + dP_j W_j, d/d W_i, W_j = dP^T feats;
      4. d/d scalars -> coordinates / edge features through the scalars' own small graph (E x S).
    Nothing of size E x H is touched by ATen; what stays there is E x m / E x S / node-level element-wise work, as in `_backward_native`."""
    from . import _abi, _ops
    dtype = ctx.exact_dtype
    esz = 8 if dtype == torch.float64 else 4
    st = _Start(ctx, g_node, g_coors, dtype)
    layer, grads, drop, by_k, want_ge, lk, g_feats = st.layer, st.grads, st.drop, st.by_k, st.want_ge, st.lk, st.g_feats
    b, n, dim = st.feats.shape
    dev = st.feats.device
    k, m, cdim = st.k, layer.m_dim, st.coors.shape[-1]
    s_in = 2 * layer.fourier_features + 1 + layer.edge_dim
    lin0, lin3 = layer.edge_mlp[0], layer.edge_mlp[3]
    h = lin0.weight.shape[0]
    u_all = ctx.saved_tensors[6].view(b, n, k, m)
    proj = ctx.saved_tensors[7]                                           # (B N, 2 hq): [P_i incl. bias | P_j], what the forward's edge pass read
    hq = proj.shape[1] // 2
    w1 = lin0.weight.detach().to(dtype).contiguous()                      # (H, Din): [W_i | W_j | scalar columns]
    w2 = lin3.weight.detach().to(dtype).contiguous()                      # (m, H)
    w_it, w_jt = w1[:, :dim].t().contiguous(), w1[:, dim:2 * dim].t().contiguous()       # (dim, H): B operands of d/d feats
    step = max(1, min(b, int(_EXACT_BWD_BYTES // max(1, 2 * n * k * h * esz))))
    route = _behind_u_route(layer, m, cdim, st.feats.is_cuda, False)

    def node_bwd(ch, m_i, overlap):                                       # (node_mlp on the exact GEMMs, node-level rows)
        g_f, g_mi = _node_mlp_backward_exact(layer, ch.f0.view(ch.bn, dim), m_i.reshape(ch.bn, m), ch.g_node.reshape(ch.bn, dim), grads, drop,
                                             ch.lo * n)
        return g_f.view(ch.bc, n, dim), g_mi.view(ch.bc, n, m)
    for lo in range(0, b, step):
        hi_ = min(b, lo + step)
        ch = st.chunk(lo, hi_)
        bc, ec, bn, f0, c0, e0, i32 = ch.bc, ch.ec, ch.bn, ch.f0, ch.c0, ch.e0, ch.i32
        dl = _ops.dest_lists(i32, bc, n, k, dev)
        # ---- 1. behind u: in closed form (m_dim <= 64), else through autograd
        if route == ROUTE_CLOSED:
            tail = _behind_u_closed(layer, ch, u_all, grads, node_bwd, lambda: dl, drop, ctx.valid_radius, by_k, want_ge, None)
        else:
            tail = _behind_u_autograd(layer, ch, u_all, grads, st.tail_params, drop, ctx.valid_radius, by_k, want_ge, None, False)
        g_u, scal = tail.g_u, tail.scal
        with torch.no_grad():
            # ---- 2. the E x H work
            a_t = _ops.empty(h, ec, dtype=dtype, device=dev)
            dz_t = _ops.empty(h, ec, dtype=dtype, device=dev)
            g_scal = _ops.empty(ec, s_in, dtype=dtype, device=dev)
            a = _abi.EdgeExactBwdArgs()
            a.B, a.N, a.K, a.m_dim, a.H = bc, n, k, m, h
            a.fourier, a.edge_dim, a.coor_dim, a.edges_by_k = layer.fourier_features, layer.edge_dim, cdim, int(by_k)
            pc = proj[lo * n:hi_ * n]
            a.Pi, a.Pj, a.ldp = pc.data_ptr(), pc.data_ptr() + esz * hq, 2 * hq
            a.Ws, a.ldws = w1.data_ptr() + esz * 2 * dim, w1.shape[1]
            a.W2, a.coors, a.edges, a.idx = w2.data_ptr(), c0.data_ptr(), _ops._ptr(e0), _ops._ptr(i32)
            a.gU, a.A_T, a.DZ_T, a.g_scal = g_u.data_ptr(), a_t.data_ptr(), dz_t.data_ptr(), g_scal.data_ptr()
            _ops.set_drop(a, drop, lo * n * k)
            _ops.edge_exact_bwd(a, dtype)
            gpi, gpi_t, gpj, gpj_t = _ops.edge_exact_node_sums(dz_t, bn, k, dl.order, dl.seg)
            # ---- 3. the contractions, on the exact GEMMs
            grads[id(lin3.weight)] += _ops.linear_f32(g_u.t().contiguous(), a_t, h, ec, name="bwd_exact_dw2")        # (m, H) = gU^T a
            grads[id(lin3.bias)] += g_u.sum(dim=0)
            scal_t = scal.detach().reshape(ec, s_in).t().contiguous()                                               # (S, E)
            gw1 = grads[id(lin0.weight)]
            gw1[:, 2 * dim:] += _ops.linear_f32(dz_t, scal_t, s_in, ec, name="bwd_exact_dws")                        # (H, S) = dz^T s
            del a_t, dz_t
            f2d = f0.view(bn, dim)
            t = _ops.linear_f32(gpi, w_it, dim, h, name="bwd_exact_dfeats")                                          # dP_i W_i
            t = _ops.linear_f32(gpj, w_jt, dim, h, residual=t, name="bwd_exact_dfeats")                              # + dP_j W_j
            g_feats[lo:hi_] += t.view(bc, n, dim)
            f_t = f2d.t().contiguous()                                                                              # (dim, B N)
            gw1[:, :dim] += _ops.linear_f32(gpi_t, f_t, dim, bn, name="bwd_exact_dw1")                               # dP_i^T feats
            gw1[:, dim:2 * dim] += _ops.linear_f32(gpj_t, f_t, dim, bn, name="bwd_exact_dw1")
            grads[id(lin0.bias)] += gpi.sum(dim=0)
            del gpi, gpi_t, gpj, gpj_t, f_t
            if lk is not None:                                            # the edge columns of d/d scalars -> the tables
                lk.add(lo, hi_, i32, n, k, g_scal[:, s_in - layer.edge_dim:])
        # ---- 4. d loss / d scalars -> coordinates (squared distance, fourier terms) and edge features
        _scalars_graph_backward(ch, tail, g_scal.view_as(scal), want_ge, st.g_edges)
    return st.finish()


def _unused_params(layer, ctx=None):
    """ids of the parameters no output depends on -- node_norm without node_mlp (update_feats=False), CoorsNorm's scale without
    coors_mlp (update_coors=False; egnn_pytorch.py:302-306 applies it inside that branch): autograd leaves their .grad None in the
    reference, and so does this Function (an optimizer treats None and zeros differently: weight decay, state creation).  Likewise
    the parameters that reach the loss only through an output nobody used (ctx.dead_outputs: the last layer of a coordinate-denoising
    network -- denoise_sparse.py:70-72 -- never has its node_mlp / node_norm differentiated upstream)."""
    out = set()
    dead_node, dead_coors = getattr(ctx, "dead_outputs", (False, False)) if ctx is not None else (False, False)
    if layer.node_mlp is None or dead_node:
        out |= {id(p) for p in layer.node_norm.parameters()}
    if layer.coors_mlp is None or dead_coors:
        out |= {id(p) for p in layer.coors_norm.parameters()}
    if dead_node and layer.node_mlp is not None:
        out |= {id(p) for p in layer.node_mlp.parameters()}
    if dead_coors and layer.coors_mlp is not None:
        out |= {id(p) for p in layer.coors_mlp.parameters()}
    return out


def _unpack(ctx):
    """(feats, coors, edges, mask, idx, rank) as saved by the forward; the caller's own tensors among them -- saved as they came, so
    that a backward under create_graph=True reaches them -- contiguous and at a 16-byte boundary (`_ops.aligned`: under create_graph
    a differentiable clone), whatever their layout."""
    from . import _ops
    feats, coors, edges, mask, idx, rank = ctx.saved_tensors[:6]
    has_mask, has_idx = ctx.flags
    return (_ops.aligned(feats), _ops.aligned(coors), _ops.aligned(edges) if ctx.has_edges else None, mask if has_mask else None,
            idx if has_idx else None, rank if has_idx else None)


def _f32_shadow(layer):
    """The layer itself if its parameters are fp32, else an fp32 copy of it (cached per parameter version): the native backward
    differentiates in fp32 whatever dtype the module has, and hands the gradients back in the parameters' dtype."""
    from . import _weights
    if all(p.dtype == torch.float32 for p in layer.parameters()):
        return layer
    key = _weights.version_key(layer)
    cached = layer.__dict__.get("_shadow32")
    if cached is None or cached[0] != key:
        import copy
        packed, layer._packed = layer._packed, None          # (not the packed kernel weights, not an older shadow)
        layer.__dict__.pop("_shadow32", None)
        try:
            mod = copy.deepcopy(layer)
        finally:
            layer._packed = packed
        cached = (key, mod.float())
        layer.__dict__["_shadow32"] = cached
    return cached[1]


def _edge_tables(layer, w, f2d, pi_split):
    """fp32 P_i | P_j rows (incl. bias, in the forward's -log2(e) units) of the nodes in f2d: (rows, 2 Hp)."""
    from . import _ops
    hp = w["Hp"]
    feats_hl = _ops.split_f16(f2d)
    return _ops.linear_hl(feats_hl, w["Wcat_split"], 2 * hp, w["bcat"], name="bwd_node_proj", split_cols=hp if pi_split else 0)


def entry_list(eids, keys, n_keys):
    """The entry list of one egnn_edge_bwd_pass_f32 call (include/egnn_hip.h): edge ids `eids` (E,) ordered so that their keys
    `keys` (E,) -- the node each entry is grouped by -- are non-decreasing (None: E / n_keys consecutive entries per node).  Every
    node's entries are padded with -1 to whole
    16-entry tiles, the list to a multiple of 128.  Returns (ent int32 (L,), seg int64 (n_keys + 1,)): seg = the range of tiles
    (= partial rows) of each key."""
    dev = eids.device
    e = eids.numel()
    if keys is None:                                          # every key has the same number of consecutive entries (by source: K)
        per = e // n_keys
        t = (per + 15) // 16
        l = (n_keys * t * 16 + 127) // 128 * 128
        ent = torch.full((max(l, 128),), -1, dtype=torch.int32, device=dev)
        ent[:n_keys * t * 16].view(n_keys, t * 16)[:, :per] = eids.view(n_keys, per).to(torch.int32)
        return ent, torch.arange(n_keys + 1, device=dev) * t
    deg = torch.bincount(keys, minlength=n_keys)
    tiles = (deg + 15) // 16
    seg = torch.zeros(n_keys + 1, dtype=torch.int64, device=dev)
    torch.cumsum(tiles, 0, out=seg[1:])
    first = torch.zeros(n_keys + 1, dtype=torch.int64, device=dev)              # first entry of each key in the sorted list
    torch.cumsum(deg, 0, out=first[1:])
    pos = seg[:-1][keys] * 16 + (torch.arange(e, device=dev) - first[:-1][keys])
    l = (int(seg[-1]) * 16 + 127) // 128 * 128
    ent = torch.full((max(l, 128),), -1, dtype=torch.int32, device=dev)
    ent[pos] = eids.to(torch.int32)
    return ent, seg


def _edge_contract_fused(layer, w, f2d, c0, e0, sc2, i32, gu16, gu_scale, w_s, bc, n, k, pi_split, dest_lists=None, proj=None, drop=None, eid0=0,
                         block=0):
    """Step 2: egnn_edge_bwd_pass_f32 (csrc/edge_bwd.hip) twice -- entries grouped by source node, then by neighbour: z, SiLU(z) and dz
    are recomputed and contracted in registers, nothing of size E x H reaches memory.  The contractions over all edges ride along, each
    pass keeping its accumulators in registers: d/d W_s and d/d scalars by source, d/d W_2 by destination.  gu16: the (E, 16) columns of
    gU of message channels 16 block .. 16 block + 15.
    Returns d/d P_i (rows, Hp), d/d P_j (rows, Hp), d/d W_s (Hp, S), d/d scalars (E, S), d/d W_2 (16, Hp)."""
    from . import _ops
    dev = f2d.device
    on_device = dev.type == "cuda"                            # (the max |.| by-products: the scales of step 3's GEMM operands)
    ec = bc * n * k
    if proj is None:
        proj = _edge_tables(layer, w, f2d, False)
    # by source every node has ceil(K / 16) tiles: one IS the node's row, two (16 < K <= 32) are summed inside the kernel (row_pairs),
    # more go through the gather-sum
    ent, seg = entry_list(torch.arange(ec, device=dev), None, bc * n)
    blk = dict(block=block) if block else {}                  # (the first block is the pass's default: one block, the call of a 16-channel head)
    o = _ops.edge_bwd_pass(w, proj, i32, gu16, gu_scale, sc2, ent, bc, n, k, by_dest=False, ws_nat=w_s, want_w2=False, row_pairs=16 < k <= 32,
                           drop=drop, eid0=eid0, want_amax=k <= 32 and on_device, **blk)
    g_ws, g_scal = o["ws"], o["scal"]
    if k <= 32:
        gz_i = o["rows"][:bc * n]
        if o.get("amax_bits") is not None:
            gz_i.amax_bits = _ops.HostRead(o["amax_bits"])   # (max |d/d P_i| as a by-product of the pass; read behind THIS pass)
    else:
        gz_i = _ops.rows_gather_sum(o["rows"], torch.arange(o["rows"].shape[0], device=dev), seg, bc * n)
    del o, ent, seg                                           # (the by-source list is E words: not kept through the second pass)
    if dest_lists is None:
        dest_lists = _ops.dest_lists(i32, bc, n, k, dev)                 # (dense: destination = k)
    o = _ops.edge_bwd_pass(w, proj, i32, gu16, gu_scale, sc2, dest_lists.ent, bc, n, k, by_dest=True, ws_nat=None, want_w2=True,
                           drop=drop, eid0=eid0, **blk)
    ident = torch.arange(o["rows"].shape[0], device=dev)
    if on_device:
        gz_j, bits = _ops.rows_gather_sum(o["rows"], ident, dest_lists.tile_seg, bc * n, want_amax=True)
        gz_j.amax_bits = _ops.HostRead(bits)                  # (max |d/d P_j| as a by-product: the scale of its gradient GEMM operands)
    else:
        gz_j = _ops.rows_gather_sum(o["rows"], ident, dest_lists.tile_seg, bc * n)
    return gz_i, gz_j, g_ws, g_scal, o["w2"]


def _node_mlp_backward(layer, w, f, m_i, g_out, grads_by_id, drop=None, row0=0, overlap=None):
    """Backward of the node update out = node_mlp(cat(node_norm(f), m_i)) + f (egnn_pytorch.py:335-337) on the split-f16 GEMMs:
    the hidden pre-activation recomputed by the forward's GEMM, then per Linear one NN product (d/d input) and one split-K TN product
    (d/d weight) that share one (plain, transposed) split of the incoming gradient; SiLU and its derivative in one pass
    (egnn_silu_bwd_f32).  node_norm (LayerNorm or Identity, element-wise per node) stays with autograd.  f: (bc, n, dim) leaf that
    requires grad; m_i (bc, n, m); g_out (bc, n, dim).  Adds the parameter gradients into grads_by_id; returns (d/d f, d/d m_i).
    drop = (p, seed), row0: training-mode dropout behind the first Linear -- the forward's hash mask of node rows row0 .. is
    re-evaluated inside the SiLU-backward pass.  overlap: a callable that queues launches which do not depend on this function's results;
    called while the SiLU pass -- whose max |.| words the next operand scales are chosen from -- is still running (_ops.HostRead)."""
    from . import _ops
    bc, n, dim = f.shape
    m = m_i.shape[-1]
    rows = bc * n
    lin5, lin6 = layer.node_mlp[0], layer.node_mlp[3]
    with torch.enable_grad():
        ln = layer.node_norm(f)
    with torch.no_grad():
        in32 = torch.cat((ln.detach(), m_i), dim=-1).view(rows, dim + m)
        g2d = g_out.reshape(rows, dim).contiguous()
        # (max |.| of the two operands that exist already: launched first, read behind the GEMM that is queued next)
        hr_g, hr_in = _ops.absmax_async(g2d), _ops.absmax_async(in32)
        z1 = _ops.linear_hl(_ops.split_f16(in32), w["W5_split"], 2 * dim, w["b5"], name="bwd_node_mlp")        # (rows, 2 dim) pre-activation
        go = _ops.GradOperand(g2d, amax=hr_g.floats()[0], colsum=lin6.bias.requires_grad)   # (column sums = d/d bias: by-products of the split)
        g_a1 = _ops.grad_nn(go, w["W6T_split"], 2 * dim, name="bwd_node_mlp")
        if z1.numel() % 4 == 0:
            a1, g_z1, bits = _ops.silu_bwd_(z1, g_a1, drop, row0)
            bits = _ops.HostRead(bits)
            if overlap is not None:
                overlap()
            amax_a1, amax_gz = bits.floats()                            # (by-products of the pass: no absmax launches for these two)
        else:
            sg = torch.sigmoid(z1)
            a1, g_z1 = z1 * sg, g_a1 * (sg * (1 + z1 * (1 - sg)))
            amax_a1 = amax_gz = None
        if lin6.weight.requires_grad:
            grads_by_id[id(lin6.weight)] += _ops.grad_tn(go, a1, name="bwd_node_mlp_w", x_operand=_ops.grad_tn_operand(a1, amax_a1))
        if lin6.bias.requires_grad:
            grads_by_id[id(lin6.bias)] += go.colsum
        del go, a1
        gz = _ops.GradOperand(g_z1, amax=amax_gz, colsum=lin5.bias.requires_grad)
        g_in = _ops.grad_nn(gz, w["W5T_split"], dim + m, name="bwd_node_mlp")
        if lin5.weight.requires_grad:
            grads_by_id[id(lin5.weight)] += _ops.grad_tn(gz, in32, name="bwd_node_mlp_w", x_operand=_ops.grad_tn_operand(in32, hr_in.floats()[0]))
        if lin5.bias.requires_grad:
            grads_by_id[id(lin5.bias)] += gz.colsum
        del gz, g_z1
        g_ln = g_in[:, :dim].reshape(bc, n, dim)
        g_mi = g_in[:, dim:].reshape(bc, n, m)
    if ln is f:                                                   # node_norm = Identity
        return g_ln + g_out, g_mi
    ln_params = [p for p in layer.node_norm.parameters() if p.requires_grad]
    tg = torch.autograd.grad([ln], [f] + ln_params, [g_ln], allow_unused=True)
    for p, g in zip(ln_params, tg[1:]):
        if g is not None:
            grads_by_id[id(p)] += g
    return (tg[0] if tg[0] is not None else torch.zeros_like(g_out)) + g_out, g_mi


_I31 = 1 << 31


def _fused_entry_capacity(g, n, k):
    """the longest entry list one egnn_edge_bwd_pass_f32 call over g graphs is handed: egnn_dest_lists_capacity (csrc/entry_lists.hip)
    restated -- every destination wastes less than one 16-entry tile, the list is whole rounds of 128 entries; the by-source list
    (`entry_list`: ceil(K / 16) tiles per node) is never longer"""
    tiles = g * (n * k // 16 + n) + 8
    return (tiles * 16 + 127) // 128 * 128


def _fused_chunk_fits(g, n, k, hp):
    """what egnn_edge_bwd_pass_f32 (csrc/edge_bwd.hip) checks of a chunk of g graphs: E and L below 2^31, the (g N, 2 Hp) fp32
    projection table below 2^31 bytes, the (L / 16, Hp) fp32 partial rows below 2^31 bytes"""
    l = _fused_entry_capacity(g, n, k)
    return g * n * k < _I31 and l < _I31 and g * n * 2 * hp * 4 < _I31 and (l >> 4) * hp * 4 < _I31


def _fused_graphs_per_chunk(b, n, k, hp):
    """How many of the b graphs (N nodes, K neighbours, padded hidden width Hp) one chunk of `_backward_native` takes: the largest
    count, at most b, that `_fused_chunk_fits`; 0 when a single graph does not fit."""
    if b <= 0 or not _fused_chunk_fits(1, n, k, hp):
        return 0
    # (each bound is linear in the count up to the rounding of the entry list: start from the closed form, then settle exactly)
    g = min(b, (_I31 - 1) // (n * 2 * hp * 4), (_I31 - 1) // (n * k), (_I31 - 1) // ((n * k // 16 + n + 16) * hp * 4))
    g = max(1, g)
    while g > 1 and not _fused_chunk_fits(g, n, k, hp):
        g -= 1
    while g < b and _fused_chunk_fits(g + 1, n, k, hp):
        g += 1
    return g


class FusedBackwardLimit(NotImplementedError):
    """one graph is larger than the training kernels address"""


def _fused_largest_graph(k, hp):
    """the largest N for which one graph of K neighbours fits a chunk (`_fused_chunk_fits` is monotone in N: bisection)"""
    lo, hi = 0, _I31 // (2 * hp * 4) + 1                                    # (the P table's bound alone admits no more)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mid >= k and _fused_chunk_fits(1, mid, k, hp):
            lo = mid
        else:
            hi = mid - 1
    return lo


def _fused_limit_message(b, n, k, hp):
    most = _fused_largest_graph(k, hp)
    return (f"egnn_pytorch_amd: training a graph of {n} nodes (B = {b}, K = {k}, padded hidden width Hp = {hp}) is beyond the fused "
            f"backward kernels: one graph's projection table (N x 2 Hp fp32 = {n * 2 * hp * 4} bytes) and partial rows "
            f"({(n * k // 16 + n) * hp * 4} bytes) must each stay below 2^31 bytes (signed 32-bit offsets in egnn_edge_bwd_pass_f32), "
            f"at most {most} nodes per graph at this K and width.  Split the graph, or run it under torch.no_grad(): inference has no such limit.")


def check_fused_training_shape(layer, b, n, k):
    """Raise FusedBackwardLimit -- before anything is launched -- when a single graph of this shape does not fit the native backward."""
    from . import _abi
    hp = _abi.load().egnn_padded_hidden(2 * (2 * layer.fourier_features + 2 * layer.dim + layer.edge_dim + 1))
    if k > 0 and n > 0 and b > 0 and _fused_graphs_per_chunk(b, n, k, hp) == 0:
        raise FusedBackwardLimit(_fused_limit_message(b, n, k, hp))


# ---------------------------------------------------------------------------------------------------------------------------
# Steps 2 - 4 of `_backward_native`, "ahead of u": the E x H passes (`_edge_contract_blocks` over `_edge_contract_fused`), the node-level
# products of edge_mlp's first Linear (`_edge_mlp0_backward`), d/d scalars -> coordinates / edge features (`_scalars_to_inputs`).
def _edge_contract_blocks(layer, w, ch, tail, w_s, pi_split, dest_lists, proj, drop):
    """Step 2 for a chunk: `_edge_contract_fused` once per block of 16 message channels that holds real ones -- dz = (W2^T gU) SiLU'(z)
    and every contraction of it are linear in gU, so the blocks' results are added; d/d W_2 is per block anyway (m_dim 33 .. 48 has four
    blocks in u -- the forward's NB = 4 -- but the fourth is all padding: two passes that would add exact zeros, its rows of d/d W_2 are 0).
    Returns d/d P_i, d/d P_j (rows, Hp), d/d W_s (Hp, S), d/d scalars (E, S), d/d W_2 (blocks of u x 16, Hp)."""
    from . import _ops, _weights
    gu16, pm = tail.g_u, tail.pm
    amax = _ops.bits_to_floats(tail.gu_bits)[0] if tail.gu_bits is not None else _ops.absmax(gu16)
    gu_scale = _weights.pow2_scale(amax) if amax > 0 else 1.0
    nblk = (layer.m_dim + 15) // 16
    with torch.no_grad():
        sc2 = tail.scal.detach().reshape(ch.ec, w["S"])
        if pm is not None:
            # Pairs the masks remove carry gU = 0, so whatever z they have they add exact zeros -- as long as SiLU(z) is finite where
            # the pass holds it: as fp16 x 2^6 for d/d W_2, i.e. up to 1023.  A padded node's neighbours are the first K nodes wherever
            # they are, so its |x_i - x_j|^2 (and with it z) is not bounded by the real pairs': 0 x inf was a NaN in d/d W_2.  Their
            # scalars are read as 0 instead.
            sc2 = sc2.masked_fill(~pm.reshape(ch.ec, 1), 0.0)
        sc2 = sc2.contiguous()
        parts = [_edge_contract_fused(layer, w, ch.f0.view(ch.bn, -1), ch.c0, ch.e0, sc2, ch.i32,
                                      gu16 if nblk == 1 else gu16[:, 16 * blk:16 * blk + 16].contiguous(), gu_scale, w_s, ch.bc, ch.n, ch.k,
                                      pi_split, dest_lists, proj, drop, ch.lo * ch.n * ch.k, blk) for blk in range(nblk)]
        if nblk == 1:                                       # (the pass's own tensors, with their max |.| words)
            return parts[0]
        # (in this order: the sums' bits)
        gz_i, gz_j, g_ws, g_scal = (sum(p[q] for p in parts[1:]) + parts[0][q] for q in range(4))
        g_w2 = torch.cat([p[4] for p in parts] + [torch.zeros_like(parts[0][4])] * (gu16.shape[1] // 16 - nblk), dim=0)
    return gz_i, gz_j, g_ws, g_scal, g_w2


def _edge_mlp0_backward(layer, w, ch, gz_i, gz_j, g_ws, hr_f, grads):
    """Step 3, the node-level products of edge_mlp's first Linear from the per-node sums d/d P_i, d/d P_j (rows, Hp) and feats:
    d/d feats = dP_i W_i + dP_j W_j (added to the chunk's rows), d/d W_i = dP_i^T feats, d/d W_j = dP_j^T feats, d/d b_1 = column sums of
    dP_i; d/d W_s (Hp, S) goes to its columns.  Everything works on the contiguous (rows, Hp) buffers the kernel wrote, the weights zero
    padded to the kernel's hidden width Hp (slicing [:, :H] first would copy 17 GB per use at the north-star shape).  On the device:
    the forward's split-f16 matrix-core GEMM (operands pre-scaled by powers of two, the weight gradients split-K over the B N nodes with
    the parts summed in fixed order; hr_f: HostRead of max |feats|) -- the fp32 library GEMMs they replace ran at 60 - 130 TFLOP/s.  Host
    tensors (the CPU tests): plain matmuls."""
    from . import _ops
    lin0 = layer.edge_mlp[0]
    dim, h = ch.f0.shape[-1], w["H"]
    f2d = ch.f0.view(ch.bn, dim)
    gw1 = grads[id(lin0.weight)]
    with torch.no_grad():
        if f2d.is_cuda:
            # (each matrix: one absmax, one read for its plain and transposed images; feats^T split once for both weight gradients)
            # (launch order: everything of d/d P_i first -- its max |.| word was written by the by-source pass, long finished -- so that
            # the device is busy with it while the host waits for the word of d/d P_j, which the last kernel queued above writes)
            ib, jb = getattr(gz_i, "amax_bits", None), getattr(gz_j, "amax_bits", None)
            op_i = _ops.GradOperand(gz_i, amax=None if ib is None else _ops.bits_to_floats(ib)[0], colsum=True)
            gb1 = op_i.colsum
            t = _ops.grad_nn(op_i, w["WiT_split"], dim, name="bwd_dfeats")
            f_op = _ops.grad_tn_operand(f2d, None if hr_f is None else hr_f.floats()[0])
            gw1[:, :dim] += _ops.grad_tn(op_i, f2d, name="bwd_dw1", x_operand=f_op)[:h]
            del op_i
            op_j = _ops.GradOperand(gz_j, amax=None if jb is None else _ops.bits_to_floats(jb)[0])
            t = _ops.grad_nn(op_j, w["WjT_split"], dim, residual=t, name="bwd_dfeats")
            ch.g_feats += t.view(ch.bc, ch.n, dim)
            gw1[:, dim:2 * dim] += _ops.grad_tn(op_j, f2d, name="bwd_dw1", x_operand=f_op)[:h]
        else:
            pads, w1 = w["bwd_pads"], lin0.weight.detach()
            w_i = _pad_cached(pads, "w_i", (w["Hp"], dim), w1[:, :dim])
            w_j = _pad_cached(pads, "w_j", (w["Hp"], dim), w1[:, dim:2 * dim])
            ch.g_feats += (gz_i @ w_i + gz_j @ w_j).view(ch.bc, ch.n, dim)
            gw1[:, :dim] += _tn(gz_i, f2d)[:h]
            gw1[:, dim:2 * dim] += _tn(gz_j, f2d)[:h]
            gb1 = gz_i.sum(dim=0)
        gw1[:, 2 * dim:] += g_ws[:h]
        grads[id(lin0.bias)] += gb1[:h]


def _scalars_to_inputs(ch, tail, g_scal, dest_lists, want_ge, g_edges):
    """Step 4: d loss / d scalars (B,N,K,S) -> coordinates (through d = |x_i - x_j|^2 and the fourier terms) and edge features: onto
    step 1's d loss / d (x_i - x_j) in closed form where the distance is the only scalar, else through the scalars' own small graph;
    then d loss / d (x_i - x_j), where step 1 left it to the caller, to the coordinates at both ends."""
    from . import _ops
    g_rel, rel, bc, n, k = tail.g_rel, tail.rel, ch.bc, ch.n, ch.k
    if tail.closed_dist:
        with torch.no_grad():                                   # d = |rel|^2:  d loss / d rel += 2 g_d rel
            if rel.shape[-1] == 4:                              # (the tail kernel's (E, 4) rows, 4th column 0)
                g_rel.addcmul_(g_scal.reshape(ch.ec, 1), rel, value=2.0)
            else:
                g_rel[:, :3] += (2.0 * g_scal.reshape(ch.ec, 1)) * rel.reshape(ch.ec, 3)
    else:
        _scalars_graph_backward(ch, tail, g_scal, want_ge, g_edges)
    if g_rel is not None:
        # rel = x_i - x_j reaches the coordinates at the source (sum over a node's edges) and, negated, at the neighbour
        # (fixed-order gather over the edges sorted by destination)
        with torch.no_grad():
            ch.g_coors_in += g_rel.view(bc, n, k, 4).sum(dim=2)[..., :3]
            if ch.i64 is None:
                ch.g_coors_in -= g_rel.view(bc, n, n, 4).sum(dim=1)[..., :3]
            else:
                ch.g_coors_in -= _ops.rows_gather_sum(g_rel, dest_lists.order, dest_lists.seg, bc * n).view(bc, n, 4)[..., :3]


def _backward_native(ctx, g_node, g_coors):
    """The backward on the HIP kernels (module docstring), per chunk of graphs:
       1. behind u = ctx.u_pre (edge_mlp's second Linear, written by the forward kernel), on the route `_behind_u_route` names:
          `_behind_u_standard` (the pooled messages on egnn_edge_pool_f32, node_mlp on the split-f16 GEMMs, the per-edge chain in closed
          form on egnn_edge_tail_bwd_f32, which also sums its parameter gradients), `_behind_u_closed` (wider heads, other coordinate
          dimensions: egnn_edge_tail_exact_bwd_f32) or `_behind_u_autograd` (`layer_tail`: host tensors)
          ->  gU = d loss / d u, d loss / d (x_i - x_j), those modules' parameter gradients;
       2. the E x H work on egnn_edge_bwd_pass_f32 (`_edge_contract_blocks`: by source and by destination, everything recomputed and
          contracted in registers, once per block of 16 message channels)
          ->  d/d P_i, d/d P_j per node, d/d W_s, d/d scalars, d/d W_2;
       3. the node-level products of edge_mlp's first Linear (`_edge_mlp0_backward`): d/d feats, d/d W_i, W_j, b_1 from the per-node sums
          and feats;
       4. d/d scalars -> coordinates (closed form when the distance is the only scalar, the scalars' own small graph otherwise) and edge
          features (`_scalars_to_inputs`).
    Every sum over edges has a fixed order.  Chunks: the kernels' tables stay below 2 GB (signed 32-bit offsets): `_fused_graphs_per_chunk`."""
    from . import _ops, _weights
    w = ctx.layer.packed_weights()
    st = _Start(ctx, g_node, g_coors, torch.float32)
    layer, grads, drop, by_k, want_ge = st.layer, st.grads, st.drop, st.by_k, st.want_ge
    b, n, dim = st.feats.shape
    k, m, h, hp, s_in = st.k, layer.m_dim, w["H"], w["Hp"], w["S"]
    dev = st.feats.device
    on_device = dev.type == "cuda"                       # (host tensors -- the CPU tests -- take the ATen body of every step)
    lin0, lin3 = layer.edge_mlp[0], layer.edge_mlp[3]
    mp = 16 * _weights.m_blocks(m)                       # u rows: whole 16-channel blocks, pad channels 0
    u_all = ctx.saved_tensors[6].view(b, n, k, mp)
    proj_all = None
    if len(ctx.saved_tensors) > 7 and ctx.saved_tensors[7].numel():
        proj_all = ctx.saved_tensors[7]                                   # (B N, 2 Hp): what the forward's edge pass read (P_i still as
                                                                          # (hi, lo) words when ctx.proj_words: decoded in `early` below)
    # nothing of size E x H: graphs are only chunked to keep the P table and the partial rows below 2 GB and E below 2^31
    # (egnn_edge_bwd_pass_f32 addresses them with signed 32-bit scalar offsets): `_fused_graphs_per_chunk`
    step = _fused_graphs_per_chunk(b, n, k, hp)
    if step == 0:
        raise FusedBackwardLimit(_fused_limit_message(b, n, k, hp))
    if _FUSED_MAX_GRAPHS > 0:
        step = min(step, _FUSED_MAX_GRAPHS)
    # (padded copies of parameters are kept with the packed weights: `w` is rebuilt whenever a parameter changes, so once per
    # optimizer step instead of a dozen small launches per backward)
    pads = w.get("bwd_pads")
    if pads is None or pads["device"] != dev:
        pads = w["bwd_pads"] = {"device": dev}
    w_s = _pad_cached(pads, "w_s", (hp, lin0.weight.shape[1] - 2 * dim), lin0.weight.detach()[:, 2 * dim:])
    pi_split = k >= 6
    route = _behind_u_route(layer, m, st.coors.shape[-1], on_device, True)

    def node_bwd(ch, m_i, overlap):                          # (node_mlp on the split-f16 GEMMs, `overlap` queued behind its SiLU pass)
        return _node_mlp_backward(layer, w, ch.f0.detach().requires_grad_(True), m_i, ch.g_node, grads, drop, ch.lo * n, overlap=overlap)
    w2_finite = ctx.w2_finite = []
    for lo in range(0, b, step):
        ch = st.chunk(lo, min(b, lo + step))
        dest_lists = None
        hr_f = _ops.absmax_async(ch.f0.view(ch.bn, dim)) if on_device else None      # (read in step 3)

        def early():
            """Launches that depend on the saved inputs only -- P_i decoded in place (once), the edges sorted by destination: queued where
            the node-level part waits for a scale, so that the device has work while the host is woken up (_ops.HostRead)."""
            nonlocal dest_lists
            if proj_all is not None and ctx.proj_words:
                _ops.unsplit_words_(proj_all, hp)
                ctx.proj_words = False
            if dest_lists is None and (ch.i32 is not None or route != ROUTE_STANDARD):
                dest_lists = _ops.dest_lists(ch.i32, ch.bc, n, k, dev)                        # (shared by the tail and the E x H passes)
            return dest_lists
        # ---- 1. behind u: gU = d loss / d u, d loss / d (x_i - x_j) or its share of d/d coors, the parameter gradients of that part
        if route == ROUTE_STANDARD:
            tail = _behind_u_standard(layer, w, ch, u_all, grads, early, drop, ctx.valid_radius, by_k, want_ge)
        elif route == ROUTE_CLOSED:
            tail = _behind_u_closed(layer, ch, u_all, grads, node_bwd, early, drop, ctx.valid_radius, by_k, want_ge, mp)
        else:
            tail = _behind_u_autograd(layer, ch, u_all, grads, st.tail_params, drop, ctx.valid_radius, by_k, want_ge, mp, True)
        # ---- 2. the E x H work: d/d P_i, d/d P_j (per node), d/d W_s, d/d scalars, d/d W_2
        early()
        gz_i, gz_j, g_ws, g_scal, g_w2 = _edge_contract_blocks(layer, w, ch, tail, w_s, pi_split, dest_lists,
                                                               None if proj_all is None else proj_all[lo * n:ch.hi * n], drop)
        with torch.no_grad():
            if on_device:                                           # (read by `_w2_in_range_or_recomputed`, behind everything below)
                w2_finite.append(_ops.HostRead(torch.isfinite(g_w2).all().to(torch.int32).view(1)))
            # ---- 3. node-level products: d/d feats, d/d W_i, W_j, b_1 (and d/d W_s to its columns); edge_mlp's second Linear
            _edge_mlp0_backward(layer, w, ch, gz_i, gz_j, g_ws, hr_f, grads)
            del gz_i, gz_j
            g_scal = g_scal.view_as(tail.scal)
            grads[id(lin3.weight)] += g_w2[:m, :h]
            grads[id(lin3.bias)] += tail.bias2 if tail.bias2 is not None else tail.g_u[:, :m].sum(dim=0)
            if st.lk is not None:                                   # the edge columns of d/d scalars -> the tables
                st.lk.add(lo, ch.hi, ch.i32, n, k, g_scal.view(ch.ec, s_in)[:, s_in - layer.edge_dim:])
        # ---- 4. d loss / d scalars -> coordinates and edge features
        _scalars_to_inputs(ch, tail, g_scal, dest_lists, want_ge, st.g_edges)
    return st.finish()


def _lookup_rows(lookup, idx, b, n, k, pos=None):
    """The (B,N,K,edge_dim) features of the selected pairs, gathered from the caller's tensors behind an EdgeLookup (`live`: the dense
    float edges, the embedding weights) by differentiable indexing: E x D, what egnn_edge_features_gather_f32 reads, under autograd.
    pos: a SparseEdges first table's positions of the selected pairs (B,N,K), -1 where its rows do not hold one -- `values` / the
    token rows are indexed through them, a missing pair reading zeros / token 0 as in the dense image."""
    edges, tok_w, deg_w = lookup.live
    dev = (lookup.tok if lookup.tok is not None else (lookup.deg if lookup.deg is not None else edges)).device
    j = torch.arange(n, device=dev)[None, None, :].expand(b, n, k) if idx is None else idx.long()
    pair = (torch.arange(b * n, device=dev).view(b, n, 1) * n + j).reshape(-1)          # (b N + i) N + j
    cols = []
    if lookup.d1 and lookup.csr is not None:
        held = pos.reshape(-1) >= 0
        at = pos.reshape(-1).long().clamp(min=0)
        if lookup.tok is not None:
            tok = lookup.tok[at] if lookup.tok.numel() else at   # (no entries: every pair is missing)
            cols.append(tok_w[torch.where(held, tok, torch.zeros_like(tok))])
        else:
            rows = edges[at] if edges.shape[0] else edges.new_zeros(at.numel(), lookup.d1)
            cols.append(torch.where(held[:, None], rows, torch.zeros_like(rows)))
    elif lookup.d1:
        cols.append(tok_w[lookup.tok.reshape(-1)[pair]] if lookup.tok is not None else edges.reshape(-1, lookup.d1)[pair])
    if lookup.d2:
        if isinstance(lookup.deg, SparseLabels):                # (label CSR: the labels of the selected pairs, per slot)
            i32 = None if idx is None else idx.to(torch.int32).contiguous()      # (the kernel reads int32; `idx` may be the long copy)
            cols.append(deg_w[_ops_mod().csr_slot_labels(lookup.deg, i32, b, n, k).reshape(-1).long()])
        else:
            cols.append(deg_w[lookup.deg.reshape(-1)[pair].long()])
    return (torch.cat(cols, dim=-1) if len(cols) > 1 else cols[0]).view(b, n, k, lookup.width)


def _backward_twice(ctx, g_node, g_coors):
    """The backward under create_graph=True: the layer re-evaluated from the saved inputs themselves (not detached copies, so that the
    graph reaches the caller's tensors) over the neighbour list the forward selected, with the E x H block as `EdgeHidden`
    (`layer_given_neighbors(edge_hidden=True)`), and differentiated by autograd with create_graph=True.  Everything else -- the node
    tables, node_norm / node_mlp, the per-edge scalars, the E x m tail -- is ATen under autograd; edge look-up tables are gathered from
    their live tensors (`_lookup_rows`); training-mode dropout re-uses the forward's hash masks.  fp32 modules compute in plain fp32,
    float64 modules in float64."""
    layer = ctx.layer
    params = list(layer.parameters())
    pd = params[0].dtype if params else torch.float32
    if pd not in (torch.float32, torch.float64):
        raise NotImplementedError(f"second-order autograd (create_graph=True) through egnn_pytorch_amd.EGNN needs a float32 or float64 "
                                  f"module (its parameters are {pd}); convert it with .float() or .double()")
    feats, coors, edges, mask, idx32, rank = _unpack(ctx)
    need = _need(ctx)                                # (layer, order_hint, mask, adj, feats, coors, edges, *params)
    b, n, _ = feats.shape
    k = idx32.shape[-1] if idx32 is not None else n
    idx = None if idx32 is None else idx32.long()
    by_k = getattr(ctx, "edges_by_k", False)
    lookup = ctx.lookup
    e_in = (_lookup_rows(lookup, idx, b, n, k, pos=getattr(ctx, "csr_pos", None)).to(pd) if by_k else
            (None if edges is None else edges.to(pd)))
    out_n, out_c = layer_given_neighbors(layer, feats.to(pd), coors.to(pd), e_in, mask, idx, None if rank is None else rank.to(pd),
                                         ctx.valid_radius, drop=getattr(ctx, "drop", None), edges_by_k=by_k, edge_hidden=True)
    unused = _unused_params(layer, ctx)
    slots = []                                       # (position in the returned layout or table name, tensor)
    for pos, t in ((4, feats), (5, coors)):
        if need[pos] and t.requires_grad:
            slots.append((pos, t))
    if by_k:
        for name, pos, t in (("edges", 6, lookup.live[0]), ("tok", 8, lookup.live[1]), ("deg", 9, lookup.live[2])):
            if t is not None and ctx.needs_input_grad[pos] and t.requires_grad:
                slots.append((name, t))
    elif edges is not None and need[6] and edges.requires_grad:
        slots.append((6, edges))
    for i, p in enumerate(params):
        if need[7 + i] and p.requires_grad and id(p) not in unused:
            slots.append((7 + i, p))
    outs, gouts = [], []
    for o, g in ((out_n, g_node), (out_c, g_coors)):
        if g is not None and o.requires_grad:
            outs.append(o)
            gouts.append(g.to(o.dtype))
    wrt = [t for _, t in slots]
    grads = torch.autograd.grad(outs, wrt, gouts, create_graph=True, allow_unused=True) if (outs and wrt) else [None] * len(wrt)
    got = {pos: g for (pos, _), g in zip(slots, grads)}
    ctx.table_grads = (got.get("tok"), got.get("deg"))
    return (None, None, None, None, got.get(4), got.get(5), got.get("edges") if by_k else got.get(6)) + tuple(
        got.get(7 + i) for i in range(len(params)))


def _backward_recompute(ctx, g_node, g_coors):
    """The pure-ATen backward: chunked recompute of the whole layer through autograd (module docstring).  Used where neither native
    path applies -- more per-edge scalars than `_backward_exact` carries, CPU tensors,
    the EGNN_NATIVE_BACKWARD* switches -- and as the native paths' reference in the tests."""
    layer = ctx.layer
    feats, coors, edges, mask, idx, rank = _unpack(ctx)
    idx = None if idx is None else idx.long()
    params = [p for p in layer.parameters()]
    # inputs whose dtype differs from the parameters' (the forward converts at the boundary): differentiate in the parameters'
    # dtype, return every gradient in the dtype of the tensor it belongs to
    in_dtypes = (feats.dtype, coors.dtype, None if edges is None else edges.dtype)
    pd = params[0].dtype if params else feats.dtype
    feats, coors = feats.to(pd), coors.to(pd)
    edges = None if edges is None else edges.to(pd)
    rank = None if rank is None else rank.to(pd)
    g_node = None if g_node is None else g_node.to(pd)
    g_coors = None if g_coors is None else g_coors.to(pd)
    b, n, _ = feats.shape
    k = idx.shape[-1] if idx is not None else n
    step = _chunk_graphs(layer, n, k, b)
    need = _need(ctx)                                # (layer, order_hint, mask, adj, feats, coors, edges, *params)
    g_feats = torch.zeros_like(feats) if need[4] else None
    g_coors_in = torch.zeros_like(coors) if need[5] else None
    by_k = getattr(ctx, "edges_by_k", False)
    lk = _LookupGrads(ctx, b, n, feats.device) if by_k else None        # (edge look-up tables: d/d the gathered features -> the tables)
    want_e = edges is not None and (lk.active if by_k else bool(need[6]))
    g_edges = torch.zeros_like(edges) if (want_e and not by_k) else None
    g_params = [torch.zeros_like(p) if need[7 + i] else None for i, p in enumerate(params)]
    if g_node is None:
        g_node = torch.zeros_like(feats)
    if g_coors is None:
        g_coors = torch.zeros_like(coors)
    for lo in range(0, b, step):
        hi = min(b, lo + step)
        with torch.enable_grad():
            f = feats[lo:hi].detach().requires_grad_(need[4])
            c = coors[lo:hi].detach().requires_grad_(need[5])
            e = None if edges is None else edges[lo:hi].detach().requires_grad_(want_e)
            out_n, out_c = layer_given_neighbors(layer, f, c, e, None if mask is None else mask[lo:hi],
                                                 None if idx is None else idx[lo:hi], None if rank is None else rank[lo:hi],
                                                 ctx.valid_radius, drop=getattr(ctx, "drop", None), graph_offset=lo, edges_by_k=by_k)
            wrt = [t for t in (f, c, e) if t is not None and t.requires_grad] + [p for p, g in zip(params, g_params) if g is not None]
            outs, gouts = [], []
            for o, g in ((out_n, g_node[lo:hi]), (out_c, g_coors[lo:hi])):
                if o.requires_grad:
                    outs.append(o)
                    gouts.append(g)
            grads = torch.autograd.grad(outs, wrt, gouts, allow_unused=True) if outs and wrt else [None] * len(wrt)
        it = iter(grads)
        if f.requires_grad:
            g = next(it)
            if g is not None:
                g_feats[lo:hi] = g
        if c.requires_grad:
            g = next(it)
            if g is not None:
                g_coors_in[lo:hi] = g
        if e is not None and e.requires_grad:
            g = next(it)
            if g is not None and by_k:
                lk.add(lo, hi, None if idx is None else idx[lo:hi].int().contiguous(), n, k, g.to(lk.dtype).reshape(-1, g.shape[-1]))
            elif g is not None:
                g_edges[lo:hi] = g
        for i, gp in enumerate(g_params):
            if gp is not None:
                g = next(it)
                if g is not None:
                    gp.add_(g)
    cast = lambda g, dt: None if g is None else g.to(dt)                                        # noqa: E731
    unused = _unused_params(layer, ctx)
    g_params = [None if id(p) in unused else g for p, g in zip(params, g_params)]
    return (None, None, None, None, cast(g_feats, in_dtypes[0]), cast(g_coors_in, in_dtypes[1]),
            lk.outputs() if lk is not None else cast(g_edges, in_dtypes[2]), *g_params)


def wants_grad(layer, *tensors):
    """True when a forward under the current autograd mode has to record a graph."""
    if not torch.is_grad_enabled():
        return False
    if any(torch.is_tensor(t) and t.is_floating_point() and t.requires_grad for t in tensors):
        return True
    return any(p.requires_grad for p in layer.parameters())

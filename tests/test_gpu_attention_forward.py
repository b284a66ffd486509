"""The two forward attention cores of EGNN_Network's global attention blocks (csrc/global_attn.hip: egnn_induced_attn_f32,
egnn_token_attn_f32) against `attention.attn_core_torch` in float64, at kernel level: all three instantiations
(`induced_attn_kernel<1|2|4>`, `token_attn_kernel<1|2|4>`: dim_head <= 64, <= 128, <= 256) on both sides of every boundary, 1 to 8
tokens, node counts from fewer nodes than waves to 4099, masks that leave whole waves without a valid row, row strides wider than the
row, logits that need the max subtraction, the grid-stride loop of the token core, determinism, the limits (refused before any
launch) -- and whole blocks against a float64 copy of the plain module, with the kernels that ran named.

Bound: CORE_TOL = 2e-6 of the output's max |.| (tests/test_gpu_attention_training.py).  At logits of +-60 and beyond fp32 itself cannot
meet it (the float64 reference evaluated in fp32 is 2.5e-6 ... 3.2e-6 away there): on those cases the bound is
max(CORE_TOL, 4 x the fp32 evaluation's own error on the same inputs), the rule of tests/test_gpu_fuzz.py for cancelling sums.
Worst measured (MI355X), per case family: induced core sweep 8.7e-7 (dim_head 1, N = 4099; 2.3e-6 before its running sums were
compensated, csrc/global_attn.hip), token core sweep 3.4e-7, blocks 5.1e-7 (x) and 6.3e-7 (tokens) absolute; logits of +-60: kernels
3.5e-7 ... 1.6e-6, the fp32 reference 6.7e-7 ... 1.8e-6; common offset of 200: kernels 7.7e-6 ... 1.6e-5, the fp32 reference
9.2e-6 ... 2.6e-5; worst kernel-to-fp32-reference ratio 1.55 (the bound allows 4)."""
import copy

import pytest
import torch

from tests._util import ATOL
from tests.test_gpu_attention_training import CORE_TOL, _block, _mask_kinds, _ragged, _rel

pytestmark = pytest.mark.gpu

DHS = (1, 8, 63, 64, 65, 96, 128, 129, 255, 256)
TS = (1, 3, 8)
NS = (1, 2, 3, 4, 5, 7, 257, 4099)
B, HEADS = 3, 2


@pytest.fixture(autouse=True)
def _inference_mode():
    with torch.no_grad():
        yield


def _masks(b, n):
    """none | ragged | leading padding | one graph all False | exactly one valid node, first and last | valid nodes at n % 4 == r only
    (the kernel deals node n to wave n % 4: three of the four waves then hold masked rows only)"""
    i = torch.arange(n, device="cuda")
    ragged = _ragged(b, n)
    dead = ragged.clone()
    dead[-1] = False
    kinds = [("none", None), ("ragged", ragged), ("leading_padding", ragged.flip(1)), ("all_false_graph", dead),
             ("only_first", (i == 0)[None].expand(b, n).contiguous()), ("only_last", (i == n - 1)[None].expand(b, n).contiguous())]
    for r in range(4):
        kinds.append((f"mod4_eq_{r}", (i % 4 == r)[None].expand(b, n).contiguous()))
    return kinds


def _induced_ref(q, kv, mask, b, n, heads, scale, dtype=torch.float64):
    from egnn_pytorch_amd.attention import attn_core_torch
    return attn_core_torch(q.to(dtype), kv.to(dtype).view(b, n, -1), mask, heads, scale)


def _token_ref(q, kv_tok, b, n, heads, scale, dtype=torch.float64):
    from egnn_pytorch_amd.attention import attn_core_torch
    return attn_core_torch(q.to(dtype).view(b, n, -1), kv_tok.to(dtype), None, heads, scale).reshape(b * n, -1)


# ------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("dh", DHS)
def test_induced_core_against_float64(dh):
    from egnn_pytorch_amd import _ops
    inner, scale = HEADS * dh, dh ** -0.5
    worst = (0.0, None)
    for t in TS:
        for n in NS:
            g = torch.Generator().manual_seed(10000 * t + 10 * dh + n)
            q = torch.randn(B, t, inner, generator=g).cuda()
            kv = torch.randn(B * n, 2 * inner, generator=g).cuda()
            for kind, mask in _masks(B, n):
                got = _ops.induced_attn(q, kv, mask, B, n, HEADS, dh, scale)          # (out comes poisoned: every element is written)
                want = _induced_ref(q, kv, mask, B, n, HEADS, scale)
                assert got.shape == (B, t, inner) and torch.isfinite(got).all(), (t, dh, n, kind)
                err = _rel(got, want)
                if err >= worst[0]:
                    worst = (err, (t, n, kind))
                assert err <= CORE_TOL, (t, dh, n, kind, err)
                if mask is not None:                                                  # a graph without a valid node: the uniform average
                    empty = ~mask.any(dim=1)
                    if bool(empty.any()):
                        mean_v = kv.double().view(B, n, 2, inner)[:, :, 1].mean(dim=1)[empty]        # (graphs, inner)
                        assert _rel(got[empty], mean_v[:, None].expand(-1, t, -1)) <= CORE_TOL, (t, dh, n, kind)
    print(f"induced dh={dh}: worst {worst[0]:.2e} at (t, n, mask) = {worst[1]}")


@pytest.mark.parametrize("dh", DHS)
def test_token_core_against_float64(dh):
    from egnn_pytorch_amd import _ops
    inner, scale = HEADS * dh, dh ** -0.5
    worst = (0.0, None)
    for t in TS:
        for n in NS:
            g = torch.Generator().manual_seed(20000 * t + 10 * dh + n)
            q = torch.randn(B * n, inner, generator=g).cuda()
            kv_tok = torch.randn(B, t, 2 * inner, generator=g).cuda()
            got = _ops.token_attn(q, kv_tok, B, n, HEADS, dh, scale)
            want = _token_ref(q, kv_tok, B, n, HEADS, scale)
            assert got.shape == (B * n, inner) and torch.isfinite(got).all(), (t, dh, n)
            err = _rel(got, want)
            if err >= worst[0]:
                worst = (err, (t, n))
            assert err <= CORE_TOL, (t, dh, n, err)
    print(f"token dh={dh}: worst {worst[0]:.2e} at (t, n) = {worst[1]}")


# ------------------------------------------------------------------------------------------------ strides
@pytest.mark.parametrize("dh", [8, 65, 129])
def test_row_strides_wider_than_the_row(dh):
    """kv (and the token core's q) as a column slice of a wider buffer whose other columns are NaN: the bits of the contiguous call"""
    from egnn_pytorch_amd import _ops
    t, n = 3, 261
    inner, scale = HEADS * dh, dh ** -0.5
    g = torch.Generator().manual_seed(dh)
    q = torch.randn(B, t, inner, generator=g).cuda()
    kv = torch.randn(B * n, 2 * inner, generator=g).cuda()
    wide = torch.full((B * n, 2 * inner + 11), float("nan"), device="cuda")
    wide[:, 3:3 + 2 * inner] = kv
    kv_view = wide[:, 3:3 + 2 * inner]
    assert kv_view.stride(0) > 2 * inner
    for kind, mask in _mask_kinds(B, n):
        assert torch.equal(_ops.induced_attn(q, kv_view, mask, B, n, HEADS, dh, scale), _ops.induced_attn(q, kv, mask, B, n, HEADS, dh, scale)), kind
    q2 = torch.randn(B * n, inner, generator=g).cuda()
    kv_tok = torch.randn(B, t, 2 * inner, generator=g).cuda()
    wide_q = torch.full((B * n, inner + 9), float("nan"), device="cuda")
    wide_q[:, 5:5 + inner] = q2
    q_view = wide_q[:, 5:5 + inner]
    assert q_view.stride(0) > inner
    got = _ops.token_attn(q_view, kv_tok, B, n, HEADS, dh, scale)
    assert torch.isfinite(got).all() and torch.equal(got, _ops.token_attn(q2, kv_tok, B, n, HEADS, dh, scale))


# ------------------------------------------------------------------------------------------------ logit range
def _logit_cases(dh, t, n, g):
    """(name, q rows, k / v rows) builders share one generator: `scaled` = N(0, 1) x 4 on q and k (logits to about +-60 at dim_head 64);
    `offset` = every k row k0 + 0.05 noise with scale q . k0 ~ 200: exp overflows without the max subtraction"""
    amp = (200.0 / dh ** 0.5) ** 0.5

    def scaled(rows_q, rows_k):
        q = 4.0 * torch.randn(*rows_q, HEADS * dh, generator=g)
        kv = torch.randn(*rows_k, 2, HEADS * dh, generator=g)
        kv[..., 0, :] *= 4.0
        return q, kv.flatten(-2)

    def offset(rows_q, rows_k):
        q = amp * (1.0 + 0.1 * torch.randn(*rows_q, HEADS * dh, generator=g))
        kv = torch.randn(*rows_k, 2, HEADS * dh, generator=g)
        kv[..., 0, :] = amp + 0.05 * kv[..., 0, :]
        return q, kv.flatten(-2)
    return (("scaled", scaled), ("offset", offset))


@pytest.mark.parametrize("dh", [8, 64, 129])
def test_logits_that_need_the_max_subtraction(dh):
    from egnn_pytorch_amd import _ops
    t, n = 8, 257
    scale = dh ** -0.5
    g = torch.Generator().manual_seed(3 * dh)
    for name, build in _logit_cases(dh, t, n, g):
        # tokens over nodes
        q, kv = (x.cuda() for x in build((B, t), (B * n,)))
        want = _induced_ref(q, kv, None, B, n, HEADS, scale)
        logits = (q.double().view(B, t, HEADS, dh).transpose(1, 2) @ kv.double().view(B, n, 2, HEADS, dh)[:, :, 0].permute(0, 2, 3, 1)) * scale
        if name == "offset":
            assert float(logits.min()) > 100.0                    # (exp(100) is beyond fp32)
        else:
            assert float(logits.abs().max()) > (30.0 if dh >= 64 else 20.0)
        for kind, mask in _mask_kinds(B, n):
            want = _induced_ref(q, kv, mask, B, n, HEADS, scale)
            own = _rel(_induced_ref(q, kv, mask, B, n, HEADS, scale, torch.float32), want)
            err = _rel(_ops.induced_attn(q, kv, mask, B, n, HEADS, dh, scale), want)
            print(f"induced {name} dh={dh} {kind}: kernel {err:.2e} fp32 reference {own:.2e} ratio {err / max(own, 1e-30):.2f}")
            assert err <= max(CORE_TOL, 4.0 * own), (name, dh, kind, err, own)
        # nodes over tokens
        q, kv_tok = (x.cuda() for x in build((B * n,), (B, t)))
        want = _token_ref(q, kv_tok, B, n, HEADS, scale)
        own = _rel(_token_ref(q, kv_tok, B, n, HEADS, scale, torch.float32), want)
        got = _ops.token_attn(q, kv_tok, B, n, HEADS, dh, scale)
        err = _rel(got, want)
        print(f"token {name} dh={dh}: kernel {err:.2e} fp32 reference {own:.2e} ratio {err / max(own, 1e-30):.2f}")
        assert torch.isfinite(got).all() and err <= max(CORE_TOL, 4.0 * own), (name, dh, err, own)


# ------------------------------------------------------------------------------------------------ grid stride, determinism, limits
def test_token_core_grid_stride_loop():
    """262 152 (row, head) items on the 65 536 workgroups x 4 waves the launch is capped at: the last eight come from the loop's
    second round"""
    from egnn_pytorch_amd import _ops
    b, n, heads, dh, t = 1, 32769, 8, 8, 3
    assert n * heads == 65536 * 4 + 8
    g = torch.Generator().manual_seed(4)
    q = torch.randn(b * n, heads * dh, generator=g).cuda()
    kv_tok = torch.randn(b, t, 2 * heads * dh, generator=g).cuda()
    got = _ops.token_attn(q, kv_tok, b, n, heads, dh, dh ** -0.5)
    want = _token_ref(q, kv_tok, b, n, heads, dh ** -0.5)
    assert torch.isfinite(got).all()
    assert _rel(got, want) <= CORE_TOL
    assert _rel(got[-2:], want[-2:]) <= CORE_TOL and _rel(got[-1, -dh:], want[-1, -dh:]) <= CORE_TOL


def test_both_cores_are_deterministic():
    from egnn_pytorch_amd import _ops
    n, t, dh = 4099, 8, 96
    g = torch.Generator().manual_seed(5)
    q = torch.randn(B, t, HEADS * dh, generator=g).cuda()
    kv = torch.randn(B * n, 2 * HEADS * dh, generator=g).cuda()
    mask = _ragged(B, n)
    assert torch.equal(_ops.induced_attn(q, kv, mask, B, n, HEADS, dh, 0.1), _ops.induced_attn(q, kv, mask, B, n, HEADS, dh, 0.1))
    q2 = torch.randn(B * n, HEADS * dh, generator=g).cuda()
    kv_tok = torch.randn(B, t, 2 * HEADS * dh, generator=g).cuda()
    assert torch.equal(_ops.token_attn(q2, kv_tok, B, n, HEADS, dh, 0.1), _ops.token_attn(q2, kv_tok, B, n, HEADS, dh, 0.1))


def test_limits_are_refused_before_any_launch():
    """nine tokens and dim_head 257 are EGNN_E_UNSUPPORTED (-3), a row stride below 2 inner is EGNN_E_SHAPE (-2): both entries return
    these in front of their launch (csrc/global_attn.hip)"""
    from egnn_pytorch_amd import _abi, _ops
    n = 5
    for t, dh in ((9, 8), (3, 257)):
        inner = HEADS * dh
        q = torch.zeros(B, t, inner, device="cuda")
        kv = torch.zeros(B * n, 2 * inner, device="cuda")
        with pytest.raises(_abi.EGNNHipError, match="egnn_induced_attn_f32 failed with code -3"):
            _ops.induced_attn(q, kv, None, B, n, HEADS, dh, 1.0)
        with pytest.raises(_abi.EGNNHipError, match="egnn_token_attn_f32 failed with code -3"):
            _ops.token_attn(torch.zeros(B * n, inner, device="cuda"), torch.zeros(B, t, 2 * inner, device="cuda"), B, n, HEADS, dh, 1.0)
    inner = HEADS * 8
    with pytest.raises(_abi.EGNNHipError, match="egnn_induced_attn_f32 failed with code -2"):
        _ops.induced_attn(torch.zeros(B, 3, inner, device="cuda"), torch.zeros(B * n, 2 * inner - 2, device="cuda"), None, B, n, HEADS, 8, 1.0)


# ------------------------------------------------------------------------------------------------ block level
def _run_block(blk, x, tokens, mask):
    from egnn_pytorch_amd import _ops
    with _ops.phase_timer() as pt:
        out = blk(x, tokens, mask=mask)
    return out, set(pt.summary())


@pytest.mark.parametrize("dim,heads,dh,t,n", [(33, 1, 256, 8, 1), (20, 2, 65, 1, 37), (64, 2, 129, 8, 300)])
def test_blocks_against_the_float64_module(dim, heads, dh, t, n):
    """GlobalLinearAttention in eval mode under no_grad against a float64 deep copy (a float64 module is the plain differentiable one),
    at the ATOL of test_global_attention_block_on_the_hip_kernels"""
    blk = _block(dim, heads, dh, seed=dim).cuda().eval()
    ref = copy.deepcopy(blk).double()
    g = torch.Generator().manual_seed(dim + n)
    x = torch.randn(B, n, dim, generator=g).cuda()
    tokens = torch.randn(B, t, dim, generator=g).cuda()
    for kind, mask in _mask_kinds(B, n)[1:]:                       # ragged, and ragged with one graph all False
        (got_x, got_t), ran = _run_block(blk, x, tokens, mask)
        assert {"induced_attn", "token_attn", "attn_ff0"} <= ran, ran
        want_x, want_t = ref(x.double(), tokens.double(), mask=mask)
        assert torch.isfinite(got_x).all() and torch.isfinite(got_t).all()
        ex, et = float((got_x.double() - want_x).abs().max()), float((got_t.double() - want_t).abs().max())
        print(f"block dim={dim} heads={heads} dh={dh} t={t} n={n} {kind}: x {ex:.2e} tokens {et:.2e}")
        assert ex <= ATOL and et <= ATOL, (kind, ex, et)


def test_blocks_beyond_the_kernels_limits_stay_on_the_plain_module():
    from egnn_pytorch_amd import exact_arithmetic
    g = torch.Generator().manual_seed(6)
    n = 37
    hip = {"induced_attn", "token_attn", "attn_ff0"}
    for dim, heads, dh, t, exact in ((20, 2, 8, 9, False), (20, 1, 257, 4, False), (20, 2, 8, 4, True)):
        blk = _block(dim, heads, dh, seed=1).cuda().eval()
        ref = copy.deepcopy(blk).double()
        x = torch.randn(B, n, dim, generator=g).cuda()
        tokens = torch.randn(B, t, dim, generator=g).cuda()
        mask = _ragged(B, n)
        if exact:
            with exact_arithmetic():
                (got_x, got_t), ran = _run_block(blk, x, tokens, mask)
            assert hip <= _run_block(blk, x, tokens, mask)[1]      # (the same block runs on the kernels outside the context)
        else:
            (got_x, got_t), ran = _run_block(blk, x, tokens, mask)
        assert not (hip & ran), (dim, heads, dh, t, exact, ran)
        want_x, want_t = ref(x.double(), tokens.double(), mask=mask)
        assert float((got_x.double() - want_x).abs().max()) <= ATOL and float((got_t.double() - want_t).abs().max()) <= ATOL

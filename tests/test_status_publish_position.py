"""The range status words are published from inside the one-call C forward, directly behind the last launch that can write them
(egnn_forward_opts.status_pub): for a layer whose node_mlp is two GEMMs that is between them, so the host has the next forward enqueued
while the second GEMM still runs.  Nothing a caller sees may change: the outputs are the same bits with the early publish on and off
(EGNN_STATUS_EARLY, read at every call), forwards queued under the previous call's last GEMM do not disturb each other, an
out-of-range call still warns and is answered by the plain-fp32 kernels, an overflow raised by the LAST launch that can raise one
(node_mlp's hidden activation, flagged by the first GEMM's epilogue) is reported by the call that produced it, and graphed() replays
are left alone."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

B, N = 2, 64
# "wide": the north-star layer, node_mlp as two GEMMs (publish between them); "fused": node_mlp in one launch (publish at the end)
LAYERS = {"wide": dict(dim=512, num_nearest_neighbors=32), "fused": dict(dim=128, num_nearest_neighbors=16)}
_cache = {}


def _setup(name):
    """(layer, two inputs, their stand-alone outputs with the early publish OFF): computed once per layer and left unchanged."""
    if name not in _cache:
        import os
        from egnn_pytorch_amd import EGNN, _abi
        torch.manual_seed(11)
        kw = LAYERS[name]
        layer = EGNN(**kw).cuda().eval()
        assert (_abi.load().egnn_node_mlp_fused_halves(kw["dim"], layer.m_dim) > 0) == (name == "fused")
        g = torch.Generator().manual_seed(5)
        inputs = []
        for _ in range(2):
            inputs.append((torch.randn(B, N, kw["dim"], generator=g).cuda(), torch.randn(B, N, 3, generator=g).cuda()))
        mask = (torch.arange(N)[None, :] < torch.tensor([[N], [N - 9]])).cuda()
        old = os.environ.get("EGNN_STATUS_EARLY")
        os.environ["EGNN_STATUS_EARLY"] = "0"
        try:
            with torch.no_grad():
                refs = [tuple(t.clone() for t in layer(f, c, mask=mask)) for f, c in inputs]
            torch.cuda.synchronize()
        finally:
            if old is None:
                del os.environ["EGNN_STATUS_EARLY"]
            else:
                os.environ["EGNN_STATUS_EARLY"] = old
        _cache[name] = (layer, inputs, mask, refs)
    return _cache[name]


@pytest.fixture
def requests(monkeypatch):
    """What `_ops.status_request` answered, call by call (None: the Python side publishes behind the forward, as before)."""
    from egnn_pytorch_amd import _ops
    seen = []
    real = _ops.status_request

    def spy(device):
        r = real(device)
        seen.append(r)
        return r

    monkeypatch.setattr(_ops, "status_request", spy)
    return seen


def _same(out, ref):
    return torch.equal(out[0], ref[0]) and torch.equal(out[1], ref[1])


@pytest.mark.parametrize("name", list(LAYERS))
def test_outputs_are_the_same_bits_with_the_early_publish_on_and_off(name, requests, monkeypatch):
    from egnn_pytorch_amd import _ops
    layer, inputs, mask, refs = _setup(name)
    requests.clear()
    seq0 = _ops.status_word(inputs[0][0].device).seq
    with torch.no_grad():
        on = layer(*inputs[0], mask=mask)
    torch.cuda.synchronize()
    assert len(requests) == 1 and requests[0] is not None                  # the C entry published, the check only waited
    assert _ops.status_word(inputs[0][0].device).seq == seq0 + 1          # one sequence number per forward
    assert _same(on, refs[0])
    monkeypatch.setenv("EGNN_STATUS_EARLY", "0")
    with torch.no_grad():
        off = layer(*inputs[0], mask=mask)
    torch.cuda.synchronize()
    assert requests[-1] is None
    assert _same(off, refs[0])
    assert not _ops.status_word(inputs[0][0].device).lock.locked()


@pytest.mark.parametrize("name", list(LAYERS))
def test_twenty_alternating_forwards_each_equal_their_stand_alone_result(name, requests):
    """No synchronisation between the calls: each forward's launches are queued while the previous call's last GEMM may still run."""
    layer, inputs, mask, refs = _setup(name)
    requests.clear()
    outs = []
    with torch.no_grad():
        for i in range(20):
            outs.append(layer(*inputs[i % 2], mask=mask))
    torch.cuda.synchronize()
    assert len(requests) == 20 and all(r is not None for r in requests)
    for i, out in enumerate(outs):
        assert _same(out, refs[i % 2]), i


@pytest.mark.parametrize("name", list(LAYERS))
def test_feats_beyond_fp16_still_warn_and_rerun_in_plain_fp32(name, requests, monkeypatch):
    from egnn_pytorch_amd import exact_arithmetic, layer as layer_mod
    layer, inputs, mask, refs = _setup(name)
    requests.clear()
    feats, coors = inputs[0][0] * 1e6, inputs[0][1]
    with torch.no_grad(), exact_arithmetic():
        want = layer(feats, coors, mask=mask)
    got = {}
    for early in ("1", "0"):
        monkeypatch.setenv("EGNN_STATUS_EARLY", early)
        monkeypatch.setattr(layer_mod, "_warned_rerun", False)
        with torch.no_grad(), pytest.warns(RuntimeWarning, match="re-run on the plain-fp32"):
            got[early] = layer(feats, coors, mask=mask)
        torch.cuda.synchronize()
    assert requests.count(None) == 1 and len(requests) == 2
    for early in got:
        assert torch.isfinite(got[early][0]).all() and torch.isfinite(got[early][1]).all()
        assert _same(got[early], want), early
    with torch.no_grad(), warnings.catch_warnings():                       # the word was cleared: an in-range call is clean again
        warnings.simplefilter("error")
        assert _same(layer(*inputs[0], mask=mask), refs[0])


def test_hidden_activation_overflow_is_reported_by_the_call_that_made_it(requests):
    """node_mlp[0].weight x 1e7 (initialised N(0, 1e-3): now sigma = 1e4, so a hidden pre-activation over 528 unit-scale inputs has
    sigma ~ 2e5 and four in ten of the positive ones pass 65504): feats, projections, edge messages and m_i stay in range; only the
    hidden activation SiLU(W_5 [h | m_i] + b_5) leaves fp16, flagged by the first GEMM's epilogue where it packs the second GEMM's
    operand (EGNN_RANGE_A_OPERAND) -- the last launch that can raise a bit.  A publish in front of that GEMM would hand the host a
    clean word for this call."""
    import copy
    from egnn_pytorch_amd import EGNNRangeError, _abi, _ops
    layer, inputs, mask, refs = _setup("wide")
    requests.clear()
    big = copy.deepcopy(layer)
    with torch.no_grad():
        big.node_mlp[0].weight.mul_(1e7)
    feats, coors = inputs[0]
    with torch.no_grad(), pytest.raises(EGNNRangeError) as err, _ops.early_publish():
        big._call(feats, coors, None, mask, None, None)
        _ops.range_check_after_forward(feats.device)
    assert len(requests) == 1 and requests[0] is not None          # published by the C entry, between the two GEMMs
    assert err.value.origin == "call" and err.value.bits == 1
    assert _abi.RANGE_BITS[1] in str(err.value)
    st = _ops.status_word(feats.device)
    assert not st.lock.locked()
    torch.cuda.synchronize()
    assert int(st.dev[0]) == 0                                             # cleared for the next call
    with torch.no_grad():
        assert _same(layer(feats, coors, mask=mask), refs[0])             # ... which is clean


def test_last_layer_of_a_network_publishes_for_the_whole_stack(requests, monkeypatch):
    from egnn_pytorch_amd import EGNN_Network
    torch.manual_seed(3)
    net = EGNN_Network(depth=3, dim=64, num_nearest_neighbors=8).cuda().eval()
    g = torch.Generator().manual_seed(9)
    feats, coors = torch.randn(B, N, 64, generator=g).cuda(), torch.randn(B, N, 3, generator=g).cuda()
    with torch.no_grad():
        on = net(feats, coors)
    torch.cuda.synchronize()
    assert [r is not None for r in requests] == [False, False, True]
    monkeypatch.setenv("EGNN_STATUS_EARLY", "0")
    with torch.no_grad():
        off = net(feats, coors)
    torch.cuda.synchronize()
    assert _same(on, off)
    # an overflow in an EARLIER layer is still this call's: feats x 1e6 re-runs the stack in plain fp32 either way
    from egnn_pytorch_amd import layer as layer_mod
    outs = []
    for early in ("1", "0"):
        monkeypatch.setenv("EGNN_STATUS_EARLY", early)
        monkeypatch.setattr(layer_mod, "_warned_rerun", False)
        with torch.no_grad(), pytest.warns(RuntimeWarning, match="re-run on the plain-fp32"):
            outs.append(net(feats * 1e6, coors))
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0][0]).all() and _same(outs[0], outs[1])


def test_nothing_changes_under_graphed(requests):
    from egnn_pytorch_amd import _ops, graphed
    layer, inputs, mask, refs = _setup("wide")
    requests.clear()
    with torch.no_grad():
        run = graphed(layer, inputs[0][0], inputs[0][1], mask=mask)
        before = len(requests)
        captured = [r for r in requests]
        for i in (1, 0, 1):
            out = run(inputs[i][0], inputs[i][1], mask=mask)
            torch.cuda.synchronize()
            assert _same(out, refs[i]), i
    assert len(requests) == before                                         # replays never enter the C entry from Python
    assert captured[-1] is None                                            # ... and the captured forward asked for no publish
    assert not _ops.status_word(inputs[0][0].device).lock.locked()

"""The status-publish request of egnn_forward_opts (ABI 44) is made inside a module's forward only, without a GPU.  (The struct's
mirror, its size and the ABI version numbers: tests/test_abi_agreement.py.)"""


def test_status_request_is_refused_outside_a_module_forward():
    """No `early_publish` scope, no request: a bare `_forward_c` (or any other caller of the C entry) keeps today's path."""
    from egnn_pytorch_amd import _ops
    assert _ops._early.get() is None
    assert _ops.status_request("cuda:0") is None
    with _ops.early_publish(last=False):
        assert _ops.status_request("cuda:0") is None                      # (layers that can still write the word follow)

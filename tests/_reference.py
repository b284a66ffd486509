"""What the reference module itself computed, for the tests that compare against it: stored under tests/golden/reference/<key>.npz,
so that the suite needs neither the reference's sources nor the oracle/_ref artefact built from them.

`reference_result(key, compute)` returns the stored arrays of `key`.  With EGNN_RECORD_REFERENCE=1 it first runs `compute(ref)` on
the reference package (oracle/_ref, built by oracle/build_ref.py where the reference's sources exist) and rewrites the file:

    EGNN_RECORD_REFERENCE=1 python -m pytest tests/test_autograd.py tests/test_oracle_vs_reference.py tests/test_gpu_fuzz.py

Recording runs the reference on the CPU.  The drop-in modules draw the same seeded initial weights as the reference (same
submodules, same order), so a test rebuilds the weights itself; `state_digest` of the reference's state is stored beside its
results and checked against the test's own module, so stored results are never compared with other weights."""
import hashlib
import os

import numpy as np
import torch

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
RECORD = os.environ.get("EGNN_RECORD_REFERENCE") == "1"


def reference_module():
    from oracle import build_ref
    if not build_ref.build():
        raise RuntimeError("EGNN_RECORD_REFERENCE=1 needs the reference (oracle/_ref, or its sources for oracle/build_ref.py)")
    return build_ref.import_reference()


def state_digest(module):
    """sha256 over the names, dtypes, shapes and bytes of a module's state_dict, as a uint8 array."""
    h = hashlib.sha256()
    for name, t in module.state_dict().items():
        t = t.detach().cpu().contiguous()
        h.update(f"{name}:{t.dtype}:{tuple(t.shape)};".encode())
        h.update(t.numpy().tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def case_key(request):
    """A file name for the running test case: its node name (test function + parameter ids)."""
    return "".join(c if c.isalnum() or c in "_-." else "_" for c in request.node.name)


def reference_result(key, compute, gpu=False):
    """`gpu`: the calling test goes on to the MI355X.  Recording on a machine without one ends such a test (skipped) once its file
    is written; run the recording with `--noconftest` there, or the GPU tests are skipped before they get here."""
    path = os.path.join(DIR, key + ".npz")
    if RECORD:
        arrays = {k: np.asarray(v) for k, v in compute(reference_module()).items()}
        os.makedirs(DIR, exist_ok=True)
        np.savez_compressed(path, **arrays)
        if gpu and not torch.cuda.is_available():
            import pytest
            pytest.skip(f"recorded {key}; no GPU to compare on")
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def check_state(module, stored):
    """The module holds the weights the stored results were computed with."""
    assert np.array_equal(state_digest(module), stored["state_sha256"]), "weights differ from the ones the reference results belong to"


def pack_grads(grads):
    """A list of gradients (None where an input gets none) as arrays: grad.<i> for each present one, n_grads for the length."""
    out = {"n_grads": np.array(len(grads))}
    for i, g in enumerate(grads):
        if g is not None:
            out[f"grad.{i}"] = g.detach().cpu().numpy()
    return out


def unpack_grads(stored):
    return [torch.from_numpy(stored[f"grad.{i}"]) if f"grad.{i}" in stored else None for i in range(int(stored["n_grads"]))]

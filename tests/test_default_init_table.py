"""tests/_default_init.py on the host: every case (row of tests/test_gpu_mask_patterns_training.py::ROWS x cotangent form) is built on
the CPU and meets, on its float64 reference alone, the conditions that make its GPU comparison (tests/test_gpu_default_init.py) say
something:

  (a) the state is the module's own draw: every Linear weight has std within [0.7e-3, 1.3e-3], every parameter equals a second
      construction under the same seed (rows with a clamp: but for coors_mlp's last bias, which `_centre_clamp` moves);
  (b) every reference gradient has max |.| > 0 -- except the tensors the form of the loss cannot reach (node_mlp / node_norm under
      coordinates only, coors_mlp / coors_norm.scale under features only), which are exactly zero;
  (c) replacing one live neighbour of every real node by another real node moves the coordinate update and each of d/d edge_mlp.*,
      d/d coors_mlp.* by at least 5e-4 of its own scale, 5 x the bar: a wrong edge path cannot pass.  The dense rows are exempt (another
      selection yields the same pairs)."""
import pytest
import torch

from tests import _default_init as D
from tests import test_gpu_mask_patterns_training as M


def test_the_cases_are_the_rows_of_the_mask_pattern_table():
    assert [r for r, _ in D.CASES[::3]] == list(M.ROWS) and len(D.CASES) == 3 * len(M.ROWS)
    assert D.PATTERN in M.PATTERNS
    assert set(D.DENSE_ROWS) == {"dense", "exact_fourier8"}
    assert D.SENSITIVITY == 5 * D.BAR


@pytest.mark.parametrize("row", list(M.ROWS))
def test_every_case_meets_its_conditions_on_the_float64_reference(row):
    shared = None
    for form in D.FORMS:
        d = D.prepare(row, form)
        c = d.case
        assert not c.feats.is_cuda and c.pattern == D.PATTERN
        pad = ~c.mask
        assert bool(pad.any()) and not bool(c.rn[pad].any()) and not bool(c.rc[pad].any())
        assert bool(c.rn.any()) == (form != "coors_only") and bool(c.rc.any()) == (form != "feats_only")
        assert set(d.zeros) == {nm for nm in M._names(c) if nm.startswith(
            {"both": ("\0",), "coors_only": ("node_mlp.", "node_norm."), "feats_only": ("coors_mlp.", "coors_norm.")}[form])}
        assert (row in D.DENSE_ROWS) == (not d.sens)
        if row not in D.DENSE_ROWS:
            assert "coors_out - coors" in d.sens and any(k.startswith("edge_mlp.") for k in d.sens)
            assert any(k.startswith("coors_mlp.") for k in d.sens) == (form != "feats_only")
        # the three forms of a row share the layer, the inputs and the neighbour list
        state = (c.feats, c.coors, c.mask, d.idx) + tuple(c.layer.parameters())
        if shared is not None:
            assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(shared, state)), (row, form)
        shared = state
        print(f"DEFAULT_INIT {row}/{form} scales " + " ".join(f"{k}={v:.1e}" for k, v in d.scales.items()))
        print(f"DEFAULT_INIT {row}/{form} moved by one neighbour " + " ".join(f"{k}={v:.1e}" for k, v in d.sens.items()))

"""tests/_glue_variants.py on the host: every cell's `prepare` meets the conditions that make its device comparison
(tests/test_gpu_glue_variants.py) decidable and non-trivial -- on the float64 reference alone --, the table names exactly the kernels
that csrc/edge_tail.hip, csrc/node_ops.hip and csrc/node_mlp_fused.hip compile to, the launcher's choice of tail kernel and
`nmf_supported` are restated, the specifications added beside egnn_pytorch_amd/autograd.py are tied to float64 autograd, and the numpy
restatements of the bit-exact parts agree with plain float64 sums and with `_weights.pack_tiles`."""
import os
import re
from collections import Counter

import numpy as np
import pytest
import torch

from tests import _glue_variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_tail_cell_meets_its_conditions_on_the_reference():
    seen = Counter()
    for c in V.TAIL_CELLS:
        d = V.prepare(c.id)                                                      # asserts the cell conditions (`_tail_conditions`)
        p = d.p
        seen["cells"] += 1
        seen[f"E{d.e}"] += 1
        seen[f"m{d.m}"] += 1
        seen[f"mask_{p['mask']}"] += 1
        seen["dense" if p["dense"] else "knn"] += 1
        for name in ("g_u", "g_rel", "g_hid", "a3", "g_w"):
            assert bool(torch.isfinite(d.ref[name]).all()), (c.id, name)
        if d.margin is not None:
            seen["margin"] += 1
            assert d.margin >= 64
        if p["clamp"] == "mid" and d.e >= 63 and p["mask"] != "all":
            live = d.pm.reshape(-1) if d.pm is not None else torch.ones(d.e, dtype=torch.bool)
            w = d.ref["w"].reshape(-1)[live]
            assert bool((w > d.clamp).any()) and bool((w < -d.clamp).any()) and bool((w.abs() < d.clamp).any()), c.id     # +c, -c and unclamped
            assert bool(d.ref["g_w"].any()) and bool(d.ref["g_hid"].any()), c.id
            seen["clamp_both_signs"] += 1
        if p["norm"] and p["dup"] and d.n >= 2:
            seen["coincident"] += 1
        if d.drop is not None:
            seen[f"drop_p{d.drop[0]}"] += 1
            seen["eid0>0"] += int(d.eid0 > 0)
        # the caps of the older tests are never exceeded (min(derived, older)), and no bar is zero where the reference is not
        for mode in V.tail_modes(c):
            bars = V.tail_bars(c.id, mode)
            for name in ("g_u", "g_rel"):
                top = float(d.ref[name].abs().max())
                assert float(torch.as_tensor(bars[name], dtype=torch.float64).max()) <= V.EDGE_CAP * max(top, 1e-30) * (1 + 1e-12), (c.id, mode, name)
                assert top == 0 or float(torch.as_tensor(bars[name], dtype=torch.float64).max()) > 0
            assert bool((bars["sums"] >= 0).all())
    assert {f"E{e}" for e in (1, 15, 16, 17, 63, 65, 255, 256, 257, 769)} <= set(seen), seen
    assert all(seen[f"m{m}"] >= 1 for m in (1, 7, 13, 16)) and seen["dense"] >= 4 and seen["knn"] >= 20, seen
    assert all(seen[f"mask_{k}"] >= 1 for k in ("none", "ragged", "scattered", "node", "all")), seen
    assert seen["clamp_both_signs"] >= 20 and seen["coincident"] >= 20 and seen["drop_p0.1"] >= 2 and seen["drop_p0.5"] >= 2 and seen["eid0>0"] >= 2, seen
    assert {V.TAIL_BY_ID[k].p["w3"] for k in V.TAIL_BY_ID} >= {0.0, 2.0 ** -8, 1.0, 3072.0, 1e-30, 1.5}
    assert V.TAIL_BY_ID["clamp_zero"].p["clamp"] == 0.0 and V.TAIL_BY_ID["clamp_none"].p["clamp"] is None
    assert float(V.prepare("norm_nodup").w["scale"]) != 1.0 and float(V.prepare("base_e80").w["scale"]) != 1.0
    # the module's own initialisation: E = 80 and 257, with and without the gate and CoorsNorm, one with dropout, one with pooled messages
    init = [c for c in V.TAIL_CELLS if c.p["init"]]
    assert {(V.prepare(c.id).e, c.p["gate"] is not None, c.p["norm"]) for c in init} == {(80, True, True), (80, False, False), (257, True, False), (257, False, True)}
    assert sum(c.p["drop"] is not None for c in init) == 1 and sum(c.p["gm"] != 0.0 for c in init) == 1 and len(init) == 6
    assert all(V.tail_modes(c) == (("mfma_drop",) if c.p["drop"] else V.TAIL_MODES) for c in init)
    print(dict(seen))


def test_the_kernel_table_equals_what_the_compiler_instantiated():
    """csrc/build.sh leaves the compiler's resource-usage remarks of every translation unit next to its object; the `Function Name:`
    remarks name the kernels that exist.  A new kernel or instantiation in the three units fails here until it has a cell."""
    pkg = os.path.join(ROOT, "egnn_pytorch_amd")
    if not os.path.exists(os.path.join(pkg, "libegnn_hip.so")):
        pytest.skip("unbuilt checkout: no libegnn_hip.so")
    compiled = set()
    for unit in ("edge_tail", "node_ops", "node_mlp_fused"):
        res = os.path.join(pkg, "csrc", "obj", unit + ".res")
        assert os.path.exists(res), f"libegnn_hip.so exists but csrc/obj/{unit}.res does not: build with csrc/build.sh"
        with open(res) as f:
            names = set(re.findall(r"Function Name: (\S+)", "\n".join(line for line in f if "Function Name:" in line)))
        assert names, unit
        for name in names:
            found = re.search(r"\d+([a-z0-9_]+_kernel)(?:IL([bi])(\d+)EE)?(?:E|P|v)", name)
            assert found, f"{unit}: a kernel this table cannot name: {name}"
            arg = ""
            if found.group(2) == "b":
                arg = "<true>" if found.group(3) == "1" else "<false>"
            elif found.group(2) == "i":
                arg = f"<{found.group(3)}>"
            compiled.add(found.group(1) + arg)
    assert compiled == set(V.GLUE_KERNELS), dict(without_a_cell=sorted(compiled - set(V.GLUE_KERNELS)), not_compiled=sorted(set(V.GLUE_KERNELS) - compiled))
    with open(os.path.join(ROOT, "tests", "test_gpu_glue_variants.py")) as f:
        text = f.read()
    for kernel, test in V.GLUE_KERNELS.items():
        assert test is None or f"def {test.split('[')[0]}(" in text, (kernel, test)


def test_the_tail_launcher_and_nmf_supported_restated():
    k = V.tail_kernel
    assert k(False, 0, False) == k(False, 0, True) == "edge_tail_bwd_kernel<false>"
    assert k(True, 0, False) == "edge_tail_mfma_kernel<false>" and k(True, 7, False) == "edge_tail_mfma_kernel<true>"
    assert k(True, 0, True) == "edge_tail_bwd_kernel<true>"
    assert k(False, 7, False) == k(False, 7, True) == k(True, 7, True) == V.E_UNSUPPORTED
    assert set(V.MODE_KERNEL.values()) == {n for n in V.GLUE_KERNELS if n.startswith("edge_tail_")}
    modes = Counter(m for c in V.TAIL_CELLS for m in V.tail_modes(c))
    assert modes["plain"] == modes["mfma"] == modes["scalar"] >= 35 and modes["mfma_drop"] >= 19, modes
    with open(os.path.join(ROOT, "egnn_pytorch_amd", "csrc", "edge_tail.hip")) as f:
        launches = re.findall(r"hipLaunchKernelGGL\((edge_tail_\w+<\w+>)", f.read())
    assert sorted(launches) == sorted(V.MODE_KERNEL.values())                     # four launch lines, four modes
    assert [(d, m) for d in range(16, 300, 16) for m in (8, 16, 32) if V.nmf_supported(d, m)] == [(32, 16), (64, 16), (128, 16), (256, 16)]
    assert {f"node_mlp_fused_kernel<{d // 16}>" for d in V.NMF_DIMS} == {n for n in V.GLUE_KERNELS if n.startswith("node_mlp_fused_kernel")}


def _param_grads(r):
    return {"coors_mlp.0.weight": r["g_hid"].t() @ r["m"], "coors_mlp.0.bias": r["g_hid"].sum(0), "coors_mlp.3.weight": (r["g_w"] @ r["a3"])[None],
            "coors_mlp.3.bias": r["g_w"].sum()[None], "coors_norm.scale": None if r["g_scale"] is None else r["g_scale"].sum()[None],
            "edge_gate.0.weight": None if r["g_gate"] is None else (r["g_gate"] @ r["m0"])[None],
            "edge_gate.0.bias": None if r["g_gate"] is None else r["g_gate"].sum()[None]}


def test_the_dropout_extension_without_a_mask_is_the_closed_form():
    from egnn_pytorch_amd import autograd as A
    for cid in ("base_e80", "mask_scattered", "norm_off", "gate_none", "combo_dense_mask_m7", "clamp_zero"):
        d = V.prepare(cid)
        want = A.tail_edge_backward(d.layer, d.u, d.coors, d.idx, d.pm, d.g_co, d.g_msum)
        keep = torch.ones(d.e, d.hid3, dtype=torch.bool)
        got = V.tail_spec_drop(d.layer, d.u, d.coors, d.idx, d.pm, d.g_co, d.g_msum, keep, 1.0)
        for name, w in want.items():
            assert (w is None and got[name] is None) or torch.equal(got[name].detach(), w.detach()), (cid, name)


@pytest.mark.parametrize("cid,graph_offset", [("drop_p1_eid0", 0), ("drop_p5_eid0", 0), ("drop_p5_eid0", 3), ("drop_p1_eid4096", 5)])
def test_the_dropout_extension_equals_autograd_of_layer_tail(cid, graph_offset):
    """`tail_spec_drop` with the hash mask of (seed, SITE_COORS, eid0 + edge, unit) against float64 autograd of
    autograd.layer_tail(..., drop=..., graph_offset=...), the way test_closed_form_tail_backward_equals_autograd ties the plain one"""
    from egnn_pytorch_amd import autograd as A, _dropout
    d = V.prepare(cid)
    layer, b, n, k, m = d.layer, d.b, d.n, d.k, d.m
    assert d.pm is None and d.drop is not None
    g = torch.Generator().manual_seed(17)
    feats = torch.randn(b, n, 4, generator=g, dtype=torch.float64)
    gn = torch.randn(b, n, 4, generator=g, dtype=torch.float64)
    u = d.u.clone().requires_grad_(True)
    rel_leaf = A.edge_scalars(layer, d.coors, None, d.idx)[0].detach().requires_grad_(True)
    out_n, out_c = A.layer_tail(layer, feats, d.coors, u, rel_leaf, None, d.idx, None, float("inf"), drop=d.drop, graph_offset=graph_offset)
    names = [nme for nme, _ in layer.named_parameters() if nme.startswith(("coors_mlp", "coors_norm", "edge_gate"))]
    params = [prm for nme, prm in layer.named_parameters() if nme in names]
    grads = torch.autograd.grad([out_n, out_c], [u, rel_leaf] + params, [gn, d.g_co])
    want = dict(g_u=grads[0].reshape(d.e, m), g_rel=grads[1].reshape(d.e, 3), **dict(zip(names, grads[2:])))
    m_leaf = d.ref["m"].reshape(b, n, k, m).sum(2).clone().requires_grad_(True)
    rows = (torch.arange(b * n) + graph_offset * n).view(b, n)
    node_out = A._mlp_drop(layer.node_mlp, torch.cat((layer.node_norm(feats), m_leaf), -1), d.drop, _dropout.SITE_NODE, rows) + feats
    g_msum = torch.autograd.grad(node_out, m_leaf, gn)[0]
    r = V.tail_spec(layer, d.u, d.coors, d.idx, None, d.g_co, g_msum, d.drop, graph_offset * n * k)
    assert 0.2 < float(r["keep"].float().mean()) < 0.97
    if graph_offset * n * k == d.eid0:                                           # the cell's own numbering: the cell's own mask
        assert torch.equal(r["keep"], d.ref["keep"])
    else:                                                                        # edges numbered from another offset: another mask
        assert not torch.equal(r["keep"], d.ref["keep"])
    got = dict(g_u=r["g_u"].reshape(d.e, m), g_rel=r["g_rel"].reshape(d.e, 3), **_param_grads(r))
    assert float(want["coors_mlp.3.weight"].abs().max()) > 0
    for key, w in want.items():
        torch.testing.assert_close(got[key].reshape(w.shape), w, rtol=1e-9, atol=1e-9 * max(1.0, float(w.abs().max())), msg=key)


def test_the_silu_dropout_specification_by_hand():
    from egnn_pytorch_amd import _dropout
    g = torch.Generator().manual_seed(2)
    z, gr = torch.randn(9, 7, generator=g, dtype=torch.float64), torch.randn(9, 7, generator=g, dtype=torch.float64)
    a, gz = V.silu_spec(z, gr, torch.float64, (0.5, 999), row0=4)
    keep = _dropout.keep_mask(999, _dropout.SITE_NODE, torch.arange(9) + 4, torch.arange(7), 0.5)
    zd = torch.where(keep, 2.0 * z, torch.zeros_like(z))
    sg = torch.sigmoid(zd)
    assert bool(keep.any()) and not bool(keep.all())
    torch.testing.assert_close(a, zd * sg, rtol=1e-14, atol=0)
    torch.testing.assert_close(gz, gr * sg * (1 + zd * (1 - sg)) * keep * 2.0, rtol=1e-13, atol=1e-300)
    a0, gz0 = V.silu_spec(z, gr, torch.float64)
    torch.testing.assert_close(gz0, gr * torch.sigmoid(z) * (1 + z * (1 - torch.sigmoid(z))), rtol=1e-13, atol=0)


def test_the_bit_exact_restatements_on_the_host():
    from egnn_pytorch_amd import _weights
    rng = np.random.default_rng(3)
    # the (hi, lo) image: hi the nearest fp16, hi + lo within 2^-22 relative of the value (fp16's normal range)
    x = (rng.standard_normal((33, 20)) * 50).astype(np.float32)
    hi, lo = V.split_image(x, 0.5)
    y = x * np.float32(0.5)
    assert np.array_equal(hi, y.astype(np.float16)) and np.abs(hi.astype(np.float64) + lo.astype(np.float64) - y).max() <= 2.0 ** -22 * np.abs(y).max()
    # `unpack_full` inverts `_weights.pack_tiles`, pad rows included
    img = np.zeros((64, 32), dtype=np.float16)
    img[:33, :20] = hi
    flat = _weights.pack_tiles(torch.from_numpy(img))
    assert V.same_bits(V.unpack_full(flat, 33, 32), img) and V.unpack_full(flat, 33, 32).shape == (64, 32)
    assert not V.same_bits(np.float16([0.0]), np.float16([-0.0]))                # bits, not values
    # the summation orders are orders of the same sum
    for rows in (1, 2, 5, 6, 768, 4096):
        part = rng.standard_normal((rows, 8)).astype(np.float32)
        got = V.sum_rows_order(part, 0.37)
        want = part.astype(np.float64).sum(0) * 0.37
        assert got.dtype == np.float32 and np.abs(got - want).max() <= 1e-6 * np.abs(part).sum(0).max()
    x = rng.standard_normal((129, 9)).astype(np.float32)
    cs, parts = V.colsum_order(x, 8.0, 12)
    assert parts.shape == (3, 12) and not parts[:, 9:].any() and not cs[9:].any()
    assert np.abs(cs[:9] - x.astype(np.float64).sum(0)).max() <= 1e-6 * np.abs(x).sum(0).max()
    flipped = x.copy()
    flipped[:64] = x[:64][::-1]                                                  # another order of the same rows: other bits somewhere
    assert np.abs(V.colsum_order(flipped, 8.0, 12)[0] - cs).max() <= 1e-5


def test_the_node_level_cells_cover_their_axes():
    assert {c["n"] for c in V.POOL_CELLS} == {1, 15, 16, 17, 33} and {c["k"] for c in V.POOL_CELLS} == {1, 5, 32, 64}
    assert {c["gate"] for c in V.POOL_CELLS} == {True, False} and {c["mask"] for c in V.POOL_CELLS} >= {"none", "ragged", "scattered", "node", "all"}
    for c in V.POOL_CELLS:
        u, gate, pm, ref, bar = V.pool_case(c)
        assert 0 < bar <= V.EDGE_CAP * float(ref.abs().max()) * (1 + 1e-12) or c["mask"] == "all"
        if c["mask"] in ("node", "all"):
            assert bool((~pm[0].any(-1)).any()) and not bool(ref[0][~pm[0].any(-1)].any())
    main = [c for c in V.PREP_CELLS if c["data"] == "randn" and c["rows"] <= 300]
    assert {c["dim"] for c in main} == set(V.PREP_DIMS) and {c["rows"] for c in main} == set(V.PREP_ROWS)
    for dim in V.PREP_DIMS:                                                      # every width with and without LayerNorm
        assert {c["ln"] for c in main if c["dim"] == dim} == {True, False}
    assert {(c["mi"], c["ln"]) for c in main} == {(True, True), (True, False), (False, True), (False, False)}
    assert any(c["raw"] for c in main) and any(c["dim"] + 16 > 128 and c["dim"] <= 124 for c in main)
    assert any(c["rows"] > 262144 for c in V.PREP_CELLS) and {c["data"] for c in V.PREP_CELLS} == {"randn", "const", "mean1e4"}
    assert {c["rows"] for c in V.SPLIT_CELLS} == set(V.SPLIT_ROWS) and {c["cols"] for c in V.SPLIT_CELLS} == set(V.SPLIT_COLS)
    assert {c["ldx_extra"] for c in V.SPLIT_CELLS} == {0, 3, 4}
    assert {c["cols"] for c in V.SILU_DROP} == {4, 5, 6, 7, 130} and {c["p"] for c in V.SILU_DROP} == {0.1, 0.5}
    assert all(c["rows"] * c["cols"] % 4 == 0 and c["rows"] > 4 for c in V.SILU_DROP)
    x, mi, gamma, beta = V.prep_case(next(c for c in V.PREP_CELLS if c["data"] == "const"))
    assert float(x[0].var()) == 0.0 and float(x[1].var()) > 0
    x, _, _, _ = V.prep_case(next(c for c in V.PREP_CELLS if c["data"] == "mean1e4"))
    assert abs(float(x.mean()) - 1e4) < 1 and 0.8 < float(x.std()) < 1.2
    c = V.nmf_case(32, 17)
    assert float(c.bar.max()) <= V.NMF_CAP * max(1.0, float(c.ref.abs().max())) * (1 + 1e-12) and float(c.bar.min()) > 0

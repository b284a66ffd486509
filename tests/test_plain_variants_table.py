"""tests/_plain_variants.py on the host: the table covers the grid of the three plain launchers (csrc/edge_exact.hip,
csrc/edge_exact_bwd.hip, csrc/edge_hidden.hip) exactly once per instantiation AND equals what the compiler instantiated, the restated
thresholds and LDS formulas hold at their boundary values, no cell's call can address memory it does not own, every cell meets the
preconditions that make its GPU comparison (tests/test_gpu_plain_variants.py) decidable -- on the float64 specification alone -- and
the specification itself is tied to the project's oracle and to the closed forms of egnn_pytorch_amd/autograd.py."""
import os
import re
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _plain_variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I = V.Inst


def test_the_table_is_exactly_the_instantiation_grid():
    insts = [c.inst for c in V.MAIN]
    assert len(insts) == 48 and len(set(insts)) == 48
    assert set(insts) == V.grid()
    assert len({c.id for c in V.CELLS}) == len(V.CELLS)
    assert Counter(c.entry for c in V.MAIN) == Counter(fwd=10, silu=2, bwd=8, sums=2, tail=6, hfwd=7, hbwd=8, hbwd2=5)
    assert Counter(c.inst.kernel for c in V.MAIN)["edge_exact_pool_kernel"] == 2 and all(c.t == c.inst.T for c in V.MAIN)
    for c in V.CELLS:
        got = V.expected(c.entry, c.t, c.p)
        if c.expect is not None:
            assert got == c.expect and c.inst is None and f"refused{-c.expect}" in c.id, c.id
        else:
            assert c.inst == got[c.p["pin"]] and c.inst in V.grid(), c.id
            assert c.id.startswith(V.inst_name(c.inst) + "_"), c.id                # the collected ids name the instantiation
    assert {c.inst for c in V.RUN} == set(insts)


def test_the_table_equals_what_the_compiler_instantiated():
    """csrc/build.sh leaves the compiler's resource-usage remarks of every translation unit next to its object; the `Function Name:`
    remarks name the kernels that exist.  A new `run(edge_..._kernel<T, N>)` line fails here until it has a cell."""
    pkg = os.path.join(ROOT, "egnn_pytorch_amd")
    if not os.path.exists(os.path.join(pkg, "libegnn_hip.so")):
        pytest.skip("unbuilt checkout: no libegnn_hip.so")
    compiled = set()
    for unit in ("edge_exact", "edge_exact_bwd", "edge_hidden"):
        res = os.path.join(pkg, "csrc", "obj", unit + ".res")
        assert os.path.exists(res), f"libegnn_hip.so exists but csrc/obj/{unit}.res does not: build with csrc/build.sh"
        with open(res) as f:
            text = "\n".join(line for line in f if "Function Name:" in line)
        names = set(re.findall(r"Function Name: (\S+)", text))
        assert names, unit
        for name in names:
            found = re.search(r"\d+((?:edge|drop)_[a-z0-9_]*kernel)I([fd])(?:Li(\d+)E)?E", name)
            assert found, f"{unit}: a kernel this table cannot name: {name}"
            compiled.add(I(found.group(1), found.group(2), int(found.group(3)) if found.group(3) else -1))
    print(f"compiled: {len(compiled)} instantiations")
    table = {c.inst for c in V.MAIN}
    assert compiled == table, dict(without_a_cell=sorted(compiled - table), not_compiled=sorted(table - compiled))
    assert len(compiled) == 48


def test_the_dispatch_restatement_at_its_thresholds_and_refusals():
    mb = lambda entry, t, m: V.dispatch(entry, t, m)[0].MB                         # noqa: E731
    ms = (16, 17, 32, 33, 64, 65)
    for t in "fd":
        assert [mb("fwd", t, m) for m in ms] == [16, 32, 32, 64, 64, -1]
        assert V.dispatch("fwd", t, 65)[0].kernel == "edge_exact_wide_kernel" and V.dispatch("fwd", t, 64)[1].kernel == "edge_exact_pool_kernel"
        assert [mb("bwd", t, m) for m in ms] == [16, 32, 32, 64, 64, 0]
        assert [mb("hbwd", t, m) for m in ms] == [16, 32, 32, 64, 64, 0]
        assert [mb("tail", t, m) for m in ms[:5]] == [16, 32, 32, 64, 64] and V.dispatch("tail", t, 65) == V.E_UNSUPPORTED
        assert V.dispatch("fwd", t, 1025) == V.E_UNSUPPORTED and V.dispatch("bwd", t, 0) == V.E_UNSUPPORTED
        assert V.dispatch("fwd", t, 16, 65, fourier=32) == V.E_UNSUPPORTED
        for entry in V.EDGE_ENTRIES:
            assert V.dispatch(entry, t, has_idx=False, k_is_n=False) == V.E_SHAPE
            assert not isinstance(V.dispatch(entry, t, has_idx=False, k_is_n=True), int)
        for entry in V.DROP_ENTRIES:                                             # the 32-bit dropout rows: drop_eid0 + E <= 2^32 - 1
            assert V.dispatch(entry, t, e=80, drop=(0.5, 0)) == V.E_SHAPE
            assert V.dispatch(entry, t, e=80, drop=(4 / 3, -1)) == V.E_SHAPE
            assert V.dispatch(entry, t, e=80, drop=(4 / 3, 2 ** 32 - 80)) == V.E_SHAPE
            assert not isinstance(V.dispatch(entry, t, e=80, drop=(4 / 3, 2 ** 32 - 81)), int)
    assert [mb("hfwd", "f", m) for m in ms] == [16, 32, 32, 64, 64, 0]            # the float64 exceptions: fwd<64> and bwd2<32> are float only
    assert [mb("hfwd", "d", m) for m in ms] == [16, 32, 32, 0, 0, 0]
    assert [mb("hbwd2", "f", m) for m in ms] == [16, 32, 32, 0, 0, 0]
    assert [mb("hbwd2", "d", m) for m in ms] == [16, 0, 0, 0, 0, 0]
    # the LDS bytes of three cells by hand, the opt-in and the refusal at their S values
    assert V.lds_bytes("fwd", "f", 65) == 65 * 1024 == 66560
    assert V.lds_bytes("bwd", "d", 17) == 2 * 17 * 256 * 8 == 69632
    assert V.lds_bytes("hbwd2", "d", 21) == 3 * 21 * 2048 == 129024
    sides = {("fwd", "f"): 64, ("fwd", "d"): 32, ("hfwd", "f"): 64, ("hfwd", "d"): 32, ("bwd", "f"): 32, ("bwd", "d"): 16,
             ("hbwd", "f"): 32, ("hbwd", "d"): 16, ("hbwd2", "f"): 21, ("hbwd2", "d"): 10}
    tops = {("fwd", "f"): 160, ("fwd", "d"): 80, ("hfwd", "f"): 160, ("hfwd", "d"): 80, ("bwd", "f"): 80, ("bwd", "d"): 40,
            ("hbwd", "f"): 80, ("hbwd", "d"): 40, ("hbwd2", "f"): 53, ("hbwd2", "d"): 26}
    for (entry, t), s in sides.items():
        assert not V.opts_in(entry, t, s) and V.opts_in(entry, t, s + 1), (entry, t)
        top = tops[entry, t]
        assert V.max_s(entry, t) == top
        assert not isinstance(V.dispatch(entry, t, 16, top), int) and V.dispatch(entry, t, 16, top + 1) == V.E_UNSUPPORTED
        cells = {V.s_of(c.p): c for c in V.CELLS if c.entry == entry and c.t == t and c.group in ("lds", "smax", "smax1")}
        assert set(cells) == {s, s + 1, top, top + 1}, (entry, t, sorted(cells))
        assert cells[top].expect is None and cells[top + 1].expect == V.E_UNSUPPORTED and cells[top + 1].group == "smax1"
        assert all(c.p["fourier"] == 0 and c.p["H"] == 8 for c in cells.values())


def test_the_cells_beside_the_grid_are_all_there():
    def has(entry, t, group, **kw):
        return any(c.entry == entry and c.t == t and c.group == group and all(c.p[k] == v for k, v in kw.items()) for c in V.CELLS)
    for t in "fd":
        for entry in ("fwd", "bwd"):
            for f in (0, 2, 31):
                assert has(entry, t, "four", fourier=f) == (2 * f + 1 <= V.max_s(entry, t)), (entry, t, f)
            assert has(entry, t, "stride", strided=True)
        assert has("fwd", t, "four", fourier=31) and has("bwd", "f", "four", fourier=31)
        for entry in ("fwd", "bwd", "tail"):
            assert {c.p["cdim"] for c in V.CELLS if c.entry == entry and c.t == t and c.group == "cdim"} == {3, 2, 5, 8, 9, 11}
        for entry in V.EDGE_ENTRIES:
            assert {V.e_of(c.p) for c in V.CELLS if c.entry == entry and c.t == t and c.group == "eshape"} == {256, 280, 40}
            assert has(entry, t, "eshape", b=2, n=16, k=8) and has(entry, t, "eshape", b=2, n=20, k=7)
            assert has(entry, t, "refuse", no_idx=True)
            # every threshold of the entry: a MAIN cell at it (the kernel's last channel in use), a cell at the first head behind it
            steps = [m for m in range(1, 100) if not isinstance(V.dispatch(entry, t, m + 1), int) and V.dispatch(entry, t, m) != V.dispatch(entry, t, m + 1)]
            assert steps and set(steps) <= {16, 32, 64}, (entry, t, steps)
            for m in steps:
                assert has(entry, t, "main", m=m) and has(entry, t, "mstep", m=m + 1), (entry, t, m)
        for o in V.FWD_OPTS:
            assert has("fwd", t, "opt", opts=(o,)), o
        assert has("fwd", t, "opt", opts=("dense",), dense=True, by_k=False) and has("fwd", t, "opt", opts=("dense_by_k",), dense=True, by_k=True)
        for o in V.TAIL_OPTS:
            assert has("tail", t, "opt", opts=(o,)), o
        for entry in V.DROP_ENTRIES:
            assert has(entry, t, "drop", drop="one") and has(entry, t, "drop", drop="split")
            assert has(entry, t, "refuse", bad_inv=True)
        assert has("tail", t, "refuse", m=65)
    for c in V.CELLS:                                                            # strided: ldp = 2 hq > H, ldws = Din > S
        if c.p["strided"]:
            d = V.prepare(c.id)
            assert 2 * d.hq > c.p["H"] and d.hq >= c.p["H"] and c.p["H"] % 4 != 0 and d.glob["w1"].shape[1] > d.s


def test_every_call_is_valid_from_the_table_alone():
    """every extent a kernel reads or writes, recomputed from the cell's arguments and compared with what `prepare` /
    `output_shapes` allocate (the GPU test allocates exactly those)"""
    for c in V.CELLS:
        p, d = c.p, V.prepare(c.id)
        shapes = V.output_shapes(c.id)
        if c.entry == "silu":
            assert tuple(d.glob["Z"].shape) == (p["rows"], p["cols"]) == shapes["Z"]
            continue
        b, n, k, m, h, cd, s, e = p["b"], p["n"], p["k"], p["m"], p["H"], p["cdim"], V.s_of(p), V.e_of(p)
        nodes = b * n
        size = lambda group, name: tuple(getattr(d, group)[name].shape)          # noqa: E731
        if "idx" in d.edge:
            assert size("edge", "idx") == (e,) and int(d.edge["idx"].min()) >= 0 and int(d.edge["idx"].max()) < n, c.id
        else:
            assert k == n, c.id
        assert int(d.dst.max()) < nodes and int(d.src.max()) == nodes - 1 and bool((d.dst // n == d.src // n).all()), c.id
        want = {}
        if c.entry in ("fwd", "bwd", "sums"):
            if p["strided"]:                                                     # rows of ldp = 2 hq: P_i at 0, P_j at hq; W_s behind 2 dim columns
                ldp, din = 2 * d.hq, 2 * d.dim + s
                assert size("node", "proj") == (nodes, ldp) and d.hq + (nodes - 1) * ldp + h <= nodes * ldp, c.id
                assert size("glob", "w1") == (h, din) and 2 * d.dim + (h - 1) * din + s <= h * din, c.id
            else:
                assert size("node", "Pi") == size("node", "Pj") == (nodes, h) and size("glob", "Ws") == (h, s), c.id
            assert size("glob", "W2") == (m, h) and size("node", "coors") == (nodes, cd), c.id
            if p["edge_dim"]:
                if p["by_k"]:                                                    # q edge_dim
                    assert size("edge", "edges") == (e, p["edge_dim"]), c.id
                else:                                                            # ((b N + i) N + j) edge_dim
                    assert size("node", "edges") == (nodes, n, p["edge_dim"]), c.id
                    assert ((nodes - 1) * n + (n - 1)) * p["edge_dim"] + p["edge_dim"] == d.node["edges"].numel(), c.id
        if c.entry == "fwd":
            want = dict(ws=(e, m + cd + 1), m_i=(nodes, m), coors_out=(nodes, cd), U_out=(e, m))       # the workspace row: m_dim + C + 1
            assert size("glob", "b2") == (m,), c.id
            for name, shp in (("gate_w", (m,)), ("gate_b", (1,)), ("W3", (4 * m, m)), ("b3", (4 * m,)), ("W4", (4 * m,)), ("b4", (1,)), ("scale", (1,))):
                assert name not in d.glob or size("glob", name) == shp, (c.id, name)
            assert "mask" not in d.node or size("node", "mask") == (nodes,)
            assert "rank" not in d.edge or size("edge", "rank") == (e,)
        elif c.entry in ("bwd", "sums"):
            want = dict(A_T=(h, e), DZ_T=(h, e), g_scal=(e, s), gPi=(nodes, h), gPi_T=(h, nodes), gPj=(nodes, h), gPj_T=(h, nodes))
            assert size("edge", "gU") == (e, m), c.id
        elif c.entry == "tail":
            want = dict(gU=(e, m), g_rel_t=(cd, e), mm_t=(m, e), ghid_t=(4 * m, e), a3_t=(4 * m, e), g_w=(e,), g_scale=(e,), m0_t=(m, e), g_gate=(e,))
            assert size("edge", "u") == (e, m) and size("node", "coors") == (nodes, cd) and size("node", "g_co") == (nodes, cd), c.id
            assert "g_msum" not in d.node or size("node", "g_msum") == (nodes, m)
            assert "pair_mask" not in d.edge or size("edge", "pair_mask") == (e,)
        else:
            want = dict(u=(e, m), A_T=(h, e), DZ_T=(h, e), g_s=(e, s), g_gU=(e, m), DAV_T=(h, e), R_T=(h, e))
            assert size("node", "Pi") == size("node", "Pj") == (nodes, h) and size("edge", "s") == (e, s), c.id
            assert size("glob", "Ws") == (h, s) and size("glob", "W2") == (m, h) and size("glob", "b2") == (m,), c.id
            if c.entry != "hfwd":
                assert size("edge", "gU") == (e, m), c.id
            if c.entry == "hbwd2":
                assert size("node", "cPi") == size("node", "cPj") == (nodes, h) and size("edge", "cs") == (e, s), c.id
                assert size("glob", "cWs") == (h, s) and size("glob", "cW2") == (m, h) and size("glob", "cb2") == (m,), c.id
        assert shapes and all(shapes[name] == want[name] for name in shapes), (c.id, shapes)
        assert V.lds_bytes(c.entry, c.t, s) <= V.LDS_MAX or c.expect == V.E_UNSUPPORTED, c.id
        assert e <= 300 and h <= 24 and m <= 80, c.id                            # every case stays a handful of tiny launches


def test_every_cell_meets_its_preconditions_on_the_reference():
    seen = Counter()
    for c in V.RUN:
        d = V.prepare(c.id)
        ref, aux = V.reference(c.id)
        opts = c.p["opts"]
        for name, r in ref.items():
            assert bool(torch.isfinite(r).all()) and r.numel() > 0, (c.id, name)
            if not (c.entry == "fwd" and name == "ws_wrel" and "no_w3" in opts) and not (c.entry == "tail" and name == "g_rel_t" and "no_w3" in opts):
                assert float(r.abs().max()) > 0, (c.id, name)
        if "clamp" in opts:                                                      # some but not all weights clamp, none undecidable
            cw = aux["cw"].abs()
            live = cw[cw > 0]
            assert bool((live > V.CLAMP).any()) and bool((live < V.CLAMP).any()), c.id
            assert float((cw - V.CLAMP).abs().min()) > 1e-6, c.id
            seen["clamp"] += 1
        if "rank" in d.edge:
            assert float((d.edge["rank"] - d.valid_radius).abs().min()) > 1e-9, c.id
            inside = d.edge["rank"] <= d.valid_radius
            assert bool(inside.any()) and not bool(inside.all()), c.id
            seen["rank"] += 1
        if "norm" in aux:                                                        # CoorsNorm: only the self pair sits below the clamp to eps
            small = aux["norm"].reshape(-1) < 1e-3
            assert bool((small == (d.src == d.dst)).all()), c.id
            seen["norm"] += 1
        for key in ("keep_e", "keep_c"):
            if d.drop is not None and (key == "keep_e" or key in aux) and aux.get(key) is not None:
                frac = float(aux[key].float().mean())
                assert 0.5 < frac < 0.95, (c.id, key, frac)
                seen[key] += 1
        if d.drop is not None:
            assert aux.get("keep_e") is not None or aux.get("keep_c") is not None, c.id
        if aux.get("pair") is not None:
            assert bool(aux["pair"].any()) and not bool(aux["pair"].all()), c.id
            assert not bool(ref["ws_m"][~aux["pair"]].any()) and not bool(ref["ws_wrel"][~aux["pair"]].any())
            seen["pair"] += 1
        if "cnt" in aux:                                                         # a query node with no kept edge: its m_i row is exact zeros
            empty = (aux["cnt"] == 0).reshape(-1)
            assert bool(empty.any()) and not bool(empty.all()) and not bool(ref["m_i"][empty].any()), c.id
            seen["cnt0"] += 1
        if c.entry == "tail":
            self_pair = d.src == d.dst
            assert bool(self_pair.any()) and not bool(ref["g_rel_t"][:, self_pair].any()), c.id
            if "pair_mask" in d.edge:
                assert not bool(ref["g_w"][~d.edge["pair_mask"]].any()), c.id
            if "clamp" in opts:
                assert not bool(ref["g_w"][aux["cw"].abs() > V.CLAMP].any()), c.id
    assert seen["clamp"] == 4 and seen["rank"] == 2 and seen["cnt0"] >= 4 and seen["norm"] >= 8 and seen["pair"] >= 8, seen
    assert seen["keep_e"] >= 20 and seen["keep_c"] >= 8, seen


def test_the_per_edge_tables_contract_to_the_closed_form_specifications():
    """the hidden block's tables against `edge_hidden_backward_spec` / `edge_hidden_double_backward_spec`, the tail's autograd
    restatement against `tail_edge_backward`: the per-edge forms the GPU cells are held to ARE those specifications"""
    from egnn_pytorch_amd import autograd as A
    close = lambda a, w: float((a - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max()))     # noqa: E731
    n_h = n_t = 0
    for c in V.RUN:
        d = V.prepare(c.id)
        ref, _ = V.reference(c.id)
        if c.entry in ("hbwd", "hbwd2") and c.group in ("main", "drop"):
            (p_i, p_j, s, w_s, w2), idx, drop, dims = V._hidden_args(d, torch.float64, 0)
            g_u = d.edge["gU"]
            zeros = torch.zeros_like(p_i)
            if c.entry == "hbwd":
                want = A.edge_hidden_backward_spec(g_u, p_i, p_j, s, w_s, w2, idx, drop, dims)
                dz = ref["DZ_T"].t()
                got = (zeros.index_add(0, d.src, dz), zeros.index_add(0, d.dst, dz), ref["g_s"], dz.t() @ s, g_u.t() @ ref["A_T"].t())
            else:
                cot = [d.node["cPi"], d.node["cPj"], d.edge["cs"], d.glob["cWs"], d.glob["cW2"], d.glob["cb2"]]
                want = A.edge_hidden_double_backward_spec(g_u, p_i, p_j, s, w_s, w2, idx, drop, dims, cot)
                r, dz = ref["R_T"].t(), ref["DZ_T"].t()
                got = (ref["g_gU"], zeros.index_add(0, d.src, r), zeros.index_add(0, d.dst, r), ref["g_s"], r.t() @ s + dz.t() @ cot[2],
                       g_u.t() @ ref["DAV_T"].t())
            for a, w in zip(got, want):
                assert close(a, w), c.id
            n_h += 1
        if c.entry == "tail" and d.drop is None and "W3" in d.glob:
            auto, _ = V.spec_tail_autograd(d, torch.float64)
            assert set(auto) == set(ref), c.id
            for name in ref:
                assert close(auto[name].detach(), ref[name]), (c.id, name)
            n_t += 1
    assert n_h >= 20 and n_t >= 20, (n_h, n_t)


def test_the_forward_restatement_reproduces_the_oracle():
    """`spec_fwd` fed with P = feats W^T + b of a float64 layer with a mask, Fourier features and edge features, followed by the oracle's
    node MLP, against `oracle.egnn_forward` at 1e-12 of each output's scale"""
    from oracle import egnn_oracle as O
    cfg = O.EGNNConfig(dim=6, edge_dim=2, m_dim=16, fourier_features=2, num_nearest_neighbors=4, norm_coors=True, soft_edges=True,
                       coor_weights_clamp_value=0.05, m_pool_method="mean", valid_radius=1.5)
    prm = O.random_params(cfg, 5, dtype=np.float64)
    rng = np.random.default_rng(11)
    b, n, k, dim = 2, 9, 4, 6
    feats, coors, edges = rng.standard_normal((b, n, dim)), rng.standard_normal((b, n, 3)) * 0.7, rng.standard_normal((b, n, n, 2))
    mask = rng.random((b, n)) > 0.2
    mask[:, 0] = True
    node, co, ranking, nbr = O.egnn_forward(cfg, prm, feats, coors, edges, mask, return_neighbors=True)
    tt = lambda name: torch.from_numpy(np.ascontiguousarray(prm[name]))           # noqa: E731
    w1, b1 = tt("edge_mlp.0.weight"), tt("edge_mlp.0.bias")
    f2d = torch.from_numpy(feats).reshape(b * n, dim)
    idx = torch.from_numpy(nbr.astype(np.int64)).reshape(-1)
    d = SimpleNamespace(node=dict(coors=torch.from_numpy(coors).reshape(b * n, 3), edges=torch.from_numpy(edges).reshape(b * n, n, 2),
                                  mask=torch.from_numpy(mask).reshape(-1)),
                        edge=dict(idx=idx, rank=torch.from_numpy(ranking).reshape(-1)),
                        glob=dict(W2=tt("edge_mlp.3.weight"), b2=tt("edge_mlp.3.bias"), gate_w=tt("edge_gate.0.weight")[0],
                                  gate_b=tt("edge_gate.0.bias"), W3=tt("coors_mlp.0.weight"), b3=tt("coors_mlp.0.bias"),
                                  W4=tt("coors_mlp.3.weight")[0], b4=tt("coors_mlp.3.bias"), scale=tt("coors_norm.scale")),
                        pi=f2d @ w1[:, :dim].t() + b1, pj=f2d @ w1[:, dim:2 * dim].t(), ws=w1[:, 2 * dim:], b=b, n=n, k=k, e=b * n * k, s=7,
                        drop=None, valid_radius=1.5)
    d.src, d.dst = V.edge_ends(idx, b, n, k)
    d.cell = SimpleNamespace(entry="fwd", p=dict(V._DEFAULTS, m=16, fourier=2, edge_dim=2, cdim=3, opts=("mean", "mask_rank", "gate", "scale", "clamp")))
    saved = V.CLAMP
    V.CLAMP = 0.05
    try:
        out, aux = V.spec_fwd(d, torch.float64)
    finally:
        V.CLAMP = saved
    assert bool((aux["cw"].abs() > 0.05).any()) and not bool(aux["pair"].all())   # the clamp and the mask both act in this layer
    node_in = np.concatenate([feats, out["m_i"].numpy().reshape(b, n, 16)], axis=-1)
    hid = O.silu(O.linear(node_in, prm["node_mlp.0.weight"], prm["node_mlp.0.bias"]))
    mine = O.linear(hid, prm["node_mlp.3.weight"], prm["node_mlp.3.bias"]) + feats
    assert np.abs(mine - node).max() <= 1e-12 * np.abs(node).max()
    assert np.abs(out["coors_out"].numpy().reshape(b, n, 3) - co).max() <= 1e-12 * np.abs(co).max()

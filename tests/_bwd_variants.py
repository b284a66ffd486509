"""One test case per template instantiation of the register-contraction edge backward (csrc/edge_bwd.hip) -- the table behind
tests/test_gpu_bwd_variants.py, importable without a GPU.

`egnn_edge_bwd_pass_f32` picks `edge_bwd_kernel<NM, ST, WANT_W2, WANT_S, CH, PAIR, DROP, DSM>` from the number of per-edge scalars S
(five classes), from which of the two all-edge contractions the call asks for (d/d W_2; d/d W_s with d/d s), from `row_pairs` and from
`drop_thr`: 5 classes x {w2, ss, pair, none} x {plain, dropout} + the S = 1 kernel that carries everything, plain and dropout = 42
instantiations, and `edge_bwd_prep_kernel<NM>` once per class.  `instantiation()` restates that dispatch, `chunks()` / `slabs()` /
`lds_bytes()` the kernel's own partition of the hidden columns and of the entry list, `CELLS` holds one fixed call of
`_ops.edge_bwd_pass` per instantiation plus a few extra ones, `prepare()` builds a cell's layer, inputs and entry list on the host and
`reference()` the five contractions in float64 from the parameters alone.  A NEW INSTANTIATION NEEDS A NEW CELL:
tests/test_bwd_variants_table.py compares the table with what the compiler instantiated.

The cells are not drawn, they follow a rule (`_build_cells`):
    S        1 | 2, 4 | 5 | 6, 8 | 9, 16, alternating within a class; each value once mostly through edge_dim, once mostly through
             fourier_features
    family   w2    want_w2, by destination (the product's role); one extra cell per class by source
             ss    ws_nat, by source, K <= 16 or K > 32; one extra cell per class by destination
             pair  ws_nat, by source, row_pairs, K = 17, 24, 32 in rotation
             none  neither: the partial rows alone, by source and by destination alternating
             both  S = 1, want_w2 and ws_nat
             each without dropout and with drop = (p, seed): p = 0.5, every fourth 0.2; eid0 = 0 and 3 E alternating
    K        1, 5, 16 (one tile: ragged, full) and 33, 40 (three tiles, padding in the last) by source through `autograd.entry_list`;
             by destination the lists of `_ops.dest_lists`, half of them with `hub`: key 3 of every graph is pointed at by every node
             (more than two tiles) next to keys nobody points at
    n        K + 1 .. about 50 (hub: at least 34), b = 2;  m_dim 16, on a third of the cells 5 (pad channels of gU and of d/d W_2)
    width    Hp / 32 = 2, 8, 9, 13 steps (less than a chunk; exactly CH_S; 5 + 4; 5 + 4 + 4 under CH_W2) through `dim`; H == Hp on the
             even-S cells of every fourth position, H < Hp elsewhere
    slabs    n_slabs = ceil(rounds / r), r = 1, 2, 8 in rotation -- `_ops.edge_bwd_pass`'s own rule with another ROUNDS_PER_SLAB, which
             never leaves a slab empty; two extra cells with r = 1 and at least 35 rounds: two slab groups, the second partial
    weights  xavier-normal (tests/test_gpu_kernels.py::test_edge_bwd_pass_contractions_match_float64: with the default N(0, 1e-3) init
             SiLU' is nearly constant);  gU = randn 1e-3 with a fifth of its rows, all edges of one source node and all edges into one
             destination exactly zero
    init     one extra cell per family at the module's own initialisation (every Linear weight N(0, 1e-3), as EGNN.__init__ leaves it):
             z is then b1 + O(1e-2), SiLU(z) ~ 0.05 and dz ~ 1e-3 |gU| -- a training run's first steps, two orders below what the fixed
             up-scales of the kernel (DZ_UP, A_UP) were sized on.  Held to the same 5e-6 of scale, WITHOUT the absolute 1e-12"""
import functools
import zlib
from collections import namedtuple

# ------------------------------------------------------------------------------------------------ the dispatcher, restated
E_NULLPTR, E_SHAPE, E_UNSUPPORTED = -1, -2, -3                   # include/egnn_hip.h:34-36
CH_S, CH_W2, GS = 8, 6, 32                                       # csrc/edge_bwd.hip:58-67, :68-71, :61-64
BW_WAVES, XLD, DLD = 4, 36, 20                                   # csrc/edge_bwd.hip:66, :72, :248
ROUNDS_PER_SLAB = 8                                              # _ops.ROUNDS_PER_SLAB
S_CLASSES = ((1,), (2, 4), (5,), (6, 8), (9, 16))                # egnn_edge_mfmas, csrc/edge_fused.hip:1196
NM_ST = ((1, 1), (3, 4), (4, 5), (6, 2), (12, 2))                # csrc/edge_bwd.hip:878-882; launch_many's ST: :807-819
FAMILIES = ("w2", "ss", "pair", "none", "both")

Instantiation = namedtuple("Instantiation", "NM ST W2 SS CH PAIR DROP DSM")


def s_class(s):
    """the chain over S of egnn_edge_bwd_pass_f32 (csrc/edge_bwd.hip:878-882)"""
    assert 1 <= s <= 16
    return 0 if s == 1 else (1 if s <= 4 else (2 if s <= 5 else (3 if s <= 8 else 4)))


def instantiation(s, want_w2, want_s, row_pairs, drop, by_dest=False, k=17, has_wsth=True):
    """The kernel a call launches, or the entry's refusal code.  row_pairs is refused by the entry off its shapes (by destination, K <= 16,
    K > 32: csrc/edge_bwd.hip:863) and by launch_v where the variant has no PAIR form (:777); `launch` (:822-843) and `launch_many`
    (:801-820) pick the variant, CH_S for every variant but the one with d/d W_2 alone (CH_W2); more than five scalars put d/d s on the
    matrix cores (DSM), which needs the W_s^T fragments (:809, :816)."""
    if row_pairs and (by_dest or k <= 16 or k > 32):
        return E_SHAPE
    nm, st = NM_ST[s_class(s)]
    many = nm >= 6
    if want_w2 and want_s:
        if many or st != 1:                                                      # :804, :829, :838
            return E_UNSUPPORTED
        inst = Instantiation(nm, st, True, True, CH_S, False, bool(drop), False)
    elif want_w2:
        inst = Instantiation(nm, st, True, False, CH_W2, False, bool(drop), False)
    elif want_s:
        if many and not has_wsth:
            return E_NULLPTR
        inst = Instantiation(nm, st, False, True, CH_S, bool(row_pairs), bool(drop), many)
    else:
        inst = Instantiation(nm, st, False, False, CH_S, False, bool(drop), False)
    if row_pairs and not inst.PAIR:                                              # launch_v, :777
        return E_UNSUPPORTED
    return inst


def grid():
    """every instantiation the dispatcher can reach"""
    out = set()
    for s in (1, 2, 5, 6, 9):
        for drop in (False, True):
            for w2, ss, pairs in ((1, 0, 0), (0, 1, 0), (0, 1, 1), (0, 0, 0), (1, 1, 0)):
                inst = instantiation(s, w2, ss, pairs, drop)
                if not isinstance(inst, int):
                    out.add(inst)
    return out


def family(inst):
    return "both" if inst.W2 and inst.SS else ("w2" if inst.W2 else ("pair" if inst.PAIR else ("ss" if inst.SS else "none")))


def default_split_reaches(inst):
    """`autograd._edge_contract_fused`, the product's one distribution (its two `_ops.edge_bwd_pass` calls): by source with ws_nat (row_pairs where
    16 < K <= 32), by destination with want_w2 -- never a pass without a contraction, never one with both."""
    return family(inst) in ("w2", "ss", "pair")


def accepts_rows_amax(inst):
    """launch_v, csrc/edge_bwd.hip:791-792: the by-product exists where the tile sums are fp32 adds"""
    return not (inst.SS and inst.ST > 1)


def chunks(steps, ch):
    """(first step, steps) of every column chunk: n_chunks = ceil(steps / CH) (csrc/edge_bwd.hip:268), dealt out evenly -- base + 1 for
    the first `extra` chunks (:278-281)"""
    n_chunks = (steps + ch - 1) // ch
    base = steps // n_chunks
    extra = steps - base * n_chunks
    return [(c * base + min(c, extra), base + (1 if c < extra else 0)) for c in range(n_chunks)]


def slabs(rounds, n_slabs):
    """(per_slab, workgroups of one column chunk, slab groups): per_slab = ceil(rounds / n_slabs) (csrc/edge_bwd.hip:336-339); the grid
    holds whole groups of GS slabs per chunk (:786), the workgroups behind n_slabs return at once (:270-275)"""
    per_slab = (rounds + n_slabs - 1) // n_slabs
    groups = (n_slabs + GS - 1) // GS
    return per_slab, groups * GS, groups


def n_slabs_of(rounds, r):
    """_ops.edge_bwd_pass's rule (its `n_slabs is None` branch) with r for ROUNDS_PER_SLAB"""
    return max(1, (rounds + r - 1) // r)


def lds_bytes(inst):
    """launch_v, csrc/edge_bwd.hip:779-780"""
    lds = inst.CH * 2048 + inst.CH * 32 * 4 * inst.NM * 4 + BW_WAVES * 32 * XLD * 4
    if inst.DSM:
        lds += inst.CH * 2048 + BW_WAVES * 2 * 16 * DLD * 4
    return lds


# ------------------------------------------------------------------------------------------------ the table
K_SRC = (1, 5, 16, 33, 40)
K_PAIR = (17, 24, 32)
STEPS = (2, 8, 9, 13)
R_VALUES = (1, 2, 8)

Cell = namedtuple("Cell", "id inst fam kw s b n k m_dim steps by_dest hub row_pairs want_w2 want_s drop eid0 r seed extra")


def _kw_of(s, mostly_fourier, steps, exact, q, k, m_dim):
    fourier, edge_dim = ((s - 1) // 2, (s - 1) % 2) if mostly_fourier else (0, s - 1)
    hp = 32 * steps
    dim = (hp - 2 * s) // 4                                                      # H = 2 (2 dim + S) <= Hp
    if not (exact and s % 2 == 0):
        dim -= 1 + q % 3                                                         # 4 .. 14 pad columns
    assert dim >= 1 and hp - 32 < 2 * (2 * dim + s) <= hp
    return dict(dim=dim, num_nearest_neighbors=k, m_dim=m_dim, fourier_features=fourier, edge_dim=edge_dim)


def _build_cells():
    cells = []
    n_drop = [0]

    def add(si, fam, dropped, by_dest, k, steps, r, hub=False, mostly_fourier=False, s_pick=0, n=None, extra=None):
        q = len(cells)
        s = S_CLASSES[si][s_pick % len(S_CLASSES[si])]
        m_dim = 5 if q % 5 == 2 or q % 8 == 4 else 16
        kw = _kw_of(s, mostly_fourier, steps, q % 4 == 0, q, k, m_dim)
        if n is None:
            n = min(max(k + 1 + (3 * q) % 9, 9 + q % 7), 50)                     # (K = 1, 5: a few rounds all the same)
            if hub:
                n = max(n, 34 + q % 5)
        b = 2
        want_w2, want_s, pairs = fam in ("w2", "both"), fam in ("ss", "pair", "both"), fam == "pair"
        drop, eid0 = None, 0
        if dropped:
            d = n_drop[0]
            n_drop[0] += 1
            drop = 0.2 if (d + d // 4) % 4 == 3 else 0.5                        # (a quarter, walking through the families)
            eid0 = 0 if d % 2 == 0 else 3 * b * n * k
        inst = instantiation(s, want_w2, want_s, pairs, dropped, by_dest, k)
        assert isinstance(inst, Instantiation), (fam, s, by_dest, k, inst)
        cid = ("I" + "-".join(str(int(v)) for v in inst) + f"_{fam}{'D' if dropped else ''}_S{s}f{kw['fourier_features']}e{kw['edge_dim']}"
               f"_{'dst' if by_dest else 'src'}{'H' if hub else ''}_k{k}n{n}m{m_dim}_d{kw['dim']}st{steps}_r{r}{'_' + extra if extra else ''}")
        seed = zlib.crc32(cid.encode()) % (2 ** 30)
        cells.append(Cell(cid, inst, fam, kw, s, b, n, k, m_dim, steps, by_dest, hub, pairs, want_w2, want_s,
                          (drop, seed % (2 ** 31 - 1)) if dropped else None, eid0, r, seed, extra))

    # one cell per instantiation
    for si in range(5):
        for fi, fam in enumerate(FAMILIES[:4]):
            for di in (0, 1):
                by_dest = fam == "w2" or (fam == "none" and (si + di) % 2 == 1)
                k = K_PAIR[(si + di) % 3] if fam == "pair" else K_SRC[(si + 2 * fi + 3 * di) % 5]
                add(si, fam, bool(di), by_dest, k, STEPS[(si + fi + 2 * di) % 4], R_VALUES[(si + fi + di) % 3],
                    hub=by_dest and ((si + di) % 2 == 0 if fam == "w2" else si in (0, 3)), mostly_fourier=fi >= 2, s_pick=fi + di)
    add(0, "both", False, False, 5, 2, 1)
    add(0, "both", True, True, 16, 2, 2, hub=True)
    # the other role of the two contraction families, one cell per class
    for si in range(5):
        add(si, "w2", si % 2 == 1, False, K_SRC[(si + 1) % 5], STEPS[(si + 1) % 4], R_VALUES[si % 3], mostly_fourier=si % 2 == 0, s_pick=si,
            extra="role")
        add(si, "ss", si % 2 == 0, True, K_SRC[(si + 3) % 5], STEPS[(si + 2) % 4], R_VALUES[(si + 1) % 3], hub=si % 2 == 0,
            mostly_fourier=si % 2 == 1, s_pick=si + 1, extra="role")
    # the S = 1 kernel that carries everything, at a second width: 5 + 4 steps
    add(0, "both", False, True, 33, 9, 8, extra="wide")
    add(0, "both", True, False, 40, 9, 1, hub=False, extra="wide")
    # at least 35 rounds with one round per slab: two slab groups, the second partial
    add(1, "pair", False, False, 32, 9, 1, n=70, s_pick=0, extra="groups")
    add(2, "w2", False, True, 32, 13, 1, n=70, mostly_fourier=True, extra="groups")
    # the module's own initialisation, one cell per family
    add(1, "w2", False, True, 16, 8, 8, extra="init")
    add(3, "ss", False, False, 40, 9, 8, mostly_fourier=True, extra="init")
    add(2, "pair", False, False, 24, 2, 8, extra="init")
    add(4, "none", False, False, 5, 13, 8, extra="init")
    add(0, "both", False, False, 33, 8, 8, extra="init")
    return cells


CELLS = _build_cells()
MAIN = [c for c in CELLS if c.extra is None]
BY_ID = {c.id: c for c in CELLS}


# ------------------------------------------------------------------------------------------------ a cell's data, on the host
class Prepared:
    pass


@functools.lru_cache(maxsize=None)
def prepare(cid):
    """Layer, inputs, scalars and entry list of a cell on the host, from its seed alone (cached: the tests share it and leave it
    unchanged).
        .layer (CPU, float32)  .feats (B N, dim)  .coors  .edges  .idx (B, N, K) int64  .scal (E, S) float32 of `autograd.edge_scalars`
        .gu16 (E, 16) float32  .zero_rows (E,) bool  .src / .dst (E,) global node of either end
        .ent (L,) int32, .seg (B N + 1,) int64: the entry list and every key's range of tiles (= partial rows)"""
    import torch
    from egnn_pytorch_amd import EGNN, autograd
    cell = BY_ID[cid]
    b, n, k, m, s = cell.b, cell.n, cell.k, cell.m_dim, cell.s
    p = Prepared()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(cell.seed)
        layer = EGNN(**cell.kw)
        for mod in layer.modules():
            if isinstance(mod, torch.nn.Linear) and cell.extra != "init":
                torch.nn.init.xavier_normal_(mod.weight)
    p.layer = layer
    g = torch.Generator().manual_seed(cell.seed + 1)
    dim = cell.kw["dim"]
    e = b * n * k
    p.feats = torch.randn(b * n, dim, generator=g)
    idx = torch.randint(0, n, (b, n, k), generator=g)
    if cell.hub:
        idx[:, :, 0] = 3
        if k >= 2:
            idx[:, ::2, 1] = 7
        idx[idx == 5] = 3                                                        # (wide K: random draws alone would reach every key)
    p.idx = idx
    p.coors = torch.randn(b, n, 3, generator=g) * 1.5
    p.edges = torch.randn(b, n, n, cell.kw["edge_dim"], generator=g) if cell.kw["edge_dim"] else None
    with torch.no_grad():
        p.scal = autograd.edge_scalars(layer, p.coors, p.edges, idx)[1].reshape(e, s).contiguous()      # [fourier, dist, edge feats]
    p.src = torch.arange(b * n).repeat_interleave(k)
    p.dst = (idx + (torch.arange(b) * n)[:, None, None]).reshape(-1)
    gu = torch.randn(e, m, generator=g) * 1e-3
    zero = torch.rand(e, generator=g) < 0.2
    zero |= p.src == 1                                                           # a source key ...
    off_hub = [int(d) for d in p.dst.tolist() if d % n not in (3, 7)]           # (hub with K = 1: every edge arrives at node 3)
    if cell.by_dest and off_hub:
        zero |= p.dst == off_hub[0]                                              # ... and a destination key whose entries all carry gU = 0
    gu[zero] = 0.0
    p.zero_rows = zero
    p.gu16 = torch.zeros(e, 16)
    p.gu16[:, :m] = gu
    if cell.by_dest:
        ds, order = torch.sort(p.dst, stable=True)
        p.ent, p.seg = autograd.entry_list(order, ds, b * n)
    else:
        p.ent, p.seg = autograd.entry_list(torch.arange(e), None, b * n)
    p.rounds = p.ent.numel() // 128
    p.n_slabs = n_slabs_of(p.rounds, cell.r)
    return p


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The five contractions of a cell in float64, from the layer's parameters, the inputs and the scalars -- nothing of the product's
    backward: z = P_i[i] + P_j[j] + W_s s, d = keep / (1 - p) (the hash mask of egnn_pytorch_amd/_dropout.py, rows = eid0 + edge id,
    columns = hidden unit), x = d z, a = SiLU(x), dz = (gU W2) SiLU'(x) d.  Returns a dict: key_rows (B N, H) = d/d P of the pass's key
    (source: d/d P_i, destination: d/d P_j), ws (H, S), scal (E, S), w2 (m, H), and z, sp = SiLU'(x), keep for the preconditions."""
    import torch
    from egnn_pytorch_amd import _dropout
    cell, p = BY_ID[cid], prepare(cid)
    dim, m = cell.kw["dim"], cell.m_dim
    lin0, lin3 = p.layer.edge_mlp[0], p.layer.edge_mlp[3]
    w1, b1, w2 = lin0.weight.detach().double(), lin0.bias.detach().double(), lin3.weight.detach().double()
    h = w1.shape[0]
    e = cell.b * cell.n * cell.k
    fd, sd, gd = p.feats.double(), p.scal.double(), p.gu16[:, :m].double()
    p_i = fd @ w1[:, :dim].t() + b1
    p_j = fd @ w1[:, dim:2 * dim].t()
    z = p_i[p.src] + p_j[p.dst] + sd @ w1[:, 2 * dim:].t()
    d = torch.ones(e, h, dtype=torch.float64)
    keep = torch.ones(e, h, dtype=torch.bool)
    if cell.drop is not None:
        prob, seed = cell.drop
        keep = _dropout.keep_mask(seed, _dropout.SITE_EDGE, cell.eid0 + torch.arange(e), torch.arange(h), prob)
        d = keep.double() * _dropout.inv_keep(prob)
    x = d * z
    sg = torch.sigmoid(x)
    sp = sg * (1 + x * (1 - sg))
    dz = (gd @ w2) * sp * d
    key = p.dst if cell.by_dest else p.src
    return dict(key_rows=torch.zeros(cell.b * cell.n, h, dtype=torch.float64).index_add_(0, key, dz),
                ws=dz.t() @ sd, scal=dz @ w1[:, 2 * dim:], w2=gd.t() @ (x * sg), z=z, sp=sp, keep=keep)


def outputs_of(cell):
    """the outputs the variant produces, by their name in `reference`"""
    return ("key_rows",) + (("w2",) if cell.want_w2 else ()) + (("ws", "scal") if cell.want_s else ())

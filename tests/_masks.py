"""Padding masks that are not prefixes, shared by the gradient tests.

Every other gradient test of the suite builds its mask as `arange(n) < len`: real nodes first, padding behind them.  The backward's
machinery reads the mask geometry in many places -- the spatial order lists padded nodes last, the by-destination entry lists are
built over all edges, a padded node's neighbours are "the first K nodes wherever they are" -- and with a prefix mask those first K
nodes are always real.  `mask_pattern(name, b, n, k, rng)` returns the (b, n) bool masks of the other kinds; each pattern checks,
from the mask alone, that it is what its name says."""
import numpy as np

PATTERNS = ("scattered", "leading_padding", "blocks_of_four", "one_graph_empty", "few_real", "interleaved")
B = 4


def is_prefix(mask):
    """every row is `arange(n) < count`: real nodes first, padding behind them"""
    mask = np.asarray(mask, dtype=bool)
    n = mask.shape[-1]
    return bool((mask == (np.arange(n)[None, :] < mask.sum(axis=-1, keepdims=True))).all())


def _draw(name, b, n, k, rng):
    mask = np.zeros((b, n), dtype=bool)
    if name == "scattered":                                   # Bernoulli(0.6) per node
        mask = rng.random((b, n)) < 0.6
    elif name == "leading_padding":                           # padding in FRONT: a padded node's first K nodes are padded themselves
        for g, p in enumerate((0, 5, n // 2, n - k - 1)):
            mask[g, min(max(p, 0), n - 1):] = True
    elif name == "blocks_of_four":                            # aligned blocks of four positions, each kept with probability 0.5
        keep = rng.random((b, (n + 3) // 4)) < 0.5
        mask = np.repeat(keep, 4, axis=1)[:, :n]
    elif name == "one_graph_empty":                           # a middle graph with no real node at all
        mask = rng.random((b, n)) < 0.7
        mask[1] = False
    elif name == "few_real":                                  # fewer real nodes than neighbours: every selection holds padded nodes
        for g, cnt in enumerate((1, 2, k - 1, k)):
            mask[g, rng.permutation(n)[:min(max(cnt, 1), n)]] = True
    elif name == "interleaved":
        mask[0, 0::2] = True
        mask[1] = True
        mask[2, 1::2] = True
        mask[3, 1:] = True                                    # exactly one padded node, at position 0
    else:
        raise KeyError(name)
    return mask


def mask_pattern(name, b, n, k, rng):
    """(b, n) bool numpy array.  k: the layer's neighbour count (None for a dense layer: taken as 4, so that `few_real` has 1, 2, 3
    and 4 real nodes); rng: a numpy Generator (the random patterns are redrawn until they are no prefix masks)."""
    assert b == B, "the patterns are written for four graphs"
    k = 4 if k is None else k
    assert n >= 2 and k >= 1
    for _ in range(64):
        mask = _draw(name, b, n, k, rng)
        if not is_prefix(mask):
            break
    assert mask.shape == (b, n) and mask.dtype == bool
    assert not is_prefix(mask), name
    assert mask.any(), name
    if name == "one_graph_empty":
        assert not mask[1].any() and mask[0].any() and mask[2].any() and mask[3].any()
    if name == "few_real":
        want = [min(max(c, 1), n) for c in (1, 2, k - 1, k)]
        assert mask.sum(axis=1).tolist() == want and max(want) <= k
    if name == "leading_padding":
        first = mask.argmax(axis=1)
        assert all(mask[g, first[g]:].all() and not mask[g, :first[g]].any() for g in range(b)) and first.max() > 0
    if name == "interleaved":
        assert mask[1].all() and not mask[3, 0] and mask[3, 1:].all() and not (mask[0, :-1] & mask[0, 1:]).any()
    if name == "blocks_of_four":
        full = mask[:, :n - n % 4].reshape(b, -1, 4)
        assert (full.all(axis=2) | ~full.any(axis=2)).all()
    return mask

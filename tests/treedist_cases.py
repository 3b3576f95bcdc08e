"""Tree sets with branch lengths for the tree-distance tests: the tree sets of
tests/treeset_cases.py in the library's three forms, one length per edge carried consistently
into each form's edge order, and the reference's results (tests/treedist_reference.py), computed
once per shape."""
import functools

import numpy as np

import treedist_reference as D
import treeset_cases as C
import treeset_reference as TR


def edge_keys(form, tree):
    """Per edge in the form's order: its split, or ("tip", i) on tip i's pendant edge."""
    edges = TR.form_edges(form, tree)
    n = (len(edges) + 3) // 2
    return [s if s is not None else ("tip", a if a < n else b)
            for (a, b), s in zip(edges, TR.edge_splits(form, tree))]


def random_lengths(rng, shape):
    """Doubles with full mantissas, about one in seven exactly 0."""
    x = rng.random(shape)
    x[rng.random(shape) < 0.15] = 0.0
    return x


def carry(form_from, tree_from, lengths, form_to, tree_to):
    """`lengths` of one tree moved from one encoding's edge order to another's."""
    by_key = dict(zip(edge_keys(form_from, tree_from), lengths))
    return np.array([by_key[k] for k in edge_keys(form_to, tree_to)], dtype=np.float64)


def trees_of(case, form):
    return list(case["edges"]) if form == "edges" else list(zip(*case[form]))


@functools.lru_cache(maxsize=None)
def case(n, T, seed=0):
    """treeset_cases.case(n, T) with len_edges, len_ops, len_joins [T][2n-3] (the same length on
    the same edge in every form) and ref: treedist_reference.distances on the edge lists."""
    base = C.case(n, T, seed)
    rng = np.random.default_rng(977 * n + 13 * T + seed)
    out = dict(base)
    out["len_edges"] = random_lengths(rng, (T, 2 * n - 3))
    e = trees_of(base, "edges")
    for form in ("ops", "joins"):
        other = trees_of(base, form)
        out["len_" + form] = np.stack([carry("edges", e[t], out["len_edges"][t], form, other[t])
                                       for t in range(T)])
    out["ref"] = D.distances("edges", e, out["len_edges"])
    return out


def arg(case, form):
    return case["edges"] if form == "edges" else case[form]


def bits(x):
    """The bit patterns of an array of doubles (or of a nested list of floats)."""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)

"""Generate tests/golden/hp_*.npz: the likelihood path in 50-digit arithmetic
(tests/hp_reference.py) on the cases of tests/hp_cases.py, rounded to the nearest float64, and
next to every quantity the error of the fp64 oracle (oracle/oracle.py) against it, under a key
named ``E_orc_*``.  Those errors are the yardstick of tests/test_gpu_hp.py.

Needs mpmath, numpy, the package's host-side classes and oracle/; no GPU.  Run from anywhere:

    python tests/golden/make_golden_hp.py

takes a few minutes (an LG expm in mpmath takes about half a second) and rewrites
hp_pmat_gtr, hp_pmat_lg, hp_tree8_gtr, hp_tree8_lg and hp_deep.  tests/test_hp_reference.py
regenerates every GTR file and three LG matrices and compares them with the committed files.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import hp_cases as H  # noqa: E402
import hp_reference as R  # noqa: E402


def _txt(s):
    return np.frombuffer(s.encode(), dtype=np.uint8)


def _floats(x):
    return np.array([float(v) for v in x])


# ---------------------------------------------------------------- P matrices
def p_taus(rm):
    """(Traversal, lengths [n_ops + 1][2]) of the P case in pu_get_pmatrices' layout: one row per
    op, then (0, root length)."""
    tr, _ = H.schedule(H.p_newick(), H.P_NAMES)
    return tr, np.vstack([tr.op_lengths(), [[0.0, tr.root_length()]]])


def gen_pmat(orc, name):
    model = H.model_of(name)
    X = R.Exact.of_model(model)
    out = dict(newick=_txt(H.p_newick()), codes=H.p_codes())
    for rmn in H.P_RATE_MODELS:
        rm = H.rate_model_of(rmn)
        tr, lens = p_taus(rm)
        assert set(H.P_LENGTHS) | {0.1} == set(lens.ravel())
        K, C = len(model.freqs), rm.ncat
        T = np.zeros(lens.shape + (C, K, K))
        for o in range(lens.shape[0]):
            for s in range(2):
                T[o, s] = [R.to_float(m) for m in X.p_cats(lens[o, s], rm.rates)]
        out.update({rmn + "_P": T, rmn + "_rates": np.asarray(rm.rates), rmn + "_len": lens})
    out.update(H.oracle_errors_pmat(orc, out, name))
    return out


# ---------------------------------------------------------------- trees
def exact_tree(X, newick, names, codes, table, rm, weights):
    """(Traversal, tips, Exact.partials) of a case on its own rooting."""
    tr, rows = H.schedule(newick, names)
    tips = {n: table[codes[i]].astype(int).tolist() for n, i in rows.items()}
    return tr, tips, X.partials(tips, tr.postorder_traversal, tr.op_lengths(), rm.rates)


def exact_root(X, tr, tips, part, rm, weights, t=None):
    return X.edge(tips, tr.postorder_traversal, tr.op_lengths(), tr.root_edge, tr.root_length(),
                  tr.root_edge, tr.root_length() if t is None else t, rm.rates, rm.weights,
                  weights, rerooted=True, part=part)


def site_block(X, key, newick, names, codes, table, rm, weights):
    """The truth of the per-pattern and total lnL of one tree case."""
    tr, tips, part = exact_tree(X, newick, names, codes, table, rm, weights)
    ex = exact_root(X, tr, tips, part, rm, weights)
    site = _floats(ex["site"])
    zero = np.isneginf(site)
    out = {key + "_site": site, key + "_f": R.to_float(ex["f"]), key + "_zero": zero}
    if not zero[weights != 0].any():
        out[key + "_lnl"] = np.float64(float(ex["lnl"]))
    return out


def gen_tree8(orc, name):
    model = H.model_of(name)
    X = R.Exact.of_model(model)
    table, _, _ = H.table_of(name)
    codes, w = H.t8_tips(name)
    out = dict(codes=codes, weights=w, table=table)
    for r in H.T8_ROOTINGS:
        out["newick_" + r] = _txt(H.t8_newick(r))
    out["newick_z"] = _txt(H.t8_newick("r5", 0.0))
    for rmn in H.TREE_RATE_MODELS:
        rm = H.rate_model_of(rmn)
        out[rmn + "_rates"], out[rmn + "_catw"] = np.asarray(rm.rates), np.asarray(rm.weights)
        out.update(site_block(X, rmn, H.t8_newick("r5"), H.T8_NAMES, codes, table, rm, w))
        out.update(site_block(X, rmn + "_z", H.t8_newick("r5", 0.0), H.T8_NAMES, codes, table,
                              rm, w))
        for r in H.EDGE_ROOTINGS:
            nwk = H.t8_newick(r)
            tr, tips, part = exact_tree(X, nwk, H.T8_NAMES, codes, table, rm, w)
            ts = sorted(set(H.EDGE_T) | {tr.root_length()})
            truth = []
            for t in ts:
                ex = exact_root(X, tr, tips, part, rm, w, t)
                truth.append([float(ex["lnl"]), float(ex["d1"]), float(ex["d2"])])
            out["%s_edge_%s_t" % (rmn, r)] = np.array(ts)
            out["%s_edge_%s" % (rmn, r)] = np.array(truth)
    out.update(H.oracle_errors_tree8(orc, out, name))
    return out


def gen_deep(orc):
    model, rm = H.model_of("gtr"), H.rate_model_of("g05")
    X = R.Exact.of_model(model)
    table, _, _ = H.table_of("gtr")
    codes, w = H.deep_tips()
    out = dict(codes=codes, weights=w, table=table, newick=_txt(H.deep_newick()),
               rates=np.asarray(rm.rates), catw=np.asarray(rm.weights))
    out.update(site_block(X, "g05", H.deep_newick(), H.DEEP_NAMES, codes, table, rm, w))
    out.update(H.oracle_errors_deep(orc, out))
    return out


FILES = {"hp_pmat_gtr": lambda orc: gen_pmat(orc, "gtr"),
         "hp_pmat_lg": lambda orc: gen_pmat(orc, "lg"),
         "hp_tree8_gtr": lambda orc: gen_tree8(orc, "gtr"),
         "hp_tree8_lg": lambda orc: gen_tree8(orc, "lg"),
         "hp_deep": gen_deep}


def main():
    from oracle import oracle as orc
    orc.build()
    for name in sys.argv[1:] or sorted(FILES):
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **FILES[name](orc))
        print("wrote", name)


if __name__ == "__main__":
    main()

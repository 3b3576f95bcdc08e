"""Neighbour joining and BIONJ on the device (pu_nj.hip) against the numpy
restatement of the rule (tests/nj_reference.py): the join sequence, root edge, criterion and
lengths over the sizes at which the kernels change path, exact ties, the two tiers and repeated
calls bit for bit, the device pipeline distances -> matrix -> joins, and the way from a simulated
alignment to an optimised tree through TreeModel and the CLI."""
import functools

import numpy as np
import pytest

import nj_reference as NR
from phylo_utils_amd import TreeModel, distance, nj, phy, simulation
from phylo_utils_amd import alignment as A
from phylo_utils_amd import substitution_models as SM
from phylo_utils_amd.rate_models import GammaRateModel
from phylo_utils_amd.synthetic import CFG2_FREQS, CFG2_GTR_RATES
from phylo_utils_amd.tree import parse_newick

pytestmark = pytest.mark.gpu

METHODS = ("nj", "bionj")
A_MAX = {m: nj.max_lds_n(m) for m in METHODS}  # tier A's largest n
# 3: no join before the last step; 64 / 65: a list row of one wave and of one lane more; tier
# A's largest n of either method and one more (the tier edge)
SHAPES = sorted({3, 4, 5, 8, 64, 65} | {A_MAX[m] + k for m in METHODS for k in (0, 1)})
KINDS = {"random": NR.random_matrix, "additive": NR.perturbed_additive}
MIN_GAP = 1e-9


@functools.lru_cache(maxsize=None)
def matrix(kind, n):
    """The fixture of a kind and size; its seed is 7 n (additive) or 7 n + 1 (random): checked on
    the CPU to keep the restatement's best and second-best Q at least MIN_GAP apart, relative,
    at every join of both methods.  (With four clusters left a pair and its complement have the
    same Q identically, so no seed can part them; there the gap is taken to the best pair
    outside those two, nj_reference.nj.  The join sequence is compared in full all the same.)"""
    D = KINDS[kind](7 * n + sorted(KINDS).index(kind), n)
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def reference(kind, n, method):
    return NR.nj(matrix(kind, n), method)


def bound(D):
    """8 n^2 2^-52 max D: every sum update of the run rounding the other way."""
    return 8.0 * len(D) ** 2 * 2.0 ** -52 * D.max()


def check(got, ref, D, what):
    joins, lens, root, root_len, q = got
    assert np.array_equal(joins, ref["joins"]), what
    assert np.array_equal(root, ref["root"]), what
    dev = max(float(np.abs(lens - ref["lens"]).max()), abs(root_len - ref["root_len"]),
              float(np.abs(q - ref["q"]).max()) if len(q) else 0.0)
    print("%s: largest deviation %.3g (bound %.3g)" % (what, dev, bound(D)))
    assert dev <= bound(D), what
    return dev


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", SHAPES)
def test_against_the_restatement(n, method):
    for kind in sorted(KINDS):
        D, ref = matrix(kind, n), reference(kind, n, method)
        if n > 3:
            assert ref["gap"].min() >= MIN_GAP, (kind, n, method, ref["gap"].min())
        check(nj.nj_joins(D, method), ref, D, "%s n=%d %s" % (kind, n, method))


@pytest.mark.parametrize("method", METHODS)
def test_matrix_in_memory_at_300(method):
    n = 300
    assert n > max(A_MAX.values())
    for kind in sorted(KINDS):
        D, ref = matrix(kind, n), reference(kind, n, method)
        assert ref["gap"].min() >= MIN_GAP, (kind, method, ref["gap"].min())
        check(nj.nj_joins(D, method), ref, D, "%s n=300 %s" % (kind, method))


@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("method", METHODS)
def test_batch_of_seven(method, tier, monkeypatch):
    n = 20
    kinds = ["random", "additive"] * 3 + ["random"]
    Ds = [KINDS[k](900 + i, n) for i, k in enumerate(kinds)]
    refs = [NR.nj(D, method) for D in Ds]
    assert min(r["gap"].min() for r in refs) >= MIN_GAP
    monkeypatch.setenv("PU_NJ_TIER", tier)
    joins, lens, root, root_len, q = nj.nj_joins(np.stack(Ds), method)
    assert joins.shape == (7, n - 2, 2) and q.shape == (7, n - 3) and root_len.shape == (7,)
    for b in range(7):
        check((joins[b], lens[b], root[b], root_len[b], q[b]), refs[b], Ds[b],
              "batch %d %s tier %s" % (b, method, tier))
    # a matrix of the batch alone: the same bits
    one = nj.nj_joins(Ds[4], method)
    for x, y in zip(one, (joins[4], lens[4], root[4], root_len[4], q[4])):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("tier", ["A", "B"])
@pytest.mark.parametrize("method", METHODS)
def test_exact_ties_go_to_the_smallest_ids(method, tier, monkeypatch):
    E = np.ones((6, 6)) - np.eye(6)
    ref = NR.nj(E, method)
    assert np.all(ref["gap"] == 0.0)
    monkeypatch.setenv("PU_NJ_TIER", tier)
    joins, lens, root, root_len, q = nj.nj_joins(E, method)
    assert joins.tolist() == ref["joins"].tolist() == [[0, 1], [2, 3], [4, 5], [6, 7]]
    assert root.tolist() == [9, 8]
    assert np.array_equal(lens, ref["lens"]) and root_len == ref["root_len"]
    assert np.array_equal(q, ref["q"])


@pytest.mark.parametrize("method", METHODS)
def test_tiers_and_repeats_are_bitwise_equal(method, monkeypatch):
    for n in (20, A_MAX[method]):
        for kind in sorted(KINDS):
            D = matrix(kind, n)
            out = {}
            for tier in ("A", "B", "A", "B"):
                monkeypatch.setenv("PU_NJ_TIER", tier)
                got = nj.nj_joins(D, method)
                for x, y in zip(got, out.setdefault("first", got)):
                    assert np.array_equal(x, y), (n, kind, tier)
            monkeypatch.delenv("PU_NJ_TIER")
            for x, y in zip(nj.nj_joins(D, method), out["first"]):
                assert np.array_equal(x, y)


def test_tier_b_batches_on_two_streams(monkeypatch):
    """Tier B keeps its working copies in per-device buffers: two batches queued on two streams
    with nothing between them give the bits each gives on one stream."""
    import torch
    monkeypatch.setenv("PU_NJ_TIER", "B")
    n, B = 5, 2
    dev = torch.device("cuda", 0)
    batches = [np.stack([NR.random_matrix(50 + 2 * b + i, n) for i in range(B)]) for b in range(2)]
    d_Ds = [torch.from_numpy(x).to(dev) for x in batches]

    def outputs():
        return [torch.zeros(shape, dtype=dt, device=dev)
                for shape, dt in (((B, n - 2, 2), torch.int32), ((B, n - 2, 2), torch.float64),
                                  ((B, 2), torch.int32), ((B,), torch.float64),
                                  ((B, n - 3), torch.float64))]

    def queue(stream, d_D, out, method):
        nj.nj_device(stream.cuda_stream, d_D.data_ptr(), n, n, *[o.data_ptr() for o in out],
                     method=method, n_mat=B)

    for method in METHODS:
        want = []
        for d_D in d_Ds:  # one stream, one batch at a time
            out = outputs()
            queue(torch.cuda.current_stream(dev), d_D, out, method)
            torch.cuda.synchronize(dev)
            want.append([o.cpu().numpy() for o in out])
        streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        outs = [outputs(), outputs()]
        torch.cuda.synchronize(dev)  # the outputs are zeroed; from here on nothing waits
        for st, d_D, out in zip(streams, d_Ds, outs):
            queue(st, d_D, out, method)
        for st in streams:
            st.synchronize()
        for out, ref in zip(outs, want):
            for x, y in zip(out, ref):
                assert np.array_equal(x.cpu().numpy(), y), method


# ---------------------------------------------------------------------------- device path
def gtr():
    return SM.GTR(CFG2_GTR_RATES, CFG2_FREQS)


@functools.lru_cache(maxsize=None)
def state_rows(n_taxa=12, S=700):
    rng = np.random.default_rng(12)
    rows = [rng.integers(0, 4, S)]
    for k in range(n_taxa - 1):
        rows.append(np.where(rng.random(S) < 0.08 + 0.02 * k, rng.integers(0, 4, S), rows[-1]))
    return np.stack(rows).astype(np.uint8)


@pytest.mark.parametrize("method", METHODS)
def test_distances_matrix_joins_on_one_stream(method):
    """pu_pair_distances_device -> pu_pair_matrix_device -> pu_nj_device: the distances never
    leave the device; the same bits as the host calls on the same codes."""
    import torch
    codes, table = state_rows(), np.eye(4)  # rows of states: code k is state k
    n, S = codes.shape
    model, rm = gtr(), GammaRateModel(4, 0.5)
    out5 = distance.evaluate_codes(codes, table, model, rm)
    D, _ = distance.matrices(out5, None, n)
    host = nj.nj_joins(D, method)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ld = n + 3
    d_codes = torch.from_numpy(codes).to(dev)
    d_out5 = torch.empty((n * (n - 1) // 2, 5), dtype=torch.float64, device=dev)
    d_D = torch.full((n, ld), -1.0, dtype=torch.float64, device=dev)
    d_joins = torch.zeros((n - 2, 2), dtype=torch.int32, device=dev)
    d_lens = torch.zeros((n - 2, 2), dtype=torch.float64, device=dev)
    d_root = torch.zeros(2, dtype=torch.int32, device=dev)
    d_rl = torch.zeros(1, dtype=torch.float64, device=dev)
    d_q = torch.zeros(n - 3, dtype=torch.float64, device=dev)
    distance.distances_device(stream, d_codes.data_ptr(), S, n, S, table, model, rm,
                              d_out5=d_out5.data_ptr())
    nj.pair_matrix_device(stream, n, d_out5.data_ptr(), d_D.data_ptr(), ld)
    nj.nj_device(stream, d_D.data_ptr(), ld, n, d_joins.data_ptr(), d_lens.data_ptr(),
                 d_root.data_ptr(), d_rl.data_ptr(), d_q.data_ptr(), method=method)
    torch.cuda.synchronize(dev)
    got_D = d_D.cpu().numpy()
    assert np.array_equal(got_D[:, :n], D) and np.all(got_D[:, n:] == -1.0)
    got = (d_joins.cpu().numpy(), d_lens.cpu().numpy(), d_root.cpu().numpy(), float(d_rl.cpu()[0]),
           d_q.cpu().numpy())
    for x, y in zip(got, host):
        assert np.array_equal(x, y)
    # a pair list in another order, (j, i) too: the listed entries and nothing else
    pairs = distance.all_pairs(n)[::-1, ::-1].copy()
    d_E = torch.full((n, ld), -1.0, dtype=torch.float64, device=dev)
    d_rev = torch.from_numpy(np.ascontiguousarray(out5[::-1])).to(dev)
    nj.pair_matrix_device(stream, n, d_rev.data_ptr(), d_E.data_ptr(), ld, pairs=pairs[:-1])
    torch.cuda.synchronize(dev)
    want = np.full((n, ld), -1.0)
    want[:, :n] = D
    want[np.arange(n), np.arange(n)] = -1.0
    want[0, 1] = want[1, 0] = -1.0  # the pair left out
    assert np.array_equal(d_E.cpu().numpy(), want)
    # without q
    nj.nj_device(stream, d_D.data_ptr(), ld, n, d_joins.data_ptr(), d_lens.data_ptr(),
                 d_root.data_ptr(), d_rl.data_ptr(), None, method=method)
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_joins.cpu().numpy(), host[0])


# ---------------------------------------------------------------------------- end to end
# internal branches of at least 0.05
NEWICK8 = ("(((a:0.1,b:0.15):0.05,(c:0.2,d:0.1):0.07):0.06,"
           "((e:0.12,f:0.3):0.05,(g:0.08,h:0.2):0.09):0.05);")
SIM_SEED = 8  # checked on the CPU (tests/sim_reference.py, tests/dist_reference.py, the
#               restatement): RF = 0 to NEWICK8 for both methods


@functools.lru_cache(maxsize=None)
def simulated():
    """(names, states [8][20000]) of TreeModel.simulate down NEWICK8 under GTR + G4."""
    model, rm = gtr(), GammaRateModel(4, 0.5)
    tm = TreeModel(keep_partials=False)
    tm.set_tree(NEWICK8)
    names = list(tm.traversal.names)
    tm.set_alignment_codes(np.zeros((8, 1), dtype=np.uint8), np.ones((1, 4)), names)
    tm.set_substitution_model(model)
    tm.set_rate_model(rm)
    tm.initialise()
    return names, tm.simulate(20000, seed=SIM_SEED)


@pytest.mark.parametrize("method", METHODS)
def test_alignment_to_optimised_tree(method):
    names, states = simulated()
    assert states.shape == (8, 20000)
    model, rm = gtr(), GammaRateModel(4, 0.5)
    tm = TreeModel()
    tm.set_alignment_codes(states, np.eye(4), names)
    tm.set_substitution_model(model)
    tm.set_rate_model(rm)
    tree = tm.set_nj_tree(method=method)
    n2, D, _ = tm.pairwise_distances()
    assert n2 == names
    ref = NR.nj(D, method)
    ref_tree = nj.joins_to_tree(names, ref["joins"], ref["lens"], ref["root"], ref["root_len"],
                                1e-8)
    true = parse_newick(NEWICK8)
    assert NR.robinson_foulds(tree, ref_tree) == 0
    assert NR.robinson_foulds(tree, true) == 0 and NR.robinson_foulds(ref_tree, true) == 0
    got_l, ref_l = NR.split_lengths(tree), NR.split_lengths(ref_tree)
    assert max(abs(got_l[s] - ref_l[s]) for s in ref_l) <= bound(D)
    tm.initialise()
    lnl_nj = tm.likelihood()
    lnl = tm.optimise_branch_lengths(sweeps=2)
    print("%s: lnL at the NJ lengths %.6f, optimised %.6f" % (method, lnl_nj, lnl))
    assert np.isfinite(lnl_nj) and np.isfinite(lnl)
    assert lnl >= lnl_nj


def test_cli_nj_end_to_end(tmp_path, capsys):
    names, states = simulated()
    fa = tmp_path / "aln.fasta"
    seqs = simulation.states_to_sequences(states[:, :2000], A.DNA)
    fa.write_text("".join(">%s\n%s\n" % r for r in zip(names, seqs)))
    out = tmp_path / "tree.nwk"
    assert phy.main(["-s", str(fa), "-m", "HKY{2.0}+G4{0.7}", "--nj", "bionj", "-o", str(out),
                     "--optimise", "1"]) == 0
    printed = capsys.readouterr().out
    assert printed.startswith("lnL = ") and np.isfinite(float(printed.split("=")[1]))
    tree = parse_newick(out.read_text())
    assert sorted(x.label for x in tree.leaf_nodes()) == sorted(names)
    assert len(tree.seed_node.children) == 2

"""TreeModel on the GPU -- mirror of ``phylo_utils/tree_model.py`` (TreeModel :12-217).

Same methods and call order as the reference (``set_alignment``,
``set_substitution_model``, ``set_rate_model``, ``set_tree``, ``initialise``,
``compute_partials``, ``compute_partials_at_edge``, ``compute_likelihood_at_edge``),
but everything between "tips uploaded" and "sitewise lnL" happens in HBM in one
``pu_run`` (P matrices, the whole post-order, the root combine, ``lnl_node``,
the logsumexp over categories and the pattern-weighted sum).  ``partials``,
``scale``, ``root_partials`` and ``root_scale`` are fetched lazily from the device
with the reference's shapes ([node][site][category][state] etc.).
"""
from __future__ import annotations

import ctypes
import os
import logging

import numpy as np

from . import _native as N
from . import optimisation
from .alignment import alignment_to_codes, invariant_sites, partials_to_codes
from .tree import Traversal, prepare_tree

logger = logging.getLogger(__name__)


class _LazyPartials(object):
    """[ntaxa][S][K] view of coded tips, materialised per row on demand."""

    def __init__(self, codes, table):
        self.codes, self.table = codes, table
        self.shape = codes.shape + (table.shape[1],)

    def __getitem__(self, i):
        return self.table[self.codes[i]]

    def __array__(self, dtype=None, copy=None):
        a = self.table[self.codes]
        return a if dtype is None else a.astype(dtype)

    def __mul__(self, other):
        return np.asarray(self) * other


class TreeModel(object):
    alignment = None
    ascbias = False

    def __init__(self, device=0, keep_partials=True, compact_tips=True, reorder=True):
        self.device = device
        self.keep_partials = keep_partials
        self.compact_tips = compact_tips
        self.reorder = reorder
        self._ctx = None
        self._slot_names = None
        self._dirty = True
        self._lnl = None
        self._site_valid = False
        self._tips_owner = None

    # ------------------------------------------------------------------ inputs
    def set_alignment(self, alignment, alphabet, compress=True):
        """tree_model.py:42-50 (Biopython-free: [(name, seq)], dict or .name/.seq records).
        Tips are kept as codes (alignment_to_codes); the pattern compression runs on this
        model's device with np.unique's exact result (pu_compress_patterns).  The
        `alignment` attribute reads as the reference's [ntaxa][S][K] partials."""
        codes, table, sw, ii, names = alignment_to_codes(alignment, alphabet, compress,
                                                          self.device)
        if self.compact_tips:
            self._codes = (codes, table)
            self.alignment = _LazyPartials(codes, table)
        else:  # dense fp64 tips (pu_set_tip_partials)
            self._codes = None
            self.alignment = np.ascontiguousarray(table[codes])
        self.inverse_index = ii
        self.siteweights = sw
        self.names = names
        self._alphabet = alphabet  # place() encodes query sequences with the same table
        self._tips_owner = None
        self._free()

    def set_alignment_partials(self, partials, names, siteweights=None, inverse_index=None):
        """Tip partials given directly ([ntaxa][S][K]), e.g. for synthetic data."""
        self._codes = None
        self.alignment = np.ascontiguousarray(partials, dtype=np.float64)
        S = self.alignment.shape[1]
        self.siteweights = np.ones(S) if siteweights is None else np.asarray(siteweights)
        self.inverse_index = np.arange(S) if inverse_index is None else np.asarray(inverse_index)
        self.names = dict(names) if isinstance(names, dict) else {n: i for i, n in enumerate(names)}
        self._alphabet = None  # no character table: place() then needs coded queries
        self._tips_owner = None
        self._free()

    def set_alignment_codes(self, codes, table, names, siteweights=None):
        """Compact tips directly: codes uint8 [ntaxa][S] into table [n_codes][K] (the engine's
        native tip format; avoids materialising [ntaxa][S][K] partials for large inputs)."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        table = np.ascontiguousarray(table, dtype=np.float64)
        self._codes = (codes, table)
        self.alignment = _LazyPartials(codes, table)
        S = codes.shape[1]
        self.siteweights = np.ones(S) if siteweights is None else np.asarray(siteweights)
        self.inverse_index = np.arange(S)
        self.names = {n: i for i, n in enumerate(names)}
        self._alphabet = None
        self._tips_owner = None
        self._free()

    def share_alignment(self, owner):
        """Read `owner`'s resident alignment instead of uploading a copy (r06, SURVEY 8(e) G2:
        one alignment per GPU for many trees; the reference swaps trees on one alignment,
        tree_model.py:42-50, 87-89).  `owner` is a TreeModel on the same device whose
        alignment is coded (compact tips); this model's context borrows owner's tip codes,
        code table and pattern weights (pu_share_tips), which then stay frozen in both.  The
        storage lives as long as any model holding it."""
        if not isinstance(owner, TreeModel) or owner is self:
            raise ValueError("share_alignment needs another TreeModel")
        if owner.device != self.device:
            raise ValueError("share_alignment: models on devices %d and %d"
                             % (owner.device, self.device))
        owner._ensure()  # the owner's context holds the tips
        self._codes = getattr(owner, "_codes", None)
        self.alignment = owner.alignment
        self.siteweights = owner.siteweights
        self.inverse_index = owner.inverse_index
        self.names = owner.names
        self._alphabet = getattr(owner, "_alphabet", None)
        self.compact_tips = owner.compact_tips
        self._free()
        self._tips_owner = owner

    def get_empirical_freqs(self, pseudocount=None, include_ambiguous=False):
        """tree_model.py:52-73."""
        if self.alignment is None:
            logger.error("No alignment has been set")
            return 0
        counts = (self.alignment * self.siteweights[np.newaxis, :, np.newaxis]).sum((0, 1))
        if pseudocount is not None:
            try:
                counts = counts + np.array(pseudocount)
            except (TypeError, ValueError):
                logger.warning("Pseudocount %s ignored", pseudocount)
        return counts / counts.sum()

    def set_substitution_model(self, model):
        self.substitution_model = model
        self._dirty = True
        if self._ctx is not None:
            self._upload_model()

    def set_rate_model(self, rate_model):
        if self._ctx is not None and getattr(self, "rate_model", None) is not None \
                and rate_model.ncat != self.rate_model.ncat:
            self._free()
        self.rate_model = rate_model
        self._dirty = True
        if self._ctx is not None:
            self._upload_model()

    def set_tree(self, tree):
        """tree_model.py:87-89; `tree` is a newick string or a phylo_utils_amd.tree.Tree.
        A device context built for the same taxa is kept: the next initialise() only
        re-binds the tips to the new node numbering (pu_set_tip_nodes) and plans the new
        schedule -- no tip data are uploaded again (many trees on one alignment)."""
        self.tree = prepare_tree(tree)
        self.traversal = Traversal(self.tree)
        self._dirty = True

    def set_ascertainment_bias_correction(self, weighted=False):
        """Lewis ascertainment-bias correction (tree_model.py:92-98): K dummy invariant
        sites are appended (:151-156) and lnL_s -= log(1 - P(invariant)) (:209-214).

        weighted=False reproduces the reference exactly: P(invariant) sums the dummy
        sites' lnl_node values over categories WITHOUT the category weights (:213), which
        exceeds 1 -- and gives NaN -- for Gamma rates with C > 1.
        weighted=True uses the weighted mixture sum_c w_c (the Lewis correction)."""
        if np.any(invariant_sites(np.asarray(self.alignment))):
            logger.warning("Using Lewis ascertainment bias correction on an alignment with "
                           "invariant sites!")
        self.ascbias = True
        self._asc_mode = 2 if weighted else 1
        self._free()  # the context is rebuilt with the K dummy patterns

    # ------------------------------------------------------------------ device context
    def _free(self):
        if self._ctx is not None:
            N.lib().pu_ctx_destroy(self._ctx)
            self._ctx = None
        self._slot_names = None  # taxon of each tip slot of the context
        self._dirty = True

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass

    def _upload_model(self):
        fr = N.f64(self.substitution_model.freqs)
        rates = N.f64(self.rate_model.rates)
        w = N.f64(self.rate_model.weights)
        if len(rates) != self.rate_model.ncat:
            raise ValueError("rate model has %d rates for ncat=%d" % (len(rates),
                                                                       self.rate_model.ncat))
        if self._host_p():
            # non-reversible: no eigen-decomposition; P = expm(Q r t) comes from the host
            # before every traversal (_upload_pmatrices)
            N.check(N.lib().pu_set_model_p(self._ctx, N.ptr(fr), N.ptr(rates), N.ptr(w)),
                    self._ctx, "pu_set_model_p")
            # the edge operations and optimisers choose lengths inside the library: they ask
            # the host for P, dP/dt, d2P/dt2 through this provider
            self._pm_provider = N.PMAT_PROVIDER(self._provide_pmatrices)
            N.check(N.lib().pu_set_pmatrix_provider(self._ctx, self._pm_provider, None),
                    self._ctx, "pu_set_pmatrix_provider")
        else:
            ev, el, iv = self.substitution_model.engine_eigen()
            N.check(N.lib().pu_set_model(self._ctx, N.ptr(ev), N.ptr(el), N.ptr(iv), N.ptr(fr),
                                         N.ptr(rates), N.ptr(w)), self._ctx, "pu_set_model")
        self._dirty = True

    def _provide_pmatrices(self, _user, order, n, t_ptr, out_ptr):
        """pu_pmat_provider: out[i] = d^order/dt^order P(t[i] r) of the current models
        (Model.p_derivative; order 0 is Model.p, as _upload_pmatrices).  Returns 0, or 1 after
        an exception (the library then reports the failure)."""
        try:
            rates = np.asarray(self.rate_model.rates, dtype=np.float64)
            K = len(self.substitution_model.freqs)
            t = np.ctypeslib.as_array(t_ptr, shape=(n,))
            out = np.ctypeslib.as_array(out_ptr, shape=(n, len(rates), K, K))
            for i in range(n):
                out[i] = self.substitution_model.p_derivative(float(t[i]), rates, order)
            return 0
        except Exception:  # noqa: BLE001 -- must not unwind through the C frames
            return 1

    def _host_p(self):
        return not getattr(self.substitution_model, "reversible", True)

    def _upload_pmatrices(self):
        """The transition matrices of the current lengths, computed exactly as the reference
        does per op (Model.p: tree_model.py:166-169 and :189-190 for the root edge; for the
        non-reversible models expm(Q r t), abstract.py:172-177), in the caller's op order
        and child order (pu_set_pmatrices)."""
        tr = self.traversal
        rates = self.rate_model.rates
        p = self.substitution_model.p
        bl = tr.op_lengths()
        P = [np.stack([p(l1, rates), p(l2, rates)]) for l1, l2 in bl]
        P.append(np.stack([p(0, rates), p(tr.root_length(), rates)]))
        P = N.f64(np.stack(P))
        N.check(N.lib().pu_set_pmatrices(self._ctx, N.ptr(P)), self._ctx, "pu_set_pmatrices")

    def initialise(self):
        """Allocate HBM buffers, upload tips/model/schedule, run compute_partials
        (tree_model.py:101-158)."""
        if self.alignment is None or not hasattr(self, "traversal"):
            raise ValueError("set_alignment and set_tree before initialise")
        n_leaves, S, K = self.alignment.shape
        C = self.rate_model.ncat
        tr = self.traversal
        Sx = S + K if self.ascbias else S  # + K dummy invariant sites (tree_model.py:113-114)
        if set(tr.names) != set(self.names):
            missing = sorted(set(tr.names) ^ set(self.names))[:5]
            raise ValueError("tree and alignment taxa differ, e.g. %s" % missing)
        ops = np.ascontiguousarray(tr.postorder_traversal, dtype=np.int32)
        bl = N.f64(tr.op_lengths())
        a, b = tr.root_edge
        if self._ctx is not None and self._slot_names is not None and \
                self._ctx_shape == (tr.n_nodes, n_leaves, Sx, C, K):
            # same taxa and sizes, new topology: re-bind the resident tips, plan the tree
            nodes = np.array([tr.names[n] for n in self._slot_names], dtype=np.int32)
            N.check(N.lib().pu_set_tip_nodes(self._ctx, len(nodes), N.ptr(nodes)), self._ctx,
                    "pu_set_tip_nodes")
            N.check(N.lib().pu_set_schedule(self._ctx, len(ops), N.ptr(ops), N.ptr(bl), a, b,
                                            tr.root_length()), self._ctx, "pu_set_schedule")
            self.compute_partials()
            return
        owner = self._tips_owner
        if owner is not None:
            owner._ensure()  # (re)built with its tips if it was freed meanwhile
            osh = owner._ctx_shape if owner._ctx is not None else None
            # tips, table and weights depend on the taxa, patterns and states, not on C
            if osh is None or (osh[1], osh[2], osh[4]) != (n_leaves, Sx, K) or \
                    owner.ascbias != self.ascbias:
                raise ValueError("share_alignment: the owner's context (%s) does not hold this "
                                 "model's alignment" % (osh,))
        self._free()
        flags = (N.PU_KEEP_PARTIALS if self.keep_partials else N.PU_LNL_ONLY) | \
            (0 if self.reorder else N.PU_NO_REORDER)
        ctx = ctypes.c_void_p()
        N.check(N.lib().pu_ctx_create(ctypes.byref(ctx), self.device, tr.n_nodes, n_leaves, Sx,
                                      C, K, flags), None, "pu_ctx_create")
        self._ctx = ctx
        if owner is not None:
            nodes = np.array([tr.names[n] for n in owner._slot_names], dtype=np.int32)
            N.check(N.lib().pu_share_tips(ctx, owner._ctx, len(nodes), N.ptr(nodes)), ctx,
                    "pu_share_tips")
            self._slot_names = list(owner._slot_names)
            self._ctx_shape = (tr.n_nodes, n_leaves, Sx, C, K)
            if self.ascbias:
                N.check(N.lib().pu_set_ascertainment(ctx, self._asc_mode, S), ctx,
                        "pu_set_ascertainment")
            self._upload_model()
            N.check(N.lib().pu_set_schedule(ctx, len(ops), N.ptr(ops), N.ptr(bl), a, b,
                                            tr.root_length()), ctx, "pu_set_schedule")
            self.compute_partials()
            return
        enc = getattr(self, "_codes", None) if isinstance(self.alignment, _LazyPartials) \
            else None
        if enc is None and self.compact_tips:
            enc = partials_to_codes(np.asarray(self.alignment))
        eye = np.eye(K)
        if enc is not None and self.ascbias:
            # dummy site k: every tip is the one-hot vector of state k (tree_model.py:151-156)
            codes, table = enc
            ids = []
            for k in range(K):
                hit = np.nonzero((table == eye[k]).all(axis=1))[0]
                if len(hit):
                    ids.append(int(hit[0]))
                else:
                    table = np.vstack([table, eye[k]])
                    ids.append(len(table) - 1)
            enc = None if len(table) > 256 else (
                np.ascontiguousarray(np.hstack([codes, np.tile(np.array(ids, dtype=np.uint8),
                                                               (len(codes), 1))])),
                np.ascontiguousarray(table))
        if enc is not None:
            codes, table = enc
            N.check(N.lib().pu_set_code_table(ctx, len(table), N.ptr(table)), ctx,
                    "pu_set_code_table")
        for name, node in tr.names.items():
            row = self.names[name]
            if enc is not None:
                cd = np.ascontiguousarray(enc[0][row])
                N.check(N.lib().pu_set_tip_codes(ctx, node, N.ptr(cd)), ctx, "pu_set_tip_codes")
            else:
                tp = np.asarray(self.alignment[row])
                if self.ascbias:
                    tp = np.vstack([tp, eye])
                tp = np.ascontiguousarray(tp, dtype=np.float64)
                N.check(N.lib().pu_set_tip_partials(ctx, node, N.ptr(tp)), ctx,
                        "pu_set_tip_partials")
        self._slot_names = list(tr.names)  # tip slot i holds this taxon
        self._ctx_shape = (tr.n_nodes, n_leaves, Sx, C, K)
        w = N.f64(np.concatenate([self.siteweights, np.zeros(Sx - S)]))
        N.check(N.lib().pu_set_pattern_weights(ctx, N.ptr(w)), ctx, "pu_set_pattern_weights")
        if self.ascbias:
            N.check(N.lib().pu_set_ascertainment(ctx, self._asc_mode, S), ctx,
                    "pu_set_ascertainment")
        self._upload_model()
        N.check(N.lib().pu_set_schedule(ctx, len(ops), N.ptr(ops), N.ptr(bl), a, b,
                                        tr.root_length()), ctx, "pu_set_schedule")
        self.compute_partials()

    def update_branch_lengths(self):
        """Re-read branch lengths from self.traversal.brlens (same topology)."""
        bl = N.f64(self.traversal.op_lengths())
        N.check(N.lib().pu_set_branch_lengths(self._ctx, N.ptr(bl),
                                              self.traversal.root_length()), self._ctx,
                "pu_set_branch_lengths")
        self._dirty = True

    def compute_partials(self):
        """One post-order traversal (tree_model.py:160-176) -- fused with the root combine
        and lnL reduction in a single device pass."""
        if self._ctx is None:
            raise ValueError("initialise first")
        if self._host_p():
            self._upload_pmatrices()
        lnl = ctypes.c_double()
        N.check(N.lib().pu_run(self._ctx, ctypes.byref(lnl), None), self._ctx, "pu_run")
        self._lnl = lnl.value
        self._dirty = False
        self._site_valid = True

    def _ensure(self):
        if self._ctx is None:
            self.initialise()
        elif self._dirty:
            self.compute_partials()

    def _check_edge(self, node_a, node_b):
        try:
            self.traversal.brlens[node_a, node_b]
        except KeyError:
            raise ValueError("There is no edge connecting nodes {} and {}".format(node_a, node_b))

    def _is_root_edge(self, node_a, node_b):
        return (node_a, node_b) == tuple(self.traversal.root_edge)

    def _edge_lnl(self, node_a, node_b):
        """Root on edge (a, b) over the nodes' current partials (pu_edge_lnl)."""
        self._check_edge(node_a, node_b)
        self._ensure()
        if not self.keep_partials:
            raise ValueError("compute_likelihood_at_edge off the root edge needs "
                             "keep_partials=True (PU_LNL_ONLY reuses CLV storage)")
        site = np.empty(self._n_patterns())
        lnl = ctypes.c_double()
        N.check(N.lib().pu_edge_lnl(self._ctx, int(node_a), int(node_b), ctypes.byref(lnl),
                                    N.ptr(site)), self._ctx, "pu_edge_lnl")
        self._site_valid = False  # the device sitewise/root buffers now hold this edge
        return lnl.value, site

    def compute_partials_at_edge(self, node_a, node_b):
        """Root combine on edge (a, b) (tree_model.py:178-198) -> (root_partials, root_scale).
        As in the reference, any edge is accepted and the nodes' current partials are used
        ("only valid if the CLVs at a and b are valid", :181-182)."""
        if self._is_root_edge(node_a, node_b):
            self._check_edge(node_a, node_b)
            self._ensure()
            if not self._site_valid:
                self.compute_partials()
        else:
            self._edge_lnl(node_a, node_b)
        return self._root()

    def compute_likelihood_at_edge(self, node_a, node_b):
        """Sitewise log-likelihood, expanded to alignment columns (tree_model.py:200-217)."""
        if self._is_root_edge(node_a, node_b):
            self._check_edge(node_a, node_b)
            self._ensure()
            return self.sitewise_patterns()[self.inverse_index]
        return self._edge_lnl(node_a, node_b)[1][self.inverse_index]

    # ------------------------------------------------------------------ edges
    def edge_derivatives(self, node_a, node_b, length=None):
        """(lnL, dlnL/dt, d2lnL/dt2) at length t of edge (a, b) (current length when None):
        the rate mixture of lnl_branch_derivs (numba_likelihood_engine.py:49-57) summed
        over patterns, on the nodes' current partials."""
        self._check_edge(node_a, node_b)
        self._ensure()
        out = np.zeros(3)
        N.check(N.lib().pu_edge_derivs(self._ctx, int(node_a), int(node_b),
                                       -1.0 if length is None else float(length), N.ptr(out)),
                self._ctx, "pu_edge_derivs")
        return float(out[0]), float(out[1]), float(out[2])

    def update_partials(self, ops, brlens):
        """In place, in order: partials[p] = clv(P(l1), P(l2), partials[c1], partials[c2]) for
        ops [n][3] (p, c1, c2) -- e.g. the re-orientation rows of optimising_traversal."""
        self._ensure()
        ops = np.ascontiguousarray(ops, dtype=np.int32).reshape(-1, 3)
        bl = N.f64(brlens).reshape(-1, 2)
        if len(bl) != len(ops):
            raise ValueError("one (len1, len2) pair per op")
        N.check(N.lib().pu_update_partials(self._ctx, len(ops), N.ptr(ops), N.ptr(bl)),
                self._ctx, "pu_update_partials")
        self._site_valid = False

    def _pull_lengths(self):
        """Device branch lengths -> self.traversal.brlens (the reference's BranchLengths)."""
        tr = self.traversal
        bl = np.empty((len(tr.postorder_traversal), 2))
        rl = ctypes.c_double()
        N.check(N.lib().pu_get_branch_lengths(self._ctx, N.ptr(bl), ctypes.byref(rl)),
                self._ctx, "pu_get_branch_lengths")
        for (p, a, b), (la, lb) in zip(tr.postorder_traversal, bl):
            tr.brlens[tuple(sorted((int(p), int(a))))] = float(la)
            tr.brlens[tuple(sorted((int(p), int(b))))] = float(lb)
        tr.brlens[tuple(sorted(tr.root_edge))] = rl.value

    def _minimise_edge(self, node_a, node_b, t0, method, tol, bracket):
        """The reference's 1-D minimisers (brent / dbrent of src/optimisation.pyx:86-297) on
        -lnL(t) of edge (a, b) over `bracket`, from t0: pu_minimise_edge, the whole
        minimisation in one persistent launch where the device takes it (r06), otherwise the
        same state machine with one k_edge launch per evaluation.  PU_PY_MINIMISE=1: the
        Python restatement (phylo_utils_amd.optimisation) over pu_edge_derivs instead (the
        tests' check of the library's state machine).  Returns (t, lnL at t)."""
        lo, hi = float(bracket[0]), float(bracket[1])
        if not 0.0 < lo < hi:
            raise ValueError("bracket must satisfy 0 < lo < hi, got %r" % (bracket,))
        if not os.environ.get("PU_PY_MINIMISE"):
            out = np.zeros(3)
            t0c = min(max(float(t0), lo), hi)
            N.check(N.lib().pu_minimise_edge(self._ctx, int(node_a), int(node_b),
                                             1 if method == "brent" else 2, lo, t0c, hi,
                                             float(tol), N.ptr(out)),
                    self._ctx, "pu_minimise_edge")
            self.last_edge_evaluations = int(out[2])
            return float(out[0]), -float(out[1])
        last = [None, None]
        out3 = np.zeros(3)

        def ev(t):
            if last[0] != t:
                N.check(N.lib().pu_edge_derivs(self._ctx, int(node_a), int(node_b), float(t),
                                               N.ptr(out3)), self._ctx, "pu_edge_derivs")
                last[0], last[1] = t, (float(out3[0]), float(out3[1]))
            return last[1]

        out = np.zeros(3)
        t0 = min(max(float(t0), lo), hi)
        if method == "brent":
            optimisation.brent(lo, t0, hi, lambda t: -ev(t)[0], tol, out)
        else:
            optimisation.dbrent(lo, t0, hi, lambda t: -ev(t)[0], lambda t: -ev(t)[1], tol, out)
        self.last_edge_evaluations = int(out[2])
        return float(out[0]), -float(out[1])

    def optimise_edge(self, node_a, node_b, tol=1e-8, max_iter=50, method="newton",
                      bracket=(1e-8, 10.0)):
        """Optimise the length of edge (a, b) with the partials of a and b held fixed (valid
        for the root edge, or after re-orientation); returns (length, lnL).
        method "newton": Newton-Raphson in the library (pu_optimise_edge); "brent" /
        "dbrent": the reference's minimisers (src/optimisation.pyx) over `bracket`."""
        self._check_edge(node_a, node_b)
        self._ensure()
        if method in ("brent", "dbrent"):
            key = tuple(sorted((int(node_a), int(node_b))))
            t, lnl = self._minimise_edge(node_a, node_b, self.traversal.brlens[key], method,
                                         tol, bracket)
            self.traversal.brlens[key] = t
            self.update_branch_lengths()
            return t, lnl
        if method != "newton":
            raise ValueError("method must be 'newton', 'brent' or 'dbrent'")
        t, lnl = ctypes.c_double(), ctypes.c_double()
        N.check(N.lib().pu_optimise_edge(self._ctx, int(node_a), int(node_b), float(tol),
                                         int(max_iter), ctypes.byref(t), ctypes.byref(lnl)),
                self._ctx, "pu_optimise_edge")
        self._pull_lengths()
        self._dirty = True
        return t.value, lnl.value

    def _sweep_minimise(self, rows, method, tol, bracket):
        """One optimising-traversal pass with brent / dbrent per edge, driven from the host:
        re-orientation rows are in-place device updates (pu_update_partials) at the lengths
        found so far, every evaluation a k_edge launch; then one traversal at the new
        lengths.  (Newton runs the whole pass inside the library: pu_optimise_sweep.)"""
        tr = self.traversal
        L = lambda u, v: tr.brlens[tuple(sorted((int(u), int(v))))]
        n_eval = 0
        for row in rows:
            if row[0] >= 0:
                op = np.ascontiguousarray(row[:3], dtype=np.int32)
                bl = N.f64([L(row[0], row[1]), L(row[0], row[2])])
                N.check(N.lib().pu_update_partials(self._ctx, 1, N.ptr(op), N.ptr(bl)),
                        self._ctx, "pu_update_partials")
            if row[3] >= 0:
                key = tuple(sorted((int(row[3]), int(row[4]))))
                t, _ = self._minimise_edge(row[3], row[4], tr.brlens[key], method, tol,
                                           bracket)
                tr.brlens[key] = t
                n_eval += self.last_edge_evaluations
        self.update_branch_lengths()
        self.compute_partials()
        return n_eval

    def optimise_branch_lengths(self, tol=1e-8, max_iter=50, sweeps=1, lnl_tol=None,
                                method="newton", bracket=(1e-8, 10.0)):
        """Branch-length optimisation over the optimising traversal
        (Traversal.optimising_traversal, utils.py:137-188): per pass, every edge in turn is
        optimised on GPU-resident re-oriented partials -- Newton-Raphson (default), or the
        reference's brent / dbrent (src/optimisation.pyx) over `bracket`.  Repeats up to
        `sweeps` passes, stopping early when a pass gains less than `lnl_tol`.  Returns the
        lnL."""
        self._ensure()
        if not self.keep_partials:
            raise ValueError("branch-length optimisation needs keep_partials=True")
        if method not in ("newton", "brent", "dbrent"):
            raise ValueError("method must be 'newton', 'brent' or 'dbrent'")
        rows = np.ascontiguousarray(self.traversal.optimising_traversal, dtype=np.int32)
        prev = self._lnl
        for _ in range(int(sweeps)):
            if method != "newton":
                self.last_newton_iterations = self._sweep_minimise(rows, method, tol, bracket)
                if lnl_tol is not None and self._lnl - prev < lnl_tol:
                    break
                prev = self._lnl
                continue
            lnl, n_it = ctypes.c_double(), ctypes.c_int()
            N.check(N.lib().pu_optimise_sweep(self._ctx, len(rows), N.ptr(rows), float(tol),
                                              int(max_iter), ctypes.byref(lnl),
                                              ctypes.byref(n_it)), self._ctx,
                    "pu_optimise_sweep")
            self._lnl = lnl.value
            self._site_valid = True
            self.last_newton_iterations = n_it.value
            if lnl_tol is not None and self._lnl - prev < lnl_tol:
                break
            prev = self._lnl
        self._pull_lengths()
        return self._lnl

    # ------------------------------------------------------------------ tree search
    def quartet_derivatives(self, nodes, lens, t=None):
        """(lnL, dlnL/dt, d2lnL/dt2) [3][3] of the three arrangements of four nodes on their
        current partials (``nni.quartet_derivatives``, pu_quartet_derivs)."""
        from . import nni
        return nni.quartet_derivatives(self, nodes, lens, t)

    def nni_scores(self, tol=1e-8, max_iter=50):
        """Every internal edge's three arrangements, central lengths optimised, in one pass of
        the optimising traversal (``nni.nni_scores``, pu_nni_sweep): (quartets [n][6], scores
        [n][3][4])."""
        from . import nni
        return nni.nni_scores(self, tol, max_iter)

    def nni_search(self, max_rounds=50, min_gain=1e-3, sweeps=1, tol=1e-8, method="newton"):
        """Nearest-neighbour-interchange search from the current tree (``nni.nni_search``):
        returns (tree, lnL, history); the model ends on that tree with its lengths optimised."""
        from . import nni
        return nni.nni_search(self, max_rounds, min_gain, sweeps, tol, method)

    def spr_scores(self, radius=None):
        """The lnL of every subtree-pruning-and-regrafting move within `radius` edges (None: all)
        at unchanged lengths, in one pass of the optimising traversal (``spr.spr_scores``,
        pu_spr_sweep): (moves [n][5] = n, o, u, v, distance; scores [n])."""
        from . import spr
        return spr.spr_scores(self, radius)

    def spr_search(self, radius=None, max_rounds=50, keep=5, min_gain=1e-3, sweeps=1, tol=1e-8,
                   method="newton"):
        """Subtree-pruning-and-regrafting search from the current tree (``spr.spr_search``):
        returns (tree, lnL, history); the model ends on that tree with its lengths optimised."""
        from . import spr
        return spr.spr_search(self, radius, max_rounds, keep, min_gain, sweeps, tol, method)

    def quartet_site_lnl(self, nodes, lens, t=None):
        """The unweighted per-pattern lnL of the three arrangements of four nodes, and their
        {lnL, d1, d2} (``support.quartet_site_lnl``, pu_quartet_site_lnl): (site [3][S],
        out [3][3])."""
        from . import support
        return support.quartet_site_lnl(self, nodes, lens, t)

    def branch_support(self, n_replicates=1000, seed=0, epsilon=0.05, tol=1e-8, max_iter=50,
                       first_replicate=0, full=False):
        """aLRT, aBayes and SH-aLRT of every internal edge in one scoring pass
        (``support.branch_support``, pu_branch_support): (quartets, scores, support dict of
        lrt, alrt_chi2, abayes, sh_alrt [n])."""
        from . import support
        return support.branch_support(self, n_replicates, seed, epsilon, tol, max_iter,
                                      first_replicate, full)

    def topology_tests(self, trees, n_replicates=10000, scales=None, seed=0, optimise=True,
                       sweeps=1):
        """RELL bootstrap proportions, KH, SH, c-ELW and AU of the candidate `trees` on this
        model's alignment and models (``topotest.topology_tests``, pu_topology_tests): a dict of
        arrays [T].  `scales` None: the ten default scales of the AU test.  The model ends on the
        tree it started on."""
        from . import topotest
        return topotest.topology_tests(
            self, trees, n_replicates, topotest.DEFAULT_SCALES if scales is None else scales, seed,
            optimise, sweeps)

    # ------------------------------------------------------------------ ancestral states
    def ancestral_states(self, full=False):
        """The most probable state of every internal node at every pattern, its posterior and,
        with `full`, all posteriors, in one pass of the optimising traversal
        (``ancestral.ancestral_states``, pu_ancestral_sweep)."""
        from . import ancestral
        return ancestral.ancestral_states(self, full)

    def ancestral_sequences(self, alphabet):
        """({"N<idx>": sequence over the alignment's columns}, the Newick that carries those
        labels) (``ancestral.ancestral_sequences``)."""
        from . import ancestral
        return ancestral.ancestral_sequences(self, alphabet)

    def site_rates(self):
        """(posterior of the rate category [sites][C], mean rate [sites]) per alignment column
        (``ancestral.site_rates``, pu_site_rates)."""
        from . import ancestral
        return ancestral.site_rates(self)

    # ------------------------------------------------------------------ gradients, model fitting
    def edge_counts(self):
        """The joint count matrices of every edge in one pass of the optimising traversal
        (``gradient.edge_counts``, pu_counts_sweep)."""
        from . import gradient
        return gradient.edge_counts(self)

    def gradient(self, params=(), branch_lengths=True):
        """(dict name -> dlnL/dparam, dict (nod, par) -> dlnL/dt or None) from one pass of the
        count kernel (``gradient.model_gradient`` / ``gradient.branch_gradient``)."""
        from . import gradient
        res = gradient.edge_counts(self)
        return (gradient.model_gradient(self, params, res) if params else {},
                gradient.branch_gradient(self, res) if branch_lengths else None)

    def optimise_model(self, params=("alpha", "rates", "freqs"), branch_lengths=True,
                       max_iter=200, lnl_tol=1e-6):
        """Fit the named model parameters and, when asked, all branch lengths jointly
        (``modelfit.optimise_model``)."""
        from . import modelfit
        return modelfit.optimise_model(self, params, branch_lengths, max_iter, lnl_tol)

    # ------------------------------------------------------------------ placement
    def place(self, queries, keep=5, pendant0=None, tol=1e-8, max_iter=50, alphabet=None):
        """Place query sequences on the model's tree without rebuilding it: every query scored
        at every edge in one pass, the `keep` best edges of each refined by Newton on the pendant
        length (``place.place``, pu_place_prescore / pu_place_refine)."""
        from . import place
        return place.place(self, queries, keep, pendant0, tol, max_iter, alphabet)

    # ------------------------------------------------------------------ simulation
    def simulate(self, n_sites, seed=0, first_site=0, return_categories=False,
                 return_ancestral=False, return_cum=False):
        """Simulate `n_sites` alignment columns down this model's tree on its own context
        (pu_simulate; the reference's src/simulation.pyx evolve_states per branch): the
        current topology, branch lengths -- after optimise_edge / optimise_branch_lengths too,
        with no re-upload -- and models.  Returns the states uint8 [n_taxa][n_sites], rows in
        `self.names` order; with any of the flags a tuple (states[, categories [n_sites]]
        [, states of every node [n_nodes][n_sites]][, the cumulative rows the draws used
        [n_nodes][C][K][K]]).  Column j is global site first_site + j and depends only on the
        seed and that number (phylo_utils_amd.simulation).  The resident partials, the lnL and
        the model's state are left as they are."""
        if self._ctx is None:
            raise ValueError("initialise first")
        from .simulation import simulate_on_context
        n_nodes, n_leaves, _, C, K = self._ctx_shape
        res = simulate_on_context(self._ctx, n_leaves, n_nodes, C, K, n_sites, seed, first_site,
                                  return_categories, return_ancestral, return_cum)
        rows = np.array([self.names[n] for n in self._slot_names])
        states = np.empty_like(res["tips"])
        states[rows] = res["tips"]
        extra = [res[k] for k in ("cats", "nodes", "cum") if k in res]
        return (states,) + tuple(extra) if extra else states

    # ------------------------------------------------------------------ outputs
    def _coded_alignment(self):
        """(codes, table, names in alignment order) of the model's alignment, for the calls that
        work on coded rows (pairwise distances, the bootstrap)."""
        if self.alignment is None:
            raise ValueError("No alignment has been set")
        names = sorted(self.names, key=self.names.get)
        if getattr(self, "_codes", None) is not None:
            codes, table = self._codes
        else:
            coded = partials_to_codes(np.asarray(self.alignment))
            if coded is None or len(coded[1]) > 32:
                raise ValueError("pairwise distances need tips of at most 32 distinct vectors")
            codes, table = coded
        return codes, table, names

    def pairwise_distances(self, **kw):
        """ML distances and variances of all pairs of the model's own alignment under its
        substitution and rate models (``distance.pairwise_distances``; the reference's
        phylo_utils/likelihood.py:226-236 per pair): (names in alignment order, D, V).  Needs no
        tree and does not touch the context."""
        from . import distance
        codes, table, names = self._coded_alignment()
        kw.setdefault("device", self.device)
        kw.setdefault("weights", np.asarray(self.siteweights, dtype=np.float64))
        return distance.pairwise_distances((codes, table, names), self.substitution_model,
                                           getattr(self, "rate_model", None), **kw)

    def set_nj_tree(self, method="nj", **distance_kw):
        """A starting tree from the model's own data: ``pairwise_distances(**distance_kw)`` on
        its alignment and models, then neighbour joining (`method` "nj" or "bionj",
        ``nj.neighbour_joining``) on that matrix, then ``set_tree``.  Branch lengths below the
        optimisers' lower bound 1e-8 (NJ lengths may be negative) are raised to it.  Needs what
        the distances need: coded tips and a reversible model.  Returns the tree."""
        from . import nj
        names, D, _ = self.pairwise_distances(**distance_kw)
        tree = nj.neighbour_joining(D, names, method=method, min_length=1e-8,
                                    device=self.device)
        self.set_tree(tree)
        return tree

    def parsimony_length(self, per_pattern=False):
        """The Fitch parsimony length of the model's tree on its own alignment and
        ``siteweights`` (``parsimony.fitch_lengths``), an integer; with
        `per_pattern` also the unweighted changes of every pattern, in pattern order as
        ``sitewise_patterns`` gives them.  Needs no context and no model, and leaves the
        likelihood state as it is."""
        from . import parsimony
        if getattr(self, "tree", None) is None:
            raise ValueError("No tree has been set")
        codes, table, names = self._coded_alignment()
        return parsimony.fitch_lengths((codes, table, names), self.tree,
                                       weights=self.siteweights, per_pattern=per_pattern,
                                       device=self.device)

    def set_parsimony_tree(self, n_rep=1, seed=0, min_length=1e-8, spr_rounds=None,
                           spr_radius=None, return_classes=False):
        """A starting tree by randomised stepwise addition under Fitch parsimony
        (``parsimony.stepwise_addition``): `n_rep` random addition orders
        (``parsimony.random_orders(n, n_rep, seed)``), the shortest tree kept, ties to the lowest
        replicate.  With `spr_rounds` a number, all `n_rep` trees are first refined in one batch
        by parsimony SPR (``parsimony.spr_search``, DESIGN 4.26: at most `spr_rounds` rounds, 0
        until no move improves, regrafts within `spr_radius` edges, None or 0 for no limit) and
        the shortest refined tree is kept.  Every branch length is ``max(edge change count / sum
        of siteweights, min_length)``.  Needs coded tips and no model at all, so it also serves
        the non-reversible models ``set_nj_tree`` refuses.  Calls ``set_tree``; returns (tree,
        length, the lengths of all replicates), and with `return_classes` also
        ``treeset.topology_classes`` of the `n_rep` (refined) trees, int [n_rep]: for each the
        index of the first replicate with the same topology, so ``len(set(classes))`` is the
        number of distinct topologies the replicates reached."""
        from . import parsimony
        aln = self._coded_alignment()
        w = parsimony.integer_weights(self.siteweights, aln[0].shape[1])
        edges, _, lengths = parsimony.stepwise_addition(aln, n_rep=n_rep, seed=seed, weights=w,
                                                        device=self.device)
        if spr_rounds is not None:
            edges, lengths, _ = parsimony.spr_search(aln, edges, weights=w, radius=spr_radius,
                                                     max_rounds=spr_rounds, device=self.device)
        best = int(np.argmin(lengths))  # the first of equal lengths
        tree = parsimony.edges_to_tree(edges[best], aln[2])
        _, per_edge = parsimony.fitch_lengths(aln, tree, weights=w, per_edge=True,
                                              device=self.device)
        tree = parsimony.edge_lengths_tree(tree, aln[2], per_edge, int(w.sum()), min_length)
        self.set_tree(tree)
        if return_classes:
            from . import treeset
            classes = treeset.topology_classes(
                treeset.compare(edges, rows=0, device=self.device, want_table=False))
            return tree, int(lengths[best]), lengths, classes
        return tree, int(lengths[best]), lengths

    def bootstrap_nj(self, n_replicates=100, seed=0, method="nj", return_replicates=False,
                     **distance_kw):
        """``set_nj_tree`` with bootstrap support (``bootstrap.bootstrap_nj`` on the model's own
        alignment and models): the reference tree becomes the model's tree, as ``set_nj_tree``
        sets it, with every internal node that carries one of its splits labelled with the
        split's support in percent over `n_replicates` resampled alignments.  Returns (tree,
        support [n-3] of clusters n + m in join order, n_ok: the replicates counted), and with
        `return_replicates` also (joins [R][n-2][2], roots [R][2]) of the replicate trees, rows
        in alignment order: a tree set for ``treeset.compare`` (``form="joins"``) as long as
        ``n_ok`` equals `n_replicates` (the tree of a replicate that is not ok is unspecified)."""
        from . import bootstrap
        codes, table, names = self._coded_alignment()
        distance_kw.setdefault("device", self.device)
        distance_kw.setdefault("weights", np.asarray(self.siteweights, dtype=np.float64))
        out = bootstrap.bootstrap_nj(
            (codes, table, names), self.substitution_model, getattr(self, "rate_model", None),
            n_replicates=n_replicates, seed=seed, method=method, min_length=1e-8,
            return_replicates=bool(return_replicates), **distance_kw)
        self.set_tree(out[0])
        return out

    def rf_distance(self, other):
        """The Robinson-Foulds distance between the model's current tree and `other` (a
        ``Tree`` or Newick over the same names), an int (``treeset.rf_distances``)."""
        from . import treeset
        if getattr(self, "tree", None) is None:
            raise ValueError("No tree has been set")
        names = sorted(self.names, key=self.names.get)
        return int(treeset.rf_distances([self.tree, other], names, device=self.device)[0, 1])

    def tree_distance(self, other, metric="kf"):
        """The distance between the model's current tree with its current branch lengths and
        `other` (a ``Tree`` or Newick over the same names, with a length on every edge), a float:
        `metric` ``"wrf"``, ``"kf"``, ``"path"`` or ``"wpath"`` of ``treeset.distances`` (DESIGN
        4.31)."""
        from . import treeset
        from .tree import with_lengths
        if getattr(self, "tree", None) is None:
            raise ValueError("No tree has been set")
        if not isinstance(metric, str):
            raise ValueError("metric is one name, not %r" % (metric,))
        names = sorted(self.names, key=self.names.get)
        current = with_lengths(self.tree, self.traversal.brlens)
        return float(treeset.distances([current, other], metric, names, rows=1,
                                       device=self.device)[0, 1])

    def map_support(self, trees):
        """Label the model's current tree with the support of the tree set `trees` -- any form
        ``treeset.compare`` takes, arrays over the alignment's rows: the replicates of
        ``bootstrap_nj(return_replicates=True)``, a list of Newick strings, edge lists -- through
        ``treeset.support``.  Returns (support [2n-3] per edge of the tree in op order, NaN on
        pendant edges, the labelled copy of the tree with the model's current branch
        lengths); the model's own tree is left as it is."""
        from . import treeset
        from .tree import with_lengths
        if getattr(self, "tree", None) is None:
            raise ValueError("No tree has been set")
        names = sorted(self.names, key=self.names.get)
        current = with_lengths(self.tree, self.traversal.brlens)
        return treeset.support(current, trees, names=names, device=self.device)

    def concordance_factors(self, trees=None, n_quartets=100, seed=0):
        """The concordance factors of every internal branch of the model's tree (DESIGN 4.29,
        ``phylo_utils_amd.concordance``): the site factors on the model's own alignment and
        ``siteweights`` (``concordance.site_concordance``: up to `n_quartets` quartets per
        branch, drawn under `seed`) and, when `trees` is given -- any form ``treeset.compare``
        takes, over the alignment's rows -- the gene factors in that tree set
        (``concordance.gene_concordance``).  One ``ConcordanceResult``, its edges the tree's in
        op order, its ``pairs`` the model's own node indices.  Needs coded tips and no
        substitution model, so it serves the non-reversible models too; the likelihood state is
        left as it is."""
        from . import concordance
        if getattr(self, "tree", None) is None:
            raise ValueError("No tree has been set")
        aln = self._coded_alignment()
        res = concordance.site_concordance(aln, self.tree, n_quartets=n_quartets, seed=seed,
                                           weights=self.siteweights, device=self.device,
                                           _prepared=True)
        if trees is not None:
            res = concordance.merge(res, concordance.gene_concordance(
                self.tree, trees, names=aln[2], device=self.device, _prepared=True))
        return res

    def likelihood_mapping(self, n_quartets=None, seed=0, clusters=None, **optimiser):
        """The likelihood map (``phylo_utils_amd.lmap``) of the model's own alignment
        and ``siteweights`` under its substitution and rate models: `n_quartets` quartets (None:
        min(C(n, 4), 25 n)) drawn under `seed` -- of the four `clusters` where given: an array
        over the rows in {-1, 0, 1, 2, 3} or four lists of taxon names -- each fitted under its
        three topologies.  Returns a ``lmap.LikelihoodMap``.  Needs coded tips and a reversible
        model, and no tree; the context is not touched.  `optimiser`: t0, tol, max_iter,
        max_rounds, min_gain of ``lmap.quartet_likelihoods``."""
        from . import lmap
        codes, table, names = self._coded_alignment()
        return lmap.likelihood_mapping(
            (codes, table, names), self.substitution_model, getattr(self, "rate_model", None),
            n_quartets=n_quartets, seed=seed, clusters=clusters, device=self.device,
            weights=np.asarray(self.siteweights, dtype=np.float64), **optimiser)

    def likelihood(self):
        """Total lnL = sum of sitewise lnL over alignment columns (bin/phy.py:146)."""
        self._ensure()
        return self._lnl

    def _n_patterns(self):
        n = self.alignment.shape[1]
        return n + self.alignment.shape[2] if self.ascbias else n

    def sitewise_patterns(self):
        """Per-pattern lnL (tree_model.py:216, before the inverse-index expansion; with
        the ascertainment correction the K dummy patterns come last)."""
        self._ensure()
        if not self._site_valid:
            self.compute_partials()
        out = np.empty(self._n_patterns())
        N.check(N.lib().pu_get_site_lnl(self._ctx, N.ptr(out)), self._ctx, "pu_get_site_lnl")
        return out

    def node_partials(self, node):
        self._ensure()
        S, K = self._n_patterns(), self.alignment.shape[2]
        C = self.rate_model.ncat
        p = np.empty((S, C, K))
        s = np.empty((S, C))
        N.check(N.lib().pu_get_partials(self._ctx, int(node), N.ptr(p), N.ptr(s)), self._ctx,
                "pu_get_partials")
        return p, s

    @property
    def partials(self):
        """[2N-2][S][C][K], tips broadcast over categories (tree_model.py:117-148)."""
        return np.stack([self.node_partials(v)[0] for v in range(self.traversal.n_nodes)])

    @property
    def scale(self):
        return np.stack([self.node_partials(v)[1] for v in range(self.traversal.n_nodes)])

    def _root(self):
        self._ensure()
        S, K = self._n_patterns(), self.alignment.shape[2]
        C = self.rate_model.ncat
        rp = np.empty((S, C, K))
        rs = np.empty((S, C))
        N.check(N.lib().pu_get_root(self._ctx, N.ptr(rp), N.ptr(rs)), self._ctx, "pu_get_root")
        return rp, rs

    @property
    def root_partials(self):
        return self._root()[0]

    @property
    def root_scale(self):
        return self._root()[1]

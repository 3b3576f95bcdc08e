"""An error in the middle of a walk over the optimising traversal (pu_resident.h): what the tests
of pu_ancestral_sweep, pu_counts_sweep, pu_nni_sweep / pu_branch_support and pu_optimise_sweep
share.  The last edge row's PAR is replaced by a node that is not NOD's neighbour; by then
earlier rows have re-oriented nodes.  The call must return PU_E_ARG with a message and leave the
context's lnL, sitewise lnL and partials bitwise as they were."""
import ctypes

import numpy as np

from phylo_utils_amd import _native as N


def rows_with_a_bad_last_edge(tm):
    tr = tm.traversal
    rows = np.ascontiguousarray(tr.optimising_traversal, dtype=np.int32)
    last = max(i for i in range(len(rows)) if rows[i][3] >= 0)
    assert any(rows[i][0] >= 0 for i in range(last))  # nodes are re-oriented before it
    nod, par = int(rows[last][3]), int(rows[last][4])
    bad = rows.copy()
    bad[last][4] = next(v for v in range(tr.n_nodes) if v not in (nod, par) and
                        (min(v, nod), max(v, nod)) not in tr.brlens)
    return bad


def snapshot(tm):
    """The context's own lnL, its sitewise lnL and the partials and scalers of every internal
    node, read from the device."""
    lnl = ctypes.c_double()
    assert N.lib().pu_synchronize(tm._ctx, ctypes.byref(lnl)) == 0
    site = np.empty(tm._n_patterns())
    assert N.lib().pu_get_site_lnl(tm._ctx, N.ptr(site)) == 0
    inner = sorted(set(int(p) for p in tm.traversal.postorder_traversal[:, 0]))
    return dict(lnl=lnl.value, site=site, parts=[tm.node_partials(v) for v in inner])


def assert_refused_and_put_back(tm, before, rc):
    assert rc == N.PU_E_ARG
    assert N.last_error(tm._ctx)
    after = snapshot(tm)
    assert after["lnl"] == before["lnl"]
    assert np.array_equal(after["site"], before["site"])
    for (p0, s0), (p1, s1) in zip(before["parts"], after["parts"]):
        assert np.array_equal(p0, p1) and np.array_equal(s0, s1)

"""numpy restatement of the simulator's specification: Philox4x32-10, the uniform
``u``, the choice rule ``pick`` and the walk down a schedule given the cumulative rows.

Test infrastructure: nothing under ``phylo_utils_amd/`` imports it.  Every function follows the
specification literally -- plain fp64 adds in index order, one multiplication ``u * total`` --
so the device result can be compared bit for bit.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 uint32 arrays (or scalars), key: 2 -> the 4 output words as uint64 arrays
    holding 32-bit values."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) & _MASK for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(x) & 0xFFFFFFFF for x in key)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]  # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _MASK,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _MASK]
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return c


def uniform(seed, g, d):
    """u of draw d of global sites g (array) under a 64-bit seed: float64 in [0, 1)."""
    g = np.atleast_1d(np.asarray(g, dtype=np.uint64))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10((g & _MASK, g >> np.uint64(32), np.uint64(d), np.uint64(0)),
                      (seed & 0xFFFFFFFF, seed >> 32))
    m = ((x[1] >> np.uint64(5)) << np.uint64(26)) | (x[0] >> np.uint64(6))
    return m.astype(np.float64) * 2.0 ** -53


def cumulate(w):
    """cum_j = cum_{j-1} + w_j along the last axis, fp64 adds in index order."""
    w = np.asarray(w, dtype=np.float64)
    out = np.empty_like(w)
    out[..., 0] = w[..., 0]
    for j in range(1, w.shape[-1]):
        out[..., j] = out[..., j - 1] + w[..., j]
    return out


def pick_cum(cum, u):
    """cum [n][m] (or [m]) cumulative rows, u [n]: the first j with cum_j > u * cum_{m-1},
    else m - 1."""
    cum = np.asarray(cum, dtype=np.float64)
    u = np.atleast_1d(np.asarray(u, dtype=np.float64))
    if cum.ndim == 1:
        cum = np.broadcast_to(cum, (len(u), len(cum)))
    r = u * cum[:, -1]
    gt = cum > r[:, None]
    return np.where(gt.any(axis=1), gt.argmax(axis=1), cum.shape[1] - 1).astype(np.uint8)


def pick(w, u):
    """The choice rule on weights w[0..n) for one u (or an array of u)."""
    out = pick_cum(cumulate(w), u)
    return out if np.ndim(u) else int(out[0])


def walk(ops, root_a, root_b, cum, weights, freqs, seed, first_site, n_sites):
    """(cats uint8 [n_sites], nodes uint8 [n_nodes][n_sites]) of the walk over `ops`
    ([n_ops][3] post-order rows (parent, child1, child2)) away from root_a, from the cumulative
    rows cum [n_nodes][C][K][K] (row v: the edge above v)."""
    cum = np.asarray(cum, dtype=np.float64)
    n_nodes = cum.shape[0]
    g = np.uint64(first_site) + np.arange(n_sites, dtype=np.uint64)
    cats = pick_cum(cumulate(weights), uniform(seed, g, 0))
    nodes = np.zeros((n_nodes, n_sites), dtype=np.uint8)
    nodes[root_a] = pick_cum(cumulate(freqs), uniform(seed, g, 1))

    def draw(v, parent):
        nodes[v] = pick_cum(cum[v][cats, nodes[parent]], uniform(seed, g, 2 + v))

    draw(root_b, root_a)
    for p, c1, c2 in np.asarray(ops, dtype=np.int64).reshape(-1, 3)[::-1]:
        draw(int(c1), int(p))
        draw(int(c2), int(p))
    return cats, nodes


def cum_rows(model, rates, ops, brlens, root_a, root_b, root_len, n_nodes):
    """Host cumulative rows [n_nodes][C][K][K] from model.p at the schedule's lengths."""
    K, C = len(model.freqs), len(rates)
    out = np.zeros((n_nodes, C, K, K))
    out[root_b] = cumulate(model.p(root_len, rates))
    for (p, c1, c2), (l1, l2) in zip(np.asarray(ops).reshape(-1, 3),
                                     np.asarray(brlens).reshape(-1, 2)):
        out[int(c1)] = cumulate(model.p(l1, rates))
        out[int(c2)] = cumulate(model.p(l2, rates))
    return out

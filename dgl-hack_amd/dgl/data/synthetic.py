"""Seeded synthetic power-law edge lists for the benchmark configs (the real datasets
need network downloads).

``chung_lu_edges`` draws the same edges on every process and every run for a seed:
multi-rank jobs build the graph independently on each rank and must agree on it
(``th.multinomial`` on the device gave a different draw per call for the same
generator state, so ranks disagreed on the C5 partition).  The weights' prefix sum is
formed on the host in fp64; the device draws uniforms from a seeded generator and
inverts the CDF with a binary search -- both order-independent."""
import torch as th

__all__ = ["chung_lu_edges", "planted_cluster_edges"]


def chung_lu_edges(n, m, alpha, seed, device):
    """(src, dst) int32 device tensors of ``m`` edges over ``n`` nodes; each end drawn
    independently with probability proportional to w_i = rank_i^-alpha, ranks
    permuted by ``seed`` (Chung-Lu, in-/out-degrees ~ power law)."""
    gc = th.Generator().manual_seed(int(seed))
    w = th.arange(1, n + 1, dtype=th.float64).pow(-float(alpha))
    w = w[th.randperm(n, generator=gc)]
    cdf = th.cumsum(w, 0)
    cdf /= cdf[-1].item()
    cdf = cdf.to(device)
    g = th.Generator(device=device)
    g.manual_seed(int(seed))
    ends = []
    for _ in range(2):
        u = th.rand(m, generator=g, device=device, dtype=th.float64)
        ends.append(th.searchsorted(cdf, u, right=True).clamp_(max=n - 1).to(th.int32))
        del u
    return ends[0], ends[1]


def planted_cluster_edges(n, clusters, m, p_in, seed, device):
    """(src, dst, label): ``m`` int32 device edges over ``n`` nodes in ``clusters`` planted
    clusters (node v belongs to cluster v mod clusters; ``label`` int64).  An edge stays
    inside its source's cluster with probability ``p_in`` and goes anywhere otherwise.  The
    draws come from a seeded host generator, so every process agrees on the graph."""
    gc = th.Generator().manual_seed(int(seed))
    src = th.randint(0, n, (m,), generator=gc)
    anywhere = th.randint(0, n, (m,), generator=gc)
    inside = th.rand(m, generator=gc) < float(p_in)
    # a node of the source's cluster: round `anywhere` down to that residue class
    same = anywhere - anywhere % clusters + src % clusters
    same = th.where(same >= n, same - clusters, same)
    dst = th.where(inside, same, anywhere)
    label = th.arange(n) % clusters
    return src.to(device, th.int32), dst.to(device, th.int32), label.to(device)

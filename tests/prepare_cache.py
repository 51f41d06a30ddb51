"""What the tests of the three cached `prepare` methods (GraphSAGE, GATRec, LightGCN) share.

The caches are keyed on (data_ptr, shape, _version) of the edge_index tensor.  An allocator hands a freed block of the
same size out again, so a caller who drops one edge_index and builds another of the same shape presents the same key with
other content; the cache must hold the tensor it was built from, or the model propagates over the previous graph."""
import numpy as np
import torch

DRAWS = 20


def draw(k, n_nodes, n_edges, device="cpu"):
    """int64 [2, n_edges], a function of k; entries below n_nodes - 1, so that adding 1 to one stays a node."""
    return torch.randint(0, n_nodes - 1, (2, n_edges), generator=torch.Generator().manual_seed(1000 + k)).to(device)


def same_csr(a, b):
    return (np.array_equal(a.rowptr_host, b.rowptr_host) and torch.equal(a.col.cpu(), b.col.cpu())
            and (a.val is None) == (b.val is None) and (a.val is None or torch.equal(a.val.cpu(), b.val.cpu())))


def check_prepare_cache(prepare, build, n_nodes, n_edges=400, device="cpu"):
    """prepare(edge_index) -> the module's cached graph; build(edge_index) -> a graph freshly built by the module's own
    builder.  Returns the number of the DRAWS fresh tensors for which `prepare` returned a graph of other content (after
    asserting that there is none), for the report."""
    e1 = draw(0, n_nodes, n_edges, device)
    g1 = prepare(e1)
    assert prepare(e1) is g1, "the same tensor twice must return the cached graph"
    assert same_csr(g1, build(e1))
    del e1, g1
    stale = 0
    for k in range(1, DRAWS + 1):
        e = draw(k, n_nodes, n_edges, device)               # same shape, other content, version 0, often the freed address
        stale += not same_csr(prepare(e), build(e))
        del e
    print(f"PREPARE cache: {stale} of {DRAWS} fresh tensors got a stale graph")
    assert stale == 0, f"{stale} of {DRAWS} fresh edge_index tensors of the same shape got the previous tensor's graph"
    e = draw(DRAWS + 1, n_nodes, n_edges, device)
    g = prepare(e)
    e[0, 0] += 1                                            # moves _version
    g2 = prepare(e)
    assert g2 is not g and same_csr(g2, build(e)), "an in-place edit must rebuild the graph"
    assert prepare(e) is g2
    return stale

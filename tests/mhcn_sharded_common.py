"""Shared by the CPU (gloo) and GPU two-rank tests of the row-sharded MHCN layer loop (BASELINE config 5):
a seeded synthetic problem, its single-process float64 reference (torch autograd on dense operators — a
restatement of oracle_np.mhcn_layer_loop, i.e. univariate/mhcn.py:422-466), and the per-rank partition.
`reference` itself is pinned to the reference's own float64 run of that loop, values and every gradient, by
tests/test_oracle_golden.py::test_sharded_mhcn_oracle_matches_reference_run (tests/golden/mhcn_wide_f64.npz).
Sizes are arguments; the defaults are the 101-user, d = 16 problem."""
import numpy as np
import torch

N_USERS, N_ITEMS, D, LAYERS = 101, 37, 16, 2          # 101 users: not divisible by 2 -> padded user rows
NNZ = (900, 700, 400, 600)                            # draws for H_s, H_j, H_p, R
GRAD_KEYS = ("user", "item", "att", "att_mat") + tuple(f"g{p}{c}" for c in range(4) for p in "wb")   # all propagate() reaches


def problem(seed=0, n_users=N_USERS, n_items=N_ITEMS, d=D, nnz=NNZ):
    rng = np.random.default_rng(seed)

    def rand_rownorm(n_r, n_c, nnz):
        m = np.zeros((n_r, n_c))
        m[rng.integers(0, n_r, nnz), rng.integers(0, n_c, nnz)] = rng.random(nnz) + 0.1
        rs = m.sum(1, keepdims=True)
        return np.divide(m, rs, out=np.zeros_like(m), where=rs > 0)

    H = [rand_rownorm(n_users, n_users, nnz[0]), rand_rownorm(n_users, n_users, nnz[1]), rand_rownorm(n_users, n_users, nnz[2])]
    R = rand_rownorm(n_users, n_items, nnz[3])
    p = {"user": rng.standard_normal((n_users, d)) * 0.3, "item": rng.standard_normal((n_items, d)) * 0.3,
         "att": rng.standard_normal((1, d)) * 0.3, "att_mat": rng.standard_normal((d, d)) * 0.3,
         "wu": rng.standard_normal((n_users, d)), "wi": rng.standard_normal((n_items, d))}
    for c in range(4):
        p[f"gw{c}"] = rng.standard_normal((d, d)) * 0.3
        p[f"gb{c}"] = rng.standard_normal((1, d)) * 0.1
    return H, R, p


def reference(H, R, p, layers=LAYERS):
    """Single-process float64 result: final user / item embeddings and the gradients of
    sum(final_user * wu) + sum(final_item * wi) w.r.t. every parameter (GRAD_KEYS).  H: three dense [U, U] operators,
    R: dense [U, I], p: the arrays of `problem` (any sizes)."""
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=k not in ("wu", "wi")) for k, v in p.items()}
    Ht = [torch.tensor(h, dtype=torch.float64) for h in H]
    Rt = torch.tensor(R, dtype=torch.float64)
    norm = lambda x: torch.nn.functional.normalize(x, p=2, dim=1)      # noqa: E731

    def gate(c):
        return t["user"] * torch.sigmoid(t["user"] @ t[f"gw{c}"] + t[f"gb{c}"])

    def attend(*e):
        w = torch.softmax(torch.stack([(t["att"] * (x @ t["att_mat"])).sum(1) for x in e]), 0)
        return sum(w[k].unsqueeze(1) * x for k, x in enumerate(e))

    c = [gate(0), gate(1), gate(2)]
    simple, items = gate(3), t["item"]
    sums = [c[0], c[1], c[2], simple, items]
    for _ in range(layers):
        mixed = attend(*c) + simple / 2
        for k in range(3):
            c[k] = Ht[k] @ c[k]
            sums[k] = sums[k] + norm(c[k])
        new_items = Rt.T @ mixed
        sums[4] = sums[4] + norm(new_items)
        simple = Rt @ items
        sums[3] = sums[3] + norm(simple)
        items = new_items
    fu = attend(sums[0], sums[1], sums[2]) + sums[3] / 2
    fi = sums[4]
    ((fu * t["wu"]).sum() + (fi * t["wi"]).sum()).backward()
    grads = {k: v.grad.numpy() for k, v in t.items() if v.grad is not None}
    return fu.detach().numpy(), fi.detach().numpy(), grads


def coo_block(m, lo, hi, n_cols_pad):
    """Rows [lo, hi) of dense m as COO over n_cols_pad columns (local row ids)."""
    blk = m[lo:hi]
    r, c = np.nonzero(blk)
    return r.astype(np.int64), c.astype(np.int64), blk[r, c].astype(np.float32), n_cols_pad


def load_params(enc, p, lo, hi, device):
    n_loc = enc.user_num
    with torch.no_grad():
        u = np.zeros((n_loc, p["user"].shape[1]), dtype=np.float32)
        u[: hi - lo] = p["user"][lo:hi]
        enc.user_embeddings.copy_(torch.from_numpy(u).to(device))
        enc.item_embeddings.copy_(torch.from_numpy(p["item"].astype(np.float32)).to(device))
        enc.attention.copy_(torch.from_numpy(p["att"].astype(np.float32)).to(device))
        enc.attention_mat.copy_(torch.from_numpy(p["att_mat"].astype(np.float32)).to(device))
        for c in range(4):
            enc.gating_weights[str(c + 1)].copy_(torch.from_numpy(p[f"gw{c}"].astype(np.float32)).to(device))
            enc.gating_bias[str(c + 1)].copy_(torch.from_numpy(p[f"gb{c}"].astype(np.float32)).to(device))


def run_rank(rank, world, device, make_graph, ops, group=None, layers=LAYERS, **sizes):
    """Builds rank's blocks with make_graph(row, col, val, n_rows, n_cols), runs propagate + backward of this
    rank's share of the loss, returns numpy results: fu, fi and g_<key> for every key of GRAD_KEYS.
    sizes: `problem`'s arguments."""
    from recommendation_amd import distributed as gd
    from recommendation_amd.mhcn import ShardedMHCNEncoder
    H, R, p = problem(**sizes)
    n_users, n_items, d = R.shape[0], R.shape[1], p["user"].shape[1]
    per_u = (n_users + world - 1) // world
    lo, hi = rank * per_u, min((rank + 1) * per_u, n_users)
    u_pad = per_u * world
    blocks = []
    for h in H:
        hp = np.zeros((u_pad, u_pad))
        hp[:n_users, :n_users] = h
        r, c, v, _ = coo_block(hp, rank * per_u, (rank + 1) * per_u, u_pad)
        blocks.append(make_graph(r, c, v, per_u, u_pad))
    rp = np.zeros((u_pad, n_items))
    rp[:n_users] = R
    r, c, v, _ = coo_block(rp, rank * per_u, (rank + 1) * per_u, n_items)
    r_local = make_graph(r, c, v, per_u, n_items)
    ch = gd.ShardedChannels(blocks, per_u, rank, world, group)
    enc = ShardedMHCNEncoder(ch, r_local, d, layers, ops=ops)
    load_params(enc, p, lo, hi, device)
    fu, fi = enc.propagate()
    wu = np.zeros((per_u, d), dtype=np.float32)
    wu[: hi - lo] = p["wu"][lo:hi]
    # items are replicated: weight their term by 1 / world so that the ranks' shares sum to the full loss
    loss = (fu * torch.from_numpy(wu).to(device)).sum() + (fi * torch.from_numpy(p["wi"].astype(np.float32)).to(device)).sum() / world
    loss.backward()
    enc.allreduce_grads()
    out = {"fu": fu.detach().cpu().numpy()[: hi - lo], "fi": fi.detach().cpu().numpy(), "lo": lo, "hi": hi,
           "g_user": enc.user_embeddings.grad.cpu().numpy()[: hi - lo], "g_item": enc.item_embeddings.grad.cpu().numpy(),
           "g_att": enc.attention.grad.cpu().numpy(), "g_att_mat": enc.attention_mat.grad.cpu().numpy()}
    for c in range(4):
        out[f"g_gw{c}"] = enc.gating_weights[str(c + 1)].grad.cpu().numpy()
        out[f"g_gb{c}"] = enc.gating_bias[str(c + 1)].grad.cpu().numpy()
    # propagate() does not reach the self-supervised gates: no gradient, or zeros
    for q in list(enc.sgating_weights.values()) + list(enc.sgating_bias.values()):
        assert q.grad is None or not bool(q.grad.any())
    assert set(out) == {"fu", "fi", "lo", "hi"} | {f"g_{k}" for k in GRAD_KEYS}
    return out


def check(results, world, rtol, layers=LAYERS, **sizes):
    """Every rank's values and EVERY parameter gradient the encoder owns (GRAD_KEYS) against `reference`."""
    H, R, p = problem(**sizes)
    fu, fi, g = reference(H, R, p, layers)
    assert set(g) == set(GRAD_KEYS)
    for r in range(world):
        res = results[r]
        lo, hi = res["lo"], res["hi"]
        tol = dict(rtol=rtol, atol=rtol * np.abs(fu).max())
        np.testing.assert_allclose(res["fu"], fu[lo:hi], **tol)
        np.testing.assert_allclose(res["fi"], fi, **tol)
        np.testing.assert_allclose(res["g_user"], g["user"][lo:hi], rtol=rtol, atol=rtol * np.abs(g["user"]).max())
        for k in GRAD_KEYS[1:]:                                  # replicated parameters: the all-reduced gradient
            np.testing.assert_allclose(res[f"g_{k}"], g[k], rtol=rtol, atol=rtol * np.abs(g[k]).max(), err_msg=k)

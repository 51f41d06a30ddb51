#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY — write tests/golden/buir_steps.npz: six training steps of univariate/buir.py run by the
reference itself.

Runs ONLY where the reference sources are (like scripts/gen_golden_sept_steps.py; the data set and the helpers are
scripts/step_golden.py's); the fixture is plain data.  buir.py imports as-is.  Per step the statements
buir.py:194-203 of `BUIR.train` (forward, get_loss, zero_grad, backward, Adam step, update_target) are lifted with
`oracle.gen_golden.load_stmts` and executed unchanged on a `BUIR_NB` and ONE `torch.optim.Adam`; every
`np.random.random()` rate and `torch.rand` draw of `LGCN_Encoder.forward` is recorded (the way `gen_buir` records one).

Per configuration, from the same float32 initial state: a float64 run (`model.double()`, both encoders'
`sparse_norm_adj.double()`; the draws stay float32 and are identical) with the per-step loss and the six final tensors as
float32(final - init); a float32 run (losses, per-tensor slack = max |f32 - f64|); float64 runs without `update_target`
and without the `loss_iu` term (what a dropped part moves).  The keep masks are stored in the reference's COO order (entry
2 t = (u, i + U), 2 t + 1 = (i + U, u) of training triple t), bit-packed.

The seed of the initial state is scanned from 3 + c upward for the first at which no non-zero element of the float64 run's
FIRST-step gradient is smaller than 10 x Adam's eps (scripts/gen_golden_sept_steps.py says why; rows the batch does not
reach have a gradient of exactly 0 in either precision and do not move).
Asserted when the file is written: f32 and f64 losses within 1e-5 relative; the sensitivity rule of
tests/step_pins.py for either dropped part.

One component case for the kernel test: B = 130 positions with recurring ids over 70 x 50 rows of the first configuration's
propagated tables, d = 64: the reference's predictor and `get_loss` on the gathered rows, its autograd gradients in float64
(dW, dbias, the two table gradients), and the float32 drift of each (max |f32 - f64| / S, S = max |f64|; 4 for the loss)."""
import os
import random

import numpy as np
import torch

import step_golden as sg  # noqa: E402  (puts the repository root and tests/ on sys.path)
from oracle.gen_golden import REF, load_stmts  # noqa: E402
from step_pins import BUIR_TENSORS as TENSORS  # noqa: E402
import buir  # noqa: E402   (oracle.gen_golden puts the reference's univariate/ on sys.path)

PATH = os.path.join(REF, "univariate", "buir.py")

BATCH, STEPS, BATCH_SEED, DRAW_SEED = 128, 6, 5, 23
MIN_FIRST_GRAD = 1e-7       # 10 x Adam's eps
BASE = {"lr": 1e-3, "drop_rate": 0.2}
CONFIGS = [dict(n_layer=2, d=64, tau=0.5), dict(n_layer=3, d=32, tau=0.1)]
BODY = load_stmts(PATH, "BUIR.train", 194, 203)


def build(data, cfg, dtype, seed):
    torch.manual_seed(seed)
    model = buir.BUIR_NB(data, cfg["d"], cfg["tau"], cfg["n_layer"], BASE["drop_rate"], True)
    if dtype == torch.float64:
        model.double()
        for enc in (model.online_encoder, model.target_encoder):
            enc.sparse_norm_adj = enc.sparse_norm_adj.double()
    return model


def loss_ui_only(output):
    """get_loss without its loss_iu term (a dropped part)."""
    import torch.nn.functional as F
    u_online, _, _, i_target = output
    return (2 - 2 * (F.normalize(u_online, dim=-1) * F.normalize(i_target, dim=-1)).sum(dim=-1)).mean()


def run(data, cfg, dtype, seed, batches, steps=STEPS, drop=None):
    """The reference's loop body over the batches -> (losses, final state in float64, rates [steps, 2], rand draws
    [steps, 2, nnz], the smallest non-zero |gradient| of the first step)."""
    model = build(data, cfg, dtype, seed)
    if drop == "update":
        model.update_target = lambda *a: None
    if drop == "iu":
        model.get_loss = loss_ui_only
    optimizer = torch.optim.Adam(model.parameters(), lr=BASE["lr"])
    rates, draws, losses = [], [], []
    real_random, real_rand = np.random.random, torch.rand

    def rec_random(*a):
        r = real_random(*a)
        rates.append(r)
        return r

    def rec_rand(*a, **kw):
        r = real_rand(*a, **kw)
        draws.append(r.numpy().copy())
        return r

    np.random.seed(DRAW_SEED)
    torch.manual_seed(DRAW_SEED)
    np.random.random, torch.rand = rec_random, rec_rand
    try:
        for n, batch in enumerate(batches[:steps]):
            env = dict(model=model, optimizer=optimizer, batch=batch, n=n, epoch=0)
            exec(BODY, env)
            losses.append(float(env["batch_loss"].detach()))
            if n == 0:
                first = min(float(g[g != 0].min()) for g in (p.grad.abs() for p in model.parameters() if p.grad is not None))
    finally:
        np.random.random, torch.rand = real_random, real_rand
    assert len(rates) == len(draws) == 2 * steps
    final = {k: v.detach().double().numpy().copy() for k, v in model.state_dict().items()}
    assert set(final) == set(TENSORS), sorted(final)
    rates = np.array(rates).reshape(steps, 2) * BASE["drop_rate"]          # :312: np.random.random() * self.drop_ratio
    return np.array(losses), final, rates, np.stack(draws).reshape(steps, 2, -1), first


def keep_of(rate, rand):
    """buir.py:301-303 on a recorded draw: floor(1 - rate + rand) as the reference forms it."""
    random_tensor = 1 - rate
    random_tensor += torch.from_numpy(rand)
    return torch.floor(random_tensor).type(torch.bool).numpy()


def reference_batches(data, seed):
    random.seed(seed)
    return sg.first_batches(buir.next_batch_pairwise(data, BATCH), STEPS, BATCH, lambda b: tuple(list(t) for t in b))


def component_case(data, out):
    """B = 130 with recurring ids, d = 64: predictor + get_loss on gathered rows of propagated tables."""
    model = build(data, CONFIGS[0], torch.float32, 3)
    rng = np.random.default_rng(77)
    n_u, n_i, b = 70, 50, 130
    with torch.no_grad():
        on_u, on_i = model.online_encoder.get_embedding()
        # another state for the targets: the online tables of another seed's model
        tg_u, tg_i = build(data, CONFIGS[0], torch.float32, 4).online_encoder.get_embedding()
    tabs = [t[:n].clone() for t, n in ((on_u, n_u), (on_i, n_i), (tg_u, n_u), (tg_i, n_i))]
    u_idx, i_idx = rng.integers(0, n_u, b), rng.integers(0, n_i, b)
    u_idx[:40] = 11                                                         # a run of one user across tiles
    i_idx[100:] = i_idx[:30]
    w = model.predictor.weight.detach() + 0.05 * torch.randn(64, 64, generator=torch.Generator().manual_seed(1))
    bias = 0.1 * torch.randn(64, generator=torch.Generator().manual_seed(2))
    res = {}
    for dtype in (torch.float64, torch.float32):
        xu, xi, tu, ti = (t.detach().clone().to(dtype).requires_grad_(k < 2) for k, t in enumerate(tabs))
        model.predictor.to(dtype)
        with torch.no_grad():
            model.predictor.weight.copy_(w)
            model.predictor.bias.copy_(bias)
        model.predictor.zero_grad()
        loss = model.get_loss((model.predictor(xu[u_idx]), tu[u_idx], model.predictor(xi[i_idx]), ti[i_idx]))
        loss.backward()
        res[dtype] = dict(loss=loss.detach().double().numpy(), g_w=model.predictor.weight.grad.double().numpy().copy(),
                          g_bias=model.predictor.bias.grad.double().numpy().copy(), g_on_user=xu.grad.double().numpy(),
                          g_on_item=xi.grad.double().numpy())
    out.update({"comp/on_user": tabs[0].numpy(), "comp/on_item": tabs[1].numpy(), "comp/tg_user": tabs[2].numpy(),
                "comp/tg_item": tabs[3].numpy(), "comp/u_idx": u_idx.astype(np.int16), "comp/i_idx": i_idx.astype(np.int16),
                "comp/w": w.numpy(), "comp/bias": bias.numpy()})
    for k, ref in res[torch.float64].items():
        scale = 4.0 if k == "loss" else float(np.abs(ref).max())
        drift = float(np.abs(res[torch.float32][k] - ref).max()) / scale
        out[f"comp/f64/{k}"], out[f"comp/scale/{k}"], out[f"comp/drift/{k}"] = ref, scale, drift
        print(f"component {k}: scale {scale:.3g} reference f32 drift {drift:.3g}")


def main(out_dir):
    rng = np.random.default_rng(20261018)
    train, _ = sg.synthetic_lists(rng)
    data = buir.Interaction({}, train, train[:10])
    assert (data.user_num, data.item_num) == (sg.N_USERS, sg.N_ITEMS)
    assert len(set((t[0], t[1]) for t in train)) < len(train), "expected a duplicate interaction"
    batches = reference_batches(data, BATCH_SEED)
    out = dict(sg.id_arrays(train, data),
               steps=STEPS, batch_size=BATCH, configs=len(CONFIGS), batch_seed=BATCH_SEED, draw_seed=DRAW_SEED,
               **{f"hp/{k}": v for k, v in BASE.items()})
    sg.store_batches(out, batches, ("users", "items"), np.int16)
    assert all(len(set(u)) < len(u) or len(set(i)) < len(i) for u, i, _ in batches)

    for c, cfg in enumerate(CONFIGS):
        pre = f"c{c}/"
        out.update({pre + k: v for k, v in cfg.items()})
        for seed in range(3 + c, 3 + c + 200):
            first = run(data, cfg, torch.float64, seed, batches, steps=1)[4]
            print(f"config {c}: table seed {seed}: smallest non-zero first-step |gradient| {first:.3g}")
            if first >= MIN_FIRST_GRAD:
                break
        else:
            raise AssertionError("no table seed satisfies the first-step gradient condition")
        out[pre + "table_seed"], out[pre + "first_grad"] = seed, first
        l64, p64, rates, draws, _ = run(data, cfg, torch.float64, seed, batches)
        l32, p32, rates32, draws32, _ = run(data, cfg, torch.float32, seed, batches)
        assert np.array_equal(rates, rates32) and np.array_equal(draws, draws32), "the draws must not depend on the precision"
        assert np.isfinite(l64).all() and (np.abs(l32 - l64) <= 1e-5 * np.abs(l64)).all(), (l32, l64)
        out[pre + "f64/losses"], out[pre + "f32/losses"], out[pre + "rates"] = l64, l32, rates
        keep = np.stack([[keep_of(rates[n, e], draws[n, e]) for e in (0, 1)] for n in range(STEPS)])
        assert keep.shape == (STEPS, 2, 2 * len(train)) and 0.75 < keep.mean() < 1.0
        out[pre + "keep_packed"], out[pre + "nnz"] = np.packbits(keep, axis=-1, bitorder="little"), keep.shape[-1]
        print(f"config {c} {cfg}: f64 losses {l64}\n  max rel |f32 - f64| {(np.abs(l32 - l64) / np.abs(l64)).max():.3g}; rates\n{rates}")
        finals = {"update": run(data, cfg, torch.float64, seed, batches, drop="update")[1],
                  "iu": run(data, cfg, torch.float64, seed, batches, drop="iu")[1]}
        init = {k: v.detach().numpy().copy() for k, v in build(data, cfg, torch.float32, seed).state_dict().items()}
        for k in TENSORS:
            online = k.replace("target_encoder", "online_encoder")          # _init_target: the targets start as copies,
            assert np.array_equal(init[k], init[online])                    # so only the online ones are stored
            sg.record_table(out, pre, "buir", k, p64[k], p32[k], finals, init=init[k], store_init=k == online)

    component_case(data, out)
    sg.save(out_dir, "buir_steps", out)


if __name__ == "__main__":
    main(sg.out_dir())
